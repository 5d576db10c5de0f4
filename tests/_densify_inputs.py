"""Inputs and float64 restatements for the densification kernels of csrc/postops.hip (NumPy only; no device).

``reference_flags``   the flag byte of dnsplat_densify_classify stated in float64 from the float32 inputs (dn_model.py:271-386 and
                      nerfstudio's cull_gaussians), with the rows whose decision float32 rounding could turn marked *undecided*.
``random_table``      a stratified table on which every flag bit, and the rare combinations, occur often.
``edge_rows``         hand-built rows ON a threshold, where float32 evaluation is exact, each with the byte it must give.
``split_inputs``      parents, quaternions, scales, means and noise for dnsplat_densify_split.
``split_reference``   the children's means and log-scales in a chosen precision, with the magnitudes an error bound is built from.
``split_ratios``      how far the float32 evaluation of that formula is from float64, in units of 2^-24 x magnitude.

tests/test_densify_reference.py proves on the CPU what tests/test_gpu_densify_edges.py relies on.
"""
import functools

import numpy as np

SPLIT, DUP, CULL, CULL_CHILD, CULL_DUP = 1, 2, 4, 8, 16          # include/dnsplat.h DNSPLAT_DENSIFY_*
BIT_NAMES = {SPLIT: "SPLIT", DUP: "DUP", CULL: "CULL", CULL_CHILD: "CULL_CHILD", CULL_DUP: "CULL_DUP"}
U24 = 2.0 ** -24
THRESHOLD_NAMES = ("densify_grad_thresh", "densify_size_thresh", "split_screen_size", "cull_alpha_thresh", "cull_scale_thresh",
                   "cull_screen_size")
# densify.RefineConfig's defaults (nerfstudio 1.1.3)
DEFAULT_THRESHOLDS = dict(densify_grad_thresh=0.0008, densify_size_thresh=0.01, split_screen_size=0.05, cull_alpha_thresh=0.1,
                          cull_scale_thresh=0.5, cull_screen_size=0.15)
MODES = [(d, s, c) for d in (0, 1) for s in (0, 1) for c in (0, 1)]      # (do_densify, screen_rules, cull_big)
TABLE_N = 4099
TABLE_SIDE = 512.0


def thresholds_f32(thresholds):
    """The six thresholds as the C struct holds them: rounded to float32.  ``thresholds``: a mapping or an object with attributes
    (densify.RefineConfig)."""
    get = thresholds.__getitem__ if hasattr(thresholds, "__getitem__") else (lambda k: getattr(thresholds, k))
    return {k: np.float32(get(k)) for k in THRESHOLD_NAMES}


def reference_flags(scales, opac, gn, vis, z, do_densify, screen_rules, cull_big, side, thresholds, margin=1e-5):
    """(flags uint8 [N], undecided bool [N]).  ``scales`` [N,3] log-scales, ``opac`` [N] logits, ``gn`` / ``vis`` / ``z`` [N] the three
    statistics (``z`` = max_2Dsize or None), all float32; evaluated in float64.  A row is undecided when a quantity it compares in
    this mode lies within ``margin`` (relative) of its threshold.  NaN follows IEEE and torch: ``max`` propagates it, and every
    comparison with it is false."""
    t = {k: float(v) for k, v in thresholds_f32(thresholds).items()}
    s = np.asarray(scales, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    N = s.shape[0]
    o = np.asarray(opac, dtype=np.float32).astype(np.float64).reshape(-1)
    zz = np.zeros(N) if z is None else np.asarray(z, dtype=np.float32).astype(np.float64).reshape(-1)
    undecided = np.zeros(N, dtype=bool)

    def near(q, thr):
        with np.errstate(invalid="ignore"):
            return np.abs(q - thr) <= margin * abs(thr)          # nan, inf: False

    with np.errstate(all="ignore"):
        e = np.exp(s)
        smax = e.max(axis=1)                                       # np.max propagates nan, as torch.max does
        smax_child = np.exp(np.log(e / 1.6)).max(axis=1)           # a child holds log(exp(s) / 1.6); the cull exponentiates it again
        smax_dup = smax
        f = np.zeros(N, dtype=np.uint8)
        if do_densify:
            g = np.asarray(gn, dtype=np.float32).astype(np.float64).reshape(-1)
            v = np.asarray(vis, dtype=np.float32).astype(np.float64).reshape(-1)
            avg = (g / v) * 0.5 * float(side)
            high = avg > t["densify_grad_thresh"]
            split = smax > t["densify_size_thresh"]
            undecided |= near(avg, t["densify_grad_thresh"]) | near(smax, t["densify_size_thresh"])
            if screen_rules:
                split = split | (zz > t["split_screen_size"])
                undecided |= near(zz, t["split_screen_size"])
            split = split & high
            # split_gaussians shrinks its parents in place before the duplicate mask is formed
            smax_dup = np.where(split, smax_child, smax)
            dup = (smax_dup <= t["densify_size_thresh"]) & high
            undecided |= split & near(smax_child, t["densify_size_thresh"])
            f |= split.astype(np.uint8) * SPLIT | dup.astype(np.uint8) * DUP
        alpha = 1.0 / (1.0 + np.exp(-o))
        low = alpha < t["cull_alpha_thresh"]
        undecided |= near(alpha, t["cull_alpha_thresh"])
        big = big_child = big_dup = np.zeros(N, dtype=bool)
        if cull_big:
            big = smax > t["cull_scale_thresh"]
            big_dup = smax_dup > t["cull_scale_thresh"]
            big_child = smax_child > t["cull_scale_thresh"]
            undecided |= near(smax, t["cull_scale_thresh"]) | near(smax_child, t["cull_scale_thresh"])
            if screen_rules and z is not None:
                big = big | (zz > t["cull_screen_size"])
                undecided |= near(zz, t["cull_screen_size"])
        f |= (((f & SPLIT) != 0) | low | big).astype(np.uint8) * CULL
        f |= (low | big_child).astype(np.uint8) * CULL_CHILD
        f |= (low | big_dup).astype(np.uint8) * CULL_DUP
    return f, undecided


def random_table(N, seed):
    """dict of float32 arrays: scales [N,3], opac [N], gn [N], vis [N], z [N].  One eighth of the rows have their largest log-scale
    in [log 0.3, log 1.0], the band that holds cull_scale_thresh and 1.6 x cull_scale_thresh ("parent too big, child not")."""
    rng = np.random.default_rng(seed)
    scales = rng.normal(-4.0, 1.6, size=(N, 3))
    band = rng.random(N) < 0.125
    top = rng.uniform(np.log(0.3), np.log(1.0), size=N)
    slot = scales.argmax(axis=1)
    capped = np.minimum(scales, top[:, None])
    capped[np.arange(N), slot] = top
    scales = np.where(band[:, None], capped, scales)
    opac = rng.normal(-1.0, 2.5, size=N)
    vis = rng.integers(1, 9, size=N).astype(np.float64)
    gn = 2e-6 * vis * np.exp(rng.normal(0.0, 1.0, size=N))
    z = np.where(rng.random(N) < 0.5, 0.0, 0.05 * np.exp(rng.normal(0.0, 1.0, size=N)))
    return dict(scales=scales.astype(np.float32), opac=opac.astype(np.float32), gn=gn.astype(np.float32),
                vis=vis.astype(np.float32), z=z.astype(np.float32))


def table_flags(table, mode, with_z=True, thresholds=DEFAULT_THRESHOLDS, side=TABLE_SIDE, margin=1e-5):
    """reference_flags over a ``random_table``."""
    d, s, c = mode
    return reference_flags(table["scales"], table["opac"], table["gn"], table["vis"], table["z"] if with_z else None, d, s, c, side,
                           thresholds, margin)


# ---- rows on a threshold ---------------------------------------------------------------------------------------------------------------

F32 = np.float32
EDGE_SIDE = 512.0
# nothing fires at these: a row states only what it moves
EDGE_THRESHOLDS = dict(densify_grad_thresh=2.0 ** -10, densify_size_thresh=1.0, split_screen_size=float(F32(0.05)),
                       cull_alpha_thresh=0.5, cull_scale_thresh=4.0, cull_screen_size=float(F32(0.15)))
NAN = float("nan")


def _up(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


def _down(x):
    return float(np.nextafter(F32(x), F32(-np.inf)))


def edge_rows():
    """[dict(name, scales (3), opac, gn, vis, z, mode, side, thresholds, expect)].  Every row sits where float32 evaluation is exact:
    exp(0) = 1, sigmoid(0) = 1 / (1 + 1) = 0.5, a screen size equal to the float32 threshold, and an average gradient made of powers
    of two (2^-16 / 4 * 0.5 * 512 = 2^-10).  Each on-threshold row has the neighbours one float32 step either side.  For the screen
    size and the gradient the step is taken on the input.  For the scales and the opacity it is taken on the threshold: one float32
    step from a log-scale (or logit) of 0 is a denormal, which exp() does not see.

    Defaults of a row: small scales (exp(-3) = 0.0498), opacity logit 3 (alpha 0.95), no gradient (gn 0 / vis 1: not high), z 0.
    ``HIGH`` is gn = 1 at vis = 1: an average gradient of 256."""
    rows = []

    def row(name, expect, mode, scales=(-3.0, -3.0, -3.0), opac=3.0, gn=0.0, vis=1.0, z=0.0, **thr):
        rows.append(dict(name=name, scales=tuple(scales), opac=opac, gn=gn, vis=vis, z=z, mode=mode, side=EDGE_SIDE,
                         thresholds={**EDGE_THRESHOLDS, **thr}, expect=expect))

    HIGH = dict(gn=1.0, vis=1.0)
    unit = (0.0, -1.0, -2.0)                                      # the largest scale is exp(0) = 1 exactly
    # densify size: smax > thresh splits; smax <= thresh duplicates.  On it: not split, duplicated.  Below the scale: split, and the
    # child's 0.625 is under the threshold, so duplicated as well
    row("size_on", DUP, (1, 0, 0), scales=unit, **HIGH, densify_size_thresh=1.0)
    row("size_thresh_up", DUP, (1, 0, 0), scales=unit, **HIGH, densify_size_thresh=_up(1.0))
    row("size_thresh_down", SPLIT | DUP | CULL, (1, 0, 0), scales=unit, **HIGH, densify_size_thresh=_down(1.0))
    row("size_on_slot1", DUP, (1, 0, 0), scales=(-1.0, 0.0, -2.0), **HIGH)
    row("size_on_slot2", DUP, (1, 0, 0), scales=(-2.0, -1.0, 0.0), **HIGH)
    row("size_on_low_grad", 0, (1, 0, 0), scales=unit)
    # cull scale: smax > thresh is too big.  On it: kept.  Below the scale: the original and its duplicate go, a child (0.625) would stay
    row("cull_scale_on", 0, (0, 0, 1), scales=unit, cull_scale_thresh=1.0)
    row("cull_scale_thresh_up", 0, (0, 0, 1), scales=unit, cull_scale_thresh=_up(1.0))
    row("cull_scale_thresh_down", CULL | CULL_DUP, (0, 0, 1), scales=unit, cull_scale_thresh=_down(1.0))
    row("cull_scale_off", 0, (0, 0, 0), scales=unit, cull_scale_thresh=_down(1.0))
    # opacity: alpha < thresh is low.  On it: kept
    row("alpha_on", 0, (0, 0, 0), opac=0.0, cull_alpha_thresh=0.5)
    row("alpha_thresh_up", CULL | CULL_CHILD | CULL_DUP, (0, 0, 0), opac=0.0, cull_alpha_thresh=_up(0.5))
    row("alpha_thresh_down", 0, (0, 0, 0), opac=0.0, cull_alpha_thresh=_down(0.5))
    row("alpha_on_negative_zero", 0, (0, 0, 0), opac=-0.0, cull_alpha_thresh=0.5)
    # split screen size: z > thresh splits (the child, 0.031, is then duplicated too); the row is duplicated either way
    z_split = EDGE_THRESHOLDS["split_screen_size"]
    row("split_screen_on", DUP, (1, 1, 0), z=z_split, **HIGH)
    row("split_screen_up", SPLIT | DUP | CULL, (1, 1, 0), z=_up(z_split), **HIGH)
    row("split_screen_down", DUP, (1, 1, 0), z=_down(z_split), **HIGH)
    row("split_screen_rules_off", DUP, (1, 0, 0), z=_up(z_split), **HIGH)
    # cull screen size: z > thresh is too big, for the original alone (appended entries start at z = 0)
    z_cull = EDGE_THRESHOLDS["cull_screen_size"]
    row("cull_screen_on", 0, (0, 1, 1), z=z_cull)
    row("cull_screen_up", CULL, (0, 1, 1), z=_up(z_cull))
    row("cull_screen_down", 0, (0, 1, 1), z=_down(z_cull))
    row("cull_screen_rules_off", 0, (0, 0, 1), z=_up(z_cull))
    row("cull_screen_not_big_yet", 0, (0, 1, 0), z=_up(z_cull))
    # average gradient: avg > thresh is high.  2^-16 / 4 * 0.5 * 512 = 2^-10 exactly
    row("grad_on", 0, (1, 0, 0), gn=2.0 ** -16, vis=4.0)
    row("grad_up", DUP, (1, 0, 0), gn=_up(2.0 ** -16), vis=4.0)
    row("grad_down", 0, (1, 0, 0), gn=_down(2.0 ** -16), vis=4.0)
    # never seen: 0 / 0 is nan (never high), x / 0 is inf (high)
    row("vis0_gn0", 0, (1, 0, 0), gn=0.0, vis=0.0)
    row("vis0_gn_positive", DUP, (1, 0, 0), gn=1e-6, vis=0.0)
    # exp() overflows to inf: split, and the child (inf) is too big as well; exp() underflows to 0: duplicated
    row("scale_plus_100", SPLIT | CULL | CULL_CHILD | CULL_DUP, (1, 0, 1), scales=(100.0, -3.0, -3.0), **HIGH)
    row("scale_minus_200", DUP, (1, 0, 1), scales=(-200.0, -200.0, -200.0), **HIGH)
    # a nan scale makes the largest scale nan (torch.max propagates it): no scale comparison holds, whatever the other two are
    for k in range(3):
        big, small = [2.0, -3.0, 2.0], [-3.0, -3.0, -3.0]
        big[k] = small[k] = NAN
        row(f"nan_scale_slot{k}_others_big", 0, (1, 0, 1), scales=big, **HIGH)
        row(f"nan_scale_slot{k}_others_small", 0, (1, 0, 1), scales=small, **HIGH)
        row(f"nan_scale_slot{k}_cull_only", 0, (0, 0, 1), scales=big)
    row("nan_scale_low_alpha", CULL | CULL_CHILD | CULL_DUP, (1, 1, 1), scales=(NAN, 2.0, -3.0), opac=-5.0, **HIGH)
    row("nan_scale_screen_split", SPLIT | CULL, (1, 1, 1), scales=(NAN, 2.0, -3.0), z=_up(z_split), **HIGH)
    # a nan opacity is not low
    row("nan_opacity", 0, (0, 0, 0), opac=NAN)
    row("nan_opacity_densify", DUP, (1, 0, 1), opac=NAN, **HIGH)
    assert len({r["name"] for r in rows}) == len(rows)
    return rows


# ---- the split children ----------------------------------------------------------------------------------------------------------------

SPLIT_PARENTS = (1, 3, 127, 128, 129)
SPLIT_SAMPLES = (1, 2, 3)
SPLIT_ROWS = 300                # Gaussians the parents are drawn from


def split_inputs(n_parents, n_samples, seed=0):
    """dict: means [M,3], scales [M,3], quats [M,4] float32 over M = SPLIT_ROWS Gaussians, parents [n_parents] int32 (drawn with
    repeats, not ascending), noise [n_parents * n_samples, 3] float32.  Quaternion norms are spread over 1e-3 .. 1e3; rows 0-7 are pure
    axes (w, x, y, z alone, either sign), a quarter of the others have a negative w.  Log-scales in [-9, 3], means up to ~50."""
    rng = np.random.default_rng(9000 + 97 * n_parents + n_samples + seed)
    M = SPLIT_ROWS
    quats = rng.normal(size=(M, 4))
    for k in range(4):
        quats[k], quats[4 + k] = 0.0, 0.0
        quats[k, k], quats[4 + k, k] = 1.0, -1.0
    flip = rng.random(M) < 0.25
    flip[8:12] = True                                              # the first parents of every size include negative w
    quats[8:, 0] = np.where(flip[8:], -np.abs(quats[8:, 0]), quats[8:, 0])
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    quats *= 10.0 ** rng.uniform(-3, 3, size=(M, 1))
    scales = rng.uniform(-9.0, 3.0, size=(M, 3))
    means = rng.uniform(-50.0, 50.0, size=(M, 3))
    # random draws (unsorted; with repeats by the birthday bound, and by force); the smallest sizes still meet a negative w and two pure axes
    parents = rng.integers(0, M, size=n_parents)
    parents[:3] = [9, 1, 4][:n_parents]
    if n_parents > 3:
        parents[-1] = parents[0]
    noise = rng.normal(size=(n_parents * n_samples, 3))
    return dict(means=means.astype(np.float32), scales=scales.astype(np.float32), quats=quats.astype(np.float32),
                parents=parents.astype(np.int32), noise=noise.astype(np.float32))


def split_reference(means, scales, quats, parents, noise, dtype):
    """(new_means, new_scales, mag_means, mag_scales), all [n_children,3]: the formula of postops.hip's comment evaluated in ``dtype``,
        child j of parent p = parents[j % n_parents]:  mean = mean_p + R(q_p / |q_p|) (exp(scale_p) * noise_j),  scale = log(exp(scale_p) / 1.6)
    and the magnitudes its rounding errors scale with:  |mean_p| + sum_k |R_ik| |v_k|  per component, and  1 + |child log-scale|."""
    dt = np.dtype(dtype).type
    parents = np.asarray(parents).astype(np.int64)
    n_children, n_parents = noise.shape[0], parents.shape[0]
    p = parents[np.arange(n_children) % n_parents]
    q = np.asarray(quats, dtype=np.float32).astype(dt)[p]
    s = np.asarray(scales, dtype=np.float32).astype(dt)[p]
    m = np.asarray(means, dtype=np.float32).astype(dt)[p]
    nz = np.asarray(noise, dtype=np.float32).astype(dt)
    one, two = dt(1.0), dt(2.0)
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True, dtype=dt))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                  two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    e = np.exp(s)
    v = e * nz
    rot = (R[:, :, 0] * v[:, None, 0] + R[:, :, 1] * v[:, None, 1]) + R[:, :, 2] * v[:, None, 2]
    new_means = rot + m
    new_scales = np.log(e / dt(1.6))
    assert new_means.dtype == np.dtype(dtype) and new_scales.dtype == np.dtype(dtype)
    mag_means = np.abs(m) + (np.abs(R) * np.abs(v)[:, None, :]).sum(axis=2)
    mag_scales = one + np.abs(new_scales)
    return new_means, new_scales, mag_means, mag_scales


@functools.lru_cache(maxsize=1)
def split_ratios():
    """(r_mean, r_scale): the worst |float32 - float64| / (2^-24 x magnitude) of ``split_reference`` over every ``split_inputs`` case
    (magnitudes from the float64 evaluation)."""
    r_mean = r_scale = 0.0
    for n_parents in SPLIT_PARENTS:
        for n_samples in SPLIT_SAMPLES:
            inp = split_inputs(n_parents, n_samples)
            m32, s32, _, _ = split_reference(**inp, dtype=np.float32)
            m64, s64, gm, gs = split_reference(**inp, dtype=np.float64)
            r_mean = max(r_mean, float((np.abs(m32 - m64) / (U24 * gm)).max()))
            r_scale = max(r_scale, float((np.abs(s32 - s64) / (U24 * gs)).max()))
    return r_mean, r_scale
