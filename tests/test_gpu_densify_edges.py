"""The oldest per-frame kernels (csrc/postops.hip), each called through the C entry and held per row at its edges:
``dnsplat_densify_classify`` in all eight modes with and without max_2Dsize, byte for byte against the float64 statement of
tests/_densify_inputs.py and on hand-built rows that sit ON a threshold; ``dnsplat_densify_split`` against float64 with
un-normalised quaternions and shuffled, repeated parents; ``dnsplat_densify_stats`` with both gradient strides and unseen rows that
carry NaN; ``dnsplat_dn_depth_normals`` on frames with no, one and a few inner pixels; ``dnsplat_camera_prepare`` with its optional
outputs.  The whole-scene tests of test_gpu_parity.py run these kernels at one size each on random data, which never lands on a
threshold.

Every output lives in the middle of a buffer pre-filled with a sentinel, and every optional or strided input in the middle of a
NaN-filled one: a write outside the output shows in the guard, a read outside the input shows as NaN in the result.  Nothing here
depends on reading or writing outside a buffer.

Tolerances: flags, fills, borders, copies, counts and maxima are exact.  The split children are within four times the float32
restatement's own distance from float64 (tests/test_densify_reference.py measures it on the CPU); the other bounds are rounding
counts stated where they are used."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _densify_inputs as di
from _postops_ref import _restated_surface_normal, surface_normal_allowance

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24
GUARD = 64                      # elements either side of every output
SENTINEL = 0x7FC0BEEF           # a NaN with a payload, as int32
BYTE_SENTINEL = 0xAA
INVALID_ARG = -1                # include/dnsplat.h DNSPLAT_ERR_INVALID_ARG
SIZES = (1, 255, 256, 257, 4099)      # one lane, one workgroup of 256 less one / exactly / plus one, seventeen workgroups


def _api():
    from dn_splatter_amd import _lib, _ops

    return _lib, _ops._ptr, _ops._stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded:
    """``n`` elements in the middle of a sentinel-filled buffer; ``intact()`` says whether the GUARD elements either side still hold
    the sentinel."""

    def __init__(self, n, dtype=torch.float32):
        self.n = n
        if dtype == torch.uint8:
            self.raw = torch.full((n + 2 * GUARD,), BYTE_SENTINEL, dtype=torch.uint8, device=DEV)
            self.buf = self.raw
        else:
            self.raw = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
            self.buf = self.raw.view(dtype)
        self.fill = int(self.raw[0])
        self.view = self.buf[GUARD:GUARD + n]

    def intact(self):
        return bool((self.raw[:GUARD] == self.fill).all()) and bool((self.raw[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.raw == self.fill).all())


def _in_nan(a, pad=GUARD):
    """A float32 array on the device in the middle of a NaN-filled buffer (``pad`` elements either side): (buffer, view)."""
    flat = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    buf = torch.full((flat.size + 2 * pad,), float("nan"), dtype=torch.float32, device=DEV)
    buf[pad:pad + flat.size] = torch.from_numpy(flat).to(DEV)
    return buf, buf[pad:pad + flat.size]


# ---- dnsplat_densify_classify ----------------------------------------------------------------------------------------------------------


def _classify_args(N, scales, opac, gn, vis, z, mode, side, thresholds, flags):
    _lib, ptr, _ = _api()
    a = _lib.DensifyArgs()
    a.N = N
    a.scales, a.opacities, a.xys_grad_norm, a.vis_counts, a.max_2Dsize = ptr(scales), ptr(opac), ptr(gn), ptr(vis), ptr(z)
    a.do_densify, a.screen_rules, a.cull_big = mode
    a.max_image_side = float(side)
    for k in di.THRESHOLD_NAMES:
        setattr(a, k, float(thresholds[k]))
    a.flags = ptr(flags)
    return a


def _classify(rows, mode, with_z, side, thresholds):
    """flags [N] uint8 (numpy) of the kernel over ``rows`` (dict of float32 arrays), written into a guarded buffer."""
    _lib, _, stream = _api()
    N = rows["opac"].shape[0]
    t = {k: _dev(rows[k]) for k in ("scales", "opac", "gn", "vis")}
    z = _dev(rows["z"]) if with_z else None
    out = Guarded(N, torch.uint8)
    a = _classify_args(N, t["scales"], t["opac"], t["gn"], t["vis"], z, mode, side, thresholds, out.view)
    rc = _lib.lib().dnsplat_densify_classify(ctypes.byref(a), stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert out.intact(), "dnsplat_densify_classify wrote outside flags[0:N]"
    return out.view.cpu().numpy()


@functools.lru_cache(maxsize=1)
def _table():
    return di.random_table(di.TABLE_N, 0)


@pytest.mark.parametrize("with_z", [True, False], ids=["z", "no_z"])
@pytest.mark.parametrize("mode", di.MODES, ids=lambda m: "densify%d_screen%d_big%d" % m)
@pytest.mark.parametrize("N", SIZES)
def test_classify_equals_the_float64_statement_on_every_decided_row(dns, N, mode, with_z):
    rows = {k: v[:N] for k, v in _table().items()}
    want, undecided = di.reference_flags(rows["scales"], rows["opac"], rows["gn"], rows["vis"], rows["z"] if with_z else None, *mode,
                                         di.TABLE_SIDE, di.DEFAULT_THRESHOLDS)
    assert undecided.mean() <= 0.01, int(undecided.sum())
    got = _classify(rows, mode, with_z, di.TABLE_SIDE, di.DEFAULT_THRESHOLDS)
    bad = np.nonzero((got != want) & ~undecided)[0]
    assert bad.size == 0, (f"{bad.size} decided rows differ; first: row {bad[0]} kernel {int(got[bad[0]])} reference {int(want[bad[0]])} "
                           f"scales {rows['scales'][bad[0]]} opac {rows['opac'][bad[0]]} gn {rows['gn'][bad[0]]} "
                           f"vis {rows['vis'][bad[0]]} z {rows['z'][bad[0]]}")
    if N == di.TABLE_N and mode[0]:
        assert len(set(got.tolist())) >= 8          # the table reaches the rare bytes on the device too


@pytest.mark.parametrize("row", di.edge_rows(), ids=lambda r: r["name"])
def test_classify_on_a_threshold(dns, row):
    """Rows where float32 evaluation is exact: the byte is pinned with no tolerance, on the threshold and one float32 step either
    side of it, so a > that became >= (or a < that became <=) fails here."""
    one = lambda k: np.array([row[k]], dtype=np.float32)          # noqa: E731
    rows = dict(scales=np.array([row["scales"]], dtype=np.float32), opac=one("opac"), gn=one("gn"), vis=one("vis"), z=one("z"))
    got = _classify(rows, row["mode"], True, row["side"], row["thresholds"])
    assert int(got[0]) == row["expect"], f"{row['name']}: kernel {int(got[0])}, expected {row['expect']}"


def test_classify_return_codes_launch_nothing(dns):
    _lib, ptr, stream = _api()
    rows = {k: _dev(v[:8]) for k, v in _table().items()}
    out = Guarded(8, torch.uint8)

    def call(N, mode, gn=rows["gn"], vis=rows["vis"], flags=out.view, scales=rows["scales"]):
        a = _classify_args(N, scales, rows["opac"], gn, vis, rows["z"], mode, di.TABLE_SIDE, di.DEFAULT_THRESHOLDS, flags)
        rc = _lib.lib().dnsplat_densify_classify(ctypes.byref(a), stream())
        torch.cuda.synchronize()
        return rc

    assert call(0, (1, 1, 1)) == 0
    assert call(0, (1, 1, 1), gn=None, flags=None, scales=None) == 0
    assert call(-1, (1, 1, 1)) == INVALID_ARG
    assert call(8, (1, 0, 0), gn=None) == INVALID_ARG
    assert call(8, (1, 0, 0), vis=None) == INVALID_ARG
    assert call(8, (0, 0, 0), flags=None) == INVALID_ARG
    assert _lib.lib().dnsplat_densify_classify(None, stream()) == INVALID_ARG
    assert out.untouched()
    assert call(8, (0, 0, 0), gn=None, vis=None) == 0          # the statistics are optional without densification
    assert out.intact() and not out.untouched()


# ---- dnsplat_densify_split -------------------------------------------------------------------------------------------------------------


def _split(inp):
    """(new_means, new_scales) [n_children,3] float32 (numpy) of the kernel, written into guarded buffers."""
    _lib, ptr, stream = _api()
    n_children, n_parents = inp["noise"].shape[0], inp["parents"].shape[0]
    t = {k: _dev(inp[k]) for k in ("parents", "noise", "means", "scales", "quats")}
    assert t["parents"].dtype == torch.int32 and int(t["parents"].min()) >= 0 and int(t["parents"].max()) < inp["means"].shape[0]
    nm, ns = Guarded(3 * n_children), Guarded(3 * n_children)
    rc = _lib.lib().dnsplat_densify_split(n_children, n_parents, ptr(t["parents"]), ptr(t["noise"]), ptr(t["means"]), ptr(t["scales"]),
                                          ptr(t["quats"]), ptr(nm.view), ptr(ns.view), stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert nm.intact() and ns.intact(), "dnsplat_densify_split wrote outside its outputs"
    return nm.view.cpu().numpy().reshape(-1, 3), ns.view.cpu().numpy().reshape(-1, 3)


@pytest.mark.parametrize("n_samples", di.SPLIT_SAMPLES)
@pytest.mark.parametrize("n_parents", di.SPLIT_PARENTS)
def test_split_children_match_float64(dns, n_parents, n_samples):
    """Quaternion norms from 1e-3 to 1e3 (a kernel that forgot to normalise is wrong by the norm squared), negative w and pure axes,
    parents shuffled with repeats.  Allowance: four times the float32 restatement's own worst distance from float64."""
    r_mean, r_scale = di.split_ratios()
    inp = di.split_inputs(n_parents, n_samples)
    m, s = _split(inp)
    m64, s64, gm, gs = di.split_reference(**inp, dtype=np.float64)
    assert np.isfinite(m).all() and np.isfinite(s).all()
    w_mean = float((np.abs(m - m64) / (4 * r_mean * U24 * gm)).max())
    w_scale = float((np.abs(s - s64) / (4 * r_scale * U24 * gs)).max())
    print(f"[densify] split {n_parents} parents x {n_samples}: worst error / allowance: means {w_mean:.3f}  log-scales {w_scale:.3f} "
          f"(allowance 4 x {r_mean:.2f} / 4 x {r_scale:.2f} x 2^-24 x magnitude)")
    assert w_mean <= 1.0, f"children's means: worst error / allowance {w_mean:.2f}"
    assert w_scale <= 1.0, f"children's log-scales: worst error / allowance {w_scale:.2f}"


@pytest.mark.parametrize("n_parents,n_samples", [(5, 3), (129, 2), (2, 1)])
def test_split_child_j_comes_from_parent_j_mod_n_parents(dns, n_parents, n_samples):
    """Gaussian i sits at 1000 (i + 1) on every axis and is tiny: a child's mean names its parent."""
    inp = di.split_inputs(n_parents, n_samples)
    M = inp["means"].shape[0]
    inp["means"] = np.repeat(1000.0 * (np.arange(M, dtype=np.float32) + 1)[:, None], 3, axis=1)
    inp["scales"] = np.full((M, 3), -6.0, dtype=np.float32)          # exp(-6) x |noise| < 0.02
    m, _ = _split(inp)
    named = np.rint(m / 1000.0).astype(np.int64) - 1
    want = inp["parents"].astype(np.int64)[np.arange(n_parents * n_samples) % n_parents]
    assert np.abs(m - 1000.0 * (named + 1)).max() < 0.1
    assert (named == want[:, None]).all(), (named[:, 0].tolist()[:12], want.tolist()[:12])


def test_split_return_codes_launch_nothing(dns):
    _lib, ptr, stream = _api()
    inp = di.split_inputs(3, 2)
    t = {k: _dev(inp[k]) for k in ("parents", "noise", "means", "scales", "quats")}
    nm, ns = Guarded(18), Guarded(18)

    def call(n_children, n_parents, parents=t["parents"]):
        rc = _lib.lib().dnsplat_densify_split(n_children, n_parents, ptr(parents), ptr(t["noise"]), ptr(t["means"]), ptr(t["scales"]),
                                              ptr(t["quats"]), ptr(nm.view), ptr(ns.view), stream())
        torch.cuda.synchronize()
        return rc

    assert call(0, 3) == 0 and call(0, 0) == 0
    assert call(6, 0) == INVALID_ARG and call(-1, 3) == INVALID_ARG and call(6, -1) == INVALID_ARG
    assert call(6, 3, parents=None) == INVALID_ARG
    assert nm.untouched() and ns.untouched()


# ---- dnsplat_densify_stats -------------------------------------------------------------------------------------------------------------

RADII = np.array([-3, 0, 1, 7, 640], dtype=np.int32)
INV_SIZES = (1.0 / 512.0, 1.0 / 640.0, 1.0 / 300.0)


@pytest.mark.parametrize("layout", ["contiguous", "stride16"])
@pytest.mark.parametrize("N", SIZES)
def test_stats_accumulate_per_row_and_skip_unseen_rows(dns, N, layout):
    """Three calls with different radii, gradients and inv_max_size.  Rows with radii <= 0 carry NaN gradients and must keep all
    three statistics bit for bit.  vis_counts and max_2Dsize are exact (float32(r) * float32(inv), as the kernel's comment says);
    xys_grad_norm after k calls is within (4 + k) 2^-24 of the float64 total: gx^2 and gy^2 round once each and their sum once
    (halved by the root: 1.5, rounded up to 2), the root once, the accumulation once per call, and one unit spare."""
    _lib, ptr, stream = _api()
    rng = np.random.default_rng(4000 + N)
    gn0 = rng.uniform(0.0, 1e-3, N).astype(np.float32)
    vis0 = rng.integers(1, 5, N).astype(np.float32)
    max0 = rng.uniform(0.0, 0.02, N).astype(np.float32)
    outs = [Guarded(N) for _ in range(3)]
    for o, init in zip(outs, (gn0, vis0, max0)):
        o.view.copy_(_dev(init))
    gn64, vis, mx = gn0.astype(np.float64), vis0.copy(), max0.copy()
    before = (gn0, vis0, max0)
    ever_seen = np.zeros(N, dtype=bool)
    for k, inv in enumerate(INV_SIZES, start=1):
        radii = RADII[rng.integers(0, RADII.size, N)]
        seen = radii > 0
        grads = (rng.normal(size=(N, 2)) * 10.0 ** rng.uniform(-6, -2, size=(N, 1))).astype(np.float32)
        grads[~seen] = np.nan
        if layout == "contiguous":
            stride = 2
            _, g_dev = _in_nan(grads)
        else:                   # columns 14 and 15 of gradient records of 16 floats, read in place; the other 14 are NaN
            stride = 16
            rec = np.full((N, 16), np.nan, dtype=np.float32)
            rec[:, 14:16] = grads
            g_dev = _in_nan(rec)[1][14:]
        assert (N - 1) * stride + 1 < g_dev.numel()              # the last row's two floats lie inside the buffer
        radii_dev = _dev(radii)
        rc = _lib.lib().dnsplat_densify_stats(N, ptr(radii_dev), ptr(g_dev), stride, inv, ptr(outs[0].view), ptr(outs[1].view),
                                              ptr(outs[2].view), stream())
        torch.cuda.synchronize()
        assert rc == 0, rc
        g64 = grads.astype(np.float64)
        gn64 = gn64 + np.where(seen, np.sqrt(g64[:, 0] ** 2 + g64[:, 1] ** 2), 0.0)
        vis = np.where(seen, vis + np.float32(1.0), vis)
        mx = np.where(seen, np.maximum(mx, radii.astype(np.float32) * np.float32(inv)), mx).astype(np.float32)
        ever_seen |= seen
        got = tuple(o.view.cpu().numpy() for o in outs)
        assert all(o.intact() for o in outs), "dnsplat_densify_stats wrote outside its outputs"
        for name, now, was in zip(("xys_grad_norm", "vis_counts", "max_2Dsize"), got, before):
            assert np.array_equal(now[~seen].view(np.int32), was[~seen].view(np.int32)), f"call {k} moved {name} of rows with radii <= 0"
        assert np.array_equal(got[1], vis), f"vis_counts after call {k}"
        assert np.array_equal(got[2].view(np.int32), mx.view(np.int32)), f"max_2Dsize after call {k}"
        worst = float((np.abs(got[0] - gn64) / ((4 + k) * U24 * gn64)).max())
        print(f"[densify] stats N={N} {layout} call {k}: xys_grad_norm worst error / allowance {worst:.3f}")
        assert worst <= 1.0, f"xys_grad_norm after call {k}: worst error / ((4 + k) 2^-24 total) = {worst:.2f}"
        before = got
    assert ever_seen.any() or N == 1
    assert N < 255 or (~ever_seen).any()


def test_stats_return_codes_launch_nothing(dns):
    _lib, ptr, stream = _api()
    N = 8
    radii, grads = _dev(np.full(N, 5, dtype=np.int32)), _dev(np.ones((N, 16), dtype=np.float32))
    outs = [Guarded(N) for _ in range(3)]

    def call(n, stride, g=grads):
        rc = _lib.lib().dnsplat_densify_stats(n, ptr(radii), ptr(g), stride, 1.0 / 512.0, ptr(outs[0].view), ptr(outs[1].view),
                                              ptr(outs[2].view), stream())
        torch.cuda.synchronize()
        return rc

    assert call(N, 1) == INVALID_ARG and call(N, 0) == INVALID_ARG and call(-1, 2) == INVALID_ARG
    assert call(N, 2, g=None) == INVALID_ARG
    assert call(0, 2) == 0
    assert all(o.untouched() for o in outs)


# ---- dnsplat_dn_depth_normals ----------------------------------------------------------------------------------------------------------

FRAMES = [(1, 1), (2, 5), (5, 2), (3, 3), (1, 300), (300, 1), (17, 31), (257, 3)]      # (W, H)
ALPHA_PATTERNS = ["random", "all_zero", "left_tap", "negative"]


def _frame(W, H, pattern):
    """depth, alphas [H,W] float32 (numpy).  Empty pixels (alpha <= 0) keep a raw depth of 0, as the compositing leaves them, except
    under ``all_zero``, where every depth is filled with the image-wide maximum."""
    rng = np.random.default_rng(100 * W + H)
    depth = rng.uniform(0.5, 5.0, size=(H, W)).astype(np.float32)
    alphas = rng.uniform(0.05, 1.0, size=(H, W)).astype(np.float32)
    if pattern == "random":
        empty = rng.random((H, W)) < 0.15
        alphas[empty], depth[empty] = 0.0, 0.0
    elif pattern == "all_zero":
        alphas[:] = 0.0
    elif pattern == "left_tap":          # the left tap of the first inner pixel (1, 1); on a frame without inner pixels, pixel 0
        i, j = (1, 0) if (W >= 3 and H >= 3) else (0, 0)
        alphas[i, j], depth[i, j] = 0.0, 0.0
    else:
        neg = rng.random((H, W)) < 0.3
        alphas[neg] = -alphas[neg]
        depth[neg] = 0.0
    return depth, alphas


@pytest.mark.parametrize("pattern", ALPHA_PATTERNS)
@pytest.mark.parametrize("W,H", FRAMES)
def test_depth_normals_on_frames_with_few_inner_pixels(dns, W, H, pattern):
    """The fill exact, the border exactly 0.5 (every pixel when W < 3 or H < 3), inner pixels within the allowance of
    test_gpu_losses.py.  Inputs in NaN-filled buffers, outputs in sentinel-filled ones: the clamped neighbour indices of the kernel
    are all that keeps it inside the image at these sizes."""
    _lib, ptr, stream = _api()
    fx, fy, cx, cy = 37.5, 52.25, 0.5 * W + 1.25, 0.5 * H - 0.75          # fx != fy, off-centre; all float32 numbers
    depth_np, alphas_np = _frame(W, H, pattern)
    # a row and a pixel of NaN either side: even a stencil that forgot its clamps would stay inside the buffers
    _, depth = _in_nan(depth_np, pad=GUARD + W + 1)
    _, alphas = _in_nan(alphas_np, pad=GUARD + W + 1)
    depth, alphas = depth.view(H, W), alphas.view(H, W)
    dmax = depth.max().reshape(1).contiguous()
    assert bool(torch.isfinite(dmax).all())
    P = W * H
    d_out, sn_out = Guarded(P), Guarded(3 * P)
    rc = _lib.lib().dnsplat_dn_depth_normals(W, H, fx, fy, cx, cy, ptr(depth), ptr(alphas), ptr(dmax), ptr(d_out.view), ptr(sn_out.view),
                                             stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert d_out.intact() and sn_out.intact(), "dnsplat_dn_depth_normals wrote outside its outputs"
    got_d, sn = d_out.view.view(H, W), sn_out.view.view(H, W, 3)
    filled32, sn32 = _restated_surface_normal(depth, alphas, fx, fy, cx, cy, torch.float32)
    _, sn64 = _restated_surface_normal(depth, alphas, fx, fy, cx, cy, torch.float64)
    assert torch.equal(got_d, filled32), "depth fill where(alpha > 0, depth, max)"
    assert bool(torch.isfinite(sn).all()), "a NaN from outside the image reached the normal image"
    border = torch.ones(H, W, dtype=torch.bool, device=DEV)
    border[1:-1, 1:-1] = False
    n_inner = max(W - 2, 0) * max(H - 2, 0)
    assert int((~border).sum()) == n_inner
    assert bool((sn[border] == 0.5).all())
    if pattern == "all_zero":
        assert bool((got_d == dmax).all())
    allow, _ = surface_normal_allowance(sn32, sn64)
    ratio = float(((sn.double() - sn64).abs() / allow).max())
    print(f"[densify] surface normal {W}x{H} {pattern}: {n_inner} inner pixels, worst error / allowance {ratio:.3f}")
    assert ratio <= 1.0, f"surface normal {W}x{H} {pattern}: worst error / (5e-6 + fp32 envelope) = {ratio:.2f}"
    if n_inner:
        assert bool((sn[~border] != 0.5).any())


# ---- dnsplat_camera_prepare ------------------------------------------------------------------------------------------------------------


def _poses():
    rng = np.random.default_rng(12)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    random = np.concatenate([q, rng.normal(size=(3, 1)) * 5], axis=1)
    identity = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    swap = np.concatenate([np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[1.5], [-2.25], [40.0]])], axis=1)
    return {"random": random.astype(np.float32), "identity": identity.astype(np.float32), "axis_swap": swap.astype(np.float32)}


INTRINSICS = (611.25, 598.5, 322.75, 241.125)          # fx, fy, cx, cy: float32 numbers


def _check_camera(c2w, viewmat, K, nf):
    """viewmat [16], K [9], nf [12] | None (numpy float32) against the float32 pose ``c2w`` [3,4]."""
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)      # noqa: E731
    R = c2w[:, :3].copy()
    R[:, 1:] = -R[:, 1:]                                   # y and z camera axes flipped (nerfstudio get_viewmat)
    t = c2w[:, 3]
    vm = viewmat.reshape(4, 4)
    assert np.array_equal(bits(vm[:3, :3]), bits(R.T)), "viewmat rotation is not a bit-exact copy of R^T"
    assert np.array_equal(bits(vm[3]), bits(np.array([0, 0, 0, 1], dtype=np.float32)))
    terms = R.astype(np.float64) * t.astype(np.float64)[:, None]          # [k, r] = R_kr t_k
    want, bound = -terms.sum(axis=0), 4 * U24 * np.abs(terms).sum(axis=0)   # three products, two sums, one unit spare
    assert (np.abs(vm[:3, 3].astype(np.float64) - want) <= bound).all(), (vm[:3, 3], want, bound)
    fx, fy, cx, cy = INTRINSICS
    assert np.array_equal(bits(K), bits(np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], dtype=np.float32)))
    if nf is not None:
        assert np.array_equal(bits(nf[:9].reshape(3, 3)), bits(c2w[:, :3].T)), "normal frame is not c2w[:3,:3]^T"
        assert np.array_equal(bits(nf[9:]), bits(t))


@pytest.mark.parametrize("with_zero,with_nf", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("n_zero_words", [1, 2, 9])
@pytest.mark.parametrize("pose", ["random", "identity", "axis_swap"])
def test_camera_prepare_through_the_c_entry(dns, pose, n_zero_words, with_zero, with_nf):
    _lib, ptr, stream = _api()
    c2w = _poses()[pose]
    vm, K, nf = Guarded(16), Guarded(9), Guarded(12)
    words = torch.full((n_zero_words + GUARD,), -1, dtype=torch.int32, device=DEV)          # 0xFFFFFFFF
    c2w_dev = _dev(c2w)
    rc = _lib.lib().dnsplat_camera_prepare(ptr(c2w_dev), *INTRINSICS, ptr(vm.view), ptr(K.view), ptr(nf.view) if with_nf else None,
                                           ptr(words) if with_zero else None, n_zero_words, stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert vm.intact() and K.intact() and nf.intact()
    _check_camera(c2w, vm.view.cpu().numpy(), K.view.cpu().numpy(), nf.view.cpu().numpy() if with_nf else None)
    if not with_nf:
        assert nf.untouched()
    if with_zero:
        assert bool((words[:n_zero_words] == 0).all()) and bool((words[n_zero_words:] == -1).all())
    else:
        assert bool((words == -1).all())


def test_camera_prepare_return_codes_launch_nothing(dns):
    _lib, ptr, stream = _api()
    c2w = _dev(_poses()["random"])
    vm, K = Guarded(16), Guarded(9)
    L = _lib.lib()
    assert L.dnsplat_camera_prepare(None, *INTRINSICS, ptr(vm.view), ptr(K.view), None, None, 0, stream()) == INVALID_ARG
    assert L.dnsplat_camera_prepare(ptr(c2w), *INTRINSICS, None, ptr(K.view), None, None, 0, stream()) == INVALID_ARG
    assert L.dnsplat_camera_prepare(ptr(c2w), *INTRINSICS, ptr(vm.view), None, None, None, 0, stream()) == INVALID_ARG
    torch.cuda.synchronize()
    assert vm.untouched() and K.untouched()


@pytest.mark.parametrize("pose", ["random", "identity", "axis_swap"])
def test_camera_prepare_through_the_op_layer(dns, pose):
    from dn_splatter_amd import _ops

    c2w = _poses()[pose]
    vm, K, nf, flag = _ops.camera_prepare(_dev(c2w)[None], *INTRINSICS, with_normal_frame=True, with_flag=True, n_depth_max=8)
    torch.cuda.synchronize()
    assert vm.shape == (4, 4) and K.shape == (3, 3) and nf.shape == (12,)
    _check_camera(c2w, vm.cpu().numpy().reshape(-1), K.cpu().numpy().reshape(-1), nf.cpu().numpy())
    assert flag.dtype == torch.int32 and int(flag[0]) == 0
    depth_max = _ops.DEPTH_MAX_OF[flag.data_ptr()]
    assert depth_max.shape == (8,) and bool((depth_max.view(torch.int32) == 0).all())
    vm2, K2, nf2 = _ops.camera_prepare(_dev(c2w), *INTRINSICS, with_normal_frame=False)
    torch.cuda.synchronize()
    assert nf2 is None
    _check_camera(c2w, vm2.cpu().numpy().reshape(-1), K2.cpu().numpy().reshape(-1), None)
