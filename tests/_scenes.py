"""Seeded scenes and comparison helpers shared by the CPU and GPU test files."""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# The parity bar BASELINE.json states: "tile/bin indices bit-exact, rendered RGB/depth/normal and grads
# within 1e-4 rel fp32".  "rel" is taken relative to the tensor's scale (max |reference|): gradients are
# sums of thousands of signed terms whose fp32 summation order differs between the oracle (pixel-major,
# omp atomics) and the GPU (splat-major registers + one atomic per tile), so an element-wise relative
# error is unbounded at cancelling entries while the scale-relative error stays ~1e-6.
REL_TOL = 1e-4


def rel_err(a, b) -> float:
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    if b.numel() == 0:
        return 0.0
    scale = b.abs().max().item()
    return (a - b).abs().max().item() / (scale + 1e-30)


# The compositing rule has hard cut-offs (skip a pair if sigma < 0 or alpha < 1/255; stop a pixel when T(1-alpha) <=
# 1e-4; pass no gradient through alpha where o vis > 0.999 — SURVEY.md A.6/A.7).  Two fp32 implementations whose exp()
# differ in the last place (libm expf in the oracle, v_exp_f32 on the GPU, ex2.approx in gsplat's CUDA) take the other
# side of a cut-off for a handful of (pixel, splat) pairs per frame.  The oracle therefore reports, per pixel, whether
# any of its decisions fell inside the fp32 rounding envelope of its threshold (info["borderline"], see
# orc_rasterize_fwd in oracle/oracle_impl.inc), and how much compositing weight those decisions can move at the pixel
# (info["flip_weight"]).  What the tests do with it:
#   * FORWARD: every pixel is compared.  A pixel without a flagged decision is held to REL_TOL; a borderline pixel is held to
#     REL_TOL + the finite bound that follows from its flip weight (flip_bound_* below: one flipped skip moves at most
#     2 alpha_k T_k max|c|, i.e. <= (2/255) T max|c|; a flipped stop at most what is left, ~1e-4 max|c|).  A kernel that wrote
#     garbage there fails.
#   * BACKWARD: the cotangents fed to BOTH backward passes are zero on the borderline pixels, so they contribute exactly
#     nothing to any gradient on either side; every gradient entry is held to REL_TOL (+ the fp64 envelope, assert_close).
EXCLUDED = []    # (what, n_borderline, n_pixels) of every masked comparison, printed by the tests


def keep_mask(borderline, what=""):
    """bool [H,W] of the pixels WITHOUT a flagged decision (they carry the cotangents of the backward comparison); records and
    prints how many are borderline."""
    b = borderline.reshape(borderline.shape[-2], borderline.shape[-1]).bool().cpu()
    n, tot = int(b.sum()), b.numel()
    EXCLUDED.append((what, n, tot))
    print(f"[parity] {what}: {n} of {tot} pixels borderline ({100.0 * n / max(tot, 1):.4f} %): images held to the flip bound there, "
          "cotangents zero on both sides")
    # a mask that swallowed a visible share of the image would make the comparison meaningless
    assert n <= max(8, 0.01 * tot), f"{what}: {n} of {tot} pixels flagged borderline"
    return ~b


# ---- finite bounds for the image values of borderline pixels (all float64, shaped like the image they bound) -------------
FLIP_SLACK = 1.05    # the weights are evaluated on the oracle's own trajectory; the other side's T differs by rounding


def flip_bound_linear(flip, cmax):
    """raw composite channels out_c = sum_i w_i c_ic (+ T bg_c): [..., H, W] flip weights, [C] per-channel max |c| -> [..., H, W, C]"""
    return FLIP_SLACK * 2.0 * flip.double()[..., None] * cmax.double().reshape(*([1] * flip.dim()), -1)


def flip_bound_alpha(flip):
    """alpha image = sum_i w_i"""
    return FLIP_SLACK * flip.double()


def flip_bound_ratio(flip, cmax, value, alpha):
    """expected depth = acc / max(alpha, 1e-10): |d| <= (|d acc| + |value| |d alpha|) / (alpha - |d alpha|); unbounded (inf) where
    the flagged weight is the whole of the pixel's alpha.  All [..., H, W]; cmax a number."""
    f = FLIP_SLACK * flip.double()
    den = alpha.double() - f
    b = (2.0 * f * float(cmax) + value.double().abs() * f) / den.clamp_min(1e-300)
    return torch.where(f > 0, torch.where(den > 0, b, torch.full_like(b, float("inf"))), torch.zeros_like(b))


def flip_bound_unit(flip, cmax, norm):
    """(n / |n| + 1) / 2 of a composited vector n [..., H, W, 3] with |n| = ``norm`` [..., H, W]: |d n|_2 <= sqrt(3) 2 w cmax and
    |d (n/|n|)| <= 2 |d n| / max(|n|, |n'|)"""
    dn = FLIP_SLACK * 2.0 * (3.0 ** 0.5) * float(cmax) * flip.double()
    b = torch.minimum(torch.ones_like(dn), dn / (norm.double() - dn).clamp_min(1e-300))
    return torch.where(dn > 0, torch.where(norm.double() > dn, b, torch.ones_like(b)), torch.zeros_like(b))[..., None].expand(*flip.shape, 3)


def render_bounds(info, render, alphas, render_mode):
    """Bounds for the outputs of a rasterization() call (oracle info dict): (bound like ``render``, bound like ``alphas``)."""
    flip = info["flip_weight"].reshape(render.shape[:-1])
    cmax = info["channel_absmax"]
    rb = flip_bound_linear(flip, cmax)
    if render_mode in ("ED", "RGB+ED"):
        rb = rb.clone()
        rb[..., -1] = flip_bound_ratio(flip, float(cmax[-1]), render.detach()[..., -1], alphas.detach().reshape(flip.shape))
    return rb, flip_bound_alpha(flip).reshape(alphas.shape)


def assert_borderline_bounded(r_g, r_o, info_o, what, alpha=False, render_mode="RGB+ED", alphas_o=None):
    """The forward comparison of one output of a rasterization() call over ALL pixels (tools/parity_seed_sweep.py)."""
    if alpha:
        assert_close(r_g, r_o, what, bound=flip_bound_alpha(info_o["flip_weight"].reshape(r_o.shape[:-1]))[..., None])
        return
    a_o = alphas_o if alphas_o is not None else info_o["_alphas"]
    rb, _ = render_bounds(info_o, r_o, a_o, render_mode)
    nc = r_o.shape[-1]
    assert_close_groups(r_g, r_o, what, [("colour", 0, nc - 1), ("depth", nc - 1, nc)], bound=rb)


def image_pixels(t, keep):
    """[..., H, W, C] or [..., H, W] image -> the rows of the kept pixels."""
    H, W = keep.shape
    t = t.detach().cpu()
    if t.shape[-2:] == (H, W):
        t = t.reshape(-1, H, W)[0][..., None]
    else:
        t = t.reshape(-1, H, W, t.shape[-1])[0]
    return t[keep]


def zero_borderline(v, keep):
    """Cotangent image with the borderline pixels zeroed (same shape as ``v``)."""
    H, W = keep.shape
    k = keep.to(v.dtype)
    if v.shape[-2:] == (H, W):
        return v * k
    return v * k[..., None]


# gradient entries per comparison that may need the fp64 envelope (beyond the plain tolerance): the suite's own scenes need none
# (worst plain ratio 0.77, gpurun_out margins), unseen anisotropic scenes a handful (tools/parity_seed_sweep.py)
ENVELOPE_MAX_ENTRIES = 8
ENVELOPE_MAX_FRACTION = 2e-5


def assert_close_groups(a, b, what, groups, dim=-1, **kw):
    """assert_close on slices of ``dim`` taken separately, each against the scale of ITS slice of the reference: rgb and expected
    depth of a render (depth ~ 3-13 would otherwise set the scale for the colours), the SH bands of a coefficient gradient
    (band 0 is an order of magnitude above the rest).  ``groups``: [(name, lo, hi), ...]."""
    env, keep, bound = kw.pop("envelope", None), kw.get("keep"), kw.pop("bound", None)
    for name, lo, hi in groups:
        idx = [slice(None)] * a.dim()
        idx[dim] = slice(lo, hi)
        if lo >= a.shape[dim]:
            continue
        assert_close(a[tuple(idx)], b[tuple(idx)], f"{what}[{name}]", envelope=None if env is None else env[tuple(idx)],
                     bound=None if bound is None else bound[tuple(idx)], **kw)


def sh_band_groups(K):
    """bands of a [N, K, 3] coefficient tensor (K = 16: full, 15: features_rest)"""
    if K == 16:
        return [("band 0", 0, 1), ("band 1", 1, 4), ("band 2", 4, 9), ("band 3", 9, 16)]
    if K == 15:
        return [("band 1", 0, 3), ("band 2", 3, 8), ("band 3", 8, 15)]
    return [("all", 0, K)]


def assert_close(a, b, what, tol=REL_TOL, atol=0.0, keep=None, envelope=None, bound=None):
    """|a-b| <= tol * max|b| + atol (+ envelope) (+ bound) at every entry (over the pixels selected by ``keep`` for images).
    ``bound``: per-entry finite bound for the image values of borderline pixels (flip_bound_*; 0 everywhere else), shaped like ``b``.
    ``atol`` is only for tensors that are mathematically zero (e.g. the quaternion gradient of isotropic
    Gaussians), where both sides hold nothing but fp32 rounding noise.
    ``envelope``: per-entry rounding envelope of the REFERENCE algorithm itself, FP32_ENVELOPE x |oracle in fp32 - the same
    oracle in fp64| (fp64_envelope below): on anisotropic scenes the fp32 evaluation of a few gradient entries (sums with
    heavy cancellation through an ill-conditioned 2x2 inverse) is itself 1-2.4 tolerances away from exact arithmetic
    (tools/parity_seed_sweep.py), so no fp32 implementation with a different summation order can be expected closer than that
    THERE.  Example (seed 103 of the sweep): d/d(scale_0) of a disc with scales (0.021, 0.30, 0.40) covering 140 tiles is
    -1.65686 in fp64, -1.65977 in the fp32 oracle, -1.66212 / -1.66300 in two HIP runs (the atomics' order differs): a
    relative error of 2e-3 in EVERY fp32 evaluation.  Everywhere else the envelope is ~1e-7 of the value and the comparison
    stays at the plain tolerance; with the envelope the suite's worst comparison sits at 0.52 of its allowance and 60 unseen
    seeds of the C1 scene pass (without it: 0.77, and 3 of 60 fail).
    DNSPLAT_MARGIN_LOG=<file>: append "what, worst error / allowance" for every comparison (how close the suite runs to its limits)."""
    a_ = a.detach().cpu()
    b_ = b.detach().cpu()
    assert a_.shape == b_.shape, f"{what}: shape {tuple(a_.shape)} vs {tuple(b_.shape)}"
    assert torch.isfinite(a_.float()).all(), f"{what}: non-finite values"
    if b_.numel() == 0:
        return
    scale = b_.double().abs().max().item()
    if keep is not None:
        a_, b_ = image_pixels(a_, keep), image_pixels(b_, keep)
    d = (a_.double() - b_.double()).abs().reshape(-1)
    allow = torch.full_like(d, tol * scale + atol)
    if envelope is not None:
        assert keep is None and envelope.shape == b.shape
        allow = allow + envelope.detach().cpu().double().reshape(-1)
    if bound is not None:
        assert keep is None and tuple(bound.shape) == tuple(b.shape), (what, tuple(bound.shape), tuple(b.shape))
        bd = bound.detach().cpu().double().reshape(-1)
        n_b = int((bd > 0).sum())
        if n_b:
            over = d[bd > 0] > (tol * scale + atol)
            print(f"[parity] {what}: {n_b} entries of borderline pixels held to their flip bound (median {float(bd[bd > 0].median()):.2e}); "
                  f"{int(over.sum())} of them differ by more than the plain tolerance, worst error / bound = "
                  f"{float((d[bd > 0] / (allow[bd > 0] + bd[bd > 0])).max()):.3f}")
        allow = allow + bd
    ratio = (d / allow.clamp_min(1e-300)) if d.numel() else d
    worst = ratio.max().item() if d.numel() else 0.0
    log = os.environ.get("DNSPLAT_MARGIN_LOG")
    if log:
        strict = (d.max().item() / (tol * scale + atol)) if d.numel() and tol * scale + atol > 0 else 0.0
        with open(log, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{what}\t{worst:.3f}\t{strict:.3f}\n")
    if envelope is not None and d.numel():
        # how many entries the plain tolerance alone would have failed: printed, and bounded — the envelope is for a handful of
        # ill-conditioned sums, not a second tolerance
        need = int((d > tol * scale + atol).sum())
        if need:
            print(f"[parity] {what}: {need} of {d.numel()} entries needed the fp64 rounding envelope")
        assert need <= max(ENVELOPE_MAX_ENTRIES, ENVELOPE_MAX_FRACTION * d.numel()), \
            f"{what}: {need} of {d.numel()} entries are beyond the plain tolerance (allowed: the fp64 envelope for at most " \
            f"{max(ENVELOPE_MAX_ENTRIES, int(ENVELOPE_MAX_FRACTION * d.numel()))})"
    if worst > 1.0:
        n_bad = int((ratio > 1.0).sum())
        raise AssertionError(f"{what}: max abs error {d.max().item():.3e} vs {tol:.1e} * scale {scale:.3e} + {atol:.1e}"
                             f"{' + fp64 envelope' if envelope is not None else ''}: worst error / allowance = {worst:.2f} "
                             f"({n_bad} of {d.numel()} entries beyond it)")


FP32_ENVELOPE = 4.0


def fp64_envelope(g32, g64):
    """FP32_ENVELOPE x |fp32 oracle - fp64 oracle| per entry: how far the reference algorithm's own fp32 evaluation is from
    exact arithmetic at that entry (assert_close)."""
    return FP32_ENVELOPE * (g32.detach().double() - g64.detach().double()).abs()


def assert_equal_int(a, b, what):
    a_ = a.detach().cpu()
    b_ = b.detach().cpu()
    assert a_.shape == b_.shape, f"{what}: shape {tuple(a_.shape)} vs {tuple(b_.shape)}"
    if not torch.equal(a_, b_):
        bad = (a_ != b_).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {a_.numel()} integers differ, first at {bad[0].tolist()}: "
                             f"{a_[tuple(bad[0])].item()} vs {b_[tuple(bad[0])].item()}")


def gsplat_inputs(N, W, H, focal, seed=0, sh_rest_std=0.1, view=0, anisotropic=False):
    """Activated inputs in the form dn_model.py:496-504 hands to gsplat.rasterization (CPU tensors)."""
    import dn_splatter_amd as dns
    from dn_splatter_amd import synthetic

    gp = synthetic.make_gauss_params(N, sh_rest_std=sh_rest_std, seed=seed)
    cam = synthetic.orbit_camera(view, width=W, height=H, focal=focal)
    g = torch.Generator().manual_seed(seed + 1000)
    scales_log = gp["scales"].detach().clone()
    if anisotropic:
        scales_log = scales_log + torch.randn(N, 3, generator=g) * 0.6
    opac_logit = gp["opacities"].detach().clone()
    if anisotropic:
        opac_logit = opac_logit + torch.randn(N, 1, generator=g) * 2.0
    quats = gp["quats"].detach()
    inp = dict(
        means=gp["means"].detach().clone(),
        quats=(quats / quats.norm(dim=-1, keepdim=True)).clone(),
        scales=torch.exp(scales_log),
        opacities=torch.sigmoid(opac_logit).squeeze(-1),
        colors=torch.cat([gp["features_dc"].detach()[:, None], gp["features_rest"].detach()], 1).clone(),
    )
    viewmat = dns.get_viewmat(cam.camera_to_worlds)
    K = cam.get_intrinsics_matrices()
    return inp, viewmat, K, cam


def to_leaf(inp, device):
    return {k: v.detach().to(device).clone().requires_grad_(True) for k, v in inp.items()}


def cotangents(shapes, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(s, generator=g) * 2 - 1 for s in shapes]


# ---- row-relative statistics ("1e-4 rel" held per Gaussian / per pixel, not only against the tensor's maximum) -----
# For a gradient tensor with one row per Gaussian: r_g = ||a_g - b_g||_2 / ||b_g||_2 over the rows whose reference norm is at
# least ROW_FLOOR x the largest row norm (rows below that are dominated by what cancels in them; they stay covered by the
# scale-relative comparison of assert_close).  Asserted where BOTH sides sum order-independently (HIP deterministic mode, oracle
# scatter accumulated in double), so that what is measured is the arithmetic, not the arrival order of atomics:
#   p99 <= ROW_P99 and max <= ROW_MAX of  max(0, ||d_g|| - FP32_ENVELOPE x ||oracle32_g - oracle64_g||) / ||ref_g||,
# i.e. outside the row's fp64 envelope.  The envelope is needed per row for the same reason as per entry (assert_close): the
# reference algorithm's OWN fp32 evaluation is that far from exact arithmetic — measured on the C1 scenes, oracle fp32 against oracle
# fp64, per Gaussian: p50 6e-6 / p99 2e-4 / max 2e-3 isotropic, p50 1.3e-4 / p99 2e-3 / max 8e-3 anisotropic (the backward starts
# from T_final = 1 - alpha image, a multiple of 2^-24: 6e-4 relative at a saturated pixel; 1 / (1 - alpha) at opacities near the
# cap) — so no second fp32 implementation can be held to 1e-4 per row against it, only to 1e-4 beyond that envelope.  The raw
# statistics are printed and logged beside the asserted ones.
# In the default (atomics) mode the statistics are logged only.  DNSPLAT_ROWREL_LOG=<file> appends one line per comparison.
# Measured (gpurun_out/r05a -> profiles/r05_rowrel.tsv): gradients, deterministic mode, outside the envelope: p99 <= 2.6e-5 everywhere
# (C2 full frame: 4.9e-6), max 1.6e-4 over the 20-scene sweep and 1.17e-3 for ONE of the 29 584 counted opacity rows of the full C2
# frame (an extreme-value statistic over 1 M rows: the kernels add a half tile's 128 terms in fp32 before the double sum, the oracle
# adds every term in double — 1e-6 x the row's cancellation factor, which the fp32-vs-fp64 envelope of the ORACLE does not contain);
# images, every mode: p99 <= 6.5e-7, max <= 1.4e-6 per pixel.  Hence: gradients p99 <= 1e-4, max <= 2e-3; images p99 <= 1e-5, max <= 1e-4.
ROW_FLOOR = 1e-3
ROW_P99 = 1e-4
ROW_MAX = 2e-3
PIX_P99 = 1e-5
PIX_MAX = 1e-4
# Default (atomics) mode, where the arrival order of ~30 atomic rows per Gaussian adds its own noise: measured over the suite
# (profiles/r05c_rowrel.tsv) outside the envelope p99 <= 9.0e-5, max <= 1.3e-3; where a test computes no fp64 run (no envelope) the
# raw statistics are p99 <= 5.0e-4, max <= 8.0e-3 (C5 frame, opacities).  Asserted with a factor ~2-4 of room — a guard against a
# kernel that corrupts whole rows which the tensor-scale comparison would not see, not a statement about rounding.
ROW_P99_DEFAULT, ROW_MAX_DEFAULT = 2e-4, 5e-3
ROW_P99_RAW, ROW_MAX_RAW = 1e-3, 2e-2


def row_rel_stats(a, b, b64=None, floor=ROW_FLOOR):
    """(p50, p99, max, max outside the fp64 envelope, rows counted, rows total) of the row-relative L2 error; rows = all leading
    dimensions but the last (a 1-D tensor is one entry per row)."""
    a_ = a.detach().double().cpu()
    b_ = b.detach().double().cpu()
    assert a_.shape == b_.shape, (a_.shape, b_.shape)
    if b_.dim() == 1:
        a_, b_ = a_[:, None], b_[:, None]
    a_, b_ = a_.reshape(-1, b_.shape[-1]), b_.reshape(-1, b_.shape[-1])
    nb = b_.norm(dim=1)
    if nb.numel() == 0 or float(nb.max()) == 0.0:
        return None
    sel = nb >= floor * nb.max()
    err = (a_ - b_).norm(dim=1)[sel]
    r = err / nb[sel]
    r_out = r
    if b64 is not None:
        e64 = b64.detach().double().cpu()
        e64 = (e64[:, None] if e64.dim() == 1 else e64).reshape(-1, b_.shape[-1])
        env = FP32_ENVELOPE * (b_ - e64).norm(dim=1)[sel]
        r_out = (err - env).clamp_min(0) / nb[sel]

    def q(t, f):
        if not t.numel():
            return 0.0
        k = min(t.numel() - 1, int(f * t.numel()))
        return float(torch.sort(t).values[k])       # torch.quantile refuses more than 16 M entries
    return q(r, 0.5), q(r, 0.99), float(r.max()), float(r_out.max()), int(sel.sum()), int(nb.numel()), q(r_out, 0.99)


ROWREL_ENFORCE = os.environ.get("DNSPLAT_ROWREL_ENFORCE", "1") != "0"      # 0: log the statistics, assert nothing (exploration runs)


def both_sides_order_independent(orc) -> bool:
    """True when the HIP path runs its deterministic gradient mode AND the oracle accumulates its scatter in double: the only
    configuration in which a row-relative bound on gradients measures arithmetic rather than the arrival order of atomics."""
    from dn_splatter_amd import _ops
    return bool(_ops.DETERMINISTIC["on"]) and bool(orc.lib().orc_get_exact_accum())


def check_rows(a, b, what, b64=None, enforce=False, p99=None, rmax=None, n_rows=None, strict=True):
    """``n_rows``: reshape to [n_rows, -1] first (one row per Gaussian whatever the trailing shape).  ``strict``: both sides sum
    order-independently (the deterministic-mode bounds ROW_P99 / ROW_MAX); otherwise the default-mode guards (with / without an fp64
    envelope)."""
    enforce = enforce and ROWREL_ENFORCE
    if p99 is None:
        p99 = ROW_P99 if strict else (ROW_P99_DEFAULT if b64 is not None else ROW_P99_RAW)
    if rmax is None:
        rmax = ROW_MAX if strict else (ROW_MAX_DEFAULT if b64 is not None else ROW_MAX_RAW)
    if n_rows is not None:
        a, b = a.detach().reshape(n_rows, -1), b.detach().reshape(n_rows, -1)
        b64 = None if b64 is None else b64.detach().reshape(n_rows, -1)
    st = row_rel_stats(a, b, b64)
    if st is None:
        return None
    p50, p99_, mx, mx_out, n, tot, p99_out = st
    print(f"[parity] {what}: row-relative error over {n} of {tot} rows: p50 {p50:.2e}  p99 {p99_:.2e}  max {mx:.2e}"
          + (f"  (outside the fp64 envelope: p99 {p99_out:.2e}  max {mx_out:.2e})" if b64 is not None else ""))
    log = os.environ.get("DNSPLAT_ROWREL_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{what}\t{n}\t{tot}\t{p50:.3e}\t{p99_:.3e}\t{mx:.3e}\t{p99_out:.3e}\t"
                    f"{mx_out:.3e}\t{('asserted <= %.0e / %.0e' % (p99, rmax)) if enforce else 'logged'}\n")
    if enforce:
        if p99_out > p99 or mx_out > rmax:
            print(f"[parity] {what}: ROW-RELATIVE BOUND EXCEEDED (p99 {p99_out:.3e} vs {p99:.1e}, max {mx_out:.3e} vs {rmax:.1e})")
        assert p99_out <= p99, f"{what}: p99 of the row-relative error{' outside the fp64 envelope' if b64 is not None else ''} {p99_out:.3e} > {p99:.1e}"
        assert mx_out <= rmax, f"{what}: largest row-relative error{' outside the fp64 envelope' if b64 is not None else ''} {mx_out:.3e} > {rmax:.1e}"
    return st


def check_pixels(a, b, what, keep=None, enforce=False, p99=PIX_P99, rmax=PIX_MAX):
    """The same statistic per PIXEL of an image [.., H, W, C] (over its C channels), borderline pixels left to their flip bound."""
    a_, b_ = a.detach().cpu(), b.detach().cpu()
    if keep is not None:
        a_, b_ = image_pixels(a_, keep), image_pixels(b_, keep)
    return check_rows(a_, b_, what, enforce=enforce, p99=p99, rmax=rmax)


# ---- condition-aware bound for EVERY visible Gaussian --------------------------------------------------------
# The floor-based statistic above counts the rows whose reference norm is >= 1e-3 x the largest (about 5 % of the visible Gaussians
# of the C2 frame).  This one covers ALL rows with radii > 0, each against its OWN running error bound from the oracle's
# ConditionTrace (oracle/oracle.py, orc_rasterize_bwd_cond in oracle_impl.inc), chained to the parameters through |J|:
#     worst case            ||d_g||_2 <= COND_C      x 2^-24 x ||A_g||_2     A = sum of term magnitudes x rounding count kappa
#     independent roundings ||d_g||_2 <= COND_LAMBDA x 2^-24 x ||S_g||_2     S = sqrt(sum of squared magnitudes x variance count)
# d = HIP (deterministic mode) - oracle fp32 (scatter in double): two fp32 evaluations of the same rule set from the same inputs.
# A row whose bound is zero (no pair blended it) must be exactly equal.  The constants are ONE pair for every tensor, scene and size;
# measured (profiles/r06_rowrel.tsv): see the numbers printed by check_rows_conditioned.  In the default (atomics) mode the same
# statistic is asserted with COND_*_DEFAULT (the arrival order of ~30 fp32 atomic rows per Gaussian adds roundings the model of the
# double-accumulated reduction does not count).
U24 = 2.0 ** -24
# c = 4.  The bound is on ONE evaluation's distance from exact arithmetic; HIP and the oracle's fp32 run are each within ~1 x of it and may
# sit on opposite sides of the exact value (2 x), with a factor 2 of room.  Worst row seen: 1.45 x A (seed 104 anisotropic, an SH-coefficient
# row of a 48-pixel-radius splat, tools/cond_outlier.py; 1.96 before kappa counted the splat's own rounded conic / centre, which shift the
# alphas of all its pixels the same way: oracle.input_perturbation); everything else <= 0.60 A over the suite and the sweep's other 59
# scenes (median 0.08), <= 2.0 S everywhere; C2 frame 0.22 A / 0.77 S.
# With atomics the arrival order adds the roundings of ~30 sequential fp32 adds per Gaussian: c = 8 there.
COND_C, COND_LAMBDA = 4.0, 8.0
COND_C_DEFAULT, COND_LAMBDA_DEFAULT = 8.0, 16.0


def check_rows_conditioned(a, b, cond_a, cond_s, visible, what, enforce=True, strict=True):
    """``a`` (HIP) vs ``b`` (oracle) gradient tensors with one row per Gaussian; ``cond_a`` / ``cond_s``: the A / S bounds of the same
    shape (units of one rounding); ``visible`` bool [N].  Returns (rows counted, worst ratio vs A, worst ratio vs S)."""
    N = visible.numel()
    a_ = a.detach().double().cpu().reshape(N, -1)[visible]
    b_ = b.detach().double().cpu().reshape(N, -1)[visible]
    ca = cond_a.detach().double().reshape(N, -1)[visible]
    cs = cond_s.detach().double().reshape(N, -1)[visible]
    d = (a_ - b_).norm(dim=1)
    na, ns, nb = ca.norm(dim=1), cs.norm(dim=1), b_.norm(dim=1)
    dead = na == 0
    n_dead_bad = int((d[dead] != 0).sum())
    live = ~dead
    ra = d[live] / (U24 * na[live])
    rs = d[live] / (U24 * ns[live]).clamp_min(1e-300)
    rel_bound = (U24 * ns[live] / nb[live].clamp_min(1e-300))
    rel_err = d[live] / nb[live].clamp_min(1e-300)

    def q(t, f):
        if not t.numel():
            return 0.0
        k = min(t.numel() - 1, int(f * t.numel()))
        return float(torch.sort(t).values[k])
    c_lim, l_lim = (COND_C, COND_LAMBDA) if strict else (COND_C_DEFAULT, COND_LAMBDA_DEFAULT)
    n = int(visible.sum())
    wa, ws = (float(ra.max()) if ra.numel() else 0.0), (float(rs.max()) if rs.numel() else 0.0)
    print(f"[parity] {what}: ALL {n} visible rows ({int(live.sum())} with a non-zero bound, {int(dead.sum())} exactly equal): "
          f"error / (2^-24 A): p50 {q(ra, .5):.2e} p99 {q(ra, .99):.2e} max {wa:.3f} (<= {c_lim});  error / (2^-24 S): p50 {q(rs, .5):.2e} "
          f"p99 {q(rs, .99):.2e} max {ws:.3f} (<= {l_lim});  row-relative error p50 {q(rel_err, .5):.1e} p99 {q(rel_err, .99):.1e} max "
          f"{(float(rel_err.max()) if rel_err.numel() else 0.0):.1e};  bound 2^-24 S / |ref| p50 {q(rel_bound, .5):.1e} p99 {q(rel_bound, .99):.1e}")
    log = os.environ.get("DNSPLAT_CONDREL_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{what}\t{n}\t{N}\t{int(live.sum())}\t{q(ra, .5):.3e}\t{q(ra, .99):.3e}\t{wa:.3e}\t"
                    f"{q(rs, .5):.3e}\t{q(rs, .99):.3e}\t{ws:.3e}\t{q(rel_err, .5):.3e}\t{q(rel_err, .99):.3e}\t"
                    f"{(float(rel_err.max()) if rel_err.numel() else 0.0):.3e}\t{q(rel_bound, .5):.3e}\t{q(rel_bound, .99):.3e}\t"
                    f"{('asserted <= %g A, <= %g S' % (c_lim, l_lim)) if enforce else 'logged'}\n")
    if enforce:
        assert n_dead_bad == 0, f"{what}: {n_dead_bad} rows differ although no pair contributes to them"
        assert wa <= c_lim, f"{what}: a row is {wa:.3f} x its worst-case running error bound (allowed {c_lim})"
        assert ws <= l_lim, f"{what}: a row is {ws:.3f} standard deviations of the independent-roundings model off (allowed {l_lim})"
    return n, wa, ws


# ---- raster-level scene for the backward of borderline pixels (tests/test_borderline_bounds.py, tests/test_gpu_parity.py) ---------


def raster_level_scene(orc, seed, N=10_000, W=256, H=256, focal=160.0, D=4, anisotropic=True, view=0):
    """Projected Gaussians (the oracle's own projection), their sorted tile lists, random per-Gaussian channels and a background:
    everything gsplat's rasterize_to_pixels takes, as CPU tensors, plus the oracle's forward with its borderline mask."""
    inp, viewmat, K, _ = gsplat_inputs(N, W, H, focal=focal, seed=seed, anisotropic=anisotropic, view=view)
    radii, xys, depths, conics, _comp, tiles = orc.project_fwd(inp["means"], inp["quats"], inp["scales"], viewmat[0], K[0], W, H)
    tw, th = (W + 15) // 16, (H + 15) // 16
    _t, ids, fid = orc.isect_tiles(xys, radii, depths, 16, tw, th)
    offs = orc.isect_offset_encode(ids, tw, th)
    g = torch.Generator().manual_seed(seed + 77)
    cols = torch.rand(N, D, generator=g)
    bg = torch.rand(D, generator=g)
    border = torch.zeros(H, W, dtype=torch.uint8)
    flip = torch.zeros(H, W, dtype=torch.float32)
    render, alphas, last = orc.rasterize_fwd(xys, conics, cols, inp["opacities"], bg, W, H, 16, offs, fid, border, flip)
    return dict(W=W, H=H, D=D, N=N, xys=xys, conics=conics, colors=cols, opacities=inp["opacities"], background=bg, radii=radii,
                depths=depths, tiles=tiles, offsets=offs, flatten_ids=fid, render=render, alphas=alphas, last_ids=last,
                borderline=border.bool(), gen=g)


# ---- raster-level scenes with an exact list structure (tests/test_gpu_raster_edges.py, tests/test_edge_scenes.py) ---------------
# Every contributing splat is a point of sigma EDGE_SIGMA centred (within EDGE_JITTER) on ONE pixel centre: alpha there is its opacity
# (x 0.965 at least), at every other pixel centre below 0.5 / 255.  So each list entry reaches exactly one pixel of one half tile, and
# a recipe fixes, entry by entry, which pixel blends it, which pixel saturates where and how many entries a half tile keeps.
EDGE_COUNTS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 143, 159, 160, 161, 191, 192, 193, 255, 256,
               257, 383, 384, 385)
# never: no pixel saturates.  early: one pixel saturates at list index 4, most pixels blend nothing after batch 0 and two pixels
# walk to the end.  boundary: pixels saturate at indices 64, 128, 256, 384 (their last blended entry ends a batch / a bucket).
# allstop: every pixel that blends anything saturates, about 3/4 down the list; the entries after that reach only stopped pixels,
# so the backward's bound `hi` lies inside the list and the entries above it are kept but never walked.
EDGE_STOPS = ("never", "early", "boundary", "allstop")
EDGE_OFFSETS = (0, 1, 63)         # range_start mod 64 of the tiles under test (padding entries in the tile in front of each)
EDGE_SIGMA = 0.27
EDGE_JITTER = 0.05
LOW_OPACITY = (0.0055, 0.009)     # low-alpha runs: alpha 1.35/255 .. 2.3/255 at the splat's own pixel, below 0.01/255 anywhere else
STACK_OPACITY = 0.95              # three of them leave T <= 5.7e-4, the fourth would take T below 4.7e-5: the pixel stops there
CAP_OPACITY = 0.9999              # 0.003 px off its pixel centre: o vis = 0.9998 > 0.999, alpha clamped: T = 1e-3, then 1e-6 (stop)
CAP_OFFSET = 0.003                # (not 0: sigma = 0 exactly would sit on the "skip if sigma < 0" decision)
CULL_OPACITY = 0.002              # listed but culled: below 1/255 at every point
EDGE_BOUNDARY_STOPS = (64, 128, 256, 384)


def edge_pixel(k):
    """A spread walk over the 128 pixels (16 x 8, row-major) of a half tile."""
    return (k * 37) % 128


def _low(i):
    lo, hi = LOW_OPACITY
    return lo + (hi - lo) * ((i * 0.6180339887) % 1.0)


def allstop_groups(n):
    """``allstop``: the first 4 x (this) entries are stacks of four on distinct pixels."""
    return max(1, (3 * n // 4) // 4)


def half_recipe(n, stop, cap=False):
    """The ``n`` contributing entries of one half tile in list order: [(pixel 0..127, opacity, capped)]."""
    stack = CAP_OPACITY if cap else STACK_OPACITY
    if stop == "never" or (stop == "early" and n < 5) or (stop == "allstop" and n < 8):
        return [(edge_pixel(i), _low(i), False) for i in range(n)]
    out = []
    if stop == "early":
        q, tail = 5, (77, 121)
        for i in range(n):
            if 1 <= i <= 4:
                out.append((q, stack, cap))
            elif i < 64:
                p = edge_pixel(i)
                out.append((p if p != q else q + 1, _low(i), False))
            else:
                out.append((tail[i % 2], _low(i), False))
        return out
    if stop == "boundary":
        stops = {s: 3 + 9 * (s // 64) for s in EDGE_BOUNDARY_STOPS if s < n}
        pix = set(stops.values())
        for i in range(n):
            s = next((s for s in stops if s - 3 <= i <= s), None)
            if s is not None:
                out.append((stops[s], stack, cap))
            else:
                p = edge_pixel(i)
                out.append((p if p not in pix else (p + 64) % 128, _low(i), False))
        return out
    if stop == "allstop":
        k = 4 * allstop_groups(n)
        return [(edge_pixel(i // 4), stack, cap) if i < k else (edge_pixel(0), _low(i), False) for i in range(n)]
    raise ValueError(stop)


# ``edge_frame(cell=)``: length of a run of one tile inside its cell's list, by cell index, in pairs of depth slots — a tile's own order
# has two slots per case entry, the even one for the entry and the odd one for the culled entry ``interleave`` puts in front of every
# second case entry.  So a run is this many case entries, plus half as many culled ones with ``interleave``.  Long runs leave whole
# 64-entry batches of a cell's list to ONE tile (all-foreign batches for the others), single entries spread a half tile's bucket over
# many sparse batches
EDGE_CELL_RUNS = (128, 1, 40)


def edge_frame(cases, W, H, *, interleave=False, phase=0, end_align=False, cap=False, seed=0, pad_to=None, cell=None):
    """Raster-level scene (the inputs of rasterize_to_pixels, CPU tensors) from ``cases`` = [(tile, half, n, stop)], one case per tile.
    Ids: the case entries first (in case order, then list order), then the culled entries ``interleave`` puts in front of every
    second case entry, then the padding; ``pad_to`` appends invisible splats (radius 0) up to that many records.
    ``phase``: the list of case k starts at range_start mod 64 = EDGE_OFFSETS[(k + phase) % 3] (padding entries at the end of the
    tile in front of it, which holds no case).  ``end_align``: the last tile of the frame holds a case, and its list ends on a
    multiple of 64.  Depths are distinct integers in recipe order.  Channels: ``colors8`` / ``background8``, 8 of them in [0.1, 0.9]
    (a D-channel render takes the first D).
    ``cell`` = (cw, ch) tiles: the depths of the tiles of one list cell of that shape interleave — runs of EDGE_CELL_RUNS case entries
    (with the culled entries ``interleave`` puts between them) of each tile in turn — where without it they are assigned tile by
    tile.  Within a tile the order stays the recipe's, so a tile's own entries, the list lengths and every per-tile regime are what they are without it; the CELL's list, which is what the kernels walk
    when the lists are kept per cell, is then mostly someone else's to each of its half tiles."""
    tw, th = (W + 15) // 16, (H + 15) // 16
    T = tw * th
    cases = sorted(cases)
    case_tiles = [c[0] for c in cases]
    assert len(set(case_tiles)) == len(case_tiles), "one case per tile"
    assert all(1 <= t < T and t - 1 not in case_tiles for t in case_tiles), "the tile in front of a case holds its padding"
    g = torch.Generator().manual_seed(seed)
    stride = 2 * max([c[2] for c in cases] + [1]) + 2 * 64 + 8
    assert (T + 1) * stride < 2 ** 24, "depths must stay exact in float32"
    if cell is not None:
        cw, ch = cell
        lw, n_cells, K = -(-tw // cw), (-(-tw // cw)) * (-(-th // ch)), cw * ch
        span = K * (stride + 2 * max(EDGE_CELL_RUNS))
        assert (n_cells + 1) * span < 2 ** 24, "depths must stay exact in float32"

    def dep(t, local):
        """the depth of the entry at position ``local`` (< stride) of tile t's own order"""
        if cell is None:
            return 1.0 + t * stride + local
        c, r = (t // tw // ch) * lw + t % tw // cw, (t // tw % ch) * cw + t % tw % cw
        G = 2 * EDGE_CELL_RUNS[c % len(EDGE_CELL_RUNS)]
        return 1.0 + c * span + (local // G) * K * G + r * G + local % G

    rows = []              # (x, y, conic a, b, c, opacity, radius, depth, kind) kind: 0 case, 1 interleaved culled, 2 padding
    a_pt = 1.0 / EDGE_SIGMA ** 2
    for t, h, n, stop in cases:
        x0, y0 = 16 * (t % tw), 16 * (t // tw) + 8 * h
        jit = torch.rand(max(n, 1), 3, generator=g) * 2 - 1
        for i, (p, o, centred) in enumerate(half_recipe(n, stop, cap)):
            dx, dy = (CAP_OFFSET, CAP_OFFSET) if centred else (EDGE_JITTER * float(jit[i, 0]), EDGE_JITTER * float(jit[i, 1]))
            rows.append((x0 + p % 16 + 0.5 + dx, y0 + p // 16 + 0.5 + dy, a_pt, 0.0 if centred else 0.3 * float(jit[i, 2]), a_pt, o, 1,
                         dep(t, 2 * i + 2), 0))
    if interleave:
        for t, h, n, stop in cases:
            x0, y0 = 16 * (t % tw), 16 * (t // tw)
            for i in range(0, n, 2):
                rows.append((x0 + 8.0, y0 + 8.0, 4.0, 0.0, 4.0, CULL_OPACITY, 1, dep(t, 2 * i + 1), 1))

    def boxes(x, y, r):
        """gsplat's tile box (A.3) of centres x, y and radii r, clipped to the grid"""
        x, y, r = (torch.as_tensor(v, dtype=torch.float32) for v in (x, y, r))
        bx0 = torch.clamp(torch.floor((x - r) / 16), 0, tw).long()
        bx1 = torch.clamp(torch.ceil((x + r) / 16), 0, tw).long()
        by0 = torch.clamp(torch.floor((y - r) / 16), 0, th).long()
        by1 = torch.clamp(torch.ceil((y + r) / 16), 0, th).long()
        return bx0, bx1, by0, by1

    # list lengths without the padding (neighbours' entries whose box reaches a tile are in its list too)
    base = [0] * T
    if rows:
        bx0, bx1, by0, by1 = boxes([r[0] for r in rows], [r[1] for r in rows], [float(r[6]) for r in rows])
        for i in range(len(rows)):
            for ty in range(int(by0[i]), int(by1[i])):
                for tx in range(int(bx0[i]), int(bx1[i])):
                    base[ty * tw + tx] += 1
    target = {t: EDGE_OFFSETS[(k + phase) % len(EDGE_OFFSETS)] for k, t in enumerate(case_tiles)}
    if end_align:
        assert case_tiles[-1] == T - 1
        target[T - 1] = (-base[T - 1]) % 64
    fill = [0] * T
    start = 0
    for t in range(T):
        if t + 1 in target:
            fill[t] = (target[t + 1] - (start + base[t])) % 64
        start += base[t] + fill[t]
    for t in range(T):
        x0, y0 = 16 * (t % tw), 16 * (t // tw)
        for j in range(fill[t]):
            rows.append((x0 + 8.0, y0 + 8.0, 4.0, 0.0, 4.0, CULL_OPACITY, 1, dep(t, stride - 72 + j), 2))
    R = torch.tensor([r[:6] for r in rows], dtype=torch.float64).reshape(-1, 6)
    radii = torch.tensor([r[6] for r in rows], dtype=torch.int32)
    depths = torch.tensor([r[7] for r in rows], dtype=torch.float32)
    kind = torch.tensor([r[8] for r in rows], dtype=torch.int8)
    if pad_to is not None:
        extra = pad_to - R.shape[0]
        assert extra >= 0
        R = torch.cat([R, torch.tensor([[8.0, 8.0, 4.0, 0.0, 4.0, CULL_OPACITY]], dtype=torch.float64).repeat(extra, 1)])
        radii = torch.cat([radii, torch.zeros(extra, dtype=torch.int32)])
        depths = torch.cat([depths, torch.ones(extra)])
        kind = torch.cat([kind, torch.full((extra,), 3, dtype=torch.int8)])
    N = R.shape[0]
    xys, conics, opac = R[:, 0:2].float().contiguous(), R[:, 2:5].float().contiguous(), R[:, 5].float().contiguous()
    bx0, bx1, by0, by1 = boxes(xys[:, 0], xys[:, 1], radii.float())
    tiles = torch.where(radii > 0, (bx1 - bx0) * (by1 - by0), torch.zeros_like(bx0)).to(torch.int32)
    gc = torch.Generator().manual_seed(1000 + seed)
    cols = 0.1 + 0.8 * torch.rand(N, 8, generator=gc)
    bg = 0.1 + 0.8 * torch.rand(8, generator=gc)
    return dict(W=W, H=H, N=N, xys=xys, conics=conics, opacities=opac, colors8=cols, background8=bg, radii=radii, depths=depths,
                tiles=tiles, kind=kind, n_case=int((kind == 0).sum()), cases=cases, target=target, fill=fill, tw=tw, th=th, phase=phase,
                interleave=interleave, cap=cap, cell=cell)


def edge_tile_boxes(s):
    """gsplat's tile boxes (A.3) of an edge frame as the binning takes them: int32 [N, 2] = (first tile id, w | h << 16), 0 | 0 for the
    invisible records."""
    x, y, r = s["xys"][:, 0], s["xys"][:, 1], s["radii"].float()
    tw, th = s["tw"], s["th"]
    bx0 = torch.clamp(torch.floor((x - r) / 16), 0, tw).long()
    bx1 = torch.clamp(torch.ceil((x + r) / 16), 0, tw).long()
    by0 = torch.clamp(torch.floor((y - r) / 16), 0, th).long()
    by1 = torch.clamp(torch.ceil((y + r) / 16), 0, th).long()
    vis = s["radii"] > 0
    assert torch.equal(torch.where(vis, (bx1 - bx0) * (by1 - by0), torch.zeros_like(bx0)).to(torch.int32), s["tiles"])
    z = torch.zeros_like(bx0)
    return torch.stack([torch.where(vis, by0 * tw + bx0, z), torch.where(vis, (bx1 - bx0) | ((by1 - by0) << 16), z)], 1).to(torch.int32)


def edge_cell_lists(frames, sx, sy):
    """The lists of a batch of edge frames per cell of 2^sx x 2^sy tiles, from the frames' tile boxes and depths alone (the numpy
    restatement of _cell_binning_ref.py): (offsets [C * cells + 1] int64, flatten_ids int64 with entry = camera x N + record)."""
    import numpy as np

    import _cell_binning_ref as ref

    boxes = torch.cat([edge_tile_boxes(s) for s in frames]).numpy()
    radii = torch.cat([s["radii"] for s in frames]).numpy()
    depths = torch.cat([s["depths"] for s in frames]).numpy()
    got = ref.cell_lists(boxes, radii, depths, frames[0]["tw"], frames[0]["th"], len(frames), sx, sy)
    return torch.from_numpy(got["offsets"].astype(np.int64)), torch.from_numpy(got["flatten_ids"].astype(np.int64))


def edge_main_cases():
    """Every count x every stop pattern, one per half tile: 124 cases on tiles 1, 3, ..., 247 of a 256 x 256 frame (16 x 16 tiles)."""
    cases = []
    for ci, n in enumerate(EDGE_COUNTS):
        for si, stop in enumerate(EDGE_STOPS):
            k = len(cases)
            cases.append((2 * k + 1, (ci + si) % 2, n, stop))
    return cases


_PARTIAL = [(1, 0, 65, "early"), (5, 1, 129, "allstop"), (9, 1, 97, "never"), (11, 0, 161, "boundary")]
# name: (W, H, cases, edge_frame options).  height40 / height44: the bottom half tiles of the last tile row lie outside the image /
# half inside it (tile 9's bottom half carries a case in both).  deep: one list of 20 000+ low-alpha entries.  cap: opacities above
# the 0.999 cap on every stack.
EDGE_SMALL = {
    "height40": (64, 40, _PARTIAL, {}),
    "height44": (64, 44, _PARTIAL, {}),
    "deep": (32, 32, [(3, 1, 20001, "never")], {}),
    "cap": (128, 128, [(2 * k + 1, k % 2, n, st) for k, (n, st) in
                       enumerate([(n, st) for n in (17, 65, 129, 161, 257) for st in ("early", "boundary", "allstop")])], {"cap": True}),
}
# a batch of three cameras (128 x 128), a different recipe in each; every camera's lists end on a multiple of 64, the last tile's
# with a case in it
EDGE_CAMERAS = [
    [(1, 0, 129, "never"), (5, 1, 33, "early"), (9, 0, 161, "boundary"), (63, 1, 65, "allstop")],
    [(3, 1, 97, "allstop"), (13, 0, 257, "never"), (63, 0, 31, "boundary")],
    [(7, 0, 193, "early"), (21, 1, 160, "never"), (63, 1, 64, "never")],
]


def edge_cameras(**kw):
    """The three frames of EDGE_CAMERAS with the same number of records (invisible padding)."""
    n = max(edge_frame(c, 128, 128, end_align=True, seed=7 + i, **kw)["N"] for i, c in enumerate(EDGE_CAMERAS))
    return [edge_frame(c, 128, 128, end_align=True, seed=7 + i, pad_to=n, **kw) for i, c in enumerate(EDGE_CAMERAS)]


def edge_lists(orc, s):
    """The reference binning of an edge frame: (offsets [th, tw] int32, flatten_ids int32), the oracle's (gsplat's) lists."""
    t, ids, fid = orc.isect_tiles(s["xys"], s["radii"], s["depths"], 16, s["tw"], s["th"])
    assert torch.equal(t, s["tiles"]), "tiles per Gaussian differ from the frame's box count"
    return orc.isect_offset_encode(ids, s["tw"], s["th"]), fid


def edge_model(s, offs, fid, cells=None):
    """What the compositing kernels do on each half tile of ``s``, recomputed in float64 from the lists (offs, fid): one dict per
    (non-empty tile, half) with rs / re (list range), kept (entries with alpha >= 1/255 at some pixel centre of the half: what the
    rectangle test keeps), contrib (those reaching an in-image pixel), stop {pixel: list index (relative) of the entry that stops it},
    hi (the backward's walk bound, relative; -1: no work), queue (kept entries up to hi), the bucket sequence with keep masks (takes /
    carries _masks: 64-entry batches aligned to the list start) and without (_scan: 64 entries down from hi) and the fold of the last
    bucket in the default mode.  Asserts that no alpha lies within 30 % of 1/255 and no transmittance within 20 % of 1e-4.
    ``cells`` = (sx, sy): (offs, fid) are the lists of ONE camera per cell of 2^sx x 2^sy tiles (edge_cell_lists), and every half tile of
    a cell walks the cell's list: an entry is the half tile's only if its own tile box holds the tile (the kernels' rule,
    dns_tile_in_box) and the rectangle test keeps it — rs, re, hi, the stops, the queue, the bucket sequences and the fold are then
    those of the list the kernels really walk (positions in the cell's list), ``list`` is the cell.
    Beside the counts: kept_ids / contrib_ids (entry ids), stop_ids {pixel: id of the entry that stops it}, batches_masks (64-entry
    batches taken per bucket with keep masks), foreign_gap (a batch none of whose entries has the tile in its box lies between two
    batches the half tile queues entries of) and stop_ends_batch (a stopping entry is the last of a batch of the list)."""
    W, H, tw, th = s["W"], s["H"], s["tw"], s["th"]
    T = tw * th
    offs = offs.reshape(-1).long()
    xy, cn, op = s["xys"].double(), s["conics"].double(), s["opacities"].double()
    amin, tmin = 1.0 / 255.0, 1e-4
    out = []
    if cells is None:
        walks = [(t, t, None) for t in range(T)]
    else:
        sx, sy = cells
        lw = (tw + (1 << sx) - 1) >> sx
        tb = edge_tile_boxes(s).long()
        bx0, by0, bw, bh = tb[:, 0] % tw, tb[:, 0] // tw, tb[:, 1] & 0xffff, tb[:, 1] >> 16
        walks = [(t, (t // tw >> sy) * lw + (t % tw >> sx), t) for t in range(T)]
    for t, l, boxed in walks:
        rs = int(offs[l])
        re = int(offs[l + 1]) if l + 1 < offs.numel() else fid.numel()
        if re <= rs:
            continue
        ids = fid[rs:re].long()
        L = re - rs
        if boxed is None:
            own = torch.ones(L, dtype=torch.bool)
        else:
            tx, ty = t % tw, t // tw
            own = (bx0[ids] <= tx) & (tx < bx0[ids] + bw[ids]) & (by0[ids] <= ty) & (ty < by0[ids] + bh[ids])
            if not bool(own.any()):
                continue                                                  # the tile's own list is empty: as without cells
        for h in (0, 1):
            px = (16 * (t % tw) + torch.arange(16, dtype=torch.float64) + 0.5).repeat(8)
            py = (16 * (t // tw) + 8 * h + torch.arange(8, dtype=torch.float64) + 0.5).repeat_interleave(16)
            inimg = (px < W) & (py < H)
            dx = px[None, :] - xy[ids, 0:1]
            dy = py[None, :] - xy[ids, 1:2]
            sig = 0.5 * (cn[ids, 0:1] * dx * dx + cn[ids, 2:3] * dy * dy) + cn[ids, 1:2] * dx * dy
            al = torch.clamp(op[ids, None] * torch.exp(-sig), max=0.999)
            assert not bool(((al > 0.7 * amin) & (al < 1.3 * amin)).any()), f"tile {t} half {h}: an alpha within 30 % of 1/255"
            valid = (sig >= 0) & (al >= amin) & own[:, None]
            kept = valid.any(1)
            vin = valid & inimg[None, :]
            lg = torch.where(vin, torch.log1p(-al), torch.zeros_like(al))
            t_after = torch.exp(torch.cumsum(lg, 0))
            hit = vin & (t_after <= tmin)
            stop = {}
            bin_final = torch.full((128,), -1, dtype=torch.long)
            for p in torch.nonzero(vin.any(0)).reshape(-1).tolist():
                hs = torch.nonzero(hit[:, p]).reshape(-1)
                st = int(hs[0]) if hs.numel() else L
                tv = t_after[:st + 1, p][vin[:st + 1, p]]
                assert not bool(((tv > tmin / 1.2) & (tv < tmin * 1.2)).any()), f"tile {t} half {h} pixel {p}: T within 20 % of 1e-4"
                blend = torch.nonzero(vin[:st, p]).reshape(-1)
                if st < L:
                    assert blend.numel(), f"tile {t} half {h} pixel {p} stops at its first entry"
                    stop[p] = st
                    bin_final[p] = rs + st - 1                   # the forward's last_ids: the entry before the one that stops it
                elif blend.numel():
                    bin_final[p] = min(rs + (int(blend[-1]) // 64) * 64 + 64, re) - 1    # else the end of its last batch with a blend
            hi = min(int(bin_final.max()), re - 1)
            q = kept & (torch.arange(L) <= hi - rs) if hi >= rs else torch.zeros(L, dtype=torch.bool)

            def buckets(masks):
                qn, takes, carries, pulled = 0, [], [], []
                if hi < rs:
                    return takes, carries, pulled
                batch, cursor = (hi - rs) >> 6, hi
                while True:
                    n_b = 0
                    while qn < 128 and (batch >= 0 if masks else cursor >= rs):
                        if masks:
                            qn += int(q[64 * batch:64 * batch + 64].sum())
                            batch -= 1
                        else:
                            qn += int(q[max(rs, cursor - 63) - rs:cursor - rs + 1].sum())
                            cursor -= 64
                        n_b += 1
                    take = min(qn, 128)
                    qn -= take
                    takes.append(take)
                    carries.append(qn)
                    pulled.append(n_b)
                    if take == 0:
                        return takes, carries, pulled
            tm, cm, bm = buckets(True)
            ts, cs, _bs = buckets(False)
            last = ([x for x in tm if x > 0] or [0])[-1]
            nb = (L + 63) // 64
            pad = torch.zeros(nb * 64 - L, dtype=torch.bool)
            own_b = torch.cat([own, pad]).reshape(nb, 64).any(1)
            q_b = torch.cat([q, pad]).reshape(nb, 64).any(1)
            with_q = torch.nonzero(q_b).reshape(-1)
            gap = bool(with_q.numel() >= 2 and (~own_b[int(with_q[0]):int(with_q[-1]) + 1]).any())
            out.append(dict(tile=t, half=h, rs=rs, re=re, L=L, kept=int(kept.sum()), contrib=int(vin.any(1).sum()), stop=stop,
                            hi=(hi - rs) if hi >= rs else -1, queue=int(q.sum()), takes_masks=tm, carries_masks=cm, takes_scan=ts,
                            carries_scan=cs, fold=4 if 0 < last <= 32 else 2 if 0 < last <= 64 else 1, n_stopped=len(stop),
                            n_blending=int((bin_final >= 0).sum()), kept_above_hi=int(kept[max(hi - rs + 1, 0):].sum()),
                            list=l, kept_ids=ids[kept].tolist(), contrib_ids=ids[vin.any(1)].tolist(),
                            stop_ids={p: int(ids[st]) for p, st in stop.items()}, batches_masks=bm, foreign_gap=gap,
                            stop_ends_batch=any(st % 64 == 63 for st in stop.values())))
    return out


def regime_line(r, what=""):
    """One printed line per half tile: the regime the kernels reach on it (edge_model)."""
    tm = r["takes_masks"][:-1]
    st = sorted(set(r["stop"].values()))
    return (f"[raster] {what}tile {r['tile']} {('top', 'bottom')[r['half']]}: list {r['L']} at range_start % 64 = {r['rs'] % 64}, "
            f"kept {r['kept']} (in the image {r['contrib']}), {r['n_stopped']} of {r['n_blending']} blending pixels stop"
            f"{' at ' + str(st[:4]) if st else ''}, hi {r['hi']}, queue {r['queue']} (+{r['kept_above_hi']} kept above hi), buckets "
            f"{tm if len(tm) <= 5 else tm[:2] + ['...'] + tm[-2:]}, fold {r['fold']}, carried max {max(r['carries_masks'] or [0])} "
            f"(masks) / {max(r['carries_scan'] or [0])} (scan)"
            + (f"; walks the list of cell {r['list']}: a bucket takes up to {max(r['batches_masks'] or [0])} batches, "
               f"{'an' if r['foreign_gap'] else 'no'} all-foreign batch inside the walk" if r.get("list", r["tile"]) != r["tile"] else ""))


HULL_KEYS = ("means2d", "absgrad", "conics", "colors", "opacities")


def assert_in_hull(grads, lo, hi, what, tol=REL_TOL, scales=None):
    """lo - tol * scale <= g <= hi + tol * scale at every entry of every tensor of HULL_KEYS; ``scales``: per-key scale (default: the
    largest |lo|, |hi| of that tensor).  Returns the worst violation in units of tol * scale."""
    worst = 0.0
    for k in HULL_KEYS:
        g = grads[k].detach().double().cpu().reshape(lo[k].shape)
        scale = float(scales[k]) if scales is not None else float(torch.maximum(lo[k].abs(), hi[k].abs()).max())
        if scale == 0.0:
            assert float(g.abs().max()) == 0.0, f"{what} {k}: non-zero gradient where every admissible evaluation gives zero"
            continue
        viol = torch.maximum(lo[k] - g, g - hi[k]).clamp_min(0)
        w = float(viol.max()) / (tol * scale)
        width = float((hi[k] - lo[k]).max()) / scale
        print(f"[parity] {what} {k}: worst distance from the hull of admissible decisions = {w:.3f} x (1e-4 x scale {scale:.3e}); "
              f"{int((hi[k] > lo[k]).sum())} entries with a non-degenerate interval, widest {width:.2e} of scale")
        log = os.environ.get("DNSPLAT_MARGIN_LOG")
        if log:
            with open(log, "a") as f:
                f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{what} {k} (hull)\t{w:.3f}\t{w:.3f}\n")
        worst = max(worst, w)
        assert w <= 1.0, f"{what} {k}: {int((viol > tol * scale).sum())} entries outside the hull by more than 1e-4 x scale, worst {w:.2f}"
    return worst


def oracle_threads():
    """Threads for the oracle's OpenMP loops: its gradient scatter uses omp atomics, and beyond ~32 threads it only gets slower
    (bench.py cpu_baseline).  os.cpu_count() counts the whole host; OMP_NUM_THREADS, where set, is what this process may use."""
    n = os.cpu_count() or 1
    env = os.environ.get("OMP_NUM_THREADS", "").strip()
    if env.isdigit() and int(env) > 0:
        n = min(n, int(env))
    torch.set_num_threads(min(32, n))


def assert_binning_properties(info, cam=0):
    """The tile lists of one camera of a product frame (``last_info`` of DNSplatterRenderer) without a reference list: status word 0,
    sum(tiles_bin) = n_isects, non-decreasing offsets, every list (depth, index)-sorted, every Gaussian exactly tiles_bin times and only
    in tiles of its gsplat box.  Holds for gsplat's boxes and for the tight ones (whose lists are sub-lists of gsplat's)."""
    from dn_splatter_amd import _ops

    dev = info["flatten_ids"].device
    assert _ops.binning_status(info["_binning"], info["radii"].numel()) == 0, "a look-back wait of the tile sort timed out"
    n = info["n_isects"]
    tiles = info["tiles_bin"][cam].long()          # the count the binning walked (== tiles_per_gauss unless tight tile boxes)
    assert int(tiles.sum()) == n, "sum(tiles_bin) != n_isects"
    if info.get("tight_tiles"):     # a visible Gaussian may reach alpha >= 1/255 at no pixel centre at all
        assert int(((tiles > 0) & ~(info["radii"][cam] > 0)).sum()) == 0
    else:
        assert int(((info["radii"][cam] > 0) != (tiles > 0)).sum()) == 0
    offs = info["isect_offsets"].reshape(-1).long()
    assert int(offs[0]) == 0 and bool((offs[1:] >= offs[:-1]).all()) and int(offs[-1]) <= n
    # every tile list is depth-sorted, ties broken by Gaussian index (stable sort, Appendix A.3)
    fid = info["flatten_ids"].long()
    d = info["depths"][cam][fid]
    tile_of = torch.searchsorted(offs, torch.arange(n, device=dev), right=True) - 1
    same = tile_of[1:] == tile_of[:-1]
    ok = (d[1:] > d[:-1]) | ((d[1:] == d[:-1]) & (fid[1:] > fid[:-1]))
    assert bool((ok | ~same).all()), "a tile list is not (depth, index)-sorted"
    # each Gaussian appears exactly tiles_bin times
    cnt = torch.bincount(fid, minlength=tiles.shape[0])
    assert torch.equal(cnt, tiles)
    # and only in tiles of its bounding box (A.3)
    xy = info["means2d"][cam][fid]
    r = info["radii"][cam][fid].float()
    tw = info["tile_width"]
    tx, ty = (tile_of % tw).float(), (tile_of // tw).float()
    inside = (tx >= torch.floor((xy[:, 0] - r) / 16)) & (tx < torch.ceil((xy[:, 0] + r) / 16)) & \
             (ty >= torch.floor((xy[:, 1] - r) / 16)) & (ty < torch.ceil((xy[:, 1] + r) / 16))
    assert bool(inside.all())
