"""The AGS-Mesh normal-loss kernel (ags.hip behind dnsplat_ags_normal_loss) against the PyTorch restatements of torch_losses evaluated
in float64 (pinned to the reference's own code by test_ags_reference.py), with the helpers and constants of _scenes.py and
test_gpu_losses.py: loss values within 1e-5 of fp64 plus the fp32 restatement's own distance from it, gradients within 2e-4 of the
tensor's scale plus that envelope, and the per-pixel statistic.  No entry is left out of a comparison.

The kernel takes two kinds of DECISIONS per frame (an element lies on the dilated edge map; a pixel's surface normal is within 0.1 rad
of the ground truth), and a decision that exact arithmetic puts within a few fp32 roundings of its threshold may fall either way
(_ags_inputs.py: the flagged decisions).  So: the kernel's selection must equal the float64 restatement's everywhere but at flagged
decisions (a dilated element: where one of its nine sources is flagged); at most 0.1 % of a frame's decisions may be flagged, none on
the fixture's frames — a condition on the inputs, which the recipe of _ags_inputs.py meets; and value and gradients are compared with
the float64 restatement evaluated UNDER THE KERNEL'S OWN SELECTION, so that a flagged flip cannot hide an arithmetic error.

Shapes are the smallest at which each mechanism can go wrong: fewer pixels than a wave; one row, one column, one pixel; the tile's
width and height and one either side; more workgroups than the fold kernel takes in one trip; plane boundaries on a tile's last and
first column and row (the Laplacian's and the dilation's halo); negative components on the frame's border.
"""
import functools
import os

import numpy as np
import pytest
import torch

import _ags_inputs as inputs
from _scenes import FP32_ENVELOPE, PIX_MAX, PIX_P99, assert_close, check_pixels, fp64_envelope, row_rel_stats

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAD_TOL = 2e-4          # test_gpu_losses.GRAD_TOL
VALUE_TOL = 1e-5         # test_gpu_losses.VALUE_TOL
TILE_W, TILE_H = 64, 16  # ags.hip AG_TW x AG_TH: one workgroup per tile, a two-pixel halo of reciprocals around it
FOLD = 256               # ags.hip AG_THREADS: partials (= workgroups) dns_fold_partials takes per trip in the fold kernel
EDGES, CONFIDENCE = 8000, 20000          # a step of each mode with the weight on (7000 < step < 15000 <= step)
LAMBDA, MASK_STEPS = 0.1, 15000


# ---- the two sides ---------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=32)
def _inputs(H, W, col_cut=None, row_cut=None, seed=0, sphere=True):
    """surf, gt, pred float32 [3,H,W] on the host (the recipe of _ags_inputs.py)."""
    _, surf, gt, pred = inputs.normal_inputs(H, W, seed=seed, col_cut=col_cut, row_cut=row_cut, sphere=sphere)
    return surf, gt, pred


def _hip(surf, gt, pred, step, layout="chw", lam=LAMBDA):
    """value, selection, d / d surf, d / d pred of fused_loss.ags_normal_loss on the device (tensors are uploaded)."""
    from dn_splatter_amd import fused_loss as fl

    s, p = surf.detach().to(DEV).clone().requires_grad_(True), pred.detach().to(DEV).clone().requires_grad_(True)
    v, sel = fl.ags_normal_loss(s, gt.to(DEV), p, step, lam, MASK_STEPS, layout=layout, return_selection=True)
    v.backward()
    assert v.dtype == torch.float32 and sel.dtype == torch.bool and s.grad.shape == s.shape and p.grad.shape == p.shape
    return v.detach(), sel, s.grad, p.grad


def _restated(surf, gt, pred, step, dtype, selection, lam=LAMBDA):
    """torch_losses.ags_normal_loss on the host in ``dtype`` under a GIVEN selection: value and the two gradients."""
    from dn_splatter_amd import torch_losses as tl

    s, p = surf.detach().to(dtype).clone().requires_grad_(True), pred.detach().to(dtype).clone().requires_grad_(True)
    v = tl.ags_normal_loss(s, gt.to(dtype), p, step, lam, MASK_STEPS, selection=selection)
    v.backward()
    return v.detach(), s.grad, p.grad


def _check_selection(sel, surf, gt, step, what, cap=inputs.FLAG_CAP):
    """The kernel's selection == the float64 restatement's except where a flagged decision reaches; the flagged share <= cap."""
    from dn_splatter_amd import torch_losses as tl

    sel = sel.cpu()
    if step < MASK_STEPS:
        want = ~tl.ags_find_edges(gt.double())
        flagged = inputs.flagged_edge_decisions(gt)
        may_differ = inputs.dilate(flagged)
    else:
        want = tl.ags_normal_confidence(surf.double(), gt.double())
        flagged = inputs.flagged_confidence_decisions(surf, gt)
        may_differ = flagged
    assert sel.shape == want.shape, what
    n_flag, n = int(flagged.sum()), flagged.numel()
    differ = sel != want
    print(f"[ags] {what}: {int(want.sum())} of {n} selected, {n_flag} decisions flagged, {int(differ.sum())} differ from fp64")
    assert n_flag <= cap * n, f"{what}: {n_flag} of {n} decisions are within the rounding envelope (the inputs break the test's condition)"
    assert not bool((differ & ~may_differ).any()), f"{what}: {int((differ & ~may_differ).sum())} selections differ from fp64 away from any flagged decision"
    return want


def _check_value(v, v64, v32, what):
    """test_gpu_losses._check_value: within VALUE_TOL of fp64 plus the fp32 restatement's own envelope."""
    v, v64, v32 = float(v), float(v64), float(v32)
    env = FP32_ENVELOPE * abs(v32 - v64)
    print(f"[ags] {what}: value {v:.9g} vs fp64 {v64:.9g}: error {abs(v - v64):.2e} (fp32 envelope {env:.2e})")
    assert abs(v - v64) <= VALUE_TOL * abs(v64) + env, f"{what}: value {v!r} vs fp64 {v64!r}"


def _check_grad(hip, g64, g32, what):
    """test_gpu_losses._check_grad, per pixel: the channels last."""
    hip, g64, g32 = (t.detach().cpu().permute(1, 2, 0) for t in (hip, g64, g32))
    assert_close(hip, g64, what, GRAD_TOL, envelope=fp64_envelope(g32, g64))
    st = row_rel_stats(g32, g64)
    p99, rmax = (PIX_P99, PIX_MAX) if st is None else (max(PIX_P99, 2 * FP32_ENVELOPE * st[1]), max(PIX_MAX, 2 * FP32_ENVELOPE * st[2]))
    check_pixels(hip, g64, what + " per pixel", enforce=True, p99=p99, rmax=rmax)


def _check(surf, gt, pred, step, what, cap=inputs.FLAG_CAP):
    """Selection against fp64 (flagged rule), then value and both gradients against fp64 under the kernel's own selection."""
    v, sel, gs, gp = _hip(surf, gt, pred, step)
    _check_selection(sel, surf, gt, step, what, cap)
    sel = sel.cpu()
    v64, gs64, gp64 = _restated(surf, gt, pred, step, torch.float64, sel)
    v32, gs32, gp32 = _restated(surf, gt, pred, step, torch.float32, sel)
    _check_value(v, v64, v32, what)
    _check_grad(gs, gs64, gs32, "d " + what + " / d surf")
    _check_grad(gp, gp64, gp32, "d " + what + " / d pred")
    # outside the selection the surface normal gets exactly nothing
    keep = sel if sel.dim() == 3 else sel[None].expand(3, -1, -1)
    assert float(gs.cpu()[~keep].abs().sum()) == 0.0
    return v, sel, gs, gp


# ---- shapes ----------------------------------------------------------------------------------------------------------------------

SHAPES = [(5, 7),                                   # smaller than one tile, fewer pixels than a wave
          (1, 150), (150, 1), (1, 1),               # one row (three tiles wide), one column (ten tiles high), one pixel
          (TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1),
          (TILE_H * 15 + 1, TILE_W * 16 + 1)]       # 17 x 16 = 272 tiles: a second trip of the fold kernel
assert (SHAPES[-1][0] + TILE_H - 1) // TILE_H * ((SHAPES[-1][1] + TILE_W - 1) // TILE_W) > FOLD
SEEDS = {(1, 1): 1}                                 # the noise at which the only pixel is confident (seed 0: the mean of nothing)


@pytest.mark.parametrize("step", [EDGES, CONFIDENCE])
@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_match_fp64(dns, H, W, step):
    """A frame of a few pixels cannot keep a SHARE of its decisions flagged: there none is (0.1 % of them is less than one)."""
    surf, gt, pred = _inputs(H, W, seed=SEEDS.get((H, W), 0))
    _, sel, _, _ = _check(surf, gt, pred, step, f"{H}x{W} step {step}")
    assert bool(sel.any()) and (H * W < 64 or not bool(sel.all()))          # the filter selects, and on a frame of any size rejects


@pytest.mark.parametrize("cut", [-1, 0, 1])
def test_plane_boundaries_on_tile_edges_match_fp64(dns, cut):
    """The boundary between two planes runs between a tile's last column and the next tile's first (and one column either side),
    likewise for rows: an edge bit of one tile is set by reciprocals of the other (the Laplacian's halo) and dilates back across
    (the second halo pixel).  The frame's border carries negative components on three sides: every such element is an edge."""
    H, W = 3 * TILE_H + 5, 2 * TILE_W + 9
    surf, gt, pred = _inputs(H, W, TILE_W + cut, TILE_H + cut)
    _, sel, _, _ = _check(surf, gt, pred, EDGES, f"planes cut at column {TILE_W + cut}, row {TILE_H + cut}")
    want = ~inputs.dilate(_raw_edges_fp64(gt))
    assert torch.equal(sel.cpu(), want)
    # both sides of the column boundary are edges in every channel (the planes differ in every component); the plane beside it is not
    c = TILE_W + cut
    assert not bool(sel[:, 2:10, c - 1:c + 1].any()) and bool(sel[:, 2:10, c - 8].all())
    border = torch.zeros(3, H, W, dtype=torch.bool)
    border[:, 0], border[:, -1], border[:, :, 0], border[:, :, -1] = True, True, True, True
    neg = border & (gt < 0)
    assert bool(neg.any()) and not bool(sel.cpu()[neg].any())
    _check(surf, gt, pred, CONFIDENCE, f"planes cut at {cut}, confidence")


def _raw_edges_fp64(gt):
    r = 1.0 / (gt.double() + 1e-6)
    p = torch.nn.functional.pad(r, (1, 1, 1, 1))
    return p[:, :-2, 1:-1] + p[:, 2:, 1:-1] + p[:, 1:-1, :-2] + p[:, 1:-1, 2:] - 4 * r > 0.01


# ---- the fixture's frames: the reference's stored outputs -----------------------------------------------------------------------


@functools.lru_cache(maxsize=1)
def _fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_ags.npz"))


@pytest.mark.parametrize("step", inputs.FIXTURE_STEPS)
@pytest.mark.parametrize("H,W", inputs.FIXTURE_FRAMES)
def test_fixture_frames_equal_the_reference(dns, H, W, step):
    """Steps 100, 7000 (weight 0: zeros), 7001, 14999 (edge map) and 15000 (confidence): the kernel's selection is the reference's mask
    exactly — no decision of these frames is flagged — and value and gradients are the reference's stored ones."""
    g = _fixture()
    f = inputs.fixture_frame(g, H, W)
    value, v_surf, v_pred = inputs.fixture_result(g, H, W, step)
    v, sel, gs, gp = _check(f["surf"], f["gt"], f["pred"], step, f"fixture {H}x{W} step {step}", cap=0.0)
    assert torch.equal(sel.cpu(), ~f["edges"] if step < MASK_STEPS else f["confident"])
    assert abs(float(v) - value) <= VALUE_TOL * abs(value), (float(v), value)
    assert_close(gs.cpu(), v_surf, "d / d surf against the reference", GRAD_TOL)
    assert_close(gp.cpu(), v_pred, "d / d pred against the reference", GRAD_TOL)
    if step <= 7000:
        assert float(v) == 0.0 and float(gs.abs().max()) == 0.0 and float(gp.abs().max()) == 0.0


# ---- degenerate selections -------------------------------------------------------------------------------------------------------

DH, DW = TILE_H + 7, TILE_W + 11


def _noise(shape, scale, seed):
    return (torch.round(scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * inputs.GRID) / inputs.GRID).float()


def test_constant_positive_normals_select_everything(dns):
    """No edge anywhere (on the border the missing neighbours make the Laplacian negative): count = 3 H W."""
    gt = inputs.to_chw(torch.tensor([166, 191, 230], dtype=torch.uint8).expand(DH, DW, 3).float() / 255.0).contiguous()
    assert bool((gt > 0).all())
    surf, pred = gt + _noise(gt.shape, 0.05, 1), gt + _noise(gt.shape, 0.2, 2)
    _, sel, _, _ = _check(surf, gt, pred, EDGES, "constant positive normals")
    assert bool(sel.all())


def test_every_element_an_edge_is_nan_as_autograd(dns):
    """A checkerboard of +-0.5 in every channel: each negative element's Laplacian is positive and its dilation covers the frame.
    Nothing is selected: the value is nan (the mean of nothing), the surface normal's gradient is zero and the predicted normal's is
    finite — the nan sets of fp64 autograd, whatever they are."""
    yy, xx = torch.meshgrid(torch.arange(DH), torch.arange(DW), indexing="ij")
    gt = (((yy + xx) % 2).float() - 0.5).expand(3, DH, DW).contiguous()
    surf, pred = gt + _noise(gt.shape, 0.05, 3), gt + _noise(gt.shape, 0.2, 4)
    v, sel, gs, gp = _hip(surf, gt, pred, EDGES)
    _check_selection(sel, surf, gt, EDGES, "checkerboard")
    assert not bool(sel.any())
    v64, gs64, gp64 = _restated(surf, gt, pred, EDGES, torch.float64, sel.cpu())
    assert torch.isnan(v64) and torch.isnan(v)
    assert torch.equal(torch.isnan(gs.cpu()), torch.isnan(gs64)) and torch.equal(torch.isnan(gp.cpu()), torch.isnan(gp64))
    assert float(gs.abs().max()) == 0.0 and float(gs64.abs().max()) == 0.0
    _check_grad(gp, gp64, _restated(surf, gt, pred, EDGES, torch.float32, sel.cpu())[2], "d checkerboard / d pred")
    # weight 0 keeps the nan (0 x nan)
    assert torch.isnan(_hip(surf, gt, pred, 100)[0])


@pytest.mark.parametrize("confident", [True, False])
def test_all_or_no_pixel_confident(dns, confident):
    """surf = gt (dot = |gt|^2 >= cos 0.1: every pixel, count = 3 H W) and surf = -gt (none: nan, gradients as autograd's)."""
    gt = inputs.to_chw(torch.tensor([128, 128, 255], dtype=torch.uint8).expand(DH, DW, 3).float() / 255.0).contiguous()
    surf = gt.clone() if confident else -gt
    pred = gt + _noise(gt.shape, 0.2, 5)
    if confident:
        _, sel, _, _ = _check(surf, gt, pred, CONFIDENCE, "all confident")
        assert bool(sel.all()) and sel.shape == (DH, DW)
        return
    v, sel, gs, gp = _hip(surf, gt, pred, CONFIDENCE)
    _check_selection(sel, surf, gt, CONFIDENCE, "none confident")
    v64, gs64, gp64 = _restated(surf, gt, pred, CONFIDENCE, torch.float64, sel.cpu())
    assert not bool(sel.any()) and torch.isnan(v) and torch.isnan(v64)
    assert torch.equal(torch.isnan(gs.cpu()), torch.isnan(gs64)) and float(gs.abs().max()) == 0.0
    _check_grad(gp, gp64, _restated(surf, gt, pred, CONFIDENCE, torch.float32, sel.cpu())[2], "d none confident / d pred")


def test_infinite_reciprocals_follow_ieee(dns):
    """Components of exactly -1e-6 (float32): n + 1e-6 = 0, r = inf.  Alone (on a tile's corner, and in the frame's corner) it makes
    its four neighbours edges and is none itself (-inf); two of them side by side give inf - inf = nan > 0.01 = false.  The masks are
    those of the float32 restatement bit for bit; value and gradients are finite and match fp64 under that selection."""
    from dn_splatter_amd import torch_losses as tl

    H, W = 2 * TILE_H + 3, 2 * TILE_W + 3
    surf, gt, pred = (t.clone() for t in _inputs(H, W, sphere=False))
    tiny = float(torch.tensor(-1e-6, dtype=torch.float32))
    gt[0, TILE_H - 1, TILE_W - 1] = tiny                   # a tile's last pixel: its neighbours lie in three other tiles
    gt[1, 0, 0] = tiny                                     # the frame's corner
    gt[2, TILE_H + 5, 20] = gt[2, TILE_H + 5, 21] = tiny   # a pair
    gt[0, 5, TILE_W] = gt[0, 6, TILE_W] = tiny             # a vertical pair on a tile's first column
    assert float(gt[0, TILE_H - 1, TILE_W - 1] + torch.tensor(1e-6)) == 0.0
    want = ~tl.ags_find_edges(gt)                          # float32, on the host
    r = 1.0 / (gt + 1e-6)
    assert int(torch.isinf(r).sum()) == 6
    v, sel, gs, gp = _hip(surf, gt, pred, EDGES)
    assert torch.equal(sel.cpu(), want), f"{int((sel.cpu() != want).sum())} selections differ from the float32 restatement"
    # what IEEE arithmetic says about the lone one: the element itself is no edge but lies under its neighbours' dilation
    assert not bool(want[0, TILE_H - 2:TILE_H + 1, TILE_W - 2:TILE_W + 1].any())
    v64, gs64, gp64 = _restated(surf, gt, pred, EDGES, torch.float64, want)
    v32, gs32, gp32 = _restated(surf, gt, pred, EDGES, torch.float32, want)
    assert bool(torch.isfinite(v)) and bool(torch.isfinite(gs).all())
    _check_value(v, v64, v32, "infinite reciprocals")
    _check_grad(gs, gs64, gs32, "d infinite reciprocals / d surf")
    _check_grad(gp, gp64, gp32, "d infinite reciprocals / d pred")


# ---- layouts, weights, reproducibility -------------------------------------------------------------------------------------------


def _images(H, W):
    """The [H,W,3] images in [0, 1] a model holds, exact in float32: the 8-bit normal map / 255 and (x + 1) / 2 of the grid values."""
    gt_u8, surf, _, pred = inputs.normal_inputs(H, W)
    back = lambda chw: ((chw.permute(1, 2, 0) + 1) / 2).contiguous()      # noqa: E731
    assert torch.equal(back(surf) * 2 - 1, surf.permute(1, 2, 0))
    return back(surf), gt_u8.float() / 255.0, back(pred)


@pytest.mark.parametrize("step", [EDGES, CONFIDENCE])
def test_both_layouts_give_the_same_bits(dns, step):
    """The [H,W,3] images in [0, 1] against (2 x - 1).permute(2, 0, 1) formed by torch: same value bits, same selection, and the
    gradients w.r.t. the images are 2 x those w.r.t. the [3,H,W] tensors (d (2 x - 1) / d x, exact)."""
    H, W = TILE_H * 2 + 3, TILE_W + 9
    s01, g01, p01 = (t.to(DEV) for t in _images(H, W))
    chw = [inputs.to_chw(t).contiguous() for t in (s01, g01, p01)]
    v_a, sel_a, gs_a, gp_a = _hip(chw[0], chw[1], chw[2], step)
    v_b, sel_b, gs_b, gp_b = _hip(s01, g01, p01, step, layout="hwc")
    assert torch.equal(v_a, v_b) and torch.equal(sel_a, sel_b) and float(v_a) > 0
    assert torch.equal(gs_b, 2 * gs_a.permute(1, 2, 0)) and torch.equal(gp_b, 2 * gp_a.permute(1, 2, 0))
    assert float(gs_a.abs().max()) > 0 and float(gp_a.abs().max()) > 0


def test_weight_and_step_thresholds(dns):
    """step <= 7000: zeros.  7001 and 14999: the edge map, the same bits.  15000: the confidence filter.  The weight is linear."""
    H, W = 33, 130
    surf, gt, pred = _inputs(H, W, seed=1)
    for step in (0, 100, 7000):
        v, sel, gs, gp = _hip(surf, gt, pred, step)
        assert float(v) == 0.0 and float(gs.abs().max()) == 0.0 and float(gp.abs().max()) == 0.0 and sel.shape == (3, H, W)
    a, b, c = _hip(surf, gt, pred, 7001), _hip(surf, gt, pred, 14999), _hip(surf, gt, pred, 15000)
    assert float(a[0]) > 0 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert c[1].shape == (H, W) and float(c[0]) != float(a[0])
    d = _hip(surf, gt, pred, 7001, lam=0.2)                # 2 x the weight: 2 x everything, exactly (a power of two)
    assert torch.equal(d[0], 2 * a[0]) and torch.equal(d[2], 2 * a[2]) and torch.equal(d[3], 2 * a[3])


@pytest.mark.parametrize("step", [EDGES, CONFIDENCE])
def test_two_calls_give_the_same_bits(dns, step):
    H, W = SHAPES[-1]
    surf, gt, pred = _inputs(H, W)
    a, b = _hip(surf, gt, pred, step), _hip(surf, gt, pred, step)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- the model's branch: capture, install ----------------------------------------------------------------------------------------


def _model_case(dtype=torch.float32, device=DEV):
    g = _fixture()
    t = lambda k: torch.from_numpy(g[k]).to(device)       # noqa: E731
    leaf = lambda k: t(k).to(dtype).requires_grad_(True)      # noqa: E731
    out = {"rgb": leaf("m_pred_rgb"), "depth": leaf("m_pred_depth"), "normal": leaf("m_pred_normal"), "surface_normal": leaf("m_surface_normal")}
    batch = {"image": t("m_image").to(dtype), "mono_depth": t("m_gt_depth").to(dtype), "normal": (t("m_gt_normal_u8").float() / 255.0).to(dtype),
             "confidence": t("m_confidence").to(dtype), "mask": t("m_mask").to(dtype)}
    return g, out, batch, leaf("m_scales")


def test_ags_mesh_loss_fused_equals_the_reference_branch(dns):
    """ags_mesh_loss_fused less its rgb term == get_loss_dict's "ags-mesh" branch less the recorded rgb term (a confidence image and a
    mask in the batch), value and the gradients w.r.t. depth, both normals and the scales — the bounds of
    test_reference_golden.test_hip_fused_loss_equals_the_reference_combination; and against the float64 restatement."""
    from dn_splatter_amd import fused_loss as fl, torch_losses as tl

    g, out, batch, sc = _model_case()
    step = int(g["m_step"])
    loss = fl.ags_mesh_loss_fused(out, batch, sc, step)
    with torch.no_grad():
        rgb_only = fl._DnLossFn.apply(out["rgb"], out["depth"], out["normal"], batch["image"], None, None, None, 0.2, 0.2, 0.1)
    reg = float(loss.detach()) - float(rgb_only)
    want = float(g["m_main"]) - float(g["m_rgb_term"])
    assert abs(reg - want) < 2e-5, (reg, want)
    grads = torch.autograd.grad(loss, [out["depth"], out["normal"], out["surface_normal"], sc, out["rgb"]])
    for got, key in zip(grads, ("m_v_depth", "m_v_normal", "m_v_surface_normal", "m_v_scales")):
        ref = torch.from_numpy(g[key])
        assert float((got.cpu() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max())), key
    assert float(grads[4].abs().max()) > 0                                        # the rgb term is part of the sum
    _, o64, b64, s64 = _model_case(torch.float64, "cpu")
    v64 = tl.ags_regularization_term(o64, b64, s64, step)
    _check_value(reg, v64.detach(), want, "ags_mesh_loss_fused less its rgb term")
    g64 = torch.autograd.grad(v64, [o64["depth"], o64["normal"], o64["surface_normal"], s64])
    for got, ref, what in zip(grads, g64, ("depth", "normal", "surface_normal", "scales")):
        assert_close(got, ref, "d ags_mesh_loss_fused / d " + what, GRAD_TOL)


def test_forward_and_backward_are_captured_and_replayed(dns):
    """ags_mesh_loss_fused + backward under torch.cuda.graph (graph.GraphedStep): the replay leaves the eager call's bits.  Nothing on
    the path reads the selected count on the host — under torch's synchronisation check the fused call passes and the restatement,
    whose two boolean-mask gathers are what the reference's method does, is refused."""
    from dn_splatter_amd import fused_loss as fl, torch_losses as tl
    from dn_splatter_amd.graph import GraphedStep

    g, out, batch, sc = _model_case()
    step = int(g["m_step"])
    leaves = dict(out, scales=sc)

    def compute():
        loss = fl.ags_mesh_loss_fused(out, batch, sc, step)
        loss.backward()
        return loss

    def eager():
        """The eager frame's bits, and no reference to its autograd graph: the AccumulateGrad nodes of the leaves belong to the stream
        they were made on, and a node of the default stream that the eager loss kept alive would pull that stream into the capture."""
        for p in leaves.values():
            p.grad = None
        return [compute().detach().clone()] + [p.grad.clone() for p in leaves.values()]

    want = eager()
    graphed = GraphedStep(compute, params=leaves)
    for p in leaves.values():
        p.grad.zero_()
    res = graphed()
    torch.cuda.synchronize()
    got = [res.detach()] + [p.grad for p in leaves.values()]
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and float(want[4].abs().max()) > 0
    del res, got
    graphed.close()

    chw = [inputs.to_chw(t.detach()).contiguous() for t in (out["surface_normal"], batch["normal"], out["normal"])]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for p in leaves.values():
            p.grad = None
        compute()
        fl.ags_normal_loss(chw[0], chw[1], chw[2], CONFIDENCE)
        with pytest.raises(RuntimeError):
            tl.ags_normal_loss(chw[0], chw[1], chw[2], step)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_installed_strategy_equals_the_reference(dns):
    """install_losses on a stand-in AGSMeshRegularization: get_normal_loss on the fixture's inputs returns the stored value and
    gradients at every stored step; normal_lambda and normal_mask_steps are read from the strategy at call time."""
    st = type("AGSMeshRegularization", (torch.nn.Module,), {"get_scale_loss": lambda self, scales: None,
                                                            "get_normal_loss": lambda self, *a: None})()
    st.normal_lambda, st.normal_mask_steps = LAMBDA, MASK_STEPS
    model = torch.nn.Module()
    model.regularization_strategy = st
    assert "regularization_strategy.get_normal_loss" in dns.install_losses(model)
    g = _fixture()
    H, W = inputs.FIXTURE_FRAMES[0]
    f = inputs.fixture_frame(g, H, W)
    for step in inputs.FIXTURE_STEPS:
        value, v_surf, v_pred = inputs.fixture_result(g, H, W, step)
        s, p = f["surf"].to(DEV).requires_grad_(True), f["pred"].to(DEV).requires_grad_(True)
        v = st.get_normal_loss(step, s, f["gt"].to(DEV), p)
        v.backward()
        assert abs(float(v) - value) <= VALUE_TOL * abs(value), (step, float(v), value)
        assert_close(s.grad.cpu(), v_surf, f"installed get_normal_loss, step {step}: d / d surf", GRAD_TOL)
        assert_close(p.grad.cpu(), v_pred, f"installed get_normal_loss, step {step}: d / d pred", GRAD_TOL)
    # the attributes are read when the method is called
    st.normal_lambda, st.normal_mask_steps = 2 * LAMBDA, 7001
    v2 = st.get_normal_loss(7001, f["surf"].to(DEV), f["gt"].to(DEV), f["pred"].to(DEV))
    assert abs(float(v2) - 2 * float(g[f"f{H}x{W}_s15000_value"])) <= 2 * VALUE_TOL * float(g[f"f{H}x{W}_s15000_value"])
