"""The Pearson depth kernels (pearson.hip behind dnsplat_pearson_depth) against the PyTorch restatements of torch_losses evaluated in
float64 (pinned to the reference's own classes by test_pearson_reference.py), value and gradient, with the helpers and constants of
test_gpu_losses.py: values within 1e-5 on the unit scale of a correlation, gradients within 2e-4 of the tensor's scale plus the fp32
restatement's own distance from fp64 as the envelope, and the per-pixel statistic.  No entry is left out of a comparison.

Shapes are the smallest at which each mechanism can go wrong: fewer pixels than a wave; the trip edges of the grid-stride loops (the
gradient kernel's 4096 x 256 = 1024 x 1024 pixels, the frame sweeps' 512 x 256); the register-resident box path up to 128 and the
re-reading path from 129; the region table's LDS piece of 128 entries; boxes at the frame's corners, repeated, overlapping;
a low-contrast frame (what tells centred moments from raw ones); a constant block; masks of two pixels and of one.
"""
import functools
import os

import numpy as np
import pytest
import torch

from _scenes import FP32_ENVELOPE, PIX_MAX, PIX_P99, assert_close, check_pixels, fp64_envelope, row_rel_stats

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAD_TOL = 2e-4          # test_gpu_losses.GRAD_TOL
VALUE_TOL = 1e-5         # test_gpu_losses.VALUE_TOL, on the unit scale of a correlation
PIECE = 128              # pearson.hip PS_PIECE: region-table entries staged in LDS at a time
REG_BOX = 128            # the largest box that stays in registers (PS_REG_PIXELS x 256 lanes = 128 x 128)


# ---- inputs and the two sides ----------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=16)
def _frame(W, H, seed=0, low_contrast=False):
    """pred, gt [H,W,1] float32 on the device: a correlated pair plus noise (co around 0.6), or the cancellation case
    pred = 5 + 0.01 u, gt = 3 + 0.01 u'."""
    g = torch.Generator().manual_seed(seed + 13 * W + H)
    if low_contrast:
        pred = 5 + 0.01 * torch.rand(H, W, 1, generator=g)
        gt = 3 + 0.01 * (0.5 * (pred - 5) / 0.01 + 0.5 * torch.rand(H, W, 1, generator=g))
    else:
        pred = torch.rand(H, W, 1, generator=g) * 4 + 1
        gt = 0.6 * pred + 1.5 * torch.rand(H, W, 1, generator=g) + 0.3
    return pred.to(DEV), gt.to(DEV)


def _origins(rows, cols):
    return torch.tensor(rows, dtype=torch.int64, device=DEV), torch.tensor(cols, dtype=torch.int64, device=DEV)


def _random_origins(n, W, H, box, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, H - box + 1, (n,), generator=g).to(DEV), torch.randint(0, W - box + 1, (n,), generator=g).to(DEV))


def _restated(pred, gt, dtype, whole, mask, rows, cols, box, w_whole=1.0, w_box=1.0):
    from dn_splatter_amd import torch_losses as tl

    x = pred.detach().to(dtype).clone().requires_grad_(True)
    t = gt.to(dtype)
    v = 0.0
    if whole:
        v = v + w_whole * tl.pearson_depth(x, t, mask)
    if rows is not None:
        v = v + w_box * tl.local_pearson_depth(x, t, rows, cols, box)
    v.backward()
    return v.detach(), x.grad


def _hip(pred, gt, whole, mask, rows, cols, box, w_whole=1.0, w_box=1.0):
    from dn_splatter_amd import fused_loss as fl

    x = pred.clone().requires_grad_(True)
    if whole and rows is not None:
        v = fl.pearson_depth_combined(x, gt, rows, cols, box, w_whole, w_box, mask)
    elif whole:
        v = w_whole * fl.pearson_depth(x, gt, mask)
    else:
        v = w_box * fl.local_pearson_depth(x, gt, rows, cols, box)
    v.backward()
    return v.detach(), x.grad


def _check_value(v, v64, what):
    v, v64 = float(v), float(v64)
    print(f"[pearson] {what}: value {v:.9g} vs fp64 {v64:.9g}: error {abs(v - v64):.2e}")
    assert abs(v - v64) <= VALUE_TOL * max(1.0, abs(v64)), f"{what}: value {v!r} vs fp64 {v64!r}"


def _check_grad(hip, g64, g32, what):
    """test_gpu_losses._check_grad."""
    assert_close(hip, g64, what, GRAD_TOL, envelope=fp64_envelope(g32, g64))
    st = row_rel_stats(g32, g64)
    p99, rmax = (PIX_P99, PIX_MAX) if st is None else (max(PIX_P99, 2 * FP32_ENVELOPE * st[1]), max(PIX_MAX, 2 * FP32_ENVELOPE * st[2]))
    check_pixels(hip, g64, what + " per pixel", enforce=True, p99=p99, rmax=rmax)


def _check(pred, gt, what, whole=True, mask=None, rows=None, cols=None, box=0, **w):
    v64, g64 = _restated(pred, gt, torch.float64, whole, mask, rows, cols, box, **w)
    _, g32 = _restated(pred, gt, torch.float32, whole, mask, rows, cols, box, **w)
    v, g = _hip(pred, gt, whole, mask, rows, cols, box, **w)
    assert g.shape == pred.shape and g.dtype == torch.float32
    _check_value(v, v64, what)
    _check_grad(g, g64, g32, "d " + what + " / d pred")
    return v, g


# ---- the whole frame -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("W,H", [(2, 2), (3, 1), (512, 256), (513, 256), (1024, 1024), (1025, 1024), (1600, 1200)])
def test_whole_frame_matches_fp64(dns, W, H):
    pred, gt = _frame(W, H)
    _check(pred, gt, f"pearson {W}x{H}")


def test_whole_frame_low_contrast_matches_fp64(dns):
    """pred = 5 + 0.01 u over 1600 x 1200: one-pass raw fp32 moments are 8 % off in the variance here."""
    pred, gt = _frame(1600, 1200, low_contrast=True)
    _check(pred, gt, "pearson 1600x1200 low contrast")


def test_masked_whole_frame_matches_fp64(dns):
    """The mask form == the reference's call on gathered pixels: a random mask, and one that keeps exactly two pixels."""
    W, H = 300, 280
    pred, gt = _frame(W, H)
    m = (torch.rand(H, W, 1, generator=torch.Generator().manual_seed(2)) > 0.3).to(DEV)
    _, g = _check(pred, gt, "pearson masked", mask=m)
    assert float(g[~m].abs().max()) == 0.0
    two = torch.zeros(H, W, 1, dtype=torch.bool, device=DEV)
    two[7, 11] = two[250, 299] = True
    _, g = _check(pred, gt, "pearson, a mask of two pixels", mask=two)
    assert int((g != 0).sum()) <= 2 and float(g[~two].abs().max()) == 0.0


def test_mask_of_one_pixel_is_nan(dns):
    """std of one element: nan in the value and at that pixel, zero elsewhere — as the reference on pred[mask]."""
    pred, gt = _frame(64, 48)
    one = torch.zeros(48, 64, 1, dtype=torch.bool, device=DEV)
    one[5, 9] = True
    v64, g64 = _restated(pred, gt, torch.float64, True, one, None, None, 0)
    v, g = _hip(pred, gt, True, one, None, None, 0)
    assert torch.isnan(v64) and torch.isnan(v)
    assert torch.equal(torch.isnan(g), torch.isnan(g64)) and bool(torch.isnan(g[5, 9, 0])) and int(torch.isnan(g).sum()) == 1
    assert float(g[~one].abs().max()) == 0.0


# ---- boxes -----------------------------------------------------------------------------------------------------------------------

FW, FH = 300, 280


@pytest.mark.parametrize("box", [2, 16, 17, REG_BOX, REG_BOX + 1, 160])
def test_boxes_match_fp64(dns, box):
    """Box sizes on both sides of the register-resident path; origins at (0, 0) and (H - box, W - box) and in between."""
    pred, gt = _frame(FW, FH)
    rows, cols = _origins([0, FH - box, (FH - box) // 2, 3], [0, FW - box, (FW - box) // 3, FW - box])
    _check(pred, gt, f"boxes of {box}", whole=False, rows=rows, cols=cols, box=box)


@pytest.mark.parametrize("layout", ["identical", "one_row_shared", "identical_pair_and_shifted"])
def test_overlapping_boxes_match_fp64(dns, layout):
    """Two identical boxes (counted twice); two boxes that share one row; and — one call has one box size, so one box can cover another
    only by being equal to it — a box, a copy of it later in the table and a third shifted by (4, 3) between them, which overlaps both."""
    pred, gt = _frame(FW, FH)
    box = 16
    rows, cols = {"identical": ([40, 40], [50, 50]), "one_row_shared": ([40, 55], [50, 50]), "identical_pair_and_shifted": ([40, 44, 40], [50, 53, 50])}[layout]
    r, c = _origins(rows, cols)
    _, g = _check(pred, gt, f"boxes {layout}", whole=False, rows=r, cols=c, box=box)
    if layout == "identical":
        _, g1 = _hip(pred, gt, False, None, r[:1], c[:1], box)          # mean over one box == mean over the box twice
        assert torch.equal(g, g1)


@pytest.mark.parametrize("n,W,H,box", [(1, FW, FH, 16), (60, FW, FH, 16), (PIECE, FW, FH, 16), (PIECE + 1, FW, FH, 16), (2 * PIECE + 1, FW, FH, 16),
                                        (1024, 400, 400, 16)])
def test_box_counts_match_fp64(dns, n, W, H, box):
    """One box, the 1080p default of 60, one past every piece of the region table, and 1024 boxes (no hidden cap)."""
    pred, gt = _frame(W, H)
    rows, cols = _random_origins(n, W, H, box, seed=n)
    _check(pred, gt, f"{n} boxes of {box} on {W}x{H}", whole=False, rows=rows, cols=cols, box=box)


def test_default_boxes_low_contrast_match_fp64(dns):
    """Boxes of 128 on pred = 5 + 0.01 u (with the whole-frame term, as the strategy calls it)."""
    W, H = 400, 272
    pred, gt = _frame(W, H, low_contrast=True)
    rows, cols = _random_origins(3, W, H, 128, seed=1)
    _check(pred, gt, "default boxes, low contrast", whole=True, rows=rows, cols=cols, box=128, w_whole=1.0, w_box=0.2)


def test_constant_block(dns):
    """A constant block of the prediction holding one whole box and part of another.  The value of the constant box is 1 - 0.
    Its gradient is what autograd gives: torch's backward of std() sends nothing through a standard deviation of exactly zero, so the
    pixels of that box get the (finite, large: 1 / 1e-6) path through the numerator and no nan appears; the nan set must be IDENTICAL
    to fp64 autograd's whatever it is, and every other pixel within tolerance."""
    pred, gt = _frame(FW, FH)
    pred = pred.clone()
    pred[30:60, 40:80] = 3.0
    box = 16
    rows, cols = _origins([35, 50, 100], [50, 70, 100])          # inside the block; half inside; outside
    v64, g64 = _restated(pred, gt, torch.float64, False, None, rows, cols, box)
    _, g32 = _restated(pred, gt, torch.float32, False, None, rows, cols, box)
    v, g = _hip(pred, gt, False, None, rows, cols, box)
    _check_value(v, v64, "constant block")
    assert torch.equal(torch.isnan(g), torch.isnan(g64)), "the nan pixels differ from fp64 autograd's"
    fin = ~torch.isnan(g64)
    z = torch.zeros_like
    _check_grad(torch.where(fin, g, z(g)), torch.where(fin, g64, z(g64)), torch.where(fin, g32, z(g32)), "d constant block / d pred")
    # the pixels outside the constant box on their own scale (the constant box's gradient is ~1e6 x larger)
    rest = fin.clone()
    rest[35:35 + box, 50:50 + box] = False
    _check_grad(torch.where(rest, g, z(g)), torch.where(rest, g64, z(g64)), torch.where(rest, g32, z(g32)), "d constant block / d pred, other pixels")
    # the whole frame constant: value 1, and the same rule
    flat = torch.full_like(pred, 2.5)
    v64, g64 = _restated(flat, gt, torch.float64, True, None, None, None, 0)
    v, g = _hip(flat, gt, True, None, None, None, 0)
    assert float(v) == 1.0 and float(v64) == 1.0
    assert torch.equal(torch.isnan(g), torch.isnan(g64))
    assert_close(g, g64, "d constant frame / d pred", GRAD_TOL)


# ---- weights, reproducibility ----------------------------------------------------------------------------------------------------


def test_combined_call_is_the_weighted_sum_of_the_separate_calls(dns):
    """Bit for bit.  The kernel rounds the whole-frame and the box gradient to fp32 separately and forms w_whole * g_whole + w_each *
    g_box with two rounded products and one rounded sum — the operations torch performs on the two separate results; w_each = w_box
    / n_boxes.  With a power-of-two number of boxes the separate call's 1 / n_boxes is an exact scaling, so w_box * (g_box / n) and
    (w_box / n) * g_box round alike and the two sides are the same fp32 expression; the values are formed from the same two sums in the
    same way.  (With another box count the two ways of applying w_box / n differ by an ulp of that term: held to 2 ulp of the larger
    term below.)"""
    from dn_splatter_amd import fused_loss as fl

    pred, gt = _frame(FW, FH)
    ww, wb = 0.7, 0.2
    for n in (4, 3):
        rows, cols = _random_origins(n, FW, FH, 16, seed=5)
        v, g = _hip(pred, gt, True, None, rows, cols, 16, ww, wb)
        v_w, g_w = _hip(pred, gt, True, None, None, None, 0)
        v_b, g_b = _hip(pred, gt, False, None, rows, cols, 16)
        want_g, want_v = ww * g_w + wb * g_b, ww * v_w + wb * v_b
        if n == 4:
            assert torch.equal(g, want_g) and torch.equal(v, want_v)
        else:
            ulp = torch.maximum((ww * g_w).abs(), (wb * g_b).abs()) * 2.0 ** -23
            assert bool(((g - want_g).abs() <= 2 * ulp).all())
            assert abs(float(v) - float(want_v)) <= 2 * 2.0 ** -23 * max(abs(ww * float(v_w)), abs(wb * float(v_b)))
    assert fl is not None


def test_two_calls_give_the_same_bits(dns):
    W, H = 400, 400
    pred, gt = _frame(W, H)
    rows, cols = _random_origins(300, W, H, 16, seed=9)
    a = _hip(pred, gt, True, None, rows, cols, 16, 1.0, 0.2)
    b = _hip(pred, gt, True, None, rows, cols, 16, 1.0, 0.2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- the modules -----------------------------------------------------------------------------------------------------------------


def test_local_module_draws_as_the_reference_and_never_synchronises(dns):
    """Seeded: the module's origins are the two randint draws of losses.py:475-476 on the device; its result is the functional form's
    on those origins, bit for bit; and the call (forward and backward) performs no host synchronisation."""
    from dn_splatter_amd import fused_loss as fl

    W, H, box = FW, FH, 16
    pred, gt = _frame(W, H)
    n_corr = int(0.5 * (H // box) * (W // box))
    torch.manual_seed(3)
    rows = torch.randint(0, H - box, size=(n_corr,), device=DEV)
    cols = torch.randint(0, W - box, size=(n_corr,), device=DEV)
    want_v, want_g = _hip(pred, gt, False, None, rows, cols, box)
    module = fl.LocalPearsonDepthLoss()
    x = pred.clone().requires_grad_(True)
    torch.manual_seed(3)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        v = module(x, gt, box_p=box)
        v.backward()
        w = fl.PearsonDepthLoss()(x, gt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(v.detach(), want_v) and torch.equal(x.grad, want_g)
    _check_value(w.detach(), _restated(pred, gt, torch.float64, True, None, None, None, 0)[0], "PearsonDepthLoss module")
    _check(pred, gt, "module origins", whole=False, rows=rows, cols=cols, box=box)
    with pytest.raises(RuntimeError):
        module(x[:box], gt[:box], box_p=box)                         # a frame no taller than a box: randint(0, 0)
    assert torch.isnan(module(x[:box + 8, :box + 8], gt[:box + 8, :box + 8], box_p=box))     # n_corr == 0: nan


def test_patched_strategy_equals_the_reference(dns, monkeypatch):
    """install_losses on a DNRegularization stand-in of type PearsonDepth: get_depth_loss on the fixture's strategy case (inputs and
    the origins the reference drew, uploaded) == the reference's value and gradient; nan without a valid ground-truth pixel."""
    import types

    from dn_splatter_amd import fused_loss as fl

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_pearson.npz"))
    tol, lam = (float(x) for x in g["strategy_defaults"])
    st = type("DNRegularization", (torch.nn.Module,), {"get_scale_loss": lambda self, scales: None,
                                                       "get_depth_loss": lambda self, p, t, **kw: None})()
    st.depth_tolerance, st.depth_lambda, st.depth_loss_type = tol, lam, types.SimpleNamespace(value="PearsonDepth")
    model = torch.nn.Module()
    model.regularization_strategy = st
    assert "regularization_strategy.get_depth_loss" in dns.install_losses(model)
    rows, cols = torch.from_numpy(g["big_rows"]).to(DEV), torch.from_numpy(g["big_cols"]).to(DEV)
    # the device generator draws other numbers than the host generator the fixture was made with: hand the fixture's origins over
    monkeypatch.setattr(fl, "draw_pearson_boxes", lambda depth_pred, box_p=128, p_corr=0.5: (rows, cols))
    pred = torch.from_numpy(g["big_pred"].astype(np.float32)).to(DEV).requires_grad_(True)
    gt = torch.from_numpy(g["big_gt"].astype(np.float32)).to(DEV)
    v = st.get_depth_loss(pred, gt)
    v.backward()
    ref, ref_g = float(g["strategy_value"]), torch.from_numpy(g["strategy_grad_rows4"]).to(DEV)
    _check_value(v.detach(), ref, "patched get_depth_loss")
    assert_close(pred.grad[::4], ref_g, "d patched get_depth_loss / d pred (every fourth row)", GRAD_TOL)
    assert torch.isnan(st.get_depth_loss(pred.detach(), gt * float(g["strategy_empty_scale"])))
