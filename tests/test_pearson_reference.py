"""The Pearson depth losses against vectors produced by THE REFERENCE's own classes (tests/golden/make_reference_pearson_golden.py:
losses.py:428-485 and the PearsonDepth branch of DNRegularization.get_depth_loss, regularization_strategy.py:161-186):
the PyTorch restatements of torch_losses — the fp64 yardstick of tests/test_gpu_pearson.py — with the origins the reference drew, and
the bookkeeping of install_losses for this depth loss type.  Tolerances: those of test_reference_golden.py for the other loss terms."""
import os
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 2e-6          # test_reference_golden.test_loss_terms_equal_the_reference


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "reference_pearson.npz"))


def _check(value, wrt, ref, ref_grad, what, rows=slice(None)):
    assert abs(float(value.detach()) - float(ref)) < TOL * max(1.0, abs(float(ref))), (what, float(value.detach()), float(ref))
    (gr,) = torch.autograd.grad(value, wrt)
    ref_grad = torch.from_numpy(ref_grad)
    gr = gr[rows]
    assert gr.shape == ref_grad.shape, what
    assert float((gr - ref_grad).abs().max()) < TOL * max(1.0, float(ref_grad.abs().max())), what + " gradient"


def test_pearson_restatements_equal_the_reference(g):
    from dn_splatter_amd import torch_losses as tl

    pred = torch.from_numpy(g["small_pred"]).requires_grad_(True)
    gt = torch.from_numpy(g["small_gt"])
    rows, cols, box = torch.from_numpy(g["small_rows"]), torch.from_numpy(g["small_cols"]), int(g["small_box"])
    assert rows.numel() == 6 and box == 16
    _check(tl.pearson_depth(pred, gt), pred, g["small_whole"], g["small_whole_grad"], "whole frame 72x48")
    _check(tl.local_pearson_depth(pred, gt, rows, cols, box), pred, g["small_local"], g["small_local_grad"], "boxes of 16, 72x48")
    # the mask form is the reference's call on gathered pixels
    m = torch.rand(gt.shape, generator=torch.Generator().manual_seed(1)) > 0.4
    a = tl.pearson_depth(pred, gt, m)
    b = tl.pearson_depth(pred[m], gt[m])
    assert float(a.detach()) == float(b.detach())

    pred = torch.from_numpy(g["big_pred"].astype(np.float32)).requires_grad_(True)
    gt = torch.from_numpy(g["big_gt"].astype(np.float32))
    rows, cols = torch.from_numpy(g["big_rows"]), torch.from_numpy(g["big_cols"])
    assert rows.numel() == 3 and pred.shape == (int(g["big_H"]), int(g["big_W"]), 1)
    _check(tl.local_pearson_depth(pred, gt, rows, cols), pred, g["big_local"], g["big_local_grad"], "default boxes, 400x272")


def test_origins_are_the_two_randint_draws_of_the_reference(g):
    """fused_loss.draw_pearson_boxes consumes the generator as LocalPearsonDepthLoss.forward does: the fixture's origins come back."""
    from dn_splatter_amd import fused_loss

    for pre, box in (("small", int(g["small_box"])), ("big", 128)):
        torch.manual_seed(int(g[pre + "_seed"]))
        rows, cols = fused_loss.draw_pearson_boxes(torch.empty(int(g[pre + "_H"]), int(g[pre + "_W"]), 1), box)
        assert rows.dtype == torch.int64 and rows.tolist() == g[pre + "_rows"].tolist() and cols.tolist() == g[pre + "_cols"].tolist()
    with pytest.raises(RuntimeError):                       # a frame no larger than a box: what randint raises
        fused_loss.draw_pearson_boxes(torch.empty(128, 300, 1))
    m = fused_loss.LocalPearsonDepthLoss()
    assert torch.isnan(m(torch.rand(200, 200, 1), torch.rand(200, 200, 1)))           # n_corr = int(0.5 * 1 * 1) = 0: 0 / 0, no launch
    with pytest.raises(NotImplementedError):
        fused_loss.PearsonDepthLoss()(torch.rand(8, 8), torch.rand(8, 8).requires_grad_(True))


def test_strategy_branch_restatement_equals_the_reference(g):
    from dn_splatter_amd import torch_losses as tl

    tol, lam = (float(x) for x in g["strategy_defaults"])
    pred = torch.from_numpy(g["big_pred"].astype(np.float32)).requires_grad_(True)
    gt = torch.from_numpy(g["big_gt"].astype(np.float32))
    rows, cols = torch.from_numpy(g["big_rows"]), torch.from_numpy(g["big_cols"])
    valid = gt > tol
    assert bool(valid.any()) and not bool(valid.all())
    v = tl.pearson_depth_term(pred, gt, rows, cols, 128, lam, tol)
    _check(v, pred, g["strategy_value"], g["strategy_grad_rows4"], "get_depth_loss, PearsonDepth", rows=slice(None, None, 4))
    empty = tl.pearson_depth_term(pred, gt * float(g["strategy_empty_scale"]), rows, cols, 128, lam, tol)
    assert np.isnan(g["strategy_empty_value"]) and torch.isnan(empty)


def _stand_ins(depth_type):
    """A model whose strategy looks like the reference's (install_losses goes by class NAMES and the enum's value)."""
    PearsonDepthLoss = type("PearsonDepthLoss", (torch.nn.Module,), {})
    EdgeAwareLogL1 = type("EdgeAwareLogL1", (torch.nn.Module,), {"implementation": "scalar"})
    TVLoss = type("TVLoss", (torch.nn.Module,), {})
    Holder = type("Holder", (torch.nn.Module,), {})

    class DNRegularization(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.depth_tolerance, self.depth_lambda = 0.1, 0.2
            self.depth_loss_type = types.SimpleNamespace(value=depth_type)
            self.depth_loss, self.normal_smooth_loss = Holder(), Holder()
            self.depth_loss.loss = PearsonDepthLoss() if depth_type == "PearsonDepth" else EdgeAwareLogL1()
            self.normal_smooth_loss.loss = TVLoss()

        def get_depth_loss(self, pred_depth, gt_depth, **kwargs):
            return "reference"

        def get_scale_loss(self, scales):
            return "reference"

    m = torch.nn.Module()
    m.regularization_strategy = DNRegularization()
    return m


def test_install_losses_swaps_the_pearson_branch_by_name_and_type_value():
    import dn_splatter_amd as dns
    from dn_splatter_amd import fused_loss

    m = _stand_ins("PearsonDepth")
    st = m.regularization_strategy
    assert dns.install_losses(m) == ["regularization_strategy.depth_loss.loss", "regularization_strategy.normal_smooth_loss.loss",
                                     "regularization_strategy.get_scale_loss", "regularization_strategy.get_depth_loss"]
    assert isinstance(st.depth_loss.loss, fused_loss.PearsonDepthLoss)
    assert st.get_depth_loss.__name__ == "_hip_pearson_depth_loss"
    patched = st.get_depth_loss
    assert dns.install_losses(m) == [] and st.get_depth_loss is patched                # idempotent
    # a holder of the local module (strategies and model paths that call it directly)
    Local = type("LocalPearsonDepthLoss", (torch.nn.Module,), {})
    m2 = torch.nn.Module()
    m2.regularization_strategy = torch.nn.Module()
    m2.regularization_strategy.depth_loss = torch.nn.Module()
    m2.regularization_strategy.depth_loss.loss = Local()
    assert dns.install_losses(m2) == ["regularization_strategy.depth_loss.loss"]
    assert isinstance(m2.regularization_strategy.depth_loss.loss, fused_loss.LocalPearsonDepthLoss)
    # the exported names
    assert dns.PearsonDepthLoss is fused_loss.PearsonDepthLoss and dns.LocalPearsonDepthLoss is fused_loss.LocalPearsonDepthLoss
    assert dns.pearson_depth is fused_loss.pearson_depth and dns.local_pearson_depth is fused_loss.local_pearson_depth


def test_install_losses_leaves_the_edge_aware_strategy_as_it_was():
    import dn_splatter_amd as dns
    from dn_splatter_amd import fused_loss

    m = _stand_ins("EdgeAwareLogL1")
    st = m.regularization_strategy
    assert dns.install_losses(m) == ["regularization_strategy.depth_loss.loss", "regularization_strategy.normal_smooth_loss.loss",
                                     "regularization_strategy.get_scale_loss"]
    assert isinstance(st.depth_loss.loss, fused_loss.EdgeAwareLogL1)
    assert st.get_depth_loss(None, None) == "reference"                                  # the method is the strategy's own


def test_entry_point_refuses_impossible_arguments_without_a_launch(dns):
    """null pred, box < 2, box > min(H, W), n_boxes < 0: an error code, on a machine without a GPU."""
    from dn_splatter_amd import _lib

    dns.build_library()
    L = _lib.lib()
    # Real buffers of the sizes a valid call needs, on the device where there is one: were a check ever lost, the call would run on
    # memory it may touch instead of on a made-up address.
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    W, H = 64, 48
    pred, gt = torch.ones(H, W, device=dev), torch.ones(H, W, device=dev)
    mask = torch.ones(H, W, dtype=torch.bool, device=dev)
    origin = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = torch.zeros(L.dnsplat_pearson_scratch_bytes(1) // 8, dtype=torch.float64, device=dev)
    sums = torch.zeros(2, device=dev)
    ok = dict(width=W, height=H, pred=pred.data_ptr(), gt=gt.data_ptr(), mask=None, whole=1, n_boxes=1, box=16, rows=origin.data_ptr(),
              cols=origin.data_ptr())

    def call(**kw):
        a = {**ok, **kw}
        return L.dnsplat_pearson_depth(a["width"], a["height"], a["pred"], a["gt"], a["mask"], a["whole"], a["n_boxes"], a["box"],
                                       a["rows"], a["cols"], 1.0, 1.0, None, scratch.data_ptr(), sums.data_ptr(), None)

    assert call(pred=None) == -1
    assert call(box=1) == -1
    assert call(box=49) == -1                     # > min(W, H)
    assert call(n_boxes=-1) == -1
    assert call(width=0) == -1 and call(height=0) == -1
    assert call(rows=None) == -1
    assert call(mask=mask.data_ptr(), whole=0) == -1
    assert L.dnsplat_pearson_scratch_bytes(-1) == 0
    assert L.dnsplat_pearson_scratch_bytes(60) - L.dnsplat_pearson_scratch_bytes(0) == 60 * 48
