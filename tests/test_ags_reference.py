"""The AGS-Mesh regularisation strategy against vectors produced by THE REFERENCE's own code (tests/golden/
make_reference_ags_golden.py: find_edges, mean_angular_error, AGSMeshRegularization.get_normal_loss / get_depth_loss of
regularization_strategy.py and the "ags-mesh" branch of DNSplatterModel.get_loss_dict executed from its text): the PyTorch restatements
of torch_losses — the fp64 yardstick of tests/test_gpu_ags.py — in float32 and float64, the bookkeeping of install_losses for this
strategy, and the argument checks of the entry point.  Tolerances: those of test_reference_golden.py for the other loss terms."""
import os

import numpy as np
import pytest
import torch

import _ags_inputs as inputs

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 2e-6          # test_reference_golden.test_loss_terms_equal_the_reference


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "reference_ags.npz"))


def _close(got, ref, what):
    ref = torch.as_tensor(ref)
    got = torch.as_tensor(got).detach()
    assert got.shape == ref.shape, what
    assert float((got.double() - ref.double()).abs().max()) <= TOL * max(1.0, float(ref.abs().max())), what


@pytest.mark.parametrize("H,W", inputs.FIXTURE_FRAMES)
def test_masks_equal_the_reference(g, H, W):
    """Exactly, in float32 and in float64; and the frames keep the recipe's condition: no decision within the rounding envelope."""
    from dn_splatter_amd import torch_losses as tl

    f = inputs.fixture_frame(g, H, W)
    assert H % 16 and W % 16
    assert int(inputs.flagged_edge_decisions(f["gt"]).sum()) == 0 and int(inputs.flagged_confidence_decisions(f["surf"], f["gt"]).sum()) == 0
    for dt in (torch.float32, torch.float64):
        assert torch.equal(tl.ags_find_edges(f["gt"].to(dt)), f["edges"]), dt
        assert torch.equal(tl.ags_normal_confidence(f["surf"].to(dt), f["gt"].to(dt)), f["confident"]), dt
    share = float(f["edges"].float().mean())
    assert 0.1 < share < 0.35 and 0.3 < float(f["confident"].float().mean()) < 0.7          # both filters select and reject
    # a border pixel with a negative component is an edge: its missing neighbours count as 0
    gt = f["gt"]
    border = torch.zeros(3, H, W, dtype=torch.bool)
    border[:, 0], border[:, -1], border[:, :, 0], border[:, :, -1] = True, True, True, True
    assert bool(f["edges"][border & (gt < 0)].all()) and bool((border & (gt < 0)).any())


@pytest.mark.parametrize("H,W", inputs.FIXTURE_FRAMES)
@pytest.mark.parametrize("step", inputs.FIXTURE_STEPS)
def test_normal_loss_restatement_equals_the_reference(g, H, W, step):
    from dn_splatter_amd import torch_losses as tl

    f = inputs.fixture_frame(g, H, W)
    _, lam_d, lam_n, mask_steps = (float(x) for x in g["defaults"])
    value, v_surf, v_pred = inputs.fixture_result(g, H, W, step)
    assert (value == 0.0) == (step <= 7000)
    for dt in (torch.float32, torch.float64):
        s, p = f["surf"].to(dt).clone().requires_grad_(True), f["pred"].to(dt).clone().requires_grad_(True)
        v = tl.ags_normal_loss(s, f["gt"].to(dt), p, step, lam_n, int(mask_steps))
        gs, gp = torch.autograd.grad(v, [s, p])
        _close(v, value, f"value, step {step}, {dt}")
        _close(gs, v_surf, f"d / d surf, step {step}, {dt}")
        _close(gp, v_pred, f"d / d pred, step {step}, {dt}")
    # a given selection takes the place of the computed one
    sel = ~f["edges"] if step < mask_steps else f["confident"]
    v2 = tl.ags_normal_loss(f["surf"], f["gt"], f["pred"], step, lam_n, int(mask_steps), selection=sel)
    assert float(v2) == float(tl.ags_normal_loss(f["surf"], f["gt"], f["pred"], step, lam_n, int(mask_steps)))
    empty = tl.ags_normal_loss(f["surf"], f["gt"], f["pred"], step, lam_n, int(mask_steps), selection=torch.zeros_like(sel))
    assert torch.isnan(empty)                                                                # the mean of nothing, times any weight


def _model_case(g, dtype=torch.float32):
    t = lambda k: torch.from_numpy(g[k])       # noqa: E731
    leaf = lambda k: t(k).to(dtype).requires_grad_(True)      # noqa: E731
    out = {"rgb": t("m_pred_rgb").to(dtype), "depth": leaf("m_pred_depth"), "normal": leaf("m_pred_normal"),
           "surface_normal": leaf("m_surface_normal")}
    batch = {"image": t("m_image").to(dtype), "mono_depth": t("m_gt_depth").to(dtype), "normal": (t("m_gt_normal_u8").float() / 255.0).to(dtype),
             "confidence": t("m_confidence").to(dtype), "mask": t("m_mask").to(dtype)}
    return out, batch, leaf("m_scales")


def test_loss_dict_branch_restatement_equals_the_reference(g):
    """torch_losses.ags_regularization_term == get_loss_dict's "ags-mesh" branch less the recorded rgb term, with a confidence image
    and a mask in the batch; value and every gradient (the surface normal's too: the factor 2 of 2 x - 1)."""
    from dn_splatter_amd import torch_losses as tl

    assert np.allclose(g["defaults"], [0.1, 0.2, 0.1, 15000])
    want = float(g["m_main"]) - float(g["m_rgb_term"])
    for dt in (torch.float32, torch.float64):
        out, batch, sc = _model_case(g, dt)
        v = tl.ags_regularization_term(out, batch, sc, int(g["m_step"]))
        assert abs(float(v.detach()) - want) < TOL, (dt, float(v.detach()), want)
        grads = torch.autograd.grad(v, [out["depth"], out["normal"], out["surface_normal"], sc])
        for got, key in zip(grads, ("m_v_depth", "m_v_normal", "m_v_surface_normal", "m_v_scales")):
            _close(got, g[key], f"{key}, {dt}")
    assert float(np.abs(g["m_v_surface_normal"]).max()) > 0


@pytest.mark.parametrize("step", [6999, 7000])
def test_depth_mask_equals_the_reference_depth_loss(g, step):
    """EdgeAwareLogL1 under ags_depth_mask x depth_lambda == AGSMeshRegularization.get_depth_loss: the confidence filter sets in AT
    step 7000 (the normal weight only after it)."""
    from dn_splatter_amd import torch_losses as tl

    out, batch, _ = _model_case(g)
    pd = out["depth"]
    conf = 1 - batch["confidence"] / 255.0
    mask = tl.ags_depth_mask(batch["mono_depth"], conf, step, 0.1)
    plain = batch["mono_depth"] > 0.1
    assert torch.equal(mask, plain) == (step < 7000) and bool(mask.any())
    v = tl.edge_aware_log_l1(pd, batch["mono_depth"], batch["image"].clamp(min=10 / 255.0), mask) * 0.2
    assert abs(float(v.detach()) - float(g[f"m_depth_loss_{step}"])) < TOL
    _close(torch.autograd.grad(v, pd)[0], g[f"m_depth_loss_{step}_grad"], "d depth loss / d depth")


def _stand_in(name="AGSMeshRegularization"):
    """A model whose strategy looks like the reference's (install_losses goes by class NAMES)."""
    EdgeAwareLogL1 = type("EdgeAwareLogL1", (torch.nn.Module,), {"implementation": "scalar"})
    TVLoss = type("TVLoss", (torch.nn.Module,), {})
    Holder = type("Holder", (torch.nn.Module,), {})

    def init(self):
        torch.nn.Module.__init__(self)
        self.depth_tolerance, self.depth_lambda, self.normal_lambda, self.normal_mask_steps = 0.1, 0.2, 0.1, 15000
        self.depth_loss, self.normal_smooth_loss = Holder(), Holder()
        self.depth_loss.loss, self.normal_smooth_loss.loss = EdgeAwareLogL1(), TVLoss()

    cls = type(name, (torch.nn.Module,), {"__init__": init, "get_normal_loss": lambda self, *a, **k: "reference",
                                         "get_depth_loss": lambda self, *a, **k: "reference",
                                         "get_scale_loss": lambda self, scales: "reference"})
    m = torch.nn.Module()
    m.regularization_strategy = cls()
    return m


def test_install_losses_replaces_the_normal_loss_of_the_ags_strategy_only():
    import dn_splatter_amd as dns
    from dn_splatter_amd import fused_loss

    m = _stand_in()
    st = m.regularization_strategy
    assert dns.install_losses(m) == ["regularization_strategy.depth_loss.loss", "regularization_strategy.normal_smooth_loss.loss",
                                     "regularization_strategy.get_scale_loss", "regularization_strategy.get_normal_loss"]
    assert st.get_normal_loss.__name__ == "_hip_ags_normal_loss" and st.get_depth_loss() == "reference"
    assert isinstance(st.depth_loss.loss, fused_loss.EdgeAwareLogL1)
    patched = st.get_normal_loss
    assert dns.install_losses(m) == [] and st.get_normal_loss is patched                  # idempotent
    # other class names keep their method
    for name in ("DNRegularization", "SomethingElse"):
        other = _stand_in(name)
        assert "regularization_strategy.get_normal_loss" not in dns.install_losses(other)
        assert other.regularization_strategy.get_normal_loss() == "reference"
    # there is no CPU path behind the closure: a missing GPU is an error, not a fall-back to PyTorch
    x = torch.zeros(3, 4, 5)
    with pytest.raises(dns.DnsplatError):
        st.get_normal_loss(8000, x, x, x)
    with pytest.raises(dns.DnsplatError):
        fused_loss.ags_mesh_loss_fused({"rgb": torch.zeros(4, 5, 3)}, {}, torch.zeros(2, 3), 8000)
    with pytest.raises(NotImplementedError):
        fused_loss.ags_normal_loss(x, x.clone().requires_grad_(True), x, 8000)
    assert dns.ags_normal_loss is fused_loss.ags_normal_loss and dns.ags_mesh_loss_fused is fused_loss.ags_mesh_loss_fused


def test_entry_point_refuses_impossible_arguments_without_a_launch(dns):
    """Every invalid-argument return of dnsplat_ags_normal_loss: an error code, on a machine without a GPU."""
    from dn_splatter_amd import _lib

    dns.build_library()
    L = _lib.lib()
    # real buffers of the sizes a valid call needs, on the device where there is one (test_pearson_reference.py: were a check ever
    # lost, the call would run on memory it may touch)
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    W, H = 70, 45
    img = torch.full((3, H, W), 0.5, device=dev)
    scratch = torch.zeros(L.dnsplat_ags_normal_scratch_bytes(W, H) // 8, dtype=torch.float64, device=dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    ok = dict(width=W, height=H, surf=img.data_ptr(), gt=img.data_ptr(), pred=img.data_ptr(), layout=0, mode=0, scratch=scratch.data_ptr(),
              sums=sums.data_ptr(), count=count.data_ptr())

    def call(**kw):
        a = {**ok, **kw}
        return L.dnsplat_ags_normal_loss(a["width"], a["height"], a["surf"], a["gt"], a["pred"], a["layout"], a["mode"], 1.0, None, None, None,
                                         a["scratch"], a["sums"], a["count"], None)

    for name in ("surf", "gt", "pred", "scratch", "sums", "count"):
        assert call(**{name: None}) == -1, name
    assert call(width=0) == -1 and call(height=0) == -1 and call(width=-3) == -1
    assert call(layout=2) == -1 and call(layout=-1) == -1
    assert call(mode=2) == -1 and call(mode=-1) == -1
    assert call(width=2 ** 31 - 1, height=2 ** 31 - 1) == -4                              # more tiles than a grid holds: unsupported
    assert L.dnsplat_ags_normal_scratch_bytes(0, 5) == 0 and L.dnsplat_ags_normal_scratch_bytes(5, -1) == 0
    # one 24-byte partial per tile of 64 x 16 pixels
    assert L.dnsplat_ags_normal_scratch_bytes(64, 16) == 24 and L.dnsplat_ags_normal_scratch_bytes(65, 17) == 4 * 24
