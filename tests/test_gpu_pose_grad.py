"""Camera pose gradient on the GPU: dnsplat_project_bwd_pose through _ProjectFn.backward, rasterization(viewmats=...), the fused
get_outputs path and GraphedStep, against fp64 references (tests/_pose_ref.py, oracle/dense_ref.py)."""
import os

import pytest
import torch

import _pose_ref
from _scenes import assert_close, cotangents, gsplat_inputs, to_leaf, zero_borderline

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U24 = 2.0 ** -24
POSE_C = 8.0      # |hip - S| <= 8 x 2^-24 x A: <= 1 per-Gaussian fp32 evaluation, 6 levels of the wave's tree, 1 rounding of the stored row


@pytest.fixture
def proj_bwd(monkeypatch):
    """Records what reaches _ProjectFn.backward (the gradient records and per-Gaussian cotangents) and what it returns."""
    from dn_splatter_amd import _ops

    class Calls(list):
        repeat = 0          # so many more launches on the same records and saved tensors, results kept in call["again"]

    calls = Calls()
    orig = _ops._ProjectFn.backward

    def backward(ctx, *grads):
        kept = [None if g is None else g.detach().clone() for g in grads]
        res = orig(ctx, *grads)
        saved = ctx.saved_tensors
        again = [orig(ctx, *[None if g is None else g.clone() for g in kept]) for _ in range(calls.repeat)]
        calls.append(dict(grads=kept, res=res, again=again, viewmat=saved[8].detach().clone(), K=saved[9].detach().clone(),
                          radii=saved[11].detach().clone(), cfg=ctx.cfg))
        return res

    monkeypatch.setattr(_ops._ProjectFn, "backward", staticmethod(backward))
    return calls


def _raw_params(inp, device):
    """gsplat_inputs (activated) -> the raw gauss_params the fused path takes."""
    eps = 1e-6
    o = inp["opacities"].clamp(eps, 1 - eps)
    gp = dict(means=inp["means"], quats=inp["quats"], scales=torch.log(inp["scales"]), opacities=torch.log(o / (1 - o))[:, None],
              features_dc=inp["colors"][:, 0].contiguous(), features_rest=inp["colors"][:, 1:].contiguous())
    return {k: v.detach().clone().to(device).requires_grad_(True) for k, v in gp.items()}


def _stage_cotangents(call, c=0):
    """The record columns and per-Gaussian cotangents of camera c as the kernel combines them, in fp64 on the CPU."""
    v_m2d, v_dep, v_con, v_cmp, v_spl = call["grads"][:5]
    N = call["radii"].shape[1]
    rec = v_spl[c * N:(c + 1) * N].double().cpu()
    cfg = call["cfg"]
    n_col = 3 if cfg.sh_degree >= 0 else None
    cot = dict(means2d=rec[:, 0:2].clone(), conics=rec[:, 2:5].clone(), opacities=rec[:, 5].clone())
    if v_m2d is not None:
        cot["means2d"] = cot["means2d"] + v_m2d.reshape(-1, N, 2)[c].double().cpu()
    if v_con is not None:
        cot["conics"] = cot["conics"] + v_con.reshape(-1, N, 3)[c].double().cpu()
    if n_col is not None:
        cot["colors"] = rec[:, 6:9].clone()
    dcol = 6 + (n_col if n_col is not None else 0)
    cot["depths"] = rec[:, dcol].clone() if cfg.with_depth else torch.zeros(N, dtype=torch.float64)
    if v_dep is not None:
        cot["depths"] = cot["depths"] + v_dep.reshape(-1, N)[c].double().cpu()
    return cot


@pytest.mark.parametrize("scene", ["c1_iso", "c1_aniso", "c2"])
def test_projection_backward_pose_gradient_within_its_condition_bound(dns, hip_deterministic, proj_bwd, scene):
    """The fused step with the real loss; the gradient records as they reach the projection backward go, in fp64, through the
    per-Gaussian reference: every entry of the HIP pose gradient within 8 x 2^-24 x A of S (A = sum_n |g_n|), exactly zero where A is.
    Measured worst |hip - S| / (2^-24 A) over the 16 entries (MI355X; profiles/pose_gradient.txt): see DESIGN.md section 5."""
    from dn_splatter_amd import synthetic, torch_losses as tl
    from dn_splatter_amd.fused_loss import dn_loss_fused

    if scene == "c2":
        N, W, H = 1_000_000, 1920, 1080
        gp = synthetic.make_gauss_params(N, sh_rest_std=0.1, seed=0, device=DEV)
        cam = synthetic.orbit_camera(0, width=W, height=H).to(DEV)
    else:
        N, W, H = 10_000, 256, 256
        inp, _, _, cam = gsplat_inputs(N, W, H, focal=160.0, seed=0 if scene == "c1_iso" else 1, anisotropic=(scene == "c1_aniso"))
        gp, cam = _raw_params(inp, DEV), cam.to(DEV)
    pose = cam.camera_to_worlds.detach().clone().requires_grad_(True)
    cam.camera_to_worlds = pose
    r = dns.DNSplatterRenderer(gp, fused=True)
    out = r.get_outputs(cam)
    loss = dn_loss_fused(out, tl.synthetic_batch(W, H, DEV, seed=3), gp["scales"])
    loss.backward()
    torch.cuda.synchronize()
    assert len(proj_bwd) == 1 and pose.grad is not None and pose.grad.shape == pose.shape
    call = proj_bwd[0]
    hip = call["res"][8].detach().double().cpu().reshape(4, 4)
    assert int(dns.load_library().dnsplat_pose_partial_rows(N)) >= (N + 63) // 64
    cpu = {k: v.detach().double().cpu() for k, v in gp.items()}
    colors = torch.cat([cpu["features_dc"][:, None], cpu["features_rest"]], 1)
    vis = call["radii"][0].cpu() > 0
    S, A = _pose_ref.pose_gradient_terms(cpu["means"], cpu["quats"], cpu["scales"].exp(), torch.sigmoid(cpu["opacities"]).squeeze(-1), colors,
                                         call["viewmat"][0].cpu(), call["K"][0].double().cpu(), W, H, 3, _stage_cotangents(call), visible=vis)
    ratio = (hip - S).abs() / (U24 * A).clamp_min(1e-300)
    worst = float(ratio[A > 0].max())
    line = (f"[pose] {scene}: N={N} visible={int(vis.sum())} worst |hip - S| / (2^-24 A) = {worst:.3f} (allowed {POSE_C}); "
            f"A / |S| max {float((A / S.abs().clamp_min(1e-300))[A > 0].max()):.0f}; per entry: "
            + " ".join(f"{float(x):.2f}" for x in ratio.reshape(-1)))
    print(line)
    if os.environ.get("DNSPLAT_POSE_LOG"):
        with open(os.environ["DNSPLAT_POSE_LOG"], "a") as f:
            f.write(line + "\n")
    assert bool((hip[A == 0] == 0).all())
    assert bool(((hip - S).abs() <= POSE_C * U24 * A).all()), line


@pytest.mark.parametrize("sh_degree,mode,aniso", [(3, "classic", False), (3, "antialiased", True), (None, "classic", True),
                                                  (None, "antialiased", False)])
def test_rasterization_viewmats_grad_matches_fp64_autograd(dns, orc, hip_deterministic, sh_degree, mode, aniso):
    """rasterization(viewmats.requires_grad) end to end against torch.autograd through oracle/dense_ref.render in fp64.  Cotangents are
    zero on the pixels the C oracle flags borderline (< 2 % of the image; seeds checked against the oracle alone).  Every entry within
    1e-4 x max|ref| of its group (rotation block, translation column, bottom row) + 4 x |ref32 - ref64|; direct colours: bottom row 0."""
    from oracle import dense_ref

    N, W, H = 256, 64, 64
    inp, viewmat, K, _ = gsplat_inputs(N, W, H, focal=40.0, seed=1 if aniso else 0, anisotropic=aniso)
    if sh_degree is None:
        inp = dict(inp, colors=torch.rand(N, 3, generator=torch.Generator().manual_seed(5)))
    kw = dict(width=W, height=H, packed=False, sh_degree=sh_degree, render_mode="RGB+ED", rasterize_mode=mode)
    _, _, info_o = orc.rasterization(**to_leaf(inp, "cpu"), viewmats=viewmat, Ks=K, **kw)
    border = info_o["borderline"].reshape(H, W).bool()
    share = float(border.sum()) / border.numel()
    print(f"[pose] end to end sh={sh_degree} {mode}: {int(border.sum())} of {border.numel()} pixels without a cotangent")
    assert share < 0.02
    keep = ~border
    v_r, v_a = cotangents([(1, H, W, 4), (1, H, W, 1)], seed=2)
    v_r, v_a = zero_borderline(v_r, keep), zero_borderline(v_a[..., 0], keep)[..., None]

    gi = to_leaf(inp, DEV)
    vm = viewmat.to(DEV).clone().requires_grad_(True)
    r_g, a_g, _ = dns.rasterization(**gi, viewmats=vm, Ks=K.to(DEV), **kw)
    ((r_g * v_r.to(DEV)).sum() + (a_g * v_a.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    assert vm.grad is not None and vm.grad.shape == (1, 4, 4)
    hip = vm.grad[0].double().cpu()

    def ref(dtype):
        c = {k: v.detach().to(dtype) for k, v in inp.items()}
        V = viewmat[0].to(dtype).clone().requires_grad_(True)
        out, alphas, _ = dense_ref.render(c["means"], c["quats"], c["scales"], c["opacities"], c["colors"], V, K[0].to(dtype), W, H,
                                          sh_degree=sh_degree, render_mode="RGB+ED", rasterize_mode=mode)
        (g,) = torch.autograd.grad((out * v_r[0].to(dtype)).sum() + (alphas * v_a[0, ..., 0].to(dtype)).sum(), V)
        return g.double()

    g64, g32 = ref(torch.float64), ref(torch.float32)
    groups = {"rotation": (slice(0, 3), slice(0, 3)), "translation": (slice(0, 3), slice(3, 4)), "bottom row": (slice(3, 4), slice(0, 4))}
    for name, idx in groups.items():
        a, b = hip[idx], g64[idx]
        allow = 1e-4 * float(b.abs().max()) + 4.0 * (g32[idx] - b).abs()
        worst = float(((a - b).abs() / allow.clamp_min(1e-300)).max()) if float(allow.max()) > 0 else 0.0
        print(f"[pose] end to end sh={sh_degree} {mode} {name}: max|ref| {float(b.abs().max()):.3e} worst error / allowance {worst:.3f}")
        assert bool(((a - b).abs() <= allow).all()), (name, a, b)
    if sh_degree is None:
        assert float(hip[3].abs().max()) == 0.0


def _raster_step(dns, inp, viewmat, K, W, H, pose_grad, seed=4, **kw):
    gi = to_leaf(inp, DEV)
    vm = viewmat.to(DEV).clone().requires_grad_(pose_grad)
    r, a, info = dns.rasterization(**gi, viewmats=vm, Ks=K.to(DEV), width=W, height=H, packed=False, absgrad=True, **kw)
    info["means2d"].retain_grad()
    v_r, v_a = cotangents([tuple(r.shape), tuple(a.shape)], seed)
    ((r * v_r.to(DEV)).sum() + (a * v_a.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in gi.items()}
    grads["means2d"], grads["means2d.absgrad"] = info["means2d"].grad, info["means2d"].absgrad
    return grads, vm.grad


@pytest.mark.parametrize("aniso", [False, True])
def test_asking_for_the_pose_leaves_every_other_gradient_bit_equal(dns, hip_deterministic, aniso):
    inp, viewmat, K, _ = gsplat_inputs(10_000, 256, 256, focal=160.0, seed=int(aniso), anisotropic=aniso)
    kw = dict(sh_degree=3, render_mode="RGB+ED")
    plain, none = _raster_step(dns, inp, viewmat, K, 256, 256, False, **kw)
    posed, v_vm = _raster_step(dns, inp, viewmat, K, 256, 256, True, **kw)
    assert none is None and v_vm is not None and float(v_vm.abs().max()) > 0
    for k in plain:
        assert torch.equal(plain[k], posed[k]), k


def test_pose_gradient_is_bit_reproducible_in_the_default_mode(dns, proj_bwd):
    """Default (atomics) mode: the gradient records differ from run to run, the pose reduction does not — the same saved records
    through the pose entry point twice give the same bits."""
    from dn_splatter_amd import _ops

    assert not _ops.DETERMINISTIC["on"]
    inp, viewmat, K, _ = gsplat_inputs(10_000, 256, 256, focal=160.0, seed=1, anisotropic=True)
    proj_bwd.repeat = 2
    _, v1 = _raster_step(dns, inp, viewmat, K, 256, 256, True, sh_degree=3, render_mode="RGB+ED")
    again = [res[8] for res in proj_bwd[0]["again"]]
    torch.cuda.synchronize()
    assert len(again) == 2 and torch.equal(again[0], again[1]) and torch.equal(again[0], v1)
    assert float(v1.abs().max()) > 0


def test_camera_batch_pose_gradients_equal_single_camera_calls(dns, hip_deterministic):
    from dn_splatter_amd import synthetic

    N, W, H = 10_000, 256, 256
    inp, _, K, _ = gsplat_inputs(N, W, H, focal=160.0, seed=1, anisotropic=True)
    vms = torch.cat([dns.get_viewmat(synthetic.orbit_camera(v, width=W, height=H, focal=160.0).camera_to_worlds) for v in (0, 2, 5)])
    Ks = K.repeat(3, 1, 1)
    kw = dict(width=W, height=H, packed=False, sh_degree=3, render_mode="RGB+ED")
    v_r, v_a = cotangents([(3, H, W, 4), (3, H, W, 1)], seed=6)
    vm = vms.to(DEV).clone().requires_grad_(True)
    r, a, _ = dns.rasterization(**to_leaf(inp, DEV), viewmats=vm, Ks=Ks.to(DEV), **kw)
    ((r * v_r.to(DEV)).sum() + (a * v_a.to(DEV)).sum()).backward()
    assert vm.grad.shape == (3, 4, 4)
    for c in range(3):
        v1 = vms[c:c + 1].to(DEV).clone().requires_grad_(True)
        r1, a1, _ = dns.rasterization(**to_leaf(inp, DEV), viewmats=v1, Ks=Ks[c:c + 1].to(DEV), **kw)
        ((r1 * v_r[c:c + 1].to(DEV)).sum() + (a1 * v_a[c:c + 1].to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        assert torch.equal(vm.grad[c], v1.grad[0]), c
        assert float(v1.grad.abs().max()) > 0


def _perturbed(c2w, seed=0, rot=0.02, shift=0.05):
    """A rigid pose a few hundredths of a radian / of a unit away from c2w [1,3,4]."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(3, generator=g) * 2 - 1) * rot
    Wm = torch.tensor([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    R = torch.linalg.matrix_exp(Wm)
    out = c2w.clone()
    out[0, :, :3] = R @ c2w[0, :, :3]
    out[0, :, 3] = c2w[0, :, 3] + (torch.rand(3, generator=g) * 2 - 1) * shift
    return out


def _optimised_pose_step(dns):
    """A 20 k-Gaussian frame whose projection pose is a [1,3,4] leaf (what a camera optimiser returns) next to the raw camera."""
    from dn_splatter_amd import synthetic

    N, W, H = 20_000, 320, 240
    gp = synthetic.make_gauss_params(N, sh_rest_std=0.1, seed=6, device=DEV)
    cam = synthetic.orbit_camera(1, width=W, height=H, focal=200.0)
    pose = _perturbed(cam.camera_to_worlds, rot=0.2).to(DEV).requires_grad_(True)
    cam = cam.to(DEV)
    keys = ("rgb", "depth", "normal", "accumulation")
    shapes = {"rgb": (H, W, 3), "depth": (H, W, 1), "normal": (H, W, 3), "accumulation": (H, W, 1)}
    gen = torch.Generator(device=DEV).manual_seed(8)
    cot = [torch.rand(shapes[k], device=DEV, generator=gen) * 2 - 1 for k in keys]
    r = dns.DNSplatterRenderer(gp, fused=True)

    def step():
        out = r.get_outputs(cam, optimized_camera_to_world=pose)
        torch.autograd.backward([out[k] for k in keys], cot)
        return out

    return gp, cam, pose, r, step


def test_fused_outputs_train_the_optimised_pose_and_keep_the_raw_camera_for_normals(dns, hip_deterministic, proj_bwd):
    """A stand-in camera optimiser returns a [1,3,4] leaf: its .grad is v_viewmat chained through get_viewmat (fp64 autograd, 1e-5 x
    max|ref|: nine multiply-adds per entry); the normal image follows the RAW camera, as DNSplatterRenderer(fused=False) fed the same
    pair renders it."""
    gp, cam, pose, r, step = _optimised_pose_step(dns)
    W, H = cam.width, cam.height
    out = step()
    torch.cuda.synchronize()
    assert pose.grad is not None and pose.grad.shape == (1, 3, 4)
    v_vm = proj_bwd[-1]["res"][8].detach().double().cpu().reshape(1, 4, 4)
    p64 = pose.detach().double().cpu().requires_grad_(True)
    (dns.get_viewmat(p64) * v_vm).sum().backward()
    assert_close(pose.grad.cpu(), p64.grad, "pose leaf .grad vs get_viewmat chain", tol=1e-5)

    # normals: the raw camera's frame.  The two-call path fed the same pair agrees; the fused path fed the optimised pose for both differs
    two_call = dns.DNSplatterRenderer({k: v.detach() for k, v in gp.items()}, fused=False)
    with torch.no_grad():
        n_ref = two_call.get_outputs(cam, optimized_camera_to_world=pose.detach())["normal"]
        n_opt = r.get_outputs(dns.Camera(pose.detach(), cam.fx, cam.fy, cam.cx, cam.cy, W, H))["normal"]
    off = ((out["normal"].detach() - n_ref).abs().amax(-1) > 1e-3).float().mean().item()
    off_opt = ((n_opt - n_ref).abs().amax(-1) > 1e-3).float().mean().item()
    print(f"[pose] normal image vs the two-call path with the same (optimised, raw) pair: {100 * off:.3f} % of pixels beyond 1e-3; "
          f"with the optimised pose for the normals too: {100 * off_opt:.1f} %")
    assert off < 0.01 and off_opt > 0.2


def test_graphed_step_replay_returns_the_eager_pose_gradient(dns, hip_deterministic):
    """The pose leaf listed in GraphedStep(params=...) gets its gradient under replay like the Gaussians' parameters."""
    from dn_splatter_amd.graph import GraphedStep

    gp, cam, pose, r, step = _optimised_pose_step(dns)
    step()
    torch.cuda.synchronize()
    eager = pose.grad.clone()
    try:
        r.forget()
        for v in list(gp.values()) + [pose]:
            v.grad = None
        g = GraphedStep(step, params=dict(gp, pose=pose))
        g()
        torch.cuda.synchronize()
        assert pose.grad is not None and torch.equal(pose.grad, eager), (pose.grad, eager)
        g.check()
        g.close()
    finally:
        dns.set_bin_policy("sync")


def test_sliced_exchange_refuses_a_pose_gradient(dns):
    """dp.SlicedShExchange launches the projection backward on slices of the Gaussians: together with a pose gradient it raises."""
    from dn_splatter_amd import _ops

    class Sliced:
        slices = 2

    inp, _, _, cam = gsplat_inputs(2_000, 64, 64, focal=40.0, seed=0)
    gp, cam = _raw_params(inp, DEV), cam.to(DEV)
    pose = cam.camera_to_worlds.clone().requires_grad_(True)
    out = dns.DNSplatterRenderer(gp, fused=True).get_outputs(cam, optimized_camera_to_world=pose)
    _ops.set_sh_exchange(Sliced())
    try:
        with pytest.raises(dns.DnsplatError, match="SlicedShExchange"):
            out["rgb"].sum().backward()
    finally:
        _ops.set_sh_exchange(None)


def test_finite_difference_sanity_of_the_translation_gradient(dns, hip_deterministic):
    """Not a statement about precision: moving the camera by 1e-3 along x changes an L2 image loss by v_t[0] x 1e-3 to within 5 % on a
    smooth scene — catches a wrong sign or a transposed matrix that a self-consistent reference could share."""
    N, W, H = 10_000, 256, 256
    inp, viewmat, K, _ = gsplat_inputs(N, W, H, focal=160.0, seed=0)
    inp = dict(inp, scales=inp["scales"] * 1.5)          # smooth: every pixel blends many wide splats
    kw = dict(Ks=K.to(DEV), width=W, height=H, packed=False, sh_degree=3, render_mode="RGB")
    gi = {k: v.to(DEV) for k, v in inp.items()}
    target = torch.full((1, H, W, 3), 0.3, device=DEV)

    def loss(vm):
        r, _, _ = dns.rasterization(**gi, viewmats=vm, **kw)
        return ((r - target).double() ** 2).sum()

    vm = viewmat.to(DEV).clone().requires_grad_(True)
    loss(vm).backward()
    v_t0 = float(vm.grad[0, 0, 3])
    h = 1e-3
    with torch.no_grad():
        d = torch.zeros_like(vm)
        d[0, 0, 3] = h
        fd = float(loss(vm.detach() + d) - loss(vm.detach() - d)) / 2.0
    print(f"[pose] finite difference along x: central difference {fd:.6e}, v_t[0] x 1e-3 = {v_t0 * h:.6e}")
    assert abs(fd - v_t0 * h) <= 0.05 * abs(v_t0 * h)
