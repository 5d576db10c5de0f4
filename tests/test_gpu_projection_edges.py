"""project_fwd_kernel / project_bwd_kernel (csrc/project.hip) per Gaussian against the fp64 reference of tests/_proj_ref.py, on scenes
that aim at the machinery keyed on a 64-lane workgroup and a visibility ballot: row-selective staging, the staged record store, the three
coefficient layouts, the backward's zero rows and inactive bands, the integer outputs, the saturation flag and the two-phase forward.

Everything goes through ``_ops.project`` and ``.backward()`` on its outputs; what is not reachable that way — a pre-filled ``splats``
buffer, NaN-filled gradient buffers, ``v_means2d`` beside garbage record columns — calls ``dnsplat_project_fwd`` / ``dnsplat_project_bwd``
through ``_lib``.

Tolerance: per entry ``k x max(a, b, c)`` (tests/_proj_ref.py), k = four times the worst ratio |kernel - fp64| / max(a, b, c) measured on
the MI355X over all scenes of this file, rounded up to a power of two, separately for the forward floats, the geometry gradients and
the SH gradients.  Measured (worst case over the cases of this file):

    group               worst ratio   where                                      4 x ratio   k
    forward floats          2.10      n1000 / split, conics[719, 1]                  8.4     16
    geometry gradients      2.66      modes_aa1_log0_logit1, v_quats[67, 3]         10.6     16
    SH gradients            1.04      colors4_logit, v_colors[87, 3]                 4.1      8

Terms (a) and (b) are taken over the +-1 ulp neighbours of the inputs that _proj_ref.unit_terms() describes.  With (a) from the
scene's inputs alone and (b) from two random draws the same kernel outputs measure 8.75 / 36.8 / 1.08, the 36.8 on v_scales[581, 0]
of n1000: an entry of -0.2009 that is a small sum of large terms, where the fp32 oracle's own error is 2.5e-7 at the scene's inputs
but 1.9e-6 in the median and 9.3e-6 at most over 32 neighbouring inputs, and the kernel's is 9.1e-6.  Over the whole scene the
kernel's and the fp32 oracle's relative errors have the same median and 99th percentile for every output.  Every test prints its
three ratios and, per group, the worst entry with its three terms (``[proj-edges] ...``, visible with ``-s``) before it asserts.
tests/test_projection_scenes.py shows that the nine mutations of a correct kernel it lists are all rejected even at k = 64.

The exclusion masks are conditions on the inputs: tests/test_projection_scenes.py asserts their caps with the reference alone.
"""
import ctypes

import pytest
import torch

import _proj_ref as P

pytestmark = pytest.mark.gpu

K_BOUND = dict(fwd=16.0, geo=16.0, sh=8.0)
CAT = P.catalogue()
DEV = "cuda"


def _leaf(t):
    return t.to(DEV).clone().requires_grad_(True)


def run_gpu(s, layout, cot=None, saturation_flag=None, side=None):
    """One ``_ops.project`` call (and backward with the cotangents ``cot``) -> dict of CPU tensors under the reference's keys."""
    from dn_splatter_amd import _ops

    cfg = s.cfg
    p = dict(means=_leaf(s.means), quats=_leaf(s.quats), scales=_leaf(s.scales), opacities=_leaf(s.opacities))
    sh = {}
    if layout == "colors":
        sh = dict(colors=_leaf(s.colors))
    else:
        sh = P.layout_tensors(s.coeffs, layout, DEV)
    need_nf = cfg.with_normals or cfg.want_normals_world
    out = _ops.project(p["means"], p["quats"], p["scales"], p["opacities"], **sh, viewmat=s.viewmat.to(DEV), K=s.K.to(DEV),
                       normal_frame=s.nf.to(DEV) if need_nf else None, cfg=cfg, saturation_flag=saturation_flag, side=side)
    torch.cuda.synchronize()
    N = s.N
    got = {k: out[k].detach().reshape((N,) + tuple(out[k].shape[2:])).cpu() for k in ("means2d", "depths", "conics", "radii", "tiles_per_gauss", "tiles_bin", "tile_boxes")}
    got["splats"] = out["splats"].detach().cpu()
    got["compensations"] = out["compensations"].detach().reshape(N).cpu() if cfg.antialiased else None
    got["normals_world"] = out["normals_world"].detach().reshape(N, 3).cpu() if cfg.want_normals_world else None
    if cot is not None and N > 0:
        outs, grads = [out["splats"]], [cot["v_splats"].to(DEV)]
        for key, name, shape in (("v_means2d", "means2d", (1, N, 2)), ("v_depths", "depths", (1, N)), ("v_conics", "conics", (1, N, 3)),
                                 ("v_compensations", "compensations", (1, N))):
            if cot[key] is not None:
                outs.append(out[name]); grads.append(cot[key].to(DEV).reshape(shape))
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
        got.update(v_means=p["means"].grad, v_quats=p["quats"].grad, v_scales=p["scales"].grad, v_opacities=p["opacities"].grad)
        if "coeffs" in sh:
            got["v_coeffs"] = sh["coeffs"].grad
        elif "sh0" in sh:
            got["v_sh0"], got["v_shN"] = sh["sh0"].grad, sh["shN"].grad
        else:
            got["v_colors"] = sh["colors"].grad
        for k in list(got):
            if k.startswith("v_"):
                assert got[k] is not None, k + ": no gradient arrived"
                got[k] = got[k].detach().cpu()
    return got


def reference_for(s, cot):
    """The reference of the TOTAL cotangent: ``_ProjectFn.backward`` hands the kernel v_means2d + the record's columns 0-1 (the kernel takes
    v_means2d INSTEAD of the columns)."""
    c = dict(cot)
    if c["v_means2d"] is not None:
        c["v_means2d"] = c["v_means2d"] + c["v_splats"][:, 0:2]
    return P.reference(s, c)


def check(got, ref, what, **kw):
    fails, ratios, worst = P.compare(got, ref, K_BOUND, **kw)
    print(f"[proj-edges] {what}: ratio fwd={ratios['fwd']:.3g} geo={ratios['geo']:.3g} sh={ratios['sh']:.3g} excluded={ref.shares()}")
    for grp, w in worst.items():
        print(f"[proj-edges]   worst {grp}: {w['key']}{list(w['index'])} got {w['got']:.9g} want {w['want']:.9g} a={w['a']:.3g} b={w['b']:.3g} c={w['c']:.3g}")
    assert not fails, (what, fails)


@pytest.mark.parametrize("name,layout", [(n, l) for n in CAT for l in CAT[n][1]])
def test_projection_matches_fp64(name, layout, orc):
    """Forward and backward of every catalogue scene in every layout it applies to: N and the partial workgroup, the visibility words
    inside a wave, degrees 0-3 (inactive bands: exact zeros, since their unit is zero), K = 9, direct colours, the modes, the culling
    boundaries and the boxes at the frame border."""
    s = CAT[name][0]()
    cot = P.make_cotangents(s.N, s.cfg, **P.ALL_ROUTES)
    ref = reference_for(s, cot)
    got = run_gpu(s, layout, cot)
    check(got, ref, f"{name}/{layout}")
    if s.cfg.want_normals_world:
        assert bool(torch.isfinite(got["normals_world"]).all()) and bool(((got["normals_world"].norm(dim=-1) - 1).abs() < 1e-5).all())


ROUTES = {"records_alone": {}, "means2d": dict(means2d=True), "conics": dict(conics=True), "depths": dict(depths=True)}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("layout", ["split", "cat"])
def test_cotangent_routes(route, layout, orc):
    s = P.random_scene(200, P.base_cfg(**P.FULL, antialiased=True, with_depth=True), seed=80, culled=P._some_culled(200, 80))
    cot = P.make_cotangents(s.N, s.cfg, seed=3, **ROUTES[route])
    check(run_gpu(s, layout, cot), reference_for(s, cot), f"route {route}/{layout}")


def test_n_zero_returns_empty_outputs():
    s = P.random_scene(1, P.base_cfg(**P.FULL), seed=1)
    e = P.replace(s, means=s.means[:0], quats=s.quats[:0], scales=s.scales[:0], opacities=s.opacities[:0], coeffs=s.coeffs[:0])
    for layout in ("split", "cat"):
        got = run_gpu(e, layout)
        assert got["radii"].shape == (0,) and got["splats"].shape == (0, 16) and got["means2d"].shape == (0, 2)
    torch.cuda.synchronize()


def forward_c_abi(s, layout, splats, skip_culled_records):
    """dnsplat_project_fwd through the C ABI into a caller-owned ``splats`` buffer (``_ops.project`` always allocates its own)."""
    from dn_splatter_amd import _lib, _ops

    cfg = P.replace(s.cfg, skip_culled_records=skip_culled_records)
    N = s.N
    d = lambda t: t.to(DEV).contiguous()      # noqa: E731
    means, quats, scales, opac = d(s.means), d(s.quats), d(s.scales), d(s.opacities)
    t = {k: v.detach() for k, v in P.layout_tensors(s.coeffs, layout, DEV).items()}
    if "coeffs" in t:
        c = t["coeffs"]
        scene = _ops._scene_struct(N, means, quats, scales, opac, cfg, c, 48, c.view(-1)[3:], 48, 16, None)
    else:
        scene = _ops._scene_struct(N, means, quats, scales, opac, cfg, t["sh0"], 3, t["shN"], 45, 16, None)
    vm, K = d(s.viewmat), d(s.K)
    cam = _ops._camera_struct(vm, K, None, cfg)
    i32 = lambda *sh: torch.empty(*sh, dtype=torch.int32, device=DEV)      # noqa: E731
    f32 = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=DEV)      # noqa: E731
    o = dict(radii=i32(N), means2d=f32(N, 2), depths=f32(N), conics=f32(N, 3), tiles=i32(N), boxes=i32(N, 2))
    out = _lib.ProjOut()
    out.radii, out.means2d, out.depths, out.conics = (_ops._ptr(o[k]) for k in ("radii", "means2d", "depths", "conics"))
    out.tiles_per_gauss, out.tile_boxes, out.splats = _ops._ptr(o["tiles"]), _ops._ptr(o["boxes"]), _ops._ptr(splats)
    out.skip_culled_records = int(skip_culled_records)
    _lib.run("dnsplat_project_fwd", _lib.lib().dnsplat_project_fwd, ctypes.byref(scene), ctypes.byref(cam), ctypes.byref(out), _ops._stream())
    torch.cuda.synchronize()
    return o["radii"].cpu()


@pytest.mark.parametrize("pattern", P.PATTERNS)
@pytest.mark.parametrize("layout", ["split", "cat", "cat_unaligned"])
def test_record_store_under_visibility_patterns(pattern, layout, orc):
    """skip_culled_records over a sentinel-filled buffer: culled records keep the sentinel, visible ones are complete; without it culled
    records are all zeros.  The buffer has a guard row behind the last Gaussian that nobody may write."""
    s = P.pattern_scene(pattern, P.base_cfg(**P.FULL), seed=3)
    ref = P.reference(s)
    vis = ref.out["radii"] > 0
    sentinel = -12345.5
    for skip in (True, False):
        buf = torch.full((s.N + 1, 16), sentinel, device=DEV)
        radii = forward_c_abi(s, layout, buf, skip)
        rec = buf.cpu()
        assert torch.equal(radii > 0, vis)
        assert bool((rec[s.N] == sentinel).all()), "the record store wrote past the last Gaussian"
        culled = rec[:s.N][~vis]
        assert bool((culled == (sentinel if skip else 0.0)).all()), "culled records: " + ("overwritten" if skip else "not all zeros")
        unit = ref.unit["splats"][vis]
        err = (rec[:s.N][vis].double() - ref.out["splats"][vis]).abs()
        ex = P._excluded(ref, "splats", ref.out["splats"].shape)[vis]
        assert bool(((err <= K_BOUND["fwd"] * unit) | ex).all()), "a visible record is incomplete or wrong"


def test_saturation_flag(orc):
    """Raised by a visible Gaussian whose activated opacity (x compensation when antialiased) exceeds 0.999; not by a culled one, not at
    0.999 exactly (the fp32 number the kernel compares against), not below."""
    from dn_splatter_amd import _ops

    cap = float(torch.tensor(P.ALPHA_MAX, dtype=torch.float32))
    above = float(torch.nextafter(torch.tensor(cap, dtype=torch.float32), torch.tensor(2.0)))
    N = 70

    def flag_of(opac, culled, antialiased=False):
        cul = torch.zeros(N, dtype=torch.bool)
        cul[culled] = True
        s = P.random_scene(N, P.base_cfg(sh_degree=3, antialiased=antialiased), seed=90, culled=cul, opac_act=opac)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = run_gpu(s, "split", saturation_flag=flag)
        return int(flag.item()), got

    base = torch.full((N,), 0.5)
    for lane in (0, 63, 69):
        hot = base.clone(); hot[lane] = above
        assert flag_of(hot, [])[0] == 1, f"lane {lane} above the cap: flag not raised"
        assert flag_of(hot, [lane])[0] == 0, f"lane {lane} above the cap but culled: flag raised"
        at = base.clone(); at[lane] = cap
        assert flag_of(at, [])[0] == 0, "opacity == 0.999: flag raised"
    assert flag_of(base, [])[0] == 0


@pytest.mark.parametrize("case", ["all_large", "all_small", "one_large_last_lane"])
def test_saturation_flag_antialiased(case, orc):
    """Antialiased: opacity x compensation decides.  Opacity 1.0 everywhere; a 50-pixel footprint has compensation 0.9999 (raises), a
    2-pixel one 0.93 (does not).  The expectation comes from the fp64 reference, at least 1e-4 away from the threshold."""
    N = 70
    g = torch.Generator().manual_seed(4)
    z = 1.5 + 4.5 * torch.rand(N, generator=g, dtype=torch.float64)
    large = {"all_large": torch.ones(N, dtype=torch.bool), "all_small": torch.zeros(N, dtype=torch.bool),
             "one_large_last_lane": torch.arange(N) == N - 1}[case]
    sc = (torch.where(large, 0.35 * z, 0.01 * z)[:, None] * torch.tensor([1.0, 0.8, 0.6], dtype=torch.float64))
    s = P.random_scene(N, P.base_cfg(sh_degree=3, antialiased=True), seed=91, z=z, scales_act=sc, opac_act=torch.ones(N))
    ref = P.reference(s)
    prod = ref.out["splats"][:, 5]
    assert not bool(ref.edge.any()) and bool((ref.out["radii"] > 0).all())
    assert not bool(((prod - P.ALPHA_MAX).abs() < 1e-4).any()), "a product sits on the threshold: the scene is badly built"
    want = int(bool((prod > P.ALPHA_MAX).any()))
    assert want == (0 if case == "all_small" else 1)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    run_gpu(s, "split", saturation_flag=flag)
    assert int(flag.item()) == want


def backward_c_abi(s, layout, radii, cot):
    """dnsplat_project_bwd through the C ABI with every gradient buffer pre-filled with NaN: a row the kernel does not write stays NaN.
    The coefficient gradients live in buffers of the coefficients' own layout (alignment included).  -> dict of CPU gradients."""
    from dn_splatter_amd import _lib, _ops

    cfg, N = s.cfg, s.N
    d = lambda t: None if t is None else t.to(DEV).contiguous()      # noqa: E731
    nan = lambda *sh: torch.full(sh, float("nan"), device=DEV)      # noqa: E731
    means, quats, scales, opac = d(s.means), d(s.quats), d(s.scales), d(s.opacities)
    t = {k: v.detach() for k, v in P.layout_tensors(s.coeffs, layout, DEV).items()}
    gt = {k: v.detach() for k, v in P.layout_tensors(torch.full_like(s.coeffs, float("nan")), layout, DEV).items()}
    g = _lib.ProjGrads()
    if "coeffs" in t:
        c, vc = t["coeffs"], gt["coeffs"]
        scene = _ops._scene_struct(N, means, quats, scales, opac, cfg, c, 48, c.view(-1)[3:], 48, 16, None)
        g.v_sh0, g.v_sh0_stride, g.v_shN, g.v_shN_stride = _ops._ptr(vc), 48, _ops._ptr(vc.view(-1)[3:]), 48
    else:
        scene = _ops._scene_struct(N, means, quats, scales, opac, cfg, t["sh0"], 3, t["shN"], 45, 16, None)
        g.v_sh0, g.v_sh0_stride, g.v_shN, g.v_shN_stride = _ops._ptr(gt["sh0"]), 3, _ops._ptr(gt["shN"]), 45
    vm, K, nf = d(s.viewmat), d(s.K), d(s.nf)
    cam = _ops._camera_struct(vm, K, nf if cfg.with_normals else None, cfg)
    fwd = _lib.ProjOut()
    fwd.with_depth_channel, fwd.with_normal_channels = int(cfg.with_depth), int(cfg.with_normals)
    keep = {k: d(v) for k, v in cot.items()}
    rad = radii.to(DEV).to(torch.int32).contiguous()
    out = dict(v_means=nan(N, 3), v_quats=nan(N, 4), v_scales=nan(N, 3), v_opacities=nan(N))
    g.radii, g.v_splats = _ops._ptr(rad), _ops._ptr(keep["v_splats"])
    g.v_means2d, g.v_depths, g.v_conics = _ops._ptr(keep["v_means2d"]), _ops._ptr(keep["v_depths"]), _ops._ptr(keep["v_conics"])
    g.v_compensations = _ops._ptr(keep["v_compensations"]) if cfg.antialiased else None
    g.v_means, g.v_quats, g.v_scales, g.v_opacities = (_ops._ptr(out[k]) for k in ("v_means", "v_quats", "v_scales", "v_opacities"))
    _lib.run("dnsplat_project_bwd", _lib.lib().dnsplat_project_bwd, ctypes.byref(scene), ctypes.byref(cam), ctypes.byref(fwd), ctypes.byref(g),
             _ops._stream())
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    if "coeffs" in gt:
        res["v_coeffs"] = gt["coeffs"].cpu()
    else:
        res["v_sh0"], res["v_shN"] = gt["sh0"].cpu(), gt["shN"].cpu()
    return res


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("layout", P.SH_LAYOUTS)
def test_backward_writes_every_row_and_ignores_record_xy(degree, layout, orc):
    """The C entry point over NaN-filled gradient buffers: the zero rows of culled Gaussians and the zero rows of the inactive bands must
    be WRITTEN (a NaN never passes the comparison), in the staged and in the direct layouts.  v_means2d is given and the gradient
    record's columns 0-1 hold NaN: the kernel must take v_means2d instead of them."""
    s = P.random_scene(P.PATTERN_N, P.base_cfg(sh_degree=degree, scales_are_log=True, opacities_are_logit=True, antialiased=True, with_depth=True),
                       seed=85, culled=P._some_culled(P.PATTERN_N, 85))
    cot = P.make_cotangents(s.N, s.cfg, seed=5, **P.ALL_ROUTES)
    cot["v_splats"][:, 0:2] = float("nan")
    ref = P.reference(s, cot)
    got = run_gpu(s, layout)
    got.update(backward_c_abi(s, layout, got["radii"], cot))
    check(got, ref, f"c-abi backward degree {degree}/{layout}")
    nb = (degree + 1) ** 2
    rows = got["v_coeffs"] if "v_coeffs" in got else torch.cat([got["v_sh0"][:, None], got["v_shN"]], 1)
    assert bool((rows[:, nb:] == 0).all()), "an inactive band's gradient row is not zero"
    assert bool((rows[got["radii"] == 0] == 0).all()), "a culled Gaussian's gradient row is not zero"


@pytest.mark.parametrize("N", [65, 257])
@pytest.mark.parametrize("layout", ["split", "cat", "cat_unaligned"])
def test_split_colours_is_bit_identical(N, layout, orc):
    s = P.random_scene(N, P.base_cfg(**P.FULL, with_depth=True), seed=95, culled=P._some_culled(N, 95))
    one = run_gpu(s, layout)
    side = {}
    two = run_gpu(P.with_cfg(s, split_colours=True), layout, side=side)
    assert "colours_ready" in side, "the two-phase path did not run"
    for k, v in one.items():
        if v is not None:
            assert torch.equal(v, two[k]), k
