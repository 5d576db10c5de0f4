"""The compositing kernels (csrc/raster_fwd.hip, csrc/raster_bwd.hip) at their batch, bucket and fold edges.

The frames (tests/_scenes.py edge_frame) are built at raster level, one case per half tile: every list entry is a point splat that
reaches exactly one pixel, so a recipe fixes how many entries a half tile keeps, where each pixel stops and where the backward's
bound `hi` lies.  edge_model recomputes all of it in float64 from the oracle's lists, and every test prints the regime each case
reaches (bucket sizes, fold, queue carry; tests/test_edge_scenes.py checks the recipes on the CPU).  Every frame goes through the
generic kernels (SPLIT = D for D in 1, 2, 3, 4, 7, 8; SPLIT = -1), the fused DN kernel (keep masks on and off, both saturation
twins, capped alphas) and a batch of three cameras, in the default and the deterministic gradient mode, against the oracle and
against each other.

Each contributing splat lies inside one tile, so its gradient record receives at most two rows (one per half tile) and their sum
does not depend on the order the atomics arrive in: runs of the same instantiation on frames that differ only in culled entries,
in list offsets or in batching must agree to the last bit, in both modes."""
import functools

import pytest
import torch

from _scenes import (COND_C_DEFAULT, COND_LAMBDA_DEFAULT, EDGE_SMALL, assert_close, assert_equal_int, check_pixels, check_rows_conditioned, edge_cameras, edge_frame,
                     edge_lists, edge_main_cases, edge_model, oracle_threads, regime_line)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_KEYS = ("means2d", "absgrad", "conics", "colors", "opacities")
BG7 = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0])     # the fused pass: no background for rgb | depth, ones for the normals
INTR = (100.0, 100.0, 64.0, 64.0)
MODES = (False, True)                                        # deterministic gradient mode off / on
EPILOGUE_ROUNDINGS = 4.0                                     # see _check_grads


@pytest.fixture(scope="module", autouse=True)
def _exact_oracle(orc):
    """The oracle's gradient scatter in double: an order-independent reference for both modes."""
    oracle_threads()
    prev = orc.set_exact_accumulation(True)
    yield
    orc.set_exact_accumulation(prev)


@functools.lru_cache(maxsize=None)
def _frame(name, interleave=False, phase=0):
    from oracle import oracle as orc

    if name == "main":
        s = edge_frame(edge_main_cases(), 256, 256, interleave=interleave, phase=phase)
    else:
        W, H, cases, kw = EDGE_SMALL[name]
        s = edge_frame(cases, W, H, interleave=interleave, phase=phase, **kw)
    offs, fid = edge_lists(orc, s)
    return s, offs, fid, edge_model(s, offs, fid)


def _print_regimes(s, model, what):
    by = {(r["tile"], r["half"]): r for r in model}
    for t, h, n, stop in s["cases"]:
        r = by.get((t, h))
        if r is None:
            assert n == 0
            print(f"[raster] {what}: {n} x {stop}: tile {t} {('top', 'bottom')[h]}: empty list")
            continue
        assert r["kept"] == n, f"tile {t} half {h}: {r['kept']} kept entries, the recipe has {n}"
        print(regime_line(r, f"{what}: {n} x {stop}: "))


def _same(a, b, what, exact=True):
    eq = bool(torch.equal(a, b))
    print(f"[raster] {what}: {'bit-equal' if eq else 'not bit-equal, max |d| %.3e' % float((a.double() - b.double()).abs().max())}")
    if exact:
        assert eq, f"{what}: the two runs differ"
    return eq


# ---- the oracle -----------------------------------------------------------------------------------------------------------------


def _ofwd(orc, s, offs, fid, cols, bg, dtype=torch.float32):
    W, H = s["W"], s["H"]
    f = lambda t: t.to(dtype).contiguous()                                   # noqa: E731
    border = torch.zeros(H, W, dtype=torch.uint8) if dtype == torch.float32 else None
    flip = torch.zeros(H, W, dtype=torch.float32) if dtype == torch.float32 else None
    r, a, last = orc.rasterize_fwd(f(s["xys"]), f(s["conics"]), f(cols), f(s["opacities"]), f(bg), W, H, 16, offs, fid, border, flip)
    if border is not None:
        assert int(border.sum()) == 0, "the edge frames keep every decision away from its threshold"
    return r, a, last


def _obwd(orc, s, offs, fid, cols, bg, alphas, last, v_r, v_a, split, dtype=torch.float32):
    """The oracle's raster-level gradients when channels [0, split) carry v_alphas and the screen-space gradient and channels
    [split, D) carry neither: two calls, as the reference's two passes (dn_model.py:562 feeds xys.detach() to the second); conic and
    opacity gradients added.  With dtype float32 also the condition bounds A / S of the sum (rasterize_bwd_cond)."""
    D = cols.shape[1]
    N, H, W = s["N"], s["H"], s["W"]
    f = lambda t: t.to(dtype).contiguous()                                   # noqa: E731
    if split == D:
        parts = [(cols, bg, v_r, v_a, True)]
    else:
        lo = (cols[:, :split], bg[:split], v_r[..., :split]) if split > 0 else (torch.zeros(N, 1), torch.zeros(1), torch.zeros(H, W, 1))
        parts = [lo + (v_a, True), (cols[:, split:], bg[split:], v_r[..., split:], torch.zeros_like(v_a), False)]
    g = {"conics": 0, "opacities": 0, "colors": []}
    A = {"conics": 0, "opacities": 0, "colors": []}
    B = {"conics": 0, "opacities": 0, "colors": []}
    for c, b, vr, va, xy in parts:
        args = (f(s["xys"]), f(s["conics"]), f(c), f(s["opacities"]), f(b), W, H, 16, offs, fid, f(alphas), last)
        m2, ab, cn, cc, op = orc.rasterize_bwd(*args, f(vr), f(va), absgrad=True)
        dummy = split == 0 and xy
        if xy:
            g["means2d"], g["absgrad"] = m2, ab
        g["conics"] = g["conics"] + cn
        g["opacities"] = g["opacities"] + op
        if not dummy:
            g["colors"].append(cc)
        if dtype == torch.float32:
            a_, b_ = orc.rasterize_bwd_cond(*args, f(vr).abs(), f(va).abs())
            for d, m in ((A, a_), (B, b_)):
                if xy:
                    d["means2d"], d["absgrad"] = m[:, 0:2], m[:, 2:4]
                d["conics"] = d["conics"] + m[:, 4:7]
                d["opacities"] = d["opacities"] + m[:, 7]
                if not dummy:
                    d["colors"].append(m[:, 8:])
    for d in (g, A, B):
        d["colors"] = torch.cat(d["colors"], 1) if d["colors"] else None
    S = {k: v.sqrt() for k, v in B.items() if torch.is_tensor(v)}
    return g, A, S


def _check_grads(hip, o, A, S, s, what, det, epilogue=False):
    """Every visible row within the oracle's running error bound: COND_C x 2^-24 x ||A_g|| in the deterministic mode, COND_C_DEFAULT
    in the default mode.  ``epilogue``: the fused kernel forms the raw composite's cotangents from its OWN images (the dn epilogue's
    derivative), the oracle from its own.  Those cotangents then differ by the epilogue's own roundings (a division by alpha, the
    unit-normal derivative: EPILOGUE_ROUNDINGS of them) on top of what the bound of the raster-level backward counts, and at
    low-alpha pixels the expected depth acc / alpha scales the differing terms by 1 / alpha.  So in both modes A is held to
    COND_C_DEFAULT + EPILOGUE_ROUNDINGS and S (the independent-roundings model, which does not see terms that cancel) to twice
    COND_LAMBDA_DEFAULT.  Measured on the main frame: 8.1 A / 26.7 S, the same bits in both modes."""
    visible = s["radii"] > 0
    for k in GRAD_KEYS:
        if not epilogue:
            check_rows_conditioned(hip[k], o[k], A[k], S[k], visible, f"{what} {k}", strict=det)
            continue
        _n, wa, ws = check_rows_conditioned(hip[k], o[k], A[k], S[k], visible, f"{what} {k}", enforce=False, strict=det)
        c_lim, l_lim = COND_C_DEFAULT, COND_LAMBDA_DEFAULT      # the epilogue's share is the same in both modes
        assert wa <= c_lim + EPILOGUE_ROUNDINGS, f"{what} {k}: a row is {wa:.3f} x its worst-case running error bound"
        assert ws <= 2 * l_lim, f"{what} {k}: a row is {ws:.3f} standard deviations of the independent-roundings model off"
    # listed but culled entries and the padding receive nothing
    for k in GRAD_KEYS:
        rest = hip[k][s["n_case"]:]
        assert not bool(rest.ne(0).any()), f"{what} {k}: a culled entry received a gradient"


def _fp64_note(hip, g64, what):
    parts = []
    for k in GRAD_KEYS:
        b = g64[k].double().reshape(g64[k].shape[0], -1)
        a = hip[k].double().reshape(b.shape)
        nb = b.norm(dim=1)
        sel = nb > 0
        parts.append(f"{k} {float(((a - b).norm(dim=1)[sel] / nb[sel]).max()) if bool(sel.any()) else 0.0:.1e}")
    print(f"[raster] {what}: largest row-relative distance from the float64 oracle: " + ", ".join(parts))


# ---- the kernels --------------------------------------------------------------------------------------------------------------


def _leaves(s, cols):
    return {k: t.to(DEV).contiguous().clone().requires_grad_(True)
            for k, t in (("xys", s["xys"]), ("conics", s["conics"]), ("colors", cols), ("opacities", s["opacities"]))}


def _grads(m2d, lv, c):
    return {"means2d": (m2d.grad[c] + lv["xys"].grad).cpu(), "absgrad": m2d.absgrad[c].reshape(-1, 2).cpu(),
            "conics": lv["conics"].grad.cpu(), "colors": lv["colors"].grad.cpu(), "opacities": lv["opacities"].grad.cpu()}


def _stacked(frames):
    st = lambda k: torch.stack([s[k] for s in frames]).to(DEV)              # noqa: E731
    return st("depths"), st("radii"), st("tiles")


def _check_binning(b, frames, lists):
    """The kernels' lists of the batch are the oracle's, camera after camera (entry = camera x N + Gaussian)."""
    N = frames[0]["N"]
    n = b.n_isects
    fid = torch.cat([l[1].long() + c * N for c, l in enumerate(lists)])
    base = torch.cumsum(torch.tensor([0] + [l[1].numel() for l in lists[:-1]]), 0)
    offs = torch.cat([l[0].reshape(-1).long() + base[c] for c, l in enumerate(lists)])
    assert_equal_int(b.flatten_ids[:n].cpu().long(), fid, "flatten_ids")
    assert_equal_int(b.filled_offsets()[:offs.numel()].cpu().long(), offs, "tile offsets")


def _hip_generic(frames, lists, D, split, cots, det, cols=None, bg=None):
    """_ops.rasterize over the cameras of ``frames`` (records packed by dnsplat_pack_splats): per camera (render, alphas, grads)."""
    from dn_splatter_amd import _ops

    prev = _ops.DETERMINISTIC["on"]
    _ops.set_deterministic(det)
    try:
        s0 = frames[0]
        lv = [_leaves(s, s["colors8"][:, :D] if cols is None else cols) for s in frames]
        splats = torch.cat([_ops._PackFn.apply(l["xys"], l["conics"], l["opacities"], l["colors"]) for l in lv])
        m2d = torch.stack([l["xys"].detach() for l in lv]).clone().requires_grad_(True)
        holder = {}
        render, alphas = _ops.rasterize(m2d, splats, *_stacked(frames), background=(s0["background8"][:D] if bg is None else bg).to(DEV),
                                        width=s0["W"], height=s0["H"], tile_size=16, D=D, xy_split=split, absgrad=True, holder=holder)
        _check_binning(holder["binning"], frames, lists)
        torch.autograd.backward([render, alphas], [torch.stack([c[0] for c in cots]).to(DEV), torch.stack([c[1] for c in cots]).to(DEV)])
        torch.cuda.synchronize()
        return [(render[c].detach().cpu(), alphas[c].detach().cpu(), _grads(m2d, lv[c], c)) for c in range(len(frames))]
    finally:
        _ops.set_deterministic(prev)


def _hip_fused(frames, lists, cots, det, masks=True, sat=1, bg_rgb=None):
    """_ops.rasterize_dn (the fused 7-channel kernels with the dn epilogue) over the cameras of ``frames``; ``sat``: the saturation
    flag word (0: the clamp-free backward twin runs, 1: the clamping loop).  Per camera ((rgb, depth, normal, accumulation), grads)."""
    from dn_splatter_amd import _ops

    assert _ops.SATURATION_FLAG
    prev = (_ops.DETERMINISTIC["on"], _ops.KEEP_MASKS)
    _ops.set_deterministic(det)
    _ops.KEEP_MASKS = masks
    try:
        s0 = frames[0]
        lv = [_leaves(s, s["colors8"][:, :7]) for s in frames]
        splats = torch.cat([_ops._PackFn.apply(l["xys"], l["conics"], l["opacities"], l["colors"]) for l in lv])
        m2d = torch.stack([l["xys"].detach() for l in lv]).clone().requires_grad_(True)
        holder = {"saturation_flag": torch.tensor([sat], dtype=torch.int32, device=DEV)}
        outs = _ops.rasterize_dn(m2d, splats, *_stacked(frames), background_rgb=(s0["background8"][:3] if bg_rgb is None else bg_rgb).to(DEV),
                                 width=s0["W"], height=s0["H"], intrinsics=[INTR] * len(frames), absgrad=True, holder=holder)[:4]
        assert bool(holder["saturation_flag"].item() == sat)
        _check_binning(holder["binning"], frames, lists)
        torch.autograd.backward(list(outs), [torch.stack([c[i] for c in cots]).to(DEV) for i in range(4)])
        torch.cuda.synchronize()
        return [(tuple(o[c].detach().cpu() for o in outs), _grads(m2d, lv[c], c)) for c in range(len(frames))]
    finally:
        _ops.set_deterministic(prev[0])
        _ops.KEEP_MASKS = prev[1]


# ---- one frame, one instantiation, against the oracle -------------------------------------------------------------------------


def _cot_generic(s, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(s["H"], s["W"], D, generator=g) * 2 - 1, torch.rand(s["H"], s["W"], generator=g) * 2 - 1


def _cot_fused(s, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.rand(s["H"], s["W"], c, generator=g) * 2 - 1 for c in (3, 1, 3, 1))


@functools.lru_cache(maxsize=None)
def _oracle_generic(key, D, split, seed=1):
    """(render, alphas, cotangents, fp32 gradients, A, S, fp64 gradients) of a cached frame."""
    from oracle import oracle as orc

    s, offs, fid, _ = _frame(*key)
    cols, bg = s["colors8"][:, :D], s["background8"][:D]
    r, a, last = _ofwd(orc, s, offs, fid, cols, bg)
    v_r, v_a = _cot_generic(s, D, seed)
    g, A, S = _obwd(orc, s, offs, fid, cols, bg, a, last, v_r, v_a, split)
    _r64, a64, last64 = _ofwd(orc, s, offs, fid, cols, bg, torch.float64)
    g64, _, _ = _obwd(orc, s, offs, fid, cols, bg, a64, last64, v_r, v_a, split, torch.float64)
    return r, a, (v_r, v_a), g, A, S, g64


def _dn_epilogue(R, A, bg_rgb):
    """dn_model.py:526-537, 577-578 on the raw composite (rgb | expected-depth accumulation | normals over ones) and its alpha."""
    rgb = torch.clamp(R[..., :3] + (1 - A)[..., None] * bg_rgb.to(R.dtype), 0.0, 1.0)
    ed = R[..., 3] / A.clamp_min(1e-10)
    depth = torch.where(A > 0, ed, ed.detach().max())[..., None]
    n = R[..., 4:7]
    return rgb, depth, (n / n.norm(dim=-1, keepdim=True) + 1) / 2, A[..., None]


def _oracle_fused_frame(orc, s, offs, fid, cot, bg_rgb):
    cols = s["colors8"][:, :7]
    out = {}
    for dt in (torch.float32, torch.float64):
        R, A, last = _ofwd(orc, s, offs, fid, cols, BG7, dt)
        Rl, Al = R.clone().requires_grad_(True), A.clone().requires_grad_(True)
        imgs = _dn_epilogue(Rl, Al, bg_rgb)
        torch.autograd.backward(list(imgs), [c.to(dt) for c in cot])
        g, A_, S_ = _obwd(orc, s, offs, fid, cols, BG7, A, last, Rl.grad, Al.grad, 4, dt)
        out[dt] = (tuple(i.detach() for i in imgs), g, A_, S_)
    imgs, g, A_, S_ = out[torch.float32]
    return imgs, g, A_, S_, out[torch.float64][1]


@functools.lru_cache(maxsize=None)
def _oracle_fused(key, seed=2):
    from oracle import oracle as orc

    s, offs, fid, _ = _frame(*key)
    cot = _cot_fused(s, seed)
    return (cot,) + _oracle_fused_frame(orc, s, offs, fid, cot, s["background8"][:3])


def _check_images(got, ref, what, names):
    every = torch.ones(ref[0].shape[0], ref[0].shape[1], dtype=torch.bool)     # one row per pixel (no borderline pixels here)
    for gi, oi, nm in zip(got, ref, names):
        assert_close(gi, oi, f"{what} {nm}")
        check_pixels(gi, oi, f"{what} {nm} per pixel", keep=every, enforce=True)


def _generic_case(key, D, split, det, what):
    s, offs, fid, _ = _frame(*key)
    r_o, a_o, cot, g, A, S, g64 = _oracle_generic(key, D, split)
    (r, a, hip), = _hip_generic([s], [(offs, fid)], D, split, [cot], det)
    name = f"{what}, D = {D}, xy_split = {split} ({'SPLIT = D' if split == D else 'SPLIT = 4' if (D, split) == (7, 4) else 'SPLIT = -1'}), " \
           f"{'deterministic' if det else 'default'} mode"
    _check_images((r, a), (r_o, a_o), name, ("render", "alpha"))
    _check_grads(hip, g, A, S, s, name, det)
    _fp64_note(hip, g64, name)
    return r, a, hip


def _fused_case(key, det, masks, sat, what):
    s, offs, fid, _ = _frame(*key)
    cot, imgs_o, g, A, S, g64 = _oracle_fused(key)
    (imgs, hip), = _hip_fused([s], [(offs, fid)], [cot], det, masks, sat)
    name = f"{what}, fused DN kernel, keep masks {'on' if masks else 'off'}, saturation flag {sat}" \
           f"{' (ignored: clamping loop)' if det else ' (clamp-free twin)' if sat == 0 else ' (clamping loop)'}, " \
           f"{'deterministic' if det else 'default'} mode"
    _check_images(imgs, imgs_o, name, ("rgb", "depth", "normal", "accumulation"))
    _check_grads(hip, g, A, S, s, name, det, epilogue=True)
    _fp64_note(hip, g64, name)
    return imgs, hip


# ---- the tests --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("D", [1, 2, 3, 4, 7, 8])
def test_generic_kernels_at_every_list_edge(orc, D):
    """Every count x stop pattern (124 half tiles) through the generic kernels with SPLIT = D, both modes, against the oracle."""
    s, offs, fid, model = _frame("main")
    _print_regimes(s, model, f"main frame, SPLIT = D = {D}")
    folds = {r["fold"] for r in model if r["queue"] > 0}
    assert folds == {1, 2, 4}, folds
    print(f"[raster] main frame: last buckets fold {sorted(folds)} in the default mode (1 in the deterministic mode); queue carries up "
          f"to {max(max(r['carries_scan'] or [0]) for r in model)} entries")
    for det in MODES:
        _generic_case(("main",), D, D, det, "main frame")


@pytest.mark.parametrize("D,split", [(5, 2), (8, 0), (7, 4)])
def test_generic_kernels_with_a_channel_split(orc, D, split):
    """xy_split != D: channels [split, D) feed neither v_alphas nor the screen-space gradient (SPLIT = -1; (7, 4): its own kernel)."""
    s, _, _, model = _frame("main")
    _print_regimes(s, model, f"main frame, D = {D}, xy_split = {split}")
    for det in MODES:
        _generic_case(("main",), D, split, det, "main frame")


@pytest.mark.parametrize("D", [4, 7])
def test_culled_entries_and_list_offsets_change_nothing(orc, D):
    """The same contributing entries with culled entries interleaved, and with every case list starting at another range_start % 64
    (0 / 1 / 63): images and gradients bit-equal to the plain frame, in both modes."""
    variants = [("main", True, 0), ("main", False, 1), ("main", True, 2)]
    for key in variants:
        s, _, _, model = _frame(*key)
        _print_regimes(s, model, f"main frame, interleave {key[1]}, phase {key[2]}, D = {D}")
    s0, offs0, fid0, _ = _frame("main")
    n = s0["n_case"]
    for det in MODES:
        cot = _cot_generic(s0, D, 3)
        bg = s0["background8"][:D]
        (r0, a0, g0), = _hip_generic([s0], [(offs0, fid0)], D, D, [cot], det, bg=bg)
        for key in variants:
            s, offs, fid, _ = _frame(*key)
            (r, a, g), = _hip_generic([s], [(offs, fid)], D, D, [cot], det, bg=bg)
            what = f"D = {D}, {'deterministic' if det else 'default'} mode, interleave {key[1]}, phase {key[2]} vs the plain frame"
            _same(r, r0, what + ": render")
            _same(a, a0, what + ": alpha")
            for k in GRAD_KEYS:
                _same(g[k][:n], g0[k][:n], f"{what}: grad {k}")
                assert not bool(g[k][n:].ne(0).any()), f"{what}: a culled entry received a gradient"


def test_each_channel_equals_its_one_channel_render(orc):
    """Channel k of a 4-channel render against the 1-channel render of channel k: images and v_colors[:, k] within COND_C of the
    oracle's row bound of that column."""
    s, offs, fid, _ = _frame("main")
    _r, _a, (v_r, v_a), _g, A, S, _ = _oracle_generic(("main",), 4, 4)
    visible = s["radii"] > 0
    for det in MODES:
        (r4, a4, g4), = _hip_generic([s], [(offs, fid)], 4, 4, [(v_r, v_a)], det)
        for k in (0, 3):
            (r1, a1, g1), = _hip_generic([s], [(offs, fid)], 1, 1, [(v_r[..., k:k + 1].contiguous(), v_a)], det,
                                         cols=s["colors8"][:, k:k + 1], bg=s["background8"][k:k + 1])
            what = f"channel {k} of D = 4 vs D = 1, {'deterministic' if det else 'default'} mode"
            _same(r1[..., 0], r4[..., k], what + ": render", exact=False)
            assert_close(r1[..., 0], r4[..., k], what + ": render")
            _same(a1, a4, what + ": alpha", exact=False)
            assert_close(a1, a4, what + ": alpha")
            _same(g1["colors"][:, 0], g4["colors"][:, k], what + ": v_colors", exact=False)
            check_rows_conditioned(g1["colors"][:, 0], g4["colors"][:, k], A["colors"][:, k], S["colors"][:, k], visible,
                                   what + ": v_colors", strict=True)


def test_fused_kernel_keep_masks_saturation_twins_and_modes(orc):
    """The fused DN kernel on the main frame: keep masks on / off x saturation flag 0 / 1 x both modes against the oracle (the dn
    epilogue differentiated in torch on the oracle's raw composite), and against each other."""
    s, _, _, model = _frame("main")
    _print_regimes(s, model, "main frame, fused DN kernel")
    _c, _i, _g, A, S, _ = _oracle_fused(("main",))
    visible = s["radii"] > 0
    runs = {}
    for masks in (True, False):
        for det in MODES:
            for sat in ((1,) if det else (0, 1)):
                runs[(masks, det, sat)] = _fused_case(("main",), det, masks, sat, "main frame")
    for det in MODES:
        for sat in ((1,) if det else (0, 1)):
            (i1, g1), (i0, g0) = runs[(True, det, sat)], runs[(False, det, sat)]
            what = f"keep masks on vs off, {'deterministic' if det else 'default'} mode, saturation flag {sat}"
            for a, b, nm in zip(i1, i0, ("rgb", "depth", "normal", "accumulation")):
                _same(a, b, f"{what}: {nm}")
            for k in GRAD_KEYS:
                _same(g1[k], g0[k], f"{what}: grad {k}", exact=False)
                check_rows_conditioned(g1[k], g0[k], A[k], S[k], visible, f"{what}: grad {k}", strict=True)
    for masks in (True, False):
        (i1, g1), (i0, g0) = runs[(masks, False, 1)], runs[(masks, False, 0)]
        what = f"clamping loop vs clamp-free twin, keep masks {'on' if masks else 'off'}, default mode"
        for a, b, nm in zip(i1, i0, ("rgb", "depth", "normal", "accumulation")):
            _same(a, b, f"{what}: {nm}")
        for k in GRAD_KEYS:
            _same(g1[k], g0[k], f"{what}: grad {k}", exact=False)
            check_rows_conditioned(g1[k], g0[k], A[k], S[k], visible, f"{what}: grad {k}", strict=True)


def test_fused_kernel_culled_entries_and_list_offsets_change_nothing(orc):
    """The fused kernel reads its keep masks at (range_start >> 6) + list + batch: interleaved culled entries and other list offsets
    must leave images and gradients bit-equal, with masks on and off, in both modes."""
    s0, offs0, fid0, _ = _frame("main")
    n = s0["n_case"]
    cot = _cot_fused(s0, 4)
    for masks in (True, False):
        for det in MODES:
            (i0, g0), = _hip_fused([s0], [(offs0, fid0)], [cot], det, masks)
            for key in [("main", True, 0), ("main", False, 1), ("main", True, 2)]:
                s, offs, fid, _ = _frame(*key)
                (i, g), = _hip_fused([s], [(offs, fid)], [cot], det, masks, bg_rgb=s0["background8"][:3])
                what = f"fused, keep masks {'on' if masks else 'off'}, {'deterministic' if det else 'default'} mode, interleave {key[1]}, " \
                       f"phase {key[2]} vs the plain frame"
                for a, b, nm in zip(i, i0, ("rgb", "depth", "normal", "accumulation")):
                    _same(a, b, f"{what}: {nm}")
                for k in GRAD_KEYS:
                    _same(g[k][:n], g0[k][:n], f"{what}: grad {k}")
                    assert not bool(g[k][n:].ne(0).any()), f"{what}: a culled entry received a gradient"


def test_fused_kernel_with_capped_alphas(orc):
    """Opacities above 0.999 (alpha clamped, no gradient through it): the saturation flag is 1, the clamping loop runs."""
    s, _, _, model = _frame("cap")
    _print_regimes(s, model, "capped alphas, fused DN kernel")
    assert bool((s["opacities"] > 0.999).any())
    for masks in (True, False):
        for det in MODES:
            _fused_case(("cap",), det, masks, 1, "capped alphas")
    for det in MODES:
        _generic_case(("cap",), 4, 4, det, "capped alphas")


@pytest.mark.parametrize("name", ["height40", "height44", "deep"])
def test_partial_tiles_and_a_deep_list(orc, name):
    """Bottom half tiles outside the image (H = 40) or half inside it (H = 44); one list of 20 000 low-alpha entries."""
    s, _, _, model = _frame(name)
    _print_regimes(s, model, f"{name} frame")
    for det in MODES:
        _generic_case((name,), 4, 4, det, f"{name} frame")
        _generic_case((name,), 5, 2, det, f"{name} frame")
        _fused_case((name,), det, True, 0 if not det else 1, f"{name} frame")


@pytest.mark.parametrize("kernel", ["generic", "fused"])
def test_camera_batch_equals_its_single_camera_calls(orc, kernel):
    """Three cameras with different recipes in one launch (lists and keep masks at non-zero camera offsets; every camera's lists end
    on a multiple of 64, so the last list of the batch ends on a mask-word boundary): bit-equal to the three single-camera calls, in
    both modes; each camera against the oracle."""
    frames = edge_cameras()
    lists, models = [], []
    for c, s in enumerate(frames):
        offs, fid = edge_lists(orc, s)
        lists.append((offs, fid))
        model = edge_model(s, offs, fid)
        _print_regimes(s, model, f"camera {c} of 3, {kernel} kernel")
    assert sum(l[1].numel() for l in lists) % 64 == 0
    bg = frames[0]["background8"]
    if kernel == "generic":
        cots = [_cot_generic(s, 4, 10 + c) for c, s in enumerate(frames)]
    else:
        cots = [_cot_fused(s, 10 + c) for c, s in enumerate(frames)]
    for det in MODES:
        mode = "deterministic" if det else "default"
        if kernel == "generic":
            batch = _hip_generic(frames, lists, 4, 4, cots, det, bg=bg[:4])
        else:
            batch = _hip_fused(frames, lists, cots, det, True, 0 if not det else 1, bg_rgb=bg[:3])
        for c, s in enumerate(frames):
            if kernel == "generic":
                (r, a, g), = _hip_generic([s], [lists[c]], 4, 4, [cots[c]], det, bg=bg[:4])
                imgs, imgs_b, gb = (r, a), batch[c][:2], batch[c][2]
            else:
                (imgs, g), = _hip_fused([s], [lists[c]], [cots[c]], det, True, 0 if not det else 1, bg_rgb=bg[:3])
                imgs_b, gb = batch[c]
            what = f"C = 3 batch, {kernel} kernel, {mode} mode, camera {c}"
            for x, y in zip(imgs_b, imgs):
                _same(x, y, what + ": image")
            for k in GRAD_KEYS:
                _same(gb[k], g[k], f"{what}: grad {k}")
            # and the camera against the oracle
            offs, fid = lists[c]
            if kernel == "generic":
                cols = s["colors8"][:, :4]
                r_o, a_o, last = _ofwd(orc, s, offs, fid, cols, bg[:4])
                go, A, S = _obwd(orc, s, offs, fid, cols, bg[:4], a_o, last, cots[c][0], cots[c][1], 4)
                _check_images(imgs_b, (r_o, a_o), what, ("render", "alpha"))
            else:
                imgs_o, go, A, S, _ = _oracle_fused_frame(orc, s, offs, fid, cots[c], bg[:3])
                _check_images(imgs_b, imgs_o, what, ("rgb", "depth", "normal", "accumulation"))
            _check_grads(gb, go, A, S, s, what, det, epilogue=kernel == "fused")
