"""Tile binning (csrc/binning.hip) at the edges of its code paths, against the CPU oracle's gsplat binning (isect_tiles + the stable
64-bit LSD sort of orc_sort_isects) or, where the oracle's compositing would be too slow at full size, against identities the GPU
path must keep exactly.

The binning picks its route from the frame: uint16 tile keys and two LSD tile passes up to 65536 tiles (of the whole camera batch),
uint32 keys and three passes beyond; the fp32-reciprocal row division of the pair generator only with <= 256 tile columns and
<= 65536 tiles (g.exact); the `all` term of the range histogram when a box row spans >= 2^dbits tiles of the first pass's digit;
capped scan segments (8 segments of more than 2048 chunk counters) beyond 2^26 pairs; chunks of 4096 pairs that belong to a
single Gaussian; 4096-key depth-sort chunks from 2^22 Gaussians on; 1 to 4 radix passes of the deterministic gradient reduction; one
tile pass that is first and last at once, at every digit width, up to 256 tiles.
Every test asserts that its frame reached the regime it is about and prints the figures ("[binning] ..." lines).

Scenes are given in camera space (camera at the origin looking down +z, viewmat = identity): a Gaussian is placed by its pixel
centre, depth and pixel-space sigmas, so tile coverage and depth ties are exact by construction."""
import math

import pytest
import torch

from _scenes import (FP32_ENVELOPE, assert_binning_properties, assert_close, assert_equal_int, cotangents, gsplat_inputs,
                     oracle_threads, to_leaf)
from test_gpu_parity import _call_both, _check_backward, _check_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT_KEYS = ("rgb", "depth", "normal", "accumulation")
KW_CALL = dict(sh_degree=3, render_mode="RGB+ED", absgrad=True)     # test_gpu_parity._call_both adds packed=False itself
KW = dict(KW_CALL, packed=False)


# ------------------------------------------------------------------------------------------------
# scenes

def _camera(W, H, f):
    """nerfstudio camera whose viewmat is exactly the identity (c2w rotation diag(1, -1, -1), no translation)."""
    from dn_splatter_amd.model import Camera

    c2w = torch.zeros(1, 3, 4)
    c2w[0, 0, 0], c2w[0, 1, 1], c2w[0, 2, 2] = 1.0, -1.0, -1.0
    return Camera(c2w, f, f, W / 2.0, H / 2.0, W, H)


def _scene(u, v, z, sx, sy, opa, W, H, f, seed=0):
    """Gaussians at pixel centre (u, v), camera-space depth z (< 0: behind the camera, culled) and pixel sigmas (sx, sy), identity
    rotations.  -> (activated inputs of rasterization(), raw parameters of DNSplatterRenderer, viewmat [1,4,4], K [1,3,3], camera)"""
    import dn_splatter_amd as dns

    N = u.numel()
    g = torch.Generator().manual_seed(seed)
    za = z.abs()
    means = torch.stack([(u - W / 2.0) * z / f, (v - H / 2.0) * z / f, z], -1).float().contiguous()
    scales = torch.stack([sx * za / f, sy * za / f, 1e-4 * za], -1).float()
    quats = torch.zeros(N, 3 + 1)
    quats[:, 0] = 1.0
    dc = torch.rand(N, 3, generator=g)
    rest = torch.randn(N, 15, 3, generator=g) * 0.1
    opa = opa.float().clamp(1e-3, 0.999)
    inp = dict(means=means, quats=quats, scales=scales, opacities=opa.clone(), colors=torch.cat([dc[:, None], rest], 1).contiguous())
    gp = dict(means=means.clone(), scales=scales.log(), quats=quats.clone(), features_dc=dc, features_rest=rest,
              opacities=torch.logit(opa)[:, None].contiguous())
    cam = _camera(W, H, f)
    viewmat = dns.get_viewmat(cam.camera_to_worlds)
    assert torch.equal(viewmat[0], torch.eye(4)), viewmat
    return inp, gp, viewmat, cam.get_intrinsics_matrices(), cam


def _clutter(N, W, H, seed, smin=1.0, smax=40.0, zmin=2.0, zmax=10.0, aniso=3.0, omin=0.05, omax=0.9, margin=0.05):
    """N Gaussians spread over (and a little beyond) the frame: log-uniform pixel sigmas, random aspect, random depth / opacity."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(N, generator=g)
    u = (r() * (1 + 2 * margin) - margin) * W
    v = (r() * (1 + 2 * margin) - margin) * H
    z = zmin + r() * (zmax - zmin)
    s = torch.exp(math.log(smin) + r() * (math.log(smax) - math.log(smin)))
    a = torch.exp((r() * 2 - 1) * math.log(aniso))
    return u, v, z, s * a.sqrt(), s / a.sqrt(), omin + r() * (omax - omin)


def _cat(*parts):
    return tuple(torch.cat([p[i].float() for p in parts]) for i in range(6))


def _big(W, H, seed, n_clutter, extra):
    """Clutter plus ``extra`` = list of (u, v, z, sx, sy, opa) tuples of tensors (wide / huge splats)."""
    return _cat(_clutter(n_clutter, W, H, seed), *extra)


def _full(n, u, v, z, sx, sy, opa):
    t = lambda x: torch.full((n,), float(x)) if not torch.is_tensor(x) else x.float()
    return (t(u), t(v), t(z), t(sx), t(sy), t(opa))


# ------------------------------------------------------------------------------------------------
# regime figures

def _tile_bits(T):
    bits = 1
    while (1 << bits) < T:
        bits += 1
    return bits


def _regime(info, what, C=1):
    """The route binning.hip takes for this frame (restated from emit_and_sort / dnsplat_bin_emit_sort / scan_segments), printed."""
    tw, th = int(info["tile_width"]), int(info["tile_height"])
    T = tw * th * C
    bits = _tile_bits(T)
    passes = (bits + 7) // 8
    dbits, shift = [], 0
    for p in range(passes):
        d = (bits - shift + (passes - p) - 1) // (passes - p)
        dbits.append(d)
        shift += d
    n = int(info["n_isects"])
    cap = int(info["_binning"].flatten_ids.numel())
    nb = max(1, -(-cap // 4096))
    segs = min(8, max(1, -(-nb // 2048)))
    seg_len = -(-nb // segs)
    radii = info["radii"].reshape(C, -1)
    m2 = info["means2d"].detach().reshape(C, -1, 2)
    r = radii.float()
    vis = radii > 0
    x0 = torch.floor((m2[..., 0] - r) / 16).clamp(0, tw)
    x1 = torch.ceil((m2[..., 0] + r) / 16).clamp(0, tw)
    row = int(torch.where(vis, x1 - x0, torch.zeros_like(x0)).max()) if bool(vis.any()) else 0
    tpg = int(info["tiles_per_gauss"].max())
    fig = dict(tiles=T, tw=tw, th=th, bits=bits, passes=passes, dbits=dbits, key=16 if T <= 0x10000 else 32,
               exact=tw <= 256 and T <= 65536, pairs=n, cap=cap, segs=segs, seg_len=seg_len, max_tiles=tpg, widest_row=row)
    print(f"[binning] {what}: {T} tiles ({tw} x {th} x {C} cameras), {bits} bits -> {passes} passes {dbits} on uint{fig['key']} keys, "
          f"row division {'fp32 reciprocal' if fig['exact'] else 'integer'}, {n} pairs (capacity {cap}: {segs} scan segments of "
          f"{seg_len} chunks), max {tpg} tiles per Gaussian, widest box row {row} tiles")
    return fig


# ------------------------------------------------------------------------------------------------
# comparisons

def _ints_against_oracle(orc, info, inp, viewmat, K, W, H, what):
    """Integer half of a single-camera rasterization() call against the oracle's projection + isect_tiles + sort, bit for bit."""
    from dn_splatter_amd import _ops

    assert _ops.binning_status(info["_binning"], info["radii"].numel()) == 0, what + ": binning status word"
    with torch.no_grad():
        radii, means2d, depths, conics, _c, tiles = orc.project_fwd(inp["means"], inp["quats"], inp["scales"], viewmat[0], K[0], W, H)
        tw, th = math.ceil(W / 16), math.ceil(H / 16)
        _t, isect_ids, flatten_ids = orc.isect_tiles(means2d, radii, depths, 16, tw, th)
        offsets = orc.isect_offset_encode(isect_ids, tw, th)
    assert_equal_int(info["radii"][0], radii, what + " radii")
    assert_equal_int(info["tiles_per_gauss"][0], tiles, what + " tiles_per_gauss")
    assert info["n_isects"] == flatten_ids.shape[0], (what, info["n_isects"], flatten_ids.shape[0])
    assert_equal_int(info["flatten_ids"], flatten_ids, what + " flatten_ids")
    assert_equal_int(info["isect_offsets"][0], offsets, what + " isect_offsets")
    assert_equal_int(info["isect_ids"], isect_ids, what + " isect_ids")
    return int(flatten_ids.shape[0])


def _dropin_ints(dns, orc, inp, viewmat, K, W, H, what):
    """rasterization() (gsplat boxes) forward at full size, integers against the oracle; returns the regime figures."""
    gi = {k: v.to(DEV) for k, v in inp.items()}
    with torch.no_grad():
        _r, _a, info = dns.rasterization(**gi, viewmats=viewmat.to(DEV), Ks=K.to(DEV), width=W, height=H, **KW)
        torch.cuda.synchronize()
        fig = _regime(info, what + ", rasterization()")
        _ints_against_oracle(orc, info, inp, viewmat, K, W, H, what)
    del _r, _a, info, gi
    torch.cuda.empty_cache()
    return fig


def _fused_tight_vs_gsplat(dns, gp, cam, what):
    """The fused pass (DNSplatterRenderer(fused=True)) with gsplat's tile boxes and with the tight ones: both lists keep the binning
    properties (_scenes.assert_binning_properties), and the images are equal bit for bit (the pairs the tight boxes leave out are
    skipped at every pixel anyway; the others are blended in the same order).  Returns the regime figures of both runs."""
    from dn_splatter_amd import _ops

    old = _ops.TIGHT_TILES
    outs, figs = {}, {}
    params = {k: v.to(DEV).requires_grad_(True) for k, v in gp.items()}
    params["normals"] = torch.zeros(params["means"].shape[0], 3, device=DEV)
    try:
        for tight in (False, True):
            _ops.TIGHT_TILES = tight
            m = dns.DNSplatterRenderer(params, fused=True)
            with torch.no_grad():
                out = m.get_outputs(cam.to(DEV))
            torch.cuda.synchronize()
            assert bool(m.last_info.get("tight_tiles")) == tight
            figs[tight] = _regime(m.last_info, f"{what}, fused pass, {'tight' if tight else 'gsplat'} boxes")
            if tight:
                # every frame this helper sees has 1024 tiles or more: the tight run keeps its lists per 2x2 cell, and the route of ITS
                # tile sort is picked from the cell grid
                info = m.last_info
                cw, ch = info["cell_shape"]
                lw, lh = -(-int(info["tile_width"]) // cw), -(-int(info["tile_height"]) // ch)
                bits = _tile_bits(lw * lh)
                print(f"[binning] {what}, fused pass, tight boxes: lists per {cw}x{ch} cell: {lw * lh} cells ({lw} x {lh}), {bits} bits -> "
                      f"{(bits + 7) // 8} passes on uint{16 if lw * lh <= 0x10000 else 32} keys, row division "
                      f"{'fp32 reciprocal' if lw <= 256 and lw * lh <= 65536 else 'integer'}, {int(info['n_cell_pairs'])} cell pairs for "
                      f"{int(info['n_isects'])} tile pairs")
                assert (cw, ch) == (2, 2) and 0 < int(info["n_cell_pairs"]) < int(info["n_isects"]), "the tight run did not take list cells"
            assert_binning_properties(m.last_info)
            outs[tight] = {k: out[k].detach().clone() for k in OUT_KEYS}
            del m, out
    finally:
        _ops.TIGHT_TILES = old
    for k in OUT_KEYS:
        assert torch.equal(outs[False][k], outs[True][k]), f"{what}: {k} differs between tight and gsplat tile boxes"
    assert figs[True]["pairs"] < figs[False]["pairs"]
    del outs, params
    torch.cuda.empty_cache()
    return figs


# ------------------------------------------------------------------------------------------------
# 1. wide strip: 480 tiles, 9 bits -> 5 + 4, box rows longer than 2^5 tiles (the `all` term of the range histogram)

def test_wide_strip_rows_longer_than_the_first_digit(dns, orc):
    W, H, f = 1920, 64, 400.0
    oracle_threads()
    wide = _clutter(300, W, H, seed=2, smin=90.0, smax=300.0, aniso=4.0, omin=0.05, omax=0.5)
    inp, _gp, viewmat, K, _cam = _scene(*_cat(_clutter(3000, W, H, seed=1, smax=20.0), wide), W, H, f, seed=1)
    o, g = _call_both(dns, orc, inp, viewmat, K, W, H, **KW_CALL)
    fig = _regime(g[2], "1920x64 strip")
    assert fig["tiles"] == 480 and fig["passes"] == 2 and fig["dbits"] == [5, 4] and fig["key"] == 16 and fig["exact"]
    assert fig["widest_row"] > 32
    _check_forward(o, g, what="1920x64 strip")
    _check_backward(o, g, what="1920x64 strip")


# ------------------------------------------------------------------------------------------------
# 2.-5. large frames: integers against the oracle through rasterization(), images through the tight / gsplat identity

def _corner(W, H):
    """One small splat on the last tile of the frame (tile id T - 1) and one full-width / full-height splat."""
    return [_full(1, W - 8, H - 8, 3.0, 2.0, 2.0, 0.8), _full(1, W / 2, H / 2, 30.0, W / 2.6, W / 2.6, 0.05)]


@pytest.mark.parametrize("W,H,case", [(4096, 4096, "65536 tiles"), (4112, 2048, "257 columns"), (4096, 4112, "65792 tiles"),
                                      (6000, 4000, "93750 tiles")])
def test_large_frames_match_oracle_and_tight_boxes_keep_the_images(dns, orc, W, H, case):
    oracle_threads()
    f = 0.5 * W
    g_ = torch.Generator().manual_seed(W + H)
    n_huge = 4
    huge = _full(n_huge, torch.rand(n_huge, generator=g_) * W, torch.rand(n_huge, generator=g_) * H, 20.0, 420.0, 400.0, 0.1)
    wide = _clutter(200, W, H, seed=W, smin=150.0, smax=700.0, aniso=8.0, omin=0.05, omax=0.4)
    inp, gp, viewmat, K, cam = _scene(*_big(W, H, W * 7 + H, 150_000, _corner(W, H) + [huge, wide]), W, H, f, seed=H)
    fig = _dropin_ints(dns, orc, inp, viewmat, K, W, H, f"{W}x{H}")
    T = fig["tiles"]
    assert fig["widest_row"] >= 1 << fig["dbits"][0], "no box row reaches the `all` term of the range histogram"
    if (W, H) == (4096, 4096):
        assert T == 65536 and fig["tw"] == 256 and fig["key"] == 16 and fig["exact"] and fig["dbits"] == [8, 8]
        assert fig["widest_row"] == 256
    elif (W, H) == (4112, 2048):
        assert T == 32896 and fig["tw"] == 257 and fig["key"] == 16 and not fig["exact"] and fig["passes"] == 2
    elif (W, H) == (4096, 4112):
        assert T == 65792 and fig["key"] == 32 and not fig["exact"] and fig["dbits"] == [6, 6, 5]
    else:
        assert T == 93750 and fig["tw"] == 375 and fig["key"] == 32 and fig["passes"] == 3 and fig["widest_row"] > 64
        assert fig["max_tiles"] > 16384
    figs = _fused_tight_vs_gsplat(dns, gp, cam, f"{W}x{H}")
    assert figs[False]["tiles"] == T


def test_large_frame_last_tile_is_binned(dns, orc):
    """4096 x 4096: the uint16 keys carry tile id 65535 (the corner splat's only tile) and the offsets place it."""
    W = H = 4096
    inp, _gp, viewmat, K, _cam = _scene(*_cat(*_corner(W, H)), W, H, 0.5 * W, seed=3)
    gi = {k: v.to(DEV) for k, v in inp.items()}
    with torch.no_grad():
        _r, _a, info = dns.rasterization(**gi, viewmats=viewmat.to(DEV), Ks=K.to(DEV), width=W, height=H, **KW)
    fig = _regime(info, "4096x4096 corner")
    assert fig["tiles"] == 65536
    n = _ints_against_oracle(orc, info, inp, viewmat, K, W, H, "4096x4096 corner")
    offs = info["isect_offsets"].reshape(-1)
    assert 0 in info["flatten_ids"][int(offs[-1]):n].tolist(), "tile 65535 holds the corner splat"
    assert float(_r[0, -8, -8, :3].abs().sum()) > 0.0


# ------------------------------------------------------------------------------------------------
# 6. nine 1080p cameras: 73 440 stacked tiles (uint32 keys), eight (65 280, uint16) as the control

@pytest.mark.parametrize("C", [8, 9])
@pytest.mark.usefixtures("hip_deterministic")
def test_camera_batch_across_the_key_width_edge(dns, orc, C):
    from dn_splatter_amd import synthetic

    oracle_threads()
    N, W, H = 60_000, 1920, 1080
    inp, _vm, K, _ = gsplat_inputs(N, W, H, focal=1200.0, seed=17, anisotropic=True)
    cams = [synthetic.orbit_camera(v, n_views=C, width=W, height=H, focal=1200.0) for v in range(C)]
    vms = torch.cat([dns.get_viewmat(c.camera_to_worlds) for c in cams])
    Ks = K.expand(C, 3, 3).contiguous()
    gi = to_leaf(inp, DEV)
    r_b, a_b, info_b = dns.rasterization(**gi, viewmats=vms.to(DEV), Ks=Ks.to(DEV), width=W, height=H, **KW)
    fig = _regime(info_b, f"{C} cameras at 1080p", C=C)
    assert fig["tiles"] == C * 8160
    if C == 9:
        assert fig["key"] == 32 and fig["passes"] == 3 and not fig["exact"]
    else:
        assert fig["key"] == 16 and fig["passes"] == 2 and fig["exact"]
    v_r, v_a = cotangents([r_b.shape, a_b.shape], 5)
    info_b["means2d"].retain_grad()
    ((r_b * v_r.to(DEV)).sum() + (a_b * v_a.to(DEV)).sum()).backward()
    # C single-camera calls
    gs = to_leaf(inp, DEV)
    base = 0
    for c in range(C):
        r, a, info = dns.rasterization(**gs, viewmats=vms[c:c + 1].to(DEV), Ks=Ks[c:c + 1].to(DEV), width=W, height=H, **KW)
        assert torch.equal(r[0], r_b[c]) and torch.equal(a[0], a_b[c]), f"camera {c}: batched image differs"
        for k in ("radii", "means2d", "depths", "conics", "tiles_per_gauss"):
            assert torch.equal(info[k][0], info_b[k][c]), (c, k)
        n = info["n_isects"]
        assert torch.equal(info["flatten_ids"] + c * N, info_b["flatten_ids"][base:base + n]), f"camera {c}: tile lists"
        assert torch.equal(info["isect_offsets"][0] + base, info_b["isect_offsets"][c])
        base += n
        info["means2d"].retain_grad()
        ((r * v_r[c:c + 1].to(DEV)).sum() + (a * v_a[c:c + 1].to(DEV)).sum()).backward()
        assert_close(info_b["means2d"].grad[c], info["means2d"].grad[0], f"camera {c} means2d.grad", 1e-5)
        del r, a, info
    assert base == info_b["n_isects"]
    for k in gi:
        assert_close(gi[k].grad, gs[k].grad, "batched grad " + k, 1e-5)
    # the oracle's batch, integers only (its compositing of nine 1080p frames is not needed for the lists): per camera, keys with
    # the camera bits of gsplat's layout
    tb = int(math.floor(math.log2(8160))) + 1
    flat, ids, offs, radii, tiles, base = [], [], [], [], [], 0
    with torch.no_grad():
        for c in range(C):
            rad, m2, dep, _con, _cmp, t = orc.project_fwd(inp["means"], inp["quats"], inp["scales"], vms[c], Ks[c], W, H)
            _t, iid, fid = orc.isect_tiles(m2, rad, dep, 16, 120, 68)
            offs.append(orc.isect_offset_encode(iid, 120, 68) + base)
            flat.append(fid + c * N)
            ids.append(iid | (c << (32 + tb)))
            radii.append(rad)
            tiles.append(t)
            base += fid.shape[0]
    assert_equal_int(info_b["radii"], torch.stack(radii), "batch radii")
    assert_equal_int(info_b["tiles_per_gauss"], torch.stack(tiles), "batch tiles_per_gauss")
    assert_equal_int(info_b["flatten_ids"], torch.cat(flat), "batch flatten_ids")
    assert_equal_int(info_b["isect_offsets"], torch.stack(offs), "batch isect_offsets")
    assert_equal_int(info_b["isect_ids"], torch.cat(ids), "batch isect_ids (camera bits)")
    del r_b, a_b, info_b, gi, gs
    torch.cuda.empty_cache()


@pytest.mark.parametrize("C", [8, 9])
def test_get_outputs_batch_across_the_key_width_edge(dns, C):
    from dn_splatter_amd import synthetic

    N, W, H = 60_000, 1920, 1080
    gp = synthetic.make_gauss_params(N, sh_rest_std=0.1, seed=23, device=DEV)
    m = dns.DNSplatterRenderer(gp, fused=True)
    cams = [synthetic.orbit_camera(v, n_views=C, width=W, height=H, focal=1200.0).to(DEV) for v in range(C)]
    with torch.no_grad():
        ref = [{k: v.clone() for k, v in m.get_outputs(c).items() if torch.is_tensor(v)} for c in cams]
        got = m.get_outputs_batch(cams, max_batch=C)
    torch.cuda.synchronize()
    assert m.last_info["n_cameras"] == C
    fig = _regime(m.last_info, f"get_outputs_batch, {C} cameras", C=C)
    assert fig["tiles"] == C * 8160 and fig["key"] == (32 if C == 9 else 16)
    assert len(got) == C
    for c, (a, b) in enumerate(zip(got, ref)):
        for k in ("rgb", "depth", "normal", "surface_normal", "accumulation"):
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (c, k)


# ------------------------------------------------------------------------------------------------
# 7. more than 2^26 pairs: capped scan segments (8 segments of more than 2048 chunk counters each)

def test_more_than_2_pow_26_pairs(dns, orc):
    oracle_threads()
    W, H, f = 3840, 2160, 1900.0
    inp, gp, viewmat, K, cam = _scene(*_clutter(200_000, W, H, seed=77, smin=25.0, smax=80.0, aniso=2.0, omin=0.3, omax=0.99),
                                      W, H, f, seed=77)
    fig = _dropin_ints(dns, orc, inp, viewmat, K, W, H, "4K, > 2^26 pairs")
    print(f"[binning] 4K frame: {fig['pairs']} pairs = {fig['pairs'] / 2 ** 26:.2f} x 2^26")
    assert fig["pairs"] > 2 ** 26 and fig["segs"] == 8 and fig["seg_len"] > 2048
    figs = _fused_tight_vs_gsplat(dns, gp, cam, "4K, > 2^26 pairs")
    assert figs[False]["pairs"] > 2 ** 26 and figs[False]["seg_len"] > 2048


# ------------------------------------------------------------------------------------------------
# 8. one Gaussian over the whole 1080p frame (8160 tiles: whole 4096-pair chunks belong to it), inside clutter

def test_whole_frame_floater(dns, orc):
    W, H, f = 1920, 1080, 1200.0
    oracle_threads()
    floater = _full(1, W / 2 + 3.3, H / 2 - 1.7, 1.5, 420.0, 380.0, 0.35)
    inp, _gp, viewmat, K, _cam = _scene(*_cat(_clutter(6000, W, H, seed=8, smax=30.0, zmin=2.0, zmax=8.0), floater, _clutter(2000, W, H, seed=9, zmin=0.5, zmax=1.2, smax=10.0)),
                                        W, H, f, seed=8)
    o, g = _call_both(dns, orc, inp, viewmat, K, W, H, **KW_CALL)
    fig = _regime(g[2], "1080p floater")
    assert fig["max_tiles"] == 8160 > 4096             # at least one whole 4096-pair chunk belongs to the floater
    _check_forward(o, g, what="1080p floater")
    _check_backward(o, g, what="1080p floater")


# ------------------------------------------------------------------------------------------------
# 9. pair counts on the 4096-pair chunk edges: one tile per splat, so I = number of visible splats

@pytest.mark.parametrize("I", [4095, 4096, 4097, 8192, 8193])
def test_pair_counts_on_chunk_edges(dns, orc, I):
    W, H, f = 256, 192, 300.0
    oracle_threads()
    g_ = torch.Generator().manual_seed(I)
    tx, ty = torch.randint(0, W // 16, (I,), generator=g_), torch.randint(0, H // 16, (I,), generator=g_)
    vis = _full(I, tx * 16 + 8.0, ty * 16 + 8.0, 2.0 + 6.0 * torch.rand(I, generator=g_), 1.2 + 0.3 * torch.rand(I, generator=g_),
                1.2 + 0.3 * torch.rand(I, generator=g_), 0.1 + 0.8 * torch.rand(I, generator=g_))
    n_cull = 777
    cull = _full(n_cull, torch.rand(n_cull, generator=g_) * W, torch.rand(n_cull, generator=g_) * H, -3.0, 2.0, 2.0, 0.5)
    allg = _cat(vis, cull)
    perm = torch.randperm(I + n_cull, generator=g_)
    inp, _gp, viewmat, K, _cam = _scene(*(x[perm] for x in allg), W, H, f, seed=I)
    o, g = _call_both(dns, orc, inp, viewmat, K, W, H, **KW_CALL)
    fig = _regime(g[2], f"{I} one-tile splats")
    assert fig["pairs"] == I and fig["max_tiles"] == 1
    assert int((g[2]["radii"] > 0).sum()) == I < I + n_cull
    _check_forward(o, g, what=f"I = {I}")
    _check_backward(o, g, what=f"I = {I}")


# ------------------------------------------------------------------------------------------------
# 10. Gaussian counts on the depth-sort edges (2048-key chunks; 4096-key chunks from 2^22 on), integers only

@pytest.mark.parametrize("N", [2047, 2048, 2049, (1 << 22) - 1, 1 << 22, (1 << 22) + 1])
def test_gaussian_counts_on_depth_sort_edges(dns, orc, N):
    W, H, f = 320, 240, 300.0
    oracle_threads()
    u, v, z, sx, sy, opa = _clutter(N, W, H, seed=N % 1000, smin=0.5, smax=6.0, margin=0.2)
    z = torch.where(torch.arange(N) % 5 == 3, -z, z)           # a fifth behind the camera: culled, never ranked
    inp, _gp, viewmat, K, _cam = _scene(u, v, z, sx, sy, opa, W, H, f, seed=N % 1000)
    fig = _dropin_ints(dns, orc, inp, viewmat, K, W, H, f"N = {N}")
    assert fig["pairs"] > N // 2


# ------------------------------------------------------------------------------------------------
# 11. exact depth ties: a plane of > 4096 splats at one camera-space depth (identity rotation: every depth rounds the same)

def test_exact_depth_ties_across_sort_chunks(dns, orc):
    W, H, f = 256, 256, 256.0
    oracle_threads()
    n_plane = 6000
    plane = _clutter(n_plane, W, H, seed=11, smin=3.0, smax=25.0, omin=0.05, omax=0.5)
    plane = plane[:2] + (torch.full((n_plane,), 4.0),) + plane[3:]
    inp, _gp, viewmat, K, _cam = _scene(*_cat(_clutter(1500, W, H, seed=12, zmin=3.0, zmax=5.0), plane), W, H, f, seed=11)
    o, g = _call_both(dns, orc, inp, viewmat, K, W, H, **KW_CALL)
    info = g[2]
    fig = _regime(info, "depth ties")
    dep = info["depths"][0]
    tied = (dep == 4.0) & (info["radii"][0] > 0)
    assert int(tied.sum()) > 4096
    fid = info["flatten_ids"].long()
    n_tied_pairs = int(tied[fid].sum())
    print(f"[binning] depth ties: {int(tied.sum())} visible splats at depth 4.0, {n_tied_pairs} of {fig['pairs']} pairs")
    assert n_tied_pairs > 2 * 4096
    _check_forward(o, g, what="depth ties")          # flatten_ids bit for bit: ties in index order inside every tile list
    _check_backward(o, g, what="depth ties")


# ------------------------------------------------------------------------------------------------
# 12. deterministic reduction: 1, 2, 3 and 4 radix passes over the records (C x N records)

@pytest.fixture
def deterministic(dns, orc):
    """As test_gpu_determinism.py: the HIP path in its deterministic mode, the oracle's scatter accumulated in double."""
    from dn_splatter_amd import _ops

    prev = _ops.DETERMINISTIC["on"]
    prev_o = orc.set_exact_accumulation(True)
    dns.set_deterministic(True)
    yield
    dns.set_deterministic(prev)
    orc.set_exact_accumulation(prev_o)


def _det_case(dns, orc, monkeypatch, inp, viewmats, Ks, W, H, seed, what, sh_degree=3):
    """Two deterministic GPU runs (bit-equal gradients) and the oracle (within 1e-4 x scale + the fp64 envelope, as
    test_gpu_determinism.py).  Returns the record count the backward handed dnsplat_det_reduce."""
    from dn_splatter_amd import _ops

    records = []
    real = _ops._det_finish

    def spy(part, b, v_splats):
        if part is not None:
            records.append(int(v_splats.shape[0]))
        return real(part, b, v_splats)

    monkeypatch.setattr(_ops, "_det_finish", spy)
    kw = dict(KW, sh_degree=sh_degree)
    ci = to_leaf(inp, "cpu")
    r_o, a_o, info_o = orc.rasterization(**ci, viewmats=viewmats, Ks=Ks, width=W, height=H, **kw)
    keep = (~info_o["borderline"]).reshape(r_o.shape[:-1])[..., None]          # [C,H,W,1]: borderline pixels carry no cotangent
    v_r, v_a = cotangents([r_o.shape, a_o.shape], seed)
    v_r, v_a = v_r * keep, v_a * keep
    ((r_o * v_r).sum() + (a_o * v_a).sum()).backward()
    c64 = {k: v.detach().double().requires_grad_(True) for k, v in inp.items()}
    r_d, a_d, _ = orc.rasterization(**c64, viewmats=viewmats.double(), Ks=Ks.double(), width=W, height=H, **kw)
    ((r_d * v_r.double()).sum() + (a_d * v_a.double()).sum()).backward()
    runs = []
    for _ in range(2):
        gi = to_leaf(inp, DEV)
        r, a, info = dns.rasterization(**gi, viewmats=viewmats.to(DEV), Ks=Ks.to(DEV), width=W, height=H, **kw)
        info["means2d"].retain_grad()
        ((r * v_r.to(DEV)).sum() + (a * v_a.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        runs.append({k: gi[k].grad.detach().clone() for k in gi})
        n_isects = int(info["n_isects"])
        del r, a, info, gi
    assert len(records) == 2 and records[0] == records[1]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), f"{what}: gradient {k} differs between two deterministic runs"
    for k in ci:
        env = FP32_ENVELOPE * (ci[k].grad.double() - c64[k].grad).abs()
        assert_close(runs[0][k], ci[k].grad, f"{what} deterministic grad {k}", envelope=env)
    bits = _tile_bits(records[0])
    print(f"[binning] {what}: {records[0]} records -> {(bits + 7) // 8} reduction passes, {n_isects} pairs")
    return records[0], n_isects


@pytest.mark.parametrize("N", [1, 200, 256, 257, 65536, 65537])
def test_deterministic_reduction_pass_counts(dns, orc, deterministic, monkeypatch, N):
    W, H, f = 128, 96, 100.0
    oracle_threads()
    u, v, z, sx, sy, opa = _clutter(N, W, H, seed=N, smin=0.7, smax=12.0, zmin=1.0, zmax=6.0, margin=0.0)
    inp, _gp, viewmat, K, _cam = _scene(u, v, z, sx, sy, opa, W, H, f, seed=N)
    rec, n = _det_case(dns, orc, monkeypatch, inp, viewmat, K, W, H, seed=N % 97, what=f"N = {N}")
    assert rec == N and n > 0
    assert (_tile_bits(rec) + 7) // 8 == {1: 1, 200: 1, 256: 1, 257: 2, 65536: 2, 65537: 3}[N]


def test_deterministic_reduction_beyond_2_pow_24_records(dns, orc, deterministic, monkeypatch):
    """4 cameras x 4.5 M Gaussians, nearly all behind the cameras: 18 M records, four radix passes."""
    W, H, f = 128, 96, 100.0
    oracle_threads()
    N, n_vis = 4_500_000, 3000
    u, v, z, sx, sy, opa = _clutter(N, W, H, seed=24, smin=0.7, smax=10.0, zmin=1.5, zmax=6.0)
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(24))[n_vis:]
    z[idx] = -z[idx]
    inp, _gp, _vm, K, _cam = _scene(u, v, z, sx, sy, opa, W, H, f, seed=24)
    inp["colors"] = inp["colors"][:, :1].contiguous()           # SH degree 0: the oracle holds 4.5 M x 1 coefficients, not x 16
    C = 4
    vms = torch.eye(4).repeat(C, 1, 1)
    vms[:, 0, 3] = torch.tensor([0.0, 0.05, -0.05, 0.1])
    Ks = K.expand(C, 3, 3).contiguous()
    rec, n = _det_case(dns, orc, monkeypatch, inp, vms, Ks, W, H, seed=24, what="4 x 4.5 M records", sh_degree=0)
    assert rec == C * N > 1 << 24 and n > 0
    assert (_tile_bits(rec) + 7) // 8 == 4


# ------------------------------------------------------------------------------------------------
# 13. single-pass tile sorts: 2 ... 256 tiles, ONE pass that is the first (generates the pairs) and the last (no key store, tile offsets)
# at once, over every digit width 1 ... 8

@pytest.mark.parametrize("W,H", [(32, 16), (32, 32), (64, 32), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256)])
def test_single_pass_tile_sort_at_every_digit_width(dns, orc, W, H):
    oracle_threads()
    T = (W // 16) * (H // 16)
    bits = T.bit_length() - 1                      # T is a power of two: 1 ... 8 bits
    inp, _gp, viewmat, K, _cam = _scene(*_clutter(300, W, H, seed=bits, smin=0.5, smax=max(W, H) / 4.0), W, H, float(W), seed=bits)
    fig = _dropin_ints(dns, orc, inp, viewmat, K, W, H, f"{W}x{H}, {T} tiles")
    assert fig["tiles"] == T and fig["passes"] == 1 and fig["dbits"] == [bits] and fig["key"] == 16 and fig["exact"]
    assert fig["pairs"] > 0 and fig["max_tiles"] > 1
