"""The frame word that selects the compositing backward's loop (dnsplat_proj_out.saturation_flag -> dnsplat_raster_args.saturation_flag):
nonzero = "the careful loop is required" — a visible opacity above the alpha cap, or a visible conic that fails dns_conic_benign
(csrc/splat_common.h; the arithmetic behind the rule: tests/test_conic_benign_bound.py).

  * the projection raises the word for exactly those frames;
  * on a benign frame the fast loop (no `e <= 0` test, no alpha cap) and the careful loop give the same bits, at the bucket and fold
    sizes of the backward.  One 16 x 16 tile; every Gaussian is kept by one half tile only, so its gradient record receives the rows
    of one wave and the sums do not depend on the order atomics arrive in;
  * a frame with needles and a record that is not definite at all goes through the careful loop and matches the oracle."""
import math

import pytest
import torch

import _proj_ref as P
from _scenes import REL_TOL, assert_close, fp64_envelope, gsplat_inputs, oracle_threads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BG7 = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0])     # the fused pass: no background for rgb | depth, ones for the normals
INTR = (100.0, 100.0, 8.0, 8.0)
NAMES = ("rgb", "depth", "normal", "accumulation")


def benign(conics: torch.Tensor) -> torch.Tensor:
    """dns_conic_benign on fp32 conics [N, 3], operation by operation."""
    a, b, c = conics.float().unbind(-1)
    lo, hi = 2.0 ** -40, 2.0 ** 40
    return (a >= lo) & (a <= hi) & (c >= lo) & (c <= hi) & (b * b <= torch.tensor(1.0 - 2.0 ** -12) * (a * c))


# ---- the projection raises the word --------------------------------------------------------------------------------------------------


def _flag_scene(needle=False, needle_culled=False, hot=False):
    """64 Gaussians on a 64 x 64 image, all visible and round enough; Gaussian 37 optionally a needle (6 x 0.002 x 0.002, some
    300 pixels long and, with eps2d = 0.3, half a pixel thick), optionally behind the camera; Gaussian 5 optionally above the cap."""
    from dn_splatter_amd._ops import ProjCfg

    N, k = 64, 37
    cfg = ProjCfg(width=64, height=64, sh_degree=3)
    g = torch.Generator().manual_seed(11)
    px, py = 4.0 + 56.0 * torch.rand(N, generator=g, dtype=torch.float64), 4.0 + 56.0 * torch.rand(N, generator=g, dtype=torch.float64)
    sa = torch.exp(math.log(0.02) + torch.rand(N, 3, generator=g) * math.log(4.0))
    oa = 0.1 + 0.8 * torch.rand(N, generator=g)
    q = torch.randn(N, 4, generator=g)
    culled = torch.zeros(N, dtype=torch.bool)
    if needle:
        sa[k] = torch.tensor([6.0, 0.002, 0.002])
        q[k] = torch.tensor([1.0, 0.0, 0.0, 0.0])
        px[k], py[k] = 32.0, 32.0
        culled[k] = needle_culled
    if hot:
        oa[5] = 0.9995
    return P.random_scene(N, cfg, seed=12, culled=culled, px=px, py=py, z=torch.full((N,), 3.0, dtype=torch.float64), scales_act=sa,
                          opac_act=oa, quats=q), k


def _projected_flag(s):
    from dn_splatter_amd import _ops

    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    _ops.project(s.means.to(DEV), s.quats.to(DEV), s.scales.to(DEV), s.opacities.to(DEV), **P.layout_tensors(s.coeffs, "split", DEV),
                 viewmat=s.viewmat.to(DEV), K=s.K.to(DEV), normal_frame=None, cfg=s.cfg, saturation_flag=flag)
    torch.cuda.synchronize()
    return int(flag.item())


def _rho2(ref):
    c = ref.out["conics"].double()
    return c[:, 1] ** 2 / (c[:, 0] * c[:, 2])


def test_projection_raises_the_word_for_what_needs_the_careful_loops(orc):
    """Expectations from the fp64 reference, every conic at least a factor two (in 1 - rho^2) away from the rule's edge."""
    edge = 2.0 ** -12
    s, k = _flag_scene()
    ref = P.reference(s)
    assert bool((ref.out["radii"] > 0).all()) and bool((1 - _rho2(ref) > 2 * edge).all())
    assert _projected_flag(s) == 0, "a benign frame raised the word"

    s, k = _flag_scene(needle=True)
    ref = P.reference(s)
    r2 = _rho2(ref)
    others = torch.arange(s.N) != k
    assert int(ref.out["radii"][k]) > 0 and float(1 - r2[k]) < edge / 2 and bool((1 - r2[others] > 2 * edge).all())
    print(f"[benign] needle: 1 - rho^2 = {float(1 - r2[k]):.3e} (rule: >= {edge:.3e}), radius {int(ref.out['radii'][k])}")
    assert _projected_flag(s) != 0, "a visible conic fails the rule and the word stayed 0"

    s, k = _flag_scene(needle=True, needle_culled=True)
    ref = P.reference(s)
    assert int(ref.out["radii"][k]) == 0
    assert _projected_flag(s) == 0, "a culled needle raised the word"

    s, k = _flag_scene(hot=True)
    assert _projected_flag(s) != 0, "a visible opacity above the cap did not raise the word"


# ---- the two loops agree bit for bit on a benign frame -------------------------------------------------------------------------------


def _one_tile_scene(k_top, k_bot, seed):
    """A 16 x 16 image (one tile).  k_top Gaussians centred in rows 1 .. 5, k_bot in rows 11 .. 15; standard deviations 0.45 .. 0.8
    pixels at random angles, opacities 0.05 .. 0.9.  Each reaches alpha >= 0.014 at the pixel centre nearest to it and has
    sigma >= 9.5 > ln(255 x 0.9) + 4 everywhere in the other half tile, 3.5 pixels away: the half tiles keep exactly k_top / k_bot."""
    g = torch.Generator().manual_seed(seed)
    N = k_top + k_bot
    u = lambda n: torch.rand(n, generator=g, dtype=torch.float64)      # noqa: E731
    x = 1.0 + 14.0 * u(N)
    y = torch.cat([1.0 + 4.0 * u(k_top), 11.0 + 4.0 * u(k_bot)])
    s1, s2, th = 0.45 + 0.35 * u(N), 0.45 + 0.35 * u(N), math.pi * u(N)
    l1, l2 = 1 / s1 ** 2, 1 / s2 ** 2
    ca = l1 * th.cos() ** 2 + l2 * th.sin() ** 2
    cc = l1 * th.sin() ** 2 + l2 * th.cos() ** 2
    cb = (l1 - l2) * th.sin() * th.cos()
    perm = torch.randperm(N, generator=g)            # list order (depth) unrelated to the half a Gaussian lies in
    xys = torch.stack([x, y], 1).float()[perm]
    conics = torch.stack([ca, cb, cc], 1).float()[perm]
    opac = (0.05 + 0.85 * u(N)).float()
    top = (torch.arange(N) < k_top)[perm]
    return dict(W=16, H=16, N=N, xys=xys, conics=conics, opacities=opac, colors=0.1 + 0.8 * torch.rand(N, 7, generator=g),
                bg_rgb=torch.rand(3, generator=g), depths=1.0 + torch.arange(N, dtype=torch.float32),
                radii=torch.full((N,), 3, dtype=torch.int32), tiles=torch.ones(N, dtype=torch.int32), top=top)


def _kept_model(s):
    """float64: per half tile, how many Gaussians reach alpha >= 1/255 at one of its 128 pixel centres, and the smallest sigma any
    Gaussian of the other half has there."""
    xy, cn, op = s["xys"].double(), s["conics"].double(), s["opacities"].double()
    out = []
    for half in (0, 1):
        py, px = torch.meshgrid(torch.arange(8, dtype=torch.float64) + 8 * half + 0.5, torch.arange(16, dtype=torch.float64) + 0.5, indexing="ij")
        dx, dy = xy[:, 0, None] - px.reshape(1, -1), xy[:, 1, None] - py.reshape(1, -1)
        sig = 0.5 * (cn[:, 0, None] * dx * dx + cn[:, 2, None] * dy * dy) + cn[:, 1, None] * dx * dy
        amax = (op[:, None] * torch.exp(-sig)).max(1).values
        mine = s["top"] if half == 0 else ~s["top"]
        assert bool((amax[mine] >= 3.0 / 255.0).all()), "a Gaussian is not clearly kept by its own half tile"
        assert bool((sig[~mine].min(1).values > torch.log(255.0 * op[~mine]) + 2.0).all()), "a Gaussian is not clearly culled by the other half"
        out.append(int((amax >= 1.0 / 255.0).sum()))
    return out


def _fused(s, flag_word, cot):
    """The fused forward and backward (_ops.rasterize_dn) on a raster-level scene -> (images, v_splats, means2d.grad, absgrad)."""
    from dn_splatter_amd import _ops

    assert _ops.SATURATION_FLAG and not _ops.DETERMINISTIC["on"]
    lv = {k: s[k].to(DEV).contiguous().clone().requires_grad_(True) for k in ("xys", "conics", "colors", "opacities")}
    splats = _ops._PackFn.apply(lv["xys"], lv["conics"], lv["opacities"], lv["colors"])
    splats.retain_grad()
    m2d = lv["xys"].detach()[None].clone().requires_grad_(True)
    holder = {"saturation_flag": torch.tensor([flag_word], dtype=torch.int32, device=DEV)}
    outs = _ops.rasterize_dn(m2d, splats, s["depths"][None].to(DEV), s["radii"][None].to(DEV), s["tiles"][None].to(DEV),
                             background_rgb=s["bg_rgb"].to(DEV), width=s["W"], height=s["H"], intrinsics=[INTR], absgrad=True,
                             holder=holder)[:4]
    assert int(holder["saturation_flag"].item()) == flag_word
    torch.autograd.backward(list(outs), [c[None].to(DEV) for c in cot])
    torch.cuda.synchronize()
    grads = {"means2d": (m2d.grad[0] + lv["xys"].grad).cpu(), "absgrad": m2d.absgrad.reshape(-1, 2).cpu(), "conics": lv["conics"].grad.cpu(),
             "colors": lv["colors"].grad.cpu(), "opacities": lv["opacities"].grad.reshape(-1).cpu()}
    return tuple(o[0].detach().cpu() for o in outs), splats.grad.detach().cpu(), grads


def _cot(s, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.rand(s["H"], s["W"], c, generator=g) * 2 - 1 for c in (3, 1, 3, 1))


# kept splats per (top, bottom) half tile: both folds of the last bucket (<= 32: four lanes per splat, <= 64: two), a full bucket,
# a bucket boundary, two and four buckets; every list from the second case on spans more than one 64-entry batch of the forward
@pytest.mark.parametrize("k_top,k_bot", [(31, 33), (64, 65), (128, 129), (128 + 33, 3 * 128 + 10)])
def test_fast_and_careful_loops_agree_bit_for_bit(orc, k_top, k_bot):
    s = _one_tile_scene(k_top, k_bot, seed=100 + k_top)
    assert _kept_model(s) == [k_top, k_bot]
    assert bool(benign(s["conics"]).all()) and float(s["opacities"].max()) <= 0.999      # what the projection reports for it: 0
    cot = _cot(s, 3)
    img0, v0, g0 = _fused(s, 0, cot)      # the fast loop
    img1, v1, g1 = _fused(s, 1, cot)      # a caller-supplied nonzero word: the careful loop
    for a, b, nm in zip(img0, img1, NAMES):
        assert torch.equal(a, b), f"{nm} differs between the two runs"
    assert bool(v0.ne(0).any()) and bool(torch.isfinite(v0).all())
    d = (v0.double() - v1.double()).abs().max()
    print(f"[benign] {k_top} + {k_bot} kept: v_splats {'bit-equal' if torch.equal(v0, v1) else 'differ, max |d| %.3e' % float(d)}; "
          f"{int(v0.ne(0).any(1).sum())} of {s['N']} records non-zero")
    assert torch.equal(v0, v1), "v_splats differs between the fast and the careful loop"
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"grad {k} differs between the fast and the careful loop"


# ---- the careful loop still serves what it exists for --------------------------------------------------------------------------------


def _dn_epilogue(R, A, bg_rgb):
    """dn_model.py:526-537, 577-578 on the raw composite (rgb | expected-depth accumulation | normals over ones) and its alpha."""
    rgb = torch.clamp(R[..., :3] + (1 - A)[..., None] * bg_rgb.to(R.dtype), 0.0, 1.0)
    ed = R[..., 3] / A.clamp_min(1e-10)
    depth = torch.where(A > 0, ed, ed.detach().max())[..., None]
    n = R[..., 4:7]
    return rgb, depth, (n / n.norm(dim=-1, keepdim=True) + 1) / 2, A[..., None]


def _needle_scene(orc):
    """1500 Gaussians on 96 x 64 through the oracle's projection; every 60th one stretched into a needle (x 40 along one axis, / 20
    along the others); one visible record's conic replaced by an indefinite one (b^2 > a c)."""
    N, W, H = 1500, 96, 64
    inp, viewmat, K, _ = gsplat_inputs(N, W, H, focal=60.0, seed=5, anisotropic=True)
    sc = inp["scales"].clone()
    sc[::60] = sc[::60] * torch.tensor([40.0, 0.05, 0.05])
    radii, xys, depths, conics, _comp, tiles = orc.project_fwd(inp["means"], inp["quats"], sc, viewmat[0], K[0], W, H)
    vis = radii > 0
    bad = vis & ~benign(conics)
    n_needles = int(bad.sum())
    assert n_needles >= 3, f"only {n_needles} visible conics fail the rule: the scene is badly built"
    # the hand-made record: a visible, benign Gaussian of moderate size near the image centre
    cand = torch.nonzero(vis & ~bad & (radii > 4) & (radii < 30) & ((xys - torch.tensor([W / 2, H / 2])).abs().max(1).values < 20)).reshape(-1)
    j = int(cand[0])
    conics = conics.clone()
    conics[j] = torch.tensor([0.05, 0.09, 0.05])
    tw, th = (W + 15) // 16, (H + 15) // 16
    _t, ids, fid = orc.isect_tiles(xys, radii, depths, 16, tw, th)
    offs = orc.isect_offset_encode(ids, tw, th)
    g = torch.Generator().manual_seed(9)
    return dict(W=W, H=H, N=N, xys=xys, conics=conics, opacities=inp["opacities"], colors=0.1 + 0.8 * torch.rand(N, 7, generator=g),
                bg_rgb=torch.rand(3, generator=g), depths=depths, radii=radii, tiles=tiles, offs=offs, fid=fid, hand_made=j, n_needles=n_needles)


def _oracle(orc, s, cot, keep, dt):
    f = lambda t: t.to(dt).contiguous()                                   # noqa: E731
    W, H = s["W"], s["H"]
    border = flip = None
    if dt == torch.float32 and keep is None:
        border, flip = torch.zeros(H, W, dtype=torch.uint8), torch.zeros(H, W, dtype=torch.float32)
    common = (f(s["xys"]), f(s["conics"]))
    R, A, last = orc.rasterize_fwd(*common, f(s["colors"]), f(s["opacities"]), f(BG7), W, H, 16, s["offs"], s["fid"], border, flip)
    if keep is None:
        keep = ~border.bool()
    Rl, Al = R.clone().requires_grad_(True), A.clone().requires_grad_(True)
    imgs = _dn_epilogue(Rl, Al, s["bg_rgb"])
    torch.autograd.backward(list(imgs), [(c * keep[..., None]).to(dt) for c in cot])
    v_r, v_a = Rl.grad, Al.grad
    # channels [0, 4) carry v_alphas and the screen-space gradient, channels [4, 7) neither: the reference's two passes
    g = {}
    for lo, hi, va, xy in ((0, 4, v_a, True), (4, 7, torch.zeros_like(v_a), False)):
        m2, ab, cn, cc, op = orc.rasterize_bwd(*common, f(s["colors"][:, lo:hi]), f(s["opacities"]), f(BG7[lo:hi]), W, H, 16, s["offs"], s["fid"],
                                               f(A), last, f(v_r[..., lo:hi]), f(va), absgrad=True)
        if xy:
            g["means2d"], g["absgrad"] = m2, ab
        g["conics"] = g.get("conics", 0) + cn
        g["opacities"] = g.get("opacities", 0) + op.reshape(-1)
        g["colors"] = cc if "colors" not in g else torch.cat([g["colors"], cc], 1)
    return tuple(i.detach() for i in imgs), g, keep


def test_careful_loop_on_needles_and_an_indefinite_record_matches_the_oracle(orc):
    """The tolerances of the parity tests (tests/_scenes.py): REL_TOL of the tensor's scale, for the gradients plus the fp64 envelope
    of the reference's own fp32 evaluation; pixels with a borderline decision carry no cotangent and are not compared."""
    oracle_threads()
    s = _needle_scene(orc)
    j = s["hand_made"]
    a, b, c = s["conics"][j].tolist()
    assert b * b > a * c and not bool(benign(s["conics"][j][None])[0])
    cot = _cot(s, 4)
    imgs_o, g_o, keep = _oracle(orc, s, cot, None, torch.float32)
    _i64, g64, _ = _oracle(orc, s, cot, keep, torch.float64)
    print(f"[benign] {s['n_needles']} visible needles, record {j} indefinite; {int((~keep).sum())} of {keep.numel()} pixels borderline")
    assert int((~keep).sum()) <= 0.1 * keep.numel()
    cot_k = tuple(c * keep[..., None] for c in cot)
    imgs, v, g = _fused(s, 1, cot_k)          # the word the projection raises for these records (benign() above is false for some)
    for got, ref, nm in zip(imgs, imgs_o, NAMES):
        assert_close(got, ref, f"careful loop, {nm}", tol=REL_TOL, keep=keep)
    assert bool(g["conics"][j].ne(0).any()), "the indefinite record took part in no pair: the scene is badly built"
    for k in ("means2d", "absgrad", "conics", "colors", "opacities"):
        ref32, ref64 = g_o[k].reshape(g[k].shape), g64[k].reshape(g[k].shape)
        assert_close(g[k], ref32, f"careful loop, grad {k}", tol=REL_TOL, envelope=fp64_envelope(ref32, ref64))
