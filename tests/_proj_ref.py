"""fp64 reference of ONE projection call (dnsplat_project_fwd / dnsplat_project_bwd), its per-entry tolerance unit, the scenes that aim
at the kernels' machinery and the comparator.  CPU only: everything here is composed from the oracle (``oracle.project_fwd / _bwd``,
``oracle.sh_fwd / _bwd``, ``oracle.project_edge``, ``oracle.tight_tile_boxes``) evaluated in float64 on the fp32 inputs cast up.

Tolerance.  Every float output gets its own bound per Gaussian and per component, ``k x unit`` with ``unit = max(a, b, c)``:
  (a) |oracle fp32 - oracle fp64| on that entry: the error of a faithful fp32 implementation,
  (b) the change of the fp64 result when the fp32 inputs move by +-1 ulp: the conditioning,
  (c) eps32 x |value|.
(a) and (b) are taken over the same set of +-1 ulp neighbours of the inputs: see unit_terms().
An entry whose three terms are all zero (a culled Gaussian's row, an inactive SH band) has to be zero exactly.

Masks of Gaussians that cannot be judged (each excludes only what its decision governs):
  edge        oracle.project_edge: an integer output hinges on a comparison inside the fp32 rounding envelope -> every output of the Gaussian
  clamp_edge  a colour with |c + 0.5| below the fp32 envelope of its sum: 16 roundings of at most sum_k |Y_k| |c_k| + 0.5 with |Y_k| <= 1.1
              (the largest real SH basis value up to degree 3 on the unit sphere is 1.02) -> the colour channels of the record, the SH
              gradients and v_means (the clamp gates the view-direction gradient, which lands on the mean)
  normal_tie  the two smallest raw scales within 4 ulp of each other, or |n . (camera - mean)| within 16 roundings of its terms' magnitude
              -> normals_world, the record's normal channels and (with normal channels) v_quats
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, replace
from typing import Dict, Optional

import numpy as np
import torch

from dn_splatter_amd._ops import ProjCfg
from oracle import oracle as orc

W, H, TILE = 200, 136, 16          # ragged frame: 12.5 x 8.5 tiles, the last tile column and the last tile row are partial
TW, TH = math.ceil(W / TILE), math.ceil(H / TILE)
EPS32 = 2.0 ** -23
JITTER_DRAWS = 2
ALPHA_MAX = 0.999
CAPS = dict(edge=0.02, clamp_edge=0.01, normal_tie=0.01)
TIGHT_NEAR_CAP = 0.01      # tight_near() flags a 1e-5 (|m| + h + 1) / 16 neighbourhood of the integers on four box edges: about one Gaussian in 10^3

FWD_KEYS = ("means2d", "depths", "conics", "compensations", "splats", "normals_world")
GEO_KEYS = ("v_means", "v_quats", "v_scales", "v_opacities")
SH_KEYS = ("v_sh0", "v_shN", "v_coeffs", "v_colors")
INT_KEYS = ("radii", "tiles_per_gauss", "tiles_bin", "tile_boxes")


# --------------------------------------------------------------------------------------------------------------- cameras and scenes


def camera(identity: bool = False):
    """(viewmat [4,4], K [3,3], normal_frame [12]) in fp32.  ``identity``: no rotation, no translation — a camera-space z is then the
    world z bit for bit, which the depth-boundary scene needs."""
    if identity:
        R, t = np.eye(3), np.zeros(3)
    else:
        ax, ay, az = 0.3, -0.5, 0.2
        Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
        Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
        Rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
        R, t = Rz @ Ry @ Rx, np.array([0.3, -0.2, 0.5])
    V = np.eye(4)
    V[:3, :3], V[:3, 3] = R, t
    viewmat = torch.from_numpy(V).float()
    K = torch.tensor([[150.0, 0.0, 101.5], [0.0, 140.0, 66.25], [0.0, 0.0, 1.0]])
    Vd = viewmat.double()
    pos = -(Vd[:3, :3].T @ Vd[:3, 3])
    # the normal frame: world -> camera rotation of the normals (rows) and the camera centre the flip test uses
    nf = torch.cat([Vd[:3, :3].reshape(-1), pos]).float()
    return viewmat, K, nf


def place(viewmat, K, px, py, z):
    """World-space means (fp32) of points that project to pixel (px, py) at camera depth z; fp64 arithmetic, rounded once."""
    V, Kd = viewmat.double(), K.double()
    px, py, z = (torch.as_tensor(v, dtype=torch.float64) for v in (px, py, z))
    mc = torch.stack([(px - Kd[0, 2]) / Kd[0, 0] * z, (py - Kd[1, 2]) / Kd[1, 1] * z, z], -1)
    return ((mc - V[:3, 3]) @ V[:3, :3]).float()


@dataclass
class Scene:
    name: str
    means: torch.Tensor
    quats: torch.Tensor
    scales: torch.Tensor          # raw: log scales when cfg.scales_are_log
    opacities: torch.Tensor       # raw: logits when cfg.opacities_are_logit
    coeffs: Optional[torch.Tensor]    # [N,K,3] SH coefficients (cfg.sh_degree >= 0)
    colors: Optional[torch.Tensor]    # [N,C] direct colours (cfg.sh_degree < 0)
    viewmat: torch.Tensor
    K: torch.Tensor
    nf: torch.Tensor
    cfg: ProjCfg
    visible: Optional[torch.Tensor] = None        # bool [N] the builder advertises (None: not advertised)
    may_be_edge: Optional[torch.Tensor] = None    # bool [N]: constructed boundary scenes — the only Gaussians that may be flagged `edge`
    tags: Dict[str, torch.Tensor] = field(default_factory=dict)

    @property
    def N(self):
        return self.means.shape[0]


def wave_words(vis: torch.Tensor):
    """The 64-bit visibility word of every 64-Gaussian workgroup (bit l = lane l), as Python ints."""
    v = vis.tolist()
    return [sum(1 << l for l, b in enumerate(v[i:i + 64]) if b) for i in range(0, len(v), 64)]


def _inv_act(x, on, kind):
    if not on:
        return x
    return torch.log(x) if kind == "log" else torch.log(x / (1 - x))


def random_scene(N, cfg: ProjCfg, seed=0, culled=None, n_colors=3, sh_K=16, name=None, identity=False, px=None, py=None, z=None,
                 scales_act=None, opac_act=None, quats=None):
    """N Gaussians inside the image in front of the camera (every one visible), except those of ``culled`` (bool [N]), which sit at
    the mirrored depth BEHIND the camera: a decision far from any threshold."""
    g = torch.Generator().manual_seed(1000 + seed)
    viewmat, K, nf = camera(identity)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)      # noqa: E731
    px = 2.0 + u(N) * (W - 4.0) if px is None else torch.as_tensor(px, dtype=torch.float64)
    py = 2.0 + u(N) * (H - 4.0) if py is None else torch.as_tensor(py, dtype=torch.float64)
    z = 1.5 + u(N) * 4.5 if z is None else torch.as_tensor(z, dtype=torch.float64)
    culled = torch.zeros(N, dtype=torch.bool) if culled is None else culled
    z = torch.where(culled, -z, z)
    means = place(viewmat, K, px, py, z).reshape(N, 3)
    q_rand = torch.randn(N, 4, generator=g) * (0.5 + torch.rand(N, 1, generator=g))       # not normalised
    quats = q_rand if quats is None else quats
    sa = torch.exp(math.log(0.01) + u(N, 3) * math.log(15.0)).float() if scales_act is None else torch.as_tensor(scales_act).float()
    oa = (0.05 + 0.9 * u(N)).float() if opac_act is None else torch.as_tensor(opac_act).float()
    coeffs = colors = None
    if cfg.sh_degree >= 0:
        coeffs = torch.randn(N, sh_K, 3, generator=g) * 0.2
        coeffs[:, 0] = torch.randn(N, 3, generator=g) * 1.2          # both sides of the clamp: c + 0.5 < 0 for about one colour in ten
    else:
        colors = torch.randn(N, n_colors, generator=g) if cfg.colors_are_logit else torch.rand(N, n_colors, generator=g)
    return Scene(name or f"random{N}", means, quats, _inv_act(sa, cfg.scales_are_log, "log"), _inv_act(oa, cfg.opacities_are_logit, "logit"),
                 coeffs, colors, viewmat, K, nf, cfg, visible=~culled)


PATTERN_N = 128 + 37


def pattern_mask(pattern: str, N: int = PATTERN_N) -> torch.Tensor:
    """bool [N] VISIBLE lanes of the named per-wave visibility pattern."""
    i = torch.arange(N)
    lane = i % 64
    if pattern == "all_culled":
        return torch.zeros(N, dtype=torch.bool)
    if pattern == "only_lane0":
        return lane == 0
    if pattern == "only_lane63":
        return lane == 63
    if pattern == "only_last_valid":
        return i == N - 1
    if pattern == "alternating":
        return lane % 2 == 0
    if pattern == "alternating_pairs":
        return (lane // 2) % 2 == 1
    if pattern == "63_of_64":
        return lane != 17
    if pattern == "culled_wave_between":
        return (i // 64) != 1
    raise KeyError(pattern)


PATTERNS = ("all_culled", "only_lane0", "only_lane63", "only_last_valid", "alternating", "alternating_pairs", "63_of_64",
            "culled_wave_between")


def pattern_scene(pattern: str, cfg: ProjCfg, seed=0, **kw) -> Scene:
    vis = pattern_mask(pattern)
    return random_scene(PATTERN_N, cfg, seed=seed, culled=~vis, name="pattern_" + pattern, **kw)


def _axis_scales(rf, z, eps2d):
    """[n,3] scales (s, s, s / 2) of axis-aligned Gaussians (identity rotation) whose 3 sqrt(lambda) is ``rf`` pixels ON the optical axis
    of the identity camera: lambda = (s fx / z)^2 + eps2d, fx = 150 > fy.  The flat third axis is the normal, far from a tie."""
    rf = torch.as_tensor(rf, dtype=torch.float64).reshape(-1)
    s = torch.sqrt((rf / 3.0) ** 2 - eps2d) * z / 150.0
    return torch.stack([s, s, 0.5 * s], -1)


def _axis_quats(n):
    return torch.tensor([[1.3, 0.0, 0.0, 0.0]]).repeat(n, 1)      # the identity rotation, not normalised


def _radius64(s: "Scene"):
    """The fp64 radius ceil(3 sqrt(lambda)) of every Gaussian BEFORE any culling, from the conic of oracle/dense_ref.py."""
    from oracle import dense_ref
    pr = dense_ref.project(s.means.double(), s.quats.double(), torch.exp(s.scales.double()) if s.cfg.scales_are_log else s.scales.double(),
                           s.viewmat.double(), s.K.double(), W, H, eps2d=s.cfg.eps2d, near=1e-9)
    a, b, c = pr["conics"].unbind(-1)
    det_c = a * c - b * b
    c00, c11 = c / det_c, a / det_c
    mid = 0.5 * (c00 + c11)
    return torch.ceil(3.0 * torch.sqrt(mid + torch.sqrt(torch.clamp(mid * mid - 1.0 / det_c, min=0.01))))


def depth_boundary_scene(cfg: ProjCfg) -> Scene:
    """Depths at near (1 +- 2^-j) and far (1 +- 2^-j), j = 1 .. 23, and at near and far exactly.  Needs cfg.near_plane and cfg.far_plane
    to be powers of two: every depth is then an exact fp32 number, and the identity camera hands it to the kernel unchanged."""
    zs, tag_j = [], []
    for plane in (cfg.near_plane, cfg.far_plane):
        for j in range(1, 24):
            for sgn in (-1.0, 1.0):
                zs.append(plane * (1.0 + sgn * 2.0 ** -j)); tag_j.append(j)
        zs.append(plane); tag_j.append(99)
    N = len(zs)
    z = torch.tensor(zs, dtype=torch.float64)
    assert torch.equal(z.float().double(), z)
    s = random_scene(N, cfg, seed=11, name="depth_boundary", identity=True, z=z, px=torch.full((N,), 101.5), py=torch.full((N,), 66.25),
                     scales_act=(0.02 * z)[:, None].repeat(1, 3) * torch.tensor([1.0, 1.5, 0.7], dtype=torch.float64))
    j = torch.tensor(tag_j)
    s.visible = (z >= cfg.near_plane) & (z <= cfg.far_plane)
    s.may_be_edge = j >= 21
    s.tags["j"] = j
    return s


def radius_clip_scene(cfg: ProjCfg) -> Scene:
    """Axis-aligned Gaussians on the optical axis whose 3 sqrt(lambda) straddles cfg.radius_clip (an integer c): culled when
    ceil(3 sqrt(lambda)) <= c."""
    c = cfg.radius_clip
    rfs = [c - 0.5, c - 0.01, c + 0.01, c + 0.5, c - 1.5, c + 1.5, c]
    z = 3.0
    N = len(rfs)
    s = random_scene(N, cfg, seed=12, name="radius_clip", identity=True, z=torch.full((N,), z), px=torch.full((N,), 101.5),
                     py=torch.full((N,), 66.25), scales_act=_axis_scales(rfs, z, cfg.eps2d), quats=_axis_quats(N))
    s.visible = torch.tensor([math.ceil(rf) > c for rf in rfs[:-1]] + [False])
    s.may_be_edge = torch.tensor([False] * (N - 1) + [True])          # 3 sqrt(lambda) on the integer itself
    return s


def frustum_scene(cfg: ProjCfg) -> Scene:
    """Centres outside the image by the splat's radius -+ d on each of the four sides (the screen cull is centre +- radius against
    0 / W / H), d in {0.5, 0.01, 0.001} pixels: well outside oracle.project_edge's 4e-6 (|x| + r + 1) envelope.  The radius depends
    (weakly) on the position, so the builder iterates position -> fp64 radius -> position and asserts that it settled."""
    z = 3.0
    ds, ins, sides = [], [], []
    for d in (0.5, 0.01, 0.001):
        for inside in (True, False):
            for side in range(4):
                ds.append(d); ins.append(inside); sides.append(side)
    N = len(ds)
    d, inside, side = torch.tensor(ds, dtype=torch.float64), torch.tensor(ins), torch.tensor(sides)
    radius = torch.full((N,), 8.0, dtype=torch.float64)
    for _ in range(4):
        off = torch.where(inside, radius - d, radius + d)
        px = torch.where(side == 0, -off, torch.where(side == 1, W + off, torch.full_like(off, 80.3)))
        py = torch.where(side == 2, -off, torch.where(side == 3, H + off, torch.full_like(off, 50.7)))
        s = random_scene(N, cfg, seed=13, name="frustum", identity=True, z=torch.full((N,), z), px=px, py=py,
                         scales_act=_axis_scales([6.5] * N, z, cfg.eps2d), quats=_axis_quats(N))
        new_radius = _radius64(s)
        if torch.equal(new_radius, radius):
            break
        radius = new_radius
    assert torch.equal(_radius64(s), radius), "the frustum scene's radii did not settle"
    s.visible = inside
    s.may_be_edge = torch.zeros(N, dtype=torch.bool)
    s.tags["radius"] = radius
    return s


def singular_scene(cfg: ProjCfg) -> Scene:
    """Covariances of rank one (two zero scales): cov2d is singular before eps2d is added.  With eps2d > 0 the splat is visible and its
    compensation is the square root of a cancelled determinant; with eps2d = 0 det itself is the cancellation: `edge` by construction.
    The two zero scales tie for the normal's axis: `normal_tie` by construction as well."""
    N = 8
    sc = torch.zeros(N, 3)
    sc[:, 0] = torch.linspace(0.02, 0.2, N)
    s = random_scene(N, cfg, seed=14, name="singular", scales_act=sc)
    s.visible = torch.ones(N, dtype=torch.bool) if cfg.eps2d > 0 else None
    s.may_be_edge = torch.full((N,), cfg.eps2d == 0.0)
    return s


def border_scene(cfg: ProjCfg) -> Scene:
    """Splats whose 3-sigma square crosses each image edge and each corner, covers the whole frame, or reaches exactly to a tile boundary
    (centre and radius integers with centre +- radius a multiple of 16: `edge` by construction, the box is then checked from the
    kernel's own centre)."""
    z = 3.0
    spec = [  # (px, py, 3 sqrt(lambda) in pixels)
        (3.3, 60.2, 9.5), (197.1, 60.2, 9.5), (90.4, 2.6, 9.5), (90.4, 133.2, 9.5),
        (2.2, 3.1, 12.5), (198.4, 3.1, 12.5), (2.2, 134.0, 12.5), (198.4, 134.0, 12.5),
        (100.3, 68.9, 400.0), (100.3, 68.9, 40.5),
        (-4.5, 70.5, 9.5), (204.5, 70.5, 9.5), (70.5, -4.5, 9.5), (70.5, 140.5, 9.5),
        (195.5, 131.5, 2.5), (8.5, 8.5, 2.5),
        (40.0, 40.0, 7.5), (104.0, 72.0, 23.5),
    ]
    N = len(spec)
    g = torch.Generator().manual_seed(5)
    s = random_scene(N, cfg, seed=15, name="border", identity=True, z=torch.full((N,), z), px=[p[0] for p in spec], py=[p[1] for p in spec],
                     scales_act=_axis_scales([p[2] for p in spec], z, cfg.eps2d), quats=_axis_quats(N),
                     opac_act=0.02 + 0.97 * torch.rand(N, generator=g))
    s.visible = torch.ones(N, dtype=torch.bool)
    s.may_be_edge = torch.tensor([False] * (N - 2) + [True, True])
    return s


# ----------------------------------------------------------------------------------------------------------------- SH layouts


def layout_tensors(coeffs: torch.Tensor, layout: str, device="cpu"):
    """The SH coefficient tensors of ``layout`` as leaves on ``device``: dict(coeffs=) or dict(sh0=, shN=).
    cat / split: the two staged layouts.  cat_unaligned / split_unaligned: the same shapes at a base one float past a 16-byte boundary,
    which the staged kernels cannot take (SH_DIRECT)."""
    N, Kb = coeffs.shape[0], coeffs.shape[1]
    c = coeffs.to(device)
    if layout == "cat":
        return dict(coeffs=c.clone().requires_grad_(True))
    if layout == "split":
        return dict(sh0=c[:, 0].clone().requires_grad_(True), shN=c[:, 1:].clone().requires_grad_(True))
    if layout == "cat_unaligned":
        buf = torch.zeros(N * Kb * 3 + 4, device=device)
        v = buf[1:1 + N * Kb * 3].view(N, Kb, 3)
        v.copy_(c)
        return dict(coeffs=v.requires_grad_(True))
    if layout == "split_unaligned":
        buf = torch.zeros(N * (Kb - 1) * 3 + 4, device=device)
        v = buf[1:1 + N * (Kb - 1) * 3].view(N, Kb - 1, 3)
        v.copy_(c[:, 1:])
        return dict(sh0=c[:, 0].clone().requires_grad_(True), shN=v.requires_grad_(True))
    raise KeyError(layout)


def binding_layout(cfg: ProjCfg, coeffs=None, sh0=None, shN=None) -> str:
    """Restatement of what reaches ``sh_layout()`` (project.hip) for the tensors ``_ops.project`` is given: the pointer pair and strides
    ``_ProjectFn.forward`` derives, then the C rule (K == 16, pointer distance, strides, 16-byte alignment of the staged base)."""
    if cfg.sh_degree < 0:
        return "direct"
    if coeffs is not None:
        assert coeffs.is_contiguous()
        K_, b0, s0, sN = coeffs.shape[1], coeffs.data_ptr(), 3 * coeffs.shape[1], 3 * coeffs.shape[1]
        bN = b0 + 12
    else:
        assert sh0.is_contiguous() and (shN is None or shN.is_contiguous())
        K_ = 1 + (shN.shape[1] if shN is not None else 0)
        b0, s0 = sh0.data_ptr(), 3
        bN, sN = (shN.data_ptr(), 3 * (K_ - 1)) if (shN is not None and shN.shape[1] > 0) else (0, 0)
    if K_ != 16 or not b0 or not bN:
        return "direct"
    if bN == b0 + 12 and s0 == 48 and sN == 48 and b0 % 16 == 0:
        return "cat"
    if s0 == 3 and sN == 45 and bN % 16 == 0:
        return "split"
    return "direct"


INTENDED_LAYOUT = {"cat": "cat", "split": "split", "cat_unaligned": "direct", "split_unaligned": "direct"}


# ------------------------------------------------------------------------------------------------------------------- the reference


def make_cotangents(N, cfg: ProjCfg, seed=0, means2d=False, depths=False, conics=False, compensations=False):
    """Cotangents of one backward: the gradient records [N,16] (every column filled: the kernel must ignore the channels beyond the used
    ones and columns 14-15) plus the optional separate ones.  fp32 CPU tensors."""
    g = torch.Generator().manual_seed(77 + seed)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    cot = dict(v_splats=r(N, 16), v_means2d=None, v_depths=None, v_conics=None, v_compensations=None)
    if means2d:
        cot["v_means2d"] = r(N, 2)
    if depths:
        cot["v_depths"] = r(N)
    if conics:
        cot["v_conics"] = r(N, 3)
    if compensations and cfg.antialiased:
        cot["v_compensations"] = r(N)
    return cot


def n_channels(s: Scene):
    return 3 if s.cfg.sh_degree >= 0 else s.colors.shape[1]


def tile_boxes_3sigma(means2d, radii, dt=torch.float32):
    """gsplat's 3-sigma tile box (oracle tile_bbox / dns_tile_bbox) evaluated in ``dt``, the operation order of both."""
    mx, my, r = means2d[:, 0].to(dt), means2d[:, 1].to(dt), radii.to(dt)
    ts = float(TILE)
    x0 = torch.floor(mx / ts - r / ts).clamp(0, TW); x1 = torch.ceil(mx / ts + r / ts).clamp(0, TW)
    y0 = torch.floor(my / ts - r / ts).clamp(0, TH); y1 = torch.ceil(my / ts + r / ts).clamp(0, TH)
    vis = radii > 0
    return tuple(torch.where(vis, t, torch.zeros_like(t)).long() for t in (x0, y0, x1, y1))


def pack_boxes(x0, y0, x1, y1):
    """tile_boxes [N,2] int32 as the kernel stores them: first tile id, width | height << 16 (zeros for a culled Gaussian)."""
    return torch.stack([y0 * TW + x0, (x1 - x0) | ((y1 - y0) << 16)], -1).to(torch.int32)


def _evaluate(s: Scene, cot, dt, jitter=None):
    """One projection call and its backward through the oracle in dtype ``dt``.  ``jitter``: a function (name, tensor) -> tensor applied to every
    fp32 parameter tensor before the cast (the +-1 ulp moves)."""
    cfg = s.cfg
    N = s.N
    j = (lambda name, t: t) if jitter is None else jitter
    up = lambda name, t: j(name, t).to(dt)      # noqa: E731
    means, quats, raw_sc, raw_op = up("means", s.means), up("quats", s.quats), up("scales", s.scales), up("opacities", s.opacities)
    V, K, nf = s.viewmat.to(dt), s.K.to(dt), s.nf.to(dt)
    sc = torch.exp(raw_sc) if cfg.scales_are_log else raw_sc
    op = torch.sigmoid(raw_op) if cfg.opacities_are_logit else raw_op
    args = (V, K, W, H, cfg.eps2d, cfg.near_plane, cfg.far_plane, cfg.radius_clip)
    radii, m2d, dep, con, comp, tiles = orc.project_fwd(means, quats, sc, *args, TILE, True)
    vis = radii > 0
    out = dict(radii=radii, means2d=m2d, depths=dep, conics=con, compensations=comp, tiles_per_gauss=tiles)
    op_rec = op * comp if cfg.antialiased else op
    rec = torch.zeros(N, 16, dtype=dt)
    rec[:, 0:2], rec[:, 2:5], rec[:, 5] = m2d, con, op_rec
    campos = -(V[:3, :3].T @ V[:3, 3])
    clamp_edge = torch.zeros(N, dtype=torch.bool)
    if cfg.sh_degree >= 0:
        coeffs = up("coeffs", s.coeffs)
        dirs = means - campos[None]
        raw = orc.sh_fwd(cfg.sh_degree, dirs, coeffs, radii)
        cols = torch.clamp_min(raw + 0.5, 0.0)
        nb = (cfg.sh_degree + 1) ** 2
        env = 16 * EPS32 * (1.1 * coeffs[:, :nb].abs().sum(1) + 0.5)
        clamp_edge = ((raw + 0.5).abs() <= env).any(-1) & vis
    else:
        colors = up("colors", s.colors)
        cols = torch.sigmoid(colors) if cfg.colors_are_logit else colors
    ch = cols.shape[1]
    rec[:, 6:6 + ch] = cols
    if cfg.with_depth:
        rec[:, 6 + ch] = dep
        ch += 1
    # per-Gaussian normal (dn_model.py:543-558): +- column argmin(scale) of R(q), facing the camera; for EVERY Gaussian
    kmin = torch.argmin(raw_sc, dim=-1)
    srt = torch.sort(raw_sc, dim=-1).values
    Rq = orc.quat_to_rotmat(quats)
    col = Rq[torch.arange(N), :, kmin]
    n = col / col.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    view = nf[9:12][None] - means
    dot = (n * view).sum(-1)
    sgn = torch.where(dot < 0, -torch.ones_like(dot), torch.ones_like(dot))
    nworld = n * sgn[:, None]
    normal_tie = ((srt[:, 1] - srt[:, 0]).abs() <= 4 * EPS32 * srt[:, :2].abs().amax(-1)) | (dot.abs() <= 16 * EPS32 * (n * view).abs().sum(-1))
    out["normals_world"] = nworld
    Mn = nf[:9].reshape(3, 3)
    if cfg.with_normals:
        rec[:, 6 + ch:9 + ch] = nworld @ Mn.T
    rec = torch.where(vis[:, None], rec, torch.zeros_like(rec))
    out["splats"] = rec
    x0, y0, x1, y1 = tile_boxes_3sigma(m2d, radii, dt)
    if cfg.tight_tiles:      # the rule is defined in fp32 (oracle.tight_tile_boxes); compare() judges it on the kernel's own projection
        x0, y0, x1, y1 = orc.tight_tile_boxes(m2d, con, op_rec, radii, TILE, TW, TH)
    out["tile_boxes"] = pack_boxes(x0, y0, x1, y1)
    out["tiles_bin"] = ((x1 - x0) * (y1 - y0)).to(torch.int32)
    masks = dict(clamp_edge=clamp_edge, normal_tie=normal_tie)
    if cot is None:
        return out, masks

    # ---- backward
    z = lambda *sh: torch.zeros(*sh, dtype=dt)      # noqa: E731
    vr = cot["v_splats"].to(dt)
    v_xy = cot["v_means2d"].to(dt) if cot["v_means2d"] is not None else vr[:, 0:2]
    v_con = vr[:, 2:5] + (cot["v_conics"].to(dt) if cot["v_conics"] is not None else 0)
    v_dep = cot["v_depths"].to(dt) if cot["v_depths"] is not None else z(N)
    v_cmp = cot["v_compensations"].to(dt) if cot["v_compensations"] is not None else z(N)
    v_o = vr[:, 5]
    if cfg.antialiased:
        v_cmp = v_cmp + v_o * op
        v_o = v_o * comp
    v_op = v_o * op * (1 - op) if cfg.opacities_are_logit else v_o
    out["v_opacities"] = torch.where(vis, v_op, z(N))
    v_means_extra = z(N, 3)
    ch = cols.shape[1]
    if cfg.sh_degree >= 0:
        vcol = torch.where(raw + 0.5 >= 0, vr[:, 6:9], z(N, 3))
        v_coeffs, v_dirs = orc.sh_bwd(cfg.sh_degree, dirs, coeffs, radii, vcol, True)
        out["v_coeffs"], out["v_sh0"], out["v_shN"] = v_coeffs, v_coeffs[:, 0], v_coeffs[:, 1:]
        v_means_extra = v_dirs
    else:
        vc = vr[:, 6:6 + ch]
        if cfg.colors_are_logit:
            vc = vc * cols * (1 - cols)
        out["v_colors"] = torch.where(vis[:, None], vc, torch.zeros_like(vc))
    if cfg.with_depth:
        v_dep = v_dep + vr[:, 6 + ch]
        ch += 1
    v_q_extra = z(N, 4)
    if cfg.with_normals:
        q = quats.clone().requires_grad_(True)
        c_ = orc.quat_to_rotmat(q)[torch.arange(N), :, kmin]
        ncam = (c_ / c_.norm(dim=-1, keepdim=True).clamp_min(1e-12) * sgn[:, None]) @ Mn.T
        (v_q_extra,) = torch.autograd.grad((ncam * vr[:, 6 + ch:9 + ch]).sum(), q)
        v_q_extra = torch.where(vis[:, None], v_q_extra, z(N, 4))
    v_means, v_quats, v_scales = orc.project_bwd(means, quats, sc, *args, radii, v_xy.contiguous(), v_dep, v_con.contiguous(),
                                                 v_cmp if cfg.antialiased else None)
    out["v_means"] = v_means + v_means_extra
    out["v_quats"] = v_quats + v_q_extra
    out["v_scales"] = v_scales * sc if cfg.scales_are_log else v_scales
    return out, masks


def _ulp_jitter(seed):
    g = torch.Generator().manual_seed(seed)

    def jitter(name, t):       # tests/test_oracle_known_answer.py test_projection_edge_flags_cover_last_place_jitter, +-1 ulp
        a = t.contiguous().numpy().copy().view(np.int32)
        a += torch.randint(-1, 2, t.shape, generator=g).numpy().astype(np.int32)
        return torch.where(t == 0, t, torch.from_numpy(a.view(np.float32)))      # a zero stays: its bit pattern has no lower neighbour
    return jitter


def _ulp_step(name, col):
    """Jitter that moves ONE scalar input of every Gaussian (column ``col`` of the flattened rows of parameter ``name``) up by one ulp."""
    def jitter(n, t):
        if n != name:
            return t
        a = t.contiguous().numpy().copy().view(np.int32).reshape(t.shape[0], -1)
        a[:, col] += np.where(a[:, col] >= 0, 1, -1).astype(np.int32)      # the next number away from zero
        return torch.where(t == 0, t, torch.from_numpy(a.reshape(t.shape).view(np.float32)))
    return jitter


def unit_terms(s: Scene, cot, out, out32, floats):
    """Terms (a) and (b) of the unit, from one fp64 and one fp32 evaluation of the oracle at each of a set of inputs within +-1 ulp of
    the scene's: ``JITTER_DRAWS`` random draws that move every input at once, and one step per scalar geometry input of a Gaussian
    (3 + 4 + 3 + 1) that moves that input alone.

    (a) the largest |oracle fp32 - oracle fp64| over the scene's inputs and those neighbours.  The fp32 oracle's error at ONE input is
        one realisation of its rounding errors, and on an entry that is a small sum of large terms (v_scales of the long axis, v_quats
        after the projection onto the tangent of q / |q|) one realisation can sit an order of magnitude below the typical one: on
        Gaussian 581 of scene n1000, v_scales[0] = -0.2009, the oracle's error is 2.5e-7 at the scene's input, 1.9e-6 in the median
        and 9.3e-6 at most over 32 neighbours — and the kernel's is 9.1e-6.  The neighbours are other realisations of the same
        implementation on (to fp32) the same Gaussian.
    (b) the change of the fp64 result: the larger of the random draws and of the worst case over the signs to first order,
        sum_i |change when input i alone moves|.  A random draw adds the ten or so sensitivities of a Gaussian with random signs and a
        third of them with weight zero, so on a cancelling gradient two draws sit 5 to 20 times below the box's worst case for one
        entry in a hundred, 64 draws still up to 2 times."""
    a = {k: (out32[k].double() - out[k]).abs() for k in floats}
    b = {k: torch.zeros_like(out[k]) for k in floats}
    first = {k: torch.zeros_like(out[k]) for k in floats}
    if s.N == 0:
        return a, b
    jitters = [(lambda d=d: _ulp_jitter(4242 + d), b, torch.maximum) for d in range(JITTER_DRAWS)]
    # the coefficients and colours enter linearly and only move with the random draws: the cancelling entries are the geometry's
    params = dict(means=s.means, quats=s.quats, scales=s.scales, opacities=s.opacities)
    for name, t in params.items():
        jitters += [(lambda name=name, col=col: _ulp_step(name, col), first, torch.add) for col in range(t[0].numel())]
    for make, into, fold in jitters:
        o64, _ = _evaluate(s, cot, torch.float64, make())
        o32, _ = _evaluate(s, cot, torch.float32, make())
        for k in floats:
            into[k] = fold(into[k], (o64[k] - out[k]).abs())
            # a neighbour on the other side of an integer decision (a radius, the clamp) is another Gaussian, not another realisation
            same = ((o64["radii"] == out["radii"]) & (o32["radii"] == out["radii"])).reshape((-1,) + (1,) * (out[k].dim() - 1))
            a[k] = torch.where(same, torch.maximum(a[k], (o32[k].double() - o64[k]).abs()), a[k])
    return a, {k: torch.maximum(b[k], first[k]) for k in floats}


@dataclass
class Reference:
    scene: Scene
    cot: Optional[dict]
    out: Dict[str, torch.Tensor]          # fp64 (integers: int32 / int64)
    out32: Dict[str, torch.Tensor]        # the fp32 oracle's outputs: a faithful fp32 implementation
    unit: Dict[str, torch.Tensor]         # max(a, b, c) per entry of every float output
    terms: Dict[str, tuple]               # (a, b, c) themselves: compare() reports them for the worst entry
    edge: torch.Tensor
    edge_raw: torch.Tensor                # oracle.project_edge before the cut to Scene.may_be_edge
    clamp_edge: torch.Tensor
    normal_tie: torch.Tensor
    tight_near: torch.Tensor              # tight_near() of the fp64 projection (cfg.tight_tiles; all False otherwise)

    def shares(self):
        return {k: float(getattr(self, k).float().mean()) if self.scene.N else 0.0 for k in ("edge", "clamp_edge", "normal_tie")}


def reference(s: Scene, cot=None) -> Reference:
    cfg = s.cfg
    out, masks = _evaluate(s, cot, torch.float64)
    out32, _ = _evaluate(s, cot, torch.float32)
    floats = [k for k in FWD_KEYS + GEO_KEYS + SH_KEYS if k in out]
    a, b = unit_terms(s, cot, out, out32, floats)
    c = {k: EPS32 * out[k].abs() for k in floats}
    terms = {k: (a[k], b[k], c[k]) for k in floats}
    unit = {k: torch.maximum(torch.maximum(a[k], b[k]), c[k]) for k in floats}
    sc = s.scales.double()
    sc = torch.exp(sc) if cfg.scales_are_log else sc
    edge = orc.project_edge(s.means.double(), s.quats.double(), sc, s.viewmat.double(), s.K.double(), W, H, cfg.eps2d, cfg.near_plane,
                            cfg.far_plane, cfg.radius_clip, TILE)
    edge_raw = edge
    if s.may_be_edge is not None:
        # constructed boundary scenes: only the members deliberately put on the boundary may be excluded; all others are judged
        edge = edge & s.may_be_edge
    tnear = torch.zeros(s.N, dtype=torch.bool)
    if cfg.tight_tiles:
        tnear = tight_near(out["means2d"], out["conics"], out["splats"][:, 5], out["radii"])
    return Reference(s, cot, out, out32, unit, terms, edge, edge_raw, masks["clamp_edge"], masks["normal_tie"], tnear)


# -------------------------------------------------------------------------------------------------------------------- the comparator


def _excluded(ref: Reference, key: str, shape):
    """bool mask (shape of the output) of entries no verdict is possible on."""
    s, cfg = ref.scene, ref.scene.cfg
    N = s.N
    ex = ref.edge.clone()
    sh = cfg.sh_degree >= 0
    if key in ("v_sh0", "v_shN", "v_coeffs", "v_means") and sh:
        ex = ex | ref.clamp_edge
    if key == "normals_world" or (key == "v_quats" and cfg.with_normals):
        ex = ex | ref.normal_tie
    m = ex.reshape((N,) + (1,) * (len(shape) - 1)).expand(shape).clone()
    if key == "splats":
        ch = n_channels(s)
        if sh:
            m[:, 6:9] |= ref.clamp_edge[:, None]
        if cfg.with_normals:
            c0 = 6 + ch + (1 if cfg.with_depth else 0)
            m[:, c0:c0 + 3] |= ref.normal_tie[:, None]
    return m


def tight_near(m2d, con, opac, rad):
    """bool [N]: the Gaussians whose tight box hinges on the last places of logf / sqrtf: a box edge (m +- h - 0.5) / 16 within
    1e-5 (|m| + h + 1) / 16 of an integer."""
    m, c, o = m2d.double(), con.double(), opac.double()
    tau = torch.log((255.0 * o).clamp_min(1e-300))
    det = (c[:, 0] * c[:, 2] - c[:, 1] ** 2).clamp_min(1e-300)
    sfac = 2.0 * tau.clamp_min(0) / det
    rel = 1e-4 + 2.4e-7 * ((c[:, 0] * c[:, 2] + c[:, 1] ** 2) / det)
    hx = torch.sqrt(sfac * c[:, 2]) * (1 + rel) + 0.01
    hy = torch.sqrt(sfac * c[:, 0]) * (1 + rel) + 0.01
    near = torch.zeros_like(tau, dtype=torch.bool)
    for mm, hh in ((m[:, 0], hx), (m[:, 1], hy)):
        for v in ((mm - hh - (TILE - 0.5)) / TILE, (mm + hh - 0.5) / TILE):
            near |= (v - torch.round(v)).abs() <= 1e-5 * (mm.abs() + hh + 1.0) / TILE
    near |= (tau.abs() <= 1e-5) | ((tau - 2e-3).abs() <= 1e-5)
    return near & (rad > 0)


def tight_reference(got, s: Scene):
    """oracle.tight_tile_boxes on the kernel's OWN projection (fp32, the kernel's operation order) and tight_near() of that projection."""
    m2d, con, rad = got["means2d"], got["conics"], got["radii"]
    opac = got["splats"][:, 5]
    return orc.tight_tile_boxes(m2d, con, opac, rad, TILE, TW, TH), tight_near(m2d, con, opac, rad)


def compare(got: Dict[str, torch.Tensor], ref: Reference, k: Dict[str, float], skip_culled_records=False):
    """-> (failures, ratios, worst).  ``got``: CPU tensors under the keys of ``ref.out`` (the float keys absent from it are not compared, the
    integer keys must all be there).  ``k``: dict(fwd=, geo=, sh=).  ratios: the worst |got - fp64| / unit per group over the judged entries;
    worst: per group the entry that ratio comes from — key, index, got, want and the three terms a, b, c of its unit."""
    s, cfg = ref.scene, ref.scene.cfg
    N = s.N
    fails = []
    ratios = dict(fwd=0.0, geo=0.0, sh=0.0)
    worst = {}
    rad = got["radii"].reshape(N)
    gvis = rad > 0
    rvis = ref.out["radii"] > 0
    judged = ~ref.edge

    # ---- integers: exact outside `edge`
    def int_eq(name, a, b, rows):
        bad = (a.long() != b.long())
        bad = bad.reshape(N, -1).any(-1) & rows
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            fails.append(f"{name}: {int(bad.sum())} Gaussians differ from the fp64 decision, first {i}: got {a[i].tolist()} want {b[i].tolist()}")

    int_eq("radii", rad, ref.out["radii"], judged)
    int_eq("tiles_per_gauss", got["tiles_per_gauss"].reshape(N), ref.out["tiles_per_gauss"], judged)
    # ---- the boxes from the kernel's own centre and radius (every Gaussian, `edge` included)
    own = tile_boxes_3sigma(got["means2d"].reshape(N, 2), rad)
    own_count = (own[2] - own[0]) * (own[3] - own[1])
    int_eq("tiles_per_gauss vs the kernel's own means2d / radii", got["tiles_per_gauss"].reshape(N), own_count, torch.ones(N, dtype=torch.bool))
    boxes = got["tile_boxes"].reshape(N, 2).long()
    bw, bh = boxes[:, 1] & 0xffff, boxes[:, 1] >> 16
    tiles_bin = got["tiles_bin"].reshape(N).long()
    if bool((bw * bh != tiles_bin).any()):
        fails.append("tile_boxes: width x height differs from the count the binning is given")
    if bool((tiles_bin > got["tiles_per_gauss"].reshape(N).long()).any()):
        fails.append("tiles_bin exceeds tiles_per_gauss")
    if cfg.tight_tiles:
        (tx0, ty0, tx1, ty1), tnear = tight_reference(got, s)
        # the exclusion is computed from the kernel's own projection, so it is held to the input's: the fp64 projection's mask (capped
        # on the CPU, tests/test_projection_scenes.py) plus the `edge` Gaussians, whose projection may be the other decision's
        if int((tnear & ~ref.edge).sum()) > int(ref.tight_near.sum()) + max(1, math.ceil(TIGHT_NEAR_CAP * N)):
            fails.append(f"tile_boxes (tight): {int(tnear.sum())} boxes excluded as hinging on the last place, the fp64 projection has {int(ref.tight_near.sum())}")
        want = pack_boxes(tx0, ty0, tx1, ty1).long()
        empty = ((tx1 - tx0) * (ty1 - ty0) == 0)      # an empty box: only the count is defined, not its first tile
        bad = ((boxes[:, 1] != want[:, 1]) | ((boxes[:, 0] != want[:, 0]) & ~empty)) & ~tnear
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            fails.append(f"tile_boxes (tight): {int(bad.sum())} differ from oracle.tight_tile_boxes, first {i}: {boxes[i].tolist()} vs {want[i].tolist()}")
        # inside gsplat's box, for every Gaussian
        bx0, by0 = boxes[:, 0] % TW, boxes[:, 0] // TW
        inside = (bx0 >= own[0]) & (bx0 + bw <= own[2]) & (by0 >= own[1]) & (by0 + bh <= own[3])
        if bool((~inside & gvis & (bw * bh > 0)).any()):
            fails.append("tile_boxes (tight): a box leaves gsplat's 3-sigma box")
    else:
        int_eq("tile_boxes vs the kernel's own means2d / radii", boxes, pack_boxes(*own), torch.ones(N, dtype=torch.bool))
        int_eq("tile_boxes", boxes, ref.out["tile_boxes"], judged)
    # ---- `edge`: either decision, but a consistent one — a culled Gaussian is all zeros
    cull_e = ref.edge & ~gvis
    for key, t in got.items():
        if key == "normals_world" or t is None or (key == "splats" and skip_culled_records):
            continue
        rows = t.reshape(N, -1)[cull_e]
        if rows.numel() and bool((rows != 0).any()):
            fails.append(f"{key}: an `edge` Gaussian the kernel culled has a non-zero output")

    # ---- floats
    def group_of(key):
        return "fwd" if key in FWD_KEYS else ("geo" if key in GEO_KEYS else "sh")

    for key in FWD_KEYS + GEO_KEYS + SH_KEYS:
        if key not in ref.out or got.get(key) is None:
            continue
        want, unit = ref.out[key], ref.unit[key]
        g = got[key].reshape(want.shape).double()
        ex = _excluded(ref, key, want.shape)
        if key == "splats" and skip_culled_records:
            ex = ex | (~rvis)[:, None]
        err = (g - want).abs()
        # a NaN never passes: not (err <= bound)
        grp = group_of(key)
        ok = (err <= k[grp] * unit) | ex
        ratio = torch.where(unit > 0, err / unit, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        ratio = torch.where(ex, torch.zeros_like(ratio), torch.nan_to_num(ratio, nan=float("inf")))
        if ratio.numel() and float(ratio.max()) > ratios[grp]:
            ratios[grp] = float(ratio.max())
            i = tuple(int(x) for x in np.unravel_index(int(ratio.argmax()), ratio.shape))
            ta, tb, tc = (float(x[i]) for x in ref.terms[key])
            worst[grp] = dict(key=key, index=i, ratio=ratios[grp], got=float(g[i]), want=float(want[i]), a=ta, b=tb, c=tc)
        if not bool(ok.all()):
            bad = torch.nonzero(~ok)
            i = tuple(bad[0].tolist())
            fails.append(f"{key}: {bad.shape[0]} entries beyond {k[grp]} x unit, first {i}: got {float(g[i]):.9g} want {float(want[i]):.9g} "
                         f"unit {float(unit[i]):.3g} (ratio {float(ratio[i]):.3g})")
    return fails, ratios, worst


def as_got(out: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Reference-shaped outputs (``Reference.out32``) in the form ``compare`` takes from a kernel run."""
    return {k: v.clone() for k, v in out.items()}


def with_cfg(s: Scene, **kw) -> Scene:
    return replace(s, cfg=replace(s.cfg, **kw))


# ------------------------------------------------------------------------------------------------------------------- the catalogue


def base_cfg(**kw) -> ProjCfg:
    return ProjCfg(width=W, height=H, **kw)


FULL = dict(sh_degree=3, scales_are_log=True, opacities_are_logit=True)
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 1000)
SH_LAYOUTS = ("split", "cat", "split_unaligned", "cat_unaligned")


def _some_culled(N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, generator=g) < 0.3 if N > 2 else torch.zeros(N, dtype=torch.bool)


def catalogue():
    """name -> (builder, layouts): every scene of the projection edge tests.  Layouts: SH_LAYOUTS entries for SH scenes, ("colors",) for
    direct colours.  Constructed boundary scenes carry ``may_be_edge``."""
    c = {}
    for N in SIZES:
        c[f"n{N}"] = (lambda N=N: random_scene(N, base_cfg(**FULL, with_depth=True), seed=N, culled=_some_culled(N, N)), ("split", "cat"))
    for p in PATTERNS:
        c["pattern_" + p] = (lambda p=p: pattern_scene(p, base_cfg(**FULL), seed=3), SH_LAYOUTS)
    for deg in (0, 1, 2):
        c[f"degree{deg}"] = (lambda deg=deg: random_scene(200, base_cfg(sh_degree=deg, scales_are_log=True), seed=20 + deg,
                                                         culled=_some_culled(200, 5)), SH_LAYOUTS)
        c[f"degree{deg}_k9"] = (lambda deg=deg: random_scene(130, base_cfg(sh_degree=deg), seed=30 + deg, culled=_some_culled(130, 6), sh_K=9),
                                ("split", "cat"))
    for C in (1, 3, 4):
        for logit in (False, True):
            c[f"colors{C}" + ("_logit" if logit else "")] = (
                lambda C=C, logit=logit: random_scene(130, base_cfg(colors_are_logit=logit, with_depth=True, with_normals=(C != 3), want_normals_world=True),
                                                      seed=40 + C, culled=_some_culled(130, 7), n_colors=C), ("colors",))
    for aa in (False, True):
        for lg in (False, True):
            for lo in (False, True):
                c[f"modes_aa{int(aa)}_log{int(lg)}_logit{int(lo)}"] = (
                    lambda aa=aa, lg=lg, lo=lo: random_scene(200, base_cfg(sh_degree=3, antialiased=aa, scales_are_log=lg, opacities_are_logit=lo,
                                                                           with_depth=lg, with_normals=lo, want_normals_world=aa),
                                                             seed=50, culled=_some_culled(200, 8)), ("split",))
    c["depth_boundary"] = (lambda: depth_boundary_scene(base_cfg(sh_degree=3, near_plane=1.0, far_plane=8.0)), ("split", "cat"))
    c["depth_boundary_eps0"] = (lambda: depth_boundary_scene(base_cfg(sh_degree=3, near_plane=1.0, far_plane=8.0, eps2d=0.0)), ("split",))
    c["radius_clip_eps0"] = (lambda: radius_clip_scene(base_cfg(sh_degree=3, radius_clip=7.0, eps2d=0.0)), ("split",))
    # the record's channel positions: with_depth x with_normals x want_normals_world, crossed, for SH colours and 1, 3, 4 direct ones
    # (4 colours + depth + normal = 8 channels: the limit)
    for C in (0, 1, 3, 4):
        for d in (False, True):
            for n in (False, True):
                for w in (False, True):
                    c[f"channels_{'sh' if C == 0 else 'c%d' % C}_d{int(d)}_n{int(n)}_w{int(w)}"] = (
                        lambda C=C, d=d, n=n, w=w: random_scene(70, base_cfg(sh_degree=3 if C == 0 else -1, with_depth=d, with_normals=n,
                                                                            want_normals_world=w), seed=45, culled=_some_culled(70, 11),
                                                                n_colors=max(C, 1)), ("cat",) if C == 0 else ("colors",))
    c["radius_clip"] = (lambda: radius_clip_scene(base_cfg(sh_degree=3, radius_clip=7.0)), ("split",))
    c["frustum"] = (lambda: frustum_scene(base_cfg(sh_degree=3)), ("split",))
    c["singular_eps0.3"] = (lambda: singular_scene(base_cfg(sh_degree=3, antialiased=True)), ("split",))
    c["singular_eps0"] = (lambda: singular_scene(base_cfg(sh_degree=3, eps2d=0.0)), ("split",))
    c["frustum_eps0"] = (lambda: frustum_scene(base_cfg(sh_degree=3, eps2d=0.0)), ("split",))
    c["border"] = (lambda: border_scene(base_cfg(sh_degree=3)), ("split",))
    c["border_tight"] = (lambda: border_scene(base_cfg(sh_degree=3, tight_tiles=True)), ("split",))
    c["random_tight"] = (lambda: random_scene(300, base_cfg(**FULL, tight_tiles=True, antialiased=True), seed=60, culled=_some_culled(300, 9)), ("cat",))
    return c


CONSTRUCTED = ("depth_boundary", "radius_clip", "depth_boundary_eps0", "radius_clip_eps0", "frustum", "singular_eps0.3", "singular_eps0", "frustum_eps0", "border", "border_tight")
ALL_ROUTES = dict(means2d=True, depths=True, conics=True, compensations=True)
