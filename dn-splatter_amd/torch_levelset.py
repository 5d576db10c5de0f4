"""The reference's level-set ray search in plain PyTorch, restated from its rule (dn_splatter/dn_model.py:1206-1447
``DNSplatterModel.compute_level_surface_points``, the per-camera hot path of export_mesh.py:514-697 ``LevelSetExtractor``).

Per pixel i = v W + u in raster order: d = depth (0 outside the mask); d <= 0 takes no part, and neither does a non-finite d (our
choice: the reference would raise inside sklearn); p = the world point of ``torch_export.get_colored_points_from_depth``, ALWAYS formed
in float32 — the rule states it bit-equal, so it is an input of everything downstream — and then taken into the working dtype;
o = the camera position; dir = normalize(p - o); the neighbours are ``knn_sk(means, p, 16)``, ranks 1 .. 16 of 17; c = the first of them;
std = | exp(s_c) * (R(q_c / |q_c|)ᵀ w) | with w = (o - mu_c) / |o - mu_c|; the 21 samples x_j = p + (r_j std) dir with r the float32
values of ``torch.linspace(-3, 3, 21)``; D_j = the density sum over the 16 neighbours of p, D_j / (D_j + 1e-5) from 1 on, no floor; per
level L (rounded to float32, as the reference's float32 tensors meet the Python number): a = the first j with D_j > L, empty unless
D_0 < L and a >= 1; t = ((L - D_{a-1}) / (D_a - D_{a-1})) (T_a - T_{a-1}) + T_{a-1}, T_j = r_j std; the point p + t dir; the normal row c
of the model's ``normals`` ("closest_gaussian") or -normalize(sum_k w_k M_k M_kᵀ (x - mu_k)) with w_k the neighbour's density term
("analytical").

Everything after p is computed in the dtype of ``means``: float64 is the yardstick of the tests, float32 the CPU path of
``levelset.install_level_sets`` and the baseline of ``tools/level_set_time.py``.  Pinned to the reference's own code by
tests/golden/reference_levelset.npz.  ``levelset.py`` is the HIP path."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn.functional as F
from torch import Tensor

from .legacy import quat_to_rotmat
from .torch_density import KNN, SKIP, _mahalanobis, knn
from .torch_export import export_c2w, get_colored_points_from_depth, within

RANGE_SIZE = 3              # dn_model.py:1277
RANGE_POINTS = 21           # :1278, include/dnsplat.h DNSPLAT_LEVEL_RANGE_POINTS
NORMAL_MODES = ("closest_gaussian", "analytical")


def range_table(device="cpu") -> Tensor:
    """The 21 float32 values of ``torch.linspace(-3, 3, 21)`` (:1282-1286): torch's own, formed on the host and then moved, as the
    reference's ``.to(self.device)`` does."""
    return torch.linspace(-RANGE_SIZE, RANGE_SIZE, RANGE_POINTS).to(device)


def level_value(level: float, dtype) -> Tensor:
    """A surface level as the reference's float32 tensors see it, in ``dtype``."""
    return torch.tensor(float(level), dtype=torch.float32).to(dtype)


def ray_std(means: Tensor, scales: Tensor, quats: Tensor, origin: Tensor, idx: Tensor) -> Tensor:
    """:1266-1275 for the Gaussians ``idx`` only: | exp(s) * (R(q / |q|)ᵀ w) |, w the unit vector from the mean to the camera."""
    w = origin - means[idx]
    w = w / w.norm(dim=-1, keepdim=True)
    q = quats[idx] / quats[idx].norm(dim=-1, keepdim=True)
    conj = torch.cat([q[..., :1], -q[..., 1:]], dim=-1)                # invert_quaternion: (w, -x, -y, -z)
    return (torch.exp(scales[idx]) * (quat_to_rotmat(conj) @ w[..., None])[..., 0]).norm(dim=-1)


def _terms(means, scales, quats, opacities, samples, neighbors):
    """(M, Mᵀ (x - mu), o exp(-m² / 2)) per sample and neighbour."""
    M_, man, m2 = _mahalanobis(means, scales, quats, samples, neighbors)
    return M_, man, torch.sigmoid(opacities.reshape(-1)[neighbors]) * torch.exp(-1.0 / 2 * m2)


def world_points(depth: Tensor, camera_to_worlds: Tensor, fx, fy, cx, cy, width: int, height: int, mask: Optional[Tensor] = None):
    """(d [P] float32 with the mask applied, p [P,3] float32): the back-projection of every pixel, in float32 whatever comes in."""
    d = depth.reshape(-1).float()
    if mask is not None:
        d = torch.where(mask.reshape(-1).bool(), d, torch.zeros_like(d))
    c2w = export_c2w(camera_to_worlds.reshape(3, 4).float())
    rgb = torch.zeros(d.numel(), 3, dtype=torch.float32, device=d.device)
    p, _ = get_colored_points_from_depth(d.reshape(height, width, 1), rgb, c2w, fx, fy, cx, cy, (width, height))
    return d, p


def level_rays(means: Tensor, scales: Tensor, quats: Tensor, opacities: Tensor, depth: Tensor, camera_to_worlds: Tensor, fx, fy, cx, cy,
               width: int, height: int, mask: Optional[Tensor] = None, surface_levels: Sequence[float] = (0.1, 0.3, 0.5),
               points: Optional[Tensor] = None, neighbors: Optional[Tensor] = None) -> dict:
    """The rule for every pixel of a frame, in the dtype of ``means``.  ``points`` [P,3] float32 replaces the back-projection (the HIP
    kernel's own, for a comparison downstream of it), ``neighbors`` [P,16] the search.  Returns, for all P pixels (n_levels first where a
    value is per level): ``part`` bool [P]; ``points``, ``dir`` [P,3]; ``closest`` int64 [P,16] (-1 where the pixel took no part);
    ``std`` [P]; ``densities`` [P,21] (nan there) and ``sums`` [P,21], the same before the ``>= 1`` switch; ``first_above`` int64 [L,P] (0 where empty); ``empty`` bool [L,P]; ``t`` [L,P] (nan
    where empty); ``hit_points``, ``normals`` (analytical) [L,P,3]; ``kappa``, ``dT`` [L,P]: the interpolation's condition number
    (|D_a| + |D_{a-1}| + L) / |D_a - D_{a-1}| and its bracket T_a - T_{a-1}; ``levels`` [L] as used."""
    dtype, dev = means.dtype, means.device
    P, nl = width * height, len(surface_levels)
    d, p32 = world_points(depth, camera_to_worlds, fx, fy, cx, cy, width, height, mask)
    if points is not None:
        p32 = points.reshape(P, 3).float()
    part = (d > 0) & torch.isfinite(d) & torch.isfinite(p32).all(dim=-1)
    if neighbors is None:
        nb = knn(means.float(), p32[part], KNN, SKIP)
    else:
        if means.shape[0] < KNN + SKIP:
            raise ValueError(f"level sets need at least {KNN + SKIP} Gaussians, got {means.shape[0]}")
        nb = neighbors.reshape(P, KNN)[part].long()
    n = int(part.sum())
    pts = p32[part].to(dtype)
    origin = camera_to_worlds.reshape(3, 4)[:, 3].to(dtype)
    dirs = F.normalize(pts - origin, dim=-1)
    std = ray_std(means, scales, quats, origin, nb[:, 0]) if n else pts.new_zeros(0)
    T = range_table(dev).to(dtype)[None, :] * std[:, None]                                     # [n,21]
    samples = pts[:, None, :] + T[..., None] * dirs[:, None, :]
    nb21 = nb[:, None, :].expand(-1, RANGE_POINTS, -1).reshape(-1, KNN)
    sums = _terms(means, scales, quats, opacities, samples.reshape(-1, 3), nb21)[2].sum(dim=-1).reshape(n, RANGE_POINTS)
    D = torch.where(sums >= 1.0, sums / (sums + 1e-5), sums)

    nan = float("nan")
    out = dict(part=part, points=torch.full((P, 3), nan, dtype=dtype, device=dev), dir=torch.full((P, 3), nan, dtype=dtype, device=dev),
               closest=torch.full((P, KNN), -1, dtype=torch.int64, device=dev), std=torch.full((P,), nan, dtype=dtype, device=dev),
               densities=torch.full((P, RANGE_POINTS), nan, dtype=dtype, device=dev),
               sums=torch.full((P, RANGE_POINTS), nan, dtype=dtype, device=dev),
               first_above=torch.zeros(nl, P, dtype=torch.int64, device=dev), empty=torch.ones(nl, P, dtype=torch.bool, device=dev),
               t=torch.full((nl, P), nan, dtype=dtype, device=dev), hit_points=torch.full((nl, P, 3), nan, dtype=dtype, device=dev),
               normals=torch.full((nl, P, 3), nan, dtype=dtype, device=dev), kappa=torch.full((nl, P), nan, dtype=dtype, device=dev),
               dT=torch.full((nl, P), nan, dtype=dtype, device=dev),
               levels=torch.stack([level_value(L, dtype) for L in surface_levels]).to(dev))
    out["points"][part], out["dir"][part], out["closest"][part], out["std"][part], out["densities"][part] = pts, dirs, nb, std, D
    out["sums"][part] = sums
    steps = torch.arange(RANGE_POINTS, device=dev)
    for l in range(nl):
        L = out["levels"][l]
        first = torch.where(D > L, steps[None, :], torch.full_like(steps, RANGE_POINTS)[None, :]).min(dim=-1).values
        empty = ~(D[:, 0] < L) | (first == RANGE_POINTS) | (first == 0)
        a = torch.where(empty, torch.ones_like(first), first)[:, None]
        Da, Db = D.gather(1, a)[:, 0], D.gather(1, a - 1)[:, 0]
        Ta, Tb = T.gather(1, a)[:, 0], T.gather(1, a - 1)[:, 0]
        t = (L - Db) / (Da - Db) * (Ta - Tb) + Tb
        x = pts + t[:, None] * dirs
        M_, man, w = _terms(means, scales, quats, opacities, torch.where(empty[:, None], pts, x), nb)
        normal = -F.normalize((w[..., None] * (M_ @ man)[..., 0]).sum(dim=-2), dim=-1)
        keep = ~empty
        for key, val in (("t", t), ("hit_points", x), ("normals", normal), ("kappa", (Da.abs() + Db.abs() + L) / (Da - Db).abs()),
                         ("dT", Ta - Tb)):
            full = out[key][l]
            full[part] = torch.where(keep.reshape((-1,) + (1,) * (val.dim() - 1)), val, torch.full_like(val, nan))
        out["first_above"][l][part] = torch.where(keep, first, torch.zeros_like(first))
        out["empty"][l][part] = empty
    return out


def level_surface_points(means, scales, quats, opacities, normals, outputs, camera, num_samples: int, mask: Optional[Tensor] = None,
                         surface_levels: Sequence[float] = (0.1, 0.3, 0.5), return_normal: str = "closest_gaussian", seed: int = 0,
                         crop_box=None) -> dict:
    """``compute_level_surface_points`` for the rendered ``outputs`` (depth, rgb) of ``camera``: {level: {"points", "normals",
    "colors"}}, the reference's return shape.  With ``num_samples`` below the number of hits the rows are a uniform draw without
    replacement from a ``torch.Generator`` seeded with ``seed`` (the reference: Python's ``random.sample``); otherwise every hit in
    raster order.  ``crop_box`` keeps the hits ``torch_export.within`` it (after the draw, as the point-cloud exporter crops)."""
    if return_normal not in NORMAL_MODES:
        raise NotImplementedError(f"return_normal = {return_normal!r}: the reference implements 'closest_gaussian' and 'analytical'")
    W, H = int(camera.width), int(camera.height)
    depth = outputs["depth"].to(means.dtype)
    r = level_rays(means, scales, quats, opacities, depth, camera.camera_to_worlds.to(depth.device), camera.fx, camera.fy, camera.cx,
                   camera.cy, W, H, mask, surface_levels)
    colors = outputs["rgb"].reshape(-1, 3)
    g = torch.Generator().manual_seed(int(seed))
    result = {}
    for l, level in enumerate(surface_levels):
        rows = torch.nonzero(~r["empty"][l]).reshape(-1)
        if num_samples < rows.numel():
            rows = rows[torch.randperm(rows.numel(), generator=g)[:num_samples].to(rows.device)]
        pts = r["hit_points"][l][rows]
        nrm = r["normals"][l][rows] if return_normal == "analytical" else normals[r["closest"][rows, 0]]
        col = colors[rows]
        if crop_box is not None:
            inside = within(crop_box, pts)
            pts, nrm, col = pts[inside], nrm[inside], col[inside]
        result[level] = {"points": pts, "normals": nrm, "colors": col}
    return result
