"""The reference's Gaussian density field in plain PyTorch, restated from its behaviour (dn_splatter/dn_model.py:1061-1135
``get_closest_gaussians`` / ``get_density``, :1449-1494 ``get_density_grad``, :1603-1611 ``scale_rot_to_inv_cov3d``; utils/knn.py:29-43
``knn_sk``; export_mesh.py:430-457 the ``density_grad`` branch of the point-cloud exporter, :740-773 the lattice of the marching-cubes
exporter).

``knn`` is the brute force: sklearn ranks the exactly converted fp32 coordinates in fp64, so the squared distances are formed in
double and sorted stably (ties in ascending index), whatever dtype the caller computes the field in.  ``knn_sk`` asks for ``k + 1``
neighbours and drops the first, for ANY queries: ``closest`` therefore returns ranks 1 .. 16, which ``skip=1`` spells out.  The field
formulas are dtype-generic: float64 is the yardstick of the tests, float32 the baseline of ``tools/density_time.py``.  Pinned to the
reference's own code by tests/golden/reference_density.npz.  ``density.py`` is the HIP path."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor

from .legacy import quat_to_rotmat
from .torch_export import export_c2w, camera_points, within

KNN = 16            # get_closest_gaussians: knn_sk(..., k=16)
SKIP = 1            # knn_sk's dropped first column


def squared_distances(points: Tensor, queries: Tensor) -> Tensor:
    """[M,N] in float64 from the coordinates as given (fp32 converts exactly): (dx dx + dy dy) + dz dz."""
    d = queries.double()[:, None, :] - points.double()[None, :, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def knn(points: Tensor, queries: Tensor, k: int, skip: int = 0, return_d2: bool = False, chunk: int = 4096):
    """int64 [M,k]: the neighbours of rank ``skip .. skip + k - 1`` of every query among ``points`` by (d², index) ascending, d² in
    float64.  A query with a non-finite coordinate gets a row of -1.  ``k + skip > N`` raises, as sklearn does."""
    N, M = points.shape[0], queries.shape[0]
    if k < 1 or skip < 0 or k + skip > N:
        raise ValueError(f"knn: k = {k}, skip = {skip} for {N} points (sklearn: n_neighbors <= n_samples_fit)")
    idx = torch.empty(M, k, dtype=torch.int64, device=points.device)
    d2 = torch.empty(M, k, dtype=torch.float64, device=points.device)
    for i in range(0, M, chunk):
        dist = squared_distances(points, queries[i:i + chunk])
        bad = ~torch.isfinite(queries[i:i + chunk]).all(dim=-1)
        dist[bad] = 0.0
        val, order = torch.sort(dist, dim=1, stable=True)
        idx[i:i + chunk] = order[:, skip:skip + k]
        d2[i:i + chunk] = val[:, skip:skip + k]
        idx[i:i + chunk][bad] = -1
        d2[i:i + chunk][bad] = float("nan")
    return (idx, d2) if return_d2 else idx


def closest(means: Tensor, samples: Tensor) -> Tensor:
    """``get_closest_gaussians``: int64 [M,16], ranks 1 .. 16 of 17."""
    return knn(means, samples, KNN, SKIP)


def inv_scaled_rotation(scales: Tensor, quats: Tensor) -> Tensor:
    """``scale_rot_to_inv_cov3d(exp(scales), quats, return_sqrt=True)``: M = R(q / |q|) diag(1 / clamp(exp(s), 1e-3)), [...,3,3]."""
    s = 1.0 / torch.exp(scales).clamp(min=1e-3)
    return quat_to_rotmat(quats) * s[..., None, :]


def _mahalanobis(means, scales, quats, samples, closest_gaussians):
    M_ = inv_scaled_rotation(scales[closest_gaussians], quats[closest_gaussians])
    dist = samples[:, None, :] - means[closest_gaussians]
    man = M_.transpose(-1, -2) @ dist[..., None]
    m2 = (man[..., 0] * man[..., 0]).sum(dim=-1).clamp(min=0.0, max=1e8)
    return M_, man, m2


def density_sum(means, scales, quats, opacities, samples, closest_gaussians) -> Tensor:
    """The sum of o exp(-m² / 2) over the neighbours, before the ``>= 1`` switch and the clamp ([M])."""
    _, _, m2 = _mahalanobis(means, scales, quats, samples, closest_gaussians)
    return (torch.sigmoid(opacities[closest_gaussians])[..., 0] * torch.exp(-1.0 / 2 * m2)).sum(dim=-1)


def density(means, scales, quats, opacities, samples, closest_gaussians: Optional[Tensor] = None) -> Tensor:
    """``get_density`` ([M]); ``opacities`` [N,1] logits, ``scales`` [N,3] logs."""
    if closest_gaussians is None:
        closest_gaussians = closest(means, samples)
    d = density_sum(means, scales, quats, opacities, samples, closest_gaussians)
    d = torch.where(d >= 1.0, d / (d + 1e-5), d)
    return d.clamp(min=1e-4)


def density_grad(means, scales, quats, samples, num_closest_gaussians: Optional[int] = None,
                 closest_gaussians: Optional[Tensor] = None) -> Tensor:
    """``get_density_grad`` ([M,3]): minus the normalised sum of m² M (Mᵀ (x - mu)) over the first ``num_closest_gaussians``."""
    if closest_gaussians is None:
        closest_gaussians = closest(means, samples)
    if num_closest_gaussians is not None:
        assert num_closest_gaussians >= 1
        closest_gaussians = closest_gaussians[..., :num_closest_gaussians]
    M_, man, m2 = _mahalanobis(means, scales, quats, samples, closest_gaussians)
    g = (m2[..., None] * (M_ @ man)[..., 0]).sum(dim=-2)
    return -F.normalize(g, dim=-1)


def lattice(resolution: int, radius: float, device="cpu"):
    """export_mesh.py:740-744: (X, Y, Z, grid_coords [R³,3]) of the marching-cubes exporter, float32."""
    X = torch.linspace(-1, 1, resolution, device=device) * radius
    xx, yy, zz = torch.meshgrid(X, X, X, indexing="ij")
    return X, X.clone(), X.clone(), torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3)


def density_volume(means, scales, quats, opacities, resolution: int, radius: float, crop_box=None) -> Tensor:
    """export_mesh.py:740-773: the [R,R,R] density lattice, -1e6 outside the crop box."""
    _, _, _, grid = lattice(resolution, radius, means.device)
    grid = grid.to(means.dtype)
    mask = within(crop_box, grid) if crop_box is not None else torch.ones(grid.shape[0], dtype=torch.bool, device=grid.device)
    flat = torch.zeros(grid.shape[0], dtype=means.dtype, device=means.device)
    flat[mask] = density(means, scales, quats, opacities, grid[mask])
    vol = flat.reshape(resolution, resolution, resolution)
    if crop_box is not None:
        vol[~mask.reshape(vol.shape)] = -1e6
    return vol


def density_grad_samples(depth: Tensor, camera):
    """export_mesh.py:370-375, :431-441: (xyz [H W, 3], c2w [3,4]) — every pixel back-projected at 0.99 of its depth with the OpenCV pose."""
    c2w = export_c2w(camera.camera_to_worlds.to(depth.dtype))
    W, H = int(camera.width), int(camera.height)
    xyz = camera_points(depth * 0.99, camera.fx, camera.fy, camera.cx, camera.cy, (W, H)) @ torch.linalg.inv(c2w[:3, :3]) + c2w[:3, 3]
    return xyz, c2w


def orient_normals(n: Tensor, xyz: Tensor, c2w: Tensor) -> Tensor:
    """export_mesh.py:445-456: flipped towards the camera, times the camera rotation and diag(1, -1, -1), normalised."""
    view = -xyz + c2w[:3, 3]
    view = view / view.norm(dim=-1, keepdim=True)
    n = torch.where(((n * view).sum(-1) < 0)[:, None], -n, n)
    n = (n @ c2w[:3, :3]) @ torch.diag(torch.tensor([1, -1, -1], device=n.device, dtype=n.dtype))
    return n / n.norm(dim=-1, keepdim=True)


def density_grad_normals(means, scales, quats, depth: Tensor, camera) -> Tensor:
    """export_mesh.py:430-457: the normals [H W, 3] the ``density_grad`` branch computes for a frame — the density gradient of the
    second-nearest Gaussian (``num_closest_gaussians=1`` of ``knn_sk``'s columns) at the samples above, oriented.  (The reference then
    overwrites the result with the rendered normal map, :459.)"""
    xyz, c2w = density_grad_samples(depth, camera)
    return orient_normals(density_grad(means, scales, quats, xyz, num_closest_gaussians=1), xyz, c2w)
