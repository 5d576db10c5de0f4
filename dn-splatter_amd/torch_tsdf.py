"""TSDF fusion in plain PyTorch: the restatement of ``csrc/tsdf.hip`` — the frames -> volume step of the reference's
``Open3DTSDFFusion`` exporter (dn_splatter/export_mesh.py:931-1047) and the colours of the mesh extracted from the volume.  No HIP; it
runs on whatever device its tensors are on, tensor-wide per camera, with the operations in the order the kernels perform them and no
fused ones: the HIP path (``tsdf.py``) is held to this file with exact equality.

THE RULE is restated from memory of Open3D's ``UniformTSDFVolume::Integrate`` as the exporter calls it (``depth_scale=1``, ``RGB8``,
``convert_rgb_to_intensity=False``).  IT IS THIS PROJECT'S DEFINITION, PARITY UNPINNED AGAINST Open3D, which is absent here.

Volume: ``tsdf`` and ``weight`` float32 [nx,ny,nz], ``color`` float32 [nx,ny,nz,3] or None; the sample point of voxel (i, j, k) is
``origin + voxel * (i, j, k)`` in float64 — the lattice coordinates of ``torch_marching``.  The caller zeroes the arrays once; calls
accumulate.  Per voxel, the cameras of a call in ascending order:

    1  p_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k in float64 (``torch_mesh_cull.opencv_w2c`` rows); skip if not p.z > 0
    2  uf = ((fx p.x) / p.z + cx) + pixel_offset, vf likewise, float64; skip unless 0.0001 <= uf < W - 0.0001 and 0.0001 <= vf < H - 0.0001
       (a NaN skips); u, v = uf, vf truncated.  pixel_offset 0.5: pixel centres at the integers (Open3D, the exporter as written);
       0.0: centres at + 0.5 (this library's renderer)
    3  d = depth[c, v, u]; skip if not d > 0 or d > depth_trunc (a NaN skips)
    4  float32: sdf = (d - float32(p.z)) * ray_scale[v, u]; skip if not sdf > -sdf_trunc; f = min(1, sdf / sdf_trunc);
       tsdf = (tsdf * w + f) / (w + 1); per channel q = trunc(min(max(rgb * 255, 0), 255)) (NaN -> 0; the exporter's uint8 cast),
       color = (color * w + q) / (w + 1); w = w + 1

``ray_scale`` [H,W] is Open3D's depth-to-camera-distance multiplier ``sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1)`` at integer
(u, v), computed once per intrinsics on the CPU in float64 and cast: a table, so that kernel and restatement read the same bytes.

``vertex_colors`` samples the colour volume at a vertex's lattice coordinates by the trilinear formula, base corner
``min(floor(x), n - 2)`` per axis (not below 0), fraction ``x - base``, blends ``(1 - f) a + f b`` in float32 along i, then j, then k,
and divides by 255.  On a lattice edge that is the linear blend of its two ends, exact at both.  A non-finite vertex gets zeros.

Out of scope: Open3D's connected-component filter (:1021-1039), vdbfusion's space carving and its ``min_weight=5`` beyond the
``min_weight`` of the extraction, sparse or hashed volumes, quadric decimation, PLY output, per-camera intrinsics within one call."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import torch_marching
from .torch_mesh_cull import _camera_space, intrinsics

PIXEL_MARGIN = 0.0001           # Open3D's image border
MAX_POINTS = torch_marching.MAX_POINTS


def ray_scale(K, height: int, width: int) -> Tensor:
    """float32 [H,W] on the CPU: sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1) in float64, then cast."""
    k = intrinsics(K)
    u = (torch.arange(int(width), dtype=torch.float64) - k[2]) / k[0]
    v = (torch.arange(int(height), dtype=torch.float64) - k[5]) / k[4]
    return torch.sqrt((u * u)[None, :] + (v * v)[:, None] + 1.0).to(torch.float32)


def voxel_points(dims, origin, voxel: float, device) -> Tensor:
    """float64 [nx,ny,nz,3]: origin + voxel * (i, j, k)."""
    axes = [float(origin[a]) + float(voxel) * torch.arange(int(dims[a]), dtype=torch.float64, device=device) for a in range(3)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)


def quantise(rgb: Tensor) -> Tensor:
    """trunc(min(max(rgb * 255, 0), 255)) in float32 with C's fmaxf / fminf on a NaN (-> 0): the values of the exporter's uint8 cast."""
    x = rgb.to(torch.float32) * torch.tensor(255.0, dtype=torch.float32, device=rgb.device)
    x = torch.where(x > 0, x, torch.zeros_like(x))
    x = torch.where(x < 255, x, torch.full_like(x, 255.0))
    return torch.trunc(x)


@torch.no_grad()
def integrate(tsdf: Tensor, weight: Tensor, color: Optional[Tensor], origin, voxel: float, w2c: Tensor, K, depth: Tensor,
              rgb: Optional[Tensor], scale: Tensor, sdf_trunc: float = 0.03, depth_trunc: float = 20.0,
              pixel_offset: float = 0.5) -> None:
    """The rule of the module docstring, IN PLACE on ``tsdf``, ``weight`` (float32 [nx,ny,nz]) and ``color`` ([nx,ny,nz,3] or None):
    ``w2c`` float64 [C,12], ``depth`` float32 [C,H,W], ``rgb`` float32 [C,H,W,3] or None (with ``color``: both or neither), ``scale`` =
    ``ray_scale(K, H, W)`` or any float32 [H,W] table."""
    if (color is None) != (rgb is None):
        raise ValueError("color and rgb are given together or not at all")
    dev = tsdf.device
    k = intrinsics(K)
    C, H, W = depth.shape
    x = voxel_points(tsdf.shape, origin, voxel, dev)
    f32 = lambda value: torch.tensor(value, dtype=torch.float32, device=dev)          # noqa: E731
    trunc, far, one = f32(sdf_trunc), f32(depth_trunc), f32(1.0)
    depth, scale = depth.to(torch.float32), scale.to(dev).to(torch.float32)
    for c in range(C):
        p = _camera_space(w2c[c].to(dev), x)
        pz = p[..., 2]
        ok = pz > 0
        uf = ((k[0] * p[..., 0]) / pz + k[2]) + pixel_offset
        vf = ((k[4] * p[..., 1]) / pz + k[5]) + pixel_offset
        ok = ok & (uf >= PIXEL_MARGIN) & (uf < W - PIXEL_MARGIN) & (vf >= PIXEL_MARGIN) & (vf < H - PIXEL_MARGIN)
        u = torch.where(ok, uf, torch.zeros_like(uf)).to(torch.int64)
        v = torch.where(ok, vf, torch.zeros_like(vf)).to(torch.int64)
        d = depth[c][v, u]
        ok = ok & (d > 0) & ~(d > far)
        sdf = (d - pz.to(torch.float32)) * scale[v, u]
        ok = ok & (sdf > -trunc)
        f = torch.minimum(one, sdf / trunc)
        w1 = weight + one
        tsdf.copy_(torch.where(ok, (tsdf * weight + f) / w1, tsdf))
        if color is not None:
            q = quantise(rgb[c])[v, u]                                                # [nx,ny,nz,3]
            color.copy_(torch.where(ok[..., None], (color * weight[..., None] + q) / w1[..., None], color))
        weight.copy_(torch.where(ok, w1, weight))


@torch.no_grad()
def vertex_colors(color: Tensor, vertices: Tensor) -> Tensor:
    """float32 [V,3]: the colour volume [nx,ny,nz,3] sampled at lattice-coordinate ``vertices`` [V,3] (float32), / 255."""
    dev = color.device
    x = vertices.to(dev).to(torch.float32)
    finite = torch.isfinite(x).all(dim=1)
    x = torch.where(finite[:, None], x, torch.zeros_like(x))
    hi = torch.tensor([n - 2 for n in color.shape[:3]], dtype=torch.float32, device=dev)
    base = torch.maximum(torch.minimum(torch.floor(x), hi), torch.zeros_like(hi))
    fr = x - base
    b = base.to(torch.int64)
    one = torch.tensor(1.0, dtype=torch.float32, device=dev)

    def corner(di, dj, dk):
        return color[b[:, 0] + di, b[:, 1] + dj, b[:, 2] + dk].to(torch.float32)

    def blend(a, c, f):
        return (one - f)[:, None] * a + f[:, None] * c

    along_i = [[blend(corner(0, dj, dk), corner(1, dj, dk), fr[:, 0]) for dk in (0, 1)] for dj in (0, 1)]
    along_j = [blend(along_i[0][dk], along_i[1][dk], fr[:, 1]) for dk in (0, 1)]
    out = blend(along_j[0], along_j[1], fr[:, 2]) / torch.tensor(255.0, dtype=torch.float32, device=dev)
    return torch.where(finite[:, None], out, torch.zeros_like(out))


def world_vertices(vertices: Tensor, origin, voxel: float) -> Tensor:
    """float64 [V,3]: origin + voxel * v, one product and one sum per component."""
    o = torch.tensor([float(c) for c in origin], dtype=torch.float64, device=vertices.device)
    return vertices.to(torch.float64) * float(voxel) + o


@torch.no_grad()
def extract_mesh(tsdf: Tensor, weight: Tensor, color: Optional[Tensor], origin, voxel: float,
                 min_weight: float = 0.0) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """(vertices float64 [V,3] in world coordinates, triangles int32 [T,3], colours float32 [V,3] or None) on the CPU: the zero level of
    ``tsdf`` over the voxels with ``weight > min_weight`` (``torch_marching.marching_cubes`` with ``observed``), ``world_vertices``,
    ``vertex_colors``."""
    seen = (weight.detach().cpu().to(torch.float32) > torch.tensor(min_weight, dtype=torch.float32)).numpy()
    v, t = torch_marching.marching_cubes(tsdf.detach().cpu().numpy(), 0.0, observed=seen)
    v, t = torch.from_numpy(v), torch.from_numpy(t)
    colors = None if color is None else vertex_colors(color.detach().cpu(), v)
    return world_vertices(v, origin, voxel), t, colors


def bounds_dims(lo, hi, voxel: float) -> Tuple[int, int, int]:
    """The lattice of an axis-aligned box: per axis ``ceil((hi - lo) / voxel) + 1`` points, at least 2 — the box's far face lies inside
    the last cell; the quotient is taken 1e-9 short, so that a box of a whole number of voxels does not gain a layer from rounding.
    ValueError at 2^31 points or more, naming the largest number of points that fits."""
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    if not (float(voxel) > 0 and np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError(f"need voxel_size > 0 and finite bounds with hi >= lo, got {voxel}, {lo.tolist()}, {hi.tolist()}")
    dims = tuple(max(int(np.ceil((hi[a] - lo[a]) / float(voxel) - 1e-9)) + 1, 2) for a in range(3))
    if dims[0] * dims[1] * dims[2] >= MAX_POINTS:
        raise ValueError(f"a volume of {dims} = {dims[0] * dims[1] * dims[2]} voxels: at most {MAX_POINTS - 1} (2^31 - 1) fit; "
                         "use a larger voxel_size or a smaller box")
    return dims
