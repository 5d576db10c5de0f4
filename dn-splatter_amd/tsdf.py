"""TSDF fusion on the device (``csrc/tsdf.hip``): the reference's ``gs-mesh o3dtsdf`` exporter (dn_splatter/export_mesh.py:931-1047,
``Open3DTSDFFusion``, the one its README recommends), which renders every training camera, copies depth and colour to the host and
fuses them on the CPU with Open3D — a library a ROCm box does not have.  Here the frames stay where they were rendered:

  * ``TSDFVolume``: a dense, bounded volume; ``integrate`` (``dnsplat_tsdf_integrate``, one launch per call whatever the number of
    frames) and ``extract_mesh`` (``dnsplat_mc_count_observed`` / ``dnsplat_mc_emit_observed`` — marching cubes over the voxels that
    were seen — and ``dnsplat_tsdf_vertex_colors``);
  * ``fuse_tsdf_mesh``: the exporter's loop (:961-1019) — render, mask, integrate ``batch`` frames per call, extract.  Its result feeds
    ``mesh_cull.cull_mesh`` and ``geometry.mesh_metrics`` unchanged, so render -> fuse -> mesh -> cull -> score stays on the GPU;
  * ``filter_clusters=`` of both: the exporter's last step (:1021-1039), Open3D's connected-component filter, through
    ``mesh_clusters.filter_small_clusters``.

The integration rule is restated from memory of Open3D's ``UniformTSDFVolume::Integrate``: IT IS THIS PROJECT'S DEFINITION, PARITY
UNPINNED AGAINST Open3D.  ``torch_tsdf`` states it in PyTorch, and the kernels are held to that file with exact equality.  Poses are
camera-to-world in the OpenGL convention, as ``mesh_cull`` takes them.

Out of scope: vdbfusion's space carving and its ``min_weight=5`` beyond the
``min_weight`` argument, sparse or hashed volumes (Open3D's ``ScalableTSDFVolume`` allocates blocks on demand; this volume is the box
it is given), quadric decimation, PLY output, per-camera intrinsics within one call.  CPU tensors are refused; there is no CPU
fallback."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._ops import _f32c, _need_gpu, _ptr, _stream, _tsdf_args
from .marching import MarchingBuffers, marching_cubes
from .mesh_clusters import _filter_arguments, filter_small_clusters
from .mesh_cull import _frame, _w2c
from .torch_mesh_cull import intrinsics
from .torch_tsdf import bounds_dims, ray_scale, world_vertices


class TSDFVolume:
    """``tsdf`` / ``weight`` float32 [nx,ny,nz] and, with ``color=True``, ``color`` float32 [nx,ny,nz,3] (0 ... 255) on ``device``,
    zeroed; the sample point of voxel (i, j, k) is ``origin + voxel_size * (i, j, k)``.  12 bytes per voxel without colour, 20 with.
    ``pixel_offset`` 0.5 is Open3D's pixel-centres-at-integers rule — the exporter as written; 0.0 matches this library's renderer,
    whose pixel centres are at + 0.5."""

    def __init__(self, origin, voxel_size: float, dims, sdf_trunc: float = 0.03, depth_trunc: float = 20.0, pixel_offset: float = 0.5,
                 color: bool = True, device="cuda"):
        self.origin = tuple(float(c) for c in np.asarray(origin, dtype=np.float64).reshape(3))
        self.voxel_size, self.sdf_trunc, self.depth_trunc = float(voxel_size), float(sdf_trunc), float(depth_trunc)
        self.pixel_offset = float(pixel_offset)
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 1:
            raise ValueError(f"dims must be three positive sizes, got {dims}")
        if self.dims[0] * self.dims[1] * self.dims[2] >= 2 ** 31:
            raise ValueError(f"a volume of {self.dims} has 2^31 voxels or more")
        if not (self.voxel_size > 0 and self.sdf_trunc > 0 and self.depth_trunc > 0):
            raise ValueError("voxel_size, sdf_trunc and depth_trunc must be positive")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DnsplatError(f"a TSDFVolume on {self.device}: TSDF fusion runs only on the GPU through libdnsplat.so (torch_tsdf is "
                                    "the PyTorch restatement; there is no CPU fallback)")
        self.tsdf = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
        self.color = torch.zeros(self.dims + (3,), dtype=torch.float32, device=self.device) if color else None
        self._ray_scale = {}                                # (k, H, W) -> the table on the device

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size: float, **kw) -> "TSDFVolume":
        """The volume of an axis-aligned box (the crop box's, say): origin ``lo``, ``ceil((hi - lo) / voxel_size) + 1`` points per axis.
        ValueError at 2^31 points or more, naming the largest count that fits."""
        return cls(lo, voxel_size, bounds_dims(lo, hi, voxel_size), **kw)

    def ray_scale(self, k: Tuple[float, ...], height: int, width: int) -> Tensor:
        key = (k, height, width)
        if key not in self._ray_scale:
            self._ray_scale[key] = ray_scale(k, height, width).to(self.device)
        return self._ray_scale[key]

    @torch.no_grad()
    def integrate(self, depth: Tensor, rgb: Optional[Tensor], poses, K) -> "TSDFVolume":
        """Fuses C frames: ``depth`` float32 [C,H,W] or [C,H,W,1], ``rgb`` float32 [C,H,W,3] (None for a volume without colour), ``poses``
        [C,4,4] camera-to-world (OpenGL), one ``K`` [3,3] for all of them (host values: a K on the device is read once).  One launch;
        nothing is read on the host.  Frames accumulate across calls, and C1 + C2 frames in two calls give the bytes of one call."""
        depth = _f32c(depth.detach(), "depth")
        if depth.dim() == 4 and depth.shape[-1] == 1:
            depth = depth[..., 0].contiguous()
        if depth.dim() != 3:
            raise ValueError(f"depth must be [C,H,W] or [C,H,W,1], got {tuple(depth.shape)}")
        C = depth.shape[0]
        height, width = _frame(depth.shape[1], depth.shape[2])
        if (rgb is None) != (self.color is None):
            raise ValueError("rgb is given exactly when the volume holds colour")
        if rgb is not None:
            rgb = _f32c(rgb.detach(), "rgb")
            if tuple(rgb.shape) != (C, height, width, 3):
                raise ValueError(f"rgb must be [{C},{height},{width},3], got {tuple(rgb.shape)}")
        w2c = _w2c(poses, self.device)
        if w2c.shape[0] != C:
            raise ValueError(f"{w2c.shape[0]} poses for {C} frames")
        k = intrinsics(K)
        a = _tsdf_args(self.tsdf, self.weight, self.color, self.origin, self.voxel_size, w2c, k, self.pixel_offset, depth, rgb,
                       self.ray_scale(k, height, width), self.sdf_trunc, self.depth_trunc)
        _lib.run("dnsplat_tsdf_integrate", _lib.lib().dnsplat_tsdf_integrate, ctypes.byref(a), _stream())
        return self

    def vertex_colors(self, vertices: Tensor) -> Tensor:
        """``dnsplat_tsdf_vertex_colors``: float32 [V,3] in 0 ... 1 for lattice-coordinate ``vertices`` float32 [V,3].  One launch."""
        if self.color is None:
            raise ValueError("the volume holds no colour")
        vertices = _f32c(vertices, "vertices")
        out = torch.empty(vertices.shape[0], 3, dtype=torch.float32, device=self.device)
        _lib.run("dnsplat_tsdf_vertex_colors", _lib.lib().dnsplat_tsdf_vertex_colors, _ptr(self.color), *self.dims, _ptr(vertices),
                 vertices.shape[0], _ptr(out), _stream())
        return out

    @torch.no_grad()
    def extract_mesh(self, min_weight: float = 0.0, capacity: Optional[Tuple[int, int]] = None, filter_clusters=None):
        """The zero level of the volume over the voxels with ``weight > min_weight``: (vertices float64 [V,3] in world coordinates,
        ``origin + voxel_size * v`` in float64; triangles int32 [T,3]; colours float32 [V,3] in 0 ... 1, or None).  One host read of
        (V, T).  With ``capacity=(cap_v, cap_t)`` nothing is read: the three are full-capacity buffers and a fourth item is the
        ``MarchingBuffers`` with the device counts and status (rows past the counts are unwritten).
        ``filter_clusters``: None (the default) returns the mesh as extracted; ``(keep_largest, min_triangles)`` — or True for the
        reference's (50, 50) — applies ``mesh_clusters.filter_small_clusters`` to it (export_mesh.py:1021-1039), world vertices and
        colours gathered; one more host read, of (V', T').  Not with ``capacity``: the filter needs the counts."""
        if min(self.dims) < 2:
            raise ValueError(f"a volume of {self.dims} has no cells")
        filter_clusters = _filter_arguments(filter_clusters)
        if filter_clusters is not None and capacity is not None:
            raise ValueError("filter_clusters needs the counts of the mesh: extract without capacity")
        out = marching_cubes(self.tsdf, 0.0, capacity=capacity, weight=self.weight, min_weight=float(min_weight))
        vertices, triangles = (out.vertices, out.triangles) if capacity is not None else out
        colors = None if self.color is None else self.vertex_colors(vertices)
        world = world_vertices(vertices, self.origin, self.voxel_size)
        if filter_clusters is not None:
            if triangles.shape[0] == 0:
                return world, triangles, colors
            return filter_small_clusters((world, triangles, colors), *filter_clusters)
        return (world, triangles, colors, out) if isinstance(out, MarchingBuffers) else (world, triangles, colors)


def _same_intrinsics(a, b) -> bool:
    return (float(a.fx), float(a.fy), float(a.cx), float(a.cy), int(a.width), int(a.height)) == \
        (float(b.fx), float(b.fy), float(b.cx), float(b.cy), int(b.width), int(b.height))


@torch.no_grad()
def fuse_tsdf_mesh(renderer, cameras, bounds, voxel_size: float = 0.01, sdf_trunc: float = 0.03, depth_trunc: float = 20.0, masks=None,
                   batch: int = 8, pixel_offset: float = 0.5, color: bool = True, min_weight: float = 0.0, filter_clusters=None):
    """The loop of ``Open3DTSDFFusion.main`` (export_mesh.py:961-1019): every one of ``cameras`` rendered through
    ``renderer.get_outputs_batch`` under ``no_grad``, depth zeroed outside ``masks[f]`` if ``masks`` is given, ``batch`` frames fused
    per ``integrate`` call into the volume of ``bounds`` = (lo, hi), then ``extract_mesh(min_weight, filter_clusters=filter_clusters)``:
    ``filter_clusters=True`` is the exporter as written, with its connected-component filter (:1021-1039); None leaves the mesh raw.
    The cameras share one set of intrinsics.  Returns (vertices float64 [V,3] world, triangles int32 [T,3], colours float32 [V,3] or None) on the device — what
    ``mesh_cull.cull_mesh`` and ``geometry.mesh_metrics`` take."""
    F_ = len(cameras)
    if F_ == 0:
        raise ValueError("fuse_tsdf_mesh needs at least one camera")
    if masks is not None and len(masks) != F_:
        raise ValueError(f"{len(masks)} masks for {F_} cameras")
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"batch must be at least 1, got {batch}")
    first = cameras[0]
    for f in range(1, F_):
        if not _same_intrinsics(first, cameras[f]):
            raise ValueError(f"camera {f} has other intrinsics than camera 0: per-camera intrinsics are out of scope")
    lo, hi = bounds
    volume = TSDFVolume.from_bounds(lo, hi, voxel_size, sdf_trunc=sdf_trunc, depth_trunc=depth_trunc, pixel_offset=pixel_offset,
                                    color=color, device=first.camera_to_worlds.device)
    K = [[float(first.fx), 0.0, float(first.cx)], [0.0, float(first.fy), float(first.cy)], [0.0, 0.0, 1.0]]
    for i in range(0, F_, batch):
        chunk = cameras[i:i + batch]
        outs = list(renderer.get_outputs_batch(chunk, max_batch=batch))
        depth = torch.stack([o["depth"].detach().reshape(o["depth"].shape[0], o["depth"].shape[1]) for o in outs]).float()
        if masks is not None:
            keep = torch.stack([masks[i + j].to(depth.device).reshape(depth.shape[1:]).bool() for j in range(len(outs))])
            depth = torch.where(keep, depth, torch.zeros_like(depth))
        rgb = torch.stack([o["rgb"].detach() for o in outs]).float() if color else None
        poses = torch.stack([c.camera_to_worlds.detach().reshape(-1, 4)[:3] for c in chunk])
        volume.integrate(depth, rgb, poses, K)
    return volume.extract_mesh(min_weight, filter_clusters=filter_clusters)
