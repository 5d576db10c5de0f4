"""Marching cubes on the device (``csrc/marching.hip``): the step between ``density_volume`` and the mesh in the reference's
``gs-mesh marching`` exporter (dn_splatter/export_mesh.py:700-820, ``MarchingCubesMesh``), which hands the lattice to
``mcubes.marching_cubes`` on the CPU — at 512³ a 512 MiB device-to-host copy and a single-threaded walk over 134 M cells.

The output is a canonical function of (volume, level), stated in ``torch_marching`` (the numpy restatement the kernels are held to with
exact equality): a point is above iff ``v > level``; one vertex per sign-changing lattice edge, numbered in ascending (flat index of
the lower end, axis), at ``float(p_a) + (level - v(p)) / (v(p + e_a) - v(p))`` in float32; triangles by cell in ascending flat index,
in the order of the generated case table, normals towards decreasing value.  Corner values equal to ``level`` give zero-area triangles;
they are kept.  Nothing here is pinned to ``mcubes``: it is a third-party library with a table and a vertex order of its own.

  * ``marching_cubes(volume, level, capacity=None)``: vertices float32 [V,3] in lattice coordinates, triangles int32 [T,3];
  * ``mc_count`` / ``mc_emit``: the two C entry points, for a caller that owns the buffers;
  * ``mcubes_marching_cubes(volume, level)``: the call shape of ``mcubes.marching_cubes`` (numpy float64 / int64), to point the
    reference's exporter at;
  * ``marching_cubes_mesh(field, resolution, radius, ...)``: lines 740-800 — lattice, surface, world mapping, vertex colours.

``weight`` / ``min_weight`` on ``mc_count`` and ``marching_cubes`` restrict the extraction to the observed part of the lattice
(``weight > min_weight``; ``dnsplat_mc_count_observed`` / ``dnsplat_mc_emit_observed``, the rule of ``torch_marching``): the surface of
a TSDF volume (``tsdf.TSDFVolume.extract_mesh``).  Without them the calls, the scratch and the bytes are what they always were.

V and T depend on the data.  ``marching_cubes`` without ``capacity`` reads the two counts on the host once, between count and emit:
ONE synchronisation per mesh, the only one.  With ``capacity=(cap_v, cap_t)`` nothing is read on the host; the caller checks
``status`` afterwards.  Simplification, cluster filtering and PLY output stay with the caller.  There is no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._lib import DnsplatError
from ._ops import _f32c, _mc_args, _mc_observed_args, _need_gpu, _stream
from .density import GaussianDensityField, density_volume
from .torch_marching import MAX_POINTS

STATUS_VERTICES, STATUS_TRIANGLES = 1, 2        # include/dnsplat.h DNSPLAT_MC_STATUS_*


class MarchingCount(NamedTuple):
    """What ``mc_count`` leaves for ``mc_emit``: the lattice, the level, the scratch with masks and offsets, counts = int64 [2] (V, T);
    ``weight`` / ``min_weight`` if the count was over the observed part only."""
    volume: Tensor
    level: float
    scratch: Optional[Tensor]
    counts: Tensor
    weight: Optional[Tensor] = None
    min_weight: float = 0.0


class MarchingBuffers(NamedTuple):
    """``marching_cubes`` with a capacity: full-capacity buffers (rows past the counts are unwritten), counts int64 [2], status int32 [1]."""
    vertices: Tensor
    triangles: Tensor
    counts: Tensor
    status: Tensor


def _lattice(volume: Tensor) -> Tensor:
    volume = _f32c(volume.detach(), "volume")
    if volume.dim() != 3:
        raise ValueError(f"volume must be [Rx,Ry,Rz], got {tuple(volume.shape)}")
    if volume.numel() >= MAX_POINTS:
        raise DnsplatError(f"a lattice of {tuple(volume.shape)} has 2^31 points or more")
    return volume


def scratch_bytes(shape, observed: bool = False) -> int:
    L = _lib.lib()
    return int((L.dnsplat_mc_observed_scratch_bytes if observed else L.dnsplat_mc_scratch_bytes)(*(int(s) for s in shape)))


def _run(name: str, count: "MarchingCount", a) -> None:
    """``dnsplat_mc_<name>`` on McArgs ``a``, or ``dnsplat_mc_<name>_observed`` if the count carries a weight lattice."""
    L = _lib.lib()
    if count.weight is None:
        _lib.run("dnsplat_mc_" + name, getattr(L, "dnsplat_mc_" + name), ctypes.byref(a), _stream())
    else:
        _lib.run("dnsplat_mc_" + name + "_observed", getattr(L, "dnsplat_mc_" + name + "_observed"), ctypes.byref(a), _stream())


def mc_count(volume: Tensor, level: float, scratch: Optional[Tensor] = None, weight: Optional[Tensor] = None,
             min_weight: float = 0.0) -> MarchingCount:
    """``dnsplat_mc_count``: masks, per-word counts and their scan into ``scratch`` (allocated if not given), V and T into a device
    int64 [2].  Four launches, nothing read on the host.  With ``weight`` (float32, the volume's shape):
    ``dnsplat_mc_count_observed`` over the points with ``weight > min_weight``; ``scratch`` is then ``scratch_bytes(shape, True)``."""
    volume = _lattice(volume)
    if weight is not None:
        weight = _f32c(weight.detach(), "weight")
        if weight.shape != volume.shape or weight.device != volume.device:
            raise ValueError(f"weight must be {tuple(volume.shape)} on {volume.device}, got {tuple(weight.shape)} on {weight.device}")
    counts = torch.empty(2, dtype=torch.int64, device=volume.device)
    if min(volume.shape) >= 2:
        need = scratch_bytes(volume.shape, weight is not None)
        if scratch is None:
            scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=volume.device)
        else:
            _need_gpu(scratch, "scratch")
            if scratch.numel() * scratch.element_size() < need or scratch.data_ptr() % 16 or not scratch.is_contiguous():
                raise ValueError(f"scratch must be a contiguous, 16-byte aligned buffer of at least {need} bytes")
    elif volume.numel() == 0:
        counts.zero_()
        return MarchingCount(volume, float(level), None, counts, weight, float(min_weight))
    else:
        scratch = None
    count = MarchingCount(volume, float(level), scratch, counts, weight, float(min_weight))
    _run("count", count, _args(count))
    return count


def _args(count: MarchingCount, *emit):
    mc = (count.volume, count.level, count.scratch, count.counts) + emit
    return _mc_args(*mc) if count.weight is None else _mc_observed_args(count.weight, count.min_weight, *mc)


def mc_emit(count: MarchingCount, vertices: Tensor, triangles: Tensor, cap_v: Optional[int] = None, cap_t: Optional[int] = None) -> Tensor:
    """``dnsplat_mc_emit`` into the caller's ``vertices`` (float32 [>= cap_v,3]) and ``triangles`` (int32 [>= cap_t,3]); the capacities
    default to the buffers' rows.  Returns status, int32 [1] on the device: ``STATUS_VERTICES`` | ``STATUS_TRIANGLES`` for a capacity
    below the count.  Nothing past a capacity is written.  Two launches, nothing read on the host."""
    for name, buf, dtype in (("vertices", vertices, torch.float32), ("triangles", triangles, torch.int32)):
        _need_gpu(buf, name)
        if buf.dtype != dtype or buf.dim() != 2 or buf.shape[1] != 3 or not buf.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} [capacity,3] buffer")
    cap_v = vertices.shape[0] if cap_v is None else int(cap_v)
    cap_t = triangles.shape[0] if cap_t is None else int(cap_t)
    if not 0 <= cap_v <= vertices.shape[0] or not 0 <= cap_t <= triangles.shape[0]:
        raise ValueError(f"capacities ({cap_v}, {cap_t}) outside the buffers ({vertices.shape[0]}, {triangles.shape[0]} rows)")
    status = torch.empty(1, dtype=torch.int32, device=count.volume.device)
    if count.volume.numel() == 0:
        return status.zero_()
    _run("emit", count, _args(count, vertices if cap_v else None, triangles if cap_t else None, cap_v, cap_t, status))
    return status


def marching_cubes(volume: Tensor, level: float, capacity: Optional[Tuple[int, int]] = None, weight: Optional[Tensor] = None,
                   min_weight: float = 0.0):
    """The iso-surface of ``volume`` (float32 [Rx,Ry,Rz] on the GPU, ``meshgrid(indexing="ij")`` order) at ``level``; with ``weight``,
    of the part of it where ``weight > min_weight`` (the module docstring).

    Without ``capacity``: (vertices float32 [V,3] in lattice coordinates, triangles int32 [T,3]); the two counts are read on the host
    once, between count and emit — one synchronisation per mesh.  With ``capacity=(cap_v, cap_t)``: a ``MarchingBuffers`` of
    full-capacity buffers, the device counts and the device status word, with no host read at all; rows past the counts are
    unwritten and a non-zero status means a capacity was too small (the rows below it are still the mesh's)."""
    count = mc_count(volume, level, weight=weight, min_weight=min_weight)
    dev = count.volume.device
    if capacity is not None:
        cap_v, cap_t = (int(c) for c in capacity)
        vertices = torch.empty(cap_v, 3, dtype=torch.float32, device=dev)
        triangles = torch.empty(cap_t, 3, dtype=torch.int32, device=dev)
        return MarchingBuffers(vertices, triangles, count.counts, mc_emit(count, vertices, triangles))
    V, T = count.counts.tolist()                    # the one synchronisation
    if max(V, T) > 2 ** 31 - 1:
        raise DnsplatError(f"the surface has {V} vertices and {T} triangles: ids are int32")
    vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
    triangles = torch.empty(T, 3, dtype=torch.int32, device=dev)
    mc_emit(count, vertices, triangles)
    return vertices, triangles


def mcubes_marching_cubes(volume, level: float):
    """``mcubes.marching_cubes(volume, level)`` as export_mesh.py:778 calls it: ``volume`` a numpy array or a tensor (copied to the
    current GPU if it is not on one), returns numpy float64 [V,3] (lattice coordinates) and int64 [T,3].  The mesh is this library's
    canonical one, not mcubes' vertex for vertex."""
    if not torch.is_tensor(volume):
        volume = torch.from_numpy(np.ascontiguousarray(volume, dtype=np.float32))
    if not volume.is_cuda:
        if not torch.cuda.is_available():
            raise DnsplatError("mcubes_marching_cubes runs on the GPU through libdnsplat.so and there is none (torch_marching is the "
                               "numpy restatement; there is no CPU fallback)")
        volume = volume.cuda()
    vertices, triangles = marching_cubes(volume.float(), level)
    return vertices.cpu().numpy().astype(np.float64), triangles.cpu().numpy().astype(np.int64)


def world_mapping(vertices: Tensor, X: Tensor, Y: Tensor, Z: Tensor) -> Tensor:
    """export_mesh.py:789-795 on the device: ``X[0] + (v / (R - 1)) * (X[-1] - X[0])`` per axis in float64, the span formed in the axes'
    own precision first, as the reference's numpy expression does.  float64 [V,3]."""
    cols = []
    for a, axis in enumerate((X, Y, Z)):
        span = (axis[-1] - axis[0]).double()
        cols.append(axis[0].double() + (vertices[:, a].double() / (axis.numel() - 1)) * span)
    return torch.stack(cols, dim=-1)


def marching_cubes_mesh(field: GaussianDensityField, resolution: int, radius: float, level: float = 0.5, crop_box=None,
                        colors: Optional[Tensor] = None):
    """export_mesh.py:740-800 for a ``GaussianDensityField``: the [R,R,R] density lattice over ``linspace(-1, 1, R) * radius``
    (``density_volume``; -1e6 outside ``crop_box``), its surface at ``level``, the vertices mapped to world coordinates and, if
    ``colors`` [N,3] is given, ``colors[field.closest(vertices_world)[:, 0]]``.  Returns (vertices_world float64 [V,3], triangles
    int32 [T,3], vertex colours or None), all on the device.  One host synchronisation (``marching_cubes``)."""
    resolution = int(resolution)
    if resolution < 2:
        raise ValueError(f"resolution must be at least 2, got {resolution}")
    volume = density_volume(field, resolution, radius, crop_box)
    vertices, triangles = marching_cubes(volume, level)
    X = torch.linspace(-1, 1, resolution, device=field.device) * radius
    world = world_mapping(vertices, X, X, X)
    vertex_colors = None
    if colors is not None:
        _need_gpu(colors, "colors")
        if colors.dim() != 2 or colors.shape[0] != field.N:
            raise ValueError(f"colors must be [{field.N},C], got {tuple(colors.shape)}")
        vertex_colors = colors[field.closest(world.float())[:, 0]] if world.shape[0] else colors[:0]
    return world, triangles, vertex_colors
