"""The two point-cloud filters of the reference on HIP (``csrc/cloudfilter.hip``): Open3D's ``remove_statistical_outlier`` — the last step
before the solver of ``GaussiansToPoisson``, ``DepthAndNormalMapsPoisson`` and ``LevelSetExtractor`` (dn_splatter/export_mesh.py:287-291,
:487-491, :640) — and ``voxel_down_sample`` (dn_splatter/eval/eval_pd.py:82 in front of ``calculate_accuracy`` /
``calculate_completeness``; export_mesh.py:284-285).  ``export_oriented_points`` and ``export_level_set_points`` build those clouds on
the device and ``geometry`` scores them there; Open3D is not on a ROCm box, and the alternative is a device-to-host copy and a CPU
kd-tree in the middle.

  * ``remove_statistical_outlier``: the exact 20-NN of ``density.KnnIndex`` per point, two fixed-order float64 folds, an ordered
    append; ONE host read, of ``n_kept`` (none with ``capacity``);
  * ``voxel_down_sample``: an open-addressing table of voxel keys, voxels numbered in order of first appearance, exact integer means;
    ONE host read, of ``(V, status)``.

Both rules are stated in ``include/dnsplat.h`` and restated in ``torch_cloud_filter``: THEY ARE THIS PROJECT'S DEFINITION, PARITY UNPINNED
AGAINST Open3D.  Two deviations are deliberate: the voxel order is canonical (Open3D's is that of a hash map), and a voxel's mean is an
exact fixed-point sum, within ``voxel_size * 2**-30`` of the float64 mean, so that equal inputs give equal bytes.

Out of scope: ``remove_radius_outlier``, ``voxel_down_sample_and_trace``'s matrix form, PLY input and output.  CPU
tensors are refused; there is no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._ops import _cloud_outlier_args, _need_gpu, _stream, _voxel_args
from .density import KnnIndex
from .torch_cloud_filter import MAX_K, NB_NEIGHBORS, STD_RATIO

STATUS_INTERNAL, STATUS_NONFINITE, STATUS_EXTENT, STATUS_ATTRIBUTE = 1, 2, 4, 8     # DNSPLAT_VOXEL_STATUS_*
STATS_WORDS = 8                                                                     # DNSPLAT_CLOUD_OUTLIER_STATS_BYTES / 8
MAX_VOXEL_POINTS = (2 ** 31 - 1) // 2


def _device_cloud(points, name: str) -> Tensor:
    if not isinstance(points, Tensor):
        raise TypeError(f"{name} must be a tensor on the GPU, got {type(points).__name__}")
    _need_gpu(points, name)
    if not points.dtype.is_floating_point or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{name} must be a floating-point [n,3] tensor, got {points.dtype} {tuple(points.shape)}")
    if points.shape[0] < 1:
        raise ValueError(f"{name} is empty")
    return points.detach().to(torch.float32).contiguous()


def _check_outlier_arguments(nb_neighbors, std_ratio) -> Tuple[int, float]:
    nb_neighbors, std_ratio = int(nb_neighbors), float(std_ratio)
    if not 1 <= nb_neighbors <= MAX_K:
        raise ValueError(f"nb_neighbors must lie in [1, {MAX_K}], got {nb_neighbors}")
    if std_ratio != std_ratio:
        raise ValueError("std_ratio is nan")
    return nb_neighbors, std_ratio


class OutlierStats:
    """What the outlier kernels left on the device: ``avg`` float64 [N] and the 64-byte record, as the 0-dim device tensors ``mean``,
    ``std``, ``threshold`` (float64) and ``n_valid``, ``n_kept`` (int64).  Nothing here reads the host."""

    def __init__(self, avg: Tensor, record: Tensor):
        self.avg, self.record = avg, record
        words = record.view(torch.int64)
        self.mean, self.std, self.threshold, self.sum = record[0], record[1], record[2], record[3]
        self.n_valid, self.n_kept = words[4], words[5]


@torch.no_grad()
def remove_statistical_outlier(points: Tensor, nb_neighbors: int = NB_NEIGHBORS, std_ratio: float = STD_RATIO,
                               index: Optional[KnnIndex] = None, capacity: Optional[int] = None) -> Tuple[Tensor, OutlierStats]:
    """Open3D's ``remove_statistical_outlier`` on ``points`` [N,3] on the device: ``(ind, stats)``.  ``ind`` is int64 [n_kept], ascending —
    Open3D's ``ind``; gather points, normals and colours with it.  ``avg[i]`` is the mean distance to the ``min(nb_neighbors, N)``
    nearest points, the point itself included; a row is kept iff ``0 < avg[i] < mean + std_ratio * std``.  ``index`` is a ``KnnIndex``
    of the same points (one is built otherwise).  One host read, of ``n_kept``; with ``capacity`` there is none: ``ind`` then has
    ``capacity`` rows, -1 past ``stats.n_kept``."""
    nb_neighbors, std_ratio = _check_outlier_arguments(nb_neighbors, std_ratio)
    points = _device_cloud(points, "points")
    N, dev = points.shape[0], points.device
    if index is None:
        index = KnnIndex(points)
    elif not isinstance(index, KnnIndex):
        raise TypeError(f"index must be a KnnIndex, got {type(index).__name__}")
    if index.N != N or index.device != dev:
        raise ValueError(f"the index is over {index.N} points on {index.device}, the cloud has {N} on {dev}")
    if capacity is not None and int(capacity) < 0:
        raise ValueError(f"capacity must be >= 0, got {capacity}")
    L = _lib.lib()
    scratch = torch.empty((L.dnsplat_cloud_outlier_scratch_bytes(N) + 7) // 8, dtype=torch.int64, device=dev)
    avg = torch.empty(N, dtype=torch.float64, device=dev)
    record = torch.empty(STATS_WORDS, dtype=torch.float64, device=dev)
    a = _cloud_outlier_args(points, index.buffer, nb_neighbors, std_ratio, scratch, avg, record)
    _lib.run("dnsplat_cloud_neighbor_mean", L.dnsplat_cloud_neighbor_mean, ctypes.byref(a), _stream())
    _lib.run("dnsplat_cloud_outlier_stats", L.dnsplat_cloud_outlier_stats, ctypes.byref(a), _stream())
    _lib.run("dnsplat_cloud_outlier_count", L.dnsplat_cloud_outlier_count, ctypes.byref(a), _stream())
    stats = OutlierStats(avg, record)
    if capacity is None:
        ind = torch.empty(int(stats.n_kept.item()), dtype=torch.int64, device=dev)          # the one synchronisation
    else:
        ind = torch.full((int(capacity),), -1, dtype=torch.int64, device=dev)
    if ind.shape[0] > 0:
        a = _cloud_outlier_args(points, index.buffer, nb_neighbors, std_ratio, scratch, avg, record, ind)
        _lib.run("dnsplat_cloud_outlier_emit", L.dnsplat_cloud_outlier_emit, ctypes.byref(a), _stream())
    return ind, stats


def _attribute(x, N: int, name: str, dev) -> Optional[Tensor]:
    if x is None:
        return None
    if not isinstance(x, Tensor):
        raise TypeError(f"{name} must be a tensor on the GPU, got {type(x).__name__}")
    _need_gpu(x, name)
    if not x.dtype.is_floating_point or tuple(x.shape) != (N, 3) or x.device != dev:
        raise ValueError(f"{name} must be a floating-point [{N},3] tensor on {dev}, got {x.dtype} {tuple(x.shape)} on {x.device}")
    return x.detach().to(torch.float32).contiguous()


def _raise_status(status: int, voxel_size: float) -> None:
    if status & STATUS_NONFINITE:
        raise ValueError("voxel_down_sample: a point has a non-finite coordinate")
    if status & STATUS_EXTENT:
        raise ValueError(f"voxel_size = {voxel_size} is too small for the cloud's extent: more than 2^21 voxels along an axis")
    if status & STATUS_ATTRIBUTE:
        raise ValueError("voxel_down_sample: a component of normals or colors is non-finite or beyond 2 in magnitude")
    if status:
        raise _lib.DnsplatError(f"voxel_down_sample: internal status {status} (a bounded probe ran out)")


@torch.no_grad()
def voxel_down_sample(points: Tensor, voxel_size: float, normals: Optional[Tensor] = None, colors: Optional[Tensor] = None,
                      return_trace: bool = False):
    """Open3D's ``voxel_down_sample`` on ``points`` [N,3] on the device: ``(points', normals', colors')``, float64 [V,3] as Open3D's
    outputs are doubles (None for an array that was not given): one row per occupied voxel of the grid that starts at
    ``min - voxel_size / 2``, the mean of the voxel's points and of their attributes (normals are not re-normalised, as in Open3D).
    Voxels are numbered in order of first appearance.  With ``return_trace`` also ``voxel_of`` int32 [N] and ``counts`` int32 [V].
    Raises ``ValueError`` for ``voxel_size <= 0``, a non-finite coordinate, more than 2^21 voxels along an axis, or an attribute
    component that is non-finite or beyond 2 in magnitude.  One host read, of (V, status)."""
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0 and voxel_size < float("inf")):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    points = _device_cloud(points, "points")
    N, dev = points.shape[0], points.device
    if N > MAX_VOXEL_POINTS:
        raise ValueError(f"a cloud of {N} points is beyond the voxel table's index ({MAX_VOXEL_POINTS} points at the most)")
    normals, colors = _attribute(normals, N, "normals", dev), _attribute(colors, N, "colors", dev)
    n_attr = (normals is not None) + (colors is not None)
    L = _lib.lib()
    scratch = torch.empty((L.dnsplat_voxel_scratch_bytes(N, n_attr) + 7) // 8, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    voxel_of = torch.empty(N, dtype=torch.int32, device=dev)
    a = _voxel_args(points, normals, colors, voxel_size, scratch, counts, voxel_of)
    _lib.run("dnsplat_voxel_count", L.dnsplat_voxel_count, ctypes.byref(a), _stream())
    V, status = counts.tolist()                                                   # the one synchronisation
    _raise_status(status, voxel_size)
    out_points = torch.empty(V, 3, dtype=torch.float64, device=dev)
    out_normals = None if normals is None else torch.empty(V, 3, dtype=torch.float64, device=dev)
    out_colors = None if colors is None else torch.empty(V, 3, dtype=torch.float64, device=dev)
    out_counts = torch.empty(V, dtype=torch.int32, device=dev) if return_trace else None
    a = _voxel_args(points, normals, colors, voxel_size, scratch, counts, voxel_of, out_points, out_normals, out_colors, out_counts)
    _lib.run("dnsplat_voxel_emit", L.dnsplat_voxel_emit, ctypes.byref(a), _stream())
    result = (out_points, out_normals, out_colors)
    return result + (voxel_of, out_counts) if return_trace else result
