"""The reference's geometry scores on HIP (``csrc/geometry.hip``): point-cloud accuracy and completeness (``PDMetrics``,
``calculate_accuracy``, ``calculate_completeness``; dn_splatter/metrics.py:11-56) and the mesh scores of ``compute_metrics``
(dn_splatter/eval/eval_mesh_vis_cull.py:290-397: Acc, Comp, Chamfer-L1, normal consistency, F-score at 0.05) on clouds and meshes that
are already on the device.

Where the reference copies both clouds to the host, builds a scipy ``cKDTree`` per direction and samples the meshes with trimesh, this
module keeps the uniform-grid index of ``density.KnnIndex`` over the target cloud and runs one direction of ``distance_p2p`` — the exact
nearest neighbour, the normal dot product, the means, the threshold shares and numpy's percentile — as ONE ``dnsplat_cloud_distances``
call, and samples a mesh with ``dnsplat_mesh_areas`` / ``dnsplat_mesh_sample``.  Nothing is read on the host unless a scalar is asked for.

  * ``cloud_distances``: one direction; ``tgt`` may be a ``KnnIndex`` so that repeated calls reuse a build;
  * ``calculate_accuracy`` / ``calculate_completeness`` / ``PDMetrics`` / ``install_pd_metrics``: the reference's signatures;
  * ``sample_mesh_surface``: ``mesh.sample(count, return_index=True)`` with the face normals, a canonical function of (mesh, seed);
  * ``mesh_metrics`` / ``cloud_metrics``: ``compute_metrics`` on two meshes, or on two already-sampled oriented clouds.

Coordinates are float32, because the index is: float64 arrays or tensors are rounded to float32 ONCE on the way in (the reference's
``compute_metrics`` does the same with ``astype(np.float32)``; its ``PDMetrics`` ranks float64 coordinates).  numpy arrays and objects with
``.points`` are uploaded to the current device; CPU tensors are refused, as everywhere else in the package.  ``torch_geometry`` is the
PyTorch restatement.  There is no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._ops import _cloud_distances_args, _mesh_sample_args, _need_gpu, _ptr, _stream
from .density import KnnIndex
from .torch_geometry import (COUNT_INDEX, GEOM_COUNT, GEOM_COUNTS, GEOM_INDEX, PERCENTILE, SAMPLES_PER_AREA, THRESHOLD,
                             metrics_from_directions)


def _device_points(x, name: str) -> Tensor:
    """[n,3] contiguous float32 on the GPU from a tensor, a numpy array or anything with ``.points``; float64 is rounded once."""
    if hasattr(x, "points") and not isinstance(x, (Tensor, np.ndarray)):
        x = np.asarray(x.points)
    if isinstance(x, Tensor):
        _need_gpu(x, name)
        t = x.detach()
    else:
        if not torch.cuda.is_available():
            raise _lib.DnsplatError(f"{name}: the geometry scores run only on the GPU through libdnsplat.so (there is no CPU fallback)")
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x))).to(torch.device("cuda", torch.cuda.current_device()))
    if not t.dtype.is_floating_point:
        raise TypeError(f"{name} must be floating point, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be [n,3], got {tuple(t.shape)}")
    return t.to(torch.float32).contiguous()


class CloudDistances:
    """One direction of ``distance_p2p``: the device tensors ``dist2`` [M] float64, ``idx`` [M] int32, ``absdot`` [M] float64 or None,
    ``scalars`` float64 [12] and ``counts`` int64 [4]; the named scalars (``mean_d``, ``mean_d2``, ``mean_absdot``, ``percentile``,
    ``share_lt``, ``share_le``, ``min_d``, ``max_d``, ``order_lo_d2``, ``order_hi_d2``; ``n``, ``n_lt``, ``n_le``, ``n_nonfinite``) are
    read lazily, all of them with one copy per tensor on first use."""

    def __init__(self, dist2, idx, absdot, scalars, counts):
        self.dist2, self.idx, self.absdot, self.scalars, self.counts = dist2, idx, absdot, scalars, counts
        self._host = None

    @property
    def distances(self) -> Tensor:
        return torch.sqrt(self.dist2)

    def scalar(self, name: str) -> Tensor:
        """The 0-dim device tensor of a named scalar or count: no host read."""
        return self.scalars[GEOM_INDEX[name]] if name in GEOM_INDEX else self.counts[COUNT_INDEX[name]]

    def __getattr__(self, name: str):
        if name in GEOM_INDEX or name in COUNT_INDEX:
            if self._host is None:
                self._host = (self.scalars.tolist(), self.counts.tolist())
            return self._host[0][GEOM_INDEX[name]] if name in GEOM_INDEX else self._host[1][COUNT_INDEX[name]]
        raise AttributeError(name)


def _index_of(tgt, name: str) -> KnnIndex:
    return tgt if isinstance(tgt, KnnIndex) else KnnIndex(_device_points(tgt, name))


@torch.no_grad()
def cloud_distances(src, tgt, src_normals=None, tgt_normals=None, threshold: float = THRESHOLD, percentile: float = PERCENTILE,
                    with_idx: bool = True) -> CloudDistances:
    """For every point of ``src`` [M,3] its nearest point of ``tgt`` ([N,3], or a ``KnnIndex`` built over it) under (d², index) with d² in
    float64, and with both normal arrays |n_src . n_tgt[idx]| of the normalised normals; the means, numpy's ``percentile`` of the
    distances, the shares ``d < threshold`` and ``d <= threshold``, min and max.  One ``dnsplat_cloud_distances`` call; float64 inputs
    are rounded to float32 once.  A source row with a non-finite coordinate gets ``idx = -1``, ``dist2 = nan`` and makes the means and the
    percentile nan; a target row with a nan or inf coordinate is nobody's neighbour, and if every target is such a row, every source row
    is non-finite."""
    if (src_normals is None) != (tgt_normals is None):
        raise ValueError("source and target normals are given together or not at all")
    if not 0.0 <= float(percentile) <= 100.0:
        raise ValueError(f"percentile must lie in [0, 100], got {percentile}")
    src = _device_points(src, "src")
    index = _index_of(tgt, "tgt")
    M, dev = src.shape[0], src.device
    if M < 1:
        raise ValueError("cloud_distances needs at least one source point")
    if index.device != dev:
        raise ValueError(f"src is on {dev}, the target index on {index.device}")
    if src_normals is not None:
        src_normals, tgt_normals = _device_points(src_normals, "src_normals"), _device_points(tgt_normals, "tgt_normals")
        if src_normals.shape[0] != M or tgt_normals.shape[0] != index.N:
            raise ValueError(f"normals: [{M},3] for the source and [{index.N},3] for the target, got {tuple(src_normals.shape)} and "
                             f"{tuple(tgt_normals.shape)}")
    L = _lib.lib()
    dist2 = torch.empty(M, dtype=torch.float64, device=dev)
    idx = torch.empty(M, dtype=torch.int32, device=dev) if with_idx else None
    absdot = torch.empty(M, dtype=torch.float64, device=dev) if src_normals is not None else None
    scalars = torch.empty(GEOM_COUNT, dtype=torch.float64, device=dev)
    counts = torch.empty(GEOM_COUNTS, dtype=torch.int64, device=dev)
    scratch = torch.empty(L.dnsplat_cloud_distances_scratch_bytes(M) // 8, dtype=torch.int64, device=dev)
    a = _cloud_distances_args(index.N, index.buffer, src, src_normals, tgt_normals, float(threshold), float(percentile), dist2, idx, absdot,
                              scalars, counts, scratch)
    _lib.run("dnsplat_cloud_distances", L.dnsplat_cloud_distances, ctypes.byref(a), _stream())
    return CloudDistances(dist2, idx, absdot, scalars, counts)


def _down_sampled(points, voxel_size, name: str) -> Tensor:
    """eval_pd.py:82: ``pcd.voxel_down_sample(voxel_size)`` — the voxel means, rounded to float32 once like every cloud here."""
    from .cloud_filter import voxel_down_sample

    return voxel_down_sample(_device_points(points, name), voxel_size)[0].to(torch.float32)


def calculate_accuracy(reconstructed_points, reference_points, percentile=90, down_sample_voxel: Optional[float] = None) -> Tensor:
    """metrics.py:39-45: how far ``percentile`` % of the reconstructed points are from the reference cloud — numpy's percentile of the
    nearest-neighbour distances, a 0-dim float64 device tensor.  ``reference_points`` may be a ``KnnIndex``.  ``down_sample_voxel``
    (eval_pd.py:82: 0.01) first replaces the reconstructed cloud by ``cloud_filter.voxel_down_sample`` of it; None leaves it alone."""
    if down_sample_voxel is not None:
        reconstructed_points = _down_sampled(reconstructed_points, down_sample_voxel, "reconstructed_points")
    return cloud_distances(reconstructed_points, reference_points, percentile=float(percentile), with_idx=False).scalar("percentile")


def calculate_completeness(reconstructed_points, reference_points, threshold=0.05) -> Tensor:
    """metrics.py:48-56: the percentage (share TIMES 100) of the reference cloud with ``d < threshold`` of the reconstruction, a 0-dim
    float64 device tensor.  ``reconstructed_points`` may be a ``KnnIndex``."""
    return cloud_distances(reference_points, reconstructed_points, threshold=float(threshold), with_idx=False).scalar("share_lt") * 100


class PDMetrics(torch.nn.Module):
    """Drop-in for ``dn_splatter.metrics.PDMetrics``: ``forward(pred, gt) -> (acc, comp)`` on anything with ``.points``, arrays or device
    tensors; 0-dim float64 device tensors, so the pipeline's ``.item()`` works.  ``down_sample_voxel`` (eval_pd.py:82 passes 0.01 to
    Open3D) down-samples the reconstructed cloud, and only it, before both scores; None, the default, scores the clouds as given."""

    def __init__(self, down_sample_voxel: Optional[float] = None, **kwargs):
        super().__init__()
        self.acc = calculate_accuracy
        self.cmp = calculate_completeness
        self.down_sample_voxel = down_sample_voxel

    @torch.no_grad()
    def forward(self, pred, gt):
        pred_points, gt_points = _device_points(pred, "pred"), _device_points(gt, "gt")
        if self.down_sample_voxel is not None:
            pred_points = _down_sampled(pred_points, self.down_sample_voxel, "pred")
        return self.acc(pred_points, gt_points), self.cmp(pred_points, gt_points)


def install_pd_metrics(pipeline):
    """Sets ``pipeline.pd_metrics`` (dn_pipeline.py:130) to the HIP ``PDMetrics``; the original, if there was one, is kept as
    ``pipeline._dnsplat_original_pd_metrics``.  Idempotent; returns the list of what was swapped."""
    old = getattr(pipeline, "pd_metrics", None)
    if isinstance(old, PDMetrics):
        return []
    if old is not None:
        object.__setattr__(pipeline, "_dnsplat_original_pd_metrics", old)
    setattr(pipeline, "pd_metrics", PDMetrics())
    return ["pd_metrics"]


# ---- meshes ------------------------------------------------------------------------------------------------------------------------

def _mesh(mesh, name: str) -> Tuple[Tensor, Tensor]:
    """(vertices float32 [V,3], triangles int32 [T,3]) from a (vertices, triangles, ...) tuple — what ``marching_cubes_mesh`` returns."""
    vertices, triangles = mesh[0], mesh[1]
    vertices = _device_points(vertices, name + " vertices")
    if not isinstance(triangles, Tensor):
        triangles = torch.from_numpy(np.ascontiguousarray(np.asarray(triangles))).to(vertices.device)
    _need_gpu(triangles, name + " triangles")
    if triangles.dtype.is_floating_point or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError(f"{name} triangles must be an integer [T,3] tensor, got {triangles.dtype} {tuple(triangles.shape)}")
    if vertices.shape[0] < 1 or triangles.shape[0] < 1:
        raise ValueError(f"{name}: an empty mesh has no surface to sample")
    return vertices, triangles.to(torch.int32).contiguous()


@torch.no_grad()
def mesh_areas(vertices: Tensor, triangles: Tensor) -> Tuple[Tensor, Tensor]:
    """``dnsplat_mesh_areas``: (areas float64 [T], unit face normals float32 [T,3]); a zero-area face has normal 0, a triangle with an index
    outside [0, V) area 0."""
    vertices, triangles = _mesh((vertices, triangles), "mesh")
    T = triangles.shape[0]
    areas = torch.empty(T, dtype=torch.float64, device=vertices.device)
    normals = torch.empty(T, 3, dtype=torch.float32, device=vertices.device)
    L = _lib.lib()
    _lib.run("dnsplat_mesh_areas", L.dnsplat_mesh_areas, vertices.shape[0], _ptr(vertices), T, _ptr(triangles), _ptr(areas), _ptr(normals),
             _stream())
    return areas, normals


@torch.no_grad()
def mesh_sample(count: int, seed: int, cdf: Tensor, vertices: Tensor, triangles: Tensor, face_normals: Tensor):
    """``dnsplat_mesh_sample`` on the caller's ``cdf`` (float64 [T], the inclusive prefix sums of the areas): (points float32 [S,3], normals
    float32 [S,3], faces int32 [S])."""
    vertices, triangles = _mesh((vertices, triangles), "mesh")
    dev = vertices.device
    _need_gpu(cdf, "cdf"); _need_gpu(face_normals, "face_normals")
    if cdf.dtype != torch.float64 or cdf.numel() != triangles.shape[0] or tuple(face_normals.shape) != (triangles.shape[0], 3):
        raise ValueError(f"cdf float64 [T] and face_normals [T,3] for T = {triangles.shape[0]}, got {cdf.dtype} {tuple(cdf.shape)} and "
                         f"{tuple(face_normals.shape)}")
    count = int(count)
    if count < 0:
        raise ValueError(f"count must be >= 0, got {count}")
    points = torch.empty(count, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(count, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(count, dtype=torch.int32, device=dev)
    a = _mesh_sample_args(int(seed) & 0xFFFFFFFFFFFFFFFF, cdf.contiguous(), vertices, triangles, face_normals.to(torch.float32).contiguous(),
                          points, normals, faces)
    L = _lib.lib()
    _lib.run("dnsplat_mesh_sample", L.dnsplat_mesh_sample, ctypes.byref(a), _stream())
    return points, normals, faces


@torch.no_grad()
def sample_mesh_surface(vertices, triangles, count: Optional[int] = None, samples_per_area: float = SAMPLES_PER_AREA, seed: int = 0):
    """``mesh.sample(count, return_index=True)`` with ``mesh.face_normals[index]``: (points [S,3], normals [S,3], faces [S]), uniform over the
    surface, a canonical function of (mesh, seed).  ``count=None`` is compute_metrics' ``int(mesh.area * samples_per_area)`` and costs one
    host read of the total area; an explicit ``count`` reads nothing.  The prefix sum of the areas is ``torch.cumsum`` in float64."""
    vertices, triangles = _mesh((vertices, triangles), "mesh")
    areas, normals = mesh_areas(vertices, triangles)
    cdf = torch.cumsum(areas, dim=0)
    if count is None:
        area = float(cdf[-1])
        if not area > 0.0:
            raise ValueError("the mesh has no area to sample")
        count = int(area * samples_per_area)
    return mesh_sample(count, seed, cdf, vertices, triangles, normals)


def _metrics(comp: CloudDistances, acc: CloudDistances) -> Dict[str, Tensor]:
    return metrics_from_directions(comp.scalars, acc.scalars)


@torch.no_grad()
def cloud_metrics(pred_points, pred_normals, tgt_points, tgt_normals, threshold: float = THRESHOLD) -> Dict[str, Tensor]:
    """``compute_metrics`` behind its two ``sample`` calls, on two already-sampled oriented clouds: ``{"Acc", "Comp", "C-L1", "C-L2", "NC",
    "F-score", "precision", "recall"}`` as 0-dim float64 device tensors.  Acc / Comp are the mean distances prediction -> target / target
    -> prediction, precision / recall the shares ``d <= threshold`` of the same two directions, ``F = 2 P R / (P + R)`` (nan when
    ``P + R == 0``), NC the mean of the two mean ``|dot|`` (nan without normals).  Two index builds, two ``dnsplat_cloud_distances`` calls."""
    pred_points, tgt_points = _device_points(pred_points, "pred_points"), _device_points(tgt_points, "tgt_points")
    comp = cloud_distances(tgt_points, pred_points, tgt_normals, pred_normals, threshold=threshold, with_idx=False)
    acc = cloud_distances(pred_points, tgt_points, pred_normals, tgt_normals, threshold=threshold, with_idx=False)
    return _metrics(comp, acc)


@torch.no_grad()
def mesh_metrics(pred, target, threshold: float = THRESHOLD, seed: int = 0, samples_per_area: float = SAMPLES_PER_AREA,
                 count: Optional[Tuple[int, int]] = None) -> Dict[str, Tensor]:
    """``compute_metrics(mesh_pred, mesh_target)``: both meshes — ``(vertices, triangles)`` pairs, or what ``marching_cubes_mesh`` returns —
    sampled at ``int(area * samples_per_area)`` points (or ``count = (n_pred, n_target)``, which saves the two host reads) with seeds
    ``seed`` and ``seed + 1``, then ``cloud_metrics``."""
    pp, pn, _ = sample_mesh_surface(pred[0], pred[1], None if count is None else count[0], samples_per_area, seed)
    tp, tn, _ = sample_mesh_surface(target[0], target[1], None if count is None else count[1], samples_per_area, seed + 1)
    if pp.shape[0] < 1 or tp.shape[0] < 1:
        raise ValueError(f"{pp.shape[0]} and {tp.shape[0]} samples: a mesh is too small for samples_per_area = {samples_per_area}")
    return cloud_metrics(pp, pn, tp, tn, threshold)
