"""The connected-component filter of a mesh on HIP (``csrc/meshclusters.hip``): the step the reference's recommended exporter ends
with (``Open3DTSDFFusion``, dn_splatter/export_mesh.py:1021-1039) — Open3D's ``cluster_connected_triangles``, the threshold
``n = max(np.sort(cluster_n_triangles)[-50], 50)``, the removal of every triangle of a cluster with fewer than ``n`` triangles,
``remove_unreferenced_vertices`` and ``remove_degenerate_triangles``.  A TSDF mesh of rendered depth is one large surface plus thousands
of floaters, one wherever a stray splat crossed the truncation band; ``geometry.mesh_metrics`` samples them by area and
``mesh_cull.cull_mesh`` renders them per pose unless they are cut first.  Open3D is not on a ROCm box, and the alternative there is a
device-to-host copy of the triangles and a CPU graph library.

  * ``cluster_connected_triangles``: labels and sizes, ``dnsplat_mesh_clusters``; one host read, of ``n_clusters``;
  * ``filter_small_clusters``: the filter on a (vertices, triangles, *per_vertex) tuple — what ``marching_cubes_mesh`` and
    ``TSDFVolume.extract_mesh`` return — ``dnsplat_mesh_clusters``, ``dnsplat_mesh_filter_count``, ONE host read of (V', T'),
    ``dnsplat_mesh_filter_emit``, and an ``index_select`` per per-vertex tensor.

Topology only: the clusters are over vertex INDICES (``marching.hip`` emits one vertex per lattice edge, so its meshes need no merging
by position).  The definition is stated in ``include/dnsplat.h`` and restated sequentially in ``torch_mesh_clusters``: IT IS THIS
PROJECT'S DEFINITION, PARITY UNPINNED AGAINST Open3D.  One deviation: Open3D compacts the vertices before it drops degenerate
triangles and can leave a vertex that only a degenerate triangle referenced; this leaves none.  ``cluster_area``, the third result of
Open3D's call, is not produced: the reference's filter never reads it.  With fewer than ``keep_largest`` clusters the reference's
``[-50]`` raises IndexError; here the threshold is then ``min_triangles``.

Out of scope: ``cluster_area``, vertex merging by position, quadric decimation, PLY output.  CPU tensors are refused; there is no CPU
fallback."""
from __future__ import annotations

import ctypes
from typing import Tuple

import torch
from torch import Tensor

from . import _lib
from ._ops import _mesh_clusters_args, _mesh_filter_args, _need_gpu, _stream
from .torch_mesh_clusters import KEEP_LARGEST, MIN_TRIANGLES

STATUS_INTERNAL = 1                                         # DNSPLAT_MESH_CLUSTERS_STATUS_INTERNAL


def _device_triangles(triangles, n_vertices: int) -> Tuple[Tensor, int]:
    if not isinstance(triangles, Tensor):
        raise TypeError(f"triangles must be a tensor on the GPU, got {type(triangles).__name__}")
    _need_gpu(triangles, "triangles")
    if triangles.dtype.is_floating_point or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError(f"triangles must be an integer [T,3] tensor, got {triangles.dtype} {tuple(triangles.shape)}")
    n_vertices = int(n_vertices)
    if n_vertices < 1 or triangles.shape[0] < 1:
        raise ValueError("an empty mesh has no triangles to cluster")
    return triangles.detach().to(torch.int32).contiguous(), n_vertices


class ClusterBuffers:
    """What ``dnsplat_mesh_clusters`` left on the device: ``labels`` int32 [T], ``sizes`` int32 [T] (zero past ``n_clusters``),
    ``counts`` int64 [2] = {n_clusters, valid triangles} and ``status`` int32 [1] (0 on a correct build)."""

    def __init__(self, labels, sizes, counts, status):
        self.labels, self.sizes, self.counts, self.status = labels, sizes, counts, status


@torch.no_grad()
def cluster_buffers(triangles: Tensor, n_vertices: int) -> ClusterBuffers:
    """One ``dnsplat_mesh_clusters`` call; nothing is read on the host."""
    triangles, V = _device_triangles(triangles, n_vertices)
    dev, T = triangles.device, triangles.shape[0]
    L = _lib.lib()
    nbytes = L.dnsplat_mesh_clusters_scratch_bytes(V, T)
    if nbytes == 0:
        raise ValueError(f"a mesh of {T} triangles is beyond the edge table's index ({(2 ** 31 - 1) // 4} triangles at the most)")
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    out = ClusterBuffers(torch.empty(T, dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.int32, device=dev),
                         torch.empty(2, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    a = _mesh_clusters_args(V, triangles, scratch, out.labels, out.sizes, out.counts, out.status)
    _lib.run("dnsplat_mesh_clusters", L.dnsplat_mesh_clusters, ctypes.byref(a), _stream())
    return out


@torch.no_grad()
def cluster_connected_triangles(triangles: Tensor, n_vertices: int) -> Tuple[Tensor, Tensor]:
    """Open3D's ``cluster_connected_triangles`` without its areas: (labels int32 [T], sizes int32 [n_clusters]) on the device.
    ``labels[t]`` is -1 for a triangle with an index outside [0, n_vertices); clusters are numbered in ascending order of their lowest
    triangle.  One host read, of ``n_clusters``."""
    b = cluster_buffers(triangles, n_vertices)
    return b.labels, b.sizes[:int(b.counts[0].item())]


@torch.no_grad()
def filter_small_clusters(mesh, keep_largest: int = KEEP_LARGEST, min_triangles: int = MIN_TRIANGLES, return_index: bool = False):
    """The reference's filter (:1021-1039) on ``mesh`` = (vertices, triangles, *per_vertex), as ``marching_cubes_mesh`` and
    ``TSDFVolume.extract_mesh`` return it: every triangle of a cluster with fewer than ``max(min_triangles, the keep_largest-th
    largest cluster size)`` triangles goes, degenerate triangles go, unreferenced vertices go; what stays keeps its order.  With fewer
    than ``keep_largest`` clusters the threshold is ``min_triangles`` (the reference's ``[-50]`` raises IndexError there).  Returns the
    same tuple shape: vertices and every further per-vertex tensor (any dtype, [V, ...]) gathered, ``None`` items passed through,
    triangles int32 [T',3] remapped; with ``return_index`` a last item ``vertex_index`` int32 [V'], the old id of each kept vertex.
    One host read, of (V', T'); a filter that keeps nothing returns empty tensors."""
    keep_largest, min_triangles = int(keep_largest), int(min_triangles)
    if keep_largest < 1 or min_triangles < 1:
        raise ValueError(f"keep_largest and min_triangles must be at least 1, got {keep_largest} and {min_triangles}")
    vertices, per_vertex = mesh[0], tuple(mesh[2:])
    if not isinstance(vertices, Tensor):
        raise TypeError(f"mesh vertices must be a tensor on the GPU, got {type(vertices).__name__}")
    _need_gpu(vertices, "mesh vertices")
    triangles, V = _device_triangles(mesh[1], vertices.shape[0])
    for k, x in enumerate(per_vertex):
        if x is not None:
            _need_gpu(x, f"mesh[{k + 2}]")
            if x.shape[0] != V:
                raise ValueError(f"mesh[{k + 2}] has {x.shape[0]} rows for {V} vertices")
    dev, T = triangles.device, triangles.shape[0]
    b = cluster_buffers(triangles, V)
    L = _lib.lib()
    scratch = torch.empty((L.dnsplat_mesh_filter_scratch_bytes(V, T) + 7) // 8, dtype=torch.int64, device=dev)
    threshold = torch.empty(1, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    a = _mesh_filter_args(V, triangles, b.labels, b.sizes, b.counts, keep_largest, min_triangles, scratch, threshold, counts)
    _lib.run("dnsplat_mesh_filter_count", L.dnsplat_mesh_filter_count, ctypes.byref(a), _stream())
    n_v, n_t = counts.tolist()                                                  # the one synchronisation
    vertex_index = torch.empty(n_v, dtype=torch.int32, device=dev)
    out_t = torch.empty(n_t, 3, dtype=torch.int32, device=dev)
    if n_t > 0:
        status = torch.empty(1, dtype=torch.int32, device=dev)
        a = _mesh_filter_args(V, triangles, b.labels, b.sizes, b.counts, keep_largest, min_triangles, scratch, threshold, counts, vertex_index,
                              out_t, status)
        _lib.run("dnsplat_mesh_filter_emit", L.dnsplat_mesh_filter_emit, ctypes.byref(a), _stream())
    index = vertex_index.to(torch.int64)
    gathered = tuple(None if x is None else x.index_select(0, index) for x in (vertices,) + per_vertex)
    result = (gathered[0], out_t) + gathered[1:]
    return result + (vertex_index,) if return_index else result


def _filter_arguments(filter_clusters):
    """``filter_clusters`` of ``TSDFVolume.extract_mesh`` / ``fuse_tsdf_mesh``: None -> None, True -> the reference's (50, 50), a pair."""
    if filter_clusters is None or filter_clusters is False:
        return None
    if filter_clusters is True:
        return KEEP_LARGEST, MIN_TRIANGLES
    keep_largest, min_triangles = filter_clusters
    return int(keep_largest), int(min_triangles)
