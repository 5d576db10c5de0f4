"""The connected-component filter of a mesh, restated on the CPU: what ``csrc/meshclusters.hip`` computes, in plain numpy / PyTorch and
one triangle after the other, so that the kernels can be held to it with exact equality (``tests/test_gpu_mesh_clusters.py``).  The
definition is the one ``include/dnsplat.h`` states (the step the reference's ``Open3DTSDFFusion`` ends with, export_mesh.py:1021-1039:
Open3D's ``cluster_connected_triangles``, ``n = max(np.sort(cluster_n_triangles)[-50], 50)``, the removal of every triangle of a
cluster with fewer than ``n``, ``remove_unreferenced_vertices``, ``remove_degenerate_triangles``).  Open3D is not at hand: IT IS THIS
PROJECT'S DEFINITION, PARITY UNPINNED AGAINST Open3D.

  * a triangle is valid iff all three indices are in [0, V); an invalid one has label -1 and is never kept;
  * two valid triangles are connected iff they share an undirected edge with two different ends (a shared vertex alone does not
    connect, winding does not matter, duplicate rows are connected, an edge of three or more triangles connects them all);
  * clusters are the connected components, numbered in ascending order of their lowest triangle; ``sizes[c]`` counts the valid
    triangles of cluster c, degenerate ones included;
  * ``threshold = max(min_triangles, the keep_largest-th largest size)`` with ``keep_largest`` clusters or more, ``min_triangles``
    with fewer (where the reference's ``[-50]`` raises IndexError);
  * a triangle is kept iff it is valid, has three distinct indices and ``sizes[labels[t]] >= threshold``; a vertex iff a kept
    triangle references it; both stay in their order, indices are remapped.  Open3D compacts the vertices before it drops the
    degenerate triangles and can leave a vertex only a degenerate triangle referenced: this leaves none — the one deviation;
  * ``cluster_area``, the third result of Open3D's call, is not produced: the reference's filter never reads it.

The union-find below is sequential and its own (a dictionary of edges, union by lowest index, path compression); it uses no graph
library, so that scipy's ``connected_components`` stays an independent witness in ``tests/test_mesh_clusters_reference.py``."""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch
from torch import Tensor

KEEP_LARGEST = 50                                           # export_mesh.py:1030, the [-50]
MIN_TRIANGLES = 50                                          # :1031


def _triangles(triangles) -> np.ndarray:
    t = triangles.detach().cpu().numpy() if isinstance(triangles, Tensor) else np.asarray(triangles)
    if t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in "iu":
        raise ValueError(f"triangles must be an integer [T,3] array, got {t.dtype} {t.shape}")
    return t.astype(np.int64)


def valid_triangles(triangles, n_vertices: int) -> np.ndarray:
    """bool [T]: all three indices in [0, n_vertices)."""
    t = _triangles(triangles)
    return ((t >= 0) & (t < int(n_vertices))).all(axis=1)


def cluster_connected_triangles(triangles, n_vertices: int) -> Tuple[Tensor, Tensor]:
    """(labels int32 [T], sizes int32 [n_clusters]) on the CPU."""
    t = _triangles(triangles)
    T = t.shape[0]
    valid = valid_triangles(t, n_vertices)
    parent = list(range(T))

    def find(x: int) -> int:
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:                               # path compression
            parent[x], x = r, parent[x]
        return r

    first = {}                                              # undirected edge -> the first triangle that had it
    rows = t.tolist()
    for i in range(T):
        if not valid[i]:
            continue
        a, b, c = rows[i]
        for u, v in ((a, b), (b, c), (c, a)):
            if u == v:
                continue
            e = (u, v) if u < v else (v, u)
            j = first.setdefault(e, i)
            if j != i:
                ri, rj = find(i), find(j)
                if ri != rj:
                    parent[max(ri, rj)] = min(ri, rj)       # the root is the lowest triangle of its tree
    labels = np.full(T, -1, dtype=np.int32)
    number = {}
    sizes = []
    for i in range(T):                                      # ascending i: a root comes before every other triangle of its cluster
        if not valid[i]:
            continue
        r = find(i)
        if r not in number:
            number[r] = len(sizes)
            sizes.append(0)
        labels[i] = number[r]
        sizes[number[r]] += 1
    return torch.from_numpy(labels), torch.tensor(sizes, dtype=torch.int32)


def size_threshold(sizes, keep_largest: int = KEEP_LARGEST, min_triangles: int = MIN_TRIANGLES) -> int:
    """``max(min_triangles, the keep_largest-th largest of sizes)``; ``min_triangles`` with fewer than ``keep_largest`` clusters."""
    keep_largest, min_triangles = int(keep_largest), int(min_triangles)
    if keep_largest < 1 or min_triangles < 1:
        raise ValueError(f"keep_largest and min_triangles must be at least 1, got {keep_largest} and {min_triangles}")
    s = np.sort(np.asarray(sizes, dtype=np.int64).reshape(-1))
    return max(min_triangles, int(s[-keep_largest])) if s.size >= keep_largest else min_triangles


def filter_triangles(triangles, n_vertices: int, keep_largest: int = KEEP_LARGEST, min_triangles: int = MIN_TRIANGLES, clusters=None):
    """The whole filter on indices: (threshold int, keep bool [T], vertex_index int32 [V'], triangles int32 [T',3]) on the CPU —
    ``vertex_index`` holds the old id of each kept vertex, the returned triangles index the kept vertices.  ``clusters``: the
    (labels, sizes) of ``cluster_connected_triangles`` for the same mesh, if the caller has them already."""
    t = _triangles(triangles)
    labels, sizes = cluster_connected_triangles(t, n_vertices) if clusters is None else clusters
    labels, sizes = np.asarray(labels), np.asarray(sizes)
    threshold = size_threshold(sizes, keep_largest, min_triangles)
    distinct = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    keep = (labels >= 0) & distinct
    keep[keep] = sizes[labels[keep]] >= threshold
    used = np.zeros(int(n_vertices), dtype=bool)
    used[t[keep].reshape(-1)] = True
    vertex_index = np.flatnonzero(used)
    new_id = np.full(int(n_vertices), -1, dtype=np.int64)
    new_id[vertex_index] = np.arange(vertex_index.size)
    out = new_id[t[keep]].reshape(-1, 3)
    return (threshold, torch.from_numpy(keep), torch.from_numpy(vertex_index.astype(np.int32)), torch.from_numpy(out.astype(np.int32)))


def filter_small_clusters(mesh, keep_largest: int = KEEP_LARGEST, min_triangles: int = MIN_TRIANGLES, return_index: bool = False):
    """``mesh_clusters.filter_small_clusters`` on CPU tensors: ``mesh`` is (vertices, triangles, *per_vertex); every per-vertex tensor
    is gathered, ``None`` items pass through."""
    vertices, triangles = mesh[0], mesh[1]
    _, _, vertex_index, out = filter_triangles(triangles, vertices.shape[0], keep_largest, min_triangles)
    index = vertex_index.to(torch.int64)
    gathered = tuple(None if x is None else torch.as_tensor(x).index_select(0, index) for x in (vertices,) + tuple(mesh[2:]))
    result = (gathered[0], out) + gathered[1:]
    return result + (vertex_index,) if return_index else result
