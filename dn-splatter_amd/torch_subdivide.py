"""The subdivision of long triangles, restated on the CPU: the rule ``include/dnsplat.h`` states for ``dnsplat_subdivide_count`` /
``dnsplat_subdivide_emit`` — trimesh's ``remesh.subdivide_to_size``, the first step of the reference's ``cull_mesh``
(eval_mesh_vis_cull.py:190-193) — in whole-array torch operations with the kernels' order of floating-point operations, so that
``csrc/subdivide.hip`` can be held to it with exact equality (``tests/test_gpu_subdivide.py``).  IT IS THIS PROJECT'S DEFINITION, PARITY
UNPINNED AGAINST trimesh, which is not at hand; ``tests/test_subdivide_reference.py`` holds it to an independent numpy statement written
the way trimesh's text reads and to invariants that need no restatement.

The state is the current vertices ``cv`` float64, the current triangles ``cf`` and the origin ``ci`` of each.  Per round: a triangle is
long iff some edge has ``sqrt((dx dx + dy dy) + dz dz) > max_edge`` (strictly; a nan is not long); the others leave with the vertices
they reference, in ascending index order and remapped; no long triangle ends the call, long ones in round ``max_iter`` raise; each
distinct undirected edge of the long triangles gets one midpoint ``(cv[lo] + cv[hi]) / 2`` below all current vertices, numbered by
first appearance over the slots ``3 t + e`` (``midpoint_order="first"``, what the kernels do) or by ``(lo, hi)`` ascending
(``"sorted"``: other numbers, the same triangle soup); a long triangle (a, b, c) becomes (a, m0, m2), (m0, b, m1), (m2, m1, c),
(m0, m1, m2)."""
from __future__ import annotations

from typing import List, Optional

import torch
from torch import Tensor


def edge_lengths(vertices: Tensor, triangles: Tensor) -> Tensor:
    """float64 [T,3]: the lengths of the edges 0->1, 1->2, 2->0 by the stated formula, one rounding per operation."""
    p = vertices.to(torch.float64)[triangles.to(torch.int64)]                   # [T,3,3]
    d = p[:, [1, 2, 0]] - p
    return torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _checked(vertices, triangles, max_edge, max_iter):
    vertices, triangles = torch.as_tensor(vertices), torch.as_tensor(triangles)
    if not vertices.dtype.is_floating_point or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices must be a floating-point [V,3] tensor, got {vertices.dtype} {tuple(vertices.shape)}")
    if triangles.dtype.is_floating_point or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError(f"triangles must be an integer [T,3] tensor, got {triangles.dtype} {tuple(triangles.shape)}")
    max_edge, max_iter = float(max_edge), int(max_iter)
    if not 0.0 < max_edge < float("inf"):
        raise ValueError(f"max_edge must be positive and finite, got {max_edge}")
    if max_iter < 0:
        raise ValueError(f"max_iter must not be negative, got {max_iter}")
    return vertices, triangles, max_edge, max_iter


@torch.no_grad()
def subdivide_to_size(vertices, triangles, max_edge: float, max_iter: int = 10, return_index: bool = False,
                      midpoint_order: str = "first", rounds: Optional[List] = None):
    """(vertices float64 [V',3], triangles int32 [T',3][, face_index int32 [T']]) on the CPU.  ``rounds``, a list, receives per round
    ``(triangles, long triangles, current vertices, done vertices)``."""
    if midpoint_order not in ("first", "sorted"):
        raise ValueError(f'midpoint_order is "first" or "sorted", got {midpoint_order!r}')
    vertices, triangles, max_edge, max_iter = _checked(vertices, triangles, max_edge, max_iter)
    cv = vertices.detach().cpu().to(torch.float64)
    cf = triangles.detach().cpu().to(torch.int64)
    if cf.numel() and (int(cf.min()) < 0 or int(cf.max()) >= cv.shape[0]):
        raise ValueError(f"a triangle has a vertex index outside [0, {cv.shape[0]})")
    ci = torch.arange(cf.shape[0], dtype=torch.int64)
    out_v, out_t, out_i, base = [], [], [], 0
    for r in range(max_iter + 1):
        V = cv.shape[0]
        is_long = (edge_lengths(cv, cf) > max_edge).any(dim=1)
        done = cf[~is_long]
        marks = torch.zeros(V, dtype=torch.bool)
        marks[done.reshape(-1)] = True
        new_id = torch.cumsum(marks, 0) - 1
        out_v.append(cv[marks])
        out_t.append(new_id[done] + base)
        out_i.append(ci[~is_long])
        n_done_v = int(marks.sum())
        base += n_done_v
        if rounds is not None:
            rounds.append((cf.shape[0], int(is_long.sum()), V, n_done_v))
        if not bool(is_long.any()):
            break
        if r == max_iter:
            raise ValueError("max_iter exceeded")
        lf = cf[is_long]                                                         # [n,3]
        a, b = lf.reshape(-1), lf[:, [1, 2, 0]].reshape(-1)                      # slot 3 t + e: the edge e of long triangle t
        key = (torch.minimum(a, b) << 32) | torch.maximum(a, b)
        uniq, inverse = torch.unique(key, return_inverse=True)                   # ascending (lo, hi)
        if midpoint_order == "first":
            first = torch.full((uniq.shape[0],), key.shape[0], dtype=torch.int64)
            first.scatter_reduce_(0, inverse, torch.arange(key.shape[0], dtype=torch.int64), "amin")
            order = torch.argsort(first)                                         # the first slots are distinct
            rank = torch.empty_like(order)
            rank[order] = torch.arange(order.shape[0], dtype=torch.int64)
            uniq, inverse = uniq[order], rank[inverse]
        mid = (cv[uniq >> 32] + cv[uniq & 0xffffffff]) / 2.0
        m = (V + inverse).reshape(-1, 3)
        m0, m1, m2 = m[:, 0], m[:, 1], m[:, 2]
        cf = torch.stack([lf[:, 0], m0, m2, m0, lf[:, 1], m1, m2, m1, lf[:, 2], m0, m1, m2], dim=1).reshape(-1, 3)
        ci = ci[is_long].repeat_interleave(4)
        cv = torch.cat([cv, mid])
    result = (torch.cat(out_v), torch.cat(out_t).to(torch.int32))
    return result + (torch.cat(out_i).to(torch.int32),) if return_index else result


def subdivide_mesh(mesh, max_edge: float, max_iter: int = 10, midpoint_order: str = "first"):
    """``subdivide.subdivide_mesh`` on CPU tensors: (vertices float64, triangles int32) of a (vertices, triangles, ...) tuple."""
    return subdivide_to_size(mesh[0], mesh[1], max_edge, max_iter, midpoint_order=midpoint_order)
