"""The subdivision of long triangles on HIP (``csrc/subdivide.hip``): the first thing the reference's ``cull_mesh`` does
(dn_splatter/eval/eval_mesh_vis_cull.py:190-193, with ``subdivide=True`` for both meshes at :439-464) —
``trimesh.remesh.subdivide_to_size(vertices, triangles, max_edge=0.015, max_iter=10)``.  The cull votes per vertex and keeps a triangle
if one of its vertices was seen often enough: a scan's or a TSDF mesh's wall triangle, metres long, survives on one visible corner unless
it is split first.  trimesh is not on a ROCm box, and the alternative there is a device-to-host copy, a numpy loop and a copy of a few
million triangles back.

  * ``subdivide_to_size``: round after round, every triangle with an edge longer than ``max_edge`` becomes four, the others leave with
    the vertices they reference; per round ``dnsplat_subdivide_count``, ONE host read (the four counts and the status word beside
    them), ``dnsplat_subdivide_emit``;
  * ``subdivide_mesh``: the same on a (vertices, triangles, ...) tuple — what ``marching_cubes_mesh`` and ``TSDFVolume.extract_mesh``
    return;
  * ``mesh_cull.cull_mesh(..., subdivide=True)`` runs it in front of the votes.

The rule is stated in ``include/dnsplat.h`` and restated on the CPU in ``torch_subdivide``: IT IS THIS PROJECT'S DEFINITION, PARITY
UNPINNED AGAINST trimesh.  All arithmetic is float64 (float32 vertices are promoted exactly), outputs are float64.  trimesh numbers the
midpoints by a row hash; here they are numbered by first appearance, which changes indices and not the triangle soup.  The current
vertices are not compacted between rounds.

Out of scope: vertex attributes through the subdivision beyond ``face_index``, Loop smoothing (``subdivide_loop``), welding the
vertices that done triangles of several rounds share, mesh files.  CPU tensors are refused; there is no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._ops import _need_gpu, _stream, _subdivide_args
from .torch_subdivide import _checked

STATUS_INTERNAL, STATUS_INDEX, STATUS_CAPACITY = 1, 2, 4    # DNSPLAT_SUBDIVIDE_STATUS_*
INT_MAX = 2 ** 31 - 1
MAX_TRIANGLES = INT_MAX // 4                                # of one round: the edge table has four slots per triangle, indexed by int32


def _on_device(x, name: str) -> Tensor:
    if isinstance(x, Tensor):
        _need_gpu(x, name)
        return x.detach()
    if not torch.cuda.is_available():
        raise _lib.DnsplatError(f"{name}: the subdivision runs only on the GPU through libdnsplat.so (there is no CPU fallback)")
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x))).to(torch.device("cuda", torch.cuda.current_device()))


@torch.no_grad()
def subdivide_to_size(vertices, triangles, max_edge: float, max_iter: int = 10, return_index: bool = False,
                      rounds: Optional[List] = None):
    """``trimesh.remesh.subdivide_to_size``: (vertices float64 [V',3], triangles int32 [T',3]) on the device, every edge at most
    ``max_edge`` long; with ``return_index`` a third item ``face_index`` int32 [T'], the input triangle each output triangle is part of.
    Triangles that are still long after ``max_iter`` rounds raise ``ValueError("max_iter exceeded")``, as trimesh does, and so does a
    vertex index outside [0, V).  One host read per round; ``rounds``, a list, receives per round ``(triangles, long triangles, current
    vertices, done vertices)``.  ``T = 0`` returns empty tensors."""
    vertices, triangles = _on_device(vertices, "vertices"), _on_device(triangles, "triangles")
    vertices, triangles, max_edge, max_iter = _checked(vertices, triangles, max_edge, max_iter)
    dev = vertices.device
    if triangles.device != dev:
        raise ValueError(f"vertices are on {dev} and triangles on {triangles.device}")
    cv = vertices.to(torch.float64).contiguous()
    cf = triangles.to(torch.int32).contiguous()
    if cf.shape[0] == 0:
        empty = (torch.empty(0, 3, dtype=torch.float64, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev))
        return empty + (torch.empty(0, dtype=torch.int32, device=dev),) if return_index else empty
    if cv.shape[0] == 0:
        raise ValueError("a triangle has a vertex index outside [0, 0)")
    ci = torch.arange(cf.shape[0], dtype=torch.int32, device=dev)
    L = _lib.lib()
    word = torch.zeros(5, dtype=torch.int64, device=dev)                        # the four counts, and the status word in the fifth
    counts, status = word[:4], word[4:]
    out_v, out_t, out_i, base = [], [], [], 0
    for r in range(max_iter + 1):
        V, T = cv.shape[0], cf.shape[0]
        if T > MAX_TRIANGLES:
            raise ValueError(f"round {r}: {T} triangles are beyond the edge table's index ({MAX_TRIANGLES} triangles at the most)")
        scratch = torch.empty((L.dnsplat_subdivide_scratch_bytes(V, T) + 7) // 8, dtype=torch.int64, device=dev)
        a = _subdivide_args(cv, cf, ci, max_edge, scratch, counts, status)
        _lib.run("dnsplat_subdivide_count", L.dnsplat_subdivide_count, ctypes.byref(a), _stream())
        n_v, n_t, n_long, n_mid, flags = word.tolist()                          # the round's one synchronisation
        if flags & STATUS_INDEX:
            raise ValueError(f"round {r}: a triangle has a vertex index outside [0, {V})")
        if flags:
            raise _lib.DnsplatError(f"round {r}: dnsplat_subdivide left status {flags} (a bounded loop ran out: a build error)")
        if rounds is not None:
            rounds.append((T, n_long, V, n_v))
        if n_long > 0 and r == max_iter:
            raise ValueError("max_iter exceeded")
        if 4 * n_long > MAX_TRIANGLES or V + n_mid > INT_MAX or base + n_v > INT_MAX:
            raise ValueError(f"round {r}: {4 * n_long} children, {V + n_mid} current and {base + n_v} emitted vertices are beyond the int32 "
                             f"indices ({MAX_TRIANGLES} children, {INT_MAX} vertices at the most)")
        done_v = torch.empty(n_v, 3, dtype=torch.float64, device=dev)
        done_t = torch.empty(n_t, 3, dtype=torch.int32, device=dev)
        done_i = torch.empty(n_t, dtype=torch.int32, device=dev)
        next_v = next_t = next_i = None
        if n_long > 0:
            next_v = torch.empty(V + n_mid, 3, dtype=torch.float64, device=dev)
            next_t = torch.empty(4 * n_long, 3, dtype=torch.int32, device=dev)
            next_i = torch.empty(4 * n_long, dtype=torch.int32, device=dev)
        a = _subdivide_args(cv, cf, ci, max_edge, scratch, counts, status, base, done_v, done_t, done_i, next_v, next_t, next_i)
        _lib.run("dnsplat_subdivide_emit", L.dnsplat_subdivide_emit, ctypes.byref(a), _stream())
        out_v.append(done_v)
        out_t.append(done_t)
        out_i.append(done_i)
        base += n_v
        if n_long == 0:
            break
        cv, cf, ci = next_v, next_t, next_i
    result = (torch.cat(out_v), torch.cat(out_t))
    return result + (torch.cat(out_i),) if return_index else result


@torch.no_grad()
def subdivide_mesh(mesh, max_edge: float, max_iter: int = 10):
    """``subdivide_to_size`` on ``mesh`` = (vertices, triangles, ...), tensors on the device or arrays: (vertices float64 [V',3],
    triangles int32 [T',3]).  Further per-vertex items of the tuple are not carried through."""
    return subdivide_to_size(mesh[0], mesh[1], max_edge, max_iter)
