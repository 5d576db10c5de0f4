"""The reference's mesh alignment on HIP (``csrc/icp.hip``): ``get_align_transformation`` of
dn_splatter/eval/eval_mesh_vis_cull.py:269-287, the step ``main`` (:427-431) runs with ``align=True`` before it culls and scores both
meshes — Open3D's ``registration_icp(source, target, 0.1, identity, TransformationEstimationPointToPoint)`` of the predicted mesh's
vertices onto the ground truth's.  Open3D is not on a ROCm box, and the alternative is a copy of millions of vertices to the host and a
CPU k-d tree per pass.

  * ``registration_icp``: up to ``max_iteration + 1`` passes, each the nearest-neighbour search of ``density.KnnIndex`` over the target
    plus a fixed-order float64 fold of the moments and a 3 x 3 rigid solve in one workgroup; the stop test runs on the device and the
    launches after it return at their first load, so the host reads ONCE, the 192-byte state at the end;
  * ``get_align_transformation``: the reference's function on ``(vertices, triangles, ...)`` tuples;
  * ``transform_points`` / ``transform_mesh``: ``fl32(T p)`` through ``dnsplat_transform_points``; normals take the rotation alone.

The rule is stated in ``include/dnsplat.h`` and restated in ``torch_icp``: IT IS THIS PROJECT'S DEFINITION, PARITY UNPINNED AGAINST
Open3D.  One deviation is deliberate: every pass transforms the ORIGINAL source by the accumulated transform, where Open3D transforms the
transformed cloud again and lets the roundings pile up in the points.

Out of scope: point-to-plane and coloured ICP, scaling, RANSAC / global registration, mesh file input and output.  CPU tensors are
refused; there is no CPU fallback."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._ops import _icp_args, _need_gpu, _ptr, _stream
from .density import KnnIndex
from .torch_icp import MAX_ITERATION, RELATIVE_FITNESS, RELATIVE_RMSE, STATUS_DEGENERATE, STATUS_NO_CORRESPONDENCE, THRESHOLD

STATE_WORDS = 24                                          # DNSPLAT_ICP_STATE_BYTES / 8
STATE_T, STATE_FITNESS, STATE_RMSE, STATE_N, STATE_ITERATIONS, STATE_DONE, STATE_STATUS, STATE_PASSES = 0, 16, 17, 18, 19, 20, 21, 22


def _device_cloud(points, name: str) -> Tensor:
    if not isinstance(points, Tensor):
        raise TypeError(f"{name} must be a tensor on the GPU, got {type(points).__name__}")
    _need_gpu(points, name)
    if not points.dtype.is_floating_point or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{name} must be a floating-point [n,3] tensor, got {points.dtype} {tuple(points.shape)}")
    if points.shape[0] < 1:
        raise ValueError(f"{name} is empty")
    return points.detach().to(torch.float32).contiguous()


def _host_matrix(T, name: str) -> Optional[np.ndarray]:
    if T is None:
        return None
    T = np.ascontiguousarray(np.asarray(T.detach().cpu() if isinstance(T, Tensor) else T, dtype=np.float64))
    if T.shape != (4, 4):
        raise ValueError(f"{name} must be [4,4], got {T.shape}")
    if not np.isfinite(T).all():
        raise ValueError(f"{name} has a non-finite entry")
    return T


def _check_arguments(max_correspondence_distance, relative_fitness, relative_rmse, max_iteration):
    r, rf, rr, it = float(max_correspondence_distance), float(relative_fitness), float(relative_rmse), int(max_iteration)
    if not (r > 0.0 and r < math.inf):
        raise ValueError(f"max_correspondence_distance must be positive and finite, got {max_correspondence_distance}")
    if rf != rf or rr != rr:
        raise ValueError("a relative tolerance is nan")
    if it < 0:
        raise ValueError(f"max_iteration must be >= 0, got {max_iteration}")
    return r, rf, rr, it


class ICPResult:
    """What the loop left on the device: ``transformation`` float64 [4,4] (a view of the state), ``state`` (24 words), ``trace`` float64
    [max_iteration + 1, 4] or None (rows ``(n, fitness, rmse, stopped)``; ``passes`` of them are written, the rest is 0), ``idx`` int32 [M]
    (-1: no correspondence) and ``dist2`` float64 [M] of the last pass.  ``fitness``, ``inlier_rmse``, ``iterations`` (updates applied),
    ``n``, ``passes`` and ``status`` (0 on success; ``STATUS_NO_CORRESPONDENCE``, the advisory ``STATUS_DEGENERATE``) come from the ONE
    host copy of the state ``registration_icp`` makes."""

    def __init__(self, state: Tensor, host, trace, idx, dist2):
        self.state, self.trace, self.idx, self.dist2 = state, trace, idx, dist2
        self.transformation = state[:16].view(4, 4)
        words = host.view(torch.int64)
        self.fitness, self.inlier_rmse = float(host[STATE_FITNESS]), float(host[STATE_RMSE])
        self.n, self.iterations, self.passes = int(words[STATE_N]), int(words[STATE_ITERATIONS]), int(words[STATE_PASSES])
        self.status = int(words[STATE_STATUS])
        self.done = bool(words[STATE_DONE])

    @property
    def correspondence_set(self) -> Tensor:
        """int64 [n,2]: (source row, target row) of the last pass, ascending by source row — Open3D's ``correspondence_set``."""
        rows = torch.nonzero(self.idx >= 0).reshape(-1)
        return torch.stack([rows, self.idx[rows].to(torch.int64)], dim=-1)


@torch.no_grad()
def registration_icp(source: Tensor, target, max_correspondence_distance: float, init=None, relative_fitness: float = RELATIVE_FITNESS,
                     relative_rmse: float = RELATIVE_RMSE, max_iteration: int = MAX_ITERATION, index: Optional[KnnIndex] = None,
                     return_trace: bool = False) -> ICPResult:
    """Open3D's ``registration_icp`` with ``TransformationEstimationPointToPoint`` on ``source`` [M,3] and ``target`` ([N,3] on the
    device, or a ``KnnIndex`` built over it; ``index`` is such an index of a ``target`` tensor, one is built otherwise): the rigid
    transform that takes the source onto the target, from ``init`` ([4,4], identity by default).  One ``dnsplat_icp_run`` call —
    ``3 + 2 max_iteration`` launches that the host does not watch — and one host read, of the state."""
    r, rf, rr, it = _check_arguments(max_correspondence_distance, relative_fitness, relative_rmse, max_iteration)
    source = _device_cloud(source, "source")
    if isinstance(target, KnnIndex):
        if index is not None and index is not target:
            raise ValueError("target is a KnnIndex already: give no other index")
        index, points = target, target.points()
    else:
        points = _device_cloud(target, "target")
        if index is None:
            index = KnnIndex(points)
        elif not isinstance(index, KnnIndex):
            raise TypeError(f"index must be a KnnIndex, got {type(index).__name__}")
        if index.N != points.shape[0]:
            raise ValueError(f"the index is over {index.N} points, the target has {points.shape[0]}")
    dev, M = source.device, source.shape[0]
    if index.device != dev or points.device != dev:
        raise ValueError(f"source is on {dev}, the target on {index.device}")
    init = _host_matrix(init, "init")
    L = _lib.lib()
    state = torch.empty(STATE_WORDS, dtype=torch.float64, device=dev)
    trace = torch.zeros(it + 1, 4, dtype=torch.float64, device=dev) if return_trace else None
    idx = torch.empty(M, dtype=torch.int32, device=dev)
    dist2 = torch.empty(M, dtype=torch.float64, device=dev)
    scratch = torch.empty(L.dnsplat_icp_scratch_bytes(M) // 8, dtype=torch.float64, device=dev)
    a = _icp_args(source, points, index.buffer, r, rf, rr, it, state, scratch, trace, idx, dist2)
    _lib.run("dnsplat_icp_run", L.dnsplat_icp_run, ctypes.byref(a), None if init is None else init.ctypes.data_as(ctypes.c_void_p), _stream())
    return ICPResult(state, state.cpu(), trace, idx, dist2)                       # the one synchronisation


@torch.no_grad()
def transform_points(points: Tensor, T, rotate_only: bool = False) -> Tensor:
    """float32 [n,3]: ``fl32(T p)`` for every row, each coordinate ``((T[a][0] x + T[a][1] y) + T[a][2] z) + T[a][3]`` in float64 and
    rounded once; with ``rotate_only`` the rotation block alone (normals).  ``T`` is [4,4]: a float64 tensor on the device
    (``ICPResult.transformation``) is read there, anything else is uploaded.  One ``dnsplat_transform_points`` call."""
    if not isinstance(points, Tensor):
        raise TypeError(f"points must be a tensor on the GPU, got {type(points).__name__}")
    _need_gpu(points, "points")
    if not points.dtype.is_floating_point or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be a floating-point [n,3] tensor, got {points.dtype} {tuple(points.shape)}")
    points = points.detach().to(torch.float32).contiguous()
    if isinstance(T, Tensor) and T.is_cuda:
        if tuple(T.shape) != (4, 4):
            raise ValueError(f"T must be [4,4], got {tuple(T.shape)}")
        T = T.detach().to(device=points.device, dtype=torch.float64).contiguous()
    else:
        T = torch.from_numpy(_host_matrix(T, "T")).to(points.device)
    out = torch.empty_like(points)
    L = _lib.lib()
    _lib.run("dnsplat_transform_points", L.dnsplat_transform_points, points.shape[0], _ptr(points), _ptr(T), _ptr(out), int(bool(rotate_only)),
             _stream())
    return out


@torch.no_grad()
def transform_mesh(mesh, T, normals_at: Optional[int] = None):
    """``mesh.transform(T)`` on a ``(vertices, triangles, ...)`` tuple: the vertices through ``transform_points``; triangles, colours and
    everything else pass through untouched.  The mesh tuples of this package carry no normals; a tuple that does names the position of
    its [V,3] normals entry with ``normals_at``, and that entry is rotated (``rotate_only``).  ``culled_mesh_metrics(align=True)`` passes
    none: ``cull_mesh`` and ``mesh_metrics`` read vertices and triangles alone and take their normals from the moved faces."""
    out = list(mesh)
    out[0] = transform_points(mesh[0] if isinstance(mesh[0], Tensor) else _as_device(mesh[0]), T)
    if normals_at is not None:
        if not 2 <= int(normals_at) < len(out):
            raise ValueError(f"normals_at = {normals_at} is no entry behind the triangles of a tuple of {len(out)}")
        out[normals_at] = transform_points(mesh[normals_at], T, rotate_only=True)
    return tuple(out)


def _as_device(x) -> Tensor:
    if not torch.cuda.is_available():
        raise _lib.DnsplatError("the mesh alignment runs only on the GPU through libdnsplat.so (there is no CPU fallback)")
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x))).to(torch.device("cuda", torch.cuda.current_device()))


@torch.no_grad()
def get_align_transformation(pred_mesh, gt_mesh, threshold: float = THRESHOLD) -> Tensor:
    """eval_mesh_vis_cull.py:269-287 on ``(vertices, triangles, ...)`` tuples: the float64 [4,4] device tensor that takes the predicted
    mesh's vertices onto the ground truth's — ``registration_icp`` at ``threshold`` from the identity with Open3D's default criteria."""
    pred = pred_mesh[0] if isinstance(pred_mesh[0], Tensor) else _as_device(pred_mesh[0])
    gt = gt_mesh[0] if isinstance(gt_mesh[0], (Tensor, KnnIndex)) else _as_device(gt_mesh[0])
    return registration_icp(pred, gt, threshold).transformation
