"""Point-cloud normals on HIP (``csrc/normals.hip``): Open3D's ``PointCloud.estimate_normals``, which the reference calls in two places.

  * The seed normals of its dataparsers (``_load_points3D_normals``: normal_nerfstudio.py:85-101, replica_dataparser.py:381,
    nrgbd_dataparser.py:378, scannetpp_dataparser.py:593, mushroom_dataparser.py:758, coolermap_dataparser.py:334,
    g_sdfstudio_dataparser.py:270): ``KDTreeSearchParamHybrid(radius=0.1, max_nn=30)``, ``normalize_normals()`` and the parser's
    transform — ``points3D_normals`` here.  dn_model.py:196-215 initialises the Gaussians' normals, flat scale and rotations from them.
  * The normals of a sensor depth frame (scripts/depth_to_normal.py:150-213, scripts/depth_normal_consistency.py:171-221):
    back-projection, ``KDTreeSearchParamKNN(knn=200)`` over every pixel, the flip towards the camera and the 10-degree mask against the
    monocular normals — ``depth_normals`` and ``normal_consistency_mask`` here.

``estimate_normals`` is ONE launch, one wave per point: an exact k-NN selection of up to 256 neighbours over ``density.KnnIndex``, the
covariance in float64 and its smallest eigenvector.  The rule is stated in ``include/dnsplat.h`` and restated in ``torch_normals``: IT IS
THIS PROJECT'S DEFINITION, PARITY UNPINNED AGAINST Open3D.  Deliberate deviations: the covariance is two passes about the mean (Open3D
uses cumulants), the sign without ``orient_toward`` is canonical (Open3D's is arbitrary), and ``depth_normals`` leaves pixels without a
depth out of the cloud (the reference sends them all to the camera centre).

Out of scope: a pure radius search with unbounded count, ``orient_normals_consistent_tangent_plane``, covariance-weighted or
fast-approximate normals, Poisson reconstruction, PLY input and output.  CPU tensors are refused; there is no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch
from torch import Tensor

from . import _lib, torch_normals
from ._ops import _cloud_normals_args, _need_gpu, _stream
from .cloud_filter import _device_cloud
from .density import KnnIndex
from .torch_normals import MAX_K, MIN_K, check_arguments, normal_consistency_mask  # noqa: F401

STATUS_INTERNAL = 1                                                                # DNSPLAT_NORMALS_STATUS_INTERNAL
SEARCH_WORDS = 4                                                                   # the scratch: int32 [4]


def _toward(orient_toward):
    if orient_toward is None:
        return None
    if isinstance(orient_toward, Tensor) and orient_toward.is_cuda:
        raise TypeError("orient_toward must be three numbers on the host (a tuple, a list, an array or a CPU tensor): a device tensor "
                        "would have to be read before the launch")
    c = tuple(float(v) for v in orient_toward)
    if len(c) != 3 or any(v != v for v in c):
        raise ValueError(f"orient_toward must be three numbers, none of them nan, got {orient_toward}")
    return c


def _launch(points: Tensor, knn: int, radius, toward, index, want_covariance: bool, want_neighbors: bool):
    """The one launch: ``(normals, covariance or None, neighbors or None, count or None, status int32 [1], search int32 [4])``, all on
    the device, nothing read.  ``search`` is the scratch: the widest ring a query reached and the most selections one query ran."""
    points = _device_cloud(points, "points")
    N, dev = points.shape[0], points.device
    if index is None:
        index = KnnIndex(points)
    elif not isinstance(index, KnnIndex):
        raise TypeError(f"index must be a KnnIndex, got {type(index).__name__}")
    if index.N != N or index.device != dev:
        raise ValueError(f"the index is over {index.N} points on {index.device}, the cloud has {N} on {dev}")
    L = _lib.lib()
    words = (L.dnsplat_cloud_normals_scratch_bytes(N, knn) + 3) // 4
    if words < SEARCH_WORDS:
        raise _lib.DnsplatError(f"dnsplat_cloud_normals_scratch_bytes({N}, {knn}) = {4 * words}")
    search = torch.zeros(words, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    normals = torch.empty(N, 3, dtype=torch.float64, device=dev)
    want_count = want_covariance or want_neighbors
    covariance = torch.empty(N, 6, dtype=torch.float64, device=dev) if want_covariance else None
    neighbors = torch.empty(N, knn, dtype=torch.int32, device=dev) if want_neighbors else None
    count = torch.empty(N, dtype=torch.int32, device=dev) if want_count else None
    a = _cloud_normals_args(points, index.buffer, knn, radius, toward, search, normals, status, covariance, neighbors, count)
    _lib.run("dnsplat_cloud_normals", L.dnsplat_cloud_normals, ctypes.byref(a), _stream())
    return normals, covariance, neighbors, count, status, search


@torch.no_grad()
def estimate_normals(points: Tensor, knn: int = 30, radius: Optional[float] = None, orient_toward=None, index: Optional[KnnIndex] = None,
                     return_covariance: bool = False, return_neighbors: bool = False):
    """Open3D's ``estimate_normals`` on ``points`` [N,3] on the device: ``normals`` float64 [N,3] (Open3D's normals are doubles), then
    ``covariance`` float64 [N,6] (xx, xy, xz, yy, yz, zz) with ``return_covariance``, ``neighbors`` int32 [N,knn] (ascending by
    (d², index), -1 past the count) with ``return_neighbors``, and ``count`` int32 [N] if either was asked for.

    ``knn=200`` is ``KDTreeSearchParamKNN(200)``; ``knn=30, radius=0.1`` is ``KDTreeSearchParamHybrid(0.1, 30)``: of the ``knn`` nearest
    (the point itself included) those with ``d² < radius²``.  Fewer than three neighbours give (0, 0, 1).  ``orient_toward`` (three
    numbers on the host) is ``orient_normals_towards_camera_location``; without it the sign is canonical (largest component positive).
    ``index`` is a ``KnnIndex`` of the same points (one is built otherwise).  No host read except ``status``, once, after the launch."""
    knn, radius = check_arguments(knn, radius)
    toward = _toward(orient_toward)
    normals, covariance, neighbors, count, status, _ = _launch(points, knn, radius, toward, index, return_covariance, return_neighbors)
    result = (normals,) + ((covariance,) if return_covariance else ()) + ((neighbors,) if return_neighbors else ())
    result += (count,) if count is not None else ()
    code = int(status.item())                                                     # the one host read, last
    if code:
        raise _lib.DnsplatError(f"estimate_normals: internal status {code} (a bounded loop ran out)")
    return result[0] if len(result) == 1 else result


def _estimate_for_restatement(points, knn=30, radius=None, orient_toward=None):
    return (estimate_normals(points, knn=knn, radius=radius, orient_toward=orient_toward),)


@torch.no_grad()
def points3D_normals(points: Tensor, transform_matrix=None, knn: int = 30, radius: Optional[float] = 0.1) -> Tensor:
    """The dataparsers' seed normals (``_load_points3D_normals``) of ``points`` [N,3] on the device: float32 [N,3], the normals of the
    hybrid search (0.1, 30), normalised.  With a 3x4 ``transform_matrix`` the result is ``cat(normals, 1) @ transform_matrix.T`` — THE
    REFERENCE'S STATEMENT, which adds the translation to a direction; it is reproduced, not corrected."""
    _device_cloud(points, "points")
    return torch_normals.points3D_normals(points, transform_matrix, knn, radius, estimate=_estimate_for_restatement)


@torch.no_grad()
def depth_normals(depth: Tensor, fx: float, fy: float, cx: float, cy: float, c2w, knn: int = 200):
    """scripts/depth_to_normal.py:150-181 for one frame: ``(normals float64 [H,W,3], valid bool [H,W])``.  ``depth`` [H,W] on the
    device; ``c2w`` the OpenCV camera-to-world (host, 3x4 or 4x4).  Every pixel is back-projected exactly as the reference's
    ``backproject`` does (float32 in the camera, float64 into the world), the normals of the ``knn`` nearest points are estimated and
    each is turned towards the camera centre.  DELIBERATE DEVIATION: pixels with ``depth <= 0`` or a non-finite depth are removed
    before the index is built — their normal is (0, 0, 0) and ``valid`` is False — where the reference sends them all to the camera
    centre, hundreds of thousands of identical points in one grid cell that every query there would scan.  One host read beside
    ``status``: the number of valid pixels."""
    if not isinstance(depth, Tensor):
        raise TypeError(f"depth must be a tensor on the GPU, got {type(depth).__name__}")
    _need_gpu(depth, "depth")
    if depth.dim() != 2:
        raise ValueError(f"depth must be [H,W], got {tuple(depth.shape)}")
    return torch_normals.depth_normals(depth, fx, fy, cx, cy, c2w, knn, estimate=_estimate_for_restatement)
