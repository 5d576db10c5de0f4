"""The reference's mesh visibility culling on HIP (``csrc/meshcull.hip``): ``cull_mesh`` of
dn_splatter/eval/eval_mesh_vis_cull.py:176-266, the step ``main`` (:439-464) runs on BOTH meshes before ``compute_metrics`` so that
only what the dataset's cameras could see is scored.

Where the reference renders depth maps with pyrender (OpenGL through EGL: no such path on a ROCm compute box), counts the votes in a
numpy loop over the poses and cuts with trimesh, this module keeps mesh, maps and votes on the device:

  * ``render_mesh_depth``: the double-sided depth render, ``dnsplat_mesh_depth`` — homogeneous edge functions in float64, no clipping,
    an integer ``atomicMin`` z-buffer: a canonical function of its inputs (``torch_mesh_cull`` states it; PARITY UNPINNED against
    pyrender's quantised z-buffer);
  * ``vertex_visibility``: ``get_grid_culling_pattern``, ``dnsplat_mesh_visibility``; the votes accumulate, so camera batches chain;
  * ``cut_mesh``: the triangle rule and ``remove_unreferenced_vertices``, ``dnsplat_mesh_cut_count`` / ``dnsplat_mesh_cut_emit``;
  * ``cull_mesh``: the three in batches of ``camera_batch`` cameras through one reused depth buffer; the host reads (V', T') once;
  * ``culled_mesh_metrics``: ``main()`` — with ``align`` the ICP alignment of ``icp`` first, then cull both meshes, then
    ``geometry.mesh_metrics``.

Poses are camera-to-world [C,4,4] in the OpenGL convention, as the reference hands them to pyrender and to ``cull_from_one_pose``;
``torch_mesh_cull.opencv_w2c`` turns them into the OpenCV ``[R | t]`` rows the kernels take.  Vertices are float32 (float64 is rounded
once, as in ``geometry``).  The reference's first step, ``trimesh.remesh.subdivide_to_size`` (:190-193), is ``subdivide`` and runs
with ``cull_mesh(..., subdivide=True)``; a marching-cubes mesh at a voxel edge at or under ``max_edge`` needs none, which is the
default.  Out of scope: ``voxel_down_sample``, PLY / JSON input and output, the CLIs, the 2-D contour cut of the MuSHRoom variant.  CPU tensors are refused; there is no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._ops import _mesh_cut_args, _mesh_depth_args, _mesh_visibility_args, _need_gpu, _stream
from .geometry import _device_points, _mesh, mesh_metrics
from .torch_mesh_cull import INVALID_SHARE, OBS_THRESHOLD, ZFAR, ZNEAR, intrinsics, opencv_w2c


def _w2c(poses, device) -> Tensor:
    w2c = opencv_w2c(poses).to(device)
    if w2c.shape[0] < 1:
        raise ValueError("at least one pose is needed")
    return w2c


def _frame(height: int, width: int) -> Tuple[int, int]:
    height, width = int(height), int(width)
    if height < 1 or width < 1 or height * width > 2 ** 31 - 1:
        raise ValueError(f"frames of {height} x {width} pixels are not supported")
    return height, width


def _maps(t, name: str, C: int, height: int, width: int, device) -> Tensor:
    """float32 [C,H,W] contiguous on the device from a tensor, an array or a list of [H,W] maps."""
    if not isinstance(t, Tensor):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float32))).to(device)
    _need_gpu(t, name)
    if tuple(t.shape) != (C, height, width):
        raise ValueError(f"{name} must be [{C},{height},{width}], got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


@torch.no_grad()
def render_mesh_depth(vertices, triangles, poses, K, height: int, width: int, znear: float = ZNEAR, zfar: float = ZFAR,
                      out: Optional[Tensor] = None, stats: Optional[Tensor] = None) -> Tensor:
    """``render_depth_maps_doublesided`` (:153-172): float32 [C,H,W], per pixel the smallest camera-space z in [znear, zfar] at which the
    ray through the pixel centre meets a triangle of either winding, 0 where nothing is hit.  One ``dnsplat_mesh_depth`` call.
    ``out`` (float32, at least C H W elements) is a buffer to render into; ``stats`` (int64 [3] on the device) receives the added
    counts {setups, fragments, atomics} of the measurement."""
    vertices, triangles = _mesh((vertices, triangles), "mesh")
    height, width = _frame(height, width)
    if not 0.0 < float(znear) <= float(zfar) < float("inf"):
        raise ValueError(f"0 < znear <= zfar < inf, got {znear} and {zfar}")
    dev = vertices.device
    w2c, k = _w2c(poses, dev), intrinsics(K)
    C = w2c.shape[0]
    if C > 65535:
        raise ValueError(f"{C} cameras in one call: render in batches of at most 65535")
    if out is None:
        depth = torch.empty(C, height, width, dtype=torch.float32, device=dev)
    else:
        _need_gpu(out, "out")
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < C * height * width or out.device != dev:
            raise ValueError(f"out must be a contiguous float32 buffer of at least {C * height * width} elements on {dev}")
        depth = out.view(-1)[:C * height * width].view(C, height, width)
    if stats is not None:
        _need_gpu(stats, "stats")
        if stats.dtype != torch.int64 or stats.numel() != 3 or not stats.is_contiguous():
            raise ValueError("stats must be a contiguous int64 [3] tensor")
    L = _lib.lib()
    scratch = torch.empty(L.dnsplat_mesh_depth_scratch_bytes(width, height) // 8, dtype=torch.float64, device=dev)
    a = _mesh_depth_args(vertices, triangles, w2c, k, width, height, float(znear), float(zfar), depth, scratch, stats)
    _lib.run("dnsplat_mesh_depth", L.dnsplat_mesh_depth, ctypes.byref(a), _stream())
    return depth


@torch.no_grad()
def vertex_visibility(vertices, poses, K, height: int, width: int, rendered_depth=None, depth_gt=None, remove_missing_depth: bool = True,
                      remove_occlusion: bool = True, obs: Optional[Tensor] = None, invalid: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """``get_grid_culling_pattern`` (:115-149): (obs, invalid) int32 [V] — per vertex the number of poses that see it (inside the frame,
    in front of the camera and, with ``remove_occlusion``, nearer than ``rendered_depth + 0.02``) and the number of poses whose
    ``depth_gt`` is missing (<= 0) where it projects.  Given ``obs`` / ``invalid``, the votes are ADDED to them in place.  One
    ``dnsplat_mesh_visibility`` call."""
    vertices = _device_points(vertices, "vertices")
    if vertices.shape[0] < 1:
        raise ValueError("vertices: an empty mesh has nothing to vote on")
    height, width = _frame(height, width)
    dev = vertices.device
    w2c, k = _w2c(poses, dev), intrinsics(K)
    C, V = w2c.shape[0], vertices.shape[0]
    if remove_occlusion and rendered_depth is None:
        raise ValueError("remove_occlusion needs rendered_depth")
    if remove_missing_depth and depth_gt is None:
        raise ValueError("remove_missing_depth needs depth_gt")
    rendered = _maps(rendered_depth, "rendered_depth", C, height, width, dev) if remove_occlusion else None
    gt = _maps(depth_gt, "depth_gt", C, height, width, dev) if remove_missing_depth else None
    if (obs is None) != (invalid is None):
        raise ValueError("obs and invalid are given together or not at all")
    if obs is None:
        obs, invalid = torch.zeros(V, dtype=torch.int32, device=dev), torch.zeros(V, dtype=torch.int32, device=dev)
    for name, t in (("obs", obs), ("invalid", invalid)):
        _need_gpu(t, name)
        if t.dtype != torch.int32 or tuple(t.shape) != (V,) or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous int32 [{V}] tensor on {dev}")
    L = _lib.lib()
    a = _mesh_visibility_args(vertices, w2c, k, width, height, rendered, gt, remove_occlusion, remove_missing_depth, obs, invalid)
    _lib.run("dnsplat_mesh_visibility", L.dnsplat_mesh_visibility, ctypes.byref(a), _stream())
    return obs, invalid


@torch.no_grad()
def cut_mesh(vertices, triangles, obs: Tensor, invalid: Tensor, obs_threshold: int = OBS_THRESHOLD,
             invalid_share: float = INVALID_SHARE) -> Tuple[Tensor, Tensor]:
    """:251-264: a triangle is kept when some vertex has ``obs > obs_threshold`` and not every vertex has ``invalid > invalid_share *
    obs``; kept triangles and the vertices they reference stay in their order, indices are remapped.  (vertices float32 [V',3],
    triangles int32 [T',3]); a cut that keeps nothing returns two empty tensors.  ``dnsplat_mesh_cut_count``, ONE host read of
    (V', T'), ``dnsplat_mesh_cut_emit``."""
    vertices, triangles = _mesh((vertices, triangles), "mesh")
    dev, V = vertices.device, vertices.shape[0]
    for name, t in (("obs", obs), ("invalid", invalid)):
        _need_gpu(t, name)
        if t.dtype != torch.int32 or tuple(t.shape) != (V,):
            raise ValueError(f"{name} must be an int32 [{V}] tensor")
    obs, invalid = obs.contiguous(), invalid.contiguous()
    L = _lib.lib()
    scratch = torch.empty((L.dnsplat_mesh_cut_scratch_bytes(V, triangles.shape[0]) + 3) // 4, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    a = _mesh_cut_args(vertices, triangles, obs, invalid, int(obs_threshold), float(invalid_share), scratch, counts)
    _lib.run("dnsplat_mesh_cut_count", L.dnsplat_mesh_cut_count, ctypes.byref(a), _stream())
    n_v, n_t = counts.tolist()                                                  # the one synchronisation
    out_v = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
    out_t = torch.empty(n_t, 3, dtype=torch.int32, device=dev)
    if n_t == 0:
        return out_v, out_t
    status = torch.empty(1, dtype=torch.int32, device=dev)
    a = _mesh_cut_args(vertices, triangles, obs, invalid, int(obs_threshold), float(invalid_share), scratch, counts, out_v, out_t, status)
    _lib.run("dnsplat_mesh_cut_emit", L.dnsplat_mesh_cut_emit, ctypes.byref(a), _stream())
    return out_v, out_t


@torch.no_grad()
def cull_mesh(mesh, poses, K, height: int, width: int, depth_gt=None, remove_missing_depth: bool = True, remove_occlusion: bool = True,
              obs_threshold: int = OBS_THRESHOLD, invalid_share: float = INVALID_SHARE, camera_batch: int = 8, subdivide: bool = False,
              max_edge: float = 0.015, max_iter: int = 10) -> Tuple[Tensor, Tensor]:
    """``cull_mesh`` (:176-266): ``mesh`` is a (vertices, triangles, ...) tuple — what ``marching_cubes_mesh``
    returns.  ``camera_batch`` poses at a time are rendered into one reused depth buffer and voted on before the next batch (a few
    hundred 1080p maps would be gigabytes); the votes are integers, so the result does not depend on the batch size.  ``depth_gt`` is
    [C,H,W] (a tensor on the device or an array), ``None`` implies ``remove_missing_depth=False``.  Returns (vertices float32 [V',3],
    triangles int32 [T',3]) on the device; the host reads (V', T') once.  With ``subdivide`` (the reference's ``subdivide=True``,
    :190-193) the depth maps are still rendered from the GIVEN mesh (:229-235), and the votes and the cut run on
    ``subdivide.subdivide_mesh(mesh, max_edge, max_iter)``, rounded to float32 once; that adds one host read per round."""
    vertices, triangles = _mesh(mesh, "mesh")
    height, width = _frame(height, width)
    render_vertices, render_triangles = vertices, triangles
    if subdivide:
        from .subdivide import subdivide_mesh

        vertices, triangles = _mesh(subdivide_mesh(mesh, max_edge, max_iter), "mesh")
    dev, V = vertices.device, vertices.shape[0]
    camera_batch = int(camera_batch)
    if camera_batch < 1:
        raise ValueError(f"camera_batch must be at least 1, got {camera_batch}")
    P = torch.as_tensor(np.asarray(poses) if not isinstance(poses, Tensor) else poses)
    P = P[None] if P.dim() == 2 else P
    C = P.shape[0]
    if C < 1:
        raise ValueError("at least one pose is needed")
    if depth_gt is None:
        remove_missing_depth = False
    elif remove_missing_depth and not isinstance(depth_gt, Tensor):
        depth_gt = np.asarray(depth_gt, dtype=np.float32)
    obs, invalid = torch.zeros(V, dtype=torch.int32, device=dev), torch.zeros(V, dtype=torch.int32, device=dev)
    buffer = torch.empty(min(camera_batch, C) * height * width, dtype=torch.float32, device=dev) if remove_occlusion else None
    for s in range(0, C, camera_batch):
        batch = P[s:s + camera_batch]
        rendered = render_mesh_depth(render_vertices, render_triangles, batch, K, height, width, out=buffer) if remove_occlusion else None
        gt = depth_gt[s:s + batch.shape[0]] if remove_missing_depth else None
        vertex_visibility(vertices, batch, K, height, width, rendered, gt, remove_missing_depth, remove_occlusion, obs, invalid)
    return cut_mesh(vertices, triangles, obs, invalid, obs_threshold, invalid_share)


@torch.no_grad()
def culled_mesh_metrics(pred, target, poses, K, height: int, width: int, depth_gt=None, threshold: float = 0.05, seed: int = 0,
                        samples_per_area: float = 1e4, count: Optional[Tuple[int, int]] = None, align: bool = False,
                        align_threshold: float = 0.1, **kw) -> Dict[str, Tensor]:
    """``main()`` of eval_mesh_vis_cull.py:427-464 behind its loading: with ``align`` (:427-431) the prediction is first moved by
    ``icp.get_align_transformation(pred, target, align_threshold)``; then both meshes go through ``cull_mesh`` with the same poses,
    intrinsics and sensor depth (``**kw``: its other arguments), then ``geometry.mesh_metrics`` on the two culled meshes.  Without
    ``align``, the default, nothing is moved."""
    if align:
        from .icp import get_align_transformation, transform_mesh

        pred = transform_mesh(pred, get_align_transformation(pred, target, align_threshold))
    pred = cull_mesh(pred, poses, K, height, width, depth_gt, **kw)
    target = cull_mesh(target, poses, K, height, width, depth_gt, **kw)
    return mesh_metrics(pred, target, threshold=threshold, seed=seed, samples_per_area=samples_per_area, count=count)
