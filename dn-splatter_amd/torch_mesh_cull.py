"""The reference's mesh visibility culling in plain PyTorch, restated from its behaviour: ``cull_mesh`` of
dn_splatter/eval/eval_mesh_vis_cull.py:176-266 — the double-sided depth renders of the mesh (``render_depth_maps_doublesided``,
:153-172, pyrender through OpenGL there), the per-vertex votes of ``cull_from_one_pose`` summed by ``get_grid_culling_pattern``
(:68-149) and the triangle rule with ``remove_unreferenced_vertices`` (:251-264).  Everything runs on whatever device the tensors are
on, in float64, with the operations in the order ``csrc/meshcull.hip`` performs them: the HIP path (``mesh_cull.py``) is held to
this file with exact equality, and this file to the reference's own outputs by tests/golden/reference_mesh_cull.npz.

THE DEPTH RENDER, independent of any rasteriser: ``depth[c, v, u]`` is the smallest camera-space z in [znear, zfar] at which the ray
through the pixel centre (u + 0.5, v + 0.5) meets a triangle, either winding, 0 where there is none.  With the OpenCV
world-to-camera ``[R | t]`` of ``opencv_w2c``, every sum below associated as written and no fused multiply-add:

    p_i = ((R_k0 x + R_k1 y) + R_k2 z) + t_k                      the three vertices in camera space, float64 from float32
    c0 = p1 x p2,  c1 = p2 x p0,  c2 = p0 x p1,  n = (c1 + c2) + c0,  D = (p0.x c0.x + p0.y c0.y) + p0.z c0.z
    d = (((u + 0.5) - cx) / fx, ((v + 0.5) - cy) / fy)
    E_i = (c_i.x d.x + c_i.y d.y) + c_i.z,   S = (n.x d.x + n.y d.y) + n.z
    inside: (every E_i >= 0 or every E_i <= 0) and S != 0;   z = D / S;   a hit: znear <= z <= zfar;   depth = min float32(z)

Swapping two indices of a triangle negates c0 and exchanges c1 with -c2: n and D change sign exactly (hence the association of n),
so both windings give the same bits; a shared edge has E of exactly opposite sign in its two triangles, so a pixel centre on it is
claimed by at least one of them.  A triangle with an index outside [0, V), a repeated index, a non-finite vertex or no area (the
area of ``dnsplat_mesh_areas``: |cross(v1 - v0, v2 - v0)| in double from the float32 vertices, not positive and finite) covers
nothing.  PARITY UNPINNED against pyrender (absent here): its 24-bit z-buffer quantises what this states exactly.

``render_mesh_depth`` is dense over (triangle, pixel): for small inputs.  Nothing here imports the oracle."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

ZNEAR, ZFAR = 0.01, 10.0        # render_depth_maps: pyrender's IntrinsicsCamera(znear=0.01, zfar=far), far = 10.0
DEPTH_EPS = 0.02                # cull_from_one_pose: eps of the occlusion test
PZ_EPS = 1e-8                   # cull_from_one_pose: pz = z + 1e-8
OBS_THRESHOLD = 3               # cull_mesh: th1
INVALID_SHARE = 0.7             # cull_mesh: inv > 0.7 * obs


def _f64(x, device=None) -> Tensor:
    if not isinstance(x, Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))
    x = x.detach().to(torch.float64)
    return x if device is None else x.to(device)


def opencv_w2c(poses) -> Tensor:
    """float64 [C,12], the rows of the OpenCV world-to-camera ``[R | t]``, from C camera-to-world poses [C,4,4] (or [C,3,4]) in the
    OpenGL convention: columns 1 and 2 negated (cull_from_one_pose :81-82), then the analytic inverse of a rigid transform,
    ``R = R_c2w^T`` and ``t_k = -((R_k0 t_0 + R_k1 t_1) + R_k2 t_2)``, where the reference calls ``np.linalg.inv``.  The one helper
    the restatement and the binding share; it stays on the device of ``poses`` (a numpy array: the CPU)."""
    P = _f64(poses)
    if P.dim() == 2:
        P = P[None]
    if P.dim() != 3 or P.shape[1] not in (3, 4) or P.shape[2] != 4:
        raise ValueError(f"poses must be [C,4,4] camera-to-world matrices, got {tuple(P.shape)}")
    Rc = P[:, :3, :3] * P.new_tensor([1.0, -1.0, -1.0])
    tc = P[:, :3, 3]
    R = Rc.transpose(1, 2)
    t = -((R[:, :, 0] * tc[:, None, 0] + R[:, :, 1] * tc[:, None, 1]) + R[:, :, 2] * tc[:, None, 2])
    return torch.cat([R, t[:, :, None]], dim=2).reshape(-1, 12).contiguous()


def intrinsics(K) -> Tuple[float, ...]:
    """The nine entries of K [3,3] as Python floats (float32 entries convert exactly), row-major."""
    k = _f64(K).reshape(-1).cpu().tolist()
    if len(k) != 9:
        raise ValueError("K must be a 3x3 intrinsics matrix")
    return tuple(k)


def _camera_space(w2c_row: Tensor, x: Tensor) -> Tensor:
    """[..., 3] float64 points -> camera space, ((R_k0 x + R_k1 y) + R_k2 z) + t_k."""
    M = w2c_row.reshape(3, 4)
    return torch.stack([((M[k, 0] * x[..., 0] + M[k, 1] * x[..., 1]) + M[k, 2] * x[..., 2]) + M[k, 3] for k in range(3)], dim=-1)


def _cross(a: Tensor, b: Tensor) -> Tensor:
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                        a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], dim=-1)


def covering_triangles(vertices: Tensor, triangles: Tensor) -> Tuple[Tensor, Tensor]:
    """(mask [T] of the triangles that can cover a pixel, their indices clamped into [0, V) so that they can be gathered)."""
    V = vertices.shape[0]
    tri = triangles.long()
    ok = ((tri >= 0) & (tri < V)).all(dim=1) & (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    tri = tri.clamp(0, max(V - 1, 0))
    x = vertices.to(torch.float64)[tri]                                           # [T,3,3]
    ok = ok & torch.isfinite(x).all(dim=2).all(dim=1)
    cr = _cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
    length = torch.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
    return ok & (length > 0) & (length < float("inf")), tri


def pixel_rays(K, height: int, width: int, device) -> Tuple[Tensor, Tensor]:
    """(d.x [W], d.y [H]) float64: ((u + 0.5) - cx) / fx and ((v + 0.5) - cy) / fy."""
    k = intrinsics(K)
    u = torch.arange(width, dtype=torch.float64, device=device)
    v = torch.arange(height, dtype=torch.float64, device=device)
    return ((u + 0.5) - k[2]) / k[0], ((v + 0.5) - k[5]) / k[4]


@torch.no_grad()
def triangle_coefficients(w2c_row: Tensor, x: Tensor):
    """(c0, c1, c2, n, D) of the docstring for triangles x [T,3,3] float64 under one camera."""
    p = _camera_space(w2c_row, x)
    p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
    c0, c1, c2 = _cross(p1, p2), _cross(p2, p0), _cross(p0, p1)
    n = (c1 + c2) + c0
    D = (p0[:, 0] * c0[:, 0] + p0[:, 1] * c0[:, 1]) + p0[:, 2] * c0[:, 2]
    return c0, c1, c2, n, D


@torch.no_grad()
def render_mesh_depth(vertices: Tensor, triangles: Tensor, poses, K, height: int, width: int, znear: float = ZNEAR,
                      zfar: float = ZFAR, chunk: int = 128) -> Tensor:
    """float32 [C,H,W]: the depth render of the module docstring, dense over (triangle, pixel) in chunks of ``chunk`` triangles."""
    if not 0.0 < float(znear) <= float(zfar):
        raise ValueError(f"0 < znear <= zfar, got {znear} and {zfar}")
    dev = vertices.device
    w2c = opencv_w2c(poses).to(dev)
    ok, tri = covering_triangles(vertices, triangles)
    x = vertices.to(torch.float64)[tri][ok]
    dx, dy = pixel_rays(K, height, width, dev)
    dx, dy = dx[None, None, :], dy[None, :, None]
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=dev)
    out = torch.empty(w2c.shape[0], height, width, dtype=torch.float32, device=dev)
    for c in range(w2c.shape[0]):
        best = inf.expand(height, width).clone()
        for s in range(0, x.shape[0], chunk):
            c0, c1, c2, n, D = triangle_coefficients(w2c[c], x[s:s + chunk])
            e = [(q[:, 0, None, None] * dx + q[:, 1, None, None] * dy) + q[:, 2, None, None] for q in (c0, c1, c2, n)]
            inside = (((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))) & (e[3] != 0)
            z = D[:, None, None] / e[3]
            hit = inside & (z >= znear) & (z <= zfar)
            z32 = torch.where(hit, z.to(torch.float32), inf)
            best = torch.minimum(best, z32.min(dim=0).values)
        out[c] = torch.where(best == inf, torch.zeros_like(best), best)
    return out


@torch.no_grad()
def vertex_visibility(vertices: Tensor, poses, K, height: int, width: int, rendered_depth: Optional[Tensor] = None,
                      depth_gt: Optional[Tensor] = None, remove_missing_depth: bool = True, remove_occlusion: bool = True,
                      obs: Optional[Tensor] = None, invalid: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """``get_grid_culling_pattern``: (obs, invalid) int32 [V], the number of poses that observe each vertex and the number whose
    sensor depth is missing there, ADDED to ``obs`` / ``invalid`` if given (camera batches chain).  Per pose, in float64:

        p = ((R_k0 x + R_k1 y) + R_k2 z) + t_k;   q_k = (K_k0 p.x + K_k1 p.y) + K_k2 p.z;   pz = q_2 + 1e-8, px = q_0 / pz, py = q_1 / pz
        in_frustum = 0 <= px <= W - 1 and 0 <= py <= H - 1 and pz > 0;   u, v = px, py truncated
        obs     = in_frustum and pz < float32(rendered[v, u] + 0.02)      (numpy adds the Python float to a float32 map in float32)
        invalid = in_frustum and depth_gt[v, u] <= 0

    ``rendered_depth`` / ``depth_gt`` are float32 [C,H,W]; either may be None when its flag is off."""
    if remove_occlusion and rendered_depth is None:
        raise ValueError("remove_occlusion needs rendered_depth")
    if remove_missing_depth and depth_gt is None:
        raise ValueError("remove_missing_depth needs depth_gt")
    dev = vertices.device
    w2c = opencv_w2c(poses).to(dev)
    k = intrinsics(K)
    x = vertices.to(torch.float64)
    V = x.shape[0]
    obs = torch.zeros(V, dtype=torch.int32, device=dev) if obs is None else obs
    invalid = torch.zeros(V, dtype=torch.int32, device=dev) if invalid is None else invalid
    for c in range(w2c.shape[0]):
        p = _camera_space(w2c[c], x)
        q = [(k[3 * r] * p[:, 0] + k[3 * r + 1] * p[:, 1]) + k[3 * r + 2] * p[:, 2] for r in range(3)]
        pz = q[2] + PZ_EPS
        px, py = q[0] / pz, q[1] / pz
        inside = (px >= 0) & (px <= width - 1) & (py >= 0) & (py <= height - 1) & (pz > 0)
        u = torch.where(inside, px, torch.zeros_like(px)).to(torch.int64)
        v = torch.where(inside, py, torch.zeros_like(py)).to(torch.int64)
        seen = inside
        if remove_occlusion:
            limit = rendered_depth[c].to(torch.float32)[v, u] + torch.tensor(DEPTH_EPS, dtype=torch.float32, device=dev)
            seen = inside & (pz < limit.to(torch.float64))
        obs += seen.to(torch.int32)
        if remove_missing_depth:
            invalid += (inside & (depth_gt[c].to(torch.float32)[v, u] <= 0)).to(torch.int32)
    return obs, invalid


@torch.no_grad()
def keep_triangles(triangles: Tensor, obs: Tensor, invalid: Tensor, obs_threshold: int = OBS_THRESHOLD,
                   invalid_share: float = INVALID_SHARE) -> Tensor:
    """The mask of :251-260: kept = (some vertex has obs > threshold) and not (every vertex has invalid > share * obs), the product
    and the comparison in double.  A triangle with an index outside [0, V) is not kept."""
    V = obs.shape[0]
    tri = triangles.long()
    ok = ((tri >= 0) & (tri < V)).all(dim=1)
    tri = tri.clamp(0, max(V - 1, 0))
    o, i = obs[tri], invalid[tri]                                                # [T,3]
    observed = (o > int(obs_threshold)).any(dim=1)
    bad = (i.to(torch.float64) > float(invalid_share) * o.to(torch.float64)).all(dim=1)
    return ok & observed & ~bad


@torch.no_grad()
def cut_mesh(vertices: Tensor, triangles: Tensor, obs: Tensor, invalid: Tensor, obs_threshold: int = OBS_THRESHOLD,
             invalid_share: float = INVALID_SHARE) -> Tuple[Tensor, Tensor]:
    """:251-264: the kept triangles in their order, the vertices they reference in their order, indices remapped — what
    ``trimesh.Trimesh(vertices, triangles[valid], process=False).remove_unreferenced_vertices()`` leaves (trimesh is absent: the order
    is stated, not pinned).  (vertices [V',3] in their dtype, triangles int32 [T',3]); both may be empty."""
    keep = keep_triangles(triangles, obs, invalid, obs_threshold, invalid_share)
    kept = triangles.long()[keep]
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=vertices.device)
    used[kept.reshape(-1)] = True
    new_id = torch.cumsum(used.to(torch.int64), dim=0) - 1
    return vertices[used], new_id[kept].to(torch.int32).reshape(-1, 3)


@torch.no_grad()
def cull_mesh(mesh, poses, K, height: int, width: int, depth_gt: Optional[Tensor] = None, remove_missing_depth: bool = True,
              remove_occlusion: bool = True, obs_threshold: int = OBS_THRESHOLD, invalid_share: float = INVALID_SHARE,
              camera_batch: int = 8, subdivide: bool = False, max_edge: float = 0.015, max_iter: int = 10) -> Tuple[Tensor, Tensor]:
    """``cull_mesh``: render, vote over the poses in batches of ``camera_batch``, cut.  ``mesh`` is a
    (vertices float32 [V,3], triangles int [T,3]) pair; ``depth_gt=None`` implies ``remove_missing_depth=False``.  With ``subdivide``
    the render is of the given mesh, and the votes and the cut are on ``torch_subdivide.subdivide_mesh(mesh, max_edge, max_iter)``,
    rounded to float32 once."""
    vertices, triangles = mesh[0].to(torch.float32), mesh[1]
    render_vertices, render_triangles = vertices, triangles
    if subdivide:
        from .torch_subdivide import subdivide_mesh

        fine_v, fine_t = subdivide_mesh((mesh[0], mesh[1]), max_edge, max_iter)
        vertices, triangles = fine_v.to(torch.float32).to(mesh[0].device), fine_t.to(mesh[1].device)
    if depth_gt is None:
        remove_missing_depth = False
    w2c_count = opencv_w2c(poses).shape[0]
    P = _f64(poses).reshape(w2c_count, -1, 4)
    obs = invalid = None
    for s in range(0, w2c_count, max(int(camera_batch), 1)):
        batch = P[s:s + max(int(camera_batch), 1)]
        rendered = render_mesh_depth(render_vertices, render_triangles, batch, K, height, width) if remove_occlusion else None
        gt = depth_gt[s:s + batch.shape[0]] if remove_missing_depth else None
        obs, invalid = vertex_visibility(vertices, batch, K, height, width, rendered, gt, remove_missing_depth, remove_occlusion,
                                         obs, invalid)
    return cut_mesh(vertices, triangles, obs, invalid, obs_threshold, invalid_share)
