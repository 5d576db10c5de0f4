"""The CPU restatement of ``normals`` (``csrc/normals.hip``): Open3D's ``estimate_normals`` as ``include/dnsplat.h`` states it — THIS
PROJECT'S DEFINITION, PARITY UNPINNED AGAINST Open3D — written with array operations and no kernel.  It is what the kernel is held to
(``tests/test_gpu_normals.py``: neighbours, counts, covariance AND normals bit for bit, since every step below is the kernel's own IEEE
operation in the kernel's own order) and is itself held to scipy's ``cKDTree``, numpy's ``cov`` and ``eigh`` and a 50-digit solve
(``tests/test_normals_reference.py``).

  * neighbours: a dense matrix of d² = fma(dz, dz, fma(dy, dy, dx dx)) in double (``torch_geometry.squared_distance`` emulates the fused
    operations exactly) and a stable sort, so equal d² go to the lowest index; with a radius the strict ``d² < radius * radius``;
  * moments: the fixed tree of the header — slot t of the ascending ranks belongs to lane t mod 64, a lane adds its slots in order, the
    64 partials are added by the xor tree 32, 16, .. 1 — first the mean, then the six sums about it.  Two passes, not Open3D's cumulants;
  * normal: 8 cyclic Jacobi sweeps (``normals_solve.h``), the column of the smallest eigenvalue, one division by its length;
  * sign: canonical, or towards ``orient_toward``.

The square roots are numpy's (the hardware's correctly rounded ones; torch's CPU float64 ``sqrt`` is not), so the solve runs in numpy on
the host whatever device the tensors are on.  Also here: the reference's ``backproject`` (scripts/depth_to_normal.py:41-65) and the
10-degree consistency mask (:192-213) in plain array code."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .torch_geometry import squared_distance

MAX_K = 256                   # include/dnsplat.h DNSPLAT_NORMALS_MAX_K
MIN_K = 3
WAVE = 64
LANE_TERMS = MAX_K // WAVE
SWEEPS = 8                    # csrc/normals_solve.h NM_SWEEPS
MIN_KP = 64                   # csrc/normals.hip NM_MIN_KP: the buffer holds 2 KP entries, KP = max(64, knn rounded up to a power of two)


def buffer_capacity(knn: int) -> int:
    """The entries of the kernel's per-wave candidate buffer for this ``knn``."""
    kp = MIN_KP
    while kp < knn:
        kp *= 2
    return 2 * kp


def check_arguments(knn, radius) -> Tuple[int, Optional[float]]:
    knn = int(knn)
    if not MIN_K <= knn <= MAX_K:
        raise ValueError(f"knn must lie in [{MIN_K}, {MAX_K}], got {knn}")
    if radius is not None:
        radius = float(radius)
        if radius != radius:
            raise ValueError("radius is nan")
        if radius <= 0.0 or radius == float("inf"):
            radius = None
    return knn, radius


def _points64(points) -> Tensor:
    points = torch.as_tensor(points)
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"points must be [n,3] with n >= 1, got {tuple(points.shape)}")
    if not points.dtype.is_floating_point:
        raise TypeError(f"points must be floating point, got {points.dtype}")
    p64 = points.detach().double()
    if not torch.equal(p64.float().double()[torch.isfinite(p64)], p64[torch.isfinite(p64)]):
        raise ValueError("points must hold float32 values: the kernel's cloud is float32")
    return p64


def neighbors(points, knn: int = 30, radius: Optional[float] = None, chunk: int = 256) -> Tuple[Tensor, Tensor]:
    """(neighbors int32 [N,knn], count int32 [N]): the kept neighbours of every point ascending by (d², index), -1 past ``count``."""
    knn, radius = check_arguments(knn, radius)
    p64 = _points64(points)
    N = p64.shape[0]
    K = min(knn, N)
    finite = torch.isfinite(p64).all(dim=1)
    r2 = float("inf") if radius is None else radius * radius
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=p64.device)
    out = torch.full((N, knn), -1, dtype=torch.int32, device=p64.device)
    count = torch.zeros(N, dtype=torch.int32, device=p64.device)
    for i in range(0, N, chunk):
        d2 = squared_distance(p64[i:i + chunk, None, :], p64[None, :, :])
        d2 = torch.where(finite[None, :] & finite[i:i + chunk, None] & torch.isfinite(d2), d2, inf)
        ranked = torch.sort(d2, dim=1, stable=True)                               # columns ascend: equal d² go to the lowest index
        vals, cols = ranked.values[:, :K], ranked.indices[:, :K]
        kept = vals < r2                                                          # strict; inf (nobody) is never kept
        out[i:i + chunk, :K] = torch.where(kept, cols, torch.full_like(cols, -1)).to(torch.int32)
        count[i:i + chunk] = kept.sum(dim=1).to(torch.int32)
    return out, count


def _tree(lanes: np.ndarray) -> np.ndarray:
    """[..., 64] partials -> [...]: v[l] = v[l] + v[l xor o] for o = 32, 16, .. 1; every lane ends with the same bits."""
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., lane ^ o]
    return lanes[..., 0]


def moments(points, nbr, count) -> np.ndarray:
    """Covariance float64 [N,6] (xx, xy, xz, yy, yz, zz) of the kept neighbours by the fixed tree of the header."""
    p = np.asarray(torch.as_tensor(points).detach().double().cpu().numpy())
    nbr = np.asarray(torch.as_tensor(nbr).cpu().numpy()).astype(np.int64)
    n = np.asarray(torch.as_tensor(count).cpu().numpy()).astype(np.int64)
    N, knn = nbr.shape
    slots = np.full((N, MAX_K), -1, dtype=np.int64)
    slots[:, :knn] = nbr
    slots = slots.reshape(N, LANE_TERMS, WAVE)                                    # slot t = 64 j + lane
    used = slots >= 0
    P = np.where(used[..., None], p[np.where(used, slots, 0)], 0.0)               # [N, 4, 64, 3]
    dn = np.maximum(n, 1).astype(np.float64)
    S = np.zeros((N, WAVE, 3))
    for j in range(LANE_TERMS):
        S = np.where(used[:, j, :, None], S + P[:, j], S)
    mean = np.stack([_tree(S[..., a]) for a in range(3)], axis=1) / dn[:, None]
    C = np.zeros((N, WAVE, 6))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for j in range(LANE_TERMS):
        d = P[:, j] - mean[:, None, :]
        terms = np.stack([d[..., a] * d[..., b] for a, b in pairs], axis=-1)
        C = np.where(used[:, j, :, None], C + terms, C)
    cov = np.stack([_tree(C[..., k]) for k in range(6)], axis=1) / dn[:, None]
    cov[n == 0] = 0.0
    return cov


def _rotate(A: np.ndarray, V: np.ndarray, P: int, Q: int) -> None:
    """nm_rotate<P, Q> on every row of A, V [N,3,3], in place."""
    R = 3 - P - Q
    apq, app, aqq = A[:, P, Q].copy(), A[:, P, P].copy(), A[:, Q, Q].copy()
    g = np.abs(apq)
    nonzero = apq != 0.0
    small = nonzero & (np.abs(app) + g == np.abs(app)) & (np.abs(aqq) + g == np.abs(aqq))
    rot = nonzero & ~small
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * np.where(rot, apq, 1.0))
        mag = np.abs(theta) + np.sqrt(theta * theta + 1.0)
        tt = np.where(theta < 0.0, -1.0, 1.0) / mag
        c = 1.0 / np.sqrt(tt * tt + 1.0)
        s = tt * c
        A[:, P, P] = np.where(rot, app - tt * apq, app)
        A[:, Q, Q] = np.where(rot, aqq + tt * apq, aqq)
        zeroed = np.where(nonzero, 0.0, apq)
        A[:, P, Q] = zeroed
        A[:, Q, P] = np.where(nonzero, 0.0, A[:, Q, P])
        arp, arq = A[:, R, P].copy(), A[:, R, Q].copy()
        new_rp, new_rq = c * arp - s * arq, s * arp + c * arq
        A[:, R, P] = np.where(rot, new_rp, arp)
        A[:, P, R] = np.where(rot, new_rp, A[:, P, R])
        A[:, R, Q] = np.where(rot, new_rq, arq)
        A[:, Q, R] = np.where(rot, new_rq, A[:, Q, R])
        for r in range(3):
            vrp, vrq = V[:, r, P].copy(), V[:, r, Q].copy()
            V[:, r, P] = np.where(rot, c * vrp - s * vrq, vrp)
            V[:, r, Q] = np.where(rot, s * vrp + c * vrq, vrq)


def jacobi(cov: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(diagonal [N,3], V [N,3,3]) after the fixed sweeps over (0,1), (0,2), (1,2) of the symmetric matrices of ``cov`` [N,6]."""
    C = np.asarray(cov, dtype=np.float64)
    A = np.stack([C[:, [0, 1, 2]], C[:, [1, 3, 4]], C[:, [2, 4, 5]]], axis=1).copy()
    V = np.broadcast_to(np.eye(3), A.shape).copy()
    for _ in range(SWEEPS):
        _rotate(A, V, 0, 1)
        _rotate(A, V, 0, 2)
        _rotate(A, V, 1, 2)
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1), V


def normal_of(cov: np.ndarray, count: np.ndarray) -> np.ndarray:
    """nm_normal: float64 [N,3], before the sign is chosen."""
    cov = np.asarray(cov, dtype=np.float64)
    n = np.asarray(count).astype(np.int64)
    lam, V = jacobi(cov)
    one = lam[:, 1] < lam[:, 0]
    l01 = np.where(one, lam[:, 1], lam[:, 0])
    two = lam[:, 2] < l01
    e = np.where(two[:, None], V[:, :, 2], np.where(one[:, None], V[:, :, 1], V[:, :, 0]))
    with np.errstate(all="ignore"):
        length = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        out = e / length[:, None]
    fallback = (n < 3) | (cov == 0.0).all(axis=1)
    out[fallback] = (0.0, 0.0, 1.0)
    return out


def orient(normals: np.ndarray, points: np.ndarray, orient_toward=None) -> np.ndarray:
    """nm_orient: towards ``orient_toward`` (negated iff the dot product with ``toward - p`` is negative), or the canonical sign."""
    nrm = np.array(normals, dtype=np.float64)
    if orient_toward is not None:
        c = np.asarray(orient_toward, dtype=np.float64).reshape(3)
        p = np.asarray(points, dtype=np.float64)
        with np.errstate(all="ignore"):
            dot = (nrm[:, 0] * (c[0] - p[:, 0]) + nrm[:, 1] * (c[1] - p[:, 1])) + nrm[:, 2] * (c[2] - p[:, 2])
        flip = dot < 0.0
    else:
        ax, ay, az = np.abs(nrm[:, 0]), np.abs(nrm[:, 1]), np.abs(nrm[:, 2])
        one = ay > ax
        m01 = np.where(one, ay, ax)
        two = az > m01
        lead = np.where(two, nrm[:, 2], np.where(one, nrm[:, 1], nrm[:, 0]))
        flip = lead < 0.0
    nrm[flip] = -nrm[flip]
    return nrm


def estimate_normals(points, knn: int = 30, radius: Optional[float] = None, orient_toward=None):
    """``(normals float64 [N,3], covariance float64 [N,6], neighbors int32 [N,knn], count int32 [N])`` on the device of ``points``."""
    p64 = _points64(points)
    nbr, count = neighbors(p64, knn, radius)
    cov = moments(p64, nbr, count)
    pn = p64.cpu().numpy()
    nrm = orient(normal_of(cov, count.cpu().numpy()), pn, orient_toward)
    dev = p64.device
    return torch.from_numpy(nrm).to(dev), torch.from_numpy(cov).to(dev), nbr, count


# ---- the reference's own steps around the call --------------------------------------------------------------------------------------------

def camera_points(depth: Tensor, fx: float, fy: float, cx: float, cy: float) -> Tensor:
    """scripts/depth_to_normal.py:56-61 in float32: ``((u + 0.5 - cx) * d / fx, (v + 0.5 - cy) * d / fy, d)`` per pixel, [H*W,3]."""
    depth = torch.as_tensor(depth)
    H, W = depth.shape
    d = depth.to(torch.float32).reshape(-1)
    f32 = dict(dtype=torch.float32, device=d.device)
    u = (torch.arange(W, **f32) + 0.5).repeat(H)
    v = (torch.arange(H, **f32) + 0.5).repeat_interleave(W)
    x = (u - torch.tensor(cx, **f32)) * d / torch.tensor(fx, **f32)
    y = (v - torch.tensor(cy, **f32)) * d / torch.tensor(fy, **f32)
    return torch.stack([x, y, d], dim=1)


def world_points(cam: Tensor, c2w) -> Tensor:
    """:64, ``cam @ inv(c2w[:3,:3]) + c2w[:3,3]`` in float64 [n,3], the three products of a row added in ascending order, then the
    translation (numpy's matrix product may add them in another order: an ulp of a double)."""
    c2w = np.asarray(torch.as_tensor(c2w).detach().cpu().numpy(), dtype=np.float64)
    Ri = torch.from_numpy(np.linalg.inv(c2w[:3, :3])).to(cam.device)
    t = torch.from_numpy(c2w[:3, 3].copy()).to(cam.device)
    c = cam.double()
    cols = [((c[:, 0] * Ri[0, a] + c[:, 1] * Ri[1, a]) + c[:, 2] * Ri[2, a]) + t[a] for a in range(3)]
    return torch.stack(cols, dim=1)


def backproject(depth, fx: float, fy: float, cx: float, cy: float, c2w) -> Tensor:
    """The reference's ``backproject``: float64 [H*W,3] world points of every pixel."""
    return world_points(camera_points(depth, fx, fy, cx, cy), c2w)


def valid_depth(depth: Tensor) -> Tensor:
    depth = torch.as_tensor(depth)
    return torch.isfinite(depth) & (depth > 0)


def depth_normals(depth, fx: float, fy: float, cx: float, cy: float, c2w, knn: int = 200, estimate=None):
    """``normals.depth_normals`` with ``estimate`` = this file's ``estimate_normals`` (the device module passes its own)."""
    depth = torch.as_tensor(depth)
    H, W = depth.shape
    valid = valid_depth(depth).reshape(-1)
    world = backproject(depth, fx, fy, cx, cy, c2w).float()                        # the kernel's cloud is float32
    c2w64 = np.asarray(torch.as_tensor(c2w).detach().cpu().numpy(), dtype=np.float64)
    centre = tuple(float(v) for v in c2w64[:3, 3])
    out = torch.zeros(H * W, 3, dtype=torch.float64, device=depth.device)
    kept = world[valid]                                                           # the one host read: how many pixels are valid
    if kept.shape[0] > 0:
        out[valid] = (estimate or estimate_normals)(kept, knn=knn, orient_toward=centre)[0]
    return out.reshape(H, W, 3), valid.reshape(H, W)


def consistency_angles(depth_normals_map: Tensor, mono_normal: Tensor, c2w) -> Tensor:
    """:183-208: the angle in degrees, float64 [H,W], between the ``(n + 1) / 2``-encoded depth normals and the encoded mono normals
    after their rotation by ``inv(c2w)[:3,:3].T`` and normalisation — the reference takes the angle between the ENCODED vectors."""
    n = torch.as_tensor(depth_normals_map).double()
    mono = torch.as_tensor(mono_normal).double().to(n.device)
    c2w = np.asarray(torch.as_tensor(c2w).detach().cpu().numpy(), dtype=np.float64)
    if c2w.shape[0] == 3:
        c2w = np.concatenate([c2w, np.array([[0.0, 0.0, 0.0, 1.0]])], axis=0)
    R = torch.from_numpy(np.linalg.inv(c2w)[:3, :3].T.copy()).to(n.device)
    H, W, _ = mono.shape
    m = ((mono.reshape(-1, 3) - 0.5) * 2) @ R.T
    m = m / torch.linalg.norm(m, dim=1, keepdim=True)
    a = (n + 1) / 2
    b = m.reshape(H, W, 3) * 0.5 + 0.5
    a = a / torch.linalg.norm(a, dim=2, keepdim=True)
    b = b / torch.linalg.norm(b, dim=2, keepdim=True)
    dot = torch.clamp((a * b).sum(dim=2), -1.0, 1.0)
    return torch.rad2deg(torch.acos(dot))


def normal_consistency_mask(depth_normals_map: Tensor, mono_normal: Tensor, c2w, degrees: float = 10.0) -> Tensor:
    """The mask of scripts/depth_to_normal.py:192-213, bool [H,W]: True where the angle exceeds ``degrees`` (the pixels the
    depth-normal consistency filter drops).  ``mono_normal`` is the monocular map in [0, 1], ``c2w`` the OpenCV camera-to-world."""
    return consistency_angles(depth_normals_map, mono_normal, c2w) > degrees


def points3D_normals(points, transform_matrix=None, knn: int = 30, radius: Optional[float] = 0.1, estimate=None) -> Tensor:
    """``normals.points3D_normals`` with ``estimate`` = this file's ``estimate_normals``."""
    points = torch.as_tensor(points)
    nrm = (estimate or estimate_normals)(points, knn=knn, radius=radius)[0]
    nrm = nrm / torch.linalg.norm(nrm, dim=1, keepdim=True)                       # normalize_normals(): already unit, as in the reference
    nrm = nrm.float()
    if transform_matrix is None:
        return nrm
    T = torch.as_tensor(transform_matrix).to(device=nrm.device, dtype=torch.float32)
    if tuple(T.shape) != (3, 4):
        raise ValueError(f"transform_matrix must be [3,4], got {tuple(T.shape)}")
    return torch.cat([nrm, torch.ones_like(nrm[:, :1])], dim=1) @ T.T
