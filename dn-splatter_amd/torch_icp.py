"""The mesh alignment of the reference in float64, restated from its behaviour: ``get_align_transformation``
(dn_splatter/eval/eval_mesh_vis_cull.py:269-287, called at :427-431), Open3D's ``registration_icp`` with
``TransformationEstimationPointToPoint``.  Open3D is not on a ROCm box: the rule is restated from memory of ``RegistrationICP`` /
``GetRegistrationResultAndCorrespondences`` / ``Eigen::umeyama(..., with_scaling=False)``, IT IS THIS PROJECT'S DEFINITION, PARITY
UNPINNED AGAINST Open3D, stated in ``include/dnsplat.h`` and implemented by ``csrc/icp.hip`` (``icp.py`` is that path).

Pass k on the accumulated ``T_k``:

  1. ``q = fl32(T_k s)``: every coordinate ``((T[a][0] x + T[a][1] y) + T[a][2] z) + T[a][3]`` in float64, rounded to float32 once.
     Every pass transforms the ORIGINAL source (Open3D transforms the transformed cloud again, so its roundings pile up);
  2. row m is a correspondence iff ``torch_geometry.nearest`` finds a target — lowest (d², index), d² as ``squared_distance`` — and
     ``d² <= r * r``; a non-finite source row never is one and still counts in M;
  3. ``fitness = n / M``, ``rmse = sqrt(sum d² / n)`` (0 without a correspondence);
  4. stop on ``n == 0`` (status ``NO_CORRESPONDENCE``), on ``k == max_iteration``, or on ``k >= 1`` with both changes below the relative
     tolerances;
  5. otherwise ``T_{k+1} = U_k T_k``, ``U_k`` the Umeyama / Kabsch solve without scale.

The moments are taken about ``c``, the centre of the target's float32 bounding box, as the kernel takes them.  ``solve`` is the kernel's
solve operation by operation — Horn's 4 x 4 quaternion matrix, a cyclic Jacobi of exactly ``SWEEPS`` sweeps — in Python floats, which
are IEEE doubles without contraction; ``solve_svd`` is the same update from ``numpy.linalg.svd``."""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
from torch import Tensor

from .torch_geometry import nearest

THRESHOLD = 0.1                     # get_align_transformation's
RELATIVE_FITNESS = 1e-6             # Open3D's ICPConvergenceCriteria
RELATIVE_RMSE = 1e-6
MAX_ITERATION = 30
SWEEPS = 10                         # csrc/icp.hip ICP_SWEEPS
PLANES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
STATUS_NO_CORRESPONDENCE, STATUS_DEGENERATE = 1, 2          # include/dnsplat.h DNSPLAT_ICP_STATUS_*
DEGENERATE_RATIO = 2.0 ** -26


def _matrix(T) -> Tensor:
    T = torch.as_tensor(np.asarray(T.detach().cpu()) if isinstance(T, Tensor) else np.asarray(T), dtype=torch.float64)
    if tuple(T.shape) != (4, 4):
        raise ValueError(f"a transform is [4,4], got {tuple(T.shape)}")
    return T


def transform_points(points: Tensor, T, rotate_only: bool = False) -> Tensor:
    """float32 [n,3]: ``fl32(T p)`` under THE rule of include/dnsplat.h; the rotation block alone with ``rotate_only``."""
    T = _matrix(T).to(points.device)
    p = points.double()
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    r = (T[None, :3, 0] * x + T[None, :3, 1] * y) + T[None, :3, 2] * z
    return (r if rotate_only else r + T[None, :3, 3]).float()


def centre(tgt: Tensor) -> Tensor:
    """float64 [3]: ``(lo + hi) * 0.5`` of the target's float32 bounding box (nan rows aside, as the index's header takes it)."""
    t = tgt.float()
    lo = torch.where(torch.isnan(t), torch.full_like(t, float("inf")), t).min(dim=0).values
    hi = torch.where(torch.isnan(t), torch.full_like(t, float("-inf")), t).max(dim=0).values
    return (lo.double() + hi.double()) * 0.5


def correspondences(src: Tensor, tgt: Tensor, T, r: float):
    """(q float32 [M,3], idx int64 [M] with -1 for none, d² float64 [M] with nan for none) of one pass."""
    q = transform_points(src, T)
    ok = torch.isfinite(src).all(dim=-1) & torch.isfinite(q).all(dim=-1)
    idx, d2 = nearest(tgt, q)
    corr = ok & (idx >= 0) & (d2 <= float(r) * float(r))
    return q, torch.where(corr, idx, torch.full_like(idx, -1)), torch.where(corr, d2, torch.full_like(d2, float("nan")))


def moments(q: Tensor, tgt: Tensor, idx: Tensor, d2: Tensor, c: Tensor) -> Dict[str, object]:
    """The sums of one pass over the correspondences, about ``c``: ``n``, ``d2``, ``q`` [3], ``g`` [3], ``gq`` [3,3] (g along the rows),
    and under ``abs`` the sums of the terms' magnitudes, which the fold bounds of the tests are made of."""
    corr = idx >= 0
    qc = q.double()[corr] - c
    gc = tgt.double()[idx[corr]] - c
    dd = d2[corr]
    outer = gc[:, :, None] * qc[:, None, :]
    return {"n": int(corr.sum()), "d2": dd.sum(), "q": qc.sum(dim=0), "g": gc.sum(dim=0), "gq": outer.sum(dim=0),
            "abs": {"d2": dd.abs().sum(), "q": qc.abs().sum(dim=0), "g": gc.abs().sum(dim=0), "gq": outer.abs().sum(dim=0)}, "c": c}


def sigma_of(sums) -> np.ndarray:
    """Sigma [3,3] float64 as the kernel forms it: ``S_gq / n - (S_g / n)(S_q / n)``."""
    n = float(sums["n"])
    mq = [float(v) / n for v in sums["q"]]
    mg = [float(v) / n for v in sums["g"]]
    return np.array([[float(sums["gq"][a][b]) / n - mg[a] * mq[b] for b in range(3)] for a in range(3)])


def _rotate(A, V, p, q):
    apq = A[p][q]
    if apq == 0.0:
        return
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    mag = abs(theta) + math.sqrt(theta * theta + 1.0)                 # a huge theta: theta² = inf in IEEE, t = 0
    t = (-1.0 if theta < 0.0 else 1.0) / mag
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    A[p][p] = A[p][p] - t * apq
    A[q][q] = A[q][q] + t * apq
    A[p][q] = A[q][p] = 0.0
    for r in range(4):
        if r != p and r != q:
            arp, arq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * arp - s * arq
            A[r][q] = A[q][r] = s * arp + c * arq
    for r in range(4):
        vrp, vrq = V[r][p], V[r][q]
        V[r][p] = c * vrp - s * vrq
        V[r][q] = s * vrp + c * vrq


def solve(sums):
    """(U float64 [4,4] numpy, degenerate bool): the rigid update of one pass's sums, the kernel's solve operation by operation."""
    n = float(sums["n"])
    c = [float(v) for v in sums["c"]]
    mq = [float(v) / n for v in sums["q"]]
    mg = [float(v) / n for v in sums["g"]]
    S = [[float(sums["gq"][a][b]) / n - mg[a] * mq[b] for b in range(3)] for a in range(3)]
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = S[0][0], S[1][0], S[2][0], S[0][1], S[1][1], S[2][1], S[0][2], S[1][2], S[2][2]
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0] = (Sxx + Syy) + Szz
    A[1][1] = (Sxx - Syy) - Szz
    A[2][2] = (Syy - Sxx) - Szz
    A[3][3] = (Szz - Sxx) - Syy
    A[0][1] = A[1][0] = Syz - Szy
    A[0][2] = A[2][0] = Szx - Sxz
    A[0][3] = A[3][0] = Sxy - Syx
    A[1][2] = A[2][1] = Sxy + Syx
    A[1][3] = A[3][1] = Szx + Sxz
    A[2][3] = A[3][2] = Syz + Szy
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(SWEEPS):
        for p, q in PLANES:
            _rotate(A, V, p, q)
    i1 = 0
    for k in range(1, 4):
        if A[k][k] > A[i1][i1]:
            i1 = k
    i2 = 1 if i1 == 0 else 0
    for k in range(4):
        if k != i1 and k != i2 and A[k][k] > A[i2][i2]:
            i2 = k
    l1, l2 = A[i1][i1], A[i2][i2]
    e = [V[r][i1] for r in range(4)]
    length = math.sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3])
    w, x, y, z = e[0] / length, e[1] / length, e[2] / length, e[3] / length
    R = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
         [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
         [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]
    fq = [mq[k] + c[k] for k in range(3)]
    fg = [mg[k] + c[k] for k in range(3)]
    U = np.eye(4)
    for a in range(3):
        U[a, :3] = R[a]
        U[a, 3] = fg[a] - ((R[a][0] * fq[0] + R[a][1] * fq[1]) + R[a][2] * fq[2])
    return U, (l1 - l2) * 0.5 <= DEGENERATE_RATIO * ((l1 + l2) * 0.5)


def solve_svd(sums):
    """(U float64 [4,4] numpy, degenerate bool): the same update by ``numpy.linalg.svd`` — Umeyama's ``U diag(1, 1, s) Vᵀ``."""
    n = float(sums["n"])
    c = np.array([float(v) for v in sums["c"]])
    mq = np.array([float(v) for v in sums["q"]]) / n
    mg = np.array([float(v) for v in sums["g"]]) / n
    S = sigma_of(sums)
    u, d, vt = np.linalg.svd(S)
    s = -1.0 if np.linalg.det(u) * np.linalg.det(vt) < 0 else 1.0
    R = u @ np.diag([1.0, 1.0, s]) @ vt
    U = np.eye(4)
    U[:3, :3] = R
    U[:3, 3] = (mg + c) - R @ (mq + c)
    return U, bool(d[1] + s * d[2] <= DEGENERATE_RATIO * d[0])


def compose(U, T) -> np.ndarray:
    """``U T`` as the kernel forms it: rows ``((R[a][0] T[0][b] + R[a][1] T[1][b]) + R[a][2] T[2][b]) (+ t[a])``; the last row stays."""
    U, T = np.asarray(U, dtype=np.float64), np.asarray(T, dtype=np.float64)
    out = np.array(T, dtype=np.float64)
    for a in range(3):
        for b in range(4):
            r = (U[a, 0] * T[0, b] + U[a, 1] * T[1, b]) + U[a, 2] * T[2, b]
            out[a, b] = r + U[a, 3] if b == 3 else r
    return out


def step(src: Tensor, tgt: Tensor, T, r: float) -> Dict[str, object]:
    """One pass on ``T``: ``q``, ``idx``, ``dist2``, ``n``, ``sums`` (of ``moments``), ``fitness``, ``rmse``, and — with a correspondence —
    ``U`` and ``degenerate`` of ``solve``."""
    q, idx, d2 = correspondences(src, tgt, T, r)
    sums = moments(q, tgt, idx, d2, centre(tgt).to(q.device))
    n, M = sums["n"], src.shape[0]
    out = {"q": q, "idx": idx, "dist2": d2, "n": n, "sums": sums, "fitness": n / M, "rmse": math.sqrt(float(sums["d2"]) / n) if n else 0.0,
           "U": None, "degenerate": False}
    if n:
        out["U"], out["degenerate"] = solve(sums)
    return out


def registration_icp(src: Tensor, tgt: Tensor, max_correspondence_distance: float, init=None, relative_fitness: float = RELATIVE_FITNESS,
                     relative_rmse: float = RELATIVE_RMSE, max_iteration: int = MAX_ITERATION, solver=None) -> Dict[str, object]:
    """The loop: ``transformation`` float64 [4,4] numpy, ``fitness``, ``inlier_rmse``, ``iterations`` (updates applied), ``status``,
    ``trace`` (rows ``(n, fitness, rmse, stopped)``) and the last pass under ``last``.  ``solver`` replaces ``solve`` (``solve_svd``)."""
    T = np.eye(4) if init is None else np.array(_matrix(init).numpy(), dtype=np.float64)
    solver = solve if solver is None else solver
    trace, status, prev = [], 0, None
    for k in range(int(max_iteration) + 1):
        s = step(src, tgt, T, max_correspondence_distance)
        stop = s["n"] == 0 or k == int(max_iteration)
        if prev is not None and abs(s["fitness"] - prev["fitness"]) < relative_fitness and abs(s["rmse"] - prev["rmse"]) < relative_rmse:
            stop = True
        if s["n"] == 0:
            status |= STATUS_NO_CORRESPONDENCE
        trace.append((s["n"], s["fitness"], s["rmse"], 1.0 if stop else 0.0))
        if stop:
            break
        U, degenerate = solver(s["sums"])
        if degenerate:
            status |= STATUS_DEGENERATE
        T = compose(U, T)
        prev = s
    return {"transformation": T, "fitness": s["fitness"], "inlier_rmse": s["rmse"], "iterations": len(trace) - 1, "status": status,
            "trace": trace, "last": s}
