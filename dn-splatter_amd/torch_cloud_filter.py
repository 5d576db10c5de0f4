"""The PyTorch restatement of ``cloud_filter`` (``csrc/cloudfilter.hip``): the two point-cloud filters as ``include/dnsplat.h`` states them
— THIS PROJECT'S DEFINITION, PARITY UNPINNED AGAINST Open3D — written with tensor operations and no kernel.  It is what the kernels are
held to (``tests/test_gpu_cloud_filter.py``) and is itself held to scipy's ``cKDTree`` and numpy's float64 mean
(``tests/test_cloud_filter_reference.py``).  It runs on the CPU, or on whatever device its tensors are on.

  * ``neighbor_mean`` / ``outlier_stats`` / ``remove_statistical_outlier``: Open3D's ``remove_statistical_outlier``;
  * ``voxel_down_sample``: Open3D's ``voxel_down_sample`` with a canonical voxel order and an exact integer mean.

The neighbours are ranked as ``df_search`` ranks them, under (d², index) with d² = fma(dz, dz, fma(dy, dy, dx dx)) in double
(``torch_geometry.squared_distance`` emulates the fused operations exactly).  The additions and multiplications of the search are IEEE
on any device; the square roots are numpy's on the CPU, the correctly rounded ones of the hardware — torch's own float64 ``sqrt`` is not
(its CPU vector library is an ulp off on 0.67 % of 4 M uniform doubles) — and their sums are taken on the CPU."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .torch_geometry import squared_distance

MAX_K = 32                    # include/dnsplat.h DNSPLAT_KNN_MAX_K
NB_NEIGHBORS = 20             # the reference's callers
STD_RATIO = 2.0               # Open3D's documented example; the reference passes its own
MAX_CELLS = 2 ** 21           # voxels per axis: three indices in one 63-bit key
POS_ONE = 2.0 ** 31
ATTR_ONE = 2.0 ** 30
_PAD = 12                     # candidates beyond K that the plain sum of squares preselects


def _check_points(points: Tensor, name: str = "points") -> Tensor:
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"{name} must be [n,3] with n >= 1, got {tuple(points.shape)}")
    if points.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {points.dtype}")
    return points


def _check_neighbors(nb_neighbors: int) -> int:
    nb_neighbors = int(nb_neighbors)
    if not 1 <= nb_neighbors <= MAX_K:
        raise ValueError(f"nb_neighbors must lie in [1, {MAX_K}], got {nb_neighbors}")
    return nb_neighbors


def _rank(d2: Tensor, cols: Tensor, K: int) -> Tensor:
    """The K lowest of each row of ``d2`` under (d², index), ascending: [rows, K]."""
    by_index = torch.sort(cols, dim=1, stable=True)
    d2 = d2.gather(1, by_index.indices)
    return torch.sort(d2, dim=1, stable=True).values[:, :K]


def neighbor_d2(points: Tensor, K: int, chunk: int = 512) -> Tensor:
    """float64 [N,K]: the K lowest d² of every point to the points of the cloud (itself included) in ascending rank under (d², index).
    A point with a non-finite coordinate is nobody's neighbour; its own row is nan.  Missing ranks (fewer than K comparable points) are
    inf.  Brute force in chunks: the plain sum of squares preselects K + 12 candidates, the fused d² ranks them, and a row whose
    preselection cannot be proven complete (its last candidate within 2^-40 relative of the K-th fused d²) is ranked over the whole cloud."""
    N = points.shape[0]
    p64 = points.double()
    finite = torch.isfinite(p64).all(dim=-1)
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=points.device)
    out = torch.empty(N, K, dtype=torch.float64, device=points.device)
    C = min(N, K + _PAD)
    cols64 = [p64[:, a].contiguous() for a in range(3)]
    for i in range(0, N, chunk):
        q = p64[i:i + chunk]
        plain = None
        for a in range(3):                                                        # (dx dx + dy dy) + dz dz, one axis at a time
            d = q[:, a, None] - cols64[a][None, :]
            d = d * d
            plain = d if plain is None else plain + d
        plain = torch.where(torch.isfinite(plain) & finite[None, :], plain, inf)
        del d
        vals, cols = torch.topk(plain, C, dim=1, largest=False)
        fused = squared_distance(q[:, None, :], p64[cols])
        fused = torch.where(torch.isfinite(vals), fused, inf)
        ranked = _rank(fused, cols, K)
        if C < N:
            unsure = ~(vals[:, -1] > ranked[:, K - 1] * (1.0 + 2.0 ** -40)) & finite[i:i + chunk]
            for r in unsure.nonzero().flatten().tolist():
                full = squared_distance(q[r][None, :], p64)
                full = torch.where(torch.isfinite(plain[r]), full, inf)
                ranked[r] = _rank(full[None, :], torch.arange(N, device=points.device)[None, :], K)[0]
        out[i:i + chunk] = ranked
    out[~finite] = float("nan")
    return out


def neighbor_mean(points: Tensor, nb_neighbors: int = NB_NEIGHBORS) -> Tensor:
    """``avg`` float64 [N] on the CPU: the mean over the K = min(nb_neighbors, N) nearest points of sqrt(d²), the point itself included,
    the roots added in ascending rank one column at a time (a loop, not ``sum()``: the order is the kernel's), then divided by K.
    -1 for a row with a non-finite coordinate."""
    points = _check_points(points)
    K = min(_check_neighbors(nb_neighbors), points.shape[0])
    d = torch.from_numpy(np.sqrt(neighbor_d2(points, K).cpu().numpy()))       # IEEE roots: see the module's docstring
    s = torch.zeros(points.shape[0], dtype=torch.float64)
    for j in range(K):
        s = s + d[:, j]
    avg = s / float(K)
    avg[~torch.isfinite(points.cpu()).all(dim=-1)] = -1.0
    return avg


def outlier_stats(avg: Tensor, std_ratio: float = STD_RATIO) -> dict:
    """``n_valid`` (rows with avg >= 0), ``mean`` = (sum of avg over avg > 0) / n_valid, ``std`` = sqrt(sum of (avg - mean)² over avg > 0
    / (n_valid - 1)), ``threshold`` = mean + std_ratio std; with n_valid <= 1 std and threshold are 0.  0-dim tensors; the sums are
    torch's, so they differ from the kernel's fixed-order folds in the last bits."""
    avg = avg.double()
    n_valid = int((avg >= 0).sum())
    pos = avg[avg > 0]
    total = pos.sum()
    mean = total / n_valid if n_valid > 0 else torch.zeros((), dtype=torch.float64)
    if n_valid > 1:
        dev = pos - mean
        std = torch.sqrt((dev * dev).sum() / (n_valid - 1))
        threshold = mean + float(std_ratio) * std
    else:
        std = threshold = torch.zeros((), dtype=torch.float64)
    return {"mean": mean, "std": std, "threshold": threshold, "sum": total, "n_valid": torch.tensor(n_valid, dtype=torch.int64)}


def keep_indices(avg: Tensor, threshold) -> Tensor:
    """int64, ascending: the rows with 0 < avg < threshold."""
    return ((avg > 0) & (avg < threshold)).nonzero().flatten()


def remove_statistical_outlier(points: Tensor, nb_neighbors: int = NB_NEIGHBORS, std_ratio: float = STD_RATIO) -> Tuple[Tensor, dict]:
    """(``ind`` int64 [n_kept] ascending, ``stats``) as ``cloud_filter.remove_statistical_outlier`` returns them, on the CPU."""
    avg = neighbor_mean(points, nb_neighbors)
    stats = outlier_stats(avg, std_ratio)
    ind = keep_indices(avg, stats["threshold"])
    stats.update(avg=avg, n_kept=torch.tensor(ind.numel(), dtype=torch.int64))
    return ind, stats


def voxel_cells(points: Tensor, voxel_size: float):
    """(lo float64 [3], idx int64 [N,3], q int64 [N,3]): lo = min - voxel_size / 2, ref = (p - lo) / voxel_size, idx = floor(ref),
    q = round-half-even((ref - idx) 2^31).  Raises as the kernel's status words do."""
    points = _check_points(points)
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0 and voxel_size < float("inf")):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    if not bool(torch.isfinite(points).all()):
        raise ValueError("voxel_down_sample: a point has a non-finite coordinate")
    p = points.double()
    lo = p.min(dim=0).values - voxel_size * 0.5
    ref = (p - lo) / voxel_size
    if not bool((ref < MAX_CELLS).all()):
        raise ValueError(f"voxel_size = {voxel_size} is too small for the cloud's extent: more than 2^21 voxels along an axis")
    cell = torch.floor(ref)
    q = torch.round((ref - cell) * POS_ONE).to(torch.int64)
    return lo, cell.to(torch.int64), q


def _attribute_terms(a: Optional[Tensor], N: int, name: str) -> Optional[Tensor]:
    if a is None:
        return None
    if a.dtype != torch.float32 or tuple(a.shape) != (N, 3):
        raise ValueError(f"{name} must be float32 [{N},3], got {a.dtype} {tuple(a.shape)}")
    a = a.double()
    if not bool((a.abs() <= 2.0).all()):                    # false for a nan
        raise ValueError(f"voxel_down_sample: a component of {name} is non-finite or beyond 2 in magnitude")
    return torch.round(a * ATTR_ONE).to(torch.int64)


def voxel_down_sample(points: Tensor, voxel_size: float, normals: Optional[Tensor] = None, colors: Optional[Tensor] = None,
                      return_trace: bool = False):
    """(points', normals', colors') float64 [V,3] (None for an array that was not given); with ``return_trace`` also ``voxel_of`` int32
    [N] and ``counts`` int32 [V].  Voxels in order of first appearance; the means are exact int64 sums (``index_add_``) of the
    fixed-point terms: p' = (lo + idx voxel_size) + (voxel_size (S / n)) / 2^31, attributes (S / n) / 2^30."""
    lo, idx, q = voxel_cells(points, voxel_size)
    voxel_size = float(voxel_size)
    N = points.shape[0]
    terms = [_attribute_terms(normals, N, "normals"), _attribute_terms(colors, N, "colors")]
    key = idx[:, 0] | (idx[:, 1] << 21) | (idx[:, 2] << 42)
    uniq, inverse = torch.unique(key, return_inverse=True)
    first = torch.full((uniq.numel(),), N, dtype=torch.int64, device=points.device).scatter_reduce(
        0, inverse, torch.arange(N, device=points.device), "amin")
    order = torch.argsort(first)                                                  # the voxels by their lowest point
    number = torch.empty_like(order)
    number[order] = torch.arange(order.numel(), device=points.device)
    voxel_of = number[inverse]
    V = uniq.numel()
    n = torch.zeros(V, dtype=torch.int64, device=points.device).index_add_(0, voxel_of, torch.ones(N, dtype=torch.int64, device=points.device))
    nd = n.double()[:, None]
    S = torch.zeros(V, 3, dtype=torch.int64, device=points.device).index_add_(0, voxel_of, q)
    cell = idx[first[order]].double()
    out_points = (lo + cell * voxel_size) + (voxel_size * (S.double() / nd)) / POS_ONE
    outs = []
    for t in terms:
        if t is None:
            outs.append(None)
            continue
        St = torch.zeros(V, 3, dtype=torch.int64, device=points.device).index_add_(0, voxel_of, t)
        outs.append((St.double() / nd) / ATTR_ONE)
    result = (out_points, outs[0], outs[1])
    return result + (voxel_of.to(torch.int32), n.to(torch.int32)) if return_trace else result
