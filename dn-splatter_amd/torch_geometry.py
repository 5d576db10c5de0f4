"""The reference's geometry scores in plain PyTorch, restated from their behaviour: ``distance_p2p`` / ``get_threshold_percentage`` /
``compute_metrics`` (dn_splatter/eval/eval_mesh_vis_cull.py:290-397) and ``calculate_accuracy`` / ``calculate_completeness`` /
``PDMetrics`` (dn_splatter/metrics.py:11-56), plus the mesh sampler ``geometry.hip`` defines (``mesh.sample(count, return_index=True)``;
PARITY UNPINNED against trimesh, whose draws come from numpy's global generator).  Everything runs on whatever device the tensors are
on; float64 throughout except the sampled points, which are the kernel's fp32 statements.

The nearest neighbour is ranked as the kernel ranks it: under (d², index) with d² = fma(dz, dz, fma(dy, dy, dx dx)) in double.  PyTorch has
no fused multiply-add for tensors, so ``fma`` emulates one exactly from IEEE additions and multiplications (Dekker's product, Knuth's sum
and a last sum rounded to odd: Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums", 2008).  It holds while nothing
over- or underflows: |a b| and |c| between 2^-960 and 2^960.  Pinned to the reference's own outputs by
tests/golden/reference_geometry.npz.  ``geometry.py`` is the HIP path."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
from torch import Tensor

THRESHOLD = 0.05            # compute_metrics' one threshold, calculate_completeness' default
PERCENTILE = 90.0           # calculate_accuracy's default
SAMPLES_PER_AREA = 1e4      # compute_metrics: int(area * 1e4) samples per mesh
GEOM_KEYS = ("mean_d", "mean_d2", "mean_absdot", "percentile", "share_lt", "share_le", "min_d", "max_d", "order_lo_d2", "order_hi_d2")
GEOM_INDEX = {k: i for i, k in enumerate(GEOM_KEYS)}        # include/dnsplat.h DNSPLAT_GEOM_*
GEOM_COUNT = 12
COUNT_KEYS = ("n", "n_lt", "n_le", "n_nonfinite")
COUNT_INDEX = {k: i for i, k in enumerate(COUNT_KEYS)}
GEOM_COUNTS = 4
METRIC_KEYS = ("Acc", "Comp", "C-L1", "C-L2", "NC", "F-score", "precision", "recall")


# ---- an exact fused multiply-add of float64 tensors --------------------------------------------------------------------------------

def _two_sum(a: Tensor, b: Tensor):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a: Tensor):
    c = a * 134217729.0                 # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a: Tensor, b: Tensor):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, (((ah * bh - p) + ah * bl) + al * bh) + al * bl


def _sum_to_odd(a: Tensor, b: Tensor) -> Tensor:
    """a + b rounded to odd: the exact sum if it is a double, else the neighbour of it whose last mantissa bit is set."""
    s, e = _two_sum(a, b)
    bits = s.contiguous().view(torch.int64)
    inexact_even = (e != 0) & ((bits & 1) == 0)
    away = (e > 0) == (s > 0)                                           # the rest points away from zero: the larger magnitude
    step = torch.where(away, torch.ones_like(bits), -torch.ones_like(bits))
    return torch.where(inexact_even, bits + step, bits).view(torch.float64)


def fma(a: Tensor, b: Tensor, c: Tensor) -> Tensor:
    """round(a b + c) with ONE rounding, float64, elementwise."""
    a, b, c = torch.broadcast_tensors(a.double(), b.double(), c.double())
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    return vh + _sum_to_odd(tl, vl)


def squared_distance(q: Tensor, p: Tensor) -> Tensor:
    """d² of rows of ``q`` and ``p`` ([..., 3], any float dtype; fp32 converts exactly) as ``df_search`` states it."""
    d = q.double() - p.double()
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return fma(dz, dz, fma(dy, dy, dx * dx))


# ---- one direction of distance_p2p -------------------------------------------------------------------------------------------------

def nearest(tgt: Tensor, src: Tensor, chunk: int = 1024):
    """(idx int64 [M], d² float64 [M]): for every row of ``src`` the row of ``tgt`` of lowest (d², index), d² as ``squared_distance``.  A
    source row with a non-finite coordinate, or one no target can be compared with, gets -1 and nan; a target row with a nan or inf
    coordinate (d² nan or inf) is compared with nobody, as include/dnsplat.h states.  Brute force: the plain sum of
    squares picks the candidates within 2^-48 relative of the row's minimum (it differs from the fused one by three roundings), the fused
    d² then ranks those."""
    N, M = tgt.shape[0], src.shape[0]
    dev = src.device
    idx = torch.full((M,), -1, dtype=torch.int64, device=dev)
    d2 = torch.full((M,), float("nan"), dtype=torch.float64, device=dev)
    t64 = tgt.double()
    for i in range(0, M, chunk):
        q = src[i:i + chunk].double()
        d = q[:, None, :] - t64[None, :, :]
        plain = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        plain = torch.where(torch.isfinite(plain), plain, torch.full_like(plain, float("inf")))
        plain[~torch.isfinite(q).all(dim=-1)] = float("inf")
        best = plain.min(dim=1).values
        cand = (plain <= best[:, None] * (1.0 + 2.0 ** -48)) & torch.isfinite(plain)
        rows, cols = cand.nonzero(as_tuple=True)
        if rows.numel() == 0:
            continue
        fused = squared_distance(q[rows], t64[cols])
        row_min = torch.full((q.shape[0],), float("inf"), dtype=torch.float64, device=dev).scatter_reduce(0, rows, fused, "amin")
        at_min = fused == row_min[rows]
        row_idx = torch.full((q.shape[0],), N, dtype=torch.int64, device=dev).scatter_reduce(0, rows[at_min], cols[at_min], "amin")
        found = row_idx < N
        idx[i:i + chunk] = torch.where(found, row_idx, torch.full_like(row_idx, -1))
        d2[i:i + chunk] = torch.where(found, row_min, torch.full_like(row_min, float("nan")))
    return idx, d2


def abs_normal_dot(src_normals: Tensor, tgt_normals: Tensor, idx: Tensor) -> Tensor:
    """| n_src / |n_src| . n_tgt[idx] / |n_tgt[idx]| | in float64, the sums (a + b) + c; nan where idx is -1 or a normal is zero."""
    s = src_normals.double()
    g = tgt_normals.double()[idx.clamp(min=0)]
    s = s / torch.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])[:, None]
    g = g / torch.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])[:, None]
    dot = ((g[:, 0] * s[:, 0] + g[:, 1] * s[:, 1]) + g[:, 2] * s[:, 2]).abs()
    return torch.where(idx >= 0, dot, torch.full_like(dot, float("nan")))


def percentile_linear(d2: Tensor, q: float):
    """(d² of rank floor(h), d² of rank min(floor(h) + 1, n - 1), numpy.percentile(sqrt(d2), q)) — numpy's default method: h = (n - 1)
    (q / 100), ``_lerp`` of the two order statistics of d = sqrt(d²).  0-dim float64 tensors; the percentile is nan if any d² is."""
    n = d2.numel()
    srt = torch.sort(d2).values                                         # nan sorts last, as its bit pattern does
    h = (n - 1) * (q / 100.0)
    k0 = min(int(math.floor(h)), n - 1)
    k1 = min(k0 + 1, n - 1)
    g = h - k0
    lo2, hi2 = srt[k0], srt[k1]
    a, b = torch.sqrt(lo2), torch.sqrt(hi2)
    diff = b - a
    value = b - diff * (1.0 - g) if g >= 0.5 else a + diff * g
    if bool(torch.isnan(d2).any()):
        value = torch.full_like(value, float("nan"))
    return lo2, hi2, value


def cloud_distances(src: Tensor, tgt: Tensor, src_normals: Optional[Tensor] = None, tgt_normals: Optional[Tensor] = None,
                    threshold: float = THRESHOLD, percentile: float = PERCENTILE) -> Dict[str, Tensor]:
    """What ``dnsplat_cloud_distances`` returns, under the same names: ``dist2`` [M] float64, ``idx`` [M] int64, ``absdot`` [M] float64 or
    None, ``scalars`` float64 [12] at ``GEOM_INDEX`` and ``counts`` int64 [4] at ``COUNT_INDEX``."""
    if (src_normals is None) != (tgt_normals is None):
        raise ValueError("source and target normals are given together or not at all")
    if not 0.0 <= percentile <= 100.0:
        raise ValueError(f"percentile must lie in [0, 100], got {percentile}")
    idx, d2 = nearest(tgt, src)
    d = torch.sqrt(d2)
    absdot = abs_normal_dot(src_normals, tgt_normals, idx) if src_normals is not None else None
    n = d.numel()
    bad = int((idx < 0).sum())
    nan = torch.full((), float("nan"), dtype=torch.float64, device=d.device)
    lo2, hi2, pct = percentile_linear(d2, percentile)
    n_lt, n_le = (d < threshold).sum(), (d <= threshold).sum()
    n_t = torch.full((), float(n), dtype=torch.float64, device=d.device)   # a tensor: division by a Python scalar may multiply by 1 / n
    scalars = torch.zeros(GEOM_COUNT, dtype=torch.float64, device=d.device)
    scalars[:10] = torch.stack([d.sum() / n_t, d2.sum() / n_t, absdot.sum() / n_t if absdot is not None else nan, pct, n_lt.double() / n_t, n_le.double() / n_t,
                                nan if bad else d.min(), nan if bad else d.max(), lo2, hi2])
    counts = torch.stack([torch.full_like(n_lt, n), n_lt, n_le, torch.full_like(n_lt, bad)])
    return {"dist2": d2, "idx": idx, "absdot": absdot, "scalars": scalars, "counts": counts}


def calculate_accuracy(reconstructed: Tensor, reference: Tensor, percentile: float = 90) -> Tensor:
    """metrics.py:39-45: the ``percentile``-th percentile of the distances from the reconstruction to the reference cloud."""
    return cloud_distances(reconstructed, reference, percentile=float(percentile))["scalars"][GEOM_INDEX["percentile"]]


def calculate_completeness(reconstructed: Tensor, reference: Tensor, threshold: float = 0.05) -> Tensor:
    """metrics.py:48-56: the share of the reference cloud with d < ``threshold`` of the reconstruction, TIMES 100."""
    return cloud_distances(reference, reconstructed, threshold=threshold)["scalars"][GEOM_INDEX["share_lt"]] * 100


def metrics_from_directions(comp: Tensor, acc: Tensor) -> Dict[str, Tensor]:
    """compute_metrics' dictionary (:360-395) from the scalars of the two directions — ``comp``: target to prediction, ``acc``: prediction
    to target — plus C-L2, precision and recall, which the reference computes and does not return.  F is nan when P + R == 0."""
    g = GEOM_INDEX
    precision, recall = acc[g["share_le"]], comp[g["share_le"]]
    return {"Acc": acc[g["mean_d"]], "Comp": comp[g["mean_d"]], "C-L1": 0.5 * (comp[g["mean_d"]] + acc[g["mean_d"]]),
            "C-L2": 0.5 * (comp[g["mean_d2"]] + acc[g["mean_d2"]]),
            "NC": 0.5 * comp[g["mean_absdot"]] + 0.5 * acc[g["mean_absdot"]],
            "F-score": 2 * precision * recall / (precision + recall), "precision": precision, "recall": recall}


def cloud_metrics(pred_points: Tensor, pred_normals: Optional[Tensor], tgt_points: Tensor, tgt_normals: Optional[Tensor],
                  threshold: float = THRESHOLD) -> Dict[str, Tensor]:
    """compute_metrics behind its two ``sample`` calls: both directions of ``distance_p2p`` on two oriented clouds."""
    comp = cloud_distances(tgt_points, pred_points, tgt_normals, pred_normals, threshold=threshold)["scalars"]
    acc = cloud_distances(pred_points, tgt_points, pred_normals, tgt_normals, threshold=threshold)["scalars"]
    return metrics_from_directions(comp, acc)


# ---- the mesh sampler --------------------------------------------------------------------------------------------------------------

def mesh_areas(vertices: Tensor, triangles: Tensor):
    """(areas float64 [T], unit face normals float32 [T,3]) as ``dnsplat_mesh_areas`` states them: the cross product in double from the
    fp32 vertices; area 0 and normal 0 for a zero-area face, an index outside [0, V) or a non-finite cross product."""
    V = vertices.shape[0]
    tri = triangles.long()
    ok = ((tri >= 0) & (tri < V)).all(dim=-1)
    v = vertices.double()[tri.clamp(0, V - 1)]
    a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    cr = torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], dim=-1)
    length = torch.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
    ok = ok & (length > 0) & torch.isfinite(length)
    safe = torch.where(ok, length, torch.ones_like(length))
    areas = torch.where(ok, 0.5 * length, torch.zeros_like(length))
    normals = torch.where(ok[:, None], cr / safe[:, None], torch.zeros_like(cr)).float()
    return areas, normals


_M32 = 0xFFFFFFFF
_GOLDEN = 0x9E3779B9


def mix32(x: Tensor) -> Tensor:
    """``dns_mix32`` (csrc/block_reduce.h) on int64 tensors that hold uint32 values."""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32                                         # wraps in int64: the low 32 bits are the product's
    return x ^ (x >> 16)


def sample_words(count: int, seed: int, device) -> Tensor:
    """int64 [count,3]: the three uint32 words of every sample, as include/dnsplat.h states them."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    one = lambda v: torch.tensor([v & _M32], dtype=torch.int64, device=device)  # noqa: E731
    key = mix32(one(seed) ^ mix32(one((seed >> 32) + _GOLDEN)))
    c = mix32((torch.arange(count, dtype=torch.int64, device=device) & _M32) ^ key)
    return torch.stack([mix32((c + k * _GOLDEN) & _M32) for k in (1, 2, 3)], dim=-1)


def mesh_sample(count: int, seed: int, cdf: Tensor, vertices: Tensor, triangles: Tensor, face_normals: Tensor):
    """(points float32 [S,3], normals float32 [S,3], faces int64 [S]) as ``dnsplat_mesh_sample`` states them, from the caller's ``cdf``."""
    dev = vertices.device
    w = sample_words(count, seed, dev)
    total = cdf[-1]
    V, T = vertices.shape[0], triangles.shape[0]
    t = (w[:, 0].double() + 0.5) / 4294967296.0 * total
    faces = torch.searchsorted(cdf, t, right=True).clamp(max=T - 1)       # the first f with cdf[f] > t
    tri = triangles.long()[faces]
    ok = ((tri >= 0) & (tri < V)).all(dim=-1) & bool((total > 0) & torch.isfinite(total))
    u, v = w[:, 1] >> 8, w[:, 2] >> 8
    flip = u + v > (1 << 24)
    u, v = torch.where(flip, (1 << 24) - u, u), torch.where(flip, (1 << 24) - v, v)
    r1, r2 = (u.float() * 2.0 ** -24)[:, None], (v.float() * 2.0 ** -24)[:, None]
    vert = vertices.float()[tri.clamp(0, V - 1)]
    v0 = vert[:, 0]
    e1, e2 = vert[:, 1] - v0, vert[:, 2] - v0
    points = (v0 + r1 * e1) + r2 * e2
    points = torch.where(ok[:, None], points, torch.full_like(points, float("nan")))
    normals = torch.where(ok[:, None], face_normals.float()[faces], torch.zeros_like(points))
    if not bool((total > 0) & torch.isfinite(total)):
        faces = torch.full_like(faces, -1)
    return points, normals, faces


def sample_mesh_surface(vertices: Tensor, triangles: Tensor, count: Optional[int] = None, samples_per_area: float = SAMPLES_PER_AREA,
                        seed: int = 0):
    """The restatement of ``geometry.sample_mesh_surface``: areas, ``torch.cumsum`` in float64, ``int(area * samples_per_area)`` samples."""
    areas, normals = mesh_areas(vertices, triangles)
    cdf = torch.cumsum(areas, dim=0)
    if count is None:
        count = int(float(cdf[-1]) * samples_per_area)
    return mesh_sample(int(count), seed, cdf, vertices, triangles, normals)


def barycentrics(points: Tensor, vertices: Tensor, triangles: Tensor, faces: Tensor) -> Tensor:
    """float64 [S,3]: the barycentric coordinates of every sample in its triangle, recomputed in double (least squares in the plane)."""
    v = vertices.double()[triangles.long()[faces]]
    e1, e2, w = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], points.double() - v[:, 0]
    d11, d12, d22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    w1, w2 = (w * e1).sum(-1), (w * e2).sum(-1)
    det = d11 * d22 - d12 * d12
    b1, b2 = (d22 * w1 - d12 * w2) / det, (d11 * w2 - d12 * w1) / det
    return torch.stack([1.0 - b1 - b2, b1, b2], dim=-1)
