"""Inputs of the density-field tests (test_density_reference.py, test_gpu_density.py) and of the fixture's generator
(golden/make_reference_density_golden.py): one recipe.

``field_inputs``: N Gaussians with the reference's init law — means ``(rand(N,3) - 0.5) * 10`` (dn_model.py:135), log-scales
``log(mean 3-NN distance)`` (:186-189) halved and made anisotropic by a per-axis factor, ``random_quat_tensor`` rotations scaled off unit norm,
opacity logits of both signs — and M samples: uniform in the box, a quarter of them a fraction of a scale away from a mean (densities on
both sides of the ``>= 1`` switch), the last ``FAR`` far outside the box."""
import math

import numpy as np
import torch

N_FIX, M_FIX, FAR = 4099, 2048, 8
SEED = 20
RANKS = 18                      # ranks 0 .. 17 of every query enter the gap condition (k + skip = 17, and the one behind)
GAP = 2.0 ** -40                # smallest allowed relative gap of consecutive fp64 d²
SWITCH_ENVELOPE = 1e-5          # |sum - 1| below this in fp64: the fp32 sum may take the other side of the >= 1 switch
GOLDEN = "reference_density.npz"

# e_ref: the error of the reference's OWN fp32 outputs against the fp64 restatement on the fixture, as the generator printed it
# (density relative to max(value, 1e-4), normals component-wise); test_density_reference.py holds the file to these numbers.  The HIP
# outputs get 4 x e_ref: the margin covers another summation order and another exp.  Samples flagged at the switch get 1e-5 more.
E_REF_DENSITY = 1.619e-06
E_REF_NORMAL = 4.509e-06
TOL_DENSITY = 4 * E_REF_DENSITY
TOL_NORMAL = 4 * E_REF_NORMAL
TOL_SWITCH_EXTRA = 1e-5


def random_quats(n, g):
    u, v, w = (torch.rand(n, generator=g) for _ in range(3))
    r1, r2 = torch.sqrt(1.0 - u), torch.sqrt(u)
    a, b = 2.0 * math.pi * v, 2.0 * math.pi * w
    return torch.stack((r1 * torch.sin(a), r1 * torch.cos(a), r2 * torch.sin(b), r2 * torch.cos(b)), dim=-1)


def brute_d2(points, queries):
    d = queries.double()[:, None, :] - points.double()[None, :, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def field_inputs(N=N_FIX, M=M_FIX, seed=SEED, far=FAR):
    """dict of float32 host tensors: means [N,3], scales [N,3] (log), quats [N,4], opacities [N,1] (logit), samples [M,3]."""
    g = torch.Generator().manual_seed(seed)
    means = (torch.rand(N, 3, generator=g) - 0.5) * 10
    k3 = min(3, N - 1)
    if k3 > 0:
        d2 = torch.sort(brute_d2(means, means), dim=1).values[:, 1:1 + k3]
        avg = d2.sqrt().mean(dim=-1, keepdim=True).float()
    else:
        avg = torch.ones(N, 1)
    scales = torch.log(avg.repeat(1, 3)) - 0.7 + 0.6 * torch.randn(N, 3, generator=g)
    quats = random_quats(N, g) * (0.5 + torch.rand(N, 1, generator=g))
    opacities = 2.5 * torch.randn(N, 1, generator=g)
    samples = (torch.rand(M, 3, generator=g) - 0.5) * 10
    near = torch.arange(0, M, 4)
    pick = torch.randint(0, N, (near.numel(),), generator=g)
    samples[near] = means[pick] + 0.3 * torch.exp(scales[pick]) * torch.randn(near.numel(), 3, generator=g)
    if far and M > far:
        samples[M - far:] = (torch.rand(far, 3, generator=g) - 0.5) * 10 + torch.tensor([[40.0, -25.0, 60.0]]) * torch.sign(
            torch.randn(far, 3, generator=g))
    return {k: v.float().contiguous() for k, v in dict(means=means, scales=scales, quats=quats, opacities=opacities, samples=samples).items()}


def smallest_rank_gap(points, queries, ranks=RANKS):
    """The smallest relative gap between consecutive ranks 0 .. ranks - 1 of the fp64 d² over all queries."""
    d2 = torch.sort(brute_d2(points, queries), dim=1).values[:, :min(ranks, points.shape[0])]
    if d2.shape[1] < 2:
        return float("inf")
    gap = (d2[:, 1:] - d2[:, :-1]) / d2[:, 1:].clamp_min(1e-300)
    return float(gap.min())


def uniform_means(N, seed):
    """float32 [N,3]: the means of ``field_inputs``' law alone, ``(rand(N,3) - 0.5) * 10``, for sizes at which its N x N scale
    initialisation is out of reach."""
    return ((torch.rand(N, 3, generator=torch.Generator().manual_seed(seed)) - 0.5) * 10).float().contiguous()


# ---- the k-NN index (csrc/density_common.h, csrc/density.hip), restated in NumPy -------------------------------------------------------

KNN_MAX_GRID = 128              # include/dnsplat.h DNSPLAT_KNN_MAX_GRID
INDEX_HEADER_BYTES = 64         # density_common.h DfHeader


def index_grid_dim(N, cap=KNN_MAX_GRID):
    """df_grid_dim: the largest G with 2 G^3 <= N (about two points per cell), at least 1, at most ``cap``.  In integers."""
    g = 1
    while 2 * (g + 1) ** 3 <= N:
        g += 1
    return min(g, cap)


def index_restatement(means):
    """The part of the index buffer a query reads, for float32 means [N,3], written from the statements of density_common.h and
    density.hip and not from their code: a dict with

      G, C            cells per axis and G^3
      lo, hi, inv_h   float32 [3]: the exact bounding box; inv_h = fl32(G / fl32(hi - lo)), 0 where the extent is 0 or infinite or the
                      quotient overflows (the axis is one cell thick there)
      g               int32 [3]: G where inv_h > 0, else 1
      cell            int64 [N]: (c2 G + c1) G + c0 with c_a = t >= 0 ? int(min(t, g_a - 1)) : 0, t = fl32(fl32(p_a - lo_a) inv_h_a) —
                      numpy's float32 operations round once each, as __fsub_rn and __fmul_rn do
      cell_start      int32 [C + 1]: the exclusive prefix sum of the cell histogram, the last entry N
      order           int64 [N]: the Gaussian indices in stable order of cell id (ascending index inside a cell)
      bytes           uint8: the 64-byte header (its padding zero), cell_start padded with zeros to 16 bytes, then the rows
                      (x, y, z, bits of index) in ``order``."""
    p = np.ascontiguousarray(means.numpy() if torch.is_tensor(means) else means, dtype=np.float32)
    N = p.shape[0]
    G = index_grid_dim(N)
    C = G ** 3
    lo, hi = p.min(axis=0), p.max(axis=0)
    inv_h = np.zeros(3, dtype=np.float32)
    with np.errstate(all="ignore"):
        ext = hi - lo
        for a in range(3):
            if ext[a] > 0 and np.isfinite(ext[a]):
                q = np.float32(G) / ext[a]
                inv_h[a] = q if np.isfinite(q) else 0.0
        g = np.where(inv_h > 0, G, 1).astype(np.int32)
        c = []
        for a in range(3):
            t = (p[:, a] - lo[a]) * inv_h[a]
            assert t.dtype == np.float32
            c.append(np.where(t >= 0, np.minimum(t, np.float32(g[a] - 1)), np.float32(0)).astype(np.int64))
    cell = (c[2] * G + c[1]) * G + c[0]
    cell_start = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=C))]).astype(np.int32)
    order = np.argsort(cell, kind="stable")
    at_sorted = (INDEX_HEADER_BYTES + 4 * (C + 1) + 15) // 16 * 16
    raw = np.zeros(at_sorted + 16 * N, dtype=np.uint8)
    raw[0:12], raw[12:24], raw[24:36], raw[36:48] = lo.view(np.uint8), hi.view(np.uint8), inv_h.view(np.uint8), g.view(np.uint8)
    raw[INDEX_HEADER_BYTES:INDEX_HEADER_BYTES + 4 * (C + 1)] = cell_start.view(np.uint8)
    rows = np.empty((N, 4), dtype=np.int32)
    rows[:, :3] = p[order].view(np.int32)
    rows[:, 3] = order
    raw[at_sorted:] = rows.reshape(-1).view(np.uint8)
    return dict(G=G, C=C, lo=lo, hi=hi, inv_h=inv_h, g=g, cell=cell, cell_start=cell_start, order=order, at_sorted=at_sorted, bytes=raw)


def load_golden(path):
    g = np.load(path)
    t = {k: torch.from_numpy(g[k].astype(np.float32)) for k in ("means", "scales", "quats", "opacities", "samples")}
    return g, t


class Box:
    """nerfstudio's OrientedBox attributes: R [3,3], T [3], S [3]."""

    def __init__(self, R, T, S):
        self.R, self.T, self.S = R, T, S


def crop_box(device="cpu"):
    c, s = math.cos(0.4), math.sin(0.4)
    return Box(torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], device=device), torch.tensor([0.3, -0.2, 0.5], device=device),
               torch.tensor([5.0, 7.0, 6.0], device=device))


VOLUME_R, VOLUME_RADIUS = 12, 4.5          # the lattice of the fixture's marching-cubes case
