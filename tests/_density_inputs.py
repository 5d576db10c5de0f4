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
