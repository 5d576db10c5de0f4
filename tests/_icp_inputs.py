"""Seeded inputs of the mesh-alignment tests (tests/test_icp_reference.py, tests/test_gpu_icp.py).  numpy only; every coordinate is an
fp32 value, so a float64 restatement sees exactly what the fp32 kernel sees.

The target is ``_geometry_inputs.room_corner``: three orthogonal walls, so the pose is fully constrained.  The source is a seeded subset
of m target rows moved by the inverse of a known pose ``T0 = [R0 | t0]``, ``s = fl32(R0ᵀ (g - t0))``: the alignment that takes the source
onto the target is T0.  R0 turns by 1-3 degrees about (0.3, -0.5, 0.8), t0 = (tau, -0.7 tau, 0.4 tau) with tau in 0.02-0.05.
"""
import numpy as np

from _geometry_inputs import BOX, room_corner

AXIS = np.array([0.3, -0.5, 0.8])
R_MAX = 0.1                                     # get_align_transformation's threshold
FIXTURES = {"large": (4000, 3000), "small": (600, 257)}      # (target rows, source rows)
SIZES = (1, 63, 64, 65, 257, 3000, 66_000)      # 66 000 rows are 258 partials: the fold's second trip


def rotation(angle_deg: float, axis=AXIS) -> np.ndarray:
    """Rodrigues' formula in float64."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    a = np.deg2rad(angle_deg)
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def pose(angle_deg: float, tau: float) -> np.ndarray:
    T = np.eye(4)
    T[:3, :3] = rotation(angle_deg)
    T[:3, 3] = (tau, -0.7 * tau, 0.4 * tau)
    return T


def fixture(n: int, m: int, seed: int = 21, angle_deg: float = 2.0, tau: float = 0.03, noise: float = 0.0, far: int = 0):
    """(source float32 [m,3], target float32 [n,3], T0 float64 [4,4], rows int64 [m]): ``rows`` are the target rows the source was drawn
    from (with repetition when m > n).  The first ``far`` source rows are pushed 3 units out of the box along +x (as
    ``_geometry_inputs.source`` does), beyond any threshold: they count in M and never in n, and their search starts outside the index's
    bounding box."""
    tgt, _ = room_corner(n, seed)
    rng = np.random.default_rng(seed + 1000)
    rows = rng.permutation(n)[:m] if m <= n else rng.integers(0, n, size=m)
    T0 = pose(angle_deg, tau)
    g = tgt[rows].astype(np.float64)
    if noise > 0.0:
        g = g + noise * rng.standard_normal(g.shape)
    src = ((g - T0[:3, 3]) @ T0[:3, :3]).astype(np.float32)                       # rows of R0ᵀ (g - t0)
    if far:
        src[:far, 0] = (BOX[0] + 3.0 + src[:far, 0] * 0.25).astype(np.float32)
    return src, tgt, T0, rows


def perturbed(T0: np.ndarray, angle_deg: float = 0.3, shift: float = 0.004) -> np.ndarray:
    """T0 a little off: what a pass in the middle of the loop sees."""
    P = np.eye(4)
    P[:3, :3] = rotation(angle_deg, axis=(0.7, 0.2, -0.4))
    P[:3, 3] = (shift, 0.5 * shift, -shift)
    return P @ T0


def mirrored():
    """(source, target): 8 targets with x, y on a grid of spacing 10 and z in +-[0.02, 0.1], the sources the same points with z negated.
    Every source's nearest target is its twin (2 |z| <= 0.2 against a spacing of 10), and the covariance of the pairs has a negative
    determinant while sigma_2 - sigma_3 stays large: the x and y extents dwarf z."""
    xy = np.array([[0, 0], [10, 0], [20, 0], [0, 10], [10, 10], [20, 10], [0, 20], [10, 20]], dtype=np.float64)
    z = np.array([0.02, -0.05, 0.1, -0.03, 0.07, -0.1, 0.04, -0.08])
    tgt = np.concatenate([xy, z[:, None]], axis=-1).astype(np.float32)
    src = tgt.copy()
    src[:, 2] = -src[:, 2]
    return src, tgt


def planar():
    """(source, target): pairs in the plane z = 1 (rank 2), the source turned by 2 degrees about z and shifted in the plane."""
    rng = np.random.default_rng(33)
    tgt = np.concatenate([rng.uniform(0.0, 4.0, size=(40, 2)), np.ones((40, 1))], axis=-1).astype(np.float32)
    R = rotation(2.0, axis=(0.0, 0.0, 1.0))
    src = ((tgt.astype(np.float64) - np.array([0.01, -0.02, 0.0])) @ R).astype(np.float32)
    return src, tgt


def single_pair():
    """One source next to one of two distant targets: n = 1, a zero covariance."""
    tgt = np.array([[1.0, 2.0, 3.0], [40.0, 40.0, 40.0]], dtype=np.float32)
    src = np.array([[1.03, 1.98, 3.01]], dtype=np.float32)
    return src, tgt


def threshold_edge():
    """(source, target, r): one target at the origin, the sources (0.5, 0, 0) and nextafter32(0.5); with r = 0.5 the first is a
    correspondence (d² = 0.25 = r r, inclusive) and the second is not."""
    tgt = np.zeros((1, 3), dtype=np.float32)
    src = np.zeros((2, 3), dtype=np.float32)
    src[0, 0] = np.float32(0.5)
    src[1, 0] = np.nextafter(np.float32(0.5), np.float32(1.0))
    return src, tgt, 0.5


# ---- the bounds both test files hold the sums and the solve to ---------------------------------------------------------------------

def _f(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)


def fold_bounds(sums):
    """n 2^-53 (the sum of the terms' magnitudes) for every sum of ``torch_icp.moments``: a sum of n doubles in ANY order is within it of
    the exact sum, to first order, so two orders differ by at most twice this."""
    n = float(sums["n"])
    return {k: n * 2.0 ** -53 * _f(sums["abs"][k]) for k in ("d2", "q", "g", "gq")}


def polar_bound(sums):
    """(bound, E_sigma, |Sigma|_F, sigma_2 + s sigma_3): the perturbation bound of the polar factor,
    |dR|_F <= 2 (E_sigma + 64 * 2^-52 |Sigma|_F) / (sigma_2 + s sigma_3).  E_sigma is the fold bound carried into
    Sigma = S_gq / n - (S_g / n)(S_q / n); 64 stands for at most ten sweeps of three rotations at about two roundings each."""
    n = float(sums["n"])
    b = fold_bounds(sums)
    mq, mg = np.abs(_f(sums["q"])) / n, np.abs(_f(sums["g"])) / n
    E = (b["gq"] + mg[:, None] * b["q"][None, :] + mq[None, :] * b["g"][:, None]) / n
    S = _f(sums["gq"]) / n - (_f(sums["g"]) / n)[:, None] * (_f(sums["q"]) / n)[None, :]
    sv = np.linalg.svd(S, compute_uv=False)
    s = -1.0 if np.linalg.det(S) < 0 else 1.0
    gap = sv[1] + s * sv[2]
    e_sigma, norm = float(np.linalg.norm(E)), float(np.linalg.norm(S))
    bound = np.inf if gap <= 0 else 2.0 * (e_sigma + 64 * 2.0 ** -52 * norm) / gap
    return float(bound), e_sigma, norm, float(gap)
