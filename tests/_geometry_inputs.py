"""Seeded inputs of the geometry-score tests (tests/test_geometry_reference.py, tests/test_gpu_geometry.py) and of
tests/golden/make_reference_geometry_golden.py.  numpy only; every coordinate is an fp32 value, so a float64 reference sees exactly what
the fp32 kernel sees.

The "room corner": points on three walls of a 4 x 3 x 2.5 box — the floor z = 0, the wall x = 0 and the wall y = 0 — drawn uniformly by
area, with the walls' inward normals (scaled by a per-point length in [0.5, 2], so that the normalisation has work to do).  A surface
cloud is what the scores are run on in practice: it fills few cells of the uniform grid.  The source is a second draw with sigma = 0.04
noise on every coordinate; its first ``FAR`` points are pushed 3 units outside the box along +x, so that the search starts outside the
bounding box of the index and must widen its cube.
"""
import numpy as np

BOX = (4.0, 3.0, 2.5)
SIGMA = 0.04
FAR = 40
N_TARGET, N_SOURCE = 4000, 3000         # the sizes of tests/golden/reference_geometry.npz


def room_corner(n: int, seed: int, noise: float = 0.0):
    """(points [n,3] float32, normals [n,3] float32)."""
    rng = np.random.default_rng(seed)
    bx, by, bz = BOX
    areas = np.array([bx * by, by * bz, bx * bz])
    wall = rng.choice(3, size=n, p=areas / areas.sum())
    u, v = rng.random(n), rng.random(n)
    pts = np.zeros((n, 3))
    nrm = np.zeros((n, 3))
    floor, wx, wy = wall == 0, wall == 1, wall == 2
    pts[floor] = np.stack([u[floor] * bx, v[floor] * by, np.zeros(floor.sum())], axis=-1)
    pts[wx] = np.stack([np.zeros(wx.sum()), u[wx] * by, v[wx] * bz], axis=-1)
    pts[wy] = np.stack([u[wy] * bx, np.zeros(wy.sum()), v[wy] * bz], axis=-1)
    nrm[floor, 2] = 1.0
    nrm[wx, 0] = 1.0
    nrm[wy, 1] = 1.0
    # a tilt and a length: |dot| spreads over (0.7, 1] and the normals are not unit vectors
    nrm = (nrm + 0.3 * rng.standard_normal((n, 3))) * rng.uniform(0.5, 2.0, size=(n, 1))
    if noise > 0.0:
        pts = pts + noise * rng.standard_normal((n, 3))
    return pts.astype(np.float32), nrm.astype(np.float32)


def target(n: int = N_TARGET, seed: int = 11):
    return room_corner(n, seed)


def source(m: int = N_SOURCE, seed: int = 12, far: int = FAR):
    """The noisy second draw; the first min(far, m // 2) points lie 3 units beyond the box along +x."""
    pts, nrm = room_corner(m, seed, noise=SIGMA)
    k = min(far, m // 2)
    pts[:k, 0] = (BOX[0] + 3.0 + pts[:k, 0] * 0.25).astype(np.float32)
    return pts, nrm


# ---- small meshes of the sampler tests ---------------------------------------------------------------------------------------------

def tetrahedron():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.5, 0.0], [0.0, 0.0, 2.0]], dtype=np.float32)
    t = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)
    return v, t


def square_with_degenerate():
    """Two triangles of the unit square with a zero-area face (two equal corners) BETWEEN them."""
    v = np.array([[0.0, 0.0, 0.5], [1.0, 0.0, 0.5], [1.0, 1.0, 0.5], [0.0, 1.0, 0.5]], dtype=np.float32)
    t = np.array([[0, 1, 2], [1, 1, 3], [0, 2, 3]], dtype=np.int32)
    return v, t


def grid_mesh(n: int = 12, seed: int = 5):
    """An n x n grid of quads over [0, 2] x [0, 1], split into triangles, on a bumpy height field: 2 n^2 faces of unequal area."""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.linspace(0.0, 2.0, n + 1) ** 1.3, np.linspace(0.0, 1.0, n + 1), indexing="ij")
    z = 0.2 * rng.standard_normal(xs.shape)
    v = np.stack([xs, ys, z], axis=-1).reshape(-1, 3).astype(np.float32)
    idx = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    t = np.concatenate([np.stack([a, b, c], axis=-1), np.stack([a, c, d], axis=-1)]).astype(np.int32)
    return v, t


def sphere_volume(n: int = 33):
    """The smooth test lattice of the marching-cubes tests: a sphere of radius 0.3 (n - 1) + 0.4 lattice units, centred off the points."""
    s = float(n - 1)
    x = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij"), axis=-1)
    centre = 0.37 * s + 0.0131
    return (0.3 * s + 0.4 - np.linalg.norm(x - centre, axis=-1)).astype(np.float32), centre, 0.3 * s + 0.4
