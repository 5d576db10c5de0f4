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


# ---- the distance lattice (tests/test_gpu_geometry_edges.py) -------------------------------------------------------------------------
# Sources (1 + a 2^-23, j 2^-21, i 2^-26) against the origin: dx² = 1 + a 2^-22 + a² 2^-46, dy² = j² 2^-42, dz² = i² 2^-52, every term a
# multiple of 2^-52 and the sum below 2, so the two FMAs of d² round nothing and its 64-bit pattern is the integer
#     0x3FF0000000000000 + (a << 30) + (a² << 6) + (j² << 10) + i²
# With a = 0 and j, i < 32 that is 0x3FF... | j² << 10 | i²: 1024 values that agree above bit 20 and differ in the bits of the last two
# rounds of the selection (bits 10-19 and 0-9).  a = 1 sets bit 30 (the fourth round's top bit), a = 2 bit 31 (the third round),
# a = 4096 bit 42 (the second); a far source (3 + k / 4, 0, 0) has another exponent (the first round).

LATTICE_TARGET = np.array([[0.0, 0.0, 0.0], [50.0, 50.0, 50.0], [-40.0, 3.0, 9.0]], dtype=np.float32)
LATTICE_ONE = 0x3FF0000000000000        # the pattern of d² = 1.0
LATTICE_A_MAX = 1 << 20                 # dx² needs 2 * 23 bits below the leading one: exact in double; and the pattern stays below 2.0


def lattice_points(a, j, i):
    """float32 [n,3]: the sources of the integer triples; every coordinate is exact in fp32 for a < 2^23, j and i < 2^24."""
    a, j, i = (np.asarray(x, dtype=np.int64) for x in (a, j, i))
    assert a.min() >= 0 and a.max() < LATTICE_A_MAX and min(j.min(), i.min()) >= 0 and max(j.max(), i.max()) < 1 << 10
    pts = np.stack([1.0 + a * 2.0 ** -23, j * 2.0 ** -21, i * 2.0 ** -26], axis=-1)
    out = pts.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), pts), "a lattice coordinate is no fp32 value"
    return out


def lattice_patterns(a, j, i):
    """int64 [n]: the 64-bit pattern of d² to the origin of every triple, in integer arithmetic (the derivation above)."""
    a, j, i = (np.asarray(x, dtype=np.int64) for x in (a, j, i))
    return LATTICE_ONE + (a << 30) + ((a * a) << 6) + ((j * j) << 10) + i * i


def far_points(k: int):
    """float32 [k,3]: (3 + n / 4, 0, 0), d² = (3 + n / 4)² to the origin — another exponent than the lattice's."""
    pts = np.zeros((k, 3), dtype=np.float32)
    pts[:, 0] = 3.0 + 0.25 * np.arange(k)
    return pts


def distance_lattice(m: int, seed: int, a_values=(0,), n_j: int = 32, n_i: int = 32, far: int = 0):
    """(src float32 [m,3], tgt float32 [3,3], patterns int64 [m], triples int64 [m,3]): m sources drawn WITH repetition (seeded) from the
    len(a_values) n_j n_i lattice triples, so that the final bins of the selection hold ties; if m - far covers the lattice, every triple
    occurs at least once.  The first ``far`` rows are ``far_points`` (triple -1).  ``patterns`` is the exact pattern of every row's d² to
    the origin, which is the nearest target of every row."""
    rng = np.random.default_rng(seed)
    a_values = np.asarray(a_values, dtype=np.int64)
    total = len(a_values) * n_j * n_i
    n = m - far
    pick = rng.integers(0, total, size=n)
    if n >= total:
        pick[:total] = rng.permutation(total)
    a, rest = a_values[pick // (n_j * n_i)], pick % (n_j * n_i)
    j, i = rest // n_i, rest % n_i
    src = np.concatenate([far_points(far), lattice_points(a, j, i)])
    x = far_points(far)[:, 0].astype(np.float64)
    patterns = np.concatenate([(x * x).view(np.int64), lattice_patterns(a, j, i)])
    triples = np.concatenate([np.full((far, 3), -1, dtype=np.int64), np.stack([a, j, i], axis=-1)])
    return src, LATTICE_TARGET.copy(), patterns, triples


ROUND_BITS = (11, 11, 11, 11, 10, 10)    # geometry.hip gm_bits; tests/test_gpu_geometry_edges.py reads them out of the source


def split_round(p, q, bits=ROUND_BITS):
    """The first round of the radix selection (``bits`` per round, from the top of a 64-bit pattern) in which the patterns p and q fall
    into different bins; len(bits) if they are equal."""
    shift = 64
    for r, b in enumerate(bits):
        shift -= b
        if (int(p) >> shift) != (int(q) >> shift):
            return r
    return len(bits)


def rank_percentile(k: int, n: int):
    """A percentile whose virtual index (n - 1) (q / 100) lies at k + 1/2: numpy's two order statistics are ranks k and k + 1."""
    return 100.0 * (k + 0.5) / (n - 1)


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


def square_between_degenerates():
    """``square_with_degenerate`` with two zero-area faces in front and two behind (T = 7): the cdf starts with two zeros and ends with
    three equal entries.  The faces with area are 2 and 4."""
    v, t = square_with_degenerate()
    front = np.array([[0, 0, 1], [2, 2, 2]], dtype=np.int32)
    back = np.array([[3, 1, 1], [0, 3, 0]], dtype=np.int32)
    return v, np.concatenate([front, t, back])


def collinear_mesh():
    """Three faces over three collinear vertices: every area is 0, and so is the whole cdf."""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 0.5], [2.0, 4.0, 1.0]], dtype=np.float32)
    t = np.array([[0, 1, 2], [2, 1, 0], [0, 2, 1]], dtype=np.int32)
    return v, t


def one_triangle():
    v = np.array([[0.25, -1.0, 0.5], [1.5, 0.0, 0.75], [0.0, 2.0, -0.5]], dtype=np.float32)
    return v, np.array([[0, 1, 2]], dtype=np.int32)


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
