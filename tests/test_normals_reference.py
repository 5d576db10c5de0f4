"""dn_splatter_amd/torch_normals.py — the restatement csrc/normals.hip is held to bit for bit — against independent statements: scipy's
cKDTree for the neighbour sets, numpy's ``cov`` for the covariance, numpy's ``eigh`` and a 50-digit mpmath solve for the normal, known
answers on a plane and a sphere, and the reference's own ``backproject`` / ``compute_angle_between_normals`` through golden arrays.
``estimate_normals`` itself cannot be pinned against Open3D, which is absent: the rule is this project's definition."""
import functools
import os

import numpy as np
import pytest
import torch

import _normals_inputs as inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_depth_normals.npz")
EPS = 2.0 ** -52
GAP_FLOOR = 2.0 ** -20
# c of the eigenvector bound c * 2^-52 * |C|_F / (lambda_1 - lambda_0): MEASURED_C is the worst ratio of the restatement's normal
# against the 50-digit solve over the ROWS OF FIXTURES THAT GO TO MPMATH — every `step`-th row of each fixture, a subsample of about 2100 rows, not every row —
# among those with a relative gap of 2^-20 or more (test_normals_against_eigh_and_mpmath
# prints it); C_BOUND is 4 times that, rounded up: the fixtures are a sample, not a proof.
MEASURED_C = 1.116
C_BOUND = 4.5
# (cloud, knn, radius, rows that are checked against mpmath: every `step`-th)
FIXTURES = [("base", 30, None, 6), ("base", 200, None, 12), ("hybrid", 30, 0.3, 4), ("n257", 40, None, 1), ("far_point", 30, None, 4),
            ("with_nan", 30, None, 2), ("tilted", 30, None, 3)]
DEGENERATE = [("lattice", 30, None, 2), ("flat", 30, None, 3), ("line", 30, None, 2), ("collinear", 30, None, 1)]


@pytest.fixture(scope="module")
def tn():
    from dn_splatter_amd import torch_normals

    return torch_normals


def full(cov):
    c = np.asarray(cov)
    return np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], axis=1)


def test_neighbour_sets_equal_ckdtree_on_tie_free_clouds(tn):
    from scipy.spatial import cKDTree

    for name, knn in (("base", 30), ("base", 200), ("n257", 40), ("hybrid", 30)):
        points = inputs.cloud(name)
        nbr, count = inputs.expected(name, knn)[2:]
        _, want = cKDTree(points.double().numpy()).query(points.double().numpy(), k=knn)
        assert (count == knn).all()
        assert np.array_equal(nbr.numpy(), want.astype(np.int32)), name              # ascending distance, no ties: the same order too
    # the hybrid search: of the K nearest those strictly within the radius
    points = inputs.cloud("hybrid").double().numpy()
    nbr, count = inputs.expected("hybrid", inputs.HYBRID_KNN, inputs.HYBRID_RADIUS)[2:]
    d, want = cKDTree(points).query(points, k=inputs.HYBRID_KNN, distance_upper_bound=inputs.HYBRID_RADIUS)
    want = np.where(np.isfinite(d), want, -1).astype(np.int32)
    assert np.array_equal(nbr.numpy(), want) and np.array_equal(count.numpy(), (want >= 0).sum(axis=1))


def test_ties_go_to_the_lowest_index_on_the_lattice(tn):
    points = inputs.cloud("lattice").double()
    d2 = ((points[:, None, :] - points[None, :, :]) ** 2).sum(dim=2)                 # integers: exact
    for knn in (10, 30, 100):
        nbr, count = inputs.expected("lattice", knn)[2:]
        assert (count == knn).all()
        tied_rows = 0
        for i in range(points.shape[0]):
            row = nbr[i].long()
            got = d2[i, row]
            assert (got[1:] >= got[:-1]).all()
            kth = got[-1]
            group = (d2[i] == kth).nonzero().flatten()                                # the group the K-th place falls into
            inside = row[got == kth]
            assert (d2[i] < kth).sum() + len(inside) == knn
            assert torch.equal(inside, group[:len(inside)])                           # its lowest indices, ascending
            tied_rows += len(group) > len(inside)
            below = got[:-1] == got[1:]
            assert (row[1:][below] > row[:-1][below]).all()                           # equal d² ascend by index everywhere
        assert tied_rows > points.shape[0] // 2


def test_covariance_against_numpy_cov(tn):
    for name, knn, radius, _ in FIXTURES + DEGENERATE:
        points = inputs.cloud(name).double().numpy()
        _, cov, nbr, count = inputs.expected(name, knn, radius)
        cov, nbr, count = full(cov.numpy()), nbr.numpy(), count.numpy()
        for i in range(0, points.shape[0], 7):
            n = int(count[i])
            if n == 0:
                assert not cov[i].any()
                continue
            p = points[nbr[i, :n]]
            want = np.cov(p.T, bias=True).reshape(3, 3)
            d = p - p.mean(axis=0)
            terms = np.abs(d[:, :, None] * d[:, None, :]).sum(axis=0) / n             # the sum of |terms| of every entry of C
            assert (np.abs(cov[i] - want) <= n * EPS * terms).all(), (name, knn, i)


@functools.lru_cache(maxsize=None)
def mp_solve(key):
    """(eigenvalues ascending, unit eigenvector of the smallest) of a symmetric 3x3 given as a tuple of six floats, at 50 digits"""
    import mpmath as mp

    mp.mp.dps = 50
    c = [mp.mpf(v) for v in key]
    E, Q = mp.eigsy(mp.matrix([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]))
    order = sorted(range(3), key=lambda k: E[k])
    return [E[k] for k in order], [Q[r, order[0]] for r in range(3)]


def mp_angle_and_residual(cov_row, normal):
    """(the sine of the angle to the 50-digit eigenvector, |C n - lambda_0 n|, lambda_1 - lambda_0, |C|_F), as floats"""
    import mpmath as mp

    lam, v = mp_solve(tuple(float(x) for x in cov_row))
    n = [mp.mpf(float(x)) for x in normal]
    cross = [n[1] * v[2] - n[2] * v[1], n[2] * v[0] - n[0] * v[2], n[0] * v[1] - n[1] * v[0]]
    c = [mp.mpf(float(x)) for x in cov_row]
    M = [[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]
    res = [sum(M[r][k] * n[k] for k in range(3)) - lam[0] * n[r] for r in range(3)]
    fro = mp.sqrt(sum(M[r][k] ** 2 for r in range(3) for k in range(3)))
    return float(mp.sqrt(sum(x * x for x in cross))), float(mp.sqrt(sum(x * x for x in res))), float(lam[1] - lam[0]), float(fro)


def test_normals_against_eigh_and_mpmath(tn):
    """Measured over the rows of FIXTURES that go to mpmath — every ``step``-th row of each fixture, a SUBSAMPLE of its rows (the 50-digit
    solve costs milliseconds per row), of those the ones with a relative gap of at least 2^-20 —: the worst ratio of the sine of the
    angle between the restatement's normal and the 50-digit eigenvector to 2^-52 |C|_F / (lambda_1 - lambda_0) is 1.1159 (MEASURED_C = 1.116;
    this test prints the current value and asserts it has not grown past it); the bound uses c = C_BOUND = 4.5, 4 times that rounded
    up.  Rows below the gap are held by the residual |C n - lambda_0 n| <= C_BOUND 2^-52 |C|_F and are at most 1 % of a fixture that
    was not built to be degenerate."""
    worst = 0.0
    for name, knn, radius, step in FIXTURES + DEGENERATE:
        normals, cov, _, count = inputs.expected(name, knn, radius)
        normals, cov, count = normals.numpy(), cov.numpy(), count.numpy()
        assert np.abs(np.linalg.norm(normals, axis=1) - 1).max() <= 4 * EPS
        lam, vec = np.linalg.eigh(full(cov))
        fro = np.linalg.norm(full(cov), axis=(1, 2))
        solved = (count >= 3) & (fro > 0)
        assert (normals[~solved] == (0.0, 0.0, 1.0)).all()
        rel_gap = np.where(solved, (lam[:, 1] - lam[:, 0]) / np.where(fro > 0, fro, 1.0), np.inf)
        low = solved & (rel_gap < GAP_FLOOR)
        if (name, knn, radius, step) in FIXTURES:
            assert low.sum() <= 0.01 * len(count), (name, knn, int(low.sum()))
        # numpy's eigh on every row: its own error is of the same order, so the bound is doubled for this comparison
        ok = solved & ~low
        sine = np.linalg.norm(np.cross(normals[ok], vec[ok][:, :, 0]), axis=1)
        assert (sine <= 2 * C_BOUND * EPS * fro[ok] / (lam[ok, 1] - lam[ok, 0]) + 4 * EPS).all(), name
        for i in np.flatnonzero(solved)[::step]:
            sine, residual, gap, f = mp_angle_and_residual(cov[i], normals[i])
            if gap / f >= GAP_FLOOR:
                ratio = sine / (EPS * f / gap)
                if (name, knn, radius, step) in FIXTURES:
                    worst = max(worst, ratio)
                assert sine <= C_BOUND * EPS * f / gap, (name, knn, i, ratio)
            else:
                assert residual <= C_BOUND * EPS * f, (name, knn, i, residual / (EPS * f))
    print("worst ratio of the angle to 2^-52 |C|_F / gap over the fixtures:", worst)
    assert worst <= MEASURED_C


def test_a_tilted_plane_gives_its_normal(tn):
    """Points exactly on z = a x + b y: the covariance is the exact one up to its own rounding, n 2^-52 per entry relative to the sum of
    its terms (test_covariance_against_numpy_cov's bound, at most n 2^-52 |C|_F-ish per entry, 3 n 2^-52 |C|_F in the Frobenius norm),
    so the normal lies within (C_BOUND + 3 n) 2^-52 |C|_F / (lambda_1 - lambda_0) of (a, b, -1) / |.|, up to sign."""
    a, b, knn = 0.5, 0.25, 30
    normals, cov, _, _ = inputs.expected("tilted", knn)
    want = np.array([a, b, -1.0]) / np.linalg.norm([a, b, -1.0])
    lam = np.linalg.eigvalsh(full(cov.numpy()))
    fro = np.linalg.norm(full(cov.numpy()), axis=(1, 2))
    sine = np.linalg.norm(np.cross(normals.numpy(), want[None]), axis=1)
    bound = (C_BOUND + 3 * knn) * EPS * fro / (lam[:, 1] - lam[:, 0])
    assert ((lam[:, 1] - lam[:, 0]) / fro > 1e-3).all() and (sine <= bound + 4 * EPS).all(), (sine / bound).max()
    assert (normals[:, 2] > 0).all()                                                  # the canonical sign: z is the largest component


def test_a_sphere_gives_the_radial_direction_within_the_curvature_term(tn):
    """Unit sphere, no noise, 4000 points, 30 neighbours.  In the frame (t1, t2, r) at a point the patch's covariance is
    [[T, b], [b^T, w]]: r is an approximate eigenvector with residual |b|, so the eigenvector of the smallest eigenvalue lies within
    sin <= |b| / (lambda_1 - w) of it (the residual bound of the symmetric eigenproblem), lambda_1 the middle eigenvalue.  On a sphere
    the radial offset of a neighbour at angle t is 1 - cos t <= t^2 / 2 and its tangential offset at most t, so |b| <= theta^3 / 2 for a
    patch of angular radius theta while lambda_1 - w is of the order theta^2 / 8: the term is linear in the patch size."""
    points = inputs.shell(61, 4000, 0.0)
    normals, cov, nbr, _ = tn.estimate_normals(points, knn=30)
    p = points.double().numpy()
    radial = p / np.linalg.norm(p, axis=1, keepdims=True)
    C = full(cov.numpy())
    worst_ratio, worst_theta = 0.0, 0.0
    for i in range(0, p.shape[0], 5):
        r = radial[i]
        t1 = np.cross(r, [1.0, 0.0, 0.0] if abs(r[0]) < 0.9 else [0.0, 1.0, 0.0])
        t1 /= np.linalg.norm(t1)
        t2 = np.cross(r, t1)
        F = np.stack([t1, t2, r])
        M = F @ C[i] @ F.T
        bnorm, w = np.linalg.norm(M[:2, 2]), M[2, 2]
        lam1 = np.linalg.eigvalsh(C[i])[1]
        theta = np.arccos(np.clip(radial[nbr[i].long().numpy()] @ r, -1, 1)).max()
        assert bnorm <= theta ** 3 / 2 + 1e-12 and lam1 - w > 0
        bound = bnorm / (lam1 - w)
        sine = np.linalg.norm(np.cross(normals[i].numpy(), r))
        assert sine <= bound + 1e-12, (i, sine, bound)
        worst_ratio, worst_theta = max(worst_ratio, bound / theta), max(worst_theta, theta)
    print("sphere: widest patch", worst_theta, "rad; the curvature term is at most", worst_ratio, "times the patch size")
    assert worst_theta < 0.3 and worst_ratio < 8.0


def test_orientation_towards_a_camera(tn):
    centre = (0.3, -0.4, 6.0)
    normals = inputs.expected("tilted", 30, None, centre)[0]
    p = inputs.cloud("tilted").double()
    assert (((torch.tensor(centre, dtype=torch.float64) - p) * normals).sum(dim=1) > 0).all()
    other = inputs.expected("tilted", 30, None, (0.3, -0.4, -6.0))[0]
    assert torch.equal(other, -normals)
    # a dot product of exactly zero does not flip; the fallback is oriented like any other normal
    flat = inputs.expected("flat", 30, None, (0.5, 0.5, 0.0))[0]
    assert flat.tolist() == [[0.0, 0.0, 1.0]] * flat.shape[0]
    assert tn.orient(np.array([[0.0, 0.0, 1.0]]), np.zeros((1, 3)), (0.0, 0.0, -2.0)).tolist() == [[-0.0, -0.0, -1.0]]
    # without a camera: the component of largest magnitude is positive, the lowest axis on equal magnitudes
    got = tn.orient(np.array([[-0.6, 0.0, 0.8], [-0.8, 0.6, 0.0], [-0.5, 0.5, -0.5], [0.5, -0.5, -0.5], [0.0, -0.6, -0.8]]), None)
    assert got.tolist() == [[-0.6, 0.0, 0.8], [0.8, -0.6, -0.0], [0.5, -0.5, 0.5], [0.5, -0.5, -0.5], [-0.0, 0.6, 0.8]]


def test_fallbacks_and_clamps(tn):
    for name in ("n1", "n2"):
        normals, cov, nbr, count = inputs.expected(name, 30)
        N = inputs.cloud(name).shape[0]
        assert normals.tolist() == [[0.0, 0.0, 1.0]] * N and count.tolist() == [N] * N and tuple(nbr.shape) == (N, 30)
    normals, cov, _, count = inputs.expected("identical", 30)
    assert not cov.any() and normals.tolist() == [[0.0, 0.0, 1.0]] * 300 and (count == 30).all()
    normals, _, nbr, count = inputs.expected("with_nan", 30)
    bad = (~torch.isfinite(inputs.cloud("with_nan")).all(dim=1)).nonzero().flatten().tolist()
    for i in bad:
        assert count[i] == 0 and normals[i].tolist() == [0.0, 0.0, 1.0] and not (nbr == i).any()
    with pytest.raises(ValueError, match="knn must lie"):
        tn.estimate_normals(inputs.cloud("n4"), knn=2)
    with pytest.raises(ValueError, match="float32 values"):
        tn.estimate_normals(torch.tensor([[0.1, 0.2, 0.3]], dtype=torch.float64))


def test_golden_backproject_and_consistency_mask(tn):
    g = np.load(GOLDEN)
    fx, fy, cx, cy = (float(v) for v in g["intrinsics"])
    H, W = int(g["height"]), int(g["width"])
    world = tn.backproject(torch.from_numpy(g["depth"]), fx, fy, cx, cy, g["c2w"])
    assert world.dtype == torch.float64 and tuple(world.shape) == (H * W, 3)
    assert np.array_equal(world.float().numpy(), g["means3d"].astype(np.float32))     # the cloud the kernel is given
    assert np.abs(world.numpy() - g["means3d"]).max() <= 4 * EPS * np.abs(g["means3d"]).max()
    assert tn.camera_points(torch.from_numpy(g["depth"]), fx, fy, cx, cy).dtype == torch.float32
    mono = torch.from_numpy(g["mono_image"].astype(np.float64) / 255.0)
    degrees = tn.consistency_angles(torch.from_numpy(g["normals"]), mono, g["c2w"])
    assert np.abs(degrees.numpy() - g["degrees"]).max() <= 1e-10
    mask = tn.normal_consistency_mask(torch.from_numpy(g["normals"]), mono, g["c2w"])
    assert mask.dtype == torch.bool and np.array_equal(mask.numpy(), g["mask"]) and 0 < int(mask.sum()) < mask.numel()
    assert np.array_equal(tn.normal_consistency_mask(torch.from_numpy(g["normals"]), mono, g["c2w"][:3]).numpy(), g["mask"])   # a 3x4 pose
    # depth_normals leaves the pixels without depth out (the deliberate deviation) and turns the rest to the camera
    normals, valid = tn.depth_normals(torch.from_numpy(g["depth"]), fx, fy, cx, cy, g["c2w"], knn=30)
    assert np.array_equal(valid.numpy(), g["depth"] > 0) and not normals[~valid].any()
    centre = torch.from_numpy(g["c2w"][:3, 3].copy())
    assert (((centre - world.reshape(H, W, 3)[valid]) * normals[valid]).sum(dim=1) > 0).all()
