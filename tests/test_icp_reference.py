"""The float64 restatement of the mesh alignment (dn_splatter_amd/torch_icp.py) held to what it restates, on the CPU: one pass against
scipy's cKDTree and plain numpy sums, the Jacobi solve against numpy's SVD and against the same solve in mpmath at 50 digits, the
properties of a rotation on every fixture, and the loop against the pose the fixtures were made with.  The kernels are held to this
restatement in tests/test_gpu_icp.py."""
import math

import numpy as np
import pytest
import torch

import _icp_inputs as inputs

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def ti():
    from dn_splatter_amd import torch_icp

    return torch_icp


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.fixture(scope="module")
def passes(ti):
    """name -> (src, tgt, T, r, step): one pass of the restatement on every fixture, computed once and left unchanged."""
    out = {}
    for name, (n, m) in inputs.FIXTURES.items():
        src, tgt, T0, _ = inputs.fixture(n, m, far=40)
        for label, T in (("identity", np.eye(4)), ("perturbed", inputs.perturbed(T0))):
            out[f"{name}-{label}"] = (src, tgt, T, inputs.R_MAX, ti.step(_t(src), _t(tgt), T, inputs.R_MAX))
    for name, make, r in (("mirrored", inputs.mirrored, 0.3), ("planar", inputs.planar, 0.3), ("single", inputs.single_pair, 0.3)):
        src, tgt = make()
        out[name] = (src, tgt, np.eye(4), r, ti.step(_t(src), _t(tgt), np.eye(4), r))
    return out


def test_step_finds_scipys_correspondences_and_numpys_sums(ti, passes):
    from scipy.spatial import cKDTree

    for name, (src, tgt, T, r, s) in passes.items():
        q = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        got_q = s["q"].numpy()
        assert (np.abs(got_q.astype(np.float64) - q) <= np.spacing(np.abs(q))).all(), name     # matmul's order may round the last bit otherwise
        q64 = got_q.astype(np.float64)
        d, j = cKDTree(tgt.astype(np.float64)).query(q64)
        corr = d * d <= r * r
        margin = np.abs(d - r) < 1e-9                                             # a row at the threshold could go either way: none here
        assert not margin.any(), name
        idx = s["idx"].numpy()
        assert np.array_equal(idx >= 0, corr), name
        assert np.array_equal(idx[corr], j[corr]), name
        assert s["n"] == int(corr.sum()) and 0 < s["n"] <= src.shape[0]
        c = ((tgt.min(axis=0).astype(np.float64) + tgt.max(axis=0).astype(np.float64)) * 0.5)
        assert np.array_equal(np.asarray(s["sums"]["c"]), c), name
        qc, gc = q64[corr] - c, tgt[j[corr]].astype(np.float64) - c
        # d² is the fused one of the definition: the restatement's own dist2, held per row to numpy's plain sum of squares (three roundings)
        dd = s["dist2"].numpy()[corr]
        plain = ((qc - gc) ** 2).sum(axis=-1)
        assert (np.abs(dd - plain) <= 4 * 2.0 ** -53 * plain).all() and np.isnan(s["dist2"].numpy()[~corr]).all(), name
        # every sum against the exactly rounded sum of its terms (math.fsum), at ONE fold bound n 2^-53 sum|term|
        exact = {"d2": math.fsum(dd), "q": np.array([math.fsum(qc[:, k]) for k in range(3)]), "g": np.array([math.fsum(gc[:, k]) for k in range(3)]),
                 "gq": np.array([[math.fsum(gc[:, a] * qc[:, k]) for k in range(3)] for a in range(3)])}
        bounds = inputs.fold_bounds(s["sums"])
        for k in ("d2", "q", "g", "gq"):
            assert (np.abs(np.asarray(s["sums"][k]) - exact[k]) <= bounds[k]).all(), (name, k)
        assert s["fitness"] == s["n"] / src.shape[0]
        assert abs(s["rmse"] - math.sqrt(exact["d2"] / s["n"])) <= (s["n"] * 2.0 ** -53 + 2 * EPS) * s["rmse"], name   # the fold bound, halved by the root


def _mp_solve(sums):
    """R of the same sums in mpmath at 50 digits: Sigma formed exactly from the double sums, svd_r, Umeyama's sign."""
    import mpmath as mp

    mp.mp.dps = 50
    n = mp.mpf(int(sums["n"]))
    Sq = [mp.mpf(float(v)) for v in sums["q"]]
    Sg = [mp.mpf(float(v)) for v in sums["g"]]
    S = mp.matrix(3, 3)
    for a in range(3):
        for b in range(3):
            S[a, b] = mp.mpf(float(sums["gq"][a][b])) / n - (Sg[a] / n) * (Sq[b] / n)
    U, D, V = mp.svd_r(S)
    s = -1 if mp.det(U) * mp.det(V) < 0 else 1
    R = U * mp.diag([1, 1, s]) * V
    return np.array([[float(R[a, b]) for b in range(3)] for a in range(3)])


def test_solve_meets_the_polar_bound_against_mpmath_and_svd(ti, passes, capsys):
    worst = {"solve": 0.0, "solve_svd": 0.0}
    for name, (src, tgt, T, r, s) in passes.items():
        bound, e_sigma, norm, gap = inputs.polar_bound(s["sums"])
        if not np.isfinite(bound):
            assert name == "single"                                               # a zero covariance determines no rotation
            continue
        want = _mp_solve(s["sums"])
        for label, fn in (("solve", ti.solve), ("solve_svd", ti.solve_svd)):
            U, degenerate = fn(s["sums"])
            err = float(np.linalg.norm(U[:3, :3] - want))
            worst[label] = max(worst[label], err / bound)
            assert err <= bound, (name, label, err, bound)
            assert not degenerate, (name, label)
        U, V = ti.solve(s["sums"])[0], ti.solve_svd(s["sums"])[0]
        m = np.abs(np.asarray(s["sums"]["c"])).max() + np.abs(tgt).max()
        # t = mu_g - R mu_q: each R is within the bound of the exact one, so the two differ by at most twice the bound times |mu_q| <= m,
        # beside the roundings of the four-term expression itself
        assert np.abs(U[:3, 3] - V[:3, 3]).max() <= 2 * bound * m + 16 * EPS * m, name
    with capsys.disabled():
        print(f"\nicp solve: worst |dR|_F / polar bound: Jacobi {worst['solve']:.3e}, numpy svd {worst['solve_svd']:.3e}")
    assert worst["solve"] <= 1.0


def test_the_kernels_solve_text_equals_the_restatement_bit_for_bit(ti, passes, tmp_path):
    """csrc/icp_solve.h is what icp_solve_kernel compiles; g++ reads the same text (tools/icp_solve_host_check.cpp)."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "icp_solve_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(root, "tools", "icp_solve_host_check.cpp"),
                    "-o", str(exe)], check=True)
    for name, (src, tgt, T, r, s) in passes.items():
        sums = s["sums"]
        values = [float(sums["d2"])] + [float(v) for v in sums["q"]] + [float(v) for v in sums["g"]] + [float(v) for v in sums["gq"].reshape(-1)]
        text = " ".join([str(sums["n"])] + [v.hex() for v in values] + [float(v).hex() for v in sums["c"]])
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split()
        got = np.array([float.fromhex(v) for v in out[:12]])
        U, degenerate = ti.solve(sums)
        assert np.array_equal(got[:9].reshape(3, 3), U[:3, :3]) and np.array_equal(got[9:], U[:3, 3]) and int(out[12]) == int(degenerate), name


def test_solve_returns_a_proper_rotation_on_every_fixture(ti, passes):
    for name, (src, tgt, T, r, s) in passes.items():
        U, degenerate = ti.solve(s["sums"])
        R = U[:3, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() <= 16 * EPS, name
        assert abs(np.linalg.det(R) - 1.0) <= 16 * EPS, name
        assert np.array_equal(U[3], [0.0, 0.0, 0.0, 1.0])
        moved = s["q"].numpy().astype(np.float64)[s["idx"].numpy() >= 0] @ R.T + U[:3, 3]
        g = tgt.astype(np.float64)[s["idx"].numpy()[s["idx"].numpy() >= 0]]
        before = ((s["q"].numpy().astype(np.float64)[s["idx"].numpy() >= 0] - g) ** 2).sum()
        assert ((moved - g) ** 2).sum() <= before * (1 + 1e-12) + 1e-24, name      # the least-squares update does not raise the residual
    # the mirrored set: a reflection would fit exactly; the proper rotation is (nearly) the identity and leaves the residual
    src, tgt, T, r, s = passes["mirrored"]
    assert np.linalg.det(ti.sigma_of(s["sums"])) < 0
    U = ti.solve(s["sums"])[0]
    assert np.abs(U[:3, :3] - np.eye(3)).max() < 0.02 and np.linalg.det(U[:3, :3]) > 0.999
    # one pair: a zero covariance, R = I and a pure translation onto the target; the rotation is flagged as not determined
    src, tgt, T, r, s = passes["single"]
    U, degenerate = ti.solve(s["sums"])
    assert s["n"] == 1 and degenerate and np.array_equal(U[:3, :3], np.eye(3))
    assert np.abs(src[0].astype(np.float64) + U[:3, 3] - tgt[0]).max() <= 8 * EPS * 40
    # a planar set: rank 2, still determined
    src, tgt, T, r, s = passes["planar"]
    assert np.linalg.svd(ti.sigma_of(s["sums"]), compute_uv=False)[2] <= 1e-12 and not ti.solve(s["sums"])[1]


def test_transform_points_states_its_order(ti):
    rng = np.random.default_rng(3)
    p = rng.standard_normal((50, 3)).astype(np.float32) * 5
    T = inputs.pose(2.5, 0.04)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    want = np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=-1).astype(np.float32)
    assert np.array_equal(ti.transform_points(_t(p), T).numpy(), want)
    want = np.stack([(T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z for a in range(3)], axis=-1).astype(np.float32)
    assert np.array_equal(ti.transform_points(_t(p), T, rotate_only=True).numpy(), want)


@pytest.mark.parametrize("name", sorted(inputs.FIXTURES))
def test_loop_recovers_the_pose(ti, name):
    n, m = inputs.FIXTURES[name]
    src, tgt, T0, _ = inputs.fixture(n, m)
    got = ti.registration_icp(_t(src), _t(tgt), inputs.R_MAX)
    assert got["status"] == 0 and 3 <= got["iterations"] <= 5                     # stopped by the relative criteria, far from 30
    assert got["trace"][-1][3] == 1.0 and all(row[3] == 0.0 for row in got["trace"][:-1])
    assert got["trace"][-1][0] == m and got["trace"][0][0] < m                    # wrong and missing pairs on the way; all of them at the end
    assert got["fitness"] == 1.0 and got["inlier_rmse"] < 1e-6
    # every source coordinate and every query is rounded to fp32 once; the least-squares fit averages those roundings
    assert np.abs(got["transformation"] - T0).max() <= 2.0 ** -24 * (1 + np.abs(tgt).max())
    svd = ti.registration_icp(_t(src), _t(tgt), inputs.R_MAX, solver=ti.solve_svd)
    assert svd["iterations"] == got["iterations"] and [row[0] for row in svd["trace"]] == [row[0] for row in got["trace"]]
    assert np.abs(svd["transformation"] - got["transformation"]).max() <= 1e-12


def test_loop_edges(ti):
    src, tgt, r = inputs.threshold_edge()
    s = ti.step(_t(src), _t(tgt), np.eye(4), r)
    assert s["idx"].tolist() == [0, -1] and s["n"] == 1 and s["fitness"] == 0.5   # d² = 0.25 <= r r, inclusive; the next fp32 is beyond
    src, tgt, T0, _ = inputs.fixture(600, 257)
    init = inputs.perturbed(T0)
    got = ti.registration_icp(_t(src), _t(tgt), inputs.R_MAX, init=init, max_iteration=0)
    assert got["iterations"] == 0 and len(got["trace"]) == 1 and np.array_equal(got["transformation"], init)
    far = src.copy()
    far[:, 2] += np.float32(50.0)
    got = ti.registration_icp(_t(far), _t(tgt), inputs.R_MAX, init=init)
    assert got["status"] == ti.STATUS_NO_CORRESPONDENCE and got["fitness"] == 0.0 and got["inlier_rmse"] == 0.0
    assert np.array_equal(got["transformation"], init) and got["iterations"] == 0
    bad = src.copy()
    bad[3, 1], bad[7, 0], bad[9, 2] = np.nan, np.inf, -np.inf
    s = ti.step(_t(bad), _t(tgt), T0, inputs.R_MAX)
    clean = ti.step(_t(src), _t(tgt), T0, inputs.R_MAX)
    assert s["n"] == clean["n"] - 3 and s["fitness"] == (clean["n"] - 3) / 257 and (s["idx"][[3, 7, 9]] == -1).all()
