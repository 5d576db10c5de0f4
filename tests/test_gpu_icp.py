"""The mesh-alignment kernels (csrc/icp.hip) held to the float64 restatement (dn_splatter_amd/torch_icp.py, itself held to scipy, numpy
and mpmath in tests/test_icp_reference.py): one pass with the transform fed in, at every size at which the launch or the fold takes
another path; the whole loop; its edges; the transform of points; and ``culled_mesh_metrics(align=True)``."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _geometry_inputs as geometry_inputs
import _icp_inputs as inputs
import _mesh_cull_inputs as cull_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -52
BASE_ROWS = 3000
TARGETS = (600, 4000)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def icp():
    from dn_splatter_amd import icp as module

    return module


@pytest.fixture(scope="module")
def ti():
    from dn_splatter_amd import torch_icp

    return torch_icp


def _rows(M):
    """The source of M rows: a prefix of the base, or the base over and over (66 000 rows of a 3000-row restatement)."""
    return np.arange(M) % BASE_ROWS


@pytest.fixture(scope="module")
def base(ti):
    """(target size, transform) -> the restatement's pass over the 3000 base rows, computed once and left unchanged; the first 40 rows
    lie 3 units outside the box."""
    out = {}
    for n in TARGETS:
        src, tgt, T0, _ = inputs.fixture(n, BASE_ROWS, far=40)
        c = ti.centre(_t(tgt)).numpy()
        for label, T in (("identity", np.eye(4)), ("perturbed", inputs.perturbed(T0))):
            q, idx, d2 = ti.correspondences(_t(src), _t(tgt), T, inputs.R_MAX)
            out[(n, label)] = dict(src=src, tgt=tgt, T=T, c=c, q=q.numpy(), idx=idx.numpy(), d2=d2.numpy())
    return out


@pytest.fixture(scope="module")
def indices():
    """One KnnIndex per target, shared by every test of this module: a caller's index reused across calls."""
    from dn_splatter_amd.density import KnnIndex

    out = {}
    for n in TARGETS:
        tgt = dev(inputs.fixture(n, 1)[1])
        out[n] = (tgt, KnnIndex(tgt))
    return out


def _sums_of(b, rows):
    """The restatement's sums over ``rows`` of a base pass, in torch_icp.moments' shape, and the exactly rounded sums (math.fsum)."""
    q, idx, d2 = _t(b["q"][rows]), _t(b["idx"][rows]), _t(b["d2"][rows])
    from dn_splatter_amd import torch_icp

    sums = torch_icp.moments(q, _t(b["tgt"]), idx, d2, _t(b["c"]))
    corr = b["idx"][rows] >= 0
    qc = b["q"][rows][corr].astype(np.float64) - b["c"]
    gc = b["tgt"][b["idx"][rows][corr]].astype(np.float64) - b["c"]
    exact = {"d2": math.fsum(b["d2"][rows][corr]), "q": np.array([math.fsum(qc[:, k]) for k in range(3)]),
             "g": np.array([math.fsum(gc[:, k]) for k in range(3)]),
             "gq": np.array([[math.fsum(gc[:, a] * qc[:, k]) for k in range(3)] for a in range(3)])}
    return sums, exact


def _translation_allowance(bound, sums, t_before):
    """What the translation of T' = U T may differ by when the rotation of U is within ``bound`` (the polar bound) and the sums are within
    their fold bounds: t' = R t_before + (mu_g - R mu_q), so |dt'| <= |dR| (|mu_q| + |t_before|) + |d mu_g| + |d mu_q| — the reach of
    the rotation's error, and the fold bounds of the two means.  Nothing else is added."""
    n = float(sums["n"])
    bounds = inputs.fold_bounds(sums)
    reach = float(np.linalg.norm(np.asarray(sums["q"]) / n + np.asarray(sums["c"]))) + float(np.linalg.norm(t_before))
    return bound * reach + float(np.linalg.norm(bounds["q"]) + np.linalg.norm(bounds["g"])) / n


def _one_pass(icp, src, tgt, index, T, r=inputs.R_MAX, max_iteration=30):
    from dn_splatter_amd import _lib
    from dn_splatter_amd._ops import _icp_args, _stream

    L = _lib.lib()
    M = src.shape[0]
    state = torch.full((icp.STATE_WORDS,), float("nan"), dtype=torch.float64, device=DEV)
    trace = torch.zeros(max_iteration + 1, 4, dtype=torch.float64, device=DEV)
    idx = torch.full((M,), -7, dtype=torch.int32, device=DEV)
    dist2 = torch.zeros(M, dtype=torch.float64, device=DEV)
    scratch = torch.zeros(L.dnsplat_icp_scratch_bytes(M) // 8, dtype=torch.float64, device=DEV)
    a = _icp_args(src, tgt, index.buffer, r, 1e-6, 1e-6, max_iteration, state, scratch, trace, idx, dist2)
    init = np.ascontiguousarray(T, dtype=np.float64)
    _lib.run("dnsplat_icp_begin", L.dnsplat_icp_begin, ctypes.byref(a), init.ctypes.data_as(ctypes.c_void_p), _stream())
    begun = state.cpu()
    _lib.run("dnsplat_icp_iterate", L.dnsplat_icp_iterate, ctypes.byref(a), _stream())
    return dict(begun=begun, state=state.cpu(), trace=trace.cpu().numpy(), idx=idx.cpu().numpy(), dist2=dist2.cpu().numpy(),
                partials=scratch.cpu().numpy().reshape(-1, 17))


@pytest.mark.parametrize("label", ["identity", "perturbed"])
@pytest.mark.parametrize("n", TARGETS)
@pytest.mark.parametrize("M", inputs.SIZES)
def test_one_pass_with_the_transform_fed_in(icp, ti, base, indices, M, n, label):
    b = base[(n, label)]
    rows = _rows(M)
    tgt, index = indices[n]
    got = _one_pass(icp, dev(b["src"][rows]), tgt, index, b["T"])
    begun = got["begun"]
    assert np.array_equal(begun[:16].numpy().reshape(4, 4), b["T"]) and not begun[16:].view(torch.int64).any()   # begin: T = init, the rest 0
    want_idx, want_d2 = b["idx"][rows], b["d2"][rows]
    corr = want_idx >= 0
    assert np.array_equal(got["idx"], want_idx)
    assert np.array_equal(got["dist2"][corr].view(np.int64), want_d2[corr].view(np.int64)) and np.isnan(got["dist2"][~corr]).all()
    words = got["state"].view(torch.int64)
    n_corr = int(corr.sum())
    assert int(words[icp.STATE_N]) == n_corr and int(words[icp.STATE_PASSES]) == 1
    parts = got["partials"]
    assert parts.shape[0] == (M + 255) // 256
    assert int(parts[:, 0].view(np.int64).sum()) == n_corr
    assert float(got["state"][icp.STATE_FITNESS]) == n_corr / M
    row = got["trace"][0]
    assert row[0] == n_corr and row[1] == n_corr / M and not got["trace"][1:].any()
    if n_corr == 0:                                                               # M = 1: the one row is a far one
        assert M == 1 and int(words[icp.STATE_STATUS]) == ti.STATUS_NO_CORRESPONDENCE and int(words[icp.STATE_DONE]) == 1
        assert float(got["state"][icp.STATE_RMSE]) == 0.0 and row[3] == 1.0 and int(words[icp.STATE_ITERATIONS]) == 0
        assert np.array_equal(got["state"][:16].numpy().reshape(4, 4), b["T"])
        return
    sums, exact = _sums_of(b, rows)
    bounds = inputs.fold_bounds(sums)
    folded = {"d2": math.fsum(parts[:, 1]), "q": np.array([math.fsum(parts[:, 2 + k]) for k in range(3)]),
              "g": np.array([math.fsum(parts[:, 5 + k]) for k in range(3)]),
              "gq": np.array([[math.fsum(parts[:, 8 + 3 * a + k]) for k in range(3)] for a in range(3)])}
    for k in ("d2", "q", "g", "gq"):                                              # the kernel's partials against the exactly rounded sums
        err = np.abs(folded[k] - exact[k])
        print(f"M={M} n={n} {label} sum {k}: worst error / fold bound {np.max(err / np.maximum(bounds[k], 1e-300)):.3e}")
        assert (err <= bounds[k]).all(), k
    want_rmse = math.sqrt(float(sums["d2"]) / n_corr)
    rmse = float(got["state"][icp.STATE_RMSE])
    print(f"M={M} n={n} {label} rmse: relative difference / 2^-52 = {abs(rmse - want_rmse) / want_rmse / EPS:.2f}")
    assert abs(rmse - want_rmse) <= 4 * EPS * want_rmse and row[2] == rmse and row[3] == 0.0
    assert int(words[icp.STATE_DONE]) == 0 and int(words[icp.STATE_ITERATIONS]) == 1
    U, degenerate = ti.solve(sums)
    assert int(words[icp.STATE_STATUS]) == (ti.STATUS_DEGENERATE if degenerate else 0) == 0
    want_T = ti.compose(U, b["T"])
    new_T = got["state"][:16].numpy().reshape(4, 4)
    assert np.array_equal(new_T[3], [0.0, 0.0, 0.0, 1.0])
    bound = inputs.polar_bound(sums)[0]
    assert np.isfinite(bound)
    err_R = float(np.linalg.norm(new_T[:3, :3] - want_T[:3, :3]))
    err_t = float(np.linalg.norm(new_T[:3, 3] - want_T[:3, 3]))
    allow_t = _translation_allowance(bound, sums, b["T"][:3, 3])
    print(f"M={M} n={n} {label} T: |dR|_F {err_R:.3e} of the polar bound {bound:.3e}; |dt| {err_t:.3e} of {allow_t:.3e}")
    assert err_R <= bound and err_t <= allow_t


@pytest.fixture(scope="module")
def loops(icp, ti):
    """name -> (the kernel's result, the restatement's, source, target, T0) of the two noise-free fixtures with 40 far rows."""
    out = {}
    for name, (n, m) in inputs.FIXTURES.items():
        src, tgt, T0, _ = inputs.fixture(n, m, far=40)
        want = ti.registration_icp(_t(src), _t(tgt), inputs.R_MAX)
        got = icp.registration_icp(dev(src), dev(tgt), inputs.R_MAX, return_trace=True)
        out[name] = (got, want, src, tgt, T0)
    return out


@pytest.mark.parametrize("name", sorted(inputs.FIXTURES))
def test_whole_loop(icp, ti, loops, name):
    from scipy.spatial import cKDTree

    got, want, src, tgt, T0 = loops[name]
    m = src.shape[0]
    # a T that differs in its last bits cannot flip a pair: in the restatement's last pass every row's best and second-best target are
    # at least 1e-6 apart, and no row is within 1e-6 of the threshold
    d, _ = cKDTree(tgt.astype(np.float64)).query(want["last"]["q"].numpy().astype(np.float64), k=2)
    assert (d[:, 1] - d[:, 0] >= 1e-6).all() and (np.abs(d[:, 0] - inputs.R_MAX) >= 1e-6).all()
    assert got.status == 0 and want["status"] == 0 and got.done
    assert got.iterations == want["iterations"] and got.passes == len(want["trace"]) and 3 <= got.iterations <= 5
    trace = got.trace.cpu().numpy()
    assert [int(v) for v in trace[:got.passes, 0]] == [row[0] for row in want["trace"]]
    assert [v for v in trace[:got.passes, 3]] == [row[3] for row in want["trace"]] and not trace[got.passes:].any()
    assert got.n == m - 40 and got.fitness == (m - 40) / m and got.inlier_rmse < 1e-6
    assert np.array_equal(got.idx.cpu().numpy(), want["last"]["idx"].numpy())
    pairs = got.correspondence_set.cpu().numpy()
    assert pairs.shape == (m - 40, 2) and np.array_equal(pairs[:, 0], np.arange(40, m)) and np.array_equal(pairs[:, 1], got.idx.cpu().numpy()[40:])
    T = got.transformation.cpu().numpy()
    assert got.transformation.is_cuda and got.transformation.dtype == torch.float64
    assert np.abs(T - T0).max() <= 2.0 ** -24 * (1 + np.abs(tgt).max())
    sums = want["last"]["sums"]                                                   # the last pass's pairs are the last solve's pairs
    bound = inputs.polar_bound(sums)[0]
    err_R = float(np.linalg.norm(T[:3, :3] - want["transformation"][:3, :3]))
    err_t = float(np.linalg.norm(T[:3, 3] - want["transformation"][:3, 3]))
    allow_t = _translation_allowance(2 * bound, sums, want["transformation"][:3, 3])
    print(f"{name}: |dR|_F {err_R:.3e}, twice the polar bound {2 * bound:.3e}; |dt| {err_t:.3e} of {allow_t:.3e}; max |T - T0| {np.abs(T - T0).max():.3e}")
    assert err_R <= 2 * bound and err_t <= allow_t


def test_edges(icp, ti, indices):
    # the threshold is inclusive
    src, tgt, r = inputs.threshold_edge()
    got = icp.registration_icp(dev(src), dev(tgt), r, max_iteration=0)
    assert got.idx.tolist() == [0, -1] and got.n == 1 and got.fitness == 0.5 and got.inlier_rmse == 0.5
    assert got.dist2.cpu().numpy()[0] == 0.25 and math.isnan(got.dist2.cpu().numpy()[1])
    # the mirrored set: a reflection would fit; the result is a proper rotation, the restatement's
    src, tgt = inputs.mirrored()
    got = icp.registration_icp(dev(src), dev(tgt), 0.3, return_trace=True)
    want = ti.registration_icp(_t(src), _t(tgt), 0.3)
    T = got.transformation.cpu().numpy()
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) <= 16 * EPS and np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() <= 16 * EPS
    assert got.iterations == want["iterations"] and got.status == want["status"] == 0 and got.n == 8
    first = ti.step(_t(src), _t(tgt), np.eye(4), 0.3)
    assert np.linalg.det(ti.sigma_of(first["sums"])) < 0
    bound = inputs.polar_bound(want["last"]["sums"])[0]                          # the pairs of the last solve, as in the whole loop
    assert np.linalg.norm(T[:3, :3] - want["transformation"][:3, :3]) <= bound
    assert np.linalg.norm(T[:3, 3] - want["transformation"][:3, 3]) <= _translation_allowance(bound, want["last"]["sums"], want["transformation"][:3, 3])
    # one pair: a zero covariance, R = I exactly, a pure translation, the rotation flagged as not determined.  With one term per sum
    # nothing depends on an order, so the kernel's T is the restatement's bit for bit
    src, tgt = inputs.single_pair()
    got = icp.registration_icp(dev(src), dev(tgt), 0.3, return_trace=True)
    want = ti.registration_icp(_t(src), _t(tgt), 0.3)
    assert got.n == 1 and got.status == want["status"] == icp.STATUS_DEGENERATE and got.iterations == want["iterations"] >= 1
    T = got.transformation.cpu().numpy()
    assert np.array_equal(T[:3, :3], np.eye(3)) and np.array_equal(T, want["transformation"])
    assert np.abs(src[0].astype(np.float64) + T[:3, 3] - tgt[0]).max() <= 2.0 ** -24 * 4 and got.idx.tolist() == [0]
    # max_iteration = 0: one pass, T = init, one row of trace
    src, tgt, T0, _ = inputs.fixture(600, 257)
    tgt_d, index = indices[600]
    init = inputs.perturbed(T0)
    got = icp.registration_icp(dev(src), index, inputs.R_MAX, init=init, max_iteration=0, return_trace=True)
    want = ti.step(_t(src), _t(tgt), init, inputs.R_MAX)
    assert got.iterations == 0 and got.passes == 1 and got.done and tuple(got.trace.shape) == (1, 4)
    assert np.array_equal(got.transformation.cpu().numpy(), init) and got.n == want["n"] and got.fitness == want["fitness"]
    assert np.array_equal(got.idx.cpu().numpy(), want["idx"].numpy())
    # a source wholly beyond r
    far = src.copy()
    far[:, 2] += np.float32(50.0)
    got = icp.registration_icp(dev(far), tgt_d, inputs.R_MAX, init=init, index=index)
    assert got.status == icp.STATUS_NO_CORRESPONDENCE and got.fitness == 0.0 and got.inlier_rmse == 0.0 and got.n == 0 and got.iterations == 0
    assert np.array_equal(got.transformation.cpu().numpy(), init) and bool((got.idx == -1).all()) and got.correspondence_set.shape == (0, 2)
    # nan / inf rows count in M and never in n
    bad = src.copy()
    bad[3, 1], bad[7, 0], bad[9, 2] = np.nan, np.inf, -np.inf
    got = icp.registration_icp(dev(bad), index, inputs.R_MAX, init=T0, max_iteration=0)
    want = ti.step(_t(bad), _t(tgt), T0, inputs.R_MAX)
    clean = ti.step(_t(src), _t(tgt), T0, inputs.R_MAX)
    assert got.n == want["n"] == clean["n"] - 3 and got.fitness == got.n / 257 and got.idx[[3, 7, 9]].tolist() == [-1, -1, -1]
    assert np.array_equal(got.idx.cpu().numpy(), want["idx"].numpy())
    # the index gives back the points it was built over
    assert torch.equal(index.points(), tgt_d)


def test_two_calls_give_equal_bytes(icp, indices):
    src, tgt, T0, _ = inputs.fixture(4000, 3000, far=40)
    tgt_d, index = indices[4000]
    a = icp.registration_icp(dev(src), index, inputs.R_MAX, return_trace=True)
    b = icp.registration_icp(dev(src), tgt_d, inputs.R_MAX, index=index, return_trace=True)
    c = icp.registration_icp(dev(src), tgt_d, inputs.R_MAX, return_trace=True)   # an index of its own
    for other in (b, c):
        assert torch.equal(a.state.view(torch.int64), other.state.view(torch.int64))
        assert torch.equal(a.trace.view(torch.int64), other.trace.view(torch.int64))
        assert torch.equal(a.idx, other.idx)
        assert torch.equal(a.dist2.view(torch.int64), other.dist2.view(torch.int64))


@pytest.mark.parametrize("N", [1, 255, 257, 66_000])
def test_transform_points_states_its_order(icp, N):
    rng = np.random.default_rng(N)
    p = (rng.standard_normal((N, 3)) * 5).astype(np.float32)
    T = inputs.pose(2.5, 0.04)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    want = np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=-1).astype(np.float32)
    assert np.array_equal(icp.transform_points(dev(p), T).cpu().numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(icp.transform_points(dev(p), dev(T)).cpu().numpy().view(np.int32), want.view(np.int32))   # T read on the device
    want = np.stack([(T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z for a in range(3)], axis=-1).astype(np.float32)
    assert np.array_equal(icp.transform_points(dev(p), T, rotate_only=True).cpu().numpy().view(np.int32), want.view(np.int32))
    mesh = (dev(p), torch.arange(3, device=DEV, dtype=torch.int32)[None], dev(p), dev(p))
    moved = icp.transform_mesh(mesh, T, normals_at=3)
    assert moved[1] is mesh[1] and moved[2] is mesh[2]                            # triangles and colours pass through
    assert np.array_equal(moved[3].cpu().numpy().view(np.int32), want.view(np.int32))


def test_culled_mesh_metrics_aligns_before_it_culls(icp):
    from dn_splatter_amd import geometry, mesh_cull

    v, t = geometry_inputs.grid_mesh()
    T0 = inputs.pose(1.5, 0.02)
    moved = ((v.astype(np.float64) - T0[:3, 3]) @ T0[:3, :3]).astype(np.float32)  # the rigid copy: T0 takes it back onto the mesh
    target, pred = (dev(v), dev(t)), (dev(moved), dev(t))
    H, W = 48, 64
    K = np.array([[0.625 * W, 0.0, 0.5 * W], [0.0, 0.625 * W, 0.5 * H], [0.0, 0.0, 1.0]])
    poses = np.stack([cull_inputs.look_at(e, (1.0, 0.5, 0.0)) for e in [(1.0, 0.5, 3.0), (0.6, 0.3, 2.8), (1.4, 0.7, 3.1), (1.1, 0.2, 2.9), (0.8, 0.8, 3.2)]])
    args, kw = (poses, K, H, W), dict(count=(2000, 2000), seed=4)
    T = icp.get_align_transformation(pred, target)
    assert np.abs(T.cpu().numpy() - T0).max() <= 2.0 ** -24 * (1 + np.abs(v).max())
    by_hand = (icp.transform_points(pred[0], T), pred[1])
    want = mesh_cull.culled_mesh_metrics(by_hand, target, *args, **kw)
    got = mesh_cull.culled_mesh_metrics(pred, target, *args, align=True, **kw)
    plain = mesh_cull.culled_mesh_metrics(pred, target, *args, **kw)
    old = geometry.mesh_metrics(mesh_cull.cull_mesh(pred, *args), mesh_cull.cull_mesh(target, *args), **kw)
    assert sorted(got) == sorted(want) == sorted(plain) and len(got) == 8
    for k in want:
        assert torch.equal(got[k], want[k]) and bool(torch.isfinite(got[k])), k
        assert torch.equal(plain[k].view(torch.int64), old[k].view(torch.int64)), k                # align=False: byte for byte what it was
    assert float(got["Acc"]) < float(plain["Acc"])
