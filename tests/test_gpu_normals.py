"""csrc/normals.hip against its restatement (dn_splatter_amd/torch_normals.py), which test_normals_reference.py holds to scipy, numpy and
a 50-digit solve.

Everything is compared EXACTLY: ``neighbors`` and ``count`` by integer equality, ``covariance`` and ``normals`` by ``torch.equal`` —
the restatement ranks by the kernel's fused d², adds the moments by the kernel's fixed tree and runs the very sweeps of
csrc/normals_solve.h, all IEEE operations in one order.

The sizes are the smallest at which a part of the kernel can go wrong (tests/_normals_inputs.py)."""
import ctypes

import numpy as np
import pytest
import torch

import _normals_inputs as inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777


@pytest.fixture(scope="module")
def nm():
    from dn_splatter_amd import normals

    return normals


@pytest.fixture(scope="module")
def tn():
    from dn_splatter_amd import torch_normals

    return torch_normals


def run(nm, name, knn, radius=None, orient_toward=None):
    """(normals, covariance, neighbors, count, search) of the one launch; search is the scratch's two maxima"""
    points = inputs.cloud(name).to(DEV)
    knn, radius = nm.check_arguments(knn, radius)
    normals, cov, nbr, count, status, search = nm._launch(points, knn, radius, nm._toward(orient_toward), None, True, True)
    assert int(status) == 0
    return normals, cov, nbr, count, search


def check(nm, name, knn, radius=None, orient_toward=None):
    """One call against the restatement, everything exact; returns the device's (normals, covariance, neighbors, count, search) on the CPU."""
    got = [t.cpu() for t in run(nm, name, knn, radius, orient_toward)]
    normals, cov, nbr, count, search = got
    want_normals, want_cov, want_nbr, want_count = inputs.expected(name, knn, radius, orient_toward)
    N = inputs.cloud(name).shape[0]
    assert normals.dtype == torch.float64 and tuple(normals.shape) == (N, 3)
    assert cov.dtype == torch.float64 and tuple(cov.shape) == (N, 6)
    assert nbr.dtype == torch.int32 and tuple(nbr.shape) == (N, knn) and count.dtype == torch.int32
    assert torch.equal(count, want_count), (name, knn, (count != want_count).nonzero().flatten()[:8])
    assert torch.equal(nbr, want_nbr), (name, knn, (nbr != want_nbr).any(dim=1).nonzero().flatten()[:8])
    assert torch.equal(cov, want_cov), (name, knn, (cov - want_cov).abs().max())
    assert torch.equal(normals, want_normals), (name, knn, (normals - want_normals).abs().max())
    return got


@pytest.mark.parametrize("name", ["n1", "n2", "n3", "n4", "collinear", "identical"])
def test_the_smallest_clouds_and_the_fallback(nm, name):
    normals, cov, nbr, count, _ = check(nm, name, 30)
    N = inputs.cloud(name).shape[0]
    assert count.tolist() == [min(30, N)] * N                                     # N < knn clamps
    if N < 3:
        assert normals.tolist() == [[0.0, 0.0, 1.0]] * N
    if name == "identical":
        assert not cov.any() and normals.tolist() == [[0.0, 0.0, 1.0]] * N       # a zero covariance
        assert nbr[:, :30].tolist() == [list(range(30))] * N                      # 300 equal d²: the lowest indices
    if name == "collinear":
        assert torch.isfinite(normals).all()
        line = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
        assert (normals @ line).abs().max() < 1e-14                               # perpendicular to the line


@pytest.mark.parametrize("knn", inputs.BASE_KNN)
def test_every_buffer_size_on_one_cloud(nm, knn):
    _, _, nbr, count, search = check(nm, "base", knn)
    assert count.tolist() == [knn] * nbr.shape[0] and int(nbr.min()) >= 0
    assert int(search[1]) >= 1


@pytest.mark.parametrize("name,knn", [("n40", 40), ("n41", 40), ("n257", 40), ("n257", 256)])
def test_cloud_sizes_at_knn_and_past_a_workgroup(nm, name, knn):
    check(nm, name, knn)


@pytest.mark.parametrize("knn", inputs.CLUSTER_KNN)
@pytest.mark.parametrize("kind", ["exact", "once", "often"])
def test_candidates_fill_and_overflow_the_buffer(nm, knn, kind):
    _, selections, most = inputs.cluster_case(knn, kind)                          # asserted there: 0, 1, at least 3 inside ring 0
    search = check(nm, ("cluster", knn, kind), knn)[4]
    assert most >= selections + 1                                                 # the last point's query, and the one at its ring's end
    assert int(search[1]) == most                                                 # the device ran what the rule says, query by query


def test_lattice_ties_through_the_kth_place(nm):
    for knn in (10, 30, 100):
        check(nm, "lattice", knn)


@pytest.mark.parametrize("name", ["flat", "line"])
def test_clouds_without_extent_along_an_axis(nm, name):
    normals = check(nm, name, 30)[0]
    if name == "flat":
        assert normals.tolist() == [[0.0, 0.0, 1.0]] * normals.shape[0]
    else:
        assert normals[:, 0].abs().max() < 1e-14


def test_a_far_isolated_point(nm):
    _, _, nbr, count, search = check(nm, "far_point", 30)
    N = nbr.shape[0]
    assert count[N - 1] == 30 and nbr[N - 1, 0] == N - 1
    assert int(search[0]) >= inputs.grid_dim(N) - 1                               # its cube grew to the whole grid


def test_rows_with_nan(nm):
    normals, cov, nbr, count, _ = check(nm, "with_nan", 30)
    bad = (~torch.isfinite(inputs.cloud("with_nan")).all(dim=1)).nonzero().flatten().tolist()
    assert len(bad) == 2
    for i in bad:
        assert count[i] == 0 and normals[i].tolist() == [0.0, 0.0, 1.0] and not cov[i].any() and (nbr[i] == -1).all()
        assert not (nbr == i).any()


def test_hybrid_search_keeps_what_lies_within_the_radius(nm):
    _, _, nbr, count, _ = check(nm, "hybrid", inputs.HYBRID_KNN, inputs.HYBRID_RADIUS)
    few, some, all_k = (count < 3), (count >= 3) & (count < inputs.HYBRID_KNN), count == inputs.HYBRID_KNN
    assert int(few.sum()) > 0 and int(some.sum()) > 0 and int(all_k.sum()) > 0
    assert ((nbr >= 0).sum(dim=1) == count).all() and (nbr[:, 0] == torch.arange(nbr.shape[0])).all()


def test_the_radius_test_is_strict(nm):
    points = inputs.cloud("quarter_lattice")
    _, _, nbr, count, _ = check(nm, "quarter_lattice", 64, 0.5)
    inner = ((points >= 0.5) & (points <= 1.0)).all(dim=1)                        # two steps from every face
    assert int(inner.sum()) > 0 and (count[inner] == 27).all()                    # |offset|² < 4: 1 + 6 + 12 + 8; the six at d² = r² are out
    i = int(inner.nonzero()[0])
    d2 = (points[nbr[i, :27].long()] - points[i]).double().pow(2).sum(dim=1)
    assert float(d2.max()) == 0.1875


def test_orientation(nm):
    flat = inputs.cloud("flat")
    for cz, want in ((1.0, 1.0), (0.0, 1.0), (-1.0, -1.0)):                       # n . (c - p) = cz exactly: 0 does not flip
        normals = check(nm, "flat", 30, None, (0.3, -0.2, cz))[0]
        assert normals.tolist() == [[0.0, 0.0, want]] * flat.shape[0]            # -0.0 == 0.0
    centre = (0.1, 0.2, -5.0)
    towards = check(nm, "tilted", 30, None, centre)[0]
    canonical = check(nm, "tilted", 30)[0]
    p = inputs.cloud("tilted").double()
    assert (((torch.tensor(centre, dtype=torch.float64) - p) * towards).sum(dim=1) > 0).all()
    assert (canonical[:, 2] > 0).all() and torch.equal(towards, -canonical)      # the largest component is z: positive; the camera is below


def test_optional_outputs_repeat_calls_and_a_given_index(nm):
    from dn_splatter_amd.density import KnnIndex

    points = inputs.cloud("n257").to(DEV)
    full = nm.estimate_normals(points, knn=40, return_covariance=True, return_neighbors=True)
    alone = nm.estimate_normals(points, knn=40)
    again = nm.estimate_normals(points, knn=40)
    given = nm.estimate_normals(points, knn=40, index=KnnIndex(points))
    assert isinstance(alone, torch.Tensor) and len(full) == 4
    for other in (alone, again, given):
        assert torch.equal(full[0].view(torch.int64), other.view(torch.int64))   # the same bytes
    only_cov = nm.estimate_normals(points, knn=40, return_covariance=True)
    assert len(only_cov) == 3 and torch.equal(only_cov[1], full[1]) and torch.equal(only_cov[2], full[3])
    with pytest.raises(ValueError, match="the index is over"):
        nm.estimate_normals(points, knn=40, index=KnnIndex(points[:100]))


def test_nothing_is_written_past_an_output_and_status_stays_zero(nm):
    from dn_splatter_amd import _lib
    from dn_splatter_amd._ops import _cloud_normals_args, _stream
    from dn_splatter_amd.density import KnnIndex

    name, knn, pad = "n257", 40, 64
    points = inputs.cloud(name).to(DEV)
    N = points.shape[0]
    index = KnnIndex(points)
    L = _lib.lib()
    normals = torch.full((N * 3 + pad,), float(SENTINEL), dtype=torch.float64, device=DEV)
    cov = torch.full((N * 6 + pad,), float(SENTINEL), dtype=torch.float64, device=DEV)
    nbr = torch.full((N * knn + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    count = torch.full((N + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    status = torch.zeros(1 + pad, dtype=torch.int32, device=DEV)
    status[1:] = SENTINEL
    scratch = torch.zeros(4 + pad, dtype=torch.int32, device=DEV)
    scratch[4:] = SENTINEL
    a = _cloud_normals_args(points, index.buffer, knn, None, None, scratch, normals, status, cov, nbr, count)
    a.scratch_bytes = L.dnsplat_cloud_normals_scratch_bytes(N, knn)
    _lib.run("dnsplat_cloud_normals", L.dnsplat_cloud_normals, ctypes.byref(a), _stream())
    want_normals, want_cov, want_nbr, want_count = inputs.expected(name, knn)
    assert torch.equal(normals[:N * 3].cpu().reshape(N, 3), want_normals) and (normals[N * 3:] == SENTINEL).all()
    assert torch.equal(cov[:N * 6].cpu().reshape(N, 6), want_cov) and (cov[N * 6:] == SENTINEL).all()
    assert torch.equal(nbr[:N * knn].cpu().reshape(N, knn), want_nbr) and (nbr[N * knn:] == SENTINEL).all()
    assert torch.equal(count[:N].cpu(), want_count) and (count[N:] == SENTINEL).all()
    assert int(status[0]) == 0 and (status[1:] == SENTINEL).all()
    assert scratch[2:4].tolist() == [0, 0] and (scratch[4:] == SENTINEL).all()


def test_depth_normals_of_a_tilted_plane(nm, tn):
    f = inputs.FRAME
    depth, c2w = inputs.frame_depth(), inputs.frame_pose()
    normals, valid = nm.depth_normals(depth.to(DEV), f["fx"], f["fy"], f["cx"], f["cy"], c2w)
    want_normals, want_valid = tn.depth_normals(depth, f["fx"], f["fy"], f["cx"], f["cy"], c2w)
    normals, valid = normals.cpu(), valid.cpu()
    assert tuple(normals.shape) == (f["H"], f["W"], 3) and normals.dtype == torch.float64 and valid.dtype == torch.bool
    assert torch.equal(valid, depth > 0) and torch.equal(valid, want_valid) and int((~valid).sum()) == 66
    assert not normals[~valid].any()
    assert torch.equal(normals, want_normals)                                     # the whole result
    world = tn.backproject(depth, f["fx"], f["fy"], f["cx"], f["cy"], c2w).float().double()[valid.reshape(-1)]
    centre = torch.from_numpy(c2w[:3, 3].copy())
    assert (((centre - world) * normals[valid]).sum(dim=1) > 0).all()             # every valid normal faces the camera
    # the plane's normal in the world, turned towards the camera; the float32 points lie within `off` of the plane, a patch of 200 of
    # them has an in-plane spread of at least `gap`: the perturbation of the covariance is at most 4 off (R + off) (R the patch radius),
    # and the eigenvector moves by at most that over the gap
    n_world = torch.from_numpy(c2w[:3, :3] @ inputs.FRAME_PLANE[0])
    n_world = n_world if float((centre - world[0]) @ n_world) > 0 else -n_world
    off = float(((world - world.mean(dim=0)) @ n_world).abs().max()) * 2
    cov = tn.estimate_normals(world.float(), knn=200)[1].numpy()
    full = np.stack([cov[:, [0, 1, 2]], cov[:, [1, 3, 4]], cov[:, [2, 4, 5]]], axis=1)
    lam = np.linalg.eigvalsh(full)
    R = float((world - world.mean(dim=0)).norm(dim=1).max())
    bound = 4 * off * (R + off) / float((lam[:, 1] - lam[:, 0]).min())
    sines = torch.linalg.cross(normals[valid], n_world.expand(world.shape[0], 3)).norm(dim=1)
    print("depth frame: off-plane", off, "bound", bound, "worst sine", float(sines.max()))
    assert bound < 1e-3 and float(sines.max()) <= bound


def test_points3d_normals_equal_the_restatement_composed_by_hand(nm, tn):
    points = inputs.cloud("hybrid")
    want = inputs.expected("hybrid", 30, 0.1)[0]
    want = (want / want.norm(dim=1, keepdim=True)).float()
    got = nm.points3D_normals(points.to(DEV))
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    T = torch.tensor([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -0.25], [0.0, 0.0, 2.0, 3.0]])
    moved = nm.points3D_normals(points.to(DEV), T)
    by_hand = torch.cat([want, torch.ones(want.shape[0], 1)], dim=1) @ T.T       # the reference's statement: the translation is added
    assert torch.equal(moved.cpu(), by_hand)
    assert torch.equal(by_hand[:, 2], want[:, 2] * 2 + 3)
