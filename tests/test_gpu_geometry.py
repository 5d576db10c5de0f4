"""The geometry scores on the MI355X (csrc/geometry.hip through dn_splatter_amd/geometry.py) against the PyTorch restatement
(dn_splatter_amd/torch_geometry.py) in float64 on the device, and against the reference's recorded outputs
(tests/golden/reference_geometry.npz).

What is exact: the nearest index (``torch.equal``), d² (the restatement states the same two FMAs: bit patterns), the counts, both order
statistics of the percentile (bit patterns), the sampled faces, points and normals (bit patterns, from the same device-computed cdf).
What has a tolerance: the means and the percentile, 4 x 2^-52 relative (the kernel's fixed-order fold of per-workgroup partials against
torch's reduction; the percentile's two square roots and ``_lerp``); |dot| 8 x 2^-53 absolute (its divisions and sums, operands <= 1);
the areas 4 x 2^-53 relative; the fixture at the tolerances of tests/test_geometry_reference.py.

Sizes: N in {1, 2, 17, 1000, 4099} targets is grid dimension 1, the first multi-cell grids and a non-round size; M in {1, 63, 64, 65, 513,
3000} sources is the wave and workgroup edges and two workgroups plus one lane (partials, histogram adds); the first min(40, M / 2)
sources lie 3 units outside the targets' box."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _geometry_inputs as inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
REL = 4 * 2.0 ** -52
REL_MEAN = 1e-12
REL_F32 = 2.0 ** -23
N_SIZES = (1, 2, 17, 1000, 4099)
M_SIZES = (1, 63, 64, 65, 513, 3000)


@pytest.fixture(scope="module")
def geo():
    from dn_splatter_amd import geometry

    return geometry


@pytest.fixture(scope="module")
def tg():
    from dn_splatter_amd import torch_geometry

    return torch_geometry


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "reference_geometry.npz")))


def dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def rel(a, b):
    a, b = float(a), float(b)
    return 0.0 if a == b else abs(a - b) / abs(b)


def compare(tg, got, want, normals=True, means=True):
    """One direction of the device against the restatement's dictionary.  ``means=False`` leaves the three means to the caller: REL is
    stated for the few partials of the sizes here (tests/test_gpu_geometry_edges.py holds them to a derived bound past one fold trip)."""
    g = tg.GEOM_INDEX
    assert got.idx.dtype == torch.int32 and torch.equal(got.idx.long(), want["idx"])
    assert torch.equal(bits(got.dist2), bits(want["dist2"]))
    assert torch.equal(got.counts, want["counts"])
    gs, ws = got.scalars.tolist(), want["scalars"].tolist()
    for k in ("order_lo_d2", "order_hi_d2"):
        assert np.float64(gs[g[k]]).view(np.int64) == np.float64(ws[g[k]]).view(np.int64), k
    for k in ("mean_d", "mean_d2", "percentile", "min_d", "max_d")[0 if means else 2:]:
        print(k, gs[g[k]], ws[g[k]], rel(gs[g[k]], ws[g[k]]) / 2.0 ** -52)
        assert rel(gs[g[k]], ws[g[k]]) <= REL, k
    assert gs[g["share_lt"]] == ws[g["share_lt"]] and gs[g["share_le"]] == ws[g["share_le"]]
    assert gs[10:] == [0.0, 0.0]
    if normals:
        assert float((got.absdot - want["absdot"]).abs().max()) <= 8 * 2.0 ** -53
        assert not means or rel(gs[g["mean_absdot"]], ws[g["mean_absdot"]]) <= REL
    else:
        assert got.absdot is None and np.isnan(gs[g["mean_absdot"]])


@pytest.mark.parametrize("N", N_SIZES)
@pytest.mark.parametrize("M", M_SIZES)
def test_cloud_distances_sizes(geo, tg, N, M):
    tgt, tgt_n = dev(*inputs.target(N, seed=20 + N))
    src, src_n = dev(*inputs.source(M, seed=30 + M))
    got = geo.cloud_distances(src, tgt, src_n, tgt_n)
    compare(tg, got, tg.cloud_distances(src, tgt, src_n, tgt_n))
    if M > 2 * inputs.FAR:
        assert float(got.distances[:inputs.FAR].min()) > 2.5, "the far points are far"


def test_without_normals_and_index_reuse(geo, tg):
    from dn_splatter_amd.density import KnnIndex

    tgt, _ = dev(*inputs.target(1000))
    src, _ = dev(*inputs.source(513))
    index = KnnIndex(tgt)
    got = geo.cloud_distances(src, index, threshold=0.08, percentile=75.0)
    compare(tg, got, tg.cloud_distances(src, tgt, threshold=0.08, percentile=75.0), normals=False)
    again = geo.cloud_distances(src, index, threshold=0.08, percentile=75.0)
    assert torch.equal(bits(again.scalars), bits(got.scalars))
    with pytest.raises(ValueError):
        geo.cloud_distances(src, tgt, src_normals=src)
    with pytest.raises(ValueError):
        geo.cloud_distances(src, tgt, percentile=101.0)


@pytest.mark.parametrize("n,q", [(1, 90.0), (2, 90.0), (11, 90.0), (513, 0.0), (513, 50.0), (513, 100.0), (3000, 37.5)])
def test_percentile_edges(geo, tg, n, q):
    """n = 11 at q = 90: h = 9.0 exactly, the weight is 0; q = 0 and 100 are min and max; n = 1 and 2 clip the second rank."""
    tgt, _ = dev(*inputs.target(1000))
    src, _ = dev(*inputs.source(n, seed=40 + n, far=0))
    got = geo.cloud_distances(src, tgt, percentile=q)
    want = tg.cloud_distances(src, tgt, percentile=q)
    compare(tg, got, want, normals=False)
    d = got.distances.cpu().numpy()
    assert rel(got.percentile, np.percentile(d, q)) <= REL
    if q in (0.0, 100.0):
        assert got.percentile == (got.min_d if q == 0.0 else got.max_d)


def test_source_equal_to_target(geo, tg):
    """Every distance is 0: one histogram bin takes every count in every round."""
    tgt, n = dev(*inputs.target(3000))
    got = geo.cloud_distances(tgt, tgt, n, n)
    assert torch.equal(got.idx.long(), torch.arange(3000, device=DEV))
    assert not bool(got.dist2.any()) and got.percentile == 0.0 and got.max_d == 0.0 and got.mean_d == 0.0
    assert got.n_lt == 3000 and got.n_le == 3000 and got.share_lt == 1.0
    assert abs(got.mean_absdot - 1.0) <= 4 * 2.0 ** -53


def test_ties_go_to_the_lowest_index(geo, tg):
    base, _ = inputs.target(300)
    tgt = np.concatenate([base, base[:120], base[50:200]])[np.random.default_rng(3).permutation(570)]
    tgt_d, = dev(tgt)
    src, _ = dev(*inputs.source(513))
    got = geo.cloud_distances(src, tgt_d)
    want = tg.cloud_distances(src, tgt_d)
    compare(tg, got, want, normals=False)
    # the restatement's rule, spelled out with a stable sort of the plain float64 distances of the duplicated rows
    d2 = ((src.double()[:, None, :] - tgt_d.double()[None, :, :]) ** 2).sum(-1)
    first = torch.sort(d2, dim=1, stable=True).indices[:, 0]
    assert torch.equal(got.idx.long(), first)
    same = (tgt_d[got.idx.long()][:, None, :] == tgt_d[None, :, :]).all(-1)
    assert bool((same.sum(1) > 1).any()), "no source point has a duplicated nearest target"
    assert torch.equal(got.idx.long(), same.long().argmax(dim=1))


def test_non_finite_rows(geo, tg):
    tgt, tgt_n = dev(*inputs.target(1000))
    src, src_n = dev(*inputs.source(513))
    clean = geo.cloud_distances(src, tgt, src_n, tgt_n)
    dirty = src.clone()
    dirty[7, 1] = float("nan")
    dirty[300, 2] = float("inf")
    got = geo.cloud_distances(dirty, tgt, src_n, tgt_n)
    assert got.idx[7] == -1 and got.idx[300] == -1 and got.n_nonfinite == 2 and got.n == 513
    assert bool(torch.isnan(got.dist2[[7, 300]]).all()) and bool(torch.isnan(got.absdot[[7, 300]]).all())
    for k in ("mean_d", "mean_d2", "mean_absdot", "percentile", "min_d", "max_d"):
        assert np.isnan(getattr(got, k)), k
    keep = torch.ones(513, dtype=torch.bool, device=DEV)
    keep[[7, 300]] = False
    assert torch.equal(got.idx[keep], clean.idx[keep]) and torch.equal(bits(got.dist2[keep]), bits(clean.dist2[keep]))
    assert torch.equal(bits(got.absdot[keep]), bits(clean.absdot[keep]))
    want = tg.cloud_distances(dirty, tgt, src_n, tgt_n)
    assert torch.equal(got.counts, want["counts"]) and torch.equal(got.idx.long(), want["idx"])
    assert got.share_lt == float(want["scalars"][tg.GEOM_INDEX["share_lt"]])


def test_both_directions_on_the_reference_fixture(geo, tg, golden):
    src, src_n, tgt, tgt_n = dev(golden["src"], golden["src_normals"], golden["tgt"], golden["tgt_normals"])
    for name, (a, an, b, bn) in {"acc": (src, src_n, tgt, tgt_n), "comp": (tgt, tgt_n, src, src_n)}.items():
        got = geo.cloud_distances(a, b, an, bn)
        assert np.array_equal(got.idx.cpu().numpy(), golden[name + "_idx"])
        d, want = got.distances.cpu().numpy(), golden[name + "_dist"]
        assert (np.abs(d - want) <= REL * want).all()
        assert (np.abs(got.absdot.cpu().numpy() - golden[name + "_dot"]) <= 8 * 2.0 ** -53).all()
    m = geo.cloud_metrics(src, src_n, tgt, tgt_n)
    want = dict(zip(golden["mesh_keys"].tolist(), golden["mesh_values"].tolist()))
    assert set(m) == set(tg.METRIC_KEYS) and all(v.is_cuda and v.dtype == torch.float64 and v.dim() == 0 for v in m.values())
    for k in ("Acc", "Comp", "C-L1", "NC"):
        assert rel(m[k], want[k]) <= REL_MEAN, k
    assert rel(golden["mesh_precision"], m["precision"]) <= REL_F32 and rel(golden["mesh_recall"], m["recall"]) <= REL_F32
    assert rel(want["F-score"], m["F-score"]) <= 4 * REL_F32
    acc, comp = geo.PDMetrics()(type("Cloud", (), {"points": golden["src"].astype(np.float64)})(), golden["tgt"])
    assert acc.dim() == 0 and acc.dtype == torch.float64 and acc.is_cuda
    assert rel(acc.item(), golden["pd_acc"]) <= REL_MEAN and rel(comp.item(), golden["pd_comp"]) <= REL_MEAN
    for q, ref in zip(golden["percentiles"], golden["accuracy"]):
        assert rel(geo.calculate_accuracy(src, tgt, percentile=float(q)), ref) <= REL_MEAN
    assert rel(geo.calculate_completeness(src, tgt, threshold=0.05), golden["completeness"]) <= REL_MEAN

    class Pipeline:
        pass

    p = Pipeline()
    assert geo.install_pd_metrics(p) == ["pd_metrics"] and geo.install_pd_metrics(p) == []
    assert rel(p.pd_metrics(src, tgt)[0].item(), golden["pd_acc"]) <= REL_MEAN


def test_cpu_tensors_are_refused(geo, dns):
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        geo.cloud_distances(torch.zeros(4, 3), torch.zeros(4, 3, device=DEV))
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        geo.sample_mesh_surface(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32, device=DEV), count=4)


# ---- the mesh sampler ----------------------------------------------------------------------------------------------------------------

def broken_grid():
    v, t = inputs.grid_mesh()
    t = t.copy()
    t[7] = (3, 10 ** 6, 4)
    t[100] = (-1, 2, 4)
    t[200] = (5, 5, 9)
    return v, t


@pytest.mark.parametrize("mesh", ["tetrahedron", "square", "grid", "broken"])
def test_mesh_areas(geo, tg, mesh):
    v, t = dev(*{"tetrahedron": inputs.tetrahedron, "square": inputs.square_with_degenerate, "grid": inputs.grid_mesh, "broken": broken_grid}[mesh]())
    areas, normals = geo.mesh_areas(v, t)
    want_a, want_n = tg.mesh_areas(v, t)
    assert areas.dtype == torch.float64 and normals.dtype == torch.float32
    assert bool(((areas - want_a).abs() <= 4 * 2.0 ** -53 * want_a).all())
    assert float((normals - want_n).abs().max()) <= 2.0 ** -23
    assert torch.equal(areas == 0, want_a == 0) and torch.equal(normals[areas == 0], torch.zeros_like(normals[areas == 0]))
    if mesh == "broken":
        assert areas[[7, 100, 200]].tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("S", [1, 64, 65, 70_000])
@pytest.mark.parametrize("mesh", ["square", "broken"])
def test_mesh_sample(geo, tg, mesh, S):
    v, t = dev(*{"square": inputs.square_with_degenerate, "broken": broken_grid}[mesh]())
    areas, normals = geo.mesh_areas(v, t)
    cdf = torch.cumsum(areas, dim=0)
    points, point_normals, faces = geo.mesh_sample(S, 9, cdf, v, t, normals)
    want_p, want_n, want_f = tg.mesh_sample(S, 9, cdf, v, t, normals)
    assert faces.dtype == torch.int32 and torch.equal(faces.long(), want_f)
    assert torch.equal(bits(points), bits(want_p)) and torch.equal(bits(point_normals), bits(want_n))
    assert float(areas[faces.long()].min()) > 0.0, "a face without area was drawn"
    assert bool(torch.isfinite(points).all())
    bary = tg.barycentrics(points, v, t, faces.long())
    assert float(bary.min()) >= -1e-6 and float(bary.max()) <= 1 + 1e-6
    again = geo.mesh_sample(S, 9, cdf, v, t, normals)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, (points, point_normals, faces)))
    if S > 64:
        assert not torch.equal(geo.mesh_sample(S, 10, cdf, v, t, normals)[2], faces)


def test_sample_mesh_surface_counts(geo, tg):
    v, t = dev(*inputs.grid_mesh())
    points, normals, faces = geo.sample_mesh_surface(v, t, samples_per_area=1e4, seed=2)
    area = float(torch.cumsum(geo.mesh_areas(v, t)[0], 0)[-1])
    assert points.shape == (int(area * 1e4), 3) and normals.shape == points.shape and faces.shape == (points.shape[0],)
    p = (geo.mesh_areas(v, t)[0] / area).cpu().numpy()
    counts = np.bincount(faces.cpu().numpy(), minlength=t.shape[0])
    S = points.shape[0]
    assert (np.abs(counts - S * p) <= 6 * np.sqrt(S * p * (1 - p))).all()


def test_marching_cubes_sphere_end_to_end(geo, dns):
    """A marching-cubes sphere of radius 1 against the same mesh pushed 0.02 outwards along its radii: Acc and Comp are each within 10 % of
    0.02 and the F-score at 0.05 is 1.  A sanity bound with no calibration behind it: at 1e4 samples per unit area the nearest sample of
    the other surface lies about 0.006 off the foot point, which adds 4 % to 0.02."""
    vol, centre, radius = inputs.sphere_volume(33)
    vertices, triangles = dns.marching_cubes(torch.from_numpy(vol).to(DEV), 0.0)
    inner = (vertices - centre) / radius
    outer = inner * 1.02
    m = geo.mesh_metrics((outer, triangles), (inner, triangles), threshold=0.05, seed=0)
    for k in ("Acc", "Comp"):
        assert abs(float(m[k]) - 0.02) <= 0.002, (k, float(m[k]))
    assert float(m["F-score"]) == 1.0 and float(m["precision"]) == 1.0 and float(m["recall"]) == 1.0
    assert float(m["NC"]) > 0.99 and abs(float(m["C-L1"]) - 0.02) <= 0.002
    counted = geo.mesh_metrics((outer, triangles), (inner, triangles), count=(50_000, 50_000))
    assert abs(float(counted["Acc"]) - 0.02) <= 0.004


# ---- the C entry points --------------------------------------------------------------------------------------------------------------

def test_invalid_arguments_return_codes_without_a_launch(geo, dns):
    from dn_splatter_amd import _lib, _ops
    from dn_splatter_amd.density import KnnIndex

    L = dns.load_library()
    assert L.dnsplat_cloud_distances_scratch_bytes(0) == 0 and L.dnsplat_cloud_distances_scratch_bytes(2 ** 31) == 0
    assert L.dnsplat_cloud_distances_scratch_bytes(1) < L.dnsplat_cloud_distances_scratch_bytes(10 ** 6)
    tgt, tgt_n = dev(*inputs.target(17))
    src, src_n = dev(*inputs.source(63))
    index = KnnIndex(tgt)
    f64 = lambda n: torch.full((n,), -7.0, dtype=torch.float64, device=DEV)  # noqa: E731
    dist2, scalars, counts = f64(63), f64(12), torch.full((4,), -7, dtype=torch.int64, device=DEV)
    scratch = torch.zeros(L.dnsplat_cloud_distances_scratch_bytes(63) // 8, dtype=torch.int64, device=DEV)

    def call(**change):
        kw = dict(N=17, index=index.buffer, src=src, src_normals=src_n, tgt_normals=tgt_n, threshold=0.05, percentile=90.0, dist2=dist2,
                  idx=None, absdot=None, scalars=scalars, counts=counts, scratch=scratch)
        M = change.pop("M", None)
        kw.update(change)
        a = _ops._cloud_distances_args(*(kw[k] for k in ("N", "index", "src", "src_normals", "tgt_normals", "threshold", "percentile", "dist2",
                                                          "idx", "absdot", "scalars", "counts", "scratch")))
        if M is not None:
            a.M = M
        return L.dnsplat_cloud_distances(ctypes.byref(a), None)

    assert L.dnsplat_cloud_distances(None, None) == -1
    for name in ("index", "dist2", "scalars", "counts", "scratch"):
        assert call(**{name: None}) == -1, name
    assert call(M=0) == -1 and call(N=0) == -1
    assert call(src_normals=None) == -1 and call(tgt_normals=None) == -1
    assert call(percentile=-0.5) == -1 and call(percentile=100.5) == -1 and call(percentile=float("nan")) == -1
    assert call(M=2 ** 31) == -4
    a = _lib.MeshSampleArgs()
    assert L.dnsplat_mesh_sample(None, None) == -1 and L.dnsplat_mesh_sample(ctypes.byref(a), None) == -1
    assert L.dnsplat_mesh_areas(0, None, 0, None, None, None, None) == -1
    v, t = dev(*inputs.tetrahedron())
    areas, normals = geo.mesh_areas(v, t)
    out = (torch.empty(4, 3, device=DEV), torch.empty(4, 3, device=DEV), torch.empty(4, dtype=torch.int32, device=DEV))
    a = _ops._mesh_sample_args(0, torch.cumsum(areas, 0), v, t, normals, *out)
    a.S = 2 ** 31
    assert L.dnsplat_mesh_sample(ctypes.byref(a), None) == -4
    a.S, a.faces = 4, None
    assert L.dnsplat_mesh_sample(ctypes.byref(a), None) == -1
    torch.cuda.synchronize()
    assert float(dist2.min()) == -7.0 and float(scalars.min()) == -7.0 and int(counts.min()) == -7, "a refused call wrote its outputs"


def test_determinism(geo):
    tgt, tgt_n = dev(*inputs.target(4099))
    src, src_n = dev(*inputs.source(3000))
    a = geo.cloud_distances(src, tgt, src_n, tgt_n)
    b = geo.cloud_distances(src, tgt, src_n, tgt_n)
    for name in ("dist2", "idx", "absdot", "scalars", "counts"):
        assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    v, t = dev(*inputs.grid_mesh())
    one, two = geo.sample_mesh_surface(v, t, count=70_000, seed=5), geo.sample_mesh_surface(v, t, count=70_000, seed=5)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(one, two))
