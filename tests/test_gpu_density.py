"""The Gaussian density field on HIP (csrc/density.hip through dn_splatter_amd.density) against the fp64 brute force of torch_density
on the device and against the reference's own outputs (tests/golden/reference_density.npz).

The search is index-exact: the kernel ranks by (d², index) with d² in double, as sklearn does, so every comparison of indices is
``torch.equal``.  Density and normals get 4 x e_ref (_density_inputs.TOL_DENSITY relative to max(value, 1e-4), TOL_NORMAL
component-wise; test_density_reference.py holds e_ref to the fixture), which belongs to inputs of the fixture's law; the cases built
here use that law.  The two neighbour sources, and the lattice against the sample list, must agree to the bit."""
import os

import numpy as np
import pytest
import torch

import _density_inputs as inputs
import _export_inputs as frames

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"
KS = ((16, 1), (3, 1), (1, 0), (31, 1))
NS = (1, 16, 17, 18, 1000, 4099)
MS = (1, 63, 64, 65, 1000)


@pytest.fixture(scope="module")
def density():
    from dn_splatter_amd import density as d

    return d


@pytest.fixture(scope="module")
def td():
    from dn_splatter_amd import torch_density as t

    return t


@pytest.fixture(scope="module")
def gold():
    g, t = inputs.load_golden(os.path.join(HERE, "golden", inputs.GOLDEN))
    return g, {k: v.to(DEV) for k, v in t.items()}


@pytest.fixture(scope="module")
def gold_field(gold, density):
    _, t = gold
    return density.GaussianDensityField(t["means"], t["scales"], t["quats"], t["opacities"])


@pytest.fixture(scope="module")
def gold_ref(gold, td):
    """The fp64 restatement on the fixture, computed once: neighbours, density, normals."""
    g, t = gold
    t64 = {k: v.double() for k, v in t.items()}
    closest = td.closest(t["means"], t["samples"])
    dens = td.density(t64["means"], t64["scales"], t64["quats"], t64["opacities"], t64["samples"], closest)
    grads = {nc: td.density_grad(t64["means"], t64["scales"], t64["quats"], t64["samples"], nc, closest) for nc in (None, 1, 5)}
    flag = torch.from_numpy(np.unpackbits(g["switch_flag"])[:inputs.M_FIX].astype(bool)).to(DEV)
    return dict(closest=closest, density=dens, grads=grads, flag=flag, t64=t64)


_CASES = {}


def _case(N):
    """means and 1000 queries of the fixture's law (8 of them far outside the box), and the full fp64 ranking, once per N."""
    if N not in _CASES:
        from dn_splatter_amd import torch_density as t

        u = inputs.field_inputs(N, 1000, seed=100 + N)
        means, queries = u["means"].to(DEV), u["samples"].to(DEV)
        order = torch.sort(t.squared_distances(means, queries), dim=1, stable=True).indices
        _CASES[N] = (means, queries, order)
    return _CASES[N]


def _dens_ok(got, ref, flag=None, extra=0.0):
    tol = torch.full_like(ref, inputs.TOL_DENSITY + extra)
    if flag is not None:
        tol = tol + flag.double() * inputs.TOL_SWITCH_EXTRA
    err = (got.double() - ref).abs() / ref.clamp_min(1e-4)
    print(f"density: worst error {float(err.max()):.3e} of {inputs.TOL_DENSITY:.3e}")
    return bool((err <= tol).all())


def _normal_ok(got, ref):
    err = (got.double() - ref).abs().max()
    print(f"normals: worst error {float(err):.3e} of {inputs.TOL_NORMAL:.3e}")
    return bool(err <= inputs.TOL_NORMAL)


# ---- the search ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("k,skip", KS)
@pytest.mark.parametrize("N", NS)
def test_search_is_index_exact(density, N, k, skip):
    means, queries, order = _case(N)
    if k + skip > N:
        with pytest.raises(ValueError):
            density.knn(means, queries, k, skip)
        return
    index = density.build_index(means)
    for M in MS:
        got = density.knn(index, queries[1000 - M:], k, skip)                       # the far queries are the last rows
        assert got.dtype == torch.int32 and tuple(got.shape) == (M, k)
        assert torch.equal(got.long(), order[1000 - M:, skip:skip + k]), (N, M, k, skip)


def test_search_equals_knn_sk_on_the_fixture(gold, gold_field, gold_ref, density, td):
    g, t = gold
    closest = torch.from_numpy(g["closest"].astype(np.int64)).to(DEV)
    got = gold_field.closest(t["samples"])
    assert got.dtype == torch.int64 and torch.equal(got, closest) and torch.equal(gold_ref["closest"], closest)
    idx, d2 = density.knn(t["means"], t["samples"], 17, skip=0, return_d2=True)
    assert torch.equal(idx[:, 1:].long(), closest)
    ref = torch.sort(td.squared_distances(t["means"], t["samples"]), dim=1).values[:, :17]
    assert torch.equal(d2, ref.float())                                             # the double, rounded once
    # the 3-NN of the scale initialisation: skip = 1 drops the point itself
    own = density.knn(t["means"], t["means"], 3, skip=1)
    assert torch.equal(own.long(), td.knn(t["means"], t["means"], 3, skip=1))
    assert not bool((own.long() == torch.arange(inputs.N_FIX, device=DEV)[:, None]).any())


def _lattice_points(n, step=1.0):
    a = torch.arange(n, dtype=torch.float32) * step
    return torch.stack(torch.meshgrid(a, a, a, indexing="ij"), dim=-1).reshape(-1, 3)


def _degenerate(name):
    g = torch.Generator().manual_seed(5)
    if name == "one_cell_plus_outlier":          # 999 points within 1e-3 of the origin and one at 100: every other cell is empty
        pts = torch.cat([1e-3 * torch.rand(999, 3, generator=g), torch.tensor([[100.0, 100.0, 100.0]])])
        q = torch.cat([1e-3 * torch.rand(60, 3, generator=g), torch.tensor([[50.0, 50.0, 50.0], [99.0, 100.0, 101.0], [-3.0, 0.0, 0.0]])])
    elif name == "coplanar":                     # no extent along z: one layer of cells
        pts = torch.cat([torch.rand(500, 2, generator=g) * 4, torch.full((500, 1), 1.5)], dim=1)
        q = torch.cat([pts[:40] + 0.01, torch.rand(40, 3, generator=g) * 6 - 1])
    elif name == "collinear":                    # extent along x alone
        pts = torch.cat([torch.rand(300, 1, generator=g) * 4, torch.full((300, 2), -2.0)], dim=1)
        q = torch.cat([pts[:40], torch.rand(40, 3, generator=g) * 6 - 3])
    elif name == "identical":                    # every distance ties: ascending index
        pts = torch.full((200, 3), 0.75)
        q = torch.cat([pts[:3], torch.rand(20, 3, generator=g)])
    elif name == "cell_boundaries":              # 12^3 = 1728 points -> 9 cells per axis over [0, 11]; integer and half-integer
        pts = _lattice_points(12)                # coordinates tie many distances exactly, and 11 / 9 is no float
        q = torch.cat([_lattice_points(12)[::7], _lattice_points(6, 2.0) + 0.5, _lattice_points(4, 11.0 / 9.0 * 3)])
    elif name == "duplicates_and_boundary":      # 1000 points -> 7 cells over [0, 7]: every point ON a cell boundary, each twice
        pts = torch.cat([_lattice_points(8)[:500], _lattice_points(8)[:500]])
        q = torch.cat([_lattice_points(8)[::5], _lattice_points(8)[::9] + 0.5])
    elif name == "outside_and_far":
        pts = (torch.rand(1000, 3, generator=g) - 0.5) * 10
        q = torch.cat([(torch.rand(30, 3, generator=g) - 0.5) * 30, torch.tensor([[1e6, 0.0, 0.0], [-1e6, 1e6, 1e6], [0.0, 0.0, -1e6], [5.0, 5.0, 5.0],
                                                                                 [3e38, 0.0, 0.0]])])
    else:
        raise KeyError(name)
    return pts.to(DEV), q.to(DEV)


@pytest.mark.parametrize("name", ["one_cell_plus_outlier", "coplanar", "collinear", "identical", "cell_boundaries", "duplicates_and_boundary",
                                  "outside_and_far"])
def test_degenerate_layouts(density, td, name):
    pts, q = _degenerate(name)
    index = density.build_index(pts)
    for k, skip in KS:
        if k + skip > pts.shape[0]:
            continue
        got, d2 = index.query(q, k, skip, return_d2=True)
        ref, ref_d2 = td.knn(pts, q, k, skip, return_d2=True)
        assert torch.equal(got.long(), ref), (name, k, skip)
        assert torch.equal(d2, ref_d2.float()), (name, k, skip)
    if name == "identical":
        assert torch.equal(index.query(q, 16, 1).long(), torch.arange(1, 17, device=DEV).expand(q.shape[0], 16))


def test_a_nan_query_gives_minus_one_and_leaves_the_others(density, td):
    means, queries, order = _case(1000)
    q = queries[:130].clone()
    q[7, 1] = float("nan")
    q[64] = float("inf")
    q[129, 2] = float("-inf")
    bad = torch.tensor([7, 64, 129], device=DEV)
    got, d2 = density.knn(means, q, 16, 1, return_d2=True)
    assert bool((got[bad] == -1).all()) and bool(torch.isnan(d2[bad]).all())
    keep = torch.ones(130, dtype=torch.bool, device=DEV)
    keep[bad] = False
    assert torch.equal(got[keep].long(), order[:130, 1:17][keep])
    field = density.GaussianDensityField(means, *(inputs.field_inputs(1000, 1, seed=1100)[k].to(DEV) for k in ("scales", "quats", "opacities")))
    d, n = field.density(q), field.density_grad(q)
    assert bool(torch.isnan(d[bad]).all()) and bool(torch.isnan(n[bad]).all())
    assert bool(torch.isfinite(d[keep]).all()) and bool(torch.isfinite(n[keep]).all())
    assert torch.equal(d[keep], field.density(q[keep]))


def test_two_builds_give_equal_bits(density):
    means, queries, _ = _case(4099)
    a, b = density.build_index(means), density.build_index(means)
    L = density._lib.lib()
    G = L.dnsplat_knn_grid_dim(4099)
    kept = (64 + ((4 * (G ** 3 + 1) + 15) // 16) * 16 + 16 * 4099) // 8          # header, cell starts, sorted copy: what a query reads
    assert torch.equal(a.buffer[:kept], b.buffer[:kept])
    sorted_rows = a.buffer[kept - 2 * 4099:kept].view(torch.int32).reshape(4099, 4)
    assert torch.equal(torch.sort(sorted_rows[:, 3]).values, torch.arange(4099, dtype=torch.int32, device=DEV))      # a permutation
    assert torch.equal(a.query(queries, 31, 1), b.query(queries, 31, 1))


# ---- density and normals -------------------------------------------------------------------------------------------------------------


def test_density_on_the_fixture(gold, gold_field, gold_ref):
    g, t = gold
    ref = gold_ref
    inside = gold_field.density(t["samples"])
    assert inside.dtype == torch.float32 and tuple(inside.shape) == (inputs.M_FIX,)
    assert _dens_ok(inside, ref["density"], ref["flag"])
    assert _dens_ok(inside, torch.from_numpy(g["density"]).to(DEV).double(), ref["flag"], extra=inputs.E_REF_DENSITY)      # its own fp32 values
    for dtype in (torch.int64, torch.int32):
        given = gold_field.density(t["samples"], closest_gaussians=ref["closest"].to(dtype))
        assert torch.equal(given, inside), dtype                                    # both neighbour sources: equal bits
    assert 0 < int((inside > 0.99).sum()) < inputs.M_FIX and int((inside == 1e-4).sum()) >= inputs.FAR


@pytest.mark.parametrize("nc", [None, 1, 5])
def test_normals_on_the_fixture(gold, gold_field, gold_ref, nc):
    g, t = gold
    ref = gold_ref
    inside = gold_field.density_grad(t["samples"], num_closest_gaussians=nc)
    assert inside.dtype == torch.float32 and tuple(inside.shape) == (inputs.M_FIX, 3)
    assert _normal_ok(inside, ref["grads"][nc])
    err = float((inside - torch.from_numpy(g[f"grad_{nc or 'all'}"]).to(DEV)).abs().max())
    assert err <= inputs.TOL_NORMAL + inputs.E_REF_NORMAL, err                      # the reference's own fp32 values
    for dtype in (torch.int64, torch.int32):
        given = gold_field.density_grad(t["samples"], num_closest_gaussians=nc, closest_gaussians=ref["closest"].to(dtype))
        assert torch.equal(given, inside), dtype
    if nc is not None:                                                              # a narrower tensor, all of it used
        cut = gold_field.density_grad(t["samples"], closest_gaussians=ref["closest"][:, :nc].contiguous())
        assert torch.equal(cut, inside)
    assert bool(((inside.double().norm(dim=-1) - 1).abs() < 1e-5).all())


def test_small_scales_a_sample_on_a_mean_and_bad_indices(density, td):
    u = {k: v.to(DEV) for k, v in inputs.field_inputs(1000, 256, seed=77).items()}
    u["scales"][::3] -= 9.0                                                         # exp(s) < 1e-3: clamped
    assert float(torch.exp(u["scales"][::3]).max()) < 1e-3
    samples = u["samples"]
    samples[:64] = u["means"][torch.arange(0, 192, 3, device=DEV)]                  # exactly on a mean (a clamped one)
    field = density.GaussianDensityField(u["means"], u["scales"], u["quats"], u["opacities"])
    u64 = {k: v.double() for k, v in u.items()}
    closest = td.closest(u["means"], samples)
    d = field.density(samples)
    assert torch.equal(field.density(samples, closest_gaussians=closest), d)
    assert _dens_ok(d, td.density(u64["means"], u64["scales"], u64["quats"], u64["opacities"], samples.double(), closest))
    assert _normal_ok(field.density_grad(samples), td.density_grad(u64["means"], u64["scales"], u64["quats"], samples.double(), None, closest))
    # knn_sk drops the mean the sample sits on; a caller's tensor that keeps it (skip = 0) has m² = 0 in column 0
    own = td.knn(u["means"], samples, 16, skip=0)
    assert torch.equal(own[:64, 0], torch.arange(0, 192, 3, device=DEV))
    n1 = field.density_grad(samples, num_closest_gaussians=1, closest_gaussians=own)
    assert bool((n1[:64] == 0).all()) and bool(torch.isfinite(n1).all())            # the normal is zero, not nan
    assert bool((td.density_grad(u64["means"], u64["scales"], u64["quats"], samples.double(), 1, own)[:64] == 0).all())
    d0 = field.density(samples, closest_gaussians=own)
    assert _dens_ok(d0, td.density(u64["means"], u64["scales"], u64["quats"], u64["opacities"], samples.double(), own))
    assert torch.equal(d0, field._eval(samples, None, None, 0.0, None, 16, 0, None, True, False)[0])
    # an index outside the field makes its row nan and reads nothing out of bounds
    bad = closest.clone()
    bad[5, 3], bad[9, 0] = 1000, -1
    db = field.density(samples, closest_gaussians=bad)
    assert bool(torch.isnan(db[[5, 9]]).all())
    keep = torch.ones(256, dtype=torch.bool, device=DEV)
    keep[[5, 9]] = False
    assert torch.equal(db[keep], d[keep])


# ---- the lattice ---------------------------------------------------------------------------------------------------------------------


def test_volume_equals_density_on_the_flattened_grid(gold, gold_field):
    X = torch.linspace(-4.0, 4.5, 33, device=DEV)
    Y = torch.linspace(-3.0, 2.0, 20, device=DEV) * 1.1
    Z = torch.linspace(-1.0, 5.5, 7, device=DEV)
    grid = torch.stack(torch.meshgrid(X, Y, Z, indexing="ij"), dim=-1).reshape(-1, 3)
    flat = gold_field.density(grid)
    vol = gold_field.volume(X, Y, Z)
    assert tuple(vol.shape) == (33, 20, 7) and torch.equal(vol.reshape(-1), flat)
    mask = torch.rand(33, 20, 7, generator=torch.Generator().manual_seed(3)).to(DEV) < 0.6
    masked = gold_field.volume(X, Y, Z, mask=mask, fill=-1e6)
    assert torch.equal(masked[mask], vol[mask]) and bool((masked[~mask] == -1e6).all()) and 0 < int(mask.sum()) < mask.numel()
    assert torch.equal(gold_field.volume(X, Y, Z, mask=torch.zeros_like(mask), fill=2.5), torch.full_like(vol, 2.5))


def test_density_volume_equals_the_reference_lattice(gold, gold_field, density):
    g, _ = gold
    R, radius = int(g["volume_spec"][0]), float(g["volume_spec"][1])
    for key, box in (("volume", None), ("volume_crop", inputs.crop_box(DEV))):
        vol = density.density_volume(gold_field, R, radius, box)
        ref = torch.from_numpy(g[key]).to(DEV)
        assert tuple(vol.shape) == (R, R, R)
        assert torch.equal(vol == -1e6, ref == -1e6), key
        inside = ref != -1e6
        err = ((vol[inside].double() - ref[inside].double()).abs() / ref[inside].double().clamp_min(1e-4)).max()
        print(f"{key}: worst error {float(err):.3e}")
        assert float(err) <= inputs.TOL_DENSITY + inputs.E_REF_DENSITY, key           # the reference's own fp32 values: e_ref more


# ---- the model's methods and the exporter's branch -----------------------------------------------------------------------------------


def test_install_density_binds_the_three_methods_and_follows_the_parameters(gold, gold_field, density):
    _, t = gold

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.gauss_params = torch.nn.ParameterDict({k: torch.nn.Parameter(t[k].clone()) for k in ("means", "scales", "quats", "opacities")})

        means = property(lambda self: self.gauss_params["means"])
        scales = property(lambda self: self.gauss_params["scales"])
        quats = property(lambda self: self.gauss_params["quats"])
        opacities = property(lambda self: self.gauss_params["opacities"])

    model = Model()
    assert density.install_density(model) == ["get_closest_gaussians", "get_density", "get_density_grad"]
    s = t["samples"]
    closest = model.get_closest_gaussians(s)
    assert torch.equal(closest, gold_field.closest(s))
    assert torch.equal(model.get_density(s), gold_field.density(s))
    assert torch.equal(model.get_density(s, closest_gaussians=closest), gold_field.density(s))
    assert torch.equal(model.get_density_grad(samples=s, num_closest_gaussians=1), gold_field.density_grad(s, 1))
    assert torch.equal(model.get_density_grad(s, closest_gaussians=closest), gold_field.density_grad(s))
    first = model.__dict__[density._FIELD][1]
    model.get_density(s)
    assert model.__dict__[density._FIELD][1] is first                               # nothing changed: the same snapshot
    with torch.no_grad():
        model.means.add_(0.25)                                                      # an optimiser step: _version moves
    moved = density.GaussianDensityField(t["means"] + 0.25, t["scales"], t["quats"], t["opacities"])
    assert model.__dict__[density._FIELD][1] is first
    assert torch.equal(model.get_density(s), moved.density(s)) and model.__dict__[density._FIELD][1] is not first
    assert torch.equal(model.get_closest_gaussians(s), moved.closest(s))
    for k in ("means", "scales", "quats", "opacities"):                             # a refinement step: other shapes
        model.gauss_params[k] = torch.nn.Parameter(model.gauss_params[k].detach()[:2000].clone())
    cut = density.GaussianDensityField(t["means"][:2000] + 0.25, t["scales"][:2000], t["quats"][:2000], t["opacities"][:2000])
    assert torch.equal(model.get_density_grad(s, num_closest_gaussians=5), cut.density_grad(s, 5))


def test_add_frame_with_density_grad_normals(density, td):
    from dn_splatter_amd import export

    H, W = 48, 64
    f = frames.frame_inputs(H, W)
    c2w_gl, fx, fy, cx, cy = frames.camera(H, W)
    cam = frames.Cam(c2w_gl.to(DEV), fx, fy, cx, cy, W, H)
    depth = f["depth"].to(DEV)
    out = dict(depth=depth, rgb=f["rgb"].to(DEV), surface_normal=f["surface_normal"].to(DEV))
    # Gaussians of the fixture's law around the surface the frame sees
    c2w_cv = export._export_c2w(cam.camera_to_worlds)
    xyz = export.density_grad_samples(depth[..., 0], cam, c2w_cv)
    xyz64, c2w64 = td.density_grad_samples(depth.double(), frames.Cam(c2w_gl.double().to(DEV), fx, fy, cx, cy, W, H))
    assert float((xyz.double() - xyz64).abs().max()) <= 1e-5                        # ~ 8 u (|p| |A| + |t|) at coordinates below 10
    u = {k: v.to(DEV) for k, v in inputs.field_inputs(1500, 1, seed=31).items()}
    centre, half = xyz.mean(dim=0), (xyz.max(dim=0).values - xyz.min(dim=0).values).max() * 0.6
    means = (centre + u["means"] / 5.0 * half).contiguous()
    scales = (u["scales"] + torch.log(half / 5.0)).contiguous()
    field = density.GaussianDensityField(means, scales, u["quats"], u["opacities"])
    indices = torch.arange(0, H * W, 3, device=DEV)
    cloud = export.OrientedPointCloud(H * W, DEV)
    cloud.add_frame(out, cam, samples_per_frame=indices.numel(), indices=indices, normal_method="density_grad", field=field)
    cloud.add_frame(out, cam, samples_per_frame=indices.numel(), indices=indices)   # the default branch, unchanged
    points, normals, _ = cloud.finish()
    m = indices.numel()
    assert points.shape[0] == 2 * m and torch.equal(points[:m], points[m:])
    # the restatement in fp64 at the SAME fp32 sample positions: the neighbours are then the same Gaussians
    n64 = td.density_grad(means.double(), scales.double(), u["quats"].double(), xyz.double(), num_closest_gaussians=1)
    want = td.orient_normals(n64, xyz.double(), c2w64)[indices]
    view = -xyz.double() + c2w64[:3, 3]
    dots = ((n64 * view / view.norm(dim=-1, keepdim=True)).sum(-1))[indices]
    sure = dots.abs() > 1e-4                                                        # the flip towards the camera is decided
    assert int(sure.sum()) > 0.95 * m
    err = float((normals[:m].double() - want)[sure].abs().max())
    # TOL_NORMAL on the gradient, carried through a rotation (row sums of |R| <= sqrt 3) and two normalisations, plus the fp32
    # rounding of the image encoding and of the kernel's transform (about 20 u)
    print(f"density_grad normals: worst error {err:.3e} of {2 * inputs.TOL_NORMAL + 2e-6:.3e}")
    assert err <= 2 * inputs.TOL_NORMAL + 2e-6
    default = export.OrientedPointCloud(H * W, DEV)
    default.add_frame(out, cam, samples_per_frame=m, indices=indices)
    assert torch.equal(default.finish()[1], normals[m:])
    with pytest.raises(ValueError):
        cloud.add_frame(out, cam, samples_per_frame=m, indices=indices, normal_method="density_grad")
    with pytest.raises(ValueError):
        cloud.add_frame(out, cam, samples_per_frame=m, indices=indices, normal_method="other")


def test_scale_init_knn_hip_equals_sklearn():
    from dn_splatter_amd import synthetic

    a = synthetic.make_gauss_params(3000, seed=4, scale_init="knn")
    b = {k: v.detach().cpu() for k, v in synthetic.make_gauss_params(3000, seed=4, scale_init="knn_hip", device=DEV).items()}
    # the same three distances (float64, rounded to float32 on either side), averaged in float32 in another order
    assert torch.equal(a["means"], b["means"])
    assert float((a["scales"].detach() - b["scales"]).abs().max()) <= 4 * 2.0 ** -23
