"""The restatements behind the TSDF exporter, on the CPU: dn_splatter_amd/torch_tsdf.py (integration, vertex colours) and the ``observed``
argument of torch_marching.marching_cubes.  The HIP kernels are held to these two files with exact equality (tests/test_gpu_tsdf.py);
this file holds the restatements to closed forms, to their strict edges one ulp apart, and to the rules written in include/dnsplat.h.
The rule itself is this project's definition, parity unpinned against Open3D (absent here)."""
import numpy as np
import pytest
import torch

import _tsdf_inputs as inputs

from dn_splatter_amd import torch_marching as tm
from dn_splatter_amd import torch_tsdf as tt
from dn_splatter_amd.torch_mesh_cull import opencv_w2c

F32 = np.float32
LOOK_DOWN_Z = np.diag([1.0, -1.0, -1.0, 1.0])[None]        # OpenGL camera-to-world whose OpenCV world-to-camera is the identity


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ----------------------------------------------------------------------------------------------- a fronto-parallel plane
def test_fronto_parallel_plane_is_the_closed_form_bit_for_bit():
    """One camera at the origin looking down +z, ray_scale = 1, a plane at depth z0, sdf_trunc = 3 voxels.  The voxel pitch is a power
    of two so that every sample point is exact.  Extracted vertices: |z - z0| <= 2^-20 z0 (measured: 0 against the float32 depth
    value, the crossing of a function linear in exactly representable z being exact here)."""
    voxel, dims, origin = 0.0625, (49, 9, 40), (-1.5, -0.25, -0.125)
    W = H = 32
    K = np.array([[20.0, 0, 16.0], [0, 20.0, 16.0], [0, 0, 1.0]])
    z0, trunc = F32(1.53), F32(3 * voxel)
    depth = torch.full((1, H, W), float(z0))
    tsdf, weight = torch.zeros(dims), torch.zeros(dims)
    w2c = opencv_w2c(LOOK_DOWN_Z)
    assert w2c.reshape(3, 4).tolist() == np.eye(4)[:3].tolist()
    tt.integrate(tsdf, weight, None, origin, voxel, w2c, K, depth, None, torch.ones(H, W), float(trunc), 20.0, 0.5)

    x, y, z = (origin[a] + voxel * np.arange(dims[a], dtype=np.float64) for a in range(3))
    x, y, z = np.meshgrid(x, y, z, indexing="ij")
    with np.errstate(all="ignore"):
        uf, vf = (20.0 * x) / z + 16.0 + 0.5, (20.0 * y) / z + 16.0 + 0.5
        sdf = z0 - z.astype(F32)
        assert sdf.dtype == F32
        want_on = (z > 0) & (uf >= 0.0001) & (uf < W - 0.0001) & (vf >= 0.0001) & (vf < H - 0.0001) & (sdf > -trunc)
        want = np.where(want_on, np.minimum(F32(1), sdf / trunc), F32(0)).astype(F32)
    assert want_on.sum() > 2000 and (~want_on).sum() > 2000
    assert (z <= 0).any() and ((z > 0) & (uf < 0.0001)).any() and ((z > 0) & (sdf <= -trunc)).any()      # each way out is taken
    assert np.array_equal(weight.numpy(), want_on.astype(F32))
    assert np.array_equal(bits(tsdf.numpy()), bits(want))
    assert bool((tsdf.numpy()[~want_on] == 0).all())

    vertices, triangles, colors = tt.extract_mesh(tsdf, weight, None, origin, voxel)
    assert colors is None and vertices.dtype == torch.float64 and len(vertices) > 100 and len(triangles) > 100
    err = float(np.abs(vertices.numpy()[:, 2] - float(z0)).max())
    print(f"plane: worst |z - z0| = {err:.3e}, bound {2.0 ** -20 * float(z0):.3e}")
    assert err <= 2.0 ** -20 * float(z0)


# ----------------------------------------------------------------------------------------------- strict edges, one voxel each
def one_voxel(z=1.0, d=1.0, cx=0.5, cy=0.5, offset=0.0, trunc=0.25, far=2.0, x=0.0, W=2, H=1):
    """The weight of a single voxel at (x, 0, z) after one frame of constant depth d under the identity camera."""
    tsdf, weight = torch.zeros(1, 1, 1), torch.zeros(1, 1, 1)
    K = np.array([[1.0, 0, cx], [0, 1.0, cy], [0, 0, 1.0]])
    tt.integrate(tsdf, weight, None, (x, 0.0, z), 1.0, opencv_w2c(LOOK_DOWN_Z), K, torch.full((1, H, W), d, dtype=torch.float32), None,
                 torch.ones(H, W), trunc, far, offset)
    return float(weight[0, 0, 0])


def test_strict_edges_one_ulp_apart():
    up = lambda v: float(np.nextafter(F32(v), F32(np.inf)))             # noqa: E731
    assert one_voxel(z=1.0, d=0.75) == 0                                # sdf == -trunc: skipped
    assert one_voxel(z=1.0, d=up(0.75)) == 1
    assert one_voxel(z=1.9, d=2.0, far=2.0) == 1                        # d == depth_trunc: kept
    assert one_voxel(z=1.9, d=up(2.0), far=2.0) == 0
    assert one_voxel(cx=0.0001) == 1                                    # uf == 0.0001: kept
    assert one_voxel(cx=float(np.nextafter(0.0001, 0.0))) == 0
    assert one_voxel(cx=2 - 0.0001) == 0                                # uf == W - 0.0001: skipped
    assert one_voxel(cx=float(np.nextafter(2 - 0.0001, 0.0))) == 1
    assert one_voxel(cy=0.0001) == 1 and one_voxel(cy=float(np.nextafter(0.0001, 0.0))) == 0
    assert one_voxel(cy=1 - 0.0001) == 0 and one_voxel(cy=float(np.nextafter(1 - 0.0001, 0.0))) == 1
    assert one_voxel(z=0.0) == 0                                        # p.z == 0: skipped
    assert one_voxel(z=5e-324) == 1
    assert one_voxel(z=-1.0, d=1.0) == 0
    for d in (float("nan"), 0.0, -1.0, -0.0):
        assert one_voxel(d=d) == 0
    assert one_voxel(d=float(np.nextafter(F32(0), F32(1)))) == 0        # the smallest depth: sdf = d - 1 <= -trunc
    assert one_voxel(z=1e-3, d=float(np.nextafter(F32(0), F32(1))), trunc=0.25) == 1
    assert one_voxel(x=float("nan")) == 0                               # a NaN projection skips


# ----------------------------------------------------------------------------------------------- the running mean
def test_running_mean_is_the_fp32_recurrence_and_colours_are_the_uint8_cast():
    assert tt.quantise(torch.tensor([0.999999, 1.0, 1.5, -0.1, float("nan"), 0.5])).tolist() == [254.0, 255.0, 255.0, 0.0, 0.0, 127.0]
    depths = [1.1, 1.2, 1.05]
    rgbs = [(0.999999, 1.0, 1.5), (-0.1, 0.5, 0.25), (0.2, 0.999999, 0.0)]
    quant = [(254.0, 255.0, 255.0), (0.0, 127.0, 63.0), (51.0, 254.0, 0.0)]
    K = np.array([[1.0, 0, 0.5], [0, 1.0, 0.5], [0, 0, 1.0]])
    depth = torch.tensor(depths, dtype=torch.float32).reshape(3, 1, 1)
    rgb = torch.tensor(rgbs, dtype=torch.float32).reshape(3, 1, 1, 3)
    w2c = opencv_w2c(np.repeat(LOOK_DOWN_Z, 3, axis=0))
    tsdf, weight, color = torch.zeros(1, 1, 1), torch.zeros(1, 1, 1), torch.zeros(1, 1, 1, 3)
    tt.integrate(tsdf, weight, color, (0.0, 0.0, 1.0), 1.0, w2c, K, depth, rgb, torch.ones(1, 1), 0.25, 20.0, 0.0)
    t, w, c = F32(0), F32(0), [F32(0)] * 3
    for d, q in zip(depths, quant):
        f = min(F32(1), (F32(d) - F32(1.0)) / F32(0.25))
        t = (t * w + f) / (w + F32(1))
        c = [(c[a] * w + F32(q[a])) / (w + F32(1)) for a in range(3)]
        w = w + F32(1)
    assert all(isinstance(v, F32) for v in [t, w] + c)
    assert float(weight) == 3.0 and bits(tsdf.numpy()).item() == bits(np.array(t)).item()
    assert bits(color.numpy()).reshape(-1).tolist() == bits(np.array(c)).tolist()
    # the first frame alone: the colours land on the cast values themselves
    tsdf, weight, color = torch.zeros(1, 1, 1), torch.zeros(1, 1, 1), torch.zeros(1, 1, 1, 3)
    tt.integrate(tsdf, weight, color, (0.0, 0.0, 1.0), 1.0, w2c[:1], K, depth[:1], rgb[:1], torch.ones(1, 1), 0.25, 20.0, 0.0)
    assert color.reshape(-1).tolist() == [254.0, 255.0, 255.0]
    # two calls = one call
    a = [torch.zeros(1, 1, 1), torch.zeros(1, 1, 1), torch.zeros(1, 1, 1, 3)]
    tt.integrate(*a, (0.0, 0.0, 1.0), 1.0, w2c[:2], K, depth[:2], rgb[:2], torch.ones(1, 1), 0.25, 20.0, 0.0)
    tt.integrate(*a, (0.0, 0.0, 1.0), 1.0, w2c[2:], K, depth[2:], rgb[2:], torch.ones(1, 1), 0.25, 20.0, 0.0)
    assert bits(a[0].numpy()).item() == bits(np.array(t)).item() and bits(a[2].numpy()).reshape(-1).tolist() == bits(np.array(c)).tolist()


def test_ray_scale_and_bounds():
    K = inputs.intrinsics(7, 5, 3.0)
    s = tt.ray_scale(K, 5, 7)
    assert s.dtype == torch.float32 and tuple(s.shape) == (5, 7)
    want = np.sqrt(((np.arange(7) - 3.5) / 3.0)[None, :] ** 2 + ((np.arange(5) - 2.5) / 3.0)[:, None] ** 2 + 1.0)
    assert np.abs(s.numpy().astype(np.float64) - want).max() <= 2.0 ** -24 * want.max()
    assert tt.bounds_dims((0, 0, 0), (1, 0.5, 0.0), 0.1) == (11, 6, 2)
    with pytest.raises(ValueError, match=str(2 ** 31 - 1)):
        tt.bounds_dims((0, 0, 0), (13, 13, 13), 0.01)


# ----------------------------------------------------------------------------------------------- `observed` in torch_marching
@pytest.mark.parametrize("shape", [(5, 6, 7), (17, 9, 33)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("field", ["noise", "smooth"])
def test_all_observed_is_the_unmasked_mesh(shape, field):
    vol, level = (inputs.noise(shape), 0.5) if field == "noise" else (inputs.smooth(shape), 0.0)
    v0, t0 = tm.marching_cubes(vol, level)
    v1, t1 = tm.marching_cubes(vol, level, observed=np.ones(shape, dtype=bool))
    assert len(v0) > 0 and len(t0) > 0
    assert np.array_equal(bits(v0), bits(v1)) and np.array_equal(t0, t1)


def test_single_cells_with_one_corner_unobserved():
    for case in range(256):
        vol = np.array([1.0 if (case >> c) & 1 else -1.0 for c in range(8)], dtype=F32)
        vol = np.ascontiguousarray(vol.reshape(2, 2, 2).transpose(2, 1, 0))         # corner c sits at (c & 1, c >> 1 & 1, c >> 2 & 1)
        full_v, _ = tm.marching_cubes(vol, 0.0)
        for corner in range(8):
            at = np.array([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1])
            seen = np.ones((2, 2, 2), dtype=bool)
            seen[tuple(at)] = False
            vol_hidden = vol.copy()
            vol_hidden[tuple(at)] = np.nan                                         # never read into a result
            v, t = tm.marching_cubes(vol_hidden, 0.0, observed=seen)
            assert len(t) == 0
            # values are +-1, so every vertex sits at the middle of its edge: the edge touches the corner iff the two other coordinates match
            axis = np.argmax(v != np.floor(v), axis=1) if len(v) else np.zeros(0, dtype=int)
            for row, a in zip(v, axis):
                assert row[a] == 0.5
                others = [b for b in range(3) if b != a]
                assert not all(row[b] == at[b] for b in others), (case, corner, row)
            # the edges that do not touch the corner keep their vertices
            keep = [row for row in full_v if not all(row[b] == at[b] for b in range(3) if row[b] != 0.5)]
            assert len(v) == len(keep)


def test_partly_observed_noise_has_only_whole_cells():
    shape = (5, 6, 7)
    vol = inputs.noise(shape)
    seen = np.random.default_rng(5).random(shape) >= 0.2
    vol_hidden = np.where(seen, vol, np.nan).astype(F32)
    v, t = tm.marching_cubes(vol_hidden, 0.5, observed=seen)
    V = len(v)
    assert V > 50 and len(t) > 20 and 0.1 < (~seen).mean() < 0.3
    assert t.dtype == np.int32 and bool((t >= 0).all()) and bool((t < V).all())
    assert bool(np.isfinite(v).all())
    # the vertices' owning edges, from the definition: ascending (flat index of p, axis), both ends observed and on different sides
    above = (vol > 0.5) & seen
    keys = []
    strides = (shape[1] * shape[2], shape[2], 1)
    for p in range(vol.size):
        ijk = np.unravel_index(p, shape)
        for a in range(3):
            if ijk[a] + 1 < shape[a]:
                q = p + strides[a]
                if seen.flat[p] and seen.flat[q] and above.flat[p] != above.flat[q]:
                    keys.append((p, a))
    assert len(keys) == V
    owner = tm.case_table()[0]                              # MC_EDGE_OWNER: di, dj, dk, axis of the twelve edges
    edge_cells = {}                                         # (p, axis) -> the cells (lowest corner, flat) that have it as an edge
    for e in range(12):
        di, dj, dk, a = (int(x) for x in owner[e])
        edge_cells.setdefault(a, []).append(di * strides[0] + dj * strides[1] + dk)

    def whole(cell):
        i, j, k = np.unravel_index(cell, shape)
        return i + 1 < shape[0] and j + 1 < shape[1] and k + 1 < shape[2] and bool(seen[i:i + 2, j:j + 2, k:k + 2].all())

    for tri in t:
        cells = None
        for vid in tri:
            p, a = keys[vid]
            mine = {p - off for off in edge_cells[a] if p - off >= 0}
            cells = mine if cells is None else cells & mine
        assert cells and any(whole(c) for c in cells), tri
    # and the mask removed something: the unmasked mesh of the same (finite) volume has more triangles
    assert len(tm.marching_cubes(vol, 0.5)[1]) > len(t)


def test_unobserved_values_never_reach_a_result():
    shape = (17, 9, 33)
    vol = inputs.smooth(shape)
    w = inputs.weights(shape, 0.2, 0.0)
    seen = inputs.observed(w, 0.0)
    meshes = [tm.marching_cubes(np.where(seen, vol, F32(fill)).astype(F32), 0.0, observed=seen) for fill in (np.nan, np.inf, 1e30, -1e30)]
    assert len(meshes[0][0]) > 100
    for v, t in meshes[1:]:
        assert np.array_equal(bits(v), bits(meshes[0][0])) and np.array_equal(t, meshes[0][1])


# ----------------------------------------------------------------------------------------------- vertex colours
def test_vertex_colours_blend_the_two_ends_of_an_edge():
    rng = np.random.default_rng(3)
    color = torch.from_numpy((rng.random((4, 5, 6, 3)) * 255).astype(F32))
    v = torch.tensor([[1.0, 2.0, 3.25], [0.5, 4.0, 5.0], [3.0, 1.75, 0.0], [3.0, 4.0, 5.0], [0.0, 0.0, 0.0], [2.0, 4.0, 4.0],
                      [float("nan"), 1.0, 1.0], [1.0, float("inf"), 1.0]])
    got = tt.vertex_colors(color, v).numpy()
    c = color.numpy()
    blend = lambda a, b, f: ((F32(1) - F32(f)) * a + F32(f) * b) / F32(255)      # noqa: E731
    assert np.array_equal(bits(got[0]), bits(blend(c[1, 2, 3], c[1, 2, 4], 0.25)))
    assert np.array_equal(bits(got[1]), bits(blend(c[0, 4, 5], c[1, 4, 5], 0.5)))
    assert np.array_equal(bits(got[2]), bits(blend(c[3, 1, 0], c[3, 2, 0], 0.75)))
    assert np.array_equal(bits(got[3]), bits(c[3, 4, 5] / F32(255)))              # the last lattice point: t = 1 on every axis
    assert np.array_equal(bits(got[4]), bits(c[0, 0, 0] / F32(255)))
    assert np.array_equal(bits(got[5]), bits(c[2, 4, 4] / F32(255)))
    assert bool((got[6:] == 0).all())


# ----------------------------------------------------------------------------------------------- the sphere
def test_sphere_scene_on_the_restatement():
    """The issue's sphere: radius 0.3 in a 48^3 volume of voxel 1/48, six axis-aligned cameras at distance 2, analytic depth at 64 x 64,
    the exporter's sdf_trunc = 0.03.  Every vertex lies within sdf_trunc of the sphere and every triangle index names a vertex.  The
    mesh is NOT closed: measured 2232 boundary edges (edges in exactly one triangle) on 6864 triangles, asserted as measured.  sdf_trunc
    is 1.44 voxels here, so behind the surface only the first one or two voxels carry weight, and a cell that the surface crosses near
    its front has a back corner deeper than that: unobserved, hence no triangles (Open3D's all-eight-corners rule).  With sdf_trunc at
    4 voxels the same scene gives 0 boundary edges, asserted below as the control."""
    s = inputs.sphere_scene()
    def fuse(trunc):
        tsdf, weight, color = torch.zeros(s["dims"]), torch.zeros(s["dims"]), torch.zeros(s["dims"] + (3,))
        tt.integrate(tsdf, weight, color, s["origin"], s["voxel"], opencv_w2c(s["poses"]), s["K"], s["depth"], s["rgb"],
                     tt.ray_scale(s["K"], s["height"], s["width"]), trunc, 20.0, 0.5)
        return tt.extract_mesh(tsdf, weight, color, s["origin"], s["voxel"]), weight

    (vertices, triangles, colors), weight = fuse(0.03)
    V, T = len(vertices), len(triangles)
    r = np.linalg.norm(vertices.numpy(), axis=1)
    unreferenced = V - len(np.unique(triangles.numpy()))
    edges = inputs.boundary_edges(triangles.numpy())
    print(f"sphere: V {V} T {T}, worst |r - 0.3| {np.abs(r - 0.3).max():.4f}, boundary edges {edges}, unreferenced vertices {unreferenced}, "
          f"observed voxels {int((weight > 0).sum())}, max weight {float(weight.max())}")
    assert V > 3000 and T > 5000
    assert float(np.abs(r - inputs.SPHERE_RADIUS).max()) <= 0.03
    assert bool((triangles.numpy() >= 0).all()) and bool((triangles.numpy() < V).all())
    assert colors.dtype == torch.float32 and tuple(colors.shape) == (V, 3) and 0.0 <= float(colors.min()) and float(colors.max()) <= 1.0
    assert edges == 2232
    (_, closed, _), _ = fuse(4.0 * s["voxel"])
    assert inputs.boundary_edges(closed.numpy()) == 0
