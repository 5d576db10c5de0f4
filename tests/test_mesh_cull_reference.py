"""The PyTorch restatement of the mesh visibility culling (dn_splatter_amd/torch_mesh_cull.py) on the CPU:

  * its votes equal the reference's own outputs (tests/golden/reference_mesh_cull.npz, made by
    tests/golden/make_reference_mesh_cull_golden.py from cull_from_one_pose / get_grid_culling_pattern as they stand), exactly, for the
    three flag combinations, and accumulated over camera batches;
  * its cut on those votes equals a numpy restatement of eval_mesh_vis_cull.py:251-264 written here;
  * its depth render equals an independent per-pixel Moeller-Trumbore intersection in float64 (tests/_mesh_cull_inputs.py) on random
    scenes of 1, 64 and 300 triangles on 64 x 48, many crossing z = 0: the same coverage on every pixel outside the rounding envelope
    (a pixel is in it when min |E_i| <= 2^-40 sum |c_i| for some triangle; at most 1 % of the pixels may be), and the same depth within
    DEPTH_REL on the float64 z before its rounding.  DEPTH_REL = 2.7e-13 = 4 x the worst case measured on these six scenes against
    that formula, 6.6e-14 relative (T = 64, seed 4: triangles seen at a grazing angle, where D / S and the barycentric form are both
    ill-conditioned; a lone triangle stays under 2.4e-15, and the worst of sixty other seeds was 1.1e-13).  The float32 maps are held
    to the float32 rounding of the independent depth: equal, or one float32 ulp apart where the two float64 values straddle a
    rounding boundary, and in every case within half an ulp plus DEPTH_REL of the un-rounded independent depth;
  * known answers: a fronto-parallel triangle, a tilted plane's closed form, a quad split along a diagonal through pixel centres, the
    triangles that cover nothing."""
import os

import numpy as np
import pytest
import torch

import _mesh_cull_inputs as inputs

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = {"tt": (True, True), "tf": (True, False), "ft": (False, True)}        # (remove_missing_depth, remove_occlusion)
H64, W64 = 48, 64
K64 = np.array([[40.0, 0.0, 32.0], [0.0, 40.0, 24.0], [0.0, 0.0, 1.0]])
DEPTH_REL = 4 * 6.6e-14
ULP32 = 2.0 ** -23


@pytest.fixture(scope="module")
def tmc():
    from dn_splatter_amd import torch_mesh_cull

    return torch_mesh_cull


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "reference_mesh_cull.npz")))


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def numpy_cut(vertices, triangles, obs, invalid):
    """eval_mesh_vis_cull.py:251-264 with remove_unreferenced_vertices spelled out."""
    o, i = obs[triangles].astype(np.float64), invalid[triangles].astype(np.float64)
    valid = (o > 3).any(axis=1) & ~(i > 0.7 * o).all(axis=1)
    kept = triangles[valid]
    used = np.zeros(len(vertices), dtype=bool)
    used[kept.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    return vertices[used], new_id[kept].astype(np.int32).reshape(-1, 3)


@pytest.mark.parametrize("name", sorted(FLAGS))
def test_votes_equal_the_reference(tmc, golden, name):
    missing, occlusion = FLAGS[name]
    g = golden
    obs, invalid = tmc.vertex_visibility(t(g["vertices"]), g["poses"], g["K"], int(g["height"]), int(g["width"]), t(g["rendered_depth"]),
                                         t(g["depth_gt"]), remove_missing_depth=missing, remove_occlusion=occlusion)
    assert obs.dtype == torch.int32 and invalid.dtype == torch.int32
    assert np.array_equal(obs.numpy(), g["obs_" + name]) and np.array_equal(invalid.numpy(), g["invalid_" + name])
    assert 0 < int((obs > 3).sum()) < obs.numel()


def test_votes_accumulate_over_camera_batches(tmc, golden):
    g = golden
    H, W = int(g["height"]), int(g["width"])
    obs = invalid = None
    for s in range(0, 8, 3):
        obs, invalid = tmc.vertex_visibility(t(g["vertices"]), g["poses"][s:s + 3], g["K"], H, W, t(g["rendered_depth"][s:s + 3]),
                                             t(g["depth_gt"][s:s + 3]), obs=obs, invalid=invalid)
    assert np.array_equal(obs.numpy(), g["obs_tt"]) and np.array_equal(invalid.numpy(), g["invalid_tt"])


def test_the_rendered_depth_of_the_fixture_is_the_restatements(tmc, golden):
    g = golden
    depth = tmc.render_mesh_depth(t(g["vertices"]), t(g["triangles"]), g["poses"], g["K"], int(g["height"]), int(g["width"]))
    assert depth.dtype == torch.float32 and np.array_equal(depth.numpy(), g["rendered_depth"])


@pytest.mark.parametrize("name", sorted(FLAGS))
def test_cut_equals_the_numpy_restatement_of_the_rule(tmc, golden, name):
    g = golden
    obs, invalid = g["obs_" + name], g["invalid_" + name]
    want_v, want_t = numpy_cut(g["vertices"], g["triangles"], obs, invalid)
    got_v, got_t = tmc.cut_mesh(t(g["vertices"]), t(g["triangles"]), t(obs), t(invalid))
    assert 0 < len(want_t) < len(g["triangles"]) and 0 < len(want_v) < len(g["vertices"])
    assert got_t.dtype == torch.int32 and np.array_equal(got_t.numpy(), want_t) and np.array_equal(got_v.numpy(), want_v)
    # every kept triangle is the original one, vertex for vertex
    assert np.array_equal(got_v.numpy()[got_t.numpy().astype(np.int64)], g["vertices"][want_t_original(g, obs, invalid)])


def want_t_original(g, obs, invalid):
    o, i = obs[g["triangles"]].astype(np.float64), invalid[g["triangles"]].astype(np.float64)
    return g["triangles"][(o > 3).any(axis=1) & ~(i > 0.7 * o).all(axis=1)].astype(np.int64)


def test_cut_keep_all_keep_none_and_bad_indices(tmc):
    vertices = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    triangles = torch.tensor([[0, 1, 2], [2, 3, 4], [1, 7, 2], [-1, 0, 1]], dtype=torch.int32)
    zeros = torch.zeros(5, dtype=torch.int32)
    v, f = tmc.cut_mesh(vertices, triangles, zeros + 4, zeros)
    assert torch.equal(v, vertices) and torch.equal(f, triangles[:2])            # an index outside [0, V) is never kept
    v, f = tmc.cut_mesh(vertices, triangles, zeros + 3, zeros)                    # obs > 3 fails everywhere
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and f.dtype == torch.int32
    v, f = tmc.cut_mesh(vertices, triangles, zeros + 10, zeros + 7)               # 7 > 0.7 * 10 is false in double: 7.0 > 7.000000000000001
    assert f.shape[0] == 2
    v, f = tmc.cut_mesh(vertices, triangles, zeros + 10, zeros + 8)
    assert f.shape[0] == 0
    obs = torch.tensor([4, 0, 0, 0, 0], dtype=torch.int32)
    v, f = tmc.cut_mesh(vertices, triangles, obs, zeros)                          # one observed vertex keeps its triangle only
    assert torch.equal(f, torch.tensor([[0, 1, 2]], dtype=torch.int32)) and torch.equal(v, vertices[:3])


def test_pose_helper_inverts_the_flipped_pose(tmc):
    poses = inputs.room_poses()
    w2c = tmc.opencv_w2c(poses).numpy().reshape(-1, 3, 4)
    for pose, m in zip(poses, w2c):
        R, tr = inputs.opencv_view(pose)
        assert np.allclose(m[:, :3], R, rtol=0, atol=1e-14) and np.allclose(m[:, 3], tr, rtol=0, atol=1e-14)
    assert tuple(tmc.opencv_w2c(poses[0]).shape) == (1, 12)


# ---- the depth render against an independent intersection ---------------------------------------------------------------------------

def envelope(tmc, vertices, triangles, pose):
    """[H,W] bool: min |E_i| <= 2^-40 sum |c_i| for some triangle."""
    ok, tri = tmc.covering_triangles(t(vertices), t(triangles))
    x = t(vertices).double()[tri][ok]
    c0, c1, c2, n, D = tmc.triangle_coefficients(tmc.opencv_w2c(pose)[0], x)
    dx, dy = tmc.pixel_rays(K64, H64, W64, "cpu")
    e = torch.stack([(q[:, 0, None, None] * dx[None, None, :] + q[:, 1, None, None] * dy[None, :, None]) + q[:, 2, None, None]
                     for q in (c0, c1, c2)])
    scale = (c0.abs().sum(dim=1) + c1.abs().sum(dim=1) + c2.abs().sum(dim=1))[:, None, None]
    return (e.abs().min(dim=0).values <= 2.0 ** -40 * scale).any(dim=0).numpy()


@pytest.mark.parametrize("n_triangles,seed", [(1, 2), (1, 8), (64, 3), (64, 4), (300, 5), (300, 6)])
def test_depth_render_equals_moller_trumbore(tmc, n_triangles, seed):
    vertices, triangles, pose = inputs.random_scene(n_triangles, seed)
    crossing = (vertices.reshape(-1, 3, 3)[:, :, 2] > 0.21).any(axis=1)
    assert n_triangles == 1 or crossing.sum() > n_triangles // 5                  # triangles with a vertex behind the camera
    got = tmc.render_mesh_depth(t(vertices), t(triangles), pose, K64, H64, W64).numpy()[0]
    want, covered = inputs.moller_trumbore_depth(vertices, triangles, pose[0], K64, H64, W64)
    env = envelope(tmc, vertices, triangles, pose)
    assert env.mean() <= 0.01
    assert n_triangles == 1 or covered.mean() > 0.2
    assert np.array_equal((got > 0)[~env], covered[~env])
    both = (got > 0) & covered & ~env
    want32 = want[both].astype(np.float32).astype(np.float64)
    err = np.abs(got[both].astype(np.float64) - want32) / want32
    # where the two float64 depths straddle a float32 rounding boundary the roundings are one ulp apart: those pixels are held to the
    # float64 bound through the un-rounded independent depth
    far = err > 0
    assert np.all(err[far] <= ULP32 * (1 + 1e-6))
    assert np.all(np.abs(got[both].astype(np.float64) - want[both]) / want[both] <= 0.5 * ULP32 * (1 + 1e-6) + DEPTH_REL)
    print(f"[mesh depth] T={n_triangles}: {int(both.sum())} pixels, {int(far.sum())} straddle a float32 boundary, envelope {int(env.sum())}")


def test_float64_depth_agrees_with_moller_trumbore_before_rounding(tmc):
    """The float64 z of the restatement's own formula, before its float32 rounding, against the independent depth: DEPTH_REL."""
    worst = 0.0
    for n_triangles, seed in [(1, 2), (1, 8), (64, 3), (64, 4), (300, 5), (300, 6)]:
        vertices, triangles, pose = inputs.random_scene(n_triangles, seed)
        want, covered = inputs.moller_trumbore_depth(vertices, triangles, pose[0], K64, H64, W64)
        x = t(vertices).double()[t(triangles).long()]
        c0, c1, c2, n, D = tmc.triangle_coefficients(tmc.opencv_w2c(pose)[0], x)
        dx, dy = tmc.pixel_rays(K64, H64, W64, "cpu")
        e = [(q[:, 0, None, None] * dx[None, None, :] + q[:, 1, None, None] * dy[None, :, None]) + q[:, 2, None, None] for q in (c0, c1, c2, n)]
        inside = (((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))) & (e[3] != 0)
        z = D[:, None, None] / e[3]
        z = torch.where(inside & (z >= 0.01) & (z <= 10.0), z, torch.full_like(z, float("inf"))).min(dim=0).values.numpy()
        both = np.isfinite(z) & covered & ~envelope(tmc, vertices, triangles, pose)
        worst = max(worst, float((np.abs(z[both] - want[both]) / want[both]).max()))
    print(f"[mesh depth] worst relative float64 difference {worst:.3e}")
    assert worst <= DEPTH_REL


# ---- known answers -----------------------------------------------------------------------------------------------------------------

IDENTITY = np.eye(4)[None]                                                       # OpenGL: the camera at the origin looks down -z
K16 = np.array([[8.0, 0.0, 8.0], [0.0, 8.0, 8.0], [0.0, 0.0, 1.0]])              # 16 x 16 pixels, d = (u + 0.5 - 8) / 8


def render16(tmc, vertices, triangles, **kw):
    return tmc.render_mesh_depth(torch.tensor(vertices, dtype=torch.float32), torch.tensor(triangles, dtype=torch.int32), IDENTITY, K16, 16,
                                 16, **kw).numpy()[0]


def test_fronto_parallel_triangle_is_exactly_two(tmc):
    # OpenCV camera space: x right, y down, z forward = -z of the world.  Vertices at z = 2 project to pixels (4,4), (12,4), (4,12):
    # x = (u - 8) / 8 * 2.  The hypotenuse u + v = 16 passes between pixel centres (u + 0.5) + (v + 0.5) = 16 <=> u + v = 15 is ON it.
    depth = render16(tmc, [[-1, 1, -2], [1, 1, -2], [-1, -1, -2]], [[0, 1, 2]])
    inside = {(u, v) for u in range(16) for v in range(16) if u >= 4 and v >= 4 and u + v <= 15}
    hand_listed = {(4, 4), (5, 4), (11, 4), (4, 11), (7, 8), (8, 7), (4, 5), (10, 5), (6, 9)}
    assert hand_listed <= inside
    for u in range(16):
        for v in range(16):
            assert depth[v, u] == (2.0 if (u, v) in inside else 0.0), (u, v)


def test_tilted_plane_gives_its_closed_form(tmc):
    # the plane z = 3 + x / 2 (OpenCV axes) through a triangle that covers the whole frame: z = 3 / (1 - d.x / 2)
    cv = np.array([[-40.0, -30.0, 0.0], [40.0, -30.0, 0.0], [0.0, 60.0, 0.0]])
    cv[:, 2] = 3 + cv[:, 0] / 2
    world = cv * np.array([1.0, -1.0, -1.0])
    depth = render16(tmc, world.tolist(), [[0, 1, 2]], zfar=100.0)
    dx = (np.arange(16) + 0.5 - 8) / 8
    want = np.broadcast_to(3.0 / (1.0 - dx / 2), (16, 16))
    assert np.all(depth > 0) and np.allclose(depth, want, rtol=2 * ULP32, atol=0)


def test_diagonal_split_quad_has_no_hole_and_both_windings_agree(tmc):
    # the quad [4,12] x [4,12] pixels at z = 2, split along the diagonal u = v through the pixel centres (k + 0.5, k + 0.5)
    quad = [[-1.0, 1.0, -2.0], [1.0, 1.0, -2.0], [1.0, -1.0, -2.0], [-1.0, -1.0, -2.0]]
    a = render16(tmc, quad, [[0, 1, 2], [0, 2, 3]])
    b = render16(tmc, quad, [[0, 2, 1], [0, 3, 2]])
    c = render16(tmc, quad, [[0, 2, 3], [0, 1, 2]])
    want = np.zeros((16, 16), dtype=np.float32)
    want[4:12, 4:12] = 2.0
    assert np.array_equal(a, want) and np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(a, c)
    for k in range(4, 12):                                                        # each half alone claims the diagonal too
        assert render16(tmc, quad, [[0, 1, 2]])[k, k] == 2.0 and render16(tmc, quad, [[0, 2, 3]])[k, k] == 2.0


def test_winding_does_not_change_a_bit_on_a_random_scene(tmc):
    vertices, triangles, pose = inputs.random_scene(64, 9)
    a = tmc.render_mesh_depth(t(vertices), t(triangles), pose, K64, H64, W64)
    b = tmc.render_mesh_depth(t(vertices), t(triangles[:, [0, 2, 1]].copy()), pose, K64, H64, W64)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and int((a > 0).sum()) > 500


def test_triangles_that_cover_nothing(tmc):
    nan, inf = float("nan"), float("inf")
    front = [[-1.0, 1.0, -2.0], [1.0, 1.0, -2.0], [-1.0, -1.0, -2.0]]
    assert render16(tmc, front, [[0, 1, 2]]).any()
    assert not render16(tmc, [[-1, 1, 2], [1, 1, 2], [-1, -1, 2]], [[0, 1, 2]]).any()          # behind the camera
    assert not render16(tmc, [[-1, 1, -11], [1, 1, -11], [-1, -1, -11]], [[0, 1, 2]]).any()    # beyond zfar
    assert not render16(tmc, front, [[0, 1, 2]], zfar=1.5).any()
    assert not render16(tmc, [[-1, 1, -2], [0, 0, -2], [1, -1, -2]], [[0, 1, 2]]).any()        # collinear: no area
    assert not render16(tmc, front, [[0, 1, 1]]).any()                                         # a repeated index
    assert not render16(tmc, front, [[0, 1, 3]]).any() and not render16(tmc, front, [[-1, 1, 2]]).any()
    assert not render16(tmc, [[-1, 1, nan], [1, 1, -2], [-1, -1, -2]], [[0, 1, 2]]).any()
    assert not render16(tmc, [[-1, inf, -2], [1, 1, -2], [-1, -1, -2]], [[0, 1, 2]]).any()
    # and they take nothing away from a triangle that does cover
    both = render16(tmc, front + [[-1, 1, nan]], [[0, 1, 3], [3, 3, 1], [0, 1, 2], [0, 1, 9]])
    assert np.array_equal(both, render16(tmc, front, [[0, 1, 2]]))


def test_a_triangle_crossing_the_near_plane_is_cut_at_znear_without_clipping(tmc):
    # the plane y = 0.5 (OpenCV) from z = -1 behind the camera to z = 4: hits have z = 0.5 / d.y, accepted from znear on
    cv = np.array([[-30.0, 0.5, -1.0], [30.0, 0.5, -1.0], [0.0, 0.5, 4.0]])
    world = (cv * np.array([1.0, -1.0, -1.0])).tolist()
    dy = (np.arange(16) + 0.5 - 8) / 8
    for znear, first_rejected in ((0.01, 16), (0.6, 15)):                         # row 15 has z = 0.5333 < 0.6
        depth = render16(tmc, world, [[0, 1, 2]], znear=znear)
        assert not depth[:8].any()                                                # d.y < 0 looks away from the plane
        col = depth[:, 8]                                                         # d.x = 1/16: inside while z/16 <= 6 (4 - z), z <= 3.96
        assert col[8] == 0.0                                                      # z = 8 lies past the far vertex
        for v in range(9, 16):
            z = 0.5 / dy[v]
            assert (col[v] == 0.0) if v >= first_rejected else abs(col[v] - z) <= ULP32 * z, (znear, v)
