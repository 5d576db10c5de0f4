"""The mesh visibility culling on the MI355X (csrc/meshcull.hip through dn_splatter_amd/mesh_cull.py) against the PyTorch restatement
(dn_splatter_amd/torch_mesh_cull.py) run in float64 on the device, and against the reference's recorded votes
(tests/golden/reference_mesh_cull.npz).

Everything here is exact (``torch.equal``): the depth maps, because both sides perform the same float64 operations in the same order
and take the same minimum of float32 values; the votes and the cut, because they are integers.  No tolerance applies anywhere.

Sizes.  Depth: T in {1, 63, 64, 65, 257} triangles is one lane, the wave edge and two workgroups; frames 37 x 29 (odd, no multiple of
anything) and 64 x 48; C in {1, 3} cameras (the grid's second axis); the random triangles are of three sizes, so that both the
per-lane walk (boxes of at most 16 pixels) and the cooperative walk run, and a third of them cross z = 0.  Votes: V in {1, 63, 64, 65,
1000}, C in {1, 5}.  Cut: T in {1, 255, 256, 257} is the workgroup edge, and 262144 + 300 is one triangle block past a single trip of
the one-workgroup scan (256 threads x 4 block counts x 256 triangles)."""
import os

import numpy as np
import pytest
import torch

import _mesh_cull_inputs as inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = {"tt": (True, True), "tf": (True, False), "ft": (False, True)}        # (remove_missing_depth, remove_occlusion)
SCAN_TRIP = 256 * 4 * 256


@pytest.fixture(scope="module")
def mc():
    from dn_splatter_amd import mesh_cull

    return mesh_cull


@pytest.fixture(scope="module")
def tmc():
    from dn_splatter_amd import torch_mesh_cull

    return torch_mesh_cull


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "reference_mesh_cull.npz")))


@pytest.fixture(scope="module")
def room(golden):
    g = golden
    return dict(vertices=dev(g["vertices"]), triangles=dev(g["triangles"]), poses=g["poses"], K=g["K"], H=int(g["height"]),
                W=int(g["width"]), rendered=dev(g["rendered_depth"]), depth_gt=dev(g["depth_gt"]))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def frame_K(H, W):
    return np.array([[0.625 * W, 0.0, 0.5 * W], [0.0, 0.625 * W, 0.5 * H], [0.0, 0.0, 1.0]])


def poses_for(C):
    eyes = [(0.13, -0.07, 0.21), (-0.6, 0.2, 0.4), (0.5, -0.3, -0.2)]
    return np.stack([inputs.look_at(e, (0.3, 0.1, -5.0)) for e in eyes[:C]])


# ---- depth -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", [(29, 37), (48, 64)])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
def test_depth_equals_the_restatement(mc, tmc, T, H, W, C):
    vertices, triangles, _ = inputs.random_scene(T, 100 + T)
    vertices, triangles, poses, K = dev(vertices), dev(triangles), poses_for(C), frame_K(H, W)
    got = mc.render_mesh_depth(vertices, triangles, poses, K, H, W)
    want = tmc.render_mesh_depth(vertices, triangles, poses, K, H, W)
    assert got.dtype == torch.float32 and tuple(got.shape) == (C, H, W)
    assert torch.equal(bits(got), bits(want))
    assert T == 1 or int((got > 0).sum()) > C * H * W // 10


def filling_scene():
    """65 triangles: number 30 fills the 64 x 48 frame at z = 4; the other 64, a third of a pixel wide at z = 2, each sit on the ray of
    a pixel centre of row 7 + k // 16, so that the same wave walks one large box cooperatively and 64 small ones lane by lane."""
    H, W = 48, 64
    K = frame_K(H, W)
    tris = []
    for k in range(64):
        u, v = 3 + 3 * (k % 16) + 0.5, 7 + 9 * (k // 16) + 0.5
        cx, cy = (u - K[0, 2]) / K[0, 0] * 2.0, (v - K[1, 2]) / K[1, 1] * 2.0
        r = 0.3 / K[0, 0] * 2.0
        tris.append([[cx - r, cy - r, 2.0], [cx + r, cy - r, 2.0], [cx, cy + r, 2.0]])
    tris.insert(30, [[-40.0, -30.0, 4.0], [40.0, -30.0, 4.0], [0.0, 60.0, 4.0]])
    cv = np.asarray(tris).reshape(-1, 3)
    world = (cv * np.array([1.0, -1.0, -1.0])).astype(np.float32)                 # OpenCV camera axes -> the OpenGL identity pose
    return world, np.arange(len(world), dtype=np.int32).reshape(-1, 3), np.eye(4)[None], K, H, W


def test_depth_one_filling_triangle_and_64_subpixel_ones_in_one_wave(mc, tmc):
    vertices, triangles, pose, K, H, W = filling_scene()
    got = mc.render_mesh_depth(dev(vertices), dev(triangles), pose, K, H, W)
    want = tmc.render_mesh_depth(dev(vertices), dev(triangles), pose, K, H, W)
    assert torch.equal(bits(got), bits(want))
    assert int((got == 4.0).sum()) == H * W - 64 and int((got == 2.0).sum()) == 64          # every small one wins its pixel


def test_depth_of_a_triangle_crossing_the_near_plane(mc, tmc):
    cv = np.array([[-30.0, 0.5, -1.0], [30.0, 0.5, -1.0], [0.0, 0.5, 4.0]])
    vertices = dev((cv * np.array([1.0, -1.0, -1.0])).astype(np.float32))
    triangles = dev(np.array([[0, 1, 2]], dtype=np.int32))
    for znear in (0.01, 0.6):
        got = mc.render_mesh_depth(vertices, triangles, np.eye(4)[None], frame_K(48, 64), 48, 64, znear=znear)
        want = tmc.render_mesh_depth(vertices, triangles, np.eye(4)[None], frame_K(48, 64), 48, 64, znear=znear)
        assert torch.equal(bits(got), bits(want))
        assert not bool(got[0, :24].any()) and bool((got[0, 24:] > 0).any()) and float(got[got > 0].min()) >= np.float32(znear)


def test_depth_does_not_depend_on_triangle_order_or_winding(mc):
    vertices, triangles, _ = inputs.random_scene(257, 7)
    poses, K = poses_for(3), frame_K(48, 64)
    base = mc.render_mesh_depth(dev(vertices), dev(triangles), poses, K, 48, 64)
    perm = np.random.default_rng(0).permutation(len(triangles))
    assert torch.equal(bits(base), bits(mc.render_mesh_depth(dev(vertices), dev(triangles[perm]), poses, K, 48, 64)))
    assert torch.equal(bits(base), bits(mc.render_mesh_depth(dev(vertices), dev(triangles[:, [0, 2, 1]]), poses, K, 48, 64)))
    assert torch.equal(bits(base), bits(mc.render_mesh_depth(dev(vertices), dev(triangles), poses, K, 48, 64)))
    assert int((base > 0).sum()) > 3 * 48 * 64 // 10


def test_depth_rows_that_cover_nothing(mc, tmc):
    nan, inf = float("nan"), float("inf")
    front = [[-1.0, 1.0, -2.0], [1.0, 1.0, -2.0], [-1.0, -1.0, -2.0]]
    vertices = dev(np.array(front + [[-1.0, 1.0, nan], [0.5, inf, -2.0], [0.0, 0.0, -2.0]], dtype=np.float32))
    bad = [[0, 1, 6], [-1, 1, 2], [0, 1, 1], [2, 2, 2], [0, 1, 3], [0, 4, 2], [0, 5, 2 ** 31 - 1]]
    collinear = [[0, 5, 0], [1, 5, 2]]                                            # (1,1), (0,0), (-1,-1) lie on a line: no area
    K, pose = frame_K(29, 37), np.eye(4)[None]
    good = mc.render_mesh_depth(vertices, dev(np.array([[0, 1, 2]], dtype=np.int32)), pose, K, 29, 37)
    assert int((good == 2.0).sum()) > 50
    for rows in (bad, collinear):
        none = mc.render_mesh_depth(vertices, dev(np.array(rows, dtype=np.int32)), pose, K, 29, 37)
        assert not bool(none.any())
    mixed = dev(np.array(bad[:3] + [[0, 1, 2]] + bad[3:] + collinear, dtype=np.int32))
    got = mc.render_mesh_depth(vertices, mixed, pose, K, 29, 37)
    assert torch.equal(bits(got), bits(good)) and torch.equal(bits(got), bits(tmc.render_mesh_depth(vertices, mixed, pose, K, 29, 37)))


def test_depth_into_a_callers_buffer_and_the_counters(mc):
    vertices, triangles, _ = inputs.random_scene(65, 11)
    poses, K = poses_for(3), frame_K(29, 37)
    buffer = torch.full((4 * 29 * 37,), -1.0, dtype=torch.float32, device=DEV)
    stats = torch.zeros(3, dtype=torch.int64, device=DEV)
    got = mc.render_mesh_depth(dev(vertices), dev(triangles), poses, K, 29, 37, out=buffer, stats=stats)
    assert got.data_ptr() == buffer.data_ptr() and torch.equal(got, mc.render_mesh_depth(dev(vertices), dev(triangles), poses, K, 29, 37))
    assert bool((buffer[3 * 29 * 37:] == -1.0).all())                             # nothing past C H W is touched
    setups, fragments, atomics = stats.tolist()
    assert 0 < setups <= 3 * 65 and fragments >= int((got > 0).sum()) and 0 < atomics <= fragments


# ---- votes -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(FLAGS))
def test_votes_equal_the_reference(mc, golden, room, name):
    missing, occlusion = FLAGS[name]
    r = room
    obs, invalid = mc.vertex_visibility(r["vertices"], r["poses"], r["K"], r["H"], r["W"], r["rendered"], r["depth_gt"],
                                        remove_missing_depth=missing, remove_occlusion=occlusion)
    assert obs.dtype == torch.int32 and invalid.dtype == torch.int32
    assert np.array_equal(obs.cpu().numpy(), golden["obs_" + name]) and np.array_equal(invalid.cpu().numpy(), golden["invalid_" + name])


def test_rendered_depth_of_the_room_is_the_fixtures(mc, room):
    r = room
    got = mc.render_mesh_depth(r["vertices"], r["triangles"], r["poses"], r["K"], r["H"], r["W"])
    assert torch.equal(bits(got), bits(r["rendered"]))


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1000])
def test_votes_equal_the_restatement(mc, tmc, room, V, C):
    r = room
    rng = np.random.default_rng(V + C)
    points = dev(rng.uniform([-2.5, -1.2, -2.5], [2.5, 1.2, 2.5], (V, 3)).astype(np.float32))
    args = (points, r["poses"][:C], r["K"], r["H"], r["W"], r["rendered"][:C], r["depth_gt"][:C])
    for missing, occlusion in list(FLAGS.values()) + [(False, False)]:
        got = mc.vertex_visibility(*args, remove_missing_depth=missing, remove_occlusion=occlusion)
        want = tmc.vertex_visibility(*args, remove_missing_depth=missing, remove_occlusion=occlusion)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if V >= 63:
        assert 0 < int(got[0].sum())


@pytest.mark.parametrize("batch", [1, 2, 8, 9])
def test_votes_accumulate_identically_over_camera_batches(mc, golden, room, batch):
    r = room
    obs = torch.zeros(r["vertices"].shape[0], dtype=torch.int32, device=DEV)
    invalid = torch.zeros_like(obs)
    for s in range(0, 8, batch):
        out = mc.vertex_visibility(r["vertices"], r["poses"][s:s + batch], r["K"], r["H"], r["W"], r["rendered"][s:s + batch],
                                   r["depth_gt"][s:s + batch], obs=obs, invalid=invalid)
        assert out[0] is obs and out[1] is invalid
    assert np.array_equal(obs.cpu().numpy(), golden["obs_tt"]) and np.array_equal(invalid.cpu().numpy(), golden["invalid_tt"])


# ---- cut ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", ["all", "none", "alternate", "shared"])
@pytest.mark.parametrize("T", [1, 255, 256, 257, SCAN_TRIP + 300])
def test_cut_equals_the_restatement(mc, tmc, T, pattern):
    g = torch.Generator().manual_seed(T)
    if pattern == "shared":                                                       # random triangles over shared vertices, random votes
        V = max(T // 2, 3)
        triangles = torch.randint(0, V, (T, 3), generator=g, dtype=torch.int32)
        obs = torch.randint(0, 9, (V,), generator=g, dtype=torch.int32)
        invalid = torch.randint(0, 9, (V,), generator=g, dtype=torch.int32)
    else:                                                                         # triangle t owns vertices 3 t .. 3 t + 2
        V = 3 * T
        triangles = torch.arange(V, dtype=torch.int32).reshape(T, 3)
        keep = {"all": torch.ones(T, dtype=torch.bool), "none": torch.zeros(T, dtype=torch.bool), "alternate": torch.arange(T) % 2 == 0}[pattern]
        obs = (keep.to(torch.int32) * 4).repeat_interleave(3)
        invalid = torch.zeros(V, dtype=torch.int32)
    vertices = torch.rand(V, 3, generator=g)
    vertices, triangles, obs, invalid = (x.to(DEV) for x in (vertices, triangles, obs, invalid))
    got_v, got_t = mc.cut_mesh(vertices, triangles, obs, invalid)
    want_v, want_t = tmc.cut_mesh(vertices, triangles, obs, invalid)
    assert got_v.dtype == torch.float32 and got_t.dtype == torch.int32
    assert tuple(got_v.shape) == tuple(want_v.shape) and tuple(got_t.shape) == tuple(want_t.shape)
    assert torch.equal(got_v, want_v) and torch.equal(got_t, want_t)
    if pattern == "none":
        assert tuple(got_v.shape) == (0, 3) and tuple(got_t.shape) == (0, 3)
    if pattern == "all":
        assert torch.equal(got_v, vertices) and torch.equal(got_t, triangles)
    if pattern == "alternate":
        assert got_t.shape[0] == (T + 1) // 2


def test_cut_thresholds_and_bad_indices(mc, tmc):
    vertices = torch.arange(15, dtype=torch.float32, device=DEV).reshape(5, 3)
    triangles = torch.tensor([[0, 1, 2], [2, 3, 4], [1, 7, 2], [-1, 0, 1]], dtype=torch.int32, device=DEV)
    zeros = torch.zeros(5, dtype=torch.int32, device=DEV)
    for obs, invalid, kw in ((zeros + 4, zeros, {}), (zeros + 3, zeros, {}), (zeros + 10, zeros + 7, {}), (zeros + 10, zeros + 8, {}),
                             (zeros + 3, zeros, dict(obs_threshold=2)), (zeros + 10, zeros + 7, dict(invalid_share=0.69))):
        got, want = mc.cut_mesh(vertices, triangles, obs, invalid, **kw), tmc.cut_mesh(vertices, triangles, obs, invalid, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- end to end --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(FLAGS))
def test_cull_mesh_equals_the_restatement(mc, tmc, room, name):
    missing, occlusion = FLAGS[name]
    r = room
    mesh = (r["vertices"], r["triangles"])
    kw = dict(depth_gt=r["depth_gt"], remove_missing_depth=missing, remove_occlusion=occlusion)
    want = tmc.cull_mesh(mesh, r["poses"], r["K"], r["H"], r["W"], **kw)
    assert 0 < want[1].shape[0] < r["triangles"].shape[0]
    for batch in (1, 2, 8, 9):
        got = mc.cull_mesh(mesh, r["poses"], r["K"], r["H"], r["W"], camera_batch=batch, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_cull_mesh_without_sensor_depth_implies_no_missing_depth_rule(mc, tmc, room):
    r = room
    mesh = (r["vertices"], r["triangles"])
    got = mc.cull_mesh(mesh, r["poses"], r["K"], r["H"], r["W"])
    want = tmc.cull_mesh(mesh, r["poses"], r["K"], r["H"], r["W"], depth_gt=r["depth_gt"], remove_missing_depth=False)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_culled_mesh_metrics_is_mesh_metrics_on_the_two_culled_meshes(mc, room):
    from dn_splatter_amd import geometry

    r = room
    target = (r["vertices"], r["triangles"])
    shift = torch.tensor([0.01, -0.02, 0.015], device=DEV)
    pred = (r["vertices"] + shift, r["triangles"])
    args = (r["poses"], r["K"], r["H"], r["W"])
    got = mc.culled_mesh_metrics(pred, target, *args, depth_gt=r["depth_gt"], remove_occlusion=False)
    want = geometry.mesh_metrics(mc.cull_mesh(pred, *args, depth_gt=r["depth_gt"], remove_occlusion=False),
                                 mc.cull_mesh(target, *args, depth_gt=r["depth_gt"], remove_occlusion=False))
    assert sorted(got) == sorted(want) and len(got) == 8
    for k in want:
        assert torch.equal(got[k], want[k]) and bool(torch.isfinite(got[k])), k
    assert 0 < float(got["Acc"]) < 0.1
