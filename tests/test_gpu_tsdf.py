"""TSDF fusion on the MI355X (csrc/tsdf.hip, the observed instantiation of csrc/marching.hip) against the restatements
(dn_splatter_amd/torch_tsdf.py, torch_marching.py with ``observed``), which run on the CPU here.  Every comparison is EXACT: tsdf, weight,
colour volumes, vertices and vertex colours as bit patterns, triangles and counts as integers.  There is no tolerance anywhere in this file.

Shapes: the lattices of test_gpu_marching.py, whose rows straddle lanes, waves and workgroups ((5,6,7) and (3,2,9) end inside a word,
(65,3,2) and (2,2,129) inside a wave's run, (17,9,33) is one workgroup and a ragged second one of the 256-thread integration kernel too,
64^3 is 1024 of them).  Camera counts 1, 8, 9, 17: the kernel passes camera rows through LDS eight at a time, so these are a ragged
trip, one full trip, a full and a ragged one, and two full trips and a ragged third."""
import ctypes

import numpy as np
import pytest
import torch

import _tsdf_inputs as inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMAGES = [(29, 37), (48, 64)]                               # (H, W)
SENTINEL = -777.25


@pytest.fixture(scope="module")
def tsdf():
    from dn_splatter_amd import tsdf as module

    return module


@pytest.fixture(scope="module")
def tt():
    from dn_splatter_amd import torch_tsdf

    return torch_tsdf


@pytest.fixture(scope="module")
def tm():
    from dn_splatter_amd import torch_marching

    return torch_marching


@pytest.fixture(scope="module")
def mc():
    from dn_splatter_amd import marching

    return marching


def same_bits(got: torch.Tensor, want) -> bool:
    got = got.cpu().numpy()
    want = want.cpu().numpy() if torch.is_tensor(want) else want
    view = np.int64 if got.dtype == np.float64 else np.int32
    return got.dtype == want.dtype and got.shape == want.shape and bool((got.view(view) == want.view(view)).all())


def reference(tt, shape, C, image, color, offset, fill=0.0, split=None):
    """The restatement's volume after C frames on the CPU: (tsdf, weight, colour or None) and the call's arguments."""
    from dn_splatter_amd.torch_mesh_cull import opencv_w2c

    H, W = image
    origin, voxel = inputs.volume_frame(shape)
    K = inputs.intrinsics(W, H, 0.9 * W)
    poses = inputs.orbit_poses(C)
    depth, rgb = inputs.frames(C, H, W)
    t, w = torch.full(shape, fill), torch.zeros(shape)
    c = torch.full(shape + (3,), fill) if color else None
    tt.integrate(t, w, c, origin, voxel, opencv_w2c(poses), K, depth, rgb if color else None, tt.ray_scale(K, H, W), inputs.SDF_TRUNC,
                 inputs.DEPTH_TRUNC, offset)
    return (t, w, c), {"origin": origin, "voxel": voxel, "K": K, "poses": poses, "depth": depth, "rgb": rgb if color else None}


def device_volume(tsdf, shape, args, color, offset, fill=0.0, parts=None):
    vol = tsdf.TSDFVolume(args["origin"], args["voxel"], shape, sdf_trunc=inputs.SDF_TRUNC, depth_trunc=inputs.DEPTH_TRUNC,
                          pixel_offset=offset, color=color, device=DEV)
    if fill:
        vol.tsdf.fill_(fill)
        if color:
            vol.color.fill_(fill)
    C = args["depth"].shape[0]
    for s, e in parts or [(0, C)]:
        vol.integrate(args["depth"][s:e].to(DEV), args["rgb"][s:e].to(DEV) if color else None, args["poses"][s:e], args["K"])
    return vol


def check_volume(vol, want) -> None:
    t, w, c = want
    assert same_bits(vol.weight, w)
    assert same_bits(vol.tsdf, t)
    assert (vol.color is None) == (c is None)
    if c is not None:
        assert same_bits(vol.color, c)


# ----------------------------------------------------------------------------------------------- integrate
@pytest.mark.parametrize("C", [1, 8, 9, 17])
@pytest.mark.parametrize("shape", inputs.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integrate_equals_the_restatement(tsdf, tt, shape, C):
    """Two runs per case, one with colour and one without, on the two image sizes and the two pixel offsets: the offset alternates with
    the shape and the image with C, so over the matrix every image meets every offset with colour and without."""
    a, b = inputs.SHAPES.index(shape) % 2, [1, 8, 9, 17].index(C) % 2
    for color, offset, image in ((True, (0.5, 0.0)[a], IMAGES[b]), (False, (0.0, 0.5)[a], IMAGES[1 - b])):
        want, args = reference(tt, shape, C, image, color, offset)
        assert int((want[1] > 0).sum()) > 0
        check_volume(device_volume(tsdf, shape, args, color, offset), want)


def test_every_way_out_of_the_rule_is_taken(tt):
    """The frames of the matrix above leave voxels unseen, seen once and seen many times at (17,9,33) with 8 cameras."""
    (t, w, _), _ = reference(tt, (17, 9, 33), 8, IMAGES[1], True, 0.5)
    counts = set(w.reshape(-1).tolist())
    assert 0.0 in counts and 1.0 in counts and max(counts) >= 5.0
    assert float(t.max()) == 1.0 and float(t.min()) < -0.5


def test_two_calls_leave_the_bytes_of_one(tsdf, tt):
    shape = (17, 9, 33)
    want, args = reference(tt, shape, 9, IMAGES[0], True, 0.5)
    check_volume(device_volume(tsdf, shape, args, True, 0.5, parts=[(0, 5), (5, 9)]), want)
    check_volume(device_volume(tsdf, shape, args, True, 0.5, parts=[(0, 9)]), want)


def test_untouched_voxels_are_not_written(tsdf, tt):
    shape = (17, 9, 33)
    want, args = reference(tt, shape, 8, IMAGES[1], True, 0.0, fill=SENTINEL)
    vol = device_volume(tsdf, shape, args, True, 0.0, fill=SENTINEL)
    unseen = vol.weight == 0
    assert 100 < int(unseen.sum()) < unseen.numel() - 100
    assert bool((vol.tsdf[unseen] == SENTINEL).all()) and bool((vol.color[unseen] == SENTINEL).all())
    check_volume(vol, want)                                  # and the touched ones averaged the sentinel in, as the restatement does


# ----------------------------------------------------------------------------------------------- observed marching cubes
def check_observed(mc, tm, vol: np.ndarray, level: float, weight: np.ndarray, min_weight: float):
    want_v, want_t = tm.marching_cubes(vol, level, observed=inputs.observed(weight, min_weight))
    got_v, got_t = mc.marching_cubes(torch.from_numpy(vol).to(DEV), level, weight=torch.from_numpy(weight).to(DEV), min_weight=min_weight)
    assert got_v.dtype == torch.float32 and got_t.dtype == torch.int32
    assert (got_v.shape[0], got_t.shape[0]) == (len(want_v), len(want_t))
    assert same_bits(got_t, want_t)
    assert same_bits(got_v, want_v)
    return want_v, want_t


@pytest.mark.parametrize("shape", [(2, 2, 2)] + inputs.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("field", ["noise", "smooth"])
def test_all_observed_is_marching_cubes_bit_for_bit(mc, tm, shape, field):
    vol, level = (inputs.noise(shape), 0.5) if field == "noise" else (inputs.smooth(shape), 0.0)
    dev = torch.from_numpy(vol).to(DEV)
    v0, t0 = mc.marching_cubes(dev, level)
    v1, t1 = mc.marching_cubes(dev, level, weight=torch.ones_like(dev), min_weight=0.0)
    assert v0.shape[0] > 0 and torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and torch.equal(t0, t1)
    want_v, want_t = tm.marching_cubes(vol, level)
    assert same_bits(v0, want_v) and same_bits(t0, want_t)


@pytest.mark.parametrize("min_weight", [0.0, 2.5])
@pytest.mark.parametrize("unobserved", [0.2, 0.9])
@pytest.mark.parametrize("shape", inputs.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_partly_observed_lattices(mc, tm, shape, unobserved, min_weight):
    weight = inputs.weights(shape, unobserved, min_weight)
    seen = inputs.observed(weight, min_weight)
    assert abs((~seen).mean() - unobserved) < 0.25
    for vol, level in ((inputs.noise(shape), 0.5), (inputs.smooth(shape), 0.0)):
        v, t = check_observed(mc, tm, vol, level, weight, min_weight)
        assert bool(np.isfinite(v).all()) and bool((t < max(len(v), 1)).all())
    if unobserved == 0.2 and min(shape) >= 9:
        assert len(t) > 0


def test_all_256_single_cells_with_each_corner_unobserved(mc, tm):
    for case in range(0, 256, 5):                           # every fifth case on the device; all 256 on the restatement (test_tsdf_reference)
        vol = np.array([1.0 if (case >> c) & 1 else -1.0 for c in range(8)], dtype=np.float32)
        vol = np.ascontiguousarray(vol.reshape(2, 2, 2).transpose(2, 1, 0))
        for corner in range(8):
            weight = np.ones((2, 2, 2), dtype=np.float32)
            weight[corner & 1, (corner >> 1) & 1, (corner >> 2) & 1] = 0.0
            _, t = check_observed(mc, tm, vol, 0.0, weight, 0.0)
            assert len(t) == 0


def test_the_fill_of_unobserved_voxels_changes_nothing(mc, tm):
    shape = (17, 9, 33)
    vol = inputs.smooth(shape) + 0.3 * (inputs.noise(shape) - 0.5)
    weight = inputs.weights(shape, 0.2, 0.0)
    seen = inputs.observed(weight, 0.0)
    meshes = []
    for fill in (np.nan, np.inf, 1e30):
        filled = np.where(seen, vol, np.float32(fill)).astype(np.float32)
        check_observed(mc, tm, filled, 0.0, weight, 0.0)
        meshes.append(mc.marching_cubes(torch.from_numpy(filled).to(DEV), 0.0, weight=torch.from_numpy(weight).to(DEV)))
    assert meshes[0][0].shape[0] > 100 and meshes[0][1].shape[0] > 100
    for v, t in meshes[1:]:
        assert torch.equal(v.view(torch.int32), meshes[0][0].view(torch.int32)) and torch.equal(t, meshes[0][1])


@pytest.mark.parametrize("short", ["triangles", "vertices"])
def test_observed_capacity_below_the_count(mc, tm, short):
    shape = (17, 9, 33)
    vol, weight = inputs.noise(shape), inputs.weights(shape, 0.2, 0.0)
    want_v, want_t = tm.marching_cubes(vol, 0.5, observed=inputs.observed(weight, 0.0))
    V, T = len(want_v), len(want_t)
    assert V > 10 and T > 10
    cap_v, cap_t = (V, T - 1) if short == "triangles" else (V - 1, T)
    guard = 16
    vertices = torch.full((V + guard, 3), -777.0, dtype=torch.float32, device=DEV)
    triangles = torch.full((T + guard, 3), -7, dtype=torch.int32, device=DEV)
    count = mc.mc_count(torch.from_numpy(vol).to(DEV), 0.5, weight=torch.from_numpy(weight).to(DEV), min_weight=0.0)
    assert count.scratch.numel() * 8 >= mc.scratch_bytes(shape, True) > mc.scratch_bytes(shape)
    status = mc.mc_emit(count, vertices, triangles, cap_v=cap_v, cap_t=cap_t)
    assert status.tolist() == [mc.STATUS_TRIANGLES if short == "triangles" else mc.STATUS_VERTICES]
    assert count.counts.tolist() == [V, T]
    assert same_bits(vertices[:cap_v], want_v[:cap_v]) and same_bits(triangles[:cap_t], want_t[:cap_t])
    assert bool((vertices[cap_v:] == -777.0).all()) and bool((triangles[cap_t:] == -7).all())
    status = mc.mc_emit(count, vertices, triangles, cap_v=V, cap_t=T)
    assert status.tolist() == [0] and same_bits(vertices[:V], want_v) and same_bits(triangles[:T], want_t)
    assert bool((vertices[V:] == -777.0).all()) and bool((triangles[T:] == -7).all())


# ----------------------------------------------------------------------------------------------- vertex colours
@pytest.mark.parametrize("shape", [s for s in inputs.SHAPES], ids=lambda s: "x".join(map(str, s)))
def test_vertex_colours_equal_the_restatement(tsdf, tt, tm, shape):
    rng = np.random.default_rng(sum(shape))
    color = torch.from_numpy((rng.random(shape + (3,)) * 255).astype(np.float32))
    weight = inputs.weights(shape, 0.2, 0.0)
    rows = [tm.marching_cubes(inputs.noise(shape), 0.5, observed=inputs.observed(weight, 0.0))[0],
            tm.marching_cubes((inputs.noise(shape) > 0.5).astype(np.float32), 0.0)[0],           # values 0 (the level) and 1: every t is 0 or 1
            np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf]], dtype=np.float32),
            np.array([[n - 1 for n in shape], [0, 0, 0], [n - 1.5 for n in shape]], dtype=np.float32)]
    assert bool((rows[1] == np.floor(rows[1])).all()) and len(rows[1]) > 0
    vertices = torch.from_numpy(np.concatenate(rows))
    want = tt.vertex_colors(color, vertices)
    vol = tsdf.TSDFVolume((0, 0, 0), 1.0, shape, device=DEV)
    vol.color.copy_(color)
    got = vol.vertex_colors(vertices.to(DEV))
    assert same_bits(got, want)
    nan_rows = len(rows[0]) + len(rows[1])
    assert bool((got[nan_rows:nan_rows + 3] == 0).all())


# ----------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def sphere(tt):
    from dn_splatter_amd.torch_mesh_cull import opencv_w2c

    s = inputs.sphere_scene()
    t, w, c = torch.zeros(s["dims"]), torch.zeros(s["dims"]), torch.zeros(s["dims"] + (3,))
    tt.integrate(t, w, c, s["origin"], s["voxel"], opencv_w2c(s["poses"]), s["K"], s["depth"], s["rgb"],
                 tt.ray_scale(s["K"], s["height"], s["width"]), 0.03, 20.0, 0.5)
    return s, (t, w, c), tt.extract_mesh(t, w, c, s["origin"], s["voxel"])


def test_sphere_volume_and_mesh_equal_the_restatement_chain(tsdf, sphere):
    s, want_volume, (want_v, want_t, want_c) = sphere
    vol = tsdf.TSDFVolume(s["origin"], s["voxel"], s["dims"], device=DEV)
    vol.integrate(s["depth"].to(DEV)[..., None], s["rgb"].to(DEV), s["poses"], s["K"])          # [C,H,W,1], as the renderer hands it out
    check_volume(vol, want_volume)
    vertices, triangles, colors = vol.extract_mesh()
    assert vertices.dtype == torch.float64 and vertices.is_cuda and triangles.dtype == torch.int32 and colors.dtype == torch.float32
    assert len(want_v) > 3000 and same_bits(triangles, want_t) and same_bits(vertices, want_v) and same_bits(colors, want_c)
    # with a capacity nothing is read on the host: full-capacity buffers, device counts and status
    V, T = len(want_v), len(want_t)
    world, tri, col, raw = vol.extract_mesh(capacity=(V + 3, T + 2))
    assert raw.counts.tolist() == [V, T] and raw.status.tolist() == [0]
    assert same_bits(world[:V], want_v) and same_bits(tri[:T], want_t) and same_bits(col[:V], want_c)
    # min_weight: the extraction over the voxels that at least three frames saw
    v3, t3, _ = vol.extract_mesh(min_weight=2.0)
    from dn_splatter_amd import torch_tsdf

    w3 = torch_tsdf.extract_mesh(*want_volume, s["origin"], s["voxel"], min_weight=2.0)
    assert 0 < len(w3[1]) < T and same_bits(t3, w3[1]) and same_bits(v3, w3[0])


class _Stub:
    """A renderer that hands out the sphere's frames: the ``get_outputs_batch`` of DNSplatterRenderer."""

    def __init__(self, scene):
        self.scene, self.at = scene, 0

    def get_outputs_batch(self, cameras, max_batch=8):
        for _ in cameras:
            i, self.at = self.at, self.at + 1
            yield {"depth": self.scene["depth"][i].to(DEV)[..., None].clone(), "rgb": self.scene["rgb"][i].to(DEV)}


def test_fuse_tsdf_mesh_feeds_culling_and_scores(dns, tsdf, sphere):
    s, _, (want_v, want_t, want_c) = sphere
    K = s["K"]
    cameras = [dns.Camera(torch.from_numpy(p[:3]).float()[None].to(DEV), K[0, 0], K[1, 1], K[0, 2], K[1, 2], s["width"], s["height"])
               for p in s["poses"]]
    lo, hi = s["origin"], tuple(o + s["voxel"] * (n - 1) for o, n in zip(s["origin"], s["dims"]))
    mesh = tsdf.fuse_tsdf_mesh(_Stub(s), cameras, (lo, hi), voxel_size=s["voxel"], batch=4)
    assert tuple(tsdf.TSDFVolume.from_bounds(lo, hi, s["voxel"], device=DEV).dims) == s["dims"]
    assert same_bits(mesh[1], want_t) and same_bits(mesh[0], want_v) and same_bits(mesh[2], want_c)
    masks = [torch.ones(s["height"], s["width"], dtype=torch.bool) for _ in cameras]
    masks[0][:] = False
    masked = tsdf.fuse_tsdf_mesh(_Stub(s), cameras, (lo, hi), voxel_size=s["voxel"], batch=8, masks=masks, color=False)
    assert masked[2] is None and 0 < masked[1].shape[0] and not torch.equal(masked[1], mesh[1])
    culled = dns.cull_mesh(mesh, s["poses"], K, s["height"], s["width"], obs_threshold=0)
    assert culled[0].shape[0] > 0 and culled[1].shape[0] > 0
    scores = dns.mesh_metrics(culled, (mesh[0], mesh[1]), threshold=0.05)
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in scores.values())
    with pytest.raises(ValueError, match="intrinsics"):
        tsdf.fuse_tsdf_mesh(_Stub(s), cameras[:1] + [dns.Camera(cameras[1].camera_to_worlds, 1.0, 1.0, 1.0, 1.0, 8, 8)], (lo, hi))


# ----------------------------------------------------------------------------------------------- argument checks
def test_refused_calls_leave_the_buffers_alone(dns, tsdf, tt):
    from dn_splatter_amd import _lib, _ops

    L = dns.load_library()
    shape, (H, W), C = (5, 6, 7), IMAGES[0], 2
    _, args = reference(tt, shape, C, (H, W), True, 0.5)
    t = torch.full(shape, SENTINEL, device=DEV)
    w = torch.full(shape, SENTINEL, device=DEV)
    c = torch.full(shape + (3,), SENTINEL, device=DEV)
    from dn_splatter_amd.torch_mesh_cull import intrinsics, opencv_w2c

    w2c, depth, rgb = opencv_w2c(args["poses"]).to(DEV), args["depth"].to(DEV), args["rgb"].to(DEV)
    scale = tt.ray_scale(args["K"], H, W).to(DEV)

    def call(**change):
        a = _ops._tsdf_args(t, w, c, args["origin"], args["voxel"], w2c, intrinsics(args["K"]), 0.5, depth, rgb, scale, 0.1, 3.0)
        for name, value in change.items():
            setattr(a, name, value)
        return L.dnsplat_tsdf_integrate(ctypes.byref(a), None)

    assert L.dnsplat_tsdf_integrate(None, None) == -1
    for name in ("tsdf", "weight", "w2c", "depth", "ray_scale", "color", "rgb"):
        assert call(**{name: None}) == -1, name
    for name in ("nx", "ny", "nz", "C", "width", "height"):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    assert call(nx=2048, ny=1024, nz=1024) == -1             # 2^31 voxels
    for name in ("voxel", "sdf_trunc", "depth_trunc"):
        for bad in (0.0, -1.0, float("nan")):
            assert call(**{name: bad}) == -1, name
    assert call(width=65536, height=32768) == -4             # 2^31 pixels
    torch.cuda.synchronize()
    for buf in (t, w, c):
        assert bool((buf == SENTINEL).all())
    assert call() == 0                                       # and the unchanged arguments are accepted
    torch.cuda.synchronize()
    assert bool((w != SENTINEL).any())

    out = torch.full((4, 3), SENTINEL, device=DEV)
    v = torch.zeros(4, 3, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())              # noqa: E731
    colors = L.dnsplat_tsdf_vertex_colors
    assert colors(None, 5, 6, 7, p(v), 4, p(out), None) == -1 and colors(p(c), 5, 6, 7, None, 4, p(out), None) == -1
    assert colors(p(c), 5, 6, 7, p(v), 4, None, None) == -1 and colors(p(c), 5, 6, 7, p(v), -1, p(out), None) == -1
    assert colors(p(c), 1, 6, 7, p(v), 4, p(out), None) == -1 and colors(p(c), 5, 6, 0, p(v), 4, p(out), None) == -1
    assert colors(p(c), 5, 6, 7, p(v), 2 ** 31, p(out), None) == -4
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())

    vol = torch.from_numpy(inputs.noise(shape)).to(DEV)
    count = _lib.McObservedArgs()
    assert L.dnsplat_mc_count_observed(None, None) == -1 and L.dnsplat_mc_emit_observed(None, None) == -1
    counts = torch.full((2,), -5, dtype=torch.int64, device=DEV)
    scratch = torch.zeros(L.dnsplat_mc_observed_scratch_bytes(*shape) // 8, dtype=torch.int64, device=DEV)
    count.mc = _ops._mc_args(vol, 0.5, scratch, counts)
    assert L.dnsplat_mc_count_observed(ctypes.byref(count), None) == -1                  # no weight
    count.weight = p(vol)
    count.mc.scratch_bytes = L.dnsplat_mc_scratch_bytes(*shape)                           # the unmasked size is too short
    assert L.dnsplat_mc_count_observed(ctypes.byref(count), None) == -2
    torch.cuda.synchronize()
    assert counts.tolist() == [-5, -5] and bool((scratch == 0).all())
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        tsdf.TSDFVolume((0, 0, 0), 1.0, (2, 2, 2), device="cpu")
