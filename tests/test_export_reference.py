"""The point-cloud export against vectors produced by THE REFERENCE's own code (tests/golden/make_reference_export_golden.py:
find_depth_edges, pick_indices_at_random, get_colored_points_from_depth and the normal-map transform of export_mesh.py): the PyTorch
restatements of torch_export — the fp64 yardstick of tests/test_gpu_export.py — in float32 and float64; the properties of the
sampler's keyed bijection from its NumPy restatement (_export_inputs.permutation); the binding's struct and the wrappers' argument
checks.  Float bounds: those of test_gpu_export.py (_export_inputs.point_bound / normal_bound), stated there."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _export_inputs as inputs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAMPLER_N = (1, 2, 3, 4, 5, 16, 17, 1000, 4096, 4097)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "reference_export.npz"))


@pytest.mark.parametrize("H,W", inputs.FIXTURE_FRAMES)
def test_inputs_are_the_recipe_and_hold_its_conditions(g, H, W):
    f = inputs.fixture_frame(g, H, W)
    r = inputs.frame_inputs(H, W)
    for k in ("depth", "rgb", "surface_normal", "mask"):
        assert torch.equal(f[k], r[k]), k
    c2w_gl, *intr = inputs.camera(H, W)
    assert torch.equal(f["c2w_gl"], c2w_gl) and f["intr"] == tuple(intr)
    for thr, _ in inputs.EDGE_SETTINGS:
        assert int(inputs.flagged_edge_decisions(f["depth"][..., 0], thr).sum()) == 0          # the allowed number is 0
    sn = f["surface_normal"]
    assert bool((sn[0] == 0.5).all() and (sn[-1] == 0.5).all() and (sn[:, 0] == 0.5).all() and (sn[:, -1] == 0.5).all())
    assert int((f["depth"] == 0).sum()) == 6


@pytest.mark.parametrize("H,W", inputs.FIXTURE_FRAMES)
def test_edge_maps_equal_the_reference(g, H, W):
    """Bit for bit, in float32 and in float64, and equal to the Chebyshev-distance form the kernel implements."""
    from dn_splatter_amd import torch_export as te

    f = inputs.fixture_frame(g, H, W)
    shares = []
    for thr, itr in inputs.EDGE_SETTINGS:
        ref = inputs.bits(g, f["pre"] + f"valid_t{thr}_i{itr}", (H, W, 1))
        for dt in (torch.float32, torch.float64):
            e = te.find_depth_edges(f["depth"].to(dt), thr, itr)
            assert e.dtype == dt and e.shape == (H, W, 1)
            assert torch.equal(e < 0.2, ref), (thr, itr, dt)
        raw = (te.depth_laplacian(f["depth"][..., 0].double()) > thr).numpy()
        assert np.array_equal(~inputs.chebyshev_dilate(raw, itr), ref[..., 0].numpy())
        shares.append(float(ref.float().mean()))
    assert 0.25 < min(shares) < 0.5 and 0.9 < max(shares) < 1.0                              # the filter selects and rejects


@pytest.mark.parametrize("H,W", inputs.FIXTURE_FRAMES)
def test_pick_and_points_equal_the_reference(g, H, W):
    from dn_splatter_amd import torch_export as te

    f = inputs.fixture_frame(g, H, W)
    pre = f["pre"]
    fx, fy, cx, cy = f["intr"]
    assert torch.equal(te.export_c2w(f["c2w_gl"]), f["c2w_cv"])
    valid = {"depth": f["depth"], "edges": inputs.bits(g, pre + "valid_t0.004_i10", (H, W, 1))}
    for tag in ("depth", "edges"):
        torch.manual_seed(inputs.PICK_SEED)
        idx = te.pick_indices_at_random(valid[tag], inputs.SAMPLES)
        ref_idx = torch.from_numpy(g[pre + f"pick_{tag}"]).long()
        assert torch.equal(idx, ref_idx)                                                     # the same randperm stream
        assert bool(valid[tag].reshape(-1)[idx].bool().all()) and len(torch.unique(idx)) == inputs.SAMPLES
        for mtag, mask in (("", None), ("_masked", f["mask"])):
            ref = torch.from_numpy(g[pre + f"points_{tag}{mtag}"])
            for dt in (torch.float32, torch.float64):
                d = f["depth"].to(dt).clone()
                if mask is not None:
                    d[~mask] = 0
                xyz, rgb = te.get_colored_points_from_depth(d, f["rgb"].to(dt), f["c2w_cv"].to(dt), fx, fy, cx, cy, (W, H), idx)
                bound = inputs.point_bound(d, f["c2w_cv"], fx, fy, cx, cy, W, idx)
                assert bool(((xyz.double() - ref.double()).abs() <= bound).all()), (tag, mtag, dt)
                assert torch.equal(rgb.float(), f["rgb"].reshape(-1, 3)[idx])
            if mask is not None:                                                             # a masked pixel is the camera centre
                out = ~f["mask"].reshape(-1)[idx]
                assert bool(out.any()) and torch.equal(ref[out], f["c2w_cv"][:3, 3].expand(int(out.sum()), 3))
        ref_n = torch.from_numpy(g[pre + f"normals_{tag}"])
        for dt in (torch.float32, torch.float64):
            n = te.world_normals(f["surface_normal"].to(dt), f["c2w_cv"].to(dt))[idx]
            n64 = te.world_normals(f["surface_normal"].double(), f["c2w_cv"].double())[idx]
            assert bool(((n.double() - ref_n.double()).abs() <= inputs.normal_bound(n64, f["c2w_cv"])).all()), (tag, dt)
        border = (idx // W == 0) | (idx // W == H - 1) | (idx % W == 0) | (idx % W == W - 1)
        assert bool(border.any()) and bool((ref_n[border] == 0).all())
    # all pixels, the tsdf exporter's call
    ref = torch.from_numpy(g[pre + "points_all"])
    xyz, rgb = te.get_colored_points_from_depth(f["depth"], f["rgb"], f["c2w_cv"], fx, fy, cx, cy, (W, H))
    allpix = torch.arange(H * W)
    assert bool(((xyz.double() - ref.double()).abs() <= inputs.point_bound(f["depth"], f["c2w_cv"], fx, fy, cx, cy, W, allpix)).all())
    assert torch.equal(rgb, f["rgb"].reshape(-1, 3))


def test_frame_points_is_the_loop_body(g):
    """torch_export.frame_points with the reference's indices: the rows of the separate calls, cropped by ``within`` in order."""
    from dn_splatter_amd import torch_export as te

    H, W = inputs.FIXTURE_FRAMES[0]
    f = inputs.fixture_frame(g, H, W)
    fx, fy, cx, cy = f["intr"]
    cam = inputs.Cam(f["c2w_gl"], fx, fy, cx, cy, W, H)
    idx = torch.from_numpy(g[f["pre"] + "pick_depth"]).long()
    out = dict(depth=f["depth"], rgb=f["rgb"], surface_normal=f["surface_normal"])
    xyz, nrm, rgb = te.frame_points(out, cam, inputs.SAMPLES, indices=idx, mask=f["mask"])
    d = f["depth"].clone()
    d[~f["mask"]] = 0
    ref = torch.from_numpy(g[f["pre"] + "points_depth_masked"])
    assert bool(((xyz.double() - ref.double()).abs() <= inputs.point_bound(d, f["c2w_cv"], fx, fy, cx, cy, W, idx)).all())
    assert torch.equal(out["depth"], f["depth"])                                             # the caller's depth image is left alone
    box = inputs.Box(torch.eye(3), xyz.mean(dim=0), torch.tensor([1.5, 1.0, 2.0]))
    inside = te.within(box, xyz)
    assert 0 < int(inside.sum()) < len(idx)
    x2, n2, c2 = te.frame_points(out, cam, inputs.SAMPLES, indices=idx, mask=f["mask"], crop_box=box)
    assert torch.equal(x2, xyz[inside]) and torch.equal(n2, nrm[inside]) and torch.equal(c2, rgb[inside])
    far = inputs.Box(torch.eye(3), torch.tensor([1e3, 0.0, 0.0]), torch.ones(3))
    assert te.frame_points(out, cam, inputs.SAMPLES, indices=idx, crop_box=far) is None
    assert te.frame_points(out, cam, inputs.SAMPLES, indices=idx[:0]) is None


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", SAMPLER_N)
def test_permutation_is_a_bijection(n):
    for seed in (0, 1, 2 ** 40 + 3, 2 ** 64 - 1):
        p = inputs.permutation(np.arange(n), n, seed)
        assert np.array_equal(np.sort(p), np.arange(n)), (n, seed)
    if n >= 1000:
        assert not np.array_equal(inputs.permutation(np.arange(n), n, 0), inputs.permutation(np.arange(n), n, 1))


def test_sampler_keeps_order_when_everything_fits_and_handles_empty():
    rng = np.random.default_rng(5)
    valid = rng.random(4900) < 0.3
    n = int(valid.sum())
    for k in (n, n + 1, 4900, 10 ** 6):
        idx, n_out, m = inputs.sample(valid, k, seed=9)
        assert (n_out, m) == (n, n) and np.array_equal(idx, np.flatnonzero(valid))             # n <= k: ascending
    idx, n_out, m = inputs.sample(valid, n - 1, seed=9)
    assert m == n - 1 and len(set(idx.tolist())) == n - 1 and bool(valid[idx].all())
    assert not np.array_equal(idx, np.sort(idx))
    idx, n_out, m = inputs.sample(np.zeros(100, dtype=bool), 7, seed=1)
    assert (n_out, m, idx.size) == (0, 0, 0)                                                   # n = 0 gives m = 0
    idx, n_out, m = inputs.sample(valid, 0, seed=1)
    assert (n_out, m, idx.size) == (n, 0, 0)


def test_sampler_is_uniform():
    """n = 1000, k = 100, seeds 0 .. 255: every pixel is included with probability 0.1, so its count over the 256 fixed seeds has
    mean 25.6 and variance 23.04, and the chi-square statistic of the 1000 counts has mean 999 and variance 2 x 999 (the counts of one
    draw are negatively correlated by a factor 1 - 1 / n, which moves neither figure at this width).  Within six standard deviations:
    [731, 1267].  Deterministic."""
    counts = np.zeros(1000)
    for seed in range(256):
        idx, n, m = inputs.sample(np.ones(1000, dtype=bool), 100, seed)
        assert (n, m) == (1000, 100) and len(set(idx.tolist())) == 100
        counts[idx] += 1
    chi2 = float(((counts - 25.6) ** 2 / 23.04).sum())
    print(f"chi-square of the inclusion counts: {chi2:.1f} (band 731 .. 1267)")
    assert 999 - 6 * (2 * 999) ** 0.5 <= chi2 <= 999 + 6 * (2 * 999) ** 0.5
    # position 0 of the draw over the seeds: 256 draws into 1000 cells, a cell's count is Poisson(0.256); six or more in one cell
    # has probability 4e-7 per cell
    first = np.array([inputs.sample(np.ones(1000, dtype=bool), 100, s)[0][0] for s in range(256)])
    assert np.bincount(first, minlength=1000).max() <= 5


def test_constants_agree_with_the_header():
    from dn_splatter_amd import export

    text = open(os.path.join(ROOT, "include", "dnsplat.h")).read()
    for name, value in (("DNSPLAT_EDGE_ROW_TILE", export.EDGE_ROW_TILE), ("DNSPLAT_EDGE_MAX_DILATION", export.EDGE_MAX_DILATION),
                        ("DNSPLAT_SAMPLE_ROUNDS", export.SAMPLE_ROUNDS)):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == value, name
    assert export.SAMPLE_ROUNDS == inputs.ROUNDS


# ---- the binding ---------------------------------------------------------------------------------------------------------------------------


def test_backproject_struct_layout_matches_the_c_compiler(dns, tmp_path):
    from dn_splatter_amd import _lib

    header = os.path.join(ROOT, "include", "dnsplat.h")
    cls = _lib.BackprojectArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void){",
             'printf("size %zu\\n", sizeof(dnsplat_backproject_args));']
    lines += [f'printf("{n} %zu\\n", offsetof(dnsplat_backproject_args, {n}));' for n, _ in cls._fields_]
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for n, _ in cls._fields_:
        assert int(got[n]) == getattr(cls, n).offset, n


def test_entry_points_refuse_bad_arguments_without_a_gpu(dns):
    from dn_splatter_amd import _lib

    L = dns.load_library()
    one = ctypes.c_void_p(16)                      # never dereferenced: every call below returns before a launch
    assert L.dnsplat_pointcloud_scratch_bytes(0, 4, 0) == 0 and L.dnsplat_pointcloud_scratch_bytes(4, 4, -1) == 0
    assert L.dnsplat_pointcloud_scratch_bytes(65536, 32768, 0) == 0                          # 2^31 pixels
    assert L.dnsplat_pointcloud_scratch_bytes(65535, 32768, 0) > 0
    small, big = L.dnsplat_pointcloud_scratch_bytes(70, 45, 500), L.dnsplat_pointcloud_scratch_bytes(1920, 1080, 20000)
    assert 0 < small < big and small % 16 == 0 and big >= 4 * 1920 * 1080
    assert L.dnsplat_depth_edge_valid(4, 4, None, 0.01, 3, one, one, None) == -1
    assert L.dnsplat_depth_edge_valid(4, 4, one, 0.01, 3, None, one, None) == -1
    assert L.dnsplat_depth_edge_valid(4, 4, one, 0.01, 3, one, None, None) == -1
    assert L.dnsplat_depth_edge_valid(0, 4, one, 0.01, 3, one, one, None) == -1
    assert L.dnsplat_depth_edge_valid(4, 4, one, 0.01, 65, one, one, None) == -4
    assert L.dnsplat_depth_edge_valid(4, 4, one, 0.01, -1, one, one, None) == -4
    assert L.dnsplat_depth_edge_valid(65536, 32768, one, 0.01, 3, one, one, None) == -4
    assert L.dnsplat_sample_valid_pixels(4, 4, None, None, 3, 0, one, one, one, None) == -1
    assert L.dnsplat_sample_valid_pixels(4, 4, one, None, 3, 0, None, one, one, None) == -1
    assert L.dnsplat_sample_valid_pixels(4, 4, one, None, 3, 0, one, None, one, None) == -1
    assert L.dnsplat_sample_valid_pixels(4, 4, one, None, -1, 0, one, one, one, None) == -1
    assert L.dnsplat_sample_valid_pixels(4, -4, one, None, 3, 0, one, one, one, None) == -1
    assert L.dnsplat_backproject_points(None, None) == -1
    a = _lib.BackprojectArgs()
    a.width, a.height, a.capacity = 4, 4, 8
    assert L.dnsplat_backproject_points(ctypes.byref(a), None) == -1                         # null buffers
    for name in ("depth", "rgb", "xform", "points", "colors", "state", "scratch"):
        setattr(a, name, 16)
    a.capacity = 0
    assert L.dnsplat_backproject_points(ctypes.byref(a), None) == -1
    a.capacity, a.normal = 8, 16
    assert L.dnsplat_backproject_points(ctypes.byref(a), None) == -1                         # a normal image without a normals buffer
    a.normal, a.indices, a.n_rows = None, 16, -1
    assert L.dnsplat_backproject_points(ctypes.byref(a), None) == -1
    a.indices, a.width, a.height = None, 65536, 32768
    assert L.dnsplat_backproject_points(ctypes.byref(a), None) == -4


def test_wrappers_validate_their_arguments(dns):
    from dn_splatter_amd import DnsplatError, export

    assert dns.export is export and dns.OrientedPointCloud is export.OrientedPointCloud
    assert dns.export_oriented_points is export.export_oriented_points
    depth = torch.ones(6, 8, 1)
    with pytest.raises(DnsplatError, match="no CPU fallback"):
        export.find_depth_edges(depth)
    with pytest.raises(DnsplatError, match="no CPU fallback"):
        export.pick_indices_at_random(depth, 4)
    with pytest.raises(DnsplatError, match="no CPU fallback"):
        export.get_colored_points_from_depth(depth, torch.ones(6, 8, 3), torch.eye(4)[:3], 5.0, 5.0, 4.0, 3.0, (8, 6))
    with pytest.raises(DnsplatError, match="no CPU"):
        export.OrientedPointCloud(10, "cpu")
    with pytest.raises(ValueError):
        export.OrientedPointCloud(0, "cuda")
    with pytest.raises(ValueError):
        export.sample_valid_pixels(None, None, 3)
    with pytest.raises(ValueError):
        export.sample_valid_pixels(None, depth, -1)
    with pytest.raises(ValueError):
        export.depth_edge_valid(torch.ones(2, 3, 4))
    with pytest.raises(ValueError):
        export.export_oriented_points(None, [])
