"""The point-cloud export on the MI355X (csrc/pointcloud.hip through dn_splatter_amd.export) against the reference's own outputs
(tests/golden/reference_export.npz), the fp64 restatement (torch_export) and the NumPy restatement of the sampler
(_export_inputs.sample).

Bounds, with u = 2^-24.  Maps, indices and colours: bit for bit.  Points: 8 u (sum_i |p_i| |A_ij| + |t_j|) per component — 2
roundings in p, 3 products, 3 additions.  Normals: 16 u sum_j |R_ij| |n_j| — 13 roundings on the path.  Threshold decisions are
compared exactly on frames with NO decision inside the rounding envelope, which each test asserts of its frame (the allowed number
is 0): a condition on the inputs, not a tolerance.  Without csrc/pointcloud.hip every test here fails at symbol lookup."""
import os

import numpy as np
import pytest
import torch

import _export_inputs as inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ITRS = (0, 1, 10, 63, 64)
SAMPLER_N = (1, 2, 3, 4, 5, 16, 17, 1000, 4096, 4097)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "reference_export.npz"))


@pytest.fixture(scope="module")
def export(dns):
    from dn_splatter_amd import export as ex

    ex.depth_edge_valid(torch.ones(2, 2, device=DEV))          # fails here at symbol lookup without the feature
    return ex


def _valid64(depth, thr, itr):
    """bool [H,W] of the fp64 restatement for a float32 [H,W] depth image."""
    from dn_splatter_amd import torch_export as te

    return (te.find_depth_edges(depth.double()[..., None], thr, itr) < 0.2)[..., 0]


def _shape_depth(H, W):
    """The recipe's frame with a far pixel every 41 pixels (each an edge of its own: thin frames have no box or bump); a single pixel
    has only its own -4 r, positive for a negative depth."""
    depth = inputs.depth_image(H, W)
    depth.view(-1)[::41] = 100.0
    if H * W == 1:
        depth[0, 0] = -2.0
    return depth


def _unflagged(depth, thr):
    assert int(inputs.flagged_edge_decisions(depth, thr).sum()) == 0, "the frame has a threshold decision inside the rounding envelope"


# ---- the edge map ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("H,W", inputs.FIXTURE_FRAMES)
def test_valid_map_equals_the_reference(g, export, H, W):
    f = inputs.fixture_frame(g, H, W)
    for thr, itr in inputs.EDGE_SETTINGS:
        ref = inputs.bits(g, f["pre"] + f"valid_t{thr}_i{itr}", (H, W))
        _unflagged(f["depth"][..., 0], thr)
        got = export.depth_edge_valid(f["depth"].to(DEV), thr, itr)
        assert got.dtype == torch.bool and got.shape == (H, W)
        assert torch.equal(got.cpu(), ref), (thr, itr)
        assert torch.equal(ref, _valid64(f["depth"][..., 0], thr, itr))
        drop_in = export.find_depth_edges(f["depth"].to(DEV), threshold=thr, dilation_itr=itr)
        assert drop_in.shape == (H, W, 1) and drop_in.dtype == torch.float32 and torch.equal((drop_in < 0.2)[..., 0].cpu(), ref)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 200), (200, 1), (9, 63), (7, 64), (7, 65), (7, 129), (31, 70), (32, 70), (33, 70), (65, 513)])
def test_valid_map_shapes_match_fp64(export, H, W):
    """Degenerate frames, widths around the 64-pixel words of a bit row, heights around the dilation kernel's row tile, a frame of
    more than one tile in both directions; every dilation distance from none to the largest."""
    assert export.EDGE_ROW_TILE == 32
    depth = _shape_depth(H, W)
    for thr in (0.004, 0.01):
        _unflagged(depth, thr)
        assert bool((~_valid64(depth, thr, 0)).any())
        for itr in ITRS:
            got = export.depth_edge_valid(depth.to(DEV), thr, itr).cpu()
            assert torch.equal(got, _valid64(depth, thr, itr)), (thr, itr)


@pytest.mark.parametrize("itr", ITRS)
def test_single_edge_pixels_dilate_to_clipped_squares(export, itr):
    """One far pixel in a flat frame is the only pixel whose Laplacian is positive: the invalid region is the (2 itr + 1)^2 square around
    it, clipped by the frame — at the four corners and either side of a word boundary."""
    H, W = 70, 130
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (35, 63), (35, 64), (33, 127), (31, 128)):
        depth = torch.full((H, W), 2.0)
        depth[y, x] = 100.0
        _unflagged(depth, 0.004)
        want = torch.ones(H, W, dtype=torch.bool)
        want[max(0, y - itr):y + itr + 1, max(0, x - itr):x + itr + 1] = False
        got = export.depth_edge_valid(depth.to(DEV), 0.004, itr).cpu()
        assert torch.equal(got, want), (y, x)
        assert torch.equal(want, _valid64(depth, 0.004, itr))


def test_all_edge_and_no_edge_frames(export):
    depth = inputs.depth_image(45, 70)
    finite = torch.isfinite(1.0 / (depth + 1e-6))
    assert bool(finite.all())
    for itr in (0, 3):
        assert not bool(export.depth_edge_valid(depth.to(DEV), -1e30, itr).any())          # every Laplacian exceeds it
        assert bool(export.depth_edge_valid(depth.to(DEV), 1e30, itr).all())               # none does
    flat = torch.full((45, 70), 2.0)                                                        # zero inside, negative on the border
    assert bool(export.depth_edge_valid(flat.to(DEV), 0.004, 10).all())


def test_dilation_outside_its_range_is_refused_without_a_launch(dns, export):
    from dn_splatter_amd import DnsplatError, _ops

    L = dns.load_library()
    depth = inputs.depth_image(45, 70).to(DEV)
    valid = torch.full((45, 70), 7, dtype=torch.uint8, device=DEV)
    scratch = export._scratch(70, 45, 0, DEV)
    for itr in (65, -1):
        rc = L.dnsplat_depth_edge_valid(70, 45, _ops._ptr(depth), 0.004, itr, _ops._ptr(valid), _ops._ptr(scratch), _ops._stream())
        assert rc == -4
        torch.cuda.synchronize()
        assert bool((valid == 7).all())
        with pytest.raises(DnsplatError, match="unsupported"):
            export.depth_edge_valid(depth, 0.004, itr)
    assert L.dnsplat_depth_edge_valid(70, 45, _ops._ptr(depth), 0.004, 64, _ops._ptr(valid), _ops._ptr(scratch), _ops._stream()) == 0
    torch.cuda.synchronize()
    assert bool((valid <= 1).all())


def test_infinite_and_nan_reciprocals_follow_ieee(export):
    """A depth of exactly float32(-1e-6) has the reciprocal inf: its four neighbours are edges (inf > t) and it is none itself (-inf);
    two of them side by side are inf - inf = nan, no edge either.  A nan depth makes itself and its four neighbours nan: no edge.
    Compared with the restatement in float32, where d + 1e-6 is the same sum."""
    from dn_splatter_amd import torch_export as te

    H, W = 40, 70
    depth = torch.full((H, W), 2.0)
    hole = torch.tensor(-1e-6, dtype=torch.float32)
    assert float(hole + torch.tensor(1e-6, dtype=torch.float32)) == 0.0
    depth[5, 5] = hole                      # alone
    depth[0, 69] = hole                     # in the frame's corner
    depth[20, 30] = depth[20, 31] = hole    # side by side
    depth[31, 63] = hole                    # on a word's and a row tile's last pixel
    depth[33, 10] = float("nan")
    for itr in (0, 1, 3):
        want = (te.find_depth_edges(depth[..., None], 0.004, itr) < 0.2)[..., 0]
        got = export.depth_edge_valid(depth.to(DEV), 0.004, itr).cpu()
        assert torch.equal(got, want), itr
    raw = ~export.depth_edge_valid(depth.to(DEV), 0.004, 0).cpu()
    expect = torch.zeros(H, W, dtype=torch.bool)
    for y, x in ((4, 5), (6, 5), (5, 4), (5, 6), (0, 68), (1, 69), (19, 30), (21, 30), (19, 31), (21, 31), (20, 29), (20, 32),
                 (30, 63), (32, 63), (31, 62), (31, 64)):
        expect[y, x] = True
    assert torch.equal(raw, expect)


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------


def _frame_with_n_valid(n, H=70, W=70):
    rng = np.random.default_rng(100 + n)
    valid = np.zeros(H * W, dtype=bool)
    valid[rng.choice(H * W, size=n, replace=False)] = True
    return valid


@pytest.mark.parametrize("n", (0,) + SAMPLER_N)
def test_sampler_equals_its_numpy_restatement(export, n):
    """Both validity sources (a byte map; the depth image itself, where a nan depth is valid as it is for torch.nonzero), k around n,
    the {n, m} words, distinct valid indices, -1 behind m."""
    H = W = 70
    valid = _frame_with_n_valid(n)
    vmap = torch.from_numpy(valid.reshape(H, W)).to(DEV)
    depth = torch.where(vmap, torch.full((H, W), 2.5, device=DEV), torch.zeros(H, W, device=DEV))
    if n >= 2:
        depth.view(-1)[int(np.flatnonzero(valid)[1])] = float("nan")
    seed = 1000 + n
    for k in sorted({0, 1, max(n - 1, 0), n, n + 1}):
        want, n_ref, m_ref = inputs.sample(valid, k, seed)
        for v, d in ((vmap, None), (None, depth[..., None])):
            idx, counts = export.sample_valid_pixels(v, d, k, seed)
            assert idx.dtype == torch.int32 and idx.shape == (k,) and counts.tolist() == [n_ref, m_ref] == [n, min(k, n)]
            got = idx.cpu().numpy().astype(np.int64)
            assert np.array_equal(got[:m_ref], want) and bool((got[m_ref:] == -1).all()), (k, v is None)
            assert len(set(got[:m_ref].tolist())) == m_ref and bool(valid[got[:m_ref]].all())


def test_sampler_is_deterministic_and_keyed(export):
    valid = _frame_with_n_valid(1000)
    vmap = torch.from_numpy(valid.reshape(70, 70)).to(DEV)
    a, ca = export.sample_valid_pixels(vmap, None, 100, seed=5)
    b, cb = export.sample_valid_pixels(vmap, None, 100, seed=5)
    c, _ = export.sample_valid_pixels(vmap, None, 100, seed=6)
    big, _ = export.sample_valid_pixels(vmap, None, 100, seed=5 + 2 ** 32)                  # the high word of the seed is part of the key
    assert torch.equal(a, b) and torch.equal(ca, cb)
    assert not torch.equal(a, c) and not torch.equal(a, big)
    assert np.array_equal(big.cpu().numpy(), inputs.sample(valid, 100, 5 + 2 ** 32)[0])
    picked = export.pick_indices_at_random(vmap[..., None], 100, seed=5)
    assert picked.dtype == torch.int64 and torch.equal(picked, a.long())
    assert torch.equal(export.pick_indices_at_random(vmap, 5000), torch.from_numpy(np.flatnonzero(valid)).to(DEV))


# ---- back-projection ---------------------------------------------------------------------------------------------------------------------


def _buffers(capacity, fill=float("nan")):
    mk = lambda: torch.full((capacity, 3), fill, dtype=torch.float32, device=DEV)            # noqa: E731
    return mk(), mk(), mk(), torch.zeros(3, dtype=torch.int64, device=DEV)


def _backproject(export, f, indices, mask=None, crop_box=None, normals=True, capacity=None, state=None, bufs=None):
    fx, fy, cx, cy = f["intr"]
    rows = f["depth"].numel() if indices is None else len(indices)
    if bufs is None:
        bufs = _buffers(capacity or max(rows, 1))
    points, colors, nrm, st = bufs
    export.backproject_points(f["depth"].to(DEV), f["rgb"].to(DEV), f["c2w_cv"], fx, fy, cx, cy, points=points, colors=colors,
                              normals=nrm if normals else None, state=st if state is None else state,
                              surface_normal=f["surface_normal"].to(DEV) if normals else None,
                              mask=None if mask is None else mask.to(DEV), indices=None if indices is None else indices.to(DEV),
                              crop_box=crop_box)
    return points.cpu(), colors.cpu(), nrm.cpu(), (st if state is None else state).tolist()


def _points_within(got, ref, f, depth, W, idx):
    fx, fy, cx, cy = f["intr"]
    bound = inputs.point_bound(depth, f["c2w_cv"], fx, fy, cx, cy, W, idx)
    err = (got.double() - ref.double()).abs()
    print(f"points: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def _normals_within(got, ref, f, idx):
    from dn_splatter_amd import torch_export as te

    n64 = te.world_normals(f["surface_normal"].double(), f["c2w_cv"].double())[idx]
    bound = inputs.normal_bound(n64, f["c2w_cv"])
    err = (got.double() - ref.double()).abs()
    print(f"normals: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("H,W", inputs.FIXTURE_FRAMES)
@pytest.mark.parametrize("tag", ("depth", "edges"))
def test_backprojection_of_the_fixtures_indices_equals_the_reference(g, export, H, W, tag):
    f = inputs.fixture_frame(g, H, W)
    pre = f["pre"]
    idx = torch.from_numpy(g[pre + f"pick_{tag}"]).long()
    m = len(idx)
    for mtag, mask in (("", None), ("_masked", f["mask"])):
        points, colors, normals, state = _backproject(export, f, idx, mask=mask)
        assert state == [m, 0, 0]
        d = f["depth"].clone()
        if mask is not None:
            d[~mask] = 0
        _points_within(points, torch.from_numpy(g[pre + f"points_{tag}{mtag}"]), f, d, W, idx)
        assert torch.equal(colors, f["rgb"].reshape(-1, 3)[idx])                            # bit for bit
        ref_n = torch.from_numpy(g[pre + f"normals_{tag}"])
        _normals_within(normals, ref_n, f, idx)
        border = (idx // W == 0) | (idx // W == H - 1) | (idx % W == 0) | (idx % W == W - 1)
        assert bool(border.any()) and bool((normals[border] == 0).all())                    # exact zeros
        if mask is not None:
            out = ~f["mask"].reshape(-1)[idx]
            assert bool(out.any()) and torch.equal(points[out], f["c2w_cv"][:3, 3].expand(int(out.sum()), 3))   # exactly t
    # the drop-in with the reference's signature, the index tensor as `mask`
    fx, fy, cx, cy = f["intr"]
    xyz, rgb = export.get_colored_points_from_depth(f["depth"].to(DEV), f["rgb"].to(DEV), f["c2w_cv"], fx, fy, cx, cy, (W, H), mask=idx.to(DEV))
    assert torch.equal(xyz.cpu(), points_of(export, f, idx)) and torch.equal(rgb.cpu(), f["rgb"].reshape(-1, 3)[idx])


def points_of(export, f, idx):
    return _backproject(export, f, idx, normals=False)[0]


@pytest.mark.parametrize("H,W", inputs.FIXTURE_FRAMES)
def test_all_pixels_equal_the_tsdf_fixture(g, export, H, W):
    f = inputs.fixture_frame(g, H, W)
    points, colors, _, state = _backproject(export, f, None, normals=False)
    assert state == [H * W, 0, 0]
    _points_within(points, torch.from_numpy(g[f["pre"] + "points_all"]), f, f["depth"], W, torch.arange(H * W))
    assert torch.equal(colors, f["rgb"].reshape(-1, 3))
    fx, fy, cx, cy = f["intr"]
    xyz, rgb = export.get_colored_points_from_depth(f["depth"].to(DEV), f["rgb"].to(DEV), f["c2w_cv"], fx, fy, cx, cy, (W, H))
    assert torch.equal(xyz.cpu(), points) and torch.equal(rgb.cpu(), colors)


def _crop_case(g):
    """The first fixture frame, its indices and a rotated box around the middle of its points; asserts in fp64 that no point lies
    within its error bound of a face (the allowed number is 0)."""
    from dn_splatter_amd import torch_export as te

    H, W = inputs.FIXTURE_FRAMES[0]
    f = inputs.fixture_frame(g, H, W)
    fx, fy, cx, cy = f["intr"]
    idx = torch.from_numpy(g[f["pre"] + "pick_depth"]).long()
    pts64, _ = te.get_colored_points_from_depth(f["depth"].double(), f["rgb"].double(), f["c2w_cv"].double(), fx, fy, cx, cy, (W, H), idx)
    a = 0.5
    R = torch.tensor([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    box = inputs.Box(R, pts64.median(dim=0).values.float(), torch.tensor([2.2, 1.6, 2.6]))
    B = torch.linalg.inv(te.box_to_world(box, torch.float64, "cpu"))
    q = pts64 @ B[:3, :3].T + B[:3, 3]
    half = box.S.double() / 2
    # the point's own bound carried through |B|, the rounding of B's fp32 inverse (4 u per entry, relative to its row), and the
    # 3 products and 3 additions of the test itself
    pb = inputs.point_bound(f["depth"], f["c2w_cv"], fx, fy, cx, cy, W, idx)
    mag = pts64.abs() @ B[:3, :3].abs().T + B[:3, 3].abs()
    err = pb @ B[:3, :3].abs().T + (8 + 4) * inputs.U24 * mag
    assert int(((q.abs() - half).abs() <= err).sum()) == 0
    inside = te.within(box, pts64)
    assert torch.equal(inside, (q.abs() < half).all(dim=-1)) and 50 < int(inside.sum()) < len(idx) - 50
    return f, idx, box, inside


def test_crop_box_keeps_the_restatements_rows_in_order(g, export):
    f, idx, box, inside = _crop_case(g)
    H, W = inputs.FIXTURE_FRAMES[0]
    full_p, full_c, full_n, _ = _backproject(export, f, idx)
    points, colors, normals, state = _backproject(export, f, idx, crop_box=box)
    kept = int(inside.sum())
    assert state == [kept, 0, 0]
    assert torch.equal(points[:kept], full_p[inside]) and torch.equal(colors[:kept], full_c[inside]) and torch.equal(normals[:kept], full_n[inside])
    assert bool(torch.isnan(points[kept:]).all())                                           # nothing behind the cursor was written
    _points_within(points[:kept], torch.from_numpy(g[f["pre"] + "points_depth"])[inside], f, f["depth"], W, idx[inside])
    # a box on the device gives the same rows
    dev_box = inputs.Box(box.R.to(DEV), box.T.to(DEV), box.S.to(DEV))
    p2, _, _, s2 = _backproject(export, f, idx, crop_box=dev_box)
    assert s2 == [kept, 0, 0] and torch.equal(p2[:kept], points[:kept])
    # an empty result leaves the cursor where it was
    far = inputs.Box(torch.eye(3), torch.tensor([1e3, 0.0, 0.0]), torch.ones(3))
    bufs = _buffers(len(idx))
    bufs[3][0] = 17
    p3, _, _, s3 = _backproject(export, f, idx, crop_box=far, bufs=bufs)
    assert s3 == [17, 0, 0] and bool(torch.isnan(p3).all())


def test_frames_append_back_to_back_and_overflow_is_reported(g, export):
    from dn_splatter_amd import DnsplatError

    frames = [inputs.fixture_frame(g, H, W) for H, W in inputs.FIXTURE_FRAMES]
    idxs = [torch.from_numpy(g[f["pre"] + "pick_depth"]).long() for f in frames]
    m = inputs.SAMPLES
    alone = [_backproject(export, f, i) for f, i in zip(frames, idxs)]
    bufs = _buffers(3 * m)
    for f, i in zip(frames, idxs):
        points, colors, normals, state = _backproject(export, f, i, bufs=bufs)
    assert state == [3 * m, 0, 0]
    for k in range(3):
        assert torch.equal(points[k * m:(k + 1) * m], alone[k][0][:m]) and torch.equal(colors[k * m:(k + 1) * m], alone[k][1][:m])
        assert torch.equal(normals[k * m:(k + 1) * m], alone[k][2][:m])
    # one row short: the last row is not written, memory past capacity stays as it was, the overflow word is raised
    cap = 3 * m - 1
    big = _buffers(cap + 8, fill=-7.0)
    short = tuple(b[:cap] for b in big[:3]) + (big[3],)
    for f, i in zip(frames, idxs):
        _, _, _, state = _backproject(export, f, i, bufs=short)
    assert state == [cap, 1, 0]
    torch.cuda.synchronize()
    for b, whole in zip(big[:3], (points, colors, normals)):
        assert bool((b[cap:] == -7.0).all()) and torch.equal(b[:cap].cpu(), whole[:cap])
    # the same through the class: finish() raises
    cams = [inputs.Cam(f["c2w_gl"], *f["intr"], W, H) for f, (H, W) in zip(frames, inputs.FIXTURE_FRAMES)]
    outs = [dict(depth=f["depth"].to(DEV), rgb=f["rgb"].to(DEV), surface_normal=f["surface_normal"].to(DEV)) for f in frames]
    cloud = export.OrientedPointCloud(cap, DEV)
    for o, c, i in zip(outs, cams, idxs):
        cloud.add_frame(o, c, samples_per_frame=m, indices=i.to(DEV))
    with pytest.raises(DnsplatError, match="overflow"):
        cloud.finish()
    cloud = export.OrientedPointCloud(3 * m, DEV)
    for o, c, i in zip(outs, cams, idxs):
        cloud.add_frame(o, c, samples_per_frame=m, indices=i.to(DEV))
    p, n, c = cloud.finish()
    assert torch.equal(p.cpu(), points) and torch.equal(n.cpu(), normals) and torch.equal(c.cpu(), colors)
    # an index outside the frame is dropped and reported
    cloud = export.OrientedPointCloud(8, DEV)
    cloud.add_frame(outs[0], cams[0], samples_per_frame=3, indices=torch.tensor([5, 45 * 70, 7], device=DEV))
    with pytest.raises(DnsplatError, match="outside"):
        cloud.finish()
    assert cloud.state.tolist() == [2, 0, 1]


# ---- the loop ------------------------------------------------------------------------------------------------------------------------------


def test_add_frame_never_synchronises_and_the_restatement_does(g, export):
    """Under torch's synchronisation check: add_frame with and without the edge filter and a crop box passes (pose and box on the
    device); the restatement — the reference's nonzero, randperm and boolean-mask crop — is refused."""
    from dn_splatter_amd import torch_export as te

    H, W = inputs.FIXTURE_FRAMES[0]
    f, _, box, _ = _crop_case(g)
    cam = inputs.Cam(f["c2w_gl"].to(DEV), *f["intr"], W, H)
    out = dict(depth=f["depth"].to(DEV), rgb=f["rgb"].to(DEV), surface_normal=f["surface_normal"].to(DEV))
    dev_box = inputs.Box(box.R.to(DEV), box.T.to(DEV), box.S.to(DEV))
    mask = f["mask"].to(DEV)
    configs = [dict(), dict(filter_edges=True), dict(crop_box=dev_box), dict(filter_edges=True, crop_box=dev_box, mask=mask)]
    warm = export.OrientedPointCloud(4 * inputs.SAMPLES, DEV)
    for kw in configs:
        warm.add_frame(out, cam, samples_per_frame=inputs.SAMPLES, seed=3, **kw)
    want = [t.clone() for t in warm.finish()]
    cloud = export.OrientedPointCloud(4 * inputs.SAMPLES, DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for kw in configs:
            cloud.add_frame(out, cam, samples_per_frame=inputs.SAMPLES, seed=3, **kw)
        with pytest.raises(RuntimeError):
            te.pick_indices_at_random(out["depth"], inputs.SAMPLES)                        # nonzero: the size of its result
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = cloud.finish()
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and inputs.SAMPLES < len(got[0]) < 4 * inputs.SAMPLES


@pytest.mark.parametrize("filter_edges", (False, True))
def test_export_oriented_points_equals_a_loop_of_the_restatement(dns, export, filter_edges):
    """300 Gaussians, 4 cameras of 40 x 56, total_points = 500: samples_per_frame = 126, frame f drawn with seed + f.  Against the
    restatement's frame_points fed the HIP sampler's indices, frame by frame."""
    from dn_splatter_amd import synthetic, torch_export as te

    W, H, F_, seed = 56, 40, 4, 11
    gp = synthetic.make_gauss_params(300, sh_rest_std=0.1, seed=2)
    params = {k: v.detach().to(DEV) for k, v in gp.items()}
    renderer = dns.DNSplatterRenderer(params)
    cameras = [synthetic.orbit_camera(i, n_views=F_, width=W, height=H, focal=45.0).to(DEV) for i in range(F_)]
    points, normals, colors = export.export_oriented_points(renderer, cameras, total_points=500, filter_edges=filter_edges, seed=seed)
    samples = (500 + F_) // F_
    assert samples == 126
    outs = renderer.get_outputs_batch(cameras)
    at = 0
    for fi, (out, cam) in enumerate(zip(outs, cameras)):
        valid = export.depth_edge_valid(out["depth"], 0.004, 10) if filter_edges else None
        idx, counts = export.sample_valid_pixels(valid, out["depth"], samples, seed + fi)
        n, m = counts.tolist()
        assert m == min(n, samples)
        if m == 0:
            continue
        idx = idx[:m].long()
        if filter_edges:                                                                     # the restatement's map, where no decision is borderline
            d = out["depth"][..., 0].cpu()
            if int(inputs.flagged_edge_decisions(d, 0.004).sum()) == 0:
                assert torch.equal(valid.cpu(), _valid64(d, 0.004, 10))
        xyz, nrm, rgb = te.frame_points(out, cam, samples, indices=idx)
        c2w_cv = te.export_c2w(cam.camera_to_worlds).cpu()
        f = dict(intr=(cam.fx, cam.fy, cam.cx, cam.cy), c2w_cv=c2w_cv, surface_normal=out["surface_normal"].cpu())
        _points_within(points[at:at + m].cpu(), xyz.cpu(), f, out["depth"].cpu(), W, idx.cpu())
        _normals_within(normals[at:at + m].cpu(), nrm.cpu(), f, idx.cpu())
        assert torch.equal(colors[at:at + m], rgb)
        at += m
    assert at == len(points) == len(normals) == len(colors) and at > 0
