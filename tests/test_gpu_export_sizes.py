"""The mesh-export kernels past the sizes at which their one-workgroup loops run once: the k-NN index (csrc/density.hip,
density_common.h), the sampler and the back-projection append (csrc/pointcloud.hip), the level-set points append (csrc/levelset.hip) and
marching cubes (csrc/marching.hip).  test_gpu_density.py, test_gpu_export.py, test_gpu_levelset.py and test_gpu_marching.py hold these
kernels to their fp64 / NumPy restatements at sizes where every such loop makes ONE trip; what the loops carry between trips is held here.

Every comparison is exact, or reuses a bound those files state (_export_inputs.point_bound / normal_bound, _density_inputs.GAP): no new
tolerance.  Every case asserts, from the constants below, that its shape lies on the far side of the edge it is named for, and has its
one-trip control beside it; ``test_constants_are_the_kernels`` reads the constants out of the sources, so that a retuned kernel fails
here instead of silently falling back to one trip.

Heavy cells are out of scope on purpose: df_order_kernel ranks a point against every other point of its cell, so a cell of 10^5 points
costs 10^10 reads (the density section).  All means here are uniform; each index case asserts its fullest cell stays small."""
import os
import re

import numpy as np
import pytest
import torch

import _density_inputs as density_inputs
import _export_inputs as frames
import _levelset_inputs as level_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24

WAVE = 64                       # splat_common.h DNS_WAVE
KNN_MAX_GRID = 128              # include/dnsplat.h DNSPLAT_KNN_MAX_GRID
DF_THREADS = 256                # density_common.h: points per workgroup of the build kernels; levelset.hip LS_THREADS is the same constant
DF_SCAN_THREADS = 1024          # df_scan_kernel: one workgroup ...
DF_SCAN_PER = 4                 # ... of 4 entries per thread: 4096 cell counts per trip
DF_MINMAX_BLOCKS = 256          # the cap of df_minmax_kernel's grid
PC_THREADS = 256                # pointcloud.hip: rows per workgroup of the appends, block counts per trip of the one-workgroup scans
PC_SAMPLE_PER = 4               # pixels per thread of the sampler's count kernel: 1024 pixels per block count
MC_THREADS = 256                # marching.hip: threads of mc_scan_bases
MC_SCAN_WORDS = 1024            # words of 64 lattice points per scan block
DF_SCAN_TRIP = DF_SCAN_THREADS * DF_SCAN_PER
PC_SAMPLE_BLOCK = PC_THREADS * PC_SAMPLE_PER
LS_THREADS = DF_THREADS


def _ceil(a, b):
    return (a + b - 1) // b


@pytest.fixture(scope="module")
def density(dns):
    from dn_splatter_amd import density as d

    return d


@pytest.fixture(scope="module")
def td():
    from dn_splatter_amd import torch_density as t

    return t


@pytest.fixture(scope="module")
def export(dns):
    from dn_splatter_amd import export as ex

    return ex


@pytest.fixture(scope="module")
def te():
    from dn_splatter_amd import torch_export as t

    return t


def test_constants_are_the_kernels(dns):
    """The constants the cases below reason from are the ones the sources compile."""
    from dn_splatter_amd import torch_marching

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(os.path.dirname(os.path.abspath(torch_marching.__file__)), "csrc")      # where it reads mc_table.h

    def rhs(path, name):
        text = open(path).read()
        found = re.search(r"(?:constexpr int|#define)\s+" + name + r"\b\s*=?\s*([^;\n/]+)", text)
        assert found, (path, name)
        return found.group(1).strip()

    want = {("splat_common.h", "DNS_WAVE"): WAVE, ("density_common.h", "DF_THREADS"): DF_THREADS,
            ("density_common.h", "DF_SCAN_THREADS"): DF_SCAN_THREADS, ("density_common.h", "DF_SCAN_PER"): DF_SCAN_PER,
            ("density_common.h", "DF_MINMAX_BLOCKS"): DF_MINMAX_BLOCKS, ("pointcloud.hip", "PC_THREADS"): PC_THREADS,
            ("pointcloud.hip", "PC_SAMPLE_PER"): PC_SAMPLE_PER, ("marching.hip", "MC_THREADS"): MC_THREADS,
            ("marching.hip", "MC_SCAN_WORDS"): MC_SCAN_WORDS}
    for (name, const), value in want.items():
        assert int(rhs(os.path.join(csrc, name), const)) == value, (name, const)
    assert rhs(os.path.join(csrc, "levelset.hip"), "LS_THREADS") == "DF_THREADS"
    assert rhs(os.path.join(csrc, "pointcloud.hip"), "PC_SAMPLE_BLOCK") == "PC_THREADS * PC_SAMPLE_PER"
    assert int(rhs(os.path.join(root, "include", "dnsplat.h"), "DNSPLAT_KNN_MAX_GRID")) == KNN_MAX_GRID == density_inputs.KNN_MAX_GRID


# ---- 1. the k-NN index -----------------------------------------------------------------------------------------------------------------

#   N          what it is the first (or last) size of
INDEX_N = (8191,        # G = 15, 3376 entries: the last size with one scan trip — the control
           8192,        # G = 16, 4097 entries: a second trip that holds exactly one entry
           16385,       # 65 min / max partials: the header's second pass; G = 20, two trips
           65537,       # 257 workgroups' worth of points on the 256-workgroup grid: the min / max stride loop; G = 32, nine trips
           4194304,     # G = 128 reached without the clamp
           4293378)     # 2 x 129^3: the clamp active
SEARCH_N = (8192, 65537, 4293378)
SEARCH_KS = ((16, 1), (31, 1))
RANKS = 33                      # ranks 0 .. 32 of every query enter the gap condition (k + skip = 32, and the one behind)
_INDEX = {}


def _index_case(density, N):
    """(means on the device, the NumPy restatement, the index), once per N."""
    if N not in _INDEX:
        means = density_inputs.uniform_means(N, seed=500 + N % 1000)
        ref = density_inputs.index_restatement(means)
        dev = means.to(DEV)
        _INDEX[N] = (dev, ref, density.build_index(dev))
    return _INDEX[N]


def _assert_index_edge(N):
    """The loops of dnsplat_knn_build that N reaches, from the constants."""
    G = density_inputs.index_grid_dim(N)
    free = density_inputs.index_grid_dim(N, cap=10 ** 9)
    entries = G ** 3 + 1
    trips, partials = _ceil(entries, DF_SCAN_TRIP), min(_ceil(N, DF_THREADS), DF_MINMAX_BLOCKS)
    stride = _ceil(N, DF_THREADS) > DF_MINMAX_BLOCKS
    if N == 8191:
        assert (G, entries, trips, partials, stride) == (15, 3376, 1, 32, False)
    elif N == 8192:
        assert (G, entries, trips) == (16, DF_SCAN_TRIP + 1, 2) and partials <= WAVE and not stride
    elif N == 16385:
        assert partials == WAVE + 1 and not stride and (G, trips) == (20, 2)
    elif N == 65537:
        assert _ceil(N, DF_THREADS) == DF_MINMAX_BLOCKS + 1 and stride and partials == DF_MINMAX_BLOCKS > WAVE
        assert (G, trips) == (32, 9) and entries == 8 * DF_SCAN_TRIP + 1
    elif N == 4194304:
        assert G == free == KNN_MAX_GRID and N == 2 * KNN_MAX_GRID ** 3 and stride and trips == 513
    elif N == 4293378:
        assert N == 2 * (KNN_MAX_GRID + 1) ** 3 and free == KNN_MAX_GRID + 1 and G == KNN_MAX_GRID and stride
    else:
        raise KeyError(N)


@pytest.mark.parametrize("N", INDEX_N)
def test_index_bytes_equal_the_restatement(density, N):
    """What a query reads of the index buffer — the 64-byte header with its zero padding, cell_start with its zeroed alignment
    padding, the sorted copy — against _density_inputs.index_restatement, as bytes.  Every cell, which random queries cannot reach."""
    _assert_index_edge(N)
    means, ref, index = _index_case(density, N)
    G, C = ref["G"], ref["C"]
    assert density._lib.lib().dnsplat_knn_grid_dim(N) == G and tuple(ref["g"].tolist()) == (G, G, G)
    kept = 64 + ((4 * (C + 1) + 15) // 16) * 16 + 16 * N                       # the layout test_two_builds_give_equal_bits spells out
    assert ref["bytes"].size == kept and int(ref["cell_start"][-1]) == N and int(ref["cell_start"][0]) == 0
    fullest = int(np.diff(ref["cell_start"]).max())
    assert fullest < 64, fullest                                             # no heavy cell: the in-cell ordering stays cheap
    got = index.buffer.view(torch.uint8)[:kept]
    want = torch.from_numpy(ref["bytes"]).to(DEV)
    at = ref["at_sorted"]
    assert torch.equal(got[:64], want[:64]), "header"
    starts_got, starts_want = got[64:at].view(torch.int32), want[64:at].view(torch.int32)
    wrong = torch.nonzero(starts_got != starts_want).reshape(-1)
    assert wrong.numel() == 0, f"cell_start: {wrong.numel()} entries differ, the first at {int(wrong[0])} of {C + 1}"
    assert torch.equal(got[at:], want[at:]), "sorted"
    assert torch.equal(got, want)


def _queries(means, ref, seed):
    """64 queries: the 8 means with the largest cell id and the 8 with the smallest (the last and the first cell_start entries), 40
    uniform in the box, 8 far outside it (field_inputs' law for those)."""
    g = torch.Generator().manual_seed(seed)
    order = torch.from_numpy(ref["order"])
    inside = (torch.rand(40, 3, generator=g) - 0.5) * 10
    far = (torch.rand(8, 3, generator=g) - 0.5) * 10 + torch.tensor([[40.0, -25.0, 60.0]]) * torch.sign(torch.randn(8, 3, generator=g))
    return torch.cat([means[order[-8:]], means[order[:8]], inside, far]).float().contiguous()


@pytest.mark.parametrize("N", SEARCH_N)
def test_search_is_index_exact_past_the_edges(density, td, N):
    """index.query against the fp64 brute force on the device: indices equal, d² the double rounded once.  One brute-force call ranks
    0 .. 32; (k, skip) of torch_density.knn is a slice of those columns."""
    _assert_index_edge(N)
    means, ref, index = _index_case(density, N)
    q = _queries(means.cpu(), ref, seed=900 + N % 1000).to(DEV)
    assert q.shape[0] == 64
    cells = torch.from_numpy(ref["cell"])[torch.from_numpy(ref["order"])]
    assert int(cells[-1]) == int(ref["cell"].max()) and int(cells[0]) == int(ref["cell"].min())
    rank, d2 = td.knn(means, q, RANKS, 0, return_d2=True, chunk=16 if N > 2 ** 20 else 4096)
    gap = float(((d2[:, 1:] - d2[:, :-1]) / d2[:, 1:].clamp_min(1e-300)).min())
    print(f"N = {N}: smallest relative gap of ranks 0 .. {RANKS - 1}: {gap:.3e} (needs > {density_inputs.GAP:.3e})")
    assert gap > density_inputs.GAP                                          # of all 64 queries: none is excluded
    for k, skip in SEARCH_KS:
        got, got_d2 = index.query(q, k, skip, return_d2=True)
        assert torch.equal(got.long(), rank[:, skip:skip + k]), (N, k, skip)
        assert torch.equal(got_d2, d2[:, skip:skip + k].float()), (N, k, skip)
    assert torch.equal(rank[:16, 0].cpu(), torch.from_numpy(np.concatenate([ref["order"][-8:], ref["order"][:8]])))   # a mean finds itself


# ---- 2. the sampler and the two appends past 256 block counts -------------------------------------------------------------------------

CLEARED = (100 * PC_SAMPLE_BLOCK + 300, 2 * PC_SAMPLE_BLOCK)                   # start and length of the run of cleared pixels


def _validity(H, W):
    """About half the pixels at random, the last one set, 2048 consecutive ones cleared."""
    valid = np.random.default_rng(7000 + H).random(H * W) < 0.5
    valid[CLEARED[0]:CLEARED[0] + CLEARED[1]] = False
    valid[-1] = True
    return valid


@pytest.mark.parametrize("H,W", [(512, 512), (513, 512)], ids=["256_blocks_one_trip", "257_blocks_two_trips"])
def test_sampler_past_256_block_counts(export, H, W):
    """dnsplat_sample_valid_pixels against _export_inputs.sample: {n, m} and the indices, from both validity sources."""
    P = H * W
    nb = _ceil(P, PC_SAMPLE_BLOCK)
    if H == 512:
        assert nb == PC_THREADS and P % PC_SAMPLE_BLOCK == 0                 # the control: one trip of pc_scan_kernel
    else:
        assert nb == PC_THREADS + 1 and P % PC_SAMPLE_BLOCK == PC_SAMPLE_BLOCK // 2      # a second trip of one, half full block
    valid = _validity(H, W)
    per_block = np.bincount(np.flatnonzero(valid) // PC_SAMPLE_BLOCK, minlength=nb)
    assert int((per_block == 0).sum()) >= 1 and per_block[-1] > 0 and bool(valid[-1])
    n = int(valid.sum())
    assert 0.45 * P < n < 0.55 * P
    vmap = torch.from_numpy(valid.reshape(H, W)).to(DEV)
    depth = torch.where(vmap, torch.full((H, W), 2.5, device=DEV), torch.zeros(H, W, device=DEV))
    depth.view(-1)[int(np.flatnonzero(valid)[1])] = float("nan")            # a nan depth is valid, as for torch.nonzero
    seed = 4000 + H
    for k in (1, 20000, n - 1, n, n + 1):
        want, n_ref, m_ref = frames.sample(valid, k, seed)
        assert (n_ref, m_ref) == (n, min(k, n))
        for v, d in ((vmap, None), (None, depth[..., None])):
            idx, counts = export.sample_valid_pixels(v, d, k, seed)
            assert idx.dtype == torch.int32 and idx.shape == (k,) and counts.tolist() == [n, m_ref], (k, v is None)
            got = idx.cpu().numpy().astype(np.int64)
            assert np.array_equal(got[:m_ref], want) and bool((got[m_ref:] == -1).all()), (k, v is None)


_FRAMES = {}
BOX_ANGLE, BOX_SIZE, BOX_ROWS = 0.5, (20.0, 16.0, 20.0), 80


def _bp_case(te, H, W):
    """The recipe's frame and camera, the fp64 restatement of all its pixels, and a rotated crop box around the median point of the
    last 80 image rows — so that it keeps rows of the LAST row block, the one behind the scan's carry, which a box around the middle
    of this wide frame does not — no face of which lies within a point's error bound (asserted, the allowed number is 0).  Once per
    frame size."""
    if (H, W) not in _FRAMES:
        f = frames.frame_inputs(H, W)
        c2w_gl, fx, fy, cx, cy = frames.camera(H, W)
        f.update(c2w_cv=te.export_c2w(c2w_gl.reshape(3, 4)), intr=(fx, fy, cx, cy))
        every = torch.arange(H * W)
        pts64, _ = te.get_colored_points_from_depth(f["depth"].double(), f["rgb"].double(), f["c2w_cv"].double(), fx, fy, cx, cy, (W, H))
        n64 = te.world_normals(f["surface_normal"].double(), f["c2w_cv"].double())
        R = torch.tensor([[np.cos(BOX_ANGLE), -np.sin(BOX_ANGLE), 0.0], [np.sin(BOX_ANGLE), np.cos(BOX_ANGLE), 0.0], [0.0, 0.0, 1.0]],
                         dtype=torch.float32)
        box = frames.Box(R, pts64[-BOX_ROWS * W:].median(dim=0).values.float(), torch.tensor(BOX_SIZE))
        B = torch.linalg.inv(te.box_to_world(box, torch.float64, "cpu"))
        q = pts64 @ B[:3, :3].T + B[:3, 3]
        half = box.S.double() / 2
        # as test_gpu_export._crop_case: the point's own bound carried through |B|, the rounding of B's fp32 inverse, the test's own sums
        pb = frames.point_bound(f["depth"], f["c2w_cv"], fx, fy, cx, cy, W, every)
        mag = pts64.abs() @ B[:3, :3].abs().T + B[:3, 3].abs()
        err = pb @ B[:3, :3].abs().T + (8 + 4) * U24 * mag
        assert int(((q.abs() - half).abs() <= err).sum()) == 0
        inside = te.within(box, pts64)
        assert torch.equal(inside, (q.abs() < half).all(dim=-1)) and H * W // 4 < int(inside.sum()) < 3 * H * W // 4
        per_block = torch.bincount(torch.nonzero(inside).reshape(-1) // PC_THREADS, minlength=_ceil(H * W, PC_THREADS))
        assert int(per_block[-1]) > 5 and int((per_block == 0).sum()) > 0          # rows kept behind the carry; blocks that count 0
        _FRAMES[(H, W)] = dict(f=f, pts64=pts64, n64=n64, box=box, inside=inside, bound=pb, nbound=frames.normal_bound(n64, f["c2w_cv"]))
    return _FRAMES[(H, W)]


def _append(export, f, crop_box, points, colors, normals, state):
    fx, fy, cx, cy = f["intr"]
    export.backproject_points(f["depth"].to(DEV), f["rgb"].to(DEV), f["c2w_cv"], fx, fy, cx, cy, points=points, colors=colors, normals=normals,
                              state=state, surface_normal=f["surface_normal"].to(DEV), crop_box=crop_box)


def _buffers(rows, fill):
    mk = lambda: torch.full((rows, 3), fill, dtype=torch.float32, device=DEV)            # noqa: E731
    return mk(), mk(), mk()


@pytest.mark.parametrize("H,W", [(256, 256), (257, 256)], ids=["256_blocks_one_trip", "257_blocks_two_trips"])
def test_backprojection_of_all_pixels_past_256_row_blocks(export, te, H, W):
    """dnsplat_backproject_points over every pixel (indices=None), without and with a crop box, against torch_export in float64:
    count, kept rows in order, points and normals within their bounds, colours bit for bit, nothing behind the cursor."""
    P = H * W
    nb = _ceil(P, PC_THREADS)
    assert nb == (PC_THREADS if H == 256 else PC_THREADS + 1)                # one trip of dns_append_scan_kernel, or a second of one block
    case = _bp_case(te, H, W)
    f, inside = case["f"], case["inside"]
    guard = 8
    full = None
    for box in (None, case["box"]):
        keep = torch.ones(P, dtype=torch.bool) if box is None else inside
        kept = int(keep.sum())
        points, colors, normals = _buffers(P + guard, float("nan"))
        state = torch.zeros(3, dtype=torch.int64, device=DEV)
        _append(export, f, box, points, colors, normals, state)
        assert state.tolist() == [kept, 0, 0], box is None
        points, colors, normals = points.cpu(), colors.cpu(), normals.cpu()
        for buf in (points, colors, normals):
            assert bool(torch.isnan(buf[kept:]).all())                       # nothing behind the cursor was written
        err = (points[:kept].double() - case["pts64"][keep]).abs()
        print(f"{H} x {W}, box {box is not None}: points, worst error / bound {float((err / case['bound'][keep]).max()):.3f}")
        assert bool((err <= case["bound"][keep]).all())
        nerr = (normals[:kept].double() - case["n64"][keep]).abs()
        print(f"{H} x {W}, box {box is not None}: normals, worst error / bound {float((nerr / case['nbound'][keep].clamp_min(1e-300)).max()):.3f}")
        assert bool((nerr <= case["nbound"][keep]).all())
        assert torch.equal(colors[:kept], f["rgb"].reshape(-1, 3)[keep])                    # bit for bit
        if box is None:
            full = (points, colors, normals)
        else:                                                                # the kept rows are the uncropped call's, in order
            for got, whole in zip((points, colors, normals), full):
                assert torch.equal(got[:kept].view(torch.int32), whole[:P][keep].view(torch.int32))


def test_backprojection_overflow_past_256_row_blocks(export, te):
    """The 257 x 256 frame with its crop box, the cursor starting at 17 in buffers five rows short: the overflow word, the cursor at
    capacity, the rows before capacity those of a call with room, the rows before the cursor and the guard rows untouched."""
    H, W = 257, 256
    assert _ceil(H * W, PC_THREADS) == PC_THREADS + 1
    case = _bp_case(te, H, W)
    f, box, kept = case["f"], case["box"], int(case["inside"].sum())
    roomy = _buffers(kept, float("nan"))
    state = torch.zeros(3, dtype=torch.int64, device=DEV)
    _append(export, f, box, *roomy, state)
    assert state.tolist() == [kept, 0, 0]
    start, guard = 17, 8
    cap = start + kept - 5
    big = _buffers(cap + guard, -7.0)
    state = torch.tensor([start, 0, 0], dtype=torch.int64, device=DEV)
    _append(export, f, box, *(b[:cap] for b in big), state)
    assert state.tolist() == [cap, 1, 0]
    for b, whole in zip(big, roomy):
        assert bool((b[:start] == -7.0).all()) and bool((b[cap:] == -7.0).all())
        assert torch.equal(b[start:cap].view(torch.int32), whole[:kept - 5].view(torch.int32))


# the level-set points


@pytest.fixture(scope="module")
def level_case(dns):
    """_levelset_inputs.scene(257, 256, N=3600), its field and ONE level_rays call, shared by the cases below."""
    from dn_splatter_amd import density as d, levelset as ls

    H, W = 257, 256
    gp, fr, cam = level_inputs.scene(H, W, N=3600)
    field = d.GaussianDensityField(*(gp[k].to(DEV) for k in ("means", "scales", "quats", "opacities")))
    dev_cam = frames.Cam(cam.camera_to_worlds.to(DEV), cam.fx, cam.fy, cam.cx, cam.cy, W, H)
    depth, rgb, mask = fr["depth"].to(DEV), fr["rgb"].to(DEV), fr["mask"].to(DEV)
    rays = ls.level_rays(field, depth, dev_cam, mask=mask, surface_levels=level_inputs.LEVELS)
    return dict(ls=ls, H=H, W=W, field=field, cam=dev_cam, depth=depth, rgb=rgb, mask=mask, rays=rays, normals=gp["normals"].to(DEV))


SPREAD = 25601                  # odd and no multiple of 257: j -> SPREAD j mod 257 * 256 is a bijection of the frame's pixels


def _level_indices(P, order):
    """``raster``: arange(P).  ``spread``: the pixels in the order SPREAD j mod P, which puts hits of the frame's middle — the only part
    of this frame a Gaussian is near — into every row block of the call, the 257th included."""
    j = torch.arange(P, dtype=torch.int64)
    return (j if order == "raster" else (j * SPREAD) % P).to(torch.int32)


def _level_points(c, l, indices, mode, box, bufs, state):
    c["ls"].level_points(c["field"], c["depth"], c["rgb"], c["cam"], c["rays"]["t_hit"][l], c["rays"]["closest"], indices.contiguous(), None,
                         points=bufs[0], colors=bufs[1], normals=bufs[2], state=state, gauss_normals=c["normals"], mask=c["mask"],
                         return_normal=mode, crop_box=box)


@pytest.mark.parametrize("order", ["raster", "spread"])
@pytest.mark.parametrize("mode", ["closest_gaussian", "analytical"])
def test_level_points_past_256_row_blocks(level_case, te, mode, order):
    """dnsplat_level_points over all 65 792 pixels in one call (257 row blocks: two trips of dns_append_scan_kernel) equals, row for row and bit
    for bit, the same rows appended in two calls of at most 65 536 — the one-trip path test_gpu_levelset.py holds to the fp64
    restatement.  Independently: the count is the number of listed pixels with a hit (inside the box, where there is one), and
    without a box the colours are those pixels' in list order.

    In raster order this frame's hits all lie in row blocks 87 .. 165 (a 257 x 256 frame of this camera sees the sheet of Gaussians
    only around its middle), so the second trip adds an empty block there; the ``spread`` order is the one that puts kept rows into
    every block and behind the carry, and asserts it."""
    c = level_case
    P = c["H"] * c["W"]
    assert _ceil(P, LS_THREADS) == LS_THREADS + 1
    split = LS_THREADS * LS_THREADS                                          # 65 536 rows: the most one trip takes
    assert split < P and _ceil(P - split, LS_THREADS) == 1
    indices = _level_indices(P, order).to(DEV)
    assert torch.equal(torch.sort(indices).values, torch.arange(P, dtype=torch.int32, device=DEV))
    for l in range(len(level_inputs.LEVELS)):
        hit = ~torch.isnan(c["rays"]["t_hit"][l])
        assert torch.equal(hit, c["rays"]["valid"][l])
        listed = hit[indices.long()]                                         # by row of the call
        n_hit = int(listed.sum())
        per_block = torch.bincount(torch.nonzero(listed).reshape(-1) // LS_THREADS, minlength=LS_THREADS + 1)
        assert n_hit > 1000
        if order == "spread":
            assert int(per_block.min()) > 0 and int(per_block[-1]) > 0          # kept rows in every block, the one behind the carry included
        whole = _buffers(P, -7.0)
        state = torch.zeros(3, dtype=torch.int64, device=DEV)
        _level_points(c, l, indices, mode, None, whole, state)
        assert state.tolist() == [n_hit, 0, 0], (l, mode)
        assert torch.equal(whole[1][:n_hit], c["rgb"].reshape(-1, 3)[indices.long()[listed]])
        assert all(bool((b[n_hit:] == -7.0).all()) for b in whole)
        # a box around the median hit; no hit within the rounding envelope of a face (test_gpu_levelset's condition)
        pts64 = whole[0][:n_hit].double().cpu()
        R = torch.tensor([[np.cos(0.5), -np.sin(0.5), 0.0], [np.sin(0.5), np.cos(0.5), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
        box = frames.Box(R, pts64.median(dim=0).values.float(), torch.tensor([3.0, 2.2, 3.4]))
        B = torch.linalg.inv(te.box_to_world(box, torch.float64, "cpu"))
        q = pts64 @ B[:3, :3].T + B[:3, 3]
        half = box.S.double() / 2
        mag = pts64.abs() @ B[:3, :3].abs().T + B[:3, 3].abs()
        assert int(((q.abs() - half).abs() <= 16 * U24 * mag).sum()) == 0
        inside = te.within(box, pts64)
        n_in = int(inside.sum())
        assert n_hit // 8 < n_in < n_hit - n_hit // 8
        if order == "spread":                                                # the box keeps rows of the last block too
            assert int((torch.nonzero(listed).reshape(-1).cpu()[inside] >= split).sum()) > 0
        for crop, n_want in ((None, n_hit), (box, n_in)):
            one = whole if crop is None else _buffers(P, -7.0)
            if crop is not None:
                state = torch.zeros(3, dtype=torch.int64, device=DEV)
                _level_points(c, l, indices, mode, crop, one, state)
                assert state.tolist() == [n_want, 0, 0], (l, mode)
                for got, full in zip(one, whole):                            # the rows inside the box, in order
                    assert torch.equal(got[:n_want].view(torch.int32), full[:n_hit][inside.to(DEV)].view(torch.int32))
            two = _buffers(P, -7.0)
            state = torch.zeros(3, dtype=torch.int64, device=DEV)
            _level_points(c, l, indices[:split], mode, crop, two, state)
            first = int(state[0])
            _level_points(c, l, indices[split:], mode, crop, two, state)
            assert state.tolist() == [n_want, 0, 0] and first <= n_want
            if order == "spread" and crop is None:
                assert first == n_want - int(per_block[-1]) < n_want             # the second call appends the last block's rows
            for a, b in zip(one, two):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (l, mode, crop is not None)


# ---- 3. marching cubes past 256 scan blocks -------------------------------------------------------------------------------------------


def _mc_volume(planes):
    """[planes,256,256]: a sphere of radius 60.4 centred off the lattice points (level 0) and the planes 0, 1, 255 and (where there is
    one) 256 filled with rand - 0.5."""
    shape = (planes, 256, 256)
    axes = [np.arange(n, dtype=np.float64) - c for n, c in zip(shape, (127.37, 126.61, 129.13))]
    r = np.sqrt(axes[0][:, None, None] ** 2 + axes[1][None, :, None] ** 2 + axes[2][None, None, :] ** 2)
    vol = (60.4 - r).astype(np.float32)
    rng = np.random.default_rng(2570)
    for i in (0, 1, 255, 256):
        noise = rng.random((256, 256), dtype=np.float32) - np.float32(0.5)
        if i < planes:
            vol[i] = noise
    return vol


@pytest.mark.parametrize("planes", [256, 257], ids=["256_blocks_per_1", "257_blocks_per_2"])
def test_marching_cubes_past_256_scan_blocks(dns, planes):
    """mc_scan_bases gives each of its 256 threads ceil(blocks / 256) scan blocks: 1 up to 256 blocks, 2 at 257 — where thread 128 takes
    the single last block and the threads behind it none.  Against torch_marching as test_gpu_marching.check compares: counts,
    triangles as integers, vertices as bit patterns."""
    from dn_splatter_amd import marching as mc, torch_marching as tm

    shape = (planes, 256, 256)
    assert shape[1] * shape[2] == WAVE * MC_SCAN_WORDS                       # with i the slowest axis, plane i is scan block i
    blocks = _ceil(_ceil(planes * 256 * 256, WAVE), MC_SCAN_WORDS)
    per = _ceil(blocks, MC_THREADS)
    assert blocks == planes and per == (1 if planes == 256 else 2)
    if planes == 257:
        assert min(128 * per, blocks) == 256 and min(128 * per + per, blocks) - 256 == 1 and min(129 * per, blocks) == blocks
    vol = _mc_volume(planes)
    want_v, want_t = tm.marching_cubes(vol, 0.0)
    got_v, got_t = mc.marching_cubes(torch.from_numpy(vol).to(DEV), 0.0)
    assert got_v.dtype == torch.float32 and got_t.dtype == torch.int32
    print(f"{shape}: {len(want_v)} vertices, {len(want_t)} triangles")
    assert (got_v.shape[0], got_t.shape[0]) == (len(want_v), len(want_t))
    got_v, got_t = got_v.cpu().numpy(), got_t.cpu().numpy()
    assert got_t.shape == want_t.shape and bool((got_t == want_t).all())
    assert got_v.shape == want_v.shape and bool((got_v.view(np.int32) == want_v.view(np.int32)).all())
    owners = set(np.floor(want_v[:, 0].astype(np.float64)).astype(int).tolist())
    assert not bool(np.isnan(want_v).any()) and owners >= {0, 255, planes - 1} and len(owners & set(range(2, 255))) > 100
