"""The tile binning over list cells alone (dnsplat_bin_prepare_cells / dnsplat_bin_emit_sort_cells through _ops.bin_tiles(cells=)), from
hand-made tile boxes, against the numpy restatement of _cell_binning_ref.py — integers only, bit for bit.

Nothing is projected or composited: ``boxes`` = (first tile id in the camera's own grid, w | h << 16) is made on the host, so the frame
size only sets the grid and every edge of the route can be placed exactly.  With cells the route is picked from the CELL grid
(list_grid / emit_and_sort in binning.hip): key width, pass count and digit widths from the number of cells of the whole batch, the
fp32-reciprocal row division from the cell columns — so each of the edges test_gpu_binning_limits.py holds the per-tile lists to sits
at another frame size here.  Every case prints the regime it reached ("[cells] ..." lines) and asserts it."""
import numpy as np
import pytest
import torch

import _cell_binning_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXTRA_SHIFTS = {"8x1": (3, 0), "1x16": (0, 4), "16x16": (4, 4)}       # (4, 4): the largest cell check_cells accepts


def _shifts():
    from dn_splatter_amd import _ops

    return dict(_ops.BIN_CELL_SHAPES, **EXTRA_SHIFTS)


@pytest.fixture(autouse=True)
def sync_policy(dns):
    """The "sync" bin policy for the test; the policy and the capacity guesses are what they were afterwards."""
    from dn_splatter_amd import _ops

    mode = _ops.BIN_POLICY["mode"]
    hints = dict(_ops.BUFFERS.capacity_hint), dict(_ops.BUFFERS.cell_hint)
    _ops.set_bin_policy("sync")
    yield
    _ops.set_bin_policy(mode)
    for d, old in zip((_ops.BUFFERS.capacity_hint, _ops.BUFFERS.cell_hint), hints):
        d.clear()
        d.update(old)


def _with_edges(boxes, radii, tw, th, sx, sy, C):
    """The first entries of every camera replaced by the edge rectangles of the grid, all visible."""
    edge = ref.edge_entries(tw, th, sx, sy)
    ex = ref.pack_boxes(*(np.array([r[i] for r in edge]) for i in range(4)), tw)
    N = len(radii) // C
    k = min(len(edge), N)
    for c in range(C):
        boxes[c * N:c * N + k] = ex[:k]
        radii[c * N:c * N + k] = 1
    return boxes, radii


def _bin(boxes, radii, depths, tw, th, C, sx, sy, what, want_ends=True):
    """bin_tiles over the given entries against the restatement; returns (regime figures, reference lists, Binning)."""
    from dn_splatter_amd import _ops

    E = len(radii)
    assert E % C == 0 and boxes.dtype == np.int32 and boxes.shape == (E, 2)
    wh = boxes[:, 1].astype(np.int64) & 0xffffffff
    tiles = ((wh & 0xffff) * (wh >> 16)).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    want = ref.cell_lists(boxes, radii, depths, tw, th, C, sx, sy)          # also checks that every box lies inside the grid
    b = _ops.bin_tiles(torch.zeros(E, 2, device=DEV), t(radii.astype(np.int32)), t(depths.astype(np.float32)), t(tiles), tw * 16, th * 16, 16,
                       n_cameras=C, tile_boxes=t(boxes), cells=(sx, sy), want_ends=want_ends)
    n = b.n_isects
    status = _ops.binning_status(b, E)
    fig = ref.regime(tw, th, C, sx, sy, n)
    print(ref.regime_line(what, fig) + f", {b.n_tile_pairs} tile pairs, {int((radii > 0).sum())} of {E} entries visible")
    assert status == 0, what + ": binning status word"
    assert (b.list_width, b.list_height) == (fig["lw"], fig["lh"]) and b.tile_offsets.numel() == fig["cells"] + 1
    assert n == want["n_isects"], (what, n, want["n_isects"])
    assert b.n_tile_pairs == want["n_tile_pairs"], (what, b.n_tile_pairs, want["n_tile_pairs"])
    got = b.flatten_ids[:n].cpu().numpy().astype(np.int64)
    bad = np.flatnonzero(got != want["flatten_ids"])
    assert bad.size == 0, f"{what}: flatten_ids differ at {bad.size} of {n} positions, first {bad[:5]}"
    offs = b.tile_offsets.cpu().numpy().astype(np.int64)
    lists = want["lists"]
    assert np.array_equal(offs[lists], want["starts"]), what + ": offsets of the non-empty lists"
    assert int(offs[-1]) == n, what + ": the closing offset"
    if want_ends:
        ends = b.tile_ends.cpu().numpy().astype(np.int64)
        assert np.array_equal(ends[lists], want["ends"]), what + ": ends of the non-empty lists"
        empty = np.ones(fig["cells"], dtype=bool)
        empty[lists] = False
        assert bool((ends[empty] <= offs[:-1][empty]).all()), what + ": an empty list is not empty to the kernels"
    else:
        assert b.tile_ends is None
        assert np.array_equal(offs, want["offsets"]), what + ": gsplat's offsets"
    filled = b.filled_offsets().cpu().numpy().astype(np.int64)
    assert np.array_equal(filled, want["offsets"]), what + ": filled_offsets()"
    return fig, want, b


# ---- shapes and grids ----------------------------------------------------------------------------------------------------------

GRIDS = [(1, 1), (5, 3), (7, 4), (1, 9), (9, 1)]


@pytest.mark.parametrize("shape", ["1x1", "2x1", "1x2", "2x2", "4x2", "8x1", "1x16", "16x16"])
def test_every_cell_shape_on_small_and_ragged_grids(dns, shape):
    from dn_splatter_amd import _ops

    assert set(_ops.BIN_CELL_SHAPES) == {"1x1", "2x1", "1x2", "2x2", "4x2"}, "a new cell shape: add it to the parametrisation"
    sx, sy = _shifts()[shape]
    for tw, th in GRIDS:
        rng = np.random.default_rng(100 * tw + th + 7 * sx + sy)
        boxes, radii, depths = ref.random_entries(rng, 300, tw, th, max_w=tw, max_h=th)
        boxes, radii = _with_edges(boxes, radii, tw, th, sx, sy, 1)
        wh = boxes[:, 1].astype(np.int64)
        assert ((radii > 0) & (wh == 0)).any() and (radii == 0).any() and ((radii > 0) & (wh != 0)).any()
        fig, want, _b = _bin(boxes, radii, depths, tw, th, 1, sx, sy, f"cells {shape} on {tw} x {th} tiles")
        assert fig["cells"] == (-(-tw // (1 << sx))) * (-(-th // (1 << sy))) and fig["passes"] == 1 and fig["key"] == 16
        assert want["n_isects"] > 0 and want["max_cells"] == fig["cells"]                 # the full-grid box
        assert want["n_isects"] <= want["n_tile_pairs"]


@pytest.mark.parametrize("C", [2, 3])
def test_camera_batches_on_odd_grids(dns, C):
    """The per-camera base is counted in cells while the boxes are numbered in the tiles of the camera's own grid."""
    for shape, (sx, sy) in _shifts().items():
        for tw, th in [(5, 3), (7, 4)]:
            rng = np.random.default_rng(C * 1000 + tw + 11 * sx + sy)
            boxes, radii, depths = ref.random_entries(rng, 200 * C, tw, th, max_w=tw, max_h=th)
            boxes, radii = _with_edges(boxes, radii, tw, th, sx, sy, C)
            fig, want, _b = _bin(boxes, radii, depths, tw, th, C, sx, sy, f"{C} cameras, cells {shape} on {tw} x {th} tiles")
            per_cam = fig["lw"] * fig["lh"]
            assert fig["cells"] == C * per_cam
            # every camera lists something in its last cell (the edge rectangles end there)
            assert set(c * per_cam + per_cam - 1 for c in range(C)) <= set(want["lists"].tolist())


# ---- one tile pass that is first and last; two passes from 257 cells -----------------------------------------------------------------

@pytest.mark.parametrize("n_cells,lw,lh", [(2, 2, 1), (3, 3, 1), (5, 5, 1), (9, 3, 3), (17, 17, 1), (33, 11, 3), (65, 13, 5), (129, 43, 3), (255, 85, 3), (256, 32, 8), (257, 257, 1)])
def test_single_pass_at_every_digit_width_over_cells(dns, n_cells, lw, lh):
    sx = sy = 1
    tw, th = 2 * lw - 1, 2 * lh - 1                           # ragged: the last cell column / row holds one tile
    rng = np.random.default_rng(n_cells)
    boxes, radii, depths = ref.random_entries(rng, 400, tw, th, max_w=max(2, tw // 2), max_h=th)
    boxes, radii = _with_edges(boxes, radii, tw, th, sx, sy, 1)
    fig, want, _b = _bin(boxes, radii, depths, tw, th, 1, sx, sy, f"{n_cells} cells")
    bits = {2: 1, 3: 2, 5: 3, 9: 4, 17: 5, 33: 6, 65: 7, 129: 8, 255: 8, 256: 8, 257: 9}[n_cells]
    assert fig["cells"] == n_cells == lw * lh and fig["bits"] == bits and fig["key"] == 16 and fig["exact"] == (lw <= 256)
    if n_cells <= 256:
        assert fig["passes"] == 1 and fig["dbits"] == [bits]
    else:
        assert fig["passes"] == 2 and fig["dbits"] == [5, 4]
    assert n_cells - 1 in want["lists"].tolist() and want["max_cells"] > 1


# ---- 256 against 257 cell columns: the fp32-reciprocal row division of the pair generator ---------------------------------------------

@pytest.mark.parametrize("shape,tw", [("2x2", 512), ("2x2", 513), ("4x2", 1024), ("4x2", 1025)])
def test_cell_columns_across_the_exact_division_edge(dns, shape, tw):
    sx, sy = _shifts()[shape]
    th = 6
    rng = np.random.default_rng(tw)
    boxes, radii, depths = ref.random_entries(rng, 1200, tw, th, max_w=tw, max_h=th)
    boxes, radii = _with_edges(boxes, radii, tw, th, sx, sy, 1)
    fig, want, _b = _bin(boxes, radii, depths, tw, th, 1, sx, sy, f"cells {shape} on {tw} tile columns")
    lw = 256 if tw in (512, 1024) else 257
    assert fig["lw"] == lw and fig["lh"] == 3 and fig["exact"] == (lw == 256) and fig["key"] == 16
    assert fig["passes"] == 2 and fig["dbits"] == [5, 5]
    print(f"[cells] {tw} tile columns: widest box row {want['widest_row']} cells, a digit range wraps: {want['wraps'](5)}")
    assert want["widest_row"] == lw >= 1 << fig["dbits"][0], "no box row reaches the `all` term of the range histogram"
    assert want["wraps"](fig["dbits"][0])


# ---- 65536 cells against more: uint16 against uint32 keys ------------------------------------------------------------------------------

@pytest.mark.parametrize("tw,th,C", [(512, 512, 1), (512, 514, 1), (512, 256, 2), (512, 258, 2)])
def test_cell_counts_across_the_key_width_edge(dns, tw, th, C):
    sx = sy = 1
    rng = np.random.default_rng(th + C)
    boxes, radii, depths = ref.random_entries(rng, 1200 * C, tw, th, max_w=tw, max_h=12)
    boxes, radii = _with_edges(boxes, radii, tw, th, sx, sy, C)
    fig, want, _b = _bin(boxes, radii, depths, tw, th, C, sx, sy, f"{C} x {tw} x {th} tiles in 2x2 cells")
    if th * C == 512:
        assert fig["cells"] == 65536 and fig["key"] == 16 and fig["exact"] and fig["dbits"] == [8, 8]
    else:
        assert fig["cells"] == (65792 if C == 1 else 66048) and fig["key"] == 32 and not fig["exact"] and fig["dbits"] == [6, 6, 5]
    assert fig["cells"] - 1 in want["lists"].tolist(), "the last cell of the batch is empty"
    # (256 cell columns and an 8-bit first digit: a box row cannot wrap, a full one is the `all` term alone)
    assert want["widest_row"] == 256 >= 1 << fig["dbits"][0] and (fig["dbits"][0] == 8 or want["wraps"](fig["dbits"][0]))


# ---- base tile ids at and above 2^24 ---------------------------------------------------------------------------------------------------

def test_base_tile_ids_beyond_2_pow_24(dns):
    """4x2 cells on 8192 x 8192 tiles: 2^23 cells, 23 bits in three passes, boxes whose first tile id no float32 holds exactly."""
    sx, sy, tw, th = 2, 1, 8192, 8192
    rect = [(0, 0, 3, 3), (8191, 8191, 1, 1), (5, 2048, 9, 3), (8190, 2047, 2, 2), (100, 6000, 1100, 5), (8000, 8190, 192, 2),
            (4097, 4097, 1, 1), (8191, 2048, 1, 1), (3, 8191, 4, 1), (4095, 2049, 2, 1), (7000, 7001, 70, 70), (1000, 5000, 200, 1)]
    rng = np.random.default_rng(24)
    boxes, radii, depths = ref.random_entries(rng, 64, tw, th, max_w=48, max_h=6)
    boxes[:len(rect)] = ref.pack_boxes(*(np.array([r[i] for r in rect]) for i in range(4)), tw)
    radii[:len(rect)] = 1
    depths[1] = depths[7]                      # a tie across far-apart cells changes nothing
    fig, want, _b = _bin(boxes, radii, depths, tw, th, 1, sx, sy, "8192 x 8192 tiles in 4x2 cells")
    assert fig["cells"] == 1 << 23 and fig["bits"] == 23 and fig["dbits"] == [8, 8, 7] and fig["key"] == 32 and not fig["exact"]
    listed = (radii > 0) & (boxes[:, 1] != 0)
    high = int((listed & (boxes[:, 0].astype(np.int64) >= 1 << 24)).sum())
    odd = int((listed & (boxes[:, 0].astype(np.int64) > 1 << 24) & (boxes[:, 0] % 2 == 1)).sum())
    print(f"[cells] 2^23 cells: {high} listed boxes start at tile 2^24 or beyond, {odd} of them at an odd id")
    assert high >= 8 and odd >= 3 and (1 << 23) - 1 in want["lists"].tolist()
    assert want["widest_row"] >= 256 and want["wraps"](8)


# ---- cell-pair counts on the 4096-pair chunk edges -------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,floater", [(4095, None), (4096, None), (4097, None), (8193, None), (4000, 3500)])
def test_cell_pair_counts_on_chunk_edges(dns, K, floater):
    """Boxes of 2x2 tiles inside one cell: one cell pair and four tile pairs each.  ``floater``: one more entry over all 5120 cells, behind
    that many of the others in depth — pairs are emitted in depth order, so its pairs are [3500, 8620) of the emission and the whole
    4096-pair chunk [4096, 8192) belongs to it."""
    sx = sy = 1
    tw, th = 160, 128                                         # 80 x 64 cells
    rng = np.random.default_rng(K)
    n_cull = 777
    E = K + n_cull + (floater is not None)
    cx, cy = rng.integers(0, 80, E), rng.integers(0, 64, E)
    boxes = ref.pack_boxes(2 * cx, 2 * cy, np.full(E, 2), np.full(E, 2), tw)
    radii = np.zeros(E, dtype=np.int32)
    radii[rng.permutation(E)[:K + (floater is not None)]] = 1
    depths = (1.0 + 7.0 * rng.random(E)).astype(np.float32)
    if floater is not None:
        f = int(np.flatnonzero(radii)[K // 2])
        boxes[f] = ref.pack_boxes([0], [0], [tw], [th], tw)[0]
        others = np.sort(depths[(radii > 0) & (np.arange(E) != f)])
        assert others[floater - 1] < others[floater]
        depths[f] = np.float32(0.5 * (float(others[floater - 1]) + float(others[floater])))
        assert others[floater - 1] < depths[f] < others[floater]
    fig, want, _b = _bin(boxes, radii, depths, tw, th, 1, sx, sy, f"{K} one-cell boxes" + (" and a floater" if floater is not None else ""))
    assert fig["cells"] == 5120 and fig["passes"] == 2 and fig["key"] == 16
    if floater is not None:
        # the pairs in front of the floater's in the emission order (depth rank, ties by entry index), from the restatement's cell boxes
        _l, _x, _y, cw, ch, _w, _h = ref.cell_boxes(boxes, radii, tw, sx, sy)
        bits = depths.view(np.uint32)
        ahead = (bits < bits[f]) | ((bits == bits[f]) & (np.arange(E) < f))
        start = int((cw * ch)[ahead].sum())
        end = start + int(cw[f] * ch[f])
        owned = [c for c in range(-(-fig["pairs"] // 4096)) if start <= 4096 * c and 4096 * (c + 1) <= end]
        print(f"[cells] floater: pairs [{start}, {end}) of {fig['pairs']} in the emission order, whole chunks {owned}")
        assert (start, end) == (floater, floater + 5120) and owned == [1] and end < fig["pairs"] == K + 5120
        assert want["max_cells"] == 5120 > 4096 and want["n_tile_pairs"] == 4 * K + tw * th
    else:
        assert fig["pairs"] == K and want["max_cells"] == 1 and want["n_tile_pairs"] == 4 * K


# ---- ranked-entry counts ---------------------------------------------------------------------------------------------------------------

def _ranked(V, E, seed, tw=40, th=30, max_w=3, max_h=3):
    """E entries, exactly V of them visible (radii > 0), a few of those with an empty box."""
    rng = np.random.default_rng(seed)
    boxes, radii, depths = ref.random_entries(rng, E, tw, th, max_w=max_w, max_h=max_h, culled=0.0, empty=0.01)
    radii[:] = 0
    radii[rng.permutation(E)[:V]] = 1
    return boxes, radii, depths


@pytest.mark.parametrize("V,E", [(2047, 2600), (2048, 2600), (2049, 2600), (530_000, 600_000)])
def test_visible_entry_counts_on_the_scan_chunk_edges(dns, V, E):
    """2048 ranks per scan chunk; beyond 256 x 2048 = 524288 ranks the workgroup of the last rank adds the per-tile chunk sums up in a second
    trip (scan_final_kernel's tile_sums loop, which runs only with cells)."""
    tw, th = 40, 30
    boxes, radii, depths = _ranked(V, E, seed=V)
    fig, want, _b = _bin(boxes, radii, depths, tw, th, 1, 1, 1, f"{V} visible of {E} entries")
    assert int((radii > 0).sum()) == V and fig["cells"] == 300
    chunks = -(-V // 2048)
    print(f"[cells] {V} ranked entries: {chunks} scan chunks, {want['n_tile_pairs']} tile pairs")
    assert chunks == {2047: 1, 2048: 1, 2049: 2, 530_000: 259}[V] and (chunks > 256) == (V > 524288)
    assert V // 2 < want["n_isects"] < want["n_tile_pairs"]


@pytest.mark.parametrize("E", [(1 << 22) - 1, 1 << 22])
def test_entry_counts_across_the_depth_sort_routes(dns, E):
    """Below 2^22 entries the range partition + bucket sorts gather the boxes into cell counts (dp_store_bucket), from 2^22 on the last
    LSD pass does (the BOXG scatter), in 4096-key chunks."""
    from dn_splatter_amd import _lib

    route = int(_lib.lib().dnsplat_bin_depth_route(E))
    tw, th = 40, 30
    boxes, radii, depths = _ranked(E - E // 8, E, seed=E % 1000, max_w=2, max_h=1)
    fig, want, _b = _bin(boxes, radii, depths, tw, th, 1, 1, 1, f"{E} entries")
    print(f"[cells] {E} entries: depth route {route} (1 = range partition, 0 = four LSD passes)")
    assert route == (1 if E < 1 << 22 else 0)
    assert fig["cells"] == 300 and want["n_isects"] > E // 2


def test_exact_depth_ties_inside_every_cell_list(dns):
    tw, th = 7, 4
    rng = np.random.default_rng(8192)
    E, n_tied = 12000, 9000
    boxes, radii, depths = ref.random_entries(rng, E, tw, th, max_w=tw, max_h=th, culled=0.0, empty=0.0)
    depths[rng.permutation(E)[:n_tied]] = np.float32(4.0)
    radii[:] = 1
    radii[rng.permutation(E)[:500]] = 0
    tied = int(((depths == np.float32(4.0)) & (radii > 0)).sum())
    fig, want, _b = _bin(boxes, radii, depths, tw, th, 1, 1, 1, "depth ties")
    ids = want["flatten_ids"]
    shortest = int((want["ends"] - want["starts"]).min())
    print(f"[cells] depth ties: {tied} visible entries at depth 4.0, {int((depths[ids] == np.float32(4.0)).sum())} of {fig['pairs']} pairs, "
          f"shortest list {shortest}")
    assert tied > 8192 and fig["cells"] == 8 and len(want["lists"]) == 8 and shortest > 2048
    assert int((depths[ids] == np.float32(4.0)).sum()) > 2 * 4096


# ---- gsplat's offsets over cells -------------------------------------------------------------------------------------------------------

def test_offsets_without_ends_are_gsplats_over_cells(dns):
    """want_ends=False: the fill launch runs and an empty list carries the offset of the next non-empty one."""
    tw, th = 14, 9
    rng = np.random.default_rng(3)
    boxes, radii, depths = ref.random_entries(rng, 300, 5, 4, max_w=2, max_h=2)          # everything in the upper left corner
    x0, y0 = boxes[:, 0] % 5, boxes[:, 0] // 5
    boxes[:, 0] = np.where(boxes[:, 1] != 0, y0 * tw + x0, 0)
    boxes[0] = ref.pack_boxes([13], [8], [1], [1], tw)[0]
    radii[0] = 1
    for shape in ("2x2", "4x2"):
        sx, sy = _shifts()[shape]
        fig, want, _b = _bin(boxes, radii, depths, tw, th, 1, sx, sy, f"no ends, cells {shape}", want_ends=False)
        n_empty = fig["cells"] - len(want["lists"])
        print(f"[cells] no ends, cells {shape}: {n_empty} of {fig['cells']} lists empty")
        assert n_empty > fig["cells"] // 2 and fig["cells"] - 1 in want["lists"].tolist()
