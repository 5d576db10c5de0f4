"""The tile binning over list cells (dnsplat_bin_prepare_cells / dnsplat_bin_emit_sort_cells), restated in numpy straight from the
tile boxes — no projection, no compositing.

Inputs as ``_ops.bin_tiles(..., tile_boxes=boxes, cells=(sx, sy))`` takes them, for C cameras of N entries each:
``boxes`` int32 [C*N, 2] = (first tile id in the camera's own grid of ``tw`` tile columns, w | h << 16), ``radii`` [C*N] and
``depths`` [C*N] positive float32.

An entry is listed iff radii > 0 and w, h > 0.  It enters the cells [x0 >> sx, (x0 + w - 1) >> sx] x [y0 >> sy, (y0 + h - 1) >> sy]
of camera e // N; the list of (camera, cell) is sorted by (float32 depth bits, entry index); the lists are stored back to back in
list order (camera, cell row, cell column).  n_isects is the sum of the cell-box areas, n_tile_pairs the sum of w * h."""
import numpy as np


def cells_of(tiles, shift):
    return (tiles + (1 << shift) - 1) >> shift


def tile_bits(n_lists):
    bits = 1
    while (1 << bits) < n_lists:
        bits += 1
    return bits


def regime(tw, th, C, sx, sy, n_pairs):
    """The route the tile sort takes for this list grid (binning.hip: list_grid, emit_and_sort), from the cell grid alone."""
    lw, lh = cells_of(tw, sx), cells_of(th, sy)
    n_lists = lw * lh * C
    bits = tile_bits(n_lists)
    passes = (bits + 7) // 8
    dbits, shift = [], 0
    for p in range(passes):
        d = (bits - shift + (passes - p) - 1) // (passes - p)
        dbits.append(d)
        shift += d
    return dict(lw=lw, lh=lh, cells=n_lists, bits=bits, passes=passes, dbits=dbits, key=16 if n_lists <= 0x10000 else 32,
                exact=lw <= 256 and n_lists <= 65536, pairs=int(n_pairs))


def regime_line(what, fig):
    return (f"[cells] {what}: {fig['cells']} cells ({fig['lw']} x {fig['lh']} per camera), {fig['bits']} bits -> {fig['passes']} passes "
            f"{fig['dbits']} on uint{fig['key']} keys, row division {'fp32 reciprocal' if fig['exact'] else 'integer'}, "
            f"{fig['pairs']} cell pairs")


def cell_boxes(boxes, radii, tw, sx, sy):
    """Per entry: (listed, cx0, cy0, cw, ch, w, h) with cw = ch = 0 for an entry that is not listed."""
    boxes = np.asarray(boxes).astype(np.int64)
    base, wh = boxes[:, 0], boxes[:, 1] & 0xffffffff
    w, h = wh & 0xffff, wh >> 16
    listed = (np.asarray(radii) > 0) & (w > 0) & (h > 0)
    y0, x0 = base // tw, base % tw
    cx0, cy0 = x0 >> sx, y0 >> sy
    cw = np.where(listed, ((x0 + w - 1) >> sx) + 1 - cx0, 0)
    ch = np.where(listed, ((y0 + h - 1) >> sy) + 1 - cy0, 0)
    return listed, cx0, cy0, cw, ch, np.where(listed, w, 0), np.where(listed, h, 0)


def cell_lists(boxes, radii, depths, tw, th, C, sx, sy):
    """-> dict(flatten_ids [n], lists (ids of the non-empty lists, ascending), starts, ends, offsets [C*cells + 1] (gsplat's rule: an
    empty list carries the next non-empty offset), n_isects, n_tile_pairs, widest_row (cells), wraps (per digit width d: does some
    box row's digit range wrap past 2^d - 1))."""
    E = len(radii)
    N = E // C
    lw, lh = cells_of(tw, sx), cells_of(th, sy)
    listed, cx0, cy0, cw, ch, w, h = cell_boxes(boxes, radii, tw, sx, sy)
    assert bool(((cx0 + cw <= lw) & (cy0 + ch <= lh))[listed].all()) and bool((np.asarray(boxes)[:, 0] >= 0).all()), "a box leaves the grid"
    assert bool(((np.asarray(boxes)[:, 0].astype(np.int64) % tw + w <= tw))[listed].all()), "a box row wraps to the next tile row"
    area = cw * ch
    n = int(area.sum())
    ent = np.repeat(np.arange(E, dtype=np.int64), area)                  # entry of every pair, pairs in entry order, row-major in the box
    first = np.cumsum(area) - area
    k = np.arange(n, dtype=np.int64) - first[ent]
    row, col = k // np.maximum(cw[ent], 1), k % np.maximum(cw[ent], 1)
    lid = ((ent // N) * lh + cy0[ent] + row) * lw + cx0[ent] + col
    dbits = np.ascontiguousarray(np.asarray(depths, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    # pairs are in entry order: a stable sort by (list, depth bits) leaves ties in entry order
    order = np.argsort((lid.astype(np.uint64) << np.uint64(32)) | dbits[ent], kind="stable")
    ids, lid_sorted = ent[order], lid[order]
    n_lists = lw * lh * C
    offsets = np.searchsorted(lid_sorted, np.arange(n_lists + 1, dtype=np.int64), side="left")
    lists = np.flatnonzero(offsets[1:] > offsets[:-1])
    # the first cell of every box row, for the regime figures
    rows = np.repeat(np.arange(E, dtype=np.int64), ch)
    r = np.arange(len(rows), dtype=np.int64) - (np.cumsum(ch) - ch)[rows]
    row_start = ((rows // N) * lh + cy0[rows] + r) * lw + cx0[rows]
    row_w = cw[rows]

    def wraps(d):
        rem = row_w & ((1 << d) - 1)
        return bool(((rem > 0) & ((row_start & ((1 << d) - 1)) + rem > (1 << d))).any())

    return dict(flatten_ids=ids, lists=lists, starts=offsets[:-1][lists], ends=offsets[1:][lists], offsets=offsets, n_isects=n,
                n_tile_pairs=int((w * h).sum()), widest_row=int(cw.max()) if E else 0, wraps=wraps, max_cells=int(area.max()) if E else 0)


def pack_boxes(x0, y0, w, h, tw):
    """int32 [E, 2] boxes of the given tile rectangles (an empty one: w = h = 0)."""
    x0, y0, w, h = (np.asarray(v, dtype=np.int64) for v in (x0, y0, w, h))
    wh = w | (h << 16)
    return np.stack([y0 * tw + x0, np.where(wh >= 1 << 31, wh - (1 << 32), wh)], 1).astype(np.int32)


def random_entries(rng, E, tw, th, max_w, max_h, culled=0.15, empty=0.05, depth_levels=None):
    """E entries with boxes inside a tw x th tile grid (widths up to max_w, heights up to max_h), a share of them culled (radii == 0)
    and a share visible with an empty box.  Depths are positive float32, from ``depth_levels`` distinct values if given (ties).
    -> (boxes, radii, depths)"""
    w = rng.integers(1, min(max_w, tw) + 1, E)
    h = rng.integers(1, min(max_h, th) + 1, E)
    x0 = (rng.random(E) * (tw - w + 1)).astype(np.int64)
    y0 = (rng.random(E) * (th - h + 1)).astype(np.int64)
    hollow = rng.random(E) < empty
    w, h = np.where(hollow, 0, w), np.where(hollow, 0, h)
    radii = (rng.random(E) >= culled).astype(np.int32)
    if depth_levels:
        depths = (1.0 + rng.integers(0, depth_levels, E) / 8.0).astype(np.float32)
    else:
        depths = (0.5 + 9.5 * rng.random(E)).astype(np.float32)
    return pack_boxes(np.where(hollow, 0, x0), np.where(hollow, 0, y0), w, h, tw), radii, depths


def edge_entries(tw, th, sx, sy):
    """Rectangles (x0, y0, w, h) at the places where a cell box can be cut wrongly: ending on the last tile column / row (of a ragged
    cell when tw or th is no multiple of the cell), one tile wide at an odd column, starting on a cell's last tile, the full grid."""
    r = [(0, 0, tw, th), (tw - 1, th - 1, 1, 1), (0, th - 1, tw, 1), (tw - 1, 0, 1, th), (0, 0, 1, 1)]
    for x in {1 % tw, (1 << sx) - 1, min(tw - 1, (1 << sx)), (tw - 1) | 1, max(0, tw - 2)}:
        if x < tw:
            r.append((x, 0, 1, min(2, th)))
            r.append((x, th - 1, min(2, tw - x), 1))
    for y in {(1 << sy) - 1, min(th - 1, 1 << sy), max(0, th - 2)}:
        if y < th:
            r.append((0, y, min(2, tw), min(2, th - y)))
            r.append((tw - 1, y, 1, th - y))
    return r


def brute_force_lists(boxes, radii, depths, tw, th, C, sx, sy):
    """The contract the compositing relies on, entry by entry and tile by tile: the list of a tile holds the entries (radii > 0) whose box
    holds the tile, by (depth bits, entry index); the list of a cell is the union of the lists of its tiles, every entry once, in that
    same order.  -> {list id: [entries]} of the non-empty cells, and the number of (tile, entry) pairs."""
    E = len(radii)
    N = E // C
    lw, lh = cells_of(tw, sx), cells_of(th, sy)
    bits = np.ascontiguousarray(np.asarray(depths, dtype=np.float32)).view(np.uint32)
    tile_lists = {}
    n_tile = 0
    for e in range(E):
        if radii[e] <= 0:
            continue
        base, wh = int(boxes[e][0]), int(boxes[e][1]) & 0xffffffff
        w, h = wh & 0xffff, wh >> 16
        x0, y0 = base % tw, base // tw
        for ty in range(y0, y0 + h):
            for tx in range(x0, x0 + w):
                tile_lists.setdefault((e // N, tx, ty), []).append(e)
                n_tile += 1
    out = {}
    for (c, tx, ty), es in tile_lists.items():
        out.setdefault((c * lh + (ty >> sy)) * lw + (tx >> sx), set()).update(es)
    return {l: sorted(es, key=lambda e: (int(bits[e]), e)) for l, es in out.items()}, n_tile
