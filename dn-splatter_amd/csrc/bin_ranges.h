// bin_ranges.h — digit counts of a run of (tile, gaussian) pairs WITHOUT generating the pairs.
//
// The first pass of the tile sort (binning.hip, GEN instantiations) works on pairs that exist only as a 16-byte record per
// Gaussian: its pairs are the tiles of a box, row-major — pair k of the record has tile id  base + (k / w) * tw + k % w.  The
// histogram kernel of that pass only needs, per 4096-pair chunk, how many pairs fall on each value of the pass's digit, and the
// digit is the LOW dbits bits of the tile id (shift 0).  Within one box row consecutive pairs have consecutive tile ids, hence
// consecutive digits modulo 2^dbits: a row contributes +1 to a cyclic RANGE of digits (plus a constant to all of them for every
// full 2^dbits it spans).  So a record's share of a chunk is a handful of range increments — one per box row it has inside the
// chunk — instead of one LDS atomic per pair behind an owner search and a record gather per pair.
//
// Plain C++ on purpose (no HIP types): tests/test_host_logic.py compiles this header with g++ and checks it against the
// pair-by-pair count on random boxes, chunk cuts and digit widths.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DNS_BR_HD __host__ __device__ __forceinline__
#else
#define DNS_BR_HD inline
#endif

// List cells.  The fused path keeps one sorted list per CELL of 2^sx x 2^sy tiles instead of one per tile (its compositing kernels
// re-test every list entry against their own half tile anyway), so a Gaussian is listed once per cell its tile box touches.
// The tile box [x0, x0 + w) x [y0, y0 + h) that starts at tile id `base_tile` = y0 * tw + x0 of a grid of `tw` tile columns becomes
// the cell box [x0 >> sx, ((x0 + w - 1) >> sx) + 1) x [y0 >> sy, ((y0 + h - 1) >> sy) + 1) of the grid of dns_cells(tw, sx) cell
// columns; an empty box (w == 0 or h == 0: a culled Gaussian) stays empty.  sx == sy == 0 returns the box as it is.
DNS_BR_HD uint32_t dns_cells(uint32_t tiles, int shift) { return (tiles + (1u << shift) - 1u) >> shift; }
struct DnsCellBox { uint32_t base, w, h; };        // id of the first cell (row-major over the cell grid), width and height in cells
DNS_BR_HD DnsCellBox dns_cell_box(uint32_t base_tile, uint32_t w, uint32_t h, uint32_t tw, int sx, int sy)
{
    DnsCellBox c;
    if (w == 0u || h == 0u) { c.base = 0u; c.w = 0u; c.h = 0u; return c; }
    const uint32_t y0 = base_tile / tw, x0 = base_tile - y0 * tw;
    const uint32_t cx0 = x0 >> sx, cy0 = y0 >> sy;
    c.base = cy0 * dns_cells(tw, sx) + cx0;
    c.w = ((x0 + w - 1u) >> sx) + 1u - cx0;
    c.h = ((y0 + h - 1u) >> sy) + 1u - cy0;
    return c;
}

// Pairs [lo, hi) (0 <= lo < hi <= rows * w) of a record whose box starts at tile id `base`, is `w` tiles wide and lies in a grid of
// `tw` tile columns.  Calls  range(d0, len)  for every cyclic digit range [d0, d0 + len) (0 < len < 2^dbits, d0 < 2^dbits; the
// range may wrap past 2^dbits - 1) that receives +1, and returns the constant every digit receives on top.
template <typename RangeFn>
DNS_BR_HD uint32_t dns_record_digit_ranges(uint32_t base, uint32_t w, uint32_t tw, uint32_t lo, uint32_t hi, int dbits, RangeFn &&range)
{
    const uint32_t mask = (1u << dbits) - 1u;
    const uint32_t r0 = lo / w, c0 = lo - r0 * w;
    const uint32_t last = hi - 1u;
    const uint32_t r1 = last / w, c1 = last - r1 * w;
    uint32_t all = 0u;
    uint32_t t_row = base + r0 * tw;                       // tile id of column 0 of the box in row r
    for (uint32_t r = r0; r <= r1; ++r, t_row += tw) {
        const uint32_t a = (r == r0) ? c0 : 0u;
        const uint32_t b = (r == r1) ? c1 : w - 1u;
        const uint32_t len = b - a + 1u;
        all += len >> dbits;
        const uint32_t rem = len & mask;
        if (rem) range((t_row + a) & mask, rem);
    }
    return all;
}
