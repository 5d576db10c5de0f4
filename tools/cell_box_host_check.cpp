// Stand-alone host check of dns_cell_box (csrc/bin_ranges.h): the box of list cells a tile box turns into, against a brute-force
// enumeration of the box's tiles -> their cells.  Every grid up to 9 x 7 tiles, every box in it (so: boxes at the grid's edges,
// widths and heights of 1, boxes that end inside a cell the grid cuts off), every cell shape up to 8 x 4 tiles, and empty boxes.
//   g++ -O2 -std=c++17 -I dn-splatter_amd/csrc tools/cell_box_host_check.cpp -o cell_box_host_check && ./cell_box_host_check
#include <cstdio>
#include <set>
#include "bin_ranges.h"

int main()
{
    long cases = 0;
    for (unsigned tw = 1; tw <= 9; ++tw)
        for (unsigned th = 1; th <= 7; ++th)
            for (int sx = 0; sx <= 3; ++sx)
                for (int sy = 0; sy <= 2; ++sy) {
                    const unsigned ctw = dns_cells(tw, sx), cth = dns_cells(th, sy);
                    if (ctw != (tw + (1u << sx) - 1) / (1u << sx) || cth != (th + (1u << sy) - 1) / (1u << sy)) {
                        printf("dns_cells: %u tiles, shift %d\n", tw, sx);
                        return 1;
                    }
                    for (unsigned x0 = 0; x0 < tw; ++x0)
                        for (unsigned y0 = 0; y0 < th; ++y0)
                            for (unsigned x1 = x0 + 1; x1 <= tw; ++x1)
                                for (unsigned y1 = y0 + 1; y1 <= th; ++y1) {
                                    std::set<unsigned> want;      // ids of the cells the box's tiles lie in
                                    for (unsigned y = y0; y < y1; ++y)
                                        for (unsigned x = x0; x < x1; ++x) want.insert((y >> sy) * ctw + (x >> sx));
                                    const DnsCellBox c = dns_cell_box(y0 * tw + x0, x1 - x0, y1 - y0, tw, sx, sy);
                                    std::set<unsigned> got;
                                    for (unsigned r = 0; r < c.h; ++r)
                                        for (unsigned k = 0; k < c.w; ++k) got.insert(c.base + r * ctw + k);
                                    const unsigned cx0 = c.base % ctw, cy0 = c.base / ctw;
                                    const bool inside = c.w >= 1 && c.h >= 1 && cx0 + c.w <= ctw && cy0 + c.h <= cth;
                                    if (!inside || got != want || got.size() != (size_t)c.w * c.h) {
                                        printf("grid %u x %u, cells 2^%d x 2^%d, box [%u, %u) x [%u, %u): cell box base %u, %u x %u\n", tw, th, sx, sy,
                                               x0, x1, y0, y1, c.base, c.w, c.h);
                                        return 1;
                                    }
                                    if (sx == 0 && sy == 0 && (c.base != y0 * tw + x0 || c.w != x1 - x0 || c.h != y1 - y0)) {
                                        printf("1 x 1 cells changed a box\n");
                                        return 1;
                                    }
                                    ++cases;
                                }
                    // a culled Gaussian's box (0 | 0) stays empty, whatever its first tile id says
                    for (unsigned base = 0; base < tw * th; ++base) {
                        const DnsCellBox a = dns_cell_box(base, 0, 0, tw, sx, sy), b = dns_cell_box(base, 0, 3, tw, sx, sy),
                                         d = dns_cell_box(base, 2, 0, tw, sx, sy);
                        if (a.w * a.h + b.w * b.h + d.w * d.h != 0u) {
                            printf("an empty box got cells\n");
                            return 1;
                        }
                    }
                }
    printf("ok %ld boxes\n", cases);
    return 0;
}
