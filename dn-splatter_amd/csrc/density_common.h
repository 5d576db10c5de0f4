// density_common.h — what density.hip and levelset.hip share of the Gaussian density field: the layout and the view of the index
// buffer, THE cell assignment, the exact k-nearest-neighbour search of one query in registers (df_search) and the evaluation of one
// neighbour record (df_accumulate).  Both files are compiled without contraction and call the very same search, so a
// search from either gives equal bits; levelset.hip evaluates at an offset from the mean and restates df_accumulate's statements
// behind x - mu for that (ls_term there).
#pragma once

#include "splat_common.h"

#include <math.h>

namespace {

constexpr int DF_THREADS = 256;
constexpr int DF_WAVES = DF_THREADS / DNS_WAVE;
constexpr int DF_SCAN_THREADS = 1024;
constexpr int DF_SCAN_PER = 4;
constexpr int DF_MINMAX_BLOCKS = 256;
constexpr double DF_SHRINK = 1.0 - 4e-7, DF_GROW = 1.0 + 4e-7;    // > (1 + 2^-24)^2: the roundings of (p - lo) and of its product with inv_h

struct DfHeader {             // 64 bytes at the start of the index buffer, written by df_header_kernel
    float lo[3], hi[3];       // the exact bounding box of the means
    float inv_h[3];           // cells per unit length; 0 along an axis without extent (one cell thick there)
    int32_t g[3];             // cells along the axis that hold points: the grid dimension, or 1
    int32_t pad[4];
};
static_assert(sizeof(DfHeader) == 64, "the index header is 64 bytes");

struct DfLayout {
    int G;
    long long C;
    size_t cell_start, sorted, cell_of, tmp, fill, partial, total;
};

size_t df_align(size_t v) { return (v + 15) & ~(size_t)15; }

int df_grid_dim(int N)
{
    int g = (int)cbrt((double)N / 2.0);
    while ((long long)(g + 1) * (g + 1) * (g + 1) * 2 <= N) ++g;
    while (g > 1 && (long long)g * g * g * 2 > N) --g;
    if (g < 1) g = 1;
    if (g > DNSPLAT_KNN_MAX_GRID) g = DNSPLAT_KNN_MAX_GRID;
    return g;
}

DfLayout df_layout(int N)
{
    DfLayout l;
    l.G = df_grid_dim(N);
    l.C = (long long)l.G * l.G * l.G;
    size_t at = sizeof(DfHeader);
    l.cell_start = at; at = df_align(at + (size_t)(l.C + 1) * sizeof(int32_t));
    l.sorted = at;     at = df_align(at + (size_t)N * sizeof(float4));
    l.cell_of = at;    at = df_align(at + (size_t)N * sizeof(int32_t));
    l.tmp = at;        at = df_align(at + (size_t)N * sizeof(int32_t));
    l.fill = at;       at = df_align(at + (size_t)l.C * sizeof(int32_t));
    l.partial = at;    at = df_align(at + (size_t)DF_MINMAX_BLOCKS * 6 * sizeof(float));
    l.total = at;
    return l;
}

struct DfIndex {              // what the search reads
    const DfHeader *header;
    const int32_t *cell_start;
    const float4 *sorted;
    int G;
};

DfIndex df_view(const void *index, const DfLayout &l)
{
    DfIndex ix;
    ix.header = (const DfHeader *)index;
    ix.cell_start = (const int32_t *)((const char *)index + l.cell_start);
    ix.sorted = (const float4 *)((const char *)index + l.sorted);
    ix.G = l.G;
    return ix;
}

// ---- the index -----------------------------------------------------------------------------------------------------------------------

// THE cell assignment along one axis, for points and for the start cell of a query: two fp32 roundings.  nan goes to cell 0.
__device__ __forceinline__ int df_axis_cell(float p, float lo, float inv_h, int g)
{
    const float t = __fmul_rn(__fsub_rn(p, lo), inv_h);
    return t >= 0.f ? (int)fminf(t, (float)(g - 1)) : 0;
}

// ---- the search ----------------------------------------------------------------------------------------------------------------------

template <int KM>
struct DfList {               // ascending by (d, i); static indices only, so it lives in registers
    double d[KM];
    int i[KM];
};

__device__ __forceinline__ bool df_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

template <int KM>
__device__ __forceinline__ void df_insert(DfList<KM> &L, double d, int i)
{
    if (!df_less(d, i, L.d[KM - 1], L.i[KM - 1])) return;
#pragma unroll
    for (int j = KM - 1; j > 0; --j) {
        const bool up = df_less(d, i, L.d[j - 1], L.i[j - 1]);          // the entry below moves up
        const bool here = df_less(d, i, L.d[j], L.i[j]);
        L.d[j] = up ? L.d[j - 1] : (here ? d : L.d[j]);
        L.i[j] = up ? L.i[j - 1] : (here ? i : L.i[j]);
    }
    if (df_less(d, i, L.d[0], L.i[0])) { L.d[0] = d; L.i[0] = i; }
}

// The K = k + skip nearest means of (x, y, z) by (d^2, index) in L[0 .. K); false (and nothing read) for a non-finite coordinate.
template <int KM>
__device__ __forceinline__ bool df_search(const DfIndex &ix, float x, float y, float z, int K, DfList<KM> &L)
{
#pragma unroll
    for (int j = 0; j < KM; ++j) { L.d[j] = INFINITY; L.i[j] = 0x7fffffff; }
    if (!(fabsf(x) < INFINITY) || !(fabsf(y) < INFINITY) || !(fabsf(z) < INFINITY)) return false;
    const DfHeader h = *ix.header;
    const float qf[3] = {x, y, z};
    double q[3], lo[3], cell_w[3], out2 = 0.0, out[3];
    int c[3], g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q[a] = (double)qf[a];
        lo[a] = (double)h.lo[a];
        g[a] = h.g[a];
        c[a] = df_axis_cell(qf[a], h.lo[a], h.inv_h[a], g[a]);
        cell_w[a] = g[a] > 1 ? 1.0 / (double)h.inv_h[a] : 0.0;
        out[a] = fmax(fmax(lo[a] - q[a], q[a] - (double)h.hi[a]), 0.0);   // every mean lies in [lo, hi]: exact
        out2 += out[a] * out[a];
    }
    for (int r = 0;; ++r) {
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g[2] - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g[1] - 1);
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g[0] - 1);
        for (int zz = z0; zz <= z1; ++zz) {
            for (int yy = y0; yy <= y1; ++yy) {
                // a row of the cube's faces is one run of cells (and of sorted points); an inner row has the two end cells
                const bool face = zz == c[2] - r || zz == c[2] + r || yy == c[1] - r || yy == c[1] + r;
                const long long row = ((long long)zz * ix.G + yy) * ix.G;
                for (int seg = 0; seg < (face ? 1 : 2); ++seg) {
                    const int xa = face ? x0 : (seg == 0 ? c[0] - r : c[0] + r), xb = face ? x1 : xa;
                    if (xa < 0 || xb > g[0] - 1) continue;
                    const int s = ix.cell_start[row + xa], e = ix.cell_start[row + xb + 1];
                    for (int p = s; p < e; ++p) {
                        const float4 v = ix.sorted[p];
                        const double dx = q[0] - (double)v.x, dy = q[1] - (double)v.y, dz = q[2] - (double)v.z;
                        df_insert(L, fma(dz, dz, fma(dy, dy, dx * dx)), __float_as_int(v.w));
                    }
                }
            }
        }
        // a lower bound of d^2 to any mean in a cell outside the cube of radius r: it lies beyond one of the cube's faces along some
        // axis a, and within [lo, hi] along the others
        double bound2 = INFINITY;
        bool open = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double rest = out2 - out[a] * out[a];
            const int jp = c[a] + r + 1, jm = c[a] - r - 1;
            if (jp < g[a]) {                                        // cells >= jp: coordinate >= lo + jp w (1 - 4e-7)
                const double f = fmax(fmax(lo[a] + (double)jp * cell_w[a] * DF_SHRINK - q[a], out[a]), 0.0);
                bound2 = fmin(bound2, f * f + rest);
                open = true;
            }
            if (jm >= 0) {                                          // cells <= jm: coordinate < lo + (jm + 1) w (1 + 4e-7)
                const double f = fmax(fmax(q[a] - (lo[a] + (double)(jm + 1) * cell_w[a] * DF_GROW), out[a]), 0.0);
                bound2 = fmin(bound2, f * f + rest);
                open = true;
            }
        }
        if (!open) break;                                           // the cube covers the grid
        double worst = INFINITY;
#pragma unroll
        for (int j = 0; j < KM; ++j) worst = j == K - 1 ? L.d[j] : worst;
        if (worst < bound2) break;
    }
    return true;
}

struct DfAcc {
    float density, g[3];
};

// one neighbour: m2 = clamp(|M^T (x - mu)|^2, 0, 1e8), density += o exp(-m2 / 2), and for the first num_closest: g += m2 M (M^T (x - mu))
__device__ __forceinline__ void df_accumulate(const float *__restrict__ records, int gi, float x, float y, float z, bool with_grad, DfAcc &acc)
{
    const float4 *rec = (const float4 *)(records + (size_t)gi * DNS_REC);
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    const float Mm[9] = {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x};
    const float d0 = x - r0.x, d1 = y - r0.y, d2 = z - r0.z;
    float v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = Mm[a] * d0 + Mm[3 + a] * d1 + Mm[6 + a] * d2;
    const float m2 = fminf(fmaxf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2], 0.f), 1e8f);
    acc.density += r0.w * expf(-0.5f * m2);
    if (with_grad) {
#pragma unroll
        for (int r = 0; r < 3; ++r) acc.g[r] += m2 * (Mm[3 * r] * v[0] + Mm[3 * r + 1] * v[1] + Mm[3 * r + 2] * v[2]);
    }
}

}  // namespace
