// splat_common.h — shared device-side helpers for the gfx950 kernels of libdnsplat.
// Wave = 64 lanes everywhere in this library (CDNA4); nothing here is written for 32-wide warps.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dnsplat.h"
#include "../../include/dnsplat_constants.h"

#define DNS_WAVE 64
#define DNS_REC DNSPLAT_RECORD_FLOATS  // floats per splat / gradient record

// Record slots
#define REC_X 0
#define REC_Y 1
#define REC_CA 2
#define REC_CB 3
#define REC_CC 4
#define REC_OPAC 5
#define REC_CH0 6
#define REC_ABSX 14
#define REC_ABSY 15

#define DNS_CHECK_LAUNCH()                                   \
    do {                                                     \
        hipError_t e__ = hipGetLastError();                  \
        if (e__ != hipSuccess) return DNSPLAT_ERR_LAUNCH;    \
    } while (0)

// wave64 ballot straight from the predicate: HIP's __ballot(int) widens the bool first, and hipcc then rebuilds the mask
// with a v_cndmask + v_cmp pair when the predicate already lives in scalar registers
__device__ __forceinline__ uint64_t dns_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

static inline int dns_tiles_w(int width, int tile) { return (width + tile - 1) / tile; }
static inline int dns_tiles_h(int height, int tile) { return (height + tile - 1) / tile; }

// A.3 tile bounding box [min,max) in tile units, clamped to the grid.  Evaluated in the same
// operation order as the oracle's tile_bbox (oracle/oracle_impl.inc) — all divisions are by a
// power of two and floor/ceil are exact, so both sides agree bit for bit.
__device__ __forceinline__ void dns_tile_bbox(float mx, float my, float radius, int tile_size, int tw, int th,
                                              int &x0, int &y0, int &x1, int &y1)
{
    float ts = (float)tile_size;
    float tr = radius / ts;
    float tcx = mx / ts, tcy = my / ts;
    float fx0 = floorf(tcx - tr), fy0 = floorf(tcy - tr);
    float fx1 = ceilf(tcx + tr), fy1 = ceilf(tcy + tr);
    fx0 = fminf(fmaxf(fx0, 0.f), (float)tw);
    fy0 = fminf(fmaxf(fy0, 0.f), (float)th);
    fx1 = fminf(fmaxf(fx1, 0.f), (float)tw);
    fy1 = fminf(fmaxf(fy1, 0.f), (float)th);
    x0 = (int)fx0; y0 = (int)fy0; x1 = (int)fx1; y1 = (int)fy1;
}

// Tile box of the part of a splat that can reach alpha >= 1/255 at some pixel centre (the "SnugBox" of Speedy-Splat): the
// axis-aligned box of the ellipse  sigma(d) = 1/2 d^T conic d <= ln(255 opacity), widened by a rounding margin and clipped to
// gsplat's 3-sigma box (dns_tile_bbox).  Every (tile, splat) pair it leaves out fails the per-pixel alpha test at all 256 pixel
// centres of the tile, so the images and gradients composited from the shorter lists are the same numbers; the tile lists
// themselves are NOT gsplat's any more, which is why only the fused get_outputs path (whose lists are internal) asks for it.
// Evaluated by the projection kernel (tile counts) and by the emit kernel (tile pairs) from the same record floats: contraction
// is pinned off so that both translation units round identically.
__device__ __forceinline__ void dns_snug_tile_bbox(float mx, float my, float ca, float cb, float cc, float opac, float radius,
                                                   int tile_size, int tw, int th, int &x0, int &y0, int &x1, int &y1)
{
#pragma clang fp contract(off)
    dns_tile_bbox(mx, my, radius, tile_size, tw, th, x0, y0, x1, y1);
    const float tau = logf(255.f * opac);          // alpha = opacity exp(-sigma) >= 1/255  <=>  sigma <= tau
    if (!(tau > 0.f)) { x1 = x0; y1 = y0; return; }   // opacity <= 1/255: never composited
    // opacity within 0.2 % of 1/255: the ellipse is a fraction of a pixel wide and the fp32 error of the compositing alpha test
    // (relative ~1e-6 in opacity x vis) is no longer small against the margins below: keep gsplat's box
    if (tau < 2e-3f) return;
    const float det = ca * cc - cb * cb;
    if (!(det > 0.f)) return;                       // degenerate conic: keep gsplat's box
    // half widths sqrt(2 tau Sigma_xx), sqrt(2 tau Sigma_yy) with Sigma = conic^-1; `rel` covers the cancellation in det
    const float s = 2.f * tau / det;
    const float rel = 1e-4f + 2.4e-7f * ((ca * cc + cb * cb) / det);
    const float hx = sqrtf(s * cc) * (1.f + rel) + 0.01f, hy = sqrtf(s * ca) * (1.f + rel) + 0.01f;
    const float ts = (float)tile_size;
    // tile column t holds the pixel centres t ts + 0.5 ... t ts + ts - 0.5
    const float fx0 = fminf(fmaxf(ceilf((mx - hx - (ts - 0.5f)) / ts), 0.f), (float)tw);
    const float fx1 = fminf(fmaxf(floorf((mx + hx - 0.5f) / ts) + 1.f, 0.f), (float)tw);
    const float fy0 = fminf(fmaxf(ceilf((my - hy - (ts - 0.5f)) / ts), 0.f), (float)th);
    const float fy1 = fminf(fmaxf(floorf((my + hy - 0.5f) / ts) + 1.f, 0.f), (float)th);
    x0 = max(x0, (int)fx0); x1 = max(min(x1, (int)fx1), x0);
    y0 = max(y0, (int)fy0); y1 = max(min(y1, (int)fy1), y0);
}

// blockIdx -> tile for the compositing kernels: the identity.  Hardware places block b on XCD b % 8; measured on the 1080p / 1 M
// benchmark frame (raster_bwd, ms; the other two orders: docs/history.md, section 13):
//   one contiguous band of tile rows per XCD (neighbouring tiles share a 4 MiB L2)                     1.89
//   identity: consecutive tiles round-robin over the XCDs                                              1.87
//   bands over a row-interleaved image (every XCD gets rows from the whole height)                     1.91
// Both kernels are bound by vector instructions, not by L2 misses (0.2 TB/s of HBM traffic), so the L2 locality of the
// bands buys nothing here and the finer interleave of the identity order balances the XCDs slightly better.
// List cells (dnsplat_raster_cells): a cell's list holds every Gaussian whose tile box touches one of the cell's tiles, but a tile only
// composites the Gaussians whose box holds the tile ITSELF — the box is clipped to gsplat's 3-sigma box (A.3), outside of which a
// splat of opacity > 0.35 still reaches alpha >= 1/255 and the reference does not blend it.  b = the Gaussian's record of
// dnsplat_proj_out.tile_boxes (first tile id within the camera's grid of tw columns, width | height << 16); inv_tw = 1.f / tw.
// The row of the first tile through the fp32 reciprocal is at most one off below 2^24 tiles and is put right; beyond, by division.
__device__ __forceinline__ bool dns_tile_in_box(int2 b, int tx, int ty, int tw, float inv_tw)
{
    int y0, x0;
    if (b.x < (1 << 24)) {
        y0 = (int)((float)b.x * inv_tw);
        x0 = b.x - y0 * tw;
        if (x0 < 0) { x0 += tw; --y0; }
        else if (x0 >= tw) { x0 -= tw; ++y0; }
    } else {
        y0 = b.x / tw;
        x0 = b.x - y0 * tw;
    }
    return (unsigned)(tx - x0) < ((unsigned)b.y & 0xffffu) && (unsigned)(ty - y0) < ((unsigned)b.y >> 16);
}

__device__ __forceinline__ int dns_tile_of_block(int b, int n_tiles, int tw)
{
    return b;
}

// ------------------------------------------------------------------------------------------------
// Compositing math shared by the forward and backward kernels, so that both take bit-identical
// decisions on (pixel, splat) pairs:
//     sigma = 1/2 (a dx^2 + c dy^2) + b dx dy,  vis = exp(-sigma),  alpha = min(0.999, o vis),
//     pair skipped if sigma < 0 or alpha < 1/255.
// The exponent is evaluated as exp2 of a pre-scaled quadratic form: e = -log2(e) * sigma with the
// scaling folded into the three conic coefficients once per splat (3 multiplies per splat instead of
// one per pair).  The fused-multiply-add sequence is spelled out so that compiler contraction
// cannot make the two kernels round differently.
#define DNS_LOG2E 1.4426950408889634f

// The quadratic form is evaluated through its two half-gradients,
//     u = na dx + hb dy,  w = hb dx + nc dy,  e = dx u + dy w        (na, hb, nc = -log2e/2 * (a, b, c)),
// which are exactly what the backward needs for d sigma / d(dx, dy) = -(2 / log2e) (u, w): the mean gradient costs one
// multiply per component instead of rebuilding a dx + b dy from the unscaled conic (3 packed instructions less per
// step, and the unscaled conic leaves the backward's registers).  The forward shares na dx and hb dx between the two
// pixels of a lane, so it pays nothing for the sixth operation.

struct DnsConicE {
    float na, nb, nc;  // -log2e/2 * (a, b, c); nb is the hb of the formulas above
};

__device__ __forceinline__ DnsConicE dns_conic_e(float ca, float cb, float cc)
{
    DnsConicE q;
    q.na = (-0.5f * DNS_LOG2E) * ca;
    q.nb = (-0.5f * DNS_LOG2E) * cb;
    q.nc = (-0.5f * DNS_LOG2E) * cc;
    return q;
}

// e = -log2e * sigma  (<= 0 for a valid pair).  The operation sequence below is THE definition both compositing kernels
// follow instruction for instruction (the backward in packed form), so that they take bit-identical skip decisions.
__device__ __forceinline__ float dns_half_grad_u(const DnsConicE &q, float dx, float dy) { return __builtin_fmaf(q.nb, dy, q.na * dx); }
__device__ __forceinline__ float dns_half_grad_w(const DnsConicE &q, float dx, float dy) { return __builtin_fmaf(q.nc, dy, q.nb * dx); }
__device__ __forceinline__ float dns_exponent(const DnsConicE &q, float dx, float dy)
{
    const float u = dns_half_grad_u(q, dx, dy), w = dns_half_grad_w(q, dx, dy);
    return __builtin_fmaf(dx, u, dy * w);
}

// WHEN THE TEST `e <= 0` CANNOT FAIL.  dns_exponent() rounds six times:
//     p1 = fl(na dx)   u = fl(nb dy + p1)   p2 = fl(nb dx)   w = fl(nc dy + p2)   p3 = fl(dy w)   e = fl(dx u + p3)
// with fl(x) = x (1 + d), |d| <= eps = 2^-24 while nothing under- or overflows.  Multiplying out, every one of the four terms
// na dx^2, nb dx dy (twice), nc dy^2 of the exact form reaches e through at most three roundings, so
//     e = E + r,    E = na dx^2 + 2 nb dx dy + nc dy^2  (exact, of the STORED na, nb, nc),    |r| <= ((1 + eps)^3 - 1) S,
//     S = |na| dx^2 + 2 |nb| |dx dy| + |nc| dy^2   (the sum of the terms' magnitudes).
// With na, nc < 0 and rho = |nb| / sqrt(na nc):  m = |na| dx^2 + |nc| dy^2 >= 2 sqrt(na nc) |dx dy| (AM-GM), so the cross term
// t = 2 |nb dx dy| <= rho m, and  -E >= m - t >= (1 - rho) m,  S = m + t <= (1 + rho) m:
//     S <= (1 + rho) / (1 - rho) |E|,        e <= 0 is certain once   3.0000002 eps (1 + rho) / (1 - rho) < 1.
// The rule below is stated on the record's conic (a, b, c) as stored: b^2 <= (1 - 2^-12) a c.  Its own three roundings and the
// three of dns_conic_e() (na = fl(k a), ...) move rho^2 by a factor within (1 + eps)^7: rho^2 <= 1 - 2^-12 + 2^-21, hence
// 1 - rho >= (1 - rho^2) / 2 >= 2^-13.001, (1 + rho) / (1 - rho) <= 2^14.001 = 1.64e4 and 3 eps S / |E| <= 2.93e-3: a margin of
// 340x.  (The largest constant with the 16x margin asked of such a bound would be 1 - 2^-16; nothing needs it.)
// "Nothing under- or overflows": a, c in [2^-40, 2^40] — eight orders of magnitude beyond what a projection with eps2d > 0 and a
// radius clip can produce.  Then a c and b^2 are finite and normal (inf <= inf cannot pass), and for a pixel offset that is 0 or at
// least 2^-25 in magnitude (a difference of a mean and a pixel centre k + 1/2 cannot be smaller) and at most 2^14, every product
// above lies between 2^-116 and 2^69 or is an exact zero, and |E| >= 2^-13 2^-41 2^-50 is far above the subnormals.
// dx = dy = 0 gives e = +0, which passes `<= 0` as it always did.  A NaN in a, b or c fails a comparison: not benign.
// tests/test_conic_benign_bound.py restates the sequence in numpy and checks 10^7 pairs, a subset in exact rationals.
// Evaluated by the projection (which raises dnsplat_proj_out.saturation_flag for a visible Gaussian that fails it) on the record
// floats as they are stored; contraction is pinned off so that the products round before they are compared.
__device__ __forceinline__ bool dns_conic_benign(float a, float b, float c)
{
#pragma clang fp contract(off)
    const float lo = 0x1p-40f, hi = 0x1p40f;
    return a >= lo && a <= hi && c >= lo && c <= hi && b * b <= (1.f - 0x1p-12f) * (a * c);
}

__device__ __forceinline__ float dns_exp2(float e) { return __builtin_amdgcn_exp2f(e); }

// Conservative test "no pixel centre of the rectangle [xl,xh] x [yl,yh] can pass alpha >= 1/255 for this
// splat".  The exact minimum of the quadratic form over the rectangle (it lies on the edge(s) nearest to
// the mean when the mean is outside) is compared with ln(255 o) plus a safety margin that dominates the
// fp32 rounding of the per-pixel evaluation, so a culled splat is one the per-pixel test would have
// skipped for every pixel: skipping it changes no result bit.  NaNs compare false => keep.
// The minimiser along an edge is located with v_rcp_f32 (1 ulp) instead of an IEEE division: an error of the location enters the
// value at second order (~1e-13 relative), eleven orders below the margin, and saves ~16 instructions per test.
__device__ __forceinline__ bool dns_cull_rect(float sx, float sy, float ca, float cb, float cc, float opac,
                                              float xl, float xh, float yl, float yh)
{
    const float dxl = sx - xh, dxh = sx - xl, dyl = sy - yh, dyh = sy - yl;
    const float X = fminf(fmaxf(0.f, dxl), dxh);  // point of [dxl,dxh] nearest to 0
    const float Y = fminf(fmaxf(0.f, dyl), dyh);
    float smin = 0.f, pos = 0.f;
    if (X != 0.f || Y != 0.f) {
        float sxe = 3.0e38f, sye = 3.0e38f, pxe = 0.f, pye = 0.f;
        if (X != 0.f) {
            const float dy = fminf(fmaxf(-cb * X * __builtin_amdgcn_rcpf(cc), dyl), dyh);
            pxe = 0.5f * (ca * X * X + cc * dy * dy);
            sxe = pxe + cb * X * dy;
        }
        if (Y != 0.f) {
            const float dx = fminf(fmaxf(-cb * Y * __builtin_amdgcn_rcpf(ca), dxl), dxh);
            pye = 0.5f * (ca * dx * dx + cc * Y * Y);
            sye = pye + cb * dx * Y;
        }
        if (sxe < sye) { smin = sxe; pos = pxe; } else { smin = sye; pos = pye; }
    }
    const float tau = __logf(255.f * opac);
    return smin > tau + 0.02f + 1e-5f * pos;
}
