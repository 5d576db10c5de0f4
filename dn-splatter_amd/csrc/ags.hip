// ags.hip — the filtered normal loss of the AGS-Mesh regularisation strategy (regularization_strategy.py:292-321
// AGSMeshRegularization.get_normal_loss with :40-96 find_edges and :11-26 mean_angular_error), value and gradients in two launches.
//
// Per channel of the ground-truth normal n in [-1, 1]:  r = 1 / (n + 1e-6),  lap = up + down + left + right - 4 r  with zeros outside the
// frame,  e = lap > 0.01,  E = OR of e over the 3 x 3 neighbourhood (zeros outside again).  Per pixel:  C = not (dot(n, surf) < cos 0.1)
// — the reference's not (arccos(clip(dot, -1, 1)) > 0.1); a nan dot product is confident on both sides.
//   mode 0:  A = sum over the ELEMENTS with ~E of |surf - n|,  count = their number
//   mode 1:  A = sum over the three channels of the confident pixels,  count = 3 x their number
//   B = sum over all elements of |pred - n|
// The reference evaluates this with six one-channel conv2d calls and two boolean-mask gathers (a host synchronisation each).  Here:
//   ags_normal_kernel   one workgroup per AG_TW x AG_TH tile.  Mode 0 stages the reciprocals of the tile plus a two-pixel halo in LDS
//                       (one pixel for the Laplacian, one more for the dilation), then the threshold bits of the tile plus one pixel,
//                       three bits to a byte; each thread then ORs 3 x 3 bytes and finishes its own four pixels.  Mode 1 needs no
//                       neighbour.  One partial (two sums in double, one integer count) per workgroup;
//   ags_fold_kernel     one workgroup adds the partials in the fixed order of block_reduce.h (dns_block_join, dns_fold_partials).
// No atomic and no floating-point sum whose order depends on scheduling: equal inputs give equal bits.  The normaliser 1 / count is
// only known here on the device; the caller divides there.  Compiled without contraction: 2 x - 1, n + 1e-6, the correctly rounded
// 1 / x and the five-term sum are the fp32 operations torch performs, in the order  ((up + down) + left) + right - 4 r.
// Traffic: 36 B read and 24 B written per pixel (plus the halo's share of the ground truth, from cache).

#include "block_reduce.h"

namespace {

constexpr int AG_THREADS = 256;
constexpr int AG_TW = 64, AG_TH = 16;                    // the tile: thread t owns column t % 64 of rows t / 64 + 4 k, k = 0 .. 3
constexpr int AG_PER = AG_TW * AG_TH / AG_THREADS;       // pixels per thread
constexpr int AG_RW = AG_TW + 4, AG_RH = AG_TH + 4;      // reciprocals: the tile and two pixels around it
constexpr int AG_EW = AG_TW + 2, AG_EH = AG_TH + 2;      // threshold bits: the tile and one pixel around it
constexpr float AG_EPS = 1e-6f;                          // find_edges: 1 / (im + 1e-6)
constexpr float AG_EDGE = 0.01f;                         // find_edges: threshold
constexpr float AG_COS = 0.99500416527802577f;           // cos(0.1): arccos(d) > 0.1  <=>  d < cos(0.1)

struct AgsPartial {                                      // 24 bytes
    double a, b;
    long long n;
    static __device__ AgsPartial identity() { return AgsPartial{0.0, 0.0, 0}; }
    __device__ void join(const AgsPartial &o) { a += o.a; b += o.b; n += o.n; }
};

template <bool HWC>
__device__ __forceinline__ size_t ag_index(int c, int y, int x, int W, size_t P)
{
    return HWC ? ((size_t)y * W + x) * 3 + c : (size_t)c * P + (size_t)y * W + x;
}

// the value the losses see: the tensor itself ([3,H,W] in [-1,1]) or 2 x - 1 of an [H,W,3] image in [0,1] (2 x is exact: one rounding)
template <bool HWC>
__device__ __forceinline__ float ag_load(const float *__restrict__ t, int c, int y, int x, int W, size_t P)
{
    const float v = t[ag_index<HWC>(c, y, x, W, P)];
    return HWC ? __fsub_rn(__fmul_rn(2.0f, v), 1.0f) : v;
}

__device__ __forceinline__ float ag_sign(float d) { return (float)((d > 0.f) - (d < 0.f)); }

template <int MODE, bool HWC>
__global__ __launch_bounds__(AG_THREADS) void ags_normal_kernel(int W, int H, int tiles_x, const float *__restrict__ surf,
                                                                 const float *__restrict__ gt, const float *__restrict__ pred, float w_surf,
                                                                 float w_pred, float *__restrict__ v_surf, float *__restrict__ v_pred,
                                                                 uint8_t *__restrict__ selection, AgsPartial *__restrict__ part)
{
    __shared__ float R[MODE == 0 ? 3 : 1][MODE == 0 ? AG_RH : 1][MODE == 0 ? AG_RW : 1];
    __shared__ uint8_t E[MODE == 0 ? AG_EH : 1][MODE == 0 ? AG_EW : 4];
    __shared__ AgsPartial red[AG_THREADS / DNS_WAVE];
    const int t = threadIdx.x;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x0 = tile_x * AG_TW, y0 = tile_y * AG_TH;
    const size_t P = (size_t)W * H;

    if constexpr (MODE == 0) {
        for (int i = t; i < AG_RH * AG_RW; i += AG_THREADS) {
            const int ly = i / AG_RW, lx = i - ly * AG_RW;
            const int y = y0 - 2 + ly, x = x0 - 2 + lx;
            const bool in = y >= 0 && y < H && x >= 0 && x < W;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                R[c][ly][lx] = in ? __fdiv_rn(1.0f, __fadd_rn(ag_load<HWC>(gt, c, y, x, W, P), AG_EPS)) : 0.f;   // conv2d pads with zeros
        }
        __syncthreads();
        for (int i = t; i < AG_EH * AG_EW; i += AG_THREADS) {
            const int ly = i / AG_EW, lx = i - ly * AG_EW;
            const int y = y0 - 1 + ly, x = x0 - 1 + lx;
            uint8_t bits = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {                       // outside the frame the dilation sees zeros
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float up = R[c][ly][lx + 1], down = R[c][ly + 2][lx + 1], left = R[c][ly + 1][lx], right = R[c][ly + 1][lx + 2];
                    const float lap = __fsub_rn(__fadd_rn(__fadd_rn(__fadd_rn(up, down), left), right), __fmul_rn(4.0f, R[c][ly + 1][lx + 1]));
                    if (lap > AG_EDGE) bits |= (uint8_t)(1u << c);          // nan > 0.01 is false
                }
            }
            E[ly][lx] = bits;
        }
        __syncthreads();
    }

    const int tx = t & (AG_TW - 1), ty = t / AG_TW;
    const int x = x0 + tx;
    AgsPartial v = AgsPartial::identity();
#pragma unroll
    for (int k = 0; k < AG_PER; ++k) {
        const int ly = ty + k * (AG_THREADS / AG_TW);
        const int y = y0 + ly;
        if (x >= W || y >= H) continue;
        float g[3], s[3], p[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g[c] = ag_load<HWC>(gt, c, y, x, W, P);
            s[c] = ag_load<HWC>(surf, c, y, x, W, P);
            p[c] = ag_load<HWC>(pred, c, y, x, W, P);
        }
        unsigned keep;                                                       // bit c: element (c, y, x) enters the mean of |surf - n|
        if constexpr (MODE == 0) {
            unsigned dil = 0;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) dil |= E[ly + dy][tx + dx];
            keep = ~dil & 7u;
            if (selection)
#pragma unroll
                for (int c = 0; c < 3; ++c) selection[(size_t)c * P + (size_t)y * W + x] = (uint8_t)((keep >> c) & 1u);
        } else {
            const float dot = __fadd_rn(__fadd_rn(__fmul_rn(g[0], s[0]), __fmul_rn(g[1], s[1])), __fmul_rn(g[2], s[2]));
            keep = !(dot < AG_COS) ? 7u : 0u;                                // a nan dot product counts as confident
            if (selection) selection[(size_t)y * W + x] = (uint8_t)(keep & 1u);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float ds = __fsub_rn(s[c], g[c]), dp = __fsub_rn(p[c], g[c]);
            const bool in = (keep >> c) & 1u;
            if (in) { v.a += (double)fabsf(ds); ++v.n; }
            v.b += (double)fabsf(dp);
            const size_t at = ag_index<HWC>(c, y, x, W, P);
            if (v_surf) v_surf[at] = in ? __fmul_rn(w_surf, ag_sign(ds)) : 0.f;
            if (v_pred) v_pred[at] = __fmul_rn(w_pred, ag_sign(dp));
        }
    }

    dns_block_join<AG_THREADS>(v, red);
    if (t == 0) part[blockIdx.x] = v;
}

// the partials of all workgroups, added in the one fixed order of dns_fold_partials (block_reduce.h)
__global__ __launch_bounds__(AG_THREADS) void ags_fold_kernel(int n_part, const AgsPartial *__restrict__ part, double *__restrict__ sums,
                                                               int64_t *__restrict__ count)
{
    __shared__ AgsPartial red[AG_THREADS / DNS_WAVE];
    AgsPartial v;
    dns_fold_partials<AG_THREADS>(part, n_part, v, red);
    if (threadIdx.x == 0) {
        sums[0] = v.a;
        sums[1] = v.b;
        count[0] = (int64_t)v.n;
    }
}

long long ags_tiles(int32_t width, int32_t height)
{
    return (((long long)width + AG_TW - 1) / AG_TW) * (((long long)height + AG_TH - 1) / AG_TH);
}

}  // namespace

extern "C" size_t dnsplat_ags_normal_scratch_bytes(int32_t width, int32_t height)
{
    if (width < 1 || height < 1) return 0;
    return (size_t)ags_tiles(width, height) * sizeof(AgsPartial);
}

extern "C" int dnsplat_ags_normal_loss(int32_t width, int32_t height, const float *surf, const float *gt, const float *pred, int32_t layout,
                                       int32_t mode, float weight, float *v_surf, float *v_pred, uint8_t *selection, void *scratch,
                                       double *sums, int64_t *count, dnsplat_stream_t stream_)
{
    if (!surf || !gt || !pred || !scratch || !sums || !count || width < 1 || height < 1) return DNSPLAT_ERR_INVALID_ARG;
    if ((layout != DNSPLAT_AGS_LAYOUT_CHW && layout != DNSPLAT_AGS_LAYOUT_HWC) || (mode != 0 && mode != 1)) return DNSPLAT_ERR_INVALID_ARG;
    const long long tiles = ags_tiles(width, height);
    // pixel coordinates of a tile's halo are ints, and there is one workgroup per tile in a one-dimensional grid
    if (width > (1 << 30) || height > (1 << 30) || tiles > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const int tiles_x = (int)(((long long)width + AG_TW - 1) / AG_TW);
    const bool hwc = layout == DNSPLAT_AGS_LAYOUT_HWC;
    // d(2 x - 1) / dx folded in; the mean of |pred - n| has a normaliser known here
    const float w_surf = hwc ? 2.0f * weight : weight;
    const float w_pred = (float)((double)w_surf / (3.0 * (double)width * (double)height));
    AgsPartial *part = (AgsPartial *)scratch;
#define AGS_LAUNCH(MODE, HWC)                                                                                                        \
    hipLaunchKernelGGL((ags_normal_kernel<MODE, HWC>), dim3((unsigned)tiles), dim3(AG_THREADS), 0, stream, width, height, tiles_x, surf, gt, \
                       pred, w_surf, w_pred, v_surf, v_pred, selection, part)
    if (mode == 0) { if (hwc) AGS_LAUNCH(0, true); else AGS_LAUNCH(0, false); }
    else           { if (hwc) AGS_LAUNCH(1, true); else AGS_LAUNCH(1, false); }
#undef AGS_LAUNCH
    hipLaunchKernelGGL(ags_fold_kernel, dim3(1), dim3(AG_THREADS), 0, stream, (int)tiles, (const AgsPartial *)part, sums, count);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
