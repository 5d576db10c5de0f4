// metrics.hip — the evaluation scores of DNSplatterModel.get_image_metrics_and_images (dn_model.py:809-926) and get_metrics_dict
// (:731-807): DepthMetrics.forward (metrics.py:130-149), NormalMetrics.forward (:171-183) with mean_angular_error (:59-74), and the
// mse / psnr of PeakSignalNoiseRatio(data_range=1.0), for one frame in one entry-point call.
//
// The reference evaluates gt[mask] / pred[mask] about twenty times (a boolean-mask gather of data-dependent size, so a host
// synchronisation, each), ends NormalMetrics in torch.median over 3 H W values (a sort-based selection) and reads fourteen results back
// with fourteen .item() calls.  Here:
//   mt_zero_kernel     (normal pair only) zeroes the three histograms and sets the wanted rank (n - 1) / 2, n = 3 H W;
//   mt_sweep_kernel    one workgroup per MT_SPAN pixels reads the given pairs ONCE: every sum as one partial per workgroup in double,
//                      the counts as integers, and round one of the median's radix selection (the top 11 of the 31 value bits of
//                      |g - p|) in an LDS histogram that is then added to the global one;
//   mt_select_kernel   one workgroup finds the bin that holds the wanted rank and leaves prefix and remaining rank in scratch;
//   mt_hist_kernel     rounds two (11 bits) and three (9 bits) re-read the two normal images as flat arrays (float4 where both are
//                      16-byte aligned) and count only the elements whose prefix matches;
//   mt_finish_kernel   the last selection, the partials added in the one fixed order of block_reduce.h (dns_fold_partials), the
//                      divisions, square roots and log10 in double, rounded once to fp32.
// The host reads nothing between the launches.  No floating-point atomic: the histograms are integers (LDS adds, then 64-bit global
// adds: order-independent), the sums are per-workgroup partials folded in a fixed order: equal inputs give equal bits.
// Non-negative floats order as their bit patterns, nan patterns above inf; torch.median returns nan if any value is nan, which is the
// count of nan differences here.  The decisions (gt > tolerance, t < 1.25^k, the bits of |g - p|) are single correctly rounded fp32
// operations, compiled without contraction: they are torch's, bit for bit.
// The hazard of an LDS histogram: on real images almost all of |g - p| falls into a few dozen of round one's bins, on identical images
// into ONE, and 64 lanes adding to one LDS word serialise.  dns_hist_add<MT_PEEL> (block_reduce.h) peels equal bins within the wave
// first (the first active lane's bin, one add of the ballot's population count), MT_PEEL times; what is left adds per lane.  Measured
// at 1600 x 1200 (docs/history.md, section 15): one peel costs 3 % on random images and covers the one-bin case; peeling until
// nothing is left (up to 64 rounds on random images) doubles the call.
// Traffic: 56 B per pixel read once, plus 24 B per pixel for each of rounds two and three.

#include "block_reduce.h"

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / DNS_WAVE;
constexpr int MT_PER = 4;                                // pixels per thread of the sweep
constexpr int MT_SPAN = MT_THREADS * MT_PER;             // pixels per workgroup of the sweep
constexpr int MT_HPER = 16;                              // elements per thread of rounds two and three
constexpr int MT_HSPAN = MT_THREADS * MT_HPER;           // elements per workgroup there
constexpr int MT_BITS1 = 11, MT_BITS2 = 11, MT_BITS3 = 9;
constexpr int MT_BINS1 = 1 << MT_BITS1, MT_BINS2 = 1 << MT_BITS2, MT_BINS3 = 1 << MT_BITS3;
#ifndef MT_PEEL
#define MT_PEEL 1
#endif
constexpr int MT_ND = 8, MT_NI = 6;                      // sums and counts of a partial

struct MtPartial {                                       // 112 bytes
    double d[MT_ND];                                     // DNSPLAT_METRIC_SUM_* order
    long long i[MT_NI];                                  // masked, a1, a2, a3, non-nan log terms, nan normal differences
    static __device__ MtPartial identity() { return MtPartial{}; }
    __device__ void join(const MtPartial &o)
    {
#pragma unroll
        for (int k = 0; k < MT_ND; ++k) d[k] += o.d[k];
#pragma unroll
        for (int k = 0; k < MT_NI; ++k) i[k] += o.i[k];
    }
};

struct MtState {                                         // 64 bytes at the head of the scratch
    unsigned long long rank;                             // the wanted rank among the elements that share `prefix`
    unsigned int prefix;                                 // the value bits selected so far
    unsigned int pad[13];
};

struct MtScratch {
    MtState *state;
    unsigned long long *hist1, *hist2, *hist3;
    MtPartial *part;
};

__host__ __device__ inline MtScratch mt_carve(void *scratch)
{
    MtScratch s;
    char *p = (char *)scratch;
    s.state = (MtState *)p;                    p += sizeof(MtState);
    s.hist1 = (unsigned long long *)p;         p += sizeof(unsigned long long) * MT_BINS1;
    s.hist2 = (unsigned long long *)p;         p += sizeof(unsigned long long) * MT_BINS2;
    s.hist3 = (unsigned long long *)p;         p += sizeof(unsigned long long) * MT_BINS3;
    s.part = (MtPartial *)p;
    return s;
}

constexpr size_t MT_HEAD_BYTES = sizeof(MtState) + sizeof(unsigned long long) * (MT_BINS1 + MT_BINS2 + MT_BINS3);

__global__ __launch_bounds__(MT_THREADS) void mt_zero_kernel(unsigned long long n, void *scratch)
{
    const MtScratch s = mt_carve(scratch);
    const int i = blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < MT_BINS1 + MT_BINS2 + MT_BINS3) s.hist1[i] = 0ull;                    // the three histograms are contiguous
    if (i == 0) { s.state->rank = (n - 1ull) / 2ull; s.state->prefix = 0u; }      // torch.median: the LOWER median
}

template <bool HWC>
__device__ __forceinline__ size_t mt_index(int c, size_t p, size_t P) { return HWC ? p * 3 + c : (size_t)c * P + p; }

template <bool NORMAL_HWC>
__global__ __launch_bounds__(MT_THREADS) void mt_sweep_kernel(long long P, const float *__restrict__ rgb, const float *__restrict__ gt_rgb,
                                                               const float *__restrict__ depth, const float *__restrict__ gt_depth,
                                                               float tolerance, const float *__restrict__ normal,
                                                               const float *__restrict__ gt_normal, void *scratch)
{
    __shared__ unsigned int hist[MT_BINS1];
    __shared__ MtPartial red[MT_WAVES];
    const MtScratch s = mt_carve(scratch);
    const int t = threadIdx.x;
    if (normal)
        for (int b = t; b < MT_BINS1; b += MT_THREADS) hist[b] = 0u;
    __syncthreads();

    double d[MT_ND];
    long long n[MT_NI];
#pragma unroll
    for (int k = 0; k < MT_ND; ++k) d[k] = 0.0;
#pragma unroll
    for (int k = 0; k < MT_NI; ++k) n[k] = 0;

    const long long base = (long long)blockIdx.x * MT_SPAN;
#pragma unroll
    for (int k = 0; k < MT_PER; ++k) {
        const long long p = base + (long long)k * MT_THREADS + t;
        const bool in = p < P;                                                   // every lane stays for the wave-wide histogram adds
        if (rgb && in) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float e = __fsub_rn(gt_rgb[(size_t)p * 3 + c], rgb[(size_t)p * 3 + c]);
                d[DNSPLAT_METRIC_SUM_RGB_SQ] += (double)e * (double)e;
            }
        }
        if (depth && in) {
            const float g = gt_depth[p], q = depth[p];
            if (g > tolerance) {                                                 // nan > tolerance is false
                const float a = __fdiv_rn(g, q), b = __fdiv_rn(q, g);
                // torch.max of the two quotients: nan if either is; a nan is below no threshold
                if (!(a != a) && !(b != b)) {
                    const float r = fmaxf(a, b);
                    n[1] += r < 1.25f;
                    n[2] += r < 1.5625f;
                    n[3] += r < 1.953125f;
                }
                ++n[0];
                const double e = (double)g - (double)q;
                d[DNSPLAT_METRIC_SUM_DEPTH_SQ] += e * e;
                d[DNSPLAT_METRIC_SUM_DEPTH_ABS_REL] += fabs(e) / (double)g;
                d[DNSPLAT_METRIC_SUM_DEPTH_SQ_REL] += e * e / (double)g;
                const double l = fabs(log((double)g) - log((double)q));        // sqrt of the square, as the reference writes it
                if (!(l != l)) { d[DNSPLAT_METRIC_SUM_DEPTH_LOG] += l; ++n[4]; }  // nanmean drops the nan terms (a negative prediction)
            }
        }
        if (normal) {                                                            // uniform over the grid
            float g[3] = {0.f, 0.f, 0.f}, q[3] = {0.f, 0.f, 0.f};
            if (in) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    g[c] = gt_normal[mt_index<NORMAL_HWC>(c, (size_t)p, (size_t)P)];
                    q[c] = normal[mt_index<NORMAL_HWC>(c, (size_t)p, (size_t)P)];
                }
                float dot = __fadd_rn(__fadd_rn(__fmul_rn(g[0], q[0]), __fmul_rn(g[1], q[1])), __fmul_rn(g[2], q[2]));
                dot = dot < -1.0f ? -1.0f : (dot > 1.0f ? 1.0f : dot);           // torch.clamp keeps a nan
                d[DNSPLAT_METRIC_SUM_NORMAL_ANGLE] += acos((double)dot);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float e = fabsf(__fsub_rn(g[c], q[c]));
                const unsigned int v = __float_as_uint(e) & 0x7fffffffu;
                if (in) {
                    d[DNSPLAT_METRIC_SUM_NORMAL_SQ] += (double)e * (double)e;
                    d[DNSPLAT_METRIC_SUM_NORMAL_ABS] += (double)e;
                    n[5] += v > 0x7f800000u;
                }
                dns_hist_add<MT_PEEL>(hist, v >> (MT_BITS2 + MT_BITS3), in);
            }
        }
    }

    // dns_block_join's order, written out field by field: with the fourteen fields in one struct this kernel, which sits exactly at
    // 64 VGPRs, needs 71 to 80 and loses up to two waves per SIMD (docs/history.md, section 24)
#pragma unroll
    for (int off = DNS_WAVE / 2; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < MT_ND; ++k) d[k] += __shfl_xor(d[k], off, DNS_WAVE);
#pragma unroll
        for (int k = 0; k < MT_NI; ++k) n[k] += __shfl_xor(n[k], off, DNS_WAVE);
    }
    if ((t & (DNS_WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < MT_ND; ++k) red[t / DNS_WAVE].d[k] = d[k];
#pragma unroll
        for (int k = 0; k < MT_NI; ++k) red[t / DNS_WAVE].i[k] = n[k];
    }
    __syncthreads();
    if (t < MT_ND) s.part[blockIdx.x].d[t] = (red[0].d[t] + red[1].d[t]) + (red[2].d[t] + red[3].d[t]);
    else if (t < MT_ND + MT_NI) {
        const int k = t - MT_ND;
        s.part[blockIdx.x].i[k] = (red[0].i[k] + red[1].i[k]) + (red[2].i[k] + red[3].i[k]);
    }
    if (normal) dns_hist_flush<MT_THREADS>(hist, s.hist1, MT_BINS1);
}

// rounds two and three: the elements of |g - p| whose upper bits equal the prefix found so far, counted by their next BITS bits.  The two
// images are flat arrays of n floats in either layout.  VEC: both are 16-byte aligned and are read as float4, four per thread; the
// n % 4 elements behind the last whole float4 go to the first threads of workgroup 0.
template <int ROUND, bool VEC>
__global__ __launch_bounds__(MT_THREADS) void mt_hist_kernel(unsigned long long n, const float *__restrict__ normal,
                                                              const float *__restrict__ gt_normal, void *scratch)
{
    constexpr int BINS = ROUND == 2 ? MT_BINS2 : MT_BINS3;
    constexpr int SHIFT = ROUND == 2 ? MT_BITS3 : 0;                             // the bits below this round's
    constexpr int BITS = ROUND == 2 ? MT_BITS2 : MT_BITS3;
    __shared__ unsigned int hist[BINS];
    const MtScratch s = mt_carve(scratch);
    const int t = threadIdx.x;
    for (int b = t; b < BINS; b += MT_THREADS) hist[b] = 0u;
    __syncthreads();
    const unsigned int prefix = s.state->prefix;
    auto count = [&](float g, float q, bool in) {
        const unsigned int v = __float_as_uint(fabsf(__fsub_rn(g, q))) & 0x7fffffffu;
        dns_hist_add<MT_PEEL>(hist, (v >> SHIFT) & (BINS - 1), in && (v >> (SHIFT + BITS)) == prefix);
    };
    if constexpr (VEC) {
        const unsigned long long n4 = n / 4ull;
        const unsigned long long base = (unsigned long long)blockIdx.x * (MT_HSPAN / 4);
        const float4 *__restrict__ g4 = (const float4 *)gt_normal;
        const float4 *__restrict__ q4 = (const float4 *)normal;
        float4 g[MT_HPER / 4], q[MT_HPER / 4];
#pragma unroll
        for (int k = 0; k < MT_HPER / 4; ++k) {
            const unsigned long long i = base + (unsigned long long)k * MT_THREADS + t;
            const bool in = i < n4;
            g[k] = in ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            q[k] = in ? q4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < MT_HPER / 4; ++k) {
            const bool in = base + (unsigned long long)k * MT_THREADS + t < n4;
            count(g[k].x, q[k].x, in);
            count(g[k].y, q[k].y, in);
            count(g[k].z, q[k].z, in);
            count(g[k].w, q[k].w, in);
        }
        if (blockIdx.x == 0) {                                                   // uniform: the wave stays whole for the ballots
            const unsigned long long i = 4ull * n4 + t;
            const bool in = i < n;
            count(in ? gt_normal[i] : 0.f, in ? normal[i] : 0.f, in);
        }
    } else {
        const unsigned long long base = (unsigned long long)blockIdx.x * MT_HSPAN;
#pragma unroll 4
        for (int k = 0; k < MT_HPER; ++k) {
            const unsigned long long i = base + (unsigned long long)k * MT_THREADS + t;
            const bool in = i < n;
            count(in ? gt_normal[i] : 0.f, in ? normal[i] : 0.f, in);
        }
    }
    __syncthreads();
    dns_hist_flush<MT_THREADS>(hist, ROUND == 2 ? s.hist2 : s.hist3, BINS);
}

template <int ROUND>
__global__ __launch_bounds__(MT_THREADS) void mt_select_kernel(void *scratch)
{
    __shared__ unsigned long long wave_sum[MT_WAVES];
    const MtScratch s = mt_carve(scratch);
    const unsigned long long rank = s.state->rank;
    const unsigned int prefix = s.state->prefix;
    __syncthreads();                                                             // every thread has read the state before one rewrites it
    unsigned int bin;
    unsigned long long rest;
    if (dns_find_bin<MT_THREADS, (ROUND == 1 ? MT_BINS1 : MT_BINS2)>(ROUND == 1 ? s.hist1 : s.hist2, rank, wave_sum, bin, rest)) {
        s.state->rank = rest;
        s.state->prefix = (prefix << (ROUND == 1 ? MT_BITS1 : MT_BITS2)) | bin;
    }
}

__global__ __launch_bounds__(MT_THREADS) void mt_finish_kernel(long long P, int n_part, int has_rgb, int has_depth, int has_normal,
                                                                void *scratch, float *__restrict__ metrics, int64_t *__restrict__ counts,
                                                                double *__restrict__ sums)
{
    __shared__ MtPartial red[MT_WAVES];
    __shared__ unsigned long long wave_sum[MT_WAVES];
    __shared__ unsigned int median_bits;
    const MtScratch s = mt_carve(scratch);
    const int t = threadIdx.x;
    if (t == 0) median_bits = 0x7fc00000u;
    __syncthreads();
    if (has_normal) {
        unsigned int bin;
        unsigned long long rest;
        if (dns_find_bin<MT_THREADS, MT_BINS3>(s.hist3, s.state->rank, wave_sum, bin, rest)) median_bits = (s.state->prefix << MT_BITS3) | bin;
    }

    MtPartial v;
    dns_fold_partials<MT_THREADS>(s.part, n_part, v, red);                       // its barriers also publish median_bits
    if (t != 0) return;
    const double (&d)[MT_ND] = v.d;
    const long long (&n)[MT_NI] = v.i;

    const float nanf_ = __uint_as_float(0x7fc00000u);
    for (int k = 0; k < DNSPLAT_METRIC_COUNT; ++k) metrics[k] = k < DNSPLAT_METRIC_USED ? nanf_ : 0.f;   // an absent pair: nan
    for (int k = 0; k < DNSPLAT_METRIC_COUNTS; ++k) counts[k] = k < MT_NI ? (int64_t)n[k] : 0;
    if (sums)
        for (int k = 0; k < DNSPLAT_METRIC_SUMS; ++k) sums[k] = d[k];
    const double px = (double)P, el = 3.0 * (double)P;
    if (has_rgb) {
        const double mse = d[DNSPLAT_METRIC_SUM_RGB_SQ] / el;
        metrics[DNSPLAT_METRIC_RGB_MSE] = (float)mse;
        metrics[DNSPLAT_METRIC_RGB_PSNR] = (float)(10.0 * log10(1.0 / mse));
    }
    if (has_depth) {
        const double m = (double)n[0];                                           // no masked pixel: 0 / 0 = nan everywhere
        metrics[DNSPLAT_METRIC_DEPTH_ABS_REL] = (float)(d[DNSPLAT_METRIC_SUM_DEPTH_ABS_REL] / m);
        metrics[DNSPLAT_METRIC_DEPTH_SQ_REL] = (float)(d[DNSPLAT_METRIC_SUM_DEPTH_SQ_REL] / m);
        metrics[DNSPLAT_METRIC_DEPTH_RMSE] = (float)sqrt(d[DNSPLAT_METRIC_SUM_DEPTH_SQ] / m);
        metrics[DNSPLAT_METRIC_DEPTH_RMSE_LOG] = (float)(d[DNSPLAT_METRIC_SUM_DEPTH_LOG] / (double)n[4]);
        metrics[DNSPLAT_METRIC_DEPTH_A1] = (float)((double)n[1] / m);
        metrics[DNSPLAT_METRIC_DEPTH_A2] = (float)((double)n[2] / m);
        metrics[DNSPLAT_METRIC_DEPTH_A3] = (float)((double)n[3] / m);
    }
    if (has_normal) {
        metrics[DNSPLAT_METRIC_NORMAL_MAE] = (float)(d[DNSPLAT_METRIC_SUM_NORMAL_ANGLE] / px);
        metrics[DNSPLAT_METRIC_NORMAL_RMSE] = (float)sqrt(d[DNSPLAT_METRIC_SUM_NORMAL_SQ] / el);
        metrics[DNSPLAT_METRIC_NORMAL_MEAN_ERR] = (float)(d[DNSPLAT_METRIC_SUM_NORMAL_ABS] / el);
        metrics[DNSPLAT_METRIC_NORMAL_MED_ERR] = n[5] > 0 ? nanf_ : __uint_as_float(median_bits);   // torch.median: nan if any is
    }
}

long long mt_spans(long long pixels) { return (pixels + MT_SPAN - 1) / MT_SPAN; }

}  // namespace

extern "C" size_t dnsplat_eval_metrics_scratch_bytes(int32_t width, int32_t height)
{
    if (width < 1 || height < 1) return 0;
    const long long P = (long long)width * (long long)height;
    if (P > 0x7fffffffLL) return 0;
    return MT_HEAD_BYTES + (size_t)mt_spans(P) * sizeof(MtPartial);
}

extern "C" int dnsplat_eval_metrics(const dnsplat_eval_metrics_args *a, dnsplat_stream_t stream_)
{
    if (!a || !a->scratch || !a->metrics || !a->counts || a->width < 1 || a->height < 1) return DNSPLAT_ERR_INVALID_ARG;
    if (!a->rgb != !a->gt_rgb || !a->depth != !a->gt_depth || !a->normal != !a->gt_normal) return DNSPLAT_ERR_INVALID_ARG;
    if (!a->rgb && !a->depth && !a->normal) return DNSPLAT_ERR_INVALID_ARG;
    if (a->normal && a->normal_layout != DNSPLAT_AGS_LAYOUT_CHW && a->normal_layout != DNSPLAT_AGS_LAYOUT_HWC) return DNSPLAT_ERR_INVALID_ARG;
    const long long P = (long long)a->width * (long long)a->height;
    if (P > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const long long spans = mt_spans(P);                                         // <= 2^21
    const unsigned long long n = 3ull * (unsigned long long)P;
    const unsigned int hist_blocks = (unsigned int)((n + MT_HSPAN - 1) / MT_HSPAN);   // <= 2^21
    void *scratch = a->scratch;
    if (a->normal)
        hipLaunchKernelGGL(mt_zero_kernel, dim3((MT_BINS1 + MT_BINS2 + MT_BINS3 + MT_THREADS - 1) / MT_THREADS), dim3(MT_THREADS), 0, stream,
                           n, scratch);
#define MT_SWEEP(HWC)                                                                                                              \
    hipLaunchKernelGGL((mt_sweep_kernel<HWC>), dim3((unsigned)spans), dim3(MT_THREADS), 0, stream, P, a->rgb, a->gt_rgb, a->depth,   \
                       a->gt_depth, a->depth_tolerance, a->normal, a->gt_normal, scratch)
    if (a->normal && a->normal_layout == DNSPLAT_AGS_LAYOUT_HWC) MT_SWEEP(true); else MT_SWEEP(false);
#undef MT_SWEEP
    if (a->normal) {
        hipLaunchKernelGGL(mt_select_kernel<1>, dim3(1), dim3(MT_THREADS), 0, stream, scratch);
        // float4 reads where both images allow them
        const bool vec = (((uintptr_t)a->normal | (uintptr_t)a->gt_normal) & 15u) == 0;
        if (vec) hipLaunchKernelGGL((mt_hist_kernel<2, true>), dim3(hist_blocks), dim3(MT_THREADS), 0, stream, n, a->normal, a->gt_normal, scratch);
        else     hipLaunchKernelGGL((mt_hist_kernel<2, false>), dim3(hist_blocks), dim3(MT_THREADS), 0, stream, n, a->normal, a->gt_normal, scratch);
        hipLaunchKernelGGL(mt_select_kernel<2>, dim3(1), dim3(MT_THREADS), 0, stream, scratch);
        if (vec) hipLaunchKernelGGL((mt_hist_kernel<3, true>), dim3(hist_blocks), dim3(MT_THREADS), 0, stream, n, a->normal, a->gt_normal, scratch);
        else     hipLaunchKernelGGL((mt_hist_kernel<3, false>), dim3(hist_blocks), dim3(MT_THREADS), 0, stream, n, a->normal, a->gt_normal, scratch);
    }
    hipLaunchKernelGGL(mt_finish_kernel, dim3(1), dim3(MT_THREADS), 0, stream, P, (int)spans, a->rgb ? 1 : 0, a->depth ? 1 : 0,
                       a->normal ? 1 : 0, scratch, a->metrics, a->counts, a->sums);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
