// geometry.hip — the reference's geometry scores on the device: one direction of distance_p2p (eval/eval_mesh_vis_cull.py:300-321) with
// the scalars PDMetrics / calculate_accuracy / calculate_completeness (metrics.py:11-56) and compute_metrics (:333-397) take from it, and
// the mesh.sample(count, return_index=True) step in front of them.  The reference runs scipy's cKDTree on the CPU for every direction.
//   dnsplat_cloud_distances   gm_search_kernel   one thread per source point: df_search<1> on the index of the targets (density_common.h: the
//                                                nearest under (d^2, index), d^2 in double), |n_src . n_tgt| in double, the per-point outputs,
//                                                and one partial per workgroup: the sums in double, min / max, the counts as integers;
//                             gm_hist_kernel     six rounds (11 + 11 + 11 + 11 + 10 + 10 bits) of a radix selection on the 64-bit patterns of
//                                                d^2 — non-negative doubles order as their patterns, nan patterns above inf — for TWO ranks
//                                                at once, floor(h) and min(floor(h) + 1, n - 1): LDS histograms added to global ones;
//                             gm_select_kernel   one workgroup picks the bin of either rank and leaves prefix and remaining rank in scratch;
//                             gm_finish_kernel   the last pick, the partials added in the one fixed order of block_reduce.h, the square
//                                                roots, numpy's _lerp and the divisions in double.
//   dnsplat_mesh_areas        gm_area_kernel     per triangle: the area in double from the fp32 vertices and the unit face normal.
//   dnsplat_mesh_sample       gm_sample_kernel   per sample: three words of a counter-based hash of (seed, i) (dns_mix32's family, stated in
//                                                dnsplat.h), a binary search in the caller's cdf, a reflected barycentric pair, the point in fp32.
// No floating-point atomic: the histograms are integers (LDS adds, then 64-bit global adds: order-independent) and the sums are
// per-workgroup partials folded in a fixed order, so equal inputs give equal bits.  The host reads nothing between the launches: the two
// ranks and the interpolation weight depend on M and the percentile alone and are kernel arguments.  Compiled without contraction; the
// two FMAs of d^2 are df_search's own.
// The hazard of an LDS histogram is the one metrics.hip names: a cloud scored against itself puts every d^2 into ONE bin in every round.
// dns_hist_add (block_reduce.h) peels the first active lane's bin within the wave once, as it does there.

#include "block_reduce.h"
#include "density_common.h"

namespace {

constexpr int GM_THREADS = 256;
constexpr int GM_WAVES = GM_THREADS / DNS_WAVE;
constexpr int GM_HPER = 8;                                // d^2 values per thread of a histogram round
constexpr int GM_HSPAN = GM_THREADS * GM_HPER;
constexpr int GM_ROUNDS = 6;
constexpr int GM_BINS = 2048;                             // of the widest round
constexpr int GM_RANKS = 2;

__host__ __device__ constexpr int gm_bits(int round) { return round < 4 ? 11 : 10; }
__host__ __device__ constexpr int gm_shift(int round) { return round < 4 ? 53 - 11 * round : (round == 4 ? 10 : 0); }   // the bits below the round's

struct GmPartial {                                        // 64 bytes
    double sum_d, sum_d2, sum_dot, min_d, max_d;
    long long n_lt, n_le, n_bad;
    static __device__ GmPartial identity() { return GmPartial{0.0, 0.0, 0.0, INFINITY, -INFINITY, 0, 0, 0}; }
    __device__ void join(const GmPartial &o)
    {
        sum_d += o.sum_d; sum_d2 += o.sum_d2; sum_dot += o.sum_dot;
        min_d = fmin(min_d, o.min_d); max_d = fmax(max_d, o.max_d);
        n_lt += o.n_lt; n_le += o.n_le; n_bad += o.n_bad;
    }
};

struct GmState {                                          // 64 bytes at the head of the scratch
    unsigned long long rank[GM_RANKS];                    // the wanted rank among the elements that share `prefix`
    unsigned long long prefix[GM_RANKS];                  // the pattern bits selected so far
    unsigned long long pad[4];
};

struct GmScratch {
    GmState *state;
    unsigned long long *hist;                             // [GM_ROUNDS][GM_RANKS][GM_BINS]
    GmPartial *part;
};

constexpr size_t GM_HEAD_BYTES = sizeof(GmState) + sizeof(unsigned long long) * GM_ROUNDS * GM_RANKS * GM_BINS;

__host__ __device__ inline GmScratch gm_carve(void *scratch)
{
    GmScratch s;
    char *p = (char *)scratch;
    s.state = (GmState *)p;
    s.hist = (unsigned long long *)(p + sizeof(GmState));
    s.part = (GmPartial *)(p + GM_HEAD_BYTES);
    return s;
}

struct GmSearch {
    DfIndex ix;
    long long M;
    const float *src, *src_normals, *tgt_normals;
    double threshold;
    double *dist2, *absdot;
    int32_t *idx;
    GmPartial *part;
};

__global__ __launch_bounds__(GM_THREADS) void gm_search_kernel(GmSearch a)
{
    __shared__ GmPartial red[GM_WAVES];
    const int t = threadIdx.x;
    const long long m = (long long)blockIdx.x * GM_THREADS + t;
    GmPartial v = GmPartial::identity();
    if (m < a.M) {
        DfList<1> L;
        const bool ok = df_search<1>(a.ix, a.src[m * 3], a.src[m * 3 + 1], a.src[m * 3 + 2], 1, L);
        // no comparable target: every one of them has a nan or an inf coordinate (df_search keeps a row of d^2 = inf; it is no neighbour)
        const bool found = ok && L.i[0] != 0x7fffffff && L.d[0] < (double)INFINITY;
        const int gi = found ? L.i[0] : -1;
        const double d2 = found ? L.d[0] : (double)NAN;
        const double d = sqrt(d2);
        a.dist2[m] = d2;
        if (a.idx) a.idx[m] = gi;
        v.sum_d = d;
        v.sum_d2 = d2;
        if (found) {
            v.min_d = v.max_d = d;
            v.n_lt = d < a.threshold;
            v.n_le = d <= a.threshold;
        } else v.n_bad = 1;
        if (a.src_normals) {
            double dot = (double)NAN;
            if (found) {
                double s[3], g[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    s[c] = (double)a.src_normals[m * 3 + c];
                    g[c] = (double)a.tgt_normals[(size_t)gi * 3 + c];
                }
                const double ls = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
                const double lg = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
#pragma unroll
                for (int c = 0; c < 3; ++c) { s[c] = s[c] / ls; g[c] = g[c] / lg; }  // a zero normal: 0 / 0 = nan, as in the reference
                dot = fabs((g[0] * s[0] + g[1] * s[1]) + g[2] * s[2]);
            }
            if (a.absdot) a.absdot[m] = dot;
            v.sum_dot = dot;
        }
    }
    dns_block_join<GM_THREADS>(v, red);
    if (t == 0) a.part[blockIdx.x] = v;
}

// round `round`: the d^2 whose upper bits equal the prefix of rank s, counted by their next bits, for both ranks
__global__ __launch_bounds__(GM_THREADS) void gm_hist_kernel(int round, long long M, const unsigned long long *__restrict__ dist2, void *scratch)
{
    __shared__ unsigned int hist[GM_RANKS][GM_BINS];
    const GmScratch s = gm_carve(scratch);
    const int t = threadIdx.x;
    for (int b = t; b < GM_RANKS * GM_BINS; b += GM_THREADS) (&hist[0][0])[b] = 0u;
    __syncthreads();
    const int bits = gm_bits(round), shift = gm_shift(round);
    const unsigned long long prefix0 = s.state->prefix[0], prefix1 = s.state->prefix[1];
    const long long base = (long long)blockIdx.x * GM_HSPAN;
#pragma unroll 4
    for (int k = 0; k < GM_HPER; ++k) {
        const long long i = base + (long long)k * GM_THREADS + t;
        const bool in = i < M;                                                   // every lane stays for the wave-wide adds
        const unsigned long long v = in ? dist2[i] : 0ull;
        const unsigned long long above = round == 0 ? 0ull : v >> (shift + bits);
        const unsigned int bin = (unsigned int)(v >> shift) & ((1u << bits) - 1u);
        dns_hist_add(hist[0], bin, in && above == prefix0);
        dns_hist_add(hist[1], bin, in && above == prefix1);
    }
    __syncthreads();
    dns_hist_flush<GM_THREADS>(&hist[0][0], s.hist + (size_t)round * GM_RANKS * GM_BINS, GM_RANKS * GM_BINS);
}

// round 0 starts from the two ranks the host derived from (M, percentile); the later rounds from what the round before left
__global__ __launch_bounds__(GM_THREADS) void gm_select_kernel(int round, unsigned long long k0, unsigned long long k1, void *scratch)
{
    __shared__ unsigned long long wave_sum[GM_WAVES];
    const GmScratch s = gm_carve(scratch);
    unsigned long long rank[GM_RANKS], prefix[GM_RANKS];
#pragma unroll
    for (int r = 0; r < GM_RANKS; ++r) {
        rank[r] = round == 0 ? (r == 0 ? k0 : k1) : s.state->rank[r];
        prefix[r] = round == 0 ? 0ull : s.state->prefix[r];
    }
    __syncthreads();                                                             // every thread has read the state before one rewrites it
#pragma unroll
    for (int r = 0; r < GM_RANKS; ++r) {                                         // wave_sum twice: dns_block_scan's barrier rule
        unsigned int bin;
        unsigned long long rest;
        if (dns_find_bin<GM_THREADS, GM_BINS>(s.hist + ((size_t)round * GM_RANKS + r) * GM_BINS, rank[r], wave_sum, bin, rest)) {
            s.state->rank[r] = rest;
            s.state->prefix[r] = (prefix[r] << gm_bits(round)) | bin;
        }
    }
}

__global__ __launch_bounds__(GM_THREADS) void gm_finish_kernel(long long M, int n_part, int has_normals, double weight, void *scratch,
                                                                double *__restrict__ scalars, int64_t *__restrict__ counts)
{
    __shared__ GmPartial red[GM_WAVES];
    __shared__ unsigned long long wave_sum[GM_WAVES];
    __shared__ unsigned long long order_bits[GM_RANKS];
    const GmScratch s = gm_carve(scratch);
    const int t = threadIdx.x;
    if (t < GM_RANKS) order_bits[t] = 0x7ff8000000000000ull;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < GM_RANKS; ++r) {                                         // wave_sum twice: dns_block_scan's barrier rule
        unsigned int bin;
        unsigned long long rest;
        if (dns_find_bin<GM_THREADS, GM_BINS>(s.hist + ((size_t)(GM_ROUNDS - 1) * GM_RANKS + r) * GM_BINS, s.state->rank[r], wave_sum, bin, rest))
            order_bits[r] = (s.state->prefix[r] << gm_bits(GM_ROUNDS - 1)) | bin;
    }

    GmPartial v;
    dns_fold_partials<GM_THREADS>(s.part, n_part, v, red);                       // its barriers also publish order_bits
    if (t != 0) return;

    const double nan_ = __longlong_as_double(0x7ff8000000000000ll);
    const double n = (double)M;
    const bool bad = v.n_bad > 0;                                                // numpy: a nan among the distances makes all of these nan
    const double lo2 = __longlong_as_double((long long)order_bits[0]), hi2 = __longlong_as_double((long long)order_bits[1]);
    const double lo = sqrt(lo2), hi = sqrt(hi2);
    const double diff = hi - lo;                                                 // numpy's _lerp
    const double lerp = weight >= 0.5 ? hi - diff * (1.0 - weight) : lo + diff * weight;
    for (int k = 0; k < DNSPLAT_GEOM_COUNT; ++k) scalars[k] = 0.0;
    scalars[DNSPLAT_GEOM_MEAN_D] = v.sum_d / n;                                  // a nan row has added its nan
    scalars[DNSPLAT_GEOM_MEAN_D2] = v.sum_d2 / n;
    scalars[DNSPLAT_GEOM_MEAN_ABSDOT] = has_normals ? v.sum_dot / n : nan_;
    scalars[DNSPLAT_GEOM_PERCENTILE] = bad ? nan_ : lerp;
    scalars[DNSPLAT_GEOM_SHARE_LT] = (double)v.n_lt / n;
    scalars[DNSPLAT_GEOM_SHARE_LE] = (double)v.n_le / n;
    scalars[DNSPLAT_GEOM_MIN_D] = bad ? nan_ : v.min_d;
    scalars[DNSPLAT_GEOM_MAX_D] = bad ? nan_ : v.max_d;
    scalars[DNSPLAT_GEOM_ORDER_LO_D2] = lo2;
    scalars[DNSPLAT_GEOM_ORDER_HI_D2] = hi2;
    counts[DNSPLAT_GEOM_N] = (int64_t)M;
    counts[DNSPLAT_GEOM_N_LT] = (int64_t)v.n_lt;
    counts[DNSPLAT_GEOM_N_LE] = (int64_t)v.n_le;
    counts[DNSPLAT_GEOM_N_NONFINITE] = (int64_t)v.n_bad;
}

// ---- the mesh sampler ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(GM_THREADS) void gm_area_kernel(int V, int T, const float *__restrict__ vertices, const int32_t *__restrict__ triangles,
                                                              double *__restrict__ areas, float *__restrict__ normals)
{
    const long long f = (long long)blockIdx.x * GM_THREADS + threadIdx.x;
    if (f >= T) return;
    const int i0 = triangles[f * 3], i1 = triangles[f * 3 + 1], i2 = triangles[f * 3 + 2];
    double area = 0.0;
    float n[3] = {0.f, 0.f, 0.f};
    if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
        double a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v0 = (double)vertices[(size_t)i0 * 3 + c];
            a[c] = (double)vertices[(size_t)i1 * 3 + c] - v0;
            b[c] = (double)vertices[(size_t)i2 * 3 + c] - v0;
        }
        const double cr[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double len = sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
        if (len > 0.0 && len < (double)INFINITY) {                               // a non-finite vertex: area 0 as well, never drawn
            area = 0.5 * len;
#pragma unroll
            for (int c = 0; c < 3; ++c) n[c] = (float)(cr[c] / len);
        }
    }
    areas[f] = area;
    normals[f * 3] = n[0]; normals[f * 3 + 1] = n[1]; normals[f * 3 + 2] = n[2];
}

struct GmSample {
    long long S;
    uint32_t key;
    int T, V;
    const double *cdf;
    const float *vertices, *face_normals;
    const int32_t *triangles;
    float *points, *normals;
    int32_t *faces;
};

__global__ __launch_bounds__(GM_THREADS) void gm_sample_kernel(GmSample a)
{
    const long long i = (long long)blockIdx.x * GM_THREADS + threadIdx.x;
    if (i >= a.S) return;
    const uint32_t c = dns_mix32((uint32_t)i ^ a.key);
    const uint32_t w0 = dns_mix32(c + 0x9e3779b9u), w1 = dns_mix32(c + 2u * 0x9e3779b9u), w2 = dns_mix32(c + 3u * 0x9e3779b9u);
    const double total = a.cdf[a.T - 1];
    const float nanf_ = __uint_as_float(0x7fc00000u);
    float p[3] = {nanf_, nanf_, nanf_}, n[3] = {0.f, 0.f, 0.f};
    int f = -1;
    if (total > 0.0 && total < (double)INFINITY) {
        const double t = ((double)w0 + 0.5) / 4294967296.0 * total;
        int lo = 0, hi = a.T - 1;                                                // the first f with cdf[f] > t; cdf[T - 1] = total > t
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (a.cdf[mid] > t) hi = mid; else lo = mid + 1;
        }
        f = lo;
        const int i0 = a.triangles[(size_t)f * 3], i1 = a.triangles[(size_t)f * 3 + 1], i2 = a.triangles[(size_t)f * 3 + 2];
        // a face with an index outside [0, V) has area 0 and no span in the cdf; this test keeps the read in bounds whatever cdf is given
        if ((unsigned)i0 < (unsigned)a.V && (unsigned)i1 < (unsigned)a.V && (unsigned)i2 < (unsigned)a.V) {
            uint32_t u = w1 >> 8, v = w2 >> 8;                                   // r = u / 2^24: exact in fp32, and so is 1 - r
            if (u + v > (1u << 24)) { u = (1u << 24) - u; v = (1u << 24) - v; }
            const float r1 = (float)u * 0x1p-24f, r2 = (float)v * 0x1p-24f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float v0 = a.vertices[(size_t)i0 * 3 + k];
                const float e1 = a.vertices[(size_t)i1 * 3 + k] - v0, e2 = a.vertices[(size_t)i2 * 3 + k] - v0;
                p[k] = (v0 + r1 * e1) + r2 * e2;
                n[k] = a.face_normals[(size_t)f * 3 + k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { a.points[i * 3 + k] = p[k]; a.normals[i * 3 + k] = n[k]; }
    a.faces[i] = f;
}

long long gm_blocks(long long n, int per) { return (n + per - 1) / per; }

}  // namespace

extern "C" size_t dnsplat_cloud_distances_scratch_bytes(int64_t M)
{
    if (M < 1 || M > 0x7fffffffLL) return 0;
    return GM_HEAD_BYTES + (size_t)gm_blocks(M, GM_THREADS) * sizeof(GmPartial);
}

extern "C" int dnsplat_cloud_distances(const dnsplat_cloud_distances_args *a, dnsplat_stream_t stream_)
{
    if (!a || !a->index || !a->src || !a->dist2 || !a->scalars || !a->counts || !a->scratch) return DNSPLAT_ERR_INVALID_ARG;
    if (a->M < 1 || a->N < 1) return DNSPLAT_ERR_INVALID_ARG;
    if (!a->src_normals != !a->tgt_normals) return DNSPLAT_ERR_INVALID_ARG;
    if (!(a->percentile >= 0.0 && a->percentile <= 100.0)) return DNSPLAT_ERR_INVALID_ARG;      // a nan fails both
    if (a->M > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const long long M = a->M;
    // numpy's default method: the virtual index (n - 1) (q / 100), its floor, the next index clipped, the weight their difference
    const double h = (double)(M - 1) * (a->percentile / 100.0);
    double fl = floor(h);
    if (fl > (double)(M - 1)) fl = (double)(M - 1);
    const unsigned long long k0 = (unsigned long long)fl;
    const unsigned long long k1 = k0 + 1ull < (unsigned long long)M ? k0 + 1ull : (unsigned long long)(M - 1);
    const double weight = h - fl;

    const GmScratch s = gm_carve(a->scratch);
    const int nb = (int)gm_blocks(M, GM_THREADS);
    if (hipMemsetAsync(a->scratch, 0, GM_HEAD_BYTES, stream) != hipSuccess) return DNSPLAT_ERR_LAUNCH;
    GmSearch q;
    q.ix = df_view(a->index, df_layout(a->N));
    q.M = M;
    q.src = a->src; q.src_normals = a->src_normals; q.tgt_normals = a->tgt_normals;
    q.threshold = a->threshold;
    q.dist2 = a->dist2; q.absdot = a->absdot; q.idx = a->idx;
    q.part = s.part;
    hipLaunchKernelGGL(gm_search_kernel, dim3((unsigned)nb), dim3(GM_THREADS), 0, stream, q);
    const unsigned hist_blocks = (unsigned)gm_blocks(M, GM_HSPAN);
    for (int round = 0; round < GM_ROUNDS; ++round) {
        hipLaunchKernelGGL(gm_hist_kernel, dim3(hist_blocks), dim3(GM_THREADS), 0, stream, round, M, (const unsigned long long *)a->dist2,
                           a->scratch);
        if (round < GM_ROUNDS - 1) hipLaunchKernelGGL(gm_select_kernel, dim3(1), dim3(GM_THREADS), 0, stream, round, k0, k1, a->scratch);
    }
    hipLaunchKernelGGL(gm_finish_kernel, dim3(1), dim3(GM_THREADS), 0, stream, M, nb, a->src_normals ? 1 : 0, weight, a->scratch, a->scalars,
                       a->counts);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_mesh_areas(int32_t V, const float *vertices, int32_t T, const int32_t *triangles, double *areas, float *face_normals,
                                  dnsplat_stream_t stream_)
{
    if (V < 1 || T < 1 || !vertices || !triangles || !areas || !face_normals) return DNSPLAT_ERR_INVALID_ARG;
    hipLaunchKernelGGL(gm_area_kernel, dim3((unsigned)gm_blocks(T, GM_THREADS)), dim3(GM_THREADS), 0, (hipStream_t)stream_, V, T, vertices,
                       triangles, areas, face_normals);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_mesh_sample(const dnsplat_mesh_sample_args *a, dnsplat_stream_t stream_)
{
    if (!a || a->S < 0 || a->V < 1 || a->T < 1 || !a->cdf || !a->vertices || !a->triangles || !a->face_normals) return DNSPLAT_ERR_INVALID_ARG;
    if (a->S > 0 && (!a->points || !a->normals || !a->faces)) return DNSPLAT_ERR_INVALID_ARG;
    if (a->S > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;
    if (a->S == 0) return DNSPLAT_OK;
    GmSample q;
    q.S = a->S;
    // the key of the draw: both halves of the seed through the hash, as pc_permute keys its rounds
    q.key = dns_mix32((uint32_t)a->seed ^ dns_mix32((uint32_t)(a->seed >> 32) + 0x9e3779b9u));
    q.T = a->T; q.V = a->V;
    q.cdf = a->cdf; q.vertices = a->vertices; q.face_normals = a->face_normals; q.triangles = a->triangles;
    q.points = a->points; q.normals = a->normals; q.faces = a->faces;
    hipLaunchKernelGGL(gm_sample_kernel, dim3((unsigned)gm_blocks(a->S, GM_THREADS)), dim3(GM_THREADS), 0, (hipStream_t)stream_, q);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
