// cloudfilter.hip — the two Open3D point-cloud filters the reference runs on the CPU between the clouds this project builds and their
// consumers: remove_statistical_outlier (the last step before the solver of all three point-cloud exporters, export_mesh.py:287-291,
// :487-491, :640) and voxel_down_sample (eval_pd.py:82 before the accuracy / completeness scores, export_mesh.py:284-285).  Both rules
// are stated in dnsplat.h (THIS PROJECT'S DEFINITION, PARITY UNPINNED AGAINST Open3D); torch_cloud_filter.py restates them on the CPU.
// Compiled with -ffp-contract=off like its siblings: every floating-point statement below is the IEEE operations it spells (the device's
// sqrt(double) is the correctly rounded one: equal to the hardware root of a CPU on 2^22 uniform doubles).
//
//   dnsplat_cloud_neighbor_mean   co_neighbor_kernel  one thread per point: df_search (density_common.h, untouched) against the index of
//                                                     the cloud itself, the square roots of the K lowest d^2 added in ascending rank, / K
//   dnsplat_cloud_outlier_stats   co_sum_kernel       fold 1 per workgroup: {sum of avg > 0, rows with avg >= 0}
//                                 co_fold_mean_kernel one workgroup: the partials in block_reduce.h's order -> n_valid, mean
//                                 co_dev_kernel       fold 2 per workgroup: sum of (avg - mean)^2 over avg > 0, mean read on the device
//                                 co_finish_kernel    one workgroup: std, threshold
//   dnsplat_cloud_outlier_count   co_count_kernel     kept rows per block of 256 (the flag rank of block_scan.h), threshold read on the device
//                                 co_scan_kernel      one workgroup: the exclusive scan of those counts; n_kept
//   dnsplat_cloud_outlier_emit    co_emit_kernel      ind[count of the block + rank in the block] = i: ascending
//   dnsplat_voxel_count           vx_init_kernel      the table empty (keys ~0, first INT32_MAX), counts = {0, 0}
//                                 vx_min_kernel       the minimum per axis per workgroup (exact in float), the non-finite check
//                                 vx_lo_kernel        one workgroup: lo[a] = min - voxel_size / 2 in double
//                                 vx_insert_kernel    one lane per point: its 63-bit voxel key into an open-addressing table of 2 N slots (a
//                                                     64-bit atomicCAS claims a slot, linear probing), atomicMin(first[slot], i)
//                                 vx_flag_kernel      the representatives (first[slot] == i) per block of 256
//                                 vx_scan_kernel      one workgroup: the scan of those counts; counts[0] = V
//                                 vx_assign_kernel    a representative's rank is its voxel's number: order of first appearance.  It zeroes
//                                                     the voxel's row of sums
//                                 vx_sum_kernel       one lane per point: voxel_of[i], and the point's fixed-point terms added to its voxel's
//                                                     row of int64 sums — once per voxel per wave where lanes share one (the peel of
//                                                     dns_hist_add), per lane otherwise
//   dnsplat_voxel_emit            vx_emit_kernel      each representative writes its voxel's row from the sums and its own cell
//
// WHY THE SUMS ARE PER VOXEL, NOT PER SLOT: a row of sums is 32 to 80 bytes; per slot of a table of 2 N that is 160 N bytes with both
// attributes, 320 MB at 2 M points.  Numbering the voxels first costs three short launches and leaves N rows, dense in voxel order.
//
// WHAT BOUNDS EVERY LOOP: a probe walks at most `cap` slots (the load never exceeds 0.5) and sets DNSPLAT_VOXEL_STATUS_INTERNAL if it
// runs out, which cannot happen on a correct build; the peel retires at most VX_PEEL voxels of a wave; df_search ends when its cube
// covers the grid.  Every write is behind an index check against N, cap, V <= N or the caller's capacity.
//
// Equal inputs give equal bytes: avg is one thread's IEEE operations in one order, the folds are block_reduce.h's, the kept rows are a
// scan; a voxel's representative is a minimum, its sums are integers, its number is a scan.  No floating-point atomic, no inline
// assembly, nothing allocated, nothing read on the host.

#include <limits.h>

#include "block_reduce.h"
#include "density_common.h"

namespace {

constexpr int CF_THREADS = 256;
constexpr int CF_WAVES = CF_THREADS / DNS_WAVE;
constexpr int CF_SCAN_PER = 4;
constexpr int CF_MIN_BLOCKS = 256;

inline int cf_blocks(long long n) { return (int)((n + CF_THREADS - 1) / CF_THREADS); }

// ---- statistical outlier removal ------------------------------------------------------------------------------------------------------

struct CoStats {                                          // the 64-byte record dnsplat.h states
    double mean, std, threshold, sum;
    long long n_valid, n_kept, pad[2];
};
static_assert(sizeof(CoStats) == DNSPLAT_CLOUD_OUTLIER_STATS_BYTES, "the record is 64 bytes");

struct CoPartial {                                        // 16 bytes
    double sum;
    long long n;
    static __device__ CoPartial identity() { return CoPartial{0.0, 0}; }
    __device__ void join(const CoPartial &o) { sum = sum + o.sum; n += o.n; }
};

// scratch: partials of fold 1 [nb], partials of fold 2 [nb], kept per block int32 [nb]
struct CoScratch {
    CoPartial *part1, *part2;
    int32_t *bcount;
};

size_t co_bytes(int N) { return (size_t)cf_blocks(N) * (2 * sizeof(CoPartial) + sizeof(int32_t)); }

CoScratch co_carve(void *scratch, int N)
{
    CoScratch s;
    const int nb = cf_blocks(N);
    s.part1 = (CoPartial *)scratch;
    s.part2 = s.part1 + nb;
    s.bcount = (int32_t *)(s.part2 + nb);
    return s;
}

int co_km(int K) { return K <= 4 ? 4 : (K <= 8 ? 8 : (K <= 20 ? 20 : DNSPLAT_KNN_MAX_K)); }

template <int KM>
__global__ __launch_bounds__(CF_THREADS) void co_neighbor_kernel(DfIndex ix, int N, const float *__restrict__ points, int K, double *__restrict__ avg)
{
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    if (i >= N) return;
    DfList<KM> L;
    const bool ok = df_search(ix, points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2], K, L);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < KM; ++j)
        if (j < K) s = s + sqrt(L.d[j]);                                          // ascending rank; the first term is the point itself, 0
    avg[i] = ok ? s / (double)K : -1.0;
}

__global__ __launch_bounds__(CF_THREADS) void co_sum_kernel(int N, const double *__restrict__ avg, CoPartial *__restrict__ part)
{
    __shared__ CoPartial red[CF_WAVES];
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    CoPartial v = CoPartial::identity();
    if (i < N) {
        const double a = avg[i];
        if (a > 0.0) v.sum = a;
        if (a >= 0.0) v.n = 1;
    }
    dns_block_join<CF_THREADS>(v, red);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

__global__ __launch_bounds__(CF_THREADS) void co_fold_mean_kernel(int nb, const CoPartial *__restrict__ part, CoStats *__restrict__ stats)
{
    __shared__ CoPartial red[CF_WAVES];
    CoPartial v;
    dns_fold_partials<CF_THREADS>(part, nb, v, red);
    if (threadIdx.x == 0) {
        stats->sum = v.sum;
        stats->n_valid = v.n;
        stats->mean = v.n > 0 ? v.sum / (double)v.n : 0.0;
    }
}

__global__ __launch_bounds__(CF_THREADS) void co_dev_kernel(int N, const double *__restrict__ avg, const CoStats *__restrict__ stats,
                                                           CoPartial *__restrict__ part)
{
    __shared__ CoPartial red[CF_WAVES];
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    const double mean = stats->mean;
    CoPartial v = CoPartial::identity();
    if (i < N) {
        const double a = avg[i];
        if (a > 0.0) {
            const double d = a - mean;
            v.sum = d * d;
        }
    }
    dns_block_join<CF_THREADS>(v, red);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

__global__ __launch_bounds__(CF_THREADS) void co_finish_kernel(int nb, const CoPartial *__restrict__ part, double std_ratio, CoStats *__restrict__ stats)
{
    __shared__ CoPartial red[CF_WAVES];
    CoPartial v;
    dns_fold_partials<CF_THREADS>(part, nb, v, red);
    if (threadIdx.x == 0) {
        const long long n = stats->n_valid;
        const double sd = n > 1 ? sqrt(v.sum / (double)(n - 1)) : 0.0;
        stats->std = sd;
        stats->threshold = n > 1 ? stats->mean + std_ratio * sd : 0.0;             // with n_valid <= 1 nothing lies below 0
        stats->n_kept = 0;
        stats->pad[0] = stats->pad[1] = 0;
    }
}

__device__ __forceinline__ bool co_kept(double a, double threshold) { return a > 0.0 && a < threshold; }

__global__ __launch_bounds__(CF_THREADS) void co_count_kernel(int N, const double *__restrict__ avg, const CoStats *__restrict__ stats,
                                                             int32_t *__restrict__ bcount)
{
    __shared__ int wave_tot[CF_WAVES];
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    const double threshold = stats->threshold;
    int total;
    dns_block_rank<CF_THREADS>(i < N && co_kept(avg[i < N ? i : 0], threshold), wave_tot, total);
    if (threadIdx.x == 0) bcount[blockIdx.x] = total;
}

__global__ __launch_bounds__(CF_THREADS) void co_scan_kernel(int nb, int32_t *__restrict__ bcount, CoStats *__restrict__ stats)
{
    const int n = dns_scan_in_place<CF_THREADS, CF_SCAN_PER>(nb, bcount);
    if (threadIdx.x == 0) stats->n_kept = n;
}

__global__ __launch_bounds__(CF_THREADS) void co_emit_kernel(int N, const double *__restrict__ avg, const CoStats *__restrict__ stats,
                                                            const int32_t *__restrict__ bcount, long long capacity, int64_t *__restrict__ ind)
{
    __shared__ int wave_tot[CF_WAVES];
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    const double threshold = stats->threshold;
    const bool kept = i < N && co_kept(avg[i < N ? i : 0], threshold);
    int total;
    const long long at = (long long)bcount[blockIdx.x] + dns_block_rank<CF_THREADS>(kept, wave_tot, total);
    if (kept && at < capacity) ind[at] = i;
}

bool co_args_ok(const dnsplat_cloud_outlier_args *a)
{
    return a && a->N >= 1 && a->avg && a->stats && a->scratch;
}

bool co_scratch_ok(const dnsplat_cloud_outlier_args *a)
{
    return a->scratch_bytes >= co_bytes(a->N) && (size_t)a->scratch % sizeof(double) == 0;
}

// ---- voxel down-sampling --------------------------------------------------------------------------------------------------------------

constexpr unsigned long long VX_EMPTY = ~0ull;
constexpr int VX_MAX_N = 0x7fffffff / 2;                  // the table has 2 N slots, indexed by int32
constexpr int VX_PEEL = 4;
constexpr double VX_CELLS = 2097152.0;                    // 2^21 per axis: three indices in one 63-bit key
constexpr double VX_POS_ONE = 2147483648.0;               // 2^31: a position inside its voxel
constexpr double VX_ATTR_ONE = 1073741824.0;              // 2^30: a normal or a colour component

struct VxMin {                                            // 12 bytes
    float m[3];
    static __device__ VxMin identity() { return VxMin{{INFINITY, INFINITY, INFINITY}}; }
    __device__ void join(const VxMin &o)
    {
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] = fminf(m[a], o.m[a]);
    }
};

// scratch: lo double [4], keys uint64 [cap], sums int64 [N][row], first int32 [cap], slot_of int32 [N], reps per block int32 [nb],
//          partial minima [CF_MIN_BLOCKS]; cap = 2 N, row = 1 + 3 (1 + attributes)
struct VxScratch {
    double *lo;
    unsigned long long *keys, *sums;
    int32_t *first, *slot_of, *bcount;
    VxMin *part;
    int cap;
};

__host__ __device__ constexpr int vx_row(int n_attr) { return 1 + 3 * (1 + n_attr); }

size_t vx_bytes(int N, int n_attr)
{
    const size_t cap = 2 * (size_t)N;
    return 4 * sizeof(double) + cap * sizeof(unsigned long long) + (size_t)N * vx_row(n_attr) * sizeof(unsigned long long) +
           (cap + (size_t)N + cf_blocks(N)) * sizeof(int32_t) + CF_MIN_BLOCKS * sizeof(VxMin);
}

VxScratch vx_carve(void *scratch, int N, int n_attr)
{
    VxScratch s;
    s.cap = 2 * N;
    s.lo = (double *)scratch;
    s.keys = (unsigned long long *)(s.lo + 4);
    s.sums = s.keys + s.cap;
    s.first = (int32_t *)(s.sums + (size_t)N * vx_row(n_attr));
    s.slot_of = s.first + s.cap;
    s.bcount = s.slot_of + N;
    s.part = (VxMin *)(s.bcount + cf_blocks(N));
    return s;
}

__device__ __forceinline__ bool vx_finite(float v) { return fabsf(v) < INFINITY; }

// The voxel of p and its fixed-point position inside it; false beyond the key's 2^21 cells per axis (and for a nan).
__device__ __forceinline__ bool vx_cell(const float *__restrict__ p, const double *__restrict__ lo, double voxel, int idx[3], long long q[3])
{
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double ref = ((double)p[a] - lo[a]) / voxel;
        const bool in = ref >= 0.0 && ref < VX_CELLS;
        const double f = floor(in ? ref : 0.0);
        idx[a] = (int)f;
        q[a] = llrint(((in ? ref : 0.0) - f) * VX_POS_ONE);
        ok = ok && in;
    }
    return ok;
}

__global__ __launch_bounds__(CF_THREADS) void vx_init_kernel(VxScratch s, int64_t *__restrict__ counts)
{
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    if (i < s.cap) { s.keys[i] = VX_EMPTY; s.first[i] = INT_MAX; }
    if (i == 0) { counts[0] = 0; counts[1] = 0; }
}

__global__ __launch_bounds__(CF_THREADS) void vx_min_kernel(int N, const float *__restrict__ points, VxScratch s, int64_t *__restrict__ counts)
{
    __shared__ VxMin red[CF_WAVES];
    VxMin v = VxMin::identity();
    bool bad = false;
    for (long long i = (long long)blockIdx.x * CF_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * CF_THREADS) {
        VxMin p;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p.m[a] = points[i * 3 + a];
            bad = bad || !vx_finite(p.m[a]);
        }
        v.join(p);
    }
    if (bad) atomicOr((unsigned long long *)&counts[1], (unsigned long long)DNSPLAT_VOXEL_STATUS_NONFINITE);
    dns_block_join<CF_THREADS>(v, red);
    if (threadIdx.x == 0) s.part[blockIdx.x] = v;
}

__global__ __launch_bounds__(CF_THREADS) void vx_lo_kernel(int n_part, double voxel, VxScratch s)
{
    __shared__ VxMin red[CF_WAVES];
    VxMin v;
    dns_fold_partials<CF_THREADS>(s.part, n_part, v, red);
    if (threadIdx.x < 3) s.lo[threadIdx.x] = (double)v.m[threadIdx.x] - voxel * 0.5;
    if (threadIdx.x == 3) s.lo[3] = 0.0;
}

__global__ __launch_bounds__(CF_THREADS) void vx_insert_kernel(int N, const float *__restrict__ points, double voxel, VxScratch s,
                                                              int64_t *__restrict__ counts)
{
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    if (i >= N) return;
    const float p[3] = {points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]};
    s.slot_of[i] = -1;
    if (!vx_finite(p[0]) || !vx_finite(p[1]) || !vx_finite(p[2])) return;        // vx_min_kernel has set the status
    int idx[3];
    long long q[3];
    if (!vx_cell(p, s.lo, voxel, idx, q)) {
        atomicOr((unsigned long long *)&counts[1], (unsigned long long)DNSPLAT_VOXEL_STATUS_EXTENT);
        return;
    }
    const unsigned long long key = (unsigned long long)idx[0] | ((unsigned long long)idx[1] << 21) | ((unsigned long long)idx[2] << 42);
    const unsigned h = dns_mix32((unsigned)key ^ dns_mix32((unsigned)(key >> 32) + 0x9e3779b9u));
    int slot = (int)(((unsigned long long)h * (unsigned)s.cap) >> 32);           // in [0, cap)
    for (int probe = 0; probe < s.cap; ++probe) {                                 // the bound: every slot once
        const unsigned long long old = atomicCAS(&s.keys[slot], VX_EMPTY, key);
        if (old == VX_EMPTY || old == key) {
            atomicMin(&s.first[slot], i);
            s.slot_of[i] = slot;
            return;
        }
        slot = slot + 1 == s.cap ? 0 : slot + 1;
    }
    atomicOr((unsigned long long *)&counts[1], (unsigned long long)DNSPLAT_VOXEL_STATUS_INTERNAL);
}

// the table is the previous launch's: plain loads
__device__ __forceinline__ bool vx_is_rep(int i, int N, const VxScratch &s)
{
    if (i >= N) return false;
    const int slot = s.slot_of[i];
    return (unsigned)slot < (unsigned)s.cap && s.first[slot] == i;
}

__global__ __launch_bounds__(CF_THREADS) void vx_flag_kernel(int N, VxScratch s)
{
    __shared__ int wave_tot[CF_WAVES];
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    int total;
    dns_block_rank<CF_THREADS>(vx_is_rep(i, N, s), wave_tot, total);
    if (threadIdx.x == 0) s.bcount[blockIdx.x] = total;
}

__global__ __launch_bounds__(CF_THREADS) void vx_scan_kernel(int nb, VxScratch s, int64_t *__restrict__ counts)
{
    const int n = dns_scan_in_place<CF_THREADS, CF_SCAN_PER>(nb, s.bcount);
    if (threadIdx.x == 0) counts[0] = n;
}

__global__ __launch_bounds__(CF_THREADS) void vx_assign_kernel(int N, int row, VxScratch s, int32_t *__restrict__ voxel_of)
{
    __shared__ int wave_tot[CF_WAVES];
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    const bool rep = vx_is_rep(i, N, s);
    int total;
    const int v = s.bcount[blockIdx.x] + dns_block_rank<CF_THREADS>(rep, wave_tot, total);
    if (i < N && !rep) voxel_of[i] = -1;                                          // until vx_sum_kernel; stays -1 for a row without a voxel
    if (!rep || v >= N) return;                                                   // v < V <= N
    voxel_of[i] = v;
    for (int j = 0; j < row; ++j) s.sums[(size_t)v * row + j] = 0ull;
}

__device__ __forceinline__ long long vx_wave_sum(long long v)
{
#pragma unroll
    for (int off = DNS_WAVE / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, DNS_WAVE);
    return v;
}

// ROW int64 terms of every active lane into row v of sums.  All 64 lanes of the wave call this together.  Lanes of one wave that share a
// voxel would serialise on its words (a voxel larger than the cloud is ALL lanes): VX_PEEL times the first lane's voxel is summed
// within the wave and added once; a first lane alone in its voxel ends the peel, and what is left adds per lane.
template <int ROW>
__device__ __forceinline__ void vx_add(unsigned long long *__restrict__ sums, int v, bool active, const long long (&val)[ROW])
{
    uint64_t todo = dns_ballot(active);
    const int lane = threadIdx.x & (DNS_WAVE - 1);
    for (int k = 0; k < VX_PEEL && todo; ++k) {                                   // wave-uniform: todo lives in scalar registers
        const int leader = __builtin_ctzll(todo);
        const int v0 = __builtin_amdgcn_readlane(v, leader);
        const uint64_t same = dns_ballot(active && v == v0) & todo;
        if (__builtin_popcountll(same) < 2) break;
        const bool mine = (same >> lane) & 1ull;
#pragma unroll
        for (int j = 0; j < ROW; ++j) {
            const long long sum = vx_wave_sum(mine ? val[j] : 0ll);
            if (lane == leader) atomicAdd(&sums[(size_t)v0 * ROW + j], (unsigned long long)sum);
        }
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) {
#pragma unroll
        for (int j = 0; j < ROW; ++j) atomicAdd(&sums[(size_t)v * ROW + j], (unsigned long long)val[j]);
    }
}

template <int NATTR>
__global__ __launch_bounds__(CF_THREADS) void vx_sum_kernel(int N, const float *__restrict__ points, const float *__restrict__ attr0,
                                                           const float *__restrict__ attr1, double voxel, VxScratch s,
                                                           int32_t *__restrict__ voxel_of, int64_t *__restrict__ counts)
{
    constexpr int ROW = vx_row(NATTR);
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    long long val[ROW];
#pragma unroll
    for (int j = 0; j < ROW; ++j) val[j] = 0;
    int v = -1;
    if (i < N) {
        const int slot = s.slot_of[i];
        const int r = (unsigned)slot < (unsigned)s.cap ? s.first[slot] : -1;      // the voxel's representative
        if ((unsigned)r < (unsigned)N) {
            v = r == i ? voxel_of[i] : voxel_of[r];                               // a representative's row is vx_assign_kernel's, final
            if (r != i) voxel_of[i] = v;                                          // nobody reads the row of a point that represents nothing
        }
        if ((unsigned)v >= (unsigned)N) v = -1;
    }
    if (v >= 0) {
        const float p[3] = {points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]};
        int idx[3];
        long long q[3];
        vx_cell(p, s.lo, voxel, idx, q);
        val[0] = 1;
        val[1] = q[0]; val[2] = q[1]; val[3] = q[2];
        bool bad = false;
#pragma unroll
        for (int t = 0; t < NATTR; ++t) {
            const float *src = t == 0 ? attr0 : attr1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double c = (double)src[(size_t)i * 3 + a];
                const bool in = fabs(c) <= 2.0;                                   // false for a nan
                bad = bad || !in;
                val[4 + 3 * t + a] = llrint((in ? c : 0.0) * VX_ATTR_ONE);
            }
        }
        if (bad) atomicOr((unsigned long long *)&counts[1], (unsigned long long)DNSPLAT_VOXEL_STATUS_ATTRIBUTE);
    }
    vx_add<ROW>(s.sums, v, v >= 0, val);
}

template <int NATTR>
__global__ __launch_bounds__(CF_THREADS) void vx_emit_kernel(int N, const float *__restrict__ points, double voxel, VxScratch s,
                                                            const int32_t *__restrict__ voxel_of, long long cap_v, double *__restrict__ out_points,
                                                            double *__restrict__ out0, double *__restrict__ out1, int32_t *__restrict__ out_counts)
{
    constexpr int ROW = vx_row(NATTR);
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    if (!vx_is_rep(i, N, s)) return;
    const int v = voxel_of[i];
    if ((unsigned)v >= (unsigned)N || v >= cap_v) return;
    const float p[3] = {points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]};
    int idx[3];
    long long q[3];
    vx_cell(p, s.lo, voxel, idx, q);
    const long long *row = (const long long *)s.sums + (size_t)v * ROW;
    const double n = (double)row[0];
    if (out_counts) out_counts[v] = (int32_t)row[0];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double mean = (double)row[1 + a] / n;
        out_points[(size_t)v * 3 + a] = (s.lo[a] + (double)idx[a] * voxel) + (voxel * mean) / VX_POS_ONE;
    }
#pragma unroll
    for (int t = 0; t < NATTR; ++t) {
        double *out = t == 0 ? out0 : out1;
#pragma unroll
        for (int a = 0; a < 3; ++a) out[(size_t)v * 3 + a] = ((double)row[4 + 3 * t + a] / n) / VX_ATTR_ONE;
    }
}

int vx_attrs(const dnsplat_voxel_args *a) { return (a->normals ? 1 : 0) + (a->colors ? 1 : 0); }

int vx_check(const dnsplat_voxel_args *a)
{
    if (!a || a->N < 1 || !a->points || !a->scratch || !a->counts || !a->voxel_of || !(a->voxel_size > 0.0) || !(a->voxel_size < (double)INFINITY))
        return DNSPLAT_ERR_INVALID_ARG;
    if (a->N > VX_MAX_N) return DNSPLAT_ERR_UNSUPPORTED;
    if (a->scratch_bytes < vx_bytes(a->N, vx_attrs(a)) || (size_t)a->scratch % sizeof(double)) return DNSPLAT_ERR_WORKSPACE;
    return DNSPLAT_OK;
}

}  // namespace

extern "C" size_t dnsplat_cloud_outlier_scratch_bytes(int32_t N) { return N < 1 ? 0 : co_bytes(N); }

extern "C" int dnsplat_cloud_neighbor_mean(const dnsplat_cloud_outlier_args *a, dnsplat_stream_t stream_)
{
    if (!a || a->N < 1 || !a->points || !a->index || !a->avg || a->nb_neighbors < 1) return DNSPLAT_ERR_INVALID_ARG;   // it needs no scratch
    if (a->nb_neighbors > DNSPLAT_KNN_MAX_K) return DNSPLAT_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const int N = a->N, K = a->nb_neighbors < N ? a->nb_neighbors : N;
    const DfIndex ix = df_view(a->index, df_layout(N));
    const dim3 grid((unsigned)cf_blocks(N)), block(CF_THREADS);
    switch (co_km(K)) {
    case 4: hipLaunchKernelGGL((co_neighbor_kernel<4>), grid, block, 0, stream, ix, N, a->points, K, a->avg); break;
    case 8: hipLaunchKernelGGL((co_neighbor_kernel<8>), grid, block, 0, stream, ix, N, a->points, K, a->avg); break;
    case 20: hipLaunchKernelGGL((co_neighbor_kernel<20>), grid, block, 0, stream, ix, N, a->points, K, a->avg); break;
    default: hipLaunchKernelGGL((co_neighbor_kernel<DNSPLAT_KNN_MAX_K>), grid, block, 0, stream, ix, N, a->points, K, a->avg); break;
    }
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_cloud_outlier_stats(const dnsplat_cloud_outlier_args *a, dnsplat_stream_t stream_)
{
    if (!co_args_ok(a) || !(a->std_ratio == a->std_ratio)) return DNSPLAT_ERR_INVALID_ARG;
    if (!co_scratch_ok(a)) return DNSPLAT_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const CoScratch s = co_carve(a->scratch, a->N);
    const int N = a->N, nb = cf_blocks(N);
    CoStats *stats = (CoStats *)a->stats;
    const dim3 grid((unsigned)nb), block(CF_THREADS);
    hipLaunchKernelGGL(co_sum_kernel, grid, block, 0, stream, N, (const double *)a->avg, s.part1);
    hipLaunchKernelGGL(co_fold_mean_kernel, dim3(1), block, 0, stream, nb, (const CoPartial *)s.part1, stats);
    hipLaunchKernelGGL(co_dev_kernel, grid, block, 0, stream, N, (const double *)a->avg, (const CoStats *)stats, s.part2);
    hipLaunchKernelGGL(co_finish_kernel, dim3(1), block, 0, stream, nb, (const CoPartial *)s.part2, a->std_ratio, stats);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_cloud_outlier_count(const dnsplat_cloud_outlier_args *a, dnsplat_stream_t stream_)
{
    if (!co_args_ok(a)) return DNSPLAT_ERR_INVALID_ARG;
    if (!co_scratch_ok(a)) return DNSPLAT_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const CoScratch s = co_carve(a->scratch, a->N);
    const int N = a->N, nb = cf_blocks(N);
    CoStats *stats = (CoStats *)a->stats;
    hipLaunchKernelGGL(co_count_kernel, dim3((unsigned)nb), dim3(CF_THREADS), 0, stream, N, (const double *)a->avg, (const CoStats *)stats, s.bcount);
    hipLaunchKernelGGL(co_scan_kernel, dim3(1), dim3(CF_THREADS), 0, stream, nb, s.bcount, stats);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_cloud_outlier_emit(const dnsplat_cloud_outlier_args *a, dnsplat_stream_t stream_)
{
    if (!co_args_ok(a) || a->capacity < 0 || (a->capacity > 0 && !a->ind)) return DNSPLAT_ERR_INVALID_ARG;
    if (!co_scratch_ok(a)) return DNSPLAT_ERR_WORKSPACE;
    if (a->capacity == 0) return DNSPLAT_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const CoScratch s = co_carve(a->scratch, a->N);
    hipLaunchKernelGGL(co_emit_kernel, dim3((unsigned)cf_blocks(a->N)), dim3(CF_THREADS), 0, stream, a->N, (const double *)a->avg,
                       (const CoStats *)a->stats, (const int32_t *)s.bcount, (long long)a->capacity, a->ind);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" size_t dnsplat_voxel_scratch_bytes(int32_t N, int32_t n_attributes)
{
    if (N < 1 || N > VX_MAX_N || n_attributes < 0 || n_attributes > 2) return 0;
    return vx_bytes(N, n_attributes);
}

extern "C" int dnsplat_voxel_count(const dnsplat_voxel_args *a, dnsplat_stream_t stream_)
{
    const int rc = vx_check(a);
    if (rc != DNSPLAT_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int N = a->N, nb = cf_blocks(N), n_attr = vx_attrs(a), mb = nb < CF_MIN_BLOCKS ? nb : CF_MIN_BLOCKS;
    const VxScratch s = vx_carve(a->scratch, N, n_attr);
    const float *attr0 = a->normals ? a->normals : a->colors, *attr1 = a->normals ? a->colors : nullptr;
    const double voxel = a->voxel_size;
    const dim3 grid((unsigned)nb), block(CF_THREADS);
    hipLaunchKernelGGL(vx_init_kernel, dim3((unsigned)cf_blocks(s.cap)), block, 0, stream, s, a->counts);
    hipLaunchKernelGGL(vx_min_kernel, dim3((unsigned)mb), block, 0, stream, N, a->points, s, a->counts);
    hipLaunchKernelGGL(vx_lo_kernel, dim3(1), block, 0, stream, mb, voxel, s);
    hipLaunchKernelGGL(vx_insert_kernel, grid, block, 0, stream, N, a->points, voxel, s, a->counts);
    hipLaunchKernelGGL(vx_flag_kernel, grid, block, 0, stream, N, s);
    hipLaunchKernelGGL(vx_scan_kernel, dim3(1), block, 0, stream, nb, s, a->counts);
    hipLaunchKernelGGL(vx_assign_kernel, grid, block, 0, stream, N, vx_row(n_attr), s, a->voxel_of);
    switch (n_attr) {
    case 0: hipLaunchKernelGGL((vx_sum_kernel<0>), grid, block, 0, stream, N, a->points, attr0, attr1, voxel, s, a->voxel_of, a->counts); break;
    case 1: hipLaunchKernelGGL((vx_sum_kernel<1>), grid, block, 0, stream, N, a->points, attr0, attr1, voxel, s, a->voxel_of, a->counts); break;
    default: hipLaunchKernelGGL((vx_sum_kernel<2>), grid, block, 0, stream, N, a->points, attr0, attr1, voxel, s, a->voxel_of, a->counts); break;
    }
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_voxel_emit(const dnsplat_voxel_args *a, dnsplat_stream_t stream_)
{
    const int rc = vx_check(a);
    if (rc != DNSPLAT_OK) return rc;
    if (a->cap_v < 0) return DNSPLAT_ERR_INVALID_ARG;
    if (a->cap_v > 0 && (!a->out_points || (a->normals && !a->out_normals) || (a->colors && !a->out_colors))) return DNSPLAT_ERR_INVALID_ARG;
    if (a->cap_v == 0) return DNSPLAT_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const int N = a->N, n_attr = vx_attrs(a);
    const VxScratch s = vx_carve(a->scratch, N, n_attr);
    double *out0 = a->normals ? a->out_normals : a->out_colors, *out1 = a->normals ? a->out_colors : nullptr;
    const dim3 grid((unsigned)cf_blocks(N)), block(CF_THREADS);
    const int32_t *voxel_of = a->voxel_of;
    switch (n_attr) {
    case 0: hipLaunchKernelGGL((vx_emit_kernel<0>), grid, block, 0, stream, N, a->points, a->voxel_size, s, voxel_of, (long long)a->cap_v,
                               a->out_points, out0, out1, a->out_counts); break;
    case 1: hipLaunchKernelGGL((vx_emit_kernel<1>), grid, block, 0, stream, N, a->points, a->voxel_size, s, voxel_of, (long long)a->cap_v,
                               a->out_points, out0, out1, a->out_counts); break;
    default: hipLaunchKernelGGL((vx_emit_kernel<2>), grid, block, 0, stream, N, a->points, a->voxel_size, s, voxel_of, (long long)a->cap_v,
                                a->out_points, out0, out1, a->out_counts); break;
    }
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
