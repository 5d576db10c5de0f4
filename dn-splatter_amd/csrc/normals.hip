// normals.hip — Open3D's PointCloud.estimate_normals, the call the reference's dataparsers seed their Gaussians' normals with
// (_load_points3D_normals: KDTreeSearchParamHybrid(0.1, 30)) and its depth scripts turn a sensor frame into normals with
// (depth_to_normal.py:150-213: KDTreeSearchParamKNN(200) over every pixel of the frame).  The rule is stated in dnsplat.h (THIS PROJECT'S
// DEFINITION, PARITY UNPINNED AGAINST Open3D); torch_normals.py restates it on the CPU.  Compiled with -ffp-contract=off: every
// floating-point statement below is the IEEE operations it spells.
//
//   dnsplat_cloud_normals   nm_kernel<KP>   ONE launch, one wave per query point (a workgroup IS one wave, so __syncthreads() is the wave's
//                                           own barrier and no wave waits for another's search):
//     search   the cube rings of df_search (density_common.h, untouched) around the query's cell, with df_search's own statements for the
//              outside-the-cube bound.  A row of a cube face is one run of `sorted`: the 64 lanes read it as coalesced float4s, compute
//              d^2 as df_search does, and those whose (d^2, index) beats the threshold are appended by ballot and prefix to the wave's
//              LDS buffer of CAP = 2 KP entries (KP = knn rounded up to a power of two, at least 64: a batch of 64 always fits behind K).
//     select   when a batch would not fit, and at the end of a ring that left K or more entries: a bitonic sort of the buffer by
//              (d^2, index), the K lowest stay, the K-th becomes the threshold.  The threshold starts at (radius^2, below every index), so
//              the hybrid search's strict d^2 < radius^2 is the same comparison.
//     end      the K-th d^2 below the bound of what lies outside the cube (df_search's rule), or that bound not below radius^2 (nothing
//              farther can be kept), or the cube covers the grid.
//     moments  lane l takes ranks l, l + 64, l + 128, l + 192 in ascending order, then the lanes are added by the xor tree 32, 16, .. 1
//              (a + b is commutative: every lane holds the same bits): the mean, then the six sums about it.
//     normal   nm_normal / nm_orient (normals_solve.h), computed alike by every lane; lane 0 writes the row.
//
// WHAT BOUNDS EVERY LOOP: the rings end when the cube covers the grid, at most DNSPLAT_KNN_MAX_GRID of them
// (DNSPLAT_NORMALS_STATUS_INTERNAL if that ran out, which cannot happen on a correct build); a row is read once; the sort is log^2 of the
// buffer; the sweeps are NM_SWEEPS.  Every LDS write is below CAP (count + batch <= CAP is tested before it), every global write is
// behind q < N, j < knn.  `search` is two integer maxima for the tests and the timing tool (the widest ring, the most selections of a query).
//
// Equal inputs give equal bytes: the neighbour set is canonical, the moments are one fixed tree, there is no floating-point atomic and
// no inline code of another language.

#include <limits.h>

#include "density_common.h"
#include "normals_solve.h"

namespace {

constexpr int NM_THREADS = DNS_WAVE;                      // a workgroup is one wave
constexpr int NM_MIN_KP = DNS_WAVE;                       // K + a batch of 64 <= 2 KP
constexpr int NM_LANE_TERMS = DNSPLAT_NORMALS_MAX_K / DNS_WAVE;
constexpr int NM_MAX_BLOCKS = 1 << 20;                    // queries beyond that stride the grid
static_assert(DNSPLAT_NORMALS_MAX_K == 4 * NM_MIN_KP, "three buffer sizes: 64, 128, 256");
constexpr size_t NM_SCRATCH_BYTES = 16;                   // int32 [4]: the widest ring, the most selections of one query, 0, 0

template <int KP>
struct NmBuf {                                            // 12 bytes per entry: 6 KiB at KP = 256
    double d[2 * KP];
    int i[2 * KP];
};

struct NmArgs {
    DfIndex ix;
    int N, K, knn, orient;
    const float *points;
    double r2, toward[3];
    double *normals, *cov;
    int32_t *nbr, *count, *status, *search;
};

__device__ __forceinline__ double nm_wave_sum(double v)
{
#pragma unroll
    for (int off = DNS_WAVE / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, DNS_WAVE);
    return v;
}

// the buffer's first `count` entries ascending by (d^2, index); entries up to the next power of two are padded behind them
template <int KP>
__device__ __forceinline__ void nm_sort(NmBuf<KP> &b, int count, int lane)
{
    int n = DNS_WAVE;
    while (n < count) n <<= 1;                                                    // count <= 2 KP, a power of two
    for (int t = count + lane; t < n; t += DNS_WAVE) { b.d[t] = INFINITY; b.i[t] = INT_MAX; }
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < n / 2; t += DNS_WAVE) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const double dl = b.d[lo], dh = b.d[hi];
                const int il = b.i[lo], ih = b.i[hi];
                const bool up = (lo & k) == 0;
                if (df_less(dh, ih, dl, il) == up) { b.d[lo] = dh; b.i[lo] = ih; b.d[hi] = dl; b.i[hi] = il; }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ void nm_note_max(int32_t *word, int v)
{
    if (v > __atomic_load_n(word, __ATOMIC_RELAXED)) atomicMax(word, v);          // monotone: a stale read only costs an atomic
}

template <int KP>
__global__ __launch_bounds__(NM_THREADS) void nm_kernel(NmArgs a)
{
    constexpr int CAP = 2 * KP;
    __shared__ NmBuf<KP> buf;
    const int lane = threadIdx.x, K = a.K;
    const DfIndex &ix = a.ix;
    const DfHeader h = *ix.header;
    for (int q = blockIdx.x; q < a.N; q += gridDim.x) {
        const float qf[3] = {a.points[(size_t)q * 3], a.points[(size_t)q * 3 + 1], a.points[(size_t)q * 3 + 2]};
        const double qd[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
        int count = 0, selections = 0, ring = 0;
        if (fabsf(qf[0]) < INFINITY && fabsf(qf[1]) < INFINITY && fabsf(qf[2]) < INFINITY) {
            double lo[3], cell_w[3], out2 = 0.0, out[3];
            int c[3], g[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {                                      // df_search's statements
                lo[ax] = (double)h.lo[ax];
                g[ax] = h.g[ax];
                c[ax] = df_axis_cell(qf[ax], h.lo[ax], h.inv_h[ax], g[ax]);
                cell_w[ax] = g[ax] > 1 ? 1.0 / (double)h.inv_h[ax] : 0.0;
                out[ax] = fmax(fmax(lo[ax] - qd[ax], qd[ax] - (double)h.hi[ax]), 0.0);
                out2 += out[ax] * out[ax];
            }
            double thr_d = a.r2;                                                  // accept iff (d2, id) < (thr_d, thr_i): at first d2 < radius^2
            int thr_i = INT_MIN;
            bool dirty = false, full = false, ended = false;
            for (int r = 0; r <= DNSPLAT_KNN_MAX_GRID; ++r) {
                ring = r;
                const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g[2] - 1);
                const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g[1] - 1);
                const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g[0] - 1);
                for (int zz = z0; zz <= z1; ++zz) {
                    for (int yy = y0; yy <= y1; ++yy) {
                        const bool face = zz == c[2] - r || zz == c[2] + r || yy == c[1] - r || yy == c[1] + r;
                        const long long row = ((long long)zz * ix.G + yy) * ix.G;
                        for (int seg = 0; seg < (face ? 1 : 2); ++seg) {
                            const int xa = face ? x0 : (seg == 0 ? c[0] - r : c[0] + r), xb = face ? x1 : xa;
                            if (xa < 0 || xb > g[0] - 1) continue;
                            const int s = ix.cell_start[row + xa], e = ix.cell_start[row + xb + 1];
                            for (int base = s; base < e; base += DNS_WAVE) {
                                const int p = base + lane;
                                double d2 = 0.0;
                                int id = 0;
                                bool acc = false;
                                if (p < e) {
                                    const float4 v = ix.sorted[p];
                                    const double dx = qd[0] - (double)v.x, dy = qd[1] - (double)v.y, dz = qd[2] - (double)v.z;
                                    d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                                    id = __float_as_int(v.w);
                                    acc = df_less(d2, id, thr_d, thr_i);                  // false for a nan
                                }
                                uint64_t mask = dns_ballot(acc);
                                int m = __builtin_popcountll(mask);
                                if (m == 0) continue;
                                if (count + m > CAP) {                                    // the batch would not fit: keep the K lowest
                                    nm_sort(buf, count, lane);
                                    count = min(count, K);
                                    full = count >= K;
                                    if (full) { thr_d = buf.d[K - 1]; thr_i = buf.i[K - 1]; }
                                    ++selections;
                                    dirty = false;
                                    acc = acc && df_less(d2, id, thr_d, thr_i);
                                    mask = dns_ballot(acc);
                                    m = __builtin_popcountll(mask);
                                }
                                const int at = count + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
                                if (acc && at < CAP) { buf.d[at] = d2; buf.i[at] = id; }
                                count += m;
                                dirty = dirty || m > 0;
                            }
                        }
                    }
                }
                if (dirty && count >= K) {
                    nm_sort(buf, count, lane);
                    count = K;
                    full = true;
                    thr_d = buf.d[K - 1]; thr_i = buf.i[K - 1];
                    ++selections;
                    dirty = false;
                }
                double bound2 = INFINITY;                                         // df_search's bound of what lies outside the cube
                bool open = false;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const double rest = out2 - out[ax] * out[ax];
                    const int jp = c[ax] + r + 1, jm = c[ax] - r - 1;
                    if (jp < g[ax]) {
                        const double f = fmax(fmax(lo[ax] + (double)jp * cell_w[ax] * DF_SHRINK - qd[ax], out[ax]), 0.0);
                        bound2 = fmin(bound2, f * f + rest);
                        open = true;
                    }
                    if (jm >= 0) {
                        const double f = fmax(fmax(qd[ax] - (lo[ax] + (double)(jm + 1) * cell_w[ax] * DF_GROW), out[ax]), 0.0);
                        bound2 = fmin(bound2, f * f + rest);
                        open = true;
                    }
                }
                if (!open) { ended = true; break; }                               // the cube covers the grid
                if ((full ? thr_d : (double)INFINITY) < bound2) { ended = true; break; }
                if (!(bound2 < a.r2)) { ended = true; break; }                    // nothing outside the cube lies within the radius
            }
            if (!ended && lane == 0) atomicOr(a.status, DNSPLAT_NORMALS_STATUS_INTERNAL);
            if (dirty) {                                                          // fewer than K were found
                nm_sort(buf, count, lane);
                ++selections;
            }
        }
        __syncthreads();
        const int n = count;                                                      // every entry has d2 < radius^2: the threshold never rose
        if (a.count && lane == 0) a.count[q] = n;
        if (a.nbr) {
            for (int j = lane; j < a.knn; j += DNS_WAVE) a.nbr[(size_t)q * a.knn + j] = j < n ? buf.i[j] : -1;
        }
        // the moments: lane l adds ranks l, l + 64, .. in ascending order, then the xor tree
        double p[NM_LANE_TERMS][3], S[3] = {0.0, 0.0, 0.0}, C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < NM_LANE_TERMS; ++j) {
            const int t = lane + DNS_WAVE * j;
            const int id = t < n ? buf.i[t] : -1;
            const bool in = (unsigned)id < (unsigned)a.N;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                p[j][ax] = in ? (double)a.points[(size_t)id * 3 + ax] : 0.0;
                S[ax] = in ? S[ax] + p[j][ax] : S[ax];
            }
        }
        if (n > 0) {
            const double dn = (double)n;
            double mean[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) mean[ax] = nm_wave_sum(S[ax]) / dn;
#pragma unroll
            for (int j = 0; j < NM_LANE_TERMS; ++j) {
                if (lane + DNS_WAVE * j < n) {
                    const double d0 = p[j][0] - mean[0], d1 = p[j][1] - mean[1], d2 = p[j][2] - mean[2];
                    C[0] = C[0] + d0 * d0; C[1] = C[1] + d0 * d1; C[2] = C[2] + d0 * d2;
                    C[3] = C[3] + d1 * d1; C[4] = C[4] + d1 * d2; C[5] = C[5] + d2 * d2;
                }
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) C[k] = nm_wave_sum(C[k]) / dn;
        }
        double nrm[3];
        nm_normal(C, n, nrm);
        nm_orient(nrm, a.orient != 0, a.toward, qd);
        if (lane == 0) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) a.normals[(size_t)q * 3 + ax] = nrm[ax];
            if (a.cov) {
#pragma unroll
                for (int k = 0; k < 6; ++k) a.cov[(size_t)q * 6 + k] = C[k];
            }
            nm_note_max(&a.search[0], ring);
            nm_note_max(&a.search[1], selections);
        }
        __syncthreads();                                                          // the next query writes the buffer
    }
}

bool nm_size_ok(int N, int knn) { return N >= 1 && knn >= 3 && knn <= DNSPLAT_NORMALS_MAX_K; }

}  // namespace

extern "C" size_t dnsplat_cloud_normals_scratch_bytes(int32_t N, int32_t knn) { return nm_size_ok(N, knn) ? NM_SCRATCH_BYTES : 0; }

extern "C" int dnsplat_cloud_normals(const dnsplat_cloud_normals_args *a, dnsplat_stream_t stream_)
{
    if (!a || a->N < 1 || !a->points || !a->index || !a->normals || !a->status || !a->scratch || a->radius != a->radius ||
        (a->orient != 0 && a->orient != 1))
        return DNSPLAT_ERR_INVALID_ARG;
    if (a->orient && !(a->toward[0] == a->toward[0] && a->toward[1] == a->toward[1] && a->toward[2] == a->toward[2])) return DNSPLAT_ERR_INVALID_ARG;
    if (a->knn < 3 || a->knn > DNSPLAT_NORMALS_MAX_K) return DNSPLAT_ERR_UNSUPPORTED;
    if (a->scratch_bytes < NM_SCRATCH_BYTES || (size_t)a->scratch % sizeof(double)) return DNSPLAT_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    NmArgs k;
    k.ix = df_view(a->index, df_layout(a->N));
    k.N = a->N;
    k.knn = a->knn;
    k.K = a->knn < a->N ? a->knn : a->N;
    k.orient = a->orient;
    k.points = a->points;
    const bool limited = a->radius > 0.0 && a->radius < (double)INFINITY;
    k.r2 = limited ? a->radius * a->radius : (double)INFINITY;
    for (int ax = 0; ax < 3; ++ax) k.toward[ax] = a->orient ? a->toward[ax] : 0.0;
    k.normals = a->normals; k.cov = a->covariance; k.nbr = a->neighbors; k.count = a->count; k.status = a->status;
    k.search = (int32_t *)a->scratch;
    const dim3 grid((unsigned)(a->N < NM_MAX_BLOCKS ? a->N : NM_MAX_BLOCKS)), block(NM_THREADS);
    if (a->knn <= NM_MIN_KP) hipLaunchKernelGGL((nm_kernel<NM_MIN_KP>), grid, block, 0, stream, k);
    else if (a->knn <= 2 * NM_MIN_KP) hipLaunchKernelGGL((nm_kernel<2 * NM_MIN_KP>), grid, block, 0, stream, k);
    else hipLaunchKernelGGL((nm_kernel<DNSPLAT_NORMALS_MAX_K>), grid, block, 0, stream, k);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
