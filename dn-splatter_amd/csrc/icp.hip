// icp.hip — the reference's mesh alignment on the device: get_align_transformation (eval/eval_mesh_vis_cull.py:269-287, called at :427-431),
// Open3D's registration_icp with TransformationEstimationPointToPoint, which the reference runs on a CPU k-d tree.  The definition is
// stated in include/dnsplat.h (PARITY UNPINNED AGAINST Open3D) and restated in torch_icp.py.
//   dnsplat_icp_begin      icp_begin_kernel      the state: T = init (a kernel argument), everything else 0;
//   dnsplat_icp_iterate    icp_corr_kernel       one thread per source point: q = fl32(T s) formed in double, df_search<1> on the index of
//                                                the targets (density_common.h: the nearest under (d^2, index), d^2 in double), the
//                                                threshold test, and one partial per workgroup: n as an integer, and in double the sums
//                                                of d^2, q - c, g - c and (g - c)(q - c)^T, c the centre of the index's bounding box;
//                          icp_solve_kernel      one workgroup adds the partials in the one fixed order of block_reduce.h; one thread
//                                                forms fitness and rmse, tests the stop criteria against the pass before, and otherwise
//                                                solves for the rigid update (Horn's 4 x 4 matrix, a fixed-order cyclic Jacobi of
//                                                ICP_SWEEPS sweeps in double) and leaves T <- U T in the state;
//   dnsplat_icp_run        begin, then max_iteration + 1 iterates.  Once `done` is set in the state, every later launch returns at its
//                          first load: the host never reads inside the loop;
//   dnsplat_transform_points   icp_transform_kernel   out = fl32(T p) under q's rule, or the rotation alone;
//   dnsplat_knn_points     icp_unsort_kernel     the points an index was built over, in their own order, from its sorted copy.
// No floating-point atomic, every loop bounded by its sizes: equal inputs give equal bytes.  Compiled without contraction; the two FMAs of
// d^2 are df_search's own.

#include "block_reduce.h"
#include "density_common.h"
#include "icp_solve.h"

namespace {

constexpr int ICP_THREADS = 256;
constexpr int ICP_WAVES = ICP_THREADS / DNS_WAVE;

struct IcpState {                                         // DNSPLAT_ICP_STATE_BYTES, stated in dnsplat.h
    double T[16];                                         // row-major 4 x 4
    double fitness, rmse;                                 // of the last pass that ran
    long long n, iterations, done, status, passes, pad;
};
static_assert(sizeof(IcpState) == DNSPLAT_ICP_STATE_BYTES, "the state record");

struct IcpInit { double T[16]; };

long long icp_blocks(long long n) { return (n + ICP_THREADS - 1) / ICP_THREADS; }

// THE transform rule: every coordinate ((T[a][0] x + T[a][1] y) + T[a][2] z) + T[a][3] in double (the last term dropped for a rotation
// alone), then ONE rounding to fp32
__device__ __forceinline__ void icp_apply(const double *T, float x, float y, float z, bool rotate_only, float out[3])
{
    const double p[3] = {(double)x, (double)y, (double)z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double r = (T[4 * a] * p[0] + T[4 * a + 1] * p[1]) + T[4 * a + 2] * p[2];
        out[a] = (float)(rotate_only ? r : r + T[4 * a + 3]);
    }
}

__global__ void icp_begin_kernel(IcpInit init, IcpState *state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    IcpState s;
    for (int k = 0; k < 16; ++k) s.T[k] = init.T[k];
    s.fitness = 0.0; s.rmse = 0.0;
    s.n = 0; s.iterations = 0; s.done = 0; s.status = 0; s.passes = 0; s.pad = 0;
    *state = s;
}

struct IcpCorr {
    DfIndex ix;
    long long M;
    int N;
    const float *src, *tgt;
    double r2;
    const IcpState *state;
    IcpPartial *part;
    int32_t *idx;
    double *dist2;
};

__global__ __launch_bounds__(ICP_THREADS) void icp_corr_kernel(IcpCorr a)
{
    __shared__ IcpPartial red[ICP_WAVES];
    if (a.state->done) return;                            // uniform over the grid: nobody reaches a barrier
    const int t = threadIdx.x;
    const long long m = (long long)blockIdx.x * ICP_THREADS + t;
    IcpPartial v = IcpPartial::identity();
    if (m < a.M) {
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = a.state->T[k];
        const float sx = a.src[m * 3], sy = a.src[m * 3 + 1], sz = a.src[m * 3 + 2];
        const bool finite = fabsf(sx) < INFINITY && fabsf(sy) < INFINITY && fabsf(sz) < INFINITY;
        float q[3];
        icp_apply(T, sx, sy, sz, false, q);
        DfList<1> L;
        const bool ok = finite && df_search<1>(a.ix, q[0], q[1], q[2], 1, L);
        const bool corr = ok && L.i[0] != 0x7fffffff && (unsigned)L.i[0] < (unsigned)a.N && L.d[0] <= a.r2;   // false for d^2 = inf or nan
        if (a.idx) a.idx[m] = corr ? L.i[0] : -1;
        if (a.dist2) a.dist2[m] = corr ? L.d[0] : (double)NAN;
        if (corr) {
            const DfHeader h = *a.ix.header;
            double qc[3], gc[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double c = ((double)h.lo[k] + (double)h.hi[k]) * 0.5;
                qc[k] = (double)q[k] - c;
                gc[k] = (double)a.tgt[(size_t)L.i[0] * 3 + k] - c;
            }
            v.n = 1;
            v.d2 = L.d[0];
#pragma unroll
            for (int k = 0; k < 3; ++k) { v.q[k] = qc[k]; v.g[k] = gc[k]; }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) v.gq[3 * i + j] = gc[i] * qc[j];
        }
    }
    dns_block_join<ICP_THREADS>(v, red);
    if (t == 0) a.part[blockIdx.x] = v;
}

__global__ __launch_bounds__(ICP_THREADS) void icp_solve_kernel(long long M, int n_part, const IcpPartial *__restrict__ part, const DfHeader *header,
                                                                 double rel_fitness, double rel_rmse, int max_iteration, IcpState *state,
                                                                 double *__restrict__ trace)
{
    __shared__ IcpPartial red[ICP_WAVES];
    if (state->done) return;                              // uniform: thread 0 writes the state only behind the fold's barriers
    IcpPartial v;
    dns_fold_partials<ICP_THREADS>(part, n_part, v, red);
    if (threadIdx.x != 0) return;
    IcpState s = *state;
    const long long k = s.passes;
    const double fitness = (double)v.n / (double)M;
    const double rmse = v.n > 0 ? sqrt(v.d2 / (double)v.n) : 0.0;
    const double df = fitness - s.fitness, dr = rmse - s.rmse;
    bool stop = v.n == 0 || k >= max_iteration;
    if (k >= 1 && (df < 0.0 ? -df : df) < rel_fitness && (dr < 0.0 ? -dr : dr) < rel_rmse) stop = true;
    if (v.n == 0) s.status |= DNSPLAT_ICP_STATUS_NO_CORRESPONDENCE;
    s.fitness = fitness; s.rmse = rmse; s.n = v.n; s.passes = k + 1;
    if (trace && k <= max_iteration) {
        trace[4 * k] = (double)v.n; trace[4 * k + 1] = fitness; trace[4 * k + 2] = rmse; trace[4 * k + 3] = stop ? 1.0 : 0.0;
    }
    if (stop) {
        s.done = 1;
    } else {
        const DfHeader h = *header;
        double c[3], R[9], tr[3], Tn[12];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = ((double)h.lo[a] + (double)h.hi[a]) * 0.5;
        if (icp_solve(v, c, R, tr)) s.status |= DNSPLAT_ICP_STATUS_DEGENERATE;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double r = (R[3 * a] * s.T[b] + R[3 * a + 1] * s.T[4 + b]) + R[3 * a + 2] * s.T[8 + b];
                Tn[4 * a + b] = b == 3 ? r + tr[a] : r;
            }
#pragma unroll
        for (int i = 0; i < 12; ++i) s.T[i] = Tn[i];
        s.iterations = k + 1;
    }
    *state = s;
}

__global__ __launch_bounds__(ICP_THREADS) void icp_transform_kernel(long long N, const float *__restrict__ p, const double *__restrict__ T,
                                                                     float *__restrict__ out, int rotate_only)
{
    const long long i = (long long)blockIdx.x * ICP_THREADS + threadIdx.x;
    if (i >= N) return;
    double M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = T[k];
    float o[3];
    icp_apply(M, p[i * 3], p[i * 3 + 1], p[i * 3 + 2], rotate_only != 0, o);
    out[i * 3] = o[0]; out[i * 3 + 1] = o[1]; out[i * 3 + 2] = o[2];
}

__global__ __launch_bounds__(ICP_THREADS) void icp_unsort_kernel(int N, const float4 *__restrict__ sorted, float *__restrict__ out)
{
    const long long p = (long long)blockIdx.x * ICP_THREADS + threadIdx.x;
    if (p >= N) return;
    const float4 v = sorted[p];
    const int i = __float_as_int(v.w);
    if ((unsigned)i >= (unsigned)N) return;               // a buffer that is no index: nothing is written out of bounds
    out[(size_t)i * 3] = v.x; out[(size_t)i * 3 + 1] = v.y; out[(size_t)i * 3 + 2] = v.z;
}

bool icp_finite(double v) { return v - v == 0.0; }

int icp_check(const dnsplat_icp_args *a)
{
    if (!a || a->M < 1 || a->N < 1 || !a->source || !a->target || !a->index || !a->state || !a->scratch) return DNSPLAT_ERR_INVALID_ARG;
    if (!(a->max_dist > 0.0) || !icp_finite(a->max_dist) || a->max_iteration < 0) return DNSPLAT_ERR_INVALID_ARG;
    if (!(a->relative_fitness == a->relative_fitness) || !(a->relative_rmse == a->relative_rmse)) return DNSPLAT_ERR_INVALID_ARG;
    if (a->M > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;
    if (a->scratch_bytes < (size_t)icp_blocks(a->M) * sizeof(IcpPartial) || (size_t)a->scratch % sizeof(double) || (size_t)a->state % sizeof(double))
        return DNSPLAT_ERR_WORKSPACE;
    return DNSPLAT_OK;
}

int icp_check_init(const double *init)
{
    if (!init) return DNSPLAT_OK;
    for (int k = 0; k < 16; ++k)
        if (!icp_finite(init[k])) return DNSPLAT_ERR_INVALID_ARG;
    return DNSPLAT_OK;
}

void icp_launch_begin(const dnsplat_icp_args *a, const double *init, hipStream_t stream)
{
    IcpInit in;
    for (int k = 0; k < 16; ++k) in.T[k] = init ? init[k] : (k % 5 == 0 ? 1.0 : 0.0);
    hipLaunchKernelGGL(icp_begin_kernel, dim3(1), dim3(DNS_WAVE), 0, stream, in, (IcpState *)a->state);
}

void icp_launch_pass(const dnsplat_icp_args *a, hipStream_t stream)
{
    const int nb = (int)icp_blocks(a->M);
    IcpCorr q;
    q.ix = df_view(a->index, df_layout(a->N));
    q.M = a->M; q.N = a->N;
    q.src = a->source; q.tgt = a->target;
    q.r2 = a->max_dist * a->max_dist;
    q.state = (const IcpState *)a->state;
    q.part = (IcpPartial *)a->scratch;
    q.idx = a->idx; q.dist2 = a->dist2;
    hipLaunchKernelGGL(icp_corr_kernel, dim3((unsigned)nb), dim3(ICP_THREADS), 0, stream, q);
    hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(ICP_THREADS), 0, stream, (long long)a->M, nb, (const IcpPartial *)a->scratch, q.ix.header,
                       a->relative_fitness, a->relative_rmse, (int)a->max_iteration, (IcpState *)a->state, a->trace);
}

}  // namespace

extern "C" size_t dnsplat_icp_scratch_bytes(int64_t M)
{
    if (M < 1 || M > 0x7fffffffLL) return 0;
    return (size_t)icp_blocks(M) * sizeof(IcpPartial);
}

extern "C" int dnsplat_icp_begin(const dnsplat_icp_args *a, const double *init, dnsplat_stream_t stream_)
{
    int rc = icp_check(a);
    if (rc == DNSPLAT_OK) rc = icp_check_init(init);
    if (rc != DNSPLAT_OK) return rc;
    icp_launch_begin(a, init, (hipStream_t)stream_);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_icp_iterate(const dnsplat_icp_args *a, dnsplat_stream_t stream_)
{
    const int rc = icp_check(a);
    if (rc != DNSPLAT_OK) return rc;
    icp_launch_pass(a, (hipStream_t)stream_);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_icp_run(const dnsplat_icp_args *a, const double *init, dnsplat_stream_t stream_)
{
    int rc = icp_check(a);
    if (rc == DNSPLAT_OK) rc = icp_check_init(init);
    if (rc != DNSPLAT_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    icp_launch_begin(a, init, stream);
    for (int k = 0; k <= a->max_iteration; ++k) icp_launch_pass(a, stream);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_transform_points(int64_t N, const float *p, const double *T, float *out, int rotate_only, dnsplat_stream_t stream_)
{
    if (N < 0 || !T || (N > 0 && (!p || !out))) return DNSPLAT_ERR_INVALID_ARG;
    if (N > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;
    if (N == 0) return DNSPLAT_OK;
    hipLaunchKernelGGL(icp_transform_kernel, dim3((unsigned)icp_blocks(N)), dim3(ICP_THREADS), 0, (hipStream_t)stream_, (long long)N, p, T, out,
                       rotate_only);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_knn_points(int32_t N, const void *index, float *out, dnsplat_stream_t stream_)
{
    if (N < 1 || !index || !out) return DNSPLAT_ERR_INVALID_ARG;
    const DfIndex ix = df_view(index, df_layout(N));
    hipLaunchKernelGGL(icp_unsort_kernel, dim3((unsigned)icp_blocks(N)), dim3(ICP_THREADS), 0, (hipStream_t)stream_, (int)N, ix.sorted, out);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
