// density.hip — the reference's Gaussian density field (dn_model.py:1061-1135 get_closest_gaussians / get_density, :1449-1494
// get_density_grad, utils/knn.py:29-43 knn_sk) on the device: an exact k-nearest-neighbour search over the means and the density and
// its analytic normal at arbitrary samples or on a lattice.  Nothing is read on the host.
//   dnsplat_knn_build      a uniform grid over the bounding box of the means (dnsplat_knn_grid_dim(N) cells per axis, about two points
//                          per cell): min / max reduction, cell id + histogram, one-workgroup scan, scatter, and an in-cell ordering by
//                          ascending Gaussian index, so that the sorted copy (x, y, z, index) is the same bits for every build.
//   dnsplat_knn_query      one thread per query: shells of cells outward from the query's (clamped) cell, the best k + skip candidates
//                          in registers (an insertion list with static indices), ranked by (d^2, index) with d^2 in DOUBLE — sklearn
//                          ranks in fp64, and consecutive ranks differ by less than fp32 resolves.  A query stops once its worst kept
//                          d^2 is below a lower bound of the d^2 of every point in an unvisited cell; the bound is widened by 4e-7
//                          relative, above the two fp32 roundings of the cell assignment (df_axis_cell).
//   dnsplat_density_pack   per Gaussian 16 floats: mean, sigmoid(opacity), M = R(q / |q|) diag(1 / max(exp(s), 1e-3)).
//   dnsplat_density_eval   density and / or normal per sample (a list [M,3], or a lattice X x Y x Z in `ij` order with a byte mask and
//                          a fill value), the neighbours either the caller's index tensor or the search run in the same thread.
// Both neighbour sources feed df_accumulate in rank order, and the file is compiled without contraction: they give equal bits.

#include "block_scan.h"
#include "density_common.h"

namespace {

constexpr int DF_BRICK_X = 4, DF_BRICK_Y = 4, DF_BRICK_Z = 16;      // lattice points of a workgroup: one 4 x 4 x 4 brick per wave

__global__ __launch_bounds__(DF_THREADS) void df_minmax_kernel(int N, const float *__restrict__ means, float *__restrict__ partial)
{
    __shared__ float red[DF_WAVES][6];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = (long long)blockIdx.x * DF_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * DF_THREADS) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = means[i * 3 + a];
            lo[a] = fminf(lo[a], v);
            hi[a] = fmaxf(hi[a], v);
        }
    }
#pragma unroll
    for (int off = DNS_WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, DNS_WAVE));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, DNS_WAVE));
        }
    }
    const int lane = threadIdx.x & (DNS_WAVE - 1), wave = threadIdx.x / DNS_WAVE;
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[wave][a] = lo[a]; red[wave][3 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = red[0][threadIdx.x];
        for (int w = 1; w < DF_WAVES; ++w) v = threadIdx.x < 3 ? fminf(v, red[w][threadIdx.x]) : fmaxf(v, red[w][threadIdx.x]);
        partial[blockIdx.x * 6 + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(DNS_WAVE) void df_header_kernel(int nb, const float *__restrict__ partial, int G, DfHeader *__restrict__ header)
{
    const int lane = threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = lane; b < nb; b += DNS_WAVE) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], partial[b * 6 + a]);
            hi[a] = fmaxf(hi[a], partial[b * 6 + 3 + a]);
        }
    }
#pragma unroll
    for (int off = DNS_WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, DNS_WAVE));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, DNS_WAVE));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float ext = __fsub_rn(hi[a], lo[a]);
            float inv = 0.f;
            if (ext > 0.f && ext < INFINITY) {
                inv = __fdiv_rn((float)G, ext);
                if (!(inv < INFINITY)) inv = 0.f;              // an extent of a few denormals: one cell thick
            }
            header->lo[a] = lo[a];
            header->hi[a] = hi[a];
            header->inv_h[a] = inv;
            header->g[a] = inv > 0.f ? G : 1;
        }
        header->pad[0] = header->pad[1] = header->pad[2] = header->pad[3] = 0;
    }
}

__global__ __launch_bounds__(DF_THREADS) void df_cell_kernel(int N, const float *__restrict__ means, const DfHeader *__restrict__ header, int G,
                                                              int32_t *__restrict__ cell_of, int32_t *__restrict__ counts)
{
    const long long i = (long long)blockIdx.x * DF_THREADS + threadIdx.x;
    if (i >= N) return;
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = df_axis_cell(means[i * 3 + a], header->lo[a], header->inv_h[a], header->g[a]);
    const int cell = (c[2] * G + c[1]) * G + c[0];
    cell_of[i] = cell;
    atomicAdd(&counts[cell], 1);                                  // integer: the sum does not depend on the order
}

// counts[0 .. n) -> their exclusive prefix sums in place (n = C + 1: the last entry becomes N)
__global__ __launch_bounds__(DF_SCAN_THREADS) void df_scan_kernel(long long n, int32_t *__restrict__ counts)
{
    dns_scan_in_place<DF_SCAN_THREADS, DF_SCAN_PER>(n, counts);
}

__global__ __launch_bounds__(DF_THREADS) void df_scatter_kernel(int N, const int32_t *__restrict__ cell_of, const int32_t *__restrict__ cell_start,
                                                                 int32_t *__restrict__ fill, int32_t *__restrict__ tmp)
{
    const long long i = (long long)blockIdx.x * DF_THREADS + threadIdx.x;
    if (i >= N) return;
    const int cell = cell_of[i];
    const int at = cell_start[cell] + atomicAdd(&fill[cell], 1);  // the order within a cell is arbitrary here; df_order_kernel fixes it
    if (at >= 0 && at < N) tmp[at] = (int32_t)i;
}

// position p of the arbitrary in-cell order -> its place in ascending Gaussian index; the cell's points are few (about two)
__global__ __launch_bounds__(DF_THREADS) void df_order_kernel(int N, const float *__restrict__ means, const int32_t *__restrict__ cell_of,
                                                               const int32_t *__restrict__ cell_start, const int32_t *__restrict__ tmp,
                                                               float4 *__restrict__ sorted)
{
    const long long p = (long long)blockIdx.x * DF_THREADS + threadIdx.x;
    if (p >= N) return;
    const int i = tmp[p];
    const int cell = cell_of[i];
    const int s = cell_start[cell], e = cell_start[cell + 1];
    int rank = 0;
    for (int q = s; q < e; ++q) rank += tmp[q] < i ? 1 : 0;
    sorted[s + rank] = make_float4(means[(size_t)i * 3], means[(size_t)i * 3 + 1], means[(size_t)i * 3 + 2], __int_as_float(i));
}

template <int KM>
__global__ __launch_bounds__(DF_THREADS) void df_query_kernel(DfIndex ix, long long M, const float *__restrict__ queries, int k, int skip,
                                                               int32_t *__restrict__ out_idx, float *__restrict__ out_d2)
{
    const long long m = (long long)blockIdx.x * DF_THREADS + threadIdx.x;
    if (m >= M) return;
    DfList<KM> L;
    const bool ok = df_search(ix, queries[m * 3], queries[m * 3 + 1], queries[m * 3 + 2], k + skip, L);
#pragma unroll
    for (int j = 0; j < KM; ++j) {
        if (j >= skip && j < skip + k) {
            const bool found = ok && L.i[j] != 0x7fffffff;               // fewer than k + skip comparable means (nan coordinates)
            out_idx[m * k + (j - skip)] = found ? L.i[j] : -1;
            if (out_d2) out_d2[m * k + (j - skip)] = found ? (float)L.d[j] : NAN;
        }
    }
}

// ---- records and evaluation ----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(DF_THREADS) void df_pack_kernel(int N, const float *__restrict__ means, const float *__restrict__ scales,
                                                              const float *__restrict__ quats, const float *__restrict__ opacities,
                                                              float *__restrict__ records)
{
    const long long i = (long long)blockIdx.x * DF_THREADS + threadIdx.x;
    if (i >= N) return;
    const float qw = quats[i * 4], qx = quats[i * 4 + 1], qy = quats[i * 4 + 2], qz = quats[i * 4 + 3];
    const float len = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
    const float div = fmaxf(len, 1e-12f);                           // F.normalize
    const float w = qw / div, x = qx / div, y = qy / div, z = qz / div;
    const float R[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - w * z),       2.f * (x * z + w * y),
                        2.f * (x * y + w * z),       1.f - 2.f * (x * x + z * z), 2.f * (y * z - w * x),
                        2.f * (x * z - w * y),       2.f * (y * z + w * x),       1.f - 2.f * (x * x + y * y)};
    float s[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) s[a] = 1.0f / fmaxf(expf(scales[i * 3 + a]), 1e-3f);
    float *rec = records + i * DNS_REC;
    rec[0] = means[i * 3];
    rec[1] = means[i * 3 + 1];
    rec[2] = means[i * 3 + 2];
    rec[3] = 1.0f / (1.0f + expf(-opacities[i]));
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int a = 0; a < 3; ++a) rec[4 + 3 * r + a] = R[3 * r + a] * s[a];
    rec[13] = rec[14] = rec[15] = 0.f;
}

struct DfEval {
    int N;
    DfIndex ix;
    const float *records;
    long long M;
    const float *samples;
    const float *X, *Y, *Z;
    int Rx, Ry, Rz, bricks_y, bricks_z;
    const uint8_t *mask;
    float fill;
    const int32_t *nb32;
    const int64_t *nb64;
    int k, skip, num_closest;
    float *density, *normals;
};

// the sample of this thread and the row it writes; false past the end
__device__ __forceinline__ bool df_sample(const DfEval &e, float &x, float &y, float &z, long long &row)
{
    if (e.samples) {
        row = (long long)blockIdx.x * DF_THREADS + threadIdx.x;
        if (row >= e.M) return false;
        x = e.samples[row * 3]; y = e.samples[row * 3 + 1]; z = e.samples[row * 3 + 2];
        return true;
    }
    long long b = blockIdx.x;
    const int bz = (int)(b % e.bricks_z); b /= e.bricks_z;
    const int by = (int)(b % e.bricks_y);
    const int bx = (int)(b / e.bricks_y);
    const int lane = threadIdx.x & (DNS_WAVE - 1), wave = threadIdx.x / DNS_WAVE;
    const int iz = bz * DF_BRICK_Z + wave * 4 + (lane & 3), iy = by * DF_BRICK_Y + ((lane >> 2) & 3), ix = bx * DF_BRICK_X + (lane >> 4);
    if (ix >= e.Rx || iy >= e.Ry || iz >= e.Rz) return false;
    row = ((long long)ix * e.Ry + iy) * e.Rz + iz;
    x = e.X[ix]; y = e.Y[iy]; z = e.Z[iz];
    return true;
}

__device__ __forceinline__ void df_write(const DfEval &e, long long row, bool ok, const DfAcc &acc)
{
    if (e.density) {
        float d = acc.density;
        if (d >= 1.0f) d = d / (d + 1e-5f);
        e.density[row] = ok ? fmaxf(d, 1e-4f) : NAN;
    }
    if (e.normals) {
        const float len = sqrtf(acc.g[0] * acc.g[0] + acc.g[1] * acc.g[1] + acc.g[2] * acc.g[2]);
        const float div = fmaxf(len, 1e-12f);
#pragma unroll
        for (int a = 0; a < 3; ++a) e.normals[row * 3 + a] = ok ? -(acc.g[a] / div) : NAN;
    }
}

// KM > 0: the neighbours are searched here; KM == 0: they are the caller's
template <int KM>
__global__ __launch_bounds__(DF_THREADS) void df_eval_kernel(DfEval e)
{
    float x, y, z;
    long long row;
    if (!df_sample(e, x, y, z, row)) return;
    if (e.mask && !e.mask[row]) {
        if (e.density) e.density[row] = e.fill;
        if (e.normals) e.normals[row * 3] = e.normals[row * 3 + 1] = e.normals[row * 3 + 2] = 0.f;
        return;
    }
    DfAcc acc;
    acc.density = 0.f;
    acc.g[0] = acc.g[1] = acc.g[2] = 0.f;
    bool ok = true;
    if constexpr (KM > 0) {
        DfList<KM> L;
        ok = df_search(e.ix, x, y, z, e.k + e.skip, L);
        if (ok) {
#pragma unroll
            for (int j = 0; j < KM; ++j)
                if (j >= e.skip && j < e.skip + e.k) {
                    if ((unsigned)L.i[j] < (unsigned)e.N) df_accumulate(e.records, L.i[j], x, y, z, j - e.skip < e.num_closest, acc);
                    else ok = false;                                      // fewer than k + skip comparable means (nan coordinates)
                }
        }
    } else {
        for (int j = 0; j < e.k; ++j) {
            const long long gi = e.nb64 ? (long long)e.nb64[row * e.k + j] : (long long)e.nb32[row * e.k + j];
            if (gi < 0 || gi >= e.N) { ok = false; break; }           // an index outside the field (the search's -1 for a nan sample): nan out
            df_accumulate(e.records, (int)gi, x, y, z, j < e.num_closest, acc);
        }
    }
    df_write(e, row, ok, acc);
}

long long df_blocks(long long n, int per) { return (n + per - 1) / per; }

int df_km(int K) { return K <= 4 ? 4 : K <= 8 ? 8 : K <= 17 ? 17 : 32; }

int df_check_k(int32_t N, int32_t k, int32_t skip)
{
    if (N < 1 || k < 1 || skip < 0) return DNSPLAT_ERR_INVALID_ARG;
    if ((long long)k + skip > DNSPLAT_KNN_MAX_K) return DNSPLAT_ERR_UNSUPPORTED;
    if ((long long)k + skip > N) return DNSPLAT_ERR_INVALID_ARG;      // as sklearn: more neighbours asked for than points fitted
    return DNSPLAT_OK;
}

}  // namespace

extern "C" int32_t dnsplat_knn_grid_dim(int32_t N) { return N < 1 ? 0 : df_grid_dim(N); }

extern "C" size_t dnsplat_knn_index_bytes(int32_t N) { return N < 1 ? 0 : df_layout(N).total; }

extern "C" int dnsplat_knn_build(int32_t N, const float *means, void *index, dnsplat_stream_t stream_)
{
    if (N < 1 || !means || !index) return DNSPLAT_ERR_INVALID_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    const DfLayout l = df_layout(N);
    char *base = (char *)index;
    DfHeader *header = (DfHeader *)base;
    int32_t *cell_start = (int32_t *)(base + l.cell_start), *cell_of = (int32_t *)(base + l.cell_of), *tmp = (int32_t *)(base + l.tmp),
            *fill = (int32_t *)(base + l.fill);
    float4 *sorted = (float4 *)(base + l.sorted);
    float *partial = (float *)(base + l.partial);
    const int nb = (int)df_blocks(N, DF_THREADS);
    const int mb = nb < DF_MINMAX_BLOCKS ? nb : DF_MINMAX_BLOCKS;
    if (hipMemsetAsync(cell_start, 0, l.sorted - l.cell_start, stream) != hipSuccess) return DNSPLAT_ERR_LAUNCH;   // with its padding
    if (hipMemsetAsync(fill, 0, (size_t)l.C * sizeof(int32_t), stream) != hipSuccess) return DNSPLAT_ERR_LAUNCH;
    hipLaunchKernelGGL(df_minmax_kernel, dim3(mb), dim3(DF_THREADS), 0, stream, N, means, partial);
    hipLaunchKernelGGL(df_header_kernel, dim3(1), dim3(DNS_WAVE), 0, stream, mb, (const float *)partial, l.G, header);
    hipLaunchKernelGGL(df_cell_kernel, dim3(nb), dim3(DF_THREADS), 0, stream, N, means, (const DfHeader *)header, l.G, cell_of, cell_start);
    hipLaunchKernelGGL(df_scan_kernel, dim3(1), dim3(DF_SCAN_THREADS), 0, stream, l.C + 1, cell_start);
    hipLaunchKernelGGL(df_scatter_kernel, dim3(nb), dim3(DF_THREADS), 0, stream, N, (const int32_t *)cell_of, (const int32_t *)cell_start, fill, tmp);
    hipLaunchKernelGGL(df_order_kernel, dim3(nb), dim3(DF_THREADS), 0, stream, N, means, (const int32_t *)cell_of, (const int32_t *)cell_start,
                       (const int32_t *)tmp, sorted);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_knn_query(int32_t N, const void *index, int64_t M, const float *queries, int32_t k, int32_t skip, int32_t *out_idx,
                                 float *out_d2, dnsplat_stream_t stream_)
{
    if (!index || M < 0 || (M > 0 && (!queries || !out_idx))) return DNSPLAT_ERR_INVALID_ARG;
    const int rc = df_check_k(N, k, skip);
    if (rc != DNSPLAT_OK) return rc;
    if (M == 0) return DNSPLAT_OK;
    const long long nb = df_blocks(M, DF_THREADS);
    if (nb > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const DfIndex ix = df_view(index, df_layout(N));
    const dim3 grid((unsigned)nb), block(DF_THREADS);
    switch (df_km(k + skip)) {
    case 4: hipLaunchKernelGGL((df_query_kernel<4>), grid, block, 0, stream, ix, (long long)M, queries, k, skip, out_idx, out_d2); break;
    case 8: hipLaunchKernelGGL((df_query_kernel<8>), grid, block, 0, stream, ix, (long long)M, queries, k, skip, out_idx, out_d2); break;
    case 17: hipLaunchKernelGGL((df_query_kernel<17>), grid, block, 0, stream, ix, (long long)M, queries, k, skip, out_idx, out_d2); break;
    default: hipLaunchKernelGGL((df_query_kernel<32>), grid, block, 0, stream, ix, (long long)M, queries, k, skip, out_idx, out_d2); break;
    }
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_density_pack(int32_t N, const float *means, const float *scales_log, const float *quats, const float *opacities_logit,
                                    float *records, dnsplat_stream_t stream_)
{
    if (N < 1 || !means || !scales_log || !quats || !opacities_logit || !records) return DNSPLAT_ERR_INVALID_ARG;
    hipLaunchKernelGGL(df_pack_kernel, dim3((unsigned)df_blocks(N, DF_THREADS)), dim3(DF_THREADS), 0, (hipStream_t)stream_, N, means, scales_log,
                       quats, opacities_logit, records);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_density_eval(const dnsplat_density_args *a, dnsplat_stream_t stream_)
{
    if (!a || !a->records || a->N < 1 || (!a->density && !a->normals)) return DNSPLAT_ERR_INVALID_ARG;
    const bool lattice = a->samples == nullptr;
    if (lattice && (!a->X || !a->Y || !a->Z || a->Rx < 1 || a->Ry < 1 || a->Rz < 1)) return DNSPLAT_ERR_INVALID_ARG;
    if (!lattice && a->M < 0) return DNSPLAT_ERR_INVALID_ARG;
    if (a->num_closest < 0 || a->num_closest > a->k) return DNSPLAT_ERR_INVALID_ARG;
    if (a->neighbors) {
        if (a->k < 1) return DNSPLAT_ERR_INVALID_ARG;
    } else {
        if (!a->index) return DNSPLAT_ERR_INVALID_ARG;
        const int rc = df_check_k(a->N, a->k, a->skip);
        if (rc != DNSPLAT_OK) return rc;
    }
    DfEval e;
    e.N = a->N;
    e.records = a->records;
    e.M = lattice ? (long long)a->Rx * a->Ry * a->Rz : (long long)a->M;
    e.samples = a->samples;
    e.X = a->X; e.Y = a->Y; e.Z = a->Z;
    e.Rx = a->Rx; e.Ry = a->Ry; e.Rz = a->Rz;
    e.bricks_y = lattice ? (int)df_blocks(a->Ry, DF_BRICK_Y) : 1;
    e.bricks_z = lattice ? (int)df_blocks(a->Rz, DF_BRICK_Z) : 1;
    e.mask = a->mask;
    e.fill = a->fill;
    e.nb32 = a->neighbors && !a->neighbors_int64 ? (const int32_t *)a->neighbors : nullptr;
    e.nb64 = a->neighbors && a->neighbors_int64 ? (const int64_t *)a->neighbors : nullptr;
    e.k = a->k;
    e.skip = a->neighbors ? 0 : a->skip;
    e.num_closest = a->num_closest == 0 ? a->k : a->num_closest;
    e.density = a->density;
    e.normals = a->normals;
    if (a->index) e.ix = df_view(a->index, df_layout(a->N));
    else { e.ix.header = nullptr; e.ix.cell_start = nullptr; e.ix.sorted = nullptr; e.ix.G = 0; }
    if (e.M == 0) return DNSPLAT_OK;
    const long long nb = lattice ? df_blocks(a->Rx, DF_BRICK_X) * e.bricks_y * e.bricks_z : df_blocks(e.M, DF_THREADS);
    if (nb > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)nb), block(DF_THREADS);
    if (a->neighbors) {
        hipLaunchKernelGGL((df_eval_kernel<0>), grid, block, 0, stream, e);
    } else {
        switch (df_km(a->k + a->skip)) {
        case 4: hipLaunchKernelGGL((df_eval_kernel<4>), grid, block, 0, stream, e); break;
        case 8: hipLaunchKernelGGL((df_eval_kernel<8>), grid, block, 0, stream, e); break;
        case 17: hipLaunchKernelGGL((df_eval_kernel<17>), grid, block, 0, stream, e); break;
        default: hipLaunchKernelGGL((df_eval_kernel<32>), grid, block, 0, stream, e); break;
        }
    }
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
