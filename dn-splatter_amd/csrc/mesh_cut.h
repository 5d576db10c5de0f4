// mesh_cut.h — the back half of a mesh cut, shared by meshcull.hip (dnsplat_mesh_cut_*) and meshclusters.hip (dnsplat_mesh_filter_*):
// once a rule has left keep flags per triangle, marks on the vertices the kept triangles reference and the kept count per block of
// MV_THREADS triangles, the rest is the same — the marked vertices per block, both scans with counts = {V', T'}, and the triangles in
// their order with their indices remapped.  What differs stays with its owner: the rule, and what is written per kept vertex (its
// coordinates there, its old id here).  Integers only, no atomics: the scans, the flag rank and the layout of the ordered append of
// block_scan.h; the marks are plain stores of the same value 1.
#pragma once

#include "block_scan.h"

namespace {

constexpr int MV_THREADS = 256;
constexpr int MV_SCAN_PER = 4;             // mv_cut_scan_kernel: MV_THREADS * MV_SCAN_PER block counts per trip

int mv_blocks(long long n) { return (int)((n + MV_THREADS - 1) / MV_THREADS); }

__global__ __launch_bounds__(MV_THREADS) void mv_mark_count_kernel(int V, const int32_t *__restrict__ marks, int32_t *__restrict__ vcount)
{
    __shared__ int wave_tot[MV_THREADS / DNS_WAVE];
    const int i = blockIdx.x * MV_THREADS + threadIdx.x;
    int total;
    dns_block_rank<MV_THREADS>(i < V && marks[i] != 0, wave_tot, total);
    if (threadIdx.x == 0) vcount[blockIdx.x] = total;
}

// One workgroup: both arrays of block counts to their exclusive prefix sums in place; counts = {V', T'}
__global__ __launch_bounds__(MV_THREADS) void mv_cut_scan_kernel(int nbv, int32_t *__restrict__ vcount, int nbt, int32_t *__restrict__ tcount,
                                                                 int64_t *__restrict__ counts)
{
    const int nv = dns_scan_in_place<MV_THREADS, MV_SCAN_PER>(nbv, vcount);
    __syncthreads();
    const int nt = dns_scan_in_place<MV_THREADS, MV_SCAN_PER>(nbt, tcount);
    if (threadIdx.x == 0) { counts[0] = nv; counts[1] = nt; }
}

// new_id: the marks after the emit of the vertices, new id + 1.  The status bits are DNSPLAT_MESH_CUT_STATUS_*; the filter's have the
// same values.
__global__ __launch_bounds__(MV_THREADS) void mv_emit_triangles_kernel(int T, const int32_t *__restrict__ triangles, const uint8_t *__restrict__ keep,
                                                                       const int32_t *__restrict__ tcount, const int32_t *__restrict__ new_id,
                                                                       const int64_t *__restrict__ counts, long long cap_v, long long cap_t,
                                                                       int32_t *__restrict__ out, int32_t *__restrict__ status)
{
    __shared__ int wave_tot[MV_THREADS / DNS_WAVE];
    const int t = blockIdx.x * MV_THREADS + threadIdx.x;
    const bool kept = t < T && keep[t] != 0;
    int total;
    const int row = tcount[blockIdx.x] + dns_block_rank<MV_THREADS>(kept, wave_tot, total);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        status[0] = (counts[0] > cap_v ? DNSPLAT_MESH_CUT_STATUS_VERTICES : 0) | (counts[1] > cap_t ? DNSPLAT_MESH_CUT_STATUS_TRIANGLES : 0);
    if (kept && row < cap_t) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[(size_t)row * 3 + k] = new_id[triangles[(size_t)t * 3 + k]] - 1;
    }
}

}  // namespace
