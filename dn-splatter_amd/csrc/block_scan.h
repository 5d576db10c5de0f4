// block_scan.h — the integer workgroup primitives of the export kernels (pointcloud.hip, levelset.hip, density.hip, metrics.hip,
// marching.hip): the exclusive scan and the flag rank over the threads of a workgroup, the one-workgroup in-place scan of an array of
// counts, and the ordered append behind a device cursor that dnsplat_backproject_points and dnsplat_level_points share.  Integers
// only: the sums are exact in any order, so nothing here is part of a tested bit pattern; the floating-point folds of the score
// kernels, whose order is, are in block_reduce.h.
//
// THE BARRIER RULE: every helper that takes `wave_tot` opens with the barrier that keeps its writes behind the previous call's
// reads of the same array.  A call site may therefore sit in a loop, or follow another call on the same array, with no barrier of
// its own.  Every thread of the workgroup calls the helper, the same number of times.
#pragma once

#include "splat_common.h"

namespace {

// before / total of the per-wave totals in wave_tot: the second half of both helpers below
template <int THREADS, typename T>
__device__ __forceinline__ T dns_waves_before(const T *wave_tot, T &total)
{
    const int wave = threadIdx.x / DNS_WAVE;
    T before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / DNS_WAVE; ++w) {
        const T c = wave_tot[w];
        if (w < wave) before += c;
        total += c;
    }
    return before;
}

// Exclusive prefix sum of v over the threads of the workgroup, in thread order; total = the sum over the whole workgroup.
// T: int, uint32_t, int64_t, unsigned long long.  wave_tot: THREADS / DNS_WAVE entries of LDS (the barrier rule above).
template <int THREADS, typename T>
__device__ __forceinline__ T dns_block_scan(T v, T *wave_tot, T &total)
{
    const int lane = threadIdx.x & (DNS_WAVE - 1);
    T inc = v;
#pragma unroll
    for (int off = 1; off < DNS_WAVE; off <<= 1) {
        const T o = __shfl_up(inc, off, DNS_WAVE);
        if (lane >= off) inc += o;
    }
    __syncthreads();                                      // the previous call's readers are done with wave_tot
    if (lane == DNS_WAVE - 1) wave_tot[threadIdx.x / DNS_WAVE] = inc;
    __syncthreads();
    return dns_waves_before<THREADS>(wave_tot, total) + inc - v;
}

// The number of threads before the caller (in thread order) whose flag is set; total = the number in the whole workgroup.
// wave_tot: THREADS / DNS_WAVE ints of LDS (the barrier rule above).
template <int THREADS>
__device__ __forceinline__ int dns_block_rank(bool flag, int *wave_tot, int &total)
{
    const int lane = threadIdx.x & (DNS_WAVE - 1);
    const uint64_t b = dns_ballot(flag);
    __syncthreads();                                      // the previous call's readers are done with wave_tot
    if (lane == 0) wave_tot[threadIdx.x / DNS_WAVE] = __popcll(b);
    __syncthreads();
    return dns_waves_before<THREADS>(wave_tot, total) + __popcll(b & ((1ull << lane) - 1ull));
}

// One workgroup of THREADS threads turns counts[0 .. n) into their exclusive prefix sums in place, PER consecutive entries per
// thread and THREADS * PER per trip; returns the total (in every thread).
template <int THREADS, int PER>
__device__ __forceinline__ int dns_scan_in_place(long long n, int32_t *__restrict__ counts)
{
    __shared__ int wave_tot[THREADS / DNS_WAVE];
    int carry = 0;
    for (long long i0 = 0; i0 < n; i0 += THREADS * PER) {
        const long long i = i0 + (long long)threadIdx.x * PER;
        int v[PER], sum = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            v[j] = i + j < n ? counts[i + j] : 0;
            sum += v[j];
        }
        int total;
        int run = carry + dns_block_scan<THREADS>(sum, wave_tot, total);
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (i + j < n) counts[i + j] = run;
            run += v[j];
        }
        carry += total;
    }
    return carry;
}

// ---- the ordered append ---------------------------------------------------------------------------------------------------------------
// state = int64 {cursor, overflow, ...}.  A call appends in three launches: a count of the kept rows per block of THREADS rows,
// dns_append_scan_kernel, and the same rows again with the write at base[0] + counts[block] + the row's rank in its block.

// base[0] = the cursor before this call; the cursor moves by `total`, up to capacity; beyond it the overflow word is set
__device__ __forceinline__ void dns_cursor_move(int64_t total, int64_t capacity, int64_t *__restrict__ state, int64_t *__restrict__ base)
{
    const int64_t at = state[0];
    base[0] = at;
    const int64_t end = at + total;
    state[0] = end > capacity ? (at > capacity ? at : capacity) : end;
    if (end > capacity) state[1] = 1;
}

// One workgroup: counts[0 .. nb) -> their exclusive prefix sums in place, then the cursor move by their total
template <int THREADS>
__global__ __launch_bounds__(THREADS) void dns_append_scan_kernel(int nb, int32_t *__restrict__ counts, int64_t capacity,
                                                                   int64_t *__restrict__ state, int64_t *__restrict__ base)
{
    const int total = dns_scan_in_place<THREADS, 1>(nb, counts);
    if (threadIdx.x == 0) dns_cursor_move(total, capacity, state, base);
}

}  // namespace
