// block_reduce.h — what the score kernels (metrics.hip, geometry.hip, ags.hip, pearson.hip) share beside block_scan.h: the fold of a
// struct of partial sums over a workgroup and over the per-workgroup partials, one step of a radix selection on LDS histograms, and the
// integer hash of the samplers (pointcloud.hip, geometry.hip).
//
// THE ORDER OF A FOLD is part of these kernels' tested promise, "equal inputs give equal bits", and is stated here alone:
//   within a wave    a butterfly of __shfl_xor over the lane distances 32, 16, 8, 4, 2, 1;
//   across the waves (wave 0 + wave 1) + (wave 2 + wave 3);
//   across partials  thread t starts from the identity and takes part[t], part[t + THREADS], ... in that order, then the two above.
// A partial P is trivially copyable, a whole number of 32-bit words, and supplies
//   static P identity()      the value that changes nothing when joined;
//   void join(const P &o)    field by field  x = x + o.x  for sums and counts,  x = fmin(x, o.x) / fmax(x, o.x)  for extremes: the
//                            partial's own value is the first operand.
// Compile without contraction (build.sh): a join must stay the additions it spells.
//
// block_scan.h's BARRIER RULE holds for `red` and `wave_sum` here as for `wave_tot` there: a helper that takes one opens with the
// barrier that keeps its writes behind the previous call's reads, so a call may sit in a loop or follow another on the same array.
// Every thread of the workgroup calls the helper, the same number of times.
#pragma once

#include <type_traits>

#include "block_scan.h"

// the "lowbias32" finaliser: the mix32 that dnsplat.h states for the pixel sampler and the mesh sampler, on the device and the host
__host__ __device__ inline uint32_t dns_mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

namespace {

// v of the lane whose number differs from the caller's in the bits of `off`, word by word (a double is two 32-bit shuffles anyway)
template <typename P>
__device__ __forceinline__ P dns_shfl_xor(const P &v, int off)
{
    static_assert(std::is_trivially_copyable<P>::value && sizeof(P) % 4 == 0, "a partial is plain 32-bit words");
    int w[sizeof(P) / 4];
    __builtin_memcpy(w, &v, sizeof(P));
#pragma unroll
    for (int k = 0; k < (int)(sizeof(P) / 4); ++k) w[k] = __shfl_xor(w[k], off, DNS_WAVE);
    P o;
    __builtin_memcpy(&o, w, sizeof(P));
    return o;
}

// v joined over the threads of the workgroup, in every thread.  red: THREADS / DNS_WAVE entries of LDS (the barrier rule above).
template <int THREADS, typename P>
__device__ __forceinline__ void dns_block_join(P &v, P *red)
{
    static_assert(THREADS == 4 * DNS_WAVE, "the tree below is the one of four waves");
#pragma unroll
    for (int off = DNS_WAVE / 2; off >= 1; off >>= 1) v.join(dns_shfl_xor(v, off));
    __syncthreads();                                      // the previous call's readers are done with red
    if ((threadIdx.x & (DNS_WAVE - 1)) == 0) red[threadIdx.x / DNS_WAVE] = v;
    __syncthreads();
    P hi = red[2];
    v = red[0];
    v.join(red[1]);
    hi.join(red[3]);
    v.join(hi);
}

// part[0 .. n_part) joined in the one fixed order, in every thread
template <int THREADS, typename P>
__device__ __forceinline__ void dns_fold_partials(const P *__restrict__ part, int n_part, P &v, P *red)
{
    v = P::identity();
    for (int i = threadIdx.x; i < n_part; i += THREADS) v.join(part[i]);
    dns_block_join<THREADS>(v, red);
}

// ---- one step of a radix selection --------------------------------------------------------------------------------------------------

// One count for `bin` from every lane with `active`, into an LDS histogram.  All 64 lanes of the wave call this together.  64 lanes
// adding to one LDS word serialise, and a frame scored against itself puts every element into ONE bin: PEEL times, the first active
// lane's bin is taken out within the wave (one add of the ballot's population count); what is left after that adds per lane.
template <int PEEL = 1>
__device__ __forceinline__ void dns_hist_add(unsigned int *hist, unsigned int bin, bool active)
{
    uint64_t todo = dns_ballot(active);
    const int lane = threadIdx.x & (DNS_WAVE - 1);
    for (int k = 0; k < PEEL && todo; ++k) {                                      // wave-uniform: todo lives in scalar registers
        const int leader = __builtin_ctzll(todo);
        const unsigned int b = (unsigned int)__builtin_amdgcn_readlane((int)bin, leader);
        const uint64_t same = dns_ballot(active && bin == b) & todo;
        if (lane == leader) atomicAdd(&hist[b], (unsigned int)__builtin_popcountll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&hist[bin], 1u);
}

// the LDS histogram of a workgroup, added to the global one (64-bit: a frame holds up to 3 (2^31 - 1) elements)
template <int THREADS>
__device__ __forceinline__ void dns_hist_flush(const unsigned int *hist, unsigned long long *global, int bins)
{
    for (int b = threadIdx.x; b < bins; b += THREADS) {
        const unsigned int c = hist[b];
        if (c) atomicAdd(&global[b], (unsigned long long)c);
    }
}

// The bin of hist[0 .. BINS) that holds rank `rank`, by one workgroup: true in the one thread that owns it, with the bin and the rank
// that remains inside it.  BINS / THREADS consecutive bins per thread, an exclusive scan of the threads' sums.  wave_sum:
// THREADS / DNS_WAVE entries of LDS, under dns_block_scan's barrier rule.
template <int THREADS, int BINS>
__device__ __forceinline__ bool dns_find_bin(const unsigned long long *__restrict__ hist, unsigned long long rank, unsigned long long *wave_sum,
                                             unsigned int &bin, unsigned long long &rest)
{
    constexpr int PER = BINS / THREADS;
    const int t = threadIdx.x;
    unsigned long long c[PER], mine = 0ull, all;
#pragma unroll
    for (int k = 0; k < PER; ++k) { c[k] = hist[t * PER + k]; mine += c[k]; }
    const unsigned long long before = dns_block_scan<THREADS>(mine, wave_sum, all);
    if (rank < before || rank >= before + mine) return false;
    unsigned long long cum = before;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (rank < cum + c[k]) { bin = (unsigned int)(t * PER + k); rest = rank - cum; return true; }
        cum += c[k];
    }
    return false;
}

}  // namespace
