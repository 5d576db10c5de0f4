// depth_buckets.h — the bucket map of the depth sort's range partition (binning.hip, step 1).
//
// The visible Gaussians are cut into B = 2^bbits buckets by  d(k) = (k - kmin) >> shift,  k = the 32 depth bits, kmin / kmax = the
// smallest / largest of them in the frame and  shift = max(0, bitlen(kmax - kmin) - bbits).  The map is monotone in k, d(kmin) = 0
// and d(kmax) < B, and the keys of one bucket agree in every bit of k - kmin at or above `shift` — so a stable sort of each bucket on
// the low `shift` bits of k - kmin, buckets taken in order, is the stable sort of all keys.
//
// Plain C++ on purpose (no HIP types): tests/test_depth_buckets_host.py compiles this header with g++ and checks these properties.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DNS_DB_HD __host__ __device__ __forceinline__
#else
#define DNS_DB_HD inline
#endif

// keys per bucket the bucket sort holds in LDS (8-byte pairs, 16 per lane in registers); a larger bucket is sorted in global memory
#ifndef DNS_DP_CAP
#define DNS_DP_CAP 4096
#endif

// log2(B) for a sort over N entries: about N / 1024 buckets, a power of two in [512, 4096]
DNS_DB_HD int dns_depth_bucket_bits(int64_t N)
{
    int bits = 9;
    while (bits < 12 && ((int64_t)1024 << bits) < N) ++bits;
    return bits;
}

DNS_DB_HD int dns_bitlen_u32(uint32_t v)
{
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}

// kmin <= kmax
DNS_DB_HD int dns_depth_bucket_shift(uint32_t kmin, uint32_t kmax, int bbits)
{
    const int s = dns_bitlen_u32(kmax - kmin) - bbits;
    return s > 0 ? s : 0;
}

DNS_DB_HD uint32_t dns_depth_bucket(uint32_t k, uint32_t kmin, int shift) { return (k - kmin) >> shift; }

// the bucket sort: LSD passes over the low `shift` bits of k - kmin, at most 8 bits each, the bits split evenly
DNS_DB_HD int dns_depth_local_passes(int shift) { return (shift + 7) / 8; }
DNS_DB_HD int dns_depth_local_bits(int shift)
{
    const int p = dns_depth_local_passes(shift);
    return p ? (shift + p - 1) / p : 0;
}
