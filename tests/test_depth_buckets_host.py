"""csrc/depth_buckets.h — the bucket map of the depth sort's range partition — compiled with g++ and checked on the host:
for random and edge (kmin, kmax) pairs and every bucket count B the map d(k) = (k - kmin) >> shift is non-decreasing in k,
d(kmin) = 0, d(kmax) < B, and the keys of one bucket agree in every bit of k - kmin at or above `shift`; and the route binning.hip
builds on it (stable partition by d, then per bucket stable LSD passes over dns_depth_local_bits(shift) bits each) yields the
stable sort of the keys."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "depth_buckets.h"
static unsigned long long seed = 4242;
static unsigned rnd32() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(seed >> 32); }
#define REQUIRE(c) do { if (!(c)) { printf("FAILED line %d: %s (kmin %u kmax %u bbits %d)\n", __LINE__, #c, kmin, kmax, bbits); return 1; } } while (0)

static int check_map(uint32_t kmin, uint32_t kmax, int bbits)
{
    const uint32_t B = 1u << bbits;
    const int shift = dns_depth_bucket_shift(kmin, kmax, bbits);
    REQUIRE(shift >= 0 && shift <= 32 - bbits);
    REQUIRE(dns_depth_bucket(kmin, kmin, shift) == 0u);
    REQUIRE(dns_depth_bucket(kmax, kmin, shift) < B);
    REQUIRE(shift == 0 || dns_depth_bucket(kmax, kmin, shift) >= B / 2);          // the smallest shift that fits: no bucket range wasted
    REQUIRE(dns_depth_local_passes(shift) * dns_depth_local_bits(shift) >= shift);
    REQUIRE(dns_depth_local_bits(shift) <= 8 && dns_depth_local_passes(shift) <= 3);
    // sorted probes: both ends, their neighbours, bucket borders, random keys in between
    std::vector<uint32_t> ks = {kmin, kmax};
    const uint32_t range = kmax - kmin;
    for (int i = 0; i < 64; ++i) ks.push_back(kmin + (range ? rnd32() % range : 0u));
    for (uint32_t b = 1; b < B && ((uint64_t)b << shift) <= range; b += 1 + rnd32() % 37) {
        ks.push_back(kmin + (b << shift));
        ks.push_back(kmin + (b << shift) - 1u);
    }
    if (range) { ks.push_back(kmin + 1u); ks.push_back(kmax - 1u); }
    std::sort(ks.begin(), ks.end());
    for (size_t i = 0; i < ks.size(); ++i) {
        const uint32_t d = dns_depth_bucket(ks[i], kmin, shift);
        REQUIRE(d < B);
        if (i) {
            const uint32_t dp = dns_depth_bucket(ks[i - 1], kmin, shift);
            REQUIRE(dp <= d);
            if (dp == d) REQUIRE(((ks[i] - kmin) >> shift) == ((ks[i - 1] - kmin) >> shift));
        }
    }
    return 0;
}

// binning.hip's route on the host: stable partition by bucket, then stable LSD passes inside every bucket
static int check_sort(uint32_t kmin, uint32_t kmax, int bbits, int n)
{
    typedef std::pair<uint32_t, uint32_t> P;
    std::vector<P> in(n);
    const uint32_t range = kmax - kmin;
    for (int i = 0; i < n; ++i) in[i] = P(i == 0 ? kmin : i == 1 ? kmax : kmin + (range ? rnd32() % range : 0u), (uint32_t)i);
    for (int i = 2; i + 1 < n; i += 3) in[i + 1].first = in[i].first;          // ties
    std::vector<P> want = in;
    std::stable_sort(want.begin(), want.end(), [](const P &a, const P &b) { return a.first < b.first; });
    const int shift = dns_depth_bucket_shift(kmin, kmax, bbits);
    const uint32_t B = 1u << bbits;
    std::vector<std::vector<P>> buckets(B);
    for (const P &p : in) buckets[dns_depth_bucket(p.first, kmin, shift)].push_back(p);
    const int passes = dns_depth_local_passes(shift), dbits = dns_depth_local_bits(shift);
    std::vector<P> got;
    for (auto &bk : buckets) {
        for (int p = 0; p < passes; ++p) {
            std::vector<std::vector<P>> dig(1u << dbits);
            for (const P &q : bk) dig[((q.first - kmin) >> (p * dbits)) & ((1u << dbits) - 1u)].push_back(q);
            bk.clear();
            for (auto &d : dig) bk.insert(bk.end(), d.begin(), d.end());
        }
        got.insert(got.end(), bk.begin(), bk.end());
    }
    REQUIRE(got == want);
    return 0;
}

int main()
{
    uint32_t kmin = 0, kmax = 0;
    int bbits = 9;
    // B from N: about N / 1024, a power of two in [512, 4096]
    REQUIRE(dns_depth_bucket_bits(0) == 9 && dns_depth_bucket_bits(524288) == 9 && dns_depth_bucket_bits(524289) == 10);
    REQUIRE(dns_depth_bucket_bits(1000000) == 10 && dns_depth_bucket_bits(5000000) == 12 && dns_depth_bucket_bits(2000000000) == 12);
    const uint32_t edges[][2] = {{0u, 0u}, {0u, 0xFFFFFFFFu}, {0x3C23D70Au, 0x3C23D70Au}, {0x3C23D70Au, 0x4E6E6B28u}, {1u, 0x80000000u},
                                 {0x40800000u, 0x408001FFu}, {0x40800000u, 0x40800200u}, {0x40800000u, 0x40800201u}, {0x7FFFFFFFu, 0xFFFFFFFFu},
                                 {0xFFFFFFFEu, 0xFFFFFFFFu}, {5u, 5u + 4095u}, {5u, 5u + 4096u}};
    for (bbits = 9; bbits <= 12; ++bbits) {
        for (const auto &e : edges) {
            kmin = e[0]; kmax = e[1];
            if (check_map(kmin, kmax, bbits) || check_sort(kmin, kmax, bbits, 3000)) return 1;
        }
        for (int t = 0; t < 4000; ++t) {
            uint32_t a = rnd32() >> (rnd32() % 32), b = rnd32() >> (rnd32() % 32);
            if (t % 3 == 0) b = a + (rnd32() >> (8 + rnd32() % 24));           // close pairs
            if (b < a) std::swap(a, b);
            kmin = a; kmax = b;
            if (check_map(kmin, kmax, bbits)) return 1;
            if (t % 40 == 0 && check_sort(kmin, kmax, bbits, 2000)) return 1;
        }
    }
    printf("ok\n");
    return 0;
}
'''


def test_bucket_map_is_monotone_and_buckets_share_their_high_bits(tmp_path):
    src = tmp_path / "buckets.cpp"
    src.write_text(SRC)
    exe = tmp_path / "buckets"
    inc = os.path.join(ROOT, "dn-splatter_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
