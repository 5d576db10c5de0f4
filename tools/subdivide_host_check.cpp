// subdivide_host_check.cpp — the host side of the mesh subdivision under AddressSanitizer and UBSan, on a machine without a GPU: the
// argument validation of the calls of subdivide.hip (every call here returns before anything touches a device, so the NULL / host
// pointers are never dereferenced) and the scratch query against its formula at the sizes where a 32-bit product would wrap.  A
// stand-alone program: it touches no device and loads nothing into Python.
//
//   cd dn-splatter_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       subdivide.hip ../../tools/subdivide_host_check.cpp -o /tmp/subdivide_host_check && /tmp/subdivide_host_check
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../include/dnsplat.h"

static int failures = 0;
#define EXPECT(call, want)                                                                      \
    do {                                                                                        \
        const long long got__ = (long long)(call);                                              \
        if (got__ != (long long)(want)) {                                                       \
            std::printf("line %d: %s = %lld, expected %lld\n", __LINE__, #call, got__, (long long)(want)); \
            ++failures;                                                                         \
        }                                                                                       \
    } while (0)

static double host_words[8];                                // stands in for every device pointer; nothing may read or write it
static const long long INT_MAX_LL = 0x7fffffffLL, MAX_T = INT_MAX_LL / 4;

static dnsplat_subdivide_args good()
{
    dnsplat_subdivide_args a;
    std::memset(&a, 0, sizeof a);
    a.V = 9; a.T = 5;
    a.vertices = host_words;
    a.triangles = a.origin = (const int32_t *)host_words;
    a.max_edge = 0.5;
    a.scratch = host_words;
    a.scratch_bytes = dnsplat_subdivide_scratch_bytes(9, 5);
    a.counts = (int64_t *)host_words;
    a.status = (int32_t *)host_words;
    a.vertex_base = 3; a.cap_v = 4; a.cap_t = 2; a.cap_long = 3; a.cap_mid = 7;
    a.out_vertices = a.next_vertices = host_words;
    a.out_triangles = a.out_index = a.next_triangles = a.next_origin = (int32_t *)host_words;
    return a;
}

static long long blocks(long long n) { return (n + 255) / 256; }
static long long formula(long long V, long long T) { return 64 * T + 4 * V + 4 * (2 * blocks(T) + blocks(V) + blocks(3 * T)); }

int main()
{
    const long long sizes[][2] = {{1, 1}, {8, 12}, {255, 256}, {257, 85}, {66000, 131073}, {40000000, 33554433}, {INT_MAX_LL, MAX_T}};
    for (const auto &s : sizes) EXPECT(dnsplat_subdivide_scratch_bytes((int32_t)s[0], (int32_t)s[1]), formula(s[0], s[1]));
    EXPECT(dnsplat_subdivide_scratch_bytes(0, 5), 0);
    EXPECT(dnsplat_subdivide_scratch_bytes(5, 0), 0);
    EXPECT(dnsplat_subdivide_scratch_bytes(5, -1), 0);
    EXPECT(dnsplat_subdivide_scratch_bytes(5, (int32_t)(MAX_T + 1)), 0);

    EXPECT(dnsplat_subdivide_count(nullptr, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_subdivide_emit(nullptr, nullptr), DNSPLAT_ERR_INVALID_ARG);
    dnsplat_subdivide_args a = good();
    a.scratch_bytes -= 1;
    EXPECT(dnsplat_subdivide_count(&a, nullptr), DNSPLAT_ERR_WORKSPACE);
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_WORKSPACE);
    a = good(); a.scratch = (char *)host_words + 4;
    EXPECT(dnsplat_subdivide_count(&a, nullptr), DNSPLAT_ERR_WORKSPACE);
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_WORKSPACE);
    const double bad_edges[] = {0.0, -1.0, INFINITY, NAN};
    for (double e : bad_edges) {
        a = good(); a.max_edge = e;
        EXPECT(dnsplat_subdivide_count(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
        EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    }
    a = good(); a.V = 0;
    EXPECT(dnsplat_subdivide_count(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.T = -3;
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.T = (int32_t)(MAX_T + 1); a.scratch_bytes = (size_t)1 << 62;
    EXPECT(dnsplat_subdivide_count(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED);
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED);
    a = good(); a.status = nullptr;
    EXPECT(dnsplat_subdivide_count(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.cap_mid = -1;
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.next_origin = nullptr;
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.out_index = nullptr;
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    // the limits, each one past and exactly at it (at it, the short scratch answers next: still no device)
    a = good(); a.cap_long = MAX_T / 4 + 1;
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED);
    a = good(); a.cap_long = MAX_T / 4; a.scratch_bytes -= 1;
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_WORKSPACE);
    a = good(); a.cap_mid = INT_MAX_LL - 8;
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED);
    a = good(); a.cap_mid = INT_MAX_LL - 9; a.scratch_bytes -= 1;
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_WORKSPACE);
    a = good(); a.cap_v = INT_MAX_LL - 2;
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED);
    a = good(); a.vertex_base = INT64_MAX; a.cap_v = 1;
    EXPECT(dnsplat_subdivide_emit(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED);
    for (double w : host_words) EXPECT(w != 0.0, 0);
    std::printf(failures ? "subdivide host check: %d FAILURES\n" : "subdivide host check: ok\n", failures);
    return failures ? 1 : 0;
}
