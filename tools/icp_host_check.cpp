// icp_host_check.cpp — the host side of the mesh alignment under AddressSanitizer and UBSan, on a machine without a GPU: the argument
// validation of the calls of icp.hip (every call here returns before anything touches a device, so the NULL / host pointers are never
// dereferenced; the init matrix IS read on the host, 16 doubles) and the scratch query against its formula at the sizes where a 32-bit
// product would wrap.  A stand-alone program: it touches no device and loads nothing into Python.
//
//   cd dn-splatter_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       icp.hip ../../tools/icp_host_check.cpp -o /tmp/icp_host_check && /tmp/icp_host_check
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

static dnsplat_icp_args good()
{
    dnsplat_icp_args a;
    std::memset(&a, 0, sizeof a);
    a.M = 300; a.N = 200;
    a.source = a.target = (const float *)host_words;
    a.index = host_words;
    a.max_dist = 0.1; a.relative_fitness = 1e-6; a.relative_rmse = 1e-6; a.max_iteration = 30;
    a.state = host_words;
    a.trace = a.dist2 = host_words;
    a.idx = (int32_t *)host_words;
    a.scratch = host_words;
    a.scratch_bytes = dnsplat_icp_scratch_bytes(300);
    return a;
}

static double init[16];
static int call_begin(const dnsplat_icp_args *a) { return dnsplat_icp_begin(a, init, nullptr); }
static int call_iterate(const dnsplat_icp_args *a) { return dnsplat_icp_iterate(a, nullptr); }
static int call_run(const dnsplat_icp_args *a) { return dnsplat_icp_run(a, init, nullptr); }

int main()
{
    for (int k = 0; k < 16; ++k) init[k] = k % 5 == 0 ? 1.0 : 0.0;
    for (long long m : {1LL, 255LL, 256LL, 257LL, 66000LL, 2000000LL, 2147483647LL}) EXPECT(dnsplat_icp_scratch_bytes(m), 136 * ((m + 255) / 256));
    for (long long bad : {0LL, -1LL, 2147483648LL, -9223372036854775807LL - 1}) EXPECT(dnsplat_icp_scratch_bytes(bad), 0);

    typedef int (*fn_t)(const dnsplat_icp_args *);
    for (fn_t fn : {call_begin, call_iterate, call_run}) {
        EXPECT(fn(nullptr), DNSPLAT_ERR_INVALID_ARG);
        dnsplat_icp_args a = good();
        a.source = nullptr;  EXPECT(fn(&a), DNSPLAT_ERR_INVALID_ARG); a = good();
        a.target = nullptr;  EXPECT(fn(&a), DNSPLAT_ERR_INVALID_ARG); a = good();
        a.index = nullptr;   EXPECT(fn(&a), DNSPLAT_ERR_INVALID_ARG); a = good();
        a.state = nullptr;   EXPECT(fn(&a), DNSPLAT_ERR_INVALID_ARG); a = good();
        a.scratch = nullptr; EXPECT(fn(&a), DNSPLAT_ERR_INVALID_ARG); a = good();
        for (long long bad : {0LL, -1LL, -9223372036854775807LL - 1}) { a.M = bad; EXPECT(fn(&a), DNSPLAT_ERR_INVALID_ARG); a = good(); }
        for (int bad : {0, -1, -2147483647 - 1}) { a.N = bad; EXPECT(fn(&a), DNSPLAT_ERR_INVALID_ARG); a = good(); }
        for (double bad : {0.0, -0.1, (double)INFINITY, std::nan("")}) { a.max_dist = bad; EXPECT(fn(&a), DNSPLAT_ERR_INVALID_ARG); a = good(); }
        a.relative_fitness = std::nan(""); EXPECT(fn(&a), DNSPLAT_ERR_INVALID_ARG); a = good();
        a.relative_rmse = std::nan("");    EXPECT(fn(&a), DNSPLAT_ERR_INVALID_ARG); a = good();
        for (int bad : {-1, -2147483647 - 1}) { a.max_iteration = bad; EXPECT(fn(&a), DNSPLAT_ERR_INVALID_ARG); a = good(); }
        a.M = 2147483648LL; a.scratch_bytes = ~(size_t)0; EXPECT(fn(&a), DNSPLAT_ERR_UNSUPPORTED); a = good();
        a.scratch_bytes -= 1;               EXPECT(fn(&a), DNSPLAT_ERR_WORKSPACE); a = good();
        a.scratch = (char *)host_words + 4; EXPECT(fn(&a), DNSPLAT_ERR_WORKSPACE); a = good();
        a.state = (char *)host_words + 4;   EXPECT(fn(&a), DNSPLAT_ERR_WORKSPACE); a = good();
        a.M = 2147483647LL; a.scratch_bytes = dnsplat_icp_scratch_bytes(a.M) - 1;              // the largest cloud: the sizes stay inside size_t
        EXPECT(fn(&a), DNSPLAT_ERR_WORKSPACE);
    }
    const dnsplat_icp_args a = good();
    for (int k : {0, 7, 15})
        for (double bad : {(double)INFINITY, -(double)INFINITY, std::nan("")}) {
            const double was = init[k];
            init[k] = bad;
            EXPECT(call_begin(&a), DNSPLAT_ERR_INVALID_ARG);
            EXPECT(call_run(&a), DNSPLAT_ERR_INVALID_ARG);
            init[k] = was;
        }

    const float *p = (const float *)host_words;
    float *out = (float *)host_words;
    EXPECT(dnsplat_transform_points(5, nullptr, host_words, out, 0, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_transform_points(5, p, nullptr, out, 0, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_transform_points(5, p, host_words, nullptr, 1, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_transform_points(-1, p, host_words, out, 0, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_transform_points(2147483648LL, p, host_words, out, 0, nullptr), DNSPLAT_ERR_UNSUPPORTED);
    EXPECT(dnsplat_transform_points(0, nullptr, host_words, nullptr, 0, nullptr), DNSPLAT_OK);                                   // nothing to move: no launch
    EXPECT(dnsplat_knn_points(0, host_words, out, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_knn_points(-1, host_words, out, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_knn_points(5, nullptr, out, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_knn_points(5, host_words, nullptr, nullptr), DNSPLAT_ERR_INVALID_ARG);

    for (double w : host_words) failures += w != 0.0;
    std::printf(failures ? "icp_host_check: %d FAILURES\n" : "icp_host_check: ok\n", failures);
    return failures != 0;
}
