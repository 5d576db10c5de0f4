// cloud_filter_host_check.cpp — the host side of the point-cloud filters under AddressSanitizer and UBSan, on a machine without a GPU:
// the argument validation of the six calls of cloudfilter.hip (every call here returns before anything touches a device, so the NULL /
// host pointers are never dereferenced) and the two scratch queries against the layout arithmetic, at the sizes where a 32-bit product
// would wrap.  A stand-alone program: it touches no device and loads nothing into Python.
//
//   cd dn-splatter_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       cloudfilter.hip ../../tools/cloud_filter_host_check.cpp -o /tmp/cloud_filter_host_check && /tmp/cloud_filter_host_check
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
static const int MAX_N = 2147483647 / 2;

static dnsplat_cloud_outlier_args good_outlier()
{
    dnsplat_cloud_outlier_args a;
    std::memset(&a, 0, sizeof a);
    a.N = 300; a.nb_neighbors = 20; a.std_ratio = 2.0;
    a.points = (const float *)host_words;
    a.index = host_words;
    a.scratch = host_words;
    a.scratch_bytes = dnsplat_cloud_outlier_scratch_bytes(300);
    a.avg = host_words;
    a.stats = host_words;
    a.capacity = 4;
    a.ind = (int64_t *)host_words;
    return a;
}

static dnsplat_voxel_args good_voxel()
{
    dnsplat_voxel_args a;
    std::memset(&a, 0, sizeof a);
    a.N = 300; a.voxel_size = 0.05;
    a.points = a.normals = a.colors = (const float *)host_words;
    a.scratch = host_words;
    a.scratch_bytes = dnsplat_voxel_scratch_bytes(300, 2);
    a.counts = (int64_t *)host_words;
    a.voxel_of = a.out_counts = (int32_t *)host_words;
    a.cap_v = 4;
    a.out_points = a.out_normals = a.out_colors = host_words;
    return a;
}

int main()
{
    // ---- the scratch queries
    for (int n : {1, 20, 256, 257, 66000, 2000000, MAX_N, 2147483647}) {
        const size_t N = (size_t)n, nb = (N + 255) / 256;
        EXPECT(dnsplat_cloud_outlier_scratch_bytes(n), nb * 36);
        if (n <= MAX_N)
            for (int k = 0; k <= 2; ++k) EXPECT(dnsplat_voxel_scratch_bytes(n, k), 32 + 2 * N * 12 + N * (8 * (4 + 3 * (size_t)k) + 4) + nb * 4 + 256 * 12);
    }
    for (int bad : {0, -1, -2147483647 - 1}) {
        EXPECT(dnsplat_cloud_outlier_scratch_bytes(bad), 0);
        EXPECT(dnsplat_voxel_scratch_bytes(bad, 0), 0);
    }
    EXPECT(dnsplat_voxel_scratch_bytes(MAX_N + 1, 0), 0);
    EXPECT(dnsplat_voxel_scratch_bytes(2147483647, 2), 0);
    EXPECT(dnsplat_voxel_scratch_bytes(5, 3), 0);
    EXPECT(dnsplat_voxel_scratch_bytes(5, -1), 0);

    // ---- the outlier calls
    typedef int (*outlier_fn)(const dnsplat_cloud_outlier_args *, dnsplat_stream_t);
    const outlier_fn with_scratch[3] = {dnsplat_cloud_outlier_stats, dnsplat_cloud_outlier_count, dnsplat_cloud_outlier_emit};
    dnsplat_cloud_outlier_args a = good_outlier();
    EXPECT(dnsplat_cloud_neighbor_mean(nullptr, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a.points = nullptr; EXPECT(dnsplat_cloud_neighbor_mean(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_outlier();
    a.index = nullptr;  EXPECT(dnsplat_cloud_neighbor_mean(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_outlier();
    a.avg = nullptr;    EXPECT(dnsplat_cloud_neighbor_mean(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_outlier();
    for (int bad : {0, -1, -2147483647 - 1}) {
        a.N = bad;            EXPECT(dnsplat_cloud_neighbor_mean(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_outlier();
        a.nb_neighbors = bad; EXPECT(dnsplat_cloud_neighbor_mean(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_outlier();
    }
    a.nb_neighbors = DNSPLAT_KNN_MAX_K + 1; EXPECT(dnsplat_cloud_neighbor_mean(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED); a = good_outlier();
    a.nb_neighbors = 2147483647;            EXPECT(dnsplat_cloud_neighbor_mean(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED); a = good_outlier();
    for (outlier_fn fn : with_scratch) {
        EXPECT(fn(nullptr, nullptr), DNSPLAT_ERR_INVALID_ARG);
        a.scratch = nullptr; EXPECT(fn(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_outlier();
        a.avg = nullptr;     EXPECT(fn(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_outlier();
        a.stats = nullptr;   EXPECT(fn(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_outlier();
        for (int bad : {0, -1, -2147483647 - 1}) { a.N = bad; EXPECT(fn(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_outlier(); }
        a.scratch_bytes -= 1;               EXPECT(fn(&a, nullptr), DNSPLAT_ERR_WORKSPACE); a = good_outlier();
        a.scratch = (char *)host_words + 4; EXPECT(fn(&a, nullptr), DNSPLAT_ERR_WORKSPACE); a = good_outlier();
        a.N = 2147483647; a.scratch_bytes = dnsplat_cloud_outlier_scratch_bytes(a.N) - 1;      // the largest cloud: the sizes stay inside size_t
        EXPECT(fn(&a, nullptr), DNSPLAT_ERR_WORKSPACE); a = good_outlier();
    }
    a.std_ratio = std::nan(""); EXPECT(dnsplat_cloud_outlier_stats(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_outlier();
    a.capacity = -1;            EXPECT(dnsplat_cloud_outlier_emit(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_outlier();
    a.ind = nullptr;            EXPECT(dnsplat_cloud_outlier_emit(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_outlier();   // a capacity without its buffer
    a.ind = nullptr; a.capacity = 0; EXPECT(dnsplat_cloud_outlier_emit(&a, nullptr), DNSPLAT_OK);                              // nothing to write: no launch

    // ---- the voxel calls
    typedef int (*voxel_fn)(const dnsplat_voxel_args *, dnsplat_stream_t);
    const voxel_fn voxel_calls[2] = {dnsplat_voxel_count, dnsplat_voxel_emit};
    for (voxel_fn fn : voxel_calls) {
        EXPECT(fn(nullptr, nullptr), DNSPLAT_ERR_INVALID_ARG);
        dnsplat_voxel_args v = good_voxel();
        v.points = nullptr;   EXPECT(fn(&v, nullptr), DNSPLAT_ERR_INVALID_ARG); v = good_voxel();
        v.scratch = nullptr;  EXPECT(fn(&v, nullptr), DNSPLAT_ERR_INVALID_ARG); v = good_voxel();
        v.counts = nullptr;   EXPECT(fn(&v, nullptr), DNSPLAT_ERR_INVALID_ARG); v = good_voxel();
        v.voxel_of = nullptr; EXPECT(fn(&v, nullptr), DNSPLAT_ERR_INVALID_ARG); v = good_voxel();
        for (int bad : {0, -1, -2147483647 - 1}) { v.N = bad; EXPECT(fn(&v, nullptr), DNSPLAT_ERR_INVALID_ARG); v = good_voxel(); }
        for (double bad : {0.0, -0.05, (double)INFINITY, std::nan("")}) { v.voxel_size = bad; EXPECT(fn(&v, nullptr), DNSPLAT_ERR_INVALID_ARG); v = good_voxel(); }
        v.scratch_bytes = ~(size_t)0;
        v.N = MAX_N + 1;  EXPECT(fn(&v, nullptr), DNSPLAT_ERR_UNSUPPORTED);
        v.N = 2147483647; EXPECT(fn(&v, nullptr), DNSPLAT_ERR_UNSUPPORTED);
        v = good_voxel();
        v.scratch_bytes -= 1;               EXPECT(fn(&v, nullptr), DNSPLAT_ERR_WORKSPACE); v = good_voxel();
        v.scratch = (char *)host_words + 4; EXPECT(fn(&v, nullptr), DNSPLAT_ERR_WORKSPACE); v = good_voxel();
        v.N = MAX_N; v.scratch_bytes = dnsplat_voxel_scratch_bytes(MAX_N, 2) - 1;              // the largest cloud: the sizes stay inside size_t
        EXPECT(fn(&v, nullptr), DNSPLAT_ERR_WORKSPACE);
    }
    dnsplat_voxel_args v = good_voxel();
    v.cap_v = -1;            EXPECT(dnsplat_voxel_emit(&v, nullptr), DNSPLAT_ERR_INVALID_ARG); v = good_voxel();
    v.out_points = nullptr;  EXPECT(dnsplat_voxel_emit(&v, nullptr), DNSPLAT_ERR_INVALID_ARG); v = good_voxel();
    v.out_normals = nullptr; EXPECT(dnsplat_voxel_emit(&v, nullptr), DNSPLAT_ERR_INVALID_ARG); v = good_voxel();
    v.out_colors = nullptr;  EXPECT(dnsplat_voxel_emit(&v, nullptr), DNSPLAT_ERR_INVALID_ARG); v = good_voxel();
    v.cap_v = 0;             EXPECT(dnsplat_voxel_emit(&v, nullptr), DNSPLAT_OK);                                              // nothing to write: no launch

    for (double w : host_words) failures += w != 0.0;
    std::printf(failures ? "cloud_filter_host_check: %d FAILURES\n" : "cloud_filter_host_check: ok\n", failures);
    return failures != 0;
}
