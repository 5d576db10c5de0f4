// mesh_clusters_host_check.cpp — the host side of the mesh cluster filter under AddressSanitizer and UBSan, on a machine without a GPU:
// the argument validation of dnsplat_mesh_clusters, dnsplat_mesh_filter_count and dnsplat_mesh_filter_emit (every call here returns
// before anything touches a device, so the NULL / host pointers are never dereferenced) and the two scratch queries against the layout
// arithmetic, at the sizes where a 32-bit product would wrap.  A stand-alone program: it touches no device and loads nothing into Python.
//
//   cd dn-splatter_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       meshclusters.hip ../../tools/mesh_clusters_host_check.cpp -o /tmp/mesh_clusters_host_check && /tmp/mesh_clusters_host_check
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
static const int MAX_T = 2147483647 / 4;

static dnsplat_mesh_clusters_args good_clusters()
{
    dnsplat_mesh_clusters_args a;
    std::memset(&a, 0, sizeof a);
    a.V = 9; a.T = 8;
    a.triangles = (const int32_t *)host_words;
    a.scratch = host_words;
    a.scratch_bytes = dnsplat_mesh_clusters_scratch_bytes(9, 8);
    a.labels = a.sizes = a.status = (int32_t *)host_words;
    a.counts = (int64_t *)host_words;
    return a;
}

static dnsplat_mesh_filter_args good_filter()
{
    dnsplat_mesh_filter_args a;
    std::memset(&a, 0, sizeof a);
    a.V = 9; a.T = 8;
    a.triangles = a.labels = a.sizes = (const int32_t *)host_words;
    a.cluster_counts = (const int64_t *)host_words;
    a.keep_largest = a.min_triangles = 50;
    a.scratch = host_words;
    a.scratch_bytes = dnsplat_mesh_filter_scratch_bytes(9, 8);
    a.threshold = a.vertex_index = a.out_triangles = a.status = (int32_t *)host_words;
    a.counts = (int64_t *)host_words;
    a.cap_v = a.cap_t = 4;
    return a;
}

int main()
{
    // ---- the scratch queries: 4 T slots of 12 bytes, one counter, three int32 per triangle, one per block of 256
    const int sizes[][2] = {{1, 1}, {9, 8}, {4800, 9344}, {200000, 70000}, {18600000, 37100000}, {2147483647, MAX_T}};
    for (const auto &s : sizes) {
        const size_t V = (size_t)s[0], T = (size_t)s[1], bt = (T + 255) / 256, bv = (V + 255) / 256;
        EXPECT(dnsplat_mesh_clusters_scratch_bytes(s[0], s[1]), 4 * T * 12 + 8 + 3 * T * 4 + bt * 4);
        EXPECT(dnsplat_mesh_filter_scratch_bytes(s[0], s[1]), (size_t)(3 * 2048 + 2) * 8 + (V + bt + bv) * 4 + T);
    }
    EXPECT(dnsplat_mesh_filter_scratch_bytes(2147483647, 2147483647), (size_t)(3 * 2048 + 2) * 8 + ((size_t)2147483647 + 2 * 8388608) * 4 + 2147483647);
    for (int bad : {0, -1, -2147483647 - 1}) {
        EXPECT(dnsplat_mesh_clusters_scratch_bytes(bad, 5), 0);
        EXPECT(dnsplat_mesh_clusters_scratch_bytes(5, bad), 0);
        EXPECT(dnsplat_mesh_filter_scratch_bytes(bad, 5), 0);
        EXPECT(dnsplat_mesh_filter_scratch_bytes(5, bad), 0);
    }
    EXPECT(dnsplat_mesh_clusters_scratch_bytes(5, MAX_T + 1), 0);
    EXPECT(dnsplat_mesh_clusters_scratch_bytes(5, 2147483647), 0);

    // ---- dnsplat_mesh_clusters
    EXPECT(dnsplat_mesh_clusters(nullptr, nullptr), DNSPLAT_ERR_INVALID_ARG);
    dnsplat_mesh_clusters_args a = good_clusters();
    a.triangles = nullptr; EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_clusters();
    a.scratch = nullptr;   EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_clusters();
    a.labels = nullptr;    EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_clusters();
    a.sizes = nullptr;     EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_clusters();
    a.counts = nullptr;    EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_clusters();
    a.status = nullptr;    EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_clusters();
    for (int bad : {0, -1, -2147483647 - 1}) {
        a.V = bad; EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_clusters();
        a.T = bad; EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_clusters();
    }
    a.scratch_bytes = ~(size_t)0;
    a.T = MAX_T + 1;     EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED);
    a.T = 2147483647;    EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED);
    a = good_clusters();
    a.scratch_bytes -= 1; EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_WORKSPACE); a = good_clusters();
    a.scratch = (char *)host_words + 4; EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_WORKSPACE);
    a = good_clusters();
    a.T = MAX_T; a.scratch_bytes = dnsplat_mesh_clusters_scratch_bytes(9, MAX_T) - 1;       // the largest mesh: the sizes stay inside size_t
    EXPECT(dnsplat_mesh_clusters(&a, nullptr), DNSPLAT_ERR_WORKSPACE);

    // ---- dnsplat_mesh_filter_count / dnsplat_mesh_filter_emit
    int (*const entries[2])(const dnsplat_mesh_filter_args *, dnsplat_stream_t) = {dnsplat_mesh_filter_count, dnsplat_mesh_filter_emit};
    for (auto fn : entries) {
        EXPECT(fn(nullptr, nullptr), DNSPLAT_ERR_INVALID_ARG);
        dnsplat_mesh_filter_args f = good_filter();
        f.triangles = nullptr;      EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
        f.labels = nullptr;         EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
        f.sizes = nullptr;          EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
        f.cluster_counts = nullptr; EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
        f.scratch = nullptr;        EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
        f.threshold = nullptr;      EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
        f.counts = nullptr;         EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
        for (int bad : {0, -1, -2147483647 - 1}) {
            f.V = bad;             EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
            f.T = bad;             EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
            f.keep_largest = bad;  EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
            f.min_triangles = bad; EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
        }
        f.scratch_bytes -= 1;      EXPECT(fn(&f, nullptr), DNSPLAT_ERR_WORKSPACE); f = good_filter();
        f.scratch = (char *)host_words + 4; EXPECT(fn(&f, nullptr), DNSPLAT_ERR_WORKSPACE); f = good_filter();
        f.V = f.T = 2147483647; f.scratch_bytes = dnsplat_mesh_filter_scratch_bytes(f.V, f.T) - 1;
        EXPECT(fn(&f, nullptr), DNSPLAT_ERR_WORKSPACE);
        if (fn == dnsplat_mesh_filter_emit) {
            f = good_filter();
            f.status = nullptr;        EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
            f.cap_v = -1;              EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
            f.cap_t = -1;              EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();
            f.vertex_index = nullptr;  EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG); f = good_filter();   // a capacity without its buffer
            f.out_triangles = nullptr; EXPECT(fn(&f, nullptr), DNSPLAT_ERR_INVALID_ARG);
        }
    }
    for (double w : host_words) failures += w != 0.0;
    std::printf(failures ? "mesh_clusters_host_check: %d FAILURES\n" : "mesh_clusters_host_check: ok\n", failures);
    return failures != 0;
}
