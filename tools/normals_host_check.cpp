// normals_host_check.cpp — the host side of the point-cloud normals under AddressSanitizer and UBSan, on a machine without a GPU: the
// argument validation of dnsplat_cloud_normals (every call here returns before anything touches a device, so the NULL / host pointers
// are never dereferenced), the scratch query against its stated 16 bytes, and the solve of normals_solve.h on the host: a plane, a
// zero covariance, fewer than three neighbours, both signs.  A stand-alone program: it touches no device and loads nothing into Python.
//
//   cd dn-splatter_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       normals.hip ../../tools/normals_host_check.cpp -o /tmp/normals_host_check && /tmp/normals_host_check
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../include/dnsplat.h"
#include "../dn-splatter_amd/csrc/normals_solve.h"

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

static dnsplat_cloud_normals_args good()
{
    dnsplat_cloud_normals_args a;
    std::memset(&a, 0, sizeof a);
    a.N = 9; a.knn = 30;
    a.points = (const float *)host_words;
    a.index = host_words;
    a.radius = 0.1;
    a.orient = 1;
    a.toward[0] = 0.5; a.toward[1] = -1.0; a.toward[2] = 2.0;
    a.scratch = host_words;
    a.scratch_bytes = dnsplat_cloud_normals_scratch_bytes(9, 30);
    a.normals = a.covariance = host_words;
    a.neighbors = a.count = a.status = (int32_t *)host_words;
    return a;
}

int main()
{
    const int sizes[][2] = {{1, 3}, {2, 30}, {257, 200}, {3000000, 256}, {0x7fffffff, 3}};
    for (const auto &s : sizes) EXPECT(dnsplat_cloud_normals_scratch_bytes(s[0], s[1]), 16);
    const int bad_sizes[][2] = {{0, 30}, {-1, 30}, {5, 2}, {5, 0}, {5, -1}, {5, 257}};
    for (const auto &s : bad_sizes) EXPECT(dnsplat_cloud_normals_scratch_bytes(s[0], s[1]), 0);

    EXPECT(dnsplat_cloud_normals(nullptr, nullptr), DNSPLAT_ERR_INVALID_ARG);
    dnsplat_cloud_normals_args a = good();
    a.points = nullptr;
    EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.index = nullptr;
    EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.normals = nullptr;
    EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.status = nullptr;
    EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.scratch = nullptr;
    EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.N = 0;
    EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.radius = NAN;
    EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.orient = 2;
    EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good(); a.toward[2] = NAN;
    EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    const int bad_knn[] = {2, 257, 0, -3};
    for (int k : bad_knn) {
        a = good(); a.knn = k;
        EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED);
    }
    const int edge_knn[] = {3, 256};                        // the limits pass; the short scratch answers next: still no device
    for (int k : edge_knn) {
        a = good(); a.knn = k; a.scratch_bytes -= 1;
        EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_WORKSPACE);
    }
    a = good(); a.scratch = (char *)host_words + 4;
    EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_WORKSPACE);
    a = good(); a.covariance = nullptr; a.neighbors = nullptr; a.count = nullptr; a.scratch_bytes = 0;   // the optional outputs may be NULL
    EXPECT(dnsplat_cloud_normals(&a, nullptr), DNSPLAT_ERR_WORKSPACE);
    for (double w : host_words) EXPECT(w != 0.0, 0);

    // the solve on the host
    double n[3];
    const double plane[6] = {2.0, 0.5, 0.0, 1.0, 0.0, 0.0};              // no extent along z
    nm_normal(plane, 30, n);
    EXPECT(n[0] == 0.0 && n[1] == 0.0 && n[2] == 1.0, 1);
    nm_normal(plane, 2, n);
    EXPECT(n[0] == 0.0 && n[1] == 0.0 && n[2] == 1.0, 1);
    const double zero[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    nm_normal(zero, 30, n);
    EXPECT(n[0] == 0.0 && n[1] == 0.0 && n[2] == 1.0, 1);
    const double tilted[6] = {1.0, 0.0, 0.5, 1.0, 0.25, 0.3125};         // z = x / 2 + y / 4 over unit variances
    nm_normal(tilted, 30, n);
    const double len = std::sqrt(0.25 + 0.0625 + 1.0);
    const double toward[3] = {0.0, 0.0, 5.0}, away[3] = {0.0, 0.0, -5.0}, p[3] = {0.0, 0.0, 0.0};
    nm_orient(n, true, toward, p);
    EXPECT(std::fabs(n[0] + 0.5 / len) < 1e-15 && std::fabs(n[1] + 0.25 / len) < 1e-15 && std::fabs(n[2] - 1.0 / len) < 1e-15, 1);
    nm_orient(n, true, away, p);
    EXPECT(n[2] < 0.0, 1);
    nm_orient(n, false, toward, p);
    EXPECT(n[2] > 0.0, 1);                                               // canonical: the largest component is positive
    std::printf(failures ? "normals host check: %d FAILURES\n" : "normals host check: ok\n", failures);
    return failures ? 1 : 0;
}
