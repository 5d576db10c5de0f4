// tsdf_host_check.cpp — the host side of the TSDF entry points under AddressSanitizer and UBSan, on a machine without a GPU: the argument
// validation of dnsplat_tsdf_integrate, dnsplat_tsdf_vertex_colors, dnsplat_mc_count_observed and dnsplat_mc_emit_observed (every call
// here returns before a launch, so the NULL / host pointers are never dereferenced) and dnsplat_mc_observed_scratch_bytes against the
// layout arithmetic.  A stand-alone program: it touches no device and loads nothing into Python.
//
//   cd dn-splatter_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tsdf.hip marching.hip ../../tools/tsdf_host_check.cpp -o /tmp/tsdf_host_check && /tmp/tsdf_host_check
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

static dnsplat_tsdf_args good_tsdf()
{
    dnsplat_tsdf_args a;
    std::memset(&a, 0, sizeof a);
    float *p = (float *)host_words;
    a.tsdf = a.weight = a.color = p;
    a.depth = a.rgb = a.ray_scale = p;
    a.w2c = host_words;
    a.nx = 2; a.ny = 3; a.nz = 4;
    a.voxel = 0.1; a.C = 1; a.width = 4; a.height = 4;
    a.fx = a.fy = 1.0;
    a.sdf_trunc = 0.03f; a.depth_trunc = 20.f;
    return a;
}

int main()
{
    // ---- dnsplat_tsdf_integrate
    EXPECT(dnsplat_tsdf_integrate(nullptr, nullptr), DNSPLAT_ERR_INVALID_ARG);
    dnsplat_tsdf_args a = good_tsdf();
    a.tsdf = nullptr;       EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
    a.weight = nullptr;     EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
    a.w2c = nullptr;        EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
    a.depth = nullptr;      EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
    a.ray_scale = nullptr;  EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
    a.color = nullptr;      EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();   // rgb without color
    a.rgb = nullptr;        EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();   // color without rgb
    for (int bad : {0, -1, -2147483647 - 1}) {
        a.nx = bad;     EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
        a.ny = bad;     EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
        a.nz = bad;     EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
        a.C = bad;      EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
        a.width = bad;  EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
        a.height = bad; EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
    }
    a.nx = 2048; a.ny = 1024; a.nz = 1024;                  // 2^31 voxels
    EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a.nx = a.ny = a.nz = 2147483647;                        // the products stay inside long long
    EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG);
    a = good_tsdf();
    for (double bad : {0.0, -1.0, (double)NAN}) {
        a.voxel = bad;              EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
        a.sdf_trunc = (float)bad;   EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
        a.depth_trunc = (float)bad; EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_INVALID_ARG); a = good_tsdf();
    }
    a.width = 65536; a.height = 32768;                      // 2^31 pixels
    EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED);
    a.width = a.height = 2147483647;
    EXPECT(dnsplat_tsdf_integrate(&a, nullptr), DNSPLAT_ERR_UNSUPPORTED);

    // ---- dnsplat_tsdf_vertex_colors
    float *p = (float *)host_words;
    EXPECT(dnsplat_tsdf_vertex_colors(nullptr, 5, 6, 7, p, 4, p, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_tsdf_vertex_colors(p, 5, 6, 7, nullptr, 4, p, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_tsdf_vertex_colors(p, 5, 6, 7, p, 4, nullptr, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_tsdf_vertex_colors(p, 5, 6, 7, p, -1, p, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_tsdf_vertex_colors(p, 1, 6, 7, p, 4, p, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_tsdf_vertex_colors(p, 5, 6, 0, p, 4, p, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_tsdf_vertex_colors(p, 2048, 1024, 1024, p, 4, p, nullptr), DNSPLAT_ERR_INVALID_ARG);
    EXPECT(dnsplat_tsdf_vertex_colors(p, 5, 6, 7, p, 1LL << 31, p, nullptr), DNSPLAT_ERR_UNSUPPORTED);
    EXPECT(dnsplat_tsdf_vertex_colors(p, 5, 6, 7, nullptr, 0, nullptr, nullptr), DNSPLAT_OK);       // no vertex: no launch

    // ---- dnsplat_mc_observed_scratch_bytes: the unmasked layout plus one uint64 per 64 points, padded to 16 B
    const int shapes[][3] = {{2, 2, 2}, {5, 6, 7}, {17, 9, 33}, {64, 64, 64}, {512, 512, 512}, {1, 9, 9}, {2047, 1024, 1024}};
    for (const auto &s : shapes) {
        const long long n = (long long)s[0] * s[1] * s[2], words = (n + 63) / 64, blocks = (words + 1023) / 1024;
        const size_t base = (size_t)words * 32 + 2 * ((((size_t)words * 4 + 15) / 16) * 16) + (size_t)blocks * 32;
        EXPECT(dnsplat_mc_scratch_bytes(s[0], s[1], s[2]), base);
        EXPECT(dnsplat_mc_observed_scratch_bytes(s[0], s[1], s[2]), base + (((size_t)words * 8 + 15) / 16) * 16);
    }
    EXPECT(dnsplat_mc_observed_scratch_bytes(0, 5, 5), 0);
    EXPECT(dnsplat_mc_observed_scratch_bytes(2048, 1024, 1024), 0);
    EXPECT(dnsplat_mc_observed_scratch_bytes(2147483647, 2147483647, 2147483647), 0);

    // ---- dnsplat_mc_count_observed / dnsplat_mc_emit_observed
    int (*const entries[2])(const dnsplat_mc_observed_args *, dnsplat_stream_t) = {dnsplat_mc_count_observed, dnsplat_mc_emit_observed};
    for (auto fn : entries) {
        EXPECT(fn(nullptr, nullptr), DNSPLAT_ERR_INVALID_ARG);
        dnsplat_mc_observed_args m;
        std::memset(&m, 0, sizeof m);
        m.mc.volume = p; m.mc.scratch = host_words; m.mc.counts = (int64_t *)host_words; m.mc.status = (int32_t *)host_words;
        m.mc.nx = 5; m.mc.ny = 6; m.mc.nz = 7;
        m.mc.scratch_bytes = dnsplat_mc_observed_scratch_bytes(5, 6, 7);
        EXPECT(fn(&m, nullptr), DNSPLAT_ERR_INVALID_ARG);                       // no weight
        m.weight = p;
        m.mc.volume = nullptr;  EXPECT(fn(&m, nullptr), DNSPLAT_ERR_INVALID_ARG); m.mc.volume = p;
        m.mc.counts = nullptr;  EXPECT(fn(&m, nullptr), DNSPLAT_ERR_INVALID_ARG); m.mc.counts = (int64_t *)host_words;
        m.mc.scratch = nullptr; EXPECT(fn(&m, nullptr), DNSPLAT_ERR_INVALID_ARG); m.mc.scratch = host_words;
        m.mc.nz = 0;            EXPECT(fn(&m, nullptr), DNSPLAT_ERR_INVALID_ARG); m.mc.nz = 7;
        m.mc.scratch_bytes = dnsplat_mc_scratch_bytes(5, 6, 7);                 // the unmasked size lacks the plane
        EXPECT(fn(&m, nullptr), DNSPLAT_ERR_WORKSPACE);
        m.mc.scratch_bytes = dnsplat_mc_observed_scratch_bytes(5, 6, 7) - 1;
        EXPECT(fn(&m, nullptr), DNSPLAT_ERR_WORKSPACE);
        if (fn == dnsplat_mc_emit_observed) {
            m.mc.scratch_bytes += 1;
            m.mc.status = nullptr;  EXPECT(fn(&m, nullptr), DNSPLAT_ERR_INVALID_ARG); m.mc.status = (int32_t *)host_words;
            m.mc.cap_v = -1;        EXPECT(fn(&m, nullptr), DNSPLAT_ERR_INVALID_ARG);
            m.mc.cap_v = 1;         EXPECT(fn(&m, nullptr), DNSPLAT_ERR_INVALID_ARG);       // a capacity without its buffer
            m.mc.cap_v = 0; m.mc.cap_t = 1; EXPECT(fn(&m, nullptr), DNSPLAT_ERR_INVALID_ARG);
        }
    }
    for (double w : host_words) failures += w != 0.0;
    std::printf(failures ? "tsdf_host_check: %d FAILURES\n" : "tsdf_host_check: ok\n", failures);
    return failures != 0;
}
