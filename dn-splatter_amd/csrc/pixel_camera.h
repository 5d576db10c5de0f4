// pixel_camera.h — THE back-projection of a pixel to its world point and THE crop-box test, for pointcloud.hip (pc_row) and
// levelset.hip (ls_point, ls_points_kernel).  Both files are compiled without contraction and every operation below is an explicit
// round-to-nearest intrinsic: the level-set points start from the very bits dnsplat_backproject_points appends.
#pragma once

#include "splat_common.h"

namespace {

struct DnsPixelCamera {
    int W, H;
    long long P;                  // W H
    const float *depth;           // [P]
    const uint8_t *mask;          // [P] or null: a pixel outside it has depth 0
    float fx, fy, cx, cy;
    const float *xform;           // [21]: A = the inverse rotation row-major, t, R
};

// from any of the argument structs of dnsplat.h that describe a frame
template <typename Args>
DnsPixelCamera dns_pixel_camera(const Args &a)
{
    return DnsPixelCamera{a.width, a.height, (long long)a.width * a.height, a.depth, a.mask, a.fx, a.fy, a.cx, a.cy, a.xform};
}

__device__ __forceinline__ float dns_pixel_depth(const DnsPixelCamera &c, long long i) { return (c.mask && !c.mask[i]) ? 0.f : c.depth[i]; }

// the world point of pixel i at depth d.  camera_utils.py:129-131: (coords - c) * depth / f, the pixel centre at + 0.5; then p A + t
__device__ __forceinline__ void dns_pixel_point(const DnsPixelCamera &c, long long i, float d, float p[3])
{
    const int v = (int)(i / c.W), u = (int)(i - (long long)v * c.W);
    const float px = __fdiv_rn(__fmul_rn(__fsub_rn((float)u + 0.5f, c.cx), d), c.fx);
    const float py = __fdiv_rn(__fmul_rn(__fsub_rn((float)v + 0.5f, c.cy), d), c.fy);
    const float *A = c.xform, *T = c.xform + 9;
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(px, A[a]), __fmul_rn(py, A[3 + a])), __fmul_rn(d, A[6 + a])), T[a]);
}

// crop = [15] floats: the world -> box affine B [3,4] row-major and the half extents h.  |B x + b| < h on every axis: strict on both
// faces; a nan coordinate is outside
__device__ __forceinline__ bool dns_in_crop_box(const float *__restrict__ crop, const float x[3])
{
    const float *B = crop, *h = crop + 12;
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float q = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(B[4 * a], x[0]), __fmul_rn(B[4 * a + 1], x[1])), __fmul_rn(B[4 * a + 2], x[2])),
                                  B[4 * a + 3]);
        in = in && fabsf(q) < h[a];
    }
    return in;
}

}  // namespace
