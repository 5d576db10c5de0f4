// tsdf.hip — TSDF fusion of depth (and colour) frames into a dense, bounded volume, and the colours of a mesh extracted from it: the
// frames -> volume step of the reference's Open3DTSDFFusion exporter (export_mesh.py:931-1047), which copies every rendered frame to
// the host and fuses it there with Open3D.  The rule below is restated from memory of Open3D's UniformTSDFVolume::Integrate as that
// exporter calls it (depth_scale = 1, RGB8, convert_rgb_to_intensity = False).  IT IS THIS PROJECT'S DEFINITION, PARITY UNPINNED
// AGAINST Open3D (absent here); torch_tsdf.py states it in PyTorch and the kernels are held to that file with exact equality.
//
// Volume: tsdf, weight float32 [nx,ny,nz], colour float32 [nx,ny,nz,3] or NULL, the last axis fastest; the sample point of voxel
// (i, j, k) is origin + voxel * (i, j, k) in float64 — the lattice coordinates of marching.hip.  The caller zeroes the arrays once;
// calls accumulate.  Per voxel, the C cameras of a call in ascending order (no contraction anywhere, every operation rounded once):
//   1  p_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k in float64 (w2c: the [R | t] rows of torch_mesh_cull.opencv_w2c); skip if !(p.z > 0);
//   2  uf = ((fx p.x) / p.z + cx) + pixel_offset, vf likewise, float64; skip unless 0.0001 <= uf < W - 0.0001 and 0.0001 <= vf < H - 0.0001
//      (a NaN skips); u = (int)uf, v = (int)vf.  pixel_offset 0.5: pixel centres at the integers (Open3D, the exporter as written);
//      0.0: centres at + 0.5 (this library's renderer);
//   3  d = depth[c, v, u]; skip if !(d > 0) or d > depth_trunc (a NaN skips);
//   4  float32: sdf = (d - (float)p.z) * ray_scale[v, u]; skip if !(sdf > -sdf_trunc); f = fminf(1, sdf / sdf_trunc);
//      tsdf = (tsdf * w + f) / (w + 1); per channel q = truncf(fminf(fmaxf(rgb * 255, 0), 255)) (the exporter's uint8 cast),
//      colour = (colour * w + q) / (w + 1); w = w + 1.
// ray_scale [H,W] is the depth-to-camera-distance multiplier sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1) at integer (u, v), handed
// in as a table: the kernel has no sqrt and the restatement reads the same bytes.
//   dnsplat_tsdf_integrate      tsdf_integrate_kernel  ONE launch per call.  A thread owns a voxel for the whole call — consecutive
//                               threads consecutive k — and keeps its running mean in registers: no atomics, so two calls with C1 and
//                               C2 cameras leave the bytes of one call with their concatenation.  The camera rows pass through LDS in
//                               chunks of TSDF_CAM_CHUNK (a broadcast ds_read per row entry instead of a global read per thread).  A
//                               voxel is loaded when its first frame lands and stored only if one did.
//   dnsplat_tsdf_vertex_colors  tsdf_colors_kernel     a thread per vertex: the trilinear sample of the colour volume at the vertex's
//                               lattice coordinates, / 255.  Base corner min(floor(x), n - 2) per axis (not below 0), fraction
//                               x - base, blends (1 - f) a + f b in float32 along i, then j, then k: on a lattice edge that is the
//                               linear blend of the edge's two ends, exact at both of them.  A non-finite coordinate gives zeros.

#include "splat_common.h"

namespace {

constexpr int TSDF_THREADS = 256;
constexpr int TSDF_CAM_CHUNK = 8;                           // camera rows in LDS at a time
constexpr long long TSDF_MAX_POINTS = 1LL << 31;            // nx ny nz stays below it, as in marching.hip

struct TsdfGrid {
    float *tsdf, *weight, *color;
    uint32_t n, sI, sJ;                                     // sI = ny nz, sJ = nz
    double ox, oy, oz, voxel;
    int32_t C, W, H;
    const double *w2c;
    double fx, fy, cx, cy, offset, u_hi, v_hi;              // u_hi = W - 0.0001, v_hi = H - 0.0001
    const float *depth, *rgb, *ray_scale;
    float sdf_trunc, depth_trunc;
};

__device__ __forceinline__ float tsdf_quantise(float c) { return truncf(fminf(fmaxf(c * 255.f, 0.f), 255.f)); }

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_kernel(TsdfGrid g)
{
    __shared__ double cam[TSDF_CAM_CHUNK * 12];
    const uint32_t f = blockIdx.x * TSDF_THREADS + threadIdx.x;
    const bool in = f < g.n;
    const uint32_t fc = in ? f : 0, i = fc / g.sI, r = fc - i * g.sI, j = r / g.sJ, k = r - j * g.sJ;
    const double x = g.ox + g.voxel * (double)i, y = g.oy + g.voxel * (double)j, z = g.oz + g.voxel * (double)k;
    const size_t pixels = (size_t)g.W * (size_t)g.H;
    float t = 0.f, w = 0.f, col[3] = {0.f, 0.f, 0.f};
    bool touched = false;
#pragma unroll 1
    for (int c0 = 0; c0 < g.C; c0 += TSDF_CAM_CHUNK) {
        const int cn = min(TSDF_CAM_CHUNK, g.C - c0);
        __syncthreads();                                    // the previous chunk has been read by every wave
        if ((int)threadIdx.x < cn * 12) cam[threadIdx.x] = g.w2c[(size_t)c0 * 12 + threadIdx.x];
        __syncthreads();
        if (!in) continue;
#pragma unroll 1
        for (int c = 0; c < cn; ++c) {
            const double *M = cam + c * 12;
            const double pz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
            if (!(pz > 0.0)) continue;
            const double px = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
            const double py = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
            const double uf = ((g.fx * px) / pz + g.cx) + g.offset, vf = ((g.fy * py) / pz + g.cy) + g.offset;
            if (!(uf >= 0.0001 && uf < g.u_hi && vf >= 0.0001 && vf < g.v_hi)) continue;
            const int u = (int)uf, v = (int)vf;             // 0 <= u < W and 0 <= v < H by the test above
            const size_t pix = (size_t)v * (size_t)g.W + (size_t)u, at = (size_t)(c0 + c) * pixels + pix;
            const float d = g.depth[at];
            if (!(d > 0.f) || d > g.depth_trunc) continue;
            const float sdf = (d - (float)pz) * g.ray_scale[pix];
            if (!(sdf > -g.sdf_trunc)) continue;
            const float v_new = fminf(1.f, sdf / g.sdf_trunc);
            if (!touched) {
                touched = true;
                t = g.tsdf[f]; w = g.weight[f];
                if (g.color) { const float *o = g.color + (size_t)f * 3; col[0] = o[0]; col[1] = o[1]; col[2] = o[2]; }
            }
            const float w1 = w + 1.f;
            t = (t * w + v_new) / w1;
            if (g.color) {
                const float *q = g.rgb + at * 3;
#pragma unroll
                for (int a = 0; a < 3; ++a) col[a] = (col[a] * w + tsdf_quantise(q[a])) / w1;
            }
            w = w1;
        }
    }
    if (touched) {
        g.tsdf[f] = t; g.weight[f] = w;
        if (g.color) { float *o = g.color + (size_t)f * 3; o[0] = col[0]; o[1] = col[1]; o[2] = col[2]; }
    }
}

__device__ __forceinline__ float tsdf_blend(float a, float b, float f) { return (1.f - f) * a + f * b; }

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_colors_kernel(const float *color, int32_t nx, int32_t ny, int32_t nz, const float *vertices,
                                                                  int64_t V, float *out)
{
    const int64_t id = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (id >= V) return;
    const float x[3] = {vertices[id * 3], vertices[id * 3 + 1], vertices[id * 3 + 2]};
    float *o = out + id * 3;
    if (!(fabsf(x[0]) < INFINITY && fabsf(x[1]) < INFINITY && fabsf(x[2]) < INFINITY)) { o[0] = o[1] = o[2] = 0.f; return; }
    const int32_t dims[3] = {nx, ny, nz};
    int32_t b[3];
    float fr[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float base = fmaxf(fminf(floorf(x[a]), (float)(dims[a] - 2)), 0.f);
        b[a] = (int32_t)base;
        fr[a] = x[a] - base;
    }
    const size_t sJ = (size_t)nz, sI = (size_t)ny * sJ;
    const float *p = color + (((size_t)b[0] * sI + (size_t)b[1] * sJ) + (size_t)b[2]) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float c[2][2];                                      // [dj][dk] after the blend along i
#pragma unroll
        for (int dj = 0; dj < 2; ++dj)
#pragma unroll
            for (int dk = 0; dk < 2; ++dk)
                c[dj][dk] = tsdf_blend(p[(dj * sJ + dk) * 3 + ch], p[(sI + dj * sJ + dk) * 3 + ch], fr[0]);
        const float c0 = tsdf_blend(c[0][0], c[1][0], fr[1]), c1 = tsdf_blend(c[0][1], c[1][1], fr[1]);
        o[ch] = tsdf_blend(c0, c1, fr[2]) / 255.f;
    }
}

// 0 for an invalid size; otherwise the number of voxels
long long tsdf_points(int32_t nx, int32_t ny, int32_t nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    const long long n = (long long)nx * ny;                 // < 2^62
    if (n >= TSDF_MAX_POINTS || n * nz >= TSDF_MAX_POINTS) return 0;
    return n * nz;
}

}  // namespace

extern "C" int dnsplat_tsdf_integrate(const dnsplat_tsdf_args *a, dnsplat_stream_t stream_)
{
    if (!a || !a->tsdf || !a->weight || !a->w2c || !a->depth || !a->ray_scale) return DNSPLAT_ERR_INVALID_ARG;
    if ((a->color != nullptr) != (a->rgb != nullptr)) return DNSPLAT_ERR_INVALID_ARG;
    const long long n = tsdf_points(a->nx, a->ny, a->nz);
    if (n == 0 || a->C < 1 || a->width < 1 || a->height < 1) return DNSPLAT_ERR_INVALID_ARG;
    if (!(a->voxel > 0.0) || !(a->sdf_trunc > 0.f) || !(a->depth_trunc > 0.f)) return DNSPLAT_ERR_INVALID_ARG;
    if ((long long)a->width * a->height > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;
    TsdfGrid g;
    g.tsdf = a->tsdf; g.weight = a->weight; g.color = a->color;
    g.n = (uint32_t)n; g.sI = (uint32_t)a->ny * (uint32_t)a->nz; g.sJ = (uint32_t)a->nz;
    g.ox = a->origin[0]; g.oy = a->origin[1]; g.oz = a->origin[2]; g.voxel = a->voxel;
    g.C = a->C; g.W = a->width; g.H = a->height;
    g.w2c = a->w2c;
    g.fx = a->fx; g.fy = a->fy; g.cx = a->cx; g.cy = a->cy; g.offset = a->pixel_offset;
    g.u_hi = (double)a->width - 0.0001; g.v_hi = (double)a->height - 0.0001;
    g.depth = a->depth; g.rgb = a->rgb; g.ray_scale = a->ray_scale;
    g.sdf_trunc = a->sdf_trunc; g.depth_trunc = a->depth_trunc;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((n + TSDF_THREADS - 1) / TSDF_THREADS)), dim3(TSDF_THREADS), 0, (hipStream_t)stream_, g);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_tsdf_vertex_colors(const float *color, int32_t nx, int32_t ny, int32_t nz, const float *vertices, int64_t V, float *out,
                                          dnsplat_stream_t stream_)
{
    if (!color || V < 0 || (V > 0 && (!vertices || !out))) return DNSPLAT_ERR_INVALID_ARG;
    if (tsdf_points(nx, ny, nz) == 0 || nx < 2 || ny < 2 || nz < 2) return DNSPLAT_ERR_INVALID_ARG;   // no cell, no trilinear sample
    if (V > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;   // vertex ids are int32
    if (V == 0) return DNSPLAT_OK;
    hipLaunchKernelGGL(tsdf_colors_kernel, dim3((unsigned)((V + TSDF_THREADS - 1) / TSDF_THREADS)), dim3(TSDF_THREADS), 0, (hipStream_t)stream_,
                       color, nx, ny, nz, vertices, V, out);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
