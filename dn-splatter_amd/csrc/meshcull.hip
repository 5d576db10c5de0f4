// meshcull.hip — the reference's mesh visibility culling (cull_mesh, dn_splatter/eval/eval_mesh_vis_cull.py:176-266) on the device:
// the double-sided depth renders of the mesh (pyrender through OpenGL there), the per-vertex votes of cull_from_one_pose summed over
// the poses, and the triangle rule with remove_unreferenced_vertices.  torch_mesh_cull.py states the same operations in the same
// order; the kernels are held to it with exact equality.  Compiled with -ffp-contract=off: every product rounds before its sum.
//
//   dnsplat_mesh_depth        mv_rays_kernel     the pixel rays d.x [W], d.y [H] in double, one division each, into the scratch
//                             mv_fill_kernel     the z-buffer to the bits of +inf
//                             mv_depth_kernel    one lane per (camera, triangle): homogeneous edge functions in double, no clipping;
//                                                a conservative pixel box; boxes of at most MV_SMALL pixels are walked by their lane,
//                                                larger ones are found by a wave ballot and walked by the whole wave, 64 pixels per
//                                                step, the coefficients broadcast by lane reads; integer atomicMin on the bits of
//                                                float32(z) behind a plain load of the current depth
//                             mv_finish_kernel   +inf -> 0
//   dnsplat_mesh_visibility   mv_votes_kernel    one lane per vertex, a loop over the cameras of the batch; obs / invalid accumulate
//   dnsplat_mesh_cut_count    hipMemset, mv_keep_kernel (the rule per triangle, marks of the referenced vertices, kept per block),
//                             mv_mark_count_kernel (marked vertices per block), mv_cut_scan_kernel (both scans, counts = {V', T'})
//   dnsplat_mesh_cut_emit     mv_emit_vertices_kernel (the vertices in order, mark -> new id), mv_emit_triangles_kernel
// mv_mark_count_kernel, mv_cut_scan_kernel and mv_emit_triangles_kernel are in mesh_cut.h: meshclusters.hip ends its cut with them too.
//
// Positive floats order as their bit patterns and an integer minimum does not depend on the order of arrival: the depth map is a
// canonical function of its inputs.  No floating-point atomic; the cut has no atomic at all (the scans, the flag rank and the layout
// of the ordered append of block_scan.h; the marks are plain stores of the same value 1).
#include "mesh_cut.h"

namespace {

constexpr int MV_SMALL = 16;               // boxes of up to this many pixels stay with their lane
constexpr unsigned MV_INF_BITS = 0x7f800000u;

struct MvDepth {
    int V, T, W, H;
    const float *vertices;
    const int32_t *triangles;
    const double *w2c;                     // [C,12]
    const double *rays;                    // d.x [W], then d.y [H]
    double fx, fy, cx, cy, znear, zfar;
    unsigned *zbits;                       // [C,H,W]
    unsigned long long *stats;             // {setups, fragments, atomics} or NULL
};

__global__ __launch_bounds__(MV_THREADS) void mv_rays_kernel(int W, int H, double fx, double fy, double cx, double cy, double *__restrict__ rays)
{
    const int i = blockIdx.x * MV_THREADS + threadIdx.x;
    if (i < W) rays[i] = (((double)i + 0.5) - cx) / fx;
    else if (i < W + H) rays[i] = (((double)(i - W) + 0.5) - cy) / fy;
}

__global__ __launch_bounds__(MV_THREADS) void mv_fill_kernel(long long n, unsigned *__restrict__ zbits)
{
    const long long i = (long long)blockIdx.x * MV_THREADS + threadIdx.x;
    if (i < n) zbits[i] = MV_INF_BITS;
}

__global__ __launch_bounds__(MV_THREADS) void mv_finish_kernel(long long n, unsigned *__restrict__ zbits)
{
    const long long i = (long long)blockIdx.x * MV_THREADS + threadIdx.x;
    if (i < n && zbits[i] == MV_INF_BITS) zbits[i] = 0u;
}

__device__ __forceinline__ double mv_lane_read(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// the edge functions of one triangle under one camera: c0, c1, c2, n, D
struct MvCoef {
    double c[4][3];
    double D;
};

// One (triangle, pixel) test.  Returns 1 for an accepted fragment; `atomics` counts the ones that reached the atomic.
__device__ __forceinline__ int mv_fragment(const MvCoef &q, int x, int y, const MvDepth &a, unsigned *zbuf, int &atomics)
{
    const double dx = a.rays[x], dy = a.rays[a.W + y];
    const double e0 = (q.c[0][0] * dx + q.c[0][1] * dy) + q.c[0][2];
    const double e1 = (q.c[1][0] * dx + q.c[1][1] * dy) + q.c[1][2];
    const double e2 = (q.c[2][0] * dx + q.c[2][1] * dy) + q.c[2][2];
    const double s = (q.c[3][0] * dx + q.c[3][1] * dy) + q.c[3][2];
    const bool inside = ((e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0)) && s != 0.0;
    if (!inside) return 0;
    const double z = q.D / s;
    if (!(z >= a.znear && z <= a.zfar)) return 0;                                 // a nan fails both
    const unsigned bits = __float_as_uint((float)z);
    unsigned *p = zbuf + (size_t)y * a.W + x;
    if (bits < *(volatile unsigned *)p) {                                         // the filter; the atomic still decides
        atomicMin(p, bits);
        ++atomics;
    }
    return 1;
}

// floor(lo) - 1 and floor(hi) + 1 clamped to [0, n] and [-1, n - 1]; a nan gives the whole range
__device__ __forceinline__ void mv_box_axis(double lo, double hi, int n, int &i0, int &i1)
{
    const double l = floor(lo) - 1.0, h = floor(hi) + 1.0;
    i0 = l > 0.0 ? (l < (double)n ? (int)l : n) : 0;
    i1 = h < (double)(n - 1) ? (h >= 0.0 ? (int)h : -1) : n - 1;
}

__global__ __launch_bounds__(MV_THREADS) void mv_depth_kernel(MvDepth a)
{
    const int cam = blockIdx.y;
    const long long t = (long long)blockIdx.x * MV_THREADS + threadIdx.x;
    const int lane = threadIdx.x & (DNS_WAVE - 1);
    const double *M = a.w2c + (size_t)cam * 12;
    unsigned *zbuf = a.zbits + (size_t)cam * a.H * a.W;

    MvCoef q;
    int x0 = 0, y0 = 0, x1 = -1, y1 = -1;
    bool live = false;
    if (t < a.T) {
        const int i0 = a.triangles[t * 3], i1 = a.triangles[t * 3 + 1], i2 = a.triangles[t * 3 + 2];
        if ((unsigned)i0 < (unsigned)a.V && (unsigned)i1 < (unsigned)a.V && (unsigned)i2 < (unsigned)a.V && i0 != i1 && i1 != i2 && i0 != i2) {
            const int id[3] = {i0, i1, i2};
            double x[3][3];
            bool finite = true;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float f = a.vertices[(size_t)id[i] * 3 + k];
                    finite = finite && fabsf(f) < INFINITY;
                    x[i][k] = (double)f;
                }
            // the area of dnsplat_mesh_areas: a face without one covers nothing
            double ea[3], eb[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { ea[k] = x[1][k] - x[0][k]; eb[k] = x[2][k] - x[0][k]; }
            const double cr[3] = {ea[1] * eb[2] - ea[2] * eb[1], ea[2] * eb[0] - ea[0] * eb[2], ea[0] * eb[1] - ea[1] * eb[0]};
            const double len = sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
            if (finite && len > 0.0 && len < (double)INFINITY) {
                double p[3][3];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        p[i][k] = ((M[k * 4] * x[i][0] + M[k * 4 + 1] * x[i][1]) + M[k * 4 + 2] * x[i][2]) + M[k * 4 + 3];
#pragma unroll
                for (int e = 0; e < 3; ++e) {                                     // c_e = p_{e+1} x p_{e+2}
                    const double *u = p[(e + 1) % 3], *w = p[(e + 2) % 3];
                    q.c[e][0] = u[1] * w[2] - u[2] * w[1];
                    q.c[e][1] = u[2] * w[0] - u[0] * w[2];
                    q.c[e][2] = u[0] * w[1] - u[1] * w[0];
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) q.c[3][k] = (q.c[1][k] + q.c[2][k]) + q.c[0][k];
                q.D = (p[0][0] * q.c[0][0] + p[0][1] * q.c[0][1]) + p[0][2] * q.c[0][2];
                // the search window: the projected part of the triangle with z >= znear, widened by a pixel
                const bool in[3] = {p[0][2] >= a.znear, p[1][2] >= a.znear, p[2][2] >= a.znear};
                const bool behind = p[0][2] < a.znear && p[1][2] < a.znear && p[2][2] < a.znear;
                const bool beyond = p[0][2] > a.zfar && p[1][2] > a.zfar && p[2][2] > a.zfar;
                if (!behind && !beyond) {
                    double ulo = (double)INFINITY, uhi = -(double)INFINITY, vlo = (double)INFINITY, vhi = -(double)INFINITY;
                    bool unknown = false;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const int j = (i + 1) % 3;
                        if (in[i]) {
                            const double u = a.fx * p[i][0] / p[i][2] + a.cx, v = a.fy * p[i][1] / p[i][2] + a.cy;
                            unknown = unknown || u != u || v != v;
                            ulo = fmin(ulo, u); uhi = fmax(uhi, u); vlo = fmin(vlo, v); vhi = fmax(vhi, v);
                        }
                        if (in[i] != in[j]) {                                     // the edge's point on z = znear
                            const double s = (a.znear - p[i][2]) / (p[j][2] - p[i][2]);
                            const double X = p[i][0] + s * (p[j][0] - p[i][0]), Y = p[i][1] + s * (p[j][1] - p[i][1]);
                            const double u = a.fx * X / a.znear + a.cx, v = a.fy * Y / a.znear + a.cy;
                            unknown = unknown || u != u || v != v;
                            ulo = fmin(ulo, u); uhi = fmax(uhi, u); vlo = fmin(vlo, v); vhi = fmax(vhi, v);
                        }
                    }
                    if (unknown || !(in[0] || in[1] || in[2])) {                        // nothing to bound it by: the whole frame
                        ulo = vlo = -(double)INFINITY; uhi = vhi = (double)INFINITY;
                    }
                    mv_box_axis(ulo, uhi, a.W, x0, x1);
                    mv_box_axis(vlo, vhi, a.H, y0, y1);
                    live = x0 <= x1 && y0 <= y1;
                }
            }
        }
    }
    const int bw = x1 - x0 + 1;
    const int npix = live ? bw * (y1 - y0 + 1) : 0;
    int fragments = 0, atomics = 0;

    if (live && npix <= MV_SMALL) {
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) fragments += mv_fragment(q, x, y, a, zbuf, atomics);
    }
    // the larger boxes, one after the other, by the whole wave: lane l takes pixels l, l + 64, ... of the box in row order
    uint64_t big = dns_ballot(live && npix > MV_SMALL);
    while (big) {
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)big) - 1);
        big &= big - 1;
        MvCoef w;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int k = 0; k < 3; ++k) w.c[e][k] = mv_lane_read(q.c[e][k], src);
        w.D = mv_lane_read(q.D, src);
        const int X0 = __builtin_amdgcn_readlane(x0, src), Y0 = __builtin_amdgcn_readlane(y0, src);
        const int BW = __builtin_amdgcn_readlane(bw, src), N = __builtin_amdgcn_readlane(npix, src);
        for (int i = lane; i < N; i += DNS_WAVE) {
            const int r = i / BW;
            fragments += mv_fragment(w, X0 + (i - r * BW), Y0 + r, a, zbuf, atomics);
        }
    }
    if (a.stats) {                                                                // the measurement's counters: one add per wave
        unsigned long long v[3] = {live ? 1ull : 0ull, (unsigned long long)fragments, (unsigned long long)atomics};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int off = DNS_WAVE / 2; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, DNS_WAVE);
            if (lane == 0 && v[k]) atomicAdd(a.stats + k, v[k]);
        }
    }
}

// ---- the votes --------------------------------------------------------------------------------------------------------------------

struct MvVotes {
    int V, C, W, H;
    const float *vertices;
    const double *w2c;
    double K[9];
    const float *rendered, *depth_gt;      // [C,H,W]; NULL when the flag is off
    int32_t *obs, *invalid;
};

__global__ __launch_bounds__(MV_THREADS) void mv_votes_kernel(MvVotes a)
{
    const int i = blockIdx.x * MV_THREADS + threadIdx.x;
    if (i >= a.V) return;
    const double x = (double)a.vertices[(size_t)i * 3], y = (double)a.vertices[(size_t)i * 3 + 1], z = (double)a.vertices[(size_t)i * 3 + 2];
    const size_t frame = (size_t)a.H * a.W;
    int seen = 0, missing = 0;
    for (int c = 0; c < a.C; ++c) {
        const double *M = a.w2c + (size_t)c * 12;
        double p[3], q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = ((M[k * 4] * x + M[k * 4 + 1] * y) + M[k * 4 + 2] * z) + M[k * 4 + 3];
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = (a.K[k * 3] * p[0] + a.K[k * 3 + 1] * p[1]) + a.K[k * 3 + 2] * p[2];
        const double pz = q[2] + 1e-8;
        const double px = q[0] / pz, py = q[1] / pz;
        if (!(px >= 0.0 && px <= (double)(a.W - 1) && py >= 0.0 && py <= (double)(a.H - 1) && pz > 0.0)) continue;
        const size_t at = (size_t)c * frame + (size_t)(int)py * a.W + (int)px;
        bool o = true;
        if (a.rendered) o = pz < (double)(a.rendered[at] + 0.02f);                // the map is float32 and numpy adds in float32
        seen += o ? 1 : 0;
        if (a.depth_gt) missing += a.depth_gt[at] <= 0.f ? 1 : 0;
    }
    a.obs[i] += seen;
    a.invalid[i] += missing;
}

// ---- the cut ----------------------------------------------------------------------------------------------------------------------
// scratch: marks int32 [V] (non-zero for a vertex some kept triangle references; after the emit of the vertices its new id + 1),
// kept-per-block int32 [nbT], marked-per-block int32 [nbV], keep uint8 [T]

struct MvScratch {
    int32_t *marks, *tcount, *vcount;
    uint8_t *keep;
};

size_t mv_cut_bytes(int V, int T)
{
    return ((size_t)V + mv_blocks(T) + mv_blocks(V)) * sizeof(int32_t) + (size_t)T;
}

MvScratch mv_carve(void *scratch, int V, int T)
{
    MvScratch s;
    s.marks = (int32_t *)scratch;
    s.tcount = s.marks + V;
    s.vcount = s.tcount + mv_blocks(T);
    s.keep = (uint8_t *)(s.vcount + mv_blocks(V));
    return s;
}

__global__ __launch_bounds__(MV_THREADS) void mv_keep_kernel(int V, int T, const int32_t *__restrict__ triangles, const int32_t *__restrict__ obs,
                                                             const int32_t *__restrict__ invalid, int threshold, double share,
                                                             int32_t *__restrict__ marks, int32_t *__restrict__ tcount, uint8_t *__restrict__ keep)
{
    __shared__ int wave_tot[MV_THREADS / DNS_WAVE];
    const int t = blockIdx.x * MV_THREADS + threadIdx.x;
    bool kept = false;
    if (t < T) {
        const int id[3] = {triangles[(size_t)t * 3], triangles[(size_t)t * 3 + 1], triangles[(size_t)t * 3 + 2]};
        if ((unsigned)id[0] < (unsigned)V && (unsigned)id[1] < (unsigned)V && (unsigned)id[2] < (unsigned)V) {
            bool observed = false, bad = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int o = obs[id[k]], m = invalid[id[k]];
                observed = observed || o > threshold;
                bad = bad && (double)m > share * (double)o;
            }
            kept = observed && !bad;
            if (kept) { marks[id[0]] = 1; marks[id[1]] = 1; marks[id[2]] = 1; }
        }
        keep[t] = kept ? 1 : 0;
    }
    int total;
    dns_block_rank<MV_THREADS>(kept, wave_tot, total);
    if (threadIdx.x == 0) tcount[blockIdx.x] = total;
}

__global__ __launch_bounds__(MV_THREADS) void mv_emit_vertices_kernel(int V, const float *__restrict__ vertices, const int32_t *__restrict__ vcount,
                                                                      int32_t *__restrict__ marks, long long cap_v, float *__restrict__ out)
{
    __shared__ int wave_tot[MV_THREADS / DNS_WAVE];
    const int i = blockIdx.x * MV_THREADS + threadIdx.x;
    const bool marked = i < V && marks[i] != 0;
    int total;
    const int id = vcount[blockIdx.x] + dns_block_rank<MV_THREADS>(marked, wave_tot, total);
    if (i >= V) return;
    if (marked) marks[i] = id + 1;                                                // still a mark: a second emit finds the same flags
    if (marked && id < cap_v) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[(size_t)id * 3 + k] = vertices[(size_t)i * 3 + k];
    }
}

bool mv_cut_args_ok(const dnsplat_mesh_cut_args *a)
{
    return a && a->V >= 1 && a->T >= 1 && a->vertices && a->triangles && a->obs && a->invalid && a->scratch && a->counts;
}

}  // namespace

extern "C" size_t dnsplat_mesh_depth_scratch_bytes(int32_t width, int32_t height)
{
    if (width < 1 || height < 1 || (long long)width * height > 0x7fffffffLL) return 0;
    return ((size_t)width + (size_t)height) * sizeof(double);
}

extern "C" int dnsplat_mesh_depth(const dnsplat_mesh_depth_args *a, dnsplat_stream_t stream_)
{
    if (!a || !a->vertices || !a->triangles || !a->w2c || !a->depth || !a->scratch) return DNSPLAT_ERR_INVALID_ARG;
    if (a->V < 1 || a->T < 1 || a->C < 1 || a->width < 1 || a->height < 1) return DNSPLAT_ERR_INVALID_ARG;
    if (!(a->znear > 0.0 && a->znear <= a->zfar && a->zfar < (double)INFINITY)) return DNSPLAT_ERR_INVALID_ARG;      // a nan fails
    if (!(fabs(a->fx) > 0.0 && fabs(a->fx) < (double)INFINITY && fabs(a->fy) > 0.0 && fabs(a->fy) < (double)INFINITY)) return DNSPLAT_ERR_INVALID_ARG;
    if ((long long)a->width * a->height > 0x7fffffffLL || a->C > 65535) return DNSPLAT_ERR_UNSUPPORTED;
    if ((size_t)a->scratch % sizeof(double)) return DNSPLAT_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    MvDepth q;
    q.V = a->V; q.T = a->T; q.W = a->width; q.H = a->height;
    q.vertices = a->vertices; q.triangles = a->triangles; q.w2c = a->w2c; q.rays = (const double *)a->scratch;
    q.fx = a->fx; q.fy = a->fy; q.cx = a->cx; q.cy = a->cy; q.znear = a->znear; q.zfar = a->zfar;
    q.zbits = (unsigned *)a->depth;
    q.stats = (unsigned long long *)a->stats;
    const long long n = (long long)a->C * a->height * a->width;
    hipLaunchKernelGGL(mv_rays_kernel, dim3((unsigned)mv_blocks((long long)a->width + a->height)), dim3(MV_THREADS), 0, stream, a->width, a->height,
                       a->fx, a->fy, a->cx, a->cy, (double *)a->scratch);
    hipLaunchKernelGGL(mv_fill_kernel, dim3((unsigned)((n + MV_THREADS - 1) / MV_THREADS)), dim3(MV_THREADS), 0, stream, n, q.zbits);
    hipLaunchKernelGGL(mv_depth_kernel, dim3((unsigned)mv_blocks(a->T), (unsigned)a->C), dim3(MV_THREADS), 0, stream, q);
    hipLaunchKernelGGL(mv_finish_kernel, dim3((unsigned)((n + MV_THREADS - 1) / MV_THREADS)), dim3(MV_THREADS), 0, stream, n, q.zbits);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_mesh_visibility(const dnsplat_mesh_visibility_args *a, dnsplat_stream_t stream_)
{
    if (!a || !a->vertices || !a->w2c || !a->obs || !a->invalid) return DNSPLAT_ERR_INVALID_ARG;
    if (a->V < 1 || a->C < 1 || a->width < 1 || a->height < 1) return DNSPLAT_ERR_INVALID_ARG;
    if ((a->remove_occlusion && !a->rendered) || (a->remove_missing_depth && !a->depth_gt)) return DNSPLAT_ERR_INVALID_ARG;
    if ((long long)a->width * a->height > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;
    MvVotes q;
    q.V = a->V; q.C = a->C; q.W = a->width; q.H = a->height;
    q.vertices = a->vertices; q.w2c = a->w2c;
    for (int k = 0; k < 9; ++k) q.K[k] = a->K[k];
    q.rendered = a->remove_occlusion ? a->rendered : nullptr;
    q.depth_gt = a->remove_missing_depth ? a->depth_gt : nullptr;
    q.obs = a->obs; q.invalid = a->invalid;
    hipLaunchKernelGGL(mv_votes_kernel, dim3((unsigned)mv_blocks(a->V)), dim3(MV_THREADS), 0, (hipStream_t)stream_, q);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" size_t dnsplat_mesh_cut_scratch_bytes(int32_t V, int32_t T)
{
    if (V < 1 || T < 1) return 0;
    return mv_cut_bytes(V, T);
}

extern "C" int dnsplat_mesh_cut_count(const dnsplat_mesh_cut_args *a, dnsplat_stream_t stream_)
{
    if (!mv_cut_args_ok(a)) return DNSPLAT_ERR_INVALID_ARG;
    if (a->scratch_bytes < mv_cut_bytes(a->V, a->T) || (size_t)a->scratch % sizeof(int32_t)) return DNSPLAT_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const MvScratch s = mv_carve(a->scratch, a->V, a->T);
    const int nbt = mv_blocks(a->T), nbv = mv_blocks(a->V);
    if (hipMemsetAsync(s.marks, 0, (size_t)a->V * sizeof(int32_t), stream) != hipSuccess) return DNSPLAT_ERR_LAUNCH;
    hipLaunchKernelGGL(mv_keep_kernel, dim3((unsigned)nbt), dim3(MV_THREADS), 0, stream, a->V, a->T, a->triangles, a->obs, a->invalid,
                       a->obs_threshold, a->invalid_share, s.marks, s.tcount, s.keep);
    hipLaunchKernelGGL(mv_mark_count_kernel, dim3((unsigned)nbv), dim3(MV_THREADS), 0, stream, a->V, s.marks, s.vcount);
    hipLaunchKernelGGL(mv_cut_scan_kernel, dim3(1), dim3(MV_THREADS), 0, stream, nbv, s.vcount, nbt, s.tcount, a->counts);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_mesh_cut_emit(const dnsplat_mesh_cut_args *a, dnsplat_stream_t stream_)
{
    if (!mv_cut_args_ok(a) || !a->status || a->cap_v < 0 || a->cap_t < 0) return DNSPLAT_ERR_INVALID_ARG;
    if ((a->cap_v > 0 && !a->out_vertices) || (a->cap_t > 0 && !a->out_triangles)) return DNSPLAT_ERR_INVALID_ARG;
    if (a->scratch_bytes < mv_cut_bytes(a->V, a->T) || (size_t)a->scratch % sizeof(int32_t)) return DNSPLAT_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const MvScratch s = mv_carve(a->scratch, a->V, a->T);
    hipLaunchKernelGGL(mv_emit_vertices_kernel, dim3((unsigned)mv_blocks(a->V)), dim3(MV_THREADS), 0, stream, a->V, a->vertices, s.vcount, s.marks,
                       (long long)a->cap_v, a->out_vertices);
    hipLaunchKernelGGL(mv_emit_triangles_kernel, dim3((unsigned)mv_blocks(a->T)), dim3(MV_THREADS), 0, stream, a->T, a->triangles, s.keep, s.tcount,
                       s.marks, a->counts, (long long)a->cap_v, (long long)a->cap_t, a->out_triangles, a->status);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
