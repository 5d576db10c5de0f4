// levelset.hip — the per-camera hot path of the reference's LevelSetExtractor (export_mesh.py:514-697):
// DNSplatterModel.compute_level_surface_points (dn_model.py:1229-1447), the SuGaR ray search, one thread per pixel.  Where the reference
// back-projects every pixel, runs sklearn's kd-tree on the CPU for 16 neighbours of each, gathers [n,16,3,3] matrices for 21 samples
// along every ray in passes of 2 M samples, gathers by boolean mask per surface level and reads the number of hits on the host, this
// file makes two entry points, neither of which reads anything on the host:
//   dnsplat_level_rays     one launch.  Per pixel i = v W + u:
//                            d = mask && !mask[i] ? 0 : depth[i]; d <= 0 takes no part; a non-finite d (or point) takes no part either
//                            and reads nothing — our choice, the reference would raise inside sklearn;
//                            p = the world point of dnsplat_backproject_points, the same code (pixel_camera.h); o = c2w[:3, 3];
//                            dir = (p - o) / max(|p - o|, 1e-12);
//                            the neighbours of p: ranks 1 .. 16 of 17 (knn_sk drops the nearest; kept), df_search in the thread or the
//                            caller's [P,16] tensor; c = the first of them;
//                            std = | exp(s_c) * (R(q_c / |q_c|)^T w) |, w = (o - mu_c) / |o - mu_c|;
//                            x_j = p + (r_j std) dir for the 21 values r of the caller's table; D_j = the density sum over the 16
//                            neighbours OF p in rank order (ls_term, 21 accumulators in registers, the neighbour indices in a
//                            thread-private LDS column so that the loop over them is a loop); D_j >= 1: D_j / (D_j + 1e-5); no floor;
//                            per level L: a = the first j with D_j > L; empty unless D_0 < L and a >= 1;
//                            t = ((L - D_{a-1}) / (D_a - D_{a-1})) (T_a - T_{a-1}) + T_{a-1}, T_j = r_j std.
//   dnsplat_level_points   per level, one thread per selected row: x = p + t dir, colour, normal (row c of the model's normals, or
//                          -normalize(sum_k w_k M_k M_k^T (x - mu_k)) with w_k the neighbour's density term, the search run again for
//                          these rows only), the crop-box test, and the ordered append behind a device cursor (count per 256 rows,
//                          one-workgroup scan that also moves the cursor, then the same rows again with the write): the append
//                          of dnsplat_backproject_points, the same code (block_scan.h).
// A DELIBERATE DEPARTURE from dn_model.py's arithmetic, which is fp32 throughout: (1) x_j is never formed.  The evaluation is handed
// the offset (p - mu_k) + (r_j std) dir, each term of the size of the Gaussian; rounding p + (r_j std) dir to an ulp of |p| first
// costs, through M, more than the whole evaluation does (the reference's own densities are 1.3e-5 from their fp64 values for it).
// The analytical normal forms (p - mu_k) + t dir likewise.  (2) dir and std, once per pixel, are formed in double and rounded once;
// T_j = r_j std is the fp32 product with that std.  Densities and t are therefore not the fp32 rule's values bit for bit but closer to
// the exact ones; the statements behind the offset are df_accumulate's (ls_term), on the same records.
// No atomic anywhere; compiled without contraction.  Both neighbour sources feed the same code after the LDS column is filled, and the
// two lane mappings differ only in which thread takes which pixel: equal bits in all four combinations.

#include "block_scan.h"
#include "density_common.h"
#include "pixel_camera.h"

namespace {

constexpr int LS_THREADS = DF_THREADS;
constexpr int LS_WAVES = LS_THREADS / DNS_WAVE;
constexpr int LS_R = DNSPLAT_LEVEL_RANGE_POINTS;
constexpr int LS_K = DNSPLAT_LEVEL_KNN;
constexpr int LS_KM = LS_K + 1;                       // knn_sk's 17
constexpr int LS_TILE = 8;                            // a wave's block of pixels is LS_TILE x LS_TILE

static_assert(LS_TILE * LS_TILE == DNS_WAVE, "one lane per pixel of a block");

using LsCam = DnsPixelCamera;

// the world point of pixel i and the unit ray direction through it; false: the pixel takes no part (nothing else was read)
__device__ __forceinline__ bool ls_point(const LsCam &c, long long i, float p[3], float dir[3])
{
    const float d = dns_pixel_depth(c, i);
    if (!(d > 0.f) || !(d < INFINITY)) return false;
    dns_pixel_point(c, i, d, p);
    const float *T = c.xform + 9;
    double e[3];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e[a] = (double)p[a] - (double)T[a];
        finite = finite && fabsf(p[a]) < INFINITY;
    }
    // F.normalize; formed in double and rounded once: every sample of the ray is a multiple of dir away from p
    const double div = fmax(sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]), 1e-12);
#pragma unroll
    for (int a = 0; a < 3; ++a) dir[a] = (float)(e[a] / div);
    return finite;
}

// | exp(s) * (R(q / |q|)^T w) | of Gaussian c, w the unit vector from its mean to the camera.  Once per pixel, so in double and rounded
// once: its relative error is the relative error of every offset r_j std of the ray, which M (the inverse scales) magnifies
__device__ __forceinline__ float ls_ray_std(const float *__restrict__ records, const float *__restrict__ scales, const float *__restrict__ quats,
                                            int c, const float *o)
{
    const float *mu = records + (size_t)c * DNS_REC;
    const double w[3] = {(double)o[0] - (double)mu[0], (double)o[1] - (double)mu[1], (double)o[2] - (double)mu[2]};
    const double wl = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const float *q = quats + (size_t)c * 4;
    const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const double ql = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const double qw = q0 / ql, x = q1 / ql, y = q2 / ql, z = q3 / ql;
    const double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - qw * z),      2.0 * (x * z + qw * y),
                         2.0 * (x * y + qw * z),      1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - qw * x),
                         2.0 * (x * z - qw * y),      2.0 * (y * z + qw * x),      1.0 - 2.0 * (x * x + y * y)};
    double s2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double u = R[a] * (w[0] / wl) + R[3 + a] * (w[1] / wl) + R[6 + a] * (w[2] / wl);      // row a of R^T
        const double s = exp((double)scales[(size_t)c * 3 + a]) * u;
        s2 += s * s;
    }
    return (float)sqrt(s2);
}

// a neighbour's record of dnsplat_density_pack: the mean, the opacity, M row-major
struct LsRecord {
    float mu[3], o, Mm[9];
};

__device__ __forceinline__ LsRecord ls_record(const float *__restrict__ records, int gi)
{
    const float4 *rec = (const float4 *)(records + (size_t)gi * DNS_REC);
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    return LsRecord{{r0.x, r0.y, r0.z}, r0.w, {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x}};
}

// one neighbour's term of the density sum at the offset d = x - mu: o exp(-clamp(|M^T d|^2, 0, 1e8) / 2), the statements of
// df_accumulate (density_common.h) behind its x - mu; v = M^T d is left for the caller
__device__ __forceinline__ float ls_term(const LsRecord &r, float d0, float d1, float d2, float v[3])
{
    const float *Mm = r.Mm;
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = Mm[a] * d0 + Mm[3 + a] * d1 + Mm[6 + a] * d2;
    const float m2 = fminf(fmaxf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2], 0.f), 1e8f);
    return r.o * expf(-0.5f * m2);
}

struct LsRays {
    LsCam cam;
    int N;
    DfIndex ix;
    const float *records, *scales, *quats, *range;
    const int32_t *nb32;
    const int64_t *nb64;
    int n_levels;
    float levels[DNSPLAT_LEVEL_MAX_LEVELS];
    int tiles_x;
    long long tiles;
    float *t_hit;
    uint8_t *valid;
    int32_t *closest, *first_above;
    float *densities;
};

// SEARCH: the neighbours are searched here, else they are the caller's.  MAP: DNSPLAT_LEVEL_MAP_*
template <bool SEARCH, int MAP>
__global__ __launch_bounds__(LS_THREADS) void ls_rays_kernel(LsRays e)
{
    __shared__ int nb_s[LS_K][LS_THREADS];                 // column threadIdx.x belongs to this thread alone: no barrier
    const int tid = threadIdx.x;
    long long i;
    if (MAP == DNSPLAT_LEVEL_MAP_ROW) {
        i = (long long)blockIdx.x * LS_THREADS + tid;
        if (i >= e.cam.P) return;
    } else {
        const int lane = tid & (DNS_WAVE - 1), wave = tid / DNS_WAVE;
        const long long tile = (long long)blockIdx.x * LS_WAVES + wave;
        if (tile >= e.tiles) return;
        const int ty = (int)(tile / e.tiles_x), tx = (int)(tile - (long long)ty * e.tiles_x);
        const int u = tx * LS_TILE + (lane & (LS_TILE - 1)), v = ty * LS_TILE + lane / LS_TILE;
        if (u >= e.cam.W || v >= e.cam.H) return;
        i = (long long)v * e.cam.W + u;
    }
    float p[3], dir[3];
    bool part = ls_point(e.cam, i, p, dir);
    if (part) {
        if constexpr (SEARCH) {
            DfList<LS_KM> L;
            part = df_search(e.ix, p[0], p[1], p[2], LS_KM, L);
#pragma unroll
            for (int j = 1; j < LS_KM; ++j) {
                if ((unsigned)L.i[j] >= (unsigned)e.N) part = false;           // fewer than 17 comparable means (nan coordinates)
                nb_s[j - 1][tid] = L.i[j];
            }
        } else {
            for (int k = 0; k < LS_K; ++k) {
                const long long gi = e.nb64 ? (long long)e.nb64[i * LS_K + k] : (long long)e.nb32[i * LS_K + k];
                if (gi < 0 || gi >= e.N) part = false;
                nb_s[k][tid] = (int)gi;
            }
        }
    }
    if (!part) {
        e.closest[i] = -1;
        for (int l = 0; l < e.n_levels; ++l) {
            e.t_hit[(long long)l * e.cam.P + i] = NAN;
            e.valid[(long long)l * e.cam.P + i] = 0;
            if (e.first_above) e.first_above[(long long)l * e.cam.P + i] = 0;
        }
        if (e.densities)
            for (int j = 0; j < LS_R; ++j) e.densities[i * LS_R + j] = NAN;
        return;
    }
    const int c = nb_s[0][tid];
    e.closest[i] = c;
    const float std = ls_ray_std(e.records, e.scales, e.quats, c, e.cam.xform + 9);
    float acc[LS_R];
#pragma unroll
    for (int j = 0; j < LS_R; ++j) acc[j] = 0.f;
#pragma unroll 1
    for (int k = 0; k < LS_K; ++k) {
        const LsRecord rec = ls_record(e.records, nb_s[k][tid]);
        const float e0 = p[0] - rec.mu[0], e1 = p[1] - rec.mu[1], e2 = p[2] - rec.mu[2];
#pragma unroll
        for (int j = 0; j < LS_R; ++j) {
            const float T = e.range[j] * std;
            float v[3];
            acc[j] += ls_term(rec, e0 + T * dir[0], e1 + T * dir[1], e2 + T * dir[2], v);
        }
    }
    float D[LS_R];
#pragma unroll
    for (int j = 0; j < LS_R; ++j) {
        float d = acc[j];
        if (d >= 1.0f) d = d / (d + 1e-5f);
        D[j] = d;
        if (e.densities) e.densities[i * LS_R + j] = d;
    }
    for (int l = 0; l < e.n_levels; ++l) {
        const float L = e.levels[l];
        int a = 0;
        bool found = false;
#pragma unroll
        for (int j = LS_R - 1; j >= 0; --j)
            if (D[j] > L) { a = j; found = true; }
        const bool hit = found && a >= 1 && D[0] < L;
        float Da = 0.f, Db = 0.f, ra = 0.f, rb = 0.f;
#pragma unroll
        for (int j = 1; j < LS_R; ++j)
            if (a == j) { Da = D[j]; Db = D[j - 1]; ra = e.range[j]; rb = e.range[j - 1]; }
        const float Ta = ra * std, Tb = rb * std;
        const float t = ((L - Db) / (Da - Db)) * (Ta - Tb) + Tb;
        const long long at = (long long)l * e.cam.P + i;
        e.t_hit[at] = hit ? t : NAN;
        e.valid[at] = hit ? 1 : 0;
        if (e.first_above) e.first_above[at] = hit ? a : 0;
    }
}

// ---- the points of a level -----------------------------------------------------------------------------------------------------------

struct LsPoints {
    LsCam cam;
    const float *rgb;
    const int32_t *indices, *counts;
    int32_t n_rows;
    const float *crop, *t_hit;
    const int32_t *closest;
    int mode;
    const float *gauss_normals;
    int N;
    DfIndex ix;
    const float *records;
};

// one neighbour of the analytical normal at x = p + t dir: g += w M (M^T (x - mu)), w = o exp(-clamp(|M^T (x - mu)|^2, 0, 1e8) / 2),
// x - mu formed as the ray kernel forms it, (p - mu) + t dir
__device__ __forceinline__ void ls_grad_term(const float *__restrict__ records, int gi, const float p[3], float t, const float dir[3], float g[3])
{
    const LsRecord rec = ls_record(records, gi);
    const float *Mm = rec.Mm;
    float v[3];
    const float w = ls_term(rec, (p[0] - rec.mu[0]) + t * dir[0], (p[1] - rec.mu[1]) + t * dir[1], (p[2] - rec.mu[2]) + t * dir[2], v);
#pragma unroll
    for (int r = 0; r < 3; ++r) g[r] += w * (Mm[3 * r] * v[0] + Mm[3 * r + 1] * v[1] + Mm[3 * r + 2] * v[2]);
}

// WRITE false: counts[block] = kept rows of the block; WRITE true: counts holds the exclusive prefix, base[0] the cursor before the call
template <bool WRITE>
__global__ __launch_bounds__(LS_THREADS) void ls_points_kernel(LsPoints f, int32_t *__restrict__ counts, const int64_t *__restrict__ base,
                                                                int64_t capacity, float *__restrict__ points, float *__restrict__ colors,
                                                                float *__restrict__ normals, int64_t *__restrict__ state)
{
    __shared__ int wave_tot[LS_WAVES];
    const long long j = (long long)blockIdx.x * LS_THREADS + threadIdx.x;
    const long long rows = f.counts ? (long long)f.counts[1] : (long long)f.n_rows;
    bool keep = false, bad = false;
    long long i = 0;
    float p[3], dir[3], x[3], t = 0.f;
    if (j < rows && j < f.n_rows) {
        i = (long long)f.indices[j];
        if (i < 0 || i >= f.cam.P) {
            bad = true;
        } else if (ls_point(f.cam, i, p, dir)) {
            t = f.t_hit[i];
            keep = t == t;                                              // nan: an empty pixel
#pragma unroll
            for (int a = 0; a < 3; ++a) x[a] = p[a] + t * dir[a];
            if (keep && f.crop) keep = dns_in_crop_box(f.crop, x);
        }
    }
    int total;
    const int rank = dns_block_rank<LS_THREADS>(keep, wave_tot, total);
    if (!WRITE) {
        if (threadIdx.x == 0) counts[blockIdx.x] = total;
        return;
    }
    if (bad) state[2] = 1;                                              // every writer stores the same value
    if (!keep) return;
    const int64_t at = base[0] + (int64_t)counts[blockIdx.x] + rank;
    if (at < 0 || at >= capacity) return;                               // the scan kernel has raised the overflow word
    float n[3] = {0.f, 0.f, 0.f};
    if (f.mode == DNSPLAT_LEVEL_NORMAL_CLOSEST) {
        const int c = f.closest[i];
        if ((unsigned)c < (unsigned)f.N) {
#pragma unroll
            for (int a = 0; a < 3; ++a) n[a] = f.gauss_normals[(size_t)c * 3 + a];
        }
    } else {
        DfList<LS_KM> L;
        float g[3] = {0.f, 0.f, 0.f};
        if (df_search(f.ix, p[0], p[1], p[2], LS_KM, L)) {
#pragma unroll
            for (int k = 1; k < LS_KM; ++k)
                if ((unsigned)L.i[k] < (unsigned)f.N) ls_grad_term(f.records, L.i[k], p, t, dir, g);
        }
        const float div = fmaxf(sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]), 1e-12f);
#pragma unroll
        for (int a = 0; a < 3; ++a) n[a] = -(g[a] / div);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        points[at * 3 + a] = x[a];
        colors[at * 3 + a] = f.rgb[i * 3 + a];
        normals[at * 3 + a] = n[a];
    }
}

long long ls_blocks(long long n, int per) { return (n + per - 1) / per; }

}  // namespace

extern "C" int dnsplat_level_rays(const dnsplat_level_rays_args *a, dnsplat_stream_t stream_)
{
    if (!a || !a->depth || !a->xform || !a->range || !a->records || !a->scales_log || !a->quats || !a->t_hit || !a->valid || !a->closest ||
        (!a->index && !a->neighbors) || a->width < 1 || a->height < 1 || a->n_levels < 1 || a->n_levels > DNSPLAT_LEVEL_MAX_LEVELS ||
        a->N < LS_KM || (a->lane_map != DNSPLAT_LEVEL_MAP_BLOCK && a->lane_map != DNSPLAT_LEVEL_MAP_ROW))
        return DNSPLAT_ERR_INVALID_ARG;
    const long long P = (long long)a->width * a->height;
    if (P > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;
    LsRays e;
    e.cam = dns_pixel_camera(*a);
    e.N = a->N;
    const bool search = a->neighbors == nullptr;
    if (search) e.ix = df_view(a->index, df_layout(a->N));
    else { e.ix.header = nullptr; e.ix.cell_start = nullptr; e.ix.sorted = nullptr; e.ix.G = 0; }
    e.records = a->records; e.scales = a->scales_log; e.quats = a->quats; e.range = a->range;
    e.nb32 = !search && !a->neighbors_int64 ? (const int32_t *)a->neighbors : nullptr;
    e.nb64 = !search && a->neighbors_int64 ? (const int64_t *)a->neighbors : nullptr;
    e.n_levels = a->n_levels;
    for (int l = 0; l < DNSPLAT_LEVEL_MAX_LEVELS; ++l) e.levels[l] = l < a->n_levels ? a->levels[l] : 0.f;
    e.tiles_x = (int)ls_blocks(a->width, LS_TILE);
    e.tiles = (long long)e.tiles_x * ls_blocks(a->height, LS_TILE);
    e.t_hit = a->t_hit; e.valid = a->valid; e.closest = a->closest; e.first_above = a->first_above; e.densities = a->densities;
    const bool row = a->lane_map == DNSPLAT_LEVEL_MAP_ROW;
    const long long nb = row ? ls_blocks(P, LS_THREADS) : ls_blocks(e.tiles, LS_WAVES);
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)nb), block(LS_THREADS);
    if (search) {
        if (row) hipLaunchKernelGGL((ls_rays_kernel<true, DNSPLAT_LEVEL_MAP_ROW>), grid, block, 0, stream, e);
        else hipLaunchKernelGGL((ls_rays_kernel<true, DNSPLAT_LEVEL_MAP_BLOCK>), grid, block, 0, stream, e);
    } else {
        if (row) hipLaunchKernelGGL((ls_rays_kernel<false, DNSPLAT_LEVEL_MAP_ROW>), grid, block, 0, stream, e);
        else hipLaunchKernelGGL((ls_rays_kernel<false, DNSPLAT_LEVEL_MAP_BLOCK>), grid, block, 0, stream, e);
    }
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_level_points(const dnsplat_level_points_args *a, dnsplat_stream_t stream_)
{
    if (!a || !a->depth || !a->rgb || !a->indices || !a->xform || !a->t_hit || !a->points || !a->colors || !a->normals || !a->state ||
        !a->scratch || a->width < 1 || a->height < 1 || a->capacity < 1 || a->n_rows < 0)
        return DNSPLAT_ERR_INVALID_ARG;
    if (a->normal_mode == DNSPLAT_LEVEL_NORMAL_CLOSEST) {
        if (!a->closest || !a->gauss_normals || a->N < 1) return DNSPLAT_ERR_INVALID_ARG;
    } else if (a->normal_mode == DNSPLAT_LEVEL_NORMAL_ANALYTICAL) {
        if (!a->index || !a->records || a->N < LS_KM) return DNSPLAT_ERR_INVALID_ARG;
    } else {
        return DNSPLAT_ERR_INVALID_ARG;
    }
    const long long P = (long long)a->width * a->height;
    if (P > 0x7fffffffLL) return DNSPLAT_ERR_UNSUPPORTED;
    if (a->n_rows == 0) return DNSPLAT_OK;
    LsPoints f;
    f.cam = dns_pixel_camera(*a);
    f.rgb = a->rgb; f.indices = a->indices; f.counts = a->counts; f.n_rows = a->n_rows;
    f.crop = a->crop; f.t_hit = a->t_hit; f.closest = a->closest; f.mode = a->normal_mode; f.gauss_normals = a->gauss_normals;
    f.N = a->N; f.records = a->records;
    if (a->normal_mode == DNSPLAT_LEVEL_NORMAL_ANALYTICAL) f.ix = df_view(a->index, df_layout(a->N));
    else { f.ix.header = nullptr; f.ix.cell_start = nullptr; f.ix.sorted = nullptr; f.ix.G = 0; }
    hipStream_t stream = (hipStream_t)stream_;
    const int nb = (int)ls_blocks(a->n_rows, LS_THREADS);
    int64_t *base = (int64_t *)a->scratch;
    int32_t *block_counts = (int32_t *)((char *)a->scratch + 16);
    hipLaunchKernelGGL((ls_points_kernel<false>), dim3(nb), dim3(LS_THREADS), 0, stream, f, block_counts, (const int64_t *)base, a->capacity,
                       a->points, a->colors, a->normals, a->state);
    hipLaunchKernelGGL(dns_append_scan_kernel<LS_THREADS>, dim3(1), dim3(LS_THREADS), 0, stream, nb, block_counts, a->capacity, a->state, base);
    hipLaunchKernelGGL((ls_points_kernel<true>), dim3(nb), dim3(LS_THREADS), 0, stream, f, block_counts, (const int64_t *)base, a->capacity,
                       a->points, a->colors, a->normals, a->state);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
