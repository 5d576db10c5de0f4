// pointcloud.hip — the per-frame tail of the reference's `gs-mesh dn` exporter (export_mesh.py:351-476 DepthAndNormalMapsPoisson, with
// :58-90 find_depth_edges, :50-55 pick_indices_at_random and utils/camera_utils.py:92-210 get_colored_points_from_depth): an oriented,
// coloured point cloud from a rendered depth, colour and surface-normal image.  Three entry points, none of which reads anything on the
// host:
//   dnsplat_depth_edge_valid      valid = not (dilated edge of the inverse-depth Laplacian).  pc_edge_bits_kernel: one wave per 64 pixels
//                                 of a row, the threshold decisions of the wave go out as one 64-bit word (ballot).  pc_edge_dilate_kernel:
//                                 one workgroup per PC_TH rows x PC_TW words; the rows y0 - itr .. y0 + PC_TH - 1 + itr are dilated
//                                 horizontally (shift-and-OR over the word and its two neighbours) into LDS, each thread ORs 2 itr + 1 of
//                                 them, and the workgroup writes the bytes.  "An edge within Chebyshev distance itr" — what itr rounds of
//                                 the reference's 3 x 3 all-ones conv2d followed by > 0 compute — directly, for any 0 <= itr <= 64.
//   dnsplat_sample_valid_pixels   m = min(k, n) of the n valid pixels, uniformly without replacement: count per 1024 pixels, one-workgroup
//                                 scan, ascending compaction, then indices[t] = compact[pi(t)] with pi a keyed bijection of [0, n)
//                                 (balanced Feistel network + cycle walking, dnsplat.h).  n stays on the device.
//   dnsplat_backproject_points    one thread per selected pixel: camera point, world point, colour, world normal, crop-box test; the kept
//                                 rows are appended in order behind a device cursor (flag count per 256 rows, one-workgroup scan that
//                                 also moves the cursor, then the same computation again with the write).
// No atomic anywhere and no sum whose order depends on scheduling: equal inputs (and seed) give equal bits.  Compiled without
// contraction: every product and sum below is the single fp32 operation torch performs.

#include "block_reduce.h"
#include "pixel_camera.h"

namespace {

constexpr int PC_THREADS = 256;
constexpr int PC_WAVES = PC_THREADS / DNS_WAVE;
constexpr int PC_TH = DNSPLAT_EDGE_ROW_TILE;             // rows of a dilation tile
constexpr int PC_TW = 8;                                 // 64-pixel words of a dilation tile: thread t owns row t / 8, word t % 8
constexpr int PC_MAX_ITR = DNSPLAT_EDGE_MAX_DILATION;    // one neighbouring word on each side reaches 64 pixels
constexpr int PC_SAMPLE_PER = 4;                         // pixels per thread of the sampler's count / compaction kernels
constexpr int PC_SAMPLE_BLOCK = PC_THREADS * PC_SAMPLE_PER;
constexpr float PC_EPS = 1e-6f;                          // find_depth_edges: 1 / (depth + 1e-6)

static_assert(PC_TH * PC_TW == PC_THREADS, "one thread per (row, word) of a dilation tile");

// ---- the sampler's scan -------------------------------------------------------------------------------------------------------------

// One workgroup turns counts[0 .. nb) into their exclusive prefix sums in place and hands the total on: words = {n, min(k, n)}
__global__ __launch_bounds__(PC_THREADS) void pc_scan_kernel(int nb, int32_t *__restrict__ counts, int32_t k, int32_t *__restrict__ words)
{
    const int n = dns_scan_in_place<PC_THREADS, 1>(nb, counts);
    if (threadIdx.x == 0) {
        words[0] = n;
        words[1] = n < k ? n : k;
    }
}

// ---- the edge map --------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float pc_inverse_depth(const float *__restrict__ depth, int x, int y, int W, int H)
{
    if (x < 0 || x >= W || y < 0 || y >= H) return 0.f;                      // conv2d pads with zeros
    return __fdiv_rn(1.0f, __fadd_rn(depth[(size_t)y * W + x], PC_EPS));
}

// bits[y * words + w] bit b = the Laplacian of 1 / (depth + 1e-6) at (w * 64 + b, y) exceeds the threshold; bits past the row's end are 0
__global__ __launch_bounds__(PC_THREADS) void pc_edge_bits_kernel(int W, int H, int words, long long units, const float *__restrict__ depth,
                                                                   float threshold, uint64_t *__restrict__ bits)
{
    const long long u = (long long)blockIdx.x * PC_WAVES + threadIdx.x / DNS_WAVE;   // uniform over the wave
    if (u >= units) return;
    const int lane = threadIdx.x & (DNS_WAVE - 1);
    const int y = (int)(u / words), w = (int)(u - (long long)y * words);
    const int x = w * DNS_WAVE + lane;
    bool edge = false;
    if (x < W) {
        const float up = pc_inverse_depth(depth, x, y - 1, W, H), down = pc_inverse_depth(depth, x, y + 1, W, H);
        const float left = pc_inverse_depth(depth, x - 1, y, W, H), right = pc_inverse_depth(depth, x + 1, y, W, H);
        const float mid = pc_inverse_depth(depth, x, y, W, H);
        const float lap = __fsub_rn(__fadd_rn(__fadd_rn(__fadd_rn(up, down), left), right), __fmul_rn(4.0f, mid));
        edge = lap > threshold;                                              // nan > threshold is false
    }
    const uint64_t b = dns_ballot(edge);
    if (lane == 0) bits[u] = b;
}

// the word `mid` with every bit spread over the itr positions to either side of it; lo and hi are the words before and after it
__device__ __forceinline__ uint64_t pc_spread(uint64_t lo, uint64_t mid, uint64_t hi, int itr)
{
    uint64_t out = mid;
    for (int s = 1; s <= itr; ++s) {
        const uint64_t keep_up = s < 64 ? mid << s : 0ull, keep_down = s < 64 ? mid >> s : 0ull;
        out |= keep_up | (lo >> (64 - s)) | keep_down | (hi << (64 - s));    // 1 <= s <= 64: both shifts of lo / hi are by 0 .. 63
    }
    return out;
}

__global__ __launch_bounds__(PC_THREADS) void pc_edge_dilate_kernel(int W, int H, int words, int tiles_x, int itr,
                                                                     const uint64_t *__restrict__ bits, uint8_t *__restrict__ valid)
{
    __shared__ uint64_t rows[PC_TH + 2 * PC_MAX_ITR][PC_TW];                  // horizontally dilated rows y0 - itr .. y0 + PC_TH - 1 + itr
    __shared__ uint64_t done[PC_TH][PC_TW];
    const int t = threadIdx.x;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int y0 = tile_y * PC_TH, w0 = tile_x * PC_TW;
    const int n_rows = PC_TH + 2 * itr;
    for (int i = t; i < n_rows * PC_TW; i += PC_THREADS) {
        const int r = i / PC_TW, c = i - r * PC_TW;
        const int y = y0 - itr + r, w = w0 + c;
        uint64_t v = 0;
        if (y >= 0 && y < H && w < words) {
            const uint64_t *row = bits + (size_t)y * words;
            v = pc_spread(w > 0 ? row[w - 1] : 0ull, row[w], w + 1 < words ? row[w + 1] : 0ull, itr);
        }
        rows[r][c] = v;
    }
    __syncthreads();
    {
        const int r = t / PC_TW, c = t - r * PC_TW;
        uint64_t v = 0;
        for (int dy = 0; dy <= 2 * itr; ++dy) v |= rows[r + dy][c];
        done[r][c] = v;
    }
    __syncthreads();
    for (int r = 0; r < PC_TH; ++r) {
        const int y = y0 + r;
        if (y >= H) break;
        for (int p = t; p < PC_TW * DNS_WAVE; p += PC_THREADS) {
            const int x = w0 * DNS_WAVE + p;
            if (x < W) valid[(size_t)y * W + x] = (uint8_t)(((done[r][p / DNS_WAVE] >> (p & (DNS_WAVE - 1))) & 1ull) == 0ull);
        }
    }
}

// ---- the sampler ---------------------------------------------------------------------------------------------------------------------

// the keyed bijection of [0, n) that dnsplat.h states, on dns_mix32 (block_reduce.h)
__device__ __forceinline__ uint32_t pc_permute(uint32_t t, uint32_t n, uint64_t seed)
{
    const int bits = n > 1u ? 32 - __clz(n - 1u) : 0;
    const int half = bits > 2 ? (bits + 1) / 2 : 1;
    const uint32_t mask = (1u << half) - 1u;
    uint32_t key[DNSPLAT_SAMPLE_ROUNDS];
#pragma unroll
    for (int r = 0; r < DNSPLAT_SAMPLE_ROUNDS; ++r)
        key[r] = dns_mix32((uint32_t)seed ^ dns_mix32((uint32_t)(seed >> 32) + 0x9e3779b9u * (uint32_t)(r + 1)));
    uint32_t x = t;
    do {
        uint32_t L = x >> half, R = x & mask;
#pragma unroll
        for (int r = 0; r < DNSPLAT_SAMPLE_ROUNDS; ++r) {
            const uint32_t f = dns_mix32(R ^ key[r]) & mask;
            const uint32_t nr = L ^ f;
            L = R;
            R = nr;
        }
        x = (L << half) | R;
    } while (x >= n);                                                        // cycle walking: t < n lies on a cycle that returns below n
    return x;
}

__device__ __forceinline__ bool pc_pixel_valid(const uint8_t *__restrict__ valid, const float *__restrict__ depth, long long i)
{
    return valid ? valid[i] != 0 : !(depth[i] == 0.f);                       // torch.nonzero of the depth image: a nan depth is valid
}

// WRITE false: counts[block] = valid pixels among the block's PC_SAMPLE_BLOCK; WRITE true: counts holds the exclusive prefix and the
// valid pixels go to compact[] in ascending order
template <bool WRITE>
__global__ __launch_bounds__(PC_THREADS) void pc_valid_kernel(long long P, const uint8_t *__restrict__ valid, const float *__restrict__ depth,
                                                               int32_t *__restrict__ counts, int32_t *__restrict__ compact)
{
    __shared__ int wave_tot[PC_WAVES];
    const int t = threadIdx.x;
    int at = WRITE ? counts[blockIdx.x] : 0;
#pragma unroll
    for (int j = 0; j < PC_SAMPLE_PER; ++j) {
        const long long i = (long long)blockIdx.x * PC_SAMPLE_BLOCK + j * PC_THREADS + t;
        const bool v = i < P && pc_pixel_valid(valid, depth, i);
        int total;
        const int rank = dns_block_rank<PC_THREADS>(v, wave_tot, total);
        if (WRITE && v) compact[at + rank] = (int32_t)i;
        at += total;
    }
    if (!WRITE && t == 0) counts[blockIdx.x] = at;
}

__global__ __launch_bounds__(PC_THREADS) void pc_pick_kernel(int32_t k, uint64_t seed, const int32_t *__restrict__ words,
                                                              const int32_t *__restrict__ compact, int32_t *__restrict__ indices)
{
    const long long t = (long long)blockIdx.x * PC_THREADS + threadIdx.x;
    if (t >= k) return;
    const int32_t n = words[0], m = words[1];
    int32_t out = -1;
    if (t < m) out = n <= k ? compact[t] : compact[pc_permute((uint32_t)t, (uint32_t)n, seed)];
    indices[t] = out;
}

// ---- back-projection -----------------------------------------------------------------------------------------------------------------

struct PcFrame {
    DnsPixelCamera cam;
    const float *rgb, *normal;
    const int32_t *indices, *counts;
    int32_t n_rows;
    const float *crop;
};

struct PcRow {
    float p[3], c[3], n[3];
    bool keep, bad;
};

__device__ __forceinline__ PcRow pc_row(const PcFrame &f, long long j)
{
    PcRow o;
    o.keep = false;
    o.bad = false;
    const long long rows = f.indices ? (f.counts ? (long long)f.counts[1] : (long long)f.n_rows) : f.cam.P;
    if (j >= rows || (f.indices && j >= f.n_rows)) return o;
    const long long i = f.indices ? (long long)f.indices[j] : j;
    if (i < 0 || i >= f.cam.P) { o.bad = true; return o; }
    dns_pixel_point(f.cam, i, dns_pixel_depth(f.cam, i), o.p);               // no gate on the depth here: the selection made it
    const float *R = f.cam.xform + 12;
#pragma unroll
    for (int c = 0; c < 3; ++c) o.c[c] = f.rgb[i * 3 + c];
    if (f.normal) {
        // export_mesh.py:414-425: 2 s - 1, y and z flipped, F.normalize (x / max(|x|, 1e-12)), then the camera's rotation
        const float n0 = __fsub_rn(__fmul_rn(2.0f, f.normal[i * 3 + 0]), 1.0f);
        const float n1 = -__fsub_rn(__fmul_rn(2.0f, f.normal[i * 3 + 1]), 1.0f);
        const float n2 = -__fsub_rn(__fmul_rn(2.0f, f.normal[i * 3 + 2]), 1.0f);
        const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(n0, n0), __fmul_rn(n1, n1)), __fmul_rn(n2, n2)));
        const float div = fmaxf(len, 1e-12f);
        const float u0 = __fdiv_rn(n0, div), u1 = __fdiv_rn(n1, div), u2 = __fdiv_rn(n2, div);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            o.n[c] = __fadd_rn(__fadd_rn(__fmul_rn(R[3 * c], u0), __fmul_rn(R[3 * c + 1], u1)), __fmul_rn(R[3 * c + 2], u2));
    } else {
        o.n[0] = o.n[1] = o.n[2] = 0.f;
    }
    o.keep = !f.crop || dns_in_crop_box(f.crop, o.p);
    return o;
}

// WRITE false: counts[block] = kept rows of the block; WRITE true: counts holds the exclusive prefix, base[0] the cursor before the call
template <bool WRITE>
__global__ __launch_bounds__(PC_THREADS) void pc_backproject_kernel(PcFrame f, int32_t *__restrict__ counts, const int64_t *__restrict__ base,
                                                                     int64_t capacity, float *__restrict__ points, float *__restrict__ colors,
                                                                     float *__restrict__ normals, int64_t *__restrict__ state)
{
    __shared__ int wave_tot[PC_WAVES];
    const long long j = (long long)blockIdx.x * PC_THREADS + threadIdx.x;
    const PcRow o = pc_row(f, j);
    int total;
    const int rank = dns_block_rank<PC_THREADS>(o.keep, wave_tot, total);
    if (!WRITE) {
        if (threadIdx.x == 0) counts[blockIdx.x] = total;
        return;
    }
    if (o.bad) state[2] = 1;                                                 // every writer stores the same value
    if (!o.keep) return;
    const int64_t at = base[0] + (int64_t)counts[blockIdx.x] + rank;
    if (at < 0 || at >= capacity) return;                                    // the scan kernel has raised the overflow word
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        points[at * 3 + c] = o.p[c];
        colors[at * 3 + c] = o.c[c];
        if (normals) normals[at * 3 + c] = o.n[c];
    }
}

long long pc_blocks(long long n, int per) { return (n + per - 1) / per; }

bool pc_frame_ok(int32_t width, int32_t height) { return (long long)width * (long long)height <= 0x7fffffffLL; }

}  // namespace

extern "C" size_t dnsplat_pointcloud_scratch_bytes(int32_t width, int32_t height, int32_t k)
{
    if (width < 1 || height < 1 || k < 0 || !pc_frame_ok(width, height)) return 0;
    const long long P = (long long)width * height;
    const long long words = pc_blocks(width, DNS_WAVE);
    const size_t edge = (size_t)height * (size_t)words * sizeof(uint64_t);
    const size_t sample = ((size_t)pc_blocks(P, PC_SAMPLE_BLOCK) + (size_t)P) * sizeof(int32_t);
    const long long rows = P > k ? P : (long long)k;
    const size_t append = 16 + (size_t)pc_blocks(rows, PC_THREADS) * sizeof(int32_t);
    size_t need = edge > sample ? edge : sample;
    if (append > need) need = append;
    return (need + 15) & ~(size_t)15;
}

extern "C" int dnsplat_depth_edge_valid(int32_t width, int32_t height, const float *depth, float threshold, int32_t dilation_itr,
                                        uint8_t *valid, void *scratch, dnsplat_stream_t stream_)
{
    if (!depth || !valid || !scratch || width < 1 || height < 1) return DNSPLAT_ERR_INVALID_ARG;
    if (dilation_itr < 0 || dilation_itr > PC_MAX_ITR || !pc_frame_ok(width, height)) return DNSPLAT_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const int words = (int)pc_blocks(width, DNS_WAVE);
    const long long units = (long long)height * words;
    uint64_t *bits = (uint64_t *)scratch;
    hipLaunchKernelGGL(pc_edge_bits_kernel, dim3((unsigned)pc_blocks(units, PC_WAVES)), dim3(PC_THREADS), 0, stream, width, height, words, units,
                       depth, threshold, bits);
    const int tiles_x = (int)pc_blocks(words, PC_TW);
    const long long tiles = (long long)tiles_x * pc_blocks(height, PC_TH);
    hipLaunchKernelGGL(pc_edge_dilate_kernel, dim3((unsigned)tiles), dim3(PC_THREADS), 0, stream, width, height, words, tiles_x, dilation_itr,
                       (const uint64_t *)bits, valid);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_sample_valid_pixels(int32_t width, int32_t height, const uint8_t *valid, const float *depth, int32_t k, uint64_t seed,
                                           int32_t *indices, int32_t *counts, void *scratch, dnsplat_stream_t stream_)
{
    if ((!valid && !depth) || !counts || !scratch || width < 1 || height < 1 || k < 0 || (k > 0 && !indices)) return DNSPLAT_ERR_INVALID_ARG;
    if (!pc_frame_ok(width, height)) return DNSPLAT_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const long long P = (long long)width * height;
    const int nb = (int)pc_blocks(P, PC_SAMPLE_BLOCK);
    int32_t *block_counts = (int32_t *)scratch, *compact = block_counts + nb;
    hipLaunchKernelGGL((pc_valid_kernel<false>), dim3(nb), dim3(PC_THREADS), 0, stream, P, valid, depth, block_counts, compact);
    hipLaunchKernelGGL(pc_scan_kernel, dim3(1), dim3(PC_THREADS), 0, stream, nb, block_counts, k, counts);
    hipLaunchKernelGGL((pc_valid_kernel<true>), dim3(nb), dim3(PC_THREADS), 0, stream, P, valid, depth, block_counts, compact);
    if (k > 0)
        hipLaunchKernelGGL(pc_pick_kernel, dim3((unsigned)pc_blocks(k, PC_THREADS)), dim3(PC_THREADS), 0, stream, k, seed, (const int32_t *)counts,
                           (const int32_t *)compact, indices);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_backproject_points(const dnsplat_backproject_args *a, dnsplat_stream_t stream_)
{
    if (!a || !a->depth || !a->rgb || !a->xform || !a->points || !a->colors || !a->state || !a->scratch || a->width < 1 || a->height < 1 ||
        a->capacity < 1 || (a->normal && !a->normals) || (a->indices && a->n_rows < 0))
        return DNSPLAT_ERR_INVALID_ARG;
    if (!pc_frame_ok(a->width, a->height)) return DNSPLAT_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    PcFrame f;
    f.cam = dns_pixel_camera(*a);
    f.rgb = a->rgb; f.normal = a->normal;
    f.indices = a->indices; f.counts = a->indices ? a->counts : nullptr; f.n_rows = a->n_rows;
    f.crop = a->crop;
    const long long rows = a->indices ? (long long)a->n_rows : f.cam.P;
    if (rows == 0) return DNSPLAT_OK;
    const int nb = (int)pc_blocks(rows, PC_THREADS);
    int64_t *base = (int64_t *)a->scratch;
    int32_t *block_counts = (int32_t *)((char *)a->scratch + 16);
    float *normals = a->normal ? a->normals : nullptr;
    hipLaunchKernelGGL((pc_backproject_kernel<false>), dim3(nb), dim3(PC_THREADS), 0, stream, f, block_counts, (const int64_t *)base, a->capacity,
                       a->points, a->colors, normals, a->state);
    hipLaunchKernelGGL(dns_append_scan_kernel<PC_THREADS>, dim3(1), dim3(PC_THREADS), 0, stream, nb, block_counts, a->capacity, a->state, base);
    hipLaunchKernelGGL((pc_backproject_kernel<true>), dim3(nb), dim3(PC_THREADS), 0, stream, f, block_counts, (const int64_t *)base, a->capacity,
                       a->points, a->colors, normals, a->state);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
