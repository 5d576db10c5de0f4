// pearson.hip — dn-splatter's Pearson depth losses and their gradient (depth_loss_type = PearsonDepth; restates
// dn_splatter/losses.py:428-485 PearsonDepthLoss / LocalPearsonDepthLoss as regularization_strategy.py:167-177 combines them).
//
// A REGION is the whole frame (optionally the pixels of a bool mask) or one box x box window.  Per region, with a = p - mean(p),
// b = t - mean(t), s = unbiased std, e = 1e-6:   co = mean(a b) / ((s_p + e)(s_t + e)),  loss = 1 - co.
// The reference evaluates its n_corr boxes in a Python loop, slicing each with device scalars; here:
//   pearson_frame_sums_kernel / _moments_kernel   two sweeps over the frame (count, sum p, sum t; then the CENTRED second moments),
//                                                 one partial per workgroup, added up in a fixed order;
//   pearson_box_kernel                            one workgroup per box, both sweeps (a box of <= 128 x 128 stays in registers);
//   pearson_finish_kernel                         the frame's coefficients, the two loss sums;
//   pearson_grad_kernel                           one thread per pixel: within a region the gradient is affine in the pixel's own two
//                                                 values, d loss / d p_j = alpha b_j + beta a_j, so a thread walks the region table
//                                                 (staged through LDS in pieces) and adds the regions that hold its pixel, in table order.
// Sums and coefficients are kept in double (a few adds per pixel beside two loads: the kernels are memory-bound), every reduction is the
// fixed tree of block_reduce.h (dns_block_join, dns_fold_partials) and there is no atomic: equal inputs give equal bits.  Raw one-pass
// fp32 moments lose the variance of a low-contrast frame (5 + 0.01 u over 1600 x 1200: 8 % off), hence two sweeps.

#include "block_reduce.h"

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_FRAME_BLOCKS = 512;     // workgroups (= partials) of the two frame sweeps
constexpr int PS_GRAD_BLOCKS = 4096;     // grid cap of the gradient kernel, as the sibling loss kernels
constexpr int PS_REG_PIXELS = 64;        // pixels per lane a box may keep in registers: 256 x 64 = 128 x 128
constexpr int PS_PIECE = 128;            // region-table entries staged in LDS at a time (6 KiB)
constexpr double PS_EPS = 1e-6;

struct PearsonRegion {                   // 48 bytes
    double mu_p, mu_t, alpha, beta, loss;
    int32_t row0, col0;
};

struct PsSums {                          // 24 bytes: three sums of one sweep, reduced together
    double v[3];
    static __device__ PsSums identity() { return PsSums{{0.0, 0.0, 0.0}}; }
    __device__ void join(const PsSums &o) { v[0] += o.v[0]; v[1] += o.v[1]; v[2] += o.v[2]; }
};

struct PearsonScratch {                  // layout of the caller's scratch (dnsplat_pearson_scratch_bytes)
    double *part1, *part2;               // [PS_FRAME_BLOCKS][3] each: the kernels read and write them as PsSums
    PearsonRegion *frame;                // [1]
    PearsonRegion *boxes;                // [n_boxes]
};

// mean-centred moments -> what the gradient pass needs.  n < 2: 0 / 0, nan as the reference's std of one element.  s_p == 0 (a
// constant prediction): the value is 1 - 0; autograd's std backward sends no gradient through a standard deviation of exactly zero,
// what is left is the path through the numerator, alpha b_j with s_p + e = e.
__device__ __forceinline__ void pearson_coefficients(double n, double mu_p, double mu_t, double m2p, double m2t, double cpt, int row0, int col0,
                                                     PearsonRegion *out)
{
    const double sp = sqrt(m2p / (n - 1.0)), st = sqrt(m2t / (n - 1.0));
    const double dp = sp + PS_EPS, dt = st + PS_EPS;
    PearsonRegion r;
    r.mu_p = mu_p; r.mu_t = mu_t;
    r.loss = 1.0 - cpt / (n * dp * dt);
    r.alpha = -1.0 / (n * dp * dt);
    r.beta = sp == 0.0 ? 0.0 : cpt / (n * dp * dp * dt * (n - 1.0) * sp);
    r.row0 = row0; r.col0 = col0;
    *out = r;
}

__global__ __launch_bounds__(PS_THREADS) void pearson_frame_sums_kernel(long long P, const float *__restrict__ pred, const float *__restrict__ gt,
                                                                         const uint8_t *__restrict__ mask, double *__restrict__ part1)
{
    __shared__ PsSums red[PS_THREADS / DNS_WAVE];
    PsSums acc = PsSums::identity();
    double (&v)[3] = acc.v;
    for (long long px = (long long)blockIdx.x * PS_THREADS + threadIdx.x; px < P; px += (long long)gridDim.x * PS_THREADS)
        if (!mask || mask[px]) { v[0] += 1.0; v[1] += (double)pred[px]; v[2] += (double)gt[px]; }
    dns_block_join<PS_THREADS>(acc, red);
    if (threadIdx.x == 0) ((PsSums *)part1)[blockIdx.x] = acc;
}

__global__ __launch_bounds__(PS_THREADS) void pearson_frame_moments_kernel(long long P, const float *__restrict__ pred, const float *__restrict__ gt,
                                                                            const uint8_t *__restrict__ mask, const double *__restrict__ part1,
                                                                            double *__restrict__ part2)
{
    __shared__ PsSums red[PS_THREADS / DNS_WAVE];
    PsSums acc;
    dns_fold_partials<PS_THREADS>((const PsSums *)part1, gridDim.x, acc, red);   // every workgroup gets the same bits
    double (&v)[3] = acc.v;
    const double mu_p = v[1] / v[0], mu_t = v[2] / v[0];
    acc = PsSums::identity();
    for (long long px = (long long)blockIdx.x * PS_THREADS + threadIdx.x; px < P; px += (long long)gridDim.x * PS_THREADS)
        if (!mask || mask[px]) {
            const double a = (double)pred[px] - mu_p, b = (double)gt[px] - mu_t;
            v[0] += a * a; v[1] += b * b; v[2] += a * b;
        }
    dns_block_join<PS_THREADS>(acc, red);
    if (threadIdx.x == 0) ((PsSums *)part2)[blockIdx.x] = acc;
}

// One workgroup per box.  REG: the box is at most PS_REG_PIXELS pixels per lane and stays in registers between the two sweeps;
// otherwise the second sweep reads it again.  Origins outside [0, H - box] x [0, W - box] are clamped into it.
template <bool REG>
__global__ __launch_bounds__(PS_THREADS) void pearson_box_kernel(int W, int H, int box, const float *__restrict__ pred, const float *__restrict__ gt,
                                                                  const int64_t *__restrict__ rows, const int64_t *__restrict__ cols,
                                                                  PearsonRegion *__restrict__ regions)
{
    __shared__ PsSums red[PS_THREADS / DNS_WAVE];
    const long long r64 = rows[blockIdx.x], c64 = cols[blockIdx.x];
    const int row0 = (int)(r64 < 0 ? 0 : (r64 > H - box ? H - box : r64)), col0 = (int)(c64 < 0 ? 0 : (c64 > W - box ? W - box : c64));
    const int n = box * box;                                  // box <= 46340 is checked at launch
    const size_t base = (size_t)row0 * W + col0;
    float p[REG ? PS_REG_PIXELS : 1], t[REG ? PS_REG_PIXELS : 1];
    PsSums acc = PsSums::identity();
    double (&v)[3] = acc.v;
    if (REG) {
#pragma unroll
        for (int k = 0; k < PS_REG_PIXELS; ++k) {
            const int e = (int)threadIdx.x + k * PS_THREADS;
            p[k] = 0.f; t[k] = 0.f;
            if (e < n) {
                const int r = e / box, c = e - r * box;
                const size_t px = base + (size_t)r * W + c;
                p[k] = pred[px]; t[k] = gt[px];
            }
        }
#pragma unroll
        for (int k = 0; k < PS_REG_PIXELS; ++k) { v[1] += (double)p[k]; v[2] += (double)t[k]; }   // pixels beyond the box hold 0
    } else {
        for (int e = threadIdx.x; e < n; e += PS_THREADS) {
            const int r = e / box, c = e - r * box;
            const size_t px = base + (size_t)r * W + c;
            v[1] += (double)pred[px]; v[2] += (double)gt[px];
        }
    }
    dns_block_join<PS_THREADS>(acc, red);
    const double mu_p = v[1] / (double)n, mu_t = v[2] / (double)n;
    acc = PsSums::identity();
    if (REG) {
#pragma unroll
        for (int k = 0; k < PS_REG_PIXELS; ++k)
            if ((int)threadIdx.x + k * PS_THREADS < n) {
                const double a = (double)p[k] - mu_p, b = (double)t[k] - mu_t;
                v[0] += a * a; v[1] += b * b; v[2] += a * b;
            }
    } else {
        for (int e = threadIdx.x; e < n; e += PS_THREADS) {
            const int r = e / box, c = e - r * box;
            const size_t px = base + (size_t)r * W + c;
            const double a = (double)pred[px] - mu_p, b = (double)gt[px] - mu_t;
            v[0] += a * a; v[1] += b * b; v[2] += a * b;
        }
    }
    dns_block_join<PS_THREADS>(acc, red);
    if (threadIdx.x == 0) pearson_coefficients((double)n, mu_p, mu_t, v[0], v[1], v[2], row0, col0, regions + blockIdx.x);
}

// sums[0] = the frame's 1 - co (0 without the frame), sums[1] = sum over the boxes of 1 - co_b in table order (0 without boxes)
__global__ __launch_bounds__(PS_THREADS) void pearson_finish_kernel(int whole, int n_part, const double *__restrict__ part1, const double *__restrict__ part2,
                                                                     PearsonRegion *__restrict__ frame, int n_boxes,
                                                                     const PearsonRegion *__restrict__ boxes, float *__restrict__ sums)
{
    __shared__ PsSums red[PS_THREADS / DNS_WAVE];
    if (whole) {
        PsSums s1, s2;
        dns_fold_partials<PS_THREADS>((const PsSums *)part1, n_part, s1, red);
        dns_fold_partials<PS_THREADS>((const PsSums *)part2, n_part, s2, red);
        if (threadIdx.x == 0) {
            pearson_coefficients(s1.v[0], s1.v[1] / s1.v[0], s1.v[2] / s1.v[0], s2.v[0], s2.v[1], s2.v[2], 0, 0, frame);
            sums[0] = (float)frame->loss;
        }
    } else if (threadIdx.x == 0) {
        sums[0] = 0.f;
    }
    PsSums acc = PsSums::identity();
    for (int i = threadIdx.x; i < n_boxes; i += PS_THREADS) acc.v[0] += boxes[i].loss;
    dns_block_join<PS_THREADS>(acc, red);
    if (threadIdx.x == 0) sums[1] = (float)acc.v[0];
}

__global__ __launch_bounds__(PS_THREADS) void pearson_grad_kernel(int W, int H, int box, const float *__restrict__ pred, const float *__restrict__ gt,
                                                                   const uint8_t *__restrict__ mask, const PearsonRegion *__restrict__ frame,
                                                                   int n_boxes, const PearsonRegion *__restrict__ boxes, float w_whole, float w_box,
                                                                   float *__restrict__ v_pred)
{
    __shared__ PearsonRegion piece[PS_PIECE];
    const long long P = (long long)W * H;
    const long long stride = (long long)gridDim.x * PS_THREADS;
    // every lane makes the same number of trips (the pieces are staged by the whole workgroup)
    for (long long first = (long long)blockIdx.x * PS_THREADS; first < P; first += stride) {
        const long long px = first + threadIdx.x;
        const bool in = px < P;
        const long long q = in ? px : P - 1;
        const int i = (int)(q / W), j = (int)(q - (long long)i * W);
        const double p = (double)pred[q], t = (double)gt[q];
        double g_whole = 0.0, g_box = 0.0;
        if (frame && (!mask || mask[q])) g_whole = frame->alpha * (t - frame->mu_t) + frame->beta * (p - frame->mu_p);
        for (int b0 = 0; b0 < n_boxes; b0 += PS_PIECE) {
            const int m = min(PS_PIECE, n_boxes - b0);
            __syncthreads();
            if ((int)threadIdx.x < m) piece[threadIdx.x] = boxes[b0 + threadIdx.x];
            __syncthreads();
            for (int k = 0; k < m; ++k) {
                const PearsonRegion &r = piece[k];
                if ((unsigned)(i - r.row0) < (unsigned)box && (unsigned)(j - r.col0) < (unsigned)box)
                    g_box += r.alpha * (t - r.mu_t) + r.beta * (p - r.mu_p);
            }
        }
        // two rounded products and one rounded sum: the weighted sum of the two separate calls, bit for bit
        if (in) v_pred[px] = __fadd_rn(__fmul_rn(w_whole, (float)g_whole), __fmul_rn(w_box, (float)g_box));
    }
}

PearsonScratch carve(void *scratch)
{
    PearsonScratch s;
    s.part1 = (double *)scratch;
    s.part2 = s.part1 + 3 * PS_FRAME_BLOCKS;
    s.frame = (PearsonRegion *)(s.part2 + 3 * PS_FRAME_BLOCKS);
    s.boxes = s.frame + 1;
    return s;
}

}  // namespace

extern "C" size_t dnsplat_pearson_scratch_bytes(int32_t n_boxes)
{
    if (n_boxes < 0) return 0;
    return 2 * 3 * PS_FRAME_BLOCKS * sizeof(double) + ((size_t)n_boxes + 1) * sizeof(PearsonRegion);
}

extern "C" int dnsplat_pearson_depth(int32_t width, int32_t height, const float *pred, const float *gt, const uint8_t *mask, int32_t whole,
                                     int32_t n_boxes, int32_t box, const int64_t *box_rows, const int64_t *box_cols, float w_whole,
                                     float w_box, float *v_pred, void *scratch, float *sums, dnsplat_stream_t stream_)
{
    if (!pred || !gt || !scratch || !sums || width < 1 || height < 1 || n_boxes < 0) return DNSPLAT_ERR_INVALID_ARG;
    if (n_boxes > 0 && (!box_rows || !box_cols || box < 2 || box > (width < height ? width : height))) return DNSPLAT_ERR_INVALID_ARG;
    if (n_boxes > 0 && box > 46340) return DNSPLAT_ERR_UNSUPPORTED;               // box * box is an int
    // without boxes, box and the origins are not looked at (the whole-frame call has no box to name)
    if (mask && !whole) return DNSPLAT_ERR_INVALID_ARG;                            // the mask belongs to the whole-frame region
    hipStream_t stream = (hipStream_t)stream_;
    const PearsonScratch s = carve(scratch);
    const long long P = (long long)width * height;
    const int per = (int)((P + PS_THREADS - 1) / PS_THREADS);
    const int fblocks = per < PS_FRAME_BLOCKS ? per : PS_FRAME_BLOCKS;
    if (whole) {
        hipLaunchKernelGGL(pearson_frame_sums_kernel, dim3(fblocks), dim3(PS_THREADS), 0, stream, P, pred, gt, mask, s.part1);
        hipLaunchKernelGGL(pearson_frame_moments_kernel, dim3(fblocks), dim3(PS_THREADS), 0, stream, P, pred, gt, mask, (const double *)s.part1,
                           s.part2);
    }
    if (n_boxes > 0) {
        if ((long long)box * box <= (long long)PS_REG_PIXELS * PS_THREADS)
            hipLaunchKernelGGL(pearson_box_kernel<true>, dim3(n_boxes), dim3(PS_THREADS), 0, stream, width, height, box, pred, gt, box_rows,
                               box_cols, s.boxes);
        else
            hipLaunchKernelGGL(pearson_box_kernel<false>, dim3(n_boxes), dim3(PS_THREADS), 0, stream, width, height, box, pred, gt, box_rows,
                               box_cols, s.boxes);
    }
    hipLaunchKernelGGL(pearson_finish_kernel, dim3(1), dim3(PS_THREADS), 0, stream, whole ? 1 : 0, fblocks, (const double *)s.part1,
                       (const double *)s.part2, s.frame, n_boxes, (const PearsonRegion *)s.boxes, sums);
    if (v_pred) {
        const int gblocks = per < PS_GRAD_BLOCKS ? per : PS_GRAD_BLOCKS;
        hipLaunchKernelGGL(pearson_grad_kernel, dim3(gblocks), dim3(PS_THREADS), 0, stream, width, height, box, pred, gt, mask,
                           whole ? (const PearsonRegion *)s.frame : (const PearsonRegion *)nullptr, n_boxes, (const PearsonRegion *)s.boxes,
                           w_whole, w_box, v_pred);
    }
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
