// subdivide.hip — the first step of the reference's cull_mesh (eval_mesh_vis_cull.py:190-193): trimesh.remesh.subdivide_to_size, the
// split of every triangle with an edge longer than max_edge into four, round after round, on the device.  The definition is stated in
// dnsplat.h (THIS PROJECT'S, PARITY UNPINNED AGAINST trimesh); torch_subdivide.py restates it on the CPU and the kernels are held to that
// file with exact equality.  Compiled with -ffp-contract=off like its siblings: a length is sqrt((dx dx + dy dy) + dz dz) in double, as
// written, and a midpoint (p + q) / 2.  One round is one dnsplat_subdivide_count and one dnsplat_subdivide_emit:
//
//   dnsplat_subdivide_count   sd_init_kernel        the edge table empty (keys ~0, values INT32_MAX), the marks 0
//                             sd_flag_kernel        one lane per triangle: the three lengths, kind = done / long (none for an index
//                                                   outside [0, V): the INDEX bit), marks on the vertices of done triangles, done and
//                                                   long per block of 256
//                             sd_insert_kernel      one lane per long triangle: its three undirected edges (lo << 32 | hi, lo <= hi) into
//                                                   the open-addressing table — a 64-bit atomicCAS claims a slot, linear probing from a
//                                                   dns_mix32 hash — and atomicMin(value, 3 t + e): an edge's value is its first slot
//                             sd_first_kernel       one lane per slot 3 t + e: the slot is its edge's first appearance iff the edge's
//                                                   value is the slot itself; first appearances per block of 256 slots
//                             mv_mark_count_kernel  (mesh_cut.h) marked vertices per block
//                             sd_scan_kernel        one workgroup, four scans: counts = {V_done, T_done, n_long, n_mid}
//   dnsplat_subdivide_emit    sd_emit_vertices_kernel  the done vertices in order, mark -> new id + 1; with a next round, cv copied
//                                                   to the head of the next vertices
//                             sd_emit_done_kernel   the done triangles remapped (+ vertex_base) and their origins, in order; the
//                                                   CAPACITY bit.  mv_emit_triangles_kernel of mesh_cut.h is not reused: it knows no
//                                                   origin rows and no base, and it ASSIGNS its status word
//                             sd_midpoints_kernel   one lane per slot: a first appearance of rank k writes midpoint V + k and leaves
//                                                   that number with its slot
//                             sd_children_kernel    one lane per triangle: a long one of rank k looks its edges up (edge -> first slot
//                                                   -> midpoint number) and writes its four children at 4 k
//
// WHAT BOUNDS EVERY LOOP: a probe walks at most `cap` = 4 T slots; the table holds at most 3 T edges, a load of 0.75.  A probe that
// runs out, or a lookup that ends on an empty slot, sets DNSPLAT_SUBDIVIDE_STATUS_INTERNAL; on a correct build neither happens.
// WHAT BOUNDS EVERY WRITE: the scratch arrays are indexed by t < T, s < 3 T, i < V, a table slot < cap and a block index below the
// grid's size; a vertex index is checked against V before any use (sd_flag_kernel: such a triangle has kind none and no later kernel
// reads its indices); an output row is written only below the capacity the caller stated.
// Equal inputs give equal bytes: an edge's value is its lowest slot whatever the order the atomics land in, every order is a scan, and
// a + b is commutative.  No floating-point atomic, no inline assembly, nothing read on the host.

#include <limits.h>

#include "block_reduce.h"
#include "mesh_cut.h"

namespace {

constexpr int SD_THREADS = MV_THREADS;
constexpr unsigned long long SD_EMPTY = ~0ull;
constexpr long long SD_INT_MAX = 0x7fffffffLL;
constexpr long long SD_MAX_T = SD_INT_MAX / 4;            // the table has 4 T slots, indexed by int32
constexpr uint8_t SD_NONE = 0, SD_DONE = 1, SD_LONG = 2;

// keys uint64 [cap]; vals int32 [cap], midid int32 [3 T], marks int32 [V], tdone int32 [nbT], tlong int32 [nbT], vcount int32 [nbV],
// mcount int32 [nbS]; kind uint8 [T], first uint8 [3 T]
struct SdScratch {
    unsigned long long *keys;
    int32_t *vals, *midid, *marks, *tdone, *tlong, *vcount, *mcount;
    uint8_t *kind, *first;
    int cap;
};

size_t sd_bytes(int V, int T)
{
    return 64 * (size_t)T + 4 * (size_t)V + 4 * (2 * (size_t)mv_blocks(T) + mv_blocks(V) + mv_blocks(3LL * T));
}

SdScratch sd_carve(void *scratch, int V, int T)
{
    SdScratch s;
    s.cap = 4 * T;
    s.keys = (unsigned long long *)scratch;
    s.vals = (int32_t *)(s.keys + s.cap);
    s.midid = s.vals + s.cap;
    s.marks = s.midid + 3 * (size_t)T;
    s.tdone = s.marks + V;
    s.tlong = s.tdone + mv_blocks(T);
    s.vcount = s.tlong + mv_blocks(T);
    s.mcount = s.vcount + mv_blocks(V);
    s.kind = (uint8_t *)(s.mcount + mv_blocks(3LL * T));
    s.first = s.kind + T;
    return s;
}

// the ends of edge e of triangle t as the table keys them: lo <= hi < V, so the key never equals SD_EMPTY.  Equal ends are an edge
// like any other here (mcl_edge of meshclusters.hip drops them).
__device__ __forceinline__ void sd_edge(int a, int b, unsigned long long &key, int &slot, int cap)
{
    const unsigned lo = (unsigned)min(a, b), hi = (unsigned)max(a, b);
    key = ((unsigned long long)lo << 32) | hi;
    const unsigned h = dns_mix32(lo ^ dns_mix32(hi + 0x9e3779b9u));
    slot = (int)(((unsigned long long)h * (unsigned)cap) >> 32);                  // in [0, cap)
}

// the table slot of the edge (a, b), -1 if the walk ends without it; the table is an earlier launch's: plain loads
__device__ __forceinline__ int sd_find(const SdScratch &s, int a, int b)
{
    unsigned long long key;
    int slot;
    sd_edge(a, b, key, slot, s.cap);
    for (int probe = 0; probe < s.cap; ++probe) {                                 // the bound: every slot once
        const unsigned long long k = s.keys[slot];
        if (k == key) return slot;
        if (k == SD_EMPTY) return -1;
        slot = slot + 1 == s.cap ? 0 : slot + 1;
    }
    return -1;
}

__global__ __launch_bounds__(SD_THREADS) void sd_init_kernel(int V, SdScratch s)
{
    const int i = blockIdx.x * SD_THREADS + threadIdx.x;
    if (i < s.cap) { s.keys[i] = SD_EMPTY; s.vals[i] = INT_MAX; }
    if (i < V) s.marks[i] = 0;
}

__global__ __launch_bounds__(SD_THREADS) void sd_flag_kernel(int V, int T, const double *__restrict__ vertices, const int32_t *__restrict__ triangles,
                                                             double max_edge, SdScratch s, int32_t *__restrict__ status)
{
    __shared__ int wave_tot[SD_THREADS / DNS_WAVE];
    const int t = blockIdx.x * SD_THREADS + threadIdx.x;
    uint8_t kind = SD_NONE;
    if (t < T) {
        const int id[3] = {triangles[(size_t)t * 3], triangles[(size_t)t * 3 + 1], triangles[(size_t)t * 3 + 2]};
        if ((unsigned)id[0] < (unsigned)V && (unsigned)id[1] < (unsigned)V && (unsigned)id[2] < (unsigned)V) {
            double p[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) p[k][c] = vertices[(size_t)id[k] * 3 + c];
            bool is_long = false;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int n = e == 2 ? 0 : e + 1;
                const double dx = p[n][0] - p[e][0], dy = p[n][1] - p[e][1], dz = p[n][2] - p[e][2];
                const double L = sqrt((dx * dx + dy * dy) + dz * dz);
                is_long = is_long || L > max_edge;                                // strict; false for a nan
            }
            kind = is_long ? SD_LONG : SD_DONE;
            if (!is_long) { s.marks[id[0]] = 1; s.marks[id[1]] = 1; s.marks[id[2]] = 1; }
        } else {
            atomicOr(status, DNSPLAT_SUBDIVIDE_STATUS_INDEX);
        }
        s.kind[t] = kind;
    }
    int total;
    dns_block_rank<SD_THREADS>(kind == SD_DONE, wave_tot, total);
    if (threadIdx.x == 0) s.tdone[blockIdx.x] = total;
    dns_block_rank<SD_THREADS>(kind == SD_LONG, wave_tot, total);
    if (threadIdx.x == 0) s.tlong[blockIdx.x] = total;
}

__global__ __launch_bounds__(SD_THREADS) void sd_insert_kernel(int T, const int32_t *__restrict__ triangles, SdScratch s, int32_t *__restrict__ status)
{
    const int t = blockIdx.x * SD_THREADS + threadIdx.x;
    if (t >= T || s.kind[t] != SD_LONG) return;
    const int id[3] = {triangles[(size_t)t * 3], triangles[(size_t)t * 3 + 1], triangles[(size_t)t * 3 + 2]};
    for (int e = 0; e < 3; ++e) {
        unsigned long long key;
        int slot;
        sd_edge(id[e], id[e == 2 ? 0 : e + 1], key, slot, s.cap);
        bool placed = false;
        for (int probe = 0; probe < s.cap; ++probe) {                             // the bound: every slot once
            const unsigned long long old = atomicCAS(&s.keys[slot], SD_EMPTY, key);
            if (old == SD_EMPTY || old == key) {
                atomicMin(&s.vals[slot], 3 * t + e);
                placed = true;
                break;
            }
            slot = slot + 1 == s.cap ? 0 : slot + 1;
        }
        if (!placed) atomicOr(status, DNSPLAT_SUBDIVIDE_STATUS_INTERNAL);
    }
}

// one lane per slot j = 3 t + e (j < 3 T <= INT_MAX)
__global__ __launch_bounds__(SD_THREADS) void sd_first_kernel(int T, const int32_t *__restrict__ triangles, SdScratch s, int32_t *__restrict__ status)
{
    __shared__ int wave_tot[SD_THREADS / DNS_WAVE];
    const long long j = (long long)blockIdx.x * SD_THREADS + threadIdx.x;
    bool first = false;
    if (j < 3LL * T) {
        const int t = (int)(j / 3), e = (int)(j - 3LL * t);
        if (s.kind[t] == SD_LONG) {
            const int at = sd_find(s, triangles[(size_t)t * 3 + e], triangles[(size_t)t * 3 + (e == 2 ? 0 : e + 1)]);
            if (at < 0) atomicOr(status, DNSPLAT_SUBDIVIDE_STATUS_INTERNAL);
            else first = s.vals[at] == (int)j;
        }
        s.first[j] = first ? 1 : 0;
    }
    int total;
    dns_block_rank<SD_THREADS>(first, wave_tot, total);
    if (threadIdx.x == 0) s.mcount[blockIdx.x] = total;
}

// One workgroup: the four arrays of block counts to their exclusive prefix sums in place
__global__ __launch_bounds__(SD_THREADS) void sd_scan_kernel(int nbv, int nbt, int nbs, SdScratch s, int64_t *__restrict__ counts)
{
    const int nv = dns_scan_in_place<SD_THREADS, MV_SCAN_PER>(nbv, s.vcount);
    __syncthreads();
    const int nd = dns_scan_in_place<SD_THREADS, MV_SCAN_PER>(nbt, s.tdone);
    __syncthreads();
    const int nl = dns_scan_in_place<SD_THREADS, MV_SCAN_PER>(nbt, s.tlong);
    __syncthreads();
    const int nm = dns_scan_in_place<SD_THREADS, MV_SCAN_PER>(nbs, s.mcount);
    if (threadIdx.x == 0) { counts[0] = nv; counts[1] = nd; counts[2] = nl; counts[3] = nm; }
}

// next: NULL without a next round, else [V + cap_mid,3]: its first V rows are cv
__global__ __launch_bounds__(SD_THREADS) void sd_emit_vertices_kernel(int V, const double *__restrict__ vertices, SdScratch s, long long cap_v,
                                                                      double *__restrict__ out, double *__restrict__ next)
{
    __shared__ int wave_tot[SD_THREADS / DNS_WAVE];
    const int i = blockIdx.x * SD_THREADS + threadIdx.x;
    const bool marked = i < V && s.marks[i] != 0;
    int total;
    const int id = s.vcount[blockIdx.x] + dns_block_rank<SD_THREADS>(marked, wave_tot, total);
    if (i >= V) return;
    const double x = vertices[(size_t)i * 3], y = vertices[(size_t)i * 3 + 1], z = vertices[(size_t)i * 3 + 2];
    if (next) { next[(size_t)i * 3] = x; next[(size_t)i * 3 + 1] = y; next[(size_t)i * 3 + 2] = z; }
    if (!marked) return;
    s.marks[i] = id + 1;                                                          // still a mark: a second emit finds the same flags
    if (id < cap_v) { out[(size_t)id * 3] = x; out[(size_t)id * 3 + 1] = y; out[(size_t)id * 3 + 2] = z; }
}

// the marks after sd_emit_vertices_kernel: new id + 1
__global__ __launch_bounds__(SD_THREADS) void sd_emit_done_kernel(int T, const int32_t *__restrict__ triangles, const int32_t *__restrict__ origin,
                                                                  SdScratch s, const int64_t *__restrict__ counts, long long base, long long cap_v,
                                                                  long long cap_t, long long cap_long, long long cap_mid,
                                                                  int32_t *__restrict__ out, int32_t *__restrict__ out_index, int32_t *__restrict__ status)
{
    __shared__ int wave_tot[SD_THREADS / DNS_WAVE];
    const int t = blockIdx.x * SD_THREADS + threadIdx.x;
    const bool kept = t < T && s.kind[t] == SD_DONE;
    int total;
    const int row = s.tdone[blockIdx.x] + dns_block_rank<SD_THREADS>(kept, wave_tot, total);
    if (blockIdx.x == 0 && threadIdx.x == 0 && (counts[0] > cap_v || counts[1] > cap_t || counts[2] > cap_long || counts[3] > cap_mid))
        atomicOr(status, DNSPLAT_SUBDIVIDE_STATUS_CAPACITY);
    if (kept && row < cap_t) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[(size_t)row * 3 + k] = (int32_t)(base + s.marks[triangles[(size_t)t * 3 + k]] - 1);
        out_index[row] = origin[t];
    }
}

__global__ __launch_bounds__(SD_THREADS) void sd_midpoints_kernel(int V, int T, const double *__restrict__ vertices, const int32_t *__restrict__ triangles,
                                                                  SdScratch s, long long cap_mid, double *__restrict__ next)
{
    __shared__ int wave_tot[SD_THREADS / DNS_WAVE];
    const long long j = (long long)blockIdx.x * SD_THREADS + threadIdx.x;
    const bool first = j < 3LL * T && s.first[j] != 0;
    int total;
    const int k = s.mcount[blockIdx.x] + dns_block_rank<SD_THREADS>(first, wave_tot, total);
    if (!first || k >= cap_mid) return;
    const int t = (int)(j / 3), e = (int)(j - 3LL * t);
    const int a = triangles[(size_t)t * 3 + e], b = triangles[(size_t)t * 3 + (e == 2 ? 0 : e + 1)];   // in [0, V): t is long
    s.midid[j] = V + k;
#pragma unroll
    for (int c = 0; c < 3; ++c) next[((size_t)V + k) * 3 + c] = (vertices[(size_t)a * 3 + c] + vertices[(size_t)b * 3 + c]) / 2.0;
}

__global__ __launch_bounds__(SD_THREADS) void sd_children_kernel(int V, int T, const int32_t *__restrict__ triangles, const int32_t *__restrict__ origin,
                                                                 SdScratch s, long long cap_long, long long cap_mid,
                                                                 int32_t *__restrict__ next_triangles, int32_t *__restrict__ next_origin,
                                                                 int32_t *__restrict__ status)
{
    __shared__ int wave_tot[SD_THREADS / DNS_WAVE];
    const int t = blockIdx.x * SD_THREADS + threadIdx.x;
    const bool is_long = t < T && s.kind[t] == SD_LONG;
    int total;
    const int row = s.tlong[blockIdx.x] + dns_block_rank<SD_THREADS>(is_long, wave_tot, total);
    if (!is_long || row >= cap_long) return;
    const int id[3] = {triangles[(size_t)t * 3], triangles[(size_t)t * 3 + 1], triangles[(size_t)t * 3 + 2]};
    int m[3];
    for (int e = 0; e < 3; ++e) {
        const int at = sd_find(s, id[e], id[e == 2 ? 0 : e + 1]);
        const int j = at < 0 ? -1 : s.vals[at];                                   // the edge's first slot
        m[e] = (unsigned)j < 3u * (unsigned)T ? s.midid[j] : -1;
        // a midpoint past cap_mid was not numbered (the CAPACITY bit is set then); anything else outside [V, V + cap_mid) is a bug
        if (m[e] < V || m[e] - V >= cap_mid) { m[e] = 0; atomicOr(status, j < 0 ? DNSPLAT_SUBDIVIDE_STATUS_INTERNAL : DNSPLAT_SUBDIVIDE_STATUS_CAPACITY); }
    }
    const int child[12] = {id[0], m[0], m[2], m[0], id[1], m[1], m[2], m[1], id[2], m[0], m[1], m[2]};
    int32_t *out = next_triangles + (size_t)row * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) out[k] = child[k];
    const int o = origin[t];
#pragma unroll
    for (int k = 0; k < 4; ++k) next_origin[(size_t)row * 4 + k] = o;
}

bool sd_args_ok(const dnsplat_subdivide_args *a)
{
    return a && a->V >= 1 && a->T >= 1 && a->vertices && a->triangles && a->origin && a->scratch && a->counts && a->status &&
           a->max_edge > 0.0 && a->max_edge < HUGE_VAL;                           // false for a nan
}

}  // namespace

extern "C" size_t dnsplat_subdivide_scratch_bytes(int32_t V, int32_t T)
{
    if (V < 1 || T < 1 || T > SD_MAX_T) return 0;
    return sd_bytes(V, T);
}

extern "C" int dnsplat_subdivide_count(const dnsplat_subdivide_args *a, dnsplat_stream_t stream_)
{
    if (!sd_args_ok(a)) return DNSPLAT_ERR_INVALID_ARG;
    if (a->T > SD_MAX_T) return DNSPLAT_ERR_UNSUPPORTED;
    if (a->scratch_bytes < sd_bytes(a->V, a->T) || (size_t)a->scratch % sizeof(unsigned long long)) return DNSPLAT_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const SdScratch s = sd_carve(a->scratch, a->V, a->T);
    const int V = a->V, T = a->T, nbt = mv_blocks(T), nbv = mv_blocks(V), nbs = mv_blocks(3LL * T);
    const dim3 block(SD_THREADS);
    hipLaunchKernelGGL(sd_init_kernel, dim3((unsigned)mv_blocks(max((long long)s.cap, (long long)V))), block, 0, stream, V, s);
    hipLaunchKernelGGL(sd_flag_kernel, dim3((unsigned)nbt), block, 0, stream, V, T, a->vertices, a->triangles, a->max_edge, s, a->status);
    hipLaunchKernelGGL(sd_insert_kernel, dim3((unsigned)nbt), block, 0, stream, T, a->triangles, s, a->status);
    hipLaunchKernelGGL(sd_first_kernel, dim3((unsigned)nbs), block, 0, stream, T, a->triangles, s, a->status);
    hipLaunchKernelGGL(mv_mark_count_kernel, dim3((unsigned)nbv), block, 0, stream, V, s.marks, s.vcount);
    hipLaunchKernelGGL(sd_scan_kernel, dim3(1), block, 0, stream, nbv, nbt, nbs, s, a->counts);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_subdivide_emit(const dnsplat_subdivide_args *a, dnsplat_stream_t stream_)
{
    if (!sd_args_ok(a) || a->vertex_base < 0 || a->cap_v < 0 || a->cap_t < 0 || a->cap_long < 0 || a->cap_mid < 0) return DNSPLAT_ERR_INVALID_ARG;
    if ((a->cap_v > 0 && !a->out_vertices) || (a->cap_t > 0 && (!a->out_triangles || !a->out_index))) return DNSPLAT_ERR_INVALID_ARG;
    if (a->cap_long > 0 && (!a->next_vertices || !a->next_triangles || !a->next_origin)) return DNSPLAT_ERR_INVALID_ARG;
    if (a->T > SD_MAX_T || a->cap_long > SD_MAX_T / 4 || a->cap_mid > SD_INT_MAX - a->V || a->cap_v > SD_INT_MAX - a->vertex_base ||
        a->vertex_base > SD_INT_MAX)
        return DNSPLAT_ERR_UNSUPPORTED;
    if (a->scratch_bytes < sd_bytes(a->V, a->T) || (size_t)a->scratch % sizeof(unsigned long long)) return DNSPLAT_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const SdScratch s = sd_carve(a->scratch, a->V, a->T);
    const int V = a->V, T = a->T, nbt = mv_blocks(T);
    const dim3 block(SD_THREADS);
    const bool more = a->cap_long > 0;
    hipLaunchKernelGGL(sd_emit_vertices_kernel, dim3((unsigned)mv_blocks(V)), block, 0, stream, V, a->vertices, s, (long long)a->cap_v,
                       a->out_vertices, more ? a->next_vertices : (double *)nullptr);
    hipLaunchKernelGGL(sd_emit_done_kernel, dim3((unsigned)nbt), block, 0, stream, T, a->triangles, a->origin, s, a->counts,
                       (long long)a->vertex_base, (long long)a->cap_v, (long long)a->cap_t, (long long)a->cap_long, (long long)a->cap_mid,
                       a->out_triangles, a->out_index, a->status);
    if (more) {
        hipLaunchKernelGGL(sd_midpoints_kernel, dim3((unsigned)mv_blocks(3LL * T)), block, 0, stream, V, T, a->vertices, a->triangles, s,
                           (long long)a->cap_mid, a->next_vertices);
        hipLaunchKernelGGL(sd_children_kernel, dim3((unsigned)nbt), block, 0, stream, V, T, a->triangles, a->origin, s, (long long)a->cap_long,
                           (long long)a->cap_mid, a->next_triangles, a->next_origin, a->status);
    }
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
