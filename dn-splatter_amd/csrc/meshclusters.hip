// meshclusters.hip — the connected-component filter the reference's recommended exporter ends with (export_mesh.py:1021-1039, Open3D's
// cluster_connected_triangles, the size threshold, remove_unreferenced_vertices and remove_degenerate_triangles) on the device.  Topology
// only: triangle indices in, integers out.  The definition is stated in dnsplat.h (THIS PROJECT'S, PARITY UNPINNED AGAINST Open3D);
// torch_mesh_clusters.py restates it sequentially on the CPU and the kernels are held to that file with exact equality.  Compiled with
// -ffp-contract=off like its siblings; there is no floating-point operation in this file.
//
//   dnsplat_mesh_clusters      mcl_init_kernel     the edge table empty (keys ~0, values INT32_MAX), parent[t] = t, the sizes 0, status 0
//                              mcl_insert_kernel   one lane per triangle: its undirected edges (lo << 32 | hi, lo < hi) into an
//                                                  open-addressing table — a 64-bit atomicCAS claims a slot, linear probing from a
//                                                  dns_mix32 hash — and atomicMin(value, t): an edge's value is its lowest triangle
//                              mcl_union_kernel    one lane per triangle: looks its edges up and unites t with each edge's value.  The
//                                                  union-find's only write is atomicMin(&parent[hi], lo) with lo < hi
//                              mcl_flatten_kernel  root[t] = the end of t's path (the component's lowest triangle), sizes per root and the
//                                                  number of valid triangles by integer atomicAdd (one add per distinct root of a
//                                                  wave and one per workgroup: the largest cluster's word takes T / 64 adds, not T)
//                              mcl_roots_kernel    the roots per block of 256 triangles (the flag rank of block_scan.h)
//                              mcl_number_kernel   one workgroup: the exclusive scan of those counts; counts = {n_clusters, n_valid}
//                              mcl_assign_kernel   root -> cluster number, sizes[number]
//                              mcl_label_kernel    labels[t] = the number of t's root, -1 for an invalid triangle
//   dnsplat_mesh_filter_count  three rounds (11 + 11 + 10 bits) of mcf_hist_kernel / mcf_select_kernel: the keep_largest-th largest of
//                              sizes[0 .. n_clusters) by radix selection (dns_hist_add, dns_hist_flush, dns_find_bin), n_clusters read
//                              on the device; the last select writes the threshold.  Then mcf_keep_kernel (the rule per triangle, the
//                              marks, kept per block) and mesh_cut.h's mv_mark_count_kernel and mv_cut_scan_kernel: counts = {V', T'}
//   dnsplat_mesh_filter_emit   mcf_emit_vertices_kernel (the old id of each kept vertex, mark -> new id) and mv_emit_triangles_kernel
//
// WHY THE UNION-FIND IS RIGHT WHATEVER A LOAD RETURNS.  Every value ever stored in parent[] is a triangle index, and parent[i] <= i
// always: it starts as i and only atomicMin with a lower index writes it.  So every path strictly descends, there is no cycle, a path
// has at most T - 1 links, and a root is the lowest index of its tree.  A link parent[x] = y is only ever made between triangles that
// belong to one component of the mesh, so whatever a (possibly stale) read of parent[] returns is a triangle of the same component:
// "a == b, nothing to do" is never wrong.  Whether a hook took effect is decided by the atomic's RETURN value alone: old == hi means hi
// was a root and now hangs under lo; otherwise hi already hung under old, parent[hi] is now min(old, lo), and the thread goes on uniting
// old with lo — both below hi, so a union takes at most T rounds.  parent[] is read with relaxed agent-scope atomic loads inside
// mcl_union_kernel (the per-XCD L2s do not make plain loads coherent within a launch); that is for progress, not for correctness.
// The flatten runs in a launch of its own: the kernel boundary is the fence, and there the forest is final.
//
// WHAT BOUNDS EVERY LOOP: a probe walks at most `cap` slots (the table's capacity: the load never exceeds 0.75), a find at most T links,
// a union at most T rounds.  A loop that runs out sets DNSPLAT_MESH_CLUSTERS_STATUS_INTERNAL in the device status word and leaves; on a
// correct build that cannot happen.  No floating-point atomic, no inline assembly, nothing read on the host.
//
// Equal inputs give equal bytes: the roots are the lowest indices whatever the order the atomics land in, the sizes are integer sums,
// the numbering and both cuts are scans.

#include <limits.h>

#include "block_reduce.h"
#include "mesh_cut.h"

namespace {

constexpr int MCL_THREADS = MV_THREADS;
static_assert(DNSPLAT_MESH_FILTER_STATUS_VERTICES == DNSPLAT_MESH_CUT_STATUS_VERTICES && DNSPLAT_MESH_FILTER_STATUS_TRIANGLES == DNSPLAT_MESH_CUT_STATUS_TRIANGLES,
              "mv_emit_triangles_kernel writes the cut's bits");
constexpr unsigned long long MCL_EMPTY = ~0ull;
constexpr int MCL_ROUNDS = 3;
constexpr int MCL_BINS = 2048;                            // of the widest round
constexpr long long MCL_MAX_T = 0x7fffffffLL / 4;         // the table has 4 T slots, indexed by int32

__host__ __device__ constexpr int mcl_bits(int round) { return round < 2 ? 11 : 10; }
__host__ __device__ constexpr int mcl_shift(int round) { return round == 0 ? 21 : (round == 1 ? 10 : 0); }   // the bits below the round's

#define MCL_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// ---- scratch ----------------------------------------------------------------------------------------------------------------------
// clusters: keys uint64 [cap], n_valid uint64 [1], values int32 [cap], parent int32 [T], root int32 [T], rsize int32 [T],
//           roots-per-block int32 [nb]; cap = 4 T: 3 T distinct edges at the most, a load of 0.75
struct MclScratch {
    unsigned long long *keys, *n_valid;
    int32_t *vals, *parent, *root, *rsize, *bcount;
    int cap;
};

size_t mcl_bytes(int T)
{
    const size_t cap = 4 * (size_t)T;
    return (cap + 1) * sizeof(unsigned long long) + (cap + 3 * (size_t)T + mv_blocks(T)) * sizeof(int32_t);
}

MclScratch mcl_carve(void *scratch, int T)
{
    MclScratch s;
    s.cap = 4 * T;
    s.keys = (unsigned long long *)scratch;
    s.n_valid = s.keys + s.cap;
    s.vals = (int32_t *)(s.n_valid + 1);
    s.parent = s.vals + s.cap;
    s.root = s.parent + T;
    s.rsize = s.root + T;
    s.bcount = s.rsize + T;
    return s;
}

// filter: histograms uint64 [MCL_ROUNDS][MCL_BINS], {rank, prefix} uint64 [2], marks int32 [V], kept-per-block int32 [nbT],
//         marked-per-block int32 [nbV], keep uint8 [T]
struct McfScratch {
    unsigned long long *hist, *state;
    int32_t *marks, *tcount, *vcount;
    uint8_t *keep;
};

size_t mcf_bytes(int V, int T)
{
    return ((size_t)MCL_ROUNDS * MCL_BINS + 2) * sizeof(unsigned long long) + ((size_t)V + mv_blocks(T) + mv_blocks(V)) * sizeof(int32_t) + (size_t)T;
}

__host__ __device__ McfScratch mcf_carve(void *scratch, int V, int T)
{
    McfScratch s;
    s.hist = (unsigned long long *)scratch;
    s.state = s.hist + (size_t)MCL_ROUNDS * MCL_BINS;
    s.marks = (int32_t *)(s.state + 2);
    s.tcount = s.marks + V;
    s.vcount = s.tcount + ((long long)T + MV_THREADS - 1) / MV_THREADS;
    s.keep = (uint8_t *)(s.vcount + ((long long)V + MV_THREADS - 1) / MV_THREADS);
    return s;
}

// ---- the edge table ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool mcl_valid(const int id[3], int V)
{
    return (unsigned)id[0] < (unsigned)V && (unsigned)id[1] < (unsigned)V && (unsigned)id[2] < (unsigned)V;
}

// edge e of a valid triangle: false for equal ends; lo < hi < V, so the key never equals MCL_EMPTY
__device__ __forceinline__ bool mcl_edge(const int id[3], int e, unsigned long long &key, int &slot, int cap)
{
    const int a = id[e], b = id[e == 2 ? 0 : e + 1];
    if (a == b) return false;
    const unsigned lo = (unsigned)min(a, b), hi = (unsigned)max(a, b);
    key = ((unsigned long long)lo << 32) | hi;
    const unsigned h = dns_mix32(lo ^ dns_mix32(hi + 0x9e3779b9u));
    slot = (int)(((unsigned long long)h * (unsigned)cap) >> 32);                  // in [0, cap)
    return true;
}

__global__ __launch_bounds__(MCL_THREADS) void mcl_init_kernel(int T, MclScratch s, int32_t *__restrict__ sizes, int32_t *__restrict__ status)
{
    const int i = blockIdx.x * MCL_THREADS + threadIdx.x;
    if (i < s.cap) { s.keys[i] = MCL_EMPTY; s.vals[i] = INT_MAX; }
    if (i < T) { s.parent[i] = i; s.rsize[i] = 0; sizes[i] = 0; }
    if (i == 0) { s.n_valid[0] = 0ull; status[0] = 0; }
}

__global__ __launch_bounds__(MCL_THREADS) void mcl_insert_kernel(int V, int T, const int32_t *__restrict__ triangles, MclScratch s,
                                                                 int32_t *__restrict__ status)
{
    const int t = blockIdx.x * MCL_THREADS + threadIdx.x;
    if (t >= T) return;
    const int id[3] = {triangles[(size_t)t * 3], triangles[(size_t)t * 3 + 1], triangles[(size_t)t * 3 + 2]};
    if (!mcl_valid(id, V)) return;
    for (int e = 0; e < 3; ++e) {
        unsigned long long key;
        int slot;
        if (!mcl_edge(id, e, key, slot, s.cap)) continue;
        bool placed = false;
        for (int probe = 0; probe < s.cap; ++probe) {                             // the bound: every slot once
            const unsigned long long old = atomicCAS(&s.keys[slot], MCL_EMPTY, key);
            if (old == MCL_EMPTY || old == key) {
                atomicMin(&s.vals[slot], t);
                placed = true;
                break;
            }
            slot = slot + 1 == s.cap ? 0 : slot + 1;
        }
        if (!placed) atomicOr(status, DNSPLAT_MESH_CLUSTERS_STATUS_INTERNAL);
    }
}

// ---- the union-find ---------------------------------------------------------------------------------------------------------------

// The end of x's path as far as this thread can see it, halving the path on the way (the same write: atomicMin with a lower index of
// the same component).  A path strictly descends, so T steps suffice; *bad is set if they did not.
__device__ __forceinline__ int mcl_find(int32_t *parent, int x, int T, bool &bad)
{
    for (int step = 0; step < T; ++step) {
        const int p = MCL_LOAD(&parent[x]);
        if (p == x) return x;
        const int g = MCL_LOAD(&parent[p]);
        if (g != p) atomicMin(&parent[x], g);
        x = g;
    }
    bad = bad || MCL_LOAD(&parent[x]) != x;
    return x;
}

__device__ __forceinline__ void mcl_unite(int32_t *parent, int a, int b, int T, bool &bad)
{
    for (int round = 0; round < T; ++round) {                                     // max(a, b) falls every round
        a = mcl_find(parent, a, T, bad);
        b = mcl_find(parent, b, T, bad);
        if (a == b) return;
        const int lo = min(a, b), hi = max(a, b);
        const int old = atomicMin(&parent[hi], lo);
        if (old == hi) return;                                                    // hi was a root and now hangs under lo
        a = old;                                                                  // hi hung under old already: old and lo remain
        b = lo;
    }
    bad = true;
}

__global__ __launch_bounds__(MCL_THREADS) void mcl_union_kernel(int V, int T, const int32_t *__restrict__ triangles, MclScratch s,
                                                                int32_t *__restrict__ status)
{
    const int t = blockIdx.x * MCL_THREADS + threadIdx.x;
    if (t >= T) return;
    const int id[3] = {triangles[(size_t)t * 3], triangles[(size_t)t * 3 + 1], triangles[(size_t)t * 3 + 2]};
    if (!mcl_valid(id, V)) return;
    bool bad = false;
    for (int e = 0; e < 3; ++e) {
        unsigned long long key;
        int slot;
        if (!mcl_edge(id, e, key, slot, s.cap)) continue;
        int first = -1;                                                           // the table is the previous launch's: plain loads
        for (int probe = 0; probe < s.cap; ++probe) {
            const unsigned long long k = s.keys[slot];
            if (k == key) { first = s.vals[slot]; break; }
            if (k == MCL_EMPTY) break;
            slot = slot + 1 == s.cap ? 0 : slot + 1;
        }
        if ((unsigned)first >= (unsigned)T || first > t) { bad = true; continue; }    // every edge of t was inserted with a value <= t
        if (first != t) mcl_unite(s.parent, t, first, T, bad);
    }
    if (bad) atomicOr(status, DNSPLAT_MESH_CLUSTERS_STATUS_INTERNAL);
}

// The forest is final here: the launch before this one has ended.  Plain loads; root[] is written beside parent[], never into it.
__global__ __launch_bounds__(MCL_THREADS) void mcl_flatten_kernel(int V, int T, const int32_t *__restrict__ triangles, MclScratch s,
                                                                  int32_t *__restrict__ status)
{
    __shared__ int wave_tot[MCL_THREADS / DNS_WAVE];
    const int t = blockIdx.x * MCL_THREADS + threadIdx.x;
    int r = -1;
    if (t < T) {
        const int id[3] = {triangles[(size_t)t * 3], triangles[(size_t)t * 3 + 1], triangles[(size_t)t * 3 + 2]};
        if (mcl_valid(id, V)) {
            r = t;
            bool found = false;
            for (int step = 0; step < T; ++step) {
                const int p = s.parent[r];
                if (p == r) { found = true; break; }
                r = p;
            }
            if (!found) atomicOr(status, DNSPLAT_MESH_CLUSTERS_STATUS_INTERNAL);
        }
        s.root[t] = r;
    }
    // The sizes: one add per distinct root of the wave.  A mesh is mostly ONE cluster, and adds to one word serialise: a lane each
    // cost 80 ms at 9 M triangles.  Wave-uniform: every trip retires its leader's root, so there are at most 64 of them.
    uint64_t todo = dns_ballot(r >= 0);
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const int r0 = __builtin_amdgcn_readlane(r, leader);
        const uint64_t same = dns_ballot(r == r0) & todo;
        if ((int)(threadIdx.x & (DNS_WAVE - 1)) == leader) atomicAdd(&s.rsize[r0], __builtin_popcountll(same));
        todo &= ~same;
    }
    int total;
    dns_block_rank<MCL_THREADS>(r >= 0, wave_tot, total);
    if (threadIdx.x == 0 && total) atomicAdd(s.n_valid, (unsigned long long)total);
}

// ---- the numbering ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(MCL_THREADS) void mcl_roots_kernel(int T, MclScratch s)
{
    __shared__ int wave_tot[MCL_THREADS / DNS_WAVE];
    const int t = blockIdx.x * MCL_THREADS + threadIdx.x;
    int total;
    dns_block_rank<MCL_THREADS>(t < T && s.root[t] == t, wave_tot, total);
    if (threadIdx.x == 0) s.bcount[blockIdx.x] = total;
}

__global__ __launch_bounds__(MCL_THREADS) void mcl_number_kernel(int nb, MclScratch s, int64_t *__restrict__ counts)
{
    const int n = dns_scan_in_place<MCL_THREADS, MV_SCAN_PER>(nb, s.bcount);
    if (threadIdx.x == 0) { counts[0] = n; counts[1] = (int64_t)s.n_valid[0]; }
}

// parent[] is free after the flatten: parent[root] becomes the root's cluster number
__global__ __launch_bounds__(MCL_THREADS) void mcl_assign_kernel(int T, MclScratch s, int32_t *__restrict__ sizes)
{
    __shared__ int wave_tot[MCL_THREADS / DNS_WAVE];
    const int t = blockIdx.x * MCL_THREADS + threadIdx.x;
    const bool is_root = t < T && s.root[t] == t;
    int total;
    const int c = s.bcount[blockIdx.x] + dns_block_rank<MCL_THREADS>(is_root, wave_tot, total);
    if (t >= T) return;
    if (is_root) { s.parent[t] = c; sizes[c] = s.rsize[t]; }                      // c < n_clusters; the rows past them stay the init's 0
}

__global__ __launch_bounds__(MCL_THREADS) void mcl_label_kernel(int T, MclScratch s, int32_t *__restrict__ labels)
{
    const int t = blockIdx.x * MCL_THREADS + threadIdx.x;
    if (t >= T) return;
    const int r = s.root[t];
    labels[t] = r < 0 ? -1 : s.parent[r];
}

// ---- the threshold ----------------------------------------------------------------------------------------------------------------

// round `round`: the sizes whose upper bits equal the prefix, counted by their next bits
__global__ __launch_bounds__(MCL_THREADS) void mcf_hist_kernel(int round, int V, int T, const int32_t *__restrict__ sizes,
                                                               const int64_t *__restrict__ cluster_counts, void *scratch)
{
    __shared__ unsigned int hist[MCL_BINS];
    const McfScratch s = mcf_carve(scratch, V, T);
    for (int b = threadIdx.x; b < MCL_BINS; b += MCL_THREADS) hist[b] = 0u;
    __syncthreads();
    const long long n = min((long long)cluster_counts[0], (long long)T);          // sizes has T rows whatever the caller's counts say
    const int bits = mcl_bits(round), shift = mcl_shift(round);
    const unsigned prefix = round == 0 ? 0u : (unsigned)s.state[1];
    const int i = blockIdx.x * MCL_THREADS + threadIdx.x;
    const bool in = i < n;                                                       // every lane stays for the wave-wide adds
    const unsigned v = in ? (unsigned)sizes[i] : 0u;
    const unsigned above = round == 0 ? 0u : v >> (shift + bits);
    dns_hist_add(hist, (v >> shift) & ((1u << bits) - 1u), in && above == prefix);
    __syncthreads();
    dns_hist_flush<MCL_THREADS>(hist, s.hist + (size_t)round * MCL_BINS, MCL_BINS);
}

// One workgroup.  Round 0 starts from the ascending rank n_clusters - keep_largest; the last round writes the threshold:
// max(min_triangles, the keep_largest-th largest size) with keep_largest clusters or more, min_triangles with fewer.
__global__ __launch_bounds__(MCL_THREADS) void mcf_select_kernel(int round, int V, int T, const int64_t *__restrict__ cluster_counts, int keep_largest,
                                                                 int min_triangles, void *scratch, int32_t *__restrict__ threshold)
{
    __shared__ unsigned long long wave_sum[MCL_THREADS / DNS_WAVE];
    __shared__ unsigned int picked;
    const McfScratch s = mcf_carve(scratch, V, T);
    const long long n = min((long long)cluster_counts[0], (long long)T);
    const bool enough = n >= keep_largest;
    const unsigned long long rank = round == 0 ? (unsigned long long)(enough ? n - keep_largest : 0) : s.state[0];
    const unsigned long long prefix = round == 0 ? 0ull : s.state[1];
    if (threadIdx.x == 0) picked = 0u;
    __syncthreads();                                                              // every thread has read the state before one rewrites it
    unsigned int bin;
    unsigned long long rest;
    if (dns_find_bin<MCL_THREADS, MCL_BINS>(s.hist + (size_t)round * MCL_BINS, rank, wave_sum, bin, rest)) {
        s.state[0] = rest;
        s.state[1] = (prefix << mcl_bits(round)) | bin;
        picked = (unsigned int)((prefix << mcl_bits(round)) | bin);
    }                                                                             // no cluster at all: the state stays the memset's 0
    if (round != MCL_ROUNDS - 1) return;
    __syncthreads();
    if (threadIdx.x == 0) threshold[0] = enough ? max(min_triangles, (int)picked) : min_triangles;
}

// ---- the cut ----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(MCL_THREADS) void mcf_keep_kernel(int V, int T, const int32_t *__restrict__ triangles, const int32_t *__restrict__ labels,
                                                               const int32_t *__restrict__ sizes, const int32_t *__restrict__ threshold,
                                                               int32_t *__restrict__ marks, int32_t *__restrict__ tcount, uint8_t *__restrict__ keep)
{
    __shared__ int wave_tot[MCL_THREADS / DNS_WAVE];
    const int t = blockIdx.x * MCL_THREADS + threadIdx.x;
    bool kept = false;
    if (t < T) {
        const int id[3] = {triangles[(size_t)t * 3], triangles[(size_t)t * 3 + 1], triangles[(size_t)t * 3 + 2]};
        const int l = labels[t];
        if (mcl_valid(id, V) && id[0] != id[1] && id[1] != id[2] && id[0] != id[2] && (unsigned)l < (unsigned)T) {
            kept = sizes[l] >= threshold[0];
            if (kept) { marks[id[0]] = 1; marks[id[1]] = 1; marks[id[2]] = 1; }
        }
        keep[t] = kept ? 1 : 0;
    }
    int total;
    dns_block_rank<MCL_THREADS>(kept, wave_tot, total);
    if (threadIdx.x == 0) tcount[blockIdx.x] = total;
}

__global__ __launch_bounds__(MCL_THREADS) void mcf_emit_vertices_kernel(int V, const int32_t *__restrict__ vcount, int32_t *__restrict__ marks,
                                                                        long long cap_v, int32_t *__restrict__ vertex_index)
{
    __shared__ int wave_tot[MCL_THREADS / DNS_WAVE];
    const int i = blockIdx.x * MCL_THREADS + threadIdx.x;
    const bool marked = i < V && marks[i] != 0;
    int total;
    const int id = vcount[blockIdx.x] + dns_block_rank<MCL_THREADS>(marked, wave_tot, total);
    if (!marked) return;
    marks[i] = id + 1;                                                            // still a mark: a second emit finds the same flags
    if (id < cap_v) vertex_index[id] = i;
}

bool mcf_args_ok(const dnsplat_mesh_filter_args *a)
{
    return a && a->V >= 1 && a->T >= 1 && a->keep_largest >= 1 && a->min_triangles >= 1 && a->triangles && a->labels && a->sizes &&
           a->cluster_counts && a->scratch && a->threshold && a->counts;
}

}  // namespace

extern "C" size_t dnsplat_mesh_clusters_scratch_bytes(int32_t V, int32_t T)
{
    if (V < 1 || T < 1 || T > MCL_MAX_T) return 0;
    return mcl_bytes(T);
}

extern "C" int dnsplat_mesh_clusters(const dnsplat_mesh_clusters_args *a, dnsplat_stream_t stream_)
{
    if (!a || a->V < 1 || a->T < 1 || !a->triangles || !a->scratch || !a->labels || !a->sizes || !a->counts || !a->status)
        return DNSPLAT_ERR_INVALID_ARG;
    if (a->T > MCL_MAX_T) return DNSPLAT_ERR_UNSUPPORTED;
    if (a->scratch_bytes < mcl_bytes(a->T) || (size_t)a->scratch % sizeof(unsigned long long)) return DNSPLAT_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const MclScratch s = mcl_carve(a->scratch, a->T);
    const int V = a->V, T = a->T, nb = mv_blocks(T);
    const dim3 grid((unsigned)nb), block(MCL_THREADS);
    hipLaunchKernelGGL(mcl_init_kernel, dim3((unsigned)mv_blocks(s.cap)), block, 0, stream, T, s, a->sizes, a->status);
    hipLaunchKernelGGL(mcl_insert_kernel, grid, block, 0, stream, V, T, a->triangles, s, a->status);
    hipLaunchKernelGGL(mcl_union_kernel, grid, block, 0, stream, V, T, a->triangles, s, a->status);
    hipLaunchKernelGGL(mcl_flatten_kernel, grid, block, 0, stream, V, T, a->triangles, s, a->status);
    hipLaunchKernelGGL(mcl_roots_kernel, grid, block, 0, stream, T, s);
    hipLaunchKernelGGL(mcl_number_kernel, dim3(1), block, 0, stream, nb, s, a->counts);
    hipLaunchKernelGGL(mcl_assign_kernel, grid, block, 0, stream, T, s, a->sizes);
    hipLaunchKernelGGL(mcl_label_kernel, grid, block, 0, stream, T, s, a->labels);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" size_t dnsplat_mesh_filter_scratch_bytes(int32_t V, int32_t T)
{
    if (V < 1 || T < 1) return 0;
    return mcf_bytes(V, T);
}

extern "C" int dnsplat_mesh_filter_count(const dnsplat_mesh_filter_args *a, dnsplat_stream_t stream_)
{
    if (!mcf_args_ok(a)) return DNSPLAT_ERR_INVALID_ARG;
    if (a->scratch_bytes < mcf_bytes(a->V, a->T) || (size_t)a->scratch % sizeof(unsigned long long)) return DNSPLAT_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const McfScratch s = mcf_carve(a->scratch, a->V, a->T);
    const int V = a->V, T = a->T, nbt = mv_blocks(T), nbv = mv_blocks(V);
    const dim3 block(MCL_THREADS);
    // the histograms, the selection's state and the marks are one run of the scratch
    if (hipMemsetAsync(s.hist, 0, ((size_t)MCL_ROUNDS * MCL_BINS + 2) * sizeof(unsigned long long) + (size_t)V * sizeof(int32_t), stream) != hipSuccess)
        return DNSPLAT_ERR_LAUNCH;
    for (int round = 0; round < MCL_ROUNDS; ++round) {
        hipLaunchKernelGGL(mcf_hist_kernel, dim3((unsigned)nbt), block, 0, stream, round, V, T, a->sizes, a->cluster_counts, a->scratch);
        hipLaunchKernelGGL(mcf_select_kernel, dim3(1), block, 0, stream, round, V, T, a->cluster_counts, a->keep_largest, a->min_triangles, a->scratch,
                           a->threshold);
    }
    hipLaunchKernelGGL(mcf_keep_kernel, dim3((unsigned)nbt), block, 0, stream, V, T, a->triangles, a->labels, a->sizes, a->threshold, s.marks, s.tcount,
                       s.keep);
    hipLaunchKernelGGL(mv_mark_count_kernel, dim3((unsigned)nbv), block, 0, stream, V, s.marks, s.vcount);
    hipLaunchKernelGGL(mv_cut_scan_kernel, dim3(1), block, 0, stream, nbv, s.vcount, nbt, s.tcount, a->counts);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}

extern "C" int dnsplat_mesh_filter_emit(const dnsplat_mesh_filter_args *a, dnsplat_stream_t stream_)
{
    if (!mcf_args_ok(a) || !a->status || a->cap_v < 0 || a->cap_t < 0) return DNSPLAT_ERR_INVALID_ARG;
    if ((a->cap_v > 0 && !a->vertex_index) || (a->cap_t > 0 && !a->out_triangles)) return DNSPLAT_ERR_INVALID_ARG;
    if (a->scratch_bytes < mcf_bytes(a->V, a->T) || (size_t)a->scratch % sizeof(unsigned long long)) return DNSPLAT_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const McfScratch s = mcf_carve(a->scratch, a->V, a->T);
    hipLaunchKernelGGL(mcf_emit_vertices_kernel, dim3((unsigned)mv_blocks(a->V)), dim3(MCL_THREADS), 0, stream, a->V, s.vcount, s.marks,
                       (long long)a->cap_v, a->vertex_index);
    hipLaunchKernelGGL(mv_emit_triangles_kernel, dim3((unsigned)mv_blocks(a->T)), dim3(MCL_THREADS), 0, stream, a->T, a->triangles, s.keep, s.tcount,
                       s.marks, a->counts, (long long)a->cap_v, (long long)a->cap_t, a->out_triangles, a->status);
    DNS_CHECK_LAUNCH();
    return DNSPLAT_OK;
}
