// mesh_colour.hip -- levelling the colours across the seams of a textured mesh on the MI355X (gfx950, wave64).
//
// The contract is the project's own (include/sfmba.h, "levelling the colours across seams"; the rules are in colour_math.h): past the
// fixed-point image coordinate everything is INTEGER arithmetic and NO RESULT COMES FROM AN ATOMIC -- so the result is BIT-EXACT with a
// CPU restatement (tests/colour_oracle.py) however the work is cut.
//
//   nodes         k_col_keys: a lane per triangle writes its three ((vertex << 32) | view, 3 t + q) pairs, COLOUR_NO_KEY for a triangle
//                 that does not contribute; one stable sort_pairs_u64 (the structure build's configuration); k_col_heads marks the first
//                 entry of every distinct key, one exclusive sum numbers the nodes, and k_col_scatter, a lane per sorted entry, writes
//                 node_of, the node's vertex and view and the start of its run: the sorted order IS the list of every node's entries.
//   colours       k_col_colours: a lane per node: one projection, (2 r + 1)^2 bilinear samples per channel, the mean in 1/256 level.
//   a pass        k_col_pass: THE HOT KERNEL.  A lane per node.  Its siblings (the nodes of its vertex) are its neighbours in the node
//                 order, so their F + g are contiguous 16-byte records; then it walks its own run of entries, and for each reads the two
//                 other nodes of the triangle's row and their offsets.  A vertex of a grid mesh has about six triangles: twelve gathers
//                 of 16 bytes, most of them from lines a nearby lane has fetched.  Jacobi between two buffers, one launch per pass, no
//                 wait between passes.  A fan is handled by the loop.
//   statistics    k_col_stats: per workgroup the sums and the maximum by a tree in LDS, stored per workgroup; k_col_total, one
//                 workgroup, adds them up.  No atomic.
//
// SCRATCH for T triangles and n <= 3 T nodes: the sort 2 (8 + 4) 3 T and its temporaries, 8 (3 T + 1) for the heads and their sum,
// 12 T node_of, 8 n vertex and view, 16 n each for F, the ranges and the two offset buffers.
#include "mesh_colour.h"
#include "ba_kernels.h"    // sort_pairs_u64

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;
using u64 = unsigned long long;

unsigned blocks_for(long long n) { return (unsigned)((n + LANES - 1) / LANES); }

__global__ __launch_bounds__(LANES) void k_col_check_view(int nt, int n_images, const int* __restrict__ view, int* __restrict__ flag) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    if (t >= nt) return;
    const int v = view[t];
    if (v < -1 || v >= n_images) { flag[0] = 1; flag[1] = 1; }
}

__global__ __launch_bounds__(LANES) void k_col_keys(int nt, const float* __restrict__ xyz, const int* __restrict__ tri, const int* __restrict__ view,
                                                    u64* __restrict__ keys, int* __restrict__ vals) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    if (t >= nt) return;
    const int idx[3] = { tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2] };
    double A[3], B[3], C[3];
    load_vertex(xyz, idx[0], A);
    load_vertex(xyz, idx[1], B);
    load_vertex(xyz, idx[2], C);
    const int v = view[t];
    const bool on = colour_contributes(v, idx[0], idx[1], idx[2], A, B, C);
    for (int q = 0; q < 3; ++q) {
        keys[3 * (size_t)t + q] = on ? colour_key(idx[q], v) : COLOUR_NO_KEY;
        vals[3 * (size_t)t + q] = (int)(3 * t + q);
    }
}

// the keys of the stand-alone levelling: the node of every entry, so that the sorted order lists every node's entries
__global__ __launch_bounds__(LANES) void k_col_node_keys(long long n, const int* __restrict__ node_of, u64* __restrict__ keys, int* __restrict__ vals) {
    const long long i = (long long)blockIdx.x * LANES + threadIdx.x;
    if (i >= n) return;
    const int v = node_of[i];
    keys[i] = v < 0 ? 0xffffffffULL : (u64)v;
    vals[i] = (int)i;
}
// run[n] for n = 0 .. n_nodes: the first sorted entry whose key is not below n
__global__ __launch_bounds__(LANES) void k_col_bounds(int n_nodes, long long n, const u64* __restrict__ keys, int* __restrict__ run) {
    const long long node = (long long)blockIdx.x * LANES + threadIdx.x;
    if (node > n_nodes) return;
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < (u64)node) lo = mid + 1; else hi = mid;
    }
    run[node] = (int)lo;
}

// head[i] = 1 where the sorted entry i begins a node; head[n] = 0
__global__ __launch_bounds__(LANES) void k_col_heads(long long n, const u64* __restrict__ keys, int* __restrict__ head) {
    const long long i = (long long)blockIdx.x * LANES + threadIdx.x;
    if (i > n) return;
    head[i] = i < n && keys[i] != COLOUR_NO_KEY && (i == 0 || keys[i - 1] != keys[i]);
}
// before[i]: the heads in front of entry i (before[n]: the number of nodes).  n + 1 lanes: the last one, or the first entry without a
// key, ends the last node's run.
__global__ __launch_bounds__(LANES) void k_col_scatter(long long n, const u64* __restrict__ keys, const int* __restrict__ vals, const int* __restrict__ head,
                                                       const int* __restrict__ before, int* __restrict__ node_of, int* __restrict__ node_vertex,
                                                       int* __restrict__ node_view, int* __restrict__ run) {
    const long long i = (long long)blockIdx.x * LANES + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        if (n == 0 || keys[n - 1] != COLOUR_NO_KEY) run[before[n]] = (int)n;
        return;
    }
    const u64 key = keys[i];
    if (key == COLOUR_NO_KEY) {
        node_of[vals[i]] = -1;
        if (i == 0 || keys[i - 1] != COLOUR_NO_KEY) run[before[i]] = (int)i;
        return;
    }
    const int id = before[i] + head[i] - 1;
    node_of[vals[i]] = id;
    if (head[i]) {
        node_vertex[id] = (int)(key >> 32);
        node_view[id] = (int)(key & 0xffffffffULL);
        run[id] = (int)i;
    }
}

__global__ __launch_bounds__(LANES) void k_col_colours(TexKernelParams prm, const int* __restrict__ n_nodes, const float* __restrict__ xyz,
                                                       const TexImage* __restrict__ tab, const unsigned char* __restrict__ raw,
                                                       const int* __restrict__ node_vertex, const int* __restrict__ node_view, int radius,
                                                       int4* __restrict__ F) {
    const long long n = (long long)blockIdx.x * LANES + threadIdx.x;
    if (n >= n_nodes[0]) return;
    double X[3];
    load_vertex(xyz, node_vertex[n], X);
    const TexView V = view_of(tab[node_view[n]], nullptr, raw);
    long long sum[3];
    int f[3];
    const bool seen = colour_node(prm.k4, V, prm.channels, X, radius, sum, f);
    F[n] = make_int4(f[0], f[1], f[2], seen ? 1 : 0);
}

// a node's ranges: its run of entries and the nodes of its vertex, itself included
__global__ __launch_bounds__(LANES) void k_col_ranges(int n_nodes, const int* __restrict__ node_vertex, const int* __restrict__ run, const int4* __restrict__ F,
                                                      int4* __restrict__ range, int4* __restrict__ ga, int4* __restrict__ gb) {
    const long long n = (long long)blockIdx.x * LANES + threadIdx.x;
    if (n >= n_nodes) return;
    const int v = node_vertex[n];
    int lo = (int)n, hi = (int)n + 1;
    while (lo > 0 && node_vertex[lo - 1] == v) --lo;
    while (hi < n_nodes && node_vertex[hi] == v) ++hi;
    range[n] = make_int4(run[n], run[n + 1], lo, hi);
    const int4 zero = make_int4(0, 0, 0, F[n].w);
    ga[n] = zero;
    gb[n] = zero;
}

__global__ __launch_bounds__(LANES) void k_col_pass(int n_nodes, int weight, const int4* __restrict__ range, const int4* __restrict__ F,
                                                    const int* __restrict__ entry, const int* __restrict__ node_of, const int4* __restrict__ g_in,
                                                    int4* __restrict__ g_out) {
    const long long n = (long long)blockIdx.x * LANES + threadIdx.x;
    if (n >= n_nodes) return;
    const int4 Fn = F[n], gn = g_in[n];
    if (!Fn.w) { g_out[n] = make_int4(0, 0, 0, 0); return; }
    const int4 R = range[n];
    long long sib[3] = { 0, 0, 0 }, B[3] = { 0, 0, 0 };
    int k = 0, b = 0;
    for (int m = R.z; m < R.w; ++m) {
        const int4 Fm = F[m];
        if (!Fm.w) continue;
        const int4 gm = g_in[m];
        sib[0] += Fm.x + gm.x; sib[1] += Fm.y + gm.y; sib[2] += Fm.z + gm.z;
        ++k;
    }
    for (int i = R.x; i < R.y; ++i) {
        const int e = entry[i], t = e / 3, q = e - 3 * t;
        for (int o = 1; o < 3; ++o) {
            const int u = node_of[3 * (size_t)t + (q + o) % 3];
            const int4 gu = g_in[u];
            if (!gu.w) continue;
            B[0] += gu.x; B[1] += gu.y; B[2] += gu.z;
            ++b;
        }
    }
    long long num, den;
    g_out[n] = make_int4(colour_update(weight, k, sib[0], Fn.x, b, B[0], gn.x, num, den), colour_update(weight, k, sib[1], Fn.y, b, B[1], gn.y, num, den),
                         colour_update(weight, k, sib[2], Fn.z, b, B[2], gn.z, num, den), 1);
}

// v[0..3] are summed and v[4] is maximised over the workgroup; lane 0 stores the five to out.  EVERY lane must call it.
__device__ __forceinline__ void block_total5(const long long* v, long long* __restrict__ out) {
    __shared__ long long s_v[5][LANES];
    for (int c = 0; c < 5; ++c) s_v[c][threadIdx.x] = v[c];
    __syncthreads();
    for (int step = LANES / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) {
            for (int c = 0; c < 4; ++c) s_v[c][threadIdx.x] += s_v[c][threadIdx.x + step];
            s_v[4][threadIdx.x] = max(s_v[4][threadIdx.x], s_v[4][threadIdx.x + step]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int c = 0; c < 5; ++c) out[c] = s_v[c][0];
}
// per workgroup: blind nodes, seam vertices, the spread of F and of F + g over the seam vertices' siblings, the largest |g|
__global__ __launch_bounds__(LANES) void k_col_stats(int n_nodes, const int4* __restrict__ range, const int4* __restrict__ F, const int4* __restrict__ g,
                                                     long long* __restrict__ partial) {
    const long long n = (long long)blockIdx.x * LANES + threadIdx.x;
    long long v[5] = { 0, 0, 0, 0, 0 };
    if (n < n_nodes) {
        const int4 Fn = F[n], gn = g[n], R = range[n];
        v[0] = !Fn.w;
        v[4] = max(max(abs(gn.x), abs(gn.y)), abs(gn.z));
        if (R.z == (int)n) {                                 // the first node of its vertex speaks for the vertex
            int k = 0, lo0[3], hi0[3], lo1[3], hi1[3];
            for (int m = R.z; m < R.w; ++m) {
                const int4 Fm = F[m];
                if (!Fm.w) continue;
                const int4 gm = g[m];
                const int f[3] = { Fm.x, Fm.y, Fm.z }, fg[3] = { Fm.x + gm.x, Fm.y + gm.y, Fm.z + gm.z };
                for (int c = 0; c < 3; ++c) {
                    lo0[c] = k ? min(lo0[c], f[c]) : f[c];
                    hi0[c] = k ? max(hi0[c], f[c]) : f[c];
                    lo1[c] = k ? min(lo1[c], fg[c]) : fg[c];
                    hi1[c] = k ? max(hi1[c], fg[c]) : fg[c];
                }
                ++k;
            }
            if (k >= 2) {
                v[1] = 1;
                for (int c = 0; c < 3; ++c) { v[2] += hi0[c] - lo0[c]; v[3] += hi1[c] - lo1[c]; }
            }
        }
    }
    block_total5(v, partial + 5 * (size_t)blockIdx.x);
}
__global__ __launch_bounds__(LANES) void k_col_total(int n_partials, const long long* __restrict__ partial, long long* __restrict__ out) {
    long long v[5] = { 0, 0, 0, 0, 0 };
    for (int i = threadIdx.x; i < n_partials; i += LANES) {
        for (int c = 0; c < 4; ++c) v[c] += partial[5 * (size_t)i + c];
        v[4] = max(v[4], partial[5 * (size_t)i + 4]);
    }
    block_total5(v, out);
}

#define COL_COPY(dst, src, bytes, kind) do { if ((bytes) > 0) UNIT_TRY(hipMemcpyAsync(dst, src, bytes, kind, s)); } while (0)
#define COL_BEGIN(p) do { if (tm) tm->begin(p); } while (0)
#define COL_END() do { if (tm) tm->end(); } while (0)

// one stable sort of n (key, value) pairs into k1, v1
int sort_entries(hipStream_t s, DeviceArena& raw, u64* k0, u64* k1, int* v0, int* v1, size_t n, int end_bit) {
    size_t sort_bytes = 0;
    if (int rc = sort_pairs_u64(s, nullptr, &sort_bytes, k0, k1, v0, v1, (unsigned)n, end_bit)) return rc;
    void* d_tmp = raw.alloc(std::max(sort_bytes, (size_t)1));
    if (!d_tmp) return (int)hipErrorOutOfMemory;
    return sort_pairs_u64(s, d_tmp, &sort_bytes, k0, k1, v0, v1, (unsigned)n, end_bit);
}

}  // namespace

int colour_nodes_dev(hipStream_t s, DeviceArena& raw, const TexKernelParams& prm, const float* d_xyz, const int* d_tri, const TexImage* d_tab,
                     const unsigned char* d_raw, const int* d_view, int radius, ColourNodes& out, int& n_nodes, PhaseTimer* tm) {
    n_nodes = 0;
    const int nt = prm.nt;
    if (nt <= 0) return 0;
    const size_t N = 3 * (size_t)nt;
    u64 *d_k0, *d_k1;
    int *d_v0, *d_head, *d_before;
    UNIT_ALLOC(raw, d_k0, u64, N);
    UNIT_ALLOC(raw, d_k1, u64, N);
    UNIT_ALLOC(raw, d_v0, int, N);
    UNIT_ALLOC(raw, out.entry, int, N);
    UNIT_ALLOC(raw, d_head, int, N + 1);
    UNIT_ALLOC(raw, d_before, int, N + 1);
    UNIT_ALLOC(raw, out.node_of, int, N);
    UNIT_ALLOC(raw, out.node_vertex, int, N);
    UNIT_ALLOC(raw, out.node_view, int, N);
    UNIT_ALLOC(raw, out.run, int, N + 1);
    UNIT_ALLOC(raw, out.F, int4, N);
    size_t scan_bytes = 0;
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, d_head, d_before, (unsigned)(N + 1), s));
    void* d_scan = raw.alloc(std::max(scan_bytes, (size_t)1));
    if (!d_scan) return (int)hipErrorOutOfMemory;

    COL_BEGIN(COL_T_KEYS);
    hipLaunchKernelGGL(k_col_keys, dim3(blocks_for(nt)), dim3(LANES), 0, s, nt, d_xyz, d_tri, d_view, d_k0, d_v0);
    UNIT_TRY(hipGetLastError());
    COL_END();
    COL_BEGIN(COL_T_SORT);
    if (int rc = sort_entries(s, raw, d_k0, d_k1, d_v0, out.entry, N, 64)) return rc;      // COLOUR_NO_KEY has every bit set
    COL_END();
    COL_BEGIN(COL_T_NODES);
    hipLaunchKernelGGL(k_col_heads, dim3(blocks_for((long long)N + 1)), dim3(LANES), 0, s, (long long)N, d_k1, d_head);
    UNIT_TRY(hipGetLastError());
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, d_head, d_before, (unsigned)(N + 1), s));
    hipLaunchKernelGGL(k_col_scatter, dim3(blocks_for((long long)N + 1)), dim3(LANES), 0, s, (long long)N, d_k1, out.entry, d_head, d_before, out.node_of,
                       out.node_vertex, out.node_view, out.run);
    UNIT_TRY(hipGetLastError());
    COL_END();
    COL_BEGIN(COL_T_COLOURS);
    hipLaunchKernelGGL(k_col_colours, dim3(blocks_for((long long)N)), dim3(LANES), 0, s, prm, d_before + N, d_xyz, d_tab, d_raw, out.node_vertex, out.node_view,
                       radius, out.F);
    UNIT_TRY(hipGetLastError());
    COL_END();
    UNIT_TRY(hipMemcpyAsync(&n_nodes, d_before + N, sizeof(int), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    return 0;
}

int colour_level_dev(hipStream_t s, DeviceArena& raw, int n_nodes, const int* d_node_vertex, const int4* d_F, const int* d_node_of, const int* d_entry,
                     const int* d_run, int weight, int passes, const int4** d_g, int64_t* stats, PhaseTimer* tm) {
    for (int i = 0; i < COLOUR_STATS; ++i) stats[i] = 0;
    stats[COLOUR_S_PASSES] = passes;
    *d_g = nullptr;
    if (n_nodes <= 0) return 0;
    const size_t NN = (size_t)n_nodes;
    const unsigned blocks = blocks_for(n_nodes);
    int4 *d_range, *d_ga, *d_gb;
    long long *d_partial, *d_total;
    UNIT_ALLOC(raw, d_range, int4, NN);
    UNIT_ALLOC(raw, d_ga, int4, NN);
    UNIT_ALLOC(raw, d_gb, int4, NN);
    UNIT_ALLOC(raw, d_partial, long long, 5 * (size_t)blocks);
    UNIT_ALLOC(raw, d_total, long long, 5);
    const dim3 grid(blocks), block(LANES);
    COL_BEGIN(COL_T_PASSES);
    hipLaunchKernelGGL(k_col_ranges, grid, block, 0, s, n_nodes, d_node_vertex, d_run, d_F, d_range, d_ga, d_gb);
    UNIT_TRY(hipGetLastError());
    const int4* cur = d_ga;
    for (int p = 0; p < passes; ++p) {
        int4* nxt = (p & 1) ? d_ga : d_gb;
        hipLaunchKernelGGL(k_col_pass, grid, block, 0, s, n_nodes, weight, d_range, d_F, d_entry, d_node_of, cur, nxt);
        UNIT_TRY(hipGetLastError());
        cur = nxt;
    }
    COL_END();
    COL_BEGIN(COL_T_STATS);
    hipLaunchKernelGGL(k_col_stats, grid, block, 0, s, n_nodes, d_range, d_F, cur, d_partial);
    UNIT_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_col_total, dim3(1), block, 0, s, (int)blocks, d_partial, d_total);
    UNIT_TRY(hipGetLastError());
    COL_END();
    long long tot[5];
    UNIT_TRY(hipMemcpyAsync(tot, d_total, sizeof(tot), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    stats[COLOUR_S_NODES] = n_nodes;
    stats[COLOUR_S_BLIND] = tot[0];
    stats[COLOUR_S_SEAM_VERTICES] = tot[1];
    stats[COLOUR_S_SPREAD_BEFORE] = tot[2];
    stats[COLOUR_S_SPREAD_AFTER] = tot[3];
    stats[COLOUR_S_MAX_G] = tot[4];
    *d_g = cur;
    return 0;
}

// ---- the two calls on host arrays ---------------------------------------------------------------------------------------------------
int mesh_colour_nodes(hipStream_t s, int device, const TexMesh& m, const TexViews& v, const int32_t* view, int radius, int64_t* n_nodes,
                      int32_t* node_vertex, int32_t* node_view, int32_t* node_of, unsigned char* seen, int32_t* F) {
    DeviceArena scratch(device), raw(device);
    raw.set_zeroing(false);                                      // the temporaries: written in full before they are read
    const size_t NV = (size_t)m.nv, NT = (size_t)m.nt;
    std::vector<TexImage> tab;
    long long n_map = 0, n_raw = 0;
    std::vector<const float*> no_maps((size_t)std::max(v.n_images, 1), nullptr);
    TexViews vv = v;
    vv.depth = no_maps.data();                                   // the labels are given: nothing is tested
    tex_view_table(vv, tab, n_map, n_raw);
    int *d_flag, *d_tri, *d_view;
    float* d_xyz;
    TexImage* d_tab;
    unsigned char* d_raw;
    UNIT_ALLOC(scratch, d_flag, int, 2);                         // zeroed
    UNIT_ALLOC(scratch, d_tri, int, NT * 3);
    UNIT_ALLOC(scratch, d_view, int, NT);
    UNIT_ALLOC(scratch, d_xyz, float, NV * 3);
    UNIT_ALLOC(scratch, d_tab, TexImage, tab.size());
    UNIT_ALLOC(scratch, d_raw, unsigned char, (size_t)n_raw);
    COL_COPY(d_tri, m.tri, sizeof(int) * NT * 3, hipMemcpyHostToDevice);
    COL_COPY(d_view, view, sizeof(int) * NT, hipMemcpyHostToDevice);
    COL_COPY(d_xyz, m.xyz, sizeof(float) * NV * 3, hipMemcpyHostToDevice);
    COL_COPY(d_tab, tab.data(), sizeof(TexImage) * tab.size(), hipMemcpyHostToDevice);
    for (int i = 0; i < v.n_images; ++i) {
        const TexImage& T = tab[(size_t)i];
        COL_COPY(d_raw + T.raw_off, v.pixels + v.img_ptr[i], (size_t)T.w * T.h * v.channels, hipMemcpyHostToDevice);
    }
    TexKernelParams prm;
    std::memset(&prm, 0, sizeof(prm));
    tex_camera_params(v, 0.0f, 0, prm);
    prm.nv = m.nv; prm.nt = m.nt;
    if (int rc = tex_check_indices(s, m.nt, m.nv, d_tri, d_flag)) return rc;
    if (m.nt > 0) {
        hipLaunchKernelGGL(k_col_check_view, dim3(blocks_for(m.nt)), dim3(LANES), 0, s, m.nt, v.n_images, d_view, d_flag);
        UNIT_TRY(hipGetLastError());
    }
    int flag[2] = { 0, 0 };
    UNIT_TRY(hipMemcpyAsync(flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));                           // a list with a bad index or a bad view goes no further
    if (flag[1]) return TEX_ERR_VIEW;
    if (flag[0]) return TEX_ERR_INDEX;
    ColourNodes nodes;
    int nn = 0;
    if (int rc = colour_nodes_dev(s, raw, prm, d_xyz, d_tri, d_tab, d_raw, d_view, radius, nodes, nn, nullptr)) return rc;
    std::vector<int4> f((size_t)nn);
    COL_COPY(node_of, nodes.node_of, sizeof(int) * NT * 3, hipMemcpyDeviceToHost);
    COL_COPY(node_vertex, nodes.node_vertex, sizeof(int) * (size_t)nn, hipMemcpyDeviceToHost);
    COL_COPY(node_view, nodes.node_view, sizeof(int) * (size_t)nn, hipMemcpyDeviceToHost);
    COL_COPY(f.data(), nodes.F, sizeof(int4) * (size_t)nn, hipMemcpyDeviceToHost);
    UNIT_TRY(hipStreamSynchronize(s));
    for (size_t n = 0; n < (size_t)nn; ++n) {
        F[3 * n] = f[n].x; F[3 * n + 1] = f[n].y; F[3 * n + 2] = f[n].z;
        seen[n] = (unsigned char)f[n].w;
    }
    *n_nodes = nn;
    return 0;
}

int mesh_colour_level(hipStream_t s, int device, int n_nodes, const int32_t* node_vertex, const unsigned char* seen, const int32_t* F, int nt,
                      const int32_t* node_of, int weight, int passes, int32_t* g, int64_t* stats) {
    DeviceArena raw(device);
    raw.set_zeroing(false);                                      // everything is written in full before it is read
    const size_t NN = (size_t)n_nodes, N = 3 * (size_t)nt;
    std::vector<int4> f(NN);
    for (size_t n = 0; n < NN; ++n) f[n] = make_int4(F[3 * n], F[3 * n + 1], F[3 * n + 2], seen[n] ? 1 : 0);
    int *d_node_vertex, *d_node_of, *d_v0, *d_entry, *d_run;
    u64 *d_k0, *d_k1;
    int4* d_F;
    UNIT_ALLOC(raw, d_node_vertex, int, NN);
    UNIT_ALLOC(raw, d_F, int4, NN);
    UNIT_ALLOC(raw, d_node_of, int, N);
    UNIT_ALLOC(raw, d_k0, u64, N);
    UNIT_ALLOC(raw, d_k1, u64, N);
    UNIT_ALLOC(raw, d_v0, int, N);
    UNIT_ALLOC(raw, d_entry, int, N);
    UNIT_ALLOC(raw, d_run, int, NN + 1);
    COL_COPY(d_node_vertex, node_vertex, sizeof(int) * NN, hipMemcpyHostToDevice);
    COL_COPY(d_F, f.data(), sizeof(int4) * NN, hipMemcpyHostToDevice);
    COL_COPY(d_node_of, node_of, sizeof(int) * N, hipMemcpyHostToDevice);
    if (N > 0) {
        hipLaunchKernelGGL(k_col_node_keys, dim3(blocks_for((long long)N)), dim3(LANES), 0, s, (long long)N, d_node_of, d_k0, d_v0);
        UNIT_TRY(hipGetLastError());
        if (int rc = sort_entries(s, raw, d_k0, d_k1, d_v0, d_entry, N, 32)) return rc;
    }
    hipLaunchKernelGGL(k_col_bounds, dim3(blocks_for((long long)NN + 1)), dim3(LANES), 0, s, n_nodes, (long long)N, d_k1, d_run);
    UNIT_TRY(hipGetLastError());
    const int4* d_g = nullptr;
    int64_t st[COLOUR_STATS];
    if (int rc = colour_level_dev(s, raw, n_nodes, d_node_vertex, d_F, d_node_of, d_entry, d_run, weight, passes, &d_g, st, nullptr)) return rc;
    std::vector<int4> out(NN);
    if (d_g) COL_COPY(out.data(), d_g, sizeof(int4) * NN, hipMemcpyDeviceToHost);
    UNIT_TRY(hipStreamSynchronize(s));                           // also: `f` is spent
    for (size_t n = 0; n < NN; ++n) { g[3 * n] = out[n].x; g[3 * n + 1] = out[n].y; g[3 * n + 2] = out[n].z; }
    for (int i = 0; i < COLOUR_STATS; ++i) stats[i] = st[i];
    return 0;
}

}  // namespace sfmba
