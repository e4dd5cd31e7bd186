// mesh_decimate.hip -- fewer, larger triangles for everything that follows the mesh, on the MI355X (gfx950, wave64): out-of-core
// vertex clustering with quadric placement (Lindstrom 2000), stated in integers.
//
// The contract is the project's own (include/sfmba.h, sfmba_mesh_decimate; arithmetic in decimate_math.h): positions are quantised as
// sfmba_mesh_smooth quantises them, a vertex belongs to the cell of its quantised position, and NOTHING BUT INTEGERS is summed across
// vertices or triangles -- so the result does not depend on the order in which atomics arrive or on how the work is cut, and is
// BIT-EXACT with a CPU restatement.
//
//   check, keys   k_dec_check: a lane per triangle holds its indices to 0 .. nv-1; k_dec_keys: a lane per vertex -> P int32 [nv][3],
//                 (cell key, index); each raises its device flag.  No kernel before the one wait follows an index.
//   sort          rocPRIM's stable radix sort of the pairs with the structure build's configuration (sort_pairs_u64), 63 bits.
//   runs          k_dec_heads, a hipCUB inclusive sum, k_dec_starts: run_start [n_clusters + 1] and the cluster of every vertex.  THE
//                 ONE WAIT before the totals: the flags and the number of clusters.
//   members       the segmented reduction of cloud_merge.hip, no atomic on a sum: k_dec_members_short, a lane per run of up to
//                 DEC_SHORT_RUN members, appends a longer run to a list; k_dec_members_long, a wave per long run with a shuffle tree.
//                 Six sums a cluster ([sum][cluster]): the remainders r and the colour bytes.
//   quadrics      k_dec_quadrics: a lane per triangle; the integer cross product, one fp64 square root, and per DISTINCT cluster of
//                 its vertices ten int64 atomicAdds into [cluster][10] (A00 A01 A02 A11 A12 A22 b0 b1 b2 n_inc); vertices that
//                 share a cluster are summed in registers first.  SCATTERED WITH ATOMICS: the sorted incidence list was not built,
//                 see DESIGN.md.
//   solve         k_dec_solve: a lane per cluster, dec_solve or the mean; the position and the colour of every cluster.
//   map           k_dec_map: a lane per triangle -> collapsed or (lo, mid, hi) of its clusters.
//   dedup         two stable radix passes over the triangles: by hi, then by lo << B | mid (B = the bits of a cluster rank; a collapsed
//                 triangle carries bit 2 B and sorts last).  Stable and fed ascending indices: the first of a run of equal triples
//                 is the lowest input index.  k_dec_dups keeps that one.
//   compact       k_dec_used, two hipCUB exclusive sums, the wait for the totals, k_dec_emit_tri, k_dec_emit_vtx, k_dec_vertex_of.
//
// SCRATCH, for V vertices, T triangles and C <= V clusters: the mesh 15 V + 12 T, P 12 V, the sort 24 V + its temporaries, runs
// 16 V, sums 48 C, quadrics 80 C, cluster outputs 15 C, triangle keys 28 T, the second sort 8 T, flags and sums 8 T + 8 C, outputs.
#include "mesh_decimate.h"
#include "decimate_math.h"
#include "ba_kernels.h"    // sort_pairs_u64
#include "device_arena.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>

namespace sfmba {

namespace {

constexpr int LANES = 256;
constexpr int WAVE = 64;
constexpr int LONG_BLOCKS = 1024;      // resident workgroups of the long-run kernel
constexpr int DEC_SHORT_RUN = 32;      // a run of more members is reduced by a wave
typedef unsigned long long u64;

struct QuantDev { double origin[3], quantum; };

__device__ __forceinline__ long long lane_index() { return (long long)blockIdx.x * LANES + threadIdx.x; }

// adds the number of lanes of the wave that pass `f` to *ctr with one atomic
__device__ __forceinline__ void count_lanes(bool f, u64* ctr) {
    const u64 m = __ballot(f);
    if (f && (int)(threadIdx.x & (WAVE - 1)) == __ffsll((long long)m) - 1) atomicAdd(ctr, (u64)__popcll(m));
}

// flags[0]: a triangle index outside the vertex list; flags[1]: a coordinate that does not quantise
__global__ __launch_bounds__(LANES) void k_dec_check(int nt, int nv, const int* __restrict__ tri, int* __restrict__ flags) {
    const long long t = lane_index();
    if (t >= nt) return;
    bool b = false;
    for (int q = 0; q < 3; ++q) {
        const int v = tri[3 * (size_t)t + q];
        b = b || v < 0 || v >= nv;
    }
    if (b) flags[0] = 1;
}

__global__ __launch_bounds__(LANES) void k_dec_keys(int nv, const float* __restrict__ xyz, QuantDev q, int cell, int* __restrict__ P, u64* __restrict__ keys,
                                                    int* __restrict__ idx, int* __restrict__ flags) {
    const long long v = lane_index();
    if (v >= nv) return;
    bool bad = false;
    long long c[3];
    for (int a = 0; a < 3; ++a) {
        long long p = 0, r;
        if (!clean_quantise(xyz[3 * (size_t)v + a], q.origin[a], q.quantum, p)) { bad = true; p = 0; }
        P[3 * (size_t)v + a] = (int)p;
        dec_cell(p, (long long)cell, c[a], r);
    }
    keys[v] = dec_key(c);
    idx[v] = (int)v;
    if (bad) flags[1] = 1;
}

__global__ __launch_bounds__(LANES) void k_dec_heads(int n, const u64* __restrict__ ks, int* __restrict__ head) {
    const long long p = lane_index();
    if (p >= n) return;
    head[p] = (p == 0 || ks[p - 1] != ks[p]) ? 1 : 0;
}

// run_start [n_runs + 1], the cluster of every vertex and info[0] = n_runs
__global__ __launch_bounds__(LANES) void k_dec_starts(int n, const int* __restrict__ head, const int* __restrict__ rank, const int* __restrict__ is,
                                                      int* __restrict__ run_start, int* __restrict__ cluster_of, int* __restrict__ info) {
    const long long p = lane_index();
    if (p >= n) return;
    const int r = rank[p];                                   // 1-based run number
    if (head[p]) run_start[r - 1] = (int)p;
    cluster_of[is[p]] = r - 1;
    if (p == n - 1) {
        run_start[r] = n;
        info[0] = r;
    }
}

// ---- member sums -----------------------------------------------------------------------------------------------------------------
struct MemberIn {
    const int* P;
    const unsigned char* bgr;     // or NULL
    int cell;
};
// [sum][run]: r 0..2, then b, g, r
struct MemberSums { long long* sum; long long stride; };

__device__ __forceinline__ void dec_add_member(const MemberIn& in, int v, long long* acc) {
    for (int a = 0; a < 3; ++a) {
        long long c, r;
        dec_cell((long long)in.P[3 * (size_t)v + a], (long long)in.cell, c, r);
        acc[a] += r;
    }
    if (in.bgr)
        for (int a = 0; a < 3; ++a) acc[3 + a] += (long long)in.bgr[3 * (size_t)v + a];
}
__device__ __forceinline__ void dec_store_sums(const MemberSums& out, int r, const long long* acc) {
    for (int k = 0; k < 6; ++k) out.sum[k * out.stride + r] = acc[k];
}

__global__ __launch_bounds__(LANES) void k_dec_members_short(int n_runs, const int* __restrict__ run_start, const int* __restrict__ is, MemberIn in,
                                                             MemberSums out, int* __restrict__ long_list, int long_cap, int* __restrict__ n_long) {
    const long long r = lane_index();
    if (r >= n_runs) return;
    const int beg = run_start[r], end = run_start[r + 1];
    if (end - beg > DEC_SHORT_RUN) {
        const int slot = atomicAdd(n_long, 1);
        if (slot < long_cap) long_list[slot] = (int)r;       // cannot fail: long_cap = nv / (DEC_SHORT_RUN + 1) + 1
        return;
    }
    long long acc[6] = { 0, 0, 0, 0, 0, 0 };
    for (int p = beg; p < end; ++p) dec_add_member(in, is[p], acc);
    dec_store_sums(out, (int)r, acc);
}

__global__ __launch_bounds__(LANES) void k_dec_members_long(const int* __restrict__ run_start, const int* __restrict__ is, MemberIn in, MemberSums out,
                                                            const int* __restrict__ long_list, int long_cap, const int* __restrict__ n_long) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = (blockIdx.x * LANES + threadIdx.x) / WAVE, n_waves = gridDim.x * (LANES / WAVE);
    const int todo = min(*n_long, long_cap);
    for (int at = wave; at < todo; at += n_waves) {           // uniform over the wave
        const int r = long_list[at];
        const int beg = run_start[r], end = run_start[r + 1];
        long long acc[6] = { 0, 0, 0, 0, 0, 0 };
        for (long long p = (long long)beg + lane; p < end; p += WAVE) dec_add_member(in, is[p], acc);
        for (int k = 0; k < 6; ++k)
            for (int d = WAVE / 2; d >= 1; d >>= 1) acc[k] += __shfl_down(acc[k], d, WAVE);
        if (lane == 0) dec_store_sums(out, r, acc);
    }
}

// ---- quadrics --------------------------------------------------------------------------------------------------------------------
// (two's complement: an unsigned add of the bit pattern is the signed add)
__global__ __launch_bounds__(LANES) void k_dec_quadrics(int nt, const int* __restrict__ tri, const int* __restrict__ P, const int* __restrict__ cluster_of,
                                                        int cell, u64* __restrict__ Q) {
    const long long t = lane_index();
    if (t >= nt) return;
    const int v[3] = { tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2] };
    if (v[0] == v[1] || v[0] == v[2] || v[1] == v[2]) return;
    long long Pv[3][3], N[3], u[3];
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) Pv[k][a] = (long long)P[3 * (size_t)v[k] + a];
    clean_cross(Pv[0], Pv[1], Pv[2], N);
    if (!dec_unit_normal(N, u)) return;
    long long q[3][10];
    int cl[3];
    for (int k = 0; k < 3; ++k) {
        long long r[3], c;
        for (int a = 0; a < 3; ++a) dec_cell(Pv[k][a], (long long)cell, c, r[a]);
        dec_quadric_terms(u, r, q[k]);
        cl[k] = cluster_of[v[k]];
    }
    // vertices that share a cluster (most triangles: the collapsed ones) are summed here first: integers, so the result is the same
    if (cl[1] == cl[0]) {
        for (int i = 0; i < 10; ++i) q[0][i] += q[1][i];
        cl[1] = -1;
    }
    if (cl[2] == cl[0]) {
        for (int i = 0; i < 10; ++i) q[0][i] += q[2][i];
        cl[2] = -1;
    } else if (cl[2] == cl[1]) {
        for (int i = 0; i < 10; ++i) q[1][i] += q[2][i];
        cl[2] = -1;
    }
    for (int k = 0; k < 3; ++k) {
        if (cl[k] < 0) continue;
        u64* dst = Q + 10 * (size_t)cl[k];
        for (int i = 0; i < 10; ++i) atomicAdd(dst + i, (u64)q[k][i]);
    }
}

// the position and the colour of every cluster; stats[3] counts the clusters that placement 1 left to the mean
__global__ __launch_bounds__(LANES) void k_dec_solve(int n_runs, const int* __restrict__ run_start, const u64* __restrict__ ks, MemberSums sums,
                                                     const u64* __restrict__ Q, QuantDev qd, int cell, int placement, int reg, int colour,
                                                     float* __restrict__ cxyz, unsigned char* __restrict__ cbgr, u64* __restrict__ stats) {
    const long long r = lane_index();
    if (r >= n_runs) return;
    const int beg = run_start[r];
    const long long n = (long long)run_start[r + 1] - beg;
    long long c[3], Sp[3], R[3];
    dec_key_cell(ks[beg], c);
    for (int a = 0; a < 3; ++a) {
        Sp[a] = sums.sum[a * sums.stride + r];
        R[a] = dec_mean(Sp[a], n);
    }
    bool fell_back = false;
    if (placement == 1) {
        long long q[10];
        for (int i = 0; i < 10; ++i) q[i] = (long long)Q[10 * (size_t)r + i];
        fell_back = !dec_solve(q, Sp, n, (long long)reg, (long long)cell, R, nullptr);
    }
    count_lanes(fell_back, stats + 3);
    for (int a = 0; a < 3; ++a) cxyz[3 * (size_t)r + a] = dec_position(qd.origin[a], c[a], (long long)cell, R[a], qd.quantum);
    if (colour)
        for (int a = 0; a < 3; ++a) cbgr[3 * (size_t)r + a] = (unsigned char)dec_mean(sums.sum[(3 + a) * sums.stride + r], n);
}

// ---- triangles -------------------------------------------------------------------------------------------------------------------
// khi[t] = hi, klm[t] = lo << B | mid, or (collapsed) 0 and 1 << 2 B; stats[1] counts the collapsed
__global__ __launch_bounds__(LANES) void k_dec_map(int nt, const int* __restrict__ tri, const int* __restrict__ cluster_of, int B, u64* __restrict__ khi,
                                                   u64* __restrict__ klm, int* __restrict__ hi_of, int* __restrict__ idx, u64* __restrict__ stats) {
    const long long t = lane_index();
    if (t >= nt) return;
    int a = cluster_of[tri[3 * (size_t)t]], b = cluster_of[tri[3 * (size_t)t + 1]], c = cluster_of[tri[3 * (size_t)t + 2]];
    const bool collapsed = a == b || a == c || b == c;
    count_lanes(collapsed, stats + 1);
    int x;
    if (a > b) { x = a; a = b; b = x; }
    if (b > c) { x = b; b = c; c = x; }
    if (a > b) { x = a; a = b; b = x; }
    khi[t] = collapsed ? 0 : (u64)c;
    hi_of[t] = collapsed ? -1 : c;
    klm[t] = collapsed ? ((u64)1 << (2 * B)) : (((u64)a << B) | (u64)b);
    idx[t] = (int)t;
}

__global__ __launch_bounds__(LANES) void k_dec_gather(int nt, const int* __restrict__ ts, const u64* __restrict__ klm, u64* __restrict__ out) {
    const long long p = lane_index();
    if (p < nt) out[p] = klm[ts[p]];
}

// tkeep[t] = 1 for the first triangle of every run of equal cluster triples; stats[2] counts the others
__global__ __launch_bounds__(LANES) void k_dec_dups(int nt, int B, const u64* __restrict__ ks, const int* __restrict__ ts, const int* __restrict__ hi_of,
                                                    int* __restrict__ tkeep, u64* __restrict__ stats) {
    const long long p = lane_index();
    if (p >= nt) return;
    const u64 k = ks[p];
    const int t = ts[p];
    const bool valid = ((k >> (2 * B)) & 1) == 0;
    const bool head = p == 0 || ks[p - 1] != k || hi_of[ts[p - 1]] != hi_of[t];
    tkeep[t] = (valid && head) ? 1 : 0;
    count_lanes(valid && !head, stats + 2);
}

__global__ __launch_bounds__(LANES) void k_dec_used(int nt, const int* __restrict__ tri, const int* __restrict__ cluster_of, const int* __restrict__ tkeep,
                                                    int* __restrict__ used) {
    const long long t = lane_index();
    if (t >= nt || !tkeep[t]) return;
    for (int q = 0; q < 3; ++q) used[cluster_of[tri[3 * (size_t)t + q]]] = 1;       // every lane stores the same 1
}

__global__ __launch_bounds__(LANES) void k_dec_emit_tri(int nt, const int* __restrict__ tri, const int* __restrict__ cluster_of, const int* __restrict__ tkeep,
                                                        const int* __restrict__ toff, const int* __restrict__ coff, int* __restrict__ tri_out,
                                                        int* __restrict__ triangle_of) {
    const long long t = lane_index();
    if (t >= nt || !tkeep[t]) return;
    const size_t o = (size_t)toff[t];
    for (int q = 0; q < 3; ++q) tri_out[3 * o + q] = coff[cluster_of[tri[3 * (size_t)t + q]]];
    triangle_of[o] = (int)t;
}

__global__ __launch_bounds__(LANES) void k_dec_emit_vtx(int n_runs, const int* __restrict__ run_start, const int* __restrict__ used, const int* __restrict__ coff,
                                                        const float* __restrict__ cxyz, const unsigned char* __restrict__ cbgr, float* __restrict__ xyz_out,
                                                        unsigned char* __restrict__ bgr_out, int* __restrict__ members) {
    const long long r = lane_index();
    if (r >= n_runs || !used[r]) return;
    const size_t o = (size_t)coff[r];
    for (int a = 0; a < 3; ++a) xyz_out[3 * o + a] = cxyz[3 * (size_t)r + a];
    if (cbgr)
        for (int a = 0; a < 3; ++a) bgr_out[3 * o + a] = cbgr[3 * (size_t)r + a];
    members[o] = run_start[r + 1] - run_start[r];
}

__global__ __launch_bounds__(LANES) void k_dec_vertex_of(int nv, const int* __restrict__ cluster_of, const int* __restrict__ used, const int* __restrict__ coff,
                                                         int* __restrict__ vertex_of) {
    const long long v = lane_index();
    if (v >= nv) return;
    const int r = cluster_of[v];
    vertex_of[v] = used[r] ? coff[r] : -1;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
unsigned blocks_for(long long n) { return (unsigned)((n + LANES - 1) / LANES); }
int bits_for(u64 n) { int b = 1; while (b < 31 && ((u64)1 << b) < n) ++b; return b; }

// a lane per item; nothing is launched for no items
#define DEC_LAUNCH(n, kernel, ...)                                                                   \
    do {                                                                                             \
        if ((n) > 0) {                                                                               \
            hipLaunchKernelGGL(kernel, dim3(blocks_for(n)), dim3(LANES), 0, s, __VA_ARGS__);         \
            UNIT_TRY(hipGetLastError());                                                             \
        }                                                                                            \
    } while (0)
#define DEC_COPY(dst, src, bytes, kind) do { if ((bytes) > 0) UNIT_TRY(hipMemcpyAsync(dst, src, bytes, kind, s)); } while (0)

}  // namespace

int mesh_decimate(hipStream_t s, int device, const CleanMesh& m, const DecimateParams& prm, const DecimateOut& out, double* timing) {
    if (timing) for (int i = 0; i < DEC_T_COUNT; ++i) timing[i] = 0.0;
    const int nv = m.nv, nt = m.nt;
    if (nv == 0) {                                             // no index can be valid
        if (nt > 0) return CLEAN_ERR_INDEX;
        *out.n_vertices = 0;
        *out.n_triangles = 0;
        if (out.stats) for (int i = 0; i < 4; ++i) out.stats[i] = 0;
        return 0;
    }
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    DeviceArena scratch(device);
    const size_t NV = (size_t)nv, NT = (size_t)nt;
    QuantDev qd;
    for (int a = 0; a < 3; ++a) qd.origin[a] = prm.origin[a];
    qd.quantum = prm.quantum;

    float* d_xyz;
    unsigned char* d_bgr = nullptr;
    int *d_tri, *d_flags, *d_P, *d_i0, *d_i1, *d_head, *d_rank, *d_start, *d_cluster, *d_info;
    u64 *d_k0, *d_k1, *d_stats;
    UNIT_ALLOC(scratch, d_flags, int, 2);                         // zeroed
    UNIT_ALLOC(scratch, d_info, int, 2);                          // n_runs, n_long: zeroed
    UNIT_ALLOC(scratch, d_stats, u64, 4);                         // zeroed
    UNIT_ALLOC(scratch, d_tri, int, NT * 3);
    UNIT_ALLOC(scratch, d_xyz, float, NV * 3);
    if (m.bgr) UNIT_ALLOC(scratch, d_bgr, unsigned char, NV * 3);
    UNIT_ALLOC(scratch, d_P, int, NV * 3);
    UNIT_ALLOC(scratch, d_k0, u64, NV);
    UNIT_ALLOC(scratch, d_k1, u64, NV);
    UNIT_ALLOC(scratch, d_i0, int, NV);
    UNIT_ALLOC(scratch, d_i1, int, NV);
    UNIT_ALLOC(scratch, d_head, int, NV);
    UNIT_ALLOC(scratch, d_rank, int, NV);
    UNIT_ALLOC(scratch, d_start, int, NV + 1);
    UNIT_ALLOC(scratch, d_cluster, int, NV);
    // the triangles' sort: keys by triangle, two key buffers, two index buffers
    u64 *d_klm = nullptr, *d_ta = nullptr, *d_tb = nullptr;
    int *d_hi = nullptr, *d_t0 = nullptr, *d_t1 = nullptr, *d_tkeep, *d_toff;
    if (nt > 0) {
        UNIT_ALLOC(scratch, d_klm, u64, NT);
        UNIT_ALLOC(scratch, d_ta, u64, NT);
        UNIT_ALLOC(scratch, d_tb, u64, NT);
        UNIT_ALLOC(scratch, d_hi, int, NT);
        UNIT_ALLOC(scratch, d_t0, int, NT);
        UNIT_ALLOC(scratch, d_t1, int, NT);
    }
    UNIT_ALLOC(scratch, d_tkeep, int, NT + 1);                    // zeroed: the last flag stays 0, so the sums end in the totals
    UNIT_ALLOC(scratch, d_toff, int, NT + 1);
    int *d_used, *d_coff;
    UNIT_ALLOC(scratch, d_used, int, NV + 1);                     // zeroed; n_runs + 1 of it are used
    UNIT_ALLOC(scratch, d_coff, int, NV + 1);

    const int vertex_bits = 63;                                   // three fields of 21 bits
    size_t sort_v = 0, sort_t = 0, scan_a = 0, scan_t = 0, scan_v = 0;
    if (int rc = sort_pairs_u64(s, nullptr, &sort_v, d_k0, d_k1, d_i0, d_i1, (unsigned)nv, vertex_bits)) return rc;
    if (nt > 0)
        if (int rc = sort_pairs_u64(s, nullptr, &sort_t, d_ta, d_tb, d_t0, d_t1, (unsigned)nt, 63)) return rc;
    UNIT_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_a, d_head, d_rank, (unsigned)nv, s));
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_t, d_tkeep, d_toff, (unsigned)(NT + 1), s));
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_v, d_used, d_coff, (unsigned)(NV + 1), s));
    const size_t tmp_bytes = std::max(std::max(std::max(sort_v, sort_t), std::max(scan_a, scan_t)), std::max(scan_v, (size_t)1));
    void* d_tmp = scratch.alloc(tmp_bytes);
    if (!d_tmp) return (int)hipErrorOutOfMemory;

    tm.begin(DEC_T_UPLOAD);
    DEC_COPY(d_tri, m.tri, sizeof(int) * NT * 3, hipMemcpyHostToDevice);
    DEC_COPY(d_xyz, m.xyz, sizeof(float) * NV * 3, hipMemcpyHostToDevice);
    if (d_bgr) DEC_COPY(d_bgr, m.bgr, NV * 3, hipMemcpyHostToDevice);
    tm.end();

    tm.begin(DEC_T_KEYS);
    DEC_LAUNCH(nt, k_dec_check, nt, nv, d_tri, d_flags);
    DEC_LAUNCH(nv, k_dec_keys, nv, d_xyz, qd, prm.cell, d_P, d_k0, d_i0, d_flags);
    tm.end();
    tm.begin(DEC_T_SORT);
    {
        size_t bytes = tmp_bytes;
        if (int rc = sort_pairs_u64(s, d_tmp, &bytes, d_k0, d_k1, d_i0, d_i1, (unsigned)nv, vertex_bits)) return rc;
    }
    tm.end();
    const u64* ks = d_k1;
    const int* is = d_i1;
    tm.begin(DEC_T_RUNS);
    DEC_LAUNCH(nv, k_dec_heads, nv, ks, d_head);
    {
        size_t bytes = tmp_bytes;
        UNIT_TRY(hipcub::DeviceScan::InclusiveSum(d_tmp, bytes, d_head, d_rank, (unsigned)nv, s));
    }
    DEC_LAUNCH(nv, k_dec_starts, nv, d_head, d_rank, is, d_start, d_cluster, d_info);
    int flags[2] = { 0, 0 }, n_runs = 0;
    UNIT_TRY(hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(&n_runs, d_info, sizeof(int), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    tm.end();
    if (flags[0]) return CLEAN_ERR_INDEX;
    if (flags[1]) return CLEAN_ERR_COORD;
    if (n_runs < 1 || n_runs > nv) return (int)hipErrorUnknown;  // (cannot happen: nv >= 1 vertices, every one in a run)

    // from here on every index is vouched for: tri in 0 .. nv-1, cluster_of in 0 .. n_runs-1
    const size_t R = (size_t)n_runs;
    MemberSums sums;
    sums.stride = n_runs;
    UNIT_ALLOC(scratch, sums.sum, long long, R * 6);
    u64* d_Q;
    UNIT_ALLOC(scratch, d_Q, u64, R * 10);                        // zeroed
    float* d_cxyz;
    unsigned char* d_cbgr = nullptr;
    UNIT_ALLOC(scratch, d_cxyz, float, R * 3);
    if (d_bgr) UNIT_ALLOC(scratch, d_cbgr, unsigned char, R * 3);
    const int long_cap = nv / (DEC_SHORT_RUN + 1) + 1;
    int* d_long;
    UNIT_ALLOC(scratch, d_long, int, (size_t)long_cap);
    const MemberIn in{ d_P, d_bgr, prm.cell };

    tm.begin(DEC_T_MEMBERS);
    DEC_LAUNCH(n_runs, k_dec_members_short, n_runs, d_start, is, in, sums, d_long, long_cap, d_info + 1);
    if (nv > DEC_SHORT_RUN) {
        const unsigned grid = (unsigned)std::min<long long>(LONG_BLOCKS, ((long long)long_cap + LANES / WAVE - 1) / (LANES / WAVE));
        hipLaunchKernelGGL(k_dec_members_long, dim3(grid), dim3(LANES), 0, s, d_start, is, in, sums, d_long, long_cap, d_info + 1);
        UNIT_TRY(hipGetLastError());
    }
    tm.end();
    if (prm.placement == 1) {
        tm.begin(DEC_T_QUADRICS);
        DEC_LAUNCH(nt, k_dec_quadrics, nt, d_tri, d_P, d_cluster, prm.cell, d_Q);
        tm.end();
    }
    tm.begin(DEC_T_SOLVE);
    DEC_LAUNCH(n_runs, k_dec_solve, n_runs, d_start, ks, sums, d_Q, qd, prm.cell, prm.placement, prm.reg, d_bgr ? 1 : 0, d_cxyz, d_cbgr, d_stats);
    tm.end();

    if (nt > 0) {
        const int B = bits_for((u64)n_runs);                      // a rank is below 2^B <= 2^31
        tm.begin(DEC_T_MAP);
        DEC_LAUNCH(nt, k_dec_map, nt, d_tri, d_cluster, B, d_ta, d_klm, d_hi, d_t0, d_stats);
        tm.end();
        tm.begin(DEC_T_DEDUP);
        size_t bytes = tmp_bytes;
        if (int rc = sort_pairs_u64(s, d_tmp, &bytes, d_ta, d_tb, d_t0, d_t1, (unsigned)nt, B)) return rc;
        DEC_LAUNCH(nt, k_dec_gather, nt, d_t1, d_klm, d_ta);
        bytes = tmp_bytes;
        if (int rc = sort_pairs_u64(s, d_tmp, &bytes, d_ta, d_tb, d_t1, d_t0, (unsigned)nt, 2 * B + 1)) return rc;
        DEC_LAUNCH(nt, k_dec_dups, nt, B, d_tb, d_t0, d_hi, d_tkeep, d_stats);
        tm.end();
    }
    tm.begin(DEC_T_COMPACT);
    DEC_LAUNCH(nt, k_dec_used, nt, d_tri, d_cluster, d_tkeep, d_used);
    {
        size_t bytes = tmp_bytes;
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, bytes, d_tkeep, d_toff, (unsigned)(NT + 1), s));
        bytes = tmp_bytes;
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, bytes, d_used, d_coff, (unsigned)(R + 1), s));
    }
    int nt_out = 0, nv_out = 0;
    u64 stats[4] = { 0, 0, 0, 0 };
    UNIT_TRY(hipMemcpyAsync(&nt_out, d_toff + NT, sizeof(int), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(&nv_out, d_coff + R, sizeof(int), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(stats, d_stats, sizeof(stats), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    tm.end();
    *out.n_vertices = nv_out;
    *out.n_triangles = nt_out;
    if (nv_out > out.vcap || nt_out > out.tcap) {
        if (timing) tm.collect(timing);
        return UNIT_ERR_CAPACITY;
    }

    float* d_oxyz;
    unsigned char* d_obgr = nullptr;
    int *d_otri, *d_otof, *d_omem, *d_vof;
    UNIT_ALLOC(scratch, d_oxyz, float, (size_t)nv_out * 3);
    if (d_bgr) UNIT_ALLOC(scratch, d_obgr, unsigned char, (size_t)nv_out * 3);
    UNIT_ALLOC(scratch, d_omem, int, (size_t)nv_out);
    UNIT_ALLOC(scratch, d_otri, int, (size_t)nt_out * 3);
    UNIT_ALLOC(scratch, d_otof, int, (size_t)nt_out);
    UNIT_ALLOC(scratch, d_vof, int, NV);
    tm.begin(DEC_T_EMIT);
    DEC_LAUNCH(nt, k_dec_emit_tri, nt, d_tri, d_cluster, d_tkeep, d_toff, d_coff, d_otri, d_otof);
    DEC_LAUNCH(n_runs, k_dec_emit_vtx, n_runs, d_start, d_used, d_coff, d_cxyz, d_cbgr, d_oxyz, d_obgr, d_omem);
    if (out.vertex_of) DEC_LAUNCH(nv, k_dec_vertex_of, nv, d_cluster, d_used, d_coff, d_vof);
    tm.end();
    tm.begin(DEC_T_DOWNLOAD);
    DEC_COPY(out.xyz, d_oxyz, sizeof(float) * (size_t)nv_out * 3, hipMemcpyDeviceToHost);
    if (d_obgr && out.bgr) DEC_COPY(out.bgr, d_obgr, (size_t)nv_out * 3, hipMemcpyDeviceToHost);
    if (out.members) DEC_COPY(out.members, d_omem, sizeof(int) * (size_t)nv_out, hipMemcpyDeviceToHost);
    DEC_COPY(out.tri, d_otri, sizeof(int) * (size_t)nt_out * 3, hipMemcpyDeviceToHost);
    if (out.triangle_of) DEC_COPY(out.triangle_of, d_otof, sizeof(int) * (size_t)nt_out, hipMemcpyDeviceToHost);
    if (out.vertex_of) DEC_COPY(out.vertex_of, d_vof, sizeof(int) * NV, hipMemcpyDeviceToHost);
    tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    if (out.stats) {
        out.stats[0] = n_runs;
        for (int i = 1; i < 4; ++i) out.stats[i] = (int64_t)stats[i];
    }
    if (timing) tm.collect(timing);
    return 0;
}

}  // namespace sfmba
