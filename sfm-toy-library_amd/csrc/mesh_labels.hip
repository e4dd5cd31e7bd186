// mesh_labels.hip -- smoothing the view labels of a textured mesh on the MI355X (gfx950, wave64).
//
// The contract is the project's own (include/sfmba.h, "smoothing the view labels"; the rules are in label_math.h): past the candidate
// kernel everything is INTEGER arithmetic, and the only atomics are integer adds on the statistics counters, whose result does not depend
// on the order -- so the result is BIT-EXACT with a CPU restatement (tests/label_oracle.py) however the work is cut.
//
//   candidates    k_lab_candidates: a lane per triangle, looping over the views in ascending index as k_tex_views does, keeping the K
//                 best in an insertion-sorted list in registers (label_insert).  Rows [T][K] of int32 and of int64.
//   adjacency     k_lab_keys: a lane per triangle writes its three (edge key, 3 t + q) pairs; one stable sort_pairs_u64; k_lab_link: a
//                 lane per sorted entry looks at the two entries on either side (label_link, label_run_head).
//   rings         k_lab_ring: THE FIRST HOT KERNEL.  A lane per triangle reads its own row and gathers the rows of its three neighbours:
//                 K = 4 is 16 + 32 bytes a neighbour, contiguous, so a neighbour costs a few wide loads; a Jacobi update between two
//                 buffers.  The mesh comes out of marching tetrahedra in grid order, so most neighbours sit in lines the same or a
//                 nearby wave has fetched: the gathers are served by L2.
//   start         k_lab_start: the rank of the largest diffused sum, the label, and D as uint16 [T][K], so that no pass divides.
//   a pass        k_lab_gain: THE SECOND HOT KERNEL: own row of views and D (24 bytes at K = 4), three neighbour labels (4 bytes each) ->
//                 gain and k*.  k_lab_move: a lane whose gain is positive reads its neighbours' gains and moves if it beats them all.
//                 Gains all come from the labels before the pass; movers are pairwise non-adjacent, so the labels need no second buffer.
//                 The mover counts come back to the host in batches of LABEL_BATCH passes: a pass after one that moved nothing moves
//                 nothing, so the batching changes no output.
//   statistics    k_lab_stats: per triangle its data term and its links to higher-numbered triangles; LDS adds per workgroup, then one
//                 global add per workgroup and counter.
//
// A row lives in LABEL_MAX_K registers whatever K is: K is a run-time value and no kernel is instantiated per K.  256 lanes a
// workgroup, no LDS beyond the counters and few registers: occupancy is the launch bound's, which is what hides the gathers.
//
// SCRATCH of the smoothing for T triangles: (4 + 8) T K for the lists, 12 T adjacency, 16 T K for the two diffusion buffers, 2 T K for
// D, 20 T for rank, label, first label, gain and k*; the adjacency build adds 2 (8 + 4) 3 T and the sort's temporaries.
#include "mesh_labels.h"
#include "ba_kernels.h"    // sort_pairs_u64

#include <algorithm>
#include <cstring>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;
constexpr int LABEL_BATCH = 8;        // passes between two looks at the mover counts
using u64 = unsigned long long;

unsigned blocks_for(long long n) { return (unsigned)((n + LANES - 1) / LANES); }

__device__ __forceinline__ void load_row_i(const int* __restrict__ p, long long t, int K, int* out) {
    for (int k = 0; k < LABEL_MAX_K; ++k) out[k] = k < K ? p[(size_t)t * K + k] : -1;
}
__device__ __forceinline__ void load_row_l(const long long* __restrict__ p, long long t, int K, long long* out) {
    for (int k = 0; k < LABEL_MAX_K; ++k) out[k] = k < K ? p[(size_t)t * K + k] : 0;
}

__global__ __launch_bounds__(LANES) void k_lab_candidates(TexKernelParams prm, const int* __restrict__ flag, const float* __restrict__ xyz,
                                                          const int* __restrict__ tri, const TexImage* __restrict__ tab,
                                                          const float* __restrict__ maps, const unsigned char* __restrict__ raw, int K,
                                                          int* __restrict__ cand_view, long long* __restrict__ cand_score) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    if (t >= prm.nt || flag[0]) return;
    const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
    double A[3], Bv[3], C[3];
    load_vertex(xyz, a, A);
    load_vertex(xyz, b, Bv);
    load_vertex(xyz, c, C);
    int cv[LABEL_MAX_K];
    long long cs[LABEL_MAX_K];
    label_clear(cv, cs);
    if (a != b && a != c && b != c && tex_finite3(A) && tex_finite3(Bv) && tex_finite3(C)) {
        for (int i = 0; i < prm.n_images; ++i) {
            const TexView V = view_of(tab[i], maps, raw);
            long long a2;
            const bool cand = tex_candidate(prm.k4, V, A, Bv, C, prm.occl_tol, a2);
            if (tex_eligible(cand, a2, prm.min_area)) label_insert(K, cv, cs, i, -a2);
        }
    }
    for (int k = 0; k < LABEL_MAX_K; ++k)
        if (k < K) { cand_view[(size_t)t * K + k] = cv[k]; cand_score[(size_t)t * K + k] = cs[k]; }
}

__global__ __launch_bounds__(LANES) void k_lab_keys(int nt, const int* __restrict__ tri, u64* __restrict__ keys, int* __restrict__ vals) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    if (t >= nt) return;
    const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
    for (int q = 0; q < 3; ++q) {
        keys[3 * (size_t)t + q] = label_edge_key(a, b, c, q);
        vals[3 * (size_t)t + q] = (int)(3 * t + q);
    }
}

// adds this lane's three numbers to counts[0..2]: LDS adds, then one global add per workgroup and counter.  EVERY lane of the
// workgroup must call it.
__device__ __forceinline__ void block_add3(u64 a, u64 b, u64 c, u64* __restrict__ counts) {
    __shared__ u64 s_acc[3];
    if (threadIdx.x < 3) s_acc[threadIdx.x] = 0;
    __syncthreads();
    if (a) atomicAdd(&s_acc[0], a);
    if (b) atomicAdd(&s_acc[1], b);
    if (c) atomicAdd(&s_acc[2], c);
    __syncthreads();
    if (threadIdx.x < 3 && s_acc[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_acc[threadIdx.x]);
}

__global__ __launch_bounds__(LANES) void k_lab_link(long long n, const u64* __restrict__ keys, const int* __restrict__ vals, int* __restrict__ adj,
                                                    u64* __restrict__ counts) {
    const long long i = (long long)blockIdx.x * LANES + threadIdx.x;
    int head = 0;
    if (i < n) {
        adj[vals[i]] = label_link(keys, vals, n, i);
        head = label_run_head(keys, n, i);
    }
    block_add3(head == 2, head == 1, head == 3, counts);
}

__global__ __launch_bounds__(LANES) void k_lab_ring(int nt, int K, const int* __restrict__ cand_view, const long long* __restrict__ s_in,
                                                    const int* __restrict__ adj, long long* __restrict__ s_out) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    if (t >= nt) return;
    int cv[LABEL_MAX_K];
    long long s[LABEL_MAX_K];
    load_row_i(cand_view, t, K, cv);
    load_row_l(s_in, t, K, s);
    for (int q = 0; q < 3; ++q) {
        const int n = adj[3 * (size_t)t + q];
        if (n < 0) continue;
        int nv[LABEL_MAX_K];
        long long ns[LABEL_MAX_K];
        load_row_i(cand_view, n, K, nv);
        load_row_l(s_in, n, K, ns);
        for (int k = 0; k < LABEL_MAX_K; ++k)
            if (k < K && cv[k] >= 0) s[k] += label_look(K, nv, ns, cv[k]);
    }
    for (int k = 0; k < LABEL_MAX_K; ++k)
        if (k < K) s_out[(size_t)t * K + k] = cv[k] >= 0 ? s[k] : 0;
}

__global__ __launch_bounds__(LANES) void k_lab_start(int nt, int K, const int* __restrict__ cand_view, const long long* __restrict__ cand_score,
                                                     const long long* __restrict__ s_final, int* __restrict__ rank, int* __restrict__ view,
                                                     int* __restrict__ view0, unsigned short* __restrict__ D) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    if (t >= nt) return;
    int cv[LABEL_MAX_K];
    long long s0[LABEL_MAX_K], s[LABEL_MAX_K];
    load_row_i(cand_view, t, K, cv);
    load_row_l(cand_score, t, K, s0);
    load_row_l(s_final, t, K, s);
    int r = label_start_rank(K, cv, s);
    int v = -1;
    for (int k = 0; k < LABEL_MAX_K; ++k) {
        if (k < K) {
            D[(size_t)t * K + k] = (unsigned short)((cv[0] >= 0 && cv[k] >= 0) ? label_D(s0[0], s0[k]) : 0);
            if (k == r) v = cv[k];
        }
    }
    rank[t] = r;
    view[t] = v;
    view0[t] = cv[0];
}

// out[0] += sum of D[t][rank[t]] (rank == NULL: nothing) + penalty * differing pairs; out[1] += differing pairs; out[2] += pairs with
// exactly one side -1.  A pair is an adj entry n of t with t < n.
__global__ __launch_bounds__(LANES) void k_lab_stats(int nt, int K, const unsigned short* __restrict__ D, const int* __restrict__ rank,
                                                     const int* __restrict__ view, const int* __restrict__ adj, int penalty, u64* __restrict__ out) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    u64 e = 0, diff = 0, frontier = 0;
    if (t < nt) {
        const int vt = view[t];
        if (rank && rank[t] >= 0) e = D[(size_t)t * K + rank[t]];
        for (int q = 0; q < 3; ++q) {
            const int n = adj[3 * (size_t)t + q];
            if (n <= t) continue;
            const int vn = view[n];
            if (vt >= 0 && vn >= 0) diff += vt != vn;
            else frontier += (vt >= 0) != (vn >= 0);
        }
        e += (u64)penalty * diff;
    }
    block_add3(e, diff, frontier, out);
}

__global__ __launch_bounds__(LANES) void k_lab_gain(int nt, int K, const int* __restrict__ cand_view, const unsigned short* __restrict__ D,
                                                    const int* __restrict__ rank, const int* __restrict__ view, const int* __restrict__ adj,
                                                    int penalty, int* __restrict__ gain, int* __restrict__ kstar) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    if (t >= nt) return;
    const int r = rank[t];
    int g = 0, ks = r;
    if (r >= 0) {
        int cv[LABEL_MAX_K], d[LABEL_MAX_K], nview[3];
        load_row_i(cand_view, t, K, cv);
        for (int k = 0; k < LABEL_MAX_K; ++k) d[k] = k < K ? (int)D[(size_t)t * K + k] : 0;
        for (int q = 0; q < 3; ++q) {
            const int n = adj[3 * (size_t)t + q];
            nview[q] = n >= 0 ? view[n] : -1;
        }
        g = label_gain(K, cv, d, penalty, nview, r, ks);
    }
    gain[t] = g;
    kstar[t] = ks;
}

__global__ __launch_bounds__(LANES) void k_lab_move(int nt, int K, const int* __restrict__ cand_view, const int* __restrict__ adj,
                                                    const int* __restrict__ gain, const int* __restrict__ kstar, int* __restrict__ rank,
                                                    int* __restrict__ view, unsigned* __restrict__ moved) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    if (t >= nt) return;
    const int g = gain[t];
    if (g <= 0) return;
    int n[3], gn[3];
    for (int q = 0; q < 3; ++q) {
        n[q] = adj[3 * (size_t)t + q];
        gn[q] = n[q] >= 0 ? gain[n[q]] : 0;
    }
    if (!label_moves((int)t, g, n, gn)) return;
    const int ks = kstar[t];
    rank[t] = ks;
    view[t] = cand_view[(size_t)t * K + ks];
    atomicAdd(moved, 1u);                    // (the compiler adds once per wave)
}

__global__ __launch_bounds__(LANES) void k_lab_score(int nt, int K, const long long* __restrict__ cand_score, const int* __restrict__ rank,
                                                     long long* __restrict__ score) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    if (t >= nt) return;
    const int r = rank[t];
    score[t] = r >= 0 ? cand_score[(size_t)t * K + r] : 0;
}

#define LAB_COPY(dst, src, bytes, kind) do { if ((bytes) > 0) UNIT_TRY(hipMemcpyAsync(dst, src, bytes, kind, s)); } while (0)
#define LAB_BEGIN(p) do { if (tm) tm->begin(p); } while (0)
#define LAB_END() do { if (tm) tm->end(); } while (0)

}  // namespace

int labels_candidates_dev(hipStream_t s, const TexKernelParams& prm, const int* d_flag, const float* d_xyz, const int* d_tri, const TexImage* d_tab,
                          const float* d_maps, const unsigned char* d_raw, int K, int* d_cand_view, long long* d_cand_score) {
    if (prm.nt <= 0) return 0;
    hipLaunchKernelGGL(k_lab_candidates, dim3(blocks_for(prm.nt)), dim3(LANES), 0, s, prm, d_flag, d_xyz, d_tri, d_tab, d_maps, d_raw, K, d_cand_view,
                       d_cand_score);
    UNIT_TRY(hipGetLastError());
    return 0;
}

int labels_adjacency_dev(hipStream_t s, DeviceArena& raw, int nt, const int* d_tri, int* d_adj, u64* d_counts, PhaseTimer* tm) {
    if (nt <= 0) return 0;
    const size_t N = 3 * (size_t)nt;
    u64 *d_k0, *d_k1;
    int *d_v0, *d_v1;
    UNIT_ALLOC(raw, d_k0, u64, N);
    UNIT_ALLOC(raw, d_k1, u64, N);
    UNIT_ALLOC(raw, d_v0, int, N);
    UNIT_ALLOC(raw, d_v1, int, N);
    size_t sort_bytes = 0;
    const int end_bit = 64;                  // LABEL_NO_EDGE has every bit set
    if (int rc = sort_pairs_u64(s, nullptr, &sort_bytes, d_k0, d_k1, d_v0, d_v1, (unsigned)N, end_bit)) return rc;
    void* d_tmp = raw.alloc(std::max(sort_bytes, (size_t)1));
    if (!d_tmp) return (int)hipErrorOutOfMemory;
    LAB_BEGIN(LAB_T_KEYS);
    hipLaunchKernelGGL(k_lab_keys, dim3(blocks_for(nt)), dim3(LANES), 0, s, nt, d_tri, d_k0, d_v0);
    UNIT_TRY(hipGetLastError());
    LAB_END();
    LAB_BEGIN(LAB_T_SORT);
    if (int rc = sort_pairs_u64(s, d_tmp, &sort_bytes, d_k0, d_k1, d_v0, d_v1, (unsigned)N, end_bit)) return rc;
    LAB_END();
    LAB_BEGIN(LAB_T_LINK);
    hipLaunchKernelGGL(k_lab_link, dim3(blocks_for((long long)N)), dim3(LANES), 0, s, (long long)N, d_k1, d_v1, d_adj, d_counts);
    UNIT_TRY(hipGetLastError());
    LAB_END();
    return 0;
}

int labels_smooth_dev(hipStream_t s, DeviceArena& scratch, DeviceArena& raw, int nt, const LabelParams& p, const int* d_cand_view, const long long* d_cand_score,
                      const int* d_adj, int* d_view, long long* d_score, int64_t* stats, PhaseTimer* tm) {
    for (int i = 0; i < LABEL_STATS; ++i) stats[i] = 0;
    if (nt <= 0) return 0;
    const int K = p.K;
    const size_t NT = (size_t)nt, NK = NT * (size_t)K;
    long long *d_sa = nullptr, *d_sb = nullptr;
    unsigned short* d_D;
    int *d_rank, *d_view0, *d_gain, *d_kstar;
    u64* d_st;
    unsigned* d_moved;
    if (p.rings > 0) {
        UNIT_ALLOC(raw, d_sa, long long, NK);
        UNIT_ALLOC(raw, d_sb, long long, NK);
    }
    UNIT_ALLOC(raw, d_D, unsigned short, NK);
    UNIT_ALLOC(raw, d_rank, int, NT);
    UNIT_ALLOC(raw, d_view0, int, NT);
    UNIT_ALLOC(raw, d_gain, int, NT);
    UNIT_ALLOC(raw, d_kstar, int, NT);
    UNIT_ALLOC(scratch, d_st, u64, 9);                                       // zeroed: three instants of three sums
    UNIT_ALLOC(scratch, d_moved, unsigned, (size_t)p.max_passes + 1);        // zeroed: a counter per pass
    const dim3 grid(blocks_for(nt)), block(LANES);

    LAB_BEGIN(LAB_T_RINGS);
    const long long* cur = d_cand_score;
    for (int r = 0; r < p.rings; ++r) {
        long long* nxt = (r & 1) ? d_sb : d_sa;
        hipLaunchKernelGGL(k_lab_ring, grid, block, 0, s, nt, K, d_cand_view, cur, d_adj, nxt);
        UNIT_TRY(hipGetLastError());
        cur = nxt;
    }
    LAB_END();
    LAB_BEGIN(LAB_T_START);
    hipLaunchKernelGGL(k_lab_start, grid, block, 0, s, nt, K, d_cand_view, d_cand_score, cur, d_rank, d_view, d_view0, d_D);
    UNIT_TRY(hipGetLastError());
    LAB_END();
    LAB_BEGIN(LAB_T_STATS);
    hipLaunchKernelGGL(k_lab_stats, grid, block, 0, s, nt, K, d_D, (const int*)nullptr, d_view0, d_adj, p.penalty, d_st);
    UNIT_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_lab_stats, grid, block, 0, s, nt, K, d_D, d_rank, d_view, d_adj, p.penalty, d_st + 3);
    UNIT_TRY(hipGetLastError());
    LAB_END();

    std::vector<unsigned> moved(LABEL_BATCH);
    int64_t moves = 0, n_passes = 0;
    bool still = false;
    for (int done = 0; done < p.max_passes && !still;) {
        const int b = std::min(LABEL_BATCH, p.max_passes - done);
        for (int i = 0; i < b; ++i) {
            LAB_BEGIN(LAB_T_GAIN);
            hipLaunchKernelGGL(k_lab_gain, grid, block, 0, s, nt, K, d_cand_view, d_D, d_rank, d_view, d_adj, p.penalty, d_gain, d_kstar);
            UNIT_TRY(hipGetLastError());
            LAB_END();
            LAB_BEGIN(LAB_T_MOVE);
            hipLaunchKernelGGL(k_lab_move, grid, block, 0, s, nt, K, d_cand_view, d_adj, d_gain, d_kstar, d_rank, d_view, d_moved + done + i);
            UNIT_TRY(hipGetLastError());
            LAB_END();
        }
        UNIT_TRY(hipMemcpyAsync(moved.data(), d_moved + done, sizeof(unsigned) * (size_t)b, hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipStreamSynchronize(s));
        for (int i = 0; i < b && !still; ++i) {
            if (moved[(size_t)i] == 0) still = true;
            else { moves += moved[(size_t)i]; ++n_passes; }
        }
        done += b;
    }

    LAB_BEGIN(LAB_T_STATS);
    hipLaunchKernelGGL(k_lab_stats, grid, block, 0, s, nt, K, d_D, d_rank, d_view, d_adj, p.penalty, d_st + 6);
    UNIT_TRY(hipGetLastError());
    if (d_score) {
        hipLaunchKernelGGL(k_lab_score, grid, block, 0, s, nt, K, d_cand_score, d_rank, d_score);
        UNIT_TRY(hipGetLastError());
    }
    LAB_END();
    u64 st[9];
    UNIT_TRY(hipMemcpyAsync(st, d_st, sizeof(st), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    stats[LABEL_S_E_START] = (int64_t)st[3];
    stats[LABEL_S_E_END] = (int64_t)st[6];
    stats[LABEL_S_DIFF_RANK0] = (int64_t)st[1];
    stats[LABEL_S_DIFF_START] = (int64_t)st[4];
    stats[LABEL_S_DIFF_END] = (int64_t)st[7];
    stats[LABEL_S_FRONTIER] = (int64_t)st[2];
    stats[LABEL_S_MOVES] = moves;
    stats[LABEL_S_PASSES] = n_passes;
    return 0;
}

// ---- the three calls on host arrays ---------------------------------------------------------------------------------------------
int mesh_view_candidates(hipStream_t s, int device, const TexMesh& m, const TexViews& v, float occl_tol, int64_t min_area, int K, int32_t* cand_view,
                         int64_t* cand_score, double* timing) {
    if (timing) for (int i = 0; i < LAB_T_COUNT; ++i) timing[i] = 0.0;
    DeviceArena scratch(device);
    PhaseTimer timer{ s, timing != nullptr, {}, {} };
    PhaseTimer* tm = &timer;
    const size_t NV = (size_t)m.nv, NT = (size_t)m.nt;
    std::vector<TexImage> tab;
    long long n_map = 0, n_raw = 0;
    tex_view_table(v, tab, n_map, n_raw);
    int *d_flag, *d_tri, *d_cv;
    float *d_xyz, *d_maps;
    long long* d_cs;
    TexImage* d_tab;
    unsigned char* d_raw;
    UNIT_ALLOC(scratch, d_flag, int, 2);                         // zeroed
    UNIT_ALLOC(scratch, d_tri, int, NT * 3);
    UNIT_ALLOC(scratch, d_xyz, float, NV * 3);
    UNIT_ALLOC(scratch, d_tab, TexImage, tab.size());
    UNIT_ALLOC(scratch, d_maps, float, (size_t)n_map);
    UNIT_ALLOC(scratch, d_raw, unsigned char, 1);                // the view choice reads no pixel
    UNIT_ALLOC(scratch, d_cv, int, NT * (size_t)K);
    UNIT_ALLOC(scratch, d_cs, long long, NT * (size_t)K);
    LAB_BEGIN(LAB_T_UPLOAD);
    LAB_COPY(d_tri, m.tri, sizeof(int) * NT * 3, hipMemcpyHostToDevice);
    LAB_COPY(d_xyz, m.xyz, sizeof(float) * NV * 3, hipMemcpyHostToDevice);
    LAB_COPY(d_tab, tab.data(), sizeof(TexImage) * tab.size(), hipMemcpyHostToDevice);
    for (int i = 0; i < v.n_images; ++i) {
        const TexImage& T = tab[(size_t)i];
        if (v.depth[i]) LAB_COPY(d_maps + T.map_off, v.depth[i], sizeof(float) * (size_t)T.w * T.h, hipMemcpyHostToDevice);
    }
    LAB_END();
    TexKernelParams prm;
    std::memset(&prm, 0, sizeof(prm));
    tex_camera_params(v, occl_tol, min_area, prm);
    prm.nv = m.nv; prm.nt = m.nt;
    LAB_BEGIN(LAB_T_CANDIDATES);
    if (int rc = tex_check_indices(s, m.nt, m.nv, d_tri, d_flag)) return rc;
    if (int rc = labels_candidates_dev(s, prm, d_flag, d_xyz, d_tri, d_tab, d_maps, d_raw, K, d_cv, d_cs)) return rc;
    LAB_END();
    int flag = 0;
    UNIT_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));                           // also: `tab` is spent
    if (flag) return TEX_ERR_INDEX;
    LAB_BEGIN(LAB_T_DOWNLOAD);
    LAB_COPY(cand_view, d_cv, sizeof(int) * NT * (size_t)K, hipMemcpyDeviceToHost);
    LAB_COPY(cand_score, d_cs, sizeof(long long) * NT * (size_t)K, hipMemcpyDeviceToHost);
    LAB_END();
    UNIT_TRY(hipStreamSynchronize(s));
    if (timing) timer.collect(timing);
    return 0;
}

int mesh_adjacency(hipStream_t s, int device, int nt, const int32_t* tri, int32_t* adj, int64_t* counts, double* timing) {
    if (timing) for (int i = 0; i < LAB_T_COUNT; ++i) timing[i] = 0.0;
    DeviceArena scratch(device);
    DeviceArena raw(device);                                     // the temporaries: written in full before they are read
    raw.set_zeroing(false);
    PhaseTimer timer{ s, timing != nullptr, {}, {} };
    PhaseTimer* tm = &timer;
    const size_t NT = (size_t)nt;
    int *d_tri, *d_adj;
    u64* d_counts;
    UNIT_ALLOC(scratch, d_tri, int, NT * 3);
    UNIT_ALLOC(scratch, d_adj, int, NT * 3);
    UNIT_ALLOC(scratch, d_counts, u64, 3);                       // zeroed
    LAB_BEGIN(LAB_T_UPLOAD);
    LAB_COPY(d_tri, tri, sizeof(int) * NT * 3, hipMemcpyHostToDevice);
    LAB_END();
    if (int rc = labels_adjacency_dev(s, raw, nt, d_tri, d_adj, d_counts, tm)) return rc;
    u64 c[3];
    LAB_BEGIN(LAB_T_DOWNLOAD);
    LAB_COPY(adj, d_adj, sizeof(int) * NT * 3, hipMemcpyDeviceToHost);
    UNIT_TRY(hipMemcpyAsync(c, d_counts, sizeof(c), hipMemcpyDeviceToHost, s));
    LAB_END();
    UNIT_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < 3; ++i) counts[i] = (int64_t)c[i];
    if (timing) timer.collect(timing);
    return 0;
}

int mesh_view_smooth(hipStream_t s, int device, int nt, const LabelParams& p, const int32_t* cand_view, const int64_t* cand_score, const int32_t* adj,
                     int32_t* view, int64_t* stats, double* timing) {
    if (timing) for (int i = 0; i < LAB_T_COUNT; ++i) timing[i] = 0.0;
    DeviceArena scratch(device);
    DeviceArena raw(device);                                     // the temporaries: written in full before they are read
    raw.set_zeroing(false);
    PhaseTimer timer{ s, timing != nullptr, {}, {} };
    PhaseTimer* tm = &timer;
    const size_t NT = (size_t)nt, NK = NT * (size_t)p.K;
    int *d_cv, *d_adj, *d_view;
    long long* d_cs;
    UNIT_ALLOC(scratch, d_cv, int, NK);
    UNIT_ALLOC(scratch, d_cs, long long, NK);
    UNIT_ALLOC(scratch, d_adj, int, NT * 3);
    UNIT_ALLOC(scratch, d_view, int, NT);
    LAB_BEGIN(LAB_T_UPLOAD);
    LAB_COPY(d_cv, cand_view, sizeof(int) * NK, hipMemcpyHostToDevice);
    LAB_COPY(d_cs, cand_score, sizeof(long long) * NK, hipMemcpyHostToDevice);
    LAB_COPY(d_adj, adj, sizeof(int) * NT * 3, hipMemcpyHostToDevice);
    LAB_END();
    int64_t st[LABEL_STATS];
    if (int rc = labels_smooth_dev(s, scratch, raw, nt, p, d_cv, d_cs, d_adj, d_view, nullptr, st, tm)) return rc;
    LAB_BEGIN(LAB_T_DOWNLOAD);
    LAB_COPY(view, d_view, sizeof(int) * NT, hipMemcpyDeviceToHost);
    LAB_END();
    UNIT_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < LABEL_STATS; ++i) stats[i] = st[i];
    if (timing) timer.collect(timing);
    return 0;
}

}  // namespace sfmba
