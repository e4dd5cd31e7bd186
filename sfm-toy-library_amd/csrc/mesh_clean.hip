// mesh_clean.hip -- what a mesh needs after its extraction, on the MI355X (gfx950, wave64): connected components, removal of the
// small ones with a stable compaction, Taubin's lambda | mu smoothing and a normal per vertex.
//
// The contract is the project's own (include/sfmba.h, sfmba_mesh_components / sfmba_mesh_filter / sfmba_mesh_smooth /
// sfmba_mesh_clean; arithmetic in mesh_clean_math.h): positions are quantised to integers once, a pass moves them in int64 with one
// floor division per axis, and NOTHING BUT INTEGERS is summed across triangles -- so the result does not depend on the order in
// which atomics arrive or on how the work is cut, and is BIT-EXACT with a CPU restatement.
//
//   check         k_tri_check: a lane per triangle holds its indices to 0 .. nv-1 and raises a device flag.  Every later kernel that
//                 follows an index reads the flag first and does nothing when it is set, so a bad list is never dereferenced and
//                 the host need not wait for the flag before it queues the rest.
//   components    union-find with hooking: parent[v] = v; k_cc_hook, a lane per triangle, unites (a, b) and (a, c): find both roots
//                 (path halving on the way), CAS the HIGHER root under the lower one, retry from the value the CAS returned when
//                 another lane was first.  A link always goes to a lower index, so there is no cycle, a root is its component's
//                 minimum whatever order the hooks land in, and the loop is lock-free (a failed CAS means another lane progressed).
//                 k_cc_flatten walks every vertex to its root (read only).  THREE LAUNCHES, whatever the mesh's diameter; no host
//                 loop on a device flag.  k_cc_count: an integer atomicAdd per triangle on the root of its first index;
//                 k_cc_summary: the number of roots with a triangle (atomicAdd) and the largest one (one 64-bit atomicMax on
//                 count << 32 | ~label: the most triangles, ties to the lower label).
//   filter        k_keep: a lane per triangle -> its keep flag and a 1 on each of its vertices (every lane stores the same 1); two
//                 hipCUB exclusive sums -> the new numbering; k_emit_tri, k_emit_vtx write the survivors in their old order.
//   smooth        k_quantise: a lane per vertex -> P int32 [nv][3] (|P| < 2^25) or the refusal flag.  k_degree: D += 2 per
//                 triangle with distinct indices, once (D does not change between passes).  Per pass: k_pass_scatter, a lane per
//                 triangle, six int64 atomicAdds of P_b + P_c; k_pass_move, a lane per vertex, clean_move, and clears its sums for
//                 the next pass.  The sums are SCATTERED WITH ATOMICS: the gather through a vertex -> triangle list was not built
//                 (profiles/mesh_clean.txt).
//   normals       k_normal_scatter: a lane per triangle, the integer cross product, one fp64 square root, nine int64 atomicAdds of
//                 the unit normal in units of 2^-20; k_normal_final: a lane per vertex.
//
// SCRATCH, for V vertices and T triangles: the mesh 15 V + 12 T, labels and counts 12 V, flags and their sums 8 V + 8 T, the filtered
// mesh 15 V + 12 T, P 12 V, D 4 V, sums 24 V, positions and normals 24 V: at most 114 V + 32 T bytes.
#include "mesh_clean.h"
#include "mesh_clean_math.h"
#include "device_arena.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>

namespace sfmba {

namespace {

constexpr int LANES = 256;
typedef unsigned long long u64;

struct QuantDev { double origin[3], quantum; };

__device__ __forceinline__ long long lane_index() { return (long long)blockIdx.x * LANES + threadIdx.x; }

// flags[0]: a triangle index outside the vertex list; flags[1]: a coordinate that does not quantise
__global__ __launch_bounds__(LANES) void k_tri_check(int nt, int nv, const int* __restrict__ tri, int* __restrict__ flags) {
    const long long t = lane_index();
    if (t >= nt) return;
    bool b = false;
    for (int q = 0; q < 3; ++q) {
        const int v = tri[3 * (size_t)t + q];
        b = b || v < 0 || v >= nv;
    }
    if (b) flags[0] = 1;
}

// ---- components ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void k_cc_init(int nv, int* __restrict__ parent) {
    const long long v = lane_index();
    if (v < nv) parent[v] = (int)v;
}

__device__ __forceinline__ int cc_load(const int* parent, int v) { return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of v.  A value read here may be out of date: it is then an ancestor of v that has stopped being a root, and the CAS of
// cc_union finds that out.  Path halving stores a grandparent, which is an ancestor still.
__device__ __forceinline__ int cc_find(int* parent, int v) {
    for (;;) {
        const int p = cc_load(parent, v);
        if (p == v) return v;
        const int g = cc_load(parent, p);
        if (g == p) return p;
        __hip_atomic_store(parent + v, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = g;
    }
}

__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;                                                 // hi was hooked by another lane meanwhile: go on from its new parent
        b = lo;
    }
}

__global__ __launch_bounds__(LANES) void k_cc_hook(int nt, const int* __restrict__ tri, const int* __restrict__ flags, int* parent) {
    const long long t = lane_index();
    if (t >= nt || flags[0]) return;
    const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
    if (a != b) cc_union(parent, a, b);
    if (a != c) cc_union(parent, a, c);
}

__global__ __launch_bounds__(LANES) void k_cc_flatten(int nv, const int* __restrict__ parent, int* __restrict__ label) {
    const long long lane = lane_index();
    if (lane >= nv) return;
    int v = (int)lane;
    for (int p = parent[v]; p != v; p = parent[v]) v = p;
    label[lane] = v;
}

__global__ __launch_bounds__(LANES) void k_cc_count(int nt, const int* __restrict__ tri, const int* __restrict__ flags, const int* __restrict__ label,
                                                    int* __restrict__ count) {
    const long long t = lane_index();
    if (t >= nt || flags[0]) return;
    atomicAdd(count + label[tri[3 * (size_t)t]], 1);
}

// stats[0]: count << 32 | (2^32 - 1 - label) of the largest component, 0 if there is none; stats[1]: the components with a triangle
__global__ __launch_bounds__(LANES) void k_cc_summary(int nv, const int* __restrict__ label, const int* __restrict__ count, u64* __restrict__ stats) {
    const long long v = lane_index();
    if (v >= nv || label[v] != (int)v || count[v] == 0) return;
    atomicAdd(stats + 1, (u64)1);
    atomicMax(stats, ((u64)(unsigned)count[v] << 32) | (u64)(0xffffffffu - (unsigned)v));
}
__host__ __device__ __forceinline__ long long stats_largest(u64 best) { return best == 0 ? -1ll : (long long)(0xffffffffu - (unsigned)(best & 0xffffffffu)); }

__global__ __launch_bounds__(LANES) void k_cc_comp_triangles(int nv, const int* __restrict__ label, const int* __restrict__ count, int* __restrict__ out) {
    const long long v = lane_index();
    if (v < nv) out[v] = count[label[v]];
}

// ---- filter ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void k_keep(int nt, const int* __restrict__ tri, const int* __restrict__ flags, const int* __restrict__ label,
                                                const int* __restrict__ count, const u64* __restrict__ stats, int min_triangles, int keep_largest,
                                                int* __restrict__ tkeep, int* __restrict__ vkeep) {
    const long long t = lane_index();
    if (t >= nt || flags[0]) return;
    const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
    const int root = label[a];
    const bool keep = count[root] >= min_triangles && (!keep_largest || (long long)root == stats_largest(stats[0]));
    tkeep[t] = keep ? 1 : 0;
    if (keep) vkeep[a] = vkeep[b] = vkeep[c] = 1;
}

__global__ __launch_bounds__(LANES) void k_emit_tri(int nt, const int* __restrict__ tri, const int* __restrict__ flags, const int* __restrict__ tkeep,
                                                    const int* __restrict__ toff, const int* __restrict__ voff, int* __restrict__ tri_out) {
    const long long t = lane_index();
    if (t >= nt || flags[0] || !tkeep[t]) return;
    for (int q = 0; q < 3; ++q) tri_out[3 * (size_t)toff[t] + q] = voff[tri[3 * (size_t)t + q]];
}

__global__ __launch_bounds__(LANES) void k_emit_vtx(int nv, const float* __restrict__ xyz, const unsigned char* __restrict__ bgr,
                                                    const int* __restrict__ vkeep, const int* __restrict__ voff, float* __restrict__ xyz_out,
                                                    unsigned char* __restrict__ bgr_out, int* __restrict__ vertex_of) {
    const long long v = lane_index();
    if (v >= nv) return;
    const bool keep = vkeep[v] != 0;
    vertex_of[v] = keep ? voff[v] : -1;
    if (!keep) return;
    const size_t r = (size_t)voff[v];
    for (int a = 0; a < 3; ++a) xyz_out[3 * r + a] = xyz[3 * (size_t)v + a];
    if (bgr)
        for (int a = 0; a < 3; ++a) bgr_out[3 * r + a] = bgr[3 * (size_t)v + a];
}

// ---- smoothing and normals -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void k_quantise(int nv, const float* __restrict__ xyz, QuantDev q, int* __restrict__ P, int* __restrict__ flags) {
    const long long v = lane_index();
    if (v >= nv) return;
    bool bad = false;
    for (int a = 0; a < 3; ++a) {
        long long p = 0;
        if (!clean_quantise(xyz[3 * (size_t)v + a], q.origin[a], q.quantum, p)) { bad = true; p = 0; }
        P[3 * (size_t)v + a] = (int)p;
    }
    if (bad) flags[1] = 1;
}

__device__ __forceinline__ bool load_distinct(const int* __restrict__ tri, long long t, int& a, int& b, int& c) {
    a = tri[3 * (size_t)t]; b = tri[3 * (size_t)t + 1]; c = tri[3 * (size_t)t + 2];
    return a != b && a != c && b != c;
}
__device__ __forceinline__ void load_p(const int* __restrict__ P, int v, long long* out) {
    for (int a = 0; a < 3; ++a) out[a] = (long long)P[3 * (size_t)v + a];
}
// (two's complement: an unsigned add of the bit pattern is the signed add)
__device__ __forceinline__ void add3(u64* __restrict__ S, int v, const long long* d) {
    for (int a = 0; a < 3; ++a) atomicAdd(S + 3 * (size_t)v + a, (u64)d[a]);
}

__global__ __launch_bounds__(LANES) void k_degree(int nt, const int* __restrict__ tri, const int* __restrict__ flags, unsigned* __restrict__ D) {
    const long long t = lane_index();
    if (t >= nt || flags[0]) return;
    int a, b, c;
    if (!load_distinct(tri, t, a, b, c)) return;
    atomicAdd(D + a, 2u);
    atomicAdd(D + b, 2u);
    atomicAdd(D + c, 2u);
}

__global__ __launch_bounds__(LANES) void k_pass_scatter(int nt, const int* __restrict__ tri, const int* __restrict__ flags, const int* __restrict__ P,
                                                        u64* __restrict__ S) {
    const long long t = lane_index();
    if (t >= nt || flags[0]) return;
    int a, b, c;
    if (!load_distinct(tri, t, a, b, c)) return;
    long long Pa[3], Pb[3], Pc[3], d[3];
    load_p(P, a, Pa); load_p(P, b, Pb); load_p(P, c, Pc);
    for (int x = 0; x < 3; ++x) d[x] = Pb[x] + Pc[x];
    add3(S, a, d);
    for (int x = 0; x < 3; ++x) d[x] = Pa[x] + Pc[x];
    add3(S, b, d);
    for (int x = 0; x < 3; ++x) d[x] = Pa[x] + Pb[x];
    add3(S, c, d);
}

// moves a vertex by its own sums and clears them for the next pass
__global__ __launch_bounds__(LANES) void k_pass_move(int nv, int* __restrict__ P, u64* __restrict__ S, const unsigned* __restrict__ D, int F) {
    const long long v = lane_index();
    if (v >= nv) return;
    long long p[3], sum[3], out[3];
    load_p(P, (int)v, p);
    for (int a = 0; a < 3; ++a) {
        sum[a] = (long long)S[3 * (size_t)v + a];
        S[3 * (size_t)v + a] = 0;
    }
    clean_move(p, sum, (long long)D[v], (long long)F, out);
    for (int a = 0; a < 3; ++a) P[3 * (size_t)v + a] = (int)out[a];
}

__global__ __launch_bounds__(LANES) void k_normal_scatter(int nt, const int* __restrict__ tri, const int* __restrict__ flags, const int* __restrict__ P,
                                                          u64* __restrict__ U) {
    const long long t = lane_index();
    if (t >= nt || flags[0]) return;
    int a, b, c;
    if (!load_distinct(tri, t, a, b, c)) return;
    long long Pa[3], Pb[3], Pc[3], N[3], u[3];
    load_p(P, a, Pa); load_p(P, b, Pb); load_p(P, c, Pc);
    clean_cross(Pa, Pb, Pc, N);
    if (!clean_unit_normal(N, u)) return;
    add3(U, a, u);
    add3(U, b, u);
    add3(U, c, u);
}

__global__ __launch_bounds__(LANES) void k_normal_final(int nv, const u64* __restrict__ U, float* __restrict__ normal) {
    const long long v = lane_index();
    if (v >= nv) return;
    const long long u[3] = { (long long)U[3 * (size_t)v], (long long)U[3 * (size_t)v + 1], (long long)U[3 * (size_t)v + 2] };
    float n[3];
    clean_vertex_normal(u, n);
    for (int a = 0; a < 3; ++a) normal[3 * (size_t)v + a] = n[a];
}

__global__ __launch_bounds__(LANES) void k_positions(int nv, const int* __restrict__ P, QuantDev q, float* __restrict__ xyz_out) {
    const long long v = lane_index();
    if (v >= nv) return;
    for (int a = 0; a < 3; ++a) xyz_out[3 * (size_t)v + a] = clean_position(q.origin[a], (long long)P[3 * (size_t)v + a], q.quantum);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
unsigned blocks_for(long long n) { return (unsigned)((n + LANES - 1) / LANES); }

// a lane per item; nothing is launched for no items
#define CLEAN_LAUNCH(n, kernel, ...)                                                                 \
    do {                                                                                             \
        if ((n) > 0) {                                                                               \
            hipLaunchKernelGGL(kernel, dim3(blocks_for(n)), dim3(LANES), 0, s, __VA_ARGS__);         \
            UNIT_TRY(hipGetLastError());                                                             \
        }                                                                                            \
    } while (0)
#define CLEAN_COPY(dst, src, bytes, kind) do { if ((bytes) > 0) UNIT_TRY(hipMemcpyAsync(dst, src, bytes, kind, s)); } while (0)

// a mesh on the device
struct DevMesh {
    int nv, nt;
    float* xyz;
    unsigned char* bgr;
    int* tri;
};
struct Components { int *label, *count; u64* stats; };

struct Call {
    hipStream_t s;
    DeviceArena scratch;
    PhaseTimer tm;
    int* d_flags = nullptr;
    Call(hipStream_t s_, int device, bool timed) : s(s_), scratch(device), tm{ s_, timed, {}, {} } {}
};

// uploads what the call reads of the mesh and queues the index check
int upload_mesh(Call& c, const CleanMesh& m, bool want_xyz, DevMesh& d) {
    hipStream_t s = c.s;
    d.nv = m.nv; d.nt = m.nt;
    d.xyz = nullptr; d.bgr = nullptr;
    const size_t NV = (size_t)m.nv, NT = (size_t)m.nt;
    UNIT_ALLOC(c.scratch, c.d_flags, int, 2);
    UNIT_ALLOC(c.scratch, d.tri, int, NT * 3);
    if (want_xyz) UNIT_ALLOC(c.scratch, d.xyz, float, NV * 3);
    if (want_xyz && m.bgr) UNIT_ALLOC(c.scratch, d.bgr, unsigned char, NV * 3);
    c.tm.begin(CLEAN_T_UPLOAD);
    CLEAN_COPY(d.tri, m.tri, sizeof(int) * NT * 3, hipMemcpyHostToDevice);
    if (want_xyz) CLEAN_COPY(d.xyz, m.xyz, sizeof(float) * NV * 3, hipMemcpyHostToDevice);
    if (d.bgr) CLEAN_COPY(d.bgr, m.bgr, NV * 3, hipMemcpyHostToDevice);
    c.tm.end();
    c.tm.begin(CLEAN_T_CHECK);
    CLEAN_LAUNCH(m.nt, k_tri_check, m.nt, m.nv, d.tri, c.d_flags);
    c.tm.end();
    return 0;
}

// labels, triangle counts and the summary of a device mesh; queues only
int components_device(Call& c, const DevMesh& d, Components& cc) {
    hipStream_t s = c.s;
    int* d_parent;
    UNIT_ALLOC(c.scratch, d_parent, int, (size_t)d.nv);
    UNIT_ALLOC(c.scratch, cc.label, int, (size_t)d.nv);
    UNIT_ALLOC(c.scratch, cc.count, int, (size_t)d.nv);           // zeroed
    UNIT_ALLOC(c.scratch, cc.stats, u64, 2);                      // zeroed
    c.tm.begin(CLEAN_T_COMPONENTS);
    CLEAN_LAUNCH(d.nv, k_cc_init, d.nv, d_parent);
    CLEAN_LAUNCH(d.nt, k_cc_hook, d.nt, d.tri, c.d_flags, d_parent);
    CLEAN_LAUNCH(d.nv, k_cc_flatten, d.nv, d_parent, cc.label);
    CLEAN_LAUNCH(d.nt, k_cc_count, d.nt, d.tri, c.d_flags, cc.label, cc.count);
    CLEAN_LAUNCH(d.nv, k_cc_summary, d.nv, cc.label, cc.count, cc.stats);
    c.tm.end();
    return 0;
}

// The filtered mesh on the device and vertex_of.  Waits once, for the totals and the index flag; on UNIT_ERR_CAPACITY out.nv
// and out.nt are valid and the rest of `out` is not.
int filter_device(Call& c, const DevMesh& d, const CleanFilterParams& f, int64_t vcap, int64_t tcap, DevMesh& out, int*& d_vertex_of) {
    hipStream_t s = c.s;
    Components cc;
    if (int rc = components_device(c, d, cc)) return rc;
    const size_t NV = (size_t)d.nv, NT = (size_t)d.nt;
    int *d_tkeep, *d_toff, *d_vkeep, *d_voff;
    UNIT_ALLOC(c.scratch, d_tkeep, int, NT + 1);                  // zeroed: the last flag stays 0, so the sums end in the totals
    UNIT_ALLOC(c.scratch, d_toff, int, NT + 1);
    UNIT_ALLOC(c.scratch, d_vkeep, int, NV + 1);
    UNIT_ALLOC(c.scratch, d_voff, int, NV + 1);
    UNIT_ALLOC(c.scratch, d_vertex_of, int, NV);
    size_t scan_t = 0, scan_v = 0;
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_t, d_tkeep, d_toff, (unsigned)(NT + 1), s));
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_v, d_vkeep, d_voff, (unsigned)(NV + 1), s));
    const size_t scan_bytes = std::max(std::max(scan_t, scan_v), (size_t)1);
    void* d_tmp = c.scratch.alloc(scan_bytes);
    if (!d_tmp) return (int)hipErrorOutOfMemory;

    c.tm.begin(CLEAN_T_FILTER);
    CLEAN_LAUNCH(d.nt, k_keep, d.nt, d.tri, c.d_flags, cc.label, cc.count, cc.stats, f.min_triangles, f.keep_largest, d_tkeep, d_vkeep);
    {
        size_t bytes = scan_bytes;
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, bytes, d_tkeep, d_toff, (unsigned)(NT + 1), s));
        bytes = scan_bytes;
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, bytes, d_vkeep, d_voff, (unsigned)(NV + 1), s));
    }
    int flags[2] = { 0, 0 }, nt = 0, nv = 0;
    UNIT_TRY(hipMemcpyAsync(flags, c.d_flags, sizeof(flags), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(&nt, d_toff + NT, sizeof(int), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(&nv, d_voff + NV, sizeof(int), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    c.tm.end();
    if (flags[0]) return CLEAN_ERR_INDEX;
    out.nv = nv; out.nt = nt;
    if (nv > vcap || nt > tcap) return UNIT_ERR_CAPACITY;

    out.bgr = nullptr;
    UNIT_ALLOC(c.scratch, out.xyz, float, (size_t)nv * 3);
    if (d.bgr) UNIT_ALLOC(c.scratch, out.bgr, unsigned char, (size_t)nv * 3);
    UNIT_ALLOC(c.scratch, out.tri, int, (size_t)nt * 3);
    c.tm.begin(CLEAN_T_FILTER);
    CLEAN_LAUNCH(d.nt, k_emit_tri, d.nt, d.tri, c.d_flags, d_tkeep, d_toff, d_voff, out.tri);
    CLEAN_LAUNCH(d.nv, k_emit_vtx, d.nv, d.xyz, d.bgr, d_vkeep, d_voff, out.xyz, out.bgr, d_vertex_of);
    c.tm.end();
    return 0;
}

// The smoothed positions and, if wanted, the normals of a device mesh whose indices the flag vouches for; queues only.  With no
// iteration the positions are the input's own.
int smooth_device(Call& c, const DevMesh& d, const CleanSmoothParams& p, bool want_normal, float*& d_xyz_out, float*& d_normal) {
    hipStream_t s = c.s;
    const size_t NV = (size_t)d.nv;
    QuantDev q;
    for (int a = 0; a < 3; ++a) q.origin[a] = p.origin[a];
    q.quantum = p.quantum;
    int* d_P;
    unsigned* d_D;
    u64* d_S;
    UNIT_ALLOC(c.scratch, d_P, int, NV * 3);
    UNIT_ALLOC(c.scratch, d_D, unsigned, NV);                     // zeroed
    UNIT_ALLOC(c.scratch, d_S, u64, NV * 3);                      // zeroed; every pass leaves it zeroed
    d_xyz_out = d.xyz;
    d_normal = nullptr;
    if (p.iterations > 0) UNIT_ALLOC(c.scratch, d_xyz_out, float, NV * 3);
    if (want_normal) UNIT_ALLOC(c.scratch, d_normal, float, NV * 3);

    c.tm.begin(CLEAN_T_QUANTISE);
    CLEAN_LAUNCH(d.nv, k_quantise, d.nv, d.xyz, q, d_P, c.d_flags);
    c.tm.end();
    if (p.iterations > 0) {
        c.tm.begin(CLEAN_T_SMOOTH);
        CLEAN_LAUNCH(d.nt, k_degree, d.nt, d.tri, c.d_flags, d_D);
        for (int it = 0; it < 2 * p.iterations; ++it) {
            CLEAN_LAUNCH(d.nt, k_pass_scatter, d.nt, d.tri, c.d_flags, d_P, d_S);
            CLEAN_LAUNCH(d.nv, k_pass_move, d.nv, d_P, d_S, d_D, (it & 1) ? p.M : p.L);
        }
        CLEAN_LAUNCH(d.nv, k_positions, d.nv, d_P, q, d_xyz_out);
        c.tm.end();
    }
    if (want_normal) {
        c.tm.begin(CLEAN_T_NORMALS);
        CLEAN_LAUNCH(d.nt, k_normal_scatter, d.nt, d.tri, c.d_flags, d_P, d_S);
        CLEAN_LAUNCH(d.nv, k_normal_final, d.nv, d_S, d_normal);
        c.tm.end();
    }
    return 0;
}

// the two refusal flags, waited for
int read_flags(Call& c) {
    hipStream_t s = c.s;
    int flags[2] = { 0, 0 };
    UNIT_TRY(hipMemcpyAsync(flags, c.d_flags, sizeof(flags), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    return flags[0] ? CLEAN_ERR_INDEX : flags[1] ? CLEAN_ERR_COORD : 0;
}

void zero_timing(double* timing) {
    if (timing) for (int i = 0; i < CLEAN_T_COUNT; ++i) timing[i] = 0.0;
}

}  // namespace

int mesh_components(hipStream_t s, int device, const CleanMesh& m, int32_t* label, int32_t* comp_triangles, int64_t* n_components, int64_t* largest,
                    double* timing) {
    zero_timing(timing);
    Call c(s, device, timing != nullptr);
    DevMesh d;
    Components cc;
    if (int rc = upload_mesh(c, m, false, d)) return rc;
    if (int rc = components_device(c, d, cc)) return rc;
    const size_t NV = (size_t)m.nv;
    int* d_comp = nullptr;
    if (comp_triangles) {
        UNIT_ALLOC(c.scratch, d_comp, int, NV);
        c.tm.begin(CLEAN_T_COMPONENTS);
        CLEAN_LAUNCH(d.nv, k_cc_comp_triangles, d.nv, cc.label, cc.count, d_comp);
        c.tm.end();
    }
    u64 stats[2] = { 0, 0 };
    UNIT_TRY(hipMemcpyAsync(stats, cc.stats, sizeof(stats), hipMemcpyDeviceToHost, s));
    if (int rc = read_flags(c)) return rc;
    c.tm.begin(CLEAN_T_DOWNLOAD);
    CLEAN_COPY(label, cc.label, sizeof(int) * NV, hipMemcpyDeviceToHost);
    if (comp_triangles) CLEAN_COPY(comp_triangles, d_comp, sizeof(int) * NV, hipMemcpyDeviceToHost);
    c.tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    *n_components = (int64_t)stats[1];
    *largest = (int64_t)stats_largest(stats[0]);
    if (timing) c.tm.collect(timing);
    return 0;
}

int mesh_filter(hipStream_t s, int device, const CleanMesh& m, const CleanFilterParams& f, const CleanFilterOut& out, double* timing) {
    zero_timing(timing);
    Call c(s, device, timing != nullptr);
    DevMesh d, kept;
    int* d_vertex_of = nullptr;
    if (int rc = upload_mesh(c, m, true, d)) return rc;
    const int rc = filter_device(c, d, f, out.vcap, out.tcap, kept, d_vertex_of);
    if (rc == 0 || rc == UNIT_ERR_CAPACITY) {
        *out.n_vertices = kept.nv;
        *out.n_triangles = kept.nt;
    }
    if (rc == 0) {
        c.tm.begin(CLEAN_T_DOWNLOAD);
        CLEAN_COPY(out.xyz, kept.xyz, sizeof(float) * (size_t)kept.nv * 3, hipMemcpyDeviceToHost);
        if (kept.bgr && out.bgr) CLEAN_COPY(out.bgr, kept.bgr, (size_t)kept.nv * 3, hipMemcpyDeviceToHost);
        CLEAN_COPY(out.tri, kept.tri, sizeof(int) * (size_t)kept.nt * 3, hipMemcpyDeviceToHost);
        if (out.vertex_of) CLEAN_COPY(out.vertex_of, d_vertex_of, sizeof(int) * (size_t)m.nv, hipMemcpyDeviceToHost);
        c.tm.end();
        UNIT_TRY(hipStreamSynchronize(s));
    }
    if (timing) c.tm.collect(timing);
    return rc;
}

int mesh_smooth(hipStream_t s, int device, const CleanMesh& m, const CleanSmoothParams& p, float* xyz_out, float* normal, double* timing) {
    zero_timing(timing);
    Call c(s, device, timing != nullptr);
    DevMesh d;
    float *d_xyz_out = nullptr, *d_normal = nullptr;
    if (int rc = upload_mesh(c, m, true, d)) return rc;
    if (int rc = smooth_device(c, d, p, normal != nullptr, d_xyz_out, d_normal)) return rc;
    if (int rc = read_flags(c)) return rc;
    const size_t NV = (size_t)m.nv;
    c.tm.begin(CLEAN_T_DOWNLOAD);
    CLEAN_COPY(xyz_out, d_xyz_out, sizeof(float) * NV * 3, hipMemcpyDeviceToHost);
    if (normal) CLEAN_COPY(normal, d_normal, sizeof(float) * NV * 3, hipMemcpyDeviceToHost);
    c.tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    if (timing) c.tm.collect(timing);
    return 0;
}

int mesh_clean(hipStream_t s, int device, const CleanMesh& m, const CleanFilterParams& f, const CleanSmoothParams& p, const CleanFilterOut& out,
               double* timing) {
    zero_timing(timing);
    Call c(s, device, timing != nullptr);
    DevMesh d, kept;
    int* d_vertex_of = nullptr;
    float *d_xyz_out = nullptr, *d_normal = nullptr;
    if (int rc = upload_mesh(c, m, true, d)) return rc;
    int rc = filter_device(c, d, f, out.vcap, out.tcap, kept, d_vertex_of);
    if (rc == 0) rc = smooth_device(c, kept, p, out.normal != nullptr, d_xyz_out, d_normal);
    if (rc == 0) rc = read_flags(c);
    if (rc == 0 || rc == UNIT_ERR_CAPACITY) {
        *out.n_vertices = kept.nv;
        *out.n_triangles = kept.nt;
    }
    if (rc == 0) {
        const size_t NV = (size_t)kept.nv;
        c.tm.begin(CLEAN_T_DOWNLOAD);
        CLEAN_COPY(out.xyz, d_xyz_out, sizeof(float) * NV * 3, hipMemcpyDeviceToHost);
        if (kept.bgr && out.bgr) CLEAN_COPY(out.bgr, kept.bgr, NV * 3, hipMemcpyDeviceToHost);
        if (out.normal) CLEAN_COPY(out.normal, d_normal, sizeof(float) * NV * 3, hipMemcpyDeviceToHost);
        CLEAN_COPY(out.tri, kept.tri, sizeof(int) * (size_t)kept.nt * 3, hipMemcpyDeviceToHost);
        if (out.vertex_of) CLEAN_COPY(out.vertex_of, d_vertex_of, sizeof(int) * (size_t)m.nv, hipMemcpyDeviceToHost);
        c.tm.end();
        UNIT_TRY(hipStreamSynchronize(s));
    }
    if (timing) c.tm.collect(timing);
    return rc;
}

}  // namespace sfmba
