// pcg_common.h -- what the reduced-system CG families share: constants, the layout of the solver state, device helpers, and the host
// entry points of every family.  One unit per family (DESIGN.md section 4 "CG families"):
//   pcg_fast.hip                 d <= 1280, rows of S~ in registers, one launch per iteration
//   pcg_segments.hip             the same geometry with the segmented coarse space (k_ml_*), workgroup = camera
//   pcg_streaming.hip            any d, both triangles of S~ streamed, one launch per iteration
//   pcg_symmetric.hip            d > 1280, ONE triangle streamed (k_sy_*), two launches per iteration
//   pcg_segments_streaming.hip   d > 1280 with the segmented coarse space (k_sg_*), three launches per iteration
// dense_solver.hip picks the family (dense_pcg_path) and owns the workspace.  The units are compiled without relocatable device code: a kernel
// is launched from the unit that defines it, which is why the entry points below are host functions.
#pragma once
#include "dense_solver.h"
#include "sfmba_device.h"
#include "coarse_inverse.h"
#include <math.h>
#include <algorithm>
#include <type_traits>
#include <utility>

namespace sfmba {

// ------------------------------------------------------------------------------------------
// Block-Jacobi preconditioned conjugate gradients on the dense reduced system.
//
// The preconditioner is folded into the matrix once per solve: with Lb = blockdiag(chol(S_jj)) (6x6
// camera blocks + the 1x1 focal), S~ = Lb^-1 S Lb^-T has identity diagonal blocks and plain CG on
// S~ x~ = Lb^-1 rhs is exactly block-Jacobi PCG on S.  Each CG iteration is then ONE kernel launch:
// every workgroup redundantly forms alpha, r, beta and the new search direction p (length d, from L2)
// in LDS, multiplies its own rows of S~ by p and publishes its slice of x, r, p, q = S~ p plus its
// partial p.q; the next launch (stream order) finishes the dot product.  Vectors are double-buffered
// by iteration parity so no workgroup overwrites what another one is still reading.  The rows a
// workgroup owns never change, so its slab of S~ stays in its XCD's L2 across iterations.
// ------------------------------------------------------------------------------------------
#ifndef SFMBA_PCG_MAXWG
#define SFMBA_PCG_MAXWG 256
#endif
constexpr int PCG_MAXWG = SFMBA_PCG_MAXWG;        // workgroups of the fast path (one partial dot product per thread)
constexpr int PCG_MAXWG_BIG = 1024;   // workgroups of the generic path
constexpr int PCG_PART = 1024;        // stride (workgroups) of the per-iteration partial-sum buffers
enum { PF_DONE = 0, PF_ITERS = 1, PF_XBUF = 2 };     // DenseSolver::flags: the first launch number with nothing left to do (0 = running), iterations, which x buffer holds the solution
enum { PS_RR0 = 0, PS_RRF = 1 };     // threshold base of the running solve; |b~|^2 of the FIRST solve of an anchored sequence

// Stopping rule: |r|^2 <= tol^2 * base.  Plain CG: base = |b~|^2 (relative residual).  Inside one LM solve the
// tolerance is ANCHORED to the first iteration's right-hand side: base = min(max(|b~_k|^2, |b~_first|^2), cap * |b~_k|^2).
// Why: the error a truncated solve leaves in the PARAMETERS is ~ cond * |r|, absolute -- the first LM step is orders of
// magnitude larger than the later ones, so a relative tolerance spends its iterations on the small steps and leaves
// the big step's error (drift along the gauge directions, 1e-4 at tol 1e-6) in the result.  Anchored, every step is
// solved to the same absolute accuracy; cap keeps every solve at least 1e-4 relative (the accept/reject and
// function-tolerance decisions of the LM loop are insensitive well beyond that).
__device__ __forceinline__ double pcg_threshold_base(double rr, double* scal, int anchor, double cap) {
    if (anchor == 1) { scal[PS_RRF] = rr; return rr; }
    if (anchor == 2) return fmin(fmax(rr, scal[PS_RRF]), cap * rr);
    return rr;
}
// vec layout: x[2] r[2] p[2] q[2], each ld doubles; btilde after them
__device__ __forceinline__ double* pcg_vec(double* vec, int which, int buf, int ld) { return vec + (size_t)(2 * which + buf) * ld; }

__device__ __forceinline__ void block_sum2(double& a, double& b, double* red) {
    { a = wave_allsum(a); b = wave_allsum(b); }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[2 * w] = a; red[2 * w + 1] = b; }
    __syncthreads();
    a = red[0] + red[2] + red[4] + red[6];
    b = red[1] + red[3] + red[5] + red[7];
}

// Host mailbox (pinned, host-mapped): {iterations, done}.  The host polls it instead of issuing a D2H copy + stream
// synchronise per batch; written by one lane with system-scope stores.  done: 0 while the solve runs, iterations + 1 once it has ended -- ONE word
// carries the verdict and the count: a host that is polling when the post arrives sees `done` before the iterations word written behind it
// (it used to read the count of the launch before: one iteration short, or the batch length for a zero right-hand side).
__device__ __forceinline__ void pcg_post(int* mailbox, int iters, int done) {
    __hip_atomic_store(mailbox + 1, done ? iters + 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(mailbox, iters, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------------------------------------------------
// Coarse space ("gauge deflation").  adjustBundle() holds no parameter block constant (BA.cpp:160-164), so the
// undamped problem is invariant under the 7 similarity transforms of the scene; the LM damping lifts those directions to
// eigenvalues ~1/radius of S~ while the rest of the spectrum sits in [0.2, 2] (measured, cfg 3: seven eigenvalues
// 2.3e-4 .. 2.8e-4, one at 3e-2 -- the focal/depth direction --, everything else >= 0.59).  Plain block-Jacobi CG spends
// most of its iterations on those 8 directions (48 .. 68 iterations to 1e-8) and leaves its truncation error exactly
// there (the "gauge drift" of the parameters).  With the 8 analytic vectors W~ (k_finalize writes them: world
// translation x3, world rotation x3, scale, focal/depth) as a coarse space and the additive two-level preconditioner
//      M^-1 = I + W~ E^-1 W~^T,      E = W~^T S~ W~   (8 x 8),
// the same accuracy takes 8 .. 12 iterations and the coarse components are solved exactly.
//
// The preconditioner is never applied to a full vector: the search direction is kept split, p = p_r + W~ p_mu, so that
//      q = S~ p   = S~ p_r + (S~ W~) p_mu          -- own rows of AW = S~ W~ only
//      W~^T r     carried by the recurrence c <- c - alpha (W~^T q), with W~^T q summed from per-workgroup partials
//      p . q      = p_r . q + p_mu . (W~^T q)
// i.e. one CG iteration still streams r, q, p_r and S~ once; W~ and AW are touched only in the rows a workgroup owns.
// k_pcg_coarse forms AW, E and c_0 = W~^T b~ (one extra pass over S~ per LM iteration), k_pcg_coarse_invert the scaled
// 8 x 8 inverse.  A vector whose pivot vanishes (degenerate configurations, fewer cameras than gauge freedoms) is dropped.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PCG_NW = 8;                 // coarse vectors
constexpr int PCG_NPART = 1 + PCG_NW;     // per-workgroup partials per iteration: p_r . q, W~^T q
// scal: [PS_RR0] [PS_RRF] ... then per iteration parity PS_STATE_LEN doubles of solver state written by workgroup 0
enum { PS_STATE = 8, PS_STATE_LEN = 32, PS_RZ = 0, PS_C = 1, PS_MU = 9, PS_PMU = 17 };      // c = W~^T r, mu = E^-1 c, p_mu
constexpr int CO_TILE = 1024;             // columns of W~ staged in LDS (fp32) per pass of k_pcg_coarse
constexpr int CO_MAXROWS = 4;             // rows per wave k_pcg_coarse can hold (rows_per_wg <= 16)

__device__ __forceinline__ double* pcg_part(double* part, int parity, int v) { return part + ((size_t)parity * PCG_NPART + v) * PCG_PART; }

// four consecutive matrix entries, loaded with 16-byte loads
template <typename FT> struct Quad;
template <> struct Quad<float> {
    float4 v;
    __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
    __device__ __forceinline__ double get(int i) const { return (double)(i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w); }
};
template <> struct Quad<double> {
    double2 a, b;
    __device__ __forceinline__ void load(const double* p) { a = reinterpret_cast<const double2*>(p)[0]; b = reinterpret_cast<const double2*>(p)[1]; }
    __device__ __forceinline__ double get(int i) const { return i == 0 ? a.x : i == 1 ? a.y : i == 2 ? b.x : b.y; }
};

// E and c_0 = sums of the per-workgroup partials of k_pcg_coarse*: NPW values per wave (18: E and c_0; 20: W~^T S~ b~ behind them, fast
// path), their lane-partials reduced in lock step; tot[0 .. 4 NPW) (LDS) is complete after the caller's next __syncthreads().  All 256 threads.
template <int NPW = 18>
__device__ __forceinline__ void coarse_sum_partials(int nwg, const double* __restrict__ epart, double* tot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double part[NPW];
#pragma unroll
    for (int m = 0; m < NPW; ++m) part[m] = 0.0;
    for (int i0 = 0; i0 < nwg; i0 += 128) {               // 2 NPW independent loads per lane and pass (clamped, branch-free)
        double t[NPW][2];
#pragma unroll
        for (int m = 0; m < NPW; ++m)
#pragma unroll
            for (int i = 0; i < 2; ++i) { const int wg = i0 + lane + 64 * i; t[m][i] = epart[(size_t)(w + 4 * m) * PCG_PART + (wg < nwg ? wg : nwg - 1)]; }
#pragma unroll
        for (int m = 0; m < NPW; ++m)
#pragma unroll
            for (int i = 0; i < 2; ++i) part[m] += (i0 + lane + 64 * i < nwg) ? t[m][i] : 0.0;
    }
#pragma unroll
    for (int m = 0; m < NPW; ++m) part[m] = wave_allsum(part[m]);
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < NPW; ++m) tot[w + 4 * m] = part[m];
    }
}

// Sum of the per-workgroup partials of the previous launch.  Wave w owns values w, w + 4, w + 8: `mine` holds this lane's
// share (loaded up front by the caller), the totals land in red[0 .. NV) after the caller's next __syncthreads().  The
// (up to three) wave reductions advance in lock step: a shuffle is ~50 cycles of latency, three dependent chains of six
// would sit on the critical path of every CG iteration.
template <int NV>
__device__ __forceinline__ void reduce_partials(double (&mine)[3], double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 3; ++j) if (4 * j < NV) mine[j] = wave_allsum(mine[j]);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) if (w + 4 * j < NV) red[w + 4 * j] = mine[j];
    }
}

// 8-term dot product as two chains of four (a dependent DFMA is ~32 cycles)
__device__ __forceinline__ double dot8(const double (&a)[PCG_NW], const double (&b)[PCG_NW]) {
    double s0 = a[0] * b[0], s1 = a[1] * b[1];
    s0 = fma(a[2], b[2], s0); s1 = fma(a[3], b[3], s1);
    s0 = fma(a[4], b[4], s0); s1 = fma(a[5], b[5], s1);
    s0 = fma(a[6], b[6], s0); s1 = fma(a[7], b[7], s1);
    return s0 + s1;
}
__device__ __forceinline__ double lane_bcast(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
// out = E^-1 v in every lane: lane t (mod 8) forms row t, eight lane broadcasts distribute the result inside the wave
// (no workgroup barrier).  einv_s: the 64 entries in LDS.
__device__ __forceinline__ void einv_apply(const double* einv_s, const double (&v)[PCG_NW], double (&out)[PCG_NW]) {
    const int t = threadIdx.x & 7;
    double row[PCG_NW];
#pragma unroll
    for (int j = 0; j < PCG_NW; ++j) row[j] = einv_s[t * PCG_NW + j];
    const double r = dot8(row, v);
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k) out[k] = lane_bcast(r, k);
}

// LDS scratch of the CG kernels behind the search direction: [0..9) partial totals, [16..20) rrn per wave,
// [32..40) p_mu of this iteration, [40..76) end-of-kernel partials per wave (4 x 9), [80..144) E^-1; first launch of the fast
// path only: [144..224) E, c_0 and W~^T S~ b~ summed from the partials, [224..352) work space of the 8 x 8 inversion
constexpr int PCG_RED = 352;

// fast path (pcg_fast.hip; the segmented fast path keeps its geometry): what the path selection and the workspace read
constexpr int PCG_EPT = 5;    // vector elements per thread  (256 * 5 >= d)
constexpr int PCG_RPW = 2;    // rows of S~ per wave         (rows_per_wg <= 8)
constexpr int PCG_CPL = 20;   // columns per lane            (64 * 20 >= d)

// symmetric streaming path (pcg_symmetric.hip): tile and accumulator sizes the workspace is built from
constexpr int SY_R = 32;              // rows of a tile: eight per wave, one batch of eight 16-byte loads in flight per lane
constexpr int SY_C = 256;             // columns of a tile: 64 lanes x four entries
constexpr int SY_SLOTS = 64;          // slots of the partial sums (one 128-byte line per value and slot: atomics on one line serialise)
constexpr int SY_SLOT_STRIDE = 16;    // doubles between two accumulators
#ifndef SFMBA_SY_CR
#define SFMBA_SY_CR 128
#endif
constexpr int SY_CR = SFMBA_SY_CR;

// Read extent of the symmetric kernels.  k_sy_prod and k_sy_coarse load every tile whole: lane l of a tile at column c0 (a multiple of SY_C, c0 < d)
// reads the four entries c0 + 4 l .. c0 + 4 l + 3 of a matrix row, of p and of the eight rows of W~ WITHOUT a test against d or ld (the values of the
// columns >= d are selected away afterwards).  The last column tile starts at c0 = SY_C floor((d - 1) / SY_C), so the highest column touched is
// SY_C ceil(d / SY_C) - 1, in rows up to d - 1 of S~ (d rows of ld), in row 7 of W~ (8 rows of ld) and in p = vec + 4 ld or 5 ld (9 rows of ld).
// With ld = 64 ceil((d + 1) / 64) that is up to
//      pcg_tile_slack(d, ld) = max(0, SY_C ceil(d / SY_C) - ld)  <=  SY_C - 64 = 192
// entries behind d ld entries of Sfull / Sfull32 and behind the 8 ld of W~ (0 where ld % SY_C == 0; 192, 128, 64 for ld % SY_C = 64, 128, 192); the
// workspace allocates every array these kernels index by tile -- Sfull, Sfull32, W, AWt, vec -- with that many entries more (dense_solver.hip), so the
// read stays inside the array's own allocation whatever the allocator's granularity.  (AWt is only indexed below d and p's overrun lands in the
// following vectors of vec: they take the slack for uniformity, not from need.)
// The other families, read for the same property at ld % 256 != 0 and d within four of ld: k_pcg_iter and k_sg_q read double2 columns 2 c, 2 c + 1 with
// c < d >> 1 and float4 columns 4 c .. 4 c + 3 with c < d >> 2 (the fp32 prefetch of k_pcg_iter: lane + 64 m <= lane + 192 < d >> 2, else column 0),
// the remainder entry by entry below d; k_pcg_coarse loads a quad only where its first column is below d, so its last column is below
// 4 ceil(d / 4) <= ld, and its W~ loads are clamped to column 0; rows are clamped to the workgroup's first row, which exists.  None leaves d rows of ld.
__host__ __device__ inline size_t pcg_tile_slack(int d, int ld) {
    const int full = (d + SY_C - 1) / SY_C * SY_C;
    return full > ld ? (size_t)(full - ld) : 0;
}

// Dynamic LDS of the iteration kernels that keep the search direction in LDS (k_pcg_iter, k_sg_q, k_pcg_iter_fast, k_pcg_iter_ml): CgPath::lds.  A
// workgroup of gfx950 may take the whole 160 KiB of its CU (hipDeviceAttributeMaxSharedMemoryPerBlock = 163 840; DenseSolver::lds_limit holds the
// device's answer); above the 64 KiB of the earlier parts the launch functions raise hipFuncAttributeMaxDynamicSharedMemorySize once per kernel.
// dense_pcg_path refuses a size whose request exceeds the limit (family 0): the solve returns an error and launches nothing.
constexpr size_t PCG_LDS_DEFAULT = (size_t)64 << 10;
constexpr size_t PCG_LDS_GFX950 = (size_t)160 << 10;

// segmented coarse space (pcg_segments.hip)
constexpr int ML_G = 8;                    // hat functions along the (cyclic) camera order
constexpr int ML_NC = 7 * ML_G + 1;        // coarse vectors: (g, k) -> 7 g + k, the global focal/depth vector last
constexpr int ML_N = 64;                   // padded: one coarse entry per lane
constexpr int ML_MIN_CAMS = 4 * ML_G;      // below this the hats have too few cameras each: the 8-vector path
constexpr int ML_LDS_TAIL = 96 + 7 * 256 + 2 * 4 * ML_N;     // doubles of LDS behind the search direction: red | tmp | gq | egq

// ... on the streaming path (pcg_segments_streaming.hip)
constexpr int SG_MAXG = 20;
constexpr int SG_NCP = 144;                 // padded coarse dimension: 7 SG_MAXG + 1 = 141 vectors
constexpr int SG_UWG = 16;                  // workgroups of the vector kernels
enum { SGS_RZ = 0, SGS_PQ = 1, SGS_LEN = 4 };     // per-parity scalars of the running solve (sg_state)
__host__ __device__ __forceinline__ int sg_hats(int nc) { const int g = nc / 25; return g < ML_G ? ML_G : g > SG_MAXG ? SG_MAXG : g; }

// In-place Gauss-Jordan inverse of the Jacobi-scaled N x N matrix E (symmetric positive definite, no pivot search) in the registers of ONE workgroup:
// thread (tr, tc) holds the TR x TC tile of rows TR tr .., columns TC tc .. -- per pivot it needs TR entries of the pivot column and TC of the pivot row
// from LDS (a column-per-thread layout reads a whole row slice per thread: the kernel was bound by that LDS traffic).  One barrier per pivot (row, column
// and the next diagonal entry double-buffered by pivot parity); the next pivot's reciprocal is formed during the current update; L = lcm(TR, TC)
// steps are instantiated with compile-time register indices and that body loops.  A pivot below 1e-10 of the unit diagonal: the vector depends on the
// earlier ones, its step is skipped and its row and column of the result are zero.  Rows / columns >= NC: zero.
template <typename F, int... S>
__device__ __forceinline__ void gj_steps(F& step, int m, std::integer_sequence<int, S...>) { (step(m, std::integral_constant<int, S>()), ...); }
template <int N, int TR, int TC, int L>
__device__ __forceinline__ void gj_invert_tiled(int NC, const double* __restrict__ E, double* __restrict__ einv,
                                                double* rowbuf, double* colbuf, double* sc, double* diagbuf, unsigned char* drop) {
    static_assert(N % TR == 0 && N % TC == 0 && L % TR == 0 && L % TC == 0, "tile geometry");
    constexpr int NTC = N / TC;
    const int tid = threadIdx.x, tr = tid / NTC, tc = tid % NTC;
    for (int t = tid; t <= N; t += blockDim.x) {
        const double dii = t < NC ? E[(size_t)t * N + t] : 0.0;
        const bool ok = dii > 0.0 && dii <= 1.7e308;
        if (t < N) sc[t] = ok ? 1.0 / sqrt(dii) : 0.0;
        drop[t] = ok ? 0 : 1;
    }
    __syncthreads();
    double a[TR][TC];
#pragma unroll
    for (int rr = 0; rr < TR; ++rr)
#pragma unroll
        for (int cc = 0; cc < TC; ++cc) {
            const int i = TR * tr + rr, j = TC * tc + cc;
            const bool in = i < NC && j < NC;
            const double v = in ? 0.5 * (E[(size_t)i * N + j] + E[(size_t)j * N + i]) * sc[i] * sc[j] : 0.0;
            a[rr][cc] = (i == j) ? 1.0 : v;
        }
    double piv = 1.0, ip = 1.0;                      // unit diagonal after the scaling
    auto step = [&](int m, auto sconst) __attribute__((always_inline)) {
        constexpr int sidx = decltype(sconst)::value, rr0 = sidx % TR, cc0 = sidx % TC, rr1 = (sidx + 1) % TR, cc1 = (sidx + 1) % TC;
        const int p = L * m + sidx;
        if (p >= NC) return;                         // uniform
        const int rg = p / TR, cg = p / TC, par = p & 1;
        if (tr == rg) {
#pragma unroll
            for (int cc = 0; cc < TC; ++cc) rowbuf[par * N + TC * tc + cc] = a[rr0][cc];
        }
        if (tc == cg) {
#pragma unroll
            for (int rr = 0; rr < TR; ++rr) colbuf[par * N + TR * tr + rr] = a[rr][cc0];
        }
        if (tr == (p + 1) / TR && tc == (p + 1) / TC) diagbuf[par] = a[rr1][cc1];
        __syncthreads();
        const bool ok = !drop[p] && piv > 1e-10;
        double dn = diagbuf[par];
        if (ok) {
            // a_ij -= (a_ip / piv) a_pj everywhere -- the pivot row itself with the multiplier 1 - 1/piv --, then the pivot column is set
            double fc[TR], f[TR], rv[TC];
#pragma unroll
            for (int rr = 0; rr < TR; ++rr) { fc[rr] = colbuf[par * N + TR * tr + rr] * ip; f[rr] = (TR * tr + rr == p) ? 1.0 - ip : fc[rr]; }
#pragma unroll
            for (int cc = 0; cc < TC; ++cc) rv[cc] = rowbuf[par * N + TC * tc + cc];
            const int q = p + 1 < N ? p + 1 : N - 1;
            dn = fma(-colbuf[par * N + q] * ip, rowbuf[par * N + q], dn);
#pragma unroll
            for (int rr = 0; rr < TR; ++rr)
#pragma unroll
                for (int cc = 0; cc < TC; ++cc) a[rr][cc] = fma(-f[rr], rv[cc], a[rr][cc]);
            if (tc == cg) {
#pragma unroll
                for (int rr = 0; rr < TR; ++rr) a[rr][cc0] = (TR * tr + rr == p) ? ip : -fc[rr];
            }
        } else if (tid == 0) drop[p] = 1;
        piv = dn;
        ip = fast_rcp(dn);
    };
    for (int m = 0; m * L < NC; ++m) gj_steps(step, m, std::make_integer_sequence<int, L>());
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < TR; ++rr)
#pragma unroll
        for (int cc = 0; cc < TC; ++cc) {
            const int i = TR * tr + rr, j = TC * tc + cc;
            einv[(size_t)i * N + j] = (drop[i] || drop[j]) ? 0.0 : a[rr][cc] * sc[i] * sc[j];
        }
}

// b~ = Lb^-1 rhs lives behind the eight CG vectors (pcg_vec)
inline double* pcg_btilde(const DenseSolver* ws) { return ws->vec + (size_t)8 * ws->ld; }

// Host entry points, two per family, both for the solve ws->run describes (dense_pcg_solve fills it in before it calls them):
//   *_setup    enqueues the family's coarse set-up (nothing where run.path.coarse is off);
//   *_iterate  enqueues one CG iteration; init = the first launch of the solve, `in` = (launch number << 1) | parity (see k_pcg_iter), 0 with init.
void pcg_fast_setup(hipStream_t s, const DenseSolver* ws, Profiler* prof);
void pcg_fast_iterate(hipStream_t s, const DenseSolver* ws, bool init, int in, int anchor, double cap);
void pcg_segments_setup(hipStream_t s, const DenseSolver* ws, Profiler* prof);
void pcg_segments_iterate(hipStream_t s, const DenseSolver* ws, bool init, int in, int anchor, double cap);
void pcg_streaming_setup(hipStream_t s, const DenseSolver* ws, Profiler* prof);
void pcg_streaming_iterate(hipStream_t s, const DenseSolver* ws, bool init, int in, int anchor, double cap);
void pcg_symmetric_setup(hipStream_t s, const DenseSolver* ws, Profiler* prof);
void pcg_symmetric_iterate(hipStream_t s, const DenseSolver* ws, bool init, int in, int anchor, double cap);
void pcg_segments_streaming_setup(hipStream_t s, const DenseSolver* ws, Profiler* prof);
void pcg_segments_streaming_iterate(hipStream_t s, const DenseSolver* ws, bool init, int in, int anchor, double cap);
// k_pcg_coarse_invert (pcg_fast.hip) on its own: E^-1, c_0 and E from nwg workgroups' partials.  The streaming and the symmetric set-up end with it.
void pcg_coarse_invert(hipStream_t s, int nwg, const double* epart, double* out);

}  // namespace sfmba
