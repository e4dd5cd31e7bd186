// dense_solver.hip -- the reduced camera system  S z = rhs  (dim 6*Nc+1) solved on the device by preconditioned CG: the block-Jacobi transform, the
// choice of the CG family, the solve loop and the workspace.
//
// Replaces what DENSE_SCHUR hands to Eigen's LLT in the reference configuration
// (SfMToyLib/SfMBundleAdjustmentUtils.cpp:172, DenseSchurComplementSolver [Ceres-upstream]); the factorisation itself
// (SFMBA_LINEAR_CHOLESKY, AUTO's fallback) is dense_cholesky.hip.  Both share the workspace of dense_solver.h and the storage:
// the linearisation passes (ba_cams.hip, ba_pairs.hip, ba_finalize.hip) accumulate the UPPER triangle of the row-major matrix, padded to a multiple of CHOL_NB.
//
// Six CG families (DESIGN.md section 4 "CG families"), one unit each behind the entry points of pcg_common.h: fast (d <= 1280, rows in registers),
// segmented fast, streaming, symmetric streaming, streaming segmented with the dense and with the block-sparse product.  dense_pcg_path picks one.
#include "pcg_common.h"
#include "../../include/sfmba.h"
#include <stdio.h>
#include <chrono>
#include <cstdlib>

namespace sfmba {

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

constexpr int NB = CHOL_NB;   // padding unit of the matrix (dense_cholesky.hip)

// Linv of each diagonal block: row-major lower 6x6 (zeros above), focal: 1/sqrt(S_ff) at [nb6*36]
// (Sibling: the factor and inverse inside k_finalize, ba_finalize.hip -- fast_rsq and reciprocal pivots there, sqrt and divisions here: they stay two.)
__global__ void k_pcg_blockchol(const double* __restrict__ S, int ld, int d, double* __restrict__ linv, int* info) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int nb6 = (d - 1) / 6;
    const int rem = d - 6 * nb6;     // trailing scalars (1 for a BA system)
    if (b >= nb6 + rem) return;
    if (b >= nb6) {
        const int e = 6 * nb6 + (b - nb6);
        const double v = S[(size_t)e * ld + e];
        if (!(v > 0.0)) atomicCAS(info, 0, e + 1);
        linv[(size_t)nb6 * 36 + (b - nb6)] = 1.0 / sqrt(v > 0.0 ? v : 1.0);
        return;
    }
    double L[6][6], Li[6][6];
    const int o = 6 * b;
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c <= r; ++c) L[r][c] = S[(size_t)(o + c) * ld + o + r];
    bool ok = true;
    for (int j = 0; j < 6; ++j) {
        double dj = L[j][j];
        for (int t = 0; t < j; ++t) dj -= L[j][t] * L[j][t];
        if (!(dj > 0.0)) { ok = false; dj = 1.0; }
        const double lj = sqrt(dj);
        L[j][j] = lj;
        for (int i = j + 1; i < 6; ++i) {
            double v = L[i][j];
            for (int t = 0; t < j; ++t) v -= L[i][t] * L[j][t];
            L[i][j] = v / lj;
        }
    }
    if (!ok) atomicCAS(info, 0, o + 1);
    for (int c = 0; c < 6; ++c)
        for (int r = 0; r < 6; ++r) {
            if (r < c) { Li[r][c] = 0.0; continue; }
            double v = (r == c) ? 1.0 : 0.0;
            for (int t = c; t < r; ++t) v -= L[r][t] * Li[t][c];
            Li[r][c] = v / L[r][r];
        }
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) linv[(size_t)b * 36 + r * 6 + c] = Li[r][c];
}

// F = Lb^-1 S Lb^-T (full symmetric, d rows x ld), btilde = Lb^-1 rhs.  One thread per block pair I <= J;
// trailing 1x1 blocks are padded to 6x6 with zeros so that every loop has compile-time bounds (registers).
template <typename FT>
__global__ __launch_bounds__(64) void k_pcg_transform(const double* __restrict__ S, int ld, int d, const double* __restrict__ linv,
                                                      const double* __restrict__ rhs, FT* __restrict__ F, double* __restrict__ bt) {
    const int nb6 = (d - 1) / 6;
    const int nB = nb6 + (d - 6 * nb6);
    const int J = blockIdx.x * blockDim.x + threadIdx.x;
    const int I = blockIdx.y;
    if (J >= nB || J < I) return;
    const int ri = I < nb6 ? 6 * I : 6 * nb6 + (I - nb6), si = I < nb6 ? 6 : 1;
    const int rj = J < nb6 ? 6 * J : 6 * nb6 + (J - nb6), sj = J < nb6 ? 6 : 1;
    double A[6][6], Lj[6][6], Li[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double fi = (r == 0 && c == 0) ? linv[(size_t)nb6 * 36 + (I < nb6 ? 0 : I - nb6)] : 0.0;
            const double fj = (r == 0 && c == 0) ? linv[(size_t)nb6 * 36 + (J < nb6 ? 0 : J - nb6)] : 0.0;
            Li[r][c] = (I < nb6) ? linv[(size_t)I * 36 + r * 6 + c] : fi;
            Lj[r][c] = (J < nb6) ? linv[(size_t)J * 36 + r * 6 + c] : fj;
            const int gr = ri + r, gc = rj + c;
            const bool in = r < si && c < sj;
            // upper storage: element (gr, gc) with column >= row, mirrored inside diagonal blocks
            A[r][c] = in ? (gc >= gr ? S[(size_t)gr * ld + gc] : S[(size_t)gc * ld + gr]) : 0.0;
        }
    double U[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double v = 0.0;
#pragma unroll
            for (int t = 0; t < 6; ++t) v += Li[r][t] * A[t][c];      // Li is lower triangular (zeros above)
            U[r][c] = v;
        }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double v = 0.0;
#pragma unroll
            for (int t = 0; t < 6; ++t) v += U[r][t] * Lj[c][t];
            if (r < si && c < sj) {
                F[(size_t)(ri + r) * ld + rj + c] = (FT)v;
                if (I != J) F[(size_t)(rj + c) * ld + ri + r] = (FT)v;
            }
        }
    if (I == J) {
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double v = 0.0;
#pragma unroll
            for (int t = 0; t < 6; ++t) v += (t < si) ? Li[r][t] * rhs[ri + t] : 0.0;
            if (r < si) bt[ri + r] = v;
        }
    }
}

// solution of the original system: z = Lb^-T x~
__global__ void k_pcg_finish(int d, int ld, const double* __restrict__ vec, const double* __restrict__ linv, const int* flags,
                             double* __restrict__ z) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= d) return;
    const double* x = vec + (size_t)(flags[PF_XBUF]) * ld;   // x buffers are vec[0], vec[1]
    const int nb6 = (d - 1) / 6;
    const int b = e / 6;
    if (b >= nb6) { z[e] = linv[(size_t)nb6 * 36 + (e - 6 * nb6)] * x[e]; return; }
    const int c = e - 6 * b;
    double v = 0.0;
    for (int t = c; t < 6; ++t) v += linv[(size_t)b * 36 + t * 6 + c] * x[6 * b + t];
    z[e] = v;
}

// The fast path's geometry, the ONE copy of the test: the vectors in registers (PCG_EPT entries per thread), a row of S~ across a wave (PCG_CPL
// columns per lane), at most 4 PCG_RPW rows per workgroup on PCG_MAXWG workgroups.  (At the default PCG_MAXWG = 256 the last clause follows from
// the first two -- d <= 1280 gives five rows --; a build with fewer workgroups moves the boundary for every caller alike.)
static bool pcg_fast_fits(int d) { return d <= 256 * PCG_EPT && d <= 64 * PCG_CPL && (d + PCG_MAXWG - 1) / PCG_MAXWG <= 4 * PCG_RPW; }

// the segmented coarse space needs the fast path's geometry with one workgroup per camera (d = 6 nc + 1) and enough cameras per hat
bool dense_pcg_segments_applicable(const DenseSolver* ws) {
    const int d = ws->d, nc = (d - 1) / 6;
    return d == 6 * nc + 1 && nc >= ML_MIN_CAMS && nc + 1 <= PCG_MAXWG && pcg_fast_fits(d);
}

bool dense_pcg_segments_streaming_applicable(const DenseSolver* ws) {
    const int d = ws->d, nc = (d - 1) / 6;
    return d == 6 * nc + 1 && nc >= ML_MIN_CAMS && !pcg_fast_fits(d) && (d + 7) / 8 <= PCG_PART && nc + 1 <= 64 * SG_UWG - SG_UWG;
}

bool dense_pcg_symmetric_applicable(const DenseSolver* ws) { return !pcg_fast_fits(ws->d); }

// fp32 storage of S~ on the streaming paths whenever the caller asked for it (dense_pcg_want_f32 allocated the buffer); the fast paths are fp64
static bool pcg_reads_f32(const DenseSolver* ws) { return !pcg_fast_fits(ws->d) && ws->use_f32 && ws->Sfull32 != nullptr; }

// The path a solve takes: a pure function of the dimension, of what the caller set per solve (use_f32, symmetric, blk_mask / blk_fill), of the buffers
// that exist, and of the two requests coarse (ws->W holds the gauge vectors) and segments (the segmented coarse space where it applies).  Everything
// else -- the set-up, the launches, the batch sizing, the step probe -- reads the result.
CgPath dense_pcg_path(const DenseSolver* ws, bool coarse, bool segments) {
    const int d = ws->d, nc = (d - 1) / 6;
    const bool fast = pcg_fast_fits(d);
    // segmented coarse space (7 x 8 hat-restricted gauge vectors + 1), workgroup = camera; its streaming form (d > 1280): classical PCG, three launches
    const bool ml = segments && coarse && dense_pcg_segments_applicable(ws) && ws->W && ws->mlAW;
    const bool sg = segments && coarse && dense_pcg_segments_streaming_applicable(ws) && ws->W && ws->sgV;
    // ... whose product is block-sparse for a reduced matrix filled below a quarter (one workgroup per camera)
    const bool sparse = sg && ws->blk_mask != nullptr && ws->blk_fill < 0.25 && nc + 1 <= PCG_PART;
    // symmetric streaming path: the caller's pair pass wrote (at least) the upper triangle; one read of it per iteration (k_sy_prod)
    const bool sym = !fast && !sg && ws->symmetric && ws->sym_tiles != nullptr;
    CgPath p;
    p.family = ml ? SFMBA_FAMILY_PCG_SEGMENTS : fast ? SFMBA_FAMILY_PCG_FAST
             : sg ? (sparse ? SFMBA_FAMILY_PCG_SEGMENTS_STREAMING_SPARSE : SFMBA_FAMILY_PCG_SEGMENTS_STREAMING)
             : sym ? SFMBA_FAMILY_PCG_SYMMETRIC : SFMBA_FAMILY_PCG_STREAMING;
    p.rows_per_wg = ml ? 6 : sg ? 8 : fast ? (d + PCG_MAXWG - 1) / PCG_MAXWG
                  : std::max(8, ((d + PCG_MAXWG_BIG - 1) / PCG_MAXWG_BIG + 7) / 8 * 8);       // (streaming: two rows per wave at a time)
    p.nwg = (d + p.rows_per_wg - 1) / p.rows_per_wg;
    p.lds = sizeof(double) * (size_t)(ws->ld + (ml ? ML_LDS_TAIL : sg ? 0 : PCG_RED));
    p.f32 = pcg_reads_f32(ws);
    // every family but the symmetric one keeps the search direction in dynamic LDS: a size the device cannot give is no family at all (dense_pcg_solve refuses it)
    if (p.family != SFMBA_FAMILY_PCG_SYMMETRIC && p.lds > (ws->lds_limit ? ws->lds_limit : PCG_LDS_DEFAULT)) p.family = 0;
    // coarse space: the caller's linearisation wrote W~ (ws->W); AW, E^-1 and c_0 are formed by the family's set-up
    p.coarse = coarse && ws->W && ws->AW && p.rows_per_wg <= 4 * CO_MAXROWS;
    p.coarse_vectors = ml ? ML_NC : sg ? 7 * sg_hats(nc) + 1 : p.coarse ? PCG_NW : 0;
    p.first_launch_is_iteration = p.family == SFMBA_FAMILY_PCG_FAST && p.coarse;      // k_pcg_iter_fast MODE 2
    return p;
}

// the coarse set-up of the running solve
static void launch_cg_setup(hipStream_t s, const DenseSolver* ws, Profiler* prof) {
    switch (ws->run.path.family) {
    case SFMBA_FAMILY_PCG_FAST: pcg_fast_setup(s, ws, prof); break;
    case SFMBA_FAMILY_PCG_SEGMENTS: pcg_segments_setup(s, ws, prof); break;
    case SFMBA_FAMILY_PCG_SYMMETRIC: pcg_symmetric_setup(s, ws, prof); break;
    case SFMBA_FAMILY_PCG_STREAMING: pcg_streaming_setup(s, ws, prof); break;
    case SFMBA_FAMILY_PCG_SEGMENTS_STREAMING:
    case SFMBA_FAMILY_PCG_SEGMENTS_STREAMING_SPARSE: pcg_segments_streaming_setup(s, ws, prof); break;
    }
}

// one CG launch of the running solve (init = the first one)
static void launch_cg_iteration(hipStream_t s, const DenseSolver* ws, bool init, int anchor, double cap) {
    const DenseSolver::CgRun& r = ws->run;
    const int in = init ? 0 : (r.in | ((r.launched + 1) << 1));     // launch number 1.. of this solve, see k_pcg_iter
    switch (r.path.family) {
    case SFMBA_FAMILY_PCG_FAST: pcg_fast_iterate(s, ws, init, in, anchor, cap); break;
    case SFMBA_FAMILY_PCG_SEGMENTS: pcg_segments_iterate(s, ws, init, in, anchor, cap); break;
    case SFMBA_FAMILY_PCG_SYMMETRIC: pcg_symmetric_iterate(s, ws, init, in, anchor, cap); break;
    case SFMBA_FAMILY_PCG_STREAMING: pcg_streaming_iterate(s, ws, init, in, anchor, cap); break;
    case SFMBA_FAMILY_PCG_SEGMENTS_STREAMING:
    case SFMBA_FAMILY_PCG_SEGMENTS_STREAMING_SPARSE: pcg_segments_streaming_iterate(s, ws, init, in, anchor, cap); break;
    }
}

int dense_pcg_more(hipStream_t s, DenseSolver* ws, int n, Profiler* prof) {
    DenseSolver::CgRun& r = ws->run;
    n = std::min(n, r.max_iters - r.launched);
    if (n <= 0) return 0;
    ProfScope psb(prof, KID_PCG_ITER, s, n);
    for (int b = 0; b < n; ++b) {
        launch_cg_iteration(s, ws, false, 0, 1.0);
        r.in ^= 1;
        ++r.launched;
    }
    return n;
}

void dense_pcg_note(DenseSolver* ws, int hist_key, int iters) {
    ws->last_iters = iters;
    if (hist_key >= 0) {
        if (hist_key >= (int)ws->hist.size()) ws->hist.resize((size_t)hist_key + 1, 0);
        ws->hist[hist_key] = iters;
    }
}

// cap of the anchored stopping rule: every solve at least max(tol, 1e-4) relative
static double pcg_cap(double tol) { const double t2 = tol * tol; return t2 > 0.0 ? fmax(t2, 1e-8) / t2 : 1.0; }

int dense_pcg_transform(hipStream_t s, DenseSolver* ws, double* S, double* rhs, int* info_dev, Profiler* prof) {
    if (dense_pcg_ensure_workspace(ws)) return -1;
    const int ld = ws->ld, d = ws->d;
    const int nb6 = (d - 1) / 6, nB = nb6 + (d - 6 * nb6);
    ProfScope ps(prof, KID_PCG_SETUP, s);
    hipLaunchKernelGGL(k_pcg_blockchol, dim3((nB + 63) / 64), dim3(64), 0, s, S, ld, d, ws->binv, info_dev);
    if (pcg_reads_f32(ws)) hipLaunchKernelGGL(k_pcg_transform<float>, dim3((nB + 63) / 64, nB), dim3(64), 0, s, S, ld, d, ws->binv, rhs, ws->Sfull32, pcg_btilde(ws));
    else hipLaunchKernelGGL(k_pcg_transform<double>, dim3((nB + 63) / 64, nB), dim3(64), 0, s, S, ld, d, ws->binv, rhs, ws->Sfull, pcg_btilde(ws));
    return 0;
}

int dense_pcg_solve(hipStream_t s, DenseSolver* ws, double* S, double* rhs, double tol, int max_iters, int* info_dev, Profiler* prof, const PcgSolveOptions& o) {
    const int ld = ws->ld, d = ws->d;
    if (dense_pcg_ensure_workspace(ws)) return PCG_ERR_ALLOC;
    if (max_iters <= 0) max_iters = 4 * d;
    const CgPath path = dense_pcg_path(ws, o.coarse, o.segments);
    if (path.family == 0) return PCG_ERR_TOO_LARGE;          // before anything is enqueued
    if (!o.pretransformed) dense_pcg_transform(s, ws, S, rhs, info_dev, prof);
    DenseSolver::CgRun& run = ws->run;
    run.path = path;
    run.tol2 = tol * tol; run.in = 1; run.launched = 0; run.max_iters = max_iters; run.info = info_dev;
    ws->family = run.path.family; ws->coarse_vectors = run.path.coarse_vectors;        // (the step probe)
    const bool clean = hipPeekAtLastError() == hipSuccess;      // (the launch check of the waiting loop below can only speak for this solve's launches)
    launch_cg_setup(s, ws, prof);
    volatile int* mb = ws->h_mailbox;
    if (mb) { mb[0] = -1; mb[1] = 0; }
    { ProfScope ps(prof, KID_PCG_ITER, s);
      launch_cg_iteration(s, ws, true, o.anchor, pcg_cap(tol)); }
    const int first = run.path.first_launch_is_iteration ? 1 : 0;       // the merged first launch IS iteration 1 (max_iters counts it)
    run.launched = first;
    int batch = 24;
    constexpr int batch_extra = 1;
    // history + 1 (was + 2; +0.6 % on the headline): a solve that needs two more iterations than last time costs a host round trip, a surplus (early-exit) launch ~2 us
    // (run to 1e-12 -- AUTO -- a solve takes 13 +- 1 iterations from one call to the next, the atomics' summation order is enough: a batch one
    // launch short costs a host round trip of ~50 us, a surplus launch ~2: one more in reserve there)
    if (o.hist_key >= 0 && o.hist_key < (int)ws->hist.size() && ws->hist[o.hist_key] > 0) batch = ws->hist[o.hist_key] + batch_extra + (tol < 1e-10 ? 1 : 0) - first;
    if (o.no_wait) return dense_pcg_more(s, ws, batch, prof);
    bool done = false, waited = false;
    while (!done) {
        // (nothing left to launch BEFORE the first wait -- max_iters spent by a first launch that is an iteration --: what is in the queue is still waited for)
        const int more = dense_pcg_more(s, ws, batch, prof);
        if (more == 0 && waited) break;
        if (clean && hipPeekAtLastError() != hipSuccess) return PCG_ERR_LAUNCH;      // a refused launch posts nothing: no wait (the error stays for the caller's launches_ok())
        const int it = run.launched;
        if (mb) {
            // poll the mailbox until the last launch of the batch has reported (or convergence was posted)
            const double t_end = now_s() + 2.0;
            while (!(mb[1] != 0 || mb[0] >= it)) {
                if (now_s() > t_end) { (void)hipStreamSynchronize(s); break; }
            }
            __sync_synchronize();
            const int dn = mb[1];                    // 0, or the iterations of the finished solve + 1 (pcg_post): the count comes with the verdict
            done = dn != 0;
            ws->h_flags[PF_DONE] = done; ws->h_flags[PF_ITERS] = done ? dn - 1 : mb[0] >= 0 ? mb[0] : it;
        } else {
            (void)hipMemcpyAsync(ws->h_flags, ws->flags, 4 * sizeof(int), hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            done = ws->h_flags[PF_DONE] != 0;
        }
        waited = true;
        if (more == 0) break;
        batch = 8;
    }
    if (o.finish) { ProfScope ps(prof, KID_PCG_FINISH, s);
      hipLaunchKernelGGL(k_pcg_finish, dim3((d + 255) / 256), dim3(256), 0, s, d, ld, ws->vec, ws->binv, ws->flags, rhs); }
    dense_pcg_note(ws, o.hist_key, ws->h_flags[PF_ITERS]);
    return ws->h_flags[PF_ITERS];
}

// every device array of the workspace comes from here: the arena's, or a hipMalloc that dense_solver_destroy frees through ws->owned
template <typename T> static int ws_alloc(DenseSolver* ws, T** p, size_t bytes) {
    if (ws->arena) { *p = static_cast<T*>(ws->arena->alloc(bytes)); return *p ? 0 : -1; }
    if (hipMalloc(reinterpret_cast<void**>(p), bytes) != hipSuccess) return -1;
    ws->owned.push_back(*p);
    return 0;
}

float* dense_pcg_want_f32(DenseSolver* ws) {
    if (pcg_fast_fits(ws->d)) return nullptr;                    // the fast path is latency-bound: fp64 there
    if (!ws->Sfull32 && ws_alloc(ws, &ws->Sfull32, sizeof(float) * ((size_t)ws->d * ws->ld + pcg_tile_slack(ws->d, ws->ld)))) return nullptr;
    return ws->Sfull32;
}

int dense_pcg_ensure_workspace(DenseSolver* ws) {
    if (!ws->Sfull) {
        if (ws_alloc(ws, &ws->Sfull, sizeof(double) * ((size_t)ws->d * ws->ld + pcg_tile_slack(ws->d, ws->ld)))) return -1;
    }
    if (!ws->W) {
        if (ws_alloc(ws, &ws->W, sizeof(double) * ((size_t)PCG_NW * ws->ld + pcg_tile_slack(ws->d, ws->ld)))) return -1;
        if (ws_alloc(ws, &ws->AW, sizeof(double) * (size_t)PCG_NW * ws->ld)) return -1;
        if (ws_alloc(ws, &ws->epart, sizeof(double) * (size_t)(PCG_NW * PCG_NW + 2 * PCG_NW) * PCG_PART)) return -1;
        if (ws_alloc(ws, &ws->coarse, sizeof(double) * (size_t)(2 * PCG_NW * PCG_NW + PCG_NW))) return -1;
    }
    {
        if (!pcg_fast_fits(ws->d) && !ws->sym_tiles) {
            // tiles of the scalar upper triangle for k_sy_prod: SY_R rows x SY_C columns, columns aligned to SY_C
            std::vector<int4> tiles;
            for (int r0 = 0; r0 < ws->d; r0 += SY_R) {
                const int nrows = std::min(SY_R, ws->d - r0);
                for (int c0 = (r0 / SY_C) * SY_C; c0 < ws->d; c0 += SY_C) tiles.push_back(make_int4(r0, c0, nrows, c0 < r0 + nrows ? 1 : 0));
            }
            if (ws_alloc(ws, &ws->q3, sizeof(double) * 2 * (size_t)ws->ld)) return -1;
            if (ws_alloc(ws, &ws->sym_part, sizeof(double) * 2 * PCG_NPART * SY_SLOTS * SY_SLOT_STRIDE)) return -1;
            std::vector<int4> ctiles;
            for (int r0 = 0; r0 < ws->d; r0 += SY_CR) {
                const int nrows = std::min(SY_CR, ws->d - r0);
                for (int c0 = (r0 / SY_C) * SY_C; c0 < ws->d; c0 += SY_C) ctiles.push_back(make_int4(r0, c0, nrows, c0 < r0 + nrows ? 1 : 0));
            }
            if (ws_alloc(ws, &ws->sym_ctiles, sizeof(int4) * ctiles.size())) return -1;
            if (hipMemcpy(ws->sym_ctiles, ctiles.data(), sizeof(int4) * ctiles.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
            ws->sym_nctiles = (int)ctiles.size();
            // what the coarse set-up ADDS into with atomics (the caller's linearisation zeroes it: DeviceBuffers::pcg_zero = sym_zero / sym_zero_n)
            ws->sym_zero_n = (size_t)PCG_NW * ws->ld;
            if (ws_alloc(ws, &ws->sym_zero, sizeof(double) * (ws->sym_zero_n + pcg_tile_slack(ws->d, ws->ld)))) return -1;
            if (hipMemset(ws->sym_zero, 0, sizeof(double) * ws->sym_zero_n) != hipSuccess) return -1;
            ws->AWt = ws->sym_zero;
            if (ws_alloc(ws, &ws->sym_tiles, sizeof(int4) * tiles.size())) return -1;
            if (hipMemcpy(ws->sym_tiles, tiles.data(), sizeof(int4) * tiles.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
            ws->sym_ntiles = (int)tiles.size();
        }
    }
    if (!ws->mlAW && dense_pcg_segments_applicable(ws)) {
        const size_t nwg = (size_t)(ws->d - 1) / 6 + 1;
        if (ws_alloc(ws, &ws->mlAW, sizeof(double) * (size_t)ws->ld * ML_N)) return -1;
        if (ws_alloc(ws, &ws->mlV, sizeof(double) * nwg * PCG_NW * ML_N)) return -1;
        if (ws_alloc(ws, &ws->mlU, sizeof(double) * nwg * PCG_NW)) return -1;
        if (ws_alloc(ws, &ws->mlE, sizeof(double) * ML_N * ML_N)) return -1;
        if (ws_alloc(ws, &ws->mlEinv, sizeof(double) * ML_N * ML_N)) return -1;
        if (ws_alloc(ws, &ws->mlC0, sizeof(double) * ML_N)) return -1;
        if (ws_alloc(ws, &ws->mlState, sizeof(double) * 2 * 3 * ML_N)) return -1;
    }
    if (!ws->sgV && dense_pcg_segments_streaming_applicable(ws)) {
        const size_t ncp1 = (size_t)(ws->d - 1) / 6 + 1;
        if (ws_alloc(ws, &ws->sgV, sizeof(double) * ncp1 * PCG_NW * SG_NCP)) return -1;
        if (ws_alloc(ws, &ws->sgE, sizeof(double) * SG_NCP * SG_NCP)) return -1;
        if (ws_alloc(ws, &ws->sgEinv, sizeof(double) * SG_NCP * SG_NCP)) return -1;
        if (ws_alloc(ws, &ws->sgT, sizeof(double) * ncp1 * PCG_NW)) return -1;
        if (ws_alloc(ws, &ws->sgRR, sizeof(double) * SG_UWG)) return -1;
        if (ws_alloc(ws, &ws->sgState, sizeof(double) * 2 * SGS_LEN)) return -1;
    }
    return 0;
}

int dense_solver_create(DenseSolver* ws, int d, int ld, DeviceArena* arena, char* pinned) {
    ws->d = d; ws->ld = ld; ws->arena = arena;
    {   // what one workgroup may take of the LDS (a query; 160 KiB on gfx950): dense_pcg_path holds the families' requests against it
        int dev = 0, lds = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || lds <= 0) { (void)hipGetLastError(); lds = (int)PCG_LDS_DEFAULT; }
        ws->lds_limit = std::min((size_t)lds, PCG_LDS_GFX950);
    }
    const int nblk = ld / NB;
    if (ws_alloc(ws, &ws->minv, sizeof(double) * (size_t)nblk * NB * NB)) return -1;
    if (ws_alloc(ws, &ws->y, sizeof(double) * ld)) return -1;
    if (ws_alloc(ws, &ws->vec, sizeof(double) * (9 * (size_t)ld + pcg_tile_slack(d, ld)))) return -1;
    if (ws_alloc(ws, &ws->part, sizeof(double) * 2 * PCG_NPART * PCG_PART)) return -1;
    if (ws_alloc(ws, &ws->binv, sizeof(double) * 36 * (size_t)(ld / 6 + 2))) return -1;
    if (ws_alloc(ws, &ws->scal, sizeof(double) * (PS_STATE + 2 * PS_STATE_LEN))) return -1;
    if (ws_alloc(ws, &ws->flags, sizeof(int) * 4)) return -1;
    if (pinned) {
        ws->pinned_external = true;
        ws->h_flags = reinterpret_cast<int*>(pinned);
        ws->h_mailbox = reinterpret_cast<volatile int*>(pinned + 64);
    } else {
        if (hipHostMalloc(reinterpret_cast<void**>(&ws->h_flags), sizeof(int) * 4, hipHostMallocDefault) != hipSuccess) return -1;
        void* hm = nullptr;
        if (hipHostMalloc(&hm, sizeof(int) * 16, hipHostMallocMapped) != hipSuccess) return -1;
        ws->h_mailbox = static_cast<volatile int*>(hm);
    }
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&ws->d_mailbox), const_cast<int*>(ws->h_mailbox), 0) != hipSuccess) return -1;
    ws->Sfull = nullptr;
    return 0;
}

// dense_pcg_poison: rows of ld entries, `rows` of them, then `slack` entries; NaN at columns >= d, behind the rows, and (lower) below the diagonal
template <typename FT>
__global__ __launch_bounds__(256) void k_pcg_poison(int d, int ld, int rows, size_t slack, int lower, FT* __restrict__ F) {
    const size_t body = (size_t)rows * ld, n = body + slack;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t r = i / (size_t)ld, c = i - r * (size_t)ld;
        if (i >= body || c >= (size_t)d || (lower && c < r)) F[i] = (FT)__builtin_nan("");
    }
}

void dense_pcg_poison(hipStream_t s, DenseSolver* ws, bool lower) {
    const int d = ws->d, ld = ws->ld;
    const size_t slack = pcg_tile_slack(d, ld);
    const int nwg = (int)std::min<size_t>(4096, ((size_t)d * ld + slack + 255) / 256);
    if (pcg_reads_f32(ws)) hipLaunchKernelGGL(k_pcg_poison<float>, dim3(nwg), dim3(256), 0, s, d, ld, d, slack, lower ? 1 : 0, ws->Sfull32);
    else if (ws->Sfull) hipLaunchKernelGGL(k_pcg_poison<double>, dim3(nwg), dim3(256), 0, s, d, ld, d, slack, lower ? 1 : 0, ws->Sfull);
    if (ws->W) hipLaunchKernelGGL(k_pcg_poison<double>, dim3((PCG_NW * ld + (int)slack + 255) / 256), dim3(256), 0, s, d, ld, PCG_NW, slack, 0, ws->W);
}

void dense_solver_destroy(DenseSolver* ws) {
    for (void* q : ws->owned) (void)hipFree(q);          // (empty for a workspace that lives in an arena)
    if (!ws->pinned_external) {
        if (ws->h_flags) (void)hipHostFree(ws->h_flags);
        if (ws->h_mailbox) (void)hipHostFree(const_cast<int*>(ws->h_mailbox));
    }
    *ws = DenseSolver();
}

}  // namespace sfmba
