// pcg_segments.hip -- the segmented fast CG family: the fast path's geometry with one workgroup per camera and a coarse space of 57 hat-restricted
// gauge vectors (camera paths at d <= 1280).  Set-up k_ml_aw, k_ml_e, k_ml_invert; one launch per iteration (k_pcg_iter_ml).
#include "pcg_common.h"

namespace sfmba {

// ---------------------------------------------------------------------------------------------------------------------
// Segmented coarse space (d <= 1280): the gauge vectors restricted to SEGMENTS of the camera order.
//
// A reduced matrix that is sparsely filled is a camera graph of large diameter -- views along a path, tracks shared by neighbouring
// cameras (what SfM.cpp:366-469 builds).  Block-Jacobi CG then needs hundreds of iterations, and the eight GLOBAL gauge vectors remove
// only the eight smallest eigenvalues: the next few dozen are similarity transforms of PIECES of the path against each other
// (tools/coarse_space_study.py on cfg3_banded: 187 iterations with block-Jacobi alone, 117 with the 8 global vectors, 33 with the seven
// similarity vectors multiplied by eight hat functions along the cyclic camera order + the global focal/depth vector).  That coarse space,
// 7 G + 1 = 57 vectors, is what this path uses.  Nothing new is stored per vector: with workgroup j = camera j (six rows; the last
// workgroup = the focal row) and the hats a partition of unity with two non-zero hats per camera,
//      W~_(g,k) = hat_g(camera) * W~_k        (W~_k: the 8 vectors k_finalize writes)
//      W~_(g,k)^T q = sum_j hat_g(j) t_k(j),  t_k(j) = sum over camera j's rows of W~_k[row] q[row]
// so a workgroup still publishes NINE partial sums per iteration (p_r . q and t_0 .. t_7) exactly like the 8-vector path; what changes is
// how the next launch adds them up (per hat instead of over all workgroups), that the coarse state c, mu, p_mu (57 each) lives one entry
// per lane in every wave, and that E^-1 is 57 x 57: each wave forms a quarter of E^-1 g, one LDS exchange completes it.
// Set-up per linear solve: k_ml_aw (AW = S~ W~ for the 57 vectors, per-camera pieces of E and c_0), k_ml_e (E, c_0 summed per hat),
// k_ml_invert (Jacobi-scaled Gauss-Jordan in one workgroup, 57 pivot steps with one barrier each; a vanishing pivot drops its vector).
// ---------------------------------------------------------------------------------------------------------------------

// cameras whose LOWER hat is a: [ml_first_cam(a), ml_first_cam(a + 1)); camera j there has weight 1 - frac in hat a and frac in hat
// (a + 1) mod G, frac = (j G - a nc) / nc -- ONE formula for every place that needs a hat weight
__device__ __forceinline__ int ml_first_cam(int a, int nc) { return (a * nc + ML_G - 1) / ML_G; }
__device__ __forceinline__ double ml_frac(int j, int a, int nc, double inv_nc) { return (double)(j * ML_G - a * nc) * inv_nc; }

// sum over the cameras of hat g of weight * f(camera): the two ranges (which_range 0: cameras whose lower hat is g - 1, weight frac; 1: lower hat
// g, weight 1 - frac); `part` of `nparts` equal slices of the range.  Fixed order: deterministic.  MAXT bounds the terms of one slice: all of them
// are fetched before the first is used (clamped, branch-free -- a loop of load / use pairs pays one memory round trip per term).
template <int MAXT, typename Fn>
__device__ __forceinline__ double ml_hat_sum(int g, int nc, double inv_nc, int which_range, int part, int nparts, Fn f) {
    const int a = which_range == 0 ? (g + ML_G - 1) % ML_G : g;
    const int lo = ml_first_cam(a, nc), hi = ml_first_cam(a + 1, nc);
    const int len = hi - lo, chunk = (len + nparts - 1) / nparts;
    const int j0 = lo + part * chunk, j1 = min(hi, j0 + chunk);
    double s = 0.0;
    for (int jb = j0; jb < j1; jb += MAXT) {
        double val[MAXT];
#pragma unroll
        for (int t = 0; t < MAXT; ++t) val[t] = f(jb + t < j1 ? jb + t : j1 - 1);
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            const double fr = ml_frac(jb + t, a, nc, inv_nc);
            s = fma(jb + t < j1 ? (which_range == 0 ? fr : 1.0 - fr) : 0.0, val[t], s);
        }
    }
    return s;
}

// AW[row][64] = S~ W~ for the 57 vectors (own rows), V[wg][8][64] = sum over own rows of W~_k[row] AW[row][:], u[wg][8] = sum over own rows
// of W~_k[row] b~[row].  Workgroup = camera (last: the focal row).  The camera's six rows of S~ and W~_0..7 (fp32: lossless) go to LDS in one
// round trip; lane (g, k) of a wave then walks the cameras of hat g for the wave's two rows.
constexpr int ML_ROWLEN = 64 * PCG_CPL;
constexpr size_t ML_AW_LDS = sizeof(double) * 6 * ML_ROWLEN + sizeof(float) * PCG_NW * ML_ROWLEN + sizeof(double) * 4 * PCG_NW * ML_N;
__global__ __launch_bounds__(256) void k_ml_aw(int d, int ld, const double* __restrict__ F, const double* __restrict__ W, const double* __restrict__ bt,
                                               double* __restrict__ AW, double* __restrict__ V, double* __restrict__ U) {
    extern __shared__ __align__(16) double sm[];
    double* rows = sm;                                                   // [6][ML_ROWLEN]
    float* wt = reinterpret_cast<float*>(rows + 6 * ML_ROWLEN);          // [8][ML_ROWLEN]
    double* vbuf = reinterpret_cast<double*>(wt + PCG_NW * ML_ROWLEN);   // [4][8][64]
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nc = (d - 1) / 6;
    const double inv_nc = 1.0 / (double)nc;
    const int row0 = 6 * blockIdx.x, row1 = min(d, row0 + 6);
    {
        double2 rv[6][3];
        double wv[PCG_NW][PCG_EPT];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int c2 = tid + 256 * m;
                const bool ok = row0 + r < row1 && 2 * c2 < d;
                rv[r][m] = reinterpret_cast<const double2*>(F + (size_t)(row0 + r < row1 ? row0 + r : row0) * ld)[ok ? c2 : 0];
                if (!ok) rv[r][m] = make_double2(0.0, 0.0);
                if (2 * c2 + 1 >= d) rv[r][m].y = 0.0;
            }
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k)
#pragma unroll
            for (int m = 0; m < PCG_EPT; ++m) { const int e = tid + 256 * m; wv[k][m] = W[(size_t)k * ld + (e < d ? e : 0)]; }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int m = 0; m < 3; ++m) { const int c2 = tid + 256 * m; if (2 * c2 < ML_ROWLEN) reinterpret_cast<double2*>(rows + r * ML_ROWLEN)[c2] = rv[r][m]; }
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k)
#pragma unroll
            for (int m = 0; m < PCG_EPT; ++m) { const int e = tid + 256 * m; wt[k * ML_ROWLEN + e] = e < d ? (float)wv[k][m] : 0.0f; }
    }
    __syncthreads();
    const int g = lane / 7, k = lane - 7 * g;        // lanes 0..55: vector (g, k); lane 56: the global vector; beyond: nothing
    const int ra = w, rb = w + 4;                    // this wave's rows (of the camera's six)
    const bool have_a = row0 + ra < row1, have_b = row0 + rb < row1;
    double awa = 0.0, awb = 0.0;
    if (lane < 7 * ML_G) {
        const float* wk = wt + k * ML_ROWLEN;
        const double* Ra = rows + ra * ML_ROWLEN;
        const double* Rb = rows + (have_b ? rb : ra) * ML_ROWLEN;
        for (int range = 0; range < 2; ++range) {
            const int a = range == 0 ? (g + ML_G - 1) % ML_G : g;
            const int lo = ml_first_cam(a, nc), hi = ml_first_cam(a + 1, nc);
#pragma unroll 3
            for (int j = lo; j < hi; ++j) {               // (three cameras' LDS reads in flight)
                const double fr = ml_frac(j, a, nc, inv_nc);
                const double wgt = range == 0 ? fr : 1.0 - fr;
                const float2 w01 = reinterpret_cast<const float2*>(wk + 6 * j)[0], w23 = reinterpret_cast<const float2*>(wk + 6 * j)[1], w45 = reinterpret_cast<const float2*>(wk + 6 * j)[2];
                const double2 a0 = reinterpret_cast<const double2*>(Ra + 6 * j)[0], a1 = reinterpret_cast<const double2*>(Ra + 6 * j)[1], a2 = reinterpret_cast<const double2*>(Ra + 6 * j)[2];
                const double2 b0 = reinterpret_cast<const double2*>(Rb + 6 * j)[0], b1 = reinterpret_cast<const double2*>(Rb + 6 * j)[1], b2 = reinterpret_cast<const double2*>(Rb + 6 * j)[2];
                const double ta = fma(a0.x, (double)w01.x, fma(a0.y, (double)w01.y, fma(a1.x, (double)w23.x, fma(a1.y, (double)w23.y, fma(a2.x, (double)w45.x, a2.y * (double)w45.y)))));
                const double tb = fma(b0.x, (double)w01.x, fma(b0.y, (double)w01.y, fma(b1.x, (double)w23.x, fma(b1.y, (double)w23.y, fma(b2.x, (double)w45.x, b2.y * (double)w45.y)))));
                awa = fma(wgt, ta, awa);
                awb = fma(wgt, tb, awb);
            }
        }
    }
    {   // the global vector: all d columns, the lanes stride them
        double sa = 0.0, sb = 0.0;
        const float* w7 = wt + (PCG_NW - 1) * ML_ROWLEN;
        for (int c = lane; c < d; c += 64) { sa = fma(rows[ra * ML_ROWLEN + c], (double)w7[c], sa); sb = fma(rows[(have_b ? rb : ra) * ML_ROWLEN + c], (double)w7[c], sb); }
        sa = wave_allsum(sa); sb = wave_allsum(sb);
        if (lane == ML_NC - 1) { awa = sa; awb = sb; }
    }
    if (!have_a) awa = 0.0;
    if (!have_b) awb = 0.0;
    if (have_a) AW[(size_t)(row0 + ra) * ML_N + lane] = awa;
    if (have_b) AW[(size_t)(row0 + rb) * ML_N + lane] = awb;
#pragma unroll
    for (int q = 0; q < PCG_NW; ++q) {
        const double wa = have_a ? (double)wt[q * ML_ROWLEN + row0 + ra] : 0.0, wb = have_b ? (double)wt[q * ML_ROWLEN + row0 + rb] : 0.0;
        vbuf[(w * PCG_NW + q) * ML_N + lane] = fma(wa, awa, wb * awb);
    }
    __syncthreads();
    for (int e = tid; e < PCG_NW * ML_N; e += 256)
        V[(size_t)blockIdx.x * PCG_NW * ML_N + e] = (vbuf[e] + vbuf[PCG_NW * ML_N + e]) + (vbuf[2 * PCG_NW * ML_N + e] + vbuf[3 * PCG_NW * ML_N + e]);
    if (tid < PCG_NW) {
        double s = 0.0;
        for (int row = row0; row < row1; ++row) s = fma((double)wt[tid * ML_ROWLEN + row], bt[row], s);
        U[(size_t)blockIdx.x * PCG_NW + tid] = s;
    }
}

// E[i][:] and c_0[i]: row i = (g, k) is the hat-weighted sum of the cameras' pieces k; the last row the plain sum of piece 7 over all workgroups.
// One workgroup per row, lane = column, the terms split over the four waves.
__global__ __launch_bounds__(256) void k_ml_e(int d, const double* __restrict__ V, const double* __restrict__ U, double* __restrict__ E, double* __restrict__ c0) {
    __shared__ double eq[4][ML_N], cq[4];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nc = (d - 1) / 6;
    const double inv_nc = 1.0 / (double)nc;
    double e = 0.0, c = 0.0;
    if (i < 7 * ML_G) {
        const int g = i / 7, k = i - 7 * g;
        e = ml_hat_sum<16>(g, nc, inv_nc, w >> 1, w & 1, 2, [&](int j) { return V[((size_t)j * PCG_NW + k) * ML_N + lane]; });
        c = ml_hat_sum<16>(g, nc, inv_nc, w >> 1, w & 1, 2, [&](int j) { return U[(size_t)j * PCG_NW + k]; });
    } else {
        for (int jb = w; jb <= nc; jb += 64) {          // wave w: workgroups w, w + 4, ...; sixteen loads in flight
            double ve[16], vc[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int j = jb + 4 * t, jc = j <= nc ? j : nc;
                ve[t] = V[((size_t)jc * PCG_NW + (PCG_NW - 1)) * ML_N + lane]; vc[t] = U[(size_t)jc * PCG_NW + (PCG_NW - 1)];
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) { const bool ok = jb + 4 * t <= nc; e += ok ? ve[t] : 0.0; c += ok ? vc[t] : 0.0; }
        }
    }
    eq[w][lane] = e;
    if (lane == 0) cq[w] = c;
    __syncthreads();
    if (tid < ML_N) E[(size_t)i * ML_N + tid] = (eq[0][tid] + eq[1][tid]) + (eq[2][tid] + eq[3][tid]);
    if (tid == 0) c0[i] = (cq[0] + cq[1]) + (cq[2] + cq[3]);
}

// E^-1 (64 x 64, rows / columns beyond the 57 vectors and of dropped vectors zero): 4 x 4 tiles on 256 threads.  (History: the compiler REFUSED a 57-step
// `#pragma unroll` -- "loop not unrolled", dynamic register indices, 74 us; a column slice per thread with compile-time indices took 32 us.)
__global__ __launch_bounds__(256) void k_ml_invert(const double* __restrict__ E, double* __restrict__ einv, double* __restrict__ c0) {
    __shared__ double rowbuf[2 * ML_N], colbuf[2 * ML_N], sc[ML_N], diagbuf[2];
    __shared__ unsigned char drop[ML_N + 1];
    if (threadIdx.x >= ML_NC && threadIdx.x < ML_N) c0[threadIdx.x] = 0.0;
    gj_invert_tiled<ML_N, 4, 4, 4>(ML_NC, E, einv, rowbuf, colbuf, sc, diagbuf, drop);
}

// One CG iteration with the segmented coarse space: k_pcg_iter_fast's structure (every global load issued up front, one memory round trip per
// launch), workgroup = camera.  LDS behind the search direction: red[96] | tmp[7][256] (the partials t_0..t_6 of every workgroup) |
// gq[4][64] (quarter sums of W~^T q per wave) | egq[4][64] (quarter products of E^-1 g per wave).
template <bool INIT>
__global__ __launch_bounds__(256) void k_pcg_iter_ml(int d, int ld, const double* __restrict__ F, double* __restrict__ vec,
                                                     const double* __restrict__ bt, double* __restrict__ part, double* __restrict__ scal,
                                                     int* flags, double tol2, int in, int* info, int* mailbox, int anchor, double cap,
                                                     const double* __restrict__ W, const double* __restrict__ AW, const double* __restrict__ einv,
                                                     const double* __restrict__ c0, double* __restrict__ mlstate) {
    extern __shared__ __align__(16) double sm[];
    double* pl = sm;
    double* red = sm + ld;
    double* tmp = red + 96;
    double* gq = tmp + 7 * 256;
    double* egq = gq + 4 * ML_N;
    const int seq = in >> 1;
    in &= 1;
    if (!INIT) { const int dn = flags[PF_DONE]; if (dn != 0 && seq >= dn) return; }
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), out = in ^ 1;
    const int nc = (d - 1) / 6, nwg = (int)gridDim.x;
    const double inv_nc = 1.0 / (double)nc;
    const int row0 = 6 * blockIdx.x, row1 = min(d, row0 + 6);
    const double* x_in = pcg_vec(vec, 0, in, ld); const double* r_in = INIT ? bt : pcg_vec(vec, 1, in, ld);
    const double* p_in = pcg_vec(vec, 2, in, ld); const double* q_in = pcg_vec(vec, 3, in, ld);
    double* x_out = pcg_vec(vec, 0, out, ld); double* r_out = pcg_vec(vec, 1, out, ld);
    double* p_out = pcg_vec(vec, 2, out, ld); double* q_out = pcg_vec(vec, 3, out, ld);
    const double* st_in = scal + PS_STATE + PS_STATE_LEN * in;
    double* st_out = scal + PS_STATE + PS_STATE_LEN * out;
    const double* ms_in = mlstate + 3 * ML_N * in;
    double* ms_out = mlstate + 3 * ML_N * out;

    // ---- all global loads of this iteration ----
    double rv[PCG_EPT], qv[PCG_EPT], pv[PCG_EPT];
#pragma unroll
    for (int m = 0; m < PCG_EPT; ++m) {
        const int e = tid + 256 * m;
        const bool ok = e < d;
        rv[m] = ok ? r_in[e] : 0.0; qv[m] = (ok && !INIT) ? q_in[e] : 0.0; pv[m] = (ok && !INIT) ? p_in[e] : 0.0;
    }
    double pp[PCG_NPART];                          // the nine partial sums workgroup `tid` published (clamped, branch-free)
#pragma unroll
    for (int v = 0; v < PCG_NPART; ++v) {
        const double t = INIT ? 0.0 : pcg_part(part, in, v)[tid < nwg ? tid : nwg - 1];
        pp[v] = tid < nwg ? t : 0.0;
    }
    double em[16];                                 // E^-1[16 w + jj][lane] (symmetric: = row `lane`, this wave's quarter of the columns)
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) em[jj] = einv[(size_t)(16 * w + jj) * ML_N + lane];
    const double c_in = INIT ? c0[lane] : ms_in[lane];
    const double mu_in = INIT ? 0.0 : ms_in[ML_N + lane];
    const double pmu_in = INIT ? 0.0 : ms_in[2 * ML_N + lane];
    const double rr0 = INIT ? 0.0 : scal[PS_RR0];
    const double rz_in = INIT ? 0.0 : st_in[PS_RZ];
    const int eo = row0 + (tid - 192);
    const bool own = tid >= 192 && eo < row1;
    double xo = 0.0, po = 0.0, ro = 0.0, qo = 0.0, wo[PCG_NW];
    if (own) { ro = r_in[eo]; if (!INIT) { xo = x_in[eo]; po = p_in[eo]; qo = q_in[eo]; } }
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k) wo[k] = (own && !INIT) ? W[(size_t)k * ld + eo] : 0.0;
    double2 fv[PCG_RPW][PCG_CPL / 2];
    double awv[PCG_RPW], wg8[PCG_RPW];             // AW[row][lane]; W~_(lane & 7)[row]
#pragma unroll
    for (int k = 0; k < PCG_RPW; ++k) {
        const int row = row0 + w + 4 * k;
        const bool have = row < row1;
        const double2* Fr = reinterpret_cast<const double2*>(F + (size_t)(have ? row : row0) * ld);
#pragma unroll
        for (int m = 0; m < PCG_CPL / 2; ++m) {
            const int c2 = lane + 64 * m;
            double2 v = make_double2(0.0, 0.0);
            if (have && 2 * c2 < d) v = Fr[c2];
            if (2 * c2 + 1 >= d) v.y = 0.0;
            fv[k][m] = v;
        }
        awv[k] = have ? AW[(size_t)row * ML_N + lane] : 0.0;
        wg8[k] = have ? W[(size_t)(lane & 7) * ld + row] : 0.0;
    }
    double c_new, mu_new, pmu_new, rz_new;
    if (INIT) {
        // x0 = 0, r0 = b~, c0 = W~^T b~ (k_ml_e), mu0 = E^-1 c0, z0 = r0 + W~ mu0, p0 = z0
        double rr = 0.0;
#pragma unroll
        for (int m = 0; m < PCG_EPT; ++m) rr += rv[m] * rv[m];
        rr = wave_allsum(rr);
        if (lane == 0) red[16 + w] = rr;
        double e = 0.0;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) e = fma(em[jj], lane_bcast(c_in, 16 * w + jj), e);
        egq[w * ML_N + lane] = e;
        __syncthreads();
        rr = red[16] + red[17] + red[18] + red[19];
        c_new = c_in;
        mu_new = (egq[lane] + egq[ML_N + lane]) + (egq[2 * ML_N + lane] + egq[3 * ML_N + lane]);
        rz_new = rr + wave_allsum(c_new * mu_new);
        pmu_new = mu_new;
#pragma unroll
        for (int m = 0; m < PCG_EPT; ++m) { const int e2 = tid + 256 * m; if (e2 < d) pl[e2] = rv[m]; }
        if (own) { x_out[eo] = 0.0; r_out[eo] = ro; p_out[eo] = ro; }
        if (blockIdx.x == 0 && tid == 0) {
            scal[PS_RR0] = pcg_threshold_base(rr, scal, anchor, cap); flags[PF_DONE] = (rr == 0.0); flags[PF_ITERS] = 0; flags[PF_XBUF] = out;
            if (mailbox && rr == 0.0) pcg_post(mailbox, 0, 1);
        }
    } else {
        // ---- p_r . q and t_7 over all workgroups (registers), t_0..t_6 per hat (through LDS) ----
#pragma unroll
        for (int v = 1; v < PCG_NW; ++v) tmp[(v - 1) * 256 + tid] = pp[v];
        {
            const double a = wave_allsum(pp[0]), b = wave_allsum(pp[PCG_NW]);
            if (lane == 0) { red[w] = a; red[4 + w] = b; }
        }
        __syncthreads();
        {
            // wave 0, 1: the two halves of the hat's lower range (cameras whose lower hat is g - 1); wave 2, 3: of its upper range
            double s = 0.0;
            if (lane < 7 * ML_G) {
                const int g = lane / 7, k = lane - 7 * g;
                const double* tk = tmp + k * 256;
                s = ml_hat_sum<8>(g, nc, inv_nc, w >> 1, w & 1, 2, [&](int j) { return tk[j]; });
            }
            gq[w * ML_N + lane] = s;
        }
        __syncthreads();
        double g = (gq[lane] + gq[ML_N + lane]) + (gq[2 * ML_N + lane] + gq[3 * ML_N + lane]);
        if (lane == ML_NC - 1) g = (red[4] + red[5]) + (red[6] + red[7]);
        const double pq = (red[0] + red[1]) + (red[2] + red[3]) + wave_allsum(pmu_in * g);
        const double alpha = rz_in * fast_rcp(pq);
        {
            double e = 0.0;                                // this wave's quarter of E^-1 g (independent of alpha)
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) e = fma(em[jj], lane_bcast(g, 16 * w + jj), e);
            egq[w * ML_N + lane] = e;
        }
        double rrn = 0.0;
#pragma unroll
        for (int m = 0; m < PCG_EPT; ++m) { rv[m] -= alpha * qv[m]; rrn += rv[m] * rv[m]; }
        rrn = wave_allsum(rrn);
        if (lane == 0) red[16 + w] = rrn;
        if (w == 3) {                                      // x += alpha (p_r + W~ p_mu): this camera's two hats
            const int jc = min((int)blockIdx.x, nc - 1);   // (the focal row: only W~_7 is non-zero there)
            const int gl = (jc * ML_G) / nc, gh = gl + 1 == ML_G ? 0 : gl + 1;
            const double fr = ml_frac(jc, gl, nc, inv_nc);
            double wp = wo[PCG_NW - 1] * lane_bcast(pmu_in, ML_NC - 1);
#pragma unroll
            for (int k = 0; k < 7; ++k)
                wp = fma(wo[k], fma(fr, lane_bcast(pmu_in, 7 * gh + k), (1.0 - fr) * lane_bcast(pmu_in, 7 * gl + k)), wp);
            if (own) x_out[eo] = xo + alpha * (po + wp);
        }
        __syncthreads();
        const double Eg = (egq[lane] + egq[ML_N + lane]) + (egq[2 * ML_N + lane] + egq[3 * ML_N + lane]);
        c_new = fma(-alpha, g, c_in);
        mu_new = fma(-alpha, Eg, mu_in);
        rrn = red[16] + red[17] + red[18] + red[19];
        rz_new = rrn + wave_allsum(c_new * mu_new);
        const bool broke = !(pq > 0.0) || !(rrn == rrn);
        const bool done = rrn <= tol2 * rr0 || broke;
        if (done) {
            if (blockIdx.x == 0 && tid == 0) {
                flags[PF_DONE] = seq + 1; flags[PF_XBUF] = out; const int it = flags[PF_ITERS] + 1; flags[PF_ITERS] = it;
                if (broke) atomicCAS(info, 0, d + 1);
                if (mailbox) pcg_post(mailbox, it, 1);
            }
            return;
        }
        const double beta = rz_new * fast_rcp(rz_in);
        pmu_new = fma(beta, pmu_in, mu_new);
#pragma unroll
        for (int m = 0; m < PCG_EPT; ++m) { const int e = tid + 256 * m; if (e < d) pl[e] = rv[m] + beta * pv[m]; }
        if (own) { const double rn = ro - alpha * qo; r_out[eo] = rn; p_out[eo] = rn + beta * po; }
        if (blockIdx.x == 0 && tid == 0) { const int it = flags[PF_ITERS] + 1; flags[PF_ITERS] = it; flags[PF_XBUF] = out; if (mailbox) pcg_post(mailbox, it, 0); }
    }
    if (blockIdx.x == 0 && w == 1) {
        ms_out[lane] = c_new; ms_out[ML_N + lane] = mu_new; ms_out[2 * ML_N + lane] = pmu_new;
        if (lane == 0) st_out[PS_RZ] = rz_new;
    }
    __syncthreads();
    // ---- q = S~ p_r + AW p_mu for the rows of this camera ----
    double pqp = 0.0, gacc = 0.0;
#pragma unroll
    for (int k = 0; k < PCG_RPW; ++k) {
        const int row = row0 + w + 4 * k;
        double sacc = awv[k] * pmu_new, sacc2 = 0.0;
#pragma unroll
        for (int m = 0; m < PCG_CPL / 2; ++m) {
            const int c2 = lane + 64 * m;
            double2 pv2 = (2 * c2 < d) ? reinterpret_cast<const double2*>(pl)[c2] : make_double2(0.0, 0.0);
            if (2 * c2 + 1 >= d) pv2.y = 0.0;
            sacc = fma(fv[k][m].x, pv2.x, sacc);
            sacc2 = fma(fv[k][m].y, pv2.y, sacc2);
        }
        sacc += sacc2;
        sacc = wave_allsum(sacc);
        if (lane == 0 && row < row1) { q_out[row] = sacc; pqp += pl[row] * sacc; }
        if (lane >= PCG_NW && lane < 2 * PCG_NW && row < row1) gacc = fma(wg8[k], sacc, gacc);
    }
    if (lane == 0) red[40 + 9 * w] = pqp;
    if (lane >= PCG_NW && lane < 2 * PCG_NW) red[40 + 9 * w + 1 + (lane - PCG_NW)] = gacc;
    __syncthreads();
    if (tid < PCG_NPART) pcg_part(part, out, tid)[blockIdx.x] = red[40 + tid] + red[49 + tid] + red[58 + tid] + red[67 + tid];
}

void pcg_segments_setup(hipStream_t s, const DenseSolver* ws, Profiler* prof) {
    const CgPath& r = ws->run.path;
    ProfScope ps(prof, KID_PCG_SETUP, s, 3);
    static bool ml_attr_set = false;
    if (!ml_attr_set) { (void)hipFuncSetAttribute((const void*)k_ml_aw, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ML_AW_LDS); ml_attr_set = true; }
    hipLaunchKernelGGL(k_ml_aw, dim3(r.nwg), dim3(256), ML_AW_LDS, s, ws->d, ws->ld, ws->Sfull, ws->W, pcg_btilde(ws), ws->mlAW, ws->mlV, ws->mlU);
    hipLaunchKernelGGL(k_ml_e, dim3(ML_NC), dim3(256), 0, s, ws->d, ws->mlV, ws->mlU, ws->mlE, ws->mlC0);
    hipLaunchKernelGGL(k_ml_invert, dim3(1), dim3(256), 0, s, ws->mlE, ws->mlEinv, ws->mlC0);
}

void pcg_segments_iterate(hipStream_t s, const DenseSolver* ws, bool init, int in, int anchor, double cap) {
    const DenseSolver::CgRun& run = ws->run;
    const CgPath& r = run.path;
#define SFMBA_IT(INIT) hipLaunchKernelGGL((k_pcg_iter_ml<INIT>), dim3(r.nwg), dim3(256), r.lds, s, ws->d, ws->ld, ws->Sfull, ws->vec, pcg_btilde(ws), ws->part, ws->scal, ws->flags, \
        run.tol2, in, run.info, ws->d_mailbox, anchor, cap, ws->W, ws->mlAW, ws->mlEinv, ws->mlC0, ws->mlState)
    if (init) SFMBA_IT(true); else SFMBA_IT(false);
#undef SFMBA_IT
}

}  // namespace sfmba
