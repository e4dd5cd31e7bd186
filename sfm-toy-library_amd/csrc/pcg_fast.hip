// pcg_fast.hip -- the fast CG family (d <= 1280: every BASELINE single-GPU configuration): a workgroup's rows of S~ in registers, one launch per
// iteration (k_pcg_iter_fast), the 8-vector coarse set-up in one (k_pcg_coarse_fast; the first CG launch inverts E itself).  Also home of k_pcg_coarse_invert, that inversion as a launch of its own for the
// streaming and the symmetric family (see there for why it lives here).
#include "pcg_common.h"

namespace sfmba {

// Fast path of one CG iteration for d <= 1280 (all BASELINE single-GPU configs): every global load of
// the iteration -- the three length-d vectors, the partial sums and this wave's rows of S~ --
// is issued up front into registers, so the launch pays ONE memory round trip; the rest is LDS + ALU.
// The special roles are spread over the waves (wave 0..3: partial sums; last wave: this workgroup's own rows of x, r, p_r) and
// everything about the 8-dimensional coarse space that does not need alpha (E^-1 g) is formed while alpha is on its way.

// MODE 0: an iteration.  MODE 1: the first launch of a solve without a coarse space (x0 = 0, r0 = p0 = b~, the product).  MODE 2: the first launch
// WITH the coarse space, which is also the first ITERATION: k_pcg_coarse_fast left t = S~ b~ (in the q buffer), AW, and the partials of E, c_0 and
// W~^T t; with p_r0 = b~ and p_mu0 = E^-1 c_0 the first product is q_0 = t + AW p_mu0 and W~^T q_0 = W~^T t + E p_mu0 -- nothing of it needs a pass
// over S~, so the launch that used to do only the initialisation and that product (10.7 us) is gone and this one (E^-1 by one wave, then a regular
// iteration) takes its place.
template <int MODE, bool COARSE>
__global__ __launch_bounds__(256) void k_pcg_iter_fast(int d, int ld, const double* __restrict__ F, double* __restrict__ vec,
                                                       const double* __restrict__ bt, double* __restrict__ part, double* __restrict__ scal,
                                                       int* flags, int rows_per_wg, double tol2, int in, int* info, int* mailbox, int anchor, double cap,
                                                       const double* __restrict__ W, const double* __restrict__ AW, double* __restrict__ coarse,
                                                       const double* __restrict__ epart) {
    extern __shared__ __align__(16) double sm[];
    double* pl = sm;
    double* red = sm + ld;
    // `in` = (launch number << 1) | parity.  PF_DONE holds the first launch number that has nothing left to do: a launch must not act
    // on the flag its own workgroup 0 raises (workgroups that start late, e.g. behind another process's kernels, would skip the
    // converging iteration's x update).
    constexpr bool INIT = MODE == 1, FIRST = MODE == 2;
    static_assert(!FIRST || COARSE, "the merged first launch exists for the coarse space only");
    const int seq = in >> 1;
    in &= 1;
    if (MODE == 0) { const int dn = flags[PF_DONE]; if (dn != 0 && seq >= dn) return; }
    constexpr int NV = COARSE ? PCG_NPART : 1;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, out = in ^ 1;
    // first launch of a solve: E^-1 and c_0 from the partials k_pcg_coarse_fast left behind -- formed by EVERY workgroup for
    // itself (no launch of its own: the 8 x 8 inversion is ~3 us of one wave), published by workgroup 0 for the launches that follow
    if (INIT && COARSE) coarse_sum_partials((int)gridDim.x, epart, red + 144);
    if (FIRST) coarse_sum_partials<20>((int)gridDim.x, epart, red + 144);
    const int row0 = blockIdx.x * rows_per_wg;
    const int row1 = min(d, row0 + rows_per_wg);
    const int nwg = (int)gridDim.x;
    const double* x_in = pcg_vec(vec, 0, in, ld); const double* r_in = (INIT || FIRST) ? bt : pcg_vec(vec, 1, in, ld);
    const double* p_in = FIRST ? bt : pcg_vec(vec, 2, in, ld); const double* q_in = pcg_vec(vec, 3, in, ld);
    double* x_out = pcg_vec(vec, 0, out, ld); double* r_out = pcg_vec(vec, 1, out, ld);
    double* p_out = pcg_vec(vec, 2, out, ld); double* q_out = pcg_vec(vec, 3, out, ld);
    const double* st_in = scal + PS_STATE + PS_STATE_LEN * in;
    double* st_out = scal + PS_STATE + PS_STATE_LEN * out;

    // ---- all global loads of this iteration ----
    double rv[PCG_EPT], qv[PCG_EPT], pv[PCG_EPT];
#pragma unroll
    for (int m = 0; m < PCG_EPT; ++m) {
        const int e = tid + 256 * m;
        const bool ok = e < d;
        rv[m] = ok ? r_in[e] : 0.0; qv[m] = (ok && !INIT) ? q_in[e] : 0.0; pv[m] = FIRST ? rv[m] : (ok && !INIT) ? p_in[e] : 0.0;      // (first launch: p_r0 = r_0 = b~)
    }
    double mine[3] = { 0.0, 0.0, 0.0 };           // partial sums of the previous launch: wave w owns values w, w + 4, w + 8
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int v = w + 4 * j;
        if (MODE == 0 && 4 * j < NV) {
            // branch-free, clamped: a conditional `+= load` makes the compiler wait for every load in turn (measured: twelve
            // dependent memory round trips, +3 us per iteration)
            const double* pp = pcg_part(part, in, v < NV ? v : 0);
            double t[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { const int wg = lane + 64 * i; t[i] = pp[wg < nwg ? wg : nwg - 1]; }
#pragma unroll
            for (int i = 0; i < 4; ++i) mine[j] += (lane + 64 * i < nwg && v < NV) ? t[i] : 0.0;
        }
    }
    const double einv_mine = (COARSE && MODE == 0 && tid < PCG_NW * PCG_NW) ? coarse[tid] : 0.0;
    double rr0 = MODE == 0 ? scal[PS_RR0] : 0.0;
    double rz_in = MODE == 0 ? st_in[PS_RZ] : 0.0;
    const double rrf = (FIRST && anchor == 2) ? scal[PS_RRF] : 0.0;
    double c_in[PCG_NW], mu_in[PCG_NW], pmu_in[PCG_NW];
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k) {
        c_in[k] = (COARSE && MODE == 0) ? st_in[PS_C + k] : 0.0;
        mu_in[k] = (COARSE && MODE == 0) ? st_in[PS_MU + k] : 0.0;
        pmu_in[k] = (COARSE && MODE == 0) ? st_in[PS_PMU + k] : 0.0;
    }
    // own rows (the last wave's lanes < rows): what the x update and the stores of r, p_r need
    const int eo = row0 + (tid - 192);
    const bool own = tid >= 192 && eo < row1;
    double xo = 0.0, po = 0.0, ro = 0.0, qo = 0.0, wo[PCG_NW];
    if (own) { ro = r_in[eo]; if (MODE == 0) { xo = x_in[eo]; po = p_in[eo]; qo = q_in[eo]; } if (FIRST) { po = ro; qo = q_in[eo]; } }
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k) wo[k] = (COARSE && own && !INIT) ? W[(size_t)k * ld + eo] : 0.0;
    double aw5[FIRST ? PCG_EPT : 1][PCG_NW], awo[PCG_NW];     // first launch: AW[e][:] for q_0 = t + AW p_mu0
    if (FIRST) {
#pragma unroll
        for (int m = 0; m < PCG_EPT; ++m) {
            const int e = tid + 256 * m;
#pragma unroll
            for (int k = 0; k < PCG_NW; ++k) { const double v = AW[(size_t)(e < d ? e : 0) * PCG_NW + k]; aw5[m][k] = e < d ? v : 0.0; }
        }
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) awo[k] = own ? AW[(size_t)eo * PCG_NW + k] : 0.0;
    }
    double2 fv[PCG_RPW][PCG_CPL / 2];          // 16-byte loads: lane takes columns 2*(lane + 64 m), +1
    double awv[PCG_RPW];                       // lanes 0..7: AW[row][lane]; lanes 8..15: W~[lane - 8][row]
#pragma unroll
    for (int k = 0; k < PCG_RPW; ++k) {
        const int row = row0 + w + 4 * k;
        const double2* Fr = reinterpret_cast<const double2*>(F + (size_t)(row < row1 ? row : row0) * ld);
#pragma unroll
        for (int m = 0; m < PCG_CPL / 2; ++m) {
            const int c2 = lane + 64 * m;
            double2 v = make_double2(0.0, 0.0);
            if (row < row1 && 2 * c2 < d) v = Fr[c2];
            if (2 * c2 + 1 >= d) v.y = 0.0;                 // padding column: never multiply garbage
            fv[k][m] = v;
        }
        awv[k] = 0.0;
        if (COARSE && row < row1 && lane < 2 * PCG_NW) awv[k] = lane < PCG_NW ? AW[(size_t)row * PCG_NW + lane] : W[(size_t)(lane - PCG_NW) * ld + row];
    }
    if (COARSE && MODE == 0 && tid < PCG_NW * PCG_NW) red[80 + tid] = einv_mine;
    double c_new[PCG_NW], mu_new[PCG_NW], pmu_new[PCG_NW];
    double rz_new;
    if (INIT) {
        if (COARSE) {
            __syncthreads();                              // E, c_0 complete in red[144 ..)
            if (w == 0) {
                const double e = coarse_invert_wave(red + 144, red + 224, red + 288);
                red[80 + lane] = e;
                if (blockIdx.x == 0) { coarse[lane] = e; if (lane < PCG_NW) coarse[PCG_NW * PCG_NW + lane] = red[144 + PCG_NW * PCG_NW + lane]; }
            }
        }
        // x0 = 0, r0 = b~, z0 = r0 + W~ E^-1 c0, p0 = z0
        double rr = 0.0;
#pragma unroll
        for (int m = 0; m < PCG_EPT; ++m) rr += rv[m] * rv[m];
        rr = wave_allsum(rr);
        if (lane == 0) red[16 + w] = rr;
        __syncthreads();
        rr = red[16] + red[17] + red[18] + red[19];
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) { c_new[k] = COARSE ? red[144 + PCG_NW * PCG_NW + k] : 0.0; mu_new[k] = 0.0; }
        if (COARSE) einv_apply(red + 80, c_new, mu_new);
        rz_new = rr + (COARSE ? dot8(c_new, mu_new) : 0.0);
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) pmu_new[k] = mu_new[k];
#pragma unroll
        for (int m = 0; m < PCG_EPT; ++m) { const int e = tid + 256 * m; if (e < d) pl[e] = rv[m]; }
        if (own) { x_out[eo] = 0.0; r_out[eo] = ro; p_out[eo] = ro; }
        if (blockIdx.x == 0 && tid == 0) {
            scal[PS_RR0] = pcg_threshold_base(rr, scal, anchor, cap); flags[PF_DONE] = (rr == 0.0); flags[PF_ITERS] = 0; flags[PF_XBUF] = out;
            if (mailbox && rr == 0.0) pcg_post(mailbox, 0, 1);
        }
    } else {
        double g[PCG_NW], Eg[PCG_NW];
        double pq;
        if (FIRST) {
            __syncthreads();                              // E, c_0, W~^T t complete in red[144 .. 224)
            if (w == 0) {
                const double e = coarse_invert_wave(red + 144, red + 224, red + 288);
                red[80 + lane] = e;
                if (blockIdx.x == 0) { coarse[lane] = e; if (lane < PCG_NW) coarse[PCG_NW * PCG_NW + lane] = red[144 + PCG_NW * PCG_NW + lane]; }
            }
            double rr = 0.0;
#pragma unroll
            for (int m = 0; m < PCG_EPT; ++m) rr += rv[m] * rv[m];
            rr = wave_allsum(rr);
            if (lane == 0) red[16 + w] = rr;
            __syncthreads();                              // E^-1 in red[80 .. 144), |b~|^2
            rr = red[16] + red[17] + red[18] + red[19];
            if (rr == 0.0) {                              // b~ = 0: x = 0 is the solution
                if (own) x_out[eo] = 0.0;
                if (blockIdx.x == 0 && tid == 0) {
                    scal[PS_RR0] = pcg_threshold_base(rr, scal, anchor, cap); flags[PF_DONE] = seq + 1; flags[PF_ITERS] = 0; flags[PF_XBUF] = out;
                    if (mailbox) pcg_post(mailbox, 0, 1);
                }
                return;
            }
            // c_0, mu_0 = E^-1 c_0 = p_mu0; q_0 = t + AW p_mu0; W~^T q_0 = W~^T t + E p_mu0; r_0 . z_0 = |b~|^2 + c_0 . mu_0
#pragma unroll
            for (int k = 0; k < PCG_NW; ++k) { c_in[k] = red[144 + PCG_NW * PCG_NW + k]; mu_in[k] = 0.0; }
            einv_apply(red + 80, c_in, mu_in);
#pragma unroll
            for (int k = 0; k < PCG_NW; ++k) pmu_in[k] = mu_in[k];
            rz_in = rr + dot8(c_in, mu_in);
            rr0 = anchor == 2 ? fmin(fmax(rr, rrf), cap * rr) : rr;          // pcg_threshold_base, without its store
            if (blockIdx.x == 0 && tid == 0) scal[PS_RR0] = pcg_threshold_base(rr, scal, anchor, cap);
#pragma unroll
            for (int k = 0; k < PCG_NW; ++k) {
                double erow[PCG_NW];
#pragma unroll
                for (int j = 0; j < PCG_NW; ++j) erow[j] = red[144 + PCG_NW * k + j];
                g[k] = red[144 + PCG_NW * PCG_NW + PCG_NW + k] + dot8(erow, pmu_in);
                Eg[k] = 0.0;
            }
            double pqr = 0.0;
#pragma unroll
            for (int m = 0; m < PCG_EPT; ++m) { qv[m] += dot8(aw5[m], pmu_in); pqr = fma(pv[m], qv[m], pqr); }     // (elements beyond d: all zero)
            qo += dot8(awo, pmu_in);
            pqr = wave_allsum(pqr);
            if (lane == 0) red[20 + w] = pqr;
            __syncthreads();
            pq = (red[20] + red[21]) + (red[22] + red[23]) + dot8(pmu_in, g);
        } else {
            reduce_partials<NV>(mine, red);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < PCG_NW; ++k) { g[k] = COARSE ? red[1 + k] : 0.0; Eg[k] = 0.0; }
            pq = red[0] + (COARSE ? dot8(pmu_in, g) : 0.0);
        }
        const double alpha = rz_in * fast_rcp(pq);       // rcp + 2 Newton steps: the generic fp64 division is a ~15-deep dependent chain on the critical path
        if (COARSE) einv_apply(red + 80, g, Eg);          // independent of alpha: overlaps the reciprocal
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) { c_new[k] = fma(-alpha, g[k], c_in[k]); mu_new[k] = fma(-alpha, Eg[k], mu_in[k]); }
        double rrn = 0.0;
#pragma unroll
        for (int m = 0; m < PCG_EPT; ++m) { rv[m] -= alpha * qv[m]; rrn += rv[m] * rv[m]; }
        rrn = wave_allsum(rrn);
        if (lane == 0) red[16 + w] = rrn;
        const double cmu = COARSE ? dot8(c_new, mu_new) : 0.0;
        if (own) {                                       // x += alpha (p_r + W~ p_mu)
            x_out[eo] = xo + alpha * (po + (COARSE ? dot8(wo, pmu_in) : 0.0));
        }
        __syncthreads();
        rrn = red[16] + red[17] + red[18] + red[19];
        rz_new = rrn + cmu;
        const bool broke = !(pq > 0.0) || !(rrn == rrn);
        const bool done = rrn <= tol2 * rr0 || broke;
        if (done) {
            if (blockIdx.x == 0 && tid == 0) {
                flags[PF_DONE] = seq + 1; flags[PF_XBUF] = out; const int it = FIRST ? 1 : flags[PF_ITERS] + 1; flags[PF_ITERS] = it;
                if (broke) atomicCAS(info, 0, d + 1);
                if (mailbox) pcg_post(mailbox, it, 1);
            }
            return;
        }
        const double beta = rz_new * fast_rcp(rz_in);
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) pmu_new[k] = fma(beta, pmu_in[k], mu_new[k]);
#pragma unroll
        for (int m = 0; m < PCG_EPT; ++m) { const int e = tid + 256 * m; if (e < d) pl[e] = rv[m] + beta * pv[m]; }
        if (own) { const double rn = ro - alpha * qo; r_out[eo] = rn; p_out[eo] = rn + beta * po; }
        if (blockIdx.x == 0 && tid == 0) {
            const int it = FIRST ? 1 : flags[PF_ITERS] + 1; flags[PF_ITERS] = it; flags[PF_XBUF] = out; if (FIRST) flags[PF_DONE] = 0;
            if (mailbox) pcg_post(mailbox, it, 0);
        }
    }
    if (blockIdx.x == 0 && tid == 64) {
        st_out[PS_RZ] = rz_new;
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) { st_out[PS_C + k] = c_new[k]; st_out[PS_MU + k] = mu_new[k]; st_out[PS_PMU + k] = pmu_new[k]; }
    }
    if (COARSE && tid < PCG_NW) red[32 + tid] = pmu_new[tid];
    __syncthreads();
    // ---- q = S~ p_r + AW p_mu for the rows of this workgroup ----
    double pqp = 0.0, gacc = 0.0;
#pragma unroll
    for (int k = 0; k < PCG_RPW; ++k) {
        const int row = row0 + w + 4 * k;
        double sacc = (COARSE && lane < PCG_NW) ? awv[k] * red[32 + lane] : 0.0, sacc2 = 0.0;       // two chains: a dependent DFMA is ~32 cycles
#pragma unroll
        for (int m = 0; m < PCG_CPL / 2; ++m) {
            const int c2 = lane + 64 * m;
            double2 pv2 = (2 * c2 < d) ? reinterpret_cast<const double2*>(pl)[c2] : make_double2(0.0, 0.0);
            if (2 * c2 + 1 >= d) pv2.y = 0.0;              // pl[d] is not written
            sacc = fma(fv[k][m].x, pv2.x, sacc);
            sacc2 = fma(fv[k][m].y, pv2.y, sacc2);
        }
        sacc += sacc2;
        sacc = wave_allsum(sacc);
        if (lane == 0 && row < row1) { q_out[row] = sacc; pqp += pl[row] * sacc; }
        if (COARSE && lane >= PCG_NW && lane < 2 * PCG_NW && row < row1) gacc = fma(awv[k], sacc, gacc);
    }
    if (lane == 0) red[40 + 9 * w] = pqp;
    if (COARSE && lane >= PCG_NW && lane < 2 * PCG_NW) red[40 + 9 * w + 1 + (lane - PCG_NW)] = gacc;
    __syncthreads();
    if (tid < NV) pcg_part(part, out, tid)[blockIdx.x] = red[40 + tid] + red[49 + tid] + red[58 + tid] + red[67 + tid];
}

// AW = S~ W~, E = W~^T AW, c_0 = W~^T b~ for d <= 1280, same workgroup geometry as k_pcg_iter_fast: the rows of S~ and this
// thread's share of W~ are loaded up front, W~ goes to LDS in fp32 (its values are fp32-representable: lossless).
__global__ __launch_bounds__(256) void k_pcg_coarse_fast(int d, int ld, const double* __restrict__ F, const double* __restrict__ W,
                                                         const double* __restrict__ bt, double* __restrict__ AW, double* __restrict__ epart, int rows_per_wg,
                                                         double* __restrict__ t_out) {
    __shared__ __align__(16) float wt[PCG_NW][64 * PCG_CPL];
    __shared__ double esum[4][PCG_NW * PCG_NW + 2 * PCG_NW];
    __shared__ __align__(16) double bl[64 * PCG_CPL];            // b~ (t = S~ b~ for the first CG launch)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row0 = blockIdx.x * rows_per_wg, row1 = min(d, row0 + rows_per_wg);
    double wreg[PCG_NW][PCG_EPT], breg[PCG_EPT];
#pragma unroll
    for (int m = 0; m < PCG_EPT; ++m) { const int e = tid + 256 * m; breg[m] = bt[e < d ? e : 0]; }
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k)
#pragma unroll
        for (int m = 0; m < PCG_EPT; ++m) { const int e = tid + 256 * m; wreg[k][m] = W[(size_t)k * ld + (e < d ? e : 0)]; }      // clamped, branch-free:
                                                                    // a conditional load whose consumer is sunk into the branch is waited for on its own
    double2 fv[PCG_RPW][PCG_CPL / 2];
    double wrow[PCG_RPW], wcol[PCG_RPW], btr[PCG_RPW];
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
        wrow[k] = have ? W[(size_t)(lane >> 3) * ld + row] : 0.0;           // E[k1][k2] += W~[k1][row] AW[row][k2], lane = 8 k1 + k2
        wcol[k] = have ? W[(size_t)(lane & 7) * ld + row] : 0.0;            // c_0[k] += W~[k][row] b~[row], lanes 0..7
        btr[k] = have ? bt[row] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k)
#pragma unroll
        for (int m = 0; m < PCG_EPT; ++m) wt[k][tid + 256 * m] = (tid + 256 * m < d) ? (float)wreg[k][m] : 0.0f;
#pragma unroll
    for (int m = 0; m < PCG_EPT; ++m) bl[tid + 256 * m] = (tid + 256 * m < d) ? breg[m] : 0.0;
    __syncthreads();
    double acc[PCG_RPW][PCG_NW], tacc[PCG_RPW];
#pragma unroll
    for (int r = 0; r < PCG_RPW; ++r) {
        tacc[r] = 0.0;
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) acc[r][k] = 0.0;
    }
#pragma unroll
    for (int m = 0; m < PCG_CPL / 2; ++m) {
        const int c2 = lane + 64 * m;
        const double2 bv = reinterpret_cast<const double2*>(bl)[c2];
#pragma unroll
        for (int r = 0; r < PCG_RPW; ++r) tacc[r] = fma(fv[r][m].x, bv.x, fma(fv[r][m].y, bv.y, tacc[r]));
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) {
            const float2 wv = reinterpret_cast<const float2*>(&wt[k][0])[c2];
#pragma unroll
            for (int r = 0; r < PCG_RPW; ++r) acc[r][k] = fma(fv[r][m].x, (double)wv.x, fma(fv[r][m].y, (double)wv.y, acc[r][k]));
        }
    }
#pragma unroll
    for (int r = 0; r < PCG_RPW; ++r)
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) acc[r][k] = wave_allsum(acc[r][k]);
    double e_acc = 0.0, c_acc = 0.0, t_acc = 0.0;
#pragma unroll
    for (int r = 0; r < PCG_RPW; ++r) {
        const int row = row0 + w + 4 * r;
        const double tr = wave_allsum(tacc[r]);          // (S~ b~)[row]: the first CG launch's q = S~ p_r with p_r = b~
        if (lane == 0 && row < row1) t_out[row] = tr;
        t_acc = fma(wcol[r], tr, t_acc);                 // W~^T S~ b~ (lanes 0..7; rows beyond row1: wcol = 0)
        double mine = 0.0;                               // AW[row][lane & 7]
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) mine = ((lane & 7) == k) ? acc[r][k] : mine;
        if (row < row1 && lane < PCG_NW) AW[(size_t)row * PCG_NW + lane] = mine;
        e_acc = fma(wrow[r], mine, e_acc);               // rows beyond row1 contribute wrow = 0
        c_acc = fma(wcol[r], btr[r], c_acc);
    }
    esum[w][lane] = e_acc;
    if (lane < PCG_NW) { esum[w][PCG_NW * PCG_NW + lane] = c_acc; esum[w][PCG_NW * PCG_NW + PCG_NW + lane] = t_acc; }
    __syncthreads();
    if (tid < PCG_NW * PCG_NW + 2 * PCG_NW) epart[(size_t)tid * PCG_PART + blockIdx.x] = esum[0][tid] + esum[1][tid] + esum[2][tid] + esum[3][tid];
}

// What the first launch of k_pcg_iter_fast does for itself, as a launch of its own for the families whose iteration kernels do not (streaming, symmetric:
// pcg_coarse_invert below).  It lives in this unit, next to the other callers of coarse_invert_wave, because the compiler's output for it depends on that:
// as the ONLY caller of coarse_invert_wave in a unit (alone, in pcg_streaming.hip, in dense_solver.hip: all tried) the inlined inversion is scheduled
// differently -- 1 467 instead of 1 488 instructions --, with any second caller in the unit, a dummy kernel included, it is the measured form.  The kernels are
// meant to stay the measured ones, instruction for instruction: before moving it, run
//     tools/kernel_isa_listing.py <the units> dist_cg.hip --check profiles/cg_split_kernel_isa_after.txt
// stand-alone version (streaming CG path: up to 1024 workgroups of partials): out = [Einv 64 | c_0 8 | E 64]
__global__ __launch_bounds__(256) void k_pcg_coarse_invert(int nwg, const double* __restrict__ epart, double* __restrict__ out) {
    constexpr int N = PCG_NW, NV = N * N + N;
    __shared__ double tot[NV];
    __shared__ double sa[N * N], sb[N * N];
    coarse_sum_partials(nwg, epart, tot);
    __syncthreads();
    if (threadIdx.x >= 64) return;
    if (threadIdx.x < N) out[N * N + threadIdx.x] = tot[N * N + threadIdx.x];
    out[N * N + N + threadIdx.x] = tot[threadIdx.x];          // E itself (symmetric streaming path: W~^T q = AW^T p_r + E p_mu)
    out[threadIdx.x] = coarse_invert_wave(tot, sa, sb);
}

// AW, the partials of E, c_0 and W~^T S~ b~, and t = S~ b~ -> the q buffer of parity 0 (pcg_vec).  No launch for the inverse: the first CG
// launch sums the partials and inverts E itself (one launch fewer per LM iteration).
void pcg_fast_setup(hipStream_t s, const DenseSolver* ws, Profiler* prof) {
    const CgPath& r = ws->run.path;
    if (!r.coarse) return;
    ProfScope ps(prof, KID_PCG_SETUP, s, 1);
    hipLaunchKernelGGL(k_pcg_coarse_fast, dim3(r.nwg), dim3(256), 0, s, ws->d, ws->ld, ws->Sfull, ws->W, pcg_btilde(ws), ws->AW, ws->epart, r.rows_per_wg,
                       ws->vec + (size_t)(2 * 3 + 0) * ws->ld);
}

void pcg_coarse_invert(hipStream_t s, int nwg, const double* epart, double* out) {
    hipLaunchKernelGGL(k_pcg_coarse_invert, dim3(1), dim3(256), 0, s, nwg, epart, out);
}

void pcg_fast_iterate(hipStream_t s, const DenseSolver* ws, bool init, int in, int anchor, double cap) {
    const DenseSolver::CgRun& run = ws->run;
    const CgPath& r = run.path;
#define SFMBA_IT(MODE, C) hipLaunchKernelGGL((k_pcg_iter_fast<MODE, C>), dim3(r.nwg), dim3(256), r.lds, s, ws->d, ws->ld, ws->Sfull, ws->vec, pcg_btilde(ws), ws->part, ws->scal, \
        ws->flags, r.rows_per_wg, run.tol2, in, run.info, ws->d_mailbox, anchor, cap, ws->W, ws->AW, ws->coarse, ws->epart)
    // (with the coarse space the first launch is also the first iteration: MODE 2, see k_pcg_iter_fast -- CgPath::first_launch_is_iteration)
    if (r.coarse) { if (init) SFMBA_IT(2, true); else SFMBA_IT(0, true); }
    else { if (init) SFMBA_IT(1, false); else SFMBA_IT(0, false); }
#undef SFMBA_IT
}

}  // namespace sfmba
