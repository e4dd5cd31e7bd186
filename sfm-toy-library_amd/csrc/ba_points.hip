// ba_points.hip -- stage 1 of an LM iteration's linearisation: the point pass (point-major).
//   reads   camtab[cur] (R, t), pts[cur], the observations in point-major order, pscale, the LM state (radius, focal, fscale)
//   leaves  per point: the table entry every other pass re-evaluates its observations from (PA: X, L^-1 diag(s_p); PB: t, y_f), pt_t, pt_M;
//           in the slots: cost at the linearisation point, S_ff / rhs_f contributions, gradient max-norm, the failure flag;
//           and it clears what the camera pass (ba_cams.hip) and the duplicate-pair pass accumulate with atomics.  NOTHING per observation.
#include "ba_common.h"
#include <algorithm>

namespace sfmba {

// ------------------------------------------------------------------------------------------
// 3x3 SPD: L^-1 (lower, 6 values l00 l10 l11 l20 l21 l22 of the INVERSE factor). Returns false if not PD.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool chol3_inverse(const double V[6] /* v00 v10 v11 v20 v21 v22 */, double Li[6]) {
    // L^-1 directly from reciprocal square roots of the pivots (no sqrt / divide chains)
    const double i00 = fast_rsq(V[0]);
    const double l10 = V[1] * i00, l20 = V[3] * i00;
    const double d1 = V[2] - l10 * l10;
    const double i11 = fast_rsq(d1);
    const double l21 = (V[4] - l20 * l10) * i11;
    const double d2 = V[5] - l20 * l20 - l21 * l21;
    const double i22 = fast_rsq(d2);
    Li[0] = i00;
    Li[1] = -l10 * i00 * i11;
    Li[2] = i11;
    Li[4] = -l21 * i11 * i22;
    Li[3] = -(l20 * i00 + l21 * Li[1]) * i22;
    Li[5] = i22;
    return (V[0] > 0.0) && (d1 > 0.0) && (d2 > 0.0);
}

// Per point, once its sums over the observations are known: Jacobi scales, LM damping, the inverse Cholesky factor of V + D^2, t, y_f, M and
// the table entry every other pass re-evaluates from.  `store`: this lane writes the point's results (lanes that share a point compute the
// same values; one of them stores and contributes to the block sums).
template <typename T>
__device__ __forceinline__ void point_finish(const DeviceBuffers& db, const LMState* st, size_t i, int ps_mode, const double (&Xl)[3], double (&V)[6], double (&bp)[3],
                                             double (&Ef)[3], double (&sp)[3], bool store, double& gmax, double& sff, double& rhsf, double& bad) {
    const double radius = st->radius;
    // Jacobi scales of the point's three columns: loaded, or -- first linearisation of a solve -- formed here from the
    // column norms this lane has just summed (s = 1 / (1 + ||J_col||), [Ceres-upstream] EstimateScale)
    if (ps_mode != 0) {
        sp[0] = ps_mode == 1 ? 1.0 / (1.0 + sqrt(V[0])) : 1.0;
        sp[1] = ps_mode == 1 ? 1.0 / (1.0 + sqrt(V[2])) : 1.0;
        sp[2] = ps_mode == 1 ? 1.0 / (1.0 + sqrt(V[5])) : 1.0;
        if (store) { db.pscale[3 * i] = sp[0]; db.pscale[3 * i + 1] = sp[1]; db.pscale[3 * i + 2] = sp[2]; }
    }
    if (store) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gmax = fmax(gmax, fabs(bp[c]));           // gradient of the unscaled problem
    }
    V[0] *= sp[0] * sp[0]; V[1] *= sp[1] * sp[0]; V[2] *= sp[1] * sp[1];
    V[3] *= sp[2] * sp[0]; V[4] *= sp[2] * sp[1]; V[5] *= sp[2] * sp[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) { bp[c] *= sp[c]; Ef[c] *= sp[c]; }
    // LM damping D^2 = clamp(diag(J~^T J~)) / radius   [LevenbergMarquardtStrategy::ComputeStep]
    V[0] += fmin(fmax(V[0], st->min_diag), st->max_diag) / radius;
    V[2] += fmin(fmax(V[2], st->min_diag), st->max_diag) / radius;
    V[5] += fmin(fmax(V[5], st->min_diag), st->max_diag) / radius;
    double Li[6];
    const bool pd = chol3_inverse(V, Li);
    const double t0 = Li[0] * bp[0];
    const double t1 = Li[1] * bp[0] + Li[2] * bp[1];
    const double t2 = Li[3] * bp[0] + Li[4] * bp[1] + Li[5] * bp[2];
    const double y0 = Li[0] * Ef[0];
    const double y1 = Li[1] * Ef[0] + Li[2] * Ef[1];
    const double y2 = Li[3] * Ef[0] + Li[4] * Ef[1] + Li[5] * Ef[2];
    if (!store) return;
    db.pt_t[3 * i] = t0; db.pt_t[3 * i + 1] = t1; db.pt_t[3 * i + 2] = t2;
    // M = diag(s_p) L^-T for the back-substitution (k_point_update): dX = M (t - sum C^T u)
    db.pt_M[6 * i] = sp[0] * Li[0]; db.pt_M[6 * i + 1] = sp[0] * Li[1]; db.pt_M[6 * i + 2] = sp[0] * Li[3];
    db.pt_M[6 * i + 3] = sp[1] * Li[2]; db.pt_M[6 * i + 4] = sp[1] * Li[4]; db.pt_M[6 * i + 5] = sp[2] * Li[5];
    sff -= y0 * y0 + y1 * y1 + y2 * y2;
    rhsf -= y0 * t0 + y1 * t1 + y2 * t2;
    if (!pd || !finite_d(t0 + t1 + t2 + y0 + y1 + y2)) bad = 1.0;
    // the per-point table (sfmba_device.h): the point itself; L^-1 with the point scales folded in, so that C = B~ L^-T =
    // B diag(s) L^-T comes from the UNSCALED point block of an observation; t and y_f in the precision of the Jacobian blocks
    PtRecA<T> ra;
    ra.X[0] = Xl[0]; ra.X[1] = Xl[1]; ra.X[2] = Xl[2];
    ra.L[0] = (T)(Li[0] * sp[0]); ra.L[1] = (T)(Li[1] * sp[0]); ra.L[2] = (T)(Li[2] * sp[1]);
    ra.L[3] = (T)(Li[3] * sp[0]); ra.L[4] = (T)(Li[4] * sp[1]); ra.L[5] = (T)(Li[5] * sp[2]);
    if (sizeof(T) == 8) reinterpret_cast<double*>(&ra)[9] = 0.0;
    reinterpret_cast<PtRecA<T>*>(db.PA)[i] = ra;
    PtRecB<T> rb;
    rb.t[0] = (T)t0; rb.t[1] = (T)t1; rb.t[2] = (T)t2;
    rb.yf[0] = (T)y0; rb.yf[1] = (T)y1; rb.yf[2] = (T)y2;
    reinterpret_cast<PtRecB<T>*>(db.PB)[i] = rb;
}

// K1: point pass.  The point pass leaves NOTHING per observation behind (rounds 1 - 3 wrote a 64-byte record per observation for the
// back-substitution: 64 MB written and read per LM iteration at BASELINE config 3): per point the table entry the reduced-system passes
// and the back-substitution re-evaluate from (PtRecA / PtRecB), t, M.  LPP = 4 LANES PER POINT: a wave owns 16 points, the four lanes of
// a point take its observations in turn (4 at a time) and keep the point's sums in registers; one quad reduction (DPP) and the
// per-point arithmetic on every lane of the quad.  (Rounds 1 - 3 and the first half of round 4 gave every observation a lane and every
// wave 64 consecutive observations: of its ~750 wave instructions ~360 were a serial row loop through LDS and ~130 the per-point phase,
// both at a tenth of the lanes -- 34.5 against 22.7 us at BASELINE config 3, 150 against 98 at config 5.)  Waves take points in the order
// of ds.pt_order (sorted by number of rounds of four observations: the quads of a wave then loop alike whatever the track lengths).  A
// lane needs the camera's R and t only (three component quads of the table: K' is the reduced-system passes' business).
template <typename T>
__global__ __launch_bounds__(PBK) void k_point_build(DeviceStructure ds, DeviceBuffers db, int ps_mode_flags) {
    if ((ps_mode_flags & 4) && (db.st->termination != -1 || db.st->retry != 0)) return;
    const int ps_mode = ps_mode_flags & 3;
    __shared__ double scratch[WPB * 4];
    const LMState* st = db.st;
    const int cur = st->cur;
    const double* tab = db.camtab[cur];
    const double focal = st->focal[cur];
    const T fscale = (T)st->fscale;
    const double* pts = db.pts[cur];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int gw = blockIdx.x * WPB + w;
    double lin_cost = 0.0, sff = 0.0, rhsf = 0.0, gmax = 0.0, bad = 0.0;
    // clear what k_cam_diag_f (and the duplicate-pair pass) accumulate with atomics: per camera the 6x6 diagonal block,
    // its focal column, the undamped diagonal, the scaled gradient and the reduced right-hand side
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < ds.ncam * 60; e += gridDim.x * blockDim.x) {
        const int j = e / 60, k = e - 60 * j, row0 = 6 * j;
        if (k < 36) db.S[(size_t)(row0 + k / 6) * ds.ld + row0 + k % 6] = 0.0;
        else if (k < 42) db.udiag[row0 + k - 36] = 0.0;
        else if (k < 48) db.bc[row0 + k - 42] = 0.0;
        else if (k < 54) db.rhs[row0 + k - 48] = 0.0;
        else db.S[(size_t)(row0 + k - 54) * ds.ld + ds.d - 1] = 0.0;
    }
    const int sub = lane & (PB_LPP - 1);
    const int slot = gw * (64 / PB_LPP) + (lane / PB_LPP);
    const bool have = slot < ds.npt;
    const int ip = have ? (ds.pt_order ? ds.pt_order[slot] : slot) : 0;
    const size_t i = (size_t)ip;
    const int q0 = have ? ds.pt_ptr[ip] : 0, q1 = have ? ds.pt_ptr[ip + 1] : 0;
    double Xl[3] = { pts[3 * i], pts[3 * i + 1], pts[3 * i + 2] };
    double sp[3] = { 1.0, 1.0, 1.0 };
    if (ps_mode == 0) { sp[0] = db.pscale[3 * i]; sp[1] = db.pscale[3 * i + 1]; sp[2] = db.pscale[3 * i + 2]; }
    T Va[6] = { (T)0, (T)0, (T)0, (T)0, (T)0, (T)0 }, Ea[3] = { (T)0, (T)0, (T)0 };
    double bp[3] = { 0, 0, 0 };
    // the camera and the coordinates of the NEXT round's observation are fetched one round ahead: a round costs one dependent memory
    // level (the camera's table row)
    int q = q0 + sub;
    int j_next = q < q1 ? ds.obs_cam[q] : 0;
    double ox_next = 0.0, oy_next = 0.0;
    if (q < q1) load_obs<T>(ds.obs_xy, q, ox_next, oy_next);
    while (__any(q < q1)) {
        const bool act = q < q1;
        const int j = j_next;
        const double ox = ox_next, oy = oy_next;
        const CamRow ct = { tab + 4 * (size_t)(j), ds.ncam };
        double Rt[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) Rt[e] = ct[CT_R + e];
        q += PB_LPP;
        if (q < q1) { j_next = ds.obs_cam[q]; load_obs<T>(ds.obs_xy, q, ox_next, oy_next); }
        if (act) {
            const Proj pr = project_point(Rt, 0, 9, Xl);
            const double r0 = focal * pr.xp - ox, r1 = focal * pr.yp - oy;
            lin_cost += r0 * r0 + r1 * r1;
            T B[6];
            point_block<T>(Rt, pr, focal, B);
            const T g0 = (T)pr.xp * fscale, g1 = (T)pr.yp * fscale;
            Va[0] += B[0] * B[0] + B[3] * B[3];
            Va[1] += B[1] * B[0] + B[4] * B[3];
            Va[2] += B[1] * B[1] + B[4] * B[4];
            Va[3] += B[2] * B[0] + B[5] * B[3];
            Va[4] += B[2] * B[1] + B[5] * B[4];
            Va[5] += B[2] * B[2] + B[5] * B[5];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Ea[c] += B[c] * g0 + B[3 + c] * g1;
                bp[c] += (double)B[c] * r0 + (double)B[3 + c] * r1;
            }
        }
    }
    // the point's sums over its quad (every lane of the quad ends up with them)
    double V[6], Ef[3];
#pragma unroll
    for (int c = 0; c < 6; ++c) { double v = (double)Va[c]; v = xlane_add<1>(v); v = xlane_add<2>(v); V[c] = v; }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double v = (double)Ea[c]; v = xlane_add<1>(v); v = xlane_add<2>(v); Ef[c] = v;
        double u = bp[c]; u = xlane_add<1>(u); u = xlane_add<2>(u); bp[c] = u;
    }
    if (have) point_finish<T>(db, st, i, ps_mode, Xl, V, bp, Ef, sp, sub == 0, gmax, sff, rhsf, bad);
    if (!finite_d(lin_cost)) bad = 1.0;
    const double gm = wave_max(gmax);
    if ((threadIdx.x & 63) == 0 && gm > 0.0) atomic_max_nonneg(slot_ptr(db, ACC_GMAX), gm);
    double sums[4] = { lin_cost, sff, rhsf, bad };
    const double tot = block_sums<4>(sums, scratch);
    if (threadIdx.x < 4) {
        const int which = threadIdx.x == 0 ? ACC_LIN_COST : threadIdx.x == 1 ? ACC_SFF : threadIdx.x == 2 ? ACC_RHSF : ACC_BAD_LIN;
        if (threadIdx.x < 3 || tot != 0.0) atomicAdd(slot_ptr(db, which), tot);
    }
}

template <typename T>
void launch_point_build(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db, int ps_mode) {
    const int per_wg = WPB * (64 / PB_LPP);
    // (at least one workgroup: the launch also clears what the camera pass accumulates -- a row-sharded rank may own no point)
    hipLaunchKernelGGL(k_point_build<T>, dim3(std::max(1, (ds.npt + per_wg - 1) / per_wg)), dim3(PBK), 0, s, ds, db, ps_mode);
}
template void launch_point_build<float>(hipStream_t, const DeviceStructure&, const DeviceBuffers&, int);
template void launch_point_build<double>(hipStream_t, const DeviceStructure&, const DeviceBuffers&, int);

}  // namespace sfmba
