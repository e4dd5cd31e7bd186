// ba_step.hip -- the second half of an LM iteration, behind the linear solve: back-substitution, trial point, accept / reject.
//   reads   the reduced step (rhs, or x~ of the CG with pcg_linv), cscale / fscale, camtab[cur], the per-point table, pt_t, pt_M, the observations
//   leaves  cam / pts / camtab / focal of the TRIAL buffer (cur ^ 1), the step table, the slots' trial cost, model cost change, step and
//           parameter norms; then k_lm_control, a launch of its own: LM state (cur flips on acceptance, radius, termination), trace row, mailbox
#include "ba_common.h"
#include <algorithm>

namespace sfmba {

// ------------------------------------------------------------------------------------------
// back-substitution + trial point
// ------------------------------------------------------------------------------------------
// CU_LANES lanes per camera (the form of k_finalize's FIN_LANES): delta = scale * y ; trial camera = camera - delta ; step table; table
// of the trial camera.  Every lane of a camera's group loads what the camera needs -- all of it, and what the focal entry's owner needs,
// in ONE level in front of the first store -- and forms the step, the trial camera and its table with the same instructions; lane t then
// stores its share of the ~90 scattered values (cam[nxt], camtab[nxt], steptab, the fp32 record: the 16- / 32-byte pieces t,
// t + CU_LANES, ... of each, picked by selects).  A workgroup holds the 64 cameras of what was one wave of the one-lane-per-camera form,
// so the grid spreads over ceil(ncam / 64) CUs and the three sums are still formed from ONE value per camera by the butterfly over those
// 64 cameras (handed to the first wave through LDS): bit for bit the sums of the one-lane form up to 64 cameras; above, the sums of the
// groups of 64 meet in the slots instead of in one workgroup.
constexpr int CU_LANES = 4;
constexpr int CU_CAMS = BLK / CU_LANES;
static_assert(CU_CAMS == 64, "k_cam_update: the cameras of a workgroup are summed by one wave");

// lane t of a group stores the pieces t, t + CU_LANES, ... (P values each) of v[N], which every lane of the group holds; at(e): where value e goes
template <int N, int P, typename V, typename At>
__device__ __forceinline__ void store_share(int t, const V (&v)[N], At at) {
    static_assert(N % P == 0, "whole pieces");
    constexpr int NP = N / P;
#pragma unroll
    for (int k0 = 0; k0 < NP; k0 += CU_LANES) {
        V w[P];
#pragma unroll
        for (int r = 0; r < P; ++r) {
            w[r] = v[P * k0 + r];
#pragma unroll
            for (int u = 1; u < CU_LANES; ++u) if (k0 + u < NP) w[r] = (t == u) ? v[P * (k0 + u) + r] : w[r];
        }
        if (k0 + t < NP) {
#pragma unroll
            for (int r = 0; r < P; ++r) *at(P * (k0 + t) + r) = w[r];
        }
    }
}

__global__ __launch_bounds__(BLK) void k_cam_update(DeviceStructure ds, DeviceBuffers db) {
    __shared__ double part[3][CU_CAMS];
    if (db.cg_gate && !db.cg_force && db.cg_gate[0] == 0) return;      // the CG batch in front of this launch was too short
    LMState* st = db.st;
    const int cur = st->cur, nxt = cur ^ 1;
    // (picked from the two kernel arguments: indexed by a loaded value the pointer itself is a load, and the one of the trial buffer sat behind a store)
    const double* const cam_c = cur ? db.cam[1] : db.cam[0];
    const double* const tab_c = cur ? db.camtab[1] : db.camtab[0];
    double* const cam_n = cur ? db.cam[0] : db.cam[1];
    double* const tab_n = cur ? db.camtab[0] : db.camtab[1];
    const int jl = threadIdx.x / CU_LANES, t = threadIdx.x % CU_LANES;         // camera of the workgroup, lane of its group
    const int j = blockIdx.x * CU_CAMS + jl;
    const bool focal_owner = blockIdx.x == 0 && threadIdx.x == 0;
    double step2 = 0.0, xn2 = 0.0, gdot = 0.0;
    // the focal entry's owner: its loads belong to the same level (behind the camera's stores they were a round trip of their own)
    double f0 = 0.0, fsc = 0.0, zf = 0.0, bcf = 0.0;
    if (focal_owner) {
        f0 = st->focal[cur]; fsc = st->fscale;
        zf = db.rhs[ds.d - 1];
        if (db.pcg_vec) zf = db.pcg_linv[(size_t)ds.ncam * 36] * db.pcg_vec[(size_t)db.pcg_flags[2] * ds.ld + ds.d - 1];
        if (db.pu32) bcf = db.bc[ds.d - 1];
    }
    if (j < ds.ncam) {
        double dlt[6], cn[6], z[6];
        // every load of this camera before the first store (the stores below may alias as far as the compiler can tell: a load behind
        // one of them waits for its own round trip)
        double c0[6], cs[6], xin[6], Lt[6][6], Q9[9];
#pragma unroll
        for (int e = 0; e < 6; ++e) { c0[e] = cam_c[6 * j + e]; cs[e] = db.cscale[6 * j + e]; }
        // Q = R K' and the first-order flag of the camera AT THE LINEARISATION POINT: the back-substitution re-evaluates the camera
        // block of an observation in the factored form A = P [ -[X_g]x | I ] diag(Q, I) (sfmba_device.h), so the step arrives as Q dw
#pragma unroll
        for (int e = 0; e < 9; ++e) Q9[e] = tab_c[cam_tab_index(CT_QD + e, j, ds.ncam)];
        const double small_cur = tab_c[cam_tab_index(CT_SMALL, j, ds.ncam)];
        double Rt_cur[12], bcj[6];
        if (db.pu32) {
#pragma unroll
            for (int e = 0; e < 12; ++e) Rt_cur[e] = tab_c[cam_tab_index(CT_R + e, j, ds.ncam)];
#pragma unroll
            for (int e = 0; e < 6; ++e) bcj[e] = db.bc[6 * j + e];
        }
        if (db.pcg_vec) {          // z_j = Linv_j^T x~_j  (block-Jacobi transformed unknowns)
            const double* x = db.pcg_vec + (size_t)db.pcg_flags[2] * ds.ld + 6 * j;
            const double* Li = db.pcg_linv + (size_t)j * 36;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                xin[r] = x[r];
#pragma unroll
                for (int c = 0; c < 6; ++c) Lt[r][c] = (c <= r) ? Li[r * 6 + c] : 0.0;
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < 6; ++r) if (r >= c) v += Lt[r][c] * xin[r];
                z[c] = v;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 6; ++c) z[c] = db.rhs[6 * j + c];
        }
        if (db.probe_z && t == 0) {
#pragma unroll
            for (int e = 0; e < 6; ++e) db.probe_z[6 * j + e] = z[e];
        }
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            dlt[e] = cs[e] * z[e];
            cn[e] = c0[e] - dlt[e];
            const double df = c0[e] - cn[e];
            step2 += df * df;
            xn2 += cn[e] * cn[e];
        }
        double ctn[CT_STRIDE];
        make_cam_table(cn, cs, ctn);
        double stb[ST_STRIDE] = {};
        for (int e = 0; e < 9; ++e) stb[ST_RN + e] = ctn[CT_R + e];
        for (int e = 0; e < 3; ++e) {
            stb[ST_DQ + e] = Q9[3 * e] * dlt[0] + Q9[3 * e + 1] * dlt[1] + Q9[3 * e + 2] * dlt[2];
            stb[ST_DT + e] = dlt[3 + e]; stb[ST_TN + e] = ctn[CT_T + e];
        }
        stb[ST_SMALL] = small_cur;
        store_share<6, 2>(t, cn, [&](int e) { return cam_n + 6 * (size_t)j + e; });
        store_share<CT_STRIDE, 4>(t, ctn, [&](int e) { return tab_n + cam_tab_index(e, j, ds.ncam); });
        store_share<ST_STRIDE, 4>(t, stb, [&](int e) { return db.steptab + cam_tab_index(e, j, ds.ncam); });
        if (db.pu32) {
            // the first sweep of k_point_update in F32J mode: what it needs of this camera as ONE 80-byte fp32 record; and the part of the model
            // cost change that sweep no longer forms per observation: sum_obs u . r = (step) . (gradient) = sum z_i bc_i in the scaled unknowns
            float rec[20];
#pragma unroll
            for (int e = 0; e < 12; ++e) rec[e] = (float)Rt_cur[e];
#pragma unroll
            for (int e = 0; e < 8; ++e) rec[12 + e] = (float)stb[e];
            store_share<20, 4>(t, rec, [&](int e) { return db.pu32 + 20 * (size_t)j + e; });
#pragma unroll
            for (int e = 0; e < 6; ++e) gdot += z[e] * bcj[e];
        }
    }
    if (focal_owner) {
        if (db.probe_z) db.probe_z[ds.d - 1] = zf;
        const double fn = f0 - fsc * zf;
        st->focal[nxt] = fn;
        const double df = f0 - fn;
        step2 += df * df;
        xn2 += fn * fn;
        if (db.pu32) gdot += zf * bcf;
    }
    // one value per camera, summed as one wave of one lane per camera would sum them
    if (t == 0) { part[0][jl] = step2; part[1][jl] = xn2; part[2][jl] = gdot; }
    __syncthreads();
    if (threadIdx.x < 64) {
        const double s2 = wave_sum(part[0][threadIdx.x]), x2 = wave_sum(part[1][threadIdx.x]), gd = wave_sum(part[2][threadIdx.x]);
        if (threadIdx.x == 0) {
            atomicAdd(slot_ptr(db, ACC_STEP2), db.shared_weight * s2);
            atomicAdd(slot_ptr(db, ACC_XNEW2), db.shared_weight * x2);
            if (db.pu32) atomicAdd(slot_ptr(db, ACC_MODEL), db.shared_weight * gd);      // (sharded: the cameras are replicated, rank 0 counts them)
        }
    }
}

// ------------------------------------------------------------------------------------------
// LM control: the accept/reject logic of ceres::internal::TrustRegionMinimizer::Minimize()
// [Ceres-upstream], one thread.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void lm_post(int* mb, int seq, int termination, int message, int iter, int cg_iters = 0) {
    if (!mb) return;
    __hip_atomic_store(mb + 4, cg_iters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(mb + 1, termination, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(mb + 2, message, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(mb + 3, iter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(mb, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// (all 64 lanes of ONE wave; every accumulator it reads must be complete and visible: a kernel of its own behind the passes)
__device__ __forceinline__ void lm_control_body(const DeviceBuffers& db) {
    LMState* st = db.st;
    if (db.cg_gate && !db.cg_force && db.cg_gate[0] == 0) {
        // the linear solve has not converged within the launches enqueued so far: tell the host (termination code -2),
        // touch nothing -- it will enqueue more CG iterations followed by the same three kernels
        if ((threadIdx.x & 63) == 0) { st->retry = 1; const int seq = ++st->mail_seq; lm_post(db.lm_mailbox, seq, -2, 0, st->iter); }
        return;
    }
    double trial2, model, step2, xnew2, bad_trial;
    if (db.shard_scal) {
        // sharded solve: the sums over the ranks sit in the all-reduced scalar block (k_shard_pack emptied the slots)
        trial2 = db.shard_scal[0]; model = db.shard_scal[1]; step2 = db.shard_scal[2]; xnew2 = db.shard_scal[3]; bad_trial = db.shard_scal[4];
    } else {
        const int ctl_acc[5] = { ACC_TRIAL_COST, ACC_MODEL, ACC_STEP2, ACC_XNEW2, ACC_BAD_TRIAL };
        double ctl[5];
        slots_take_n<5>(db, ctl_acc, ctl);
        trial2 = ctl[0]; model = ctl[1]; step2 = ctl[2]; xnew2 = ctl[3]; bad_trial = ctl[4];
    }
    if ((threadIdx.x & 63) != 0) return;
    st->retry = 0;
    st->lin_info = *db.lin_info;
    *db.lin_info = 0;
    const int seq = ++st->mail_seq;
    const int cg_iters = db.cg_gate ? db.cg_gate[1] : 0;          // CG iterations of this LM iteration (device-side count)
    if (st->termination != -1) { if (db.st_mirror) *db.st_mirror = *st; lm_post(db.lm_mailbox, seq, st->termination, st->message, st->iter, cg_iters); return; }
    const int it = ++st->iter;
    TraceRow row = {};
    row.iteration = it;
    const bool lin_fail = st->lin_info != 0 || !finite_d(step2) || !finite_d(model);
    const bool step_valid = !lin_fail && model > 0.0;
    row.step_is_valid = step_valid;
    row.gradient_max_norm = st->gmax;
    double report_cost = st->cost;
    st->last_step_successful = 0;
    if (!step_valid) {
        if (++st->consecutive_invalid >= st->max_consecutive_invalid) {
            st->termination = SFMBA_FAILURE;
            st->message = MSG_INVALID_STEPS;
        } else {
            st->radius *= st->invalid_shrink;
            st->unsuccessful++;
        }
    } else {
        st->consecutive_invalid = 0;
        double cand = 0.5 * trial2;
        if (bad_trial != 0.0 || !finite_d(cand)) cand = DBL_MAX;
        st->residual_evals++;
        row.step_norm = sqrt(step2);
        const double step_tol = st->parameter_tolerance * (st->x_norm + st->parameter_tolerance);
        if (row.step_norm <= step_tol) {
            st->termination = SFMBA_CONVERGENCE;
            st->message = MSG_PARAMETER_TOL;
        } else {
            row.cost_change = st->cost - cand;
            if (fabs(row.cost_change) <= st->function_tolerance * st->cost) {
                st->termination = SFMBA_CONVERGENCE;
                st->message = MSG_FUNCTION_TOL;
            } else {
                row.relative_decrease = row.cost_change / model;
                if (row.relative_decrease > st->min_relative_decrease) {
                    row.step_is_successful = 1;
                    st->last_step_successful = 1;
                    st->cur ^= 1;
                    st->cost = cand;
                    st->x_norm = sqrt(xnew2);
                    const double t = 2.0 * row.relative_decrease - 1.0;
                    st->radius = st->radius / fmax(1.0 / 3.0, 1.0 - t * t * t);
                    st->radius = fmin(st->max_radius, st->radius);
                    st->decrease_factor = 2.0;
                    st->successful++;
                    st->x_is_new = 1;
                    report_cost = cand;
                } else {
                    st->radius = st->radius / st->decrease_factor;
                    st->decrease_factor *= 2.0;
                    st->unsuccessful++;
                    report_cost = cand;
                }
            }
        }
    }
    if (st->termination == -1 && st->radius <= st->min_radius) {
        st->termination = SFMBA_CONVERGENCE;
        st->message = MSG_MIN_RADIUS;
    }
    row.cost = report_cost;
    row.trust_region_radius = st->radius;
    if (it < db.trace_cap) db.trace[it] = row;
    st->lin_info = 0;
    if (db.st_mirror) *db.st_mirror = *st;      // plain stores; the release store of the sequence number in lm_post orders them
    lm_post(db.lm_mailbox, seq, st->termination, st->message, st->iter, cg_iters);
}

__global__ void k_lm_control(DeviceBuffers db) { lm_control_body(db); }

// Back-substitution + trial point, four lanes per point like k_point_build:
//   y_p = (V + D^2)^-1 (b_p - W^T y_c), trial point, model cost change, trial cost.
// With V + D^2 = L L^T, t = L^-1 b_p and C = B~ L^-T (left behind per POINT by k_point_build: pt_t, M = diag(s_p) L^-T, the table entry):
//   u   = A (camera step) + g (focal step)     per observation
//   z   = t - sum_obs C^T u                      per point
//   dX  = M z ;   J step = -(u + C z)            (model cost change; B~ y_p = C L^T y_p = C z)
// Nothing per observation is read but its camera and coordinates (rounds 2 / 3 streamed a 64-byte record per observation here): the
// projection at the linearisation point is re-evaluated in fp64 from the camera's R, t and the point-table entry, the camera block acts
// on the step in the factored form of sfmba_device.h,  A [dw; dt] = P (Q dw x X_g + dt),  P = (f / p_z) [[1, 0, -x_p], [0, 1, -y_p]],
// with Q dw formed once per camera by k_cam_update, and C = (P R) L~ in the precision of the Jacobian blocks, exactly as the
// reduced-system passes form it.  The quad's lanes take the point's observations in turn and keep
//   sum C^T u (3),  sum u.r,  sum |u|^2,  sum C^T C (6)
// in registers; after ONE quad reduction every lane of the quad has z = t - sum C^T u, the trial point, and the point's share of the model
// cost change in closed form --
//   sum_obs [ (u + C z).r - |u + C z|^2 / 2 ] = sum u.r + z.t - sum |u|^2 / 2 - z.(sum C^T u) - z^T (sum C^T C) z / 2      (sum C^T r = L^-1 b_p = t)
// -- so the second sweep over the observations only evaluates the TRIAL residual (projection with the trial pose at the trial point): nothing
// per observation has to survive the first sweep, no LDS, and the per-point arithmetic runs on all lanes (the lane-per-observation form
// of the first half of round 4: 33.6 against 29.9 us at BASELINE config 3, 242 against 189 at config 5).
// (Measured in round 5 and not kept: the LM control logic run by the LAST WORKGROUP TO ARRIVE of this launch instead of a launch of its own.
// With a release fence per workgroup the launch went from 27 to 83 us at BASELINE config 3 (747 from 190 at config 5: buffer_wbl2 3 125 times);
// with the slots read as agent atomics and no release, one ticket counter serialised the 3 125 arrivals (57 us); with two-level tickets on
// separate cache lines 36.5 us against 29.9 + 5.6 for the two launches: 4 260 against 4 270 LM iterations/s -- a wash, so the simpler form stays.)
#ifndef SFMBA_TRIAL_POSE_MIN_CAMS
#define SFMBA_TRIAL_POSE_MIN_CAMS 400     // 96 bytes of [R | t] per camera against a 32 KB L1: between the two measured sizes (200: table, 1 000: parameters)
#endif
template <typename T>
__global__ __launch_bounds__(PBK, 4) void k_point_update(DeviceStructure ds, DeviceBuffers db) {
    __shared__ double scratch[WPB * 5];
    if (db.cg_gate && !db.cg_force && db.cg_gate[0] == 0) return;      // see k_cam_update
    const LMState* st = db.st;
    const int cur = st->cur, nxt = cur ^ 1;
    const double* tab = db.camtab[cur];
    const double* stab = db.steptab;
    const double focal = st->focal[cur], focal_n = st->focal[nxt];
    const double dfoc = focal - focal_n;           // unscaled focal step to SUBTRACT (= fscale * y_f)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int gw = blockIdx.x * WPB + w;
    double trial = 0.0, model = 0.0, step2 = 0.0, xn2 = 0.0, bad = 0.0;
    const int sub = lane & (PB_LPP - 1);
    const int slot = gw * (64 / PB_LPP) + (lane / PB_LPP);
    const bool have = slot < ds.npt;
    const int ip = have ? (ds.pt_order ? ds.pt_order[slot] : slot) : 0;
    const size_t i = (size_t)ip;
    const int q0 = have ? ds.pt_ptr[ip] : 0, q1 = have ? ds.pt_ptr[ip + 1] : 0;
    const PtRecA<T> pa = load_ptrec(reinterpret_cast<const PtRecA<T>*>(db.PA) + i);
    double zacc[3] = { 0, 0, 0 }, ur = 0.0, uu = 0.0;
    T G[6] = { (T)0, (T)0, (T)0, (T)0, (T)0, (T)0 };       // (sum C^T C: a second-order term of the model cost change; summed in the precision of C)
    if (sizeof(T) == 4 && db.pu32) {
        // F32J, unsharded: the camera's R, t and step as ONE fp32 record (k_cam_update), five 16-byte gathers instead of ten -- the pass is bound by the
        // number of gather instructions (every lane another camera: 64 lines each; TA_TA_BUSY 92 % at BASELINE config 5).  sum u . r is not formed here.
        const float4* recs = reinterpret_cast<const float4*>(db.pu32);
        int q = q0 + sub;
        int j_next = q < q1 ? ds.obs_cam[q] : 0;
        while (__any(q < q1)) {
            const bool act = q < q1;
            const float4* rec = recs + 5 * (size_t)j_next;
            const float4 a0 = rec[0], a1 = rec[1], a2 = rec[2], a3 = rec[3], a4 = rec[4];
            const double Rt[12] = { a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w };
            const double dr[8] = { a3.x, a3.y, a3.z, a3.w, a4.x, a4.y, a4.z, a4.w };
            q += PB_LPP;
            if (q < q1) j_next = ds.obs_cam[q];
            if (act) {
                ImpObs o; T C[6];
                imp_eval<T>(Rt, dr, focal, pa, o, C);
                const double u0 = o.u[0] + o.xp * dfoc, u1 = o.u[1] + o.yp * dfoc;
                uu += u0 * u0 + u1 * u1;
                zacc[0] += (double)C[0] * u0 + (double)C[3] * u1; zacc[1] += (double)C[1] * u0 + (double)C[4] * u1; zacc[2] += (double)C[2] * u0 + (double)C[5] * u1;
                G[0] += C[0] * C[0] + C[3] * C[3]; G[1] += C[0] * C[1] + C[3] * C[4]; G[2] += C[0] * C[2] + C[3] * C[5];
                G[3] += C[1] * C[1] + C[4] * C[4]; G[4] += C[1] * C[2] + C[4] * C[5]; G[5] += C[2] * C[2] + C[5] * C[5];
            }
        }
    } else {
        int q = q0 + sub;
        int j_next = q < q1 ? ds.obs_cam[q] : 0;
        double ox_next = 0.0, oy_next = 0.0;
        if (q < q1) load_obs<T>(ds.obs_xy, q, ox_next, oy_next);
        while (__any(q < q1)) {
            const bool act = q < q1;
            const int j = j_next;
            const double ox = ox_next, oy = oy_next;
            const CamRow ct = { tab + 4 * (size_t)(j), ds.ncam };
            const CamRow stb = { stab + 4 * (size_t)(j), ds.ncam };
            double Rt[12], dr[8];
#pragma unroll
            for (int e = 0; e < 12; ++e) Rt[e] = ct[CT_R + e];
#pragma unroll
            for (int e = 0; e < 8; ++e) dr[e] = stb[e];
            q += PB_LPP;
            if (q < q1) { j_next = ds.obs_cam[q]; load_obs<T>(ds.obs_xy, q, ox_next, oy_next); }
            if (act) {
                ImpObs o; T C[6];
                imp_eval<T>(Rt, dr, focal, pa, o, C);                    // projection, X_g, u = P (Q dw x X_g + dt), C = (P R) L~
                const double u0 = o.u[0] + o.xp * dfoc, u1 = o.u[1] + o.yp * dfoc;      // + the focal step
                const double r0 = focal * o.xp - ox, r1 = focal * o.yp - oy;
                ur += u0 * r0 + u1 * r1;
                uu += u0 * u0 + u1 * u1;
                zacc[0] += (double)C[0] * u0 + (double)C[3] * u1; zacc[1] += (double)C[1] * u0 + (double)C[4] * u1; zacc[2] += (double)C[2] * u0 + (double)C[5] * u1;
                G[0] += C[0] * C[0] + C[3] * C[3]; G[1] += C[0] * C[1] + C[3] * C[4]; G[2] += C[0] * C[2] + C[3] * C[5];
                G[3] += C[1] * C[1] + C[4] * C[4]; G[4] += C[1] * C[2] + C[4] * C[5]; G[5] += C[2] * C[2] + C[5] * C[5];
            }
        }
    }
#define SFMBA_QUADSUM(x) { x = xlane_add<1>(x); x = xlane_add<2>(x); }
#pragma unroll
    for (int c = 0; c < 3; ++c) SFMBA_QUADSUM(zacc[c])
    SFMBA_QUADSUM(ur) SFMBA_QUADSUM(uu)
    double Gd[6];            // (the lane's own sum in the precision of C, across the quad in fp64 like every cross-lane sum)
#pragma unroll
    for (int c = 0; c < 6; ++c) { Gd[c] = (double)G[c]; SFMBA_QUADSUM(Gd[c]) }
#undef SFMBA_QUADSUM
    // (the point's t and M: loaded here, behind the sweep -- in front of it they cost the sweep its fourth wave per SIMD)
    double tp[3], Mp[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) tp[c] = db.pt_t[3 * i + c];
#pragma unroll
    for (int c = 0; c < 6; ++c) Mp[c] = db.pt_M[6 * i + c];
    const double z0 = tp[0] - zacc[0], z1 = tp[1] - zacc[1], z2 = tp[2] - zacc[2];
    const double dX[3] = { Mp[0] * z0 + Mp[1] * z1 + Mp[2] * z2, Mp[3] * z1 + Mp[4] * z2, Mp[5] * z2 };
    double Xn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) Xn[c] = pa.X[c] - dX[c];
    if (have && sub == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double df = pa.X[c] - Xn[c];
            step2 += df * df;
            xn2 += Xn[c] * Xn[c];
            db.pts[nxt][3 * i + c] = Xn[c];
            if (db.probe_dpt) db.probe_dpt[3 * i + c] = dX[c];
        }
        const double zGz = Gd[0] * z0 * z0 + Gd[3] * z1 * z1 + Gd[5] * z2 * z2 + 2.0 * (Gd[1] * z0 * z1 + Gd[2] * z0 * z2 + Gd[4] * z1 * z2);
        model += ur + (z0 * tp[0] + z1 * tp[1] + z2 * tp[2]) - 0.5 * uu - (z0 * zacc[0] + z1 * zacc[1] + z2 * zacc[2]) - 0.5 * zGz;
    }
    // Trial sweep.  F32J with more cameras than an L1 holds rows of (SFMBA_TRIAL_POSE_MIN_CAMS): three gathers of the trial camera's PARAMETERS and R rebuilt per
    // observation (fp64 sincos on a VALU that is a third busy) instead of six gathers of the stored [R | t] -- measured 142 -> 116 us at BASELINE config 5
    // (1 000 cameras: the pass is bound by its gather instructions), but 23.4 -> 25.4 us at config 3 (200 cameras: it is not), hence the threshold.
    const bool pose_from_cam = sizeof(T) == 4 && ds.ncam >= SFMBA_TRIAL_POSE_MIN_CAMS;
    {
        int q = q0 + sub;
        int j_next = q < q1 ? ds.obs_cam[q] : 0;
        double ox_next = 0.0, oy_next = 0.0;
        if (q < q1) load_obs<T>(ds.obs_xy, q, ox_next, oy_next);
        while (__any(q < q1)) {
            const bool act = q < q1;
            const int j = j_next;
            const double ox = ox_next, oy = oy_next;
            double RTn[12];
            if (pose_from_cam) {
                // the trial camera's six parameters (three 16-byte gathers) and R rebuilt here, instead of six gathers of the stored [R | t]
                const double2* cp = reinterpret_cast<const double2*>(db.cam[nxt] + 6 * (size_t)j);
                const double2 c0 = cp[0], c1 = cp[1], c2 = cp[2];
                const double cn6[6] = { c0.x, c0.y, c1.x, c1.y, c2.x, c2.y };
                pose_from_params(cn6, RTn);
            } else {
                const CamRow stb = { stab + 4 * (size_t)(j), ds.ncam };
#pragma unroll
                for (int e = 0; e < 12; ++e) RTn[e] = stb[ST_RN + e];
            }
            q += PB_LPP;
            if (q < q1) { j_next = ds.obs_cam[q]; load_obs<T>(ds.obs_xy, q, ox_next, oy_next); }
            if (act) {
                const Proj pn = project_point(RTn, 0, 9, Xn);
                const double n0 = focal_n * pn.xp - ox, n1 = focal_n * pn.yp - oy;
                if (!finite_d(n0) || !finite_d(n1)) bad = 1.0;
                trial += n0 * n0 + n1 * n1;
            }
        }
    }
    double sums[5] = { trial, model, step2, xn2, bad };
    const double tot = block_sums<5>(sums, scratch);
    if (threadIdx.x < 5) {
        const int which = threadIdx.x == 0 ? ACC_TRIAL_COST : threadIdx.x == 1 ? ACC_MODEL : threadIdx.x == 2 ? ACC_STEP2 : threadIdx.x == 3 ? ACC_XNEW2 : ACC_BAD_TRIAL;
        if (threadIdx.x < 4 || tot != 0.0) atomicAdd(slot_ptr(db, which), tot);
    }
}

void launch_cam_update(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db) {
    hipLaunchKernelGGL(k_cam_update, dim3((ds.ncam + CU_CAMS - 1) / CU_CAMS), dim3(BLK), 0, s, ds, db);
}

template <typename T>
void launch_point_update(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db) {
    const int per_wg = WPB * (64 / PB_LPP);
    hipLaunchKernelGGL(k_point_update<T>, dim3(std::max(1, (ds.npt + per_wg - 1) / per_wg)), dim3(PBK), 0, s, ds, db);
}
template void launch_point_update<float>(hipStream_t, const DeviceStructure&, const DeviceBuffers&);
template void launch_point_update<double>(hipStream_t, const DeviceStructure&, const DeviceBuffers&);

void launch_control(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db) {
    (void)ds;
    hipLaunchKernelGGL(k_lm_control, dim3(1), dim3(64), 0, s, db);
}

}  // namespace sfmba
