// lm_loop.h -- internal: the host side of an LM iteration, one definition of each piece that the loops share (lm_solve.hip): run_solve,
// the two loops of solve_sharded_impl and the step-wise sfmba_shard_* protocol (sharded_solve.hip), the kernel-level entry points (sfmba_api.hip).
#pragma once
#include "problem.h"

namespace sfmba {
void init_state(sfmba_problem* p, LMState& st, const sfmba_options& o);
int upload_state(sfmba_problem* p, const LMState& st);
int download_state(sfmba_problem* p);
int ensure_trace(sfmba_problem* p, int rows);
// Step probe: arms db.probe_z / db.probe_dpt for the next solve (or leaves them null), sized to the current structure ...
int probe_arm(sfmba_problem* p);
// ... and what the host decided for the back-substitution it has just enqueued (the probe describes the last one that ran)
void probe_note(sfmba_problem* p, int family, int f32_matrix, int coarse_vectors, int cholesky_fallback);
void probe_note_solver(sfmba_problem* p, bool pcg, int cholesky_fallback);
// The one-GPU LM driver (sfmba_problem_solve of a handle with a pair list)
int run_solve(sfmba_problem* p, const sfmba_options& o, sfmba_summary* summary, sfmba_iteration* trace, int trace_cap, int* trace_len);

// ... and of one without (SFMBA_CREATE_NO_PAIR_LIST): the CG loop of the sharded path on one rank, matrix-free (sharded_solve.hip)
int solve_matrix_free(sfmba_problem* p, const sfmba_options& o, sfmba_summary* summary, sfmba_iteration* trace, int trace_cap, int* trace_len);

void launch_unit_cscale(sfmba_problem* p);      // camera column scales := 1 (k_fill's one launcher: the library has no relocatable device code)

// The back-substitution is ONE step in two launches that share a convention: in F32J k_cam_update writes the fp32 camera records (pu32) AND adds
// the gradient . step term of the model cost change, and k_point_update<float> then forms no residual term -- pairing a cam_update that saw pu32 with a
// point_update that did not (or the other way round) would count that term twice or not at all and skew the step quality rho.  Every LM loop goes through
// this helper: both kernels see the SAME DeviceBuffers, and an fp64 point pass can never meet a pu32 camera pass.  ds_points: the point pass's structure
// (a row-sharded rank passes the view with its own point range).
template <typename T>
void launch_back_substitution(hipStream_t s, const DeviceStructure& ds, const DeviceStructure& ds_points, const DeviceBuffers& dbu, Profiler* prof) {
    DeviceBuffers b = dbu;
    if (sizeof(T) == 8) b.pu32 = nullptr;
    { ProfScope ps(prof, KID_CAM_UPDATE, s); launch_cam_update(s, ds, b); }
    { ProfScope ps(prof, KID_POINT_UPDATE, s); launch_point_update<T>(s, ds_points, b); }
}

template <typename T>
void launch_linearise_setup(sfmba_problem* p, int jacobi, bool begun = false) {
    if (begun) {
        // inside a solve: k_begin has written the LM state, cleared the accumulators and built the camera tables; the point
        // scales are formed by the first k_point_build; ||x|| is finished by k_colnorm_finish
        // (||x||^2 rides in the camera pass of the column norms where that pass runs: k_xnorm as a launch of its own was 4.6 us per solve)
        const bool fold = jacobi && p->ds.nchunk_coarse > 0;
        if (!fold) launch_xnorm(p->stream, p->ds, p->db);
        launch_colnorm<T>(p->stream, p->ds, p->db, jacobi, /*clear_udiag=*/false, /*points=*/false, /*finish_xnorm=*/true, /*with_xnorm=*/fold);
        return;
    }
    launch_unit_cscale(p);
    launch_cam_setup<T>(p->stream, p->ds, p->db, p->cur);
    launch_xnorm(p->stream, p->ds, p->db);
    launch_iter0(p->stream, p->ds, p->db);
    launch_colnorm<T>(p->stream, p->ds, p->db, jacobi);
}

// The partial linearisation: per-point table, camera diagonal, duplicate pairs inside diagonal blocks, off-diagonal blocks of S (unpreconditioned).
// ps_mode: launch_point_build (0: point scales from db.pscale; 1 / 2: form them here).  point_pass_done: the early linearisation kernel
// behind the last control kernel (launch_point_build, mode 4) has run the point pass at this very point already.
template <typename T>
void launch_partial_linearisation(sfmba_problem* p, int ps_mode, bool point_pass_done = false) {
    if (!point_pass_done) launch_point_build<T>(p->stream, p->ds, p->db, ps_mode);
    launch_cam_diag<T>(p->stream, p->ds, p->db);
    launch_schur_pairs<T>(p->stream, p->ds, p->db, 2);
    launch_schur_pairs<T>(p->stream, p->ds, p->db, 0);
}

// How the reduced system of a linearisation is solved, from (options, d).
struct LinearPlan {
    bool cg;            // the CG (else: the factorisation)
    bool exact;         // ... run as AUTO's way to the DENSE_SCHUR result: plain relative residual <= 1e-12, not anchored
    double tol;
    int max_iters;      // 0 = the CG's own bound
    bool anchored;
    int anchor(bool first_solve) const { return anchored ? (first_solve ? 1 : 2) : 0; }
};
// always_cg: the caller runs the CG whatever the options say, and everything that is not SFMBA_LINEAR_PCG is then the exact CG;
// cap_auto_iters: AUTO's CG gives up after min(4 d, 200) iterations (the caller has a factorisation to fall back on).
LinearPlan linear_plan(const sfmba_options& o, int d, bool always_cg, bool cap_auto_iters);
// The symmetric streaming path is run_solve's alone: every other CG user resets the solver and the pair pass to both triangles of S~
inline void keep_both_triangles(sfmba_problem* p) { p->solver.symmetric = false; p->db.pcg_upper_only = 0; p->db.pcg_zero = nullptr; p->db.pcg_zero_n = 0; }

// Every launch of an LM iteration is in the queue: a failed launch must not leave the host waiting for a post
int launches_ok();
// dense_pcg_solve returned it < 0 (nothing is running): the error code and message of the call
inline int pcg_refused(int it) {
    if (it == PCG_ERR_LAUNCH) { const int rc = launches_ok(); if (rc) return rc; }
    return fail(it == PCG_ERR_TOO_LARGE ? SFMBA_ERR_INVALID_ARG : it == PCG_ERR_LAUNCH ? SFMBA_ERR_HIP : SFMBA_ERR_ALLOC, dense_pcg_error(it));
}
// Waits for k_lm_control's mailbox post number `want`; a stream that drained without it is SFMBA_ERR_HIP: `what` + the HIP error, or + `lost`
int await_control(sfmba_problem* p, int want, const char* what, const char* lost);
void set_termination(sfmba_summary& sum, int termination, int message_id);
// LMState (mirrored or downloaded into p->h_state) -> the counters and costs of a summary; p->cur / p->focal follow the accepted point
void fill_summary(sfmba_problem* p, sfmba_summary& sum, double t0);
int read_trace_rows(sfmba_problem* p, TraceRow* rows, int n);       // out of the pinned block, or from the device
void copy_trace_out(const TraceRow* rows, int n, sfmba_iteration* trace, int trace_cap, int* trace_len);
}  // namespace sfmba
