// lm_solve.hip -- the one-GPU LM driver (run_solve) and the host-side pieces every LM loop shares (lm_loop.h).
//
// Every LM iteration is a fixed sequence of kernels on the problem's private HIP stream.  The accept/reject logic runs on the
// device (k_lm_control); the host meets the device once per iteration, at the control kernel's mailbox post, to learn whether to stop.
#include "lm_loop.h"
#include "sfmba_device.h"
#include <dlfcn.h>
#include <mutex>
#include <thread>

namespace sfmba {
namespace {
const char* message_text(int id) {      // MSG_* (ba_kernels.h) -> the reference's wording
    static const char* const text[] = { "", "Gradient tolerance reached.", "Parameter tolerance reached.", "Function tolerance reached.",
        "Minimum trust region radius reached.", "Number of consecutive invalid steps more than max_num_consecutive_invalid_steps.",
        "Initial residual and Jacobian evaluation failed.", "Residual and Jacobian evaluation failed.", "Maximum number of iterations reached.",
        "Maximum solver time reached." };
    static_assert(MSG_NONE == 0 && MSG_MAX_TIME == 9, "message ids index the table");
    return id >= 0 && id <= MSG_MAX_TIME ? text[id] : "";
}

// Host side of the one meeting point per LM iteration: wait until the device has posted sequence number `want` to a
// host-mapped mailbox word.  Three phases so that a solve does not pin a core: a short pause-spin (the common case: the
// post arrives within microseconds of the host getting here), then yielding, then short sleeps.  While waiting, the
// stream is queried now and then: a stream that has drained WITHOUT the post means a launch failed or was lost --
// reported instead of waiting on a wall clock.  Returns 0 = posted, 1 = stream idle and nothing posted, 2 = HIP error.
int wait_mailbox(volatile int* word, int want, hipStream_t stream) {
    const double t0 = now_seconds();
    unsigned spins = 0;
    double next_query = 2e-3;
    for (;;) {
        if (*word >= want) { __sync_synchronize(); return 0; }
        ++spins;
        if ((spins & 63u) != 0u) { __builtin_ia32_pause(); continue; }
        const double waited = now_seconds() - t0;
        if (waited < 30e-6) continue;
        if (waited >= next_query) {
            next_query = waited * 1.5;
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) {
                __sync_synchronize();
                return *word >= want ? 0 : 1;
            }
            if (q != hipErrorNotReady) return 2;
        }
        if (waited < 1e-3) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

// ---- roctx ranges around the phases of an LM iteration: `rocprofv3 --marker-trace` then shows linearise / reduce / solve / update
// per iteration on the host timeline next to the kernels they enqueue.  Bound at run time like RCCL (no link-time dependency); switched on when a
// problem is BUILT with SFMBA_ROCTX=1 in the environment (nothing below sfmba_problem_create* reads the environment). ----
struct RoctxApi { int (*push)(const char*) = nullptr; int (*pop)() = nullptr; };
const RoctxApi* roctx_api() {
    static RoctxApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : { "librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4" }) {
            if (void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
                api.push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
                api.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (api.push && api.pop) break;
                api.push = nullptr; api.pop = nullptr;
            }
        }
    });
    return api.push ? &api : nullptr;
}
struct RoctxRange {
    const RoctxApi* a;
    RoctxRange(bool on, const char* name) : a(on ? roctx_api() : nullptr) { if (a) a->push(name); }
    void end() { if (a) { a->pop(); a = nullptr; } }
    ~RoctxRange() { end(); }
    RoctxRange(const RoctxRange&) = delete;
    RoctxRange& operator=(const RoctxRange&) = delete;
};

__global__ void k_fill(double* p, size_t n, double v) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) p[e] = v;
}

constexpr double auto_cg_tol() { return 1e-12; }      // relative residual AUTO runs the CG to (see run_solve)
}  // namespace

void launch_unit_cscale(sfmba_problem* p) {
    const size_t n = 6 * (size_t)p->ds.ncam;
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, p->stream, p->db.cscale, n, 1.0);
}

LinearPlan linear_plan(const sfmba_options& o, int d, bool always_cg, bool cap_auto_iters) {
    const bool cg_by_options = o.linear_solver == SFMBA_LINEAR_PCG || (o.linear_solver == SFMBA_LINEAR_AUTO && d > 256);
    LinearPlan pl;
    pl.cg = always_cg || cg_by_options;
    // AUTO above 256 unknowns = the DENSE_SCHUR result through the CG: plain relative residual <= 1e-12 (include/sfmba.h)
    pl.exact = always_cg ? o.linear_solver != SFMBA_LINEAR_PCG : cg_by_options && o.linear_solver == SFMBA_LINEAR_AUTO;
    pl.tol = pl.exact ? std::min(o.pcg_tolerance > 0.0 ? o.pcg_tolerance : auto_cg_tol(), auto_cg_tol()) : o.pcg_tolerance;
    pl.max_iters = pl.exact && cap_auto_iters && o.pcg_max_iters <= 0 ? std::min(4 * d, 200) : o.pcg_max_iters;
    pl.anchored = !pl.exact && o.pcg_anchored != 0;
    return pl;
}

int launches_ok() {
    const hipError_t le = hipGetLastError();
    return le == hipSuccess ? SFMBA_OK : fail(SFMBA_ERR_HIP, std::string("kernel launch failed: ") + hipGetErrorString(le));
}
int await_control(sfmba_problem* p, int want, const char* what, const char* lost) {
    if (wait_mailbox(p->h_lm_mail, want, p->stream) == 0) return SFMBA_OK;
    const hipError_t se = hipStreamSynchronize(p->stream);
    return fail(SFMBA_ERR_HIP, std::string(what) + (se != hipSuccess ? hipGetErrorString(se) : lost));
}

void set_termination(sfmba_summary& sum, int termination, int message_id) {
    sum.termination = termination;
    std::snprintf(sum.message, sizeof(sum.message), "%s", message_text(message_id));
}
void fill_summary(sfmba_problem* p, sfmba_summary& sum, double t0) {
    const LMState& hs = *p->h_state;
    p->cur = hs.cur; p->focal = hs.focal[hs.cur];
    sum.iterations = hs.iter; sum.successful_steps = hs.successful; sum.unsuccessful_steps = hs.unsuccessful;
    sum.residual_evals = hs.residual_evals; sum.jacobian_evals = hs.jacobian_evals;
    sum.final_cost = hs.cost;
    sum.seconds = now_seconds() - t0;
}

int read_trace_rows(sfmba_problem* p, TraceRow* rows, int n) {
    if (p->trace_mapped) std::memcpy(rows, p->kit.pinned + 4096, sizeof(TraceRow) * (size_t)n);
    else HIP_TRY(hipMemcpy(rows, p->db.trace, sizeof(TraceRow) * (size_t)n, hipMemcpyDeviceToHost));
    return SFMBA_OK;
}
void copy_trace_out(const TraceRow* rows, int n, sfmba_iteration* trace, int trace_cap, int* trace_len) {
    static_assert(sizeof(TraceRow) == sizeof(sfmba_iteration), "trace row layout");
    if (trace && trace_cap > 0) std::memcpy(trace, rows, sizeof(TraceRow) * (size_t)std::min(n, trace_cap));
    if (trace_len) *trace_len = trace ? std::min(n, std::max(trace_cap, 0)) : n;     // rows written (all rows if only the count was asked for)
}

int probe_arm(sfmba_problem* p) {
    p->db.probe_z = nullptr; p->db.probe_dpt = nullptr;
    p->probe = sfmba_step_probe{};
    if (!p->probe_on) return SFMBA_OK;
    const size_t npt_slots = (size_t)std::max(p->ds.npt, p->own_pt_stride * p->shard_world);
    const size_t need = (size_t)p->ds.ld + 3 * npt_slots;
    if (need > p->probe_cap) {
        if (p->d_probe) (void)hipFree(p->d_probe);
        p->d_probe = nullptr; p->probe_cap = 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p->d_probe), sizeof(double) * need));
        p->probe_cap = need;
    }
    HIP_TRY(hipMemsetAsync(p->d_probe, 0, sizeof(double) * need, p->stream));
    p->db.probe_z = p->d_probe; p->db.probe_dpt = p->d_probe + p->ds.ld;
    return SFMBA_OK;
}
void probe_note(sfmba_problem* p, int family, int f32_matrix, int coarse_vectors, int cholesky_fallback) {
    if (!p->probe_on) return;
    p->probe.family = family; p->probe.f32_matrix = f32_matrix; p->probe.coarse_vectors = coarse_vectors;
    p->probe.cholesky_fallback = cholesky_fallback;
}
void probe_note_solver(sfmba_problem* p, bool pcg, int cholesky_fallback) {
    probe_note(p, p->solver.family, pcg && p->solver.run.path.f32 ? 1 : 0, pcg ? p->solver.coarse_vectors : 0, cholesky_fallback);
}

void init_state(sfmba_problem* p, LMState& st, const sfmba_options& o) {
    std::memset(&st, 0, sizeof(st));
    st.cur = p->cur;
    st.iter = 0;
    st.termination = -1;
    st.x_is_new = 1;
    st.radius = o.initial_radius;
    st.decrease_factor = 2.0;
    st.focal[p->cur] = p->focal;
    st.focal[p->cur ^ 1] = p->focal;
    st.fscale = 1.0;
    st.function_tolerance = o.function_tolerance;
    st.gradient_tolerance = o.gradient_tolerance;
    st.parameter_tolerance = o.parameter_tolerance;
    st.max_radius = o.max_radius;
    st.min_radius = o.min_radius;
    st.min_relative_decrease = o.min_relative_decrease;
    st.min_diag = o.min_lm_diagonal;
    st.max_diag = o.max_lm_diagonal;
    st.max_consecutive_invalid = o.max_consecutive_invalid_steps;
    // An invalid step (the linear solver failed) halves the radius [Ceres-upstream: LevenbergMarquardtStrategy::StepIsInvalid].  In fp64 that is all there
    // is to it -- it does not happen on the problems the oracle solves.  With fp32 Jacobians it is what a trust region that has grown past ~1e7 looks
    // like: the damping diag / radius is then below the rounding of the blocks and the reduced matrix is no longer positive definite; five halvings
    // (a factor 32) do not bring it back and the run ends in FAILURE where the reference converges (tests/fuzz_parity.py: a weakly determined problem,
    // radius 8.6e8).  F32J therefore divides by eight: five in a row cover 3e4.  Runs without invalid steps -- every parity fixture -- are untouched.
    st.invalid_shrink = p->precision == SFMBA_PRECISION_F32J ? 0.125 : 0.5;
}

int upload_state(sfmba_problem* p, const LMState& st) {
    *p->h_state = st;
    HIP_TRY(hipMemcpyAsync(p->db.st, p->h_state, sizeof(LMState), hipMemcpyHostToDevice, p->stream));
    return SFMBA_OK;
}
int download_state(sfmba_problem* p) {
    HIP_TRY(hipMemcpyAsync(p->h_state, p->db.st, sizeof(LMState), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return SFMBA_OK;
}

int ensure_trace(sfmba_problem* p, int rows) {
    if (rows <= p->db.trace_cap) return SFMBA_OK;
    if (p->db.trace && !p->trace_mapped) (void)hipFree(p->db.trace);
    p->db.trace = nullptr;
    p->db.trace_cap = 0;
    p->trace_mapped = false;
    if (p->d_pinned && sizeof(TraceRow) * (size_t)rows <= HOSTKIT_PINNED_BYTES - 4096) {
        // the rows live in the handle's host-mapped block: k_lm_control writes them over PCIe, nothing is copied back
        p->db.trace = reinterpret_cast<TraceRow*>(p->d_pinned + 4096);
        p->trace_mapped = true;
    } else {
        HIP_TRY(dev_alloc(&p->db.trace, (size_t)rows));
    }
    p->db.trace_cap = rows;
    return SFMBA_OK;
}

namespace {
template <typename T>
int run_solve(sfmba_problem* p, const sfmba_options& o, sfmba_summary* summary, sfmba_iteration* trace, int trace_cap, int* trace_len) {
    sfmba_summary sum;
    std::memset(&sum, 0, sizeof(sum));
    if (trace_len) *trace_len = 0;
    if (p->empty) {
        sum.termination = SFMBA_CONVERGENCE;
        std::snprintf(sum.message, sizeof(sum.message), "Function tolerance reached. No non-constant parameter blocks found.");
        if (summary) *summary = sum;
        return SFMBA_OK;
    }
    HIP_TRY(hipSetDevice(p->device));
    const int want_rows = std::min(std::max(o.max_iters, 0) + 2, 1 << 16);
    int rc = ensure_trace(p, want_rows);
    if (rc) return rc;
    if ((rc = probe_arm(p))) return rc;
    // no stream synchronisation here: whatever the caller enqueued before (reset, set_params) is ordered by the stream
    const double t0 = now_seconds();

    LMState st;
    init_state(p, st, o);
    *p->h_state = st;
    { ProfScope ps(p->prof.on ? &p->prof : nullptr, KID_SETUP, p->stream);
      launch_begin(p->stream, p->ds, p->db, st, p->reset_pending ? p->d_cam0 : nullptr, p->reset_pending ? p->d_pts0 : nullptr);
      p->reset_pending = false;
      launch_linearise_setup<T>(p, o.jacobi_scaling, /*begun=*/true); }

    int term = -1, msg = MSG_NONE;
    int host_iter = 0;
    bool state_mirrored = false;
    bool first_linearisation = true;
    bool first_linear_solve = true;
    const bool f32_matrix = option_switch(o.pcg_f32_matrix, true);
    // two-level preconditioner (8 gauge vectors as a coarse space, pcg_common.h)
    const bool coarse_cg = option_switch(o.pcg_coarse_space, true);
    // ... and for a sparsely filled reduced matrix (a camera graph of large diameter) the same vectors restricted to eight segments of the
    // camera order (pcg_segments.hip "Segmented coarse space"); SFMBA_PCG_SEGMENTS=0|1 forces it off / on wherever it applies
    // -- where the structure says the camera order IS that path: a sparsely filled matrix whose blocks sit near the (cyclic) diagonal
    // (options.pcg_coarse_space: 0 = by structure, 1 = the eight global vectors only, 2 = the segments wherever they apply)
    const bool segments_cg = coarse_cg && (dense_pcg_segments_applicable(&p->solver) || dense_pcg_segments_streaming_applicable(&p->solver)) &&
                             option_switch(o.pcg_coarse_space == 2 ? 1 : o.pcg_coarse_space == 1 ? -1 : 0, p->block_fill < 0.5 && p->block_band >= 0.9);
    const bool symmetric_cg = option_switch(o.pcg_symmetric, true) && !p->deterministic &&
                              !(segments_cg && dense_pcg_segments_streaming_applicable(&p->solver));
    // AUTO above 256 unknowns = the DENSE_SCHUR result through the CG: plain relative residual <= 1e-12, bounded iteration count,
    // Cholesky on the same linearisation if the CG does not get there (include/sfmba.h; the fallback is decided where the gated
    // loop learns that the batch was too short)
    const LinearPlan plan = linear_plan(o, p->ds.d, /*always_cg=*/false, /*cap_auto_iters=*/true);
    const bool pcg_mode = plan.cg, exact_pcg = plan.exact;
    // AUTO picks per LM iteration: the CG while it is the cheaper way to the DENSE_SCHUR result, the factorisation once a linearisation
    // has needed more CG iterations than a factorisation costs (measured at d = 1201: 0.41 ms against 6.4 us per iteration = ~64
    // iterations; uniform co-visibility needs 14 per LM iteration, a banded reduced system ~160 -- profiles/r03_*_banded_*).
    const int nblk64 = p->ds.ld / 64;
    const int cg_break_even = std::max(30, (nblk64 <= 40 ? 33 : 20) * nblk64 / 10);
    int launched_controls = 0;
    const bool speculate = option_switch(o.early_linearise, true) && !p->prof.on;
    bool build_enqueued = false;
    std::vector<int> lin_hist;
    int cholesky_fallbacks = 0;
    // AUTO: a linearisation of this solve cost more CG iterations than a factorisation would have.  Local to the solve: a
    // resident problem solved twice from the same point takes the same path twice -- solve / reset / solve is bitwise repeatable in
    // deterministic mode.
    bool auto_prefers_cholesky = false;
    // ... and what the STRUCTURE says before the first iteration: a sparsely filled reduced matrix is a camera graph of large diameter
    // (views along a path, tracks of neighbouring cameras: SfM.cpp:366-469 builds exactly that) -- block-Jacobi CG then needs hundreds of
    // iterations per linearisation (cfg3_banded, fill 0.29: ~160 at 1e-12) and the factorisation is the cheaper way to the DENSE_SCHUR
    // result from the first linearisation on.  A property of the problem, not of the call history: deterministic.
    // (With the segmented coarse space the CG needs ~49 iterations per linearisation at 1e-12 on cfg3_banded: 1 566 LM iterations/s against the
    // factorisation's 1 639 -- the factorisation stays AUTO's choice there; the PCG mode is where the segments pay: 1 224 -> 2 220.)
    // On the streaming path (d > 1280) it is the other way round: a 600-camera path costs 4.5 ms per factorisation against ~1.7 ms for the
    // segmented CG run to 1e-12 (tools/large_banded_check.py) -- AUTO keeps the CG there.
    // (fill alone is not the signature of a path: an unordered but well-connected collection is sparsely filled too and its CG converges in a
    // few iterations -- there the per-solve break-even below decides)
    if (exact_pcg && p->block_fill < 0.5 && p->block_band >= 0.9 && !(segments_cg && dense_pcg_segments_streaming_applicable(&p->solver))) auto_prefers_cholesky = true;
    p->h_lm_mail[0] = 0; p->h_lm_mail[1] = -1;
    for (;;) {
        if (o.max_seconds > 0.0 && now_seconds() - t0 >= o.max_seconds) { term = SFMBA_NO_CONVERGENCE; msg = MSG_MAX_TIME; break; }
        if (host_iter >= o.max_iters) {
            term = SFMBA_NO_CONVERGENCE; msg = MSG_MAX_ITERS;
            if (host_iter == 0) {
                // max_iters <= 0: Ceres still evaluates iteration 0 [Ceres-upstream: TrustRegionMinimizer::IterationZero] -- a non-finite evaluation ends the run
                // there as FAILURE -- and reports that cost as the final one; then the iteration limit is looked at BEFORE the gradient tolerance
                // (FinalizeIterationAndCheckIfMinimizerCanContinue: run time, iteration count, gradient, radius): NO_CONVERGENCE even at a stationary point
                // (tests/fuzz_parity.py --options: the summary used to come back with a cost of 0)
                launch_partial_linearisation<T>(p, o.jacobi_scaling ? 1 : 2);
                launch_finalize(p->stream, p->ds, p->db, 0);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(p->stream));
                rc = download_state(p);
                if (rc) return rc;
                if (p->h_state->termination == SFMBA_FAILURE) { term = p->h_state->termination; msg = p->h_state->message; }
            }
            break;
        }
        Profiler* prof = p->prof.on ? &p->prof : nullptr;
        const bool pcg = pcg_mode && !(exact_pcg && auto_prefers_cholesky);
        if (pcg) {
            if (dense_pcg_ensure_workspace(&p->solver)) return fail(SFMBA_ERR_ALLOC, "PCG workspace allocation failed");
            p->db.pcg_F = p->solver.Sfull;
            p->db.pcg_W = coarse_cg ? p->solver.W : nullptr;
            // fp32 Jacobian mode + streaming CG path: the preconditioned matrix is stored in fp32 (halves the HBM-bound matvec)
            p->db.pcg_F32 = (p->precision == SFMBA_PRECISION_F32J && f32_matrix) ? dense_pcg_want_f32(&p->solver) : nullptr;
            p->solver.use_f32 = p->db.pcg_F32 != nullptr;
            // the streaming CG on ONE triangle of S~ (pcg_symmetric.hip "Symmetric streaming path"); its sums arrive through atomics: not for deterministic handles
            p->solver.symmetric = symmetric_cg && dense_pcg_symmetric_applicable(&p->solver);
            p->db.pcg_upper_only = p->solver.symmetric ? 1 : 0;      // ... and the pair pass then writes that triangle only
            p->db.pcg_zero = p->solver.symmetric ? p->solver.sym_zero : nullptr;        // S~ W~, the CG's products and partial sums: added into with atomics
            p->db.pcg_zero_n = p->solver.symmetric ? (int)p->solver.sym_zero_n : 0;
        }
        RoctxRange rx_iter(p->roctx, "sfmba LM iteration");
        {
        RoctxRange rx(p->roctx, "linearise: point_build + cam_diag");
        if (!build_enqueued) {
            ProfScope ps(prof, KID_POINT_BUILD, p->stream);
            launch_point_build<T>(p->stream, p->ds, p->db, first_linearisation ? (o.jacobi_scaling ? 1 : 2) : 0);
        }
        build_enqueued = false;
        first_linearisation = false;
        { ProfScope ps(prof, KID_CAM_DIAG, p->stream); launch_cam_diag<T>(p->stream, p->ds, p->db); }
        launch_schur_pairs<T>(p->stream, p->ds, p->db, 2);      // duplicate pairs inside diagonal blocks (usually none)
        }
        RoctxRange rx_reduce(p->roctx, "reduce: finalize + schur_pairs (reduced camera system)");
        if (pcg) {
            // the preconditioner (Linv of the damped diagonal blocks) is known before the pair pass, which then writes the
            // preconditioned matrix directly
            { ProfScope ps(prof, KID_FINALIZE, p->stream); launch_finalize(p->stream, p->ds, p->db, 1); }
            { ProfScope ps(prof, KID_SCHUR_PAIRS, p->stream); launch_schur_pairs<T>(p->stream, p->ds, p->db, 1); }
        } else {
            { ProfScope ps(prof, KID_SCHUR_PAIRS, p->stream); launch_schur_pairs<T>(p->stream, p->ds, p->db, 0); }
            { ProfScope ps(prof, KID_FINALIZE, p->stream); launch_finalize(p->stream, p->ds, p->db, 0); }
        }
        rx_reduce.end();
        DeviceBuffers dbu = p->db;
        if (sizeof(T) == 4) dbu.pu32 = p->d_pu32;       // F32J: the back-substitution's first sweep gathers fp32 camera records (ba_step.hip, k_cam_update / k_point_update)
        bool pcg_gated = false;
        bool fell_back = false;
        RoctxRange rx_solve(p->roctx, pcg ? "solve: two-level CG on the reduced system" : "solve: Cholesky of the reduced system");
        if (pcg) {
            // Launch-per-iteration CG: a batch of the length the previous solve needed (+2) goes into the queue together
            // with the three kernels that consume the solution; those are GATED on the CG's done flag, so the host does
            // not wait for the linear solve.  If the batch was too short k_lm_control says so and more is enqueued.
            pcg_gated = true;
            const int it = dense_pcg_solve(p->stream, &p->solver, p->db.S, p->db.rhs, plan.tol, plan.max_iters, p->d_info, prof,
                                           { .finish = false, .hist_key = host_iter, .pretransformed = true, .anchor = plan.anchor(first_linear_solve), .no_wait = true,
                                             .coarse = coarse_cg, .segments = segments_cg });
            first_linear_solve = false;
            if (it < 0) return pcg_refused(it);
            dbu.pcg_vec = p->solver.vec; dbu.pcg_linv = p->solver.binv; dbu.pcg_flags = p->solver.flags;
            dbu.cg_gate = pcg_gated ? p->solver.flags : nullptr;
            dbu.cg_force = 0;
        } else {
            dense_cholesky_solve(p->stream, &p->solver, p->db.S, p->db.rhs, p->d_info, prof);
            lin_hist.push_back(0);
        }
        rx_solve.end();
        RoctxRange rx_update(p->roctx, "update: cam_update + point_update + lm_control (and the wait for its verdict)");
        bool lm_done = false;
        while (!lm_done) {
            launch_back_substitution<T>(p->stream, p->ds, p->ds, dbu, prof);
            probe_note_solver(p, pcg && !fell_back, fell_back ? 1 : 0);
            { ProfScope ps(prof, KID_CONTROL, p->stream); launch_control(p->stream, p->ds, dbu); }
            { ProfScope ps(prof, KID_EMPTY, p->stream); }   // two back-to-back event records: the bracketing overhead itself
            ++launched_controls;
            if ((rc = launches_ok())) return rc;
            // The next linearisation's first kernel goes into the queue BEFORE the host waits for the control kernel's verdict: the
            // mailbox round trip plus the launch latency into an empty queue were 16-19 us of idle GPU per LM iteration.  The kernel
            // looks at the LM state itself and returns at once if the solve ended or the iteration wants more CG first (bit 2).
            if (speculate && host_iter + 2 <= o.max_iters) {
                ProfScope ps(prof, KID_POINT_BUILD, p->stream);
                launch_point_build<T>(p->stream, p->ds, p->db, 4);
                build_enqueued = true;
            }
            // wait for k_lm_control's mailbox post (system-scope stores to host-mapped memory)
            if ((rc = await_control(p, launched_controls, "LM iteration did not complete on the device: ", "stream drained without the control kernel's post"))) return rc;
            volatile int* mb = p->h_lm_mail;
            if (mb[1] == -2) {
                // the CG batch was too short: enqueue more iterations (or force the step once max_iters are spent), then the trio again
                // (the early linearisation kernel behind that control kernel has returned without doing anything)
                if (dense_pcg_more(p->stream, &p->solver, 8, prof) == 0) {
                    if (exact_pcg) {
                        // AUTO: the CG has spent its iterations without reaching 1e-12 -- solve THIS linearisation exactly instead.  The
                        // damped diagonal blocks, the focal column and the right-hand side are in db.S / db.rhs already (camera pass +
                        // k_finalize); the pair pass writes the off-diagonal blocks again, unpreconditioned, and the Cholesky takes over.
                        { ProfScope ps(prof, KID_SCHUR_PAIRS, p->stream); launch_schur_pairs<T>(p->stream, p->ds, p->db, 0); }
                        dense_cholesky_solve(p->stream, &p->solver, p->db.S, p->db.rhs, p->d_info, prof);
                        dbu.pcg_vec = nullptr; dbu.pcg_linv = nullptr; dbu.pcg_flags = nullptr; dbu.cg_gate = nullptr;
                        pcg_gated = false;
                        fell_back = true;
                        ++cholesky_fallbacks;
                    } else {
                        dbu.cg_force = 1;
                    }
                }
                build_enqueued = false;
                continue;
            }
            lm_done = true;
            state_mirrored = true;
            host_iter = mb[3];
            if (mb[1] != -1) { term = mb[1]; msg = mb[2]; }
            if (pcg_gated || (pcg && exact_pcg && dbu.cg_gate == nullptr)) {
                const int it = (pcg_gated || dbu.pcg_vec) ? mb[4] : p->solver.run.launched;      // after a fallback: the launches that were spent
                if (exact_pcg && it > cg_break_even) auto_prefers_cholesky = true;                 // the next linearisations of THIS solve are factorised
                dense_pcg_note(&p->solver, (int)lin_hist.size(), it);
                if (p->probe_on) p->probe.cg_iters = it;
                sum.linear_iters += it;
                lin_hist.push_back(it);
            }
        }
        if (term != -1) break;
        if (o.verbose) {
            rc = download_state(p);
            if (rc) return rc;
            std::fprintf(stderr, "[sfmba] it %3d cost %.12e |g|inf %.3e radius %.3e term %d\n", p->h_state->iter, p->h_state->cost,
                         p->h_state->gmax, p->h_state->radius, p->h_state->termination);
        }
    }
    // The run ends on a LIMIT behind an accepted step: the row of that step reports the gradient AT the accepted point, as Ceres' does
    // (HandleSuccessfulStep evaluates there before FinalizeIterationAndCheckIfMinimizerCanContinue looks at the limits), and that evaluation
    // counts among the jacobian_evals.  Inside the loop it is the next iteration's linearisation that writes it (post_linearisation); here
    // there is none, so the point is linearised once more -- one linearisation per limit exit, nothing on a run that a tolerance ends.  The
    // limit keeps its precedence over the gradient tolerance (the termination stays NO_CONVERGENCE); an evaluation that fails is FAILURE.
    if (host_iter > 0 && term == SFMBA_NO_CONVERGENCE && (msg == MSG_MAX_ITERS || msg == MSG_MAX_TIME) && state_mirrored &&
        p->h_state->termination == -1 && p->h_state->x_is_new) {
        // (as the max_iters = 0 branch above; build_enqueued can be set on the time limit only: the iteration limit is known when the
        // early kernel would be enqueued)
        launch_partial_linearisation<T>(p, 0, /*point_pass_done=*/build_enqueued);
        launch_finalize(p->stream, p->ds, p->db, 0);
        if ((rc = launches_ok())) return rc;
        HIP_TRY(hipStreamSynchronize(p->stream));
        if ((rc = download_state(p))) return rc;
        if (p->h_state->termination == SFMBA_FAILURE) { term = p->h_state->termination; msg = p->h_state->message; }
    }
    // k_lm_control mirrored the LM state into the pinned block before its last mailbox post, and it is the last kernel of
    // an iteration: unless that post was missed (or events have to be collected) there is nothing to wait for or to copy
    if (!state_mirrored || p->prof.on) {
        HIP_TRY(hipStreamSynchronize(p->stream));
        rc = download_state(p);
        if (rc) return rc;
    }
    if (p->prof.on) p->prof.collect();
    fill_summary(p, sum, t0);
    set_termination(sum, term, msg);
    sum.cholesky_fallbacks = cholesky_fallbacks;
    // trace rows
    const int rows = std::min(sum.iterations + 1, p->db.trace_cap);
    std::vector<TraceRow> tr((size_t)std::max(rows, 1));
    if ((rc = read_trace_rows(p, tr.data(), rows))) return rc;
    sum.initial_cost = rows > 0 ? tr[0].cost : sum.final_cost;
    for (int r = 1; r < rows && r - 1 < (int)lin_hist.size(); ++r) tr[(size_t)r].linear_iters = lin_hist[(size_t)r - 1];
    copy_trace_out(tr.data(), rows, trace, trace_cap, trace_len);
    if (summary) *summary = sum;
    return SFMBA_OK;
}
}  // namespace

int run_solve(sfmba_problem* p, const sfmba_options& o, sfmba_summary* summary, sfmba_iteration* trace, int trace_cap, int* trace_len) {
    return with_precision(p, [&](auto t) { return run_solve<decltype(t)>(p, o, summary, trace, trace_cap, trace_len); });
}
}  // namespace sfmba
