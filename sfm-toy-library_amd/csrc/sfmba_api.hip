// sfmba_api.hip -- C ABI of include/sfmba.h: the error state, the device checks and the problem / solver entry points (argument
// checks and dispatch).  The work is in problem_build.hip (structure build), lm_solve.hip (LM driver), sharded_solve.hip (multi-GPU
// and matrix-free loops), comm_rccl.hip and the kernel units; the front-end entry points are in api_frontend.hip.
//
// There is NO CPU fallback in this library: without a HIP device every entry point returns SFMBA_ERR_NO_DEVICE.
#include "lm_loop.h"
#include "pcg_common.h"
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

using namespace sfmba;

namespace { thread_local std::string g_last_error; }

int sfmba::fail(int rc, const std::string& msg) { g_last_error = msg; return rc; }

int sfmba::check_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(SFMBA_ERR_NO_DEVICE, "no HIP device available: the MI355X back end has no CPU fallback");
    if (device < 0 || device >= n) return fail(SFMBA_ERR_INVALID_ARG, "device index out of range");
    return SFMBA_OK;
}

int sfmba::check_handle(const sfmba_problem* p, bool may_be_empty) {
    if (!p) return fail(SFMBA_ERR_INVALID_ARG, may_be_empty ? "NULL problem" : "NULL or empty problem");
    if (p->poisoned) return fail(SFMBA_ERR_INVALID_ARG, "poisoned problem (a failed sfmba_problem_append): destroy it");
    if (p->empty && !may_be_empty) return fail(SFMBA_ERR_INVALID_ARG, "NULL or empty problem");
    return SFMBA_OK;
}

// the LM state of a handle that no solve has touched since its parameters were (re)set
static int upload_default_state(sfmba_problem* p) {
    sfmba_options o;
    sfmba_options_default(&o);
    LMState st;
    init_state(p, st, o);
    return upload_state(p, st);
}

// the device side of a reset, for the callers that are not a solve
int sfmba::flush_reset(sfmba_problem* p) {
    if (!p || !p->reset_pending) return SFMBA_OK;
    p->reset_pending = false;
    if (p->empty) return SFMBA_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpyAsync(p->db.cam[0], p->d_cam0, sizeof(double) * 6 * (size_t)p->ds.ncam, hipMemcpyDeviceToDevice, p->stream));
    HIP_TRY(hipMemcpyAsync(p->db.pts[0], p->d_pts0, sizeof(double) * 3 * (size_t)p->ds.npt, hipMemcpyDeviceToDevice, p->stream));
    return upload_default_state(p);
}

// The device keeps the reduced unknowns in SLOT order; the test hooks hand them out as include/sfmba.h states it: active cameras by
// ascending caller index, focal last.  Empty when the slots already ascend (every fresh create: the device arrays go out as they are);
// otherwise src[i] = the device unknown that unknown i of the caller is (an append that registered cameras out of index order).
static std::vector<int> reduced_unknown_order(const sfmba_problem* p) {
    const std::vector<int>& id = p->acam_id;
    std::vector<int> src;
    if (std::is_sorted(id.begin(), id.end())) return src;
    const int ncam = (int)id.size();
    std::vector<int> slots((size_t)ncam);
    for (int j = 0; j < ncam; ++j) slots[(size_t)j] = j;
    std::sort(slots.begin(), slots.end(), [&](int a, int b) { return id[(size_t)a] < id[(size_t)b]; });
    src.resize((size_t)6 * ncam + 1);
    for (int r = 0; r < ncam; ++r)
        for (int c = 0; c < 6; ++c) src[6 * (size_t)r + c] = 6 * slots[(size_t)r] + c;
    src[(size_t)6 * ncam] = 6 * ncam;
    return src;
}

// out[i] = device[src[i]] for a vector of the reduced unknowns (src empty: a plain copy)
static int download_reduced_vector(double* out, const double* d_vec, int d, const std::vector<int>& src) {
    if (src.empty()) { HIP_TRY(hipMemcpy(out, d_vec, sizeof(double) * (size_t)d, hipMemcpyDeviceToHost)); return SFMBA_OK; }
    std::vector<double> h((size_t)d);
    HIP_TRY(hipMemcpy(h.data(), d_vec, sizeof(double) * (size_t)d, hipMemcpyDeviceToHost));
    for (int i = 0; i < d; ++i) out[i] = h[(size_t)src[(size_t)i]];
    return SFMBA_OK;
}

extern "C" {
void sfmba_options_default(sfmba_options* o) {
    std::memset(o, 0, sizeof(*o));
    o->max_iters = 500;               // BA.cpp:174
    o->max_seconds = 10.0;            // BA.cpp:176
    o->function_tolerance = 1e-6;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
    o->initial_radius = 1e4;
    o->max_radius = 1e16;
    o->min_radius = 1e-32;
    o->min_relative_decrease = 1e-3;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->jacobi_scaling = 1;
    o->max_consecutive_invalid_steps = 5;
    o->linear_solver = SFMBA_LINEAR_AUTO;       // DENSE_SCHUR-equivalent result (BA.cpp:172), cheapest solver that delivers it
    o->precision = SFMBA_PRECISION_F64;
    o->pcg_tolerance = 1e-8;
    o->pcg_max_iters = 0;
    o->verbose = 0;
    o->pcg_anchored = 1;
}

int sfmba_abi_version(void) { return SFMBA_ABI_VERSION; }

const char* sfmba_last_error(void) { return g_last_error.c_str(); }

long long sfmba_release_cache(void) { return (long long)arena_cache_release(); }

int sfmba_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

namespace { __global__ void k_warm(int* p) { if (p && threadIdx.x == 0) *p = 1; } }

// What the first call of a process pays once (measured at BASELINE config 3, profiles/r05_b_shim_incremental.txt: 138 ms of which 113 in
// sfmba_problem_create -- the HIP context, the first pinned allocation, the first device chunks -- against 2.6 - 3 ms for every later adjustBundle()):
// a host can pay it at start-up instead.  Creates the context, one stream + pinned block (cached for the first problem), a pinned upload buffer and
// device chunks for a problem of `expected_obs` observations (0: contexts and the fixed-size pieces only), launches one kernel.  Idempotent.
int sfmba_device_warmup(int device, int64_t expected_obs) {
    if (expected_obs < 0) return fail(SFMBA_ERR_INVALID_ARG, "negative size");
    int rc = check_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(nullptr));
    HostKit kit;
    if (!hostkit_acquire(device, &kit)) return fail(SFMBA_ERR_HIP, "stream / pinned memory creation failed");
    struct KitGuard { HostKit* k; ~KitGuard() { if (k->stream) (void)hipStreamSynchronize(k->stream); hostkit_release(*k); } } kg{ &kit };
    if (expected_obs > 0) (void)hostkit_upload(&kit, std::min((size_t)HOSTKIT_UPLOAD_MAX, (size_t)expected_obs * 24));      // (camera, point, xy as doubles: the packed upload of a build)
    {
        DeviceArena arena(device);
        // a resident problem holds ~150 bytes per observation in structure, tables and sort temporaries (18 + 20 + 12 + 18 MB ... at one million: DESIGN.md section 3)
        const size_t want = (size_t)(4 << 20) + (size_t)expected_obs * 160;
        int* flag = static_cast<int*>(arena.alloc(want));
        if (!flag) return fail(SFMBA_ERR_ALLOC, "device allocation failed");
        hipLaunchKernelGGL(k_warm, dim3(1), dim3(64), 0, kit.stream, flag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(kit.stream));
        arena.release();          // -> the chunk cache the first problem draws from
    }
    return SFMBA_OK;
}

int sfmba_problem_reset(sfmba_problem* p) {
    if (const int hrc = check_handle(p)) return hrc;
    p->focal = p->focal0;
    p->cur = 0;
    // nothing is enqueued here: the next solve's first kernel copies the initial parameters itself (k_begin); any other entry point
    // that looks at the parameters flushes the reset first
    p->reset_pending = !p->empty;
    return SFMBA_OK;
}

int sfmba_problem_set_params(sfmba_problem* p, const double* cam6, const double* pt3, double focal) {
    if (!p || !cam6 || !pt3) return fail(SFMBA_ERR_INVALID_ARG, "NULL argument");
    if (const int hrc = check_handle(p)) return hrc;
    p->reset_pending = false;           // everything a reset would restore is overwritten here
    p->focal = focal;
    p->cur = 0;
    if (p->empty) return SFMBA_OK;
    HIP_TRY(hipSetDevice(p->device));
    std::vector<double> cam((size_t)6 * p->ds.ncam), pts((size_t)3 * p->ds.npt);
    for (int j = 0; j < p->ds.ncam; ++j) std::memcpy(&cam[6 * (size_t)j], cam6 + 6 * (size_t)p->acam_id[j], 6 * sizeof(double));
    for (int i = 0; i < p->ds.npt; ++i) std::memcpy(&pts[3 * (size_t)i], pt3 + 3 * (size_t)p->apt_id[i], 3 * sizeof(double));
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipMemcpy(p->db.cam[0], cam.data(), sizeof(double) * cam.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p->db.pts[0], pts.data(), sizeof(double) * pts.size(), hipMemcpyHostToDevice));
    return upload_default_state(p);
}

int sfmba_problem_get_params(sfmba_problem* p, double* cam6, double* pt3, double* focal) {
    if (p && !p->poisoned) { const int frc = flush_reset(p); if (frc) return frc; }
    if (const int hrc = check_handle(p)) return hrc;
    if (focal) *focal = p->focal;
    if (p->empty) return SFMBA_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    // slot == caller index everywhere (the usual case): straight into the caller's arrays, no gathered copy
    if (cam6) {
        if (p->cam_identity) HIP_TRY(hipMemcpy(cam6, p->db.cam[p->cur], sizeof(double) * 6 * (size_t)p->ds.ncam, hipMemcpyDeviceToHost));
        else {
            std::vector<double> cam((size_t)6 * p->ds.ncam);
            HIP_TRY(hipMemcpy(cam.data(), p->db.cam[p->cur], sizeof(double) * cam.size(), hipMemcpyDeviceToHost));
            for (int j = 0; j < p->ds.ncam; ++j) std::memcpy(cam6 + 6 * (size_t)p->acam_id[j], &cam[6 * (size_t)j], 6 * sizeof(double));
        }
    }
    if (pt3) {
        if (p->pt_identity) HIP_TRY(hipMemcpy(pt3, p->db.pts[p->cur], sizeof(double) * 3 * (size_t)p->ds.npt, hipMemcpyDeviceToHost));
        else {
            std::vector<double> pts((size_t)3 * p->ds.npt);
            HIP_TRY(hipMemcpy(pts.data(), p->db.pts[p->cur], sizeof(double) * pts.size(), hipMemcpyDeviceToHost));
            for (int i = 0; i < p->ds.npt; ++i) std::memcpy(pt3 + 3 * (size_t)p->apt_id[i], &pts[3 * (size_t)i], 3 * sizeof(double));
        }
    }
    return SFMBA_OK;
}

int sfmba_problem_solve(sfmba_problem* p, const sfmba_options* opt, sfmba_summary* summary,
                        sfmba_iteration* trace, int trace_cap, int* trace_len) {
    if (const int hrc = check_handle(p)) return hrc;
    if (p->row_sharded) return fail(SFMBA_ERR_INVALID_ARG, "a row-sharded problem is solved with sfmba_problem_solve_sharded only");
    sfmba_options o;
    if (opt) o = *opt; else sfmba_options_default(&o);
    if (p->no_pairs && !p->empty) return solve_matrix_free(p, o, summary, trace, trace_cap, trace_len);
    return run_solve(p, o, summary, trace, trace_cap, trace_len);
}

void* sfmba_problem_stream(sfmba_problem* p) { return p ? (void*)p->stream : nullptr; }

int sfmba_problem_reduced_dim(const sfmba_problem* p) { return p && !p->empty ? p->ds.d : 0; }

int sfmba_solve(int n_cam, double* cam6, int n_pt, double* pt3, int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt,
                const double* obs_xy, double* focal, const sfmba_options* opt, sfmba_summary* summary,
                sfmba_iteration* trace, int trace_cap, int* trace_len) {
    if (!focal) return fail(SFMBA_ERR_INVALID_ARG, "focal is NULL");
    sfmba_options o;
    if (opt) o = *opt; else sfmba_options_default(&o);
    const double t0 = now_seconds();
    sfmba_problem* p = nullptr;
    int rc = sfmba_problem_create(0, o.precision, n_cam, cam6, n_pt, pt3, n_obs, obs_cam, obs_pt, obs_xy, *focal, &p);
    if (rc) return rc;
    const double setup = now_seconds() - t0;
    sfmba_summary sum;
    std::memset(&sum, 0, sizeof(sum));
    rc = sfmba_problem_solve(p, &o, &sum, trace, trace_cap, trace_len);
    // Ceres leaves the user's parameter blocks untouched when the solve terminates with FAILURE (solver.cc: "do not update
    // user state" [Ceres-upstream]); every other termination writes the best accepted point back
    if (rc == SFMBA_OK && sum.termination != SFMBA_FAILURE) rc = sfmba_problem_get_params(p, cam6, pt3, focal);
    sum.setup_seconds = setup;
    if (summary && rc == SFMBA_OK) *summary = sum;
    sfmba_problem_destroy(p);
    return rc;
}

int sfmba_problem_set_profiling(sfmba_problem* p, int enable) {
    if (const int hrc = check_handle(p)) return hrc;
    p->prof.reset();
    p->prof.on = enable != 0;
    return SFMBA_OK;
}

int sfmba_problem_get_profile(sfmba_problem* p, sfmba_kernel_time* out, int cap, int* n) {
    if (!p || !n) return fail(SFMBA_ERR_INVALID_ARG, "NULL argument");
    int k = 0;
    for (int id = 0; id < KID_COUNT; ++id) {
        if (p->prof.count[id] == 0) continue;
        if (out && k < cap) {
            std::snprintf(out[k].name, sizeof(out[k].name), "%s", kernel_name(id));
            out[k].total_us = 1e3 * p->prof.total_ms[id];
            out[k].launches = p->prof.count[id];
        }
        ++k;
    }
    *n = k;
    return SFMBA_OK;
}

int sfmba_problem_set_step_probe(sfmba_problem* p, int enable) {
    if (const int hrc = check_handle(p)) return hrc;
    HIP_TRY(hipSetDevice(p->device));
    if (p->stream) HIP_TRY(hipStreamSynchronize(p->stream));
    p->probe_on = enable != 0;
    p->probe = sfmba_step_probe{};
    p->db.probe_z = nullptr; p->db.probe_dpt = nullptr;      // (armed by the next solve)
    if (!p->probe_on && p->d_probe) { (void)hipFree(p->d_probe); p->d_probe = nullptr; p->probe_cap = 0; }
    return SFMBA_OK;
}

int sfmba_problem_get_step_probe(sfmba_problem* p, double* z, double* dpt, sfmba_step_probe* info) {
    if (!p) return fail(SFMBA_ERR_INVALID_ARG, "NULL problem");
    if (!p->probe_on) return fail(SFMBA_ERR_INVALID_ARG, "the step probe is off (sfmba_problem_set_step_probe)");
    if (info) *info = p->probe;
    if (p->probe.family == 0 || !p->d_probe) return SFMBA_OK;      // no back-substitution has run since the probe was enabled
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (z) { const int zrc = download_reduced_vector(z, p->d_probe, p->ds.d, reduced_unknown_order(p)); if (zrc) return zrc; }
    if (dpt) {
        const int npt = (int)p->apt_id.size();
        std::vector<double> h((size_t)3 * std::max(npt, 1));
        if (npt > 0) HIP_TRY(hipMemcpy(h.data(), p->d_probe + p->ds.ld, sizeof(double) * 3 * (size_t)npt, hipMemcpyDeviceToHost));
        std::memset(dpt, 0, sizeof(double) * 3 * (size_t)p->n_pt_full);
        for (int i = 0; i < npt; ++i)
            for (int c = 0; c < 3; ++c) dpt[3 * (size_t)p->apt_id[i] + c] = h[3 * (size_t)i + c];
    }
    return SFMBA_OK;
}

// ---- kernel-level entry points ----------------------------------------------------------------
int sfmba_problem_eval_residuals(sfmba_problem* p, double* residuals_out, double* cost_out) {
    if (p && !p->poisoned) { const int frc = flush_reset(p); if (frc) return frc; }
    if (const int hrc = check_handle(p)) return hrc;
    if (cost_out) *cost_out = 0.0;
    if (p->empty) return SFMBA_OK;
    HIP_TRY(hipSetDevice(p->device));
    double *d_res = nullptr, *d_cost = nullptr;
    DeviceTemps tmp(&d_res, &d_cost);
    HIP_TRY(dev_alloc(&d_res, (size_t)2 * p->ds.nobs));
    HIP_TRY(dev_alloc(&d_cost, 1));
    HIP_TRY(hipMemsetAsync(d_cost, 0, sizeof(double), p->stream));
    launch_unit_cscale(p);
    launch_cam_setup<double>(p->stream, p->ds, p->db, p->cur);
    with_precision(p, [&](auto t) { launch_eval_residuals<decltype(t)>(p->stream, p->ds, p->db, p->d_obs_pt, d_res, d_cost); });
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (residuals_out) HIP_TRY(hipMemcpy(residuals_out, d_res, sizeof(double) * 2 * (size_t)p->ds.nobs, hipMemcpyDeviceToHost));
    if (cost_out) HIP_TRY(hipMemcpy(cost_out, d_cost, sizeof(double), hipMemcpyDeviceToHost));
    return SFMBA_OK;
}

int sfmba_problem_eval_jacobian(sfmba_problem* p, double* jc, double* jp, double* jf) {
    if (p && !p->poisoned) { const int frc = flush_reset(p); if (frc) return frc; }
    if (const int hrc = check_handle(p)) return hrc;
    if (p->empty) return SFMBA_OK;
    HIP_TRY(hipSetDevice(p->device));
    const size_t n = (size_t)p->ds.nobs;
    double *d_jc = nullptr, *d_jp = nullptr, *d_jf = nullptr;
    DeviceTemps tmp(&d_jc, &d_jp, &d_jf);
    if (jc) HIP_TRY(dev_alloc(&d_jc, 12 * n));
    if (jp) HIP_TRY(dev_alloc(&d_jp, 6 * n));
    if (jf) HIP_TRY(dev_alloc(&d_jf, 2 * n));
    launch_unit_cscale(p);
    launch_cam_setup<double>(p->stream, p->ds, p->db, p->cur);
    with_precision(p, [&](auto t) { launch_eval_jacobian<decltype(t)>(p->stream, p->ds, p->db, p->d_obs_pt, p->d_perm, d_jc, d_jp, d_jf); });
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (jc) HIP_TRY(hipMemcpy(jc, d_jc, sizeof(double) * 12 * n, hipMemcpyDeviceToHost));
    if (jp) HIP_TRY(hipMemcpy(jp, d_jp, sizeof(double) * 6 * n, hipMemcpyDeviceToHost));
    if (jf) HIP_TRY(hipMemcpy(jf, d_jf, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
    return SFMBA_OK;
}

int sfmba_problem_build_reduced(sfmba_problem* p, const sfmba_options* opt, double radius, double* S, double* rhs, double* scale) {
    if (p && !p->poisoned) { const int frc = flush_reset(p); if (frc) return frc; }
    if (const int hrc = check_handle(p, /*may_be_empty=*/false)) return hrc;
    if (p->row_sharded) return fail(SFMBA_ERR_INVALID_ARG, "a row-sharded problem is solved with sfmba_problem_solve_sharded only");
    if (p->no_pairs) return fail(SFMBA_ERR_INVALID_ARG, "this problem has no pair list (SFMBA_CREATE_NO_PAIR_LIST / too many pairs): its reduced matrix is never formed");
    sfmba_options o;
    if (opt) o = *opt; else sfmba_options_default(&o);
    HIP_TRY(hipSetDevice(p->device));
    LMState st;
    init_state(p, st, o);
    st.radius = radius;
    int rc = upload_state(p, st);
    if (rc) return rc;
    rc = ensure_trace(p, 4);
    if (rc) return rc;
    with_precision(p, [&](auto t) {
        launch_linearise_setup<decltype(t)>(p, o.jacobi_scaling);
        launch_partial_linearisation<decltype(t)>(p, /*ps_mode=*/0);
    });
    launch_finalize(p->stream, p->ds, p->db, 0);
    const int d = p->ds.d;
    double *d_full = nullptr, *d_scale = nullptr;
    DeviceTemps tmp(&d_full, &d_scale);
    HIP_TRY(dev_alloc(&d_full, (size_t)d * d));
    HIP_TRY(dev_alloc(&d_scale, (size_t)d));
    launch_mirror_scale(p->stream, p->ds, p->db, d_full, d_scale);
    HIP_TRY(hipStreamSynchronize(p->stream));
    const std::vector<int> src = reduced_unknown_order(p);
    if (S) {
        if (src.empty()) HIP_TRY(hipMemcpy(S, d_full, sizeof(double) * (size_t)d * d, hipMemcpyDeviceToHost));
        else {
            std::vector<double> h((size_t)d * d);
            HIP_TRY(hipMemcpy(h.data(), d_full, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
            for (int r = 0; r < d; ++r) {
                const double* row = &h[(size_t)src[(size_t)r] * d];
                for (int c = 0; c < d; ++c) S[(size_t)r * d + c] = row[(size_t)src[(size_t)c]];
            }
        }
    }
    if (rhs) { rc = download_reduced_vector(rhs, p->db.rhs, d, src); if (rc) return rc; }
    if (scale) { rc = download_reduced_vector(scale, d_scale, d, src); if (rc) return rc; }
    return SFMBA_OK;
}

int sfmba_dense_spd_solve(int device, int n, const double* A, const double* b, double* x, int method,
                          double pcg_tol, int pcg_max_iters, int* info, int* iters) {
    if (n <= 0 || !A || !b || !x) return fail(SFMBA_ERR_INVALID_ARG, "bad arguments");
    int rc = check_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    const int ld = dense_padded_dim(n);
    std::vector<double> Ap((size_t)ld * ld, 0.0), bp((size_t)ld, 0.0);
    for (int r = 0; r < n; ++r) for (int c = r; c < n; ++c) Ap[(size_t)r * ld + c] = A[(size_t)r * n + c];
    for (int e = n; e < ld; ++e) Ap[(size_t)e * ld + e] = 1.0;
    std::memcpy(bp.data(), b, sizeof(double) * (size_t)n);
    double *dA = nullptr, *db_ = nullptr;
    int* dinfo = nullptr;
    DeviceTemps tmp(&dA, &db_, &dinfo);
    HIP_TRY(dev_upload(&dA, Ap));
    HIP_TRY(dev_upload(&db_, bp));
    HIP_TRY(dev_alloc(&dinfo, 1));
    HIP_TRY(hipMemset(dinfo, 0, sizeof(int)));
    DenseSolver ws;
    if (dense_solver_create(&ws, n, ld)) return fail(SFMBA_ERR_ALLOC, "dense solver workspace allocation failed");
    hipStream_t s = nullptr;
    struct Guard { DenseSolver* ws; hipStream_t* s; ~Guard() { dense_solver_destroy(ws); if (*s) (void)hipStreamDestroy(*s); } } guard{ &ws, &s };
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    int it = 0;
    if (method == SFMBA_LINEAR_PCG) it = dense_pcg_solve(s, &ws, dA, db_, pcg_tol > 0 ? pcg_tol : 1e-10, pcg_max_iters, dinfo);
    else dense_cholesky_solve(s, &ws, dA, db_, dinfo);
    
    if (it < 0) return pcg_refused(it);
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(x, db_, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    int hinfo = 0;
    HIP_TRY(hipMemcpy(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost));
    if (info) *info = hinfo;
    if (iters) *iters = it;
    return SFMBA_OK;
}

int sfmba_dense_pcg_probe(int device, int n, const double* A, int nrhs, const double* B, const double* Wt, int flags, double tol,
                          const int* max_iters, double* X, int* info, int* iters, sfmba_step_probe* path) {
    constexpr int known = SFMBA_PCG_PROBE_SYMMETRIC | SFMBA_PCG_PROBE_F32_MATRIX | SFMBA_PCG_PROBE_SEGMENTS | SFMBA_PCG_PROBE_POISON;
    if (n <= 0 || nrhs <= 0 || !A || !B || !X || !max_iters || !(tol > 0.0) || (flags & ~known)) return fail(SFMBA_ERR_INVALID_ARG, "bad arguments");
    for (int i = 0; i < nrhs; ++i)
        if (max_iters[i] <= 0 || max_iters[i] > 1000) return fail(SFMBA_ERR_INVALID_ARG, "max_iters must lie in 1 .. 1000");
    if ((flags & SFMBA_PCG_PROBE_SEGMENTS) && !Wt) return fail(SFMBA_ERR_INVALID_ARG, "the segmented coarse space needs Wt");
    int rc = check_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    const int ld = dense_padded_dim(n);
    double *dA = nullptr, *db_ = nullptr;
    int* dinfo = nullptr;
    DeviceTemps tmp(&dA, &db_, &dinfo);
    HIP_TRY(dev_alloc(&dA, (size_t)n * ld));
    HIP_TRY(hipMemset(dA, 0, sizeof(double) * (size_t)n * ld));
    HIP_TRY(hipMemcpy2D(dA, sizeof(double) * (size_t)ld, A, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(dev_alloc(&db_, (size_t)ld));
    HIP_TRY(dev_alloc(&dinfo, 1));
    HIP_TRY(hipMemset(dinfo, 0, sizeof(int)));
    DenseSolver ws;
    if (dense_solver_create(&ws, n, ld)) return fail(SFMBA_ERR_ALLOC, "dense solver workspace allocation failed");
    hipStream_t s = nullptr;
    struct Guard { DenseSolver* ws; hipStream_t* s; ~Guard() { dense_solver_destroy(ws); if (*s) (void)hipStreamDestroy(*s); } } guard{ &ws, &s };
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    // what a handle sets per solve (lm_solve.hip): the triangle the product reads, the matrix precision, the coarse vectors
    ws.symmetric = (flags & SFMBA_PCG_PROBE_SYMMETRIC) != 0;
    ws.use_f32 = (flags & SFMBA_PCG_PROBE_F32_MATRIX) != 0 && dense_pcg_want_f32(&ws) != nullptr;
    if (dense_pcg_ensure_workspace(&ws)) return fail(SFMBA_ERR_ALLOC, dense_pcg_error(PCG_ERR_ALLOC));
    const size_t wn = (size_t)PCG_NW * ld + pcg_tile_slack(n, ld);
    PcgSolveOptions o;
    o.pretransformed = true; o.coarse = Wt != nullptr; o.segments = (flags & SFMBA_PCG_PROBE_SEGMENTS) != 0;
    const CgPath plan = dense_pcg_path(&ws, o.coarse, o.segments);
    for (int i = 0; i < nrhs; ++i) {
        HIP_TRY(hipMemsetAsync(db_, 0, sizeof(double) * (size_t)ld, s));
        HIP_TRY(hipMemcpyAsync(db_, B + (size_t)i * n, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(ws.W, 0, sizeof(double) * wn, s));
        if (Wt) HIP_TRY(hipMemcpy2DAsync(ws.W, sizeof(double) * (size_t)ld, Wt, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, PCG_NW, hipMemcpyHostToDevice, s));
        if (dense_pcg_transform(s, &ws, dA, db_, dinfo)) return fail(SFMBA_ERR_ALLOC, dense_pcg_error(PCG_ERR_ALLOC));
        if (flags & SFMBA_PCG_PROBE_POISON) dense_pcg_poison(s, &ws, plan.family == SFMBA_FAMILY_PCG_SYMMETRIC);
        if (ws.sym_zero) HIP_TRY(hipMemsetAsync(ws.sym_zero, 0, sizeof(double) * ws.sym_zero_n, s));       // (the linearisation's part: DeviceBuffers::pcg_zero)
        if ((rc = launches_ok())) return rc;
        const int it = dense_pcg_solve(s, &ws, dA, db_, tol, max_iters[i], dinfo, nullptr, o);
        if ((rc = launches_ok())) return rc;
        if (it < 0) return pcg_refused(it);
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(X + (size_t)i * n, db_, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
        if (iters) iters[i] = it;
        if (path) *path = sfmba_step_probe{ ws.family, ws.run.path.f32 ? 1 : 0, ws.coarse_vectors, it, 0 };
    }
    int hinfo = 0;
    HIP_TRY(hipMemcpy(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost));
    if (info) *info = hinfo;
    return SFMBA_OK;
}

int sfmba_dist_cg_probe(int device, int n, const double* A, int world, int nrhs, const double* B, const double* Wt, int flags, double tol,
                        const int* max_iters, int surplus, double* Xt, int* info, int* iters, int* rows, long long* chunk_blocks, int* replicas_differ) {
    constexpr int known = SFMBA_DCG_PROBE_F32 | SFMBA_DCG_PROBE_POISON;
    if (n <= 0 || n % 6 != 1 || nrhs <= 0 || !A || !B || !Xt || !max_iters || !(tol > 0.0) || (flags & ~known) || surplus < 0 || surplus > 1000)
        return fail(SFMBA_ERR_INVALID_ARG, "bad arguments");
    if (world < 1 || world > DCG_PROBE_MAX_WORLD) return fail(SFMBA_ERR_INVALID_ARG, "world must lie in 1 .. 16");
    for (int i = 0; i < nrhs; ++i)
        if (max_iters[i] <= 0 || max_iters[i] > 1000) return fail(SFMBA_ERR_INVALID_ARG, "max_iters must lie in 1 .. 1000");
    int rc = check_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    const int ld = dense_padded_dim(n), ncam = (n - 1) / 6;
    const bool poison = (flags & SFMBA_DCG_PROBE_POISON) != 0;
    double *dA = nullptr, *db_ = nullptr, *dx = nullptr;
    int *dinfo = nullptr, *dwords = nullptr, *dfirst = nullptr;
    void* downed = nullptr;
    DeviceTemps tmp(&dA, &db_, &dx, &dinfo, &dwords, &dfirst, &downed);
    HIP_TRY(dev_alloc(&dA, (size_t)n * ld));
    HIP_TRY(hipMemset(dA, 0, sizeof(double) * (size_t)n * ld));
    HIP_TRY(hipMemcpy2D(dA, sizeof(double) * (size_t)ld, A, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(dev_alloc(&db_, (size_t)ld));
    HIP_TRY(dev_alloc(&dinfo, 1));
    HIP_TRY(hipMemset(dinfo, 0, sizeof(int)));
    DenseSolver ws;
    if (dense_solver_create(&ws, n, ld)) return fail(SFMBA_ERR_ALLOC, "dense solver workspace allocation failed");
    hipStream_t s = nullptr;
    DeviceArena arena(device);          // the ranks' workspaces (dcg_create); goes back to the cache with the call
    struct Guard { DenseSolver* ws; hipStream_t* s; ~Guard() { if (*s) { (void)hipStreamSynchronize(*s); (void)hipStreamDestroy(*s); } dense_solver_destroy(ws); } } guard{ &ws, &s };
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (dense_pcg_ensure_workspace(&ws)) return fail(SFMBA_ERR_ALLOC, dense_pcg_error(PCG_ERR_ALLOC));
    // blocks and focal row in fp32 together, as the sharded loop pairs them (sharded_solve.hip: da.owned_f32 / da.focal_row32) -- only where the size stores fp32
    const bool f32 = (flags & SFMBA_DCG_PROBE_F32) != 0;
    if (f32 && dense_pcg_want_f32(&ws) == nullptr) return fail(SFMBA_ERR_INVALID_ARG, "SFMBA_DCG_PROBE_F32: the reduced matrix is not stored in fp32 at this size");
    ws.use_f32 = f32;

    // every simulated rank: a DistCg, x, flags, an info word and its chunk of the reduce-scatter layout
    std::vector<DistCg> ranks((size_t)world);
    std::vector<int*> rflags((size_t)world), rinfo((size_t)world);
    std::vector<char*> owned((size_t)world);
    for (int k = 0; k < world; ++k)
        if (dcg_create(&ranks[(size_t)k], n, ld, ncam, k, world, &arena)) return fail(SFMBA_ERR_ALLOC, "distributed CG workspace allocation failed");
    const size_t chunk_bytes = (size_t)dcg_chunk_values(ranks[0]) * (f32 ? 4 : 8);
    HIP_TRY(dev_alloc(&dx, (size_t)world * ld));
    HIP_TRY(hipMemset(dx, 0, sizeof(double) * (size_t)world * ld));
    HIP_TRY(dev_alloc(&dwords, (size_t)world * 8));
    HIP_TRY(hipMemset(dwords, 0, sizeof(int) * (size_t)world * 8));
    HIP_TRY(hipMalloc(&downed, chunk_bytes * (size_t)world));
    for (int k = 0; k < world; ++k) {
        ranks[(size_t)k].x = dx + (size_t)k * ld;
        rflags[(size_t)k] = dwords + (size_t)k * 8; rinfo[(size_t)k] = dwords + (size_t)k * 8 + 4;
        owned[(size_t)k] = static_cast<char*>(downed) + (size_t)k * chunk_bytes;
    }
    HIP_TRY(dev_alloc(&dfirst, 1));          // the number of the first check of the replicas that found a difference
    HIP_TRY(hipMemset(dfirst, 0, sizeof(int)));
    if (rows) for (int k = 0; k <= world; ++k) rows[k] = ranks[0].rows[(size_t)k];
    if (chunk_blocks) *chunk_blocks = ranks[0].chunk_blocks;

    // lockstep: one host thread per rank on ONE stream; the ranks meet inside the all-reduce callback, where the last to arrive enqueues the check of the
    // replicas and the sum (every rank's launches in front of its collective are in the stream by then), and at the end of every batch
    struct Lockstep {
        std::mutex m; std::condition_variable cv; int world = 1, waiting = 0; long gen = 0;
        void meet(const std::function<void()>& last) {
            std::unique_lock<std::mutex> lk(m);
            if (++waiting == world) { last(); waiting = 0; ++gen; cv.notify_all(); }
            else { const long g = gen; cv.wait(lk, [&] { return gen != g; }); }
        }
    } step;
    step.world = world;
    struct Shared { Lockstep* step; int world; const DistCg* ranks; int* const* flags; int* const* info; int* first; int checks; double* bufs[DCG_PROBE_MAX_WORLD]; } sh{
        &step, world, ranks.data(), rflags.data(), rinfo.data(), dfirst, 0, {} };
    struct RankCtx { Shared* sh; int rank; };
    auto ar = [](void* c, void* buf, long long len, hipStream_t st) -> int {
        RankCtx* r = static_cast<RankCtx*>(c);
        Shared* q = r->sh;
        { std::lock_guard<std::mutex> lk(q->step->m); q->bufs[r->rank] = static_cast<double*>(buf); }
        q->step->meet([&] {
            dcg_probe_compare(st, q->world, q->ranks, q->flags, q->info, ++q->checks, q->first);
            dcg_probe_allreduce(st, q->world, q->bufs, len);
        });
        return 0;
    };

    for (int i = 0; i < nrhs; ++i) {
        HIP_TRY(hipMemsetAsync(db_, 0, sizeof(double) * (size_t)ld, s));
        HIP_TRY(hipMemcpyAsync(db_, B + (size_t)i * n, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(ws.W, 0, sizeof(double) * ((size_t)PCG_NW * ld + pcg_tile_slack(n, ld)), s));
        if (Wt) HIP_TRY(hipMemcpy2DAsync(ws.W, sizeof(double) * (size_t)ld, Wt, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, PCG_NW, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(pcg_btilde(&ws), 0, sizeof(double) * (size_t)ld, s));
        if (dense_pcg_transform(s, &ws, dA, db_, dinfo)) return fail(SFMBA_ERR_ALLOC, dense_pcg_error(PCG_ERR_ALLOC));
        if (poison) {
            dense_pcg_poison(s, &ws, false);
            const std::vector<double> nan((size_t)(ld - n), __builtin_nan(""));
            HIP_TRY(hipMemcpyAsync(pcg_btilde(&ws) + n, nan.data(), sizeof(double) * nan.size(), hipMemcpyHostToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));       // (the host vector goes out of scope)
        }
        const void* F = f32 ? static_cast<const void*>(ws.Sfull32) : static_cast<const void*>(ws.Sfull);
        for (int k = 0; k < world; ++k) dcg_probe_fill_owned(s, ranks[(size_t)k], F, f32, owned[(size_t)k], poison);
        if ((rc = launches_ok())) return rc;

        // what the sharded loop passes (sharded_solve.hip): the rank's chunk, row d - 1 of the CG's matrix, b~, W~; plain relative stopping rule
        std::vector<DcgSolveArgs> args((size_t)world);
        std::vector<RankCtx> ctx((size_t)world);
        for (int k = 0; k < world; ++k) {
            DcgSolveArgs& da = args[(size_t)k];
            da.owned = owned[(size_t)k]; da.owned_f32 = f32;
            if (f32) da.focal_row32 = ws.Sfull32 + (size_t)(n - 1) * ld; else da.focal_row = ws.Sfull + (size_t)(n - 1) * ld;
            da.bt = pcg_btilde(&ws); da.W = Wt ? ws.W : nullptr;
            da.flags = rflags[(size_t)k]; da.info = rinfo[(size_t)k]; da.tol = tol; da.anchor = 0; da.cap = 1.0;
            ctx[(size_t)k] = RankCtx{ &sh, k };
        }
        const int cap = max_iters[i];
        int launched = 0, failed = 0;            // (written by the last rank to arrive, under the lock)
        bool ended = false;
        auto run_rank = [&](int k) {
            (void)hipSetDevice(device);
            DistCg* g = &ranks[(size_t)k];
            // (the callback never fails, so neither do dcg_begin / dcg_iterate: every rank makes the same sequence of calls and meetings)
            int lrc = dcg_begin(s, g, args[(size_t)k], ar, &ctx[(size_t)k]);
            bool sync_failed = false;
            for (;;) {
                // a batch, then the verdict of rank 0's flags for everybody (the replicas are held to it by the check)
                const int batch = std::min(24, cap - launched);
                if (!lrc && batch > 0) lrc = dcg_iterate(s, g, args[(size_t)k], batch, ar, &ctx[(size_t)k]);
                bool stop = false;
                step.meet([&] {
                    launched += batch;
                    int h[4] = { 0, 0, 0, 0 };
                    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(h, rflags[0], sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) failed = 1;
                    ended = failed || h[PF_DONE] != 0 || launched >= cap;
                    if (ended && !failed) for (int j = 0; j < world; ++j) dcg_probe_stop(s, rflags[(size_t)j], launched);
                });
                { std::lock_guard<std::mutex> lk(step.m); stop = ended; sync_failed = failed != 0; }      // (both as the meeting left them: the same on every rank)
                if (stop) break;
            }
            // surplus launches: each issues its collective, as the fixed batch of the sharded loop does
            if (!sync_failed && surplus > 0) lrc = dcg_iterate(s, g, args[(size_t)k], surplus, ar, &ctx[(size_t)k]);
            if (lrc || hipGetLastError() != hipSuccess) { std::lock_guard<std::mutex> lk(step.m); failed = 1; }      // (a refused launch is this thread's error)
        };
        {
            std::vector<std::thread> threads;
            for (int k = 1; k < world; ++k) threads.emplace_back(run_rank, k);
            run_rank(0);
            for (std::thread& t : threads) t.join();
        }
        dcg_probe_compare(s, world, ranks.data(), rflags.data(), rinfo.data(), ++sh.checks, dfirst);
        if ((rc = launches_ok())) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        if (failed) return fail(SFMBA_ERR_HIP, "distributed CG probe: a rank's launches failed");
        HIP_TRY(hipMemcpy(Xt + (size_t)i * n, ranks[0].x, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
        int h[4] = { 0, 0, 0, 0 };
        HIP_TRY(hipMemcpy(h, rflags[0], sizeof(h), hipMemcpyDeviceToHost));
        if (iters) iters[i] = h[PF_ITERS];
    }
    int hinfo = 0, hrank = 0, hfirst = 0;
    HIP_TRY(hipMemcpy(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&hrank, rinfo[0], sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&hfirst, dfirst, sizeof(int), hipMemcpyDeviceToHost));
    if (info) *info = hinfo ? hinfo : hrank;
    if (replicas_differ) *replicas_differ = hfirst;
    return SFMBA_OK;
}
}  // extern "C"
