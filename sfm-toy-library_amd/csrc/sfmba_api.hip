// sfmba_api.hip -- C ABI of include/sfmba.h: argument checks and dispatch.  The work is in problem_build.hip (structure build),
// lm_solve.hip (LM driver), sharded_solve.hip (multi-GPU and matrix-free loops), comm_rccl.hip and the kernel units.
//
// There is NO CPU fallback in this library: without a HIP device every entry point returns SFMBA_ERR_NO_DEVICE.
#include "association.h"
#include "feature_match.h"
#include "match_l2.h"
#include "lm_loop.h"
#include "pnp_ransac.h"
#include "homography_ransac.h"
#include "essential_ransac.h"
#include "orb_extract.h"
#include "surf_extract.h"
#include "depth_sweep.h"
#include "cloud_merge.h"
#include "flow_track.h"
#include "flow_math.h"
#include "jpeg_decode.h"
#include "jpeg_math.h"
#include "png_decode.h"
#include <climits>
#include <cmath>

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

namespace {
// `device` checked and current, a stream + pinned block on it for the duration of one call of the wrappers below
struct CallKit {
    HostKit kit;
    int open(int device) {
        if (const int rc = check_device(device)) return rc;
        HIP_TRY(hipSetDevice(device));
        return hostkit_acquire(device, &kit) ? SFMBA_OK : fail(SFMBA_ERR_HIP, "stream creation failed");
    }
    ~CallKit() { if (kit.stream) (void)hipStreamSynchronize(kit.stream); hostkit_release(kit); }
};
}  // namespace

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
    if (z) HIP_TRY(hipMemcpy(z, p->d_probe, sizeof(double) * (size_t)p->ds.d, hipMemcpyDeviceToHost));
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
    if (S) HIP_TRY(hipMemcpy(S, d_full, sizeof(double) * (size_t)d * d, hipMemcpyDeviceToHost));
    if (rhs) HIP_TRY(hipMemcpy(rhs, p->db.rhs, sizeof(double) * (size_t)d, hipMemcpyDeviceToHost));
    if (scale) HIP_TRY(hipMemcpy(scale, d_scale, sizeof(double) * (size_t)d, hipMemcpyDeviceToHost));
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
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(x, db_, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    int hinfo = 0;
    HIP_TRY(hipMemcpy(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost));
    if (info) *info = hinfo;
    if (iters) *iters = it;
    return SFMBA_OK;
}

int sfmba_triangulate(int device, int64_t n, const float* left_xy, const float* right_xy, const float* K, const float* P_left,
                      const float* P_right, float max_reproj_px, float* points3d, unsigned char* keep, float* reproj_err) {
    if (n < 0 || !K || !P_left || !P_right || (n > 0 && (!left_xy || !right_xy || !points3d || !keep)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (n == 0) return check_device(device);
    DeviceArena arena(device);
    CallKit ck;
    if (const int rc = ck.open(device)) return rc;
    const HostKit& kit = ck.kit;
    float* d_l = arena.alloc_n<float>((size_t)2 * n);
    float* d_r = arena.alloc_n<float>((size_t)2 * n);
    float* d_x = arena.alloc_n<float>((size_t)3 * n);
    float* d_e = reproj_err ? arena.alloc_n<float>((size_t)2 * n) : nullptr;
    unsigned char* d_k = arena.alloc_n<unsigned char>((size_t)n);
    if (!d_l || !d_r || !d_x || !d_k || (reproj_err && !d_e)) return fail(SFMBA_ERR_ALLOC, "device allocation failed");
    HIP_TRY(hipMemcpyAsync(d_l, left_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, kit.stream));
    HIP_TRY(hipMemcpyAsync(d_r, right_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, kit.stream));
    launch_triangulate(kit.stream, (long long)n, d_l, d_r, K, P_left, P_right, max_reproj_px, d_x, d_k, d_e);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(points3d, d_x, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, kit.stream));
    HIP_TRY(hipMemcpyAsync(keep, d_k, (size_t)n, hipMemcpyDeviceToHost, kit.stream));
    if (reproj_err) HIP_TRY(hipMemcpyAsync(reproj_err, d_e, sizeof(float) * 2 * (size_t)n, hipMemcpyDeviceToHost, kit.stream));
    HIP_TRY(hipStreamSynchronize(kit.stream));
    return SFMBA_OK;
}

int sfmba_triangulate_pairs(int device, int n_images, const int64_t* img_ptr, const float* pts, const float* K, int n_pairs, const int32_t* pair_left,
                            const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx,
                            const unsigned char* mask, const float* P_left, const float* P_right, float max_reproj_px, float* points3d,
                            unsigned char* keep, float* reproj_err, int64_t* kept_ptr, int64_t* kept_idx) {
    // every check comes before the first write: a refused call leaves the outputs as they were
    if (n_images < 0 || n_pairs < 0 || !img_ptr || !pair_ptr || !K || !kept_ptr || (n_pairs > 0 && (!pair_left || !pair_right || !P_left || !P_right)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (!std::isfinite(max_reproj_px) || max_reproj_px < 0.0f) return fail(SFMBA_ERR_INVALID_ARG, "max_reproj_px must be finite and >= 0");
    if (img_ptr[0] < 0 || pair_ptr[0] < 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr and pair_ptr must not be negative");
    for (int i = 0; i < n_images; ++i)
        if (img_ptr[i + 1] < img_ptr[i]) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr not monotone");
    for (int p = 0; p < n_pairs; ++p) {
        if (pair_ptr[p + 1] < pair_ptr[p]) return fail(SFMBA_ERR_INVALID_ARG, "pair_ptr not monotone");
        if (pair_ptr[p + 1] - pair_ptr[p] > (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "triangulate_pairs: a pair has 2^31 or more matches");
        if (pair_left[p] < 0 || pair_left[p] >= n_images || pair_right[p] < 0 || pair_right[p] >= n_images)
            return fail(SFMBA_ERR_INVALID_ARG, "pair index out of range");
    }
    const int64_t total = pair_ptr[n_pairs];
    if (total > 0 && (!points3d || !keep || !kept_idx)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (total > pair_ptr[0] && (!query_idx || !train_idx || !pts)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    for (int p = 0; p < n_pairs; ++p) {
        const int64_t nl = img_ptr[pair_left[p] + 1] - img_ptr[pair_left[p]], nr = img_ptr[pair_right[p] + 1] - img_ptr[pair_right[p]];
        for (int64_t e = pair_ptr[p]; e < pair_ptr[p + 1]; ++e)
            if (query_idx[e] < 0 || query_idx[e] >= nl || train_idx[e] < 0 || train_idx[e] >= nr)
                return fail(SFMBA_ERR_INVALID_ARG, "triangulate_pairs: a query_idx / train_idx lies outside its image");
    }
    if (total >= (int64_t)INT_MAX - 256) return fail(SFMBA_ERR_INVALID_ARG, "triangulate_pairs: too many entries for one call (2^31)");
    if (total == pair_ptr[0]) {                                       // no entry belongs to a pair: nothing runs on the device
        if (const int rc = check_device(device)) return rc;
        for (int64_t e = 0; e < total; ++e) {
            points3d[3 * e] = points3d[3 * e + 1] = points3d[3 * e + 2] = 0.0f;
            keep[e] = 0;
            if (reproj_err) reproj_err[2 * e] = reproj_err[2 * e + 1] = 0.0f;
        }
        for (int p = 0; p <= n_pairs; ++p) kept_ptr[p] = 0;
        return SFMBA_OK;
    }
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    rc = triangulate_pairs(ck.kit.stream, device, n_images, img_ptr, pts, K, n_pairs, pair_left, pair_right, pair_ptr, query_idx, train_idx, mask,
                           P_left, P_right, max_reproj_px, points3d, keep, reproj_err, kept_ptr, kept_idx);
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "triangulate_pairs: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("triangulate_pairs: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}

// ---- association joins -----------------------------------------------------------------------
static int assoc_result(int rc, const char* what) {
    if (rc == 0) return SFMBA_OK;
    if (rc == ASSOC_ERR_CAPACITY) return fail(SFMBA_ERR_CAPACITY, std::string(what) + ": output capacity too small");
    if (rc == ASSOC_ERR_TOO_LARGE) return fail(SFMBA_ERR_INVALID_ARG, std::string(what) + ": problem too large for 32-bit indices");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, std::string(what) + ": device allocation failed");
    return fail(SFMBA_ERR_HIP, std::string(what) + ": " + hipGetErrorString((hipError_t)rc));
}

int sfmba_find_2d3d_matches(int device, int n_views, const unsigned char* view_done, int n_pt, const int64_t* view_ptr,
                            const int32_t* view_idx, const int32_t* feat_idx, int n_pairs, const int32_t* pair_left,
                            const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx,
                            int64_t* out_ptr, int32_t* out_point, int32_t* out_feature, int64_t cap, int64_t* total) {
    if (n_views < 0 || n_pt < 0 || n_pairs < 0 || cap < 0 || !out_ptr || !total || (n_views > 0 && !view_done) || !view_ptr ||
        (n_pairs > 0 && (!pair_left || !pair_right || !pair_ptr)) || (cap > 0 && (!out_point || !out_feature)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (view_ptr[0] != 0 || (n_pairs > 0 && pair_ptr[0] != 0)) return fail(SFMBA_ERR_INVALID_ARG, "CSR pointers must start at 0");
    for (int i = 0; i < n_pt; ++i) if (view_ptr[i + 1] < view_ptr[i]) return fail(SFMBA_ERR_INVALID_ARG, "view_ptr not monotone");
    for (int p = 0; p < n_pairs; ++p) if (pair_ptr[p + 1] < pair_ptr[p]) return fail(SFMBA_ERR_INVALID_ARG, "pair_ptr not monotone");
    if ((view_ptr[n_pt] > 0 && (!view_idx || !feat_idx)) || (n_pairs > 0 && pair_ptr[n_pairs] > 0 && (!query_idx || !train_idx)))
        return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    CallKit ck;
    if (const int rc = ck.open(device)) return rc;
    return assoc_result(assoc_find_2d3d(ck.kit.stream, device, n_views, view_done, n_pt, view_ptr, view_idx, feat_idx, n_pairs, pair_left, pair_right,
                                        pair_ptr, query_idx, train_idx, out_ptr, out_point, out_feature, cap, total), "find_2d3d_matches");
}

int sfmba_merge_candidates(int device, int n_exist, const float* exist_xyz, int n_new, const float* new_xyz, float max_dist,
                           int64_t* cand_ptr, int32_t* cand_idx, int64_t cap, int64_t* total) {
    if (n_exist < 0 || n_new < 0 || cap < 0 || !cand_ptr || !total || (n_exist > 0 && !exist_xyz) || (n_new > 0 && !new_xyz) || (cap > 0 && !cand_idx))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    CallKit ck;
    if (const int rc = ck.open(device)) return rc;
    return assoc_result(assoc_radius_candidates(ck.kit.stream, device, n_exist, exist_xyz, n_new, new_xyz, max_dist, cand_ptr, cand_idx, cap, total),
                        "merge_candidates");
}

// ---- feature match matrix (SfM::createFeatureMatchMatrix) ---------------------------------------------------------
int sfmba_match_features(int device, int n_images, const int64_t* img_ptr, const unsigned char* desc, int desc_bytes, int n_pairs,
                         const int32_t* pair_left, const int32_t* pair_right, double ratio, int64_t* pair_ptr, int32_t* query_idx,
                         int32_t* train_idx, float* distance, int64_t cap, int64_t* total) {
    if (n_images < 0 || n_pairs < 0 || cap < 0 || !img_ptr || !pair_ptr || !total || (n_pairs > 0 && (!pair_left || !pair_right)) ||
        (cap > 0 && (!query_idx || !train_idx)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (desc_bytes < 1 || desc_bytes > 64) return fail(SFMBA_ERR_INVALID_ARG, "desc_bytes must be in 1..64");
    if (!std::isfinite(ratio) || !(ratio > 0.0)) return fail(SFMBA_ERR_INVALID_ARG, "ratio must be finite and > 0");
    if (img_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr must start at 0");
    for (int i = 0; i < n_images; ++i) {
        const int64_t n = img_ptr[i + 1] - img_ptr[i];
        if (n < 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr not monotone");
        if (n >= ((int64_t)1 << 22)) return fail(SFMBA_ERR_INVALID_ARG, "an image has 2^22 or more descriptor rows (the train index is packed in 22 bits)");
    }
    if (img_ptr[n_images] > 0 && !desc) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    int64_t rows = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int l = pair_left[p], r = pair_right[p];
        if (l < 0 || l >= n_images || r < 0 || r >= n_images) return fail(SFMBA_ERR_INVALID_ARG, "pair index out of range");
        if (img_ptr[r + 1] - img_ptr[r] >= 2) rows += img_ptr[l + 1] - img_ptr[l];
    }
    if (rows >= (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "match_features: too many query rows in one call (2^31)");
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    // SFMBA_MATCH_TIMING: one stderr line per call with the HIP-event times of its phases (tools/match_bench.py)
    double tm[5];
    const bool timing = std::getenv("SFMBA_MATCH_TIMING") != nullptr;
    rc = match_features(ck.kit.stream, device, n_images, img_ptr, desc, desc_bytes, n_pairs, pair_left, pair_right, ratio, pair_ptr, query_idx,
                        train_idx, distance, cap, total, timing ? tm : nullptr);
    if (rc == 0 && timing)
        std::fprintf(stderr, "[sfmba match] upload_ms %.6f top2_ms %.6f compact_ms %.6f download_ms %.6f batches %d\n", tm[0], tm[1], tm[2], tm[3], (int)tm[4]);
    if (rc == MATCH_ERR_CAPACITY) return fail(SFMBA_ERR_CAPACITY, "match_features: output capacity too small");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "match_features: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("match_features: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
// ---- the same for float descriptors: exact L2 2-NN (cv::BFMatcher with NORM_L2) ---------------------------------------------
int sfmba_match_features_l2(int device, int n_images, const int64_t* img_ptr, const float* desc, int dims, int n_pairs,
                            const int32_t* pair_left, const int32_t* pair_right, double ratio, int64_t* pair_ptr, int32_t* query_idx,
                            int32_t* train_idx, float* distance, int64_t cap, int64_t* total) {
    if (n_images < 0 || n_pairs < 0 || cap < 0 || !img_ptr || !pair_ptr || !total || (n_pairs > 0 && (!pair_left || !pair_right)) ||
        (cap > 0 && (!query_idx || !train_idx)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (dims < 1 || dims > MATCH_L2_MAX_DIMS) return fail(SFMBA_ERR_INVALID_ARG, "dims must be in 1..512");
    if (!std::isfinite(ratio) || !(ratio > 0.0)) return fail(SFMBA_ERR_INVALID_ARG, "ratio must be finite and > 0");
    if (img_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr must start at 0");
    for (int i = 0; i < n_images; ++i) {
        const int64_t n = img_ptr[i + 1] - img_ptr[i];
        if (n < 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr not monotone");
        if (n >= ((int64_t)1 << 22)) return fail(SFMBA_ERR_INVALID_ARG, "an image has 2^22 or more descriptor rows");
    }
    if (img_ptr[n_images] > 0 && !desc) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    int64_t rows = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int l = pair_left[p], r = pair_right[p];
        if (l < 0 || l >= n_images || r < 0 || r >= n_images) return fail(SFMBA_ERR_INVALID_ARG, "pair index out of range");
        if (img_ptr[r + 1] - img_ptr[r] >= 2) rows += img_ptr[l + 1] - img_ptr[l];
    }
    if (rows >= (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "match_features_l2: too many query rows in one call (2^31)");
    for (int i = 0; i < n_images; ++i)                      // the contract is stated for finite values only
        for (int64_t r = img_ptr[i]; r < img_ptr[i + 1]; ++r) {
            const float* row = desc + (size_t)r * (size_t)dims;
            for (int k = 0; k < dims; ++k)
                if (!std::isfinite(row[k]))
                    return fail(SFMBA_ERR_INVALID_ARG, "match_features_l2: non-finite descriptor value in image " + std::to_string(i) + ", row " +
                                                           std::to_string((long long)(r - img_ptr[i])));
        }
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    // SFMBA_MATCH_TIMING: one stderr line per call with the HIP-event times of its phases (tools/match_l2_bench.py)
    double tm[5];
    const bool timing = std::getenv("SFMBA_MATCH_TIMING") != nullptr;
    rc = match_features_l2(ck.kit.stream, device, n_images, img_ptr, desc, dims, n_pairs, pair_left, pair_right, ratio, pair_ptr, query_idx,
                           train_idx, distance, cap, total, timing ? tm : nullptr);
    if (rc == 0 && timing)
        std::fprintf(stderr, "[sfmba match_l2] upload_ms %.6f top2_ms %.6f compact_ms %.6f download_ms %.6f batches %d\n", tm[0], tm[1], tm[2], tm[3], (int)tm[4]);
    if (rc == MATCH_L2_ERR_CAPACITY) return fail(SFMBA_ERR_CAPACITY, "match_features_l2: output capacity too small");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "match_features_l2: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("match_features_l2: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
// ---- feature extraction (SfM::extractFeatures) ------------------------------------------------------------------------
int sfmba_orb_extract(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                      int channels, int n_features, float scale_factor, int n_levels, int fast_threshold, int64_t* kp_ptr, sfmba_orb_keypoint* kp,
                      unsigned char* desc, int64_t cap, int64_t* total, int32_t* dbg_level_xy, int32_t* dbg_bin, int64_t* dbg_harris,
                      int32_t* dbg_candidates) {
    if (n_images < 0 || cap < 0 || !img_ptr || !kp_ptr || !total || (n_images > 0 && (!width || !height)) || (cap > 0 && (!kp || !desc)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (channels != 1 && channels != 3) return fail(SFMBA_ERR_INVALID_ARG, "orb_extract: channels must be 1 or 3");
    if (n_features < 1) return fail(SFMBA_ERR_INVALID_ARG, "orb_extract: n_features must be >= 1");
    if (n_levels < 1 || n_levels > 12) return fail(SFMBA_ERR_INVALID_ARG, "orb_extract: n_levels must be in 1..12");
    if (!std::isfinite(scale_factor) || !(scale_factor > 1.0f) || scale_factor > 2.0f)
        return fail(SFMBA_ERR_INVALID_ARG, "orb_extract: scale_factor must be finite and in (1, 2]");
    if (fast_threshold < 1 || fast_threshold > 254) return fail(SFMBA_ERR_INVALID_ARG, "orb_extract: fast_threshold must be in 1..254");
    if (img_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr must start at 0");
    for (int i = 0; i < n_images; ++i) {
        if (width[i] < 1 || width[i] > 16384 || height[i] < 1 || height[i] > 16384)
            return fail(SFMBA_ERR_INVALID_ARG, "orb_extract: an image dimension lies outside 1..16384");
        if (img_ptr[i + 1] - img_ptr[i] != (int64_t)width[i] * height[i] * channels)
            return fail(SFMBA_ERR_INVALID_ARG, "orb_extract: img_ptr does not agree with width * height * channels");
    }
    if (n_images > 0 && !pixels) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    // SFMBA_ORB_TIMING: one stderr line per call with the HIP-event times of its phases (tools/orb_bench.py)
    double tm[ORB_T_COUNT];
    const bool timing = std::getenv("SFMBA_ORB_TIMING") != nullptr;
    rc = orb_extract(ck.kit.stream, device, n_images, img_ptr, pixels, width, height, channels, n_features, scale_factor, n_levels, fast_threshold,
                     kp_ptr, kp, desc, cap, total, dbg_level_xy, dbg_bin, dbg_harris, dbg_candidates, timing ? tm : nullptr);
    if (rc == 0 && timing)
        std::fprintf(stderr, "[sfmba orb] upload_ms %.6f pyramid_ms %.6f score_ms %.6f candidates_ms %.6f response_ms %.6f select_ms %.6f smooth_ms %.6f "
                     "describe_ms %.6f download_ms %.6f groups %d\n", tm[ORB_T_UPLOAD], tm[ORB_T_PYRAMID], tm[ORB_T_SCORE], tm[ORB_T_CANDIDATES],
                     tm[ORB_T_HARRIS], tm[ORB_T_SELECT], tm[ORB_T_SMOOTH], tm[ORB_T_DESCRIBE], tm[ORB_T_DOWNLOAD], (int)tm[ORB_T_GROUPS]);
    if (rc == ORB_ERR_CAPACITY) return fail(SFMBA_ERR_CAPACITY, "orb_extract: output capacity too small");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "orb_extract: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("orb_extract: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
// ---- float descriptors: Fast-Hessian detect and SURF-style describe, the extractor in front of sfmba_match_features_l2 ---------
int sfmba_surf_extract(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                       int channels, int n_features, int n_octaves, float hessian_threshold, int upright, int64_t* kp_ptr, sfmba_surf_keypoint* kp,
                       float* desc, int64_t cap, int64_t* total, int32_t* dbg_bin, int64_t* dbg_moments, int64_t* dbg_sums, int32_t* dbg_candidates) {
    if (n_images < 0 || cap < 0 || !img_ptr || !kp_ptr || !total || (n_images > 0 && (!width || !height)) || (cap > 0 && (!kp || !desc)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (channels != 1 && channels != 3) return fail(SFMBA_ERR_INVALID_ARG, "surf_extract: channels must be 1 or 3");
    if (n_features < 1) return fail(SFMBA_ERR_INVALID_ARG, "surf_extract: n_features must be >= 1");
    if (n_octaves < 1 || n_octaves > 4) return fail(SFMBA_ERR_INVALID_ARG, "surf_extract: n_octaves must be in 1..4");
    if (!std::isfinite(hessian_threshold) || hessian_threshold < 0.0f)
        return fail(SFMBA_ERR_INVALID_ARG, "surf_extract: hessian_threshold must be finite and >= 0");
    if (upright != 0 && upright != 1) return fail(SFMBA_ERR_INVALID_ARG, "surf_extract: upright must be 0 or 1");
    if (img_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr must start at 0");
    for (int i = 0; i < n_images; ++i) {
        if (width[i] < 1 || width[i] > 16384 || height[i] < 1 || height[i] > 16384)
            return fail(SFMBA_ERR_INVALID_ARG, "surf_extract: an image dimension lies outside 1..16384");
        if (img_ptr[i + 1] - img_ptr[i] != (int64_t)width[i] * height[i] * channels)
            return fail(SFMBA_ERR_INVALID_ARG, "surf_extract: img_ptr does not agree with width * height * channels");
    }
    if (n_images > 0 && !pixels) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    // SFMBA_SURF_TIMING: one stderr line per call with the HIP-event times of its phases (tools/surf_bench.py)
    double tm[SURF_T_COUNT];
    const bool timing = std::getenv("SFMBA_SURF_TIMING") != nullptr;
    rc = surf_extract(ck.kit.stream, device, n_images, img_ptr, pixels, width, height, channels, n_features, n_octaves, hessian_threshold, upright,
                      kp_ptr, kp, desc, cap, total, dbg_bin, dbg_moments, dbg_sums, dbg_candidates, timing ? tm : nullptr);
    if (rc == 0 && timing)
        std::fprintf(stderr, "[sfmba surf] upload_ms %.6f integral_ms %.6f response_ms %.6f candidates_ms %.6f select_ms %.6f describe_ms %.6f "
                     "download_ms %.6f groups %d response_bytes %.0f\n", tm[SURF_T_UPLOAD], tm[SURF_T_INTEGRAL], tm[SURF_T_RESPONSE],
                     tm[SURF_T_CANDIDATES], tm[SURF_T_SELECT], tm[SURF_T_DESCRIBE], tm[SURF_T_DOWNLOAD], (int)tm[SURF_T_GROUPS], tm[SURF_T_RESPONSE_BYTES]);
    if (rc == SURF_ERR_CAPACITY) return fail(SFMBA_ERR_CAPACITY, "surf_extract: output capacity too small");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "surf_extract: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("surf_extract: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
// ---- dense depth maps and a dense cloud: plane-sweep stereo and the consistency filter (SfM::densify) ---------------------------
namespace {
// what every dense call refuses about the sizes, K and P; 0 or the failure
int depth_check_cameras(const char* who, int n_images, const int32_t* width, const int32_t* height, const float* K, const float* P) {
    const std::string w(who);
    if (n_images < 0 || !K || (n_images > 0 && (!width || !height || !P))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    for (int i = 0; i < n_images; ++i) {
        if (width[i] < 1 || width[i] > 16384 || height[i] < 1 || height[i] > 16384)
            return fail(SFMBA_ERR_INVALID_ARG, w + ": an image dimension lies outside 1..16384");
        for (int q = 0; q < 12; ++q)
            if (!std::isfinite(P[(size_t)i * 12 + q])) return fail(SFMBA_ERR_INVALID_ARG, w + ": non-finite pose of image " + std::to_string(i));
    }
    for (int q : { 0, 4, 2, 5 })
        if (!std::isfinite(K[q])) return fail(SFMBA_ERR_INVALID_ARG, w + ": fx, fy, cx and cy must be finite");
    if (!(K[0] > 0.0f) || !(K[4] > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, w + ": fx and fy must be > 0");
    return 0;
}
// what the sweep and the fuse refuse about the images, K and P; 0 or the failure
int depth_check_images(const char* who, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                       int channels, const float* K, const float* P) {
    const std::string w(who);
    if (n_images < 0 || !img_ptr || !K || (n_images > 0 && (!width || !height || !P || !pixels))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (channels != 1 && channels != 3) return fail(SFMBA_ERR_INVALID_ARG, w + ": channels must be 1 or 3");
    if (img_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr must start at 0");
    for (int i = 0; i < n_images; ++i)
        if (width[i] >= 1 && height[i] >= 1 && img_ptr[i + 1] - img_ptr[i] != (int64_t)width[i] * height[i] * channels)
            return fail(SFMBA_ERR_INVALID_ARG, w + ": img_ptr does not agree with width * height * channels");
    return depth_check_cameras(who, n_images, width, height, K, P);
}
// a CSR list of 0 / 1 .. 4 other images per row; 0 or the failure
int depth_check_lists(const char* who, const char* what, int n_images, int n_rows, const int32_t* row_image, const int64_t* ptr, const int32_t* idx,
                      int min_len) {
    const std::string w(who);
    if (!ptr || ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, w + ": " + what + " pointer array must start at 0");
    for (int j = 0; j < n_rows; ++j) {
        const int64_t n = ptr[j + 1] - ptr[j];
        if (n < min_len || n > 4) return fail(SFMBA_ERR_INVALID_ARG, w + ": a row has " + std::to_string((long long)n) + " " + what + " images, outside " +
                                                                       std::to_string(min_len) + "..4");
        if (n > 0 && !idx) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
        const int own = row_image ? row_image[j] : j;
        for (int64_t a = ptr[j]; a < ptr[j + 1]; ++a) {
            if (idx[a] < 0 || idx[a] >= n_images) return fail(SFMBA_ERR_INVALID_ARG, w + ": " + what + " image index out of range");
            if (idx[a] == own) return fail(SFMBA_ERR_INVALID_ARG, w + ": a " + what + " image equals the image it belongs to");
            for (int64_t c = ptr[j]; c < a; ++c)
                if (idx[c] == idx[a]) return fail(SFMBA_ERR_INVALID_ARG, w + ": a " + what + " image is listed twice");
        }
    }
    return 0;
}
}  // namespace
int sfmba_depth_sweep(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                      int channels, const float* K, const float* P, int n_jobs, const int32_t* job_ref, const int64_t* job_src_ptr,
                      const int32_t* job_src, const float* z_near, const float* z_far, int n_planes, int radius, int min_std, float min_score,
                      int min_sources, float* depth, float* score, int16_t* plane) {
    if (n_jobs < 0 || (n_jobs > 0 && (!job_ref || !job_src_ptr || !job_src || !z_near || !z_far))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (int rc = depth_check_images("depth_sweep", n_images, img_ptr, pixels, width, height, channels, K, P)) return rc;
    if (n_planes < 2 || n_planes > 256) return fail(SFMBA_ERR_INVALID_ARG, "depth_sweep: n_planes must be in 2..256");
    if (radius < 1 || radius > 4) return fail(SFMBA_ERR_INVALID_ARG, "depth_sweep: radius must be in 1..4");
    if (min_std < 0 || min_std > 127) return fail(SFMBA_ERR_INVALID_ARG, "depth_sweep: min_std must be in 0..127");
    if (!(min_score >= -1.0f) || !(min_score <= 1.0f)) return fail(SFMBA_ERR_INVALID_ARG, "depth_sweep: min_score must be in [-1, 1]");
    if (min_sources < 1 || min_sources > 4) return fail(SFMBA_ERR_INVALID_ARG, "depth_sweep: min_sources must be in 1..4");
    int64_t out_px = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (job_ref[j] < 0 || job_ref[j] >= n_images) return fail(SFMBA_ERR_INVALID_ARG, "depth_sweep: reference image index out of range");
        if (!std::isfinite(z_near[j]) || !std::isfinite(z_far[j]) || !(z_near[j] > 0.0f) || !(z_near[j] < z_far[j]))
            return fail(SFMBA_ERR_INVALID_ARG, "depth_sweep: a job needs 0 < z_near < z_far, both finite");
        out_px += (int64_t)width[job_ref[j]] * height[job_ref[j]];
    }
    if (n_jobs > 0)
        if (int rc = depth_check_lists("depth_sweep", "source", n_images, n_jobs, job_ref, job_src_ptr, job_src, 1)) return rc;
    if (out_px > 0 && (!depth || !score)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (n_jobs == 0) return check_device(device);
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    // SFMBA_DEPTH_TIMING: one stderr line per call with the HIP-event times of its phases (tools/dense_bench.py)
    double tm[DEPTH_T_COUNT];
    const bool timing = std::getenv("SFMBA_DEPTH_TIMING") != nullptr;
    rc = depth_sweep(ck.kit.stream, device, n_images, img_ptr, pixels, width, height, channels, K, P, n_jobs, job_ref, job_src_ptr, job_src, z_near,
                     z_far, n_planes, radius, min_std, min_score, min_sources, depth, score, plane, timing ? tm : nullptr);
    if (rc == 0 && timing)
        std::fprintf(stderr, "[sfmba depth_sweep] upload_ms %.6f gray_ms %.6f sweep_ms %.6f download_ms %.6f groups %d\n", tm[DEPTH_T_UPLOAD],
                     tm[DEPTH_T_GRAY], tm[DEPTH_T_SWEEP], tm[DEPTH_T_DOWNLOAD], (int)tm[DEPTH_T_GROUPS]);
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "depth_sweep: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("depth_sweep: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
int sfmba_depth_fuse(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                     int channels, const float* K, const float* P, const float* const* depth, const int64_t* chk_ptr, const int32_t* chk,
                     float rel_tol, int min_consistent, int64_t* pt_ptr, float* xyz, unsigned char* bgr, int32_t* src_image, int32_t* src_pixel,
                     int64_t cap, int64_t* total) {
    if (cap < 0 || !pt_ptr || !total || (n_images > 0 && !depth) || (cap > 0 && (!xyz || !bgr || !src_image || !src_pixel)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (int rc = depth_check_images("depth_fuse", n_images, img_ptr, pixels, width, height, channels, K, P)) return rc;
    if (n_images > 65535) return fail(SFMBA_ERR_INVALID_ARG, "depth_fuse: more than 65535 images in one call");
    if (!std::isfinite(rel_tol) || rel_tol < 0.0f) return fail(SFMBA_ERR_INVALID_ARG, "depth_fuse: rel_tol must be finite and >= 0");
    if (min_consistent < 0 || min_consistent > 4) return fail(SFMBA_ERR_INVALID_ARG, "depth_fuse: min_consistent must be in 0..4");
    if (int rc = depth_check_lists("depth_fuse", "check", n_images, n_images, nullptr, chk_ptr, chk, 0)) return rc;
    int64_t px = 0;
    for (int i = 0; i < n_images; ++i)
        if (depth[i]) px += (int64_t)width[i] * height[i];
    if (px >= (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "depth_fuse: too many pixels with a depth map in one call (2^31)");
    if (px == 0) {
        for (int i = 0; i <= n_images; ++i) pt_ptr[i] = 0;
        *total = 0;
        return check_device(device);
    }
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    double tm[FUSE_T_COUNT];
    const bool timing = std::getenv("SFMBA_DEPTH_TIMING") != nullptr;
    rc = depth_fuse(ck.kit.stream, device, n_images, img_ptr, pixels, width, height, channels, K, P, depth, chk_ptr, chk, rel_tol, min_consistent,
                    pt_ptr, xyz, bgr, src_image, src_pixel, cap, total, timing ? tm : nullptr);
    if (rc == 0 && timing)
        std::fprintf(stderr, "[sfmba depth_fuse] upload_ms %.6f flag_ms %.6f scan_ms %.6f emit_ms %.6f download_ms %.6f\n", tm[FUSE_T_UPLOAD],
                     tm[FUSE_T_FLAG], tm[FUSE_T_SCAN], tm[FUSE_T_EMIT], tm[FUSE_T_DOWNLOAD]);
    if (rc == DEPTH_ERR_CAPACITY) return fail(SFMBA_ERR_CAPACITY, "depth_fuse: output capacity too small");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "depth_fuse: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("depth_fuse: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
// ---- matching by optical flow: pyramidal Lucas-Kanade and the snap to key points (SfMFeatureMatching::createFlowMatchMatrix) -----
namespace {
// what both flow calls refuse about the pair list and the points' CSR; 0 or the failure
int flow_check_pairs(const char* who, int n_images, int n_pairs, const int32_t* pair_a, const int32_t* pair_b, const int64_t* pt_ptr) {
    const std::string w(who);
    if (n_images < 0 || n_pairs < 0 || !pt_ptr || (n_pairs > 0 && !pair_b)) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (pt_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, w + ": pt_ptr must start at 0");
    for (int p = 0; p < n_pairs; ++p) {
        if ((pair_a && (pair_a[p] < 0 || pair_a[p] >= n_images)) || pair_b[p] < 0 || pair_b[p] >= n_images)
            return fail(SFMBA_ERR_INVALID_ARG, w + ": pair index out of range");
        if (pt_ptr[p + 1] < pt_ptr[p]) return fail(SFMBA_ERR_INVALID_ARG, w + ": pt_ptr not monotone");
    }
    if (pt_ptr[n_pairs] >= (int64_t)1 << 31) return fail(SFMBA_ERR_INVALID_ARG, w + ": 2^31 or more points in one call");
    return 0;
}
}  // namespace
int sfmba_flow_track(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                     int channels, int n_pairs, const int32_t* pair_src, const int32_t* pair_dst, const int64_t* pt_ptr, const float* pts,
                     int n_levels, int radius, int max_iters, float min_eig, float* next, unsigned char* status, float* err, int64_t* dbg_G,
                     int32_t* dbg_state, unsigned char* dbg_pyramid) {
    if (n_images < 0 || !img_ptr || (n_images > 0 && (!width || !height)) || (n_pairs > 0 && !pair_src))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (channels != 1 && channels != 3) return fail(SFMBA_ERR_INVALID_ARG, "flow_track: channels must be 1 or 3");
    if (n_levels < 1 || n_levels > FLOW_MAX_LEVELS) return fail(SFMBA_ERR_INVALID_ARG, "flow_track: n_levels must be in 1..8");
    if (radius < 1 || radius > FLOW_MAX_RADIUS) return fail(SFMBA_ERR_INVALID_ARG, "flow_track: radius must be in 1..10");
    if (max_iters < 1 || max_iters > FLOW_MAX_ITERS) return fail(SFMBA_ERR_INVALID_ARG, "flow_track: max_iters must be in 1..64");
    if (!std::isfinite(min_eig) || min_eig < 0.0f) return fail(SFMBA_ERR_INVALID_ARG, "flow_track: min_eig must be finite and >= 0");
    if (img_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr must start at 0");
    for (int i = 0; i < n_images; ++i) {
        if (width[i] < 1 || width[i] > 16384 || height[i] < 1 || height[i] > 16384)
            return fail(SFMBA_ERR_INVALID_ARG, "flow_track: an image dimension lies outside 1..16384");
        if (img_ptr[i + 1] - img_ptr[i] != (int64_t)width[i] * height[i] * channels)
            return fail(SFMBA_ERR_INVALID_ARG, "flow_track: img_ptr does not agree with width * height * channels");
    }
    if (n_images > 0 && !pixels) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (int rc = flow_check_pairs("flow_track", n_images, n_pairs, pair_src, pair_dst, pt_ptr)) return rc;
    const int64_t n_pts = pt_ptr[n_pairs];
    if (n_pts > 0 && (!pts || !next || !status || !err)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    for (int64_t q = 0; q < 2 * n_pts; ++q)
        if (!std::isfinite(pts[q])) return fail(SFMBA_ERR_INVALID_ARG, "flow_track: non-finite coordinate of point " + std::to_string((long long)(q / 2)));
    if (n_pairs == 0) return check_device(device);
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    // SFMBA_FLOW_TIMING: one stderr line per call with the HIP-event times of its phases (tools/flow_bench.py)
    double tm[FLOW_T_COUNT];
    const bool timing = std::getenv("SFMBA_FLOW_TIMING") != nullptr;
    rc = flow_track(ck.kit.stream, device, n_images, img_ptr, pixels, width, height, channels, n_pairs, pair_src, pair_dst, pt_ptr, pts, n_levels,
                    radius, max_iters, min_eig, next, status, err, dbg_G, dbg_state, dbg_pyramid, timing ? tm : nullptr);
    if (rc == 0 && timing)
        std::fprintf(stderr, "[sfmba flow_track] upload_ms %.6f gray_ms %.6f pyramid_ms %.6f track_ms %.6f download_ms %.6f groups %d\n",
                     tm[FLOW_T_UPLOAD], tm[FLOW_T_GRAY], tm[FLOW_T_PYRAMID], tm[FLOW_T_TRACK], tm[FLOW_T_DOWNLOAD], (int)tm[FLOW_T_GROUPS]);
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "flow_track: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("flow_track: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
int sfmba_flow_match(int device, int n_images, const int64_t* kp_ptr, const float* kp_xy, int n_pairs, const int32_t* pair_dst,
                     const int64_t* pt_ptr, const float* next, const unsigned char* status, const float* err, float max_err, float radius,
                     double ratio, int64_t* pair_ptr, int32_t* query_idx, int32_t* train_idx, float* distance, int64_t cap, int64_t* total) {
    if (cap < 0 || !kp_ptr || !pair_ptr || !total || (cap > 0 && (!query_idx || !train_idx))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (!std::isfinite(max_err)) return fail(SFMBA_ERR_INVALID_ARG, "flow_match: max_err must be finite");
    if (!std::isfinite(radius) || !(radius > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "flow_match: radius must be finite and > 0");
    if (!std::isfinite(ratio) || !(ratio > 0.0)) return fail(SFMBA_ERR_INVALID_ARG, "flow_match: ratio must be finite and > 0");
    if (int rc = flow_check_pairs("flow_match", n_images, n_pairs, nullptr, pair_dst, pt_ptr)) return rc;
    if (kp_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, "flow_match: kp_ptr must start at 0");
    for (int i = 0; i < n_images; ++i) {
        const int64_t n = kp_ptr[i + 1] - kp_ptr[i];
        if (n < 0) return fail(SFMBA_ERR_INVALID_ARG, "flow_match: kp_ptr not monotone");
        if (n >= ((int64_t)1 << 22)) return fail(SFMBA_ERR_INVALID_ARG, "flow_match: an image has 2^22 or more key points");
    }
    const int64_t n_pts = pt_ptr[n_pairs];
    if ((n_pts > 0 && (!next || !status || !err)) || (kp_ptr[n_images] > 0 && !kp_xy)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (n_pts == 0) {
        for (int p = 0; p <= n_pairs; ++p) pair_ptr[p] = 0;
        *total = 0;
        return check_device(device);
    }
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    double tm[FLOWM_T_COUNT];
    const bool timing = std::getenv("SFMBA_FLOW_TIMING") != nullptr;
    rc = flow_match(ck.kit.stream, device, n_images, kp_ptr, kp_xy, n_pairs, pair_dst, pt_ptr, next, status, err, max_err, radius, ratio, pair_ptr,
                    query_idx, train_idx, distance, cap, total, timing ? tm : nullptr);
    if (rc == 0 && timing)
        std::fprintf(stderr, "[sfmba flow_match] upload_ms %.6f near_ms %.6f compact_ms %.6f download_ms %.6f\n", tm[FLOWM_T_UPLOAD], tm[FLOWM_T_NEAR],
                     tm[FLOWM_T_COMPACT], tm[FLOWM_T_DOWNLOAD]);
    if (rc == FLOW_ERR_CAPACITY) return fail(SFMBA_ERR_CAPACITY, "flow_match: output capacity too small");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "flow_match: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("flow_match: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
// ---- one oriented point per surface element: a normal per depth pixel and the voxel merge (SfM::mergeDenseCloud) ------------------
int sfmba_depth_normals(int device, int n_images, const int32_t* width, const int32_t* height, const float* K, const float* P,
                        const float* const* depth, float max_rel_step, float* const* normal) {
    if ((n_images > 0 && (!depth || !normal))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (int rc = depth_check_cameras("depth_normals", n_images, width, height, K, P)) return rc;
    if (n_images > 65535) return fail(SFMBA_ERR_INVALID_ARG, "depth_normals: more than 65535 images in one call");
    if (!std::isfinite(max_rel_step) || max_rel_step < 0.0f) return fail(SFMBA_ERR_INVALID_ARG, "depth_normals: max_rel_step must be finite and >= 0");
    int64_t px = 0;
    for (int i = 0; i < n_images; ++i) {
        if (!depth[i]) continue;
        if (!normal[i]) return fail(SFMBA_ERR_INVALID_ARG, "depth_normals: an image with a depth map needs an output map");
        px += (int64_t)width[i] * height[i];
    }
    if (px >= (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "depth_normals: too many pixels with a depth map in one call (2^31)");
    if (px == 0) return check_device(device);
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    // SFMBA_CLOUD_TIMING: one stderr line per call with the HIP-event times of its phases (tools/cloud_bench.py)
    double tm[NORMALS_T_COUNT];
    const bool timing = std::getenv("SFMBA_CLOUD_TIMING") != nullptr;
    rc = depth_normals(ck.kit.stream, device, n_images, width, height, K, P, depth, max_rel_step, normal, timing ? tm : nullptr);
    if (rc == 0 && timing)
        std::fprintf(stderr, "[sfmba depth_normals] upload_ms %.6f kernel_ms %.6f download_ms %.6f\n", tm[NORMALS_T_UPLOAD], tm[NORMALS_T_KERNEL],
                     tm[NORMALS_T_DOWNLOAD]);
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "depth_normals: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("depth_normals: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
int sfmba_cloud_merge(int device, int64_t n, const float* xyz, const unsigned char* bgr, const float* normal, float voxel, int min_count,
                      float* xyz_out, unsigned char* bgr_out, float* normal_out, int32_t* count, int32_t* first, int32_t* voxel_of, int64_t cap,
                      int64_t* total, int64_t* n_skipped) {
    if (n < 0 || cap < 0 || !total || !n_skipped || (n > 0 && !xyz) ||
        (cap > 0 && (!xyz_out || !count || !first || (bgr && !bgr_out) || (normal && !normal_out))))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (n >= (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "cloud_merge: too many points in one call (2^31)");
    if (!std::isfinite(voxel) || !(voxel > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "cloud_merge: voxel must be finite and > 0");
    if (min_count < 1) return fail(SFMBA_ERR_INVALID_ARG, "cloud_merge: min_count must be >= 1");
    if (n == 0) {
        *total = 0;
        *n_skipped = 0;
        return check_device(device);
    }
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    double tm[MERGE_T_COUNT];
    const bool timing = std::getenv("SFMBA_CLOUD_TIMING") != nullptr;
    rc = cloud_merge(ck.kit.stream, device, (int)n, xyz, bgr, normal, voxel, min_count, xyz_out, bgr_out, normal_out, count, first, voxel_of, cap, total,
                     n_skipped, timing ? tm : nullptr);
    if ((rc == 0 || rc == CLOUD_ERR_CAPACITY) && timing)
        std::fprintf(stderr,
                     "[sfmba cloud_merge] upload_ms %.6f quantise_ms %.6f sort_ms %.6f runs_ms %.6f reduce_ms %.6f compact_ms %.6f finalise_ms %.6f "
                     "download_ms %.6f points %lld voxels %lld\n",
                     tm[MERGE_T_UPLOAD], tm[MERGE_T_QUANTISE], tm[MERGE_T_SORT], tm[MERGE_T_RUNS], tm[MERGE_T_REDUCE], tm[MERGE_T_COMPACT],
                     tm[MERGE_T_FINALISE], tm[MERGE_T_DOWNLOAD], (long long)n, (long long)*total);
    if (rc == CLOUD_ERR_CAPACITY) return fail(SFMBA_ERR_CAPACITY, "cloud_merge: output capacity too small");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "cloud_merge: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("cloud_merge: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
// ---- pose of a new view (SfMStereoUtilities::findCameraPoseFrom2D3DMatch) -------------------------------------------
int sfmba_pnp_ransac(int device, int n_prob, const int64_t* prob_ptr, const float* xyz, const float* uv, const float* K, int n_hyp,
                     float threshold_px, uint64_t seed, int max_refine_iters, double* pose, unsigned char* inlier,
                     sfmba_pnp_result* result, double* hyp_pose, int32_t* hyp_count) {
    if (n_prob < 0 || !prob_ptr || !K || (n_prob > 0 && (!pose || !result))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (n_hyp < 1 || n_hyp > 65536) return fail(SFMBA_ERR_INVALID_ARG, "n_hyp must be in 1..65536");
    if (!std::isfinite(threshold_px) || !(threshold_px > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "threshold_px must be finite and > 0");
    if (!std::isfinite(K[0]) || !(K[0] > 0.0f) || !std::isfinite(K[4]) || !(K[4] > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "fx and fy must be finite and > 0");
    if (max_refine_iters < 0) return fail(SFMBA_ERR_INVALID_ARG, "max_refine_iters must be >= 0");
    if (prob_ptr[0] < 0) return fail(SFMBA_ERR_INVALID_ARG, "prob_ptr must not be negative");
    for (int p = 0; p < n_prob; ++p) {
        if (prob_ptr[p + 1] < prob_ptr[p]) return fail(SFMBA_ERR_INVALID_ARG, "prob_ptr not monotone");
        if (prob_ptr[p + 1] - prob_ptr[p] >= (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "pnp_ransac: a problem has 2^31 or more points");
    }
    if (prob_ptr[n_prob] > 0 && (!xyz || !uv || !inlier)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (n_prob == 0) return check_device(device);
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    // SFMBA_PNP_TIMING: one stderr line per call with the HIP-event times of its phases (tools/pnp_bench.py)
    double tm[3];
    const bool timing = std::getenv("SFMBA_PNP_TIMING") != nullptr;
    rc = pnp_ransac(ck.kit.stream, device, n_prob, prob_ptr, xyz, uv, K, n_hyp, threshold_px, seed, max_refine_iters, pose, inlier, result,
                    hyp_pose, hyp_count, timing ? tm : nullptr);
    if (rc == 0 && timing) std::fprintf(stderr, "[sfmba pnp] upload_ms %.6f kernels_ms %.6f download_ms %.6f\n", tm[0], tm[1], tm[2]);
    if (rc == PNP_ERR_TOO_LARGE) return fail(SFMBA_ERR_INVALID_ARG, "pnp_ransac: too many problems x hypotheses for one call");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "pnp_ransac: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("pnp_ransac: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
// ---- baseline pair ranking (SfMStereoUtilities::findHomographyInliers) ------------------------------------------------
int sfmba_homography_ransac(int device, int n_images, const int64_t* img_ptr, const float* pts, int n_pairs, const int32_t* pair_left,
                            const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx, int n_hyp,
                            float threshold_px, uint64_t seed, double* H, unsigned char* inlier, sfmba_homography_result* result, double* hyp_H,
                            int32_t* hyp_count) {
    if (n_images < 0 || n_pairs < 0 || !img_ptr || !pair_ptr || (n_pairs > 0 && (!pair_left || !pair_right || !H || !result)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (n_hyp < 1 || n_hyp > 65536) return fail(SFMBA_ERR_INVALID_ARG, "n_hyp must be in 1..65536");
    if (!std::isfinite(threshold_px) || !(threshold_px > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "threshold_px must be finite and > 0");
    if (img_ptr[0] < 0 || pair_ptr[0] < 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr and pair_ptr must not be negative");
    for (int i = 0; i < n_images; ++i)
        if (img_ptr[i + 1] < img_ptr[i]) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr not monotone");
    for (int p = 0; p < n_pairs; ++p) {
        if (pair_ptr[p + 1] < pair_ptr[p]) return fail(SFMBA_ERR_INVALID_ARG, "pair_ptr not monotone");
        if (pair_ptr[p + 1] - pair_ptr[p] > (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "homography_ransac: a pair has 2^31 or more matches");
        if (pair_left[p] < 0 || pair_left[p] >= n_images || pair_right[p] < 0 || pair_right[p] >= n_images)
            return fail(SFMBA_ERR_INVALID_ARG, "pair index out of range");
    }
    if (pair_ptr[n_pairs] > pair_ptr[0] && (!query_idx || !train_idx || !inlier || !pts)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    for (int p = 0; p < n_pairs; ++p) {
        const int64_t nl = img_ptr[pair_left[p] + 1] - img_ptr[pair_left[p]], nr = img_ptr[pair_right[p] + 1] - img_ptr[pair_right[p]];
        for (int64_t e = pair_ptr[p]; e < pair_ptr[p + 1]; ++e)
            if (query_idx[e] < 0 || query_idx[e] >= nl || train_idx[e] < 0 || train_idx[e] >= nr)
                return fail(SFMBA_ERR_INVALID_ARG, "homography_ransac: a query_idx / train_idx lies outside its image");
    }
    if (n_pairs == 0) return check_device(device);
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    // SFMBA_HOMOGRAPHY_TIMING: one stderr line per call with the HIP-event times of its phases (tools/homography_bench.py)
    double tm[5];
    const bool timing = std::getenv("SFMBA_HOMOGRAPHY_TIMING") != nullptr;
    rc = homography_ransac(ck.kit.stream, device, n_images, img_ptr, pts, n_pairs, pair_left, pair_right, pair_ptr, query_idx, train_idx, n_hyp,
                           threshold_px, seed, H, inlier, result, hyp_H, hyp_count, timing ? tm : nullptr);
    if (rc == 0 && timing)
        std::fprintf(stderr, "[sfmba homography] upload_ms %.6f hypotheses_ms %.6f score_ms %.6f select_ms %.6f download_ms %.6f\n", tm[0], tm[1], tm[2],
                     tm[3], tm[4]);
    if (rc == HOM_ERR_TOO_LARGE) return fail(SFMBA_ERR_INVALID_ARG, "homography_ransac: too many pairs x hypotheses for one call");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "homography_ransac: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("homography_ransac: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
// ---- pose of an image pair (SfMStereoUtilities::findCameraMatricesFromMatch) -------------------------------------------
int sfmba_essential_ransac(int device, int n_images, const int64_t* img_ptr, const float* pts, int n_pairs, const int32_t* pair_left,
                           const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx, const float* K,
                           int n_hyp, float threshold_px, uint64_t seed, double* E, double* pose, unsigned char* inlier,
                           sfmba_essential_result* result, double* hyp_E, int32_t* hyp_count, int32_t* hyp_nsol) {
    if (n_images < 0 || n_pairs < 0 || !img_ptr || !pair_ptr || !K || (n_pairs > 0 && (!pair_left || !pair_right || !E || !pose || !result)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (n_hyp < 1 || n_hyp > 65536) return fail(SFMBA_ERR_INVALID_ARG, "n_hyp must be in 1..65536");
    if (!std::isfinite(threshold_px) || !(threshold_px > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "threshold_px must be finite and > 0");
    if (!std::isfinite(K[0]) || !(K[0] > 0.0f) || !std::isfinite(K[4]) || !(K[4] > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "fx and fy must be finite and > 0");
    if (img_ptr[0] < 0 || pair_ptr[0] < 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr and pair_ptr must not be negative");
    for (int i = 0; i < n_images; ++i)
        if (img_ptr[i + 1] < img_ptr[i]) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr not monotone");
    for (int p = 0; p < n_pairs; ++p) {
        if (pair_ptr[p + 1] < pair_ptr[p]) return fail(SFMBA_ERR_INVALID_ARG, "pair_ptr not monotone");
        if (pair_ptr[p + 1] - pair_ptr[p] > (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "essential_ransac: a pair has 2^31 or more matches");
        if (pair_left[p] < 0 || pair_left[p] >= n_images || pair_right[p] < 0 || pair_right[p] >= n_images)
            return fail(SFMBA_ERR_INVALID_ARG, "pair index out of range");
    }
    if (pair_ptr[n_pairs] > pair_ptr[0] && (!query_idx || !train_idx || !inlier || !pts)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    for (int p = 0; p < n_pairs; ++p) {
        const int64_t nl = img_ptr[pair_left[p] + 1] - img_ptr[pair_left[p]], nr = img_ptr[pair_right[p] + 1] - img_ptr[pair_right[p]];
        for (int64_t e = pair_ptr[p]; e < pair_ptr[p + 1]; ++e)
            if (query_idx[e] < 0 || query_idx[e] >= nl || train_idx[e] < 0 || train_idx[e] >= nr)
                return fail(SFMBA_ERR_INVALID_ARG, "essential_ransac: a query_idx / train_idx lies outside its image");
    }
    if (n_pairs == 0) return check_device(device);
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    // SFMBA_ESSENTIAL_TIMING: one stderr line per call with the HIP-event times of its phases (tools/essential_bench.py)
    double tm[5];
    const bool timing = std::getenv("SFMBA_ESSENTIAL_TIMING") != nullptr;
    rc = essential_ransac(ck.kit.stream, device, n_images, img_ptr, pts, n_pairs, pair_left, pair_right, pair_ptr, query_idx, train_idx, K, n_hyp,
                          threshold_px, seed, E, pose, inlier, result, hyp_E, hyp_count, hyp_nsol, timing ? tm : nullptr);
    if (rc == 0 && timing)
        std::fprintf(stderr, "[sfmba essential] upload_ms %.6f hypotheses_ms %.6f score_ms %.6f select_ms %.6f download_ms %.6f\n", tm[0], tm[1], tm[2],
                     tm[3], tm[4]);
    if (rc == ESS_ERR_TOO_LARGE) return fail(SFMBA_ERR_INVALID_ARG, "essential_ransac: too many pairs x hypotheses for one call");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, "essential_ransac: device allocation failed");
    if (rc) return fail(SFMBA_ERR_HIP, std::string("essential_ransac: ") + hipGetErrorString((hipError_t)rc));
    return SFMBA_OK;
}
// ---- reading photographs (SfM::setImagesDirectory: imread + resize) ---------------------------------------------------
static int check_file_ptr(int n_images, const int64_t* file_ptr, const unsigned char* bytes) {
    if (n_images < 0 || !file_ptr) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (file_ptr[0] < 0) return fail(SFMBA_ERR_INVALID_ARG, "file_ptr must not be negative");
    for (int i = 0; i < n_images; ++i)
        if (file_ptr[i + 1] < file_ptr[i]) return fail(SFMBA_ERR_INVALID_ARG, "file_ptr not monotone");
    if (file_ptr[n_images] > file_ptr[0] && !bytes) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    return SFMBA_OK;
}

static int image_result(int rc, const char* what, const double* tm) {
    if (rc == 0 && tm)
        std::fprintf(stderr, "[sfmba %s] entropy_ms %.6f upload_ms %.6f idct_ms %.6f colour_ms %.6f resize_ms %.6f download_ms %.6f groups %d\n", what,
                     tm[JPEG_T_ENTROPY], tm[JPEG_T_UPLOAD], tm[JPEG_T_IDCT], tm[JPEG_T_COLOUR], tm[JPEG_T_RESIZE], tm[JPEG_T_DOWNLOAD], (int)tm[JPEG_T_GROUPS]);
    if (rc == 0) return SFMBA_OK;
    if (rc == JPEG_ERR_CAPACITY) return fail(SFMBA_ERR_CAPACITY, std::string(what) + ": output capacity too small");
    if (rc == JPEG_ERR_HOST_ALLOC) return fail(SFMBA_ERR_ALLOC, std::string(what) + ": host allocation failed");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, std::string(what) + ": device allocation failed");
    return fail(SFMBA_ERR_HIP, std::string(what) + ": " + hipGetErrorString((hipError_t)rc));
}

int sfmba_jpeg_info(int n_images, const int64_t* file_ptr, const unsigned char* bytes, sfmba_image_info* info) {
    if (const int rc = check_file_ptr(n_images, file_ptr, bytes)) return rc;
    if (n_images > 0 && !info) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    std::vector<JpegHeader> hdr;
    jpeg_parse_batch(n_images, file_ptr, bytes, hdr);
    for (int i = 0; i < n_images; ++i) jpeg_fill_info(hdr[(size_t)i], &info[i]);
    return SFMBA_OK;
}

int sfmba_resized_size(int width, int height, float factor, int32_t* out_width, int32_t* out_height) {
    if (!out_width || !out_height) return fail(SFMBA_ERR_INVALID_ARG, "NULL argument");
    if (!std::isfinite(factor) || !(factor > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "factor must be finite and > 0");
    if (width < 1 || width > JPEG_MAX_SIDE || height < 1 || height > JPEG_MAX_SIDE) return fail(SFMBA_ERR_INVALID_ARG, "an image dimension lies outside 1..16384");
    const int ow = resized_length(width, factor), oh = resized_length(height, factor);
    if (ow == 0 || oh == 0) return fail(SFMBA_ERR_INVALID_ARG, "the factor gives the image a side outside 1..16384");
    *out_width = ow; *out_height = oh;
    return SFMBA_OK;
}

int sfmba_jpeg_decode(int device, int n_images, const int64_t* file_ptr, const unsigned char* bytes, float factor, sfmba_image_info* info,
                      int64_t* out_ptr, unsigned char* out, int64_t cap, int64_t* total) {
    if (const int rc = check_file_ptr(n_images, file_ptr, bytes)) return rc;
    if (cap < 0 || !out_ptr || !total || (n_images > 0 && !info) || (cap > 0 && !out)) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (!std::isfinite(factor) || !(factor > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "jpeg_decode: factor must be finite and > 0");
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    // SFMBA_JPEG_TIMING: one stderr line per call with the host time of the entropy decode and the HIP-event times of the phases (tools/image_io_bench.py)
    double tm[JPEG_T_COUNT];
    const bool timing = std::getenv("SFMBA_JPEG_TIMING") != nullptr;
    rc = jpeg_decode(ck.kit.stream, device, n_images, file_ptr, bytes, factor, info, out_ptr, out, cap, total, timing ? tm : nullptr);
    if (rc == JPEG_ERR_SIZE) return fail(SFMBA_ERR_INVALID_ARG, "jpeg_decode: the factor gives an image a side outside 1..16384");
    return image_result(rc, "jpeg_decode", timing ? tm : nullptr);
}

int sfmba_resize_images(int device, int n_images, const int64_t* img_ptr, const unsigned char* px, const int32_t* width, const int32_t* height,
                        int channels, float factor, int64_t* out_ptr, unsigned char* out, int64_t cap, int64_t* total) {
    if (n_images < 0 || cap < 0 || !img_ptr || !out_ptr || !total || (n_images > 0 && (!width || !height)) || (cap > 0 && !out))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (channels != 1 && channels != 3) return fail(SFMBA_ERR_INVALID_ARG, "resize_images: channels must be 1 or 3");
    if (!std::isfinite(factor) || !(factor > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "resize_images: factor must be finite and > 0");
    if (img_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr must start at 0");
    for (int i = 0; i < n_images; ++i) {
        if (width[i] < 1 || width[i] > JPEG_MAX_SIDE || height[i] < 1 || height[i] > JPEG_MAX_SIDE)
            return fail(SFMBA_ERR_INVALID_ARG, "resize_images: an image dimension lies outside 1..16384");
        if (img_ptr[i + 1] - img_ptr[i] != (int64_t)width[i] * height[i] * channels)
            return fail(SFMBA_ERR_INVALID_ARG, "resize_images: img_ptr does not agree with width * height * channels");
        if (resized_length(width[i], factor) == 0 || resized_length(height[i], factor) == 0)
            return fail(SFMBA_ERR_INVALID_ARG, "resize_images: the factor gives an image a side outside 1..16384");
    }
    if (n_images > 0 && !px) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    double tm[JPEG_T_COUNT];
    const bool timing = std::getenv("SFMBA_JPEG_TIMING") != nullptr;
    rc = resize_images(ck.kit.stream, device, n_images, img_ptr, px, width, height, channels, factor, out_ptr, out, cap, total, timing ? tm : nullptr);
    if (rc == JPEG_ERR_SIZE) return fail(SFMBA_ERR_INVALID_ARG, "resize_images: the factor gives an image a side outside 1..16384");
    return image_result(rc, "resize_images", timing ? tm : nullptr);
}

int sfmba_png_info(int n_images, const int64_t* file_ptr, const unsigned char* bytes, struct sfmba_png_info* info) {
    if (const int rc = check_file_ptr(n_images, file_ptr, bytes)) return rc;
    if (n_images > 0 && !info) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    std::vector<PngHeader> hdr;
    png_parse_batch(n_images, file_ptr, bytes, hdr);
    for (int i = 0; i < n_images; ++i) png_fill_info(hdr[(size_t)i], &info[i]);
    return SFMBA_OK;
}

int sfmba_png_decode(int device, int n_images, const int64_t* file_ptr, const unsigned char* bytes, float factor, struct sfmba_png_info* info,
                     int64_t* out_ptr, unsigned char* out, int64_t cap, int64_t* total) {
    if (const int rc = check_file_ptr(n_images, file_ptr, bytes)) return rc;
    if (cap < 0 || !out_ptr || !total || (n_images > 0 && !info) || (cap > 0 && !out)) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (!std::isfinite(factor) || !(factor > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "png_decode: factor must be finite and > 0");
    CallKit ck;
    int rc = ck.open(device);
    if (rc) return rc;
    // SFMBA_PNG_TIMING: one stderr line per call with the host time of the inflate and the HIP-event times of the phases (tools/image_io_bench.py)
    double tm[PNG_T_COUNT];
    const bool timing = std::getenv("SFMBA_PNG_TIMING") != nullptr;
    rc = png_decode(ck.kit.stream, device, n_images, file_ptr, bytes, factor, info, out_ptr, out, cap, total, timing ? tm : nullptr);
    if (rc == JPEG_ERR_SIZE) return fail(SFMBA_ERR_INVALID_ARG, "png_decode: the factor gives an image a side outside 1..16384");
    if (rc == 0 && timing)
        std::fprintf(stderr, "[sfmba png_decode] inflate_ms %.6f upload_ms %.6f unfilter_ms %.6f pixels_ms %.6f resize_ms %.6f download_ms %.6f groups %d\n",
                     tm[PNG_T_INFLATE], tm[PNG_T_UPLOAD], tm[PNG_T_UNFILTER], tm[PNG_T_PIXELS], tm[PNG_T_RESIZE], tm[PNG_T_DOWNLOAD], (int)tm[PNG_T_GROUPS]);
    return image_result(rc, "png_decode", nullptr);
}
}  // extern "C"
