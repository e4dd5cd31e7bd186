/*
 * sfmba_oracle.c -- CPU fp64 restatement of the reference bundle-adjustment path.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load it; the product path (sfm-toy-library_amd)
 * never links or calls anything in oracle/.
 *
 * What it restates (paths relative to the reference checkout):
 *   SfMToyLib/SfMBundleAdjustmentUtils.cpp:58-97   SimpleReprojectionError functor
 *   SfMToyLib/SfMBundleAdjustmentUtils.cpp:111-166 marshalling (float angle-axis, pp subtraction)
 *   SfMToyLib/SfMBundleAdjustmentUtils.cpp:171-179 ceres::Solve(DENSE_SCHUR, 500 it, 10 s)
 *   SfMToyLib/SfMBundleAdjustmentUtils.cpp:182-221 convergence gate + write-back
 *   SfMToyLib/SfMUnitTests.cpp:80-95,153-189       projection known-answer fixture
 *
 * The arithmetic of the path lives in Ceres Solver, an UN-VENDORED, UN-PINNED dependency
 * (reference CMakeLists.txt:30 `find_package(Ceres REQUIRED)`; 2016-era => 1.11/1.12).  Ceres
 * is not in /root/reference and not installable here, so the functions below restate its
 * published algorithms [Ceres-upstream]: rotation.h (AngleAxisRotatePoint,
 * RotationMatrixToAngleAxis via quaternion, AngleAxisToRotationMatrix,
 * EulerAnglesToRotationMatrix), jet.h forward-mode autodiff (Jet<double,10>),
 * TrustRegionMinimizer + LevenbergMarquardtStrategy (Jacobi scaling, diagonal clamp
 * [1e-6,1e32], radius update, tolerance tests) and SchurEliminator + dense LLT.
 *
 * PARITY STATUS: the projection model is pinned by the reference's own known-answer
 * fixture (SfMUnitTests.cpp:153-189, tests/test_oracle_kat.py).  The SOLVER result on a bundle
 * adjustment is "parity unpinned": the reference stores no expected cost / pose for adjustBundle
 * and cannot be built here.  What IS pinned since round 6 is the LM / trust-region CONTROL FLOW:
 * lm_trust_region() below is one function that runs both the bundle adjustment and Powell's
 * function, and on the latter it reproduces the minimizer output Ceres itself published in its
 * tutorial to every printed digit (14 rows x 6 numbers, the final cost and x, the gradient of the
 * termination message: tests/golden/ceres_powell_trace.json, tests/test_oracle_kat.py) -- and
 * the tutorial's first example (f = 10 - x: three rows, ending on the PARAMETER tolerance, the
 * brief report's iteration count and final cost: tests/golden/ceres_helloworld_trace.json).  The
 * Schur elimination underneath is cross-checked against scipy.optimize.least_squares, the KKT
 * conditions and the full normal equations (tests/test_oracle_solver.py).
 */
#include <math.h>
#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "../include/sfmba.h"

#define ORACLE_API __attribute__((visibility("default")))

ORACLE_API void sfmba_oracle_options_default(sfmba_options* o);

static double wall_seconds(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* ------------------------------------------------------------------------------------------
 * rotation.h restatements [Ceres-upstream]
 * ---------------------------------------------------------------------------------------- */

/* ceres::AngleAxisRotatePoint<double> (called at BA.cpp:69). */
ORACLE_API void sfmba_oracle_angle_axis_rotate_point(const double w[3], const double pt[3], double out[3]) {
    const double theta2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    if (theta2 > DBL_EPSILON) {
        const double theta = sqrt(theta2);
        const double costheta = cos(theta);
        const double sintheta = sin(theta);
        const double theta_inverse = 1.0 / theta;
        const double k[3] = { w[0] * theta_inverse, w[1] * theta_inverse, w[2] * theta_inverse };
        const double kxp[3] = { k[1] * pt[2] - k[2] * pt[1], k[2] * pt[0] - k[0] * pt[2], k[0] * pt[1] - k[1] * pt[0] };
        const double tmp = (k[0] * pt[0] + k[1] * pt[1] + k[2] * pt[2]) * (1.0 - costheta);
        out[0] = pt[0] * costheta + kxp[0] * sintheta + k[0] * tmp;
        out[1] = pt[1] * costheta + kxp[1] * sintheta + k[1] * tmp;
        out[2] = pt[2] * costheta + kxp[2] * sintheta + k[2] * tmp;
    } else {
        /* first-order branch: R ~ I + [w]x */
        const double wxp[3] = { w[1] * pt[2] - w[2] * pt[1], w[2] * pt[0] - w[0] * pt[2], w[0] * pt[1] - w[1] * pt[0] };
        out[0] = pt[0] + wxp[0];
        out[1] = pt[1] + wxp[1];
        out[2] = pt[2] + wxp[2];
    }
}

/* Same in float: the reference's unit test runs it with T=float (SfMUnitTests.cpp:165-170). */
ORACLE_API void sfmba_oracle_angle_axis_rotate_point_f(const float w[3], const float pt[3], float out[3]) {
    const float theta2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    if (theta2 > (float)DBL_EPSILON) {
        const float theta = sqrtf(theta2);
        const float costheta = cosf(theta);
        const float sintheta = sinf(theta);
        const float theta_inverse = 1.0f / theta;
        const float k[3] = { w[0] * theta_inverse, w[1] * theta_inverse, w[2] * theta_inverse };
        const float kxp[3] = { k[1] * pt[2] - k[2] * pt[1], k[2] * pt[0] - k[0] * pt[2], k[0] * pt[1] - k[1] * pt[0] };
        const float tmp = (k[0] * pt[0] + k[1] * pt[1] + k[2] * pt[2]) * (1.0f - costheta);
        out[0] = pt[0] * costheta + kxp[0] * sintheta + k[0] * tmp;
        out[1] = pt[1] * costheta + kxp[1] * sintheta + k[1] * tmp;
        out[2] = pt[2] * costheta + kxp[2] * sintheta + k[2] * tmp;
    } else {
        const float wxp[3] = { w[1] * pt[2] - w[2] * pt[1], w[2] * pt[0] - w[0] * pt[2], w[0] * pt[1] - w[1] * pt[0] };
        out[0] = pt[0] + wxp[0];
        out[1] = pt[1] + wxp[1];
        out[2] = pt[2] + wxp[2];
    }
}

/*
 * ceres::RotationMatrixToAngleAxis<float> on a COLUMN-major 3x3 (BA.cpp:126 passes R.t().val,
 * i.e. R in column-major; SfMUnitTests.cpp:162 does the same): RotationMatrixToQuaternion
 * followed by QuaternionToAngleAxis, all in float.
 */
ORACLE_API void sfmba_oracle_rotation_matrix_to_angle_axis_f(const float Rcm[9], float aa[3]) {
#define RM(r, c) Rcm[(c) * 3 + (r)]
    float q[4];
    const float trace = RM(0, 0) + RM(1, 1) + RM(2, 2);
    if (trace >= 0.0f) {
        float t = sqrtf(trace + 1.0f);
        q[0] = 0.5f * t;
        t = 0.5f / t;
        q[1] = (RM(2, 1) - RM(1, 2)) * t;
        q[2] = (RM(0, 2) - RM(2, 0)) * t;
        q[3] = (RM(1, 0) - RM(0, 1)) * t;
    } else {
        int i = 0;
        if (RM(1, 1) > RM(0, 0)) i = 1;
        if (RM(2, 2) > RM(i, i)) i = 2;
        const int j = (i + 1) % 3;
        const int k = (j + 1) % 3;
        float t = sqrtf(RM(i, i) - RM(j, j) - RM(k, k) + 1.0f);
        q[i + 1] = 0.5f * t;
        t = 0.5f / t;
        q[0] = (RM(k, j) - RM(j, k)) * t;
        q[j + 1] = (RM(j, i) + RM(i, j)) * t;
        q[k + 1] = (RM(k, i) + RM(i, k)) * t;
    }
#undef RM
    const float q1 = q[1], q2 = q[2], q3 = q[3];
    const float sin_squared_theta = q1 * q1 + q2 * q2 + q3 * q3;
    if (sin_squared_theta > 0.0f) {
        const float sin_theta = sqrtf(sin_squared_theta);
        const float cos_theta = q[0];
        const float two_theta = 2.0f * ((cos_theta < 0.0f) ? atan2f(-sin_theta, -cos_theta)
                                                           : atan2f(sin_theta, cos_theta));
        const float k = two_theta / sin_theta;
        aa[0] = q1 * k; aa[1] = q2 * k; aa[2] = q3 * k;
    } else {
        aa[0] = q1 * 2.0f; aa[1] = q2 * 2.0f; aa[2] = q3 * 2.0f;
    }
}

/* ceres::AngleAxisToRotationMatrix<double>, COLUMN-major output (BA.cpp:203, 207). */
ORACLE_API void sfmba_oracle_angle_axis_to_rotation_matrix(const double aa[3], double Rcm[9]) {
#define RM(r, c) Rcm[(c) * 3 + (r)]
    const double theta2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
    if (theta2 > DBL_EPSILON) {
        const double theta = sqrt(theta2);
        const double wx = aa[0] / theta, wy = aa[1] / theta, wz = aa[2] / theta;
        const double costheta = cos(theta), sintheta = sin(theta);
        RM(0, 0) = costheta + wx * wx * (1.0 - costheta);
        RM(1, 0) = wz * sintheta + wx * wy * (1.0 - costheta);
        RM(2, 0) = -wy * sintheta + wx * wz * (1.0 - costheta);
        RM(0, 1) = wx * wy * (1.0 - costheta) - wz * sintheta;
        RM(1, 1) = costheta + wy * wy * (1.0 - costheta);
        RM(2, 1) = wx * sintheta + wy * wz * (1.0 - costheta);
        RM(0, 2) = wy * sintheta + wx * wz * (1.0 - costheta);
        RM(1, 2) = -wx * sintheta + wy * wz * (1.0 - costheta);
        RM(2, 2) = costheta + wz * wz * (1.0 - costheta);
    } else {
        RM(0, 0) = 1.0;     RM(1, 0) = aa[2];   RM(2, 0) = -aa[1];
        RM(0, 1) = -aa[2];  RM(1, 1) = 1.0;     RM(2, 1) = aa[0];
        RM(0, 2) = aa[1];   RM(1, 2) = -aa[0];  RM(2, 2) = 1.0;
    }
#undef RM
}

/* ceres::EulerAnglesToRotationMatrix<float>(euler_deg, 3, R) -> ROW-major R (SfMUnitTests.cpp:85). */
ORACLE_API void sfmba_oracle_euler_angles_to_rotation_matrix_f(const float euler[3], float Rrm[9]) {
    const double kPi = 3.14159265358979323846;
    const float degrees_to_radians = (float)(kPi / 180.0);
    const float pitch = euler[0] * degrees_to_radians;
    const float roll = euler[1] * degrees_to_radians;
    const float yaw = euler[2] * degrees_to_radians;
    const float c1 = cosf(yaw), s1 = sinf(yaw);
    const float c2 = cosf(roll), s2 = sinf(roll);
    const float c3 = cosf(pitch), s3 = sinf(pitch);
    Rrm[0] = c1 * c2; Rrm[1] = -s1 * c3 + c1 * s2 * s3; Rrm[2] = s1 * s3 + c1 * s2 * c3;
    Rrm[3] = s1 * c2; Rrm[4] = c1 * c3 + s1 * s2 * s3;  Rrm[5] = -c1 * s3 + s1 * s2 * c3;
    Rrm[6] = -s2;     Rrm[7] = c2 * s3;                 Rrm[8] = c2 * c3;
}

/* ------------------------------------------------------------------------------------------
 * SimpleReprojectionError (BA.cpp:58-97): T=double and T=Jet<double,10>
 * ---------------------------------------------------------------------------------------- */

/* T = double: residual only (what Ceres calls for the trial-point cost). */
ORACLE_API void sfmba_oracle_residual(const double cam[6], const double pt[3], double focal,
                                      double ox, double oy, double r[2]) {
    double p[3];
    sfmba_oracle_angle_axis_rotate_point(cam, pt, p);
    p[0] += cam[3]; p[1] += cam[4]; p[2] += cam[5];
    const double xp = p[0] / p[2];
    const double yp = p[1] / p[2];
    r[0] = focal * xp - ox;
    r[1] = focal * yp - oy;
}

/* Minimal forward-mode dual number: value + 10 partials (cam 0..5, point 6..8, focal 9),
 * i.e. ceres::Jet<double,10> as AutoDiffCostFunction<...,2,6,3,1> instantiates it (BA.cpp:92). */
#define NJ 10
typedef struct { double a; double v[NJ]; } jet;

static inline jet jet_var(double a, int k) { jet j; j.a = a; for (int i = 0; i < NJ; ++i) j.v[i] = 0.0; j.v[k] = 1.0; return j; }
static inline jet jet_const(double a) { jet j; j.a = a; for (int i = 0; i < NJ; ++i) j.v[i] = 0.0; return j; }
static inline jet jet_add(jet x, jet y) { jet z; z.a = x.a + y.a; for (int i = 0; i < NJ; ++i) z.v[i] = x.v[i] + y.v[i]; return z; }
static inline jet jet_sub(jet x, jet y) { jet z; z.a = x.a - y.a; for (int i = 0; i < NJ; ++i) z.v[i] = x.v[i] - y.v[i]; return z; }
static inline jet jet_mul(jet x, jet y) { jet z; z.a = x.a * y.a; for (int i = 0; i < NJ; ++i) z.v[i] = x.a * y.v[i] + x.v[i] * y.a; return z; }
static inline jet jet_div(jet x, jet y) {
    /* Ceres jet.h: h = f/g ; dh = (df - h dg)/g */
    jet z; const double ginv = 1.0 / y.a; z.a = x.a * ginv;
    for (int i = 0; i < NJ; ++i) z.v[i] = (x.v[i] - z.a * y.v[i]) * ginv;
    return z;
}
static inline jet jet_sqrt(jet x) { jet z; z.a = sqrt(x.a); const double t = 1.0 / (2.0 * z.a); for (int i = 0; i < NJ; ++i) z.v[i] = x.v[i] * t; return z; }
static inline jet jet_cos(jet x) { jet z; z.a = cos(x.a); const double s = -sin(x.a); for (int i = 0; i < NJ; ++i) z.v[i] = s * x.v[i]; return z; }
static inline jet jet_sin(jet x) { jet z; z.a = sin(x.a); const double c = cos(x.a); for (int i = 0; i < NJ; ++i) z.v[i] = c * x.v[i]; return z; }

/*
 * T = Jet: residual + the 2x6 / 2x3 / 2x1 Jacobian blocks exactly as Ceres autodiff yields
 * them, including the derivative of the first-order branch when theta^2 <= epsilon.
 * jc[2][6], jp[2][3], jf[2] row-major.
 */
ORACLE_API void sfmba_oracle_residual_jacobian(const double cam[6], const double pt[3], double focal,
                                               double ox, double oy, double r[2],
                                               double jc[12], double jp[6], double jf[2]) {
    jet c[6], X[3], f = jet_var(focal, 9);
    for (int k = 0; k < 6; ++k) c[k] = jet_var(cam[k], k);
    for (int k = 0; k < 3; ++k) X[k] = jet_var(pt[k], 6 + k);
    jet p[3];
    const jet theta2 = jet_add(jet_add(jet_mul(c[0], c[0]), jet_mul(c[1], c[1])), jet_mul(c[2], c[2]));
    if (theta2.a > DBL_EPSILON) {
        const jet theta = jet_sqrt(theta2);
        const jet costheta = jet_cos(theta);
        const jet sintheta = jet_sin(theta);
        const jet theta_inverse = jet_div(jet_const(1.0), theta);
        const jet w[3] = { jet_mul(c[0], theta_inverse), jet_mul(c[1], theta_inverse), jet_mul(c[2], theta_inverse) };
        const jet wxp[3] = { jet_sub(jet_mul(w[1], X[2]), jet_mul(w[2], X[1])),
                             jet_sub(jet_mul(w[2], X[0]), jet_mul(w[0], X[2])),
                             jet_sub(jet_mul(w[0], X[1]), jet_mul(w[1], X[0])) };
        const jet dot = jet_add(jet_add(jet_mul(w[0], X[0]), jet_mul(w[1], X[1])), jet_mul(w[2], X[2]));
        const jet tmp = jet_mul(dot, jet_sub(jet_const(1.0), costheta));
        for (int k = 0; k < 3; ++k)
            p[k] = jet_add(jet_add(jet_mul(X[k], costheta), jet_mul(wxp[k], sintheta)), jet_mul(w[k], tmp));
    } else {
        const jet wxp[3] = { jet_sub(jet_mul(c[1], X[2]), jet_mul(c[2], X[1])),
                             jet_sub(jet_mul(c[2], X[0]), jet_mul(c[0], X[2])),
                             jet_sub(jet_mul(c[0], X[1]), jet_mul(c[1], X[0])) };
        for (int k = 0; k < 3; ++k) p[k] = jet_add(X[k], wxp[k]);
    }
    p[0] = jet_add(p[0], c[3]); p[1] = jet_add(p[1], c[4]); p[2] = jet_add(p[2], c[5]);
    const jet xp = jet_div(p[0], p[2]);
    const jet yp = jet_div(p[1], p[2]);
    const jet res[2] = { jet_sub(jet_mul(f, xp), jet_const(ox)), jet_sub(jet_mul(f, yp), jet_const(oy)) };
    for (int row = 0; row < 2; ++row) {
        r[row] = res[row].a;
        if (jc) for (int k = 0; k < 6; ++k) jc[row * 6 + k] = res[row].v[k];
        if (jp) for (int k = 0; k < 3; ++k) jp[row * 3 + k] = res[row].v[6 + k];
        if (jf) jf[row] = res[row].v[9];
    }
}

/* Batched versions (caller's observation order). */
ORACLE_API double sfmba_oracle_eval_residuals(int n_cam, const double* cam6, int n_pt, const double* pt3,
                                              int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt,
                                              const double* obs_xy, double focal, double* residuals) {
    (void)n_cam; (void)n_pt;
    double cost = 0.0;
#pragma omp parallel for reduction(+ : cost) schedule(static)
    for (int64_t k = 0; k < n_obs; ++k) {
        double r[2];
        sfmba_oracle_residual(cam6 + 6 * (int64_t)obs_cam[k], pt3 + 3 * (int64_t)obs_pt[k], focal,
                              obs_xy[2 * k], obs_xy[2 * k + 1], r);
        if (residuals) { residuals[2 * k] = r[0]; residuals[2 * k + 1] = r[1]; }
        cost += r[0] * r[0] + r[1] * r[1];
    }
    return 0.5 * cost;
}

ORACLE_API void sfmba_oracle_eval_jacobian(int n_cam, const double* cam6, int n_pt, const double* pt3,
                                           int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt,
                                           const double* obs_xy, double focal,
                                           double* residuals, double* jc, double* jp, double* jf) {
    (void)n_cam; (void)n_pt;
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < n_obs; ++k) {
        double r[2];
        sfmba_oracle_residual_jacobian(cam6 + 6 * (int64_t)obs_cam[k], pt3 + 3 * (int64_t)obs_pt[k], focal,
                                       obs_xy[2 * k], obs_xy[2 * k + 1], r,
                                       jc ? jc + 12 * k : NULL, jp ? jp + 6 * k : NULL, jf ? jf + 2 * k : NULL);
        if (residuals) { residuals[2 * k] = r[0]; residuals[2 * k + 1] = r[1]; }
    }
}

/* ------------------------------------------------------------------------------------------
 * Dense LLT (Eigen LLT of DenseSchurComplementSolver [Ceres-upstream]); row-major, lower.
 * Returns 0 on success, k>0 if the leading minor k is not positive definite.
 * ---------------------------------------------------------------------------------------- */
static int dense_cholesky_lower(int n, double* A) {
    const int NB = 64;
    for (int kb = 0; kb < n; kb += NB) {
        const int ke = kb + NB < n ? kb + NB : n;
        /* factor the diagonal block and the panel below it, column by column */
        for (int j = kb; j < ke; ++j) {
            double d = A[(size_t)j * n + j];
            for (int t = kb; t < j; ++t) d -= A[(size_t)j * n + t] * A[(size_t)j * n + t];
            if (!(d > 0.0) || !isfinite(d)) return j + 1;
            d = sqrt(d);
            A[(size_t)j * n + j] = d;
            const double dinv = 1.0 / d;
#pragma omp parallel for schedule(static) if (n - j > 256)
            for (int i = j + 1; i < n; ++i) {
                double s = A[(size_t)i * n + j];
                const double* ai = A + (size_t)i * n;
                const double* aj = A + (size_t)j * n;
                for (int t = kb; t < j; ++t) s -= ai[t] * aj[t];
                A[(size_t)i * n + j] = s * dinv;
            }
        }
        /* trailing update: A22 -= L21 L21^T (lower part only) */
#pragma omp parallel for schedule(dynamic, 8)
        for (int i = ke; i < n; ++i) {
            const double* li = A + (size_t)i * n + kb;
            for (int j = ke; j <= i; ++j) {
                const double* lj = A + (size_t)j * n + kb;
                double s = 0.0;
                for (int t = 0; t < ke - kb; ++t) s += li[t] * lj[t];
                A[(size_t)i * n + j] -= s;
            }
        }
    }
    return 0;
}

static void dense_cholesky_solve_lower(int n, const double* L, double* x) {
    for (int i = 0; i < n; ++i) {
        double s = x[i];
        const double* li = L + (size_t)i * n;
        for (int t = 0; t < i; ++t) s -= li[t] * x[t];
        x[i] = s / li[i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = x[i];
        for (int t = i + 1; t < n; ++t) s -= L[(size_t)t * n + i] * x[t];
        x[i] = s / L[(size_t)i * n + i];
    }
}

/* A [n*n] symmetric row-major, b -> x.  info as above. */
ORACLE_API int sfmba_oracle_dense_spd_solve(int n, const double* A, const double* b, double* x) {
    double* L = (double*)malloc((size_t)n * n * sizeof(double));
    if (!L) return -1;
    memcpy(L, A, (size_t)n * n * sizeof(double));
    memcpy(x, b, (size_t)n * sizeof(double));
    const int info = dense_cholesky_lower(n, L);
    if (info == 0) dense_cholesky_solve_lower(n, L, x);
    free(L);
    return info;
}

/* ------------------------------------------------------------------------------------------
 * Problem structure shared by the solver pieces
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int n_cam, n_pt;
    int64_t n_obs;
    const int32_t* obs_cam;
    const int32_t* obs_pt;
    const double* obs_xy;
    /* active (observed) cameras / points, compacted */
    int n_acam, n_apt;
    int* cam_slot;      /* [n_cam] -> active index or -1 */
    int* pt_slot;       /* [n_pt]  -> active index or -1 */
    int* acam_id;       /* [n_acam] */
    int* apt_id;        /* [n_apt] */
    int64_t* pt_ptr;    /* [n_apt+1] CSR by active point */
    int64_t* pt_obs;    /* [n_obs] observation indices grouped by point, input order kept within a point */
    int dim;            /* 6*n_acam + 1 */
} ba_structure;

static int ba_structure_init(ba_structure* s, int n_cam, int n_pt, int64_t n_obs,
                             const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy) {
    memset(s, 0, sizeof(*s));
    s->n_cam = n_cam; s->n_pt = n_pt; s->n_obs = n_obs;
    s->obs_cam = obs_cam; s->obs_pt = obs_pt; s->obs_xy = obs_xy;
    s->cam_slot = (int*)malloc(sizeof(int) * (size_t)(n_cam > 0 ? n_cam : 1));
    s->pt_slot = (int*)malloc(sizeof(int) * (size_t)(n_pt > 0 ? n_pt : 1));
    if (!s->cam_slot || !s->pt_slot) return -1;
    for (int j = 0; j < n_cam; ++j) s->cam_slot[j] = -1;
    for (int i = 0; i < n_pt; ++i) s->pt_slot[i] = -1;
    for (int64_t k = 0; k < n_obs; ++k) {
        if (obs_cam[k] < 0 || obs_cam[k] >= n_cam || obs_pt[k] < 0 || obs_pt[k] >= n_pt) return -2;
        s->cam_slot[obs_cam[k]] = 0;
        s->pt_slot[obs_pt[k]] = 0;
    }
    for (int j = 0; j < n_cam; ++j) if (s->cam_slot[j] == 0) s->cam_slot[j] = s->n_acam++;
    for (int i = 0; i < n_pt; ++i) if (s->pt_slot[i] == 0) s->pt_slot[i] = s->n_apt++;
    s->acam_id = (int*)malloc(sizeof(int) * (size_t)(s->n_acam + 1));
    s->apt_id = (int*)malloc(sizeof(int) * (size_t)(s->n_apt + 1));
    s->pt_ptr = (int64_t*)calloc((size_t)s->n_apt + 2, sizeof(int64_t));
    s->pt_obs = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n_obs + 1));
    if (!s->acam_id || !s->apt_id || !s->pt_ptr || !s->pt_obs) return -1;
    for (int j = 0; j < n_cam; ++j) if (s->cam_slot[j] >= 0) s->acam_id[s->cam_slot[j]] = j;
    for (int i = 0; i < n_pt; ++i) if (s->pt_slot[i] >= 0) s->apt_id[s->pt_slot[i]] = i;
    for (int64_t k = 0; k < n_obs; ++k) s->pt_ptr[s->pt_slot[obs_pt[k]] + 1]++;
    for (int i = 0; i < s->n_apt; ++i) s->pt_ptr[i + 1] += s->pt_ptr[i];
    int64_t* fill = (int64_t*)malloc(sizeof(int64_t) * (size_t)(s->n_apt + 1));
    if (!fill) return -1;
    memcpy(fill, s->pt_ptr, sizeof(int64_t) * (size_t)s->n_apt);
    for (int64_t k = 0; k < n_obs; ++k) s->pt_obs[fill[s->pt_slot[obs_pt[k]]]++] = k;
    free(fill);
    s->dim = 6 * s->n_acam + 1;
    return 0;
}

static void ba_structure_free(ba_structure* s) {
    free(s->cam_slot); free(s->pt_slot); free(s->acam_id); free(s->apt_id); free(s->pt_ptr); free(s->pt_obs);
    memset(s, 0, sizeof(*s));
}

/* 3x3 SPD inverse through LLT (Ceres InvertPSDMatrix for fixed-size blocks). Returns 0 if OK. */
static int inv3_spd(const double V[9], double Vi[9]) {
    const double l00 = sqrt(V[0]);
    if (!(V[0] > 0.0)) return 1;
    const double l10 = V[3] / l00, l20 = V[6] / l00;
    const double d1 = V[4] - l10 * l10;
    if (!(d1 > 0.0)) return 1;
    const double l11 = sqrt(d1);
    const double l21 = (V[7] - l20 * l10) / l11;
    const double d2 = V[8] - l20 * l20 - l21 * l21;
    if (!(d2 > 0.0)) return 1;
    const double l22 = sqrt(d2);
    /* Linv (lower) */
    const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
    const double i10 = -l10 * i00 * i11;
    const double i21 = -l21 * i11 * i22;
    const double i20 = -(l20 * i00 + l21 * i10) * i22;
    /* Vinv = Linv^T Linv */
    Vi[0] = i00 * i00 + i10 * i10 + i20 * i20;
    Vi[1] = Vi[3] = i10 * i11 + i20 * i21;
    Vi[2] = Vi[6] = i20 * i22;
    Vi[4] = i11 * i11 + i21 * i21;
    Vi[5] = Vi[7] = i21 * i22;
    Vi[8] = i22 * i22;
    return 0;
}

/*
 * Linearisation workspace: residuals and SCALED Jacobian blocks in the caller's observation
 * order.  Unknown ordering of the full parameter vector x (size 6*n_acam + 3*n_apt + 1):
 *   [cameras (active order) | focal | points (active order)]
 * (the order only matters for norms, which are permutation invariant).
 */
typedef struct {
    double* r;    /* [2*n_obs] */
    double* jc;   /* [12*n_obs] */
    double* jp;   /* [6*n_obs]  */
    double* jf;   /* [2*n_obs]  */
} ba_lin;

/*
 * SchurEliminator + dense LLT [Ceres-upstream], for the scaled Jacobian in `lin` and the LM
 * diagonal D^2 (per parameter: dcam[6*n_acam], dfocal, dpt[3*n_apt]).
 * Solves (J^T J + D^2) y = J^T r and returns y (NOT negated) in ycam/yfocal/ypt.
 * If S_out/rhs_out are given (dim*dim / dim), the reduced system is copied there.
 * z_in (dim, or NULL): the reduced step to back-substitute instead of solving for it (sfmba_oracle_lm_step).
 * vcond (n_apt, or NULL): 2-norm condition number of every damped 3x3 point block V_i; ymag (n_apt, or NULL): |(|V_i^-1| (|b_p| + sum |E^T u|))|,
 * the size of the terms that cancel into the point step y_i (its rounding error is relative to THAT, not to |y_i|).
 * Returns 0 OK, >0 linear solver failure.
 */
static double cond3_spd(const double V[9]);
static int schur_solve(const ba_structure* s, const ba_lin* lin,
                       const double* dcam2, double dfocal2, const double* dpt2,
                       double* ycam, double* yfocal, double* ypt,
                       double* S_out, double* rhs_out, int solve, const double* z_in, double* vcond, double* ymag) {
    const int d = s->dim;
    const int fo = d - 1; /* focal index in the reduced system */
    int nthreads = 1;
#ifdef _OPENMP
    nthreads = omp_get_max_threads();
    if (nthreads > 16) nthreads = 16;
    /* private copies of S: cap memory at ~4 GB */
    while (nthreads > 1 && (double)nthreads * d * d * 8.0 > 4e9) nthreads--;
#endif
    double* Sall = (double*)calloc((size_t)nthreads * d * d, sizeof(double));
    double* rall = (double*)calloc((size_t)nthreads * d, sizeof(double));
    double* vinv = (double*)malloc(sizeof(double) * 9 * (size_t)(s->n_apt + 1));
    double* bp = (double*)malloc(sizeof(double) * 3 * (size_t)(s->n_apt + 1));
    if (!Sall || !rall || !vinv || !bp) { free(Sall); free(rall); free(vinv); free(bp); return -1; }
    int fail = 0;

#pragma omp parallel num_threads(nthreads)
    {
        int tid = 0;
#ifdef _OPENMP
        tid = omp_get_thread_num();
#endif
        double* S = Sall + (size_t)tid * d * d;
        double* rhs = rall + (size_t)tid * d;
        int maxk = 64;
        double* W = (double*)malloc(sizeof(double) * (size_t)(18 * maxk + 3)); /* per obs 6x3, then focal 1x3 */
        double* T = (double*)malloc(sizeof(double) * (size_t)(18 * maxk + 3));
        int* cj = (int*)malloc(sizeof(int) * (size_t)maxk);
#pragma omp for schedule(dynamic, 64)
        for (int i = 0; i < s->n_apt; ++i) {
            const int64_t b0 = s->pt_ptr[i], b1 = s->pt_ptr[i + 1];
            const int k = (int)(b1 - b0);
            if (k > maxk) {
                maxk = 2 * k;
                W = (double*)realloc(W, sizeof(double) * (size_t)(18 * maxk + 3));
                T = (double*)realloc(T, sizeof(double) * (size_t)(18 * maxk + 3));
                cj = (int*)realloc(cj, sizeof(int) * (size_t)maxk);
            }
            double V[9] = { dpt2[3 * i], 0, 0, 0, dpt2[3 * i + 1], 0, 0, 0, dpt2[3 * i + 2] };
            double g[3] = { 0, 0, 0 };
            double* Wf = W + 18 * k;
            Wf[0] = Wf[1] = Wf[2] = 0.0;
            for (int q = 0; q < k; ++q) {
                const int64_t o = s->pt_obs[b0 + q];
                const double* A = lin->jc + 12 * o;
                const double* B = lin->jp + 6 * o;
                const double* G = lin->jf + 2 * o;
                const double* r = lin->r + 2 * o;
                const int j = s->cam_slot[s->obs_cam[o]];
                cj[q] = j;
                for (int a = 0; a < 3; ++a) {
                    for (int b = 0; b < 3; ++b) V[3 * a + b] += B[a] * B[b] + B[3 + a] * B[3 + b];
                    g[a] += B[a] * r[0] + B[3 + a] * r[1];
                    Wf[a] += G[0] * B[a] + G[1] * B[3 + a];
                }
                double* Wq = W + 18 * q;
                for (int a = 0; a < 6; ++a)
                    for (int b = 0; b < 3; ++b) Wq[3 * a + b] = A[a] * B[b] + A[6 + a] * B[3 + b];
                /* camera-side normal-equation pieces (F^T F, F^T b) */
                double* Sjj = S + (size_t)(6 * j) * d + 6 * j;
                for (int a = 0; a < 6; ++a) {
                    for (int b = 0; b < 6; ++b) Sjj[(size_t)a * d + b] += A[a] * A[b] + A[6 + a] * A[6 + b];
                    const double af = A[a] * G[0] + A[6 + a] * G[1];
                    S[(size_t)(6 * j + a) * d + fo] += af;
                    S[(size_t)fo * d + 6 * j + a] += af;
                    rhs[6 * j + a] += A[a] * r[0] + A[6 + a] * r[1];
                }
                S[(size_t)fo * d + fo] += G[0] * G[0] + G[1] * G[1];
                rhs[fo] += G[0] * r[0] + G[1] * r[1];
            }
            double Vi[9];
            if (vcond) vcond[i] = cond3_spd(V);
            if (inv3_spd(V, Vi)) {
#pragma omp atomic write
                fail = 1;
                continue;
            }
            memcpy(vinv + 9 * i, Vi, sizeof(Vi));
            bp[3 * i] = g[0]; bp[3 * i + 1] = g[1]; bp[3 * i + 2] = g[2];
            /* T = W V^-1 for every row of the stack (6k + 1 rows) */
            const int rows = 6 * k + 1;
            for (int a = 0; a < rows; ++a)
                for (int b = 0; b < 3; ++b)
                    T[3 * a + b] = W[3 * a] * Vi[b] + W[3 * a + 1] * Vi[3 + b] + W[3 * a + 2] * Vi[6 + b];
            /* S -= T W^T ; rhs -= T g */
            for (int qa = 0; qa <= k; ++qa) {
                const int ra = qa < k ? 6 * cj[qa] : fo;
                const int na = qa < k ? 6 : 1;
                for (int a = 0; a < na; ++a) {
                    const double* Ta = T + 3 * (6 * qa + a);
                    rhs[ra + a] -= Ta[0] * g[0] + Ta[1] * g[1] + Ta[2] * g[2];
                    double* Srow = S + (size_t)(ra + a) * d;
                    for (int qb = 0; qb <= k; ++qb) {
                        const int rb = qb < k ? 6 * cj[qb] : fo;
                        const int nb = qb < k ? 6 : 1;
                        for (int b = 0; b < nb; ++b) {
                            const double* Wb = W + 3 * (6 * qb + b);
                            Srow[rb + b] -= Ta[0] * Wb[0] + Ta[1] * Wb[1] + Ta[2] * Wb[2];
                        }
                    }
                }
            }
        }
        free(W); free(T); free(cj);
    }
    /* reduce thread-private copies */
    double* S = Sall;
    double* rhs = rall;
    for (int t = 1; t < nthreads; ++t) {
        const double* St = Sall + (size_t)t * d * d;
        const double* rt = rall + (size_t)t * d;
#pragma omp parallel for schedule(static)
        for (int64_t e = 0; e < (int64_t)d * d; ++e) S[e] += St[e];
        for (int e = 0; e < d; ++e) rhs[e] += rt[e];
    }
    for (int j = 0; j < s->n_acam; ++j)
        for (int a = 0; a < 6; ++a) S[(size_t)(6 * j + a) * d + 6 * j + a] += dcam2[6 * j + a];
    S[(size_t)fo * d + fo] += dfocal2;

    if (S_out) memcpy(S_out, S, sizeof(double) * (size_t)d * d);
    if (rhs_out) memcpy(rhs_out, rhs, sizeof(double) * (size_t)d);

    int info = fail;
    if (!fail && solve) {
        if (z_in) { info = 0; memcpy(rhs, z_in, sizeof(double) * (size_t)d); }
        else info = dense_cholesky_lower(d, S);
        if (info == 0) {
            if (!z_in) dense_cholesky_solve_lower(d, S, rhs);
            for (int e = 0; e < 6 * s->n_acam; ++e) ycam[e] = rhs[e];
            *yfocal = rhs[fo];
            /* back substitution: y_e = V^-1 (E^T b - E^T F z) */
#pragma omp parallel for schedule(static)
            for (int i = 0; i < s->n_apt; ++i) {
                double t[3] = { bp[3 * i], bp[3 * i + 1], bp[3 * i + 2] };
                double ta[3] = { fabs(t[0]), fabs(t[1]), fabs(t[2]) };
                for (int64_t q = s->pt_ptr[i]; q < s->pt_ptr[i + 1]; ++q) {
                    const int64_t o = s->pt_obs[q];
                    const double* A = lin->jc + 12 * o;
                    const double* B = lin->jp + 6 * o;
                    const double* G = lin->jf + 2 * o;
                    const int j = s->cam_slot[s->obs_cam[o]];
                    double u0 = G[0] * rhs[fo], u1 = G[1] * rhs[fo];
                    for (int a = 0; a < 6; ++a) { u0 += A[a] * rhs[6 * j + a]; u1 += A[6 + a] * rhs[6 * j + a]; }
                    for (int a = 0; a < 3; ++a) { t[a] -= B[a] * u0 + B[3 + a] * u1; ta[a] += fabs(B[a] * u0) + fabs(B[3 + a] * u1); }
                }
                const double* Vi = vinv + 9 * i;
                if (ymag) {
                    double m2 = 0.0;
                    for (int a = 0; a < 3; ++a) { const double v = fabs(Vi[3 * a]) * ta[0] + fabs(Vi[3 * a + 1]) * ta[1] + fabs(Vi[3 * a + 2]) * ta[2]; m2 += v * v; }
                    ymag[i] = sqrt(m2);
                }
                for (int a = 0; a < 3; ++a) ypt[3 * i + a] = Vi[3 * a] * t[0] + Vi[3 * a + 1] * t[1] + Vi[3 * a + 2] * t[2];
            }
        }
    }
    free(Sall); free(rall); free(vinv); free(bp);
    return info;
}

/* ------------------------------------------------------------------------------------------
 * Evaluation helpers on the compacted parameter vectors
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    double* cam;   /* [6*n_acam] */
    double* pt;    /* [3*n_apt]  */
    double focal;
} ba_params;

/* Residual-only cost; returns 0 and sets *cost, or 1 if any residual is non-finite
 * (Ceres: evaluation failure -> candidate cost = DBL_MAX). */
static int eval_cost(const ba_structure* s, const ba_params* x, double* cost) {
    double c = 0.0;
    int bad = 0;
#pragma omp parallel for reduction(+ : c) reduction(| : bad) schedule(static)
    for (int64_t k = 0; k < s->n_obs; ++k) {
        double r[2];
        sfmba_oracle_residual(x->cam + 6 * (int64_t)s->cam_slot[s->obs_cam[k]],
                              x->pt + 3 * (int64_t)s->pt_slot[s->obs_pt[k]], x->focal,
                              s->obs_xy[2 * k], s->obs_xy[2 * k + 1], r);
        if (!isfinite(r[0]) || !isfinite(r[1])) bad |= 1;
        c += r[0] * r[0] + r[1] * r[1];
    }
    *cost = 0.5 * c;
    return bad;
}

/* Residuals + UNSCALED Jacobian blocks; returns 1 on non-finite values. */
static int eval_lin(const ba_structure* s, const ba_params* x, ba_lin* lin, double* cost) {
    double c = 0.0;
    int bad = 0;
#pragma omp parallel for reduction(+ : c) reduction(| : bad) schedule(static)
    for (int64_t k = 0; k < s->n_obs; ++k) {
        double* r = lin->r + 2 * k;
        sfmba_oracle_residual_jacobian(x->cam + 6 * (int64_t)s->cam_slot[s->obs_cam[k]],
                                       x->pt + 3 * (int64_t)s->pt_slot[s->obs_pt[k]], x->focal,
                                       s->obs_xy[2 * k], s->obs_xy[2 * k + 1], r,
                                       lin->jc + 12 * k, lin->jp + 6 * k, lin->jf + 2 * k);
        int b = !isfinite(r[0]) || !isfinite(r[1]);
        for (int e = 0; e < 12; ++e) b |= !isfinite(lin->jc[12 * k + e]);
        for (int e = 0; e < 6; ++e) b |= !isfinite(lin->jp[6 * k + e]);
        b |= !isfinite(lin->jf[2 * k]) || !isfinite(lin->jf[2 * k + 1]);
        bad |= b;
        c += r[0] * r[0] + r[1] * r[1];
    }
    *cost = 0.5 * c;
    return bad;
}

/* gradient g = J^T r (UNSCALED J) and squared column norms; any output may be NULL. */
static void accumulate_columns(const ba_structure* s, const ba_lin* lin,
                               double* gcam, double* gfocal, double* gpt,
                               double* ncam, double* nfocal, double* npt) {
    const int nc = 6 * s->n_acam, np = 3 * s->n_apt;
    if (gcam) memset(gcam, 0, sizeof(double) * (size_t)nc);
    if (gpt) memset(gpt, 0, sizeof(double) * (size_t)np);
    if (ncam) memset(ncam, 0, sizeof(double) * (size_t)nc);
    if (npt) memset(npt, 0, sizeof(double) * (size_t)np);
    double gf = 0.0, nf = 0.0;
    for (int64_t k = 0; k < s->n_obs; ++k) {
        const int j = s->cam_slot[s->obs_cam[k]];
        const int i = s->pt_slot[s->obs_pt[k]];
        const double* A = lin->jc + 12 * k;
        const double* B = lin->jp + 6 * k;
        const double* G = lin->jf + 2 * k;
        const double* r = lin->r + 2 * k;
        for (int a = 0; a < 6; ++a) {
            if (gcam) gcam[6 * j + a] += A[a] * r[0] + A[6 + a] * r[1];
            if (ncam) ncam[6 * j + a] += A[a] * A[a] + A[6 + a] * A[6 + a];
        }
        for (int a = 0; a < 3; ++a) {
            if (gpt) gpt[3 * i + a] += B[a] * r[0] + B[3 + a] * r[1];
            if (npt) npt[3 * i + a] += B[a] * B[a] + B[3 + a] * B[3 + a];
        }
        gf += G[0] * r[0] + G[1] * r[1];
        nf += G[0] * G[0] + G[1] * G[1];
    }
    if (gfocal) *gfocal = gf;
    if (nfocal) *nfocal = nf;
}

static void scale_columns(const ba_structure* s, ba_lin* lin, const double* scam, double sfocal, const double* spt) {
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < s->n_obs; ++k) {
        const int j = s->cam_slot[s->obs_cam[k]];
        const int i = s->pt_slot[s->obs_pt[k]];
        for (int a = 0; a < 6; ++a) { lin->jc[12 * k + a] *= scam[6 * j + a]; lin->jc[12 * k + 6 + a] *= scam[6 * j + a]; }
        for (int a = 0; a < 3; ++a) { lin->jp[6 * k + a] *= spt[3 * i + a]; lin->jp[6 * k + 3 + a] *= spt[3 * i + a]; }
        lin->jf[2 * k] *= sfocal; lin->jf[2 * k + 1] *= sfocal;
    }
}

static double params_norm(const ba_structure* s, const ba_params* x) {
    double n = x->focal * x->focal;
    for (int e = 0; e < 6 * s->n_acam; ++e) n += x->cam[e] * x->cam[e];
    for (int e = 0; e < 3 * s->n_apt; ++e) n += x->pt[e] * x->pt[e];
    return sqrt(n);
}

static double max_abs(const double* v, int n) {
    double m = 0.0;
    for (int e = 0; e < n; ++e) { const double a = fabs(v[e]); if (a > m || a != a) m = a; }
    return m;
}

/* ------------------------------------------------------------------------------------------
 * Reduced system only (parity check of the HIP Schur kernels).  S [dim*dim], rhs [dim],
 * scale [dim] in (active cameras..., focal) order.
 * ---------------------------------------------------------------------------------------- */
/* 2-norm condition number of a symmetric positive definite 3x3 matrix: its eigenvalues in closed form (the trigonometric
 * solution of the characteristic cubic); infinity if it is not positive definite */
static double cond3_spd(const double V[9]) {
    const double p1 = V[1] * V[1] + V[2] * V[2] + V[5] * V[5];
    const double q = (V[0] + V[4] + V[8]) / 3.0;
    const double p2 = (V[0] - q) * (V[0] - q) + (V[4] - q) * (V[4] - q) + (V[8] - q) * (V[8] - q) + 2.0 * p1;
    const double p = sqrt(p2 / 6.0);
    if (!(p > 0.0)) return q > 0.0 ? 1.0 : INFINITY;
    double B[9];
    for (int e = 0; e < 9; ++e) B[e] = (V[e] - ((e % 4) == 0 ? q : 0.0)) / p;
    const double detB = B[0] * (B[4] * B[8] - B[5] * B[7]) - B[1] * (B[3] * B[8] - B[5] * B[6]) + B[2] * (B[3] * B[7] - B[4] * B[6]);
    const double r = fmin(1.0, fmax(-1.0, detB / 2.0));
    const double phi = acos(r) / 3.0;
    const double e1 = q + 2.0 * p * cos(phi), e3 = q + 2.0 * p * cos(phi + 2.0 * M_PI / 3.0);
    return e3 > 0.0 ? e1 / e3 : INFINITY;
}

/* build_reduced and lm_step: the damped, scaled reduced system at the given parameters; solve = 1 also the step */
static int reduced_step(int n_cam, const double* cam6, int n_pt, const double* pt3,
                        int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt,
                        const double* obs_xy, double focal, const sfmba_options* opt_in,
                        double radius, double* S, double* rhs, double* scale,
                        int solve, const double* z_in, double* z_out, double* dpt_out, double* vcond_out, double* dmag_out) {
    sfmba_options opt;
    if (opt_in) opt = *opt_in; else sfmba_oracle_options_default(&opt);
    ba_structure s;
    if (ba_structure_init(&s, n_cam, n_pt, n_obs, obs_cam, obs_pt, obs_xy)) { ba_structure_free(&s); return -1; }
    const int nc = 6 * s.n_acam, np = 3 * s.n_apt;
    ba_params x = { (double*)malloc(sizeof(double) * (size_t)(nc + 1)), (double*)malloc(sizeof(double) * (size_t)(np + 1)), focal };
    for (int j = 0; j < s.n_acam; ++j) memcpy(x.cam + 6 * j, cam6 + 6 * (size_t)s.acam_id[j], 6 * sizeof(double));
    for (int i = 0; i < s.n_apt; ++i) memcpy(x.pt + 3 * i, pt3 + 3 * (size_t)s.apt_id[i], 3 * sizeof(double));
    ba_lin lin = { (double*)malloc(sizeof(double) * 2 * (size_t)(n_obs + 1)), (double*)malloc(sizeof(double) * 12 * (size_t)(n_obs + 1)),
                   (double*)malloc(sizeof(double) * 6 * (size_t)(n_obs + 1)), (double*)malloc(sizeof(double) * 2 * (size_t)(n_obs + 1)) };
    double cost;
    eval_lin(&s, &x, &lin, &cost);
    double* scam = (double*)malloc(sizeof(double) * (size_t)(nc + 1));
    double* spt = (double*)malloc(sizeof(double) * (size_t)(np + 1));
    double* dcam = (double*)malloc(sizeof(double) * (size_t)(nc + 1));
    double* dpt = (double*)malloc(sizeof(double) * (size_t)(np + 1));
    double sfocal = 1.0, dfocal;
    accumulate_columns(&s, &lin, NULL, NULL, NULL, scam, &sfocal, spt);
    if (opt.jacobi_scaling) {
        for (int e = 0; e < nc; ++e) scam[e] = 1.0 / (1.0 + sqrt(scam[e]));
        for (int e = 0; e < np; ++e) spt[e] = 1.0 / (1.0 + sqrt(spt[e]));
        sfocal = 1.0 / (1.0 + sqrt(sfocal));
    } else {
        for (int e = 0; e < nc; ++e) scam[e] = 1.0;
        for (int e = 0; e < np; ++e) spt[e] = 1.0;
        sfocal = 1.0;
    }
    scale_columns(&s, &lin, scam, sfocal, spt);
    accumulate_columns(&s, &lin, NULL, NULL, NULL, dcam, &dfocal, dpt);
#define CLAMPD(v) fmin(fmax((v), opt.min_lm_diagonal), opt.max_lm_diagonal) / radius
    for (int e = 0; e < nc; ++e) dcam[e] = CLAMPD(dcam[e]);
    for (int e = 0; e < np; ++e) dpt[e] = CLAMPD(dpt[e]);
    dfocal = CLAMPD(dfocal);
#undef CLAMPD
    double* ycam = solve ? (double*)malloc(sizeof(double) * (size_t)(nc + 1)) : NULL;
    double* ypt = solve ? (double*)malloc(sizeof(double) * (size_t)(np + 1)) : NULL;
    double* vcond_a = vcond_out ? (double*)malloc(sizeof(double) * (size_t)(s.n_apt + 1)) : NULL;
    double* ymag_a = dmag_out ? (double*)calloc((size_t)s.n_apt + 1, sizeof(double)) : NULL;
    double yfocal = 0.0;
    const int info = schur_solve(&s, &lin, dcam, dfocal, dpt, ycam, &yfocal, ypt, S, rhs, solve, z_in, vcond_a, ymag_a);
    if (scale) { memcpy(scale, scam, sizeof(double) * (size_t)nc); scale[nc] = sfocal; }
    if (solve && info == 0) {
        /* z in the reduced unknowns (scaled); the point step unscaled, in caller order, as k_point_update subtracts it */
        if (z_out) { memcpy(z_out, ycam, sizeof(double) * (size_t)nc); z_out[nc] = yfocal; }
        if (dpt_out) {
            memset(dpt_out, 0, sizeof(double) * 3 * (size_t)n_pt);
            for (int i = 0; i < s.n_apt; ++i)
                for (int c = 0; c < 3; ++c) dpt_out[3 * (size_t)s.apt_id[i] + c] = ypt[3 * i + c] * spt[3 * i + c];
        }
    }
    if (vcond_out) {
        memset(vcond_out, 0, sizeof(double) * (size_t)n_pt);
        for (int i = 0; i < s.n_apt; ++i) vcond_out[s.apt_id[i]] = vcond_a[i];
    }
    if (dmag_out) {      /* (unscaled like dpt) */
        memset(dmag_out, 0, sizeof(double) * (size_t)n_pt);
        for (int i = 0; i < s.n_apt; ++i) dmag_out[s.apt_id[i]] = ymag_a[i] * fmax(spt[3 * i], fmax(spt[3 * i + 1], spt[3 * i + 2]));
    }
    free(x.cam); free(x.pt); free(lin.r); free(lin.jc); free(lin.jp); free(lin.jf);
    free(scam); free(spt); free(dcam); free(dpt); free(ycam); free(ypt); free(vcond_a); free(ymag_a);
    ba_structure_free(&s);
    return info;
}

ORACLE_API int sfmba_oracle_build_reduced(int n_cam, const double* cam6, int n_pt, const double* pt3,
                                          int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt,
                                          const double* obs_xy, double focal, const sfmba_options* opt_in,
                                          double radius, double* S, double* rhs, double* scale) {
    return reduced_step(n_cam, cam6, n_pt, pt3, n_obs, obs_cam, obs_pt, obs_xy, focal, opt_in, radius, S, rhs, scale, 0, NULL, NULL, NULL, NULL, NULL);
}

/* One LM step of the DENSE_SCHUR solver at the given parameters and radius (tests/linear_step_check.py): build_reduced's S, rhs
 * and scale, the exact reduced step z (Cholesky of S) -- or, with z_in, that z taken as given and only back-substituted --, the
 * unscaled point step dpt [3 * n_pt] in caller order (x0 - dpt are the trial points), cond(V_i) [n_pt] of every damped 3x3
 * point block and dmag [n_pt], the size of the terms that cancel into each point's step (0 for points without observations).  Any
 * output may be NULL.  Returns 0, or > 0 if a factorisation failed. */
ORACLE_API int sfmba_oracle_lm_step(int n_cam, const double* cam6, int n_pt, const double* pt3,
                                    int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt,
                                    const double* obs_xy, double focal, const sfmba_options* opt_in,
                                    double radius, double* S, double* rhs, double* scale,
                                    const double* z_in, double* z, double* dpt, double* vcond, double* dmag) {
    return reduced_step(n_cam, cam6, n_pt, pt3, n_obs, obs_cam, obs_pt, obs_xy, focal, opt_in, radius, S, rhs, scale, 1, z_in, z, dpt, vcond, dmag);
}

/* ------------------------------------------------------------------------------------------
 * ceres::Solve restatement: TrustRegionMinimizer + LevenbergMarquardtStrategy + DENSE_SCHUR
 * [Ceres-upstream], options as BA.cpp:171-177 (defaults in sfmba_options_default).
 * ---------------------------------------------------------------------------------------- */
/* Which upstream ordering of the function-tolerance exit the loop below follows.  The reference links an UN-PINNED Ceres
 * (CMakeLists.txt:30), so the parity claim has to hold under every ordering an upstream release could have had:
 *   0 (default)  the >= 1.12 minimizer: ParameterToleranceReached() -> FunctionToleranceReached() -> IsStepSuccessful();
 *                a tolerance exit returns with x NOT advanced to the candidate (|cost_change| <= tol * cost).
 *   1            "step first": the candidate of the terminating iteration is accepted (if IsStepSuccessful()) BEFORE the
 *                function-tolerance exit is taken, i.e. the final x is one (tiny) step further -- the ordering VERDICT r4
 *                attributes to the <= 1.11 minimizer.
 *   2            the >= 1.12 order with the strict comparison of the <= 1.11 sources (|cost_change| < tol * cost).
 * tests/test_oracle_solver.py holds the final RMS of the fixtures to < 1e-6 px across all three: the unpinned solver parity
 * is bounded against the upstream differences we know of. */
static int g_minimizer_variant = 0;
ORACLE_API void sfmba_oracle_set_minimizer_variant(int v) { g_minimizer_variant = (v == 1 || v == 2) ? v : 0; }
ORACLE_API int sfmba_oracle_minimizer_variant(void) { return g_minimizer_variant; }

static void trace_push(sfmba_iteration* trace, int cap, int* len, const sfmba_iteration* it) {
    if (trace && *len < cap) trace[*len] = *it;
    if (len) (*len)++;
}

/* ------------------------------------------------------------------------------------------
 * The trust-region loop itself, on a generic (evaluate, solve) pair -- round 6: the SAME loop runs the bundle adjustment below and
 * the dense test problems of sfmba_oracle_solve_dense (Powell's function from the Ceres tutorial, whose per-iteration output Ceres
 * itself published: tests/golden/ceres_powell_trace.json).  Everything that is LM / trust-region CONTROL FLOW lives here --
 * IterationZero, Jacobi scaling computed once at x_0, the clamped diagonal re-used after an unsuccessful step, invalid-step handling,
 * parameter tolerance -> function tolerance -> IsStepSuccessful, the radius update of LevenbergMarquardtStrategy::StepAccepted /
 * StepRejected / StepIsInvalid, gradient tolerance, minimum radius, the iteration and time limits [Ceres-upstream
 * TrustRegionMinimizer::Minimize, LevenbergMarquardtStrategy]; a model supplies the arithmetic on its own storage.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    void* ctx;
    double (*x_norm)(void* ctx);                             /* |x| at the current point */
    int    (*linearise)(void* ctx, double* cost);            /* residuals + UNSCALED Jacobian at the current point; 1 = evaluation failed */
    double (*gradient_max)(void* ctx, int with_col_norms);   /* max |J^T r| of the unscaled Jacobian just evaluated; with_col_norms: also keep its squared column norms */
    void   (*jacobi_scale_init)(void* ctx, int enabled);     /* s = 1 / (1 + sqrt(column norm^2)) from the norms kept above (or 1) */
    void   (*apply_scale)(void* ctx);                        /* J <- J diag(s) */
    void   (*lm_diagonal)(void* ctx, double lo, double hi);  /* diag <- clamp(diag(J~^T J~), lo, hi) */
    int    (*solve)(void* ctx, double radius);               /* (J~^T J~ + diag / radius) y = J~^T r; 1 = failed or non-finite */
    double (*model_cost_change)(void* ctx);                  /* -(J~ step)^T (r + J~ step / 2), step = -y */
    double (*candidate)(void* ctx, double* cand_cost);       /* x_n = x + step * s; returns |x - x_n|; cost at x_n (DBL_MAX if the evaluation fails) */
    void   (*accept)(void* ctx);                             /* x <- x_n */
} lm_model;

static void lm_trust_region(const lm_model* m, const sfmba_options* optp, sfmba_summary* sump, double* cost_out,
                            sfmba_iteration* trace, int trace_cap, int* tlp, double t_start) {
    const sfmba_options opt = *optp;
    sfmba_summary sum = *sump;
    int tl = *tlp;
    double cost = 0.0;
    double radius = opt.initial_radius;
    double decrease_factor = 2.0;
    int reuse_diagonal = 0;
    int consecutive_invalid = 0;
    sfmba_iteration it;
    memset(&it, 0, sizeof(it));

    /* ---- iteration 0: IterationZero() ---- */
    double x_norm = m->x_norm(m->ctx);
    if (m->linearise(m->ctx, &cost)) {
        sum.termination = SFMBA_FAILURE;
        snprintf(sum.message, sizeof(sum.message), "Initial residual and Jacobian evaluation failed.");
        goto done;
    }
    sum.jacobian_evals = 1;
    sum.initial_cost = cost;
    it.gradient_max_norm = m->gradient_max(m->ctx, 1);
    m->jacobi_scale_init(m->ctx, opt.jacobi_scaling);
    m->apply_scale(m->ctx);
    it.iteration = 0; it.cost = cost; it.trust_region_radius = radius;
    trace_push(trace, trace_cap, &tl, &it);
    if (opt.verbose) fprintf(stderr, "[oracle] it %3d cost %.12e |g|inf %.3e radius %.3e\n", 0, cost, it.gradient_max_norm, radius);
    for (;;) {
        /* FinalizeIterationAndCheckIfMinimizerCanContinue(): "a. run time  b. iteration count  c. max norm of the gradient  d. size of the trust region
         * radius" [Ceres-upstream, in that order: an iteration that meets the gradient tolerance AND the iteration limit ends as NO_CONVERGENCE --
         * tests/fuzz_parity.py --options found the two the other way round here; it.gradient_max_norm of a rejected or invalid step is the previous one] */
        if (opt.max_seconds > 0.0 && wall_seconds() - t_start >= opt.max_seconds) {
            sum.termination = SFMBA_NO_CONVERGENCE;
            snprintf(sum.message, sizeof(sum.message), "Maximum solver time reached.");
            break;
        }
        if (it.iteration >= opt.max_iters) {
            sum.termination = SFMBA_NO_CONVERGENCE;
            snprintf(sum.message, sizeof(sum.message), "Maximum number of iterations reached.");
            break;
        }
        if (it.gradient_max_norm <= opt.gradient_tolerance) {
            sum.termination = SFMBA_CONVERGENCE;
            snprintf(sum.message, sizeof(sum.message), "Gradient tolerance reached.");
            break;
        }
        if (radius <= opt.min_radius) {
            sum.termination = SFMBA_CONVERGENCE;
            snprintf(sum.message, sizeof(sum.message), "Minimum trust region radius reached.");
            break;
        }
        const double prev_gmax = it.gradient_max_norm;
        memset(&it, 0, sizeof(it));
        it.iteration = sum.iterations + 1;
        sum.iterations = it.iteration;

        /* LevenbergMarquardtStrategy::ComputeStep */
        if (!reuse_diagonal) m->lm_diagonal(m->ctx, opt.min_lm_diagonal, opt.max_lm_diagonal);
        const int lin_fail = m->solve(m->ctx, radius);
        reuse_diagonal = 1;

        double model_cost_change = 0.0;
        int step_valid = 0;
        if (!lin_fail) {
            model_cost_change = m->model_cost_change(m->ctx);
            step_valid = model_cost_change > 0.0;
        }
        it.step_is_valid = step_valid;

        if (!step_valid) {
            /* HandleInvalidStep() */
            if (++consecutive_invalid >= opt.max_consecutive_invalid_steps) {
                sum.termination = SFMBA_FAILURE;
                snprintf(sum.message, sizeof(sum.message), "Number of consecutive invalid steps more than max_num_consecutive_invalid_steps.");
                it.cost = cost; it.gradient_max_norm = prev_gmax; it.trust_region_radius = radius;
                trace_push(trace, trace_cap, &tl, &it);
                break;
            }
            radius *= 0.5; /* StepIsInvalid */
            reuse_diagonal = 1;
            it.cost = cost; it.gradient_max_norm = prev_gmax; it.trust_region_radius = radius;
            sum.unsuccessful_steps++;
            trace_push(trace, trace_cap, &tl, &it);
            if (opt.verbose) fprintf(stderr, "[oracle] it %3d invalid step, radius -> %.3e\n", it.iteration, radius);
            continue;
        }
        consecutive_invalid = 0;

        /* candidate x + delta, delta = step * scale (undo Jacobi scaling) */
        double cand_cost;
        it.step_norm = m->candidate(m->ctx, &cand_cost);
        sum.residual_evals++;

        /* ParameterToleranceReached() */
        const double step_size_tolerance = opt.parameter_tolerance * (x_norm + opt.parameter_tolerance);
        if (it.step_norm <= step_size_tolerance) {
            sum.termination = SFMBA_CONVERGENCE;
            snprintf(sum.message, sizeof(sum.message), "Parameter tolerance reached.");
            it.cost = cost; it.gradient_max_norm = prev_gmax; it.trust_region_radius = radius;
            trace_push(trace, trace_cap, &tl, &it);
            break;
        }
        /* FunctionToleranceReached() */
        it.cost_change = cost - cand_cost;
        const int ftol_hit = g_minimizer_variant == 2 ? fabs(it.cost_change) < opt.function_tolerance * cost
                                                      : fabs(it.cost_change) <= opt.function_tolerance * cost;
        if (ftol_hit && g_minimizer_variant != 1) {
            sum.termination = SFMBA_CONVERGENCE;
            snprintf(sum.message, sizeof(sum.message), "Function tolerance reached.");
            it.cost = cost; it.gradient_max_norm = prev_gmax; it.trust_region_radius = radius;
            trace_push(trace, trace_cap, &tl, &it);
            break;
        }
        /* IsStepSuccessful() (monotonic steps) */
        it.relative_decrease = it.cost_change / model_cost_change;
        it.step_is_successful = it.relative_decrease > opt.min_relative_decrease;
        if (ftol_hit) {
            /* variant 1 ("step first"): the terminating iteration's candidate is taken if it is a successful step, then the exit */
            if (it.step_is_successful) {
                m->accept(m->ctx);
                cost = cand_cost;
                sum.successful_steps++;
            }
            sum.termination = SFMBA_CONVERGENCE;
            snprintf(sum.message, sizeof(sum.message), "Function tolerance reached.");
            it.cost = cost; it.gradient_max_norm = prev_gmax; it.trust_region_radius = radius;
            trace_push(trace, trace_cap, &tl, &it);
            break;
        }

        if (it.step_is_successful) {
            /* HandleSuccessfulStep() */
            m->accept(m->ctx);
            x_norm = m->x_norm(m->ctx);
            if (m->linearise(m->ctx, &cost)) {
                sum.termination = SFMBA_FAILURE;
                snprintf(sum.message, sizeof(sum.message), "Residual and Jacobian evaluation failed.");
                break;
            }
            sum.jacobian_evals++;
            it.gradient_max_norm = m->gradient_max(m->ctx, 0);
            m->apply_scale(m->ctx);
            /* StepAccepted */
            radius = radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * it.relative_decrease - 1.0, 3));
            radius = fmin(opt.max_radius, radius);
            decrease_factor = 2.0;
            reuse_diagonal = 0;
            sum.successful_steps++;
        } else {
            it.gradient_max_norm = prev_gmax;
            /* StepRejected */
            radius = radius / decrease_factor;
            decrease_factor *= 2.0;
            reuse_diagonal = 1;
            sum.unsuccessful_steps++;
        }
        it.cost = it.step_is_successful ? cost : cand_cost;
        it.trust_region_radius = radius;
        trace_push(trace, trace_cap, &tl, &it);
        if (opt.verbose)
            fprintf(stderr, "[oracle] it %3d cost %.12e dcost %.3e |g|inf %.3e |step| %.3e rho %.3e radius %.3e %s\n",
                    it.iteration, cost, it.cost_change, it.gradient_max_norm, it.step_norm, it.relative_decrease, radius,
                    it.step_is_successful ? "ok" : "rejected");
        /* (the checks of FinalizeIterationAndCheckIfMinimizerCanContinue() follow at the top of the loop) */
    }
done:
    *cost_out = cost;
    *sump = sum;
    *tlp = tl;
}

/* ---- the bundle-adjustment model of that loop: SchurEliminator + dense LLT on the storage of ba_structure / ba_lin ---- */
typedef struct {
    const ba_structure* s;
    ba_params x, xn;
    ba_lin lin;
    double *scam, *spt, *gcam, *gpt, *diagc, *diagp, *dcam, *dpt, *ycam, *ypt;
    double sfocal, gfocal, diagf, yfocal;
} ba_model;

static double bam_x_norm(void* c) { ba_model* b = (ba_model*)c; return params_norm(b->s, &b->x); }
static int bam_linearise(void* c, double* cost) { ba_model* b = (ba_model*)c; return eval_lin(b->s, &b->x, &b->lin, cost); }
static double bam_gradient_max(void* c, int with_col_norms) {
    ba_model* b = (ba_model*)c;
    const int nc = 6 * b->s->n_acam, np = 3 * b->s->n_apt;
    if (with_col_norms) accumulate_columns(b->s, &b->lin, b->gcam, &b->gfocal, b->gpt, b->scam, &b->sfocal, b->spt);
    else accumulate_columns(b->s, &b->lin, b->gcam, &b->gfocal, b->gpt, NULL, NULL, NULL);
    return fmax(fmax(max_abs(b->gcam, nc), max_abs(b->gpt, np)), fabs(b->gfocal));
}
static void bam_jacobi_scale_init(void* c, int enabled) {
    ba_model* b = (ba_model*)c;
    const int nc = 6 * b->s->n_acam, np = 3 * b->s->n_apt;
    if (enabled) {
        for (int e = 0; e < nc; ++e) b->scam[e] = 1.0 / (1.0 + sqrt(b->scam[e]));
        for (int e = 0; e < np; ++e) b->spt[e] = 1.0 / (1.0 + sqrt(b->spt[e]));
        b->sfocal = 1.0 / (1.0 + sqrt(b->sfocal));
    } else {
        for (int e = 0; e < nc; ++e) b->scam[e] = 1.0;
        for (int e = 0; e < np; ++e) b->spt[e] = 1.0;
        b->sfocal = 1.0;
    }
}
static void bam_apply_scale(void* c) { ba_model* b = (ba_model*)c; scale_columns(b->s, &b->lin, b->scam, b->sfocal, b->spt); }
static void bam_lm_diagonal(void* c, double lo, double hi) {
    ba_model* b = (ba_model*)c;
    const int nc = 6 * b->s->n_acam, np = 3 * b->s->n_apt;
    accumulate_columns(b->s, &b->lin, NULL, NULL, NULL, b->diagc, &b->diagf, b->diagp);
    for (int e = 0; e < nc; ++e) b->diagc[e] = fmin(fmax(b->diagc[e], lo), hi);
    for (int e = 0; e < np; ++e) b->diagp[e] = fmin(fmax(b->diagp[e], lo), hi);
    b->diagf = fmin(fmax(b->diagf, lo), hi);
}
static int bam_solve(void* c, double radius) {
    ba_model* b = (ba_model*)c;
    const int nc = 6 * b->s->n_acam, np = 3 * b->s->n_apt;
    for (int e = 0; e < nc; ++e) b->dcam[e] = b->diagc[e] / radius;
    for (int e = 0; e < np; ++e) b->dpt[e] = b->diagp[e] / radius;
    const double dfocal = b->diagf / radius;
    int lin_fail = schur_solve(b->s, &b->lin, b->dcam, dfocal, b->dpt, b->ycam, &b->yfocal, b->ypt, NULL, NULL, 1, NULL, NULL, NULL);
    if (!lin_fail) {
        int ok = isfinite(b->yfocal);
        for (int e = 0; e < nc && ok; ++e) ok = isfinite(b->ycam[e]);
        for (int e = 0; e < np && ok; ++e) ok = isfinite(b->ypt[e]);
        lin_fail = !ok;
    }
    return lin_fail;
}
static double bam_model_cost_change(void* c) {
    ba_model* b = (ba_model*)c;
    const ba_structure* s = b->s;
    const ba_lin lin = b->lin;
    const double* ycam = b->ycam; const double* ypt = b->ypt; const double yfocal = b->yfocal;
    /* step = -y ; model_cost_change = -(J step)^T (r + J step / 2) */
    double m = 0.0;
#pragma omp parallel for reduction(+ : m) schedule(static)
    for (int64_t k = 0; k < s->n_obs; ++k) {
        const int j = s->cam_slot[s->obs_cam[k]];
        const int i = s->pt_slot[s->obs_pt[k]];
        const double* A = lin.jc + 12 * k;
        const double* B = lin.jp + 6 * k;
        const double* G = lin.jf + 2 * k;
        double u0 = -G[0] * yfocal, u1 = -G[1] * yfocal;
        for (int a = 0; a < 6; ++a) { u0 -= A[a] * ycam[6 * j + a]; u1 -= A[6 + a] * ycam[6 * j + a]; }
        for (int a = 0; a < 3; ++a) { u0 -= B[a] * ypt[3 * i + a]; u1 -= B[3 + a] * ypt[3 * i + a]; }
        m -= u0 * (lin.r[2 * k] + 0.5 * u0) + u1 * (lin.r[2 * k + 1] + 0.5 * u1);
    }
    return m;
}
static double bam_candidate(void* c, double* cand_cost) {
    ba_model* b = (ba_model*)c;
    const int nc = 6 * b->s->n_acam, np = 3 * b->s->n_apt;
    ba_params x = b->x, xn = b->xn;
    double step_norm2 = 0.0;
    for (int e = 0; e < nc; ++e) { const double dlt = -b->ycam[e] * b->scam[e]; xn.cam[e] = x.cam[e] + dlt; const double df = x.cam[e] - xn.cam[e]; step_norm2 += df * df; }
    for (int e = 0; e < np; ++e) { const double dlt = -b->ypt[e] * b->spt[e]; xn.pt[e] = x.pt[e] + dlt; const double df = x.pt[e] - xn.pt[e]; step_norm2 += df * df; }
    { const double dlt = -b->yfocal * b->sfocal; xn.focal = x.focal + dlt; const double df = x.focal - xn.focal; step_norm2 += df * df; }
    b->xn.focal = xn.focal;
    if (eval_cost(b->s, &b->xn, cand_cost)) *cand_cost = DBL_MAX;
    return sqrt(step_norm2);
}
static void bam_accept(void* c) {
    ba_model* b = (ba_model*)c;
    const int nc = 6 * b->s->n_acam, np = 3 * b->s->n_apt;
    memcpy(b->x.cam, b->xn.cam, sizeof(double) * (size_t)nc);
    memcpy(b->x.pt, b->xn.pt, sizeof(double) * (size_t)np);
    b->x.focal = b->xn.focal;
}

ORACLE_API int sfmba_oracle_solve(int n_cam, double* cam6, int n_pt, double* pt3,
                                  int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy,
                                  double* focal, const sfmba_options* opt_in, sfmba_summary* summary,
                                  sfmba_iteration* trace, int trace_cap, int* trace_len) {
    sfmba_options opt;
    if (opt_in) opt = *opt_in; else sfmba_oracle_options_default(&opt);
    sfmba_summary sum;
    memset(&sum, 0, sizeof(sum));
    int tl = 0;
    const double t_start = wall_seconds();

    ba_structure s;
    if (ba_structure_init(&s, n_cam, n_pt, n_obs, obs_cam, obs_pt, obs_xy)) {
        ba_structure_free(&s);
        sum.termination = SFMBA_FAILURE;
        snprintf(sum.message, sizeof(sum.message), "invalid observation indices");
        if (summary) *summary = sum;
        if (trace_len) *trace_len = 0;
        return SFMBA_ERR_INVALID_ARG;
    }
    if (n_obs == 0) {
        /* Ceres: nothing to optimise -> CONVERGENCE without touching parameters. */
        sum.termination = SFMBA_CONVERGENCE;
        snprintf(sum.message, sizeof(sum.message), "Function tolerance reached. No non-constant parameter blocks found.");
        if (summary) *summary = sum;
        if (trace_len) *trace_len = 0;
        ba_structure_free(&s);
        return SFMBA_OK;
    }
    const int nc = 6 * s.n_acam, np = 3 * s.n_apt;
    ba_model b;
    memset(&b, 0, sizeof(b));
    b.s = &s;
    b.x.cam = (double*)malloc(sizeof(double) * (size_t)nc); b.x.pt = (double*)malloc(sizeof(double) * (size_t)np); b.x.focal = *focal;
    b.xn.cam = (double*)malloc(sizeof(double) * (size_t)nc); b.xn.pt = (double*)malloc(sizeof(double) * (size_t)np); b.xn.focal = 0.0;
    for (int j = 0; j < s.n_acam; ++j) memcpy(b.x.cam + 6 * j, cam6 + 6 * (size_t)s.acam_id[j], 6 * sizeof(double));
    for (int i = 0; i < s.n_apt; ++i) memcpy(b.x.pt + 3 * i, pt3 + 3 * (size_t)s.apt_id[i], 3 * sizeof(double));
    b.lin.r = (double*)malloc(sizeof(double) * 2 * (size_t)n_obs); b.lin.jc = (double*)malloc(sizeof(double) * 12 * (size_t)n_obs);
    b.lin.jp = (double*)malloc(sizeof(double) * 6 * (size_t)n_obs); b.lin.jf = (double*)malloc(sizeof(double) * 2 * (size_t)n_obs);
    b.scam = (double*)malloc(sizeof(double) * (size_t)nc); b.spt = (double*)malloc(sizeof(double) * (size_t)np);
    b.gcam = (double*)malloc(sizeof(double) * (size_t)nc); b.gpt = (double*)malloc(sizeof(double) * (size_t)np);
    b.diagc = (double*)malloc(sizeof(double) * (size_t)nc); b.diagp = (double*)malloc(sizeof(double) * (size_t)np);
    b.dcam = (double*)malloc(sizeof(double) * (size_t)nc); b.dpt = (double*)malloc(sizeof(double) * (size_t)np);
    b.ycam = (double*)malloc(sizeof(double) * (size_t)nc); b.ypt = (double*)malloc(sizeof(double) * (size_t)np);
    b.sfocal = 1.0;

    const lm_model model = { &b, bam_x_norm, bam_linearise, bam_gradient_max, bam_jacobi_scale_init, bam_apply_scale, bam_lm_diagonal, bam_solve,
                             bam_model_cost_change, bam_candidate, bam_accept };
    double cost = 0.0;
    lm_trust_region(&model, &opt, &sum, &cost, trace, trace_cap, &tl, t_start);

    sum.final_cost = cost;
    sum.seconds = wall_seconds() - t_start;
    /* parameters are updated whatever the termination type, as ceres::Solve does */
    for (int j = 0; j < s.n_acam; ++j) memcpy(cam6 + 6 * (size_t)s.acam_id[j], b.x.cam + 6 * j, 6 * sizeof(double));
    for (int i = 0; i < s.n_apt; ++i) memcpy(pt3 + 3 * (size_t)s.apt_id[i], b.x.pt + 3 * i, 3 * sizeof(double));
    *focal = b.x.focal;
    if (summary) *summary = sum;
    if (trace_len) *trace_len = tl;
    free(b.x.cam); free(b.x.pt); free(b.xn.cam); free(b.xn.pt);
    free(b.lin.r); free(b.lin.jc); free(b.lin.jp); free(b.lin.jf);
    free(b.scam); free(b.spt); free(b.gcam); free(b.gpt); free(b.diagc); free(b.diagp); free(b.dcam); free(b.dpt); free(b.ycam); free(b.ypt);
    ba_structure_free(&s);
    return SFMBA_OK;
}

/* ---- a DENSE model of the same loop: m residuals of n parameters with a caller-supplied evaluator; the LM step by Householder QR of the
 * stacked [J~; sqrt(D)] (DENSE_QR [Ceres-upstream]: the solver the Ceres tutorial runs Powell's function with).  This is how the loop above is
 * anchored to output Ceres itself published.  problem: 0 = Powell's function (examples/powell.cc [Ceres-upstream], four residuals of four
 * parameters: f1 = x1 + 10 x2, f2 = sqrt(5) (x3 - x4), f3 = (x2 - 2 x3)^2, f4 = sqrt(10) (x1 - x4)^2); 1 = the tutorial's first example,
 * f = 10 - x from x = 0.5 (examples/helloworld.cc [Ceres-upstream]; its three-row minimizer table is printed in the tutorial as well). ---- */
enum { DENSE_MAX_N = 8, DENSE_MAX_M = 8 };
typedef struct {
    int problem, n, m;
    double x[DENSE_MAX_N], xn[DENSE_MAX_N], y[DENSE_MAX_N], s[DENSE_MAX_N], g[DENSE_MAX_N], diag[DENSE_MAX_N], colsq[DENSE_MAX_N];
    double r[DENSE_MAX_M], J[DENSE_MAX_M][DENSE_MAX_N];
} dense_model;

static int dense_eval(int problem, const double* x, double* r, double (*J)[DENSE_MAX_N]) {
    if (problem == 0) {
        const double s5 = sqrt(5.0), s10 = sqrt(10.0);
        r[0] = x[0] + 10.0 * x[1];
        r[1] = s5 * (x[2] - x[3]);
        r[2] = (x[1] - 2.0 * x[2]) * (x[1] - 2.0 * x[2]);
        r[3] = s10 * (x[0] - x[3]) * (x[0] - x[3]);
        if (J) {
            memset(J, 0, sizeof(double) * DENSE_MAX_M * DENSE_MAX_N);
            J[0][0] = 1.0; J[0][1] = 10.0;
            J[1][2] = s5; J[1][3] = -s5;
            J[2][1] = 2.0 * (x[1] - 2.0 * x[2]); J[2][2] = -4.0 * (x[1] - 2.0 * x[2]);
            J[3][0] = 2.0 * s10 * (x[0] - x[3]); J[3][3] = -2.0 * s10 * (x[0] - x[3]);
        }
        return 0;
    }
    if (problem == 1) {          /* examples/helloworld.cc [Ceres-upstream]: one residual f = 10 - x */
        r[0] = 10.0 - x[0];
        if (J) { memset(J, 0, sizeof(double) * DENSE_MAX_M * DENSE_MAX_N); J[0][0] = -1.0; }
        return 0;
    }
    return 1;
}
static double dm_x_norm(void* c) { dense_model* d = (dense_model*)c; double n = 0.0; for (int e = 0; e < d->n; ++e) n += d->x[e] * d->x[e]; return sqrt(n); }
static int dm_linearise(void* c, double* cost) {
    dense_model* d = (dense_model*)c;
    if (dense_eval(d->problem, d->x, d->r, d->J)) return 1;
    double cc = 0.0; int bad = 0;
    for (int k = 0; k < d->m; ++k) { cc += d->r[k] * d->r[k]; bad |= !isfinite(d->r[k]); for (int e = 0; e < d->n; ++e) bad |= !isfinite(d->J[k][e]); }
    *cost = 0.5 * cc;
    return bad;
}
static double dm_gradient_max(void* c, int with_col_norms) {
    dense_model* d = (dense_model*)c;
    for (int e = 0; e < d->n; ++e) {
        double g = 0.0, q = 0.0;
        for (int k = 0; k < d->m; ++k) { g += d->J[k][e] * d->r[k]; q += d->J[k][e] * d->J[k][e]; }
        d->g[e] = g;
        if (with_col_norms) d->colsq[e] = q;
    }
    return max_abs(d->g, d->n);
}
static void dm_jacobi_scale_init(void* c, int enabled) { dense_model* d = (dense_model*)c; for (int e = 0; e < d->n; ++e) d->s[e] = enabled ? 1.0 / (1.0 + sqrt(d->colsq[e])) : 1.0; }
static void dm_apply_scale(void* c) { dense_model* d = (dense_model*)c; for (int k = 0; k < d->m; ++k) for (int e = 0; e < d->n; ++e) d->J[k][e] *= d->s[e]; }
static void dm_lm_diagonal(void* c, double lo, double hi) {
    dense_model* d = (dense_model*)c;
    for (int e = 0; e < d->n; ++e) { double q = 0.0; for (int k = 0; k < d->m; ++k) q += d->J[k][e] * d->J[k][e]; d->diag[e] = fmin(fmax(q, lo), hi); }
}
/* min |J~ y - r|^2 + |sqrt(diag / radius) y|^2 by Householder QR of the (m + n) x n stacked matrix */
static int dm_solve(void* c, double radius) {
    dense_model* d = (dense_model*)c;
    const int n = d->n, rows = d->m + d->n;
    double A[DENSE_MAX_M + DENSE_MAX_N][DENSE_MAX_N], b[DENSE_MAX_M + DENSE_MAX_N];
    for (int k = 0; k < d->m; ++k) { for (int e = 0; e < n; ++e) A[k][e] = d->J[k][e]; b[k] = d->r[k]; }
    for (int e = 0; e < n; ++e) { for (int f = 0; f < n; ++f) A[d->m + e][f] = 0.0; A[d->m + e][e] = sqrt(d->diag[e] / radius); b[d->m + e] = 0.0; }
    for (int col = 0; col < n; ++col) {
        double nrm = 0.0;
        for (int k = col; k < rows; ++k) nrm += A[k][col] * A[k][col];
        nrm = sqrt(nrm);
        if (!(nrm > 0.0)) return 1;
        const double alpha = A[col][col] > 0.0 ? -nrm : nrm;
        double v[DENSE_MAX_M + DENSE_MAX_N], vtv = 0.0;
        for (int k = col; k < rows; ++k) { v[k] = A[k][col]; }
        v[col] -= alpha;
        for (int k = col; k < rows; ++k) vtv += v[k] * v[k];
        if (!(vtv > 0.0)) continue;
        for (int f = col; f < n; ++f) {
            double dot = 0.0;
            for (int k = col; k < rows; ++k) dot += v[k] * A[k][f];
            const double t = 2.0 * dot / vtv;
            for (int k = col; k < rows; ++k) A[k][f] -= t * v[k];
        }
        double dot = 0.0;
        for (int k = col; k < rows; ++k) dot += v[k] * b[k];
        const double t = 2.0 * dot / vtv;
        for (int k = col; k < rows; ++k) b[k] -= t * v[k];
    }
    for (int e = n - 1; e >= 0; --e) {
        double v = b[e];
        for (int f = e + 1; f < n; ++f) v -= A[e][f] * d->y[f];
        d->y[e] = v / A[e][e];
        if (!isfinite(d->y[e])) return 1;
    }
    return 0;
}
static double dm_model_cost_change(void* c) {
    dense_model* d = (dense_model*)c;
    double mc = 0.0;
    for (int k = 0; k < d->m; ++k) { double u = 0.0; for (int e = 0; e < d->n; ++e) u -= d->J[k][e] * d->y[e]; mc -= u * (d->r[k] + 0.5 * u); }
    return mc;
}
static double dm_candidate(void* c, double* cand_cost) {
    dense_model* d = (dense_model*)c;
    double sn = 0.0, r[DENSE_MAX_M] = { 0.0 }, cc = 0.0;
    for (int e = 0; e < d->n; ++e) { const double dlt = -d->y[e] * d->s[e]; d->xn[e] = d->x[e] + dlt; const double df = d->x[e] - d->xn[e]; sn += df * df; }
    int bad = dense_eval(d->problem, d->xn, r, NULL);
    for (int k = 0; k < d->m; ++k) { cc += r[k] * r[k]; bad |= !isfinite(r[k]); }
    *cand_cost = bad ? DBL_MAX : 0.5 * cc;
    return sqrt(sn);
}
static void dm_accept(void* c) { dense_model* d = (dense_model*)c; memcpy(d->x, d->xn, sizeof(double) * (size_t)d->n); }

/* x [n] in-out.  The options are the solver's (the reference's: BA.cpp:171-177 + Ceres defaults); the linear solver field is ignored (dense QR). */
ORACLE_API int sfmba_oracle_solve_dense(int problem, int n, double* x, const sfmba_options* opt_in, sfmba_summary* summary,
                                        sfmba_iteration* trace, int trace_cap, int* trace_len) {
    if (!x || !((problem == 0 && n == 4) || (problem == 1 && n == 1))) return SFMBA_ERR_INVALID_ARG;
    sfmba_options opt;
    if (opt_in) opt = *opt_in; else sfmba_oracle_options_default(&opt);
    sfmba_summary sum;
    memset(&sum, 0, sizeof(sum));
    int tl = 0;
    const double t_start = wall_seconds();
    dense_model d;
    memset(&d, 0, sizeof(d));
    d.problem = problem; d.n = n; d.m = n;
    memcpy(d.x, x, sizeof(double) * (size_t)n);
    const lm_model model = { &d, dm_x_norm, dm_linearise, dm_gradient_max, dm_jacobi_scale_init, dm_apply_scale, dm_lm_diagonal, dm_solve,
                             dm_model_cost_change, dm_candidate, dm_accept };
    double cost = 0.0;
    lm_trust_region(&model, &opt, &sum, &cost, trace, trace_cap, &tl, t_start);
    sum.final_cost = cost;
    sum.seconds = wall_seconds() - t_start;
    memcpy(x, d.x, sizeof(double) * (size_t)n);
    if (summary) *summary = sum;
    if (trace_len) *trace_len = tl;
    return SFMBA_OK;
}

/* The oracle carries its own copy of the defaults so that it never links the product library. */
ORACLE_API void sfmba_oracle_options_default(sfmba_options* o) {
    memset(o, 0, sizeof(*o));
    o->max_iters = 500;              /* BA.cpp:174 */
    o->max_seconds = 10.0;           /* BA.cpp:176 */
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
    o->linear_solver = SFMBA_LINEAR_AUTO;   /* (the oracle itself always factorises: the field only mirrors the product's default) */
    o->precision = SFMBA_PRECISION_F64;
    o->pcg_tolerance = 1e-8;
    o->pcg_max_iters = 0;
    o->verbose = 0;
    o->pcg_anchored = 1;
}

/* OMP_NUM_THREADS is read once when libgomp initialises (torch may have done that already), so the
 * bench sets the thread count of the CPU baseline explicitly. */
ORACLE_API void sfmba_oracle_set_num_threads(int n) {
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}

ORACLE_API int sfmba_oracle_num_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* ------------------------------------------------------------------------------------------
 * adjustBundle() marshalling restated on flat arrays (BA.cpp:111-166 in, :187-221 out).
 *   poses      [n_views][12] float, row-major 3x4 (cv::Matx34f::val), in-out
 *   K          [9] float row-major 3x3 (only K(0,0), K(0,2), K(1,2) read; K(0,0), K(1,1) written)
 *   points     [n_pts][3] float, in-out
 *   view_ptr   [n_pts+1], view_idx/feat_idx [nnz]: originatingViews in ascending view order
 *   feat_ptr   [n_views+1], feat_xy [total_feats][2] float: Features::points per view
 * Returns the termination type; on anything but CONVERGENCE the in-out arrays are untouched.
 * ---------------------------------------------------------------------------------------- */
ORACLE_API int sfmba_oracle_adjust_bundle(int n_views, float* poses, float* K,
                                          int n_pts, float* points, const int64_t* view_ptr,
                                          const int32_t* view_idx, const int32_t* feat_idx,
                                          const int64_t* feat_ptr, const float* feat_xy,
                                          const sfmba_options* opt, sfmba_summary* summary) {
    double* cam6 = (double*)calloc((size_t)(6 * n_views + 1), sizeof(double));
    unsigned char* empty = (unsigned char*)calloc((size_t)n_views + 1, 1);
    for (int v = 0; v < n_views; ++v) {
        const float* P = poses + 12 * v;
        if (P[0] == 0 && P[5] == 0 && P[10] == 0) { empty[v] = 1; continue; } /* BA.cpp:118-122 */
        /* R.t().val read as column-major == R; our helper wants column-major R */
        float Rcm[9];
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rcm[c * 3 + r] = P[4 * r + c];
        float aa[3];
        sfmba_oracle_rotation_matrix_to_angle_axis_f(Rcm, aa);
        cam6[6 * v + 0] = aa[0]; cam6[6 * v + 1] = aa[1]; cam6[6 * v + 2] = aa[2];
        cam6[6 * v + 3] = P[3]; cam6[6 * v + 4] = P[7]; cam6[6 * v + 5] = P[11];
    }
    double focal = K[0];
    const int64_t nnz = view_ptr[n_pts];
    double* pt3 = (double*)malloc(sizeof(double) * (size_t)(3 * n_pts + 1));
    int32_t* oc = (int32_t*)malloc(sizeof(int32_t) * (size_t)(nnz + 1));
    int32_t* op = (int32_t*)malloc(sizeof(int32_t) * (size_t)(nnz + 1));
    double* oxy = (double*)malloc(sizeof(double) * (size_t)(2 * nnz + 2));
    for (int i = 0; i < n_pts; ++i) {
        pt3[3 * i] = points[3 * i]; pt3[3 * i + 1] = points[3 * i + 1]; pt3[3 * i + 2] = points[3 * i + 2];
        for (int64_t q = view_ptr[i]; q < view_ptr[i + 1]; ++q) {
            const int v = view_idx[q];
            const float* f2 = feat_xy + 2 * (feat_ptr[v] + feat_idx[q]);
            float px = f2[0], py = f2[1];
            px -= K[2]; py -= K[5]; /* float subtraction, BA.cpp:151-153 */
            oc[q] = v; op[q] = i; oxy[2 * q] = px; oxy[2 * q + 1] = py;
        }
    }
    sfmba_summary sum;
    sfmba_oracle_solve(n_views, cam6, n_pts, pt3, nnz, oc, op, oxy, &focal, opt, &sum, NULL, 0, NULL);
    if (summary) *summary = sum;
    if (sum.termination == SFMBA_CONVERGENCE) {
        K[0] = (float)focal; K[4] = (float)focal;
        for (int v = 0; v < n_views; ++v) {
            if (empty[v]) continue;
            double Rcm[9];
            sfmba_oracle_angle_axis_to_rotation_matrix(cam6 + 6 * v, Rcm);
            float* P = poses + 12 * v;
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) P[4 * c + r] = (float)Rcm[r * 3 + c]; /* pose(c,r)=rotationMat[r*3+c] */
            P[3] = (float)cam6[6 * v + 3]; P[7] = (float)cam6[6 * v + 4]; P[11] = (float)cam6[6 * v + 5];
        }
        for (int i = 0; i < n_pts; ++i) {
            points[3 * i] = (float)pt3[3 * i]; points[3 * i + 1] = (float)pt3[3 * i + 1]; points[3 * i + 2] = (float)pt3[3 * i + 2];
        }
    }
    free(cam6); free(empty); free(pt3); free(oc); free(op); free(oxy);
    return sum.termination;
}
