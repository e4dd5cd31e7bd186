// triangulate_math.h -- the per-match arithmetic of sfmba_triangulate and sfmba_triangulate_pairs (triangulate.hip): ONE function,
// triangulate_match, that both kernels call, so that a match of a batch gets the bytes the single call gives it.
//
// SfMStereoUtilities::triangulateViews per match (SfMToyLib/SfMStereoUtilities.cpp:120-206):
//   :145-149  undistortPoints with no distortion         x_n = (u - cx)/fx, y_n = (v - cy)/fy            (-> float)
//                                                        (NaN, NaN) for a pixel that is not finite, see normalise_px
//   :151-152  cv::triangulatePoints [OpenCV-upstream]    A = [x P3 - P1; y P3 - P2] of both views, 4x4, fp64;
//                                                        X_h = right singular vector of the smallest singular value (-> float)
//   :154-155  convertPointsFromHomogeneous               X = X_h.xyz / X_h.w                               (float)
//   :157-169  projectPoints (Rodrigues(R) == R)          u = fx (R X + t)_x / (R X + t)_z + cx, fp64      (-> float)
//   :183-190  kept unless a reprojection error > max_err (MIN_REPROJECTION_ERROR = 10, :42): a NaN error is kept
// Byte equality of the two kernels rests on the compiler contracting (fusing multiply-adds in) the two inlined copies of
// triangulate_match alike, although one kernel takes its cameras from kernel arguments and the other from registers loaded from
// memory.  Nothing in the language promises that.  It holds for the compiler this was built with: the gfx950 code of both kernels has
// the same floating-point instruction mix, and tests/test_gpu_triangulate_pairs.py compares the bytes on
// the device.  Should a compiler update break that test, make triangulate_match __noinline__ or serve both entry points from
// k_triangulate_pairs; do not loosen the test.
// Everything stays in registers: the 4x4 SVD is a one-sided (Hestenes) Jacobi iteration on the columns of A with V accumulated --
// 8 sweeps of the 6 column pairs, every array index a compile-time constant, no divergence beyond the rotation skip.
#pragma once
#include <hip/hip_runtime.h>

namespace sfmba {

__device__ __forceinline__ void jacobi_pair(double A[4][4], double V[4][4], int p, int q) {
    double app = 0.0, aqq = 0.0, apq = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) { app += A[r][p] * A[r][p]; aqq += A[r][q] * A[r][q]; apq += A[r][p] * A[r][q]; }
    if (fabs(apq) <= 1e-300 || fabs(apq) <= 1e-17 * sqrt(app * aqq)) return;
    const double zeta = (aqq - app) / (2.0 * apq);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double ap = A[r][p], aq = A[r][q];
        A[r][p] = c * ap - s * aq; A[r][q] = s * ap + c * aq;
        const double vp = V[r][p], vq = V[r][q];
        V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq;
    }
}

// undistortPoints without distortion still takes the normalised point through its homogeneous product with R = I
// [OpenCV-upstream: xx = 1 x + 0 y + 0, yy = 0 x + 1 y + 0, ww = 1 / (0 x + 0 y + 1), (xx ww, yy ww)]: a finite pixel passes
// unchanged, a pixel with a NaN or an infinite coordinate comes out as (NaN, NaN) through 0 * inf -- and then has a NaN point
// and NaN errors, which the filter keeps.  Without this an infinite pixel met the rotation skip of jacobi_pair as inf <= inf,
// left V the identity and gave the finite point (1, 0, 0), dropped on its infinite error.
__device__ __forceinline__ float2 normalise_px(float2 p, double fx, double fy, double cx, double cy) {
    const double x = ((double)p.x - cx) / fx, y = ((double)p.y - cy) / fy;
    const bool finite = isfinite(x) && isfinite(y);
    const double nan = __builtin_nan("");
    return make_float2((float)(finite ? x : nan), (float)(finite ? y : nan));
}

__device__ __forceinline__ float2 project_px(const float* P, const float* K, const float X[3]) {
    const double x = (double)P[0] * X[0] + (double)P[1] * X[1] + (double)P[2] * X[2] + (double)P[3];
    const double y = (double)P[4] * X[0] + (double)P[5] * X[1] + (double)P[6] * X[2] + (double)P[7];
    const double z = (double)P[8] * X[0] + (double)P[9] * X[1] + (double)P[10] * X[2] + (double)P[11];
    return make_float2((float)((double)K[0] * x / z + (double)K[2]), (float)((double)K[4] * y / z + (double)K[5]));
}

// One match: the pixels l / r under the cameras Pl / Pr [12] and K [9] (row-major) -> the point X, the two reprojection errors
// and the verdict of the filter (true = kept).
__device__ __forceinline__ bool triangulate_match(float2 l, float2 r, const float* K, const float* Pl, const float* Pr, float max_err, float X[3],
                                                  double& el, double& er) {
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const float2 nl = normalise_px(l, fx, fy, cx, cy), nr = normalise_px(r, fx, fy, cx, cy);
    const double xl = (double)nl.x, yl = (double)nl.y, xr = (double)nr.x, yr = (double)nr.y;
    double A[4][4], V[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        A[0][c] = xl * (double)Pl[8 + c] - (double)Pl[c];
        A[1][c] = yl * (double)Pl[8 + c] - (double)Pl[4 + c];
        A[2][c] = xr * (double)Pr[8 + c] - (double)Pr[c];
        A[3][c] = yr * (double)Pr[8 + c] - (double)Pr[4 + c];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) V[rr][c] = (rr == c) ? 1.0 : 0.0;
    }
#pragma unroll 1
    for (int sweep = 0; sweep < 8; ++sweep) {
        jacobi_pair(A, V, 0, 1); jacobi_pair(A, V, 0, 2); jacobi_pair(A, V, 0, 3);
        jacobi_pair(A, V, 1, 2); jacobi_pair(A, V, 1, 3); jacobi_pair(A, V, 2, 3);
    }
    // column of the smallest singular value (branch-free selection)
    double best = 0.0, v[4] = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double nn = 0.0;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) nn += A[rr][c] * A[rr][c];
        const bool take = (c == 0) || (nn < best);
        best = take ? nn : best;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) v[rr] = take ? V[rr][c] : v[rr];
    }
    const float h[4] = { (float)v[0], (float)v[1], (float)v[2], (float)v[3] };
    const float scale = h[3] != 0.0f ? 1.0f / h[3] : 1.0f;
    X[0] = h[0] * scale; X[1] = h[1] * scale; X[2] = h[2] * scale;
    const float2 pl = project_px(Pl, K, X), pr = project_px(Pr, K, X);
    el = sqrt((double)(pl.x - l.x) * (double)(pl.x - l.x) + (double)(pl.y - l.y) * (double)(pl.y - l.y));
    er = sqrt((double)(pr.x - r.x) * (double)(pr.x - r.x) + (double)(pr.y - r.y) * (double)(pr.y - r.y));
    return !(el > (double)max_err || er > (double)max_err);
}

}  // namespace sfmba
