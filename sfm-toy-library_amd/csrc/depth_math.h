// depth_math.h -- the arithmetic of sfmba_depth_sweep and sfmba_depth_fuse (the contract is in include/sfmba.h), as
// __host__ __device__ functions: the kernels of depth_sweep.hip and the serial host program tools/micro/depth_math_host.hip run the
// same code, and tests/test_depth_oracle_cpu.py holds the host program to the numpy restatement bit for bit without a GPU.
// Coordinates are fp64 with every operation rounded on its own: hipcc contracts a multiply and an add into an fma by default, so
// every function with a double product that is followed by a sum switches the contraction off for its own body.  Everything between
// the coordinate and the score is integer arithmetic.
#pragma once
#include "orb_math.h"

#include <cmath>
#include <cstdint>

namespace sfmba {

#define DEPTH_HD __host__ __device__ __forceinline__

constexpr int DEPTH_TILE = 16;                 // a workgroup's tile of reference pixels is 16 x 16
constexpr int DEPTH_MAX_RADIUS = 4;
constexpr int DEPTH_MAX_SOURCES = 4;
constexpr int DEPTH_MAX_PLANES = 256;
constexpr int DEPTH_MAX_CHECKS = 4;
constexpr int DEPTH_NO_SAMPLE = 0xffff;        // a sample that is not valid (a valid one is 0..4080)

// ---- the warp of a (reference, source) pair ----------------------------------------------------------------------------------
// c = a b for row-major 3 x 3 matrices: every entry ((a_i0 b_0j) + a_i1 b_1j) + a_i2 b_2j
DEPTH_HD void depth_mat3_mul(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = a[3 * i] * b[j];
            s = s + a[3 * i + 1] * b[3 + j];
            s = s + a[3 * i + 2] * b[6 + j];
            c[3 * i + j] = s;
        }
}
// y = a x: ((a_i0 x_0) + a_i1 x_1) + a_i2 x_2
DEPTH_HD void depth_mat3_vec(const double* a, const double* x, double* y) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i) {
        double s = a[3 * i] * x[0];
        s = s + a[3 * i + 1] * x[1];
        s = s + a[3 * i + 2] * x[2];
        y[i] = s;
    }
}
// k4 = fx, fy, cx, cy; pr, ps = [R | t] of the reference and the source, row-major 3 x 4.  A = (K Rrel) Kinv, b = K trel with
// Rrel = R_s R_r^T, trel = t_s - Rrel t_r, K = [fx 0 cx; 0 fy cy; 0 0 1] and Kinv = [1/fx 0 -(cx/fx); 0 1/fy -(cy/fy); 0 0 1]; the
// zeros and the one of K and Kinv take part in the products like any other entry.
DEPTH_HD void depth_warp(const double* k4, const double* pr, const double* ps, double* A, double* b) {
#pragma clang fp contract(off)
    double RrT[9], Rs[9], tr[3], ts[3], Rrel[9], Rt[3], trel[3], M[9];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) { RrT[3 * j + i] = pr[4 * i + j]; Rs[3 * i + j] = ps[4 * i + j]; }
        tr[i] = pr[4 * i + 3];
        ts[i] = ps[4 * i + 3];
    }
    depth_mat3_mul(Rs, RrT, Rrel);
    depth_mat3_vec(Rrel, tr, Rt);
    for (int i = 0; i < 3; ++i) trel[i] = ts[i] - Rt[i];
    const double K[9] = { k4[0], 0.0, k4[2], 0.0, k4[1], k4[3], 0.0, 0.0, 1.0 };
    const double Ki[9] = { 1.0 / k4[0], 0.0, -(k4[2] / k4[0]), 0.0, 1.0 / k4[1], -(k4[3] / k4[1]), 0.0, 0.0, 1.0 };
    depth_mat3_mul(K, Rrel, M);
    depth_mat3_mul(M, Ki, A);
    depth_mat3_vec(K, trel, b);
}

// ---- planes ------------------------------------------------------------------------------------------------------------------
DEPTH_HD void depth_planes(double z_near, double z_far, int D, double& wf, double& step) {
    const double wn = 1.0 / z_near;
    wf = 1.0 / z_far;
    step = (wn - wf) / (double)(D - 1);
}
DEPTH_HD double depth_plane_w(double wf, double step, int k) {
#pragma clang fp contract(off)
    const double ks = (double)k * step;
    return wf + ks;
}

// ---- one sample --------------------------------------------------------------------------------------------------------------
// q_i = ((A_i0 u + A_i1 v) + A_i2) + w b_i, u' = q_0 / q_2, v' = q_1 / q_2; valid iff q_2 > 0, 0 <= u' <= ws - 1, 0 <= v' <= hs - 1
// (a NaN fails).
DEPTH_HD bool depth_project(const double* A, const double* b, int u, int v, double w, int ws, int hs, double& up, double& vp) {
#pragma clang fp contract(off)
    const double du = (double)u, dv = (double)v;
    double q[3];
    for (int i = 0; i < 3; ++i) {
        const double au = A[3 * i] * du, av = A[3 * i + 1] * dv, wb = w * b[i];
        q[i] = ((au + av) + A[3 * i + 2]) + wb;
    }
    up = q[0] / q[2];
    vp = q[1] / q[2];
    return q[2] > 0.0 && up >= 0.0 && up <= (double)(ws - 1) && vp >= 0.0 && vp <= (double)(hs - 1);
}
// floor(16 c + 0.5) of a valid coordinate: 0 .. 16 (n - 1)
DEPTH_HD int depth_fix(double c) {
#pragma clang fp contract(off)
    const double c16 = 16.0 * c;
    return (int)floor(c16 + 0.5);
}
// the bilinear sample at (su, sv) / 16 of a gray image, a 12-bit integer 0..4080
// (`img` is the first byte of one channel of an image whose pixels lie `channels` bytes apart)
DEPTH_HD int depth_sample_channel(const unsigned char* img, int ws, int hs, int su, int sv, int channels) {
    const int x0 = su >> 4, fx = su & 15, y0 = sv >> 4, fy = sv & 15;
    const int x1 = x0 + 1 < ws - 1 ? x0 + 1 : ws - 1, y1 = y0 + 1 < hs - 1 ? y0 + 1 : hs - 1;
    const size_t c = (size_t)channels;
    const unsigned char *r0 = img + (size_t)y0 * (size_t)ws * c, *r1 = img + (size_t)y1 * (size_t)ws * c;
    return ((16 - fx) * (16 - fy) * (int)r0[x0 * c] + fx * (16 - fy) * (int)r0[x1 * c] + (16 - fx) * fy * (int)r1[x0 * c] + fx * fy * (int)r1[x1 * c] + 8) >> 4;
}
DEPTH_HD int depth_sample(const unsigned char* img, int ws, int hs, int su, int sv) { return depth_sample_channel(img, ws, hs, su, sv, 1); }
// DEPTH_NO_SAMPLE or the sample of source pixels `img` for reference pixel (u, v) on the plane of inverse depth w
DEPTH_HD int depth_warped_sample(const double* A, const double* b, int u, int v, double w, const unsigned char* img, int ws, int hs) {
    double up, vp;
    if (!depth_project(A, b, u, v, w, ws, hs, up, vp)) return DEPTH_NO_SAMPLE;
    return depth_sample(img, ws, hs, depth_fix(up), depth_fix(vp));
}

// ---- window score ------------------------------------------------------------------------------------------------------------
// With r <= 4 (n <= 81), I <= 255 and J <= 4080: SI <= 20655, SII <= 5267025, SJ <= 330480, SIJ <= 84272400,
// SJJ <= 1348358400 < 2^31.  The variances and num are formed in int64.
DEPTH_HD long long depth_var(int n, long long s, long long ss) { return (long long)n * ss - s * s; }
DEPTH_HD long long depth_num(int n, long long si, long long sj, long long sij) { return (long long)n * sij - si * sj; }
// the reference pixel takes part (its window being inside the image) iff varI >= n^2 min_std^2 and varI > 0
DEPTH_HD bool depth_textured(int n, long long varI, int min_std) { return varI > 0 && varI >= (long long)n * n * min_std * min_std; }
// varI, varJ > 0: the product is rounded once, the root is correctly rounded, one division
DEPTH_HD double depth_score(long long num, long long varI, long long varJ) {
    const double prod = (double)varI * (double)varJ;
    return (double)num / sqrt(prod);
}

// ---- winner ------------------------------------------------------------------------------------------------------------------
// the offset of the parabola's vertex through (-1, cm), (0, c0), (1, cp) in plane steps, or 0 where it has no maximum
DEPTH_HD double depth_refine(double cm, double c0, double cp) {
#pragma clang fp contract(off)
    const double c2 = 2.0 * c0;
    const double den = (cm - c2) + cp;
    if (!(den < 0.0)) return 0.0;
    const double half = 0.5 * (cm - cp);
    return half / den;
}
DEPTH_HD float depth_value(double wf, double step, int k, double delta) {
#pragma clang fp contract(off)
    const double ds = delta * step;
    const double w = depth_plane_w(wf, step, k) + ds;
    return (float)(1.0 / w);
}

// ---- fuse --------------------------------------------------------------------------------------------------------------------
// X = R^T (Xc - t) with Xc = (z ((u - cx) / fx), z ((v - cy) / fy), z); X_j = ((R_0j d_0) + R_1j d_1) + R_2j d_2
DEPTH_HD void depth_unproject(const double* k4, const double* p, int u, int v, double z, double* X) {
#pragma clang fp contract(off)
    const double xn = ((double)u - k4[2]) / k4[0], yn = ((double)v - k4[3]) / k4[1];
    const double d[3] = { z * xn - p[3], z * yn - p[7], z - p[11] };
    for (int j = 0; j < 3; ++j) {
        double s = p[j] * d[0];
        s = s + p[4 + j] * d[1];
        s = s + p[8 + j] * d[2];
        X[j] = s;
    }
}
// q = R X + t as (((R_i0 X_0) + R_i1 X_1) + R_i2 X_2) + t_i
DEPTH_HD void depth_camera_point(const double* p, const double* X, double* q) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i) {
        double s = p[4 * i] * X[0];
        s = s + p[4 * i + 1] * X[1];
        s = s + p[4 * i + 2] * X[2];
        q[i] = s + p[4 * i + 3];
    }
}
// u = (fx q_x) / q_z + cx, v = (fy q_y) / q_z + cy
DEPTH_HD void depth_image_point(const double* k4, const double* q, double& u, double& v) {
#pragma clang fp contract(off)
    const double fu = k4[0] * q[0], fv = k4[1] * q[1];
    u = fu / q[2] + k4[2];
    v = fv / q[2] + k4[3];
}
// false unless q_z > 0 and the pixel (floor(u + 0.5), floor(v + 0.5)) of the two functions above lies inside the ws x hs image
DEPTH_HD bool depth_reproject(const double* k4, const double* p, const double* X, int ws, int hs, int& px, int& py, double& qz) {
#pragma clang fp contract(off)
    double q[3], u, v;
    depth_camera_point(p, X, q);
    qz = q[2];
    if (!(q[2] > 0.0)) return false;
    depth_image_point(k4, q, u, v);
    const double x = floor(u + 0.5), y = floor(v + 0.5);
    if (!(x >= 0.0 && x <= (double)(ws - 1) && y >= 0.0 && y <= (double)(hs - 1))) return false;
    px = (int)x;
    py = (int)y;
    return true;
}
// |zs - qz| <= rel_tol qz, for zs > 0
DEPTH_HD bool depth_agrees(double zs, double qz, double rel_tol) {
#pragma clang fp contract(off)
    const double tol = rel_tol * qz;
    return zs > 0.0 && fabs(zs - qz) <= tol;
}

}  // namespace sfmba
