// pnp_math.h -- the per-lane arithmetic of sfmba_pnp_ransac (pnp_ransac.hip): the seeded sampler (ransac_common.h), P3P in closed
// form with the fourth-point disambiguation, and THE inlier decision.  Plain C++ apart from the qualifiers, so a host build can exercise it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "ransac_common.h"

namespace sfmba {

// THE inlier decision, for the count (k_pnp_score) and for the mask (k_pnp_select_refine) alike.  kp = diag(fx, fy, 1) [R|t]
// rounded to fp32, (du, dv) = the observation minus the principal point in fp32.  Division-free: with (x, y, z) = kp (X, 1) the
// pixel error is |(x, y) / z - (du, dv)|, so the test is z > 0 and |(x, y) - z (du, dv)|^2 <= thr^2 z^2.  Every operation is
// spelled out (no contraction is left to the compiler), so both kernels take the same decision for the same operands.
PNP_HD bool pnp_inlier(const float (&kp)[12], float X, float Y, float Z, float du, float dv, float thr2) {
    const float x = fmaf(kp[0], X, fmaf(kp[1], Y, fmaf(kp[2], Z, kp[3])));
    const float y = fmaf(kp[4], X, fmaf(kp[5], Y, fmaf(kp[6], Z, kp[7])));
    const float z = fmaf(kp[8], X, fmaf(kp[9], Y, fmaf(kp[10], Z, kp[11])));
    const float ex = fmaf(-du, z, x), ey = fmaf(-dv, z, y);
    const float e2 = fmaf(ex, ex, ey * ey);
    const float lim = (thr2 * z) * z;
    return z > 0.0f && e2 <= lim;
}

PNP_HD double pnp_poly4(const double (&e)[5], double x) { return (((e[4] * x + e[3]) * x + e[2]) * x + e[1]) * x + e[0]; }
PNP_HD double pnp_dpoly4(const double (&e)[5], double x) { return ((4.0 * e[4] * x + 3.0 * e[3]) * x + 2.0 * e[2]) * x + e[1]; }

// Real roots of e[4] x^4 + ... + e[0] (e[4] != 0) in closed form: Ferrari's resolvent cubic (its largest real root, by Cardano
// or the trigonometric form, polished), two quadratics, then two Newton steps per root on the quartic itself.
PNP_HD int pnp_quartic_roots(const double (&e)[5], double (&x)[4]) {
    const double a = e[3] / e[4], b = e[2] / e[4], c = e[1] / e[4], d = e[0] / e[4];
    const double a2 = a * a;
    const double p = b - 0.375 * a2;
    const double q = c - 0.5 * a * b + 0.125 * a2 * a;
    const double r = d - 0.25 * a * c + 0.0625 * a2 * b - (3.0 / 256.0) * a2 * a2;
    // m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8 = 0: its largest real root is >= 0
    const double ca = p, cb = 0.25 * p * p - r, cc = -0.125 * q * q;
    const double P = cb - ca * ca / 3.0, Q = 2.0 * ca * ca * ca / 27.0 - ca * cb / 3.0 + cc;
    const double disc = 0.25 * Q * Q + P * P * P / 27.0;
    double t;
    if (disc > 0.0) {
        const double s = sqrt(disc);
        t = cbrt(-0.5 * Q + s) + cbrt(-0.5 * Q - s);
    } else if (P < 0.0) {
        double arg = 1.5 * Q / P * sqrt(-3.0 / P);
        arg = arg > 1.0 ? 1.0 : (arg < -1.0 ? -1.0 : arg);
        t = 2.0 * sqrt(-P / 3.0) * cos(acos(arg) / 3.0);
    } else {
        t = 0.0;
    }
    double m = t - ca / 3.0;
    for (int it = 0; it < 2; ++it) {
        const double f = ((m + ca) * m + cb) * m + cc, df = (3.0 * m + 2.0 * ca) * m + cb;
        if (df != 0.0) m -= f / df;
    }
    // fixed slots (no indexed stores, so the roots stay in registers): bit i of the returned mask says x[i] is a real root
    int mask = 0;
    const double shift = -0.25 * a;
    x[0] = x[1] = x[2] = x[3] = 0.0;
    if (m > 1e-14 * (fabs(p) + 1.0)) {
        const double sq = sqrt(2.0 * m), qs = q / sq;
        const double dp = -2.0 * m - 2.0 * p - 2.0 * qs;        // y^2 - sq y + (p / 2 + m + q / (2 sq)) = 0
        const double dm = -2.0 * m - 2.0 * p + 2.0 * qs;        // y^2 + sq y + (p / 2 + m - q / (2 sq)) = 0
        if (dp >= 0.0) { const double s = sqrt(dp); x[0] = 0.5 * (sq + s) + shift; x[1] = 0.5 * (sq - s) + shift; mask |= 3; }
        if (dm >= 0.0) { const double s = sqrt(dm); x[2] = 0.5 * (-sq + s) + shift; x[3] = 0.5 * (-sq - s) + shift; mask |= 12; }
    } else {                                                     // q = 0: biquadratic in y
        const double dd = p * p - 4.0 * r;
        if (dd >= 0.0) {
            const double s = sqrt(dd), y2a = 0.5 * (-p + s), y2b = 0.5 * (-p - s);
            if (y2a >= 0.0) { const double y = sqrt(y2a); x[0] = y + shift; x[1] = -y + shift; mask |= 3; }
            if (y2b >= 0.0) { const double y = sqrt(y2b); x[2] = y + shift; x[3] = -y + shift; mask |= 12; }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const double df = pnp_dpoly4(e, x[i]);
            if (df != 0.0) x[i] -= pnp_poly4(e, x[i]) / df;
        }
    }
    return mask;
}

struct PnpIntrinsics { double fx, fy, cx, cy; };

PNP_HD void pnp_bearing(const PnpIntrinsics& k, double u, double v, double (&f)[3]) {
    const double x = (u - k.cx) / k.fx, y = (v - k.cy) / k.fy;
    const double inv = 1.0 / sqrt(x * x + y * y + 1.0);
    f[0] = x * inv; f[1] = y * inv; f[2] = inv;
}

PNP_HD void pnp_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// orthonormal triad (columns x, y, z) of the triangle a, b, c: x along b - a, z along the normal
PNP_HD void pnp_triad(const double (&a)[3], const double (&b)[3], const double (&c)[3], double (&T)[9]) {
    double e1[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] }, e2[3] = { c[0] - a[0], c[1] - a[1], c[2] - a[2] }, n[3], y[3];
    const double i1 = 1.0 / sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    e1[0] *= i1; e1[1] *= i1; e1[2] *= i1;
    pnp_cross(e1, e2, n);
    const double i2 = 1.0 / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    n[0] *= i2; n[1] *= i2; n[2] *= i2;
    pnp_cross(n, e1, y);
#pragma unroll
    for (int r = 0; r < 3; ++r) { T[3 * r] = e1[r]; T[3 * r + 1] = y[r]; T[3 * r + 2] = n[r]; }
}

// squared pixel error and depth of world point X under pose [R|t] (row-major 3x4), fp64
PNP_HD double pnp_pixel_err2(const PnpIntrinsics& k, const double (&pose)[12], const double (&X)[3], double u, double v, double& depth) {
    const double x = pose[0] * X[0] + pose[1] * X[1] + pose[2] * X[2] + pose[3];
    const double y = pose[4] * X[0] + pose[5] * X[1] + pose[6] * X[2] + pose[7];
    const double z = pose[8] * X[0] + pose[9] * X[1] + pose[10] * X[2] + pose[11];
    depth = z;
    const double eu = k.fx * x / z + k.cx - u, ev = k.fy * y / z + k.cy - v;
    return eu * eu + ev * ev;
}

// The contract's hypothesis: P3P on correspondences 0..2 (Grunert's quartic in v = s3 / s1: the resultant of the two quadratics in
// u = s2 / s1 that the three distance equations s_i^2 + s_j^2 - 2 s_i s_j cos(ij) = d_ij^2 leave), every real root polished, the
// distances polished by Newton on the three equations, the pose from two orthonormal triads; of the solutions with positive depth at
// all four points the one with the smallest pixel error at point 3.  false = invalid (pose untouched).
PNP_HD bool pnp_hypothesis(const PnpIntrinsics& k, const double (&X)[4][3], const double (&uv)[4][2], double (&pose)[12]) {
    double f[3][3];
    #pragma unroll
    for (int i = 0; i < 3; ++i) pnp_bearing(k, uv[i][0], uv[i][1], f[i]);
    const double c12 = f[0][0] * f[1][0] + f[0][1] * f[1][1] + f[0][2] * f[1][2];
    const double c13 = f[0][0] * f[2][0] + f[0][1] * f[2][1] + f[0][2] * f[2][2];
    const double c23 = f[1][0] * f[2][0] + f[1][1] * f[2][1] + f[1][2] * f[2][2];
    double d12 = 0.0, d13 = 0.0, d23 = 0.0;
    #pragma unroll
    for (int r = 0; r < 3; ++r) {
        d12 += (X[0][r] - X[1][r]) * (X[0][r] - X[1][r]);
        d13 += (X[0][r] - X[2][r]) * (X[0][r] - X[2][r]);
        d23 += (X[1][r] - X[2][r]) * (X[1][r] - X[2][r]);
    }
    if (!(d12 > 0.0) || !(d13 > 0.0) || !(d23 > 0.0)) return false;      // two of the three points coincide (or a NaN)
    // u^2 + p1 u + p0(v) = 0 (pair 12 against 13) and u^2 + q1(v) u + q0(v) = 0 (pair 23 against 13); with w(v) = 1 - 2 c13 v + v^2:
    //   p1 = -2 c12, p0 = 1 - A w, q1 = -2 c23 v, q0 = v^2 - B w;  E = q0 - p0, F = q1 - p1, G = p1 q0 - p0 q1;  E^2 - F G = 0, u = -E / F
    const double A = d12 / d13, B = d23 / d13, D = A - B;
    const double E[3] = { D - 1.0, -2.0 * c13 * D, D + 1.0 };
    const double F[2] = { 2.0 * c12, -2.0 * c23 };
    const double G[4] = { 2.0 * c12 * B, -4.0 * c12 * c13 * B + 2.0 * c23 * (1.0 - A), -2.0 * c12 * (1.0 - B) + 4.0 * c23 * c13 * A, -2.0 * c23 * A };
    const double e[5] = { E[0] * E[0] - F[0] * G[0],
                          2.0 * E[0] * E[1] - (F[0] * G[1] + F[1] * G[0]),
                          2.0 * E[0] * E[2] + E[1] * E[1] - (F[0] * G[2] + F[1] * G[1]),
                          2.0 * E[1] * E[2] - (F[0] * G[3] + F[1] * G[2]),
                          E[2] * E[2] - F[1] * G[3] };
    if (!(fabs(e[4]) > 0.0)) return false;
    double roots[4] = { 0.0, 0.0, 0.0, 0.0 };
    const int root_mask = pnp_quartic_roots(e, roots);
    double T0[9];
    pnp_triad(X[0], X[1], X[2], T0);
    bool found = false;
    double best = 0.0;
    for (int i = 0; i < 4; ++i) {
        if (!((root_mask >> i) & 1)) continue;
        const double v = i == 0 ? roots[0] : (i == 1 ? roots[1] : (i == 2 ? roots[2] : roots[3]));
        const double Fv = F[0] + F[1] * v, wv = 1.0 + v * (v - 2.0 * c13);
        const double u = -(E[0] + v * (E[1] + v * E[2])) / Fv;
        double s1 = sqrt(d13 / wv), s2 = u * s1, s3 = v * s1;
        #pragma unroll
        for (int it = 0; it < 2; ++it) {                       // Newton on the three distance equations (Cramer)
            const double g0 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * c12 - d12;
            const double g1 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * c13 - d13;
            const double g2 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * c23 - d23;
            const double j00 = 2.0 * (s1 - s2 * c12), j01 = 2.0 * (s2 - s1 * c12);
            const double j10 = 2.0 * (s1 - s3 * c13), j12 = 2.0 * (s3 - s1 * c13);
            const double j21 = 2.0 * (s2 - s3 * c23), j22 = 2.0 * (s3 - s2 * c23);
            const double det = -j00 * j12 * j21 - j01 * j10 * j22;          // rows (j00 j01 0), (j10 0 j12), (0 j21 j22)
            const double n1 = (-g0 * j12 * j21 - j01 * (g1 * j22 - j12 * g2)) / det;
            const double n2 = (j00 * (g1 * j22 - j12 * g2) - g0 * j10 * j22) / det;
            const double n3 = (j00 * (-g1 * j21) - j01 * (j10 * g2) + g0 * j10 * j21) / det;
            if (!(fabs(det) > 0.0) || !isfinite(n1) || !isfinite(n2) || !isfinite(n3)) break;
            s1 -= n1; s2 -= n2; s3 -= n3;
        }
        const double Y0[3] = { s1 * f[0][0], s1 * f[0][1], s1 * f[0][2] };
        const double Y1[3] = { s2 * f[1][0], s2 * f[1][1], s2 * f[1][2] };
        const double Y2[3] = { s3 * f[2][0], s3 * f[2][1], s3 * f[2][2] };
        double T1[9], cand[12];
        pnp_triad(Y0, Y1, Y2, T1);
        #pragma unroll
        for (int r = 0; r < 3; ++r)
            #pragma unroll
            for (int c = 0; c < 3; ++c) cand[4 * r + c] = T1[3 * r] * T0[3 * c] + T1[3 * r + 1] * T0[3 * c + 1] + T1[3 * r + 2] * T0[3 * c + 2];
        #pragma unroll
        for (int r = 0; r < 3; ++r) {
            double acc = 0.0;                                   // t = mean(Y) - R mean(X)
            #pragma unroll
            for (int c = 0; c < 3; ++c) acc += cand[4 * r + c] * (X[0][c] + X[1][c] + X[2][c]);
            cand[4 * r + 3] = ((Y0[r] + Y1[r] + Y2[r]) - acc) / 3.0;
        }
        bool ok = true;
        #pragma unroll
        for (int j = 0; j < 12; ++j) ok = ok && isfinite(cand[j]);
        double e4 = 0.0;
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            double depth;
            const double err = pnp_pixel_err2(k, cand, X[j], uv[j][0], uv[j][1], depth);
            ok = ok && depth > 0.0;
            if (j == 3) e4 = err;
        }
        ok = ok && isfinite(e4);
        if (ok && (!found || e4 < best)) {
            found = true;
            best = e4;
            #pragma unroll
            for (int j = 0; j < 12; ++j) pose[j] = cand[j];
        }
    }
    return found;
}

}  // namespace sfmba
