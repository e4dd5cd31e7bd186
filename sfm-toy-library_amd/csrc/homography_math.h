// homography_math.h -- the per-lane arithmetic of sfmba_homography_ransac (homography_ransac.hip): the four-point homography in
// closed form and THE inlier decision.  The sampler is the one of ransac_common.h.  Plain C++ apart from the qualifiers, so a host
// build can exercise it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "ransac_common.h"

namespace sfmba {

#define HOM_HD __host__ __device__ __forceinline__

constexpr double HOM_MIN_DET = 1e-3;         // |triple determinant| of normalised points at or below this: three of the four nearly collinear

// det[a b c] of the homogeneous points (x, y, 1): twice the signed area of the triangle
HOM_HD double hom_det3(double ax, double ay, double bx, double by, double cx, double cy) {
    return (bx - ax) * (cy - ay) - (cx - ax) * (by - ay);
}

// Four points -> mean c, scale s = the mean of |coordinate - c| over the eight numbers, and the normalised points (p - c) / s in
// place.  false when s is not > 0 (all four coincide, or a non-finite coordinate).
HOM_HD bool hom_normalise(double& x0, double& y0, double& x1, double& y1, double& x2, double& y2, double& x3, double& y3, double& cx, double& cy,
                          double& s) {
    cx = 0.25 * (x0 + x1 + x2 + x3);
    cy = 0.25 * (y0 + y1 + y2 + y3);
    x0 -= cx; x1 -= cx; x2 -= cx; x3 -= cx;
    y0 -= cy; y1 -= cy; y2 -= cy; y3 -= cy;
    s = 0.125 * (fabs(x0) + fabs(x1) + fabs(x2) + fabs(x3) + fabs(y0) + fabs(y1) + fabs(y2) + fabs(y3));
    if (!(s > 0.0)) return false;
    const double inv = 1.0 / s;
    x0 *= inv; x1 *= inv; x2 *= inv; x3 *= inv;
    y0 *= inv; y1 *= inv; y2 *= inv; y3 *= inv;
    return true;
}

// The contract's hypothesis.  l / r = the four correspondences x -> x' as (x, y) pairs; H row-major.  With a_i / b_i the
// normalised homogeneous points of the two sides, a_3 = sum_i lambda_i a_i and b_3 = sum_i mu_i b_i over i = 0..2 (Cramer: the
// ratios of the triple determinants dl_k, dr_k that the validity test needs anyway), and H a_i ~ b_i for all four gives
//   Hn = [b_0 b_1 b_2] diag(mu_i / lambda_i) adj([a_0 a_1 a_2]),     mu_i / lambda_i ~ dr_i / dl_i,
// with Hn a_i = dl_3 (dr_i / dl_i) b_i for every i = 0..3: the four products dl_k dr_k of one sign <=> one sign of w at the four
// points.  H = Tr^-1 Hn Tl, scaled by 1 / Hn[2][2] = 1 / (third row of H applied to (c_left, 1)); the mean of the a_i is (0, 0, 1),
// so Hn[2][2] is the mean of the four w and cannot vanish.  No pivoting, no indexed array: registers only.
// false = invalid (H untouched).
HOM_HD bool hom_hypothesis(const double (&l)[8], const double (&r)[8], double (&H)[9]) {
    double ax0 = l[0], ay0 = l[1], ax1 = l[2], ay1 = l[3], ax2 = l[4], ay2 = l[5], ax3 = l[6], ay3 = l[7];
    double bx0 = r[0], by0 = r[1], bx1 = r[2], by1 = r[3], bx2 = r[4], by2 = r[5], bx3 = r[6], by3 = r[7];
    double clx, cly, sl, crx, cry, sr;
    if (!hom_normalise(ax0, ay0, ax1, ay1, ax2, ay2, ax3, ay3, clx, cly, sl)) return false;
    if (!hom_normalise(bx0, by0, bx1, by1, bx2, by2, bx3, by3, crx, cry, sr)) return false;
    // triple k omits point k and keeps ascending order
    const double dl0 = hom_det3(ax1, ay1, ax2, ay2, ax3, ay3), dl1 = hom_det3(ax0, ay0, ax2, ay2, ax3, ay3);
    const double dl2 = hom_det3(ax0, ay0, ax1, ay1, ax3, ay3), dl3 = hom_det3(ax0, ay0, ax1, ay1, ax2, ay2);
    const double dr0 = hom_det3(bx1, by1, bx2, by2, bx3, by3), dr1 = hom_det3(bx0, by0, bx2, by2, bx3, by3);
    const double dr2 = hom_det3(bx0, by0, bx1, by1, bx3, by3), dr3 = hom_det3(bx0, by0, bx1, by1, bx2, by2);
    if (!(fabs(dl0) > HOM_MIN_DET) || !(fabs(dl1) > HOM_MIN_DET) || !(fabs(dl2) > HOM_MIN_DET) || !(fabs(dl3) > HOM_MIN_DET)) return false;
    if (!(fabs(dr0) > HOM_MIN_DET) || !(fabs(dr1) > HOM_MIN_DET) || !(fabs(dr2) > HOM_MIN_DET) || !(fabs(dr3) > HOM_MIN_DET)) return false;
    const bool pos = dl0 * dr0 > 0.0;
    if ((dl1 * dr1 > 0.0) != pos || (dl2 * dr2 > 0.0) != pos || (dl3 * dr3 > 0.0) != pos) return false;
    const double s0 = dr0 / dl0, s1 = dr1 / dl1, s2 = dr2 / dl2;
    // rows of adj([a_0 a_1 a_2]): a_1 x a_2, a_2 x a_0, a_0 x a_1, each scaled by its s_i
    const double r00 = s0 * (ay1 - ay2), r01 = s0 * (ax2 - ax1), r02 = s0 * (ax1 * ay2 - ax2 * ay1);
    const double r10 = s1 * (ay2 - ay0), r11 = s1 * (ax0 - ax2), r12 = s1 * (ax2 * ay0 - ax0 * ay2);
    const double r20 = s2 * (ay0 - ay1), r21 = s2 * (ax1 - ax0), r22 = s2 * (ax0 * ay1 - ax1 * ay0);
    const double n22 = r02 + r12 + r22;
    if (!(fabs(n22) > 0.0) || !isfinite(n22)) return false;                 // unreachable for valid determinants: n22 = the mean of the four w
    const double inv = 1.0 / n22;
    const double n00 = (bx0 * r00 + bx1 * r10 + bx2 * r20) * inv, n01 = (bx0 * r01 + bx1 * r11 + bx2 * r21) * inv, n02 = (bx0 * r02 + bx1 * r12 + bx2 * r22) * inv;
    const double n10 = (by0 * r00 + by1 * r10 + by2 * r20) * inv, n11 = (by0 * r01 + by1 * r11 + by2 * r21) * inv, n12 = (by0 * r02 + by1 * r12 + by2 * r22) * inv;
    const double n20 = (r00 + r10 + r20) * inv, n21 = (r01 + r11 + r21) * inv;
    // Tr^-1 Hn: rows 0, 1 <- sr row + c_right row 2 (n22 = 1 now); then Tl on the right: columns 0, 1 / sl, column 2 -= them at c_left
    const double isl = 1.0 / sl;
    const double m00 = (sr * n00 + crx * n20) * isl, m01 = (sr * n01 + crx * n21) * isl, m02 = sr * n02 + crx;
    const double m10 = (sr * n10 + cry * n20) * isl, m11 = (sr * n11 + cry * n21) * isl, m12 = sr * n12 + cry;
    const double m20 = n20 * isl, m21 = n21 * isl;
    H[0] = m00; H[1] = m01; H[2] = m02 - (m00 * clx + m01 * cly);
    H[3] = m10; H[4] = m11; H[5] = m12 - (m10 * clx + m11 * cly);
    H[6] = m20; H[7] = m21; H[8] = 1.0 - (m20 * clx + m21 * cly);
    return true;
}

// THE inlier decision, for the count (k_hom_score) and for the mask (k_hom_select) alike.  h = H rounded to fp32, (x, y) -> (xr, yr)
// one correspondence.  Division-free: with (X, Y, W) = h (x, y, 1) the transfer error is |(X, Y) / W - (xr, yr)|, so the test is
// W > 0 and |(X, Y) - W (xr, yr)|^2 <= thr^2 W^2.  Every operation is spelled out (no contraction is left to the compiler), so both
// kernels take the same decision for the same operands.
HOM_HD bool hom_inlier(const float (&h)[9], float x, float y, float xr, float yr, float thr2) {
    const float X = fmaf(h[0], x, fmaf(h[1], y, h[2]));
    const float Y = fmaf(h[3], x, fmaf(h[4], y, h[5]));
    const float W = fmaf(h[6], x, fmaf(h[7], y, h[8]));
    const float ex = fmaf(-xr, W, X), ey = fmaf(-yr, W, Y);
    const float e2 = fmaf(ex, ex, ey * ey);
    const float lim = (thr2 * W) * W;
    return W > 0.0f && e2 <= lim;
}

}  // namespace sfmba
