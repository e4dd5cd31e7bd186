// cloud_math.h -- the per-element arithmetic of sfmba_depth_normals and sfmba_cloud_merge (the contract is in include/sfmba.h), as
// __host__ __device__ functions: the kernels of cloud_merge.hip and the serial host program tools/micro/cloud_math_host.hip run the
// same code, and tests/test_cloud_oracle_cpu.py holds the host program to the Python restatement bit for bit without a GPU.
// Every fp64 operation is rounded on its own: hipcc contracts a multiply and an add into an fma by default, so every function with
// a double product that is followed by a sum switches the contraction off for its own body.  Everything a voxel sums is an integer.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace sfmba {

#define CLOUD_HD __host__ __device__ __forceinline__

constexpr int CLOUD_SUB_BITS = 10;                         // 1024 position quanta per voxel edge
constexpr long long CLOUD_Q_LIMIT = 1ll << 30;             // q in [-2^30, 2^30)
constexpr int CLOUD_INDEX_BITS = 21;                       // i + 2^20 in [0, 2^21)
constexpr long long CLOUD_INDEX_BIAS = 1ll << 20;
constexpr long long CLOUD_NORMAL_LIMIT = 1ll << 20;        // normal quanta are clamped to [-2^20, 2^20]
constexpr unsigned long long CLOUD_KEY_SKIPPED = ~0ull;    // above every valid key (those stay below 2^63)

// ---- merge: quantise ---------------------------------------------------------------------------------------------------------
// q = floor(((double)x / (double)voxel) * 1024 + 0.5); false (the point is SKIPPED) unless x is finite and -2^30 <= q < 2^30,
// tested in double: an infinite or NaN quotient fails
CLOUD_HD bool cloud_quantise(float x, double voxel, long long& q) {
#pragma clang fp contract(off)
    const double t = (double)x / voxel;
    double r = t * 1024.0;
    r = r + 0.5;
    r = floor(r);
    q = 0;
    if (!(std::isfinite(x) && r >= -(double)CLOUD_Q_LIMIT && r < (double)CLOUD_Q_LIMIT)) return false;
    q = (long long)r;
    return true;
}
// the three q of a point and its key; CLOUD_KEY_SKIPPED if any axis is skipped
CLOUD_HD unsigned long long cloud_key(const float* xyz, double voxel, long long* q) {
    bool ok = true;
    for (int a = 0; a < 3; ++a) ok = cloud_quantise(xyz[a], voxel, q[a]) && ok;
    if (!ok) return CLOUD_KEY_SKIPPED;
    unsigned long long key = 0;
    for (int a = 0; a < 3; ++a) key = (key << CLOUD_INDEX_BITS) | (unsigned long long)((q[a] >> CLOUD_SUB_BITS) + CLOUD_INDEX_BIAS);
    return key;
}
// m = floor((double)n * 16384 + 0.5) clamped to [-2^20, 2^20]; a NaN gives 0
CLOUD_HD long long cloud_normal_quantum(float n) {
#pragma clang fp contract(off)
    double r = (double)n * 16384.0;
    r = r + 0.5;
    r = floor(r);
    if (!(r == r)) return 0;
    if (r < -(double)CLOUD_NORMAL_LIMIT) return -CLOUD_NORMAL_LIMIT;
    if (r > (double)CLOUD_NORMAL_LIMIT) return CLOUD_NORMAL_LIMIT;
    return (long long)r;
}

// ---- merge: what leaves a voxel ----------------------------------------------------------------------------------------------
CLOUD_HD float cloud_final_coord(long long Sq, int c, double voxel) {
#pragma clang fp contract(off)
    double r = (double)Sq / (double)c;
    r = r / 1024.0;
    r = r * voxel;
    return (float)r;
}
CLOUD_HD unsigned char cloud_final_colour(long long S, int c) { return (unsigned char)((2 * S + c) / (2 * (long long)c)); }
CLOUD_HD void cloud_final_normal(const long long* Sm, float* out) {
#pragma clang fp contract(off)
    const double a = (double)Sm[0], b = (double)Sm[1], c = (double)Sm[2];
    double s = a * a;
    s = s + b * b;
    s = s + c * c;
    const double L = sqrt(s);
    if (L == 0.0) { out[0] = out[1] = out[2] = 0.0f; return; }
    out[0] = (float)(a / L); out[1] = (float)(b / L); out[2] = (float)(c / L);
}

// ---- a normal per depth pixel ------------------------------------------------------------------------------------------------
// p = (z xn, z yn, z) with xn = ((double)u - cx) / fx, yn = ((double)v - cy) / fy; k4 = fx, fy, cx, cy
CLOUD_HD void cloud_cam_point(const double* k4, int u, int v, double z, double* p) {
#pragma clang fp contract(off)
    const double xn = ((double)u - k4[2]) / k4[0], yn = ((double)v - k4[3]) / k4[1];
    p[0] = z * xn; p[1] = z * yn; p[2] = z;
}
// a neighbour of depth zn is usable beside z0 iff zn > 0 and |zn - z0| <= max_rel_step z0
CLOUD_HD bool cloud_usable(double zn, double z0, double max_rel_step) {
#pragma clang fp contract(off)
    return zn > 0.0 && fabs(zn - z0) <= max_rel_step * z0;
}
// the difference along one axis: plus - minus, plus - centre, centre - minus; false if neither neighbour is usable
CLOUD_HD bool cloud_axis_diff(bool has_minus, bool has_plus, const double* pm, const double* p0, const double* pp, double* d) {
    if (!has_minus && !has_plus) return false;
    const double* hi = has_plus ? pp : p0;
    const double* lo = has_minus ? pm : p0;
    for (int j = 0; j < 3; ++j) d[j] = hi[j] - lo[j];
    return true;
}
// c = dv x du turned towards the camera, its length, n_cam = c / len and the world normal n_j = (R_0j n_0 + R_1j n_1) + R_2j n_2
// (p = [R | t] row-major 3 x 4).  mid (may be NULL) receives c [3] after the flip, len, n_cam [3].  false: no normal.
CLOUD_HD bool cloud_normal_from_diffs(const double* du, const double* dv, const double* p0, const double* p, float* n, double* mid) {
#pragma clang fp contract(off)
    double c[3];
    for (int j = 0; j < 3; ++j) {
        const int a = (j + 1) % 3, b = (j + 2) % 3;
        const double x = dv[a] * du[b], y = dv[b] * du[a];
        c[j] = x - y;
    }
    double dot = c[0] * p0[0];
    dot = dot + c[1] * p0[1];
    dot = dot + c[2] * p0[2];
    if (dot > 0.0) for (int j = 0; j < 3; ++j) c[j] = -c[j];
    double s = c[0] * c[0];
    s = s + c[1] * c[1];
    s = s + c[2] * c[2];
    const double len = sqrt(s);
    if (mid) { for (int j = 0; j < 3; ++j) mid[j] = c[j]; mid[3] = len; mid[4] = mid[5] = mid[6] = 0.0; }
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    double nc[3];
    for (int j = 0; j < 3; ++j) nc[j] = c[j] / len;
    if (mid) for (int j = 0; j < 3; ++j) mid[4 + j] = nc[j];
    for (int j = 0; j < 3; ++j) {
        double w = p[j] * nc[0];
        w = w + p[4 + j] * nc[1];
        w = w + p[8 + j] * nc[2];
        n[j] = (float)w;
    }
    return true;
}
// the normal of pixel (u, v) of a w x h depth map; false (n untouched) where the pixel has none.  mid (may be NULL) [13]: as above,
// then du [3] and dv [3]; it is filled as far as the pixel got
CLOUD_HD bool cloud_pixel_normal(const double* k4, const double* p, const float* depth, int w, int h, int u, int v, double max_rel_step, float* n,
                                 double* mid) {
    const double z0 = (double)depth[(size_t)v * w + u];
    if (!(z0 > 0.0)) return false;
    double p0[3], pe[3], pw[3], ps[3], pn[3], du[3], dv[3];
    cloud_cam_point(k4, u, v, z0, p0);
    bool he = false, hw = false, hs = false, hn = false;
    if (u + 1 < w) { const double z = (double)depth[(size_t)v * w + u + 1]; if ((he = cloud_usable(z, z0, max_rel_step))) cloud_cam_point(k4, u + 1, v, z, pe); }
    if (u >= 1)    { const double z = (double)depth[(size_t)v * w + u - 1]; if ((hw = cloud_usable(z, z0, max_rel_step))) cloud_cam_point(k4, u - 1, v, z, pw); }
    if (v + 1 < h) { const double z = (double)depth[(size_t)(v + 1) * w + u]; if ((hs = cloud_usable(z, z0, max_rel_step))) cloud_cam_point(k4, u, v + 1, z, ps); }
    if (v >= 1)    { const double z = (double)depth[(size_t)(v - 1) * w + u]; if ((hn = cloud_usable(z, z0, max_rel_step))) cloud_cam_point(k4, u, v - 1, z, pn); }
    if (!cloud_axis_diff(hw, he, pw, p0, pe, du) || !cloud_axis_diff(hn, hs, pn, p0, ps, dv)) return false;
    if (mid) for (int j = 0; j < 3; ++j) { mid[7 + j] = du[j]; mid[10 + j] = dv[j]; }
    return cloud_normal_from_diffs(du, dv, p0, p, n, mid);
}

}  // namespace sfmba
