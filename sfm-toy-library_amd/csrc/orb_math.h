// orb_math.h -- the per-pixel and per-key-point arithmetic of sfmba_orb_extract (the contract is in include/sfmba.h), as
// __host__ __device__ functions: the kernels of orb_extract.hip and the serial host program tools/micro/orb_math_host.hip run
// the same code, and tests/test_orb_oracle_cpu.py holds the host program to the numpy oracle bit for bit without a GPU.
// Everything here is integer arithmetic apart from the three doubles of the pyramid (scales, quotas, key point coordinates).
#pragma once
#include "ransac_common.h"

#include <cmath>

namespace sfmba {

#define ORB_HD __host__ __device__ __forceinline__

constexpr int ORB_EDGE = 31;            // a key point lies at least this far from every edge of its level
constexpr int ORB_MIN_SIDE = 62;        // a level this wide or high, or less, has no key points
constexpr int ORB_DISC = 15;            // orientation disc: u^2 + v^2 <= 225
constexpr int ORB_BINS = 30;            // 12 degrees each
constexpr int ORB_PAIRS = 256;
constexpr int ORB_DESC_BYTES = 32;
constexpr int ORB_MAX_LEVELS = 12;
constexpr int ORB_MAX_SIDE = 16384;

// floor(16384 cos(2 pi k / 30) + 0.5) and the same of sin: the literals of include/sfmba.h
#define ORB_COS_LITERALS { 16384, 16026, 14968, 13255, 10963, 8192, 5063, 1713, -1713, -5063, -8192, -10963, -13255, -14968, -16026, \
                           -16384, -16026, -14968, -13255, -10963, -8192, -5063, -1713, 1713, 5063, 8192, 10963, 13255, 14968, 16026 }
#define ORB_SIN_LITERALS { 0, 3406, 6664, 9630, 12176, 14189, 15582, 16294, 16294, 15582, 14189, 12176, 9630, 6664, 3406, \
                           0, -3406, -6664, -9630, -12176, -14189, -15582, -16294, -16294, -15582, -14189, -12176, -9630, -6664, -3406 }

// ---- gray -----------------------------------------------------------------------------------------------------------------
ORB_HD int orb_gray_bgr(int b, int g, int r) { return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14; }

// ---- pyramid --------------------------------------------------------------------------------------------------------------
// Source indices i0, i1 and the 11-bit weight f of destination index d, for source length n and destination length m <= n.
ORB_HD void orb_resample_axis(int d, int n, int m, int& i0, int& i1, int& f) {
    const int num = (2 * d + 1) * n - m, den = 2 * m;            // num >= 0 and (2 d + 1) n < 2^30 for n <= 16384
    i0 = num / den;
    f = ((num - i0 * den) * 2048 + den / 2) / den;
    i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
}

ORB_HD int orb_resample_value(int i00, int i01, int i10, int i11, int fx, int fy) {
    return ((i00 * (2048 - fx) + i01 * fx) * (2048 - fy) + (i10 * (2048 - fx) + i11 * fx) * fy + (1 << 21)) >> 22;    // < 2^31
}

ORB_HD int orb_resample_pixel(const unsigned char* src, int sw, int sh, int dw, int dh, int x, int y) {
    int x0, x1, fx, y0, y1, fy;
    orb_resample_axis(x, sw, dw, x0, x1, fx);
    orb_resample_axis(y, sh, dh, y0, y1, fy);
    const unsigned char* r0 = src + (size_t)y0 * sw;
    const unsigned char* r1 = src + (size_t)y1 * sw;
    return orb_resample_value(r0[x0], r0[x1], r1[x0], r1[x1], fx, fy);
}

// ---- FAST score -------------------------------------------------------------------------------------------------------------
// The 16-pixel circle of radius 3, clockwise from (0, -3).
ORB_HD int orb_circle_dx(int k) { const int dx[16] = { 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1 }; return dx[k]; }
ORB_HD int orb_circle_dy(int k) { const int dy[16] = { -3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3 }; return dy[k]; }

// Does a 16-bit ring mask hold 9 consecutive set bits (cyclically)?
ORB_HD bool orb_has_arc9(unsigned m) {
    unsigned r = m | (m << 16);                    // the ring twice: every cyclic arc is contiguous
    r &= r >> 1;                                   // runs of 2
    r &= r >> 2;                                   // runs of 4
    r &= r >> 4;                                   // runs of 8
    r &= (m | (m << 16)) >> 8;                     // runs of 9
    return (r & 0xffffu) != 0u;
}

// max over the 16 starts of the minimum of v over 9 consecutive ring entries (sliding minima by doubling: 64 min, 15 max)
ORB_HD int orb_arc9_maxmin(const int (&v)[16]) {
    int m2[16], m4[16], best = -256;
#pragma unroll
    for (int k = 0; k < 16; ++k) m2[k] = v[k] < v[(k + 1) & 15] ? v[k] : v[(k + 1) & 15];
#pragma unroll
    for (int k = 0; k < 16; ++k) m4[k] = m2[k] < m2[(k + 2) & 15] ? m2[k] : m2[(k + 2) & 15];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int m8 = m4[k] < m4[(k + 4) & 15] ? m4[k] : m4[(k + 4) & 15];
        const int m9 = m8 < v[(k + 8) & 15] ? m8 : v[(k + 8) & 15];
        best = m9 > best ? m9 : best;
    }
    return best;
}

// S of the contract from the centre p and the 16 circle bytes; 0 when S <= threshold.  S > threshold exactly when 9 consecutive
// circle pixels are all brighter than p + threshold or all darker than p - threshold, so the two ring masks decide without
// divergence whether the exact value is needed at all.
ORB_HD int orb_fast_score(int p, const int (&c)[16], int threshold) {
    unsigned brighter = 0u, darker = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        brighter |= (c[k] - p > threshold ? 1u : 0u) << k;
        darker |= (p - c[k] > threshold ? 1u : 0u) << k;
    }
    const bool up = orb_has_arc9(brighter), down = orb_has_arc9(darker);
    if (!up && !down) return 0;
    int d[16];
    int s = 0;
    if (up) {
#pragma unroll
        for (int k = 0; k < 16; ++k) d[k] = c[k] - p;
        s = orb_arc9_maxmin(d);
    }
    if (down) {
#pragma unroll
        for (int k = 0; k < 16; ++k) d[k] = p - c[k];
        const int t = orb_arc9_maxmin(d);
        s = t > s ? t : s;
    }
    return s;                                      // > threshold by construction
}

// ---- Harris response --------------------------------------------------------------------------------------------------------
// R = 25 (a b - c^2) - (a + b)^2 from the 9 x 9 window centred on the candidate (w[(v + 4) * 9 + (u + 4)] = I(x + u, y + v)):
// 3 x 3 Sobel derivatives over the 7 x 7 block.  |Ix| <= 1020, so a, b <= 5.1e7 and every term stays below 2^63.
ORB_HD long long orb_harris_response(const int (&w)[81]) {
    long long a = 0, b = 0, c = 0;
#pragma unroll
    for (int v = 1; v < 8; ++v)
#pragma unroll
        for (int u = 1; u < 8; ++u) {
            const int ix = (w[(v - 1) * 9 + u + 1] + 2 * w[v * 9 + u + 1] + w[(v + 1) * 9 + u + 1]) -
                           (w[(v - 1) * 9 + u - 1] + 2 * w[v * 9 + u - 1] + w[(v + 1) * 9 + u - 1]);
            const int iy = (w[(v + 1) * 9 + u - 1] + 2 * w[(v + 1) * 9 + u] + w[(v + 1) * 9 + u + 1]) -
                           (w[(v - 1) * 9 + u - 1] + 2 * w[(v - 1) * 9 + u] + w[(v - 1) * 9 + u + 1]);
            a += ix * ix; b += iy * iy; c += ix * iy;
        }
    return 25 * (a * b - c * c) - (a + b) * (a + b);
}

// R as a sort key: ascending unsigned order of the key is DESCENDING order of R.
ORB_HD uint64_t orb_response_key(long long R) { return ~((uint64_t)R ^ 0x8000000000000000ull); }
ORB_HD long long orb_key_response(uint64_t k) { return (long long)(~k ^ 0x8000000000000000ull); }

// ---- orientation ------------------------------------------------------------------------------------------------------------
// The lowest bin k that maximises m10 C_k + m01 S_k.
ORB_HD int orb_bin(long long m10, long long m01) {
    const int C[ORB_BINS] = ORB_COS_LITERALS;
    const int S[ORB_BINS] = ORB_SIN_LITERALS;
    int best = 0;
    long long bv = m10 * C[0] + m01 * S[0];
    for (int k = 1; k < ORB_BINS; ++k) {
        const long long v = m10 * C[k] + m01 * S[k];
        if (v > bv) { bv = v; best = k; }
    }
    return best;
}

// ---- smoothing ----------------------------------------------------------------------------------------------------------------
ORB_HD int orb_smooth_tap7(int a, int b, int c, int d, int e, int f, int g) { return 18 * (a + g) + 34 * (b + f) + 49 * (c + e) + 54 * d; }
ORB_HD int orb_smooth_round(int v) { return (v + 32768) >> 16; }

// the smoothed pixel (x, y) of a level, at least 3 from every edge: horizontal pass, vertical pass, rounding
ORB_HD int orb_smooth_pixel(const unsigned char* I, int w, int x, int y) {
    int r[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const unsigned char* p = I + (size_t)(y + j - 3) * w + x;
        r[j] = orb_smooth_tap7(p[-3], p[-2], p[-1], p[0], p[1], p[2], p[3]);
    }
    return orb_smooth_round(orb_smooth_tap7(r[0], r[1], r[2], r[3], r[4], r[5], r[6]));
}

// ---- pattern and descriptor -----------------------------------------------------------------------------------------------------
ORB_HD void orb_rotate(int k, int x, int y, int& xr, int& yr) {
    const int C[ORB_BINS] = ORB_COS_LITERALS;
    const int S[ORB_BINS] = ORB_SIN_LITERALS;
    xr = (C[k] * x - S[k] * y + 8192) >> 14;       // arithmetic shift
    yr = (S[k] * x + C[k] * y + 8192) >> 14;
}

ORB_HD int orb_desc_bit(int b0, int b1) { return b0 < b1 ? 1 : 0; }

// table [30][256][4] int8 (x0' y0' x1' y1'): the first 256 accepted pairs of the splitmix64 stream, rotated into every bin
inline void orb_build_pattern(signed char* table) {
    uint64_t k = 0;
    int n = 0;
    while (n < ORB_PAIRS) {
        int c[4];
        for (int j = 0; j < 4; ++j) {
            c[j] = (int)(pnp_mix(k) % 13u) + (int)(pnp_mix(k + 1) % 13u) - 12;
            k += 2;
        }
        if (c[0] * c[0] + c[1] * c[1] > 169 || c[2] * c[2] + c[3] * c[3] > 169 || (c[0] == c[2] && c[1] == c[3])) continue;
        for (int b = 0; b < ORB_BINS; ++b) {
            int x0, y0, x1, y1;
            orb_rotate(b, c[0], c[1], x0, y0);
            orb_rotate(b, c[2], c[3], x1, y1);
            signed char* t = table + ((size_t)b * ORB_PAIRS + (size_t)n) * 4;
            t[0] = (signed char)x0; t[1] = (signed char)y0; t[2] = (signed char)x1; t[3] = (signed char)y1;
        }
        ++n;
    }
}

// ---- pyramid geometry and quotas (host) -------------------------------------------------------------------------------------
// scale[l], and the level sizes of a w x h image; returns the number of levels in front of the first one of size 0
inline int orb_level_sizes(int w, int h, float scale_factor, int n_levels, double* scale, int* lw, int* lh) {
    double s = 1.0;
    int n = n_levels;
    for (int l = 0; l < n_levels; ++l) {
        scale[l] = s;
        lw[l] = (int)std::floor((double)w / s + 0.5);
        lh[l] = (int)std::floor((double)h / s + 0.5);
        if ((lw[l] <= 0 || lh[l] <= 0) && l < n) n = l;
        s = s * (double)scale_factor;
    }
    return n;
}

inline void orb_quotas(int n_features, float scale_factor, int n_levels, int* q) {
    const double f = 1.0 / (double)scale_factor;
    double fn = 1.0;
    for (int l = 0; l < n_levels; ++l) fn = fn * f;
    double want = (double)n_features * (1.0 - f) / (1.0 - fn);
    long long sum = 0;
    for (int l = 0; l + 1 < n_levels; ++l) {
        q[l] = (int)std::nearbyint(want);          // round-half-even (the default rounding mode)
        sum += q[l];
        want = want * f;
    }
    q[n_levels - 1] = (int)((long long)n_features - sum > 0 ? (long long)n_features - sum : 0);
}

}  // namespace sfmba
