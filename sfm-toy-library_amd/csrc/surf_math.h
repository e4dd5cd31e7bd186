// surf_math.h -- the per-sample and per-key-point arithmetic of sfmba_surf_extract (the contract is in include/sfmba.h), as
// __host__ __device__ functions: the kernels of surf_extract.hip and the serial host program tools/micro/surf_math_host.hip run
// the same code, and tests/test_surf_oracle_cpu.py holds the host program to the numpy oracle bit for bit without a GPU.
// Everything here is integer arithmetic apart from the one division of the detector (surf_hessian) and the normalisation
// (surf_desc_value: one square root, one division, one rounding to float).  No floating-point multiply is followed by an add.
#pragma once
#include "orb_math.h"

#include <cmath>
#include <cstdint>

namespace sfmba {

#define SURF_HD __host__ __device__ __forceinline__

constexpr int SURF_MAX_OCTAVES = 4;
constexpr int SURF_LAYERS = 4;                 // filter sizes per octave; the middle two are searched
constexpr int SURF_DESC_DIMS = 64;
constexpr int SURF_ORI_SIDE = 11;              // orientation samples: i, j in -5..5 with i^2 + j^2 < 36 (109 of the 121)
constexpr int SURF_DESC_HALF = 5 * 16384;      // d of the sample offsets

// Wg(i, j) = floor(65536 exp(-(i^2 + j^2) / 12.5) + 0.5) as [|j|][|i|], 0..5: the literals of include/sfmba.h
#define SURF_WG_LITERALS { 65536, 60497, 47589, 31900, 18221, 8869,  60497, 55846, 43930, 29447, 16821, 8187, \
                           47589, 43930, 34557, 23164, 13231, 6440,  31900, 29447, 23164, 15527, 8869, 4317, \
                           18221, 16821, 13231, 8869, 5066, 2466,  8869, 8187, 6440, 4317, 2466, 1200 }
// Wd(a, b) = floor(4096 exp(-(a^2 + b^2) / 87.12) + 0.5) as [(|b| - 1) / 2][(|a| - 1) / 2], |a|, |b| = 1, 3, .. 19
#define SURF_WD_LITERALS { 4003, 3652, 3039, 2307, 1598, 1010, 582, 306, 147, 64,  3652, 3331, 2772, 2105, 1458, 921, 531, 279, 134, 59, \
                           3039, 2772, 2307, 1752, 1213, 767, 442, 232, 111, 49,  2307, 2105, 1752, 1330, 921, 582, 335, 176, 85, 37, \
                           1598, 1458, 1213, 921, 638, 403, 232, 122, 59, 26,  1010, 921, 767, 582, 403, 255, 147, 77, 37, 16, \
                           582, 531, 442, 335, 232, 147, 85, 44, 21, 9,  306, 279, 232, 176, 122, 77, 44, 23, 11, 5, \
                           147, 134, 111, 85, 59, 37, 21, 11, 5, 2,  64, 59, 49, 37, 26, 16, 9, 5, 2, 1 }

SURF_HD int surf_abs(int v) { return v < 0 ? -v : v; }
SURF_HD int surf_wg(int i, int j) { const int W[36] = SURF_WG_LITERALS; return W[surf_abs(j) * 6 + surf_abs(i)]; }
SURF_HD int surf_wd(int a, int b) { const int W[100] = SURF_WD_LITERALS; return W[((surf_abs(b) - 1) >> 1) * 10 + ((surf_abs(a) - 1) >> 1)]; }

// floor(n / d) for d > 0, also for negative n
SURF_HD long long surf_floor_div(long long n, long long d) { const long long q = n / d; return (n % d != 0 && n < 0) ? q - 1 : q; }

// ---- layers ---------------------------------------------------------------------------------------------------------------
// filter size of layer i of octave o: 9 15 21 27 / 15 27 39 51 / 27 51 75 99 / 51 99 147 195
SURF_HD int surf_layer_size(int o, int i) { return 3 * ((2 << o) * (i + 1) + 1); }
// number of grid positions (step 2^o) along an axis of n pixels
SURF_HD int surf_grid_len(int n, int o) { return (n + (1 << o) - 1) >> o; }

// ---- integral image -------------------------------------------------------------------------------------------------------
// I is (h + 1) x (w + 1), mod 2^32: I[y][x] = sum of the gray values of rows < y and columns < x.  The box is clipped by clamping
// its four coordinates into the integral image, so nothing outside it is read; every box of the contract sums to less than 2^32.
SURF_HD int surf_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
SURF_HD long long surf_box(const uint32_t* I, int w, int h, int y0, int x0, int bh, int bw) {
    const size_t ya = (size_t)surf_clamp(y0, h), yb = (size_t)surf_clamp(y0 + bh, h);
    const size_t xa = (size_t)surf_clamp(x0, w), xb = (size_t)surf_clamp(x0 + bw, w);
    const size_t st = (size_t)w + 1;
    return (long long)(uint32_t)(I[yb * st + xb] - I[ya * st + xb] - I[yb * st + xa] + I[ya * st + xa]);
}

// ---- detector -------------------------------------------------------------------------------------------------------------
// H of the contract at (y, x) for filter size L; lap receives Dxx + Dyy.  N is exact in int64 (|N| < 2^53), the division is the only
// floating-point operation.
SURF_HD double surf_hessian(const uint32_t* I, int w, int h, int y, int x, int L, long long& lap) {
    const int l = L / 3, b = (L - 1) / 2;
    const long long Dyy = surf_box(I, w, h, y - b, x - l + 1, L, 2 * l - 1) - 3 * surf_box(I, w, h, y - (l - 1) / 2, x - l + 1, l, 2 * l - 1);
    const long long Dxx = surf_box(I, w, h, y - l + 1, x - b, 2 * l - 1, L) - 3 * surf_box(I, w, h, y - l + 1, x - (l - 1) / 2, 2 * l - 1, l);
    const long long Dxy = surf_box(I, w, h, y - l, x + 1, l, l) + surf_box(I, w, h, y + 1, x - l, l, l) - surf_box(I, w, h, y - l, x - l, l, l) -
                          surf_box(I, w, h, y + 1, x + 1, l, l);
    const long long N = 100 * Dxx * Dyy - 81 * Dxy * Dxy;
    const long long L2 = (long long)L * L;
    lap = Dxx + Dyy;
    return (double)N / (double)(100 * L2 * L2);
}
// the filter of size L centred on (y, x) lies inside the image
SURF_HD bool surf_filter_inside(int w, int h, int y, int x, int L) {
    const int b = (L - 1) / 2;
    return x - b >= 0 && x + b <= w - 1 && y - b >= 0 && y + b <= h - 1;
}
// (y, x) may be a candidate of layer m (1 or 2) of octave o: none of the 27 filters involved is clipped
SURF_HD bool surf_candidate_inside(int w, int h, int y, int x, int o, int m) {
    const int s = 1 << o, bt = (surf_layer_size(o, m + 1) - 1) / 2;
    return x - s - bt >= 0 && x + s + bt <= w - 1 && y - s - bt >= 0 && y + s + bt <= h - 1;
}
// H > 0 as a sort key: ascending unsigned order of the key is DESCENDING order of H
SURF_HD uint64_t surf_response_key(double H) { union { double d; uint64_t u; } c; c.d = H; return ~c.u; }
SURF_HD double surf_key_response(uint64_t k) { union { double d; uint64_t u; } c; c.u = ~k; return c.d; }

// ---- Haar responses -------------------------------------------------------------------------------------------------------
SURF_HD long long surf_haar_x(const uint32_t* I, int w, int h, int y, int x, int p) {
    return surf_box(I, w, h, y - p, x, 2 * p, p) - surf_box(I, w, h, y - p, x - p, 2 * p, p);
}
SURF_HD long long surf_haar_y(const uint32_t* I, int w, int h, int y, int x, int p) {
    return surf_box(I, w, h, y, x - p, p, 2 * p) - surf_box(I, w, h, y - p, x - p, p, 2 * p);
}
// sigma = 0.4 l as a rational: r = round(sigma), rnd(i) = round(sigma i)
SURF_HD int surf_r(int l) { return (4 * l + 5) / 10; }
SURF_HD int surf_rnd(int l, int i) { return (int)surf_floor_div(4 * l * i + 5, 10); }

// ---- orientation ----------------------------------------------------------------------------------------------------------
// sample t in 0 .. 120 is (i, j) = (t % 11 - 5, t / 11 - 5); adds its weighted Haar responses to (mx, my) if i^2 + j^2 < 36
SURF_HD void surf_orient_sample(const uint32_t* I, int w, int h, int y, int x, int l, int t, long long& mx, long long& my) {
    const int i = t % SURF_ORI_SIDE - 5, j = t / SURF_ORI_SIDE - 5;
    if (i * i + j * j >= 36) return;
    const int r = surf_r(l), yy = y + surf_rnd(l, j), xx = x + surf_rnd(l, i);
    const long long wg = surf_wg(i, j);
    mx += wg * surf_haar_x(I, w, h, yy, xx, 2 * r);
    my += wg * surf_haar_y(I, w, h, yy, xx, 2 * r);
}

// ---- descriptor -----------------------------------------------------------------------------------------------------------
// sample (i, j), i, j in -10..9, of the window rotated into `bin`: adds w dx, w dy, w |dx|, w |dy| to v[0..3] (the four sums of the
// sample's sub-region)
SURF_HD void surf_desc_sample(const uint32_t* I, int w, int h, int y, int x, int l, int bin, int i, int j, long long (&v)[4]) {
    const int Ct[ORB_BINS] = ORB_COS_LITERALS;
    const int St[ORB_BINS] = ORB_SIN_LITERALS;
    const long long C = Ct[bin], S = St[bin], d = SURF_DESC_HALF;
    const int a = 2 * i + 1, b = 2 * j + 1, r = surf_r(l);
    const int ox = (int)surf_floor_div(2 * l * (C * a - S * b) + d, 2 * d), oy = (int)surf_floor_div(2 * l * (S * a + C * b) + d, 2 * d);
    const long long hx = surf_haar_x(I, w, h, y + oy, x + ox, r), hy = surf_haar_y(I, w, h, y + oy, x + ox, r);
    const long long dx = C * hx + S * hy, dy = -S * hx + C * hy, wd = surf_wd(a, b);
    v[0] += wd * dx;
    v[1] += wd * dy;
    v[2] += wd * (dx < 0 ? -dx : dx);
    v[3] += wd * (dy < 0 ? -dy : dy);
}
// the sub-region of sample (i, j): base index of its four sums in the 64
SURF_HD int surf_desc_base(int i, int j) { return (4 * ((j + 10) / 5) + (i + 10) / 5) * 4; }

// ---- normalisation --------------------------------------------------------------------------------------------------------
// sh = max(0, bitlength(M) - 23) for M = max |v|
SURF_HD int surf_norm_shift(long long M) {
    int bits = 0;
    while (M > 0) { ++bits; M >>= 1; }
    return bits > 23 ? bits - 23 : 0;
}
// (float)((double)t / sqrt((double)n2)); n2 = sum of t^2 < 2^52 is exact, the square root is correctly rounded
SURF_HD float surf_desc_value(long long t, long long n2) {
    if (n2 == 0) return 0.0f;
    const double root = sqrt((double)n2);
    return (float)((double)t / root);
}

}  // namespace sfmba
