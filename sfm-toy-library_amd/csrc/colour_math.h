// colour_math.h -- the rules of the seam levelling (the contract is in include/sfmba.h, "levelling the colours across seams"), as
// __host__ __device__ functions: the kernels of mesh_colour.hip, the raster of mesh_texture.hip and the serial host program
// tools/micro/colour_math_host.hip run the same code, and tests/test_colour_oracle_cpu.py holds the host program to the Python
// restatement without a GPU.  Past the fixed-point image coordinate of texture_math.h EVERYTHING HERE IS INTEGER ARITHMETIC, and
// every division is a FLOOR division.
#pragma once
#include "texture_math.h"

#include <cstdint>

namespace sfmba {

#define COLOUR_HD __host__ __device__ __forceinline__

constexpr int COLOUR_MAX_RADIUS = 2;
constexpr int COLOUR_MAX_WEIGHT = 256;
constexpr int COLOUR_MAX_PASSES = 1024;
constexpr int COLOUR_F_MAX = 65280;                        // 255 in 1/256 grey level: the largest F and the largest |g|
constexpr int COLOUR_STATS = 8;
enum { COLOUR_S_NODES = 0, COLOUR_S_BLIND, COLOUR_S_SEAM_VERTICES, COLOUR_S_SPREAD_BEFORE, COLOUR_S_SPREAD_AFTER, COLOUR_S_MAX_G, COLOUR_S_CLAMPED,
       COLOUR_S_PASSES };
constexpr unsigned long long COLOUR_NO_KEY = ~0ULL;       // the three keys of a triangle that does not contribute

// ---- nodes -------------------------------------------------------------------------------------------------------------------
COLOUR_HD unsigned long long colour_key(int vertex, int view) {
    return ((unsigned long long)(unsigned)vertex << 32) | (unsigned long long)(unsigned)view;
}
// a triangle contributes iff it has a view, no repeated index and three finite vertices
COLOUR_HD bool colour_contributes(int view, int a, int b, int c, const double* A, const double* B, const double* C) {
    return view >= 0 && a != b && a != c && b != c && tex_finite3(A) && tex_finite3(B) && tex_finite3(C);
}
// floor(num / den), den > 0
COLOUR_HD long long colour_floor_div(long long num, long long den) {
    long long f = num / den;
    if (num % den != 0 && num < 0) --f;
    return f;
}
// floor((32 sum + n) / (2 n)): the mean of n 12-bit samples in 1/256 grey level, 0..65280
COLOUR_HD int colour_mean(long long sum, int n) { return (int)((32 * sum + n) / (2 * (long long)n)); }
// The colour of the node (X, view V): false (F = 0) for a BLIND node.  sum[c] is the sum of the (2 r + 1)^2 samples of channel c.
COLOUR_HD bool colour_node(const double* k4, const TexView& V, int channels, const double* X, int r, long long* sum, int* F) {
    double q[3], u, v;
    int su, sv;
    for (int c = 0; c < 3; ++c) { sum[c] = 0; F[c] = 0; }
    if (!tex_texel_coord(k4, V, X, q, u, v, su, sv)) return false;
    const int umax = 16 * (V.w - 1), vmax = 16 * (V.h - 1);
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx) {
            int x = su + 16 * dx, y = sv + 16 * dy;
            x = x < 0 ? 0 : (x > umax ? umax : x);
            y = y < 0 ? 0 : (y > vmax ? vmax : y);
            if (channels == 3) {
                for (int c = 0; c < 3; ++c) sum[c] += tex_sample12(V, 3, c, x, y);
            } else {
                const int s = tex_sample12(V, 1, 0, x, y);
                for (int c = 0; c < 3; ++c) sum[c] += s;
            }
        }
    const int n = (2 * r + 1) * (2 * r + 1);
    for (int c = 0; c < 3; ++c) F[c] = colour_mean(sum[c], n);
    return true;
}

// ---- a pass ------------------------------------------------------------------------------------------------------------------
// One channel of one seeing node.  k, sib: the number of seeing nodes on the node's vertex, itself included, and the sum of their
// F + g.  b, B: the number of the node's links and the sum of their g.  A = sib - k F and a = k where k >= 2, else A = a = 0;
// den = w a + b, num = w A + B; g stays where den is 0 and becomes clamp(floor((2 num + den) / (2 den)), -65280, 65280) otherwise.
COLOUR_HD int colour_update(int w, int k, long long sib, int F, int b, long long B, int g, long long& num, long long& den) {
    const long long A = k >= 2 ? sib - (long long)k * F : 0, a = k >= 2 ? k : 0;
    den = (long long)w * a + b;
    num = (long long)w * A + B;
    if (den == 0) return g;
    const long long f = colour_floor_div(2 * num + den, 2 * den);
    return (int)(f < -COLOUR_F_MAX ? -COLOUR_F_MAX : (f > COLOUR_F_MAX ? COLOUR_F_MAX : f));
}

// ---- the raster --------------------------------------------------------------------------------------------------------------
// G = (wA gA + wB gB) + wC gC with the texel's own weights wB = i, wC = j, wA = S - 2 - i - j (the least is -1)
COLOUR_HD long long colour_blend(int S, int i, int j, int gA, int gB, int gC) {
    return ((long long)(S - 2 - i - j) * gA + (long long)i * gB) + (long long)j * gC;
}
// floor((16 (S - 2) s12 + G + 128 (S - 2)) / (256 (S - 2))) clamped to 0..255; clamped is set where the clamp changed the value.
// With G = 0 this is (s12 + 8) >> 4.
COLOUR_HD unsigned char colour_texel(int S, int s12, long long G, bool& clamped) {
    const long long d = S - 2;
    const long long f = colour_floor_div(16 * d * s12 + G + 128 * d, 256 * d);
    if (f < 0) { clamped = true; return 0; }
    if (f > 255) { clamped = true; return 255; }
    return (unsigned char)f;
}

}  // namespace sfmba
