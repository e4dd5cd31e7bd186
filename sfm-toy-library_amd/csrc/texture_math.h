// texture_math.h -- the arithmetic of sfmba_mesh_texture (the contract is in include/sfmba.h), as __host__ __device__ functions: the
// kernels of mesh_texture.hip and the serial host program tools/micro/texture_math_host.hip run the same code, and
// tests/test_texture_oracle_cpu.py holds the host program to the numpy restatement bit for bit without a GPU.
// The projection, depth_fix and the sample formula are depth_math.h's: there is one copy of each.  Coordinates are fp64 with every
// operation rounded on its own (every function with a double product that is followed by a sum switches the contraction off for its
// own body); everything from the fixed-point image coordinate to the texel is integer arithmetic.
#pragma once
#include "depth_math.h"

#include <cmath>
#include <cstdint>

namespace sfmba {

#define TEX_HD __host__ __device__ __forceinline__

constexpr int TEX_MIN_PATCH = 3;
constexpr int TEX_MAX_PATCH = 64;
constexpr int TEX_MAX_SIDE = 16384;            // of the atlas

// one view as the kernels see it: map is NULL for a view without a depth map, pixels the first byte of its first pixel
struct TexView {
    const double* P;             // [12], [R | t] row-major
    const float* map;            // [h][w] or NULL
    const unsigned char* pixels; // [h][w][channels]
    int w, h;
};

// ---- layout ------------------------------------------------------------------------------------------------------------------
// W = B (S + 1), H = ceil(n_blocks / B) S with n_blocks = ceil(nt / 2); no triangle: one empty block, S + 1 by S.  false when a side
// leaves 1..16384.
TEX_HD bool tex_atlas_size(long long nt, int S, int B, long long& W, long long& H) {
    const long long blocks = (nt + 1) / 2;
    if (blocks == 0) { W = S + 1; H = S; return true; }
    W = (long long)B * (S + 1);
    H = ((blocks + B - 1) / B) * S;
    return W <= TEX_MAX_SIDE && H <= TEX_MAX_SIDE;
}
// the texel (x, y) of a block, 0 <= x <= S, 0 <= y < S, belongs to half 0 as (i, j) = (x, y) when x + y <= S - 1 and to half 1,
// the block turned by 180 degrees, as (i, j) = (S - x, S - 1 - y) otherwise
TEX_HD int tex_half_of(int S, int x, int y, int& i, int& j) {
    if (x + y <= S - 1) { i = x; j = y; return 0; }
    i = S - x; j = S - 1 - y;
    return 1;
}
// the atlas pixel of the texel (i, j) of triangle t's own frame
TEX_HD void tex_atlas_pixel(long long t, int S, int B, int i, int j, long long& X, long long& Y) {
    const long long b = t >> 1, ox = (b % B) * (S + 1), oy = (b / B) * S;
    X = ox + ((t & 1) ? S - i : i);
    Y = oy + ((t & 1) ? S - 1 - j : j);
}
// the corners A, B, C sit on the texel centres (0, 0), (S - 2, 0), (0, S - 2) of the frame: uv[corner][0..1] = integer + 0.5
TEX_HD void tex_corner_uv(long long t, int S, int B, float* uv) {
    const int ci[3] = { 0, S - 2, 0 }, cj[3] = { 0, 0, S - 2 };
    for (int c = 0; c < 3; ++c) {
        long long X, Y;
        tex_atlas_pixel(t, S, B, ci[c], cj[c], X, Y);
        uv[2 * c] = (float)((double)X + 0.5);
        uv[2 * c + 1] = (float)((double)Y + 0.5);
    }
}

// ---- view choice -------------------------------------------------------------------------------------------------------------
// a vertex in a view: q = R X + t and (u, v) by depth_math.h.  It passes iff q_2 > 0, 0 <= u <= w - 1, 0 <= v <= h - 1 (a NaN fails)
// and, where the view has a map, zs = map[py][px] > 0 and q_2 - zs <= occl_tol at the pixel depth_reproject rounds to.
TEX_HD bool tex_vertex(const double* k4, const TexView& V, const double* X, double occl_tol, double* q, double& u, double& v, int& su, int& sv) {
    depth_camera_point(V.P, X, q);
    u = v = 0.0;
    su = sv = 0;
    if (!(q[2] > 0.0)) return false;
    depth_image_point(k4, q, u, v);
    if (!(u >= 0.0 && u <= (double)(V.w - 1) && v >= 0.0 && v <= (double)(V.h - 1))) return false;
    su = depth_fix(u);
    sv = depth_fix(v);
    if (V.map) {
        const int px = (int)floor(u + 0.5), py = (int)floor(v + 0.5);
        const double zs = (double)V.map[(size_t)py * (size_t)V.w + (size_t)px];
        if (!(zs > 0.0 && (q[2] - zs) <= occl_tol)) return false;
    }
    return true;
}
// the doubled signed image area in (1/16 px)^2: negative for a triangle that faces the camera (image y runs down)
TEX_HD long long tex_area2(const int* su, const int* sv) {
    return (long long)(su[1] - su[0]) * (long long)(sv[2] - sv[0]) - (long long)(sv[1] - sv[0]) * (long long)(su[2] - su[0]);
}
TEX_HD bool tex_eligible(bool candidate, long long a2, long long min_area) { return candidate && -a2 > 0 && -a2 >= min_area; }
// the triangle's candidate flag and a2 in one view
TEX_HD bool tex_candidate(const double* k4, const TexView& V, const double* A, const double* B, const double* C, double occl_tol, long long& a2) {
    const double* X[3] = { A, B, C };
    int su[3], sv[3];
    bool all = true;
    for (int c = 0; c < 3; ++c) {
        double q[3], u, v;
        all = tex_vertex(k4, V, X[c], occl_tol, q, u, v, su[c], sv[c]) && all;
    }
    a2 = all ? tex_area2(su, sv) : 0;
    return all;
}
// (x - x is 0 for a finite x and a NaN otherwise)
TEX_HD bool tex_finite3(const double* X) { return X[0] - X[0] == 0.0 && X[1] - X[1] == 0.0 && X[2] - X[2] == 0.0; }

// ---- texels ------------------------------------------------------------------------------------------------------------------
// X_a = ((wA A_a + wB B_a) + wC C_a) / (S - 2) with wB = i, wC = j, wA = S - 2 - i - j
TEX_HD void tex_point(int S, int i, int j, const double* A, const double* B, const double* C, double* X) {
#pragma clang fp contract(off)
    const double wA = (double)(S - 2 - i - j), wB = (double)i, wC = (double)j, den = (double)(S - 2);
    for (int a = 0; a < 3; ++a) {
        const double pa = wA * A[a], pb = wB * B[a], pc = wC * C[a];
        X[a] = ((pa + pb) + pc) / den;
    }
}
// false: the texel takes the fallback.  Otherwise (su, sv) of the projection, clamped into the image.
TEX_HD bool tex_texel_coord(const double* k4, const TexView& V, const double* X, double* q, double& u, double& v, int& su, int& sv) {
    depth_camera_point(V.P, X, q);
    u = v = 0.0;
    su = sv = 0;
    if (!(q[2] > 0.0)) return false;
    depth_image_point(k4, q, u, v);
    if (u != u || v != v) return false;
    const double uc = u < 0.0 ? 0.0 : (u > (double)(V.w - 1) ? (double)(V.w - 1) : u);
    const double vc = v < 0.0 ? 0.0 : (v > (double)(V.h - 1) ? (double)(V.h - 1) : v);
    su = depth_fix(uc);
    sv = depth_fix(vc);
    return true;
}
// channel ch of the texel: (s12 + 8) >> 4 of depth_math.h's sample; a gray image gives g, g, g
TEX_HD int tex_sample12(const TexView& V, int channels, int ch, int su, int sv) {
    return depth_sample_channel(V.pixels + (channels == 3 ? ch : 0), V.w, V.h, su, sv, channels);
}
TEX_HD unsigned char tex_texel(int s12) { return (unsigned char)((s12 + 8) >> 4); }
// floor((2 (wA cA + wB cB + wC cC) + (S - 2)) / (2 (S - 2))), clamped to 0..255: a floor division, the sum may be negative
TEX_HD unsigned char tex_fallback(int S, int i, int j, int cA, int cB, int cC) {
    const int num = 2 * ((S - 2 - i - j) * cA + i * cB + j * cC) + (S - 2), den = 2 * (S - 2);
    int f = num / den;
    if (num % den != 0 && num < 0) --f;
    return (unsigned char)(f < 0 ? 0 : (f > 255 ? 255 : f));
}

}  // namespace sfmba
