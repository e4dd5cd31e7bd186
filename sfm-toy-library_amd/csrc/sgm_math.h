// sgm_math.h -- the arithmetic of sfmba_depth_cost_volume, sfmba_sgm_aggregate and sfmba_depth_sweep_sgm (the contract is in
// include/sfmba.h), as __host__ __device__ functions: the kernels of depth_sgm.hip / depth_sweep.hip and the serial host program
// tools/micro/sgm_math_host.hip run the same code, and tests/test_sgm_oracle_cpu.py holds the host program to the numpy restatement
// bit for bit without a GPU.  Everything between the quantised cost and the selection is integer arithmetic; the three fp64
// expressions (quantise, delta, score) have every operation rounded on its own, so the contraction is switched off for their bodies.
//
// Bounds.  A volume entry is 0..254 or the sentinel 255; read with invalid_cost 0..254 it is c in 0..254.  Along a path
// L = c + min(...) - m: every term of the minimum is >= m (m is the minimum of the previous pixel's L and the penalties are >= 0) and
// the term m + p2 is always present, so 0 <= min(...) - m <= p2 and 0 <= L <= 254 + p2 <= 1277.  S is a sum of at most 8 such values:
// S <= 10216 < 2^16.  den = (S- - 2 S0) + S+ lies in -20432..20432 and S- - S+ in -10216..10216: int32 holds them all.
#pragma once
#include "depth_math.h"

#include <cmath>
#include <cstdint>

namespace sfmba {

constexpr int SGM_SENTINEL = 255;              // a volume entry of an invalid plane or of a pixel that does not take part
constexpr int SGM_MAX_COST = 254;
constexpr int SGM_MAX_PENALTY = 1023;
constexpr int SGM_NO_SECOND = 0xffff;          // `second` where no plane lies further than one step from k*
constexpr int SGM_FAR = 0x3fff;                // stands for a term that is left out of the minimum: above every L + penalty (2300)

// ---- the volume ----------------------------------------------------------------------------------------------------------------
// q = (int)floor((1.0 - C) * 127.0 + 0.5) of a valid plane's cost C in [-1, 1]: 0 (C = 1) .. 254 (C = -1)
DEPTH_HD int sgm_quantise(double C) {
#pragma clang fp contract(off)
    const double one_minus = 1.0 - C;
    const double scaled = one_minus * 127.0;
    return (int)floor(scaled + 0.5);
}
// what the aggregation reads of a volume entry
DEPTH_HD int sgm_cost(int q, int invalid_cost) { return q == SGM_SENTINEL ? invalid_cost : q; }

// ---- one step along a path -------------------------------------------------------------------------------------------------------
// L_r(p, d) from the previous pixel's L at d, d - 1 and d + 1 (SGM_FAR where the plane does not exist) and their minimum m
DEPTH_HD int sgm_step(int c, int prev, int prev_lo, int prev_hi, int m, int p1, int p2) {
    int best = prev;
    best = prev_lo + p1 < best ? prev_lo + p1 : best;
    best = prev_hi + p1 < best ? prev_hi + p1 : best;
    best = m + p2 < best ? m + p2 : best;
    return c + best - m;
}
// the direction r of path i (0..7) and the first pixel of line l of that direction in a w x h image; a direction has
// sgm_lines(dx, dy, w, h) lines and every pixel lies on exactly one of them
DEPTH_HD void sgm_direction(int i, int& dx, int& dy) {
    const int DX[8] = { 1, -1, 0, 0, 1, -1, 1, -1 }, DY[8] = { 0, 0, 1, -1, 1, -1, -1, 1 };
    dx = DX[i];
    dy = DY[i];
}
DEPTH_HD int sgm_lines(int dx, int dy, int w, int h) { return dy == 0 ? h : dx == 0 ? w : w + h - 1; }
DEPTH_HD void sgm_line_start(int dx, int dy, int w, int h, int l, int& x, int& y) {
    if (dy == 0) { x = dx > 0 ? 0 : w - 1; y = l; return; }
    if (dx == 0 || l < w) { x = l; y = dy > 0 ? 0 : h - 1; return; }       // the lines that enter through the top / bottom row
    x = dx > 0 ? 0 : w - 1;                                                 // ... and through the left / right column, below / above it
    y = dy > 0 ? l - w + 1 : h - 1 - (l - w + 1);
}

// ---- selection -------------------------------------------------------------------------------------------------------------------
// k* = the lowest d with the smallest S, best = S(k*), second = the smallest S over |d - k*| > 1 or SGM_NO_SECOND
DEPTH_HD void sgm_select(const uint16_t* S, int D, int& k, int& best, int& second) {
    k = 0;
    for (int d = 1; d < D; ++d)
        if (S[d] < S[k]) k = d;
    best = S[k];
    second = SGM_NO_SECOND;
    for (int d = 0; d < D; ++d)
        if ((d < k - 1 || d > k + 1) && (int)S[d] < second) second = S[d];
}
// ACCEPTED iff second is absent or 100 (second - best) >= uniqueness second (at most 100 * 10216: int32)
DEPTH_HD bool sgm_accepted(int best, int second, int uniqueness) {
    return second == SGM_NO_SECOND || 100 * (second - best) >= uniqueness * second;
}
// den = (S- - 2 S0) + S+; the offset of the parabola's vertex in plane steps where den > 0, else 0
DEPTH_HD int sgm_den(int sm, int s0, int sp) { return (sm - 2 * s0) + sp; }
DEPTH_HD double sgm_delta(int sm, int s0, int sp) {
#pragma clang fp contract(off)
    const int den = sgm_den(sm, s0, sp);
    if (den <= 0) return 0.0;
    const double half = 0.5 * (double)(sm - sp);
    return half / (double)den;
}
// the three maps of one pixel from its selection, the sums beside k* (read only where 0 < k* < D-1) and its own volume entry q at k*
DEPTH_HD void sgm_pixel(double wf, double step, int D, int k, int best, int second, int sm, int sp, int q, int uniqueness, float& depth,
                        float& score) {
#pragma clang fp contract(off)
    depth = 0.0f;
    if (sgm_accepted(best, second, uniqueness)) {
        const double delta = (k > 0 && k < D - 1) ? sgm_delta(sm, best, sp) : 0.0;
        depth = depth_value(wf, step, k, delta);
    }
    score = 0.0f;
    if (q != SGM_SENTINEL) {
        const double qs = (double)q / 127.0;
        score = (float)(1.0 - qs);
    }
}

}  // namespace sfmba
