// flow_math.h -- the arithmetic of sfmba_flow_track and sfmba_flow_match (the contract is in include/sfmba.h), as
// __host__ __device__ functions: the kernels of flow_track.hip and the serial host program tools/micro/flow_math_host.hip run the
// same code, and tests/test_flow_oracle_cpu.py holds the host program to the numpy restatement bit for bit without a GPU.
// Samples, the template, the gradients and the five window sums are exact integers; the few fp64 operations of a level are rounded
// one by one: hipcc contracts a multiply and an add into an fma by default, so every function with a double product that is followed
// by a sum switches the contraction off for its own body.
#pragma once
#include "depth_math.h"

#include <cmath>
#include <cstdint>

namespace sfmba {

#define FLOW_HD __host__ __device__ __forceinline__

constexpr int FLOW_MAX_LEVELS = 8;
constexpr int FLOW_MAX_RADIUS = 10;
constexpr int FLOW_MAX_ITERS = 64;
constexpr int FLOW_MAX_SIDE = 2 * FLOW_MAX_RADIUS + 3;                 // the template carries a ring of one sample for the differences
constexpr int FLOW_MAX_WINDOW = (2 * FLOW_MAX_RADIUS + 1) * (2 * FLOW_MAX_RADIUS + 1);
constexpr int FLOW_CENTRE_LIMIT = 1 << 28;                             // a centre saturates here: far outside every image, far inside int32

FLOW_HD int flow_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- pyramid -----------------------------------------------------------------------------------------------------------------
FLOW_HD int flow_half(int n) { return (n + 1) >> 1; }
// pixel (x, y) of the level above `img` (w x h): the 5 x 5 binomial of the pixels around (2x, 2y), coordinates clamped to the image
FLOW_HD int flow_pyr_down(const unsigned char* img, int w, int h, int x, int y) {
    const int k[5] = { 1, 4, 6, 4, 1 };
    int s = 0;
    for (int j = 0; j < 5; ++j) {
        const unsigned char* row = img + (size_t)flow_clamp(2 * y + j - 2, 0, h - 1) * (size_t)w;
        int t = 0;
        for (int i = 0; i < 5; ++i) t += k[i] * (int)row[flow_clamp(2 * x + i - 2, 0, w - 1)];
        s += k[j] * t;
    }
    return (s + 128) >> 8;
}

// ---- sampler -----------------------------------------------------------------------------------------------------------------
// depth_sample's 1/16 px bilinear rule after the coordinate has been clamped to the image: defined for every (su, sv)
FLOW_HD int flow_sample(const unsigned char* img, int w, int h, int su, int sv) {
    return depth_sample(img, w, h, flow_clamp(su, 0, 16 * (w - 1)), flow_clamp(sv, 0, 16 * (h - 1)));
}

// ---- a level -----------------------------------------------------------------------------------------------------------------
// floor(16 (x / 2^l) + 0.5), saturated at +-2^28 (a centre that far out reads the clamped edge whatever the displacement adds and
// never has status 1, so no output can tell the saturated value from the exact one)
FLOW_HD int flow_centre(float x, int level) {
#pragma clang fp contract(off)
    const double xs = (double)x / (double)(1 << level);
    const double c16 = 16.0 * xs;
    const double c = floor(c16 + 0.5);
    if (c >= (double)FLOW_CENTRE_LIMIT) return FLOW_CENTRE_LIMIT;
    if (c <= -(double)FLOW_CENTRE_LIMIT) return -FLOW_CENTRE_LIMIT;
    return (int)c;
}
// det and the TRACKABLE flag of a level from its exact sums
FLOW_HD bool flow_trackable(long long Gxx, long long Gyy, long long Gxy, float min_eig, int n, double& det) {
#pragma clang fp contract(off)
    const double xx = (double)Gxx, yy = (double)Gyy, xy = (double)Gxy;
    const double p = xx * yy, q = xy * xy;
    det = p - q;
    const double df = (double)(Gxx - Gyy);
    const double d2 = df * df, q4 = 4.0 * q;
    const double lam = ((double)(Gxx + Gyy) - sqrt(d2 + q4)) * 0.5;
    const double floor_ = ((double)min_eig * (double)n) * 1024.0;
    return det > 0.0 && lam >= floor_;
}
// one Newton step in 1/16 px, clamped to +-16 r
FLOW_HD void flow_step(long long Gxx, long long Gyy, long long Gxy, double det, long long bx, long long by, int r, int& sx, int& sy) {
#pragma clang fp contract(off)
    const double xx = (double)Gxx, yy = (double)Gyy, xy = (double)Gxy, dbx = (double)bx, dby = (double)by;
    const double a = yy * dbx, b = xy * dby, c = xx * dby, d = xy * dbx;
    const double nx = a - b, ny = c - d;
    const double nx32 = 32.0 * nx, ny32 = 32.0 * ny;
    double fx = floor(nx32 / det + 0.5), fy = floor(ny32 / det + 0.5);
    const double lim = (double)(16 * r);
    fx = fx > lim ? lim : (fx < -lim ? -lim : fx);
    fy = fy > lim ? lim : (fy < -lim ? -lim : fy);
    sx = (int)fx;
    sy = (int)fy;
}
FLOW_HD float flow_next(float x, int dq) {
#pragma clang fp contract(off)
    const double d = (double)dq / 16.0;
    return (float)((double)x + d);
}
FLOW_HD float flow_err(long long sad, int n) {
    return (float)((double)sad / (16.0 * (double)n));
}
// c + dq inside [0, 16 (n - 1)], tested unclamped
FLOW_HD bool flow_inside(int c, int dq, int n) { const int v = c + dq; return v >= 0 && v <= 16 * (n - 1); }

// ---- the tracker of one point, serially (the host program; the kernel spreads the same window over a wave) --------------------
struct FlowLevels {
    const unsigned char* px[FLOW_MAX_LEVELS];
    int w[FLOW_MAX_LEVELS], h[FLOW_MAX_LEVELS];
};
struct FlowLevelState { long long Gxx, Gyy, Gxy; int trackable, iters, dqx, dqy; };

// T must hold (2r+3)^2 values, gx and gy (2r+1)^2 each
FLOW_HD void flow_template(const unsigned char* img, int w, int h, int cx, int cy, int r, short* T) {
    const int side = 2 * r + 3;
    for (int c = 0; c < side * side; ++c) T[c] = (short)flow_sample(img, w, h, cx + 16 * (c % side - r - 1), cy + 16 * (c / side - r - 1));
}
// window pixel (i, j), i, j in 0 .. 2r, of a template of side 2r+3: its cell t and the two central differences
FLOW_HD void flow_gradient_at(const short* T, int side, int i, int j, int& t, int& gx, int& gy) {
    t = (j + 1) * side + i + 1;
    gx = (int)T[t + 1] - (int)T[t - 1];
    gy = (int)T[t + side] - (int)T[t - side];
}
FLOW_HD void flow_gradient(const short* T, int r, int c, int& t, int& gx, int& gy) {
    const int win = 2 * r + 1;
    flow_gradient_at(T, win + 2, c % win, c / win, t, gx, gy);
}
inline void flow_track_point(const FlowLevels& S, const FlowLevels& D, float x, float y, int L, int r, int max_iters, float min_eig,
                             float* next, unsigned char* status, float* err, FlowLevelState* st) {
    short T[FLOW_MAX_SIDE * FLOW_MAX_SIDE], GX[FLOW_MAX_WINDOW], GY[FLOW_MAX_WINDOW];
    const int win = 2 * r + 1, n = win * win;
    int dqx = 0, dqy = 0, cx = 0, cy = 0;
    bool ok = false;
    for (int l = L - 1; l >= 0; --l) {
        if (l < L - 1) { dqx *= 2; dqy *= 2; }
        cx = flow_centre(x, l);
        cy = flow_centre(y, l);
        flow_template(S.px[l], S.w[l], S.h[l], cx, cy, r, T);
        long long Gxx = 0, Gyy = 0, Gxy = 0;
        for (int c = 0; c < n; ++c) {
            int t, gx, gy;
            flow_gradient(T, r, c, t, gx, gy);
            GX[c] = (short)gx; GY[c] = (short)gy;
            Gxx += gx * gx; Gyy += gy * gy; Gxy += gx * gy;
        }
        double det;
        ok = flow_trackable(Gxx, Gyy, Gxy, min_eig, n, det);
        int it = 0;
        while (ok && it < max_iters) {
            long long bx = 0, by = 0;
            for (int c = 0; c < n; ++c) {
                const int t = (c / win + 1) * (win + 2) + c % win + 1;
                const int J = flow_sample(D.px[l], D.w[l], D.h[l], cx + dqx + 16 * (c % win - r), cy + dqy + 16 * (c / win - r));
                const int d = (int)T[t] - J;
                bx += d * (int)GX[c]; by += d * (int)GY[c];
            }
            int sx, sy;
            flow_step(Gxx, Gyy, Gxy, det, bx, by, r, sx, sy);
            ++it;
            if (sx == 0 && sy == 0) break;
            dqx += sx; dqy += sy;
        }
        if (st) st[l] = FlowLevelState{ Gxx, Gyy, Gxy, ok ? 1 : 0, it, dqx, dqy };
    }
    long long sad = 0;
    if (ok)
        for (int c = 0; c < n; ++c) {
            const int t = (c / win + 1) * (win + 2) + c % win + 1;
            const int J = flow_sample(D.px[0], D.w[0], D.h[0], cx + dqx + 16 * (c % win - r), cy + dqy + 16 * (c / win - r));
            const int d = (int)T[t] - J;
            sad += d < 0 ? -d : d;
        }
    next[0] = flow_next(x, dqx);
    next[1] = flow_next(y, dqy);
    *status = ok && flow_inside(cx, dqx, D.w[0]) && flow_inside(cy, dqy, D.h[0]) ? 1 : 0;
    *err = ok ? flow_err(sad, n) : 0.0f;
}

// ---- the matcher -------------------------------------------------------------------------------------------------------------
FLOW_HD double flow_dist2(float qx, float qy, float kx, float ky) {
#pragma clang fp contract(off)
    const double dx = (double)qx - (double)kx, dy = (double)qy - (double)ky;
    const double a = dx * dx, b = dy * dy;
    return a + b;
}
FLOW_HD bool flow_in_range(double s, float radius) { return s <= (double)radius * (double)radius; }
// in_range = 1: the one is the candidate; >= 2: the ratio test on correctly rounded roots
FLOW_HD bool flow_candidate(int in_range, double s_best, double s_second, double ratio) {
    if (in_range < 2) return in_range == 1;
    return sqrt(s_best) < ratio * sqrt(s_second);
}

}  // namespace sfmba
