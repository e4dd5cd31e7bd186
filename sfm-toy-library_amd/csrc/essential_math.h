// essential_math.h -- the arithmetic of sfmba_essential_ransac (essential_ransac.hip): the five-point essential matrix of one
// hypothesis (Nister's route: null space, ten cubic constraints, elimination, the degree-10 polynomial in z, its real roots by
// Sturm's sequence and bisection), THE inlier decision, and recoverPose in closed form (Horn 1990).  The sampler is the one of
// ransac_common.h.  Plain C++ apart from the qualifiers, so a host build can exercise it (tools/micro/essential_math_host.hip).
//
// Everything that is indexed at run time (pivot rows and columns, the Sturm chain) lives in a work area of ESS_WORK doubles per
// hypothesis behind a small store type: on the device a strided view of LDS (essential_ransac.hip), on the host a plain array.
// Everything else is unrolled over compile-time indices and stays in registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "ransac_common.h"

namespace sfmba {

#define ESS_HD __host__ __device__ __forceinline__

constexpr int ESS_WORK = 200;                // doubles of indexed storage per hypothesis: the 10 x 20 system is the largest tenant
constexpr double ESS_MIN_PIVOT = 1e-12;      // a pivot of the 5 x 9 epipolar system at or below this x its largest entry: rank-deficient
constexpr double ESS_MIN_PIVOT10 = 1e-13;    // the same for the 10 x 10 block of the constraint system
constexpr double ESS_MAX_DEPTH = 50.0;       // OpenCV's distanceThresh of recoverPose, with |t| = 1

// work area of one hypothesis: element i sits STRIDE doubles after element i - 1 (64 lanes interleaved in LDS, or 1 on the host)
template <int STRIDE>
struct EssStore {
    double* p;
    ESS_HD double& operator[](int i) const { return p[i * STRIDE]; }
};

// ---- polynomials in (x, y, z) on compile-time indices ----------------------------------------------------------------------
// variables 0 = x, 1 = y, 2 = z, 3 = the constant 1; a monomial of degree <= d is a sorted d-tuple of them, numbered in
// lexicographic order: 4 linear, 10 quadratic, 20 cubic.
constexpr int ess_q2(int a, int b) { return a * 4 - a * (a - 1) / 2 + (b - a); }               // a <= b
constexpr int ess_q(int a, int b) { return a <= b ? ess_q2(a, b) : ess_q2(b, a); }
constexpr int ess_c3(int a, int b, int c) {                                                     // a <= b <= c
    const int off = a == 0 ? 0 : (a == 1 ? 10 : (a == 2 ? 16 : 19));
    const int m = 4 - a, bb = b - a, cc = c - a;
    return off + bb * m - bb * (bb - 1) / 2 + (cc - bb);
}
constexpr int ess_c(int a, int b, int c) {
    const int lo = a < b ? (a < c ? a : c) : (b < c ? b : c);
    const int hi = a > b ? (a > c ? a : c) : (b > c ? b : c);
    return ess_c3(lo, a + b + c - lo - hi, hi);
}
// cubic monomial (numbering above) -> column of the constraint system, Nister's order:
//   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
constexpr int ess_col(int m) {
    constexpr int t[20] = { 0, 2, 4, 5, 3, 8, 9, 10, 11, 12, 1, 6, 7, 13, 14, 15, 16, 17, 18, 19 };
    return t[m];
}

// q += s * a * b (linear x linear)
ESS_HD void ess_mul11(double (&q)[10], const double (&a)[4], const double (&b)[4], double s) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) q[ess_q(i, j)] += s * a[i] * b[j];
}

// c += q * l (quadratic x linear)
ESS_HD void ess_mul21(double (&c)[20], const double (&q)[10], const double (&l)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) c[ess_c(i, j, k)] += q[ess_q2(i, j)] * l[k];
}

// ---- univariate polynomials in z, ascending powers, compile-time sizes --------------------------------------------------------
template <int NA, int NB, int NC>
ESS_HD void ess_pmul(double (&c)[NC], const double (&a)[NA], const double (&b)[NB], double s) {
    static_assert(NC >= NA + NB - 1, "product does not fit");
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) c[i + j] += s * a[i] * b[j];
}

template <int N>
ESS_HD double ess_horner(const double (&a)[N], double z) {
    double v = a[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 0; --i) v = fma(v, z, a[i]);
    return v;
}

// ---- step 1: the null space of the 5 x 9 epipolar system -----------------------------------------------------------------------
// xl / xr = the five normalised correspondences (x, y) / (x', y').  Row i = x'_i (x) x_i (E row-major: x'^T E x = 0).  Gauss-
// Jordan with complete pivoting in w[0 .. 44]; the four null vectors (one per free column: 1 there, minus the eliminated entries
// in the pivot columns) go to w[45 .. 80] and come back orthonormalised (modified Gram-Schmidt, in free-column order) as N[4][9].
template <class Store>
ESS_HD bool ess_null_space(const Store& w, const double (&xl)[10], const double (&xr)[10], double (&N)[4][9]) {
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const double x = xl[2 * i], y = xl[2 * i + 1], u = xr[2 * i], v = xr[2 * i + 1];
        w[9 * i + 0] = u * x; w[9 * i + 1] = u * y; w[9 * i + 2] = u;
        w[9 * i + 3] = v * x; w[9 * i + 4] = v * y; w[9 * i + 5] = v;
        w[9 * i + 6] = x;     w[9 * i + 7] = y;     w[9 * i + 8] = 1.0;
    }
    double amax = 0.0;
    for (int i = 0; i < 45; ++i) amax = fmax(amax, fabs(w[i]));
    if (!isfinite(amax)) return false;
    unsigned used = 0, pcs = 0;                       // pivot columns: a bit mask, and 4 bits per row
    for (int r = 0; r < 5; ++r) {
        double best = -1.0;
        int pi = r, pj = 0;
        for (int i = r; i < 5; ++i)
            for (int j = 0; j < 9; ++j) {
                const double a = fabs(w[9 * i + j]);
                if (!((used >> j) & 1u) && a > best) { best = a; pi = i; pj = j; }
            }
        if (!(best > ESS_MIN_PIVOT * amax)) return false;
        const double inv = 1.0 / w[9 * pi + pj];
        for (int j = 0; j < 9; ++j) {
            const double a = w[9 * pi + j], b = w[9 * r + j];
            w[9 * pi + j] = b;
            w[9 * r + j] = a * inv;
        }
        for (int i = 0; i < 5; ++i) {
            if (i == r) continue;
            const double f = w[9 * i + pj];
            for (int j = 0; j < 9; ++j) w[9 * i + j] -= f * w[9 * r + j];
        }
        used |= 1u << pj;
        pcs |= (unsigned)pj << (4 * r);
    }
    int k = 0;
    for (int f = 0; f < 9; ++f) {
        if ((used >> f) & 1u) continue;
        for (int c = 0; c < 9; ++c) w[45 + 9 * k + c] = 0.0;
        w[45 + 9 * k + f] = 1.0;
        for (int r = 0; r < 5; ++r) w[45 + 9 * k + (int)((pcs >> (4 * r)) & 15u)] = -w[9 * r + f];
        ++k;
    }
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int c = 0; c < 9; ++c) N[v][c] = w[45 + 9 * v + c];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int u = 0; u < v; ++u) {
            double d = 0.0;
#pragma unroll
            for (int c = 0; c < 9; ++c) d += N[u][c] * N[v][c];
#pragma unroll
            for (int c = 0; c < 9; ++c) N[v][c] -= d * N[u][c];
        }
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) s += N[v][c] * N[v][c];
        if (!(s > 0.0) || !isfinite(s)) return false;
        s = 1.0 / sqrt(s);
#pragma unroll
        for (int c = 0; c < 9; ++c) N[v][c] *= s;
    }
    return true;
}

// ---- step 2: the ten cubic constraints on E = x N0 + y N1 + z N2 + N3 ----------------------------------------------------------
// Row 0 = det E; rows 1 .. 9 = the entries of (E E^T - 1/2 tr(E E^T) I) E (half of 2 E E^T E - tr(E E^T) E), row-major.  Written to
// w[row * 20 + column], columns in Nister's order (ess_col).
template <class Store>
ESS_HD void ess_constraints(const Store& w, const double (&N)[4][9]) {
    double e[9][4];
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int v = 0; v < 4; ++v) e[j][v] = N[v][j];
    {   // det E along the first row
        double c[20];
#pragma unroll
        for (int m = 0; m < 20; ++m) c[m] = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            double q[10];
#pragma unroll
            for (int m = 0; m < 10; ++m) q[m] = 0.0;
            ess_mul11(q, e[3 + j1], e[6 + j2], 1.0);
            ess_mul11(q, e[3 + j2], e[6 + j1], -1.0);
            ess_mul21(c, q, e[j]);
        }
#pragma unroll
        for (int m = 0; m < 20; ++m) w[ess_col(m)] = c[m];
    }
    double L[6][10];                                  // E E^T - 1/2 tr I, the upper triangle: 00 01 02 11 12 22
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const int s = i == 0 ? j : (i == 1 ? 2 + j : 5);
#pragma unroll
            for (int m = 0; m < 10; ++m) L[s][m] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) ess_mul11(L[s], e[3 * i + k], e[3 * j + k], 1.0);
        }
#pragma unroll
    for (int m = 0; m < 10; ++m) {
        const double h = 0.5 * (L[0][m] + L[3][m] + L[5][m]);
        L[0][m] -= h; L[3][m] -= h; L[5][m] -= h;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double c[20];
#pragma unroll
            for (int m = 0; m < 20; ++m) c[m] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int a = i < k ? i : k, b = i < k ? k : i;
                ess_mul21(c, L[a == 0 ? b : (a == 1 ? 2 + b : 5)], e[3 * k + j]);
            }
#pragma unroll
            for (int m = 0; m < 20; ++m) w[20 * (1 + 3 * i + j) + ess_col(m)] = c[m];
        }
}

// ---- step 3: Gauss-Jordan on the left 10 x 10 block, partial pivoting ------------------------------------------------------------
// Afterwards rows 4 .. 9 are  x^2z, x^2, y^2z, y^2, xyz, xy  +  their right halves (columns 10 .. 19).  Rows 0 .. 3 are only pivot
// rows: nothing is eliminated from them above the diagonal.  false = singular.
template <class Store>
ESS_HD bool ess_eliminate(const Store& w) {
    double amax = 0.0;
    for (int i = 0; i < 200; ++i) amax = fmax(amax, fabs(w[i]));
    if (!isfinite(amax)) return false;
    for (int c = 0; c < 10; ++c) {
        double best = -1.0;
        int pr = c;
        for (int r = c; r < 10; ++r) {
            const double a = fabs(w[20 * r + c]);
            if (a > best) { best = a; pr = r; }
        }
        if (!(best > ESS_MIN_PIVOT10 * amax)) return false;
        const double inv = 1.0 / w[20 * pr + c];
        for (int j = c; j < 20; ++j) {
            const double a = w[20 * pr + j], b = w[20 * c + j];
            w[20 * pr + j] = b;
            w[20 * c + j] = a * inv;
        }
        for (int r = 0; r < 10; ++r) {
            if (r == c || (r < c && r < 4)) continue;
            const double f = w[20 * r + c];
            for (int j = c + 1; j < 20; ++j) w[20 * r + j] -= f * w[20 * c + j];
        }
    }
    return true;
}

// ---- step 4: the real roots of a polynomial by Sturm's sequence -----------------------------------------------------------------
// Polynomial i of the chain has degree <= 10 - i and lives in w[ess_chain(i) + k] (power k): 66 doubles, w[0 .. 65]; w[66 .. 76] is
// the scratch of the polynomial division.  That leaves w[80 ..] -- rows 4 .. 9 of the eliminated system -- alone.  degs holds 4 bits
// of degree per polynomial.
ESS_HD int ess_chain(int i) { return 11 * i - i * (i - 1) / 2; }
constexpr int ESS_CHAIN_TMP = 66;

template <class Store>
ESS_HD int ess_sign_changes(const Store& w, int n_chain, uint64_t degs, double z) {
    int changes = 0, last = 0;
    for (int i = 0; i < n_chain; ++i) {
        const int d = (int)((degs >> (4 * i)) & 15u);
        const int o = ess_chain(i);
        double v = w[o + d];
        for (int k = d - 1; k >= 0; --k) v = v * z + w[o + k];
        const int s = v > 0.0 ? 1 : (v < 0.0 ? -1 : 0);
        if (s != 0) {
            if (last != 0 && s != last) ++changes;
            last = s;
        }
    }
    return changes;
}

// sign changes at -infinity (dir = -1) or +infinity (dir = +1)
template <class Store>
ESS_HD int ess_sign_changes_inf(const Store& w, int n_chain, uint64_t degs, int dir) {
    int changes = 0, last = 0;
    for (int i = 0; i < n_chain; ++i) {
        const int d = (int)((degs >> (4 * i)) & 15u);
        const double v = w[ess_chain(i) + d];
        int s = v > 0.0 ? 1 : (v < 0.0 ? -1 : 0);
        if (dir < 0 && (d & 1)) s = -s;
        if (s != 0) {
            if (last != 0 && s != last) ++changes;
            last = s;
        }
    }
    return changes;
}

// Distinct real roots of f (ascending powers, 11 coefficients) in ascending order into roots; returns their number (<= 10), -1 on
// a non-finite coefficient.  Root k is bracketed with the sign-change count until it is alone in its interval, then bisected on the
// sign of f, then polished by two Newton steps.
template <class Store>
ESS_HD int ess_real_roots(const Store& w, const double (&f)[11], double (&roots)[10]) {
#pragma unroll
    for (int k = 0; k < 10; ++k) roots[k] = 0.0;
    double fmx = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) fmx = fmax(fmx, fabs(f[k]));
    if (!(fmx > 0.0) || !isfinite(fmx)) return -1;
    const double fs = 1.0 / fmx;
#pragma unroll
    for (int k = 0; k < 11; ++k) w[k] = f[k] * fs;
    int d0 = 10;
    while (d0 > 0 && w[d0] == 0.0) --d0;
    if (d0 < 1) return 0;
    for (int k = 1; k <= d0; ++k) w[ess_chain(1) + k - 1] = (double)k * w[k];
    uint64_t degs = (uint64_t)d0 | ((uint64_t)(d0 - 1) << 4);
    int n_chain = 2;
    while (n_chain < 11) {
        const int ia = n_chain - 2, ib = n_chain - 1, ic = n_chain;
        const int da = (int)((degs >> (4 * ia)) & 15u), db = (int)((degs >> (4 * ib)) & 15u);
        if (db == 0) break;
        const int oa = ess_chain(ia), ob = ess_chain(ib), oc = ess_chain(ic), tmp = ESS_CHAIN_TMP;
        for (int k = 0; k <= da; ++k) w[tmp + k] = w[oa + k];
        const double lead = 1.0 / w[ob + db];
        for (int k = da; k >= db; --k) {
            const double q = w[tmp + k] * lead;
            for (int j = 0; j < db; ++j) w[tmp + k - db + j] -= q * w[ob + j];
        }
        int dc = db - 1;
        while (dc >= 0 && w[tmp + dc] == 0.0) --dc;
        if (dc < 0) break;                                     // f and f' share a factor: the chain ends at their gcd
        double mx = 0.0;
        for (int k = 0; k <= dc; ++k) mx = fmax(mx, fabs(w[tmp + k]));
        if (!isfinite(mx)) return -1;
        const double s = -1.0 / mx;                            // minus the remainder, scaled by a positive factor
        for (int k = 0; k <= dc; ++k) w[oc + k] = w[tmp + k] * s;
        degs |= (uint64_t)dc << (4 * ic);
        ++n_chain;
    }
    const int v_minf = ess_sign_changes_inf(w, n_chain, degs, -1);
    int n_real = v_minf - ess_sign_changes_inf(w, n_chain, degs, +1);
    if (n_real <= 0) return 0;
    if (n_real > 10) n_real = 10;
    double bound = 0.0;                                        // Cauchy: every root lies inside (-bound, bound)
    for (int k = 0; k < d0; ++k) bound = fmax(bound, fabs(w[k]));
    bound = 1.0 + bound / fabs(w[d0]);
    if (!isfinite(bound)) return -1;
    double prev_hi = -bound;
    int found = 0;
    for (int k = 1; k <= n_real; ++k) {
        double lo = prev_hi, hi = bound;
        int chi = n_real;                                      // the number of roots in (-bound, hi]; k - 1 in (-bound, lo]
        for (int it = 0; it < 256 && chi != k; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (!(mid > lo) || !(mid < hi)) break;
            const int cm = v_minf - ess_sign_changes(w, n_chain, degs, mid);
            if (cm >= k) { hi = mid; chi = cm; }
            else lo = mid;
        }
        prev_hi = hi;
        double flo = w[d0], fhi = w[d0];
        for (int j = d0 - 1; j >= 0; --j) { flo = flo * lo + w[j]; fhi = fhi * hi + w[j]; }
        double z = 0.5 * (lo + hi);
        if (fhi == 0.0) z = hi;
        else if ((flo < 0.0) != (fhi < 0.0)) {
            for (int it = 0; it < 128; ++it) {
                const double mid = 0.5 * (lo + hi);
                if (!(mid > lo) || !(mid < hi)) break;
                double fm = w[d0];
                for (int j = d0 - 1; j >= 0; --j) fm = fm * mid + w[j];
                if (fm == 0.0) { lo = hi = mid; break; }
                if ((fm < 0.0) == (flo < 0.0)) lo = mid;
                else hi = mid;
            }
            z = 0.5 * (lo + hi);
        }
        for (int it = 0; it < 2; ++it) {
            double v = w[d0], dv = 0.0;
            for (int j = d0 - 1; j >= 0; --j) { dv = dv * z + v; v = v * z + w[j]; }
            const double zn = z - v / dv;
            if (isfinite(zn)) z = zn;
        }
#pragma unroll
        for (int j = 0; j < 10; ++j)
            if (j == found) roots[j] = z;
        ++found;
    }
    return found;
}

// C = A B, C = A B^T, C = A^T B for 3 x 3 row-major matrices
ESS_HD void ess_mm(double (&C)[9], const double (&A)[9], const double (&B)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
ESS_HD void ess_mmt(double (&C)[9], const double (&A)[9], const double (&B)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
}
ESS_HD void ess_mtm(double (&C)[9], const double (&A)[9], const double (&B)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}

// Three Gauss-Newton steps on the ten constraints themselves, det E and 2 E E^T E - tr(E E^T) E, evaluated on E = sum c_k N_k.  A
// root of the degree-10 polynomial and the x, y back-substituted from it carry the conditioning of the chart N3 = 1 the
// elimination worked in -- poor when the solution's own N3 coordinate is small.  Here the coordinate of largest magnitude is the
// one held at 1 (its null vector trades places with N3), so the three free ones are at most 1 and the step is as well-posed as the
// solution itself.  c comes back in the caller's order.
ESS_HD void ess_polish(const double (&N)[4][9], double (&c)[4]) {
    int ks = 3;
    double big = fabs(c[3]);
#pragma unroll
    for (int k = 2; k >= 0; --k)
        if (fabs(c[k]) >= big) { big = fabs(c[k]); ks = k; }
    double P[4][9];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 9; ++j) P[k][j] = k == 3 ? (ks == 0 ? N[0][j] : (ks == 1 ? N[1][j] : (ks == 2 ? N[2][j] : N[3][j]))) : (k == ks ? N[3][j] : N[k][j]);
    const double lead = ks == 0 ? c[0] : (ks == 1 ? c[1] : (ks == 2 ? c[2] : c[3]));
    double v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (k == ks ? c[3] : c[k]) / lead;
    if (!isfinite(v[0]) || !isfinite(v[1]) || !isfinite(v[2])) return;
#pragma unroll 1
    for (int it = 0; it < 3; ++it) {
        double E[9], A[9], B[9], f[10], J[10][3];
#pragma unroll
        for (int j = 0; j < 9; ++j) E[j] = v[0] * P[0][j] + v[1] * P[1][j] + v[2] * P[2][j] + P[3][j];
        ess_mmt(A, E, E);                              // E E^T
        ess_mtm(B, E, E);                              // E^T E
        const double tr = A[0] + A[4] + A[8];
        double cof[9], T[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
            cof[3 * i + 0] = E[3 * i1 + 1] * E[3 * i2 + 2] - E[3 * i1 + 2] * E[3 * i2 + 1];
            cof[3 * i + 1] = E[3 * i1 + 2] * E[3 * i2 + 0] - E[3 * i1 + 0] * E[3 * i2 + 2];
            cof[3 * i + 2] = E[3 * i1 + 0] * E[3 * i2 + 1] - E[3 * i1 + 1] * E[3 * i2 + 0];
        }
        f[0] = E[0] * cof[0] + E[1] * cof[1] + E[2] * cof[2];
        ess_mm(T, A, E);
#pragma unroll
        for (int j = 0; j < 9; ++j) f[1 + j] = 2.0 * T[j] - tr * E[j];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double d0 = 0.0, trd = 0.0, T1[9], T2[9], T3[9], U[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) { d0 += cof[j] * P[k][j]; trd += E[j] * P[k][j]; }
            J[0][k] = d0;
            ess_mm(T1, P[k], B);                       // D E^T E
            ess_mtm(U, P[k], E);                       // D^T E
            ess_mm(T2, E, U);                          // E D^T E
            ess_mm(T3, A, P[k]);                       // E E^T D
#pragma unroll
            for (int j = 0; j < 9; ++j) J[1 + j][k] = 2.0 * (T1[j] + T2[j] + T3[j]) - 2.0 * trd * E[j] - tr * P[k][j];
        }
        double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            a00 += J[r][0] * J[r][0]; a01 += J[r][0] * J[r][1]; a02 += J[r][0] * J[r][2];
            a11 += J[r][1] * J[r][1]; a12 += J[r][1] * J[r][2]; a22 += J[r][2] * J[r][2];
            g0 += J[r][0] * f[r]; g1 += J[r][1] * f[r]; g2 += J[r][2] * f[r];
        }
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double inv = 1.0 / (a00 * c00 + a01 * c01 + a02 * c02);
        const double d0 = (c00 * g0 + c01 * g1 + c02 * g2) * inv, d1 = (c01 * g0 + c11 * g1 + c12 * g2) * inv;
        const double d2 = (c02 * g0 + c12 * g1 + c22 * g2) * inv;
        if (!isfinite(d0) || !isfinite(d1) || !isfinite(d2)) break;
        v[0] -= d0; v[1] -= d1; v[2] -= d2;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = k == ks ? 1.0 : v[k];
    c[3] = ks == 3 ? 1.0 : (ks == 0 ? v[0] : (ks == 1 ? v[1] : v[2]));
}

// squared Sampson distance of the correspondence (x, y) -> (u, v) under E, in the units of the points
ESS_HD double ess_sampson2(const double (&E)[9], double x, double y, double u, double v) {
    const double a0 = E[0] * x + E[1] * y + E[2], a1 = E[3] * x + E[4] * y + E[5], a2 = E[6] * x + E[7] * y + E[8];
    const double b0 = E[0] * u + E[3] * v + E[6], b1 = E[1] * u + E[4] * v + E[7];
    const double e = u * a0 + v * a1 + a2;
    return e * e / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
}

// ---- the contract's hypothesis ---------------------------------------------------------------------------------------------------
// xl / xr = six normalised correspondences ((u - cx) / fx, (v - cy) / fy): 0 .. 4 go to the solver, 5 selects among its solutions.
// E row-major with Frobenius norm sqrt 2 and its entry of largest magnitude positive; nsol = the real solutions found.  false =
// invalid (E untouched; nsol = 0 unless the solver ran).
template <class Store>
ESS_HD bool ess_hypothesis(const Store& w, const double (&xl)[12], const double (&xr)[12], double (&E)[9], int& nsol) {
    nsol = 0;
    double N[4][9];
    {
        double l5[10], r5[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) { l5[j] = xl[j]; r5[j] = xr[j]; }
        if (!ess_null_space(w, l5, r5, N)) return false;
    }
    ess_constraints(w, N);
    if (!ess_eliminate(w)) return false;
    // B(z) [x y 1]^T = 0: rows <k> = <e> - z <f>, <l> = <g> - z <h>, <m> = <i> - z <j> of Nister's elimination; every row is
    // x (cubic in z) + y (cubic in z) + (quartic in z)
    double bx[3][4], by[3][4], b1[3][5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int e = 20 * (4 + 2 * r) + 10, f = 20 * (5 + 2 * r) + 10;
        bx[r][0] = w[e + 2]; bx[r][1] = w[e + 1] - w[f + 2]; bx[r][2] = w[e + 0] - w[f + 1]; bx[r][3] = -w[f + 0];
        by[r][0] = w[e + 5]; by[r][1] = w[e + 4] - w[f + 5]; by[r][2] = w[e + 3] - w[f + 4]; by[r][3] = -w[f + 3];
        b1[r][0] = w[e + 9]; b1[r][1] = w[e + 8] - w[f + 9]; b1[r][2] = w[e + 7] - w[f + 8]; b1[r][3] = w[e + 6] - w[f + 7];
        b1[r][4] = -w[f + 6];
    }
    double p1[8], p2[8], p3[7], n[11];
#pragma unroll
    for (int k = 0; k < 8; ++k) p1[k] = p2[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) p3[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) n[k] = 0.0;
    ess_pmul(p1, by[0], b1[1], 1.0); ess_pmul(p1, b1[0], by[1], -1.0);
    ess_pmul(p2, b1[0], bx[1], 1.0); ess_pmul(p2, bx[0], b1[1], -1.0);
    ess_pmul(p3, bx[0], by[1], 1.0); ess_pmul(p3, by[0], bx[1], -1.0);
    ess_pmul(n, p1, bx[2], 1.0); ess_pmul(n, p2, by[2], 1.0); ess_pmul(n, p3, b1[2], 1.0);
    double roots[10];
    const int n_roots = ess_real_roots(w, n, roots);
    if (n_roots < 0) return false;
    double best = 0.0, Eb[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) Eb[j] = 0.0;
    bool have = false;
#pragma unroll 1
    for (int k = 0; k < 10; ++k) {
        if (k >= n_roots) break;
        double z = 0.0;
#pragma unroll
        for (int j = 0; j < 10; ++j)
            if (j == k) z = roots[j];
        const double d = 1.0 / ess_horner(p3, z);
        const double x = ess_horner(p1, z) * d, y = ess_horner(p2, z) * d;
        if (!isfinite(x) || !isfinite(y)) continue;
        double co[4] = { x, y, z, 1.0 };
        ess_polish(N, co);
        double C[9], s = 0.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            C[j] = co[0] * N[0][j] + co[1] * N[1][j] + co[2] * N[2][j] + co[3] * N[3][j];
            s += C[j] * C[j];
        }
        s = sqrt(2.0 / s);
#pragma unroll
        for (int j = 0; j < 9; ++j) C[j] *= s;
        const double dist = ess_sampson2(C, xl[10], xl[11], xr[10], xr[11]);
        if (!isfinite(s) || !isfinite(dist)) continue;
        ++nsol;
        if (!have || dist < best) {
            have = true;
            best = dist;
#pragma unroll
            for (int j = 0; j < 9; ++j) Eb[j] = C[j];
        }
    }
    if (!have) return false;
    double big = 0.0, sign = 1.0;
#pragma unroll
    for (int j = 0; j < 9; ++j)
        if (fabs(Eb[j]) > big) { big = fabs(Eb[j]); sign = Eb[j] < 0.0 ? -1.0 : 1.0; }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        E[j] = sign * Eb[j];
        if (!isfinite(E[j])) have = false;
    }
    if (!have) {
#pragma unroll
        for (int j = 0; j < 9; ++j) E[j] = 0.0;
    }
    return have;
}

// ---- the score ---------------------------------------------------------------------------------------------------------------------
// G = fx fy diag(1/fx, 1/fy, 1) E diag(1/fx, 1/fy, 1) in fp64: the fundamental matrix on CENTRED pixels up to a scale the decision
// does not see.
ESS_HD void ess_pixel_matrix(const double (&E)[9], double fx, double fy, double (&G)[9]) {
    G[0] = E[0] * (fy / fx); G[1] = E[1];             G[2] = E[2] * fy;
    G[3] = E[3];             G[4] = E[4] * (fx / fy); G[5] = E[5] * fx;
    G[6] = E[6] * fy;        G[7] = E[7] * fx;        G[8] = E[8] * (fx * fy);
}

// THE inlier decision, for the count (k_ess_score) and for the mask (k_ess_select) alike.  (x, y) -> (xr, yr) one correspondence in
// centred pixels (u - cx, v - cy), as fp32 holds them.  Division-free squared Sampson distance: with l' = G p, l = G^T p' and
// e = p' . l' the test is e^2 <= thr^2 (l'_1^2 + l'_2^2 + l_1^2 + l_2^2); an all-zero G (an invalid hypothesis) has no inliers.
// The residual e is taken in fp64: its terms reach fx fy |E_33| + f |p| + |p|^2 and cancel down to a pixel times the gradient, and
// the worst-case fp32 bound of that cancellation, 6 ulp of the sum of their magnitudes over the gradient, is 8e-3 .. 1.4e-2 px on
// the test scenes -- outside the 5e-3 px band.  The gradient has no cancellation and stays in fp32 (a relative
// 2.4e-7 of the threshold).  Every operation is spelled out (no contraction is left to the compiler), so both kernels take the same
// decision for the same operands.
ESS_HD bool ess_inlier(const double (&G)[9], float x, float y, float xr, float yr, float thr2) {
    const double xd = (double)x, yd = (double)y, ud = (double)xr, vd = (double)yr;
    const double a0 = fma(G[0], xd, fma(G[1], yd, G[2]));
    const double a1 = fma(G[3], xd, fma(G[4], yd, G[5]));
    const double a2 = fma(G[6], xd, fma(G[7], yd, G[8]));
    const double e = fma(ud, a0, fma(vd, a1, a2));
    const float a0f = (float)a0, a1f = (float)a1;
    const float b0 = fmaf((float)G[0], xr, fmaf((float)G[3], yr, (float)G[6]));
    const float b1 = fmaf((float)G[1], xr, fmaf((float)G[4], yr, (float)G[7]));
    const float s = fmaf(a0f, a0f, fmaf(a1f, a1f, fmaf(b0, b0, b1 * b1)));
    return s > 0.0f && e * e <= (double)(thr2 * s);
}

// ---- recoverPose in closed form ------------------------------------------------------------------------------------------------------
// Horn 1990: with |E|_F^2 = 2, t t^T = 1/2 tr(E E^T) I - E E^T; t = its column with the largest diagonal entry (the first on ties)
// over the root of that entry, so |t| = 1.  R(+-t) = cof(E) - [+-t]x E with cof the cofactor matrix (row i = row i+1 x row i+2).
// Rp = R(+t), Rm = R(-t); the candidates are (Rp, +t), (Rm, -t), (Rm, +t), (Rp, -t).  false on a non-finite value or t = 0.
ESS_HD bool ess_pose_candidates(const double (&E)[9], double (&Rp)[9], double (&Rm)[9], double (&t)[3]) {
    double A[9];                                       // E E^T
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[3 * i + j] = E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1] + E[3 * i + 2] * E[3 * j + 2];
    const double h = 0.5 * (A[0] + A[4] + A[8]);
    const double d0 = h - A[0], d1 = h - A[4], d2 = h - A[8];
    const int c = (d0 >= d1 && d0 >= d2) ? 0 : (d1 >= d2 ? 1 : 2);
    const double dc = c == 0 ? d0 : (c == 1 ? d1 : d2);
    if (!(dc > 0.0) || !isfinite(dc)) return false;
    const double inv = 1.0 / sqrt(dc);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = c == 0 ? A[3 * i] : (c == 1 ? A[3 * i + 1] : A[3 * i + 2]);
        t[i] = ((i == c ? h : 0.0) - a) * inv;
    }
    double cof[9], tE[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        cof[3 * i + 0] = E[3 * i1 + 1] * E[3 * i2 + 2] - E[3 * i1 + 2] * E[3 * i2 + 1];
        cof[3 * i + 1] = E[3 * i1 + 2] * E[3 * i2 + 0] - E[3 * i1 + 0] * E[3 * i2 + 2];
        cof[3 * i + 2] = E[3 * i1 + 0] * E[3 * i2 + 1] - E[3 * i1 + 1] * E[3 * i2 + 0];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {                      // [t]x E, column by column: t x (column j of E)
        tE[0 + j] = t[1] * E[6 + j] - t[2] * E[3 + j];
        tE[3 + j] = t[2] * E[0 + j] - t[0] * E[6 + j];
        tE[6 + j] = t[0] * E[3 + j] - t[1] * E[0 + j];
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        Rp[j] = cof[j] - tE[j];
        Rm[j] = cof[j] + tE[j];
        ok = ok && isfinite(Rp[j]) && isfinite(Rm[j]);
    }
    return ok;
}

// Is the correspondence x = (x, y, 1) -> x' = (u, v, 1) (normalised points) in front of both cameras of the pose (R, sgn * t)?  The
// least-squares depths of lambda' x' = lambda R x + t: with a = R x and c = a x x' the 2 x 2 normal equations have the determinant
// |c|^2 (Lagrange) and the solution lambda = ((x' x t) . c) / |c|^2, lambda' = ((a x t) . c) / |c|^2.  In front iff |c|^2 > 0 and
// both depths lie inside (0, ESS_MAX_DEPTH); division-free.
ESS_HD bool ess_in_front(const double (&R)[9], const double (&t)[3], double sgn, double x, double y, double u, double v) {
    const double a0 = R[0] * x + R[1] * y + R[2], a1 = R[3] * x + R[4] * y + R[5], a2 = R[6] * x + R[7] * y + R[8];
    const double t0 = sgn * t[0], t1 = sgn * t[1], t2 = sgn * t[2];
    const double c0 = a1 - a2 * v, c1 = a2 * u - a0, c2 = a0 * v - a1 * u;                 // a x x', x' = (u, v, 1)
    const double det = c0 * c0 + c1 * c1 + c2 * c2;
    const double l = (v * t2 - t1) * c0 + (t0 - u * t2) * c1 + (u * t1 - v * t0) * c2;      // (x' x t) . c
    const double lp = (a1 * t2 - a2 * t1) * c0 + (a2 * t0 - a0 * t2) * c1 + (a0 * t1 - a1 * t0) * c2;   // (a x t) . c
    const double lim = ESS_MAX_DEPTH * det;
    return det > 0.0 && l > 0.0 && l < lim && lp > 0.0 && lp < lim;
}

}  // namespace sfmba
