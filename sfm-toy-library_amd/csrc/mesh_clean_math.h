// mesh_clean_math.h -- the per-element arithmetic of sfmba_mesh_smooth / sfmba_mesh_clean (the contract is in include/sfmba.h), as
// __host__ __device__ functions: the kernels of mesh_clean.hip and the serial host program tools/micro/mesh_clean_math_host.hip run
// the same code, and tests/test_mesh_clean_oracle_cpu.py holds the host program to the Python restatement bit for bit without a GPU.
// Every fp64 operation is rounded on its own: hipcc contracts a multiply and an add into an fma by default, so every function with
// a double product that is followed by a sum switches the contraction off for its own body.  Everything that is summed across
// triangles is an integer.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace sfmba {

#define CLEAN_HD __host__ __device__ __forceinline__

constexpr long long CLEAN_MAX_P = 1ll << 25;               // a quantised coordinate satisfies |P| < 2^25, before and after every pass
constexpr int CLEAN_MAX_D = 1 << 17;                       // a vertex with a larger degree sum does not move
constexpr int CLEAN_MAX_ITERATIONS = 100;
constexpr double CLEAN_UNIT = 1048576.0;                   // a triangle's unit normal is summed in units of 2^-20

// F = (int)floor((double)f 65536 + 0.5) if that lies in lo..hi; false otherwise (a NaN fails)
CLEAN_HD bool clean_factor(float f, int lo, int hi, int& F) {
#pragma clang fp contract(off)
    double r = (double)f * 65536.0;
    r = r + 0.5;
    r = floor(r);
    if (!(r >= (double)lo && r <= (double)hi)) return false;
    F = (int)r;
    return true;
}

// P = (int64)floor(((double)x - origin) / quantum + 0.5), false if x is not finite or |P| >= 2^25 (a NaN fails the comparison)
CLEAN_HD bool clean_quantise(float x, double origin, double quantum, long long& P) {
#pragma clang fp contract(off)
    double r = (double)x - origin;
    r = r / quantum;
    r = r + 0.5;
    r = floor(r);
    if (!(r > -(double)CLEAN_MAX_P && r < (double)CLEAN_MAX_P)) return false;
    P = (long long)r;
    return true;
}

// floor(num / den) for den > 0
CLEAN_HD long long clean_floor_div(long long num, long long den) {
    const long long q = num / den;
    return (num % den < 0) ? q - 1 : q;
}

// One axis of one pass with factor F: n = F (S - D P), den = D 65536, P' = P + floor((2 n + den) / (2 den)).  1 <= D <= 2^17.
CLEAN_HD long long clean_step(long long P, long long S, long long D, long long F) {
    const long long n = F * (S - D * P), den = D * 65536;
    return P + clean_floor_div(2 * n + den, 2 * den);
}

// A whole vertex of one pass: D == 0 or D > 2^17 does not move; neither does a vertex that a pass would carry to |P'| >= 2^25 on
// some axis (only a mu near -2 on a spike at the rim of the range can; it keeps every later bound of the contract true).
CLEAN_HD void clean_move(const long long* P, const long long* S, long long D, long long F, long long* out) {
    for (int a = 0; a < 3; ++a) out[a] = P[a];
    if (D == 0 || D > CLEAN_MAX_D) return;
    long long Q[3];
    for (int a = 0; a < 3; ++a) {
        Q[a] = clean_step(P[a], S[a], D, F);
        if (Q[a] <= -CLEAN_MAX_P || Q[a] >= CLEAN_MAX_P) return;
    }
    for (int a = 0; a < 3; ++a) out[a] = Q[a];
}

// (float)(origin + (double)P quantum)
CLEAN_HD float clean_position(double origin, long long P, double quantum) {
#pragma clang fp contract(off)
    const double s = (double)P * quantum;
    return (float)(origin + s);
}

// N = (Pb - Pa) x (Pc - Pa), exact in int64 and, below 2^53, in double
CLEAN_HD void clean_cross(const long long* Pa, const long long* Pb, const long long* Pc, long long* N) {
    const long long e[3] = { Pb[0] - Pa[0], Pb[1] - Pa[1], Pb[2] - Pa[2] }, f[3] = { Pc[0] - Pa[0], Pc[1] - Pa[1], Pc[2] - Pa[2] };
    N[0] = e[1] * f[2] - e[2] * f[1];
    N[1] = e[2] * f[0] - e[0] * f[2];
    N[2] = e[0] * f[1] - e[1] * f[0];
}

// What a triangle with the integer normal N adds to each of its vertices: u_a = (int64)floor((N_a / len) 2^20 + 0.5) with
// len = sqrt((Nx Nx + Ny Ny) + Nz Nz); false (nothing) when len == 0
CLEAN_HD bool clean_unit_normal(const long long* N, long long* u) {
#pragma clang fp contract(off)
    const double n[3] = { (double)N[0], (double)N[1], (double)N[2] };
    const double xx = n[0] * n[0], yy = n[1] * n[1], zz = n[2] * n[2];
    const double len = sqrt((xx + yy) + zz);
    if (len == 0.0) return false;
    for (int a = 0; a < 3; ++a) {
        double r = n[a] / len;
        r = r * CLEAN_UNIT;
        r = r + 0.5;
        u[a] = (long long)floor(r);
    }
    return true;
}

// The vertex normal of the sums U: (float)(U_a / sqrt((Ux Ux + Uy Uy) + Uz Uz)), (0, 0, 0) for a zero sum
CLEAN_HD void clean_vertex_normal(const long long* U, float* out) {
#pragma clang fp contract(off)
    out[0] = out[1] = out[2] = 0.0f;
    if (U[0] == 0 && U[1] == 0 && U[2] == 0) return;
    const double n[3] = { (double)U[0], (double)U[1], (double)U[2] };
    const double xx = n[0] * n[0], yy = n[1] * n[1], zz = n[2] * n[2];
    const double len = sqrt((xx + yy) + zz);
    for (int a = 0; a < 3; ++a) out[a] = (float)(n[a] / len);
}

}  // namespace sfmba
