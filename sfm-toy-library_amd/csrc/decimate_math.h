// decimate_math.h -- the per-element arithmetic of sfmba_mesh_decimate (the contract is in include/sfmba.h), as __host__ __device__
// functions: the kernels of mesh_decimate.hip and the serial host program tools/micro/decimate_math_host.hip run the same code, and
// tests/test_decimate_oracle_cpu.py holds the host program to the Python restatement bit for bit without a GPU.  The quantisation,
// the floor division, the cross product and the position are those of mesh_clean_math.h.  Every fp64 operation is rounded on its
// own: every function with a double product that is followed by a sum switches the compiler's contraction off for its own body.
// Everything that is summed across vertices or triangles is an integer.
//
// Bounds (cell <= 2^20, |u| <= 1024, n_inc <= 2^16): 0 <= r < 2^20; |e| <= 3 * 1024 * 2^20 < 2^32; per triangle |u_i u_j| <= 2^20 and
// |u_i e| < 2^42, so up to the cap |A_ij| <= 2^36 and |b_i| < 2^58; a sum of r over n < 2^31 members stays below 2^51.
#pragma once
#include "mesh_clean_math.h"

namespace sfmba {

constexpr int DEC_MIN_CELL = 32;
constexpr int DEC_MAX_CELL = 1 << 20;
constexpr int DEC_MAX_REG = 1 << 20;
constexpr long long DEC_MAX_INC = 1ll << 16;               // a cluster with more incident triangles takes the mean
constexpr long long DEC_KEY_BIAS = 1ll << 20;
constexpr double DEC_UNIT = 1024.0;                         // a triangle's unit normal enters the quadric in units of 2^-10

// c = floor_div(P, cell), r = P - c cell in 0 .. cell-1
CLEAN_HD void dec_cell(long long P, long long cell, long long& c, long long& r) {
    c = clean_floor_div(P, cell);
    r = P - c * cell;
}

// c_a in [-2^20, 2^20): 21 bits an axis
CLEAN_HD unsigned long long dec_key(const long long* c) {
    return ((unsigned long long)(c[2] + DEC_KEY_BIAS) << 42) | ((unsigned long long)(c[1] + DEC_KEY_BIAS) << 21) | (unsigned long long)(c[0] + DEC_KEY_BIAS);
}
CLEAN_HD void dec_key_cell(unsigned long long key, long long* c) {
    for (int a = 0; a < 3; ++a) c[a] = (long long)((key >> (21 * a)) & 0x1fffffull) - DEC_KEY_BIAS;
}

// the rounded mean of a sum S >= 0 over n >= 1 members
CLEAN_HD long long dec_mean(long long S, long long n) { return clean_floor_div(2 * S + n, 2 * n); }

// u_a = (int64)floor((N_a / len) 1024 + 0.5) with len = sqrt((Nx Nx + Ny Ny) + Nz Nz); false when len == 0
CLEAN_HD bool dec_unit_normal(const long long* N, long long* u) {
#pragma clang fp contract(off)
    const double n[3] = { (double)N[0], (double)N[1], (double)N[2] };
    const double xx = n[0] * n[0], yy = n[1] * n[1], zz = n[2] * n[2];
    const double len = sqrt((xx + yy) + zz);
    if (len == 0.0) return false;
    for (int a = 0; a < 3; ++a) {
        double r = n[a] / len;
        r = r * DEC_UNIT;
        r = r + 0.5;
        u[a] = (long long)floor(r);
    }
    return true;
}

// e = (u_x r_x + u_y r_y) + u_z r_z, and what a triangle with the normal u adds to the cluster of a vertex with the remainder r:
// q[0..5] = A00 A01 A02 A11 A12 A22, q[6..8] = b, q[9] = 1 (n_inc)
CLEAN_HD long long dec_plane_offset(const long long* u, const long long* r) { return (u[0] * r[0] + u[1] * r[1]) + u[2] * r[2]; }
CLEAN_HD void dec_quadric_terms(const long long* u, const long long* r, long long* q) {
    const long long e = dec_plane_offset(u, r);
    q[0] = u[0] * u[0]; q[1] = u[0] * u[1]; q[2] = u[0] * u[2];
    q[3] = u[1] * u[1]; q[4] = u[1] * u[2]; q[5] = u[2] * u[2];
    q[6] = u[0] * e; q[7] = u[1] * e; q[8] = u[2] * e;
    q[9] = 1;
}

// everything the solve computes on its way, for the host program and the tests
struct DecSolveTrace { double s[6], g[3], c[6], det, x[3]; };

// The representative of a cluster from its quadric sums q (as dec_quadric_terms), the member sums Sp over n members, reg and cell:
// false (R untouched) when the cluster takes the mean: n_inc == 0, n_inc > 2^16, !(det > 0) or a solution that is not finite.
CLEAN_HD bool dec_solve(const long long* q, const long long* Sp, long long n, long long reg, long long cell, long long* R, DecSolveTrace* tr) {
#pragma clang fp contract(off)
    const long long n_inc = q[9];
    if (n_inc == 0 || n_inc > DEC_MAX_INC) return false;
    const double rho = (double)reg * (double)n_inc;
    double s[6], g[3];
    for (int k = 0; k < 6; ++k) s[k] = (double)q[k];
    s[0] = s[0] + rho; s[3] = s[3] + rho; s[5] = s[5] + rho;
    for (int a = 0; a < 3; ++a) {
        const double m = (double)Sp[a] / (double)n;
        const double rm = rho * m;
        g[a] = (double)q[6 + a] + rm;
    }
    const double s00 = s[0], s01 = s[1], s02 = s[2], s11 = s[3], s12 = s[4], s22 = s[5];
    double p, t;
    double c[6];
    p = s11 * s22; t = s12 * s12; c[0] = p - t;      // c00
    p = s02 * s12; t = s01 * s22; c[1] = p - t;      // c01
    p = s01 * s12; t = s02 * s11; c[2] = p - t;      // c02
    p = s00 * s22; t = s02 * s02; c[3] = p - t;      // c11
    p = s01 * s02; t = s00 * s12; c[4] = p - t;      // c12
    p = s00 * s11; t = s01 * s01; c[5] = p - t;      // c22
    double d0 = s00 * c[0], d1 = s01 * c[1], d2 = s02 * c[2];
    const double det = (d0 + d1) + d2;
    const int row[3][3] = { { 0, 1, 2 }, { 1, 3, 4 }, { 2, 4, 5 } };
    double x[3];
    for (int a = 0; a < 3; ++a) {
        d0 = c[row[a][0]] * g[0]; d1 = c[row[a][1]] * g[1]; d2 = c[row[a][2]] * g[2];
        x[a] = ((d0 + d1) + d2) / det;
    }
    if (tr) {
        for (int k = 0; k < 6; ++k) { tr->s[k] = s[k]; tr->c[k] = c[k]; }
        for (int a = 0; a < 3; ++a) { tr->g[a] = g[a]; tr->x[a] = x[a]; }
        tr->det = det;
    }
    if (!(det > 0.0)) return false;
    for (int a = 0; a < 3; ++a)
        if (!(x[a] - x[a] == 0.0)) return false;                // inf or NaN
    for (int a = 0; a < 3; ++a) {
        const double f = floor(x[a] + 0.5);
        R[a] = f < 0.0 ? 0 : f > (double)(cell - 1) ? cell - 1 : (long long)f;
    }
    return true;
}

// (float)(origin + (double)(c cell + R) quantum)
CLEAN_HD float dec_position(double origin, long long c, long long cell, long long R, double quantum) { return clean_position(origin, c * cell + R, quantum); }

}  // namespace sfmba
