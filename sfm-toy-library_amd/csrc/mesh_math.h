// mesh_math.h -- the per-element arithmetic of sfmba_tsdf_integrate / sfmba_tsdf_extract / sfmba_tsdf_mesh (the contract is in
// include/sfmba.h), as __host__ __device__ functions: the kernels of tsdf_mesh.hip and the serial host program
// tools/micro/mesh_math_host.hip run the same code, and tests/test_mesh_oracle_cpu.py holds the host program to the Python
// restatement bit for bit without a GPU.  Every fp64 operation is rounded on its own: hipcc contracts a multiply and an add into an
// fma by default, so every function with a double product that is followed by a sum switches the contraction off for its own body.
// Everything a voxel sums is an integer.  The projection is the fuse's (depth_math.h, depth_reproject): one copy.
#pragma once
#include "depth_math.h"

#include <cmath>
#include <cstdint>

namespace sfmba {

#define MESH_HD __host__ __device__ __forceinline__

constexpr int MESH_MAX_DIM = 1024;                         // a grid dimension lies in 1..1024
constexpr long long MESH_MAX_VOXELS = 1ll << 26;           // nx ny nz; a key (lin * 8 + code) stays below 2^29
constexpr int MESH_MAX_WEIGHT = 65535;                     // images of one call, and the largest min_weight
constexpr int MESH_NO_EDGE = 255;

// ---- the grid ----------------------------------------------------------------------------------------------------------------
// G_a = origin_a + (i_a voxel)
MESH_HD double mesh_grid_coord(double origin, int i, double voxel) {
#pragma clang fp contract(off)
    const double s = (double)i * voxel;
    return origin + s;
}

// ---- integration -------------------------------------------------------------------------------------------------------------
// What the image with pose p [12] and the w x h depth map adds to the voxel at X: false (nothing), or e in [-1024, 1024], whether the
// colour counts too (sdf <= T) and the pixel py w + px.  qz, px, py and sdf are left as far as the voxel got (for the host program).
MESH_HD bool mesh_observe(const double* k4, const double* p, const double* X, const float* map, int w, int h, double T, int& e, bool& colour,
                          int& px, int& py, double& qz, double& sdf) {
#pragma clang fp contract(off)
    if (!depth_reproject(k4, p, X, w, h, px, py, qz)) return false;
    const double zs = (double)map[(size_t)py * (size_t)w + (size_t)px];
    if (!(zs > 0.0)) return false;
    sdf = zs - qz;
    if (!(sdf >= -T)) return false;
    const double m = sdf < T ? sdf : T;
    double r = m / T;
    r = r * 1024.0;
    r = r + 0.5;
    e = (int)floor(r);
    colour = sdf <= T;
    return true;
}

// ---- extraction --------------------------------------------------------------------------------------------------------------
// An edge runs from grid vertex A to A + d, d in {0, 1}^3 \ {0}; code = d_x + 2 d_y + 4 d_z - 1 in 0..6; key = lin(A) * 8 + code.
// THE CASE TABLE.  Row [p][mask]: tetrahedron p of Kuhn's triangulation (the p-th permutation (a, b, c) of the axes in lexicographic
// order; local vertices v0 = corner, v1 = v0 + e_a, v2 = v1 + e_b, v3 = corner + (1, 1, 1)), bit l of mask set iff local vertex l is
// inside.  A row is n, e0 .. e5: n triangles (e0, e1, e2) and (e3, e4, e5), oriented (normals face the outside) and rotated (lowest
// key first).  An edge e = corner * 8 + code with corner = x + 2 y + 4 z of its lower end inside the cell; inside one cell the keys
// are ordered as these numbers are, whatever nx, ny >= 2.  MESH_NO_EDGE pads.  tests/test_mesh_oracle_cpu.py holds all 96 rows
// equal to the geometric rule of the contract.
MESH_HD const unsigned char* mesh_table_row(int p, int mask) {
    static constexpr unsigned char T[6][16][7] = {
    // tetrahedron 0: axes (0, 1, 2)
    { {   0, 255, 255, 255, 255, 255, 255 }, {   1,   0,   2,   6, 255, 255, 255 }, {   1,   0,  13,   9, 255, 255, 255 }, {   2,   2,   6,  13,   2,  13,   9 },
      {   1,   2,   9,  27, 255, 255, 255 }, {   2,   0,  27,   6,   0,   9,  27 }, {   2,   0,  13,  27,   0,  27,   2 }, {   1,   6,  13,  27, 255, 255, 255 },
      {   1,   6,  27,  13, 255, 255, 255 }, {   2,   0,   2,  27,   0,  27,  13 }, {   2,   0,  27,   9,   0,   6,  27 }, {   1,   2,  27,   9, 255, 255, 255 },
      {   2,   2,   9,  13,   2,  13,   6 }, {   1,   0,   9,  13, 255, 255, 255 }, {   1,   0,   6,   2, 255, 255, 255 }, {   0, 255, 255, 255, 255, 255, 255 } },
    // tetrahedron 1: axes (0, 2, 1)
    { {   0, 255, 255, 255, 255, 255, 255 }, {   1,   0,   6,   4, 255, 255, 255 }, {   1,   0,  11,  13, 255, 255, 255 }, {   2,   4,  13,   6,   4,  11,  13 },
      {   1,   4,  41,  11, 255, 255, 255 }, {   2,   0,   6,  41,   0,  41,  11 }, {   2,   0,  41,  13,   0,   4,  41 }, {   1,   6,  41,  13, 255, 255, 255 },
      {   1,   6,  13,  41, 255, 255, 255 }, {   2,   0,  41,   4,   0,  13,  41 }, {   2,   0,  11,  41,   0,  41,   6 }, {   1,   4,  11,  41, 255, 255, 255 },
      {   2,   4,  13,  11,   4,   6,  13 }, {   1,   0,  13,  11, 255, 255, 255 }, {   1,   0,   4,   6, 255, 255, 255 }, {   0, 255, 255, 255, 255, 255, 255 } },
    // tetrahedron 2: axes (1, 0, 2)
    { {   0, 255, 255, 255, 255, 255, 255 }, {   1,   1,   6,   2, 255, 255, 255 }, {   1,   1,  16,  20, 255, 255, 255 }, {   2,   2,  20,   6,   2,  16,  20 },
      {   1,   2,  27,  16, 255, 255, 255 }, {   2,   1,   6,  27,   1,  27,  16 }, {   2,   1,  27,  20,   1,   2,  27 }, {   1,   6,  27,  20, 255, 255, 255 },
      {   1,   6,  20,  27, 255, 255, 255 }, {   2,   1,  27,   2,   1,  20,  27 }, {   2,   1,  16,  27,   1,  27,   6 }, {   1,   2,  16,  27, 255, 255, 255 },
      {   2,   2,  20,  16,   2,   6,  20 }, {   1,   1,  20,  16, 255, 255, 255 }, {   1,   1,   2,   6, 255, 255, 255 }, {   0, 255, 255, 255, 255, 255, 255 } },
    // tetrahedron 3: axes (1, 2, 0)
    { {   0, 255, 255, 255, 255, 255, 255 }, {   1,   1,   5,   6, 255, 255, 255 }, {   1,   1,  20,  19, 255, 255, 255 }, {   2,   5,   6,  20,   5,  20,  19 },
      {   1,   5,  19,  48, 255, 255, 255 }, {   2,   1,  48,   6,   1,  19,  48 }, {   2,   1,  20,  48,   1,  48,   5 }, {   1,   6,  20,  48, 255, 255, 255 },
      {   1,   6,  48,  20, 255, 255, 255 }, {   2,   1,   5,  48,   1,  48,  20 }, {   2,   1,  48,  19,   1,   6,  48 }, {   1,   5,  48,  19, 255, 255, 255 },
      {   2,   5,  19,  20,   5,  20,   6 }, {   1,   1,  19,  20, 255, 255, 255 }, {   1,   1,   6,   5, 255, 255, 255 }, {   0, 255, 255, 255, 255, 255, 255 } },
    // tetrahedron 4: axes (2, 0, 1)
    { {   0, 255, 255, 255, 255, 255, 255 }, {   1,   3,   4,   6, 255, 255, 255 }, {   1,   3,  34,  32, 255, 255, 255 }, {   2,   4,   6,  34,   4,  34,  32 },
      {   1,   4,  32,  41, 255, 255, 255 }, {   2,   3,  41,   6,   3,  32,  41 }, {   2,   3,  34,  41,   3,  41,   4 }, {   1,   6,  34,  41, 255, 255, 255 },
      {   1,   6,  41,  34, 255, 255, 255 }, {   2,   3,   4,  41,   3,  41,  34 }, {   2,   3,  41,  32,   3,   6,  41 }, {   1,   4,  41,  32, 255, 255, 255 },
      {   2,   4,  32,  34,   4,  34,   6 }, {   1,   3,  32,  34, 255, 255, 255 }, {   1,   3,   6,   4, 255, 255, 255 }, {   0, 255, 255, 255, 255, 255, 255 } },
    // tetrahedron 5: axes (2, 1, 0)
    { {   0, 255, 255, 255, 255, 255, 255 }, {   1,   3,   6,   5, 255, 255, 255 }, {   1,   3,  33,  34, 255, 255, 255 }, {   2,   5,  34,   6,   5,  33,  34 },
      {   1,   5,  48,  33, 255, 255, 255 }, {   2,   3,   6,  48,   3,  48,  33 }, {   2,   3,  48,  34,   3,   5,  48 }, {   1,   6,  48,  34, 255, 255, 255 },
      {   1,   6,  34,  48, 255, 255, 255 }, {   2,   3,  48,   5,   3,  34,  48 }, {   2,   3,  33,  48,   3,  48,   6 }, {   1,   5,  33,  48, 255, 255, 255 },
      {   2,   5,  34,  33,   5,   6,  34 }, {   1,   3,  34,  33, 255, 255, 255 }, {   1,   3,   5,   6, 255, 255, 255 }, {   0, 255, 255, 255, 255, 255, 255 } },
    };
    return T[p][mask];
}
// the corner (x + 2 y + 4 z inside the cell) of local vertex l of tetrahedron p
MESH_HD int mesh_tet_corner(int p, int l) {
    // the permutations of the axes in lexicographic order: the first axis, then the lower or the higher of the other two
    const int a = p >> 1, b = (p & 1) ? (a == 2 ? 1 : 2) : (a == 0 ? 1 : 0);
    return l == 0 ? 0 : l == 1 ? (1 << a) : l == 2 ? ((1 << a) | (1 << b)) : 7;
}
// the 4-bit case of tetrahedron p from the 8 inside bits of its cell
MESH_HD int mesh_tet_mask(int p, int inside8) {
    int m = 0;
    for (int l = 0; l < 4; ++l) m |= ((inside8 >> mesh_tet_corner(p, l)) & 1) << l;
    return m;
}
// the number of triangles of a cell with these inside bits
MESH_HD int mesh_cell_triangles(int inside8) {
    int n = 0;
    for (int p = 0; p < 6; ++p) n += mesh_table_row(p, mesh_tet_mask(p, inside8))[0];
    return n;
}

// t = fA / (fA - fB) with f = (double)S / (double)W: the vertex lies at A + t d
MESH_HD double mesh_edge_t(int SA, int WA, int SB, int WB) {
    const double fA = (double)SA / (double)WA, fB = (double)SB / (double)WB;
    return fA / (fA - fB);
}
// pos_a = origin_a + ((i_a + (t d_a)) voxel), stored as float
MESH_HD float mesh_vertex_coord(double origin, int i, int d, double t, double voxel) {
#pragma clang fp contract(off)
    const double td = t * (double)d;
    const double g = (double)i + td;
    const double s = g * voxel;
    return (float)(origin + s);
}
// (2 (S_A + S_B) + w) / (2 w) with w = Wc_A + Wc_B, 0 when w == 0
MESH_HD unsigned char mesh_vertex_colour(int SA, int SB, int WA, int WB) {
    const long long w = (long long)WA + WB, s = (long long)SA + SB;
    return w == 0 ? (unsigned char)0 : (unsigned char)((2 * s + w) / (2 * w));
}

}  // namespace sfmba
