// mesh_math_host.hip -- runs the contract of sfmba_tsdf_integrate / sfmba_tsdf_extract serially on the HOST through
// csrc/mesh_math.h (the arithmetic the kernels of tsdf_mesh.hip run), so tests/test_mesh_oracle_cpu.py can hold it against the
// Python restatement without a GPU.
//   hipcc -O2 -std=c++17 -I sfm-toy-library_amd/csrc -o mesh_math_host tools/micro/mesh_math_host.hip
//   mesh_math_host table FILE      (FILE is not read) -> 96 lines "p mask n e0 .. e5 c0 c1 c2 c3 triangles": the case table's row, the
//                                  corners of the tetrahedron's local vertices, and mesh_cell_triangles of the 8 bits p * 16 + mask
//                                  stands for (bits = (p * 16 + mask) * 37 % 256, so that all arguments get a look)
//   mesh_math_host grid FILE       lines "origin i voxel"                        -> the coordinate (%a)
//   mesh_math_host observe FILE    "w h fx fy cx cy P_0..P_11 trunc", the w * h depths, then lines "X_0 X_1 X_2"
//                                  -> "ok e colour px py qz sdf" (qz and sdf %a, as far as the voxel got, 0 beyond)
//   mesh_math_host vertex FILE     lines "SA WA SB WB origin i d voxel CA CB WcA WcB" (integers in decimal, origin and voxel floats)
//                                  -> "t pos colour" (t %a, pos: 8 hex digits)
// Floats are read with strtod (hex floats, inf and nan welcome), integers with strtoll; doubles are printed with %a: they round-trip.
#include "mesh_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sfmba;

static FILE* g_f;
static bool tok(char* t) { return std::fscanf(g_f, "%127s", t) == 1; }
static bool num(double& v) {
    char t[128];
    if (!tok(t)) return false;
    v = std::strtod(t, nullptr);
    return true;
}
static bool nums(double* v, int n) { for (int i = 0; i < n; ++i) if (!num(v[i])) return false; return true; }
static bool integer(long long& v) {
    char t[128];
    if (!tok(t)) return false;
    v = std::strtoll(t, nullptr, 10);
    return true;
}
static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

static int run_table() {
    for (int p = 0; p < 6; ++p)
        for (int mask = 0; mask < 16; ++mask) {
            const unsigned char* row = mesh_table_row(p, mask);
            std::printf("%d %d", p, mask);
            for (int q = 0; q < 7; ++q) std::printf(" %d", (int)row[q]);
            for (int l = 0; l < 4; ++l) std::printf(" %d", mesh_tet_corner(p, l));
            std::printf(" %d\n", mesh_cell_triangles((p * 16 + mask) * 37 % 256));
        }
    return 0;
}

static int run_grid() {
    double v[3];
    while (nums(v, 3)) std::printf("%a\n", mesh_grid_coord((double)(float)v[0], (int)v[1], (double)(float)v[2]));
    return 0;
}

static int run_observe() {
    double hdr[19];
    if (!nums(hdr, 19)) return 2;
    const int w = (int)hdr[0], h = (int)hdr[1];
    if (w < 1 || h < 1) return 2;
    std::vector<float> depth((size_t)w * h);
    for (float& d : depth) {
        double v;
        if (!num(v)) return 2;
        d = (float)v;
    }
    double X[3];
    while (nums(X, 3)) {
        int e = 0, px = 0, py = 0;
        bool colour = false;
        double qz = 0.0, sdf = 0.0;
        const bool ok = mesh_observe(hdr + 2, hdr + 6, X, depth.data(), w, h, (double)(float)hdr[18], e, colour, px, py, qz, sdf);
        std::printf("%d %d %d %d %d %a %a\n", ok ? 1 : 0, e, colour ? 1 : 0, px, py, qz, sdf);
    }
    return 0;
}

static int run_vertex() {
    long long s[4], c[4];
    for (;;) {
        for (int i = 0; i < 4; ++i) if (!integer(s[i])) return 0;
        double origin, voxel;
        long long i, d;
        if (!num(origin) || !integer(i) || !integer(d) || !num(voxel)) return 2;
        for (int q = 0; q < 4; ++q) if (!integer(c[q])) return 2;
        const double t = mesh_edge_t((int)s[0], (int)s[1], (int)s[2], (int)s[3]);
        std::printf("%a %08x %d\n", t, bits(mesh_vertex_coord((double)(float)origin, (int)i, (int)d, t, (double)(float)voxel)),
                    (int)mesh_vertex_colour((int)c[0], (int)c[1], (int)c[2], (int)c[3]));
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    if (!std::strcmp(argv[1], "table")) return run_table();
    if (!(g_f = std::fopen(argv[2], "r"))) return 2;
    if (!std::strcmp(argv[1], "grid")) return run_grid();
    if (!std::strcmp(argv[1], "observe")) return run_observe();
    if (!std::strcmp(argv[1], "vertex")) return run_vertex();
    return 2;
}
