// mesh_clean_math_host.hip -- runs the contract of sfmba_mesh_smooth serially on the HOST through csrc/mesh_clean_math.h (the
// arithmetic the kernels of mesh_clean.hip run), so tests/test_mesh_clean_oracle_cpu.py can hold it against the Python restatement
// without a GPU.
//   hipcc -O2 -std=c++17 -I sfm-toy-library_amd/csrc -o mesh_clean_math_host tools/micro/mesh_clean_math_host.hip
//   mesh_clean_math_host factor FILE     lines "f lo hi"                         -> "ok F"
//   mesh_clean_math_host quantise FILE   lines "x origin quantum"                -> "ok P"
//   mesh_clean_math_host move FILE       lines "Px Py Pz Sx Sy Sz D F"           -> "P'x P'y P'z" (clean_move: one vertex of one pass)
//   mesh_clean_math_host position FILE   lines "origin P quantum"                -> the float (8 hex digits)
//   mesh_clean_math_host normal FILE     lines "Pa (3) Pb (3) Pc (3)"            -> "Nx Ny Nz ok ux uy uz"
//   mesh_clean_math_host vnormal FILE    lines "Ux Uy Uz"                        -> the three floats (8 hex digits each)
// Floats are read with strtod (hex floats, inf and nan welcome), integers with strtoll.
#include "mesh_clean_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace sfmba;

static FILE* g_f;
static bool tok(char* t) { return std::fscanf(g_f, "%127s", t) == 1; }
static bool num(double& v) {
    char t[128];
    if (!tok(t)) return false;
    v = std::strtod(t, nullptr);
    return true;
}
static bool integers(long long* v, int n) {
    char t[128];
    for (int i = 0; i < n; ++i) {
        if (!tok(t)) return false;
        v[i] = std::strtoll(t, nullptr, 10);
    }
    return true;
}
static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

static int run_factor() {
    double f;
    long long r[2];
    while (num(f) && integers(r, 2)) {
        int F = 0;
        const bool ok = clean_factor((float)f, (int)r[0], (int)r[1], F);
        std::printf("%d %d\n", ok ? 1 : 0, ok ? F : 0);
    }
    return 0;
}

static int run_quantise() {
    double x, o, q;
    while (num(x) && num(o) && num(q)) {
        long long P = 0;
        const bool ok = clean_quantise((float)x, (double)(float)o, (double)(float)q, P);
        std::printf("%d %lld\n", ok ? 1 : 0, ok ? P : 0ll);
    }
    return 0;
}

static int run_move() {
    long long v[8], out[3];
    while (integers(v, 8)) {
        clean_move(v, v + 3, v[6], v[7], out);
        std::printf("%lld %lld %lld\n", out[0], out[1], out[2]);
    }
    return 0;
}

static int run_position() {
    double o, q;
    long long P;
    while (num(o) && integers(&P, 1) && num(q)) std::printf("%08x\n", bits(clean_position((double)(float)o, P, (double)(float)q)));
    return 0;
}

static int run_normal() {
    long long v[9], N[3], u[3];
    while (integers(v, 9)) {
        clean_cross(v, v + 3, v + 6, N);
        u[0] = u[1] = u[2] = 0;
        const bool ok = clean_unit_normal(N, u);
        std::printf("%lld %lld %lld %d %lld %lld %lld\n", N[0], N[1], N[2], ok ? 1 : 0, u[0], u[1], u[2]);
    }
    return 0;
}

static int run_vnormal() {
    long long U[3];
    float n[3];
    while (integers(U, 3)) {
        clean_vertex_normal(U, n);
        std::printf("%08x %08x %08x\n", bits(n[0]), bits(n[1]), bits(n[2]));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    if (!(g_f = std::fopen(argv[2], "r"))) return 2;
    if (!std::strcmp(argv[1], "factor")) return run_factor();
    if (!std::strcmp(argv[1], "quantise")) return run_quantise();
    if (!std::strcmp(argv[1], "move")) return run_move();
    if (!std::strcmp(argv[1], "position")) return run_position();
    if (!std::strcmp(argv[1], "normal")) return run_normal();
    if (!std::strcmp(argv[1], "vnormal")) return run_vnormal();
    return 2;
}
