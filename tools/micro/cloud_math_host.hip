// cloud_math_host.hip -- runs the contracts of sfmba_depth_normals and sfmba_cloud_merge serially on the HOST through
// csrc/cloud_math.h (the arithmetic the kernels of cloud_merge.hip run), so tests/test_cloud_oracle_cpu.py can hold it against the
// Python restatement without a GPU.
//   hipcc -O2 -std=c++17 -I sfm-toy-library_amd/csrc -o cloud_math_host tools/micro/cloud_math_host.hip
//   cloud_math_host quantise FILE  lines "x y z voxel" (floats)            -> "valid q_0 q_1 q_2 key" (key: 16 hex digits)
//   cloud_math_host nquant FILE    lines "n" (a float)                     -> "m"
//   cloud_math_host final FILE     lines "c Sq_0 Sq_1 Sq_2 Sb Sg Sr Sm_0 Sm_1 Sm_2 voxel" (integers in decimal, voxel a float)
//                                                                          -> "x y z b g r nx ny nz" (floats: 8 hex digits)
//   cloud_math_host normal FILE    "w h fx fy cx cy P_0..P_11 max_rel_step" and the w * h depths.  Prints per pixel
//                                  "has n_0 n_1 n_2 c_0 c_1 c_2 len nc_0 nc_1 nc_2 du_0..du_2 dv_0..dv_2" (n: 8 hex digits, 0 without a
//                                  normal; the intermediates as far as the pixel got, 0 beyond)
// Floats are read with strtod (hex floats, inf and nan welcome), integers with strtoll; doubles are printed with %a: they round-trip.
#include "cloud_math.h"

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

static int run_quantise() {
    double v[4];
    while (nums(v, 4)) {
        const float p[3] = { (float)v[0], (float)v[1], (float)v[2] };
        long long q[3];
        const unsigned long long key = cloud_key(p, (double)(float)v[3], q);
        std::printf("%d %lld %lld %lld %016llx\n", key != CLOUD_KEY_SKIPPED ? 1 : 0, q[0], q[1], q[2], key);
    }
    return 0;
}

static int run_nquant() {
    double v;
    while (num(v)) std::printf("%lld\n", cloud_normal_quantum((float)v));
    return 0;
}

static int run_final() {
    long long s[10];
    for (;;) {
        for (int i = 0; i < 10; ++i) if (!integer(s[i])) return 0;
        double voxel;
        if (!num(voxel)) return 2;
        const int c = (int)s[0];
        float n[3];
        cloud_final_normal(s + 7, n);
        std::printf("%08x %08x %08x %d %d %d %08x %08x %08x\n", bits(cloud_final_coord(s[1], c, (double)(float)voxel)),
                    bits(cloud_final_coord(s[2], c, (double)(float)voxel)), bits(cloud_final_coord(s[3], c, (double)(float)voxel)),
                    (int)cloud_final_colour(s[4], c), (int)cloud_final_colour(s[5], c), (int)cloud_final_colour(s[6], c), bits(n[0]), bits(n[1]),
                    bits(n[2]));
    }
}

static int run_normal() {
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
    for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u) {
            float n[3] = { 0.0f, 0.0f, 0.0f };
            double mid[13];
            for (double& m : mid) m = 0.0;
            const bool has = cloud_pixel_normal(hdr + 2, hdr + 6, depth.data(), w, h, u, v, (double)(float)hdr[18], n, mid);
            std::printf("%d %08x %08x %08x", has ? 1 : 0, bits(n[0]), bits(n[1]), bits(n[2]));
            for (double m : mid) std::printf(" %a", m);
            std::printf("\n");
        }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3 || !(g_f = std::fopen(argv[2], "r"))) return 2;
    if (!std::strcmp(argv[1], "quantise")) return run_quantise();
    if (!std::strcmp(argv[1], "nquant")) return run_nquant();
    if (!std::strcmp(argv[1], "final")) return run_final();
    if (!std::strcmp(argv[1], "normal")) return run_normal();
    return 2;
}
