// sgm_math_host.hip -- runs the contract of sfmba_sgm_aggregate and the selection of sfmba_depth_sweep_sgm serially on the HOST through
// csrc/sgm_math.h (the arithmetic the kernels of depth_sgm.hip run), so tests/test_sgm_oracle_cpu.py can hold it against the numpy
// restatement without a GPU.  Built with the host sanitizers:
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I sfm-toy-library_amd/csrc -o sgm_math_host tools/micro/sgm_math_host.hip
//   sgm_math_host quantise FILE   lines "C" (a double)            -> "q"
//   sgm_math_host delta FILE      lines "sm s0 sp" (integers)     -> "den delta"
//   sgm_math_host volume FILE     "w h D p1 p2 n_paths invalid_cost uniqueness wf step" and the w * h * D volume entries, the plane
//                                 fastest.  Prints every intermediate:
//                                   "C x y c_0 .. c_{D-1}"        the costs as the aggregation reads them,
//                                   "L r x y m L_0 .. L_{D-1}"    per direction r and pixel (m = -1 at the first pixel of a line),
//                                   "S x y S_0 .. S_{D-1}",
//                                   "O x y k best second den delta depth score accepted q" (depth, score: 8 hex digits).
// Numbers are read with strtod (hex floats welcome) and doubles are printed with %a: they round-trip.
#include "sgm_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sfmba;

static FILE* g_f;
static bool num(double& v) {
    char tok[128];
    if (std::fscanf(g_f, "%127s", tok) != 1) return false;
    v = std::strtod(tok, nullptr);
    return true;
}
static bool nums(double* v, int n) { for (int i = 0; i < n; ++i) if (!num(v[i])) return false; return true; }
static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

static int run_quantise() {
    double C;
    while (num(C)) std::printf("%d\n", sgm_quantise(C));
    return 0;
}

static int run_delta() {
    double v[3];
    while (nums(v, 3)) std::printf("%d %a\n", sgm_den((int)v[0], (int)v[1], (int)v[2]), sgm_delta((int)v[0], (int)v[1], (int)v[2]));
    return 0;
}

static int run_volume() {
    double hdr[10];
    if (!nums(hdr, 10)) return 2;
    const int w = (int)hdr[0], h = (int)hdr[1], D = (int)hdr[2], p1 = (int)hdr[3], p2 = (int)hdr[4], n_paths = (int)hdr[5];
    const int invalid_cost = (int)hdr[6], uniqueness = (int)hdr[7];
    const double wf = hdr[8], step = hdr[9];
    if (w < 1 || h < 1 || D < 2 || D > DEPTH_MAX_PLANES || (n_paths != 4 && n_paths != 8) || p1 < 0 || p2 < p1 || p2 > SGM_MAX_PENALTY) return 2;
    const size_t n_px = (size_t)w * h;
    std::vector<unsigned char> vol(n_px * D);
    for (unsigned char& e : vol) { double g; if (!num(g)) return 2; e = (unsigned char)g; }
    std::vector<uint16_t> S(n_px * D, 0);
    std::vector<int> L((size_t)D), prev((size_t)D);

    for (size_t p = 0; p < n_px; ++p) {
        std::printf("C %d %d", (int)(p % w), (int)(p / w));
        for (int d = 0; d < D; ++d) std::printf(" %d", sgm_cost(vol[p * D + d], invalid_cost));
        std::printf("\n");
    }
    for (int r = 0; r < n_paths; ++r) {
        int dx, dy;
        sgm_direction(r, dx, dy);
        for (int l = 0; l < sgm_lines(dx, dy, w, h); ++l) {
            int x, y;
            sgm_line_start(dx, dy, w, h, l, x, y);
            for (int t = 0; x >= 0 && x < w && y >= 0 && y < h; ++t, x += dx, y += dy) {
                const size_t p = (size_t)y * w + x;
                int m = -1;
                if (t > 0) {
                    m = prev[0];
                    for (int d = 1; d < D; ++d) m = prev[(size_t)d] < m ? prev[(size_t)d] : m;
                }
                for (int d = 0; d < D; ++d) {
                    const int c = sgm_cost(vol[p * D + d], invalid_cost);
                    L[(size_t)d] = t == 0 ? c
                                          : sgm_step(c, prev[(size_t)d], d > 0 ? prev[(size_t)d - 1] : SGM_FAR, d < D - 1 ? prev[(size_t)d + 1] : SGM_FAR, m, p1, p2);
                }
                std::printf("L %d %d %d %d", r, x, y, m);
                for (int d = 0; d < D; ++d) {
                    std::printf(" %d", L[(size_t)d]);
                    S[p * D + d] = (uint16_t)(S[p * D + d] + L[(size_t)d]);
                }
                std::printf("\n");
                prev = L;
            }
        }
    }
    for (size_t p = 0; p < n_px; ++p) {
        std::printf("S %d %d", (int)(p % w), (int)(p / w));
        for (int d = 0; d < D; ++d) std::printf(" %d", (int)S[p * D + d]);
        std::printf("\n");
    }
    for (size_t p = 0; p < n_px; ++p) {
        int k, best, second, sm = 0, sp = 0;
        sgm_select(&S[p * D], D, k, best, second);
        const bool inner = k > 0 && k < D - 1;
        if (inner) { sm = S[p * D + k - 1]; sp = S[p * D + k + 1]; }
        float z, sc;
        const int q = vol[p * D + k];
        sgm_pixel(wf, step, D, k, best, second, sm, sp, q, uniqueness, z, sc);
        std::printf("O %d %d %d %d %d %d %a %08x %08x %d %d\n", (int)(p % w), (int)(p / w), k, best, second, inner ? sgm_den(sm, best, sp) : 0,
                    inner ? sgm_delta(sm, best, sp) : 0.0, bits(z), bits(sc), sgm_accepted(best, second, uniqueness) ? 1 : 0, q);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    g_f = std::fopen(argv[2], "rb");
    if (!g_f) return 2;
    int rc = 2;
    if (!std::strcmp(argv[1], "quantise")) rc = run_quantise();
    else if (!std::strcmp(argv[1], "delta")) rc = run_delta();
    else if (!std::strcmp(argv[1], "volume")) rc = run_volume();
    std::fclose(g_f);
    return rc;
}
