// pnp_math_host.hip -- runs the per-lane arithmetic of sfmba_pnp_ransac (csrc/pnp_math.h: sampler, closed-form P3P, fourth-point
// choice) on the HOST, so tests/test_pnp_oracle_cpu.py can hold it against the oracle without a GPU.
//   hipcc -O2 -std=c++17 -I sfm-toy-library_amd/csrc -o pnp_math_host tools/micro/pnp_math_host.hip
//   pnp_math_host FILE      FILE: "n n_hyp seed p fx fy cx cy" then n lines "X Y Z u v"
// prints one line per hypothesis: valid i0 i1 i2 i3 pose[12]
#include "pnp_math.h"

#include <cstdio>
#include <vector>

using namespace sfmba;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long long n;
    int n_hyp, p;
    unsigned long long seed;
    PnpIntrinsics k;
    if (std::fscanf(f, "%lld %d %llu %d %lf %lf %lf %lf", &n, &n_hyp, &seed, &p, &k.fx, &k.fy, &k.cx, &k.cy) != 8) return 2;
    std::vector<double> X(3 * (size_t)n + 1), uv(2 * (size_t)n + 1);
    for (long long i = 0; i < n; ++i)
        if (std::fscanf(f, "%lf %lf %lf %lf %lf", &X[3 * i], &X[3 * i + 1], &X[3 * i + 2], &uv[2 * i], &uv[2 * i + 1]) != 5) return 2;
    std::fclose(f);
    const uint64_t key = pnp_mix((uint64_t)seed + (uint64_t)p);
    for (int h = 0; h < n_hyp; ++h) {
        long long id[4];
        bool ok = pnp_sample(key, h, n, id[0], id[1], id[2], id[3]);
        double pose[12] = { 0 };
        if (ok) {
            double Xs[4][3], us[4][2];
            for (int j = 0; j < 4; ++j) {
                for (int r = 0; r < 3; ++r) Xs[j][r] = X[3 * id[j] + r];
                us[j][0] = uv[2 * id[j]];
                us[j][1] = uv[2 * id[j] + 1];
            }
            ok = pnp_hypothesis(k, Xs, us, pose);
        }
        std::printf("%d %lld %lld %lld %lld", ok ? 1 : 0, id[0], id[1], id[2], id[3]);
        for (int j = 0; j < 12; ++j) std::printf(" %.17g", pose[j]);
        std::printf("\n");
    }
    return 0;
}
