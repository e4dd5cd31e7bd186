// essential_math_host.hip -- runs the arithmetic of sfmba_essential_ransac (csrc/essential_math.h: the six-index sampler of
// ransac_common.h, the five-point hypothesis, the inlier decision, recoverPose in closed form) on the HOST, so
// tests/test_essential_oracle_cpu.py can hold it against the oracle without a GPU.  The work area the device keeps in LDS is a
// plain array here.
//   hipcc -O2 -std=c++17 -I sfm-toy-library_amd/csrc -o essential_math_host tools/micro/essential_math_host.hip
//   essential_math_host FILE      FILE: "n n_hyp seed p threshold_px fx fy cx cy" then n lines "u v u' v'" (pixels)
// prints one line per hypothesis: valid i0 .. i5 nsol E[9] count   (count: ess_inlier over the n correspondences, -1 if invalid)
// then one line for the first hypothesis of the largest count: "pose" best ok count[4] candidate n_front Rp[9] Rm[9] t[3]
#include "essential_math.h"

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
    double thr, kfx, kfy, kcx, kcy;
    if (std::fscanf(f, "%lld %d %llu %d %lf %lf %lf %lf %lf", &n, &n_hyp, &seed, &p, &thr, &kfx, &kfy, &kcx, &kcy) != 9) return 2;
    std::vector<float> c(4 * (size_t)n + 1);
    for (long long i = 0; i < n; ++i)
        if (std::fscanf(f, "%f %f %f %f", &c[4 * i], &c[4 * i + 1], &c[4 * i + 2], &c[4 * i + 3]) != 4) return 2;
    std::fclose(f);
    const float fx = (float)kfx, fy = (float)kfy, cx = (float)kcx, cy = (float)kcy;
    const uint64_t key = pnp_mix((uint64_t)seed + (uint64_t)p);
    const float thr2 = (float)thr * (float)thr;
    std::vector<double> work(ESS_WORK);
    const EssStore<1> w{ work.data() };
    long long best_count = -1;
    int best = -1;
    double bestE[9] = { 0 };
    double bestg[9] = { 0 };
    for (int h = 0; h < n_hyp; ++h) {
        long long id[6];
        bool ok = pnp_sample6(key, h, n, id);
        double E[9] = { 0 };
        int nsol = 0;
        if (ok) {
            double l[12], r[12];
            for (int j = 0; j < 6; ++j) {
                l[2 * j] = ((double)c[4 * id[j]] - (double)cx) / (double)fx;     l[2 * j + 1] = ((double)c[4 * id[j] + 1] - (double)cy) / (double)fy;
                r[2 * j] = ((double)c[4 * id[j] + 2] - (double)cx) / (double)fx; r[2 * j + 1] = ((double)c[4 * id[j] + 3] - (double)cy) / (double)fy;
            }
            ok = ess_hypothesis(w, l, r, E, nsol);
        }
        double g[9];
        ess_pixel_matrix(E, (double)fx, (double)fy, g);
        long long count = ok ? 0 : -1;
        if (ok)
            for (long long i = 0; i < n; ++i)
                count += ess_inlier(g, c[4 * i] - cx, c[4 * i + 1] - cy, c[4 * i + 2] - cx, c[4 * i + 3] - cy, thr2) ? 1 : 0;
        if (count > best_count) {
            best_count = count; best = h;
            for (int j = 0; j < 9; ++j) { bestE[j] = E[j]; bestg[j] = g[j]; }
        }
        std::printf("%d", ok ? 1 : 0);
        for (int j = 0; j < 6; ++j) std::printf(" %lld", id[j]);
        std::printf(" %d", nsol);
        for (int j = 0; j < 9; ++j) std::printf(" %.17g", E[j]);
        std::printf(" %lld\n", count);
    }
    double Rp[9] = { 0 }, Rm[9] = { 0 }, t[3] = { 0 };
    int cnt[4] = { 0, 0, 0, 0 }, cand = -1;
    bool ok = best >= 0 && best_count >= 0 && ess_pose_candidates(bestE, Rp, Rm, t);
    if (ok) {
        for (long long i = 0; i < n; ++i) {
            if (!ess_inlier(bestg, c[4 * i] - cx, c[4 * i + 1] - cy, c[4 * i + 2] - cx, c[4 * i + 3] - cy, thr2)) continue;
            const double x = ((double)c[4 * i] - (double)cx) / (double)fx, y = ((double)c[4 * i + 1] - (double)cy) / (double)fy;
            const double u = ((double)c[4 * i + 2] - (double)cx) / (double)fx, v = ((double)c[4 * i + 3] - (double)cy) / (double)fy;
            cnt[0] += ess_in_front(Rp, t, 1.0, x, y, u, v) ? 1 : 0;
            cnt[1] += ess_in_front(Rm, t, -1.0, x, y, u, v) ? 1 : 0;
            cnt[2] += ess_in_front(Rm, t, 1.0, x, y, u, v) ? 1 : 0;
            cnt[3] += ess_in_front(Rp, t, -1.0, x, y, u, v) ? 1 : 0;
        }
        cand = 0;
        for (int k = 1; k < 4; ++k)
            if (cnt[k] > cnt[cand]) cand = k;
    }
    std::printf("pose %d %d %d %d %d %d %d %d", best, ok ? 1 : 0, cnt[0], cnt[1], cnt[2], cnt[3], cand, cand >= 0 ? cnt[cand] : 0);
    for (int j = 0; j < 9; ++j) std::printf(" %.17g", Rp[j]);
    for (int j = 0; j < 9; ++j) std::printf(" %.17g", Rm[j]);
    for (int j = 0; j < 3; ++j) std::printf(" %.17g", t[j]);
    std::printf("\n");
    return 0;
}
