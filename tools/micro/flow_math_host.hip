// flow_math_host.hip -- runs the contract of sfmba_flow_track / sfmba_flow_match serially on the HOST through csrc/flow_math.h (the
// arithmetic the kernels of flow_track.hip run), so tests/test_flow_oracle_cpu.py can hold it against the numpy restatement without a GPU.
//   hipcc -O2 -std=c++17 -I sfm-toy-library_amd/csrc -o flow_math_host tools/micro/flow_math_host.hip
//   flow_math_host pyramid FILE    "w h L" and the w * h gray values -> per level "V l w h" and its values on one line
//   flow_math_host template FILE   "w h" and the gray values, then lines "cx cy r" -> the (2r+3)^2 template values on one line
//   flow_math_host track FILE      "n_images L r max_iters min_eig", per image "w h" and its gray values, then "src dst n_pts" and the
//                                  points "x y".  Prints per point "P next_x next_y status err" (floats as 8 hex digits) and per level
//                                  "S l Gxx Gyy Gxy trackable iters dq_x dq_y"
//   flow_math_host match FILE      "n_kp n_q max_err radius ratio", the key points "x y", the queries "x y status err".  Prints
//                                  "M q j distance" (8 hex digits) per match, in query order
// Numbers are read with strtod (hex floats welcome).
#include "flow_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
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

struct Pyramid {
    std::vector<std::vector<unsigned char>> px;
    FlowLevels lv;
};
static bool read_image(int& w, int& h, std::vector<unsigned char>& px) {
    double wh[2];
    if (!nums(wh, 2)) return false;
    w = (int)wh[0]; h = (int)wh[1];
    if (w < 1 || h < 1) return false;
    px.resize((size_t)w * h);
    for (unsigned char& p : px) { double g; if (!num(g)) return false; p = (unsigned char)g; }
    return true;
}
// levels 1 .. FLOW_MAX_LEVELS-1 from level 0 (all of them: the sizes of the unused ones cost nothing here)
static void build(Pyramid& P, int w, int h, std::vector<unsigned char>&& level0, int L) {
    P.px.resize((size_t)L);
    P.px[0] = std::move(level0);
    for (int l = 0; l < L; ++l) {
        P.lv.w[l] = w; P.lv.h[l] = h;
        if (l > 0) {
            P.px[(size_t)l].resize((size_t)w * h);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x)
                    P.px[(size_t)l][(size_t)y * w + x] = (unsigned char)flow_pyr_down(P.px[(size_t)l - 1].data(), P.lv.w[l - 1], P.lv.h[l - 1], x, y);
        }
        P.lv.px[l] = P.px[(size_t)l].data();
        w = flow_half(w); h = flow_half(h);
    }
}

static int run_pyramid() {
    int w, h;
    double hdr[3];
    if (!nums(hdr, 3)) return 2;
    w = (int)hdr[0]; h = (int)hdr[1];
    const int L = (int)hdr[2];
    if (w < 1 || h < 1 || L < 1 || L > FLOW_MAX_LEVELS) return 2;
    std::vector<unsigned char> px((size_t)w * h);
    for (unsigned char& p : px) { double g; if (!num(g)) return 2; p = (unsigned char)g; }
    Pyramid P;
    build(P, w, h, std::move(px), L);
    for (int l = 0; l < L; ++l) {
        std::printf("V %d %d %d", l, P.lv.w[l], P.lv.h[l]);
        for (unsigned char v : P.px[(size_t)l]) std::printf(" %d", (int)v);
        std::printf("\n");
    }
    return 0;
}

static int run_template() {
    int w, h;
    std::vector<unsigned char> px;
    if (!read_image(w, h, px)) return 2;
    double v[3];
    while (nums(v, 3)) {
        const int r = (int)v[2];
        if (r < 1 || r > FLOW_MAX_RADIUS) return 2;
        short T[FLOW_MAX_SIDE * FLOW_MAX_SIDE];
        flow_template(px.data(), w, h, (int)v[0], (int)v[1], r, T);
        for (int c = 0; c < (2 * r + 3) * (2 * r + 3); ++c) std::printf("%d ", (int)T[c]);
        std::printf("\n");
    }
    return 0;
}

static int run_track() {
    double hdr[5];
    if (!nums(hdr, 5)) return 2;
    const int n_images = (int)hdr[0], L = (int)hdr[1], r = (int)hdr[2], max_iters = (int)hdr[3];
    const float min_eig = (float)hdr[4];
    if (n_images < 1 || L < 1 || L > FLOW_MAX_LEVELS || r < 1 || r > FLOW_MAX_RADIUS || max_iters < 1) return 2;
    std::vector<Pyramid> pyr((size_t)n_images);
    for (Pyramid& P : pyr) {
        int w, h;
        std::vector<unsigned char> px;
        if (!read_image(w, h, px)) return 2;
        build(P, w, h, std::move(px), L);
    }
    double job[3];
    if (!nums(job, 3)) return 2;
    const int src = (int)job[0], dst = (int)job[1], n_pts = (int)job[2];
    if (src < 0 || src >= n_images || dst < 0 || dst >= n_images) return 2;
    for (int q = 0; q < n_pts; ++q) {
        double xy[2];
        if (!nums(xy, 2)) return 2;
        float next[2], err;
        unsigned char status;
        FlowLevelState st[FLOW_MAX_LEVELS];
        flow_track_point(pyr[(size_t)src].lv, pyr[(size_t)dst].lv, (float)xy[0], (float)xy[1], L, r, max_iters, min_eig, next, &status, &err, st);
        std::printf("P %08x %08x %d %08x\n", bits(next[0]), bits(next[1]), (int)status, bits(err));
        for (int l = 0; l < L; ++l)
            std::printf("S %d %lld %lld %lld %d %d %d %d\n", l, st[l].Gxx, st[l].Gyy, st[l].Gxy, st[l].trackable, st[l].iters, st[l].dqx, st[l].dqy);
    }
    return 0;
}

static int run_match() {
    double hdr[5];
    if (!nums(hdr, 5)) return 2;
    const int n_kp = (int)hdr[0], n_q = (int)hdr[1];
    const float max_err = (float)hdr[2], radius = (float)hdr[3];
    const double ratio = hdr[4];
    std::vector<float> kp((size_t)n_kp * 2);
    for (float& v : kp) { double d; if (!num(d)) return 2; v = (float)d; }
    std::set<int> taken;
    for (int q = 0; q < n_q; ++q) {
        double v[4];
        if (!nums(v, 4)) return 2;
        const float qx = (float)v[0], qy = (float)v[1], err = (float)v[3];
        if ((int)v[2] == 0 || !(err < max_err)) continue;
        double s1 = 0.0, s2 = 0.0;
        int j1 = -1, in_range = 0;
        for (int j = 0; j < n_kp; ++j) {
            const double s = flow_dist2(qx, qy, kp[(size_t)2 * j], kp[(size_t)2 * j + 1]);
            if (!flow_in_range(s, radius)) continue;
            if (in_range == 0 || s < s1) { s2 = s1; s1 = s; j1 = j; }
            else if (in_range == 1 || s < s2) s2 = s;
            ++in_range;
        }
        if (!flow_candidate(in_range, s1, s2, ratio) || taken.count(j1)) continue;
        taken.insert(j1);
        std::printf("M %d %d %08x\n", q, j1, bits((float)std::sqrt(s1)));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    g_f = std::fopen(argv[2], "rb");
    if (!g_f) return 2;
    if (!std::strcmp(argv[1], "pyramid")) return run_pyramid();
    if (!std::strcmp(argv[1], "template")) return run_template();
    if (!std::strcmp(argv[1], "track")) return run_track();
    if (!std::strcmp(argv[1], "match")) return run_match();
    return 2;
}
