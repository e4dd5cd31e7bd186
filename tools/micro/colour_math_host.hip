// colour_math_host.hip -- runs the contract of the seam levelling serially on the HOST through csrc/colour_math.h (the rules the kernels of
// mesh_colour.hip and the levelled raster of mesh_texture.hip run) and prints EVERY INTERMEDIATE, so tests/test_colour_oracle_cpu.py can
// hold it against the Python restatement without a GPU.  Built with the host sanitizers and run as its own process:
//   hipcc -O1 -std=c++17 -Xarch_host -fsanitize=address,undefined -I sfm-toy-library_amd/csrc -o colour_math_host tools/micro/colour_math_host.hip
//   colour_math_host FILE
// FILE (integers separated by white space; a float is given by its 32 bits as an unsigned integer):
//   mode: 0 a scene, 1 planted nodes
//   scene:   nv nt n_images channels radius weight passes S B; K (9 floats); per image "w h", P (12 floats), h w channels pixels;
//            nv x 3 floats; nt x "a b c"; nt x view
//   planted: n_nodes nt weight passes; n_nodes x "vertex seen F0 F1 F2"; nt x 3 node_of
// Output:
//   K t q key                          the key of every entry (scene)
//   N n vertex view                    the nodes, and "O t n0 n1 n2" the rows of node_of (scene)
//   C n seen sum(3) F(3)               the colour of every node (scene)
//   P pass n c A a B b num den g       every seeing node and channel of every pass, g the NEW offset
//   G n g(3)                           the final offsets
//   X t i j G(3) texel(3) clamped      every sampled texel of the levelled raster (scene)
//   Z stats(8)                         [6] = the clamped texels (scene) or 0 (planted)
#include "colour_math.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sfmba;

static FILE* g_f;
static long long integer() {
    char t[128];
    if (std::fscanf(g_f, "%127s", t) != 1) { std::fprintf(stderr, "short file\n"); std::exit(2); }
    return std::strtoll(t, nullptr, 10);
}
static float real() {
    const uint32_t bits = (uint32_t)integer();
    float f;
    std::memcpy(&f, &bits, sizeof(f));
    return f;
}

struct Image { int w, h; double P[12]; std::vector<unsigned char> px; };

int main(int argc, char** argv) {
    if (argc != 2 || !(g_f = std::fopen(argv[1], "r"))) return 2;
    const int mode = (int)integer();
    int nv = 0, nt = 0, n_images = 0, channels = 3, radius = 0, weight = 1, passes = 0, S = 3, B = 1, n_nodes = 0;
    double k4[4] = { 1, 1, 0, 0 };
    std::vector<Image> img;
    std::vector<float> xyz;
    std::vector<int> tri, view, node_vertex, node_view, node_of, seen;
    std::vector<int> F;
    if (mode == 0) {
        nv = (int)integer(); nt = (int)integer(); n_images = (int)integer(); channels = (int)integer(); radius = (int)integer();
        weight = (int)integer(); passes = (int)integer(); S = (int)integer(); B = (int)integer();
        float K[9];
        for (int i = 0; i < 9; ++i) K[i] = real();
        k4[0] = (double)K[0]; k4[1] = (double)K[4]; k4[2] = (double)K[2]; k4[3] = (double)K[5];
        img.resize((size_t)n_images);
        for (Image& I : img) {
            I.w = (int)integer(); I.h = (int)integer();
            for (int q = 0; q < 12; ++q) I.P[q] = (double)real();
            I.px.resize((size_t)I.w * I.h * channels);
            for (unsigned char& p : I.px) p = (unsigned char)integer();
        }
        xyz.resize((size_t)nv * 3 + 1);
        for (size_t i = 0; i < (size_t)nv * 3; ++i) xyz[i] = real();
        tri.resize((size_t)nt * 3 + 1);
        for (size_t i = 0; i < (size_t)nt * 3; ++i) tri[i] = (int)integer();
        view.resize((size_t)nt + 1);
        for (int t = 0; t < nt; ++t) view[(size_t)t] = (int)integer();
    } else {
        n_nodes = (int)integer(); nt = (int)integer(); weight = (int)integer(); passes = (int)integer();
        node_vertex.resize((size_t)n_nodes + 1); seen.resize((size_t)n_nodes + 1); F.resize((size_t)n_nodes * 3 + 1);
        for (int n = 0; n < n_nodes; ++n) {
            node_vertex[(size_t)n] = (int)integer(); seen[(size_t)n] = integer() != 0;
            for (int c = 0; c < 3; ++c) F[3 * (size_t)n + c] = (int)integer();
        }
        node_of.resize((size_t)nt * 3 + 1);
        for (size_t i = 0; i < (size_t)nt * 3; ++i) node_of[i] = (int)integer();
    }
    std::fclose(g_f);
    const long long N = 3LL * nt;
    auto vertex = [&](int v, double* X) { for (int a = 0; a < 3; ++a) X[a] = (double)xyz[3 * (size_t)v + a]; };
    auto tex_view = [&](int l) { const Image& I = img[(size_t)l]; return TexView{ I.P, nullptr, I.px.data(), I.w, I.h }; };

    if (mode == 0) {
        // ---- nodes: keys, a stable sort, heads, numbers ----
        std::vector<unsigned long long> key((size_t)N + 1);
        std::vector<int> order((size_t)N);
        for (int t = 0; t < nt; ++t) {
            const int* idx = &tri[3 * (size_t)t];
            double A[3], Bv[3], C[3];
            vertex(idx[0], A); vertex(idx[1], Bv); vertex(idx[2], C);
            const bool on = colour_contributes(view[(size_t)t], idx[0], idx[1], idx[2], A, Bv, C);
            for (int q = 0; q < 3; ++q) {
                key[3 * (size_t)t + q] = on ? colour_key(idx[q], view[(size_t)t]) : COLOUR_NO_KEY;
                order[3 * (size_t)t + q] = 3 * t + q;
                std::printf("K %d %d %llu\n", t, q, key[3 * (size_t)t + q]);
            }
        }
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[(size_t)a] < key[(size_t)b]; });
        node_of.assign((size_t)N + 1, -1);
        for (long long i = 0; i < N; ++i) {
            const unsigned long long k = key[(size_t)order[(size_t)i]];
            if (k == COLOUR_NO_KEY) continue;
            if (i == 0 || key[(size_t)order[(size_t)i - 1]] != k) {
                node_vertex.push_back((int)(k >> 32));
                node_view.push_back((int)(k & 0xffffffffULL));
            }
            node_of[(size_t)order[(size_t)i]] = (int)node_vertex.size() - 1;
        }
        n_nodes = (int)node_vertex.size();
        for (int n = 0; n < n_nodes; ++n) std::printf("N %d %d %d\n", n, node_vertex[(size_t)n], node_view[(size_t)n]);
        for (int t = 0; t < nt; ++t) std::printf("O %d %d %d %d\n", t, node_of[3 * (size_t)t], node_of[3 * (size_t)t + 1], node_of[3 * (size_t)t + 2]);
        // ---- colours ----
        seen.assign((size_t)n_nodes + 1, 0);
        F.assign((size_t)n_nodes * 3 + 1, 0);
        for (int n = 0; n < n_nodes; ++n) {
            double X[3];
            vertex(node_vertex[(size_t)n], X);
            long long sum[3];
            seen[(size_t)n] = colour_node(k4, tex_view(node_view[(size_t)n]), channels, X, radius, sum, &F[3 * (size_t)n]);
            std::printf("C %d %d %lld %lld %lld %d %d %d\n", n, seen[(size_t)n], sum[0], sum[1], sum[2], F[3 * (size_t)n], F[3 * (size_t)n + 1], F[3 * (size_t)n + 2]);
        }
    }

    // ---- the passes ----
    std::vector<int> g((size_t)n_nodes * 3 + 1, 0), nxt((size_t)n_nodes * 3 + 1, 0);
    std::vector<std::vector<long long>> entries((size_t)n_nodes + 1);       // of every node, in ascending 3 t + q
    for (long long e = 0; e < N; ++e)
        if (node_of[(size_t)e] >= 0) entries[(size_t)node_of[(size_t)e]].push_back(e);
    for (int p = 0; p < passes; ++p) {
        for (int n = 0; n < n_nodes; ++n) {
            for (int c = 0; c < 3; ++c) nxt[3 * (size_t)n + c] = 0;
            if (!seen[(size_t)n]) continue;
            int lo = n, hi = n + 1, k = 0, b = 0;
            while (lo > 0 && node_vertex[(size_t)lo - 1] == node_vertex[(size_t)n]) --lo;
            while (hi < n_nodes && node_vertex[(size_t)hi] == node_vertex[(size_t)n]) ++hi;
            long long sib[3] = { 0, 0, 0 }, Bs[3] = { 0, 0, 0 };
            for (int m = lo; m < hi; ++m) {
                if (!seen[(size_t)m]) continue;
                for (int c = 0; c < 3; ++c) sib[c] += F[3 * (size_t)m + c] + g[3 * (size_t)m + c];
                ++k;
            }
            for (const long long e : entries[(size_t)n]) {
                const long long t = e / 3, q = e % 3;
                for (int o = 1; o < 3; ++o) {
                    const int u = node_of[(size_t)(3 * t + (q + o) % 3)];
                    if (!seen[(size_t)u]) continue;
                    for (int c = 0; c < 3; ++c) Bs[c] += g[3 * (size_t)u + c];
                    ++b;
                }
            }
            for (int c = 0; c < 3; ++c) {
                long long num, den;
                const int Fn = F[3 * (size_t)n + c];
                nxt[3 * (size_t)n + c] = colour_update(weight, k, sib[c], Fn, b, Bs[c], g[3 * (size_t)n + c], num, den);
                std::printf("P %d %d %d %lld %d %lld %d %lld %lld %d\n", p, n, c, k >= 2 ? sib[c] - (long long)k * Fn : 0LL, k >= 2 ? k : 0, Bs[c], b, num, den,
                            nxt[3 * (size_t)n + c]);
            }
        }
        g.swap(nxt);
    }
    for (int n = 0; n < n_nodes; ++n) std::printf("G %d %d %d %d\n", n, g[3 * (size_t)n], g[3 * (size_t)n + 1], g[3 * (size_t)n + 2]);

    // ---- statistics ----
    long long stats[COLOUR_STATS] = { 0 };
    stats[COLOUR_S_NODES] = n_nodes;
    stats[COLOUR_S_PASSES] = passes;
    for (int n = 0; n < n_nodes; ++n) {
        stats[COLOUR_S_BLIND] += !seen[(size_t)n];
        for (int c = 0; c < 3; ++c) stats[COLOUR_S_MAX_G] = std::max(stats[COLOUR_S_MAX_G], (long long)std::abs(g[3 * (size_t)n + c]));
        if (n > 0 && node_vertex[(size_t)n - 1] == node_vertex[(size_t)n]) continue;
        int k = 0, lo0[3], hi0[3], lo1[3], hi1[3];
        for (int m = n; m < n_nodes && node_vertex[(size_t)m] == node_vertex[(size_t)n]; ++m) {
            if (!seen[(size_t)m]) continue;
            for (int c = 0; c < 3; ++c) {
                const int f = F[3 * (size_t)m + c], fg = f + g[3 * (size_t)m + c];
                lo0[c] = k ? std::min(lo0[c], f) : f; hi0[c] = k ? std::max(hi0[c], f) : f;
                lo1[c] = k ? std::min(lo1[c], fg) : fg; hi1[c] = k ? std::max(hi1[c], fg) : fg;
            }
            ++k;
        }
        if (k < 2) continue;
        ++stats[COLOUR_S_SEAM_VERTICES];
        for (int c = 0; c < 3; ++c) { stats[COLOUR_S_SPREAD_BEFORE] += hi0[c] - lo0[c]; stats[COLOUR_S_SPREAD_AFTER] += hi1[c] - lo1[c]; }
    }

    // ---- the levelled raster: the sampled texels ----
    if (mode == 0) {
        for (int t = 0; t < nt; ++t) {
            if (view[(size_t)t] < 0) continue;
            const TexView V = tex_view(view[(size_t)t]);
            double A[3], Bv[3], C[3];
            vertex(tri[3 * (size_t)t], A); vertex(tri[3 * (size_t)t + 1], Bv); vertex(tri[3 * (size_t)t + 2], C);
            int off[3][3];
            for (int c = 0; c < 3; ++c)
                for (int ch = 0; ch < 3; ++ch) off[c][ch] = node_of[3 * (size_t)t + c] >= 0 ? g[3 * (size_t)node_of[3 * (size_t)t + c] + ch] : 0;
            for (int j = 0; j < S; ++j)
                for (int i = 0; i < S - j; ++i) {
                    double P3[3], q[3], u, v;
                    int su, sv;
                    tex_point(S, i, j, A, Bv, C, P3);
                    if (!tex_texel_coord(k4, V, P3, q, u, v, su, sv)) continue;
                    long long G[3];
                    int px[3];
                    bool clamped = false;
                    for (int ch = 0; ch < 3; ++ch) {
                        G[ch] = colour_blend(S, i, j, off[0][ch], off[1][ch], off[2][ch]);
                        px[ch] = colour_texel(S, tex_sample12(V, channels, ch, su, sv), G[ch], clamped);
                    }
                    stats[COLOUR_S_CLAMPED] += clamped;
                    std::printf("X %d %d %d %lld %lld %lld %d %d %d %d\n", t, i, j, G[0], G[1], G[2], px[0], px[1], px[2], (int)clamped);
                }
        }
    }
    (void)B;
    std::printf("Z");
    for (int i = 0; i < COLOUR_STATS; ++i) std::printf(" %lld", stats[i]);
    std::printf("\n");
    return 0;
}
