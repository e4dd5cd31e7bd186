// match_l2_math_host.hip -- the arithmetic of csrc/match_l2_math.h (what the kernels of match_l2.hip run) as a serial host program,
// so that tests/test_match_l2_oracle_cpu.py can hold it to the numpy restatement (tests/match_l2_oracle.py) without a GPU.
//   match_l2_math_host rows IN.bin OUT.bin     IN = int32 { n, dims }, then a [n][dims] and b [n][dims] float32.
//                                              OUT = s [n] float32 (l2_sq of row i of a against row i of b, scalar chain), the same
//                                              from the two-query step l2_step2 (rows i and (i + 1) mod n of a against row i of b: the
//                                              first half, [n] float32), dist [n] float32 (l2_dist(s)), keep [n] uint8
//                                              (l2_keep(dist[i], dist[(i + 1) mod n], (double)0.8f))
// Build: hipcc -O2 -std=c++17 --offload-arch=gfx950 -I sfm-toy-library_amd/csrc tools/micro/match_l2_math_host.hip
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "match_l2_math.h"

using namespace sfmba;

int main(int argc, char** argv) {
    if (argc != 4 || std::strcmp(argv[1], "rows") != 0) { std::fprintf(stderr, "usage: match_l2_math_host rows IN.bin OUT.bin\n"); return 2; }
    std::ifstream in(argv[2], std::ios::binary);
    if (!in) return 2;
    int32_t head[2] = { 0, 0 };
    in.read(reinterpret_cast<char*>(head), sizeof(head));
    const int n = head[0], dims = head[1];
    if (!in || n < 1 || dims < 1) return 2;
    std::vector<float> a((size_t)n * dims), b((size_t)n * dims);
    in.read(reinterpret_cast<char*>(a.data()), (std::streamsize)(a.size() * sizeof(float)));
    in.read(reinterpret_cast<char*>(b.data()), (std::streamsize)(b.size() * sizeof(float)));
    if (!in) return 2;
    std::vector<float> s((size_t)n), s2((size_t)n), dist((size_t)n);
    std::vector<unsigned char> keep((size_t)n);
    for (int i = 0; i < n; ++i) {
        const float* ra = &a[(size_t)i * dims];
        const float* rn = &a[(size_t)((i + 1) % n) * dims];
        const float* rb = &b[(size_t)i * dims];
        s[(size_t)i] = l2_sq(ra, rb, dims);
        l2_float2 acc = { 0.0f, 0.0f };
        for (int k = 0; k < dims; ++k) acc = l2_step2(acc, l2_float2{ ra[k], rn[k] }, rb[k]);
        s2[(size_t)i] = acc.x;
        // the key keeps the bits of s
        dist[(size_t)i] = l2_dist(l2_key_sq(l2_key(s[(size_t)i], (unsigned)i)));
    }
    const double ratio = (double)0.8f;
    for (int i = 0; i < n; ++i) keep[(size_t)i] = l2_keep(dist[(size_t)i], dist[(size_t)((i + 1) % n)], ratio) ? 1 : 0;
    std::ofstream out(argv[3], std::ios::binary);
    out.write(reinterpret_cast<const char*>(s.data()), (std::streamsize)(s.size() * sizeof(float)));
    out.write(reinterpret_cast<const char*>(s2.data()), (std::streamsize)(s2.size() * sizeof(float)));
    out.write(reinterpret_cast<const char*>(dist.data()), (std::streamsize)(dist.size() * sizeof(float)));
    out.write(reinterpret_cast<const char*>(keep.data()), (std::streamsize)keep.size());
    return out ? 0 : 2;
}
