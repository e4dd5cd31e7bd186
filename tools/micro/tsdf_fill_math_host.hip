// tsdf_fill_math_host.hip -- runs the contract of sfmba_tsdf_fill serially on the HOST through csrc/tsdf_fill_math.h (the arithmetic
// the kernels of tsdf_fill.hip run: the quantisation, one vertex's update, the write-back), so tests/test_tsdf_fill_oracle_cpu.py can
// hold it against the Python restatement without a GPU.  The test builds it with AddressSanitizer and UBSan on the host side:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         -I sfm-toy-library_amd/csrc -o tsdf_fill_math_host tools/micro/tsdf_fill_math_host.hip
//   tsdf_fill_math_host FILE
// FILE: "nx ny nz colour min_weight iterations min_neighbours", then per vertex in lin order "S W" (colour 0) or "S W Sb Sg Sr Wc".
// Output: per vertex "S W Sb Sg Sr Wc state" (zeros for the colour without it), then "filled N".
#include "tsdf_fill_math.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sfmba;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nx, ny, nz, colour, min_weight, iterations, k;
    if (std::fscanf(f, "%d %d %d %d %d %d %d", &nx, &ny, &nz, &colour, &min_weight, &iterations, &k) != 7) return 2;
    const int nvox = nx * ny * nz;
    std::vector<int> S(nvox), W(nvox), CS(3 * (size_t)nvox, 0), CW(nvox, 0);
    for (int l = 0; l < nvox; ++l) {
        if (std::fscanf(f, "%d %d", &S[l], &W[l]) != 2) return 2;
        if (colour && std::fscanf(f, "%d %d %d %d", &CS[3 * l], &CS[3 * l + 1], &CS[3 * l + 2], &CW[l]) != 4) return 2;
    }
    std::fclose(f);

    std::vector<uint64_t> buf[2] = { std::vector<uint64_t>(nvox), std::vector<uint64_t>(nvox) };
    for (int l = 0; l < nvox; ++l) buf[0][l] = buf[1][l] = fill_quantise(S[l], W[l], colour ? &CS[3 * l] : nullptr, CW[l], min_weight);
    for (int p = 1; p <= iterations; ++p) {
        const std::vector<uint64_t>& src = buf[(p - 1) & 1];
        std::vector<uint64_t>& dst = buf[p & 1];
        for (int l = 0; l < nvox; ++l) {
            const int i = l % nx, j = (l / nx) % ny, kk = l / (nx * ny);
            uint64_t nb[6];
            int n = 0;
            if (i > 0) nb[n++] = src[l - 1];
            if (i < nx - 1) nb[n++] = src[l + 1];
            if (j > 0) nb[n++] = src[l - nx];
            if (j < ny - 1) nb[n++] = src[l + nx];
            if (kk > 0) nb[n++] = src[l - nx * ny];
            if (kk < nz - 1) nb[n++] = src[l + nx * ny];
            dst[l] = fill_update(src[l], nb, n, k, p);
        }
    }
    const std::vector<uint64_t>& fin = buf[iterations & 1];
    const int FW = fill_weight(min_weight);
    long long filled = 0;
    for (int l = 0; l < nvox; ++l) {
        if (fill_is_filled(fin[l])) {
            fill_write_back(fin[l], FW, S[l], W[l], &CS[3 * l], CW[l]);
            ++filled;
        }
        std::printf("%d %d %d %d %d %d %d\n", S[l], W[l], CS[3 * l], CS[3 * l + 1], CS[3 * l + 2], CW[l], fill_state(fin[l]));
    }
    std::printf("filled %lld\n", filled);
    return 0;
}
