// png_math_host.hip -- csrc/png_inflate.cpp and the arithmetic of csrc/png_math.h (what the kernels of png_decode.hip run) as a
// serial host program, so that tests/test_png_oracle_cpu.py can hold both to the Python restatement without a GPU.
//   png_math_host decode IN.png OUT.bin     OUT = int32 [8] { status, width, height, channels, bit_depth, colour_type, rowbytes, bpp },
//                                           then, with status 0: the inflated scanline stream [height][1 + rowbytes], the
//                                           reconstructed bytes [height][rowbytes], the pixels [height][width][channels]
// Build: hipcc -O2 -std=c++17 --offload-arch=gfx950 -I sfm-toy-library_amd/csrc tools/micro/png_math_host.hip sfm-toy-library_amd/csrc/png_inflate.cpp
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "png_inflate.h"
#include "png_math.h"

using namespace sfmba;

int main(int argc, char** argv) {
    if (argc != 4 || std::strcmp(argv[1], "decode") != 0) { std::fprintf(stderr, "usage: png_math_host decode IN.png OUT.bin\n"); return 2; }
    std::ifstream in(argv[2], std::ios::binary);
    if (!in) return 2;
    const std::vector<unsigned char> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    PngHeader h;
    int status = png_parse(data.data(), data.size(), &h);
    std::vector<unsigned char> stream;
    if (status == PNG_OK) {
        stream.resize((size_t)h.stream_bytes);
        status = png_inflate_image(data.data(), data.size(), h, stream.data());
    }
    std::ofstream out(argv[3], std::ios::binary);
    int32_t head[8] = { status, 0, 0, 0, 0, 0, 0, 0 };
    if (status != PNG_OK) { out.write(reinterpret_cast<const char*>(head), sizeof(head)); return 0; }
    head[1] = h.width; head[2] = h.height; head[3] = h.channels; head[4] = h.bit_depth; head[5] = h.colour_type; head[6] = (int32_t)h.rowbytes; head[7] = h.bpp;
    out.write(reinterpret_cast<const char*>(head), sizeof(head));
    out.write(reinterpret_cast<const char*>(stream.data()), (std::streamsize)stream.size());
    // the unfilter, byte by byte in raster order
    const size_t rb = (size_t)h.rowbytes, stride = rb + 1;
    std::vector<unsigned char> rec((size_t)h.height * rb);
    for (int y = 0; y < h.height; ++y) {
        const int ft = stream[(size_t)y * stride];
        for (size_t x = 0; x < rb; ++x) {
            const int a = x >= (size_t)h.bpp ? rec[(size_t)y * rb + x - h.bpp] : 0;
            const int b = y > 0 ? rec[(size_t)(y - 1) * rb + x] : 0;
            const int c = y > 0 && x >= (size_t)h.bpp ? rec[(size_t)(y - 1) * rb + x - h.bpp] : 0;
            rec[(size_t)y * rb + x] = (unsigned char)png_unfilter_byte(ft, stream[(size_t)y * stride + 1 + x], a, b, c);
        }
    }
    out.write(reinterpret_cast<const char*>(rec.data()), (std::streamsize)rec.size());
    std::vector<unsigned char> px((size_t)h.width * h.height * h.channels);
    for (int y = 0; y < h.height; ++y)
        for (int x = 0; x < h.width; ++x) {
            int v[3];
            png_pixel(rec.data() + (size_t)y * rb, x, h.colour_type, h.bit_depth, h.palette, v);
            for (int k = 0; k < h.channels; ++k) px[((size_t)y * h.width + x) * h.channels + k] = (unsigned char)v[k];
        }
    out.write(reinterpret_cast<const char*>(px.data()), (std::streamsize)px.size());
    return 0;
}
