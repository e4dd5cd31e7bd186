// png_math.h -- the per-byte and per-pixel arithmetic of sfmba_png_decode (the contract is in include/sfmba.h), as
// __host__ __device__ functions: the kernels of png_decode.hip and the serial host program tools/micro/png_math_host.hip run the
// same code, and tests/test_png_oracle_cpu.py holds the host program to the Python restatement (tests/png_oracle.py) byte for
// byte without a GPU.  Everything here is integer arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sfmba {

#define PNG_HD __host__ __device__ __forceinline__

// ---- unfilter -------------------------------------------------------------------------------------------------------------------
// a = the reconstructed byte bpp to the left, b = the one above, c = the one above a; each 0 where it lies outside the image.
PNG_HD int png_abs(int v) { return v < 0 ? -v : v; }
PNG_HD int png_paeth(int a, int b, int c) {
    const int pa = png_abs(b - c), pb = png_abs(a - c), pc = png_abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// The predictor of filter type ft (0..4) as selects, so that the lanes of a wave that hold rows of different types do not diverge.
PNG_HD int png_predict(int ft, int a, int b, int c) {
    const int avg = (a + b) >> 1, paeth = png_paeth(a, b, c);
    int p = 0;
    p = ft == 1 ? a : p;
    p = ft == 2 ? b : p;
    p = ft == 3 ? avg : p;
    p = ft == 4 ? paeth : p;
    return p;
}
PNG_HD int png_unfilter_byte(int ft, int filtered, int a, int b, int c) { return (filtered + png_predict(ft, a, b, c)) & 255; }

// The same on the BYTES bytes of a pixel carried in dwords (byte k of the pixel in bits 8 (k & 3) of word k >> 2).
template <int BYTES> PNG_HD void png_unfilter_pixel(int ft, const unsigned (&x)[(BYTES + 3) / 4], const unsigned (&a)[(BYTES + 3) / 4],
                                                    const unsigned (&b)[(BYTES + 3) / 4], const unsigned (&c)[(BYTES + 3) / 4],
                                                    unsigned (&out)[(BYTES + 3) / 4]) {
    for (int w = 0; w < (BYTES + 3) / 4; ++w) out[w] = 0u;
    for (int k = 0; k < BYTES; ++k) {
        const int w = k >> 2, s = 8 * (k & 3);
        const int r = png_unfilter_byte(ft, (int)((x[w] >> s) & 255u), (int)((a[w] >> s) & 255u), (int)((b[w] >> s) & 255u), (int)((c[w] >> s) & 255u));
        out[w] |= (unsigned)r << s;
    }
}

// ---- samples to pixels ------------------------------------------------------------------------------------------------------------
PNG_HD int png_samples(int colour_type) { return colour_type == 0 || colour_type == 3 ? 1 : colour_type == 4 ? 2 : colour_type == 2 ? 3 : 4; }
PNG_HD int png_out_channels(int colour_type) { return colour_type == 0 || colour_type == 4 ? 1 : 3; }

// Sample i of a reconstructed row (the filter byte not included) as the file states it, a 16-bit one reduced to its high byte.
PNG_HD int png_sample(const unsigned char* row, long long i, int depth) {
    if (depth == 16) return row[2 * i];
    if (depth == 8) return row[i];
    const long long bit = i * depth;
    return (row[bit >> 3] >> (8 - depth - (int)(bit & 7))) & ((1 << depth) - 1);        // packed samples are MSB first
}
PNG_HD int png_gray_scale(int depth) { return depth == 1 ? 255 : depth == 2 ? 85 : depth == 4 ? 17 : 1; }

// Pixel x of a reconstructed row: px[0] (one channel) or px[0..2] = B, G, R.  palette = 256 entries of R, G, B, zero at and past
// the length of PLTE.  Alpha is dropped.
PNG_HD void png_pixel(const unsigned char* row, int x, int colour_type, int depth, const unsigned char* palette, int (&px)[3]) {
    const int samples = png_samples(colour_type);
    const long long s0 = (long long)x * samples;
    if (colour_type == 0 || colour_type == 4) {
        px[0] = px[1] = px[2] = png_sample(row, s0, depth) * png_gray_scale(depth);
    } else if (colour_type == 3) {
        const int index = png_sample(row, s0, depth);
        px[0] = palette[3 * index + 2]; px[1] = palette[3 * index + 1]; px[2] = palette[3 * index];
    } else {
        px[0] = png_sample(row, s0 + 2, depth); px[1] = png_sample(row, s0 + 1, depth); px[2] = png_sample(row, s0, depth);
    }
}

}  // namespace sfmba
