// jpeg_math.h -- the per-block and per-pixel arithmetic of sfmba_jpeg_decode and sfmba_resize_images (the contract is in
// include/sfmba.h), as __host__ __device__ functions: the kernels of jpeg_decode.hip and the serial host program
// tools/micro/jpeg_math_host.hip run the same code, and tests/test_jpeg_oracle_cpu.py holds the host program to the Python
// restatement (tests/jpeg_oracle.py) bit for bit without a GPU.  Everything here is integer arithmetic; the only doubles are
// those of the resize tables, which are built on the host alone (resize_axis_entry) so that no device contraction can change
// a weight.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace sfmba {

#define JPEG_HD __host__ __device__ __forceinline__

constexpr int JPEG_MAX_SIDE = 16384;        // of a decoded image and of a resized one
constexpr int JPEG_CONST_BITS = 13;
constexpr int JPEG_PASS1_BITS = 2;

// ---- inverse DCT ----------------------------------------------------------------------------------------------------------
// (x + 2^(n-1)) >> n on 32-bit two's complement; the sum wraps (it is formed unsigned), the shift is arithmetic
JPEG_HD int jpeg_descale(unsigned x, int n) { return (int)(x + (1u << (n - 1))) >> n; }

// One 8-point pass of the "islow" transform: in[0..7] -> out[0..7], each output descaled by `shift` bits.  All sums and products
// are formed in unsigned arithmetic: they wrap like 32-bit two's complement and are never undefined, whatever the coefficients.
JPEG_HD void jpeg_idct_1d(const int (&in)[8], int shift, int (&out)[8]) {
    const unsigned i0 = (unsigned)in[0], i1 = (unsigned)in[1], i2 = (unsigned)in[2], i3 = (unsigned)in[3];
    const unsigned i4 = (unsigned)in[4], i5 = (unsigned)in[5], i6 = (unsigned)in[6], i7 = (unsigned)in[7];
    // even part
    unsigned z1 = (i2 + i6) * 4433u;
    const unsigned e2 = z1 - i6 * 15137u;
    const unsigned e3 = z1 + i2 * 6270u;
    const unsigned e0 = (i0 + i4) << JPEG_CONST_BITS;
    const unsigned e1 = (i0 - i4) << JPEG_CONST_BITS;
    const unsigned t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    // odd part
    unsigned o0 = i7, o1 = i5, o2 = i3, o3 = i1;
    z1 = o0 + o3;
    unsigned z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const unsigned z5 = (z3 + z4) * 9633u;
    o0 *= 2446u; o1 *= 16819u; o2 *= 25172u; o3 *= 12299u;
    z1 *= 0u - 7373u; z2 *= 0u - 20995u; z3 *= 0u - 16069u; z4 *= 0u - 3196u;
    z3 += z5; z4 += z5;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    out[0] = jpeg_descale(t10 + o3, shift); out[7] = jpeg_descale(t10 - o3, shift);
    out[1] = jpeg_descale(t11 + o2, shift); out[6] = jpeg_descale(t11 - o2, shift);
    out[2] = jpeg_descale(t12 + o1, shift); out[5] = jpeg_descale(t12 - o1, shift);
    out[3] = jpeg_descale(t13 + o0, shift); out[4] = jpeg_descale(t13 - o0, shift);
}

// column pass: coefficient x quantiser in, DESCALE(., 11) out; row pass: DESCALE(., 18), then the level shift and the clamp
JPEG_HD void jpeg_idct_column(const int (&coef_times_q)[8], int (&out)[8]) { jpeg_idct_1d(coef_times_q, JPEG_CONST_BITS - JPEG_PASS1_BITS, out); }
JPEG_HD int jpeg_clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
JPEG_HD void jpeg_idct_row(const int (&ws)[8], int (&sample)[8]) {
    jpeg_idct_1d(ws, JPEG_CONST_BITS + JPEG_PASS1_BITS + 3, sample);
    for (int i = 0; i < 8; ++i) sample[i] = jpeg_clamp255((int)((unsigned)sample[i] + 128u));
}
JPEG_HD int jpeg_dequant(int coef, int q) { return (int)((unsigned)coef * (unsigned)q); }

// ---- chroma upsampling: the triangle filter ---------------------------------------------------------------------------------
// Output column x of a row of cw samples doubled horizontally (h2v1).
JPEG_HD int jpeg_up_h2v1(const unsigned char* row, int cw, int x) {
    const int i = x >> 1;
    if (x & 1) return i == cw - 1 ? row[i] : (3 * row[i] + row[i + 1] + 2) >> 2;
    return i == 0 ? row[0] : (3 * row[i] + row[i - 1] + 1) >> 2;
}
// Output (x, y) of a cw x ch component doubled both ways (h2v2); `plane` has `stride` bytes per row.
JPEG_HD int jpeg_up_h2v2(const unsigned char* plane, int stride, int cw, int ch, int x, int y) {
    const int r = y >> 1, i = x >> 1;
    int rf = (y & 1) ? r + 1 : r - 1;
    rf = rf < 0 ? 0 : rf > ch - 1 ? ch - 1 : rf;
    const unsigned char* near = plane + (size_t)r * stride;
    const unsigned char* far = plane + (size_t)rf * stride;
    const int s = 3 * near[i] + far[i];
    if (x & 1) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + (3 * near[i + 1] + far[i + 1]) + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + (3 * near[i - 1] + far[i - 1]) + 8) >> 4;
}

// ---- colour -----------------------------------------------------------------------------------------------------------------
JPEG_HD void jpeg_ycc_to_bgr(int y, int cb, int cr, int& b, int& g, int& r) {
    cb -= 128; cr -= 128;
    r = jpeg_clamp255(y + ((91881 * cr + 32768) >> 16));
    b = jpeg_clamp255(y + ((116130 * cb + 32768) >> 16));
    g = jpeg_clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
}

// ---- resize -----------------------------------------------------------------------------------------------------------------
struct ResizeEntry { int32_t index, w1; };       // source index (the next one is min(index + 1, n - 1)) and the 11-bit weight of it

// lrint(n f) in double, f a float widened; 0 when the result lies outside 1..JPEG_MAX_SIDE (the call is then refused)
inline int resized_length(int n, float factor) {
    const double v = (double)n * (double)factor;
    if (!(v >= 0.0) || v > 1e9) return 0;
    const long r = std::lrint(v);
    return r >= 1 && r <= JPEG_MAX_SIDE ? (int)r : 0;
}
// Entry d of the table of one axis: source length n, inv = 1 / (double)factor.  HOST only.
inline ResizeEntry resize_axis_entry(int d, int n, double inv) {
    const double f = ((double)d + 0.5) * inv - 0.5;
    double fl = std::floor(f);
    double a = f - fl;
    long s = (long)fl;
    if (fl < 0.0) { s = 0; a = 0.0; }
    if (fl >= (double)(n - 1)) { s = n - 1; a = 0.0; }
    ResizeEntry e;
    e.index = (int32_t)s;
    e.w1 = (int32_t)std::lrint(2048.0 * a);
    return e;
}
JPEG_HD int resize_value(int p00, int p01, int p10, int p11, int wx1, int wy1) {
    const int wx0 = 2048 - wx1, wy0 = 2048 - wy1;
    return (wy0 * (wx0 * p00 + wx1 * p01) + wy1 * (wx0 * p10 + wx1 * p11) + (1 << 21)) >> 22;        // < 2^31
}
// Byte c of output pixel (x, y) of a w x h image of `channels` interleaved bytes.
JPEG_HD int resize_pixel(const unsigned char* src, int w, int h, int channels, const ResizeEntry* xt, const ResizeEntry* yt, int x, int y, int c) {
    const ResizeEntry ex = xt[x], ey = yt[y];
    const int x1 = ex.index + 1 < w - 1 ? ex.index + 1 : w - 1, y1 = ey.index + 1 < h - 1 ? ey.index + 1 : h - 1;
    const unsigned char* r0 = src + (size_t)ey.index * w * channels + c;
    const unsigned char* r1 = src + (size_t)y1 * w * channels + c;
    return resize_value(r0[(size_t)ex.index * channels], r0[(size_t)x1 * channels], r1[(size_t)ex.index * channels], r1[(size_t)x1 * channels], ex.w1, ey.w1);
}

}  // namespace sfmba
