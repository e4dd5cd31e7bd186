// tsdf_fill_math.h -- the per-vertex arithmetic of sfmba_tsdf_fill / sfmba_tsdf_mesh_fill (the contract is in include/sfmba.h), as
// __host__ __device__ functions: the kernels of tsdf_fill.hip and the serial host program tools/micro/tsdf_fill_math_host.hip run the
// same code, and tests/test_tsdf_fill_oracle_cpu.py holds the host program to the Python restatement bit for bit without a GPU.
// NOTHING BUT INTEGERS: the quantisation of a grid vertex to V and c, one vertex's update in one pass, and the write-back.
//
// THE WORKING STATE OF A VERTEX IS ONE 64-BIT WORD, so a neighbour is one load:
//   bits  0..17   V + 65536 (V in -65536..65536)
//   bit   18      KNOWN (observed, or filled in an earlier pass)
//   bit   19      hasC
//   bits 24..31   the state byte: 0 observed, p in 1..254 the pass in which the vertex became known, 255 unknown
//   bits 32..55   the colour c, one byte per channel
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sfmba {

#define FILL_HD __host__ __device__ __forceinline__

constexpr int FILL_MAX_ITERATIONS = 254;
constexpr int FILL_V_BIAS = 65536;
constexpr uint64_t FILL_KNOWN = 1ull << 18;
constexpr uint64_t FILL_HAS_C = 1ull << 19;
constexpr int FILL_STATE_SHIFT = 24;
constexpr int FILL_COLOUR_SHIFT = 32;
constexpr int FILL_UNKNOWN = 255;

// a / b rounded towards minus infinity, b > 0
FILL_HD long long fill_floor_div(long long a, long long b) {
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// floor_div(a, 2 n) for n in 1..7 and |a| < 2^24, as the passes need it: the divisor is a constant in every branch, so the compiler
// multiplies and shifts where a 64-bit quotient would run a division loop.  The bias keeps the dividend non-negative.
FILL_HD int fill_floor_div_2n(int a, int n) {
    const unsigned K = 1u << 21, b = (unsigned)(a + (int)(2 * n) * (int)K);     // a + 2 n K >= 0, below 2^26
    unsigned q;
    switch (n) {
        case 1: q = b / 2u; break;
        case 2: q = b / 4u; break;
        case 3: q = b / 6u; break;
        case 4: q = b / 8u; break;
        case 5: q = b / 10u; break;
        case 6: q = b / 12u; break;
        default: q = b / 14u; break;
    }
    return (int)q - (int)K;
}

FILL_HD uint64_t fill_pack(int V, bool known, int state, bool has_c, const int* c) {
    uint64_t w = (uint64_t)(unsigned)(V + FILL_V_BIAS) | ((uint64_t)(unsigned)state << FILL_STATE_SHIFT);
    if (known) w |= FILL_KNOWN;
    if (has_c) w |= FILL_HAS_C | ((uint64_t)(unsigned)c[0] << FILL_COLOUR_SHIFT) | ((uint64_t)(unsigned)c[1] << (FILL_COLOUR_SHIFT + 8)) |
                    ((uint64_t)(unsigned)c[2] << (FILL_COLOUR_SHIFT + 16));
    return w;
}
FILL_HD int fill_value(uint64_t w) { return (int)(w & 0x3ffffu) - FILL_V_BIAS; }
FILL_HD bool fill_known(uint64_t w) { return (w & FILL_KNOWN) != 0; }
FILL_HD bool fill_has_colour(uint64_t w) { return (w & FILL_HAS_C) != 0; }
FILL_HD int fill_state(uint64_t w) { return (int)((w >> FILL_STATE_SHIFT) & 0xffu); }
FILL_HD int fill_colour(uint64_t w, int a) { return (int)((w >> (FILL_COLOUR_SHIFT + 8 * a)) & 0xffu); }

// FW = 64 ceil(min_weight / 64): the weight of a filled vertex, 64 .. 65536
FILL_HD int fill_weight(int min_weight) { return 64 * ((min_weight + 63) / 64); }

// The word of a grid vertex before the first pass.  OBSERVED iff W >= min_weight: V = floor_div(128 S + W, 2 W) (64 S / W rounded
// half up), c = (2 Sc + Wc) / (2 Wc) per channel with hasC = (Wc > 0); every other vertex is UNKNOWN.  cs may be NULL (no colour).
FILL_HD uint64_t fill_quantise(int S, int W, const int* cs, int Wc, int min_weight) {
    const int none[3] = { 0, 0, 0 };
    if (W < min_weight) return fill_pack(0, false, FILL_UNKNOWN, false, none);
    const int V = (int)fill_floor_div(128ll * S + W, 2ll * W);
    int c[3] = { 0, 0, 0 };
    const bool has_c = cs && Wc > 0;
    if (has_c)
        for (int a = 0; a < 3; ++a) c[a] = (int)((2ll * cs[a] + Wc) / (2ll * Wc));
    return fill_pack(V, true, 0, has_c, c);
}

// One vertex in pass `pass` (1..254): self and its n_nb face neighbours that exist (at most 6) as they were before the pass.  An
// observed vertex never changes; an unknown one becomes known iff n6 >= min_neighbours; a filled one is updated in every pass.
// V' = floor_div(2 sum V + n, 2 n) over the known face neighbours and the vertex itself if it was known; the colour likewise over
// the m terms with hasC.  |sum V| <= 7 * 65536: int32.
FILL_HD uint64_t fill_update(uint64_t self, const uint64_t* nb, int n_nb, int min_neighbours, int pass) {
    if (fill_state(self) == 0) return self;
    int n = 0, m = 0, sum = 0, cs[3] = { 0, 0, 0 };
    for (int q = 0; q < n_nb; ++q) {
        const uint64_t w = nb[q];
        if (!fill_known(w)) continue;
        ++n;
        sum += fill_value(w);
        if (fill_has_colour(w)) {
            ++m;
            for (int a = 0; a < 3; ++a) cs[a] += fill_colour(w, a);
        }
    }
    const bool was = fill_known(self);
    if (!was && n < min_neighbours) return self;
    if (was) {
        ++n;
        sum += fill_value(self);
        if (fill_has_colour(self)) {
            ++m;
            for (int a = 0; a < 3; ++a) cs[a] += fill_colour(self, a);
        }
    }
    const int V = fill_floor_div_2n(2 * sum + n, n);
    int c[3] = { 0, 0, 0 };
    if (m > 0)
        for (int a = 0; a < 3; ++a) c[a] = fill_floor_div_2n(2 * cs[a] + m, m);
    return fill_pack(V, true, was ? fill_state(self) : pass, m > 0, c);
}

// A vertex is FILLED iff its state is 1..254; the write-back of such a vertex: W = FW, S = V (FW / 64), csum = c and cweight = 1 if
// hasC, else zeros.  Every other vertex keeps its input bits (the caller copies them).
FILL_HD bool fill_is_filled(uint64_t w) { const int s = fill_state(w); return s >= 1 && s <= FILL_MAX_ITERATIONS; }
FILL_HD void fill_write_back(uint64_t w, int FW, int& S, int& W, int* cs, int& Wc) {
    S = fill_value(w) * (FW / 64);
    W = FW;
    const bool has_c = fill_has_colour(w);
    for (int a = 0; a < 3; ++a) cs[a] = has_c ? fill_colour(w, a) : 0;
    Wc = has_c ? 1 : 0;
}

}  // namespace sfmba
