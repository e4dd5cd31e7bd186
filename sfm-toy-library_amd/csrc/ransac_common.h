// ransac_common.h -- what the batched RANSAC units share (pnp_ransac.hip, homography_ransac.hip, essential_ransac.hip): the seeded sampler of their
// contracts (include/sfmba.h) and the wave-wide maximum their select kernels take the winner with.  Plain C++ apart from the
// qualifiers, so a host build can exercise the sampler.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sfmba {

#define PNP_HD __host__ __device__ __forceinline__

// splitmix64's output function (with its increment)
PNP_HD uint64_t pnp_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the first draw from k on (k advances past it) that differs from a, b and c; -1 when the 64 draws are used up
PNP_HD long long pnp_next_draw(uint64_t key, int h, uint64_t n, int& k, long long a, long long b, long long c) {
    while (k < 64) {
        const long long i = (long long)(pnp_mix(key ^ (((uint64_t)(unsigned)h << 8) | (uint64_t)k)) % n);
        ++k;
        if (i != a && i != b && i != c) return i;
    }
    return -1;
}

// The first four distinct indices of the draws mix(key ^ ((h << 8) | k)) mod n, k = 0 .. 63; false when there are fewer.
PNP_HD bool pnp_sample(uint64_t key, int h, long long n, long long& i0, long long& i1, long long& i2, long long& i3) {
    i0 = i1 = i2 = i3 = -1;
    if (n < 4) return false;
    int k = 0;
    i0 = pnp_next_draw(key, h, (uint64_t)n, k, -1, -1, -1);
    i1 = pnp_next_draw(key, h, (uint64_t)n, k, i0, -1, -1);
    i2 = pnp_next_draw(key, h, (uint64_t)n, k, i0, i1, -1);
    i3 = pnp_next_draw(key, h, (uint64_t)n, k, i0, i1, i2);
    return i3 >= 0;
}

// The first six distinct indices of the same draws (sfmba_essential_ransac); false when there are fewer.  No run-time index into
// id: every store is a select, so the array stays in registers.
PNP_HD bool pnp_sample6(uint64_t key, int h, long long n, long long (&id)[6]) {
#pragma unroll
    for (int j = 0; j < 6; ++j) id[j] = -1;
    if (n < 6) return false;
    int got = 0;
    for (int k = 0; k < 64 && got < 6; ++k) {
        const long long i = (long long)(pnp_mix(key ^ (((uint64_t)(unsigned)h << 8) | (uint64_t)k)) % (uint64_t)n);
        bool dup = false;
#pragma unroll
        for (int j = 0; j < 6; ++j) dup = dup || id[j] == i;
        if (dup) continue;
#pragma unroll
        for (int j = 0; j < 6; ++j)
            if (j == got) id[j] = i;
        ++got;
    }
    return got == 6;
}

// the largest value of the wave, in every lane
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(v & 0xffffffffull), off);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

}  // namespace sfmba
