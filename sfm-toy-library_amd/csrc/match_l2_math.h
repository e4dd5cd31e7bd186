// match_l2_math.h -- the squared distance of the float matcher's contract (include/sfmba.h, sfmba_match_features_l2), as
// __host__ __device__ functions: the kernel of match_l2.hip and the serial host program tools/micro/match_l2_math_host.hip
// run the same code, and tests/test_match_l2_oracle_cpu.py holds the host program to the numpy restatement bit for bit.
//
//   acc = 0.0f;  for k = 0 .. dims-1 ascending:  t = a[k] - b[k] (one fp32 subtraction);  acc = fmaf(t, t, acc) (one fused op)
//
// IEEE throughout: subnormals kept, nothing reassociated; acc >= +0 always, so its bit pattern as an unsigned integer has the
// order of the value (+inf last), and from finite inputs it is never NaN.  The fma is written out (__builtin_fmaf /
// __builtin_elementwise_fma): the result does not depend on a contraction setting.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sfmba {

#define L2_HD __host__ __device__ __forceinline__

typedef float l2_float2 __attribute__((ext_vector_type(2)));

// one step of the chain for one (query, train) pair
L2_HD float l2_step(float acc, float a, float b) {
    const float t = a - b;
    return __builtin_fmaf(t, t, acc);
}

// the same step for two query rows against one train value: on gfx950 one v_pk_add_f32 (b negated and broadcast) and one
// v_pk_fma_f32; each half is exactly l2_step
L2_HD l2_float2 l2_step2(l2_float2 acc, l2_float2 a, float b) {
    const l2_float2 t = a - (l2_float2)(b);
    return __builtin_elementwise_fma(t, t, acc);
}

L2_HD float l2_sq(const float* a, const float* b, int dims) {
    float acc = 0.0f;
    for (int k = 0; k < dims; ++k) acc = l2_step(acc, a[k], b[k]);
    return acc;
}

// (s, j) -> the key whose unsigned order is the contract's lexicographic (s, j) order
L2_HD unsigned long long l2_key(float s, unsigned j) {
    union { float f; uint32_t u; } c;
    c.f = s;
    return ((unsigned long long)c.u << 32) | j;
}
L2_HD float l2_key_sq(unsigned long long key) {
    union { float f; uint32_t u; } c;
    c.u = (uint32_t)(key >> 32);
    return c.f;
}

// the correctly rounded fp32 square root: the fp64 root of an fp32 value rounds to fp32 without a double-rounding error
// (53 >= 2 * 24 + 2 bits), whatever the fp32 sqrt / denormal settings of the build
L2_HD float l2_dist(float s) { return (float)sqrt((double)s); }

// q is kept iff (double)dist_best < ratio * (double)dist_second
L2_HD bool l2_keep(float dist_best, float dist_second, double ratio) { return (double)dist_best < ratio * (double)dist_second; }

}  // namespace sfmba
