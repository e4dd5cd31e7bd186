// label_math.h -- the rules of the view-label smoothing (the contract is in include/sfmba.h, "smoothing the view labels"), as
// __host__ __device__ functions: the kernels of mesh_labels.hip and the serial host program tools/micro/label_math_host.hip run the
// same code, and tests/test_label_oracle_cpu.py holds the host program to the Python restatement without a GPU.
// EVERYTHING HERE IS INTEGER ARITHMETIC.  A candidate row has LABEL_MAX_K slots in registers whatever the run-time K: every loop runs
// over the constant and is guarded by k < K, so that the compiler unrolls it and no row goes to scratch memory.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sfmba {

#define LABEL_HD __host__ __device__ __forceinline__

constexpr int LABEL_MAX_K = 8;
constexpr int LABEL_MAX_RINGS = 8;
constexpr int LABEL_MAX_PENALTY = 65535;
constexpr int LABEL_MAX_PASSES = 10000;
constexpr int LABEL_D_SCALE = 1024;
constexpr long long LABEL_SCORE_LIMIT = 1LL << 37;       // every score lies below it: (1 + 3)^8 2^37 = 2^53 bounds the diffused sums
constexpr int LABEL_STATS = 8;
// the statistics
enum { LABEL_S_E_START = 0, LABEL_S_E_END, LABEL_S_DIFF_RANK0, LABEL_S_DIFF_START, LABEL_S_DIFF_END, LABEL_S_FRONTIER, LABEL_S_MOVES, LABEL_S_PASSES };
constexpr unsigned long long LABEL_NO_EDGE = ~0ULL;     // the key of an edge of a triangle with a repeated index

// ---- the candidate list ------------------------------------------------------------------------------------------------------
LABEL_HD void label_clear(int* cv, long long* cs) {
    for (int k = 0; k < LABEL_MAX_K; ++k) { cv[k] = -1; cs[k] = 0; }
}
// Views arrive in ascending index with score > 0.  The new entry goes in front of the first entry of a SMALLER score (an equal
// score stays in front: ties go to the lower view index) and everything behind moves down; the K-th entry falls off.
LABEL_HD void label_insert(int K, int* cv, long long* cs, int view, long long score) {
    bool shifting = false;
    for (int k = 0; k < LABEL_MAX_K; ++k) {
        if (k < K && (shifting || score > cs[k])) {
            const int v = cv[k];
            const long long s = cs[k];
            cv[k] = view; cs[k] = score;
            view = v; score = s;
            shifting = true;
        }
    }
}

// ---- adjacency ---------------------------------------------------------------------------------------------------------------
// the key of the edge q of a triangle (a, b, c): (min << 32) | max of its two indices (both >= 0); LABEL_NO_EDGE with a repeated index
LABEL_HD unsigned long long label_edge_key(int a, int b, int c, int q) {
    if (a == b || a == c || b == c) return LABEL_NO_EDGE;
    const int i = q == 0 ? a : (q == 1 ? b : c), j = q == 0 ? b : (q == 1 ? c : a);
    const unsigned long long lo = (unsigned long long)(unsigned)(i < j ? i : j), hi = (unsigned long long)(unsigned)(i < j ? j : i);
    return (lo << 32) | hi;
}
// The entry at position i of the sorted (key, 3 t + q) list of n entries: the triangle across the edge, or -1.  An edge links two
// triangles iff its key occurs EXACTLY twice.
LABEL_HD int label_link(const unsigned long long* keys, const int* vals, long long n, long long i) {
    const unsigned long long k = keys[i];
    if (k == LABEL_NO_EDGE) return -1;
    const bool prev = i > 0 && keys[i - 1] == k, next = i + 1 < n && keys[i + 1] == k;
    if (prev == next) return -1;                          // alone, or in the middle of three
    if (prev) return (i > 1 && keys[i - 2] == k) ? -1 : vals[i - 1] / 3;
    return (i + 2 < n && keys[i + 2] == k) ? -1 : vals[i + 1] / 3;
}
// 0: position i does not begin a run; else the run's length, 3 standing for three or more
LABEL_HD int label_run_head(const unsigned long long* keys, long long n, long long i) {
    const unsigned long long k = keys[i];
    if (k == LABEL_NO_EDGE || (i > 0 && keys[i - 1] == k)) return 0;
    if (!(i + 1 < n && keys[i + 1] == k)) return 1;
    return (i + 2 < n && keys[i + 2] == k) ? 3 : 2;
}

// ---- diffusion ---------------------------------------------------------------------------------------------------------------
// the neighbour's entry for `view`, 0 if the view is not in its list (the first match counts); view >= 0
LABEL_HD long long label_look(int K, const int* nv, const long long* ns, int view) {
    long long r = 0;
    bool found = false;
    for (int j = 0; j < LABEL_MAX_K; ++j)
        if (j < K && !found && nv[j] == view) { r = ns[j]; found = true; }
    return r;
}
// the rank of the largest s among the triangle's candidates, the lowest on a tie; -1 without a candidate
LABEL_HD int label_start_rank(int K, const int* cv, const long long* s) {
    int best = -1;
    long long bs = 0;
    for (int k = 0; k < LABEL_MAX_K; ++k)
        if (k < K && cv[k] >= 0 && (best < 0 || s[k] > bs)) { best = k; bs = s[k]; }
    return best;
}

// ---- relaxation --------------------------------------------------------------------------------------------------------------
// D = floor(1024 (s0 - sk) / s0) with 0 < sk <= s0 < 2^37: 0..1023
LABEL_HD int label_D(long long s0, long long sk) { return (int)(((long long)LABEL_D_SCALE * (s0 - sk)) / s0); }
// e[k] = D[k] + p #{n: view_n >= 0 and view_n != cv[k]} over the three neighbours' views (nview: -1 for no neighbour as well as for a
// neighbour without a view); k* the lowest rank of minimal e; returns gain = e[rank] - e[k*] (0 without a candidate)
LABEL_HD int label_gain(int K, const int* cv, const int* D, int penalty, const int* nview, int rank, int& kstar) {
    kstar = rank;
    if (rank < 0) return 0;
    int best = 0, e_rank = 0;
    bool any = false;
    for (int k = 0; k < LABEL_MAX_K; ++k) {
        if (k < K && cv[k] >= 0) {
            int e = D[k];
            for (int q = 0; q < 3; ++q) e += (nview[q] >= 0 && nview[q] != cv[k]) ? penalty : 0;
            if (!any || e < best) { best = e; kstar = k; any = true; }
            if (k == rank) e_rank = e;
        }
    }
    return e_rank - best;
}
// t moves iff gain_t > 0 and it beats every neighbour n >= 0: gain_t > gain_n, or gain_t == gain_n and t < n
LABEL_HD bool label_moves(int t, int gain_t, const int* n, const int* gain_n) {
    bool m = gain_t > 0;
    for (int q = 0; q < 3; ++q)
        if (n[q] >= 0) m = m && (gain_t > gain_n[q] || (gain_t == gain_n[q] && t < n[q]));
    return m;
}

}  // namespace sfmba
