// match_l2.hip -- SfM2DFeatureUtilities::matchFeatures for FLOAT descriptors (SIFT, SURF, RootSIFT, learned ones; what
// cv::BFMatcher serves with NORM_L2) for a whole list of image pairs on the MI355X (gfx950).
//
// The squared distance is defined operation by operation (include/sfmba.h, sfmba_match_features_l2; match_l2_math.h): a chain
// of one fp32 subtraction and one fused fp32 multiply-add per column, in ascending column order.  So the result is BIT-EXACT
// with a CPU restatement, and it is the DIFFERENCE form on the vector ALU: |a|^2 + |b|^2 - 2 a.b cancels exactly where the near
// matches are, and no matrix-core form reproduces the chain.  The shape is that of feature_match.hip:
//
//   upload    the rows once per call, zero-padded to a multiple of 32 floats (a padded column gives t = 0 and fmaf(0, 0, acc)
//             = acc exactly, acc being >= +0 or +inf: the padding changes no bit of any distance).
//   top-2     k_l2_top2: grid = (query tile of a pair) x (train slice), a batch of tiles per launch.  A lane holds two query
//             rows INTERLEAVED in VGPRs (column k of both in one 64-bit register pair), 64 columns at a time; the block stages
//             8192 / padded dims (256 .. 16) train rows of its slice at a time in LDS (32 KiB), the 4-column blocks of all
//             rows side by side, and every lane reads the same block (a ds_read_b128 broadcast, 8 rows' blocks in flight).
//             The chain of one (q, j) is serial, so a lane runs 16 train rows x 2 queries = 32 independent accumulators: per
//             column and train row one v_pk_add_f32 (the train value negated and broadcast to both halves through op_sel) and
//             one v_pk_fma_f32, each half being one query's own chain in ascending k.  Up to 64 columns the query rows are
//             loaded once per block (k_l2_top2<true>); above, the lane reloads its 64-column window per group of 16 train
//             rows (k_l2_top2<false>; the rows come from L2).  212 / 224 VGPRs, no scratch: two waves per SIMD.  s >= +0, so the bits of s order as s does: the pair (s, j) is the 64-bit key (bits(s) << 32) | j
//             and the top-2 update is branch-free: b2 = min(b2, max(b1, k)); b1 = min(b1, k).
//   merge     k_l2_merge: the 2 smallest keys over the slices with the same update (a total order: the result does not
//             depend on the slice count or on arrival order -- deterministic by construction, no atomics), the two square
//             roots (the only ones taken), then the ratio test in double.
//   compact   an inclusive scan of the kept flags over all query rows of the call (hipCUB) gives the CSR positions; one
//             scatter writes (query, train, distance) in ascending query order inside a pair, pairs in list order.
//
// The per-slice keys of a batch live in a scratch buffer bounded by MATCH_L2_SCRATCH_BYTES whatever the number of pairs.
#include "match_l2.h"
#include "match_l2_math.h"
#include "device_arena.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;              // threads per block; a lane holds query rows q0 + lane and q0 + lane + 256
constexpr int KP = 64;                  // columns of the two query rows a lane holds in VGPRs at a time
constexpr int GROUP = MATCH_L2_GROUP;
constexpr int HALF = 8;                 // train rows whose 4-column blocks are read together
static_assert(MATCH_L2_TILE == 2 * LANES, "two queries per lane");
static_assert(KP % MATCH_L2_PAD == 0 && MATCH_L2_PAD % 4 == 0, "column blocks");
typedef unsigned long long u64;

struct L2Pair {
    long long qoff, toff;               // first descriptor row of the query (left) / train (right) image
    long long row0;                     // first query row of the pair in the call's row numbering
    int nq, nt;
};
struct L2Item { int pair, q0; };        // one query tile

__device__ __forceinline__ void top2(u64& b1, u64& b2, u64 k) {
    b2 = min(b2, max(b1, k));
    b1 = min(b1, k);
}

// columns kp .. kp + KP - 1 (those below dp) of the lane's two query rows, interleaved
__device__ __forceinline__ void load_queries(const float* __restrict__ ra, const float* __restrict__ rb, int dp, int kp, l2_float2 (&aq)[KP]) {
#pragma unroll
    for (int kb = 0; kb < KP / MATCH_L2_PAD; ++kb) {
        if (kp + MATCH_L2_PAD * kb < dp) {
#pragma unroll
            for (int k = MATCH_L2_PAD * kb; k < MATCH_L2_PAD * (kb + 1); k += 4) {
                const float4 x = *reinterpret_cast<const float4*>(ra + kp + k);
                const float4 y = *reinterpret_cast<const float4*>(rb + kp + k);
                aq[k] = l2_float2{ x.x, y.x }; aq[k + 1] = l2_float2{ x.y, y.y };
                aq[k + 2] = l2_float2{ x.z, y.z }; aq[k + 3] = l2_float2{ x.w, y.w };
            }
        }
    }
}

// keys[s * slice_stride + item * TILE + lane (+ 256)] = the two smallest keys of the query row over train slice s.
// dp = the padded row length (a multiple of 32), stage_rows = train rows per LDS stage (a multiple of GROUP, stage_rows * dp <= 8192).
template <bool SINGLE>
__global__ __launch_bounds__(LANES) void k_l2_top2(const float* __restrict__ desc, int dp, int stage_rows, const L2Pair* __restrict__ pairs,
                                                   const L2Item* __restrict__ items, int n_slices, long long slice_stride,
                                                   ulonglong2* __restrict__ keys) {
    __shared__ float4 sh4[MATCH_L2_STAGE_FLOATS / 4];
    const L2Item it = items[blockIdx.x];
    const L2Pair P = pairs[it.pair];
    const int s = blockIdx.y;
    const int len = (P.nt + n_slices - 1) / n_slices;
    const int t0 = min(P.nt, s * len), t1 = min(P.nt, t0 + len);
    const int qa = it.q0 + threadIdx.x, qb = qa + LANES;
    // a lane past the pair's last query row reads the last row again: it computes, and the merge never looks at its keys
    const float* ra = desc + (P.qoff + min(qa, P.nq - 1)) * dp;
    const float* rb = desc + (P.qoff + min(qb, P.nq - 1)) * dp;
    l2_float2 aq[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) aq[k] = l2_float2{ 0.f, 0.f };
    if (SINGLE) load_queries(ra, rb, dp, 0, aq);       // SINGLE: dp <= KP, the whole row fits the registers and is loaded once
    u64 a1 = ~0ull, a2 = ~0ull, b1 = ~0ull, b2 = ~0ull;
    for (int c = t0; c < t1; c += stage_rows) {
        const int n = min(stage_rows, t1 - c);
        __syncthreads();                                   // the previous stage has been read by every wave
        {
            // n rows of the slice are contiguous in memory; in LDS the 4-column blocks of all rows lie side by side
            // (sh4[k4 * stage_rows + row]), so the GROUP rows of one block are one run of immediate offsets
            const float4* src = reinterpret_cast<const float4*>(desc + (P.toff + c) * dp);
            const int d4 = dp / 4, n4 = n * d4;            // n4 <= 2048
            for (int i = threadIdx.x; i < n4; i += LANES) sh4[(i % d4) * stage_rows + i / d4] = src[i];
        }
        __syncthreads();
        for (int g = 0; g < n; g += GROUP) {               // rows g + j >= n of the last group: computed from stale LDS, never used
            l2_float2 acc[GROUP];
#pragma unroll
            for (int j = 0; j < GROUP; ++j) acc[j] = l2_float2{ 0.f, 0.f };
            for (int kp = 0; kp < dp; kp += KP) {
                if (!SINGLE) load_queries(ra, rb, dp, kp, aq);
                const float4* base = sh4 + (kp / 4) * stage_rows + g;
#pragma unroll
                for (int kb = 0; kb < KP / MATCH_L2_PAD; ++kb) {
                    if (kp + MATCH_L2_PAD * kb < dp) {
#pragma unroll
                        for (int k = MATCH_L2_PAD * kb; k < MATCH_L2_PAD * (kb + 1); k += 4) {
                            const float4* row = base + (k / 4) * stage_rows;
#pragma unroll
                            for (int h = 0; h < GROUP; h += HALF) {
                                float t[HALF][4];
#pragma unroll
                                for (int j = 0; j < HALF; ++j) {
                                    const float4 v = row[h + j];         // same address in every lane: broadcast
                                    t[j][0] = v.x; t[j][1] = v.y; t[j][2] = v.z; t[j][3] = v.w;
                                }
#pragma unroll
                                for (int kk = 0; kk < 4; ++kk)           // HALF independent chains side by side, each ascending in k
#pragma unroll
                                    for (int j = 0; j < HALF; ++j) acc[h + j] = l2_step2(acc[h + j], aq[k + kk], t[j][kk]);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < GROUP; ++j) {
                if (g + j < n) {
                    const unsigned jj = (unsigned)(c + g + j);
                    top2(a1, a2, l2_key(acc[j].x, jj));
                    top2(b1, b2, l2_key(acc[j].y, jj));
                }
            }
        }
    }
    ulonglong2* out = keys + (size_t)s * (size_t)slice_stride + (size_t)blockIdx.x * MATCH_L2_TILE + threadIdx.x;
    out[0] = make_ulonglong2(a1, a2);
    out[LANES] = make_ulonglong2(b1, b2);
}

// Merge over the slices + ratio test: best_t[row] = train index, best_d[row] = distance, flag[row] = kept, qidx[row] = query
// index.  Only tiles of pairs with >= 2 train rows are launched, so the second key is always a real one.
__global__ __launch_bounds__(LANES) void k_l2_merge(const L2Pair* __restrict__ pairs, const L2Item* __restrict__ items, int n_slices,
                                                    long long slice_stride, const ulonglong2* __restrict__ keys, double ratio,
                                                    int* __restrict__ best_t, float* __restrict__ best_d, int* __restrict__ flag,
                                                    int* __restrict__ qidx) {
    const L2Item it = items[blockIdx.x];
    const L2Pair P = pairs[it.pair];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int q = it.q0 + threadIdx.x + h * LANES;
        if (q >= P.nq) continue;
        const size_t slot = (size_t)blockIdx.x * MATCH_L2_TILE + threadIdx.x + h * LANES;
        u64 k1 = ~0ull, k2 = ~0ull;
        for (int s = 0; s < n_slices; ++s) {
            const ulonglong2 v = keys[(size_t)s * (size_t)slice_stride + slot];
            top2(k1, k2, v.x);
            top2(k1, k2, v.y);
        }
        const float d1 = l2_dist(l2_key_sq(k1)), d2 = l2_dist(l2_key_sq(k2));
        const long long row = P.row0 + q;
        best_t[row] = (int)(k1 & 0xffffffffull);
        best_d[row] = d1;
        flag[row] = l2_keep(d1, d2, ratio) ? 1 : 0;
        qidx[row] = q;
    }
}

// pos[0..n_rows] = exclusive positions (pos[0] = 0, pos[n_rows] = total); pair_ptr[p] = pos[prow[p]].
__global__ __launch_bounds__(256) void k_l2_pair_ptr(int n, const long long* __restrict__ prow, const int* __restrict__ pos,
                                                     long long* __restrict__ pair_ptr) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p <= n) pair_ptr[p] = pos[prow[p]];
}

__global__ __launch_bounds__(256) void k_l2_scatter(long long n_rows, const int* __restrict__ flag, const int* __restrict__ pos,
                                                    const int* __restrict__ best_t, const float* __restrict__ best_d,
                                                    const int* __restrict__ qidx, long long cap,
                                                    int* __restrict__ out_q, int* __restrict__ out_t, float* __restrict__ out_d) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows || !flag[r]) return;
    const long long o = pos[r];
    if (o >= cap) return;
    out_q[o] = qidx[r];
    out_t[o] = best_t[r];
    out_d[o] = best_d[r];
}

unsigned grid_for(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int match_features_l2(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const float* desc, int dims,
                      int n_pairs, const int32_t* pair_left, const int32_t* pair_right, double ratio, int64_t* pair_ptr,
                      int32_t* query_idx, int32_t* train_idx, float* distance, int64_t cap, int64_t* total, double* timing) {
    for (int p = 0; p <= n_pairs; ++p) pair_ptr[p] = 0;
    *total = 0;
    if (timing) for (int i = 0; i < 5; ++i) timing[i] = 0.0;
    // pairs, query rows (only pairs that can keep anything: >= 2 train rows) and query tiles
    std::vector<L2Pair> pairs((size_t)std::max(n_pairs, 1));
    std::vector<long long> prow((size_t)n_pairs + 1, 0);
    std::vector<L2Item> items;
    long long n_rows = 0;
    for (int p = 0; p < n_pairs; ++p) {
        L2Pair& P = pairs[(size_t)p];
        const int l = pair_left[p], r = pair_right[p];
        P.qoff = img_ptr[l]; P.toff = img_ptr[r];
        P.nq = (int)(img_ptr[l + 1] - img_ptr[l]); P.nt = (int)(img_ptr[r + 1] - img_ptr[r]);
        if (P.nt < 2) P.nq = 0;                  // no second neighbour: nothing is kept (include/sfmba.h)
        P.row0 = n_rows;
        prow[(size_t)p] = n_rows;
        n_rows += P.nq;
        for (int q0 = 0; q0 < P.nq; q0 += MATCH_L2_TILE) items.push_back(L2Item{ p, q0 });
    }
    prow[(size_t)n_pairs] = n_rows;
    if (n_rows == 0) return 0;

    DeviceArena scratch(device);
    const int dp = (dims + MATCH_L2_PAD - 1) / MATCH_L2_PAD * MATCH_L2_PAD;
    const int stage_rows = std::min(256, MATCH_L2_STAGE_FLOATS / dp / GROUP * GROUP);     // 256 at dp = 32 .. 16 at dp = 512
    const long long n_desc = img_ptr[n_images];
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    // allocations first (the arena zeroes them), then the stream work
    const int n_items = (int)items.size();
    const int n_batches = (n_items + MATCH_L2_BATCH_TILES - 1) / MATCH_L2_BATCH_TILES;
    std::vector<int> slices((size_t)n_batches);
    long long key_slots = 0;
    for (int b = 0; b < n_batches; ++b) {
        const int i0 = b * MATCH_L2_BATCH_TILES, i1 = std::min(n_items, i0 + MATCH_L2_BATCH_TILES), nb = i1 - i0;
        int max_nt = 0;
        for (int i = i0; i < i1; ++i) max_nt = std::max(max_nt, pairs[(size_t)items[(size_t)i].pair].nt);
        const int by_rows = std::max(1, (max_nt + MATCH_L2_MIN_SLICE_ROWS - 1) / MATCH_L2_MIN_SLICE_ROWS);
        const int by_fill = (MATCH_L2_TARGET_BLOCKS + nb - 1) / nb;
        slices[(size_t)b] = std::max(1, std::min(std::min(by_fill, by_rows), MATCH_L2_MAX_SLICES));
        key_slots = std::max(key_slots, (long long)slices[(size_t)b] * nb * MATCH_L2_TILE);
    }
    float* d_desc;
    L2Pair* d_pairs;
    L2Item* d_items;
    ulonglong2* d_keys;
    float* d_bestd;
    int *d_bestt, *d_flag, *d_pos, *d_qidx;
    long long *d_prow, *d_pptr;
    UNIT_ALLOC(scratch, d_desc, float, (size_t)std::max(n_desc, 1ll) * dp);
    UNIT_ALLOC(scratch, d_pairs, L2Pair, pairs.size());
    UNIT_ALLOC(scratch, d_items, L2Item, items.size());
    UNIT_ALLOC(scratch, d_keys, ulonglong2, (size_t)key_slots);
    UNIT_ALLOC(scratch, d_bestt, int, (size_t)n_rows);
    UNIT_ALLOC(scratch, d_bestd, float, (size_t)n_rows);
    UNIT_ALLOC(scratch, d_flag, int, (size_t)n_rows);
    UNIT_ALLOC(scratch, d_qidx, int, (size_t)n_rows);
    UNIT_ALLOC(scratch, d_pos, int, (size_t)n_rows + 1);
    UNIT_ALLOC(scratch, d_prow, long long, prow.size());
    UNIT_ALLOC(scratch, d_pptr, long long, prow.size());
    size_t tmp_bytes = 0;
    UNIT_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_bytes, d_flag, d_pos + 1, (int)n_rows, s));
    void* d_tmp = scratch.alloc(tmp_bytes ? tmp_bytes : 1);
    if (!d_tmp) return (int)hipErrorOutOfMemory;
    const long long ocap = std::min<long long>(std::max<long long>(cap, 0), n_rows);
    int *d_oq, *d_ot;
    float* d_od;
    UNIT_ALLOC(scratch, d_oq, int, (size_t)std::max(ocap, 1ll));
    UNIT_ALLOC(scratch, d_ot, int, (size_t)std::max(ocap, 1ll));
    UNIT_ALLOC(scratch, d_od, float, (size_t)std::max(ocap, 1ll));

    // upload: rows of exactly dp floats go as they are, others are padded with zeros on the host
    tm.begin(0);
    std::vector<float> padded;
    if (n_desc > 0) {
        if (dims == dp) {
            UNIT_TRY(hipMemcpyAsync(d_desc, desc, (size_t)n_desc * dp * sizeof(float), hipMemcpyHostToDevice, s));
        } else {
            padded.assign((size_t)n_desc * dp, 0.0f);
            for (long long i = 0; i < n_desc; ++i) std::memcpy(&padded[(size_t)i * dp], desc + (size_t)i * dims, (size_t)dims * sizeof(float));
            UNIT_TRY(hipMemcpyAsync(d_desc, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice, s));
        }
    }
    UNIT_TRY(hipMemcpyAsync(d_pairs, pairs.data(), sizeof(L2Pair) * pairs.size(), hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_items, items.data(), sizeof(L2Item) * items.size(), hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_prow, prow.data(), sizeof(long long) * prow.size(), hipMemcpyHostToDevice, s));
    tm.next(1);

    for (int b = 0; b < n_batches; ++b) {
        const int i0 = b * MATCH_L2_BATCH_TILES, nb = std::min(n_items, i0 + MATCH_L2_BATCH_TILES) - i0;
        const long long stride = (long long)nb * MATCH_L2_TILE;
        const dim3 grid((unsigned)nb, (unsigned)slices[(size_t)b]);
        if (dp <= KP) hipLaunchKernelGGL(k_l2_top2<true>, grid, dim3(LANES), 0, s, d_desc, dp, stage_rows, d_pairs, d_items + i0, slices[(size_t)b], stride, d_keys);
        else          hipLaunchKernelGGL(k_l2_top2<false>, grid, dim3(LANES), 0, s, d_desc, dp, stage_rows, d_pairs, d_items + i0, slices[(size_t)b], stride, d_keys);
        hipLaunchKernelGGL(k_l2_merge, dim3((unsigned)nb), dim3(LANES), 0, s, d_pairs, d_items + i0, slices[(size_t)b], stride, d_keys, ratio,
                           d_bestt, d_bestd, d_flag, d_qidx);
    }
    tm.next(2);
    UNIT_TRY(hipMemsetAsync(d_pos, 0, sizeof(int), s));
    UNIT_TRY(hipcub::DeviceScan::InclusiveSum(d_tmp, tmp_bytes, d_flag, d_pos + 1, (int)n_rows, s));
    hipLaunchKernelGGL(k_l2_pair_ptr, dim3(grid_for(n_pairs + 1)), dim3(256), 0, s, n_pairs, d_prow, d_pos, d_pptr);
    hipLaunchKernelGGL(k_l2_scatter, dim3(grid_for(n_rows)), dim3(256), 0, s, n_rows, d_flag, d_pos, d_bestt, d_bestd, d_qidx, ocap, d_oq, d_ot, d_od);
    UNIT_TRY(hipGetLastError());
    tm.next(3);
    UNIT_TRY(hipMemcpyAsync(pair_ptr, d_pptr, sizeof(long long) * prow.size(), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    const long long tot = pair_ptr[n_pairs];
    *total = tot;
    if (tot > cap) return UNIT_ERR_CAPACITY;
    if (tot > 0) {
        UNIT_TRY(hipMemcpyAsync(query_idx, d_oq, sizeof(int) * (size_t)tot, hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipMemcpyAsync(train_idx, d_ot, sizeof(int) * (size_t)tot, hipMemcpyDeviceToHost, s));
        if (distance) UNIT_TRY(hipMemcpyAsync(distance, d_od, sizeof(float) * (size_t)tot, hipMemcpyDeviceToHost, s));
    }
    tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    if (timing) {
        tm.collect(timing);
        timing[4] = n_batches;
    }
    return 0;
}

}  // namespace sfmba
