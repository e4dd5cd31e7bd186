// feature_match.hip -- SfM2DFeatureUtilities::matchFeatures for a whole list of image pairs on the MI355X (gfx950).
//
// Reference: SfM::createFeatureMatchMatrix (SfMToyLib/SfM.cpp:157-212) calls matchFeatures (SfM2DFeatureUtilities.cpp:53-71)
// for every pair i < j: a brute-force Hamming kNN with K = 2 (BFMatcher::knnMatch) and the 0.8 ratio test.  The result is
// integer work and exactly defined (include/sfmba.h, sfmba_match_features), so it is BIT-EXACT with a CPU restatement:
//
//   upload    the descriptor rows once per call, zero-padded to W 32-bit words (W = 8 up to 32 bytes, 16 up to 64 bytes); the
//             padding adds nothing to any distance.
//   top-2     k_match_top2<W>: grid = (query tile of a pair) x (train slice), a batch of tiles per launch.  A lane holds two
//             query rows in VGPRs; the block stages 256 train rows of its slice at a time in LDS and every lane reads the same
//             row (an LDS broadcast).  A distance is W v_xor_b32 + W v_bcnt_u32_b32 (accumulating through src1); the pair
//             (d, j) is packed into the 32-bit key (d << 22) | j, whose unsigned order IS the contract's (d, j) order, and the
//             top-2 update is branch-free: b2 = min(b2, max(b1, k)); b1 = min(b1, k).  Per query and train row at W = 8 that
//             is 8 xor + 8 bcnt + 1 lshl_or + 3 min/max = 20 VALU instructions; the gfx950 disassembly of the unrolled loop
//             (4 rows x 2 queries) counts 157 VALU per 8 distances = 19.6 (two of the min pairs fuse into v_min3_u32), and the
//             two ds_read_b128 of a row are shared by the lane's two queries.  Measured (profiles/r07_match_features.txt):
//             1.7-1.9e12 distances/s, 43-51 % of the issue ceiling 3.93e12 at the 2.4 GHz peak clock.
//   merge     k_match_merge: the 2 smallest keys over the slices with the same update (a total order: the result does not
//             depend on the slice count or on arrival order -- deterministic by construction, no atomics), then the ratio
//             test in double.
//   compact   an inclusive scan of the kept flags over all query rows of the call (hipCUB) gives the CSR positions; one
//             scatter writes (query, train, distance) in ascending query order inside a pair, pairs in list order.
//
// The per-slice keys of a batch live in a scratch buffer bounded by MATCH_SCRATCH_BYTES whatever the number of pairs.
#include "feature_match.h"
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
constexpr int CHUNK = 256;              // train rows staged in LDS at a time
static_assert(MATCH_TILE == 2 * LANES, "two queries per lane");

struct MatchPair {
    long long qoff, toff;               // first descriptor row of the query (left) / train (right) image
    long long row0;                     // first query row of the pair in the call's row numbering
    int nq, nt;
};
struct MatchItem { int pair, q0; };     // one query tile

__device__ __forceinline__ void top2(unsigned& b1, unsigned& b2, unsigned k) {
    b2 = min(b2, max(b1, k));
    b1 = min(b1, k);
}

template <int W>
__device__ __forceinline__ void load_row(const uint32_t* __restrict__ desc, long long row, bool valid, uint32_t (&r)[W]) {
#pragma unroll
    for (int k = 0; k < W; ++k) r[k] = 0u;
    if (!valid) return;                                    // a lane past the pair's last query row: computes, never stored
    const uint4* src = reinterpret_cast<const uint4*>(desc + row * W);
#pragma unroll
    for (int k = 0; k < W / 4; ++k) {
        const uint4 v = src[k];
        r[4 * k] = v.x; r[4 * k + 1] = v.y; r[4 * k + 2] = v.z; r[4 * k + 3] = v.w;
    }
}

// keys[s * slice_stride + item * MATCH_TILE + lane (+ 256)] = the two smallest keys of the query row over train slice s.
template <int W>
__global__ __launch_bounds__(LANES) void k_match_top2(const uint32_t* __restrict__ desc, const MatchPair* __restrict__ pairs,
                                                      const MatchItem* __restrict__ items, int n_slices, long long slice_stride,
                                                      uint2* __restrict__ keys) {
    __shared__ uint4 sh[CHUNK * (W / 4)];
    const MatchItem it = items[blockIdx.x];
    const MatchPair P = pairs[it.pair];
    const int s = blockIdx.y;
    const int len = (P.nt + n_slices - 1) / n_slices;
    const int t0 = min(P.nt, s * len), t1 = min(P.nt, t0 + len);
    const int qa = it.q0 + threadIdx.x, qb = qa + LANES;
    uint32_t ra[W], rb[W];
    load_row<W>(desc, P.qoff + qa, qa < P.nq, ra);
    load_row<W>(desc, P.qoff + qb, qb < P.nq, rb);
    unsigned a1 = ~0u, a2 = ~0u, b1 = ~0u, b2 = ~0u;
    for (int c = t0; c < t1; c += CHUNK) {
        const int n = min(CHUNK, t1 - c);
        __syncthreads();                                   // the previous chunk has been read by every wave
        if ((int)threadIdx.x < n) {
            const uint4* src = reinterpret_cast<const uint4*>(desc + (P.toff + c + threadIdx.x) * W);
#pragma unroll
            for (int k = 0; k < W / 4; ++k) sh[threadIdx.x * (W / 4) + k] = src[k];
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            unsigned da = 0, db = 0;
#pragma unroll
            for (int k = 0; k < W / 4; ++k) {
                const uint4 t = sh[j * (W / 4) + k];       // same address in every lane: broadcast
                const uint32_t tw[4] = { t.x, t.y, t.z, t.w };
#pragma unroll
                for (int w = 0; w < 4; ++w) {                  // a serial chain: v_bcnt_u32_b32 accumulates through src1
                    da = __popc(ra[4 * k + w] ^ tw[w]) + da;
                    db = __popc(rb[4 * k + w] ^ tw[w]) + db;
                }
            }
            const unsigned jj = (unsigned)(c + j);
            top2(a1, a2, (da << 22) | jj);
            top2(b1, b2, (db << 22) | jj);
        }
    }
    uint2* out = keys + (size_t)s * (size_t)slice_stride + (size_t)blockIdx.x * MATCH_TILE + threadIdx.x;
    out[0] = make_uint2(a1, a2);
    out[LANES] = make_uint2(b1, b2);
}

// Merge over the slices + ratio test: best[row] = smallest key, flag[row] = kept, qidx[row] = query index.  Only tiles of pairs
// with >= 2 train rows are launched, so the second key is always a real one.
__global__ __launch_bounds__(LANES) void k_match_merge(const MatchPair* __restrict__ pairs, const MatchItem* __restrict__ items, int n_slices,
                                                       long long slice_stride, const uint2* __restrict__ keys, double ratio,
                                                       unsigned* __restrict__ best, int* __restrict__ flag, int* __restrict__ qidx) {
    const MatchItem it = items[blockIdx.x];
    const MatchPair P = pairs[it.pair];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int q = it.q0 + threadIdx.x + h * LANES;
        if (q >= P.nq) continue;
        const size_t slot = (size_t)blockIdx.x * MATCH_TILE + threadIdx.x + h * LANES;
        unsigned k1 = ~0u, k2 = ~0u;
        for (int s = 0; s < n_slices; ++s) {
            const uint2 v = keys[(size_t)s * (size_t)slice_stride + slot];
            top2(k1, k2, v.x);
            top2(k1, k2, v.y);
        }
        const long long row = P.row0 + q;
        best[row] = k1;
        flag[row] = (double)(k1 >> 22) < ratio * (double)(k2 >> 22) ? 1 : 0;
        qidx[row] = q;
    }
}

// pos[0..n_rows] = exclusive positions (pos[0] = 0, pos[n_rows] = total); pair_ptr[p] = pos[prow[p]].
__global__ __launch_bounds__(256) void k_match_pair_ptr(int n, const long long* __restrict__ prow, const int* __restrict__ pos,
                                                        long long* __restrict__ pair_ptr) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p <= n) pair_ptr[p] = pos[prow[p]];
}

__global__ __launch_bounds__(256) void k_match_scatter(long long n_rows, const int* __restrict__ flag, const int* __restrict__ pos,
                                                       const unsigned* __restrict__ best, const int* __restrict__ qidx, long long cap,
                                                       int* __restrict__ out_q, int* __restrict__ out_t, float* __restrict__ out_d) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows || !flag[r]) return;
    const long long o = pos[r];
    if (o >= cap) return;
    const unsigned k = best[r];
    out_q[o] = qidx[r];
    out_t[o] = (int)(k & 0x3fffffu);
    out_d[o] = (float)(k >> 22);
}

unsigned grid_for(long long n) { return (unsigned)((n + 255) / 256); }

template <int W>
void launch_top2(hipStream_t s, int n_items, int n_slices, const uint32_t* desc, const MatchPair* pairs, const MatchItem* items,
                 long long stride, uint2* keys) {
    hipLaunchKernelGGL(k_match_top2<W>, dim3((unsigned)n_items, (unsigned)n_slices), dim3(LANES), 0, s, desc, pairs, items, n_slices, stride, keys);
}

}  // namespace

int match_features(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* desc, int desc_bytes,
                   int n_pairs, const int32_t* pair_left, const int32_t* pair_right, double ratio, int64_t* pair_ptr,
                   int32_t* query_idx, int32_t* train_idx, float* distance, int64_t cap, int64_t* total, double* timing) {
    for (int p = 0; p <= n_pairs; ++p) pair_ptr[p] = 0;
    *total = 0;
    if (timing) for (int i = 0; i < 5; ++i) timing[i] = 0.0;
    // pairs, query rows (only pairs that can keep anything: >= 2 train rows) and query tiles
    std::vector<MatchPair> pairs((size_t)std::max(n_pairs, 1));
    std::vector<long long> prow((size_t)n_pairs + 1, 0);
    std::vector<MatchItem> items;
    long long n_rows = 0;
    for (int p = 0; p < n_pairs; ++p) {
        MatchPair& P = pairs[(size_t)p];
        const int l = pair_left[p], r = pair_right[p];
        P.qoff = img_ptr[l]; P.toff = img_ptr[r];
        P.nq = (int)(img_ptr[l + 1] - img_ptr[l]); P.nt = (int)(img_ptr[r + 1] - img_ptr[r]);
        if (P.nt < 2) P.nq = 0;                  // no second neighbour: nothing is kept (include/sfmba.h)
        P.row0 = n_rows;
        prow[(size_t)p] = n_rows;
        n_rows += P.nq;
        for (int q0 = 0; q0 < P.nq; q0 += MATCH_TILE) items.push_back(MatchItem{ p, q0 });
    }
    prow[(size_t)n_pairs] = n_rows;
    if (n_rows == 0) return 0;

    DeviceArena scratch(device);
    const int W = desc_bytes <= 32 ? 8 : 16;
    const long long n_desc = img_ptr[n_images];
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    // allocations first (the arena zeroes them), then the stream work
    const int n_items = (int)items.size();
    const int n_batches = (n_items + MATCH_BATCH_TILES - 1) / MATCH_BATCH_TILES;
    std::vector<int> slices((size_t)n_batches);
    long long key_slots = 0;
    for (int b = 0; b < n_batches; ++b) {
        const int i0 = b * MATCH_BATCH_TILES, i1 = std::min(n_items, i0 + MATCH_BATCH_TILES), nb = i1 - i0;
        int max_nt = 0;
        for (int i = i0; i < i1; ++i) max_nt = std::max(max_nt, pairs[(size_t)items[(size_t)i].pair].nt);
        const int by_rows = std::max(1, (max_nt + MATCH_MIN_SLICE_ROWS - 1) / MATCH_MIN_SLICE_ROWS);
        const int by_fill = (MATCH_TARGET_BLOCKS + nb - 1) / nb;
        slices[(size_t)b] = std::max(1, std::min(std::min(by_fill, by_rows), MATCH_MAX_SLICES));
        key_slots = std::max(key_slots, (long long)slices[(size_t)b] * nb * MATCH_TILE);
    }
    uint32_t* d_desc;
    MatchPair* d_pairs;
    MatchItem* d_items;
    uint2* d_keys;
    unsigned* d_best;
    int *d_flag, *d_pos, *d_qidx;
    long long *d_prow, *d_pptr;
    UNIT_ALLOC(scratch, d_desc, uint32_t, (size_t)n_desc * W);
    UNIT_ALLOC(scratch, d_pairs, MatchPair, pairs.size());
    UNIT_ALLOC(scratch, d_items, MatchItem, items.size());
    UNIT_ALLOC(scratch, d_keys, uint2, (size_t)key_slots);
    UNIT_ALLOC(scratch, d_best, unsigned, (size_t)n_rows);
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

    // upload: rows of exactly 4 W bytes go as they are, others are padded with zero bytes on the host
    tm.begin(0);
    std::vector<uint32_t> padded;
    if (n_desc > 0) {
        if (desc_bytes == 4 * W) {
            UNIT_TRY(hipMemcpyAsync(d_desc, desc, (size_t)n_desc * desc_bytes, hipMemcpyHostToDevice, s));
        } else {
            padded.assign((size_t)n_desc * W, 0u);
            unsigned char* dst = reinterpret_cast<unsigned char*>(padded.data());
            for (long long i = 0; i < n_desc; ++i) std::memcpy(dst + (size_t)i * 4 * W, desc + (size_t)i * desc_bytes, (size_t)desc_bytes);
            UNIT_TRY(hipMemcpyAsync(d_desc, padded.data(), padded.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        }
    }
    UNIT_TRY(hipMemcpyAsync(d_pairs, pairs.data(), sizeof(MatchPair) * pairs.size(), hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_items, items.data(), sizeof(MatchItem) * items.size(), hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_prow, prow.data(), sizeof(long long) * prow.size(), hipMemcpyHostToDevice, s));
    tm.next(1);

    for (int b = 0; b < n_batches; ++b) {
        const int i0 = b * MATCH_BATCH_TILES, nb = std::min(n_items, i0 + MATCH_BATCH_TILES) - i0;
        const long long stride = (long long)nb * MATCH_TILE;
        if (W == 8) launch_top2<8>(s, nb, slices[(size_t)b], d_desc, d_pairs, d_items + i0, stride, d_keys);
        else        launch_top2<16>(s, nb, slices[(size_t)b], d_desc, d_pairs, d_items + i0, stride, d_keys);
        hipLaunchKernelGGL(k_match_merge, dim3((unsigned)nb), dim3(LANES), 0, s, d_pairs, d_items + i0, slices[(size_t)b], stride, d_keys, ratio,
                           d_best, d_flag, d_qidx);
    }
    tm.next(2);
    UNIT_TRY(hipMemsetAsync(d_pos, 0, sizeof(int), s));
    UNIT_TRY(hipcub::DeviceScan::InclusiveSum(d_tmp, tmp_bytes, d_flag, d_pos + 1, (int)n_rows, s));
    hipLaunchKernelGGL(k_match_pair_ptr, dim3(grid_for(n_pairs + 1)), dim3(256), 0, s, n_pairs, d_prow, d_pos, d_pptr);
    hipLaunchKernelGGL(k_match_scatter, dim3(grid_for(n_rows)), dim3(256), 0, s, n_rows, d_flag, d_pos, d_best, d_qidx, ocap, d_oq, d_ot, d_od);
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
