// homography_ransac.hip -- SfMStereoUtilities::findHomographyInliers for a batch of image pairs on the MI355X (gfx950).
//
// Reference: SfM::sortViewsForBaseline (SfMToyLib/SfM.cpp:333-364) calls cv::findHomography(RANSAC, 10 px) + countNonZero(mask) once
// per image pair with at least 100 matches (SfMStereoUtilities.cpp:51-72).  Its sample stream is OpenCV's global RNG; the contract
// here (include/sfmba.h, sfmba_homography_ransac) is our own and deterministic.  A pair's correspondences are never materialised:
// every kernel goes through query_idx / train_idx into the key points of the two images (GetAlignedPointsFromMatch, folded in).
// Three launches on one stream, no host round trip between them:
//
//   hypotheses   k_hom_hypotheses: one lane per (pair, hypothesis), fp64, everything in registers (homography_math.h): the seeded
//                sample, the four-point homography in closed form (Cramer on the triple determinants, no pivoting).  Writes H in
//                fp64 (the winner's goes to the caller) and rounded to fp32 (what the score reads, 48 B rows), and the count
//                0 / -1 (invalid).
//   score        k_hom_score: the hot loop, n_hyp x n transfers.  A block = a tile of 64 hypotheses of one pair x chunks of its
//                correspondences.  It gathers a chunk of 1024 correspondences ONCE into LDS as (x, y, x', y'): one float4 each --
//                the only place the indirect reads happen.  The 4 waves of the block hold the SAME 64 hypotheses (9 fp32 numbers
//                per lane, in registers) and interleave the chunk, so every lane of a wave reads the same LDS address: one
//                ds_read_b128 broadcast per evaluation, conflict-free.  hom_inlier is 6 + 2 + 1 FMA, 3 multiplies and 2
//                compares, no division.  One integer atomicAdd per lane and chunk goes into hyp_count: integer sums do not
//                depend on their order.
//   select       k_hom_select: one block per pair.  Arg-max of (count, -h) over the hypotheses, the winner's mask with the same
//                hom_inlier, the winner's H as it stands (no refit), the result.
#include "homography_ransac.h"
#include "homography_math.h"
#include "device_arena.h"

#include <algorithm>
#include <climits>

namespace sfmba {

namespace {

constexpr int HYP_THREADS = 64;              // fp64 and register-hungry: small blocks spread the lanes over many CUs

// what the kernels need to find correspondence i of pair p: x = pts[img_ptr[pair_left[p]] + query_idx[i]] -> x' likewise
struct HomProblem {
    const long long* img_ptr;
    const float2* pts;
    const int* pair_left;
    const int* pair_right;
    const long long* pair_ptr;
    const int* query_idx;
    const int* train_idx;
};

__global__ __launch_bounds__(HYP_THREADS) void k_hom_hypotheses(long long n_items, int n_hyp, HomProblem pr, uint64_t seed, double* __restrict__ hyp_H,
                                                                float* __restrict__ hyp_hf, int* __restrict__ hyp_count) {
    const long long g = (long long)blockIdx.x * HYP_THREADS + threadIdx.x;
    if (g >= n_items) return;
    const long long p = g / n_hyp;
    const int h = (int)(g - p * n_hyp);
    const long long base = pr.pair_ptr[p], n = pr.pair_ptr[p + 1] - base;
    double H[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) H[j] = 0.0;
    long long i0, i1, i2, i3;
    bool ok = pnp_sample(pnp_mix(seed + (uint64_t)p), h, n, i0, i1, i2, i3);
    if (ok) {
        const float2* pl = pr.pts + pr.img_ptr[pr.pair_left[p]];
        const float2* pq = pr.pts + pr.img_ptr[pr.pair_right[p]];
        double l[8], r[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = base + (j == 0 ? i0 : (j == 1 ? i1 : (j == 2 ? i2 : i3)));
            const float2 a = pl[pr.query_idx[i]], b = pq[pr.train_idx[i]];
            l[2 * j] = (double)a.x; l[2 * j + 1] = (double)a.y;
            r[2 * j] = (double)b.x; r[2 * j + 1] = (double)b.y;
        }
        ok = hom_hypothesis(l, r, H);
    }
    double* dst = hyp_H + 9 * g;
    float* dhf = hyp_hf + HOM_HF_STRIDE * g;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        dst[j] = H[j];
        dhf[j] = (float)H[j];
    }
    hyp_count[g] = ok ? 0 : -1;
}

// hyp_count[p][h] += the number of inliers of hypothesis h among the correspondences of the chunks this block walks.  An invalid
// hypothesis has an all-zero H: W = 0, never an inlier, so its count stays -1.
__global__ __launch_bounds__(HOM_SCORE_THREADS) void k_hom_score(int n_hyp, int tiles, HomProblem pr, float thr2, const float* __restrict__ hyp_hf,
                                                                 int* __restrict__ hyp_count) {
    __shared__ float4 sh[HOM_CHUNK];         // x, y, x', y'
    const long long p = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - p * tiles);
    const long long base = pr.pair_ptr[p], n = pr.pair_ptr[p + 1] - base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = tile * HOM_TILE + lane;
    const long long slot = p * n_hyp + h;
    float hf[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) hf[j] = 0.0f;
    if (h < n_hyp) {
        const float4* src = reinterpret_cast<const float4*>(hyp_hf + HOM_HF_STRIDE * slot);      // 48 B rows of a 256 B aligned array
        const float4 r0 = src[0], r1 = src[1], r2 = src[2];
        hf[0] = r0.x; hf[1] = r0.y; hf[2] = r0.z; hf[3] = r0.w;
        hf[4] = r1.x; hf[5] = r1.y; hf[6] = r1.z; hf[7] = r1.w;
        hf[8] = r2.x;
    }
    const float2* pl = pr.pts + pr.img_ptr[pr.pair_left[p]];
    const float2* pq = pr.pts + pr.img_ptr[pr.pair_right[p]];
    const long long n_chunks = (n + HOM_CHUNK - 1) / HOM_CHUNK;
    for (long long c = blockIdx.y; c < n_chunks; c += gridDim.y) {
        const long long c0 = c * HOM_CHUNK;
        const int m = (int)min((long long)HOM_CHUNK, n - c0);
        __syncthreads();                                   // the previous chunk has been read by every wave
        for (int j = threadIdx.x; j < m; j += HOM_SCORE_THREADS) {
            const long long i = base + c0 + j;
            const float2 a = pl[pr.query_idx[i]], b = pq[pr.train_idx[i]];
            sh[j] = make_float4(a.x, a.y, b.x, b.y);
        }
        __syncthreads();
        int cnt = 0;
#pragma unroll 4
        for (int j = wave; j < m; j += HOM_SCORE_THREADS / 64) {
            const float4 a = sh[j];                        // same address in every lane: broadcast
            cnt += hom_inlier(hf, a.x, a.y, a.z, a.w, thr2) ? 1 : 0;
        }
        if (cnt > 0 && h < n_hyp) atomicAdd(&hyp_count[slot], cnt);
    }
}

__global__ __launch_bounds__(HOM_SELECT_THREADS) void k_hom_select(int n_hyp, HomProblem pr, float thr2, const double* __restrict__ hyp_H,
                                                                   const float* __restrict__ hyp_hf, const int* __restrict__ hyp_count,
                                                                   double* __restrict__ H_out, unsigned char* __restrict__ inlier,
                                                                   sfmba_homography_result* __restrict__ result) {
    constexpr int WAVES = HOM_SELECT_THREADS / 64;
    __shared__ unsigned long long s_key[WAVES];
    const long long p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = pr.pair_ptr[p];
    const int n = (int)(pr.pair_ptr[p + 1] - base);
    const int* counts = hyp_count + p * n_hyp;

    // the winner: the largest (count, -h); key 0 = no valid hypothesis (a valid key has non-zero low bits: h < 65536)
    unsigned long long key = 0;
    for (int h = tid; h < n_hyp; h += HOM_SELECT_THREADS) {
        const int c = counts[h];
        if (c >= 0) {
            const unsigned long long cand = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(0xffffffffu - (unsigned)h);
            key = cand > key ? cand : key;
        }
    }
    key = wave_max_u64(key);
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    key = s_key[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) key = s_key[w] > key ? s_key[w] : key;
    double* out = H_out + 9 * p;
    sfmba_homography_result r;
    r.n_matches = n;
    if (n < 4 || key == 0) {                                  // block-uniform
        if (tid == 0) {
#pragma unroll
            for (int j = 0; j < 9; ++j) out[j] = (j == 0 || j == 4 || j == 8) ? 1.0 : 0.0;
            r.status = n < 4 ? 1 : 2; r.best_hypothesis = -1; r.n_inliers = 0;
            result[p] = r;
        }
        return;                                               // the mask stays zero (zeroed at allocation)
    }
    const int best = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
    const long long slot = p * n_hyp + best;
    float hf[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) hf[j] = hyp_hf[HOM_HF_STRIDE * slot + j];
    const float2* pl = pr.pts + pr.img_ptr[pr.pair_left[p]];
    const float2* pq = pr.pts + pr.img_ptr[pr.pair_right[p]];
    for (int i = tid; i < n; i += HOM_SELECT_THREADS) {
        const float2 a = pl[pr.query_idx[base + i]], b = pq[pr.train_idx[base + i]];
        inlier[base + i] = hom_inlier(hf, a.x, a.y, b.x, b.y, thr2) ? 1 : 0;
    }
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < 9; ++j) out[j] = hyp_H[9 * slot + j];
        r.status = 0; r.best_hypothesis = best; r.n_inliers = (int)(key >> 32);
        result[p] = r;
    }
}

}  // namespace

int homography_ransac(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const float* pts, int n_pairs, const int32_t* pair_left,
                      const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx, int n_hyp,
                      float threshold_px, uint64_t seed, double* H, unsigned char* inlier, sfmba_homography_result* result, double* hyp_H,
                      int32_t* hyp_count, double* timing) {
    if (timing) for (int i = 0; i < 5; ++i) timing[i] = 0.0;
    if (n_pairs <= 0) return 0;
    const long long total = pair_ptr[n_pairs];             // entries in front of pair_ptr[0] belong to no pair: uploaded, never read
    const long long n_pts = img_ptr[n_images];
    const long long n_items = (long long)n_pairs * n_hyp;
    const int tiles = (n_hyp + HOM_TILE - 1) / HOM_TILE;
    long long max_n = 0;
    for (int p = 0; p < n_pairs; ++p) max_n = std::max<long long>(max_n, pair_ptr[p + 1] - pair_ptr[p]);
    // HIP launches at most 2^32 - 1 threads along a grid dimension
    const long long max_threads = 0xffffffffll;
    if (max_n > (long long)INT_MAX || (long long)n_pairs * tiles * HOM_SCORE_THREADS > max_threads || n_items + HYP_THREADS > max_threads ||
        (long long)n_pairs * HOM_SELECT_THREADS > max_threads)
        return UNIT_ERR_TOO_LARGE;

    DeviceArena arena(device);
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    // allocations first (the arena zeroes them: the masks of status 1 / 2 pairs stay zero), then the stream work
    long long *d_img, *d_ptr;
    float2* d_pts;
    int *d_left, *d_right, *d_query, *d_train, *d_count;
    double *d_hH, *d_H;
    float* d_hf;
    unsigned char* d_inl;
    sfmba_homography_result* d_res;
    UNIT_ALLOC(arena, d_img, long long, (size_t)n_images + 1);
    UNIT_ALLOC(arena, d_pts, float2, (size_t)n_pts);
    UNIT_ALLOC(arena, d_left, int, (size_t)n_pairs);
    UNIT_ALLOC(arena, d_right, int, (size_t)n_pairs);
    UNIT_ALLOC(arena, d_ptr, long long, (size_t)n_pairs + 1);
    UNIT_ALLOC(arena, d_query, int, (size_t)total);
    UNIT_ALLOC(arena, d_train, int, (size_t)total);
    UNIT_ALLOC(arena, d_hH, double, (size_t)9 * n_items);
    UNIT_ALLOC(arena, d_hf, float, (size_t)HOM_HF_STRIDE * n_items);
    UNIT_ALLOC(arena, d_count, int, (size_t)n_items);
    UNIT_ALLOC(arena, d_H, double, (size_t)9 * n_pairs);
    UNIT_ALLOC(arena, d_inl, unsigned char, (size_t)total);
    UNIT_ALLOC(arena, d_res, sfmba_homography_result, (size_t)n_pairs);

    tm.begin(0);
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "the index arrays are uploaded as they are");
    UNIT_TRY(hipMemcpyAsync(d_img, img_ptr, sizeof(int64_t) * ((size_t)n_images + 1), hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_ptr, pair_ptr, sizeof(int64_t) * ((size_t)n_pairs + 1), hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_left, pair_left, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_right, pair_right, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice, s));
    if (n_pts > 0) UNIT_TRY(hipMemcpyAsync(d_pts, pts, sizeof(float) * 2 * (size_t)n_pts, hipMemcpyHostToDevice, s));
    if (total > 0) {
        UNIT_TRY(hipMemcpyAsync(d_query, query_idx, sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, s));
        UNIT_TRY(hipMemcpyAsync(d_train, train_idx, sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, s));
    }
    tm.next(1);
    const HomProblem pr{ d_img, d_pts, d_left, d_right, d_ptr, d_query, d_train };
    const float thr2 = threshold_px * threshold_px;
    hipLaunchKernelGGL(k_hom_hypotheses, dim3((unsigned)((n_items + HYP_THREADS - 1) / HYP_THREADS)), dim3(HYP_THREADS), 0, s, n_items, n_hyp, pr,
                       seed, d_hH, d_hf, d_count);
    tm.next(2);
    const long long max_chunks = (max_n + HOM_CHUNK - 1) / HOM_CHUNK;
    if (max_chunks > 0)
        hipLaunchKernelGGL(k_hom_score, dim3((unsigned)(n_pairs * tiles), (unsigned)std::min<long long>(max_chunks, HOM_MAX_CHUNK_BLOCKS)),
                           dim3(HOM_SCORE_THREADS), 0, s, n_hyp, tiles, pr, thr2, d_hf, d_count);
    tm.next(3);
    hipLaunchKernelGGL(k_hom_select, dim3((unsigned)n_pairs), dim3(HOM_SELECT_THREADS), 0, s, n_hyp, pr, thr2, d_hH, d_hf, d_count, d_H,
                       d_inl, d_res);
    UNIT_TRY(hipGetLastError());
    tm.next(4);
    UNIT_TRY(hipMemcpyAsync(H, d_H, sizeof(double) * 9 * (size_t)n_pairs, hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(result, d_res, sizeof(sfmba_homography_result) * (size_t)n_pairs, hipMemcpyDeviceToHost, s));
    if (total > 0) UNIT_TRY(hipMemcpyAsync(inlier, d_inl, (size_t)total, hipMemcpyDeviceToHost, s));
    if (hyp_H) UNIT_TRY(hipMemcpyAsync(hyp_H, d_hH, sizeof(double) * 9 * (size_t)n_items, hipMemcpyDeviceToHost, s));
    if (hyp_count) UNIT_TRY(hipMemcpyAsync(hyp_count, d_count, sizeof(int) * (size_t)n_items, hipMemcpyDeviceToHost, s));
    tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    if (timing) tm.collect(timing);
    return 0;
}

}  // namespace sfmba
