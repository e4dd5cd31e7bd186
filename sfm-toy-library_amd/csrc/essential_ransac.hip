// essential_ransac.hip -- SfMStereoUtilities::findCameraMatricesFromMatch for a batch of image pairs on the MI355X (gfx950).
//
// Reference: SfM::findBaselineTriangulation (SfMToyLib/SfM.cpp:236-320) and addMoreViewsToReconstruction (:413-431) call
// cv::findEssentialMat(RANSAC, 0.999, 1 px) + cv::recoverPose once per image pair (SfMStereoUtilities.cpp:74-118).  Their sample
// stream is OpenCV's global RNG; the contract here (include/sfmba.h, sfmba_essential_ransac) is our own and deterministic.  A pair's
// correspondences are never materialised: every kernel goes through query_idx / train_idx into the key points of the two images
// (GetAlignedPointsFromMatch, folded in).  Three launches on one stream, no host round trip between them:
//
//   hypotheses   k_ess_hypotheses: one lane per (pair, hypothesis), fp64 (essential_math.h): the seeded six-point sample, the
//                five-point solver, the sixth point's choice among its solutions.  What the solver indexes at run time (pivot rows
//                and columns of the 5 x 9 and 10 x 20 eliminations, the Sturm chain) is a 200-double work area per lane in LDS,
//                the 64 lanes of the block interleaved double by double (conflict-free whatever index a lane is at: one index is
//                512 B, a whole turn of the banks); everything else is unrolled over compile-time indices in registers.  One wave
//                per block, 100 KiB of LDS: one wave per CU.  Writes E in fp64 (the winner's goes to the caller), the pixel
//                matrix G = fx fy diag(1/fx, 1/fy, 1) E diag(1/fx, 1/fy, 1) in fp64 (what the score reads, 72 B rows), the number
//                of real solutions and the count 0 / -1 (invalid).
//   score        k_ess_score: the hot loop, n_hyp x n Sampson decisions, the layout of k_hom_score.  A block = a tile of 64
//                hypotheses of one pair x chunks of its correspondences.  It gathers a chunk of 1024 correspondences ONCE into LDS
//                as centred pixels (x, y, x', y'): one float4 each -- the only place the indirect reads happen.  The 4 waves of the
//                block hold the SAME 64 hypotheses (9 fp64 numbers per lane, in registers: the residual is taken in fp64,
//                essential_math.h) and interleave the chunk, so every lane of a wave reads the same LDS address: one ds_read_b128
//                broadcast per evaluation.  One integer atomicAdd per lane and chunk goes into hyp_count: integer sums do not
//                depend on their order.
//   select       k_ess_select: one block per pair.  Arg-max of (count, -h) over the hypotheses; the winner's mask with the same
//                ess_inlier; the four pose candidates in closed form (one lane, fp64); the block walks the winner's inliers and
//                counts the points in front for each candidate (integer sums); the candidate with the most, the final mask =
//                winner's mask AND in front for it, the result.
#include "essential_ransac.h"
#include "essential_math.h"
#include "device_arena.h"

#include <algorithm>
#include <climits>

namespace sfmba {

namespace {

// what the kernels need to find correspondence i of pair p: x = pts[img_ptr[pair_left[p]] + query_idx[i]] -> x' likewise
struct EssProblem {
    const long long* img_ptr;
    const float2* pts;
    const int* pair_left;
    const int* pair_right;
    const long long* pair_ptr;
    const int* query_idx;
    const int* train_idx;
};

struct EssCamera { float fx, fy, cx, cy; };

__global__ __launch_bounds__(ESS_HYP_THREADS) void k_ess_hypotheses(long long n_items, int n_hyp, EssProblem pr, EssCamera cam, uint64_t seed,
                                                                    double* __restrict__ hyp_E, double* __restrict__ hyp_G,
                                                                    int* __restrict__ hyp_count, int* __restrict__ hyp_nsol) {
    __shared__ double work[ESS_WORK * ESS_HYP_THREADS];
    const long long g = (long long)blockIdx.x * ESS_HYP_THREADS + threadIdx.x;
    if (g >= n_items) return;
    const long long p = g / n_hyp;
    const int h = (int)(g - p * n_hyp);
    const long long base = pr.pair_ptr[p], n = pr.pair_ptr[p + 1] - base;
    double E[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) E[j] = 0.0;
    int nsol = 0;
    long long id[6];
    bool ok = pnp_sample6(pnp_mix(seed + (uint64_t)p), h, n, id);
    if (ok) {
        const float2* pl = pr.pts + pr.img_ptr[pr.pair_left[p]];
        const float2* pq = pr.pts + pr.img_ptr[pr.pair_right[p]];
        const double fx = (double)cam.fx, fy = (double)cam.fy, cx = (double)cam.cx, cy = (double)cam.cy;
        double l[12], r[12];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const long long i = base + id[j];
            const float2 a = pl[pr.query_idx[i]], b = pq[pr.train_idx[i]];
            l[2 * j] = ((double)a.x - cx) / fx; l[2 * j + 1] = ((double)a.y - cy) / fy;
            r[2 * j] = ((double)b.x - cx) / fx; r[2 * j + 1] = ((double)b.y - cy) / fy;
        }
        const EssStore<ESS_HYP_THREADS> w{ work + threadIdx.x };
        ok = ess_hypothesis(w, l, r, E, nsol);
    }
    double G[9];
    ess_pixel_matrix(E, (double)cam.fx, (double)cam.fy, G);
    double* dst = hyp_E + 9 * g;
    double* dG = hyp_G + 9 * g;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        dst[j] = E[j];
        dG[j] = G[j];
    }
    hyp_count[g] = ok ? 0 : -1;
    hyp_nsol[g] = nsol;
}

// hyp_count[p][h] += the number of inliers of hypothesis h among the correspondences of the chunks this block walks.  An invalid
// hypothesis has an all-zero G: never an inlier, so its count stays -1.
__global__ __launch_bounds__(ESS_SCORE_THREADS) void k_ess_score(int n_hyp, int tiles, EssProblem pr, EssCamera cam, float thr2,
                                                                 const double* __restrict__ hyp_G, int* __restrict__ hyp_count) {
    __shared__ float4 sh[ESS_CHUNK];         // centred pixels x, y, x', y'
    const long long p = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - p * tiles);
    const long long base = pr.pair_ptr[p], n = pr.pair_ptr[p + 1] - base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = tile * ESS_TILE + lane;
    const long long slot = p * n_hyp + h;
    double G[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) G[j] = h < n_hyp ? hyp_G[9 * slot + j] : 0.0;
    const float2* pl = pr.pts + pr.img_ptr[pr.pair_left[p]];
    const float2* pq = pr.pts + pr.img_ptr[pr.pair_right[p]];
    const long long n_chunks = (n + ESS_CHUNK - 1) / ESS_CHUNK;
    for (long long c = blockIdx.y; c < n_chunks; c += gridDim.y) {
        const long long c0 = c * ESS_CHUNK;
        const int m = (int)min((long long)ESS_CHUNK, n - c0);
        __syncthreads();                                   // the previous chunk has been read by every wave
        for (int j = threadIdx.x; j < m; j += ESS_SCORE_THREADS) {
            const long long i = base + c0 + j;
            const float2 a = pl[pr.query_idx[i]], b = pq[pr.train_idx[i]];
            sh[j] = make_float4(a.x - cam.cx, a.y - cam.cy, b.x - cam.cx, b.y - cam.cy);
        }
        __syncthreads();
        int cnt = 0;
#pragma unroll 4
        for (int j = wave; j < m; j += ESS_SCORE_THREADS / 64) {
            const float4 a = sh[j];                        // same address in every lane: broadcast
            cnt += ess_inlier(G, a.x, a.y, a.z, a.w, thr2) ? 1 : 0;
        }
        if (cnt > 0 && h < n_hyp) atomicAdd(&hyp_count[slot], cnt);
    }
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(ESS_SELECT_THREADS) void k_ess_select(int n_hyp, EssProblem pr, EssCamera cam, float thr2,
                                                                   const double* __restrict__ hyp_E, const double* __restrict__ hyp_G,
                                                                   const int* __restrict__ hyp_count, double* __restrict__ E_out,
                                                                   double* __restrict__ pose_out, unsigned char* __restrict__ inlier,
                                                                   sfmba_essential_result* __restrict__ result) {
    constexpr int WAVES = ESS_SELECT_THREADS / 64;
    __shared__ unsigned long long s_key[WAVES];
    __shared__ double s_pose[21];                      // R(+t), R(-t), t
    __shared__ int s_cnt[4], s_ok;
    const long long p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = pr.pair_ptr[p];
    const int n = (int)(pr.pair_ptr[p + 1] - base);
    const int* counts = hyp_count + p * n_hyp;

    // the winner: the largest (count, -h); key 0 = no valid hypothesis (a valid key has non-zero low bits: h < 65536)
    unsigned long long key = 0;
    for (int h = tid; h < n_hyp; h += ESS_SELECT_THREADS) {
        const int c = counts[h];
        if (c >= 0) {
            const unsigned long long cand = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(0xffffffffu - (unsigned)h);
            key = cand > key ? cand : key;
        }
    }
    key = wave_max_u64(key);
    if (lane == 0) s_key[wave] = key;
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();
    key = s_key[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) key = s_key[w] > key ? s_key[w] : key;
    double* eo = E_out + 9 * p;
    double* po = pose_out + 12 * p;
    sfmba_essential_result r;
    r.n_matches = n;
    r.n_pose_inliers = 0;
    r.pose_candidate = -1;
    if (n < 6 || key == 0) {                                  // block-uniform
        if (tid == 0) {
#pragma unroll
            for (int j = 0; j < 9; ++j) eo[j] = 0.0;
#pragma unroll
            for (int j = 0; j < 12; ++j) po[j] = (j == 0 || j == 5 || j == 10) ? 1.0 : 0.0;
            r.status = n < 6 ? 1 : 2; r.best_hypothesis = -1; r.n_inliers = 0;
            result[p] = r;
        }
        return;                                               // the mask stays zero (zeroed at allocation)
    }
    const int best = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
    const long long slot = p * n_hyp + best;
    double G[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) G[j] = hyp_G[9 * slot + j];
    if (tid == 0) {
        double E[9], Rp[9], Rm[9], t[3];
#pragma unroll
        for (int j = 0; j < 9; ++j) { E[j] = hyp_E[9 * slot + j]; eo[j] = E[j]; Rp[j] = Rm[j] = 0.0; }
        t[0] = t[1] = t[2] = 0.0;
        s_ok = ess_pose_candidates(E, Rp, Rm, t) ? 1 : 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) { s_pose[j] = Rp[j]; s_pose[9 + j] = Rm[j]; }
        s_pose[18] = t[0]; s_pose[19] = t[1]; s_pose[20] = t[2];
    }
    __syncthreads();
    const bool have_pose = s_ok != 0;
    double Rp[9], Rm[9], t[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) { Rp[j] = s_pose[j]; Rm[j] = s_pose[9 + j]; }
    t[0] = s_pose[18]; t[1] = s_pose[19]; t[2] = s_pose[20];
    const double fx = (double)cam.fx, fy = (double)cam.fy, cx = (double)cam.cx, cy = (double)cam.cy;
    const float2* pl = pr.pts + pr.img_ptr[pr.pair_left[p]];
    const float2* pq = pr.pts + pr.img_ptr[pr.pair_right[p]];
    // pass 1: the winner's mask, and for its inliers the four in-front counts
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int i = tid; i < n; i += ESS_SELECT_THREADS) {
        const float2 a = pl[pr.query_idx[base + i]], b = pq[pr.train_idx[base + i]];
        const bool in = ess_inlier(G, a.x - cam.cx, a.y - cam.cy, b.x - cam.cx, b.y - cam.cy, thr2);
        inlier[base + i] = in ? 1 : 0;
        if (in && have_pose) {
            const double x = ((double)a.x - cx) / fx, y = ((double)a.y - cy) / fy, u = ((double)b.x - cx) / fx, v = ((double)b.y - cy) / fy;
            c0 += ess_in_front(Rp, t, 1.0, x, y, u, v) ? 1 : 0;
            c1 += ess_in_front(Rm, t, -1.0, x, y, u, v) ? 1 : 0;
            c2 += ess_in_front(Rm, t, 1.0, x, y, u, v) ? 1 : 0;
            c3 += ess_in_front(Rp, t, -1.0, x, y, u, v) ? 1 : 0;
        }
    }
    c0 = wave_sum_i32(c0); c1 = wave_sum_i32(c1); c2 = wave_sum_i32(c2); c3 = wave_sum_i32(c3);
    if (lane == 0) {                                          // integer sums: the order does not matter
        atomicAdd(&s_cnt[0], c0); atomicAdd(&s_cnt[1], c1); atomicAdd(&s_cnt[2], c2); atomicAdd(&s_cnt[3], c3);
    }
    __syncthreads();
    int cand = 0, n_front = s_cnt[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (s_cnt[k] > n_front) { n_front = s_cnt[k]; cand = k; }
    const bool posed = have_pose && n_front > 0;               // block-uniform
    // pass 2: the final mask = the winner's mask AND in front for the chosen candidate (every lane re-reads its own bytes)
    const bool use_rp = cand == 0 || cand == 3;
    const double sgn = (cand == 0 || cand == 2) ? 1.0 : -1.0;
    for (int i = tid; i < n; i += ESS_SELECT_THREADS) {
        if (!inlier[base + i]) continue;
        bool keep = false;
        if (posed) {
            const float2 a = pl[pr.query_idx[base + i]], b = pq[pr.train_idx[base + i]];
            const double x = ((double)a.x - cx) / fx, y = ((double)a.y - cy) / fy, u = ((double)b.x - cx) / fx, v = ((double)b.y - cy) / fy;
            keep = use_rp ? ess_in_front(Rp, t, sgn, x, y, u, v) : ess_in_front(Rm, t, sgn, x, y, u, v);
        }
        inlier[base + i] = keep ? 1 : 0;
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) po[4 * i + j] = posed ? (use_rp ? Rp[3 * i + j] : Rm[3 * i + j]) : (i == j ? 1.0 : 0.0);
            po[4 * i + 3] = posed ? sgn * t[i] : 0.0;
        }
        r.status = posed ? 0 : 3; r.best_hypothesis = best; r.n_inliers = (int)(key >> 32);
        r.n_pose_inliers = posed ? n_front : 0;
        r.pose_candidate = posed ? cand : -1;
        result[p] = r;
    }
}

}  // namespace

int essential_ransac(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const float* pts, int n_pairs, const int32_t* pair_left,
                     const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx, const float* K,
                     int n_hyp, float threshold_px, uint64_t seed, double* E, double* pose, unsigned char* inlier,
                     sfmba_essential_result* result, double* hyp_E, int32_t* hyp_count, int32_t* hyp_nsol, double* timing) {
    if (timing) for (int i = 0; i < 5; ++i) timing[i] = 0.0;
    if (n_pairs <= 0) return 0;
    const long long total = pair_ptr[n_pairs];             // entries in front of pair_ptr[0] belong to no pair: uploaded, never read
    const long long n_pts = img_ptr[n_images];
    const long long n_items = (long long)n_pairs * n_hyp;
    const int tiles = (n_hyp + ESS_TILE - 1) / ESS_TILE;
    long long max_n = 0;
    for (int p = 0; p < n_pairs; ++p) max_n = std::max<long long>(max_n, pair_ptr[p + 1] - pair_ptr[p]);
    // HIP launches at most 2^32 - 1 threads along a grid dimension
    const long long max_threads = 0xffffffffll;
    if (max_n > (long long)INT_MAX || (long long)n_pairs * tiles * ESS_SCORE_THREADS > max_threads || n_items + ESS_HYP_THREADS > max_threads ||
        (long long)n_pairs * ESS_SELECT_THREADS > max_threads)
        return UNIT_ERR_TOO_LARGE;

    DeviceArena arena(device);
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    // allocations first (the arena zeroes them: the masks of status 1 / 2 pairs stay zero), then the stream work
    long long *d_img, *d_ptr;
    float2* d_pts;
    int *d_left, *d_right, *d_query, *d_train, *d_count, *d_nsol;
    double *d_hE, *d_hG, *d_E, *d_pose;
    unsigned char* d_inl;
    sfmba_essential_result* d_res;
    UNIT_ALLOC(arena, d_img, long long, (size_t)n_images + 1);
    UNIT_ALLOC(arena, d_pts, float2, (size_t)n_pts);
    UNIT_ALLOC(arena, d_left, int, (size_t)n_pairs);
    UNIT_ALLOC(arena, d_right, int, (size_t)n_pairs);
    UNIT_ALLOC(arena, d_ptr, long long, (size_t)n_pairs + 1);
    UNIT_ALLOC(arena, d_query, int, (size_t)total);
    UNIT_ALLOC(arena, d_train, int, (size_t)total);
    UNIT_ALLOC(arena, d_hE, double, (size_t)9 * n_items);
    UNIT_ALLOC(arena, d_hG, double, (size_t)9 * n_items);
    UNIT_ALLOC(arena, d_count, int, (size_t)n_items);
    UNIT_ALLOC(arena, d_nsol, int, (size_t)n_items);
    UNIT_ALLOC(arena, d_E, double, (size_t)9 * n_pairs);
    UNIT_ALLOC(arena, d_pose, double, (size_t)12 * n_pairs);
    UNIT_ALLOC(arena, d_inl, unsigned char, (size_t)total);
    UNIT_ALLOC(arena, d_res, sfmba_essential_result, (size_t)n_pairs);

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
    const EssProblem pr{ d_img, d_pts, d_left, d_right, d_ptr, d_query, d_train };
    const EssCamera cam{ K[0], K[4], K[2], K[5] };
    const float thr2 = threshold_px * threshold_px;
    hipLaunchKernelGGL(k_ess_hypotheses, dim3((unsigned)((n_items + ESS_HYP_THREADS - 1) / ESS_HYP_THREADS)), dim3(ESS_HYP_THREADS), 0, s, n_items,
                       n_hyp, pr, cam, seed, d_hE, d_hG, d_count, d_nsol);
    tm.next(2);
    const long long max_chunks = (max_n + ESS_CHUNK - 1) / ESS_CHUNK;
    if (max_chunks > 0)
        hipLaunchKernelGGL(k_ess_score, dim3((unsigned)(n_pairs * tiles), (unsigned)std::min<long long>(max_chunks, ESS_MAX_CHUNK_BLOCKS)),
                           dim3(ESS_SCORE_THREADS), 0, s, n_hyp, tiles, pr, cam, thr2, d_hG, d_count);
    tm.next(3);
    hipLaunchKernelGGL(k_ess_select, dim3((unsigned)n_pairs), dim3(ESS_SELECT_THREADS), 0, s, n_hyp, pr, cam, thr2, d_hE, d_hG, d_count, d_E,
                       d_pose, d_inl, d_res);
    UNIT_TRY(hipGetLastError());
    tm.next(4);
    UNIT_TRY(hipMemcpyAsync(E, d_E, sizeof(double) * 9 * (size_t)n_pairs, hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(pose, d_pose, sizeof(double) * 12 * (size_t)n_pairs, hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(result, d_res, sizeof(sfmba_essential_result) * (size_t)n_pairs, hipMemcpyDeviceToHost, s));
    if (total > 0) UNIT_TRY(hipMemcpyAsync(inlier, d_inl, (size_t)total, hipMemcpyDeviceToHost, s));
    if (hyp_E) UNIT_TRY(hipMemcpyAsync(hyp_E, d_hE, sizeof(double) * 9 * (size_t)n_items, hipMemcpyDeviceToHost, s));
    if (hyp_count) UNIT_TRY(hipMemcpyAsync(hyp_count, d_count, sizeof(int) * (size_t)n_items, hipMemcpyDeviceToHost, s));
    if (hyp_nsol) UNIT_TRY(hipMemcpyAsync(hyp_nsol, d_nsol, sizeof(int) * (size_t)n_items, hipMemcpyDeviceToHost, s));
    tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    if (timing) tm.collect(timing);
    return 0;
}

}  // namespace sfmba
