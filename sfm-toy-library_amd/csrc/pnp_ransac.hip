// pnp_ransac.hip -- SfMStereoUtilities::findCameraPoseFrom2D3DMatch for a batch of views on the MI355X (gfx950).
//
// Reference: SfMToyLib/SfMStereoUtilities.cpp:208-243 calls cv::solvePnPRansac (100 iterations, 10 px) once per view it wants
// to register.  Its sample stream is OpenCV's global RNG; the contract here (include/sfmba.h, sfmba_pnp_ransac) is our own and
// deterministic.  Three launches on one stream, no host round trip between them:
//
//   hypotheses   k_pnp_hypotheses: one lane per (problem, hypothesis), fp64, everything in registers (pnp_math.h): the seeded
//                sample, P3P in closed form, the fourth-point choice.  Writes the pose as [R|t] (fp64, the winner's goes to the
//                caller) and pre-multiplied by diag(fx, fy, 1) in fp32 (what the score reads), and the count 0 / -1 (invalid).
//   score        k_pnp_score: the hot loop, n_hyp x n projections.  A block = a tile of 64 hypotheses of one problem x chunks of
//                its points.  It stages a chunk of 1024 points once in LDS as (X, Y, Z, u - cx | v - cy): 20 B per point, a
//                float4 and a float array, so a point is one ds_read_b128 + one ds_read_b32.  The 4 waves of the block hold
//                the SAME 64 hypotheses (12 fp32 numbers per lane, in registers) and interleave the chunk's points, so every
//                lane of a wave reads the same LDS address: a broadcast, conflict-free.  pnp_inlier is 9 + 2 + 1 FMA,
//                3 multiplies and 2 compares per (hypothesis, point), no division.  One integer atomicAdd per lane and
//                chunk goes into hyp_count: integer sums do not depend on their order.
//   select +     k_pnp_select_refine: one block per problem.  Arg-max of (count, -h) over the hypotheses, the winner's mask with
//   refine       the same pnp_inlier (written in the first pass), then Gauss-Newton in fp64: a lane accumulates 21 + 6 + 1 sums (upper triangle of J^T J,
//                J^T r, the cost) over its points in ascending order, the wave reduces them with a fixed shuffle tree, the 4
//                waves through LDS in wave order, lane 0 factors the 6 x 6 matrix (Cholesky, unrolled into registers), applies
//                R <- exp([dw]x) R, t <- t + dt and broadcasts pose and verdict through LDS.  The pass after the last
//                step yields the cost at the returned pose, so there are steps + 1 passes.
#include "pnp_ransac.h"
#include "pnp_math.h"
#include "device_arena.h"

#include <algorithm>
#include <climits>
#include <vector>

namespace sfmba {

namespace {

constexpr int HYP_THREADS = 64;              // fp64 and register-hungry: small blocks spread a few hundred lanes over many CUs
constexpr int REFINE_BATCH = 4;             // points a lane of the refinement loads together
constexpr int N_SUMS = 28;                   // 21 (upper triangle of J^T J) + 6 (J^T r) + 1 (cost)

__global__ __launch_bounds__(HYP_THREADS) void k_pnp_hypotheses(long long n_items, int n_hyp, const long long* __restrict__ prob_ptr,
                                                                const float* __restrict__ xyz, const float* __restrict__ uv, PnpIntrinsics k,
                                                                uint64_t seed, double* __restrict__ hyp_pose, float* __restrict__ hyp_kp,
                                                                int* __restrict__ hyp_count) {
    const long long g = (long long)blockIdx.x * HYP_THREADS + threadIdx.x;
    if (g >= n_items) return;
    const long long p = g / n_hyp;
    const int h = (int)(g - p * n_hyp);
    const long long base = prob_ptr[p], n = prob_ptr[p + 1] - base;
    double pose[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) pose[j] = 0.0;
    long long i0, i1, i2, i3;
    bool ok = pnp_sample(pnp_mix(seed + (uint64_t)p), h, n, i0, i1, i2, i3);
    if (ok) {
        double X[4][3], o[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = base + (j == 0 ? i0 : (j == 1 ? i1 : (j == 2 ? i2 : i3)));
            X[j][0] = (double)xyz[3 * i]; X[j][1] = (double)xyz[3 * i + 1]; X[j][2] = (double)xyz[3 * i + 2];
            o[j][0] = (double)uv[2 * i];  o[j][1] = (double)uv[2 * i + 1];
        }
        ok = pnp_hypothesis(k, X, o, pose);
    }
    double* dst = hyp_pose + 12 * g;
    float* dkp = hyp_kp + 12 * g;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        dst[j] = pose[j];
        dkp[j] = (float)(j < 4 ? k.fx * pose[j] : (j < 8 ? k.fy * pose[j] : pose[j]));
    }
    hyp_count[g] = ok ? 0 : -1;
}

// hyp_count[p][h] += the number of inliers of hypothesis h among the points of the chunks this block walks.  An invalid
// hypothesis has an all-zero kp: depth 0, never an inlier, so its count stays -1.
__global__ __launch_bounds__(PNP_SCORE_THREADS) void k_pnp_score(int n_hyp, int tiles, const long long* __restrict__ prob_ptr,
                                                                 const float* __restrict__ xyz, const float* __restrict__ uv, float cx, float cy,
                                                                 float thr2, const float* __restrict__ hyp_kp, int* __restrict__ hyp_count) {
    __shared__ float4 sh_a[PNP_CHUNK];       // X, Y, Z, u - cx
    __shared__ float sh_b[PNP_CHUNK];        // v - cy
    const long long p = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - p * tiles);
    const long long base = prob_ptr[p], n = prob_ptr[p + 1] - base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = tile * PNP_TILE + lane;
    const long long slot = p * n_hyp + h;
    float kp[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) kp[j] = 0.0f;
    if (h < n_hyp) {
        const float4* src = reinterpret_cast<const float4*>(hyp_kp + 12 * slot);     // 48 B rows of a 256 B aligned array
        const float4 r0 = src[0], r1 = src[1], r2 = src[2];
        kp[0] = r0.x; kp[1] = r0.y; kp[2] = r0.z; kp[3] = r0.w;
        kp[4] = r1.x; kp[5] = r1.y; kp[6] = r1.z; kp[7] = r1.w;
        kp[8] = r2.x; kp[9] = r2.y; kp[10] = r2.z; kp[11] = r2.w;
    }
    const long long n_chunks = (n + PNP_CHUNK - 1) / PNP_CHUNK;
    for (long long c = blockIdx.y; c < n_chunks; c += gridDim.y) {
        const long long c0 = c * PNP_CHUNK;
        const int m = (int)min((long long)PNP_CHUNK, n - c0);
        __syncthreads();                                   // the previous chunk has been read by every wave
        for (int j = threadIdx.x; j < m; j += PNP_SCORE_THREADS) {
            const long long i = base + c0 + j;
            sh_a[j] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], uv[2 * i] - cx);
            sh_b[j] = uv[2 * i + 1] - cy;
        }
        __syncthreads();
        int cnt = 0;
#pragma unroll 4
        for (int j = wave; j < m; j += PNP_SCORE_THREADS / 64) {
            const float4 a = sh_a[j];                      // same address in every lane: broadcast
            const float b = sh_b[j];
            cnt += pnp_inlier(kp, a.x, a.y, a.z, a.w, b, thr2) ? 1 : 0;
        }
        if (cnt > 0 && h < n_hyp) atomicAdd(&hyp_count[slot], cnt);
    }
}

// lane 0 only: solve H d = -g by Cholesky.  H = the 21 entries of the upper triangle, row by row.  Every loop has constant bounds
// and is unrolled, so the factor lives in registers (an indexed 6 x 6 array would sit in scratch or cost an LDS round trip per
// entry on the one lane everybody waits for).  false = not positive definite / a non-finite value.
__device__ __forceinline__ bool chol6_solve(const double (&H)[21], const double (&g)[6], double (&d)[6]) {
    double L[6][6];
    {
        int s = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = r; c < 6; ++c) { L[c][r] = H[s]; ++s; }     // lower triangle
        }
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double v = L[j][j];
#pragma unroll
        for (int q = 0; q < j; ++q) v -= L[j][q] * L[j][q];
        ok = ok && v > 0.0 && isfinite(v);
        const double l = sqrt(v), il = 1.0 / l;
        L[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = L[i][j];
#pragma unroll
            for (int q = 0; q < j; ++q) t -= L[i][q] * L[j][q];
            L[i][j] = t * il;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {                            // L y = -g
        double t = -g[i];
#pragma unroll
        for (int q = 0; q < i; ++q) t -= L[i][q] * d[q];
        d[i] = t / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {                           // L^T d = y
        double t = d[i];
#pragma unroll
        for (int q = i + 1; q < 6; ++q) t -= L[q][i] * d[q];
        d[i] = t / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) ok = ok && isfinite(d[i]);
    return ok;
}

// lane 0 only: pose <- (exp([dw]x) R, t + dt)
__device__ __forceinline__ void apply_step(double (&pose)[12], const double (&d)[6]) {
    const double wx = d[0], wy = d[1], wz = d[2];
    const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
    const double A = th < 1e-8 ? 1.0 : sin(th) / th, B = th < 1e-8 ? 0.5 : (1.0 - cos(th)) / th2;
    // E = I + A W + B W^2, W^2 = w w^T - |w|^2 I
    const double E[9] = { 1.0 + B * (wx * wx - th2), -A * wz + B * wx * wy,       A * wy + B * wx * wz,
                          A * wz + B * wx * wy,       1.0 + B * (wy * wy - th2), -A * wx + B * wy * wz,
                          -A * wy + B * wx * wz,      A * wx + B * wy * wz,       1.0 + B * (wz * wz - th2) };
    double R[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = E[3 * r] * pose[c] + E[3 * r + 1] * pose[4 + c] + E[3 * r + 2] * pose[8 + c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pose[4 * r + c] = R[3 * r + c];
        pose[4 * r + 3] += d[3 + r];
    }
}

__global__ __launch_bounds__(PNP_REFINE_THREADS) void k_pnp_select_refine(int n_hyp, const long long* __restrict__ prob_ptr,
                                                                          const float* __restrict__ xyz, const float* __restrict__ uv,
                                                                          PnpIntrinsics k, float thr2, int max_iters,
                                                                          const double* __restrict__ hyp_pose, const float* __restrict__ hyp_kp,
                                                                          const int* __restrict__ hyp_count, double* __restrict__ pose_out,
                                                                          unsigned char* __restrict__ inlier, sfmba_pnp_result* __restrict__ result) {
    constexpr int WAVES = PNP_REFINE_THREADS / 64;
    __shared__ unsigned long long s_key[WAVES];
    __shared__ double s_red[WAVES][N_SUMS];
    __shared__ double s_pose[12];
    __shared__ int s_ctl;                                     // 0: a step was taken, 1: finished, 2: failed (status 3)
    const long long p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = prob_ptr[p];
    const int n = (int)(prob_ptr[p + 1] - base);
    const int* counts = hyp_count + p * n_hyp;

    // the winner: the largest (count, -h); key 0 = no valid hypothesis (a valid key has non-zero low bits: h < 65536)
    unsigned long long key = 0;
    for (int h = tid; h < n_hyp; h += PNP_REFINE_THREADS) {
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
    if (n < 4 || key == 0) {                                  // block-uniform
        if (tid == 0) {
            double* out = pose_out + 12 * p;
            for (int j = 0; j < 12; ++j) out[j] = (j == 0 || j == 5 || j == 10) ? 1.0 : 0.0;
            sfmba_pnp_result r;
            r.status = n < 4 ? 1 : 2; r.best_hypothesis = -1; r.n_inliers = 0; r.refine_iters = 0; r.refine_cost = 0.0;
            result[p] = r;
        }
        return;                                               // the mask stays zero (zeroed at allocation)
    }
    const int best = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
    const int n_inl = (int)(key >> 32);
    const long long slot = p * n_hyp + best;
    float kp[12];
    double P[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) { kp[j] = hyp_kp[12 * slot + j]; P[j] = hyp_pose[12 * slot + j]; }
    const float cxf = (float)k.cx, cyf = (float)k.cy;
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < 12; ++j) s_pose[j] = P[j];
    }
    const bool refine_on = max_iters > 0 && n_inl >= 4;
    int it = 0;
    double cost_w = 0.0, cost = 0.0;                          // lane 0's: the cost at the winner, at the returned pose
    bool converged = false;                                   // lane 0's
    int status = 0;
    for (;;) {
        double acc[N_SUMS];
#pragma unroll
        for (int j = 0; j < N_SUMS; ++j) acc[j] = 0.0;
        // a lane's points in ascending order, four at a time: the loads of a batch are issued together (one memory latency per
        // batch, not per point); the first pass also writes the winner's mask
        for (long long i0 = tid; i0 < n; i0 += REFINE_BATCH * PNP_REFINE_THREADS) {
            float Xf[REFINE_BATCH], Yf[REFINE_BATCH], Zf[REFINE_BATCH], uf[REFINE_BATCH], vf[REFINE_BATCH];
#pragma unroll
            for (int b = 0; b < REFINE_BATCH; ++b) {
                const long long i = i0 + b * PNP_REFINE_THREADS;
                const long long q = base + (i < n ? i : n - 1);          // n >= 4 here; a clamped read is never used
                Xf[b] = xyz[3 * q]; Yf[b] = xyz[3 * q + 1]; Zf[b] = xyz[3 * q + 2]; uf[b] = uv[2 * q]; vf[b] = uv[2 * q + 1];
            }
#pragma unroll
            for (int b = 0; b < REFINE_BATCH; ++b) {
                const long long i = i0 + b * PNP_REFINE_THREADS;
                if (i >= n) continue;
                const bool in = pnp_inlier(kp, Xf[b], Yf[b], Zf[b], uf[b] - cxf, vf[b] - cyf, thr2);
                if (it == 0) inlier[base + i] = in ? 1 : 0;
                if (!in) continue;
                const double X = Xf[b], Y = Yf[b], Z = Zf[b];
                const double qx = P[0] * X + P[1] * Y + P[2] * Z, qy = P[4] * X + P[5] * Y + P[6] * Z, qz = P[8] * X + P[9] * Y + P[10] * Z;
                const double x = qx + P[3], y = qy + P[7], z = qz + P[11];
                const double iz = 1.0 / z;
                const double ru = k.fx * x * iz + k.cx - (double)uf[b], rv = k.fy * y * iz + k.cy - (double)vf[b];
                const double a = k.fx * iz, bb = -k.fx * x * iz * iz, c = k.fy * iz, d = -k.fy * y * iz * iz;
                const double ju[6] = { bb * qy, a * qz - bb * qx, -a * qy, a, 0.0, bb };
                const double jv[6] = { -c * qz + d * qy, -d * qx, c * qx, 0.0, c, d };
                int s = 0;
#pragma unroll
                for (int r = 0; r < 6; ++r) {
#pragma unroll
                    for (int cc = r; cc < 6; ++cc) { acc[s] += ju[r] * ju[cc] + jv[r] * jv[cc]; ++s; }
                }
#pragma unroll
                for (int r = 0; r < 6; ++r) acc[21 + r] += ju[r] * ru + jv[r] * rv;
                acc[27] += 0.5 * (ru * ru + rv * rv);
            }
        }
#pragma unroll
        for (int j = 0; j < N_SUMS; ++j) {
            double v = acc[j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
            if (lane == 0) s_red[wave][j] = v;
        }
        __syncthreads();
        if (tid == 0) {
            int ctl;
            double sum[N_SUMS];
#pragma unroll
            for (int j = 0; j < N_SUMS; ++j) {
                double v = s_red[0][j];
#pragma unroll
                for (int w = 1; w < WAVES; ++w) v += s_red[w][j];
                sum[j] = v;
            }
            const double cur = sum[27];
            if (it == 0) cost_w = cur;
            if (!isfinite(cur)) {
                ctl = 2;
            } else if (!refine_on || it >= max_iters || converged) {
                ctl = 1;
                cost = cur;
            } else {
                double H[21], g[6], d[6];
#pragma unroll
                for (int j = 0; j < 21; ++j) H[j] = sum[j];
#pragma unroll
                for (int j = 0; j < 6; ++j) g[j] = sum[21 + j];
                ctl = 0;
                if (chol6_solve(H, g, d)) {
                    apply_step(P, d);                         // lane 0's copy; everybody reloads it from LDS below
                    double nn = 0.0;
                    bool fin = true;
#pragma unroll
                    for (int r = 0; r < 6; ++r) nn += d[r] * d[r];
#pragma unroll
                    for (int j = 0; j < 12; ++j) { fin = fin && isfinite(P[j]); s_pose[j] = P[j]; }
                    converged = sqrt(nn) < 1e-12;
                    if (!fin) ctl = 2;
                } else {
                    ctl = 2;
                }
            }
            if (ctl == 2) {                                   // the unrefined winner goes back
                const double* w = hyp_pose + 12 * slot;
#pragma unroll
                for (int j = 0; j < 12; ++j) s_pose[j] = w[j];
                cost = cost_w;
            }
            s_ctl = ctl;
        }
        __syncthreads();
        const int ctl = s_ctl;
#pragma unroll
        for (int j = 0; j < 12; ++j) P[j] = s_pose[j];
        if (ctl == 2) { status = 3; it = 0; break; }
        if (ctl == 1) break;
        ++it;
    }
    if (tid == 0) {
        double* out = pose_out + 12 * p;
#pragma unroll
        for (int j = 0; j < 12; ++j) out[j] = P[j];
        sfmba_pnp_result r;
        r.status = status; r.best_hypothesis = best; r.n_inliers = n_inl; r.refine_iters = it; r.refine_cost = cost;
        result[p] = r;
    }
}

}  // namespace

int pnp_ransac(hipStream_t s, int device, int n_prob, const int64_t* prob_ptr, const float* xyz, const float* uv, const float* K,
               int n_hyp, float threshold_px, uint64_t seed, int max_refine_iters, double* pose, unsigned char* inlier,
               sfmba_pnp_result* result, double* hyp_pose, int32_t* hyp_count, double* timing) {
    if (timing) for (int i = 0; i < 3; ++i) timing[i] = 0.0;
    if (n_prob <= 0) return 0;
    const long long total = prob_ptr[n_prob];
    const long long n_items = (long long)n_prob * n_hyp;
    const int tiles = (n_hyp + PNP_TILE - 1) / PNP_TILE;
    long long max_n = 0;
    for (int p = 0; p < n_prob; ++p) max_n = std::max<long long>(max_n, prob_ptr[p + 1] - prob_ptr[p]);
    // HIP launches at most 2^32 - 1 threads along a grid dimension
    const long long max_threads = 0xffffffffll;
    if (max_n >= (long long)INT_MAX || (long long)n_prob * tiles * PNP_SCORE_THREADS > max_threads || n_items + HYP_THREADS > max_threads ||
        (long long)n_prob * PNP_REFINE_THREADS > max_threads)
        return UNIT_ERR_TOO_LARGE;
    const PnpIntrinsics k{ (double)K[0], (double)K[4], (double)K[2], (double)K[5] };

    DeviceArena arena(device);
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    // allocations first (the arena zeroes them: the masks of status 1 / 2 problems stay zero), then the stream work
    long long* d_ptr;
    float *d_xyz, *d_uv, *d_kp;
    double *d_hpose, *d_pose;
    int* d_count;
    unsigned char* d_inl;
    sfmba_pnp_result* d_res;
    UNIT_ALLOC(arena, d_ptr, long long, (size_t)n_prob + 1);
    UNIT_ALLOC(arena, d_xyz, float, (size_t)3 * total);
    UNIT_ALLOC(arena, d_uv, float, (size_t)2 * total);
    UNIT_ALLOC(arena, d_hpose, double, (size_t)12 * n_items);
    UNIT_ALLOC(arena, d_kp, float, (size_t)12 * n_items);
    UNIT_ALLOC(arena, d_count, int, (size_t)n_items);
    UNIT_ALLOC(arena, d_pose, double, (size_t)12 * n_prob);
    UNIT_ALLOC(arena, d_inl, unsigned char, (size_t)total);
    UNIT_ALLOC(arena, d_res, sfmba_pnp_result, (size_t)n_prob);

    tm.begin(0);
    static_assert(sizeof(long long) == sizeof(int64_t), "prob_ptr is uploaded as it is");
    UNIT_TRY(hipMemcpyAsync(d_ptr, prob_ptr, sizeof(int64_t) * ((size_t)n_prob + 1), hipMemcpyHostToDevice, s));
    if (total > 0) {
        UNIT_TRY(hipMemcpyAsync(d_xyz, xyz, sizeof(float) * 3 * (size_t)total, hipMemcpyHostToDevice, s));
        UNIT_TRY(hipMemcpyAsync(d_uv, uv, sizeof(float) * 2 * (size_t)total, hipMemcpyHostToDevice, s));
    }
    tm.next(1);
    const float thr2 = threshold_px * threshold_px;
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3((unsigned)((n_items + HYP_THREADS - 1) / HYP_THREADS)), dim3(HYP_THREADS), 0, s, n_items, n_hyp,
                       d_ptr, d_xyz, d_uv, k, seed, d_hpose, d_kp, d_count);
    const long long max_chunks = (max_n + PNP_CHUNK - 1) / PNP_CHUNK;
    if (max_chunks > 0)
        hipLaunchKernelGGL(k_pnp_score, dim3((unsigned)(n_prob * tiles), (unsigned)std::min<long long>(max_chunks, PNP_MAX_CHUNK_BLOCKS)),
                           dim3(PNP_SCORE_THREADS), 0, s, n_hyp, tiles, d_ptr, d_xyz, d_uv, (float)k.cx, (float)k.cy, thr2, d_kp, d_count);
    hipLaunchKernelGGL(k_pnp_select_refine, dim3((unsigned)n_prob), dim3(PNP_REFINE_THREADS), 0, s, n_hyp, d_ptr, d_xyz, d_uv, k, thr2,
                       max_refine_iters, d_hpose, d_kp, d_count, d_pose, d_inl, d_res);
    UNIT_TRY(hipGetLastError());
    tm.next(2);
    UNIT_TRY(hipMemcpyAsync(pose, d_pose, sizeof(double) * 12 * (size_t)n_prob, hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(result, d_res, sizeof(sfmba_pnp_result) * (size_t)n_prob, hipMemcpyDeviceToHost, s));
    if (total > 0) UNIT_TRY(hipMemcpyAsync(inlier, d_inl, (size_t)total, hipMemcpyDeviceToHost, s));
    if (hyp_pose) UNIT_TRY(hipMemcpyAsync(hyp_pose, d_hpose, sizeof(double) * 12 * (size_t)n_items, hipMemcpyDeviceToHost, s));
    if (hyp_count) UNIT_TRY(hipMemcpyAsync(hyp_count, d_count, sizeof(int) * (size_t)n_items, hipMemcpyDeviceToHost, s));
    tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    if (timing) tm.collect(timing);
    return 0;
}

}  // namespace sfmba
