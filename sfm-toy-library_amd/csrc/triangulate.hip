// triangulate.hip -- two-view DLT triangulation + reprojection filter (gfx950), SURVEY 8(f) row 2.
//
// Device counterpart of SfMStereoUtilities::triangulateViews (SfMToyLib/SfMStereoUtilities.cpp:120-206); the per-match arithmetic is
// triangulate_match of triangulate_math.h, which both kernels here call.
//   k_triangulate        ALIGNED matches of ONE pair (sfmba_triangulate): one lane per match, the cameras are kernel arguments.
//   k_triangulate_pairs  the flattened match lists of MANY pairs (sfmba_triangulate_pairs) as sfmba_match_features returns them: one
//                        lane per entry.  The lane finds its pair by a binary search in pair_ptr (the largest p with
//                        pair_ptr[p] <= i: empty pairs are stepped over), gathers its two key points through query_idx /
//                        train_idx and reads its pair's P_left / P_right from device memory into registers -- n_pairs is unbounded,
//                        so they cannot be kernel arguments.  pair_ptr is a few KB that every lane walks the same way: it stays in
//                        cache, and the log2(n_pairs) dependent reads are what a lane pays for needing no host-side tile table.
//   kept list            a hipCUB exclusive scan over keep and k_tri_compact (entry i goes to slot pos[i]: ascending by
//                        construction, no atomics decide anything); kept_ptr[p] = pos[pair_ptr[p]].
// The pass is HBM-trivial (16 B in, 13 B out per match); it exists so that the step in front of bundle adjustment need not leave
// the GPU, and its batched form so that an added view costs one call and not one per good view.
#include "ba_kernels.h"
#include "device_arena.h"
#include "triangulate_math.h"
#include "unit_common.h"

#include <hipcub/hipcub.hpp>

namespace sfmba {

namespace {

struct TriCams {
    float K[9];
    float Pl[12];
    float Pr[12];
};

__global__ __launch_bounds__(256) void k_triangulate(long long n, const float2* __restrict__ left, const float2* __restrict__ right,
                                                     TriCams cams, float max_err, float* __restrict__ points3d,
                                                     unsigned char* __restrict__ keep, float* __restrict__ err) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 l = left[i], r = right[i];
    float X[3];
    double el, er;
    const bool kept = triangulate_match(l, r, cams.K, cams.Pl, cams.Pr, max_err, X, el, er);
    points3d[3 * i] = X[0]; points3d[3 * i + 1] = X[1]; points3d[3 * i + 2] = X[2];
    keep[i] = kept ? 1 : 0;
    if (err) { err[2 * i] = (float)el; err[2 * i + 1] = (float)er; }
}

struct TriK { float v[9]; };

// what a lane needs to find entry i: its pair p, x = pts[img_ptr[pair_left[p]] + query_idx[i]] -> x' likewise
struct TriProblem {
    const long long* img_ptr;
    const float2* pts;
    const int* pair_left;
    const int* pair_right;
    const long long* pair_ptr;
    const int* query_idx;
    const int* train_idx;
    const unsigned char* mask;               // or nullptr
    const float* P_left;                     // [n_pairs][12]
    const float* P_right;
};

// Entries i in [first, total), first = pair_ptr[0].  A masked entry is left as the arena handed it out: zero point, zero errors,
// keep 0; so is every entry in front of `first`, for which no lane runs.
__global__ __launch_bounds__(256) void k_triangulate_pairs(long long first, long long total, int n_pairs, TriProblem pr, TriK K, float max_err,
                                                           float* __restrict__ points3d, unsigned char* __restrict__ keep,
                                                           float* __restrict__ err) {
    const long long i = first + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    if (pr.mask && !pr.mask[i]) return;
    // the largest p with pair_ptr[p] <= i; pair_ptr[n_pairs] = total > i, so p + 1 <= n_pairs
    int lo = 0, hi = n_pairs;                // pair_ptr[lo] <= i < pair_ptr[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (pr.pair_ptr[mid] <= i) lo = mid; else hi = mid;
    }
    const long long p = lo;
    const float2 l = pr.pts[pr.img_ptr[pr.pair_left[p]] + (long long)pr.query_idx[i]];
    const float2 r = pr.pts[pr.img_ptr[pr.pair_right[p]] + (long long)pr.train_idx[i]];
    float Pl[12], Pr[12];
    const float4* sl = reinterpret_cast<const float4*>(pr.P_left + 12 * p);        // 48 B rows of a 256 B aligned array
    const float4* sr = reinterpret_cast<const float4*>(pr.P_right + 12 * p);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float4 a = sl[j], b = sr[j];
        Pl[4 * j] = a.x; Pl[4 * j + 1] = a.y; Pl[4 * j + 2] = a.z; Pl[4 * j + 3] = a.w;
        Pr[4 * j] = b.x; Pr[4 * j + 1] = b.y; Pr[4 * j + 2] = b.z; Pr[4 * j + 3] = b.w;
    }
    float X[3];
    double el, er;
    const bool kept = triangulate_match(l, r, K.v, Pl, Pr, max_err, X, el, er);
    points3d[3 * i] = X[0]; points3d[3 * i + 1] = X[1]; points3d[3 * i + 2] = X[2];
    keep[i] = kept ? 1 : 0;
    if (err) { err[2 * i] = (float)el; err[2 * i + 1] = (float)er; }
}

// pos = the exclusive scan of keep over [0, total]: kept entry i is number pos[i] of the list, pair p starts at pos[pair_ptr[p]]
__global__ __launch_bounds__(256) void k_tri_compact(long long total, int n_pairs, const unsigned char* __restrict__ keep,
                                                     const long long* __restrict__ pos, const long long* __restrict__ pair_ptr,
                                                     long long* __restrict__ kept_idx, long long* __restrict__ kept_ptr) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total && keep[i]) kept_idx[pos[i]] = i;
    if (i <= (long long)n_pairs) kept_ptr[i] = pos[pair_ptr[i]];
}

struct KeepToCount {
    __host__ __device__ long long operator()(unsigned char k) const { return k ? 1 : 0; }
};

}  // namespace

void launch_triangulate(hipStream_t s, long long n, const float* d_left, const float* d_right, const float K[9], const float Pl[12],
                        const float Pr[12], float max_err, float* d_points3d, unsigned char* d_keep, float* d_err) {
    if (n <= 0) return;
    TriCams cams;
    for (int e = 0; e < 9; ++e) cams.K[e] = K[e];
    for (int e = 0; e < 12; ++e) { cams.Pl[e] = Pl[e]; cams.Pr[e] = Pr[e]; }
    hipLaunchKernelGGL(k_triangulate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, reinterpret_cast<const float2*>(d_left),
                       reinterpret_cast<const float2*>(d_right), cams, max_err, d_points3d, d_keep, d_err);
}

int triangulate_pairs(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const float* pts, const float* K, int n_pairs,
                      const int32_t* pair_left, const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx,
                      const unsigned char* mask, const float* P_left, const float* P_right, float max_err, float* points3d, unsigned char* keep,
                      float* reproj_err, int64_t* kept_ptr, int64_t* kept_idx) {
    const long long first = pair_ptr[0], total = pair_ptr[n_pairs], n_pts = img_ptr[n_images];
    // total < 2^31 - 257 (the caller's check): the scan counts its items in an int, and a grid dimension holds 2^32 - 1 threads
    DeviceArena arena(device);
    // every return below, the early ones included, waits for what is queued on s before the arena's chunks go back to the cache
    struct StreamDrain { hipStream_t s; ~StreamDrain() { (void)hipStreamSynchronize(s); } } drain{ s };
    // allocations first (the arena zeroes them: masked entries and those in front of pair_ptr[0] stay zero), then the stream work
    long long *d_img, *d_ptr, *d_pos, *d_kidx, *d_kptr;
    float2* d_pts;
    int *d_left, *d_right, *d_query, *d_train;
    float *d_Pl, *d_Pr, *d_x, *d_e = nullptr;
    unsigned char *d_mask = nullptr, *d_keep;
    UNIT_ALLOC(arena, d_img, long long, (size_t)n_images + 1);
    UNIT_ALLOC(arena, d_pts, float2, (size_t)n_pts);
    UNIT_ALLOC(arena, d_left, int, (size_t)n_pairs);
    UNIT_ALLOC(arena, d_right, int, (size_t)n_pairs);
    UNIT_ALLOC(arena, d_ptr, long long, (size_t)n_pairs + 1);
    UNIT_ALLOC(arena, d_query, int, (size_t)total);
    UNIT_ALLOC(arena, d_train, int, (size_t)total);
    if (mask) UNIT_ALLOC(arena, d_mask, unsigned char, (size_t)total);
    UNIT_ALLOC(arena, d_Pl, float, (size_t)12 * n_pairs);
    UNIT_ALLOC(arena, d_Pr, float, (size_t)12 * n_pairs);
    UNIT_ALLOC(arena, d_x, float, (size_t)3 * total);
    if (reproj_err) UNIT_ALLOC(arena, d_e, float, (size_t)2 * total);
    UNIT_ALLOC(arena, d_keep, unsigned char, (size_t)total + 1);           // one past the end stays 0: the scan's last item
    UNIT_ALLOC(arena, d_pos, long long, (size_t)total + 1);
    UNIT_ALLOC(arena, d_kidx, long long, (size_t)total);
    UNIT_ALLOC(arena, d_kptr, long long, (size_t)n_pairs + 1);
    size_t scan_bytes = 0;
    hipcub::TransformInputIterator<long long, KeepToCount, const unsigned char*> keep_in(d_keep, KeepToCount());
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, keep_in, d_pos, (int)(total + 1), s));
    void* d_tmp = arena.alloc(scan_bytes ? scan_bytes : 1);
    if (!d_tmp) return (int)hipErrorOutOfMemory;

    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "the index arrays are uploaded as they are");
    UNIT_TRY(hipMemcpyAsync(d_img, img_ptr, sizeof(int64_t) * ((size_t)n_images + 1), hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_ptr, pair_ptr, sizeof(int64_t) * ((size_t)n_pairs + 1), hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_left, pair_left, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_right, pair_right, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_Pl, P_left, sizeof(float) * 12 * (size_t)n_pairs, hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_Pr, P_right, sizeof(float) * 12 * (size_t)n_pairs, hipMemcpyHostToDevice, s));
    if (n_pts > 0) UNIT_TRY(hipMemcpyAsync(d_pts, pts, sizeof(float) * 2 * (size_t)n_pts, hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_query, query_idx, sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_train, train_idx, sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, s));
    if (mask) UNIT_TRY(hipMemcpyAsync(d_mask, mask, (size_t)total, hipMemcpyHostToDevice, s));

    const TriProblem pr{ d_img, d_pts, d_left, d_right, d_ptr, d_query, d_train, d_mask, d_Pl, d_Pr };
    TriK Kv;
    for (int e = 0; e < 9; ++e) Kv.v[e] = K[e];
    hipLaunchKernelGGL(k_triangulate_pairs, dim3((unsigned)((total - first + 255) / 256)), dim3(256), 0, s, first, total, n_pairs, pr, Kv, max_err,
                       d_x, d_keep, d_e);
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, scan_bytes, keep_in, d_pos, (int)(total + 1), s));
    const long long lanes = total > (long long)n_pairs + 1 ? total : (long long)n_pairs + 1;
    hipLaunchKernelGGL(k_tri_compact, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, total, n_pairs, d_keep, d_pos, d_ptr, d_kidx, d_kptr);
    UNIT_TRY(hipGetLastError());
    UNIT_TRY(hipMemcpyAsync(points3d, d_x, sizeof(float) * 3 * (size_t)total, hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(keep, d_keep, (size_t)total, hipMemcpyDeviceToHost, s));
    if (reproj_err) UNIT_TRY(hipMemcpyAsync(reproj_err, d_e, sizeof(float) * 2 * (size_t)total, hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(kept_ptr, d_kptr, sizeof(int64_t) * ((size_t)n_pairs + 1), hipMemcpyDeviceToHost, s));
    // only the first kept_ptr[n_pairs] entries are defined; the rest of the buffer comes back as the arena's zeros
    UNIT_TRY(hipMemcpyAsync(kept_idx, d_kidx, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    return 0;
}

}  // namespace sfmba
