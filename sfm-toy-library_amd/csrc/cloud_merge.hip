// cloud_merge.hip -- the last step from images to a model on the MI355X (gfx950): a normal per depth pixel, and the voxel merge that
// turns the fused dense cloud (one point per view that saw a surface element) into one oriented point per occupied voxel.
//
// The contract is the project's own (include/sfmba.h, sfmba_depth_normals / sfmba_cloud_merge; arithmetic in cloud_math.h): fp64 with
// every operation rounded on its own per element, and NOTHING BUT INTEGERS is summed over a voxel -- so the result does not depend on
// the order of accumulation and is BIT-EXACT with a CPU restatement.
//
//   normals       k_depth_normals: one lane per pixel of an image with a map (grid.y = image); central or one-sided differences of
//                 the back-projected neighbours, cross product, turned to the camera, rotated to the world.
//   quantise      k_cloud_keys: one lane per point -> (key, index); a skipped point gets a key above every valid one.
//   sort          rocPRIM's stable radix sort of the pairs with the structure build's configuration (sort_pairs_u64).  Stable and
//                 fed ascending indices: the members of a run stand in ascending input index, so `first` is the run's first entry.
//   runs          k_cloud_heads (a run begins where the key changes), a hipCUB inclusive sum (the run number of every sorted
//                 position), k_cloud_starts (run_start [n_runs + 1], n_runs and the number of valid points).
//   reduce        NO ATOMIC TOUCHES A SUM.  k_cloud_reduce_short: one lane per run walks its 1 .. CLOUD_SHORT_RUN members, gathers
//                 each point through the sorted index, quantises it again (12 bytes read instead of 24 written and read) and keeps
//                 the nine sums in registers; a longer run is appended to a list (one int atomic per LONG run, at most n / 33 of
//                 them).  k_cloud_reduce_long: resident waves walk that list, a wave per run, lanes striding over the members, a
//                 shuffle tree at the end.  The sums leave as [sum][run] so that a wave's stores are contiguous.
//   compact       k_cloud_keep (count >= min_count), a hipCUB exclusive sum -> the output row of every kept run; k_cloud_voxel_of.
//   finalise      k_cloud_finalise: one lane per kept run, the arithmetic of cloud_math.h.
#include "cloud_merge.h"
#include "cloud_math.h"
#include "ba_kernels.h"    // sort_pairs_u64
#include "device_arena.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;
constexpr int WAVE = 64;
constexpr int LONG_BLOCKS = 1024;      // resident workgroups of the long-run kernel: 4096 waves walk the list

typedef unsigned long long u64;

// ---- normals -------------------------------------------------------------------------------------------------------------------
struct NormalImage {
    double P[12];
    long long off;           // first pixel of its map among the maps on the device, -1: none
    int w, h;
};
struct NormalParams { double k4[4]; double max_rel_step; };

__global__ __launch_bounds__(LANES) void k_depth_normals(const NormalImage* __restrict__ tab, NormalParams prm, const float* __restrict__ maps,
                                                         float* __restrict__ normal) {
    const NormalImage& T = tab[blockIdx.y];
    const long long q = (long long)blockIdx.x * LANES + threadIdx.x;
    if (T.off < 0 || q >= (long long)T.w * T.h) return;
    float n[3] = { 0.0f, 0.0f, 0.0f };
    cloud_pixel_normal(prm.k4, T.P, maps + T.off, T.w, T.h, (int)(q % T.w), (int)(q / T.w), prm.max_rel_step, n, nullptr);
    float* o = normal + 3 * (T.off + q);
    o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
}

// ---- merge ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void k_cloud_keys(int n, const float* __restrict__ xyz, double voxel, u64* __restrict__ keys, int* __restrict__ idx) {
    const int i = blockIdx.x * LANES + threadIdx.x;
    if (i >= n) return;
    const float p[3] = { xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2] };
    long long q[3];
    keys[i] = cloud_key(p, voxel, q);
    idx[i] = i;
}

__global__ __launch_bounds__(LANES) void k_cloud_heads(int n, const u64* __restrict__ ks, int* __restrict__ head) {
    const int p = blockIdx.x * LANES + threadIdx.x;
    if (p >= n) return;
    const u64 k = ks[p];
    head[p] = (k != CLOUD_KEY_SKIPPED && (p == 0 || ks[p - 1] != k)) ? 1 : 0;
}

// run_start [n_runs + 1]; info[0] = n_runs, info[1] = the number of valid points (both stay 0, as handed out, when none is valid)
__global__ __launch_bounds__(LANES) void k_cloud_starts(int n, const u64* __restrict__ ks, const int* __restrict__ head, const int* __restrict__ rank,
                                                        int* __restrict__ run_start, int* __restrict__ info) {
    const int p = blockIdx.x * LANES + threadIdx.x;
    if (p >= n || ks[p] == CLOUD_KEY_SKIPPED) return;
    const int r = rank[p];                                   // 1-based run number
    if (head[p]) run_start[r - 1] = p;
    if (p == n - 1 || ks[p + 1] == CLOUD_KEY_SKIPPED) {
        run_start[r] = p + 1;
        info[0] = r;
        info[1] = p + 1;
    }
}

// the sums of a run, [sum][run]: q 0..2, then m 0..2 (with normals), then b, g, r (with colours)
struct RunSums {
    long long* q;
    long long* m;            // NULL without normals
    long long* b;            // NULL without colours
    long long stride;        // n_runs
};
struct MergeIn {
    const float* xyz;
    const unsigned char* bgr;
    const float* normal;
    double voxel;
};

__device__ __forceinline__ void cloud_add_member(const MergeIn& in, int i, long long* acc) {
    const float p[3] = { in.xyz[3 * (size_t)i], in.xyz[3 * (size_t)i + 1], in.xyz[3 * (size_t)i + 2] };
    long long q[3];
    cloud_key(p, in.voxel, q);
    for (int a = 0; a < 3; ++a) acc[a] += q[a];
    if (in.normal)
        for (int a = 0; a < 3; ++a) acc[3 + a] += cloud_normal_quantum(in.normal[3 * (size_t)i + a]);
    if (in.bgr)
        for (int a = 0; a < 3; ++a) acc[6 + a] += (long long)in.bgr[3 * (size_t)i + a];
}
__device__ __forceinline__ void cloud_store_sums(const RunSums& out, int r, const long long* acc) {
    for (int a = 0; a < 3; ++a) out.q[a * out.stride + r] = acc[a];
    if (out.m) for (int a = 0; a < 3; ++a) out.m[a * out.stride + r] = acc[3 + a];
    if (out.b) for (int a = 0; a < 3; ++a) out.b[a * out.stride + r] = acc[6 + a];
}

__global__ __launch_bounds__(LANES) void k_cloud_reduce_short(int n_runs, const int* __restrict__ run_start, const int* __restrict__ is, MergeIn in,
                                                              RunSums out, int* __restrict__ long_list, int long_cap, int* __restrict__ n_long) {
    const int r = blockIdx.x * LANES + threadIdx.x;
    if (r >= n_runs) return;
    const int beg = run_start[r], end = run_start[r + 1];
    if (end - beg > CLOUD_SHORT_RUN) {
        const int slot = atomicAdd(n_long, 1);
        if (slot < long_cap) long_list[slot] = r;            // cannot fail: long_cap = n_valid / (CLOUD_SHORT_RUN + 1) + 1
        return;
    }
    long long acc[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    for (int p = beg; p < end; ++p) cloud_add_member(in, is[p], acc);
    cloud_store_sums(out, r, acc);
}

__global__ __launch_bounds__(LANES) void k_cloud_reduce_long(const int* __restrict__ run_start, const int* __restrict__ is, MergeIn in, RunSums out,
                                                             const int* __restrict__ long_list, int long_cap, const int* __restrict__ n_long) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = (blockIdx.x * LANES + threadIdx.x) / WAVE, n_waves = gridDim.x * (LANES / WAVE);
    const int todo = min(*n_long, long_cap);
    for (int at = wave; at < todo; at += n_waves) {           // uniform over the wave
        const int r = long_list[at];
        const int beg = run_start[r], end = run_start[r + 1];
        long long acc[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        for (int p = beg + lane; p < end; p += WAVE) cloud_add_member(in, is[p], acc);
        for (int k = 0; k < 9; ++k)
            for (int d = WAVE / 2; d >= 1; d >>= 1) acc[k] += __shfl_down(acc[k], d, WAVE);
        if (lane == 0) cloud_store_sums(out, r, acc);
    }
}

__global__ __launch_bounds__(LANES) void k_cloud_keep(int n_runs, const int* __restrict__ run_start, int min_count, int* __restrict__ keep) {
    const int r = blockIdx.x * LANES + threadIdx.x;
    if (r >= n_runs) return;
    keep[r] = (run_start[r + 1] - run_start[r] >= min_count) ? 1 : 0;
}

__global__ __launch_bounds__(LANES) void k_cloud_voxel_of(int n, int n_valid, const int* __restrict__ is, const int* __restrict__ rank,
                                                          const int* __restrict__ keep, const int* __restrict__ pos, int* __restrict__ voxel_of) {
    const int p = blockIdx.x * LANES + threadIdx.x;
    if (p >= n) return;
    int o = -1;
    if (p < n_valid) {
        const int r = rank[p] - 1;
        if (keep[r]) o = pos[r];
    }
    voxel_of[is[p]] = o;
}

__global__ __launch_bounds__(LANES) void k_cloud_finalise(int n_runs, const int* __restrict__ run_start, const int* __restrict__ is,
                                                          const int* __restrict__ keep, const int* __restrict__ pos, RunSums sums, double voxel,
                                                          float* __restrict__ xyz, unsigned char* __restrict__ bgr, float* __restrict__ normal,
                                                          int* __restrict__ count, int* __restrict__ first) {
    const int r = blockIdx.x * LANES + threadIdx.x;
    if (r >= n_runs || !keep[r]) return;
    const size_t o = (size_t)pos[r];
    const int beg = run_start[r], c = run_start[r + 1] - beg;
    for (int a = 0; a < 3; ++a) xyz[3 * o + a] = cloud_final_coord(sums.q[a * sums.stride + r], c, voxel);
    if (sums.b)
        for (int a = 0; a < 3; ++a) bgr[3 * o + a] = cloud_final_colour(sums.b[a * sums.stride + r], c);
    if (sums.m) {
        const long long Sm[3] = { sums.m[r], sums.m[sums.stride + r], sums.m[2 * sums.stride + r] };
        float nrm[3];
        cloud_final_normal(Sm, nrm);
        for (int a = 0; a < 3; ++a) normal[3 * o + a] = nrm[a];
    }
    count[o] = c;
    first[o] = is[beg];
}

unsigned blocks_for(long long n) { return (unsigned)((n + LANES - 1) / LANES); }

}  // namespace

int depth_normals(hipStream_t s, int device, int n_images, const int32_t* width, const int32_t* height, const float* K, const float* P,
                  const float* const* depth, float max_rel_step, float* const* normal, double* timing) {
    if (timing) for (int i = 0; i < NORMALS_T_COUNT; ++i) timing[i] = 0.0;
    std::vector<NormalImage> tab((size_t)std::max(n_images, 1));
    long long n_dom = 0, max_px = 0;
    for (int i = 0; i < n_images; ++i) {
        NormalImage& T = tab[(size_t)i];
        std::memset(&T, 0, sizeof(T));
        for (int q = 0; q < 12; ++q) T.P[q] = (double)P[(size_t)i * 12 + q];
        T.w = width[i]; T.h = height[i];
        T.off = -1;
        if (depth[i]) {
            const long long px = (long long)T.w * T.h;
            T.off = n_dom;
            n_dom += px;
            max_px = std::max(max_px, px);
        }
    }
    if (n_dom == 0) return 0;

    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    DeviceArena scratch(device);
    NormalImage* d_tab;
    float *d_maps, *d_normal;
    UNIT_ALLOC(scratch, d_tab, NormalImage, tab.size());
    UNIT_ALLOC(scratch, d_maps, float, (size_t)n_dom);
    UNIT_ALLOC(scratch, d_normal, float, (size_t)n_dom * 3);

    tm.begin(NORMALS_T_UPLOAD);
    UNIT_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(NormalImage) * tab.size(), hipMemcpyHostToDevice, s));
    for (int i = 0; i < n_images; ++i)
        if (depth[i])
            UNIT_TRY(hipMemcpyAsync(d_maps + tab[(size_t)i].off, depth[i], sizeof(float) * (size_t)width[i] * height[i], hipMemcpyHostToDevice, s));
    tm.end();

    NormalParams prm;
    prm.k4[0] = (double)K[0]; prm.k4[1] = (double)K[4]; prm.k4[2] = (double)K[2]; prm.k4[3] = (double)K[5];
    prm.max_rel_step = (double)max_rel_step;
    tm.begin(NORMALS_T_KERNEL);
    hipLaunchKernelGGL(k_depth_normals, dim3(blocks_for(max_px), (unsigned)n_images), dim3(LANES), 0, s, d_tab, prm, d_maps, d_normal);
    UNIT_TRY(hipGetLastError());
    tm.end();
    tm.begin(NORMALS_T_DOWNLOAD);
    for (int i = 0; i < n_images; ++i)
        if (depth[i])
            UNIT_TRY(hipMemcpyAsync(normal[i], d_normal + 3 * tab[(size_t)i].off, sizeof(float) * 3 * (size_t)width[i] * height[i],
                                     hipMemcpyDeviceToHost, s));
    tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    if (timing) tm.collect(timing);
    return 0;
}

int cloud_merge(hipStream_t s, int device, int n, const float* xyz, const unsigned char* bgr, const float* normal, float voxel, int min_count,
                float* xyz_out, unsigned char* bgr_out, float* normal_out, int32_t* count, int32_t* first, int32_t* voxel_of, int64_t cap,
                int64_t* total, int64_t* n_skipped, double* timing) {
    *total = 0;
    *n_skipped = 0;
    if (timing) for (int i = 0; i < MERGE_T_COUNT; ++i) timing[i] = 0.0;
    if (n <= 0) return 0;

    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    DeviceArena scratch(device);
    const size_t N = (size_t)n;
    float *d_xyz, *d_normal = nullptr;
    unsigned char* d_bgr = nullptr;
    u64 *d_k0, *d_k1;
    int *d_i0, *d_i1, *d_head, *d_rank, *d_start, *d_info;
    UNIT_ALLOC(scratch, d_xyz, float, N * 3);
    if (bgr) UNIT_ALLOC(scratch, d_bgr, unsigned char, N * 3);
    if (normal) UNIT_ALLOC(scratch, d_normal, float, N * 3);
    UNIT_ALLOC(scratch, d_k0, u64, N);
    UNIT_ALLOC(scratch, d_k1, u64, N);
    UNIT_ALLOC(scratch, d_i0, int, N);
    UNIT_ALLOC(scratch, d_i1, int, N);
    UNIT_ALLOC(scratch, d_head, int, N + 1);                 // voxel_of reuses it once the runs are known
    UNIT_ALLOC(scratch, d_rank, int, N + 1);
    UNIT_ALLOC(scratch, d_start, int, N + 1);
    UNIT_ALLOC(scratch, d_info, int, 4);                     // n_runs, n_valid, n_long: zero as handed out
    size_t sort_bytes = 0, scan_a = 0, scan_b = 0;
    // every bit of a key is significant: an index carries the bias 2^20 in its field, and the key of a skipped point has bit 63
    const int end_bit = 64;
    if (int rc = sort_pairs_u64(s, nullptr, &sort_bytes, d_k0, d_k1, d_i0, d_i1, (unsigned)n, end_bit)) return rc;
    UNIT_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_a, d_head, d_rank, n, s));
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, d_head, d_rank, n + 1, s));
    const size_t tmp_bytes = std::max(std::max(sort_bytes, scan_a), std::max(scan_b, (size_t)1));
    void* d_tmp = scratch.alloc(tmp_bytes);
    if (!d_tmp) return (int)hipErrorOutOfMemory;

    tm.begin(MERGE_T_UPLOAD);
    UNIT_TRY(hipMemcpyAsync(d_xyz, xyz, sizeof(float) * N * 3, hipMemcpyHostToDevice, s));
    if (bgr) UNIT_TRY(hipMemcpyAsync(d_bgr, bgr, N * 3, hipMemcpyHostToDevice, s));
    if (normal) UNIT_TRY(hipMemcpyAsync(d_normal, normal, sizeof(float) * N * 3, hipMemcpyHostToDevice, s));
    tm.end();

    const double vox = (double)voxel;
    tm.begin(MERGE_T_QUANTISE);
    hipLaunchKernelGGL(k_cloud_keys, dim3(blocks_for(n)), dim3(LANES), 0, s, n, d_xyz, vox, d_k0, d_i0);
    UNIT_TRY(hipGetLastError());
    tm.end();
    tm.begin(MERGE_T_SORT);
    {
        size_t bytes = sort_bytes;
        if (int rc = sort_pairs_u64(s, d_tmp, &bytes, d_k0, d_k1, d_i0, d_i1, (unsigned)n, end_bit)) return rc;
    }
    tm.end();
    const u64* ks = d_k1;
    const int* is = d_i1;
    tm.begin(MERGE_T_RUNS);
    hipLaunchKernelGGL(k_cloud_heads, dim3(blocks_for(n)), dim3(LANES), 0, s, n, ks, d_head);
    UNIT_TRY(hipGetLastError());
    {
        size_t bytes = scan_a;
        UNIT_TRY(hipcub::DeviceScan::InclusiveSum(d_tmp, bytes, d_head, d_rank, n, s));
    }
    hipLaunchKernelGGL(k_cloud_starts, dim3(blocks_for(n)), dim3(LANES), 0, s, n, ks, d_head, d_rank, d_start, d_info);
    UNIT_TRY(hipGetLastError());
    int info[2] = { 0, 0 };
    UNIT_TRY(hipMemcpyAsync(info, d_info, sizeof(info), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    tm.end();
    const int n_runs = info[0], n_valid = info[1];
    *n_skipped = (int64_t)n - n_valid;
    if (n_runs == 0) {
        if (voxel_of) for (int i = 0; i < n; ++i) voxel_of[i] = -1;
        if (timing) tm.collect(timing);
        return 0;
    }

    const size_t R = (size_t)n_runs;
    RunSums sums;
    sums.stride = n_runs;
    sums.m = nullptr;
    sums.b = nullptr;
    UNIT_ALLOC(scratch, sums.q, long long, R * 3);
    if (normal) UNIT_ALLOC(scratch, sums.m, long long, R * 3);
    if (bgr) UNIT_ALLOC(scratch, sums.b, long long, R * 3);
    const int long_cap = n_valid / (CLOUD_SHORT_RUN + 1) + 1;
    int *d_long, *d_keep, *d_pos;
    UNIT_ALLOC(scratch, d_long, int, (size_t)long_cap);
    UNIT_ALLOC(scratch, d_keep, int, R + 1);                 // zeroed: the last flag stays 0
    UNIT_ALLOC(scratch, d_pos, int, R + 1);
    const MergeIn in{ d_xyz, d_bgr, d_normal, vox };

    tm.begin(MERGE_T_REDUCE);
    hipLaunchKernelGGL(k_cloud_reduce_short, dim3(blocks_for(n_runs)), dim3(LANES), 0, s, n_runs, d_start, is, in, sums, d_long, long_cap, d_info + 2);
    UNIT_TRY(hipGetLastError());
    if (n_valid > CLOUD_SHORT_RUN) {
        const unsigned grid = (unsigned)std::min<long long>(LONG_BLOCKS, ((long long)long_cap + LANES / WAVE - 1) / (LANES / WAVE));
        hipLaunchKernelGGL(k_cloud_reduce_long, dim3(grid), dim3(LANES), 0, s, d_start, is, in, sums, d_long, long_cap, d_info + 2);
        UNIT_TRY(hipGetLastError());
    }
    tm.end();
    tm.begin(MERGE_T_COMPACT);
    hipLaunchKernelGGL(k_cloud_keep, dim3(blocks_for(n_runs)), dim3(LANES), 0, s, n_runs, d_start, min_count, d_keep);
    UNIT_TRY(hipGetLastError());
    {
        size_t bytes = scan_b;                                // sized for n + 1 >= n_runs + 1 items
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, bytes, d_keep, d_pos, n_runs + 1, s));
    }
    int tot = 0;
    UNIT_TRY(hipMemcpyAsync(&tot, d_pos + n_runs, sizeof(int), hipMemcpyDeviceToHost, s));
    if (voxel_of) {
        int* d_vox = d_head;                                  // the head flags are spent
        hipLaunchKernelGGL(k_cloud_voxel_of, dim3(blocks_for(n)), dim3(LANES), 0, s, n, n_valid, is, d_rank, d_keep, d_pos, d_vox);
        UNIT_TRY(hipGetLastError());
        UNIT_TRY(hipMemcpyAsync(voxel_of, d_vox, sizeof(int) * N, hipMemcpyDeviceToHost, s));
    }
    UNIT_TRY(hipStreamSynchronize(s));
    tm.end();
    *total = tot;
    if (tot > cap) return UNIT_ERR_CAPACITY;
    if (tot > 0) {
        const size_t T = (size_t)tot;
        float *d_oxyz, *d_onrm = nullptr;
        unsigned char* d_obgr = nullptr;
        int *d_count, *d_first;
        UNIT_ALLOC(scratch, d_oxyz, float, T * 3);
        if (bgr) UNIT_ALLOC(scratch, d_obgr, unsigned char, T * 3);
        if (normal) UNIT_ALLOC(scratch, d_onrm, float, T * 3);
        UNIT_ALLOC(scratch, d_count, int, T);
        UNIT_ALLOC(scratch, d_first, int, T);
        tm.begin(MERGE_T_FINALISE);
        hipLaunchKernelGGL(k_cloud_finalise, dim3(blocks_for(n_runs)), dim3(LANES), 0, s, n_runs, d_start, is, d_keep, d_pos, sums, vox, d_oxyz, d_obgr,
                           d_onrm, d_count, d_first);
        UNIT_TRY(hipGetLastError());
        tm.end();
        tm.begin(MERGE_T_DOWNLOAD);
        UNIT_TRY(hipMemcpyAsync(xyz_out, d_oxyz, sizeof(float) * T * 3, hipMemcpyDeviceToHost, s));
        if (bgr && bgr_out) UNIT_TRY(hipMemcpyAsync(bgr_out, d_obgr, T * 3, hipMemcpyDeviceToHost, s));
        if (normal && normal_out) UNIT_TRY(hipMemcpyAsync(normal_out, d_onrm, sizeof(float) * T * 3, hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipMemcpyAsync(count, d_count, sizeof(int) * T, hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipMemcpyAsync(first, d_first, sizeof(int) * T, hipMemcpyDeviceToHost, s));
        tm.end();
        UNIT_TRY(hipStreamSynchronize(s));
    }
    if (timing) tm.collect(timing);
    return 0;
}

}  // namespace sfmba
