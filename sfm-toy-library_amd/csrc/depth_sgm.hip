// depth_sgm.hip -- semi-global matching over the plane sweep's cost volume on the MI355X (gfx950).
//
// The contract is the project's own (include/sfmba.h, sfmba_depth_cost_volume / sfmba_sgm_aggregate / sfmba_depth_sweep_sgm;
// arithmetic in sgm_math.h): integers from the quantised cost to the selection, three fp64 expressions at the ends -- so the result is
// BIT-EXACT with a CPU restatement (tests/sgm_oracle.py).
//
//   volume        k_depth_sweep<R, true> of depth_sweep.hip: uint8 [pixel][D], the plane index fastest, so the D costs of one pixel
//                 are one contiguous run.
//   aggregate     k_sgm_path<NP, FIRST, FULL>: ONE WAVE OWNS ONE PATH LINE of one direction, lane l owns the planes l, l + 64, .. (NP = ceil(D / 64)
//                 of them, in registers).  A step is a dependent chain -- the d - 1 / d + 1 neighbours come across lanes
//                 (ds_bpermute), the minimum over the planes is a butterfly in the VALU (the DPP / permlane exchanges of
//                 sfmba_device.h), then the update -- so the D cost bytes of the NEXT pixel are fetched RAW at the top of a step, together
//                 with the sums the step adds to, and both are first read after the update (FULL: D = 64 NP, no lane idles, and that
//                 is what the code object does; otherwise see the loop).  A workgroup holds four adjacent lines: for vertical and diagonal directions its waves read adjacent
//                 runs.  ONE LAUNCH PER DIRECTION, and S += L is a plain read-modify-write: within a direction every (pixel, plane)
//                 lies on exactly one line, so exactly one lane touches it, and the launches of one stream follow each other.  The
//                 first direction (FIRST) stores instead of adding, so S needs no clearing.  (The alternative, integer atomics from all
//                 directions at once, has no 16-bit form on this device: it would double S or need compare-and-swap on pairs.)
//   select        k_sgm_select<NP>: a wave per pixel at a time over its D sums, two butterflies (the key S * 256 + d gives the lowest
//                 plane of the smallest sum; then the smallest sum further than one plane away).
//   finish        k_sgm_finish: a lane per pixel -- the uniqueness test, the parabola through the sums beside k*, depth and score.
#include "depth_sgm.h"
#include "device_arena.h"
#include "sfmba_device.h"
#include "sgm_math.h"

#include <algorithm>
#include <climits>
#include <vector>

namespace sfmba {

namespace {

constexpr int SGM_WAVES = 4;                   // path lines per workgroup
constexpr int SGM_LANES = 64 * SGM_WAVES;

struct SgmJob { long long px_off; int w, h; double wf, step; };

__device__ __forceinline__ int wave_min(int v) {
    v = min(v, xlane_get_i<32>(v)); v = min(v, xlane_get_i<16>(v)); v = min(v, xlane_get_i<8>(v));
    v = min(v, xlane_get_i<4>(v)); v = min(v, xlane_get_i<2>(v)); v = min(v, xlane_get_i<1>(v));
    return v;
}

template <int NP, bool FIRST, bool FULL>
__global__ __launch_bounds__(SGM_LANES) void k_sgm_path(const SgmJob* __restrict__ jobs, const unsigned char* __restrict__ cost,
                                                        uint16_t* __restrict__ sums, int D, int p1, int p2, int invalid_cost, int dx, int dy) {
    const SgmJob J = jobs[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = (int)blockIdx.x * SGM_WAVES + wave;
    if (l >= sgm_lines(dx, dy, J.w, J.h)) return;             // uniform over the wave; the kernel has no barrier
    int x, y;
    sgm_line_start(dx, dy, J.w, J.h, l, x, y);
    const int nx = dx > 0 ? J.w - x : dx < 0 ? x + 1 : INT_MAX, ny = dy > 0 ? J.h - y : dy < 0 ? y + 1 : INT_MAX;
    const int n = nx < ny ? nx : ny;                          // pixels on the line: every one of them inside the image

    // A lane whose plane does not exist (d >= D) loads the pixel's last plane instead and never stores: every load of the loop is
    // unconditional and inside the pixel's run, so none of them sits behind a branch on the lane.
    bool act[NP];
    int off[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        act[i] = FULL || lane + 64 * i < D;                   // FULL: D == 64 NP, known when the kernel is compiled: no lane idles
        off[i] = act[i] ? lane + 64 * i : D - 1;
    }
    long long e = (J.px_off + (long long)y * J.w + x) * D;                 // plane 0 of the pixel
    const long long stride = ((long long)dy * J.w + dx) * D;
    int L[NP], c[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        L[i] = SGM_FAR;
        c[i] = sgm_cost(cost[e + off[i]], invalid_cost);
    }
    for (int t = 0; t < n; ++t) {
        // The step's two loads are issued here, ahead of the chain, which needs neither: the sums this step adds to and the RAW cost
        // bytes of the next pixel.  Both are first read after the update, at the bottom of the step.  In the code object (read from
        // the disassembly): with FULL both loads stand at the top of the loop and the one wait for them after the butterfly; where
        // lanes idle (D is no multiple of 64) the compiler sinks the sums' load into the store's branch, so there only the cost fetch
        // overlaps the chain and the read-modify-write of S is a round trip of its own at the end of each step.
        int old[NP];
        unsigned char nxt[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) old[i] = FIRST ? 0 : (int)sums[e + off[i]];
        const long long ahead = e + (t + 1 < n ? stride : 0);             // the line's last pixel fetches itself again: no branch
#pragma unroll
        for (int i = 0; i < NP; ++i) nxt[i] = cost[ahead + off[i]];
        if (t == 0) {
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (act[i]) L[i] = c[i];
        } else {
            int m = L[0], up[NP], dn[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                m = L[i] < m ? L[i] : m;                      // a plane that does not exist holds SGM_FAR
                up[i] = __shfl(L[i], (lane + 63) & 63);       // plane d - 1; lane 0 receives lane 63's, which it needs of the slab BEFORE
                dn[i] = __shfl(L[i], (lane + 1) & 63);        // plane d + 1; lane 63 receives lane 0's, which it needs of the NEXT slab
            }
            m = wave_min(m);
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const int lo = lane > 0 ? up[i] : (i > 0 ? up[i > 0 ? i - 1 : 0] : SGM_FAR);
                const int hi = lane < 63 ? dn[i] : (i < NP - 1 ? dn[i < NP - 1 ? i + 1 : 0] : SGM_FAR);
                const int step = sgm_step(c[i], L[i], lo, hi, m, p1, p2);
                L[i] = act[i] ? step : SGM_FAR;
            }
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            c[i] = sgm_cost(nxt[i], invalid_cost);            // before the store: the next step then waits for no store
            if (act[i]) sums[e + off[i]] = (uint16_t)(old[i] + L[i]);
        }
        e += stride;
    }
}

template <int NP>
__global__ __launch_bounds__(SGM_LANES) void k_sgm_select(const uint16_t* __restrict__ sums, long long n_px, int D, int16_t* __restrict__ plane,
                                                          uint16_t* __restrict__ best, uint16_t* __restrict__ second) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long p = (long long)blockIdx.x * SGM_WAVES + wave; p < n_px; p += (long long)gridDim.x * SGM_WAVES) {
        const uint16_t* S = sums + p * D;
        int v[NP], key = INT_MAX;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int d = lane + 64 * i;
            v[i] = d < D ? (int)S[d] : 0;
            if (d < D && v[i] * 256 + d < key) key = v[i] * 256 + d;       // S <= 10216: the key stays below 2^22
        }
        key = wave_min(key);
        const int k = key & 255;
        int sec = SGM_NO_SECOND;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int d = lane + 64 * i;
            if (d < D && (d < k - 1 || d > k + 1) && v[i] < sec) sec = v[i];
        }
        sec = wave_min(sec);
        if (lane == 0) {
            plane[p] = (int16_t)k;
            best[p] = (uint16_t)(key >> 8);
            second[p] = (uint16_t)sec;
        }
    }
}

__global__ __launch_bounds__(SGM_LANES) void k_sgm_finish(const SgmJob* __restrict__ jobs, const unsigned char* __restrict__ cost,
                                                          const uint16_t* __restrict__ sums, const int16_t* __restrict__ plane,
                                                          const uint16_t* __restrict__ best, const uint16_t* __restrict__ second, int D,
                                                          int uniqueness, float* __restrict__ depth, float* __restrict__ score) {
    const SgmJob J = jobs[blockIdx.y];
    const long long q = (long long)blockIdx.x * SGM_LANES + threadIdx.x;
    if (q >= (long long)J.w * J.h) return;
    const long long p = J.px_off + q;
    const int k = plane[p];
    int sm = 0, sp = 0;
    if (k > 0 && k < D - 1) { sm = sums[p * D + k - 1]; sp = sums[p * D + k + 1]; }
    float z, sc;
    sgm_pixel(J.wf, J.step, D, k, best[p], second[p], sm, sp, cost[p * D + k], uniqueness, z, sc);
    depth[p] = z;
    score[p] = sc;
}

struct SgmParams { int D, p1, p2, n_paths, invalid_cost; };

template <int NP>
void launch_path(hipStream_t s, dim3 grid, const SgmJob* jobs, const unsigned char* cost, uint16_t* sums, const SgmParams& prm, int dx, int dy,
                 int first) {
    const bool full = prm.D == 64 * NP;
    auto kernel = first ? (full ? k_sgm_path<NP, true, true> : k_sgm_path<NP, true, false>) : (full ? k_sgm_path<NP, false, true> : k_sgm_path<NP, false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(SGM_LANES), 0, s, jobs, cost, sums, prm.D, prm.p1, prm.p2, prm.invalid_cost, dx, dy);
}
template <int NP>
void launch_select(hipStream_t s, dim3 grid, const uint16_t* sums, long long n_px, int D, int16_t* plane, uint16_t* best, uint16_t* second) {
    hipLaunchKernelGGL(k_sgm_select<NP>, grid, dim3(SGM_LANES), 0, s, sums, n_px, D, plane, best, second);
}

// the aggregation and the selection of the jobs `tab` (host; d_tab the same on the device) whose volumes lie in d_cost
int sgm_run(hipStream_t s, PhaseTimer& tm, const std::vector<SgmJob>& tab, const SgmJob* d_tab, long long n_px, const unsigned char* d_cost,
            uint16_t* d_sums, const SgmParams& prm, int16_t* d_plane, uint16_t* d_best, uint16_t* d_second) {
    const int np = (prm.D + 63) / 64;
    for (int i = 0; i < prm.n_paths; ++i) {
        int dx, dy, lines = 0;
        sgm_direction(i, dx, dy);
        for (const SgmJob& J : tab) lines = std::max(lines, sgm_lines(dx, dy, J.w, J.h));
        const dim3 grid((unsigned)((lines + SGM_WAVES - 1) / SGM_WAVES), (unsigned)tab.size());
        tm.begin(SGM_T_PATH0 + i);
        switch (np) {
        case 1: launch_path<1>(s, grid, d_tab, d_cost, d_sums, prm, dx, dy, i == 0); break;
        case 2: launch_path<2>(s, grid, d_tab, d_cost, d_sums, prm, dx, dy, i == 0); break;
        case 3: launch_path<3>(s, grid, d_tab, d_cost, d_sums, prm, dx, dy, i == 0); break;
        default: launch_path<4>(s, grid, d_tab, d_cost, d_sums, prm, dx, dy, i == 0); break;
        }
        UNIT_TRY(hipGetLastError());
        tm.end();
    }
    tm.begin(SGM_T_SELECT);
    const dim3 grid((unsigned)std::min<long long>((n_px + SGM_WAVES - 1) / SGM_WAVES, 16384));
    switch (np) {
    case 1: launch_select<1>(s, grid, d_sums, n_px, prm.D, d_plane, d_best, d_second); break;
    case 2: launch_select<2>(s, grid, d_sums, n_px, prm.D, d_plane, d_best, d_second); break;
    case 3: launch_select<3>(s, grid, d_sums, n_px, prm.D, d_plane, d_best, d_second); break;
    default: launch_select<4>(s, grid, d_sums, n_px, prm.D, d_plane, d_best, d_second); break;
    }
    UNIT_TRY(hipGetLastError());
    tm.end();
    return 0;
}

void collect(PhaseTimer& tm, double* t) {
    for (int i = 0; i < SGM_T_COUNT; ++i) t[i] = 0.0;
    tm.collect(t);
    for (int i = 0; i < 8; ++i) t[SGM_T_AGGREGATE] += t[SGM_T_PATH0 + i];
}

// sfmba_depth_cost_volume: the group's volume goes to the host as it is
struct VolumeSink : DepthCostSink {
    unsigned char* cost;
    explicit VolumeSink(unsigned char* c) : cost(c) {}
    int group(hipStream_t s, DeviceArena&, const DepthCostGroup& g) override {
        UNIT_TRY(hipMemcpyAsync(cost + (size_t)g.first_px * (size_t)g.D, g.d_cost, (size_t)g.n_px * (size_t)g.D, hipMemcpyDeviceToHost, s));
        return 0;
    }
};

// sfmba_depth_sweep_sgm: the volume and the sums stay on the device, the three maps of the group are filled
struct SgmSink : DepthCostSink {
    SgmParams prm;
    int uniqueness;
    PhaseTimer& tm;
    std::vector<SgmJob> tab;           // lives until the next group: the sweep drains the stream between groups
    SgmSink(const SgmParams& p, int u, PhaseTimer& t) : prm(p), uniqueness(u), tm(t) {
        extra_bytes_per_entry = 2;
        maps = true;
    }
    int group(hipStream_t s, DeviceArena& scratch, const DepthCostGroup& g) override {
        tab.resize((size_t)g.n_jobs);
        long long max_px = 0;
        for (int j = 0; j < g.n_jobs; ++j) {
            tab[(size_t)j] = SgmJob{ g.jobs[j].px_off, g.jobs[j].w, g.jobs[j].h, g.jobs[j].wf, g.jobs[j].step };
            max_px = std::max(max_px, (long long)g.jobs[j].w * g.jobs[j].h);
        }
        SgmJob* d_tab;
        uint16_t *d_sums, *d_best, *d_second;
        UNIT_ALLOC(scratch, d_tab, SgmJob, tab.size());
        UNIT_ALLOC(scratch, d_sums, uint16_t, (size_t)g.n_px * (size_t)g.D);
        UNIT_ALLOC(scratch, d_best, uint16_t, (size_t)g.n_px);
        UNIT_ALLOC(scratch, d_second, uint16_t, (size_t)g.n_px);
        UNIT_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(SgmJob) * tab.size(), hipMemcpyHostToDevice, s));
        if (const int rc = sgm_run(s, tm, tab, d_tab, g.n_px, g.d_cost, d_sums, prm, g.d_plane, d_best, d_second)) return rc;
        tm.begin(SGM_T_FINISH);
        hipLaunchKernelGGL(k_sgm_finish, dim3((unsigned)((max_px + SGM_LANES - 1) / SGM_LANES), (unsigned)g.n_jobs), dim3(SGM_LANES), 0, s, d_tab,
                           g.d_cost, d_sums, g.d_plane, d_best, d_second, g.D, uniqueness, g.d_depth, g.d_score);
        UNIT_TRY(hipGetLastError());
        tm.end();
        return 0;
    }
};

}  // namespace

int depth_cost_volume(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
                      const int32_t* height, int channels, const float* K, const float* P, int n_jobs, const int32_t* job_ref,
                      const int64_t* job_src_ptr, const int32_t* job_src, const float* z_near, const float* z_far, int n_planes, int radius,
                      int min_std, int min_sources, unsigned char* cost, double* sweep_timing) {
    VolumeSink sink(cost);
    return depth_sweep(s, device, n_images, img_ptr, pixels, width, height, channels, K, P, n_jobs, job_ref, job_src_ptr, job_src, z_near, z_far,
                       n_planes, radius, min_std, 0.0f, min_sources, nullptr, nullptr, nullptr, sweep_timing, &sink);
}

int depth_sweep_sgm(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
                    const int32_t* height, int channels, const float* K, const float* P, int n_jobs, const int32_t* job_ref,
                    const int64_t* job_src_ptr, const int32_t* job_src, const float* z_near, const float* z_far, int n_planes, int radius,
                    int min_std, int min_sources, int p1, int p2, int n_paths, int invalid_cost, int uniqueness, float* depth, float* score,
                    int16_t* plane, double* sweep_timing, double* sgm_timing) {
    PhaseTimer tm{ s, sgm_timing != nullptr, {}, {} };
    SgmSink sink(SgmParams{ n_planes, p1, p2, n_paths, invalid_cost }, uniqueness, tm);
    const int rc = depth_sweep(s, device, n_images, img_ptr, pixels, width, height, channels, K, P, n_jobs, job_ref, job_src_ptr, job_src, z_near,
                               z_far, n_planes, radius, min_std, 0.0f, min_sources, depth, score, plane, sweep_timing, &sink);
    if (rc == 0 && sgm_timing) collect(tm, sgm_timing);
    return rc;
}

int sgm_aggregate(hipStream_t s, int device, int n_jobs, const unsigned char* const* cost, const int32_t* width, const int32_t* height, int D,
                  int p1, int p2, int n_paths, int invalid_cost, int16_t* const* plane, uint16_t* const* best, uint16_t* const* second,
                  uint16_t* const* sums, double* sgm_timing) {
    PhaseTimer tm{ s, sgm_timing != nullptr, {}, {} };
    const SgmParams prm{ D, p1, p2, n_paths, invalid_cost };
    for (int j = 0; j < n_jobs; ++j) {                        // a job at a time: the volumes come from the host anyway
        const long long n_px = (long long)width[j] * height[j];
        const size_t entries = (size_t)n_px * (size_t)D;
        const std::vector<SgmJob> tab(1, SgmJob{ 0, width[j], height[j], 0.0, 0.0 });
        DeviceArena scratch(device);
        SgmJob* d_tab;
        unsigned char* d_cost;
        uint16_t *d_sums, *d_best, *d_second;
        int16_t* d_plane;
        UNIT_ALLOC(scratch, d_tab, SgmJob, 1);
        UNIT_ALLOC(scratch, d_cost, unsigned char, entries);
        UNIT_ALLOC(scratch, d_sums, uint16_t, entries);
        UNIT_ALLOC(scratch, d_best, uint16_t, (size_t)n_px);
        UNIT_ALLOC(scratch, d_second, uint16_t, (size_t)n_px);
        UNIT_ALLOC(scratch, d_plane, int16_t, (size_t)n_px);
        UNIT_DRAIN_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(SgmJob), hipMemcpyHostToDevice, s));
        UNIT_DRAIN_TRY(hipMemcpyAsync(d_cost, cost[j], entries, hipMemcpyHostToDevice, s));
        if (const int rc = sgm_run(s, tm, tab, d_tab, n_px, d_cost, d_sums, prm, d_plane, d_best, d_second)) { (void)hipStreamSynchronize(s); return rc; }
        UNIT_DRAIN_TRY(hipMemcpyAsync(plane[j], d_plane, sizeof(int16_t) * (size_t)n_px, hipMemcpyDeviceToHost, s));
        UNIT_DRAIN_TRY(hipMemcpyAsync(best[j], d_best, sizeof(uint16_t) * (size_t)n_px, hipMemcpyDeviceToHost, s));
        UNIT_DRAIN_TRY(hipMemcpyAsync(second[j], d_second, sizeof(uint16_t) * (size_t)n_px, hipMemcpyDeviceToHost, s));
        if (sums && sums[j]) UNIT_DRAIN_TRY(hipMemcpyAsync(sums[j], d_sums, sizeof(uint16_t) * entries, hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipStreamSynchronize(s));                    // the job's arena goes back to the cache below
    }
    if (sgm_timing) collect(tm, sgm_timing);
    return 0;
}

}  // namespace sfmba
