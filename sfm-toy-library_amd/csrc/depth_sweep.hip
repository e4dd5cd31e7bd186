// depth_sweep.hip -- dense depth maps and a dense cloud on the MI355X (gfx950): multi-view plane-sweep stereo over a list of jobs
// and the consistency filter that turns the maps into coloured points.
//
// The contract is the project's own (include/sfmba.h, sfmba_depth_sweep / sfmba_depth_fuse; arithmetic in depth_math.h): fp64
// coordinates with every operation rounded on its own, exact integers from the sample to the window sums, a handful of fp64
// operations for the score -- so the result is BIT-EXACT with a CPU restatement.
//
//   gray          k_depth_gray: BGR images are reduced once per group with the ORB unit's rule; gray input is used as uploaded.
//   sweep         k_depth_sweep<R>: one workgroup of 256 lanes per 16 x 16 tile of a job's reference image (grid.y = job of the
//                 group).  The reference tile with its halo of R goes to LDS once and every lane forms SI / SII of its own window.
//                 Then the planes: the lanes write the (16 + 2R)^2 warped samples of every source to LDS as uint16 (0xffff = not
//                 valid), ONE barrier (the sample buffers alternate between two planes), and every lane sums its own window per
//                 source: SJ, SJJ, SIJ in int32, the score in fp64.  A lane keeps the best cost, the cost before it, the previous
//                 cost and a "take the next one" flag, so the refinement needs no cost volume: nothing but the three maps goes to
//                 HBM.  k_depth_sweep<R, true> is the same code with the other ending: it keeps no winner and stores the quantised
//                 cost of every (pixel, plane) instead -- the volume that depth_sgm.hip aggregates.
//   fuse          k_fuse_flag: one lane per pixel with a depth, the agreement count over the check images -> a 0 / 1 flag;
//                 a hipCUB exclusive sum over the flags in (image, row, column) order gives every kept pixel its output row;
//                 k_fuse_emit writes the rows.  The compaction is stable by construction.
#include "depth_sweep.h"
#include "depth_math.h"
#include "sgm_math.h"
#include "device_arena.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;

// One job of a group.  Offsets are bytes into the group's gray region (one byte per pixel) and pixels into its output maps.
struct DepthJob {
    double A[DEPTH_MAX_SOURCES][9], b[DEPTH_MAX_SOURCES][3];
    double wf, step;
    long long ref_off, src_off[DEPTH_MAX_SOURCES], out_off;
    int w, h, sw[DEPTH_MAX_SOURCES], sh[DEPTH_MAX_SOURCES];
    int n_src;
};

struct GrayJob { long long raw_off, gray_off, pixels; };

__global__ __launch_bounds__(LANES) void k_depth_gray(const GrayJob* __restrict__ tab, const unsigned char* __restrict__ raw,
                                                      unsigned char* __restrict__ gray) {
    const GrayJob g = tab[blockIdx.y];
    for (long long i = (long long)blockIdx.x * LANES + threadIdx.x; i < g.pixels; i += (long long)gridDim.x * LANES) {
        const unsigned char* p = raw + g.raw_off + 3 * i;
        gray[g.gray_off + i] = (unsigned char)orb_gray_bgr(p[0], p[1], p[2]);
    }
}

template <int R, bool COST>
__global__ __launch_bounds__(LANES) void k_depth_sweep(const DepthJob* __restrict__ jobs, const unsigned char* __restrict__ gray, int D, int min_std,
                                                       double min_score, int min_sources, float* __restrict__ depth, float* __restrict__ score,
                                                       int16_t* __restrict__ plane, unsigned char* __restrict__ cost) {
    constexpr int SIDE = DEPTH_TILE + 2 * R, CELLS = SIDE * SIDE, N = (2 * R + 1) * (2 * R + 1);
    __shared__ unsigned short s_ref[CELLS];
    __shared__ unsigned short s_smp[2][DEPTH_MAX_SOURCES][CELLS];

    const DepthJob& J = jobs[blockIdx.y];
    const int w = J.w, h = J.h, n_src = J.n_src;
    const int tiles_x = (w + DEPTH_TILE - 1) / DEPTH_TILE, tiles_y = (h + DEPTH_TILE - 1) / DEPTH_TILE;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;         // uniform over the workgroup, before any barrier
    const int x0 = ((int)blockIdx.x % tiles_x) * DEPTH_TILE, y0 = ((int)blockIdx.x / tiles_x) * DEPTH_TILE;
    const int tid = threadIdx.x, lx = tid & (DEPTH_TILE - 1), ly = tid >> 4;
    const unsigned char* ref = gray + J.ref_off;

    for (int c = tid; c < CELLS; c += LANES) {
        const int u = x0 - R + c % SIDE, v = y0 - R + c / SIDE;
        s_ref[c] = (u >= 0 && u < w && v >= 0 && v < h) ? ref[(size_t)v * (size_t)w + u] : 0;
    }
    __syncthreads();

    const int x = x0 + lx, y = y0 + ly;
    bool part = x - R >= 0 && x + R < w && y - R >= 0 && y + R < h;
    int SI = 0, SII = 0;
    long long varI = 0;
    if (part) {
#pragma unroll
        for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
            for (int dx = 0; dx <= 2 * R; ++dx) {
                const int I = s_ref[(ly + dy) * SIDE + lx + dx];
                SI += I;
                SII += I * I;
            }
        varI = depth_var(N, SI, SII);
        part = depth_textured(N, varI, min_std);
    }

    bool have = false, take_next = false, pred_ok = false, succ_ok = false, prev_ok = false;
    double best = 0.0, pred = 0.0, succ = 0.0, prev = 0.0;
    int best_k = -1;
    // the cost store: a lane owns the D bytes of its pixel and writes them four planes at a time where the run is aligned (D % 4 == 0)
    const bool inside = x < w && y < h;
    unsigned char* run = nullptr;
    unsigned pack = 0u;
    if constexpr (COST)
        if (inside) run = cost + ((size_t)J.out_off + (size_t)y * (size_t)w + x) * (size_t)D;
    for (int k = 0; k < D; ++k) {
        const double wk = depth_plane_w(J.wf, J.step, k);
        const int buf = k & 1;
        for (int s = 0; s < n_src; ++s) {
            const unsigned char* img = gray + J.src_off[s];
            for (int c = tid; c < CELLS; c += LANES) {
                const int u = x0 - R + c % SIDE, v = y0 - R + c / SIDE;
                int val = DEPTH_NO_SAMPLE;                     // a cell outside the reference image is read by no window that takes part
                if (u >= 0 && u < w && v >= 0 && v < h) val = depth_warped_sample(J.A[s], J.b[s], u, v, wk, img, J.sw[s], J.sh[s]);
                s_smp[buf][s][c] = (unsigned short)val;
            }
        }
        __syncthreads();                                       // the other buffer is written next: one barrier per plane
        int q = SGM_SENTINEL;
        if (part) {
            double acc = 0.0;
            int count = 0;
            for (int s = 0; s < n_src; ++s) {
                unsigned SJ = 0u, SJJ = 0u, SIJ = 0u, worst = 0u;   // unsigned: SJJ wraps where worst says the sums are not used
#pragma unroll
                for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
                    for (int dx = 0; dx <= 2 * R; ++dx) {
                        const int c = (ly + dy) * SIDE + lx + dx;
                        const unsigned I = s_ref[c], Jv = s_smp[buf][s][c];
                        worst = Jv > worst ? Jv : worst;
                        SJ += Jv;
                        SJJ += Jv * Jv;
                        SIJ += I * Jv;
                    }
                if (worst == (unsigned)DEPTH_NO_SAMPLE) continue;
                const long long varJ = depth_var(N, SJ, SJJ);
                if (varJ <= 0) continue;
                const double sc = depth_score(depth_num(N, SI, SJ, SIJ), varI, varJ);
                acc = count ? acc + sc : sc;
                ++count;
            }
            const bool valid = count >= min_sources;          // min_sources >= 1
            const double C = valid ? acc / (double)count : 0.0;
            if constexpr (COST) {
                if (valid) q = sgm_quantise(C);
            } else {
                if (take_next) { succ = C; succ_ok = valid; take_next = false; }
                if (valid && (!have || C > best)) {
                    have = true; best = C; best_k = k;
                    pred = prev; pred_ok = prev_ok;
                    take_next = true; succ_ok = false;
                }
                prev = C; prev_ok = valid;
            }
        }
        if constexpr (COST) if (inside) {
            if ((D & 3) == 0) {
                pack |= (unsigned)q << (8 * (k & 3));
                if ((k & 3) == 3) { *reinterpret_cast<unsigned*>(run + k - 3) = pack; pack = 0u; }
            } else {
                run[k] = (unsigned char)q;
            }
        }
    }
    if constexpr (COST) return;

    if (x < w && y < h) {
        float z = 0.0f, sc = 0.0f;
        if (have) {
            sc = (float)best;
            if (best >= min_score) {
                double delta = 0.0;
                if (best_k > 0 && best_k < D - 1 && pred_ok && succ_ok) delta = depth_refine(pred, best, succ);
                z = depth_value(J.wf, J.step, best_k, delta);
            }
        }
        const size_t o = (size_t)J.out_off + (size_t)y * (size_t)w + x;
        depth[o] = z;
        score[o] = sc;
        plane[o] = (int16_t)best_k;
    }
}

// ---- fuse ----------------------------------------------------------------------------------------------------------------------
struct FuseImage {
    double P[12];
    long long raw_off;       // first byte of its pixels
    long long depth_off;     // first float of its depth map, -1: none
    long long dom_off;       // first flag of its pixels (images with a map only)
    int w, h;
    int n_chk, chk[DEPTH_MAX_CHECKS];
};
struct FuseParams { double k4[4]; double rel_tol; int min_consistent, channels; };

__device__ __forceinline__ bool fuse_keep(const FuseImage* __restrict__ tab, const FuseImage& T, const FuseParams& prm, const float* __restrict__ maps,
                                          int u, int v, double* X) {
    const double z = (double)maps[T.depth_off + (long long)v * T.w + u];
    if (!(z > 0.0)) return false;
    depth_unproject(prm.k4, T.P, u, v, z, X);
    int agree = 0;
    for (int c = 0; c < T.n_chk; ++c) {
        const FuseImage& S = tab[T.chk[c]];
        int px, py;
        double qz;
        if (S.depth_off < 0 || !depth_reproject(prm.k4, S.P, X, S.w, S.h, px, py, qz)) continue;
        if (depth_agrees((double)maps[S.depth_off + (long long)py * S.w + px], qz, prm.rel_tol)) ++agree;
    }
    return agree >= prm.min_consistent;
}

__global__ __launch_bounds__(LANES) void k_fuse_flag(const FuseImage* __restrict__ tab, FuseParams prm, const float* __restrict__ maps,
                                                     int* __restrict__ flag) {
    const FuseImage& T = tab[blockIdx.y];
    const long long q = (long long)blockIdx.x * LANES + threadIdx.x;
    if (T.depth_off < 0 || q >= (long long)T.w * T.h) return;
    double X[3];
    flag[T.dom_off + q] = fuse_keep(tab, T, prm, maps, (int)(q % T.w), (int)(q / T.w), X) ? 1 : 0;
}

__global__ __launch_bounds__(LANES) void k_fuse_emit(const FuseImage* __restrict__ tab, FuseParams prm, const float* __restrict__ maps,
                                                     const unsigned char* __restrict__ raw, const int* __restrict__ flag, const int* __restrict__ pos,
                                                     float* __restrict__ xyz, unsigned char* __restrict__ bgr, int* __restrict__ src_image,
                                                     int* __restrict__ src_pixel) {
    const FuseImage& T = tab[blockIdx.y];
    const long long q = (long long)blockIdx.x * LANES + threadIdx.x;
    if (T.depth_off < 0 || q >= (long long)T.w * T.h || !flag[T.dom_off + q]) return;
    const int u = (int)(q % T.w), v = (int)(q / T.w);
    double X[3];
    depth_unproject(prm.k4, T.P, u, v, (double)maps[T.depth_off + q], X);
    const size_t o = (size_t)pos[T.dom_off + q];
    for (int j = 0; j < 3; ++j) xyz[3 * o + j] = (float)X[j];
    const unsigned char* p = raw + T.raw_off + (size_t)q * prm.channels;
    for (int j = 0; j < 3; ++j) bgr[3 * o + j] = prm.channels == 3 ? p[j] : p[0];
    src_image[o] = (int)blockIdx.y;
    src_pixel[o] = (int)q;
}

__global__ void k_fuse_ptr(const FuseImage* __restrict__ tab, int n_images, long long n_dom, const int* __restrict__ pos, long long* __restrict__ pt_ptr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_images) return;
    // an image without a map has the dom_off of the next image with one
    pt_ptr[i] = pos[i < n_images ? tab[i].dom_off : n_dom];
}

long long align64(long long n) { return (n + 63) & ~63ll; }

template <int R>
void launch_sweep(hipStream_t s, unsigned tiles, unsigned n_jobs, const DepthJob* jobs, const unsigned char* gray, int D, int min_std, double min_score,
                  int min_sources, float* depth, float* score, int16_t* plane, unsigned char* cost) {
    if (cost)
        hipLaunchKernelGGL((k_depth_sweep<R, true>), dim3(tiles, n_jobs), dim3(LANES), 0, s, jobs, gray, D, min_std, min_score, min_sources, depth, score,
                           plane, cost);
    else
        hipLaunchKernelGGL((k_depth_sweep<R, false>), dim3(tiles, n_jobs), dim3(LANES), 0, s, jobs, gray, D, min_std, min_score, min_sources, depth, score,
                           plane, cost);
}

}  // namespace

int depth_sweep(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
                const int32_t* height, int channels, const float* K, const float* P, int n_jobs, const int32_t* job_ref,
                const int64_t* job_src_ptr, const int32_t* job_src, const float* z_near, const float* z_far, int n_planes, int radius,
                int min_std, float min_score, int min_sources, float* depth, float* score, int16_t* plane, double* timing, DepthCostSink* sink) {
    if (timing) for (int i = 0; i < DEPTH_T_COUNT; ++i) timing[i] = 0.0;
    if (n_jobs == 0) return 0;
    const double k4[4] = { (double)K[0], (double)K[4], (double)K[2], (double)K[5] };
    std::vector<long long> out_off((size_t)n_jobs + 1, 0);
    for (int j = 0; j < n_jobs; ++j) out_off[(size_t)j + 1] = out_off[(size_t)j] + (long long)width[job_ref[j]] * height[job_ref[j]];

    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    const long long group_bytes = group_bytes_limit(DEPTH_SCRATCH_BYTES);
    const int group_jobs = group_items_limit(DEPTH_MAX_GROUP_JOBS);
    int n_groups = 0;
    std::vector<long long> slot((size_t)n_images, -1);       // first gray byte of an image in the group, -1: not in it
    for (int j0 = 0; j0 < n_jobs;) {
        // the group: consecutive jobs while the images they name and their maps fit
        std::fill(slot.begin(), slot.end(), -1);
        std::vector<int> used;
        long long raw_bytes = 0, gray_bytes = 0, out_px = 0, max_tiles = 0;
        int j1 = j0;
        while (j1 < n_jobs && j1 - j0 < group_jobs) {
            long long add_raw = 0, add_gray = 0;
            std::vector<int> fresh;
            auto want = [&](int i) {
                if (slot[(size_t)i] >= 0 || std::find(fresh.begin(), fresh.end(), i) != fresh.end()) return;
                fresh.push_back(i);
                add_gray += align64((long long)width[i] * height[i]);
                if (channels == 3) add_raw += align64((long long)width[i] * height[i] * 3);
            };
            want(job_ref[j1]);
            for (int64_t e = job_src_ptr[j1]; e < job_src_ptr[j1 + 1]; ++e) want(job_src[e]);
            const long long px = out_off[(size_t)j1 + 1] - out_off[(size_t)j1];
            long long bytes = raw_bytes + gray_bytes + add_raw + add_gray + 10 * (out_px + px);
            if (sink) bytes += (long long)(1 + sink->extra_bytes_per_entry) * n_planes * (out_px + px);   // the volume and what the sink adds
            if (j1 > j0 && bytes > group_bytes) break;
            for (int i : fresh) {
                slot[(size_t)i] = gray_bytes;
                gray_bytes += align64((long long)width[i] * height[i]);
                used.push_back(i);
            }
            raw_bytes += add_raw;
            out_px += px;
            const long long tiles = (long long)((width[job_ref[j1]] + DEPTH_TILE - 1) / DEPTH_TILE) * ((height[job_ref[j1]] + DEPTH_TILE - 1) / DEPTH_TILE);
            max_tiles = std::max(max_tiles, tiles);
            ++j1;
        }
        const int nj = j1 - j0;
        ++n_groups;

        std::vector<DepthJob> tab((size_t)nj);
        for (int j = 0; j < nj; ++j) {
            DepthJob& T = tab[(size_t)j];
            std::memset(&T, 0, sizeof(T));
            const int r = job_ref[j0 + j];
            T.w = width[r]; T.h = height[r];
            T.ref_off = slot[(size_t)r];
            T.out_off = out_off[(size_t)(j0 + j)] - out_off[(size_t)j0];
            depth_planes((double)z_near[j0 + j], (double)z_far[j0 + j], n_planes, T.wf, T.step);
            double pr[12], ps[12];
            for (int q = 0; q < 12; ++q) pr[q] = (double)P[(size_t)r * 12 + q];
            T.n_src = (int)(job_src_ptr[j0 + j + 1] - job_src_ptr[j0 + j]);
            for (int e = 0; e < T.n_src; ++e) {
                const int si = job_src[job_src_ptr[j0 + j] + e];
                for (int q = 0; q < 12; ++q) ps[q] = (double)P[(size_t)si * 12 + q];
                depth_warp(k4, pr, ps, T.A[e], T.b[e]);
                T.src_off[e] = slot[(size_t)si];
                T.sw[e] = width[si]; T.sh[e] = height[si];
            }
        }

        DeviceArena scratch(device);
        DepthJob* d_tab;
        GrayJob* d_gtab;
        unsigned char *d_raw = nullptr, *d_gray;
        float *d_depth, *d_score;
        int16_t* d_plane;
        UNIT_ALLOC(scratch, d_tab, DepthJob, (size_t)nj);
        UNIT_ALLOC(scratch, d_gtab, GrayJob, used.size());
        UNIT_ALLOC(scratch, d_gray, unsigned char, (size_t)gray_bytes);
        if (channels == 3) UNIT_ALLOC(scratch, d_raw, unsigned char, (size_t)raw_bytes);
        UNIT_ALLOC(scratch, d_depth, float, (size_t)out_px);
        UNIT_ALLOC(scratch, d_score, float, (size_t)out_px);
        UNIT_ALLOC(scratch, d_plane, int16_t, (size_t)out_px);
        unsigned char* d_cost = nullptr;
        if (sink) UNIT_ALLOC(scratch, d_cost, unsigned char, (size_t)out_px * (size_t)n_planes);

        tm.begin(DEPTH_T_UPLOAD);
        UNIT_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(DepthJob) * tab.size(), hipMemcpyHostToDevice, s));
        std::vector<GrayJob> gtab(used.size());
        long long raw_at = 0, max_px = 0;
        for (size_t q = 0; q < used.size(); ++q) {
            const int i = used[q];
            const long long px = (long long)width[i] * height[i];
            gtab[q] = GrayJob{ raw_at, slot[(size_t)i], px };
            max_px = std::max(max_px, px);
            if (channels == 3) {
                UNIT_TRY(hipMemcpyAsync(d_raw + raw_at, pixels + img_ptr[i], (size_t)px * 3, hipMemcpyHostToDevice, s));
                raw_at += align64(px * 3);
            } else {
                UNIT_TRY(hipMemcpyAsync(d_gray + slot[(size_t)i], pixels + img_ptr[i], (size_t)px, hipMemcpyHostToDevice, s));
            }
        }
        if (channels == 3) UNIT_TRY(hipMemcpyAsync(d_gtab, gtab.data(), sizeof(GrayJob) * gtab.size(), hipMemcpyHostToDevice, s));
        tm.end();
        if (channels == 3) {
            tm.begin(DEPTH_T_GRAY);
            const unsigned gx = (unsigned)std::min<long long>((max_px + LANES - 1) / LANES, 4096);
            hipLaunchKernelGGL(k_depth_gray, dim3(gx, (unsigned)used.size()), dim3(LANES), 0, s, d_gtab, d_raw, d_gray);
            UNIT_TRY(hipGetLastError());
            tm.end();
        }
        tm.begin(DEPTH_T_SWEEP);
        const unsigned tiles = (unsigned)max_tiles;
        const double ms = (double)min_score;
        switch (radius) {
        case 1: launch_sweep<1>(s, tiles, (unsigned)nj, d_tab, d_gray, n_planes, min_std, ms, min_sources, d_depth, d_score, d_plane, d_cost); break;
        case 2: launch_sweep<2>(s, tiles, (unsigned)nj, d_tab, d_gray, n_planes, min_std, ms, min_sources, d_depth, d_score, d_plane, d_cost); break;
        case 3: launch_sweep<3>(s, tiles, (unsigned)nj, d_tab, d_gray, n_planes, min_std, ms, min_sources, d_depth, d_score, d_plane, d_cost); break;
        default: launch_sweep<4>(s, tiles, (unsigned)nj, d_tab, d_gray, n_planes, min_std, ms, min_sources, d_depth, d_score, d_plane, d_cost); break;
        }
        UNIT_TRY(hipGetLastError());
        tm.end();
        const size_t at = (size_t)out_off[(size_t)j0];
        if (sink) {
            std::vector<DepthCostJob> cj((size_t)nj);
            for (int j = 0; j < nj; ++j) cj[(size_t)j] = DepthCostJob{ tab[(size_t)j].w, tab[(size_t)j].h, tab[(size_t)j].out_off, tab[(size_t)j].wf, tab[(size_t)j].step };
            const DepthCostGroup g{ j0, nj, n_planes, cj.data(), (long long)at, out_px, d_cost, d_depth, d_score, d_plane };
            if (const int rc = sink->group(s, scratch, g)) { (void)hipStreamSynchronize(s); return rc; }
        }
        tm.begin(DEPTH_T_DOWNLOAD);
        if (!sink || sink->maps) {
            UNIT_TRY(hipMemcpyAsync(depth + at, d_depth, sizeof(float) * (size_t)out_px, hipMemcpyDeviceToHost, s));
            UNIT_TRY(hipMemcpyAsync(score + at, d_score, sizeof(float) * (size_t)out_px, hipMemcpyDeviceToHost, s));
            if (plane) UNIT_TRY(hipMemcpyAsync(plane + at, d_plane, sizeof(int16_t) * (size_t)out_px, hipMemcpyDeviceToHost, s));
        }
        tm.end();
        UNIT_TRY(hipStreamSynchronize(s));                    // the group's arena goes back to the cache below
        j0 = j1;
    }
    if (timing) {
        tm.collect(timing);
        timing[DEPTH_T_GROUPS] = n_groups;
    }
    return 0;
}

int depth_fuse(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
               const int32_t* height, int channels, const float* K, const float* P, const float* const* depth, const int64_t* chk_ptr,
               const int32_t* chk, float rel_tol, int min_consistent, int64_t* pt_ptr, float* xyz, unsigned char* bgr, int32_t* src_image,
               int32_t* src_pixel, int64_t cap, int64_t* total, double* timing) {
    for (int i = 0; i <= n_images; ++i) pt_ptr[i] = 0;
    *total = 0;
    if (timing) for (int i = 0; i < FUSE_T_COUNT; ++i) timing[i] = 0.0;

    std::vector<FuseImage> tab((size_t)std::max(n_images, 1));
    long long raw_bytes = 0, n_dom = 0, max_px = 0;
    for (int i = 0; i < n_images; ++i) {
        FuseImage& T = tab[(size_t)i];
        std::memset(&T, 0, sizeof(T));
        for (int q = 0; q < 12; ++q) T.P[q] = (double)P[(size_t)i * 12 + q];
        T.w = width[i]; T.h = height[i];
        const long long px = (long long)T.w * T.h;
        T.dom_off = n_dom;
        T.depth_off = depth[i] ? n_dom : -1;                 // the maps lie on the device as the flags do
        T.raw_off = -1;
        if (depth[i]) {
            T.raw_off = raw_bytes;
            raw_bytes += align64(px * channels);
            n_dom += px;
            max_px = std::max(max_px, px);
        }
        T.n_chk = (int)(chk_ptr[i + 1] - chk_ptr[i]);
        for (int c = 0; c < T.n_chk; ++c) T.chk[c] = chk[chk_ptr[i] + c];
    }
    if (n_dom == 0) return 0;

    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    DeviceArena scratch(device);
    FuseImage* d_tab;
    float* d_maps;
    unsigned char* d_raw;
    int *d_flag, *d_pos;
    long long* d_ptr;
    UNIT_ALLOC(scratch, d_tab, FuseImage, tab.size());
    UNIT_ALLOC(scratch, d_maps, float, (size_t)n_dom);
    UNIT_ALLOC(scratch, d_raw, unsigned char, (size_t)raw_bytes);
    UNIT_ALLOC(scratch, d_flag, int, (size_t)n_dom + 1);     // handed out zeroed: the last flag stays 0
    UNIT_ALLOC(scratch, d_pos, int, (size_t)n_dom + 1);
    UNIT_ALLOC(scratch, d_ptr, long long, (size_t)n_images + 1);
    size_t tmp_bytes = 0;
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_flag, d_pos, (int)(n_dom + 1), s));
    void* d_tmp = scratch.alloc(std::max(tmp_bytes, (size_t)1));
    if (!d_tmp) return (int)hipErrorOutOfMemory;

    tm.begin(FUSE_T_UPLOAD);
    UNIT_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(FuseImage) * tab.size(), hipMemcpyHostToDevice, s));
    for (int i = 0; i < n_images; ++i) {
        if (!depth[i]) continue;
        const size_t px = (size_t)width[i] * height[i];
        UNIT_TRY(hipMemcpyAsync(d_maps + tab[(size_t)i].depth_off, depth[i], sizeof(float) * px, hipMemcpyHostToDevice, s));
        UNIT_TRY(hipMemcpyAsync(d_raw + tab[(size_t)i].raw_off, pixels + img_ptr[i], px * channels, hipMemcpyHostToDevice, s));
    }
    tm.end();

    FuseParams prm;
    prm.k4[0] = (double)K[0]; prm.k4[1] = (double)K[4]; prm.k4[2] = (double)K[2]; prm.k4[3] = (double)K[5];
    prm.rel_tol = (double)rel_tol;
    prm.min_consistent = min_consistent;
    prm.channels = channels;
    const dim3 grid((unsigned)((max_px + LANES - 1) / LANES), (unsigned)n_images);
    tm.begin(FUSE_T_FLAG);
    hipLaunchKernelGGL(k_fuse_flag, grid, dim3(LANES), 0, s, d_tab, prm, d_maps, d_flag);
    UNIT_TRY(hipGetLastError());
    tm.end();
    tm.begin(FUSE_T_SCAN);
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_flag, d_pos, (int)(n_dom + 1), s));
    hipLaunchKernelGGL(k_fuse_ptr, dim3((unsigned)((n_images + 1 + LANES - 1) / LANES)), dim3(LANES), 0, s, d_tab, n_images, n_dom, d_pos, d_ptr);
    UNIT_TRY(hipGetLastError());
    static_assert(sizeof(long long) == sizeof(int64_t), "pt_ptr leaves as it is");
    UNIT_TRY(hipMemcpyAsync(pt_ptr, d_ptr, sizeof(int64_t) * ((size_t)n_images + 1), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    tm.end();
    const long long tot = pt_ptr[n_images];
    *total = tot;
    if (tot > cap) return UNIT_ERR_CAPACITY;
    if (tot > 0) {
        float* d_xyz;
        unsigned char* d_bgr;
        int *d_img, *d_pix;
        UNIT_ALLOC(scratch, d_xyz, float, (size_t)tot * 3);
        UNIT_ALLOC(scratch, d_bgr, unsigned char, (size_t)tot * 3);
        UNIT_ALLOC(scratch, d_img, int, (size_t)tot);
        UNIT_ALLOC(scratch, d_pix, int, (size_t)tot);
        tm.begin(FUSE_T_EMIT);
        hipLaunchKernelGGL(k_fuse_emit, grid, dim3(LANES), 0, s, d_tab, prm, d_maps, d_raw, d_flag, d_pos, d_xyz, d_bgr, d_img, d_pix);
        UNIT_TRY(hipGetLastError());
        tm.end();
        tm.begin(FUSE_T_DOWNLOAD);
        UNIT_TRY(hipMemcpyAsync(xyz, d_xyz, sizeof(float) * (size_t)tot * 3, hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipMemcpyAsync(bgr, d_bgr, (size_t)tot * 3, hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipMemcpyAsync(src_image, d_img, sizeof(int) * (size_t)tot, hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipMemcpyAsync(src_pixel, d_pix, sizeof(int) * (size_t)tot, hipMemcpyDeviceToHost, s));
        tm.end();
        UNIT_TRY(hipStreamSynchronize(s));
    }
    if (timing) tm.collect(timing);
    return 0;
}

}  // namespace sfmba
