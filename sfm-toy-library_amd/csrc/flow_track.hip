// flow_track.hip -- matching by optical flow on the MI355X (gfx950): pyramidal Lucas-Kanade tracking of the points of a list of
// image pairs, and the snap of the end points to the key points of the destination image.
//
// The contract is the project's own (include/sfmba.h, sfmba_flow_track / sfmba_flow_match; arithmetic in flow_math.h): integer-exact
// sampling at 1/16 px, exact window sums, a handful of fp64 operations per step -- so the result is BIT-EXACT with a CPU restatement.
//
//   gray          k_flow_gray: BGR images are reduced once per group with the ORB unit's rule into level 0 of their pyramid; gray input
//                 is uploaded into it.
//   pyramid       k_flow_pyr: ONE launch per level over all distinct images of the group (grid.y = image), a lane per pixel.
//   track         k_flow_track: ONE WAVE PER POINT, all levels in one launch.  Per level the wave writes the (2r+3)^2 template to
//                 LDS as int16, then the two gradient planes ((2r+1)^2 int16 each; 2822 bytes in all at r = 10), each lane owning
//                 ceil(n / 64) window pixels.  A workgroup is one wave, so a workgroup's LDS is one point's and the barriers cost
//                 nothing; with under 3 KB per wave LDS never limits the 32 waves a CU holds.  The destination samples are read
//                 straight from global memory (they move with every iteration).  The five window sums are INTEGERS: a lane sums
//                 its own pixels in int32 (at most 7 terms below 2^25), the wave reduces in int64, and any reduction order gives
//                 the same bits.  The fp64 step is formed from those integers, so every lane forms the same value; the first
//                 lane's is broadcast, which makes the loop conditions scalar.
//   match         k_flow_near: one lane per query, a workgroup (one wave) of 64 queries of one pair, so that a pair of a few thousand
//                 queries still spreads over the chip; the pair's train key points go through LDS in stages of 256.  An fp32 screen
//                 on |dx| and |dy| passes only the few key points near the query on to the exact fp64 test.  A lane keeps the two smallest (s, j) in range and the count in range, decides its candidate
//                 and enters an integer atomicMin per train key point (order-free: the lowest query wins whatever the arrival
//                 order).  k_flow_winner flags the candidates that won; a hipCUB inclusive sum and a scatter compact them.
#include "flow_track.h"
#include "flow_math.h"
#include "device_arena.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;
constexpr int WAVE = 64;

// An image of a group: its pyramid levels as byte offsets into the group's pyramid region.
struct FlowImage {
    long long off[FLOW_MAX_LEVELS];
    long long raw_off;
    int w[FLOW_MAX_LEVELS], h[FLOW_MAX_LEVELS];
};
// A pair of a group: image slots and its first point in the group (ascending; the search below reads it).
struct FlowPair { long long pt0; int src, dst; };

__global__ __launch_bounds__(LANES) void k_flow_gray(const FlowImage* __restrict__ tab, const unsigned char* __restrict__ raw,
                                                     unsigned char* __restrict__ pyr) {
    const FlowImage& T = tab[blockIdx.y];
    const long long px = (long long)T.w[0] * T.h[0];
    for (long long i = (long long)blockIdx.x * LANES + threadIdx.x; i < px; i += (long long)gridDim.x * LANES) {
        const unsigned char* p = raw + T.raw_off + 3 * i;
        pyr[T.off[0] + i] = (unsigned char)orb_gray_bgr(p[0], p[1], p[2]);
    }
}

// level `l` (>= 1) of every image from its level l - 1
__global__ __launch_bounds__(LANES) void k_flow_pyr(const FlowImage* __restrict__ tab, unsigned char* __restrict__ pyr, int l) {
    const FlowImage& T = tab[blockIdx.y];
    const int w = T.w[l], h = T.h[l];
    const unsigned char* src = pyr + T.off[l - 1];
    for (long long i = (long long)blockIdx.x * LANES + threadIdx.x; i < (long long)w * h; i += (long long)gridDim.x * LANES)
        pyr[T.off[l] + i] = (unsigned char)flow_pyr_down(src, T.w[l - 1], T.h[l - 1], (int)(i % w), (int)(i / w));
}

// integers: the order of the additions does not change the bits
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(WAVE) void k_flow_track(const FlowImage* __restrict__ tab, const FlowPair* __restrict__ pairs, int n_pairs,
                                                     const unsigned char* __restrict__ pyr, const float* __restrict__ pts, int L, int r,
                                                     int max_iters, float min_eig, float* __restrict__ next, unsigned char* __restrict__ status,
                                                     float* __restrict__ err, long long* __restrict__ dbg_G, int* __restrict__ dbg_state) {
    __shared__ short s_T[FLOW_MAX_SIDE * FLOW_MAX_SIDE];
    __shared__ short s_gx[FLOW_MAX_WINDOW], s_gy[FLOW_MAX_WINDOW];
    const long long pt = blockIdx.x;
    const int lane = threadIdx.x;
    int lo = 0, hi = n_pairs - 1;                                    // the last pair whose first point is <= pt
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pairs[mid].pt0 <= pt) lo = mid; else hi = mid - 1;
    }
    const FlowImage& S = tab[pairs[lo].src];
    const FlowImage& D = tab[pairs[lo].dst];
    const float x = pts[2 * pt], y = pts[2 * pt + 1];
    const int side = 2 * r + 3, win = 2 * r + 1, n = win * win, cells = side * side;

    // a lane's cells c = lane, lane + 64, ..: their (column, row) advance by (64 % width, 64 / width) with a carry, so no loop divides
    const int ti0 = lane % side, tj0 = lane / side, tdi = WAVE % side, tdj = WAVE / side;
    const int wi0 = lane % win, wj0 = lane / win, wdi = WAVE % win, wdj = WAVE / win;
#define FLOW_NEXT_CELL(i, j, di, dj, width) do { i += di; j += dj; if (i >= width) { i -= width; ++j; } } while (0)

    int dqx = 0, dqy = 0, cx = 0, cy = 0, ok = 0;
    for (int l = L - 1; l >= 0; --l) {
        if (l < L - 1) { dqx *= 2; dqy *= 2; }
        cx = flow_centre(x, l);
        cy = flow_centre(y, l);
        const unsigned char* simg = pyr + S.off[l];
        const unsigned char* dimg = pyr + D.off[l];
        const int sw = S.w[l], sh = S.h[l], dw = D.w[l], dh = D.h[l];
        for (int c = lane, i = ti0, j = tj0; c < cells; c += WAVE) {
            s_T[c] = (short)flow_sample(simg, sw, sh, cx + 16 * (i - r - 1), cy + 16 * (j - r - 1));
            FLOW_NEXT_CELL(i, j, tdi, tdj, side);
        }
        __syncthreads();
        int pxx = 0, pyy = 0, pxy = 0;
        for (int c = lane, i = wi0, j = wj0; c < n; c += WAVE) {
            int t, gx, gy;
            flow_gradient_at(s_T, side, i, j, t, gx, gy);
            s_gx[c] = (short)gx; s_gy[c] = (short)gy;             // read back by this lane only
            pxx += gx * gx; pyy += gy * gy; pxy += gx * gy;
            FLOW_NEXT_CELL(i, j, wdi, wdj, win);
        }
        const long long Gxx = wave_sum(pxx), Gyy = wave_sum(pyy), Gxy = wave_sum(pxy);
        double det;
        ok = __builtin_amdgcn_readfirstlane(flow_trackable(Gxx, Gyy, Gxy, min_eig, n, det) ? 1 : 0);
        int it = 0;
        while (ok && it < max_iters) {
            int pbx = 0, pby = 0;
            for (int c = lane, i = wi0, j = wj0; c < n; c += WAVE) {
                const int J = flow_sample(dimg, dw, dh, cx + dqx + 16 * (i - r), cy + dqy + 16 * (j - r));
                const int d = (int)s_T[(j + 1) * side + i + 1] - J;
                pbx += d * (int)s_gx[c]; pby += d * (int)s_gy[c];
                FLOW_NEXT_CELL(i, j, wdi, wdj, win);
            }
            const long long bx = wave_sum(pbx), by = wave_sum(pby);
            int sx, sy;
            flow_step(Gxx, Gyy, Gxy, det, bx, by, r, sx, sy);
            sx = __builtin_amdgcn_readfirstlane(sx);
            sy = __builtin_amdgcn_readfirstlane(sy);
            ++it;
            if (sx == 0 && sy == 0) break;
            dqx += sx; dqy += sy;
        }
        if (lane == 0) {
            const long long o = pt * L + l;
            if (dbg_G) { dbg_G[3 * o] = Gxx; dbg_G[3 * o + 1] = Gyy; dbg_G[3 * o + 2] = Gxy; }
            if (dbg_state) { dbg_state[4 * o] = ok; dbg_state[4 * o + 1] = it; dbg_state[4 * o + 2] = dqx; dbg_state[4 * o + 3] = dqy; }
        }
        if (l > 0) __syncthreads();                                // the next level overwrites the template
    }
    long long sad = 0;
    if (ok) {                                                      // level 0's template is still in LDS
        int part = 0;
        const unsigned char* dimg = pyr + D.off[0];
        for (int c = lane, i = wi0, j = wj0; c < n; c += WAVE) {
            const int d = (int)s_T[(j + 1) * side + i + 1] - flow_sample(dimg, D.w[0], D.h[0], cx + dqx + 16 * (i - r), cy + dqy + 16 * (j - r));
            part += d < 0 ? -d : d;
            FLOW_NEXT_CELL(i, j, wdi, wdj, win);
        }
        sad = wave_sum(part);
    }
    if (lane == 0) {
        next[2 * pt] = flow_next(x, dqx);
        next[2 * pt + 1] = flow_next(y, dqy);
        status[pt] = ok && flow_inside(cx, dqx, D.w[0]) && flow_inside(cy, dqy, D.h[0]) ? 1 : 0;
        err[pt] = ok ? flow_err(sad, n) : 0.0f;
    }
#undef FLOW_NEXT_CELL
}

// ---- match ---------------------------------------------------------------------------------------------------------------------
struct MatchPair { long long q0, kp0, win0; int nq, nt; };       // first query, first train key point, first winner slot
struct MatchTile { int pair, q0; };

__global__ __launch_bounds__(FLOW_MATCH_QUERIES) void k_flow_near(const MatchPair* __restrict__ pairs, const MatchTile* __restrict__ tiles,
                                                               const float* __restrict__ next, const unsigned char* __restrict__ status,
                                                               const float* __restrict__ err, const float* __restrict__ kp, float max_err,
                                                               float radius, double ratio, int* __restrict__ cand, float* __restrict__ dist,
                                                               unsigned* __restrict__ winner) {
    __shared__ float4 s_kx4[FLOW_MATCH_TILE / 4], s_ky4[FLOW_MATCH_TILE / 4];
    float* const s_kx = reinterpret_cast<float*>(s_kx4);
    float* const s_ky = reinterpret_cast<float*>(s_ky4);
    const MatchTile tile = tiles[blockIdx.x];
    const MatchPair P = pairs[tile.pair];
    const int ql = tile.q0 + (int)threadIdx.x;                     // the query within its pair
    const bool live = ql < P.nq;
    const long long q = P.q0 + ql;
    bool eligible = false;
    float qx = 0.0f, qy = 0.0f;
    if (live) {
        eligible = status[q] != 0 && err[q] < max_err;
        qx = next[2 * q]; qy = next[2 * q + 1];
    }
    // The fp32 screen drops only key points that are provably out of range: s <= r^2 needs |dx| <= r (1 + 2^-52), the fp32 difference
    // is off by at most 2^-24 relative, and reach >= r (1 + 9e-7).  A NaN or an overflowed reach passes on to the exact test.
    const float reach = radius * 1.000001f;
    double s1 = 0.0, s2 = 0.0;
    int j1 = -1, in_range = 0;
    for (int t0 = 0; t0 < P.nt; t0 += FLOW_MATCH_TILE) {
        const int m = min(FLOW_MATCH_TILE, P.nt - t0), m8 = (m + 7) & ~7;
        __syncthreads();                                           // the stage before has been read
        for (int k = threadIdx.x; k < m8; k += FLOW_MATCH_QUERIES) {   // the stage is read eight at a time: its tail is +inf, never in range
            s_kx[k] = k < m ? kp[2 * (P.kp0 + t0 + k)] : INFINITY;
            s_ky[k] = k < m ? kp[2 * (P.kp0 + t0 + k) + 1] : INFINITY;
        }
        __syncthreads();
        if (!eligible) continue;
        for (int k = 0; k < m8; k += 8) {                          // eight broadcast values per LDS round trip
            const float4 xa = s_kx4[k >> 2], xb = s_kx4[(k >> 2) + 1], ya = s_ky4[k >> 2], yb = s_ky4[(k >> 2) + 1];
            const float kx[8] = { xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w }, ky[8] = { ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w };
            unsigned near = 0u;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (!(fabsf(qx - kx[u]) > reach || fabsf(qy - ky[u]) > reach)) near |= 1u << u;
            if (!near) continue;
#pragma unroll
            for (int u = 0; u < 8; ++u) {                          // ascending j with strict <: a tie on s stays with the lower j
                if (!(near >> u & 1u)) continue;
                const double s = flow_dist2(qx, qy, kx[u], ky[u]);
                if (!flow_in_range(s, radius)) continue;
                if (in_range == 0 || s < s1) { s2 = s1; s1 = s; j1 = t0 + k + u; }
                else if (in_range == 1 || s < s2) s2 = s;
                ++in_range;
            }
        }
    }
    if (!live) return;
    const bool is_cand = eligible && flow_candidate(in_range, s1, s2, ratio);
    cand[q] = is_cand ? j1 : -1;
    dist[q] = is_cand ? (float)sqrt(s1) : 0.0f;
    if (is_cand) atomicMin(&winner[P.win0 + j1], (unsigned)ql);
}

__global__ __launch_bounds__(FLOW_MATCH_QUERIES) void k_flow_winner(const MatchPair* __restrict__ pairs, const MatchTile* __restrict__ tiles,
                                                       const int* __restrict__ cand, const unsigned* __restrict__ winner, int* __restrict__ flag,
                                                       int* __restrict__ qidx) {
    const MatchTile tile = tiles[blockIdx.x];
    const MatchPair P = pairs[tile.pair];
    const int ql = tile.q0 + (int)threadIdx.x;
    if (ql >= P.nq) return;
    const long long q = P.q0 + ql;
    const int j = cand[q];
    flag[q] = j >= 0 && winner[P.win0 + j] == (unsigned)ql ? 1 : 0;
    qidx[q] = ql;
}

// pos[0..n_rows] = exclusive positions (pos[0] = 0, pos[n_rows] = total); pair_ptr[p] = pos[prow[p]].
__global__ __launch_bounds__(LANES) void k_flow_pair_ptr(int n, const long long* __restrict__ prow, const int* __restrict__ pos,
                                                         long long* __restrict__ pair_ptr) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p <= n) pair_ptr[p] = pos[prow[p]];
}

__global__ __launch_bounds__(LANES) void k_flow_scatter(long long n_rows, const int* __restrict__ flag, const int* __restrict__ pos,
                                                        const int* __restrict__ cand, const float* __restrict__ dist, const int* __restrict__ qidx,
                                                        long long cap, int* __restrict__ out_q, int* __restrict__ out_t, float* __restrict__ out_d) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows || !flag[r]) return;
    const long long o = pos[r];
    if (o >= cap) return;
    out_q[o] = qidx[r];
    out_t[o] = cand[r];
    out_d[o] = dist[r];
}

long long align64(long long n) { return (n + 63) & ~63ll; }
unsigned grid_for(long long n) { return (unsigned)((n + LANES - 1) / LANES); }

// sizes and (relative) offsets of the L levels of a w x h image; returns the bytes they take
long long pyramid_layout(int w, int h, int L, FlowImage& T) {
    long long at = 0;
    for (int l = 0; l < FLOW_MAX_LEVELS; ++l) {
        T.w[l] = w; T.h[l] = h;
        T.off[l] = at;
        if (l < L) at += align64((long long)w * h);
        w = flow_half(w); h = flow_half(h);
    }
    return at;
}

}  // namespace

int flow_track(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
               const int32_t* height, int channels, int n_pairs, const int32_t* pair_src, const int32_t* pair_dst, const int64_t* pt_ptr,
               const float* pts, int n_levels, int radius, int max_iters, float min_eig, float* next, unsigned char* status, float* err,
               int64_t* dbg_G, int32_t* dbg_state, unsigned char* dbg_pyramid, double* timing) {
    if (timing) for (int i = 0; i < FLOW_T_COUNT; ++i) timing[i] = 0.0;
    if (n_pairs == 0) return 0;
    const int L = n_levels;
    // where image i's levels start in dbg_pyramid: levels 0 .. L-1 back to back, images in order
    std::vector<long long> dbg_off((size_t)n_images + 1, 0);
    for (int i = 0; i < n_images; ++i) {
        long long b = 0;
        for (int l = 0, w = width[i], h = height[i]; l < L; ++l, w = flow_half(w), h = flow_half(h)) b += (long long)w * h;
        dbg_off[(size_t)i + 1] = dbg_off[(size_t)i] + b;
    }
    const long long per_point = 8 + 8 + 1 + 4 + (dbg_G ? 24ll * L : 0) + (dbg_state ? 16ll * L : 0);

    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    const long long group_bytes = group_bytes_limit(FLOW_SCRATCH_BYTES);
    const int group_pairs = group_items_limit(INT_MAX);      // the unit itself caps the images of a group, not its pairs: the hook counts pairs
    int n_groups = 0;
    std::vector<int> slot((size_t)n_images, -1);              // an image's row in the group's table, -1: not in it
    for (int p0 = 0; p0 < n_pairs;) {
        // the group: consecutive pairs while the images they name and their points fit
        std::fill(slot.begin(), slot.end(), -1);
        std::vector<int> used;
        std::vector<FlowImage> tab;
        long long raw_bytes = 0, pyr_bytes = 0, n_pts = 0;
        int p1 = p0;
        while (p1 < n_pairs && p1 - p0 < group_pairs) {
            long long add_raw = 0, add_pyr = 0;
            int fresh[2], n_fresh = 0;
            for (int i : { pair_src[p1], pair_dst[p1] }) {
                if (slot[(size_t)i] >= 0 || (n_fresh == 1 && fresh[0] == i)) continue;
                fresh[n_fresh++] = i;
                FlowImage T;
                add_pyr += pyramid_layout(width[i], height[i], L, T);
                if (channels == 3) add_raw += align64((long long)width[i] * height[i] * 3);
            }
            const long long np = pt_ptr[p1 + 1] - pt_ptr[p1];
            const long long bytes = raw_bytes + pyr_bytes + add_raw + add_pyr + per_point * (n_pts + np);
            if (p1 > p0 && (bytes > group_bytes || n_pts + np >= (long long)INT_MAX || used.size() + n_fresh > 65535)) break;   // grid.y
            for (int q = 0; q < n_fresh; ++q) {
                const int i = fresh[q];
                FlowImage T;
                const long long b = pyramid_layout(width[i], height[i], L, T);
                for (int l = 0; l < FLOW_MAX_LEVELS; ++l) T.off[l] += pyr_bytes;
                T.raw_off = raw_bytes;
                pyr_bytes += b;
                if (channels == 3) raw_bytes += align64((long long)width[i] * height[i] * 3);
                slot[(size_t)i] = (int)tab.size();
                tab.push_back(T);
                used.push_back(i);
            }
            n_pts += np;
            ++p1;
        }
        const int np_ = p1 - p0;
        ++n_groups;
        std::vector<FlowPair> ptab((size_t)np_);
        for (int p = 0; p < np_; ++p)
            ptab[(size_t)p] = FlowPair{ pt_ptr[p0 + p] - pt_ptr[p0], slot[(size_t)pair_src[p0 + p]], slot[(size_t)pair_dst[p0 + p]] };

        DeviceArena scratch(device);
        FlowImage* d_tab;
        FlowPair* d_ptab;
        unsigned char *d_raw = nullptr, *d_pyr, *d_status;
        float *d_pts, *d_next, *d_err;
        long long* d_G = nullptr;
        int* d_state = nullptr;
        UNIT_ALLOC(scratch, d_tab, FlowImage, tab.size());
        UNIT_ALLOC(scratch, d_ptab, FlowPair, ptab.size());
        UNIT_ALLOC(scratch, d_pyr, unsigned char, (size_t)pyr_bytes);
        if (channels == 3) UNIT_ALLOC(scratch, d_raw, unsigned char, (size_t)raw_bytes);
        UNIT_ALLOC(scratch, d_pts, float, (size_t)n_pts * 2);
        UNIT_ALLOC(scratch, d_next, float, (size_t)n_pts * 2);
        UNIT_ALLOC(scratch, d_status, unsigned char, (size_t)n_pts);
        UNIT_ALLOC(scratch, d_err, float, (size_t)n_pts);
        if (dbg_G) UNIT_ALLOC(scratch, d_G, long long, (size_t)n_pts * L * 3);
        if (dbg_state) UNIT_ALLOC(scratch, d_state, int, (size_t)n_pts * L * 4);

        tm.begin(FLOW_T_UPLOAD);
        UNIT_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(FlowImage) * tab.size(), hipMemcpyHostToDevice, s));
        UNIT_TRY(hipMemcpyAsync(d_ptab, ptab.data(), sizeof(FlowPair) * ptab.size(), hipMemcpyHostToDevice, s));
        long long max_px = 0;
        for (size_t q = 0; q < used.size(); ++q) {
            const int i = used[q];
            const long long px = (long long)width[i] * height[i];
            max_px = std::max(max_px, px);
            if (channels == 3) UNIT_TRY(hipMemcpyAsync(d_raw + tab[q].raw_off, pixels + img_ptr[i], (size_t)px * 3, hipMemcpyHostToDevice, s));
            else               UNIT_TRY(hipMemcpyAsync(d_pyr + tab[q].off[0], pixels + img_ptr[i], (size_t)px, hipMemcpyHostToDevice, s));
        }
        const size_t at = (size_t)pt_ptr[p0];
        if (n_pts > 0) UNIT_TRY(hipMemcpyAsync(d_pts, pts + 2 * at, sizeof(float) * 2 * (size_t)n_pts, hipMemcpyHostToDevice, s));
        tm.end();
        if (channels == 3) {
            tm.begin(FLOW_T_GRAY);
            hipLaunchKernelGGL(k_flow_gray, dim3(std::min(grid_for(max_px), 4096u), (unsigned)used.size()), dim3(LANES), 0, s, d_tab, d_raw, d_pyr);
            UNIT_TRY(hipGetLastError());
            tm.end();
        }
        tm.begin(FLOW_T_PYRAMID);
        for (int l = 1; l < L; ++l) {
            long long lvl_px = 1;
            for (const FlowImage& T : tab) lvl_px = std::max(lvl_px, (long long)T.w[l] * T.h[l]);
            hipLaunchKernelGGL(k_flow_pyr, dim3(std::min(grid_for(lvl_px), 4096u), (unsigned)used.size()), dim3(LANES), 0, s, d_tab, d_pyr, l);
            UNIT_TRY(hipGetLastError());
        }
        tm.end();
        if (n_pts > 0) {
            tm.begin(FLOW_T_TRACK);
            hipLaunchKernelGGL(k_flow_track, dim3((unsigned)n_pts), dim3(WAVE), 0, s, d_tab, d_ptab, np_, d_pyr, d_pts, L, radius, max_iters, min_eig,
                               d_next, d_status, d_err, d_G, d_state);
            UNIT_TRY(hipGetLastError());
            tm.end();
            tm.begin(FLOW_T_DOWNLOAD);
            UNIT_TRY(hipMemcpyAsync(next + 2 * at, d_next, sizeof(float) * 2 * (size_t)n_pts, hipMemcpyDeviceToHost, s));
            UNIT_TRY(hipMemcpyAsync(status + at, d_status, (size_t)n_pts, hipMemcpyDeviceToHost, s));
            UNIT_TRY(hipMemcpyAsync(err + at, d_err, sizeof(float) * (size_t)n_pts, hipMemcpyDeviceToHost, s));
            static_assert(sizeof(long long) == sizeof(int64_t), "dbg_G leaves as it is");
            if (dbg_G) UNIT_TRY(hipMemcpyAsync(dbg_G + at * L * 3, d_G, sizeof(int64_t) * (size_t)n_pts * L * 3, hipMemcpyDeviceToHost, s));
            if (dbg_state) UNIT_TRY(hipMemcpyAsync(dbg_state + at * L * 4, d_state, sizeof(int32_t) * (size_t)n_pts * L * 4, hipMemcpyDeviceToHost, s));
            tm.end();
        }
        if (dbg_pyramid) {
            tm.begin(FLOW_T_DOWNLOAD);
            for (size_t q = 0; q < used.size(); ++q) {
                long long o = dbg_off[(size_t)used[q]];
                for (int l = 0; l < L; ++l) {
                    const size_t b = (size_t)tab[q].w[l] * tab[q].h[l];
                    UNIT_TRY(hipMemcpyAsync(dbg_pyramid + o, d_pyr + tab[q].off[l], b, hipMemcpyDeviceToHost, s));
                    o += (long long)b;
                }
            }
            tm.end();
        }
        UNIT_TRY(hipStreamSynchronize(s));                     // the group's arena goes back to the cache below
        p0 = p1;
    }
    if (timing) {
        tm.collect(timing);
        timing[FLOW_T_GROUPS] = n_groups;
    }
    return 0;
}

int flow_match(hipStream_t s, int device, int n_images, const int64_t* kp_ptr, const float* kp_xy, int n_pairs, const int32_t* pair_dst,
               const int64_t* pt_ptr, const float* next, const unsigned char* status, const float* err, float max_err, float radius,
               double ratio, int64_t* pair_ptr, int32_t* query_idx, int32_t* train_idx, float* distance, int64_t cap, int64_t* total,
               double* timing) {
    for (int p = 0; p <= n_pairs; ++p) pair_ptr[p] = 0;
    *total = 0;
    if (timing) for (int i = 0; i < FLOWM_T_COUNT; ++i) timing[i] = 0.0;
    const long long n_rows = n_pairs > 0 ? pt_ptr[n_pairs] : 0;
    if (n_rows == 0) return 0;

    std::vector<MatchPair> pairs((size_t)n_pairs);
    std::vector<MatchTile> tiles;
    std::vector<long long> prow((size_t)n_pairs + 1, 0);
    long long n_win = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int d = pair_dst[p];
        MatchPair& P = pairs[(size_t)p];
        P.q0 = pt_ptr[p]; P.nq = (int)(pt_ptr[p + 1] - pt_ptr[p]);
        P.kp0 = kp_ptr[d]; P.nt = (int)(kp_ptr[d + 1] - kp_ptr[d]);
        P.win0 = n_win;
        n_win += P.nt;
        prow[(size_t)p] = pt_ptr[p];
        for (int q0 = 0; q0 < P.nq; q0 += FLOW_MATCH_QUERIES) tiles.push_back(MatchTile{ p, q0 });
    }
    prow[(size_t)n_pairs] = n_rows;
    const long long n_kp = kp_ptr[n_images];

    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    DeviceArena scratch(device);
    MatchPair* d_pairs;
    MatchTile* d_tiles;
    float *d_next, *d_err, *d_kp, *d_dist;
    unsigned char* d_status;
    int *d_cand, *d_flag, *d_qidx, *d_pos;
    unsigned* d_winner;
    long long *d_prow, *d_pptr;
    UNIT_ALLOC(scratch, d_pairs, MatchPair, pairs.size());
    UNIT_ALLOC(scratch, d_tiles, MatchTile, tiles.size());
    UNIT_ALLOC(scratch, d_next, float, (size_t)n_rows * 2);
    UNIT_ALLOC(scratch, d_err, float, (size_t)n_rows);
    UNIT_ALLOC(scratch, d_status, unsigned char, (size_t)n_rows);
    UNIT_ALLOC(scratch, d_kp, float, (size_t)std::max(n_kp, 1ll) * 2);
    UNIT_ALLOC(scratch, d_cand, int, (size_t)n_rows);
    UNIT_ALLOC(scratch, d_dist, float, (size_t)n_rows);
    UNIT_ALLOC(scratch, d_winner, unsigned, (size_t)std::max(n_win, 1ll));
    UNIT_ALLOC(scratch, d_flag, int, (size_t)n_rows);
    UNIT_ALLOC(scratch, d_qidx, int, (size_t)n_rows);
    UNIT_ALLOC(scratch, d_pos, int, (size_t)n_rows + 1);           // handed out zeroed: pos[0] stays 0
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

    tm.begin(FLOWM_T_UPLOAD);
    UNIT_TRY(hipMemcpyAsync(d_pairs, pairs.data(), sizeof(MatchPair) * pairs.size(), hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_tiles, tiles.data(), sizeof(MatchTile) * tiles.size(), hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_prow, prow.data(), sizeof(long long) * prow.size(), hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_next, next, sizeof(float) * 2 * (size_t)n_rows, hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_err, err, sizeof(float) * (size_t)n_rows, hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_status, status, (size_t)n_rows, hipMemcpyHostToDevice, s));
    if (n_kp > 0) UNIT_TRY(hipMemcpyAsync(d_kp, kp_xy, sizeof(float) * 2 * (size_t)n_kp, hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemsetAsync(d_winner, 0xff, sizeof(unsigned) * (size_t)std::max(n_win, 1ll), s));     // above every query index
    tm.end();

    tm.begin(FLOWM_T_NEAR);
    const unsigned n_tiles = (unsigned)tiles.size();
    hipLaunchKernelGGL(k_flow_near, dim3(n_tiles), dim3(FLOW_MATCH_QUERIES), 0, s, d_pairs, d_tiles, d_next, d_status, d_err, d_kp, max_err, radius, ratio,
                       d_cand, d_dist, d_winner);
    hipLaunchKernelGGL(k_flow_winner, dim3(n_tiles), dim3(FLOW_MATCH_QUERIES), 0, s, d_pairs, d_tiles, d_cand, d_winner, d_flag, d_qidx);
    UNIT_TRY(hipGetLastError());
    tm.end();
    tm.begin(FLOWM_T_COMPACT);
    UNIT_TRY(hipcub::DeviceScan::InclusiveSum(d_tmp, tmp_bytes, d_flag, d_pos + 1, (int)n_rows, s));
    hipLaunchKernelGGL(k_flow_pair_ptr, dim3(grid_for(n_pairs + 1)), dim3(LANES), 0, s, n_pairs, d_prow, d_pos, d_pptr);
    hipLaunchKernelGGL(k_flow_scatter, dim3(grid_for(n_rows)), dim3(LANES), 0, s, n_rows, d_flag, d_pos, d_cand, d_dist, d_qidx, ocap, d_oq, d_ot, d_od);
    UNIT_TRY(hipGetLastError());
    static_assert(sizeof(long long) == sizeof(int64_t), "pair_ptr leaves as it is");
    UNIT_TRY(hipMemcpyAsync(pair_ptr, d_pptr, sizeof(int64_t) * prow.size(), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    tm.end();
    const long long tot = pair_ptr[n_pairs];
    *total = tot;
    if (tot > cap) return UNIT_ERR_CAPACITY;
    if (tot > 0) {
        tm.begin(FLOWM_T_DOWNLOAD);
        UNIT_TRY(hipMemcpyAsync(query_idx, d_oq, sizeof(int) * (size_t)tot, hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipMemcpyAsync(train_idx, d_ot, sizeof(int) * (size_t)tot, hipMemcpyDeviceToHost, s));
        if (distance) UNIT_TRY(hipMemcpyAsync(distance, d_od, sizeof(float) * (size_t)tot, hipMemcpyDeviceToHost, s));
        tm.end();
        UNIT_TRY(hipStreamSynchronize(s));
    }
    if (timing) tm.collect(timing);
    return 0;
}

}  // namespace sfmba
