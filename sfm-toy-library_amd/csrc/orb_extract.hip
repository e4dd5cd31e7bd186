// orb_extract.hip -- SfM2DFeatureUtilities::extractFeatures for a whole list of images on the MI355X (gfx950).
//
// Reference: SfM::extractFeatures (SfMToyLib/SfM.cpp:141-154) calls ORB::create(5000)->detectAndCompute per image, serially
// (SfM2DFeatureUtilities.cpp:46-51).  The contract here is the project's own, integer-exact one (include/sfmba.h,
// sfmba_orb_extract; arithmetic in orb_math.h), so the result is BIT-EXACT with a CPU restatement.
//
// Images are taken in consecutive groups bounded by ORB_SCRATCH_BYTES; a group is worked level by level, every launch covering
// all images of the group (grid.y = image):
//
//   gray / resample   four consecutive pixels of the (row-tight) level per lane, one packed 32-bit store; level l from level
//                     l - 1 (two ping-pong buffers).  A one-channel input is copied straight into level 0.
//   score             k_orb_score: a 64 x 16 tile plus a 3-pixel halo staged as bytes in LDS; the brighter / darker ring masks
//                     are built without a branch and the exact S (sliding minima by doubling) is computed only where a 9-arc
//                     exists.  The map is bytes.
//   candidates        k_orb_flags (non-maximum suppression + border -> byte flags), a hipCUB exclusive scan over the level of
//                     the whole group, k_orb_compact (raster order inside an image, images in order: no atomics decide anything)
//                     and k_orb_response, one lane per candidate.
//   selection         two stable hipCUB radix sorts: by the response key (descending R; raster order survives among equal R),
//                     then by the image bits, which restores one contiguous segment per image.  The first quota entries of a
//                     segment are kept.
//   smooth            k_orb_smooth: the separable 7-tap filter through the same LDS tile, the horizontal pass kept as 16-bit.
//   describe          k_orb_describe: one wave per key point; the moments over the disc are reduced by shuffles, lane j gathers
//                     the eight smoothed pixels of bits 4j .. 4j + 3 and the row leaves as eight 32-bit words (32 bytes).
//
// The host reads one integer per level (the number of candidates, which sizes the sorts); the per-image counts stay on the
// device (k_orb_counts) until the end, when kp_ptr is formed and k_orb_pack closes the gaps of the staged rows.
#include "orb_extract.h"
#include "orb_math.h"
#include "device_arena.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;
constexpr int HALO = 3;
constexpr int TILE_LW = ORB_TILE_W + 2 * HALO;        // 70 staged columns
constexpr int TILE_LH = ORB_TILE_H + 2 * HALO;        // 22 staged rows
constexpr int TILE_STRIDE = 72;                       // LDS row stride in bytes
static_assert(LANES * 4 == ORB_TILE_W * ORB_TILE_H, "four pixels per lane");

// One image of the group at one level.  w == 0: the image has no key points at this level (the level does not exist or is
// 62 or less wide or high) and no kernel touches it.
struct OrbLevel {
    long long off, poff;        // first byte of this level / of the previous level in their regions (multiples of 4)
    int w, h, pw, ph;
    int quota, image;           // image: index in the call
};
// What k_orb_counts leaves for the later kernels of the level.
struct OrbSegment {
    long long stage;            // first staged row of (image, level)
    int begin, count, kept;     // the image's candidates are entries begin .. begin + count - 1 of the level's list
};

struct ToInt { __host__ __device__ int operator()(unsigned char v) const { return (int)v; } };

__device__ __forceinline__ unsigned pack4(const int (&v)[4]) {
    return (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
}
// four consecutive bytes from q on (q a multiple of 4, dst + q 4-byte aligned), the last ones dropped past n
__device__ __forceinline__ void store4(unsigned char* dst, long long q, long long n, const int (&v)[4]) {
    if (q + 3 < n) *reinterpret_cast<unsigned*>(dst + q) = pack4(v);
    else for (int j = 0; j < 4 && q + j < n; ++j) dst[q + j] = (unsigned char)v[j];
}

__global__ __launch_bounds__(LANES) void k_orb_gray(const OrbLevel* __restrict__ tab, const unsigned char* __restrict__ raw,
                                                    unsigned char* __restrict__ dst) {
    const OrbLevel T = tab[blockIdx.y];
    const long long n = (long long)T.w * T.h, q = ((long long)blockIdx.x * LANES + threadIdx.x) * 4;
    if (q >= n) return;
    const unsigned char* src = raw + 3 * T.off;
    int v[4] = { 0, 0, 0, 0 };
    for (int j = 0; j < 4 && q + j < n; ++j) v[j] = orb_gray_bgr(src[3 * (q + j)], src[3 * (q + j) + 1], src[3 * (q + j) + 2]);
    store4(dst + T.off, q, n, v);
}

__global__ __launch_bounds__(LANES) void k_orb_resample(const OrbLevel* __restrict__ tab, const unsigned char* __restrict__ prev,
                                                        unsigned char* __restrict__ dst) {
    const OrbLevel T = tab[blockIdx.y];
    const long long n = (long long)T.w * T.h, q = ((long long)blockIdx.x * LANES + threadIdx.x) * 4;
    if (q >= n) return;
    const unsigned char* src = prev + T.poff;
    int v[4] = { 0, 0, 0, 0 };
    for (int j = 0; j < 4 && q + j < n; ++j) {
        const int y = (int)((q + j) / T.w), x = (int)((q + j) - (long long)y * T.w);
        v[j] = orb_resample_pixel(src, T.pw, T.ph, T.w, T.h, x, y);
    }
    store4(dst + T.off, q, n, v);
}

// Stage the tile of blockIdx.x with its halo: sh[ly * TILE_STRIDE + lx] = I(x0 - 3 + lx, y0 - 3 + ly), 0 outside the level.
__device__ __forceinline__ bool stage_tile(const OrbLevel& T, const unsigned char* __restrict__ I, unsigned char* sh, int& x0, int& y0) {
    const int tx = (T.w + ORB_TILE_W - 1) / ORB_TILE_W, ty = (T.h + ORB_TILE_H - 1) / ORB_TILE_H;
    if ((long long)blockIdx.x >= (long long)tx * ty) return false;               // the whole block leaves: no barrier is skipped
    x0 = (int)(blockIdx.x % (unsigned)tx) * ORB_TILE_W;
    y0 = (int)(blockIdx.x / (unsigned)tx) * ORB_TILE_H;
    for (int i = threadIdx.x; i < TILE_LW * TILE_LH; i += LANES) {
        const int ly = i / TILE_LW, lx = i - ly * TILE_LW;
        const int gx = x0 - HALO + lx, gy = y0 - HALO + ly;
        sh[ly * TILE_STRIDE + lx] = (gx >= 0 && gx < T.w && gy >= 0 && gy < T.h) ? I[(size_t)gy * T.w + gx] : (unsigned char)0;
    }
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(LANES) void k_orb_score(const OrbLevel* __restrict__ tab, const unsigned char* __restrict__ pyr,
                                                     int threshold, unsigned char* __restrict__ score) {
    __shared__ unsigned char sh[TILE_LH * TILE_STRIDE];
    const OrbLevel T = tab[blockIdx.y];
    int x0, y0;
    if (T.w == 0 || !stage_tile(T, pyr + T.off, sh, x0, y0)) return;
    const int lx = threadIdx.x & (ORB_TILE_W - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ly = (threadIdx.x >> 6) + 4 * j;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= T.w || y >= T.h) continue;
        int S = 0;
        if (x >= HALO && x < T.w - HALO && y >= HALO && y < T.h - HALO) {
            const unsigned char* c0 = sh + (ly + HALO) * TILE_STRIDE + lx + HALO;
            int c[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) c[k] = c0[orb_circle_dy(k) * TILE_STRIDE + orb_circle_dx(k)];
            S = orb_fast_score(c0[0], c, threshold);
        }
        score[T.off + (size_t)y * T.w + x] = (unsigned char)S;
    }
}

__global__ __launch_bounds__(LANES) void k_orb_smooth(const OrbLevel* __restrict__ tab, const unsigned char* __restrict__ pyr,
                                                      unsigned char* __restrict__ smooth) {
    __shared__ unsigned char sh[TILE_LH * TILE_STRIDE];
    __shared__ unsigned short hs[TILE_LH * ORB_TILE_W];          // the horizontal pass: <= 255 * 256
    const OrbLevel T = tab[blockIdx.y];
    int x0, y0;
    if (T.w == 0 || !stage_tile(T, pyr + T.off, sh, x0, y0)) return;
    for (int i = threadIdx.x; i < TILE_LH * ORB_TILE_W; i += LANES) {
        const unsigned char* p = sh + (i / ORB_TILE_W) * TILE_STRIDE + (i % ORB_TILE_W);
        hs[i] = (unsigned short)orb_smooth_tap7(p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
    }
    __syncthreads();
    const int lx = threadIdx.x & (ORB_TILE_W - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ly = (threadIdx.x >> 6) + 4 * j;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= T.w || y >= T.h) continue;
        int B = 0;
        if (x >= HALO && x < T.w - HALO && y >= HALO && y < T.h - HALO) {
            const unsigned short* p = hs + ly * ORB_TILE_W + lx;
            B = orb_smooth_round(orb_smooth_tap7(p[0], p[ORB_TILE_W], p[2 * ORB_TILE_W], p[3 * ORB_TILE_W], p[4 * ORB_TILE_W],
                                                 p[5 * ORB_TILE_W], p[6 * ORB_TILE_W]));
        }
        smooth[T.off + (size_t)y * T.w + x] = (unsigned char)B;
    }
}

// flag = 1 for a candidate: S > 0, strictly above its 8 neighbours, at least ORB_EDGE from every edge
__global__ __launch_bounds__(LANES) void k_orb_flags(const OrbLevel* __restrict__ tab, const unsigned char* __restrict__ score,
                                                     unsigned char* __restrict__ flag) {
    const OrbLevel T = tab[blockIdx.y];
    const long long n = (long long)T.w * T.h, q = ((long long)blockIdx.x * LANES + threadIdx.x) * 4;
    if (q >= n) return;
    const unsigned char* S = score + T.off;
    int v[4] = { 0, 0, 0, 0 };
    for (int j = 0; j < 4 && q + j < n; ++j) {
        const int y = (int)((q + j) / T.w), x = (int)((q + j) - (long long)y * T.w);
        if (x < ORB_EDGE || x >= T.w - ORB_EDGE || y < ORB_EDGE || y >= T.h - ORB_EDGE) continue;
        const unsigned char* p = S + (size_t)y * T.w + x;
        const int s = p[0];
        if (s == 0) continue;
        const unsigned char* a = p - T.w;
        const unsigned char* b = p + T.w;
        const int m = max(max(max(a[-1], a[0]), max(a[1], p[-1])), max(max(p[1], b[-1]), max(b[0], b[1])));
        v[j] = s > m ? 1 : 0;
    }
    store4(flag + T.off, q, n, v);
}

// One lane per image of the group: its slice of the level's candidate list, what it keeps, where its rows are staged.
__global__ __launch_bounds__(LANES) void k_orb_counts(int n_img, int level, int n_levels, const OrbLevel* __restrict__ tab,
                                                      const int* __restrict__ pos, OrbSegment* __restrict__ seg,
                                                      long long* __restrict__ stage_cur, int* __restrict__ cand_count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img) return;
    const OrbLevel T = tab[i];
    OrbSegment g;
    g.begin = 0; g.count = 0; g.kept = 0; g.stage = stage_cur[T.image];
    if (T.w != 0) {
        g.begin = pos[T.off];
        g.count = pos[T.off + (long long)T.w * T.h] - g.begin;
        g.kept = min(g.count, T.quota);
        stage_cur[T.image] = g.stage + g.kept;
    }
    cand_count[(size_t)T.image * n_levels + level] = g.count;
    seg[i] = g;
}

// entry = (image of the group << 32) | (y << 16) | x, in raster order inside an image, images in order
__global__ __launch_bounds__(LANES) void k_orb_compact(const OrbLevel* __restrict__ tab, const unsigned char* __restrict__ flag,
                                                       const int* __restrict__ pos, int cap, uint64_t* __restrict__ entry) {
    const OrbLevel T = tab[blockIdx.y];
    const long long n = (long long)T.w * T.h, q = ((long long)blockIdx.x * LANES + threadIdx.x) * 4;
    if (q >= n) return;
    for (int j = 0; j < 4 && q + j < n; ++j) {
        if (!flag[T.off + q + j]) continue;
        const int o = pos[T.off + q + j];
        if (o < 0 || o >= cap) continue;
        const int y = (int)((q + j) / T.w), x = (int)((q + j) - (long long)y * T.w);
        entry[o] = ((uint64_t)blockIdx.y << 32) | ((uint64_t)(unsigned)y << 16) | (uint64_t)(unsigned)x;
    }
}

__global__ __launch_bounds__(LANES) void k_orb_response(int n, const OrbLevel* __restrict__ tab, const unsigned char* __restrict__ pyr,
                                                        const uint64_t* __restrict__ entry, uint64_t* __restrict__ key) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const uint64_t e = entry[c];
    const OrbLevel T = tab[(int)(e >> 32)];
    const int x = (int)(e & 0xffffu), y = (int)((e >> 16) & 0xffffu);
    const unsigned char* p = pyr + T.off + (size_t)(y - 4) * T.w + (x - 4);
    int w[81];
#pragma unroll
    for (int v = 0; v < 9; ++v)
#pragma unroll
        for (int u = 0; u < 9; ++u) w[v * 9 + u] = p[(size_t)v * T.w + u];
    key[c] = orb_response_key(orb_harris_response(w));
}

// One wave per key point: rank r of image blockIdx.y at this level.
__global__ __launch_bounds__(LANES) void k_orb_describe(const OrbLevel* __restrict__ tab, const OrbSegment* __restrict__ seg,
                                                        const unsigned char* __restrict__ pyr, const unsigned char* __restrict__ smooth,
                                                        const uint64_t* __restrict__ entry, const uint64_t* __restrict__ key,
                                                        const signed char* __restrict__ table, int level, double scale,
                                                        sfmba_orb_keypoint* __restrict__ kp, unsigned char* __restrict__ desc,
                                                        int* __restrict__ level_xy, int* __restrict__ bins, long long* __restrict__ harris) {
    const OrbSegment g = seg[blockIdx.y];
    const int r = blockIdx.x * (LANES / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= g.kept) return;                                   // wave-uniform; the kernel has no barrier
    const OrbLevel T = tab[blockIdx.y];
    const uint64_t e = entry[g.begin + r];
    const int x = (int)(e & 0xffffu), y = (int)((e >> 16) & 0xffffu);
    const unsigned char* I = pyr + T.off;
    int m10 = 0, m01 = 0;                                      // |m| <= 709 * 15 * 255
    for (int t = lane; t < (2 * ORB_DISC + 1) * (2 * ORB_DISC + 1); t += 64) {
        const int v = t / (2 * ORB_DISC + 1) - ORB_DISC, u = t % (2 * ORB_DISC + 1) - ORB_DISC;
        if (u * u + v * v > ORB_DISC * ORB_DISC) continue;
        const int p = I[(size_t)(y + v) * T.w + x + u];
        m10 += u * p; m01 += v * p;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { m10 += __shfl_xor(m10, d, 64); m01 += __shfl_xor(m01, d, 64); }
    const int bin = orb_bin(m10, m01);
    const int4 tw = *reinterpret_cast<const int4*>(table + (size_t)bin * ORB_PAIRS * 4 + (size_t)lane * 16);
    const int words[4] = { tw.x, tw.y, tw.z, tw.w };
    const unsigned char* B = smooth + T.off;
    unsigned nib = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int wv = words[b];
        const int ax = (signed char)(wv & 0xff), ay = (signed char)((wv >> 8) & 0xff);
        const int bx = (signed char)((wv >> 16) & 0xff), by = (signed char)((wv >> 24) & 0xff);
        const int b0 = B[(size_t)(y + ay) * T.w + x + ax], b1 = B[(size_t)(y + by) * T.w + x + bx];
        nib |= (unsigned)orb_desc_bit(b0, b1) << b;
    }
    unsigned word = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) word |= (unsigned)__shfl((int)nib, ((lane & 7) << 3) + k, 64) << (4 * k);
    const long long o = g.stage + r;
    if (lane < 8) reinterpret_cast<unsigned*>(desc + (size_t)o * ORB_DESC_BYTES)[lane] = word;
    if (lane == 0) {
        const long long R = orb_key_response(key[g.begin + r]);
        sfmba_orb_keypoint k;
        k.x = (float)((double)x * scale);
        k.y = (float)((double)y * scale);
        k.size = (float)(31.0 * scale);
        k.angle = (float)(12 * bin);
        k.response = (float)R;
        k.octave = level;
        kp[o] = k;
        level_xy[2 * o] = x; level_xy[2 * o + 1] = y;
        bins[o] = bin;
        harris[o] = R;
    }
}

// Output row o of the call <- staged row stage_base[i] + (o - kp_ptr[i]) of its image i.
__global__ __launch_bounds__(LANES) void k_orb_pack(long long total, int n_images, const long long* __restrict__ kp_ptr,
                                                    const long long* __restrict__ stage_base, const sfmba_orb_keypoint* __restrict__ kp_in,
                                                    const unsigned char* __restrict__ desc_in, const int* __restrict__ xy_in,
                                                    const int* __restrict__ bin_in, const long long* __restrict__ R_in,
                                                    sfmba_orb_keypoint* __restrict__ kp, unsigned char* __restrict__ desc,
                                                    int* __restrict__ xy, int* __restrict__ bins, long long* __restrict__ R) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    int lo = 0, hi = n_images;                                 // the last image with kp_ptr[i] <= o
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (kp_ptr[mid] <= o) lo = mid; else hi = mid;
    }
    const long long src = stage_base[lo] + (o - kp_ptr[lo]);
    kp[o] = kp_in[src];
    const uint4* di = reinterpret_cast<const uint4*>(desc_in + (size_t)src * ORB_DESC_BYTES);
    uint4* dd = reinterpret_cast<uint4*>(desc + (size_t)o * ORB_DESC_BYTES);
    dd[0] = di[0]; dd[1] = di[1];
    xy[2 * o] = xy_in[2 * src]; xy[2 * o + 1] = xy_in[2 * src + 1];
    bins[o] = bin_in[src];
    R[o] = R_in[src];
}

long long align4(long long n) { return (n + 3) & ~3ll; }
// no two candidates touch (each is strictly above its 8 neighbours), so a 2 x 2 cell of the admissible area holds at most one
long long candidate_bound(int w, int h) {
    if (w <= ORB_MIN_SIDE || h <= ORB_MIN_SIDE) return 0;
    return (long long)((w - 2 * ORB_EDGE + 1) / 2) * ((h - 2 * ORB_EDGE + 1) / 2);
}

const signed char* pattern_table() {
    static std::vector<signed char> table;
    static std::once_flag once;
    std::call_once(once, [] { table.resize((size_t)ORB_BINS * ORB_PAIRS * 4); orb_build_pattern(table.data()); });
    return table.data();
}

struct ImagePlan {
    int levels;                                     // levels with key points (a prefix: sizes do not grow)
    int lw[ORB_MAX_LEVELS], lh[ORB_MAX_LEVELS];
    long long scratch;                              // bytes of the group's per-level arrays this image accounts for
    long long stage_rows;                           // upper bound on its key points
};

unsigned grid_quads(long long px) { return (unsigned)((px + 4 * LANES - 1) / (4 * LANES)); }

}  // namespace

int orb_extract(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
                const int32_t* height, int channels, int n_features, float scale_factor, int n_levels, int fast_threshold,
                int64_t* kp_ptr, sfmba_orb_keypoint* kp, unsigned char* desc, int64_t cap, int64_t* total, int32_t* dbg_level_xy,
                int32_t* dbg_bin, int64_t* dbg_harris, int32_t* dbg_candidates, double* timing) {
    for (int i = 0; i <= n_images; ++i) kp_ptr[i] = 0;
    *total = 0;
    if (timing) for (int i = 0; i < ORB_T_COUNT; ++i) timing[i] = 0.0;
    if (n_images == 0) return 0;

    int quota[ORB_MAX_LEVELS];
    double scale[ORB_MAX_LEVELS];
    orb_quotas(n_features, scale_factor, n_levels, quota);
    std::vector<ImagePlan> plan((size_t)n_images);
    std::vector<long long> stage_base((size_t)n_images + 1, 0);
    for (int i = 0; i < n_images; ++i) {
        ImagePlan& P = plan[(size_t)i];
        const int lv = orb_level_sizes(width[i], height[i], scale_factor, n_levels, scale, P.lw, P.lh);
        P.levels = 0;
        P.stage_rows = 0;
        long long cb = 0;
        for (int l = 0; l < lv; ++l) {
            const long long b = candidate_bound(P.lw[l], P.lh[l]);
            if (b == 0) break;
            P.levels = l + 1;
            cb = std::max(cb, b);
            P.stage_rows += std::min<long long>(b, quota[l]);
        }
        const long long a = align4((long long)width[i] * height[i]);
        P.scratch = (channels == 3 ? 3 * a : 0) + 2 * a + a + a + (a + 4) + 4 * (a + 4) + 4 * 8 * cb;
        stage_base[(size_t)i + 1] = stage_base[(size_t)i] + P.stage_rows;
    }
    const long long stage_rows = stage_base[(size_t)n_images];

    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    // what outlives the groups: the pattern, the staged rows, the per-image counters
    DeviceArena keep(device);
    signed char* d_table;
    sfmba_orb_keypoint* d_skp;
    unsigned char* d_sdesc;
    int *d_sxy, *d_sbin, *d_ccount;
    long long *d_sR, *d_stage_cur;
    UNIT_ALLOC(keep, d_table, signed char, (size_t)ORB_BINS * ORB_PAIRS * 4);
    UNIT_ALLOC(keep, d_skp, sfmba_orb_keypoint, (size_t)stage_rows);
    UNIT_ALLOC(keep, d_sdesc, unsigned char, (size_t)stage_rows * ORB_DESC_BYTES);
    UNIT_ALLOC(keep, d_sxy, int, (size_t)stage_rows * 2);
    UNIT_ALLOC(keep, d_sbin, int, (size_t)stage_rows);
    UNIT_ALLOC(keep, d_sR, long long, (size_t)stage_rows);
    UNIT_ALLOC(keep, d_ccount, int, (size_t)n_images * n_levels);
    UNIT_ALLOC(keep, d_stage_cur, long long, (size_t)n_images);
    tm.begin(ORB_T_UPLOAD);
    UNIT_TRY(hipMemcpyAsync(d_table, pattern_table(), (size_t)ORB_BINS * ORB_PAIRS * 4, hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(d_stage_cur, stage_base.data(), sizeof(long long) * (size_t)n_images, hipMemcpyHostToDevice, s));
    tm.end();

    const long long group_bytes = group_bytes_limit(ORB_SCRATCH_BYTES);
    const int group_items = group_items_limit(ORB_MAX_GROUP_IMAGES);
    int n_groups = 0;
    for (int i0 = 0; i0 < n_images;) {
        int i1 = i0 + 1;
        long long bytes = plan[(size_t)i0].scratch;
        while (i1 < n_images && i1 - i0 < group_items && bytes + plan[(size_t)i1].scratch <= group_bytes)
            bytes += plan[(size_t)i1++].scratch;
        const int ng = i1 - i0;
        ++n_groups;
        int levels = 0;
        for (int i = i0; i < i1; ++i) levels = std::max(levels, plan[(size_t)i].levels);
        if (levels == 0) { i0 = i1; continue; }

        // the level tables, the region sizes and the candidate bound of the group
        std::vector<OrbLevel> tab((size_t)levels * ng);
        std::vector<long long> region((size_t)levels, 0), max_px((size_t)levels, 0);
        long long cand_cap = 0;
        for (int l = 0; l < levels; ++l) {
            long long off = 0, cb = 0;
            for (int i = 0; i < ng; ++i) {
                const ImagePlan& P = plan[(size_t)(i0 + i)];
                OrbLevel& T = tab[(size_t)l * ng + i];
                std::memset(&T, 0, sizeof(T));
                T.image = i0 + i;
                T.quota = quota[l];
                if (l >= P.levels) continue;
                T.w = P.lw[l]; T.h = P.lh[l];
                T.off = off;
                if (l > 0) { T.pw = P.lw[l - 1]; T.ph = P.lh[l - 1]; T.poff = tab[(size_t)(l - 1) * ng + i].off; }
                off += align4((long long)T.w * T.h);
                max_px[(size_t)l] = std::max(max_px[(size_t)l], (long long)T.w * T.h);
                cb += candidate_bound(T.w, T.h);
            }
            region[(size_t)l] = off;
            cand_cap = std::max(cand_cap, cb);
        }
        const long long r0 = region[0];
        if (r0 + 1 > (long long)INT32_MAX || cand_cap > (long long)INT32_MAX) return (int)hipErrorInvalidValue;   // unreachable below 16384^2 per group

        DeviceArena scratch(device);
        OrbLevel* d_tab;
        OrbSegment* d_seg;
        unsigned char *d_raw = nullptr, *d_pyr[2], *d_score, *d_smooth, *d_flag;
        int *d_pos, *d_total;
        uint64_t *d_key[2], *d_ent[2];
        UNIT_ALLOC(scratch, d_tab, OrbLevel, tab.size());
        UNIT_ALLOC(scratch, d_seg, OrbSegment, (size_t)ng);
        if (channels == 3) UNIT_ALLOC(scratch, d_raw, unsigned char, (size_t)r0 * 3);
        UNIT_ALLOC(scratch, d_pyr[0], unsigned char, (size_t)r0);
        UNIT_ALLOC(scratch, d_pyr[1], unsigned char, (size_t)r0);
        UNIT_ALLOC(scratch, d_score, unsigned char, (size_t)r0);
        UNIT_ALLOC(scratch, d_smooth, unsigned char, (size_t)r0);
        UNIT_ALLOC(scratch, d_flag, unsigned char, (size_t)r0 + 4);
        UNIT_ALLOC(scratch, d_pos, int, (size_t)r0 + 4);
        UNIT_ALLOC(scratch, d_total, int, 1);
        for (int b = 0; b < 2; ++b) {
            UNIT_ALLOC(scratch, d_key[b], uint64_t, (size_t)cand_cap);
            UNIT_ALLOC(scratch, d_ent[b], uint64_t, (size_t)cand_cap);
        }
        int img_bits = 1;
        while ((1 << img_bits) < ng) ++img_bits;
        size_t scan_bytes = 0, sort_bytes = 0, sort2_bytes = 0;
        hipcub::TransformInputIterator<int, ToInt, const unsigned char*> flags_in(d_flag, ToInt());
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, flags_in, d_pos, (int)(r0 + 1), s));
        {
            hipcub::DoubleBuffer<uint64_t> k(d_key[0], d_key[1]), e(d_ent[0], d_ent[1]);
            UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, k, e, (int)std::max(cand_cap, 1ll), 0, 64, s));
            UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort2_bytes, e, k, (int)std::max(cand_cap, 1ll), 32, 32 + img_bits, s));
        }
        const size_t tmp_bytes = std::max(std::max(scan_bytes, sort_bytes), std::max(sort2_bytes, (size_t)1));
        void* d_tmp = scratch.alloc(tmp_bytes);
        if (!d_tmp) return (int)hipErrorOutOfMemory;

        tm.begin(ORB_T_UPLOAD);
        UNIT_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(OrbLevel) * tab.size(), hipMemcpyHostToDevice, s));
        for (int i = 0; i < ng; ++i) {
            const OrbLevel& T = tab[(size_t)i];
            if (T.w == 0) continue;
            const size_t px = (size_t)T.w * T.h;
            if (channels == 3) UNIT_TRY(hipMemcpyAsync(d_raw + 3 * T.off, pixels + img_ptr[i0 + i], 3 * px, hipMemcpyHostToDevice, s));
            else               UNIT_TRY(hipMemcpyAsync(d_pyr[0] + T.off, pixels + img_ptr[i0 + i], px, hipMemcpyHostToDevice, s));
        }
        tm.end();

        for (int l = 0; l < levels; ++l) {
            const OrbLevel* t_l = d_tab + (size_t)l * ng;
            unsigned char* cur = d_pyr[l & 1];
            const long long rl = region[(size_t)l];
            const dim3 g_quads(grid_quads(max_px[(size_t)l]), (unsigned)ng);
            long long tiles = 0;
            for (int i = 0; i < ng; ++i) {
                const OrbLevel& T = tab[(size_t)l * ng + i];
                tiles = std::max(tiles, (long long)((T.w + ORB_TILE_W - 1) / ORB_TILE_W) * ((T.h + ORB_TILE_H - 1) / ORB_TILE_H));
            }
            const dim3 g_tiles((unsigned)tiles, (unsigned)ng);
            if (l == 0 && channels == 3) {
                tm.begin(ORB_T_PYRAMID);
                hipLaunchKernelGGL(k_orb_gray, g_quads, dim3(LANES), 0, s, t_l, d_raw, cur);
                tm.end();
            } else if (l > 0) {
                tm.begin(ORB_T_PYRAMID);
                hipLaunchKernelGGL(k_orb_resample, g_quads, dim3(LANES), 0, s, t_l, d_pyr[(l - 1) & 1], cur);
                tm.end();
            }
            tm.begin(ORB_T_SCORE);
            hipLaunchKernelGGL(k_orb_score, g_tiles, dim3(LANES), 0, s, t_l, cur, fast_threshold, d_score);
            tm.end();
            tm.begin(ORB_T_CANDIDATES);
            UNIT_TRY(hipMemsetAsync(d_flag, 0, (size_t)rl + 4, s));
            hipLaunchKernelGGL(k_orb_flags, g_quads, dim3(LANES), 0, s, t_l, d_score, d_flag);
            UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, scan_bytes, flags_in, d_pos, (int)(rl + 1), s));
            hipLaunchKernelGGL(k_orb_counts, dim3((unsigned)((ng + LANES - 1) / LANES)), dim3(LANES), 0, s, ng, l, n_levels, t_l, d_pos, d_seg,
                               d_stage_cur, d_ccount);
            UNIT_TRY(hipGetLastError());
            int n_cand = 0;
            UNIT_TRY(hipMemcpyAsync(&n_cand, d_pos + rl, sizeof(int), hipMemcpyDeviceToHost, s));
            UNIT_TRY(hipStreamSynchronize(s));
            if (n_cand < 0 || n_cand > cand_cap) return (int)hipErrorUnknown;          // cannot happen: candidate_bound
            if (n_cand == 0 || quota[l] == 0) { tm.end(); continue; }         // nothing to rank or describe at this level
            hipLaunchKernelGGL(k_orb_compact, g_quads, dim3(LANES), 0, s, t_l, d_flag, d_pos, n_cand, d_ent[0]);
            tm.end();
            tm.begin(ORB_T_HARRIS);
            hipLaunchKernelGGL(k_orb_response, dim3((unsigned)((n_cand + LANES - 1) / LANES)), dim3(LANES), 0, s, n_cand, t_l, cur, d_ent[0], d_key[0]);
            tm.end();
            tm.begin(ORB_T_SELECT);
            hipcub::DoubleBuffer<uint64_t> k(d_key[0], d_key[1]), e(d_ent[0], d_ent[1]);
            size_t bytes1 = sort_bytes, bytes2 = sort2_bytes;
            UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, bytes1, k, e, n_cand, 0, 64, s));
            if (ng > 1) UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, bytes2, e, k, n_cand, 32, 32 + img_bits, s));
            tm.end();
            tm.begin(ORB_T_SMOOTH);
            hipLaunchKernelGGL(k_orb_smooth, g_tiles, dim3(LANES), 0, s, t_l, cur, d_smooth);
            tm.end();
            tm.begin(ORB_T_DESCRIBE);
            const long long waves = std::min<long long>(quota[l], n_cand);
            hipLaunchKernelGGL(k_orb_describe, dim3((unsigned)((waves + LANES / 64 - 1) / (LANES / 64)), (unsigned)ng), dim3(LANES), 0, s, t_l, d_seg,
                               cur, d_smooth, e.Current(), k.Current(), d_table, l, scale[l], d_skp, d_sdesc, d_sxy, d_sbin, d_sR);
            UNIT_TRY(hipGetLastError());
            tm.end();
            // the next level's scan and sorts reuse d_pos, d_seg and the sort buffers: in stream order, behind this level's kernels
        }
        UNIT_TRY(hipStreamSynchronize(s));                      // the group's arena goes back to the cache below
        i0 = i1;
    }

    // kp_ptr from the per-level candidate counts, then the packed rows
    tm.begin(ORB_T_DOWNLOAD);
    std::vector<int> ccount((size_t)n_images * n_levels, 0);
    UNIT_TRY(hipMemcpyAsync(ccount.data(), d_ccount, sizeof(int) * ccount.size(), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < n_images; ++i) {
        long long n = 0;
        for (int l = 0; l < n_levels; ++l) n += std::min(ccount[(size_t)i * n_levels + l], quota[l]);
        kp_ptr[i + 1] = kp_ptr[i] + n;
    }
    const long long tot = kp_ptr[n_images];
    *total = tot;
    if (tot > cap) return UNIT_ERR_CAPACITY;
    if (dbg_candidates) std::memcpy(dbg_candidates, ccount.data(), sizeof(int) * ccount.size());
    if (tot > 0) {
        long long *d_kptr, *d_sbase, *d_oR;
        sfmba_orb_keypoint* d_okp;
        unsigned char* d_odesc;
        int *d_oxy, *d_obin;
        UNIT_ALLOC(keep, d_kptr, long long, (size_t)n_images + 1);
        UNIT_ALLOC(keep, d_sbase, long long, (size_t)n_images + 1);
        UNIT_ALLOC(keep, d_okp, sfmba_orb_keypoint, (size_t)tot);
        UNIT_ALLOC(keep, d_odesc, unsigned char, (size_t)tot * ORB_DESC_BYTES);
        UNIT_ALLOC(keep, d_oxy, int, (size_t)tot * 2);
        UNIT_ALLOC(keep, d_obin, int, (size_t)tot);
        UNIT_ALLOC(keep, d_oR, long long, (size_t)tot);
        static_assert(sizeof(long long) == sizeof(int64_t), "kp_ptr goes to the device as it is");
        UNIT_TRY(hipMemcpyAsync(d_kptr, kp_ptr, sizeof(long long) * ((size_t)n_images + 1), hipMemcpyHostToDevice, s));
        UNIT_TRY(hipMemcpyAsync(d_sbase, stage_base.data(), sizeof(long long) * ((size_t)n_images + 1), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_orb_pack, dim3((unsigned)((tot + LANES - 1) / LANES)), dim3(LANES), 0, s, tot, n_images, d_kptr, d_sbase, d_skp, d_sdesc,
                           d_sxy, d_sbin, d_sR, d_okp, d_odesc, d_oxy, d_obin, d_oR);
        UNIT_TRY(hipGetLastError());
        UNIT_TRY(hipMemcpyAsync(kp, d_okp, sizeof(sfmba_orb_keypoint) * (size_t)tot, hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipMemcpyAsync(desc, d_odesc, (size_t)tot * ORB_DESC_BYTES, hipMemcpyDeviceToHost, s));
        if (dbg_level_xy) UNIT_TRY(hipMemcpyAsync(dbg_level_xy, d_oxy, sizeof(int) * 2 * (size_t)tot, hipMemcpyDeviceToHost, s));
        if (dbg_bin) UNIT_TRY(hipMemcpyAsync(dbg_bin, d_obin, sizeof(int) * (size_t)tot, hipMemcpyDeviceToHost, s));
        if (dbg_harris) UNIT_TRY(hipMemcpyAsync(dbg_harris, d_oR, sizeof(long long) * (size_t)tot, hipMemcpyDeviceToHost, s));
    }
    tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    if (timing) {
        tm.collect(timing);
        timing[ORB_T_GROUPS] = n_groups;
    }
    return 0;
}

}  // namespace sfmba
