// surf_extract.hip -- float descriptors for a whole list of images on the MI355X (gfx950): a Fast-Hessian detector and a SURF-style
// descriptor of 64 floats, the extractor in front of match_l2.hip.
//
// The contract is the project's own, integer-exact one (include/sfmba.h, sfmba_surf_extract; arithmetic in surf_math.h), so the
// result is BIT-EXACT with a CPU restatement.
//
// Images are taken in consecutive groups bounded by SURF_SCRATCH_BYTES; every launch covers all images of the group (grid.y = image):
//
//   integral      k_surf_rows: one wave per image row, gray conversion and a 64-lane inclusive scan per chunk of the row;
//                 k_surf_cols: one lane per column, eight rows in flight.  uint32, mod 2^32, (h + 1) x (w + 1).
//   response      k_surf_response, per octave: one lane per grid sample and layer (grid.z = the four layers); H leaves as a double.
//                 A sample whose own filter is clipped is never consulted by a candidate and is not computed.
//   candidates    k_surf_candidates, per octave: one lane per grid sample of the two middle layers (grid.z), the 26 neighbours read
//                 from the response maps; a candidate is appended to one list through a counter.  The arrival order decides
//                 nothing: the list is then sorted on the whole total order.
//   selection     three stable hipCUB radix sorts: by (image, octave, layer, y, x), by the response key (descending H), by the
//                 image bits.  The first n_features entries of an image's segment are kept.
//   describe      k_surf_describe: one wave per key point.  The 109 orientation samples go over the lanes and are reduced by
//                 shuffles in int64; then lane d owns output value d: the four lanes of a sub-region share its 25 samples, a quad
//                 reduction follows, and the normalisation is a wave maximum and a wave sum.
//
// The host reads the candidate counts once per group (they size the sorts and give kp_ptr); the rows of a group leave the device
// already in output order.
#include "surf_extract.h"
#include "surf_math.h"
#include "device_arena.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;
constexpr int ENT_IMAGE_SHIFT = 31;            // entry = image of the group << 31 | octave << 29 | (layer - 1) << 28 | y << 14 | x

// One image of the group.  A too small image (no key points) keeps its entry; its kernels find nothing to do.
struct SurfImage {
    long long poff;                            // first byte of its pixels in the group's input region
    long long ioff;                            // first uint32 of its integral image
    long long roff[SURF_MAX_OCTAVES];          // first double of its response maps of octave o: [4 layers][gh][gw]
    int w, h;
    int octaves;                               // octaves that can hold a candidate in this image (a prefix; 0: no kernel touches it)
};
// An image's slice of the sorted candidate list and of the group's output rows.
struct SurfSegment {
    long long out;                             // first output row of the image within the group
    int begin, kept;
};

// I[yy][1 .. w] = running sums of gray row yy - 1; I[0][*] = I[*][0] = 0.  One wave per row of the integral image.
__global__ __launch_bounds__(LANES) void k_surf_rows(const SurfImage* __restrict__ tab, const unsigned char* __restrict__ raw, int channels,
                                                     uint32_t* __restrict__ integral) {
    const SurfImage T = tab[blockIdx.y];
    const int yy = blockIdx.x * (LANES / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (T.octaves == 0 || yy > T.h) return;                    // wave-uniform; the kernel has no barrier
    uint32_t* row = integral + T.ioff + (size_t)yy * ((size_t)T.w + 1);
    if (lane == 0) row[0] = 0u;
    const unsigned char* src = raw + T.poff + (size_t)(yy > 0 ? yy - 1 : 0) * (size_t)T.w * channels;
    uint32_t carry = 0u;
    for (int x0 = 0; x0 < T.w; x0 += 64) {
        const int x = x0 + lane;
        uint32_t v = 0u;
        if (yy > 0 && x < T.w)
            v = channels == 1 ? (uint32_t)src[x] : (uint32_t)orb_gray_bgr(src[3 * (size_t)x], src[3 * (size_t)x + 1], src[3 * (size_t)x + 2]);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = (uint32_t)__shfl_up((int)v, d, 64);
            if (lane >= d) v += u;
        }
        v += carry;
        if (x < T.w) row[x + 1] = v;
        carry = (uint32_t)__shfl((int)v, 63, 64);
    }
}

// I[yy][x] += I[yy - 1][x] down every column.  One lane per column; eight loads are in flight before the running sum needs them.
__global__ __launch_bounds__(LANES) void k_surf_cols(const SurfImage* __restrict__ tab, uint32_t* __restrict__ integral) {
    const SurfImage T = tab[blockIdx.y];
    const int x = blockIdx.x * LANES + threadIdx.x;
    if (T.octaves == 0 || x < 1 || x > T.w) return;
    const size_t st = (size_t)T.w + 1;
    uint32_t* col = integral + T.ioff + (size_t)x;
    uint32_t acc = 0u;
    int yy = 1;
    for (; yy + 7 <= T.h; yy += 8) {
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = col[(size_t)(yy + k) * st];
#pragma unroll
        for (int k = 0; k < 8; ++k) { acc += v[k]; col[(size_t)(yy + k) * st] = acc; }
    }
    for (; yy <= T.h; ++yy) { acc += col[(size_t)yy * st]; col[(size_t)yy * st] = acc; }
}

__global__ __launch_bounds__(LANES) void k_surf_response(const SurfImage* __restrict__ tab, const uint32_t* __restrict__ integral, int o,
                                                         double* __restrict__ resp) {
    const SurfImage& T = tab[blockIdx.y];                      // a reference: roff[o] is read where it lies, not from a private copy
    const int gw = surf_grid_len(T.w, o), gh = surf_grid_len(T.h, o), layer = blockIdx.z;
    const long long q = (long long)blockIdx.x * LANES + threadIdx.x;
    if (o >= T.octaves || q >= (long long)gw * gh) return;
    const int gy = (int)(q / gw), gx = (int)(q - (long long)gy * gw);
    const int L = surf_layer_size(o, layer);
    if (!surf_filter_inside(T.w, T.h, gy << o, gx << o, L)) return;           // never consulted (surf_candidate_inside)
    long long lap;
    resp[T.roff[o] + (long long)layer * gw * gh + q] = surf_hessian(integral + T.ioff, T.w, T.h, gy << o, gx << o, L, lap);
}

__global__ __launch_bounds__(LANES) void k_surf_candidates(const SurfImage* __restrict__ tab, const double* __restrict__ resp, int o, int n_octaves,
                                                           int image0, double threshold, int cap, int* __restrict__ n_cand,
                                                           int* __restrict__ counts, uint64_t* __restrict__ entry, uint64_t* __restrict__ key) {
    const SurfImage& T = tab[blockIdx.y];
    const int gw = surf_grid_len(T.w, o), gh = surf_grid_len(T.h, o), m = (int)blockIdx.z + 1;
    const long long q = (long long)blockIdx.x * LANES + threadIdx.x, plane = (long long)gw * gh;
    if (o >= T.octaves || q >= plane) return;
    const int gy = (int)(q / gw), gx = (int)(q - (long long)gy * gw);
    const int x = gx << o, y = gy << o;
    if (!surf_candidate_inside(T.w, T.h, y, x, o, m)) return;                 // so gx, gy >= 1 and gx + 1 < gw, gy + 1 < gh
    const double* R = resp + T.roff[o];
    const double v = R[m * plane + q];
    if (!(v > threshold)) return;
    bool top = true;
#pragma unroll
    for (int dl = -1; dl <= 1; ++dl)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
                if ((dl | dy | dx) != 0 && !(v > R[(m + dl) * plane + (long long)(gy + dy) * gw + (gx + dx)])) top = false;
    if (!top) return;
    atomicAdd(&counts[((image0 + (int)blockIdx.y) * n_octaves + o) * 2 + (m - 1)], 1);
    const int at = atomicAdd(n_cand, 1);
    if (at >= cap) return;                                                    // cannot happen: candidate_bound
    entry[at] = ((uint64_t)blockIdx.y << ENT_IMAGE_SHIFT) | ((uint64_t)o << 29) | ((uint64_t)(m - 1) << 28) | ((uint64_t)y << 14) | (uint64_t)x;
    key[at] = surf_response_key(v);
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// One wave per key point: rank r of image blockIdx.y.
__global__ __launch_bounds__(LANES) void k_surf_describe(const SurfImage* __restrict__ tab, const SurfSegment* __restrict__ seg,
                                                         const uint32_t* __restrict__ integral, const uint64_t* __restrict__ entry,
                                                         const uint64_t* __restrict__ key, int upright, sfmba_surf_keypoint* __restrict__ kp,
                                                         float* __restrict__ desc, int* __restrict__ bins, long long* __restrict__ moments,
                                                         long long* __restrict__ sums) {
    const SurfSegment g = seg[blockIdx.y];
    const int r = blockIdx.x * (LANES / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= g.kept) return;                                   // wave-uniform; the kernel has no barrier
    const SurfImage T = tab[blockIdx.y];
    const uint64_t e = entry[g.begin + r];
    const int x = (int)(e & 0x3fffu), y = (int)((e >> 14) & 0x3fffu), m = (int)((e >> 28) & 1u) + 1, o = (int)((e >> 29) & 3u);
    const int L = surf_layer_size(o, m), l = L / 3;
    const uint32_t* I = integral + T.ioff;

    long long mx = 0, my = 0;
    int bin = 0;
    if (!upright) {
        for (int t = lane; t < SURF_ORI_SIDE * SURF_ORI_SIDE; t += 64) surf_orient_sample(I, T.w, T.h, y, x, l, t, mx, my);
        mx = wave_sum(mx);
        my = wave_sum(my);
        bin = orb_bin(mx, my);
    }

    // lane = 4 * sub-region + component; the quad shares the 25 samples of the sub-region
    const int sr = lane >> 2, c = lane & 3, p = sr & 3, q = sr >> 2;
    long long v[4] = { 0, 0, 0, 0 };
    for (int t = c; t < 25; t += 4) surf_desc_sample(I, T.w, T.h, y, x, l, bin, 5 * p - 10 + t % 5, 5 * q - 10 + t / 5, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] += __shfl_xor(v[k], 1, 64);
        v[k] += __shfl_xor(v[k], 2, 64);
    }
    const long long mine = c == 0 ? v[0] : (c == 1 ? v[1] : (c == 2 ? v[2] : v[3]));
    long long M = mine < 0 ? -mine : mine;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const long long u = __shfl_xor(M, d, 64); M = u > M ? u : M; }
    const long long t = mine >> surf_norm_shift(M);
    const long long n2 = wave_sum(t * t);

    const long long row = g.out + r;
    desc[(size_t)row * SURF_DESC_DIMS + lane] = surf_desc_value(t, n2);
    sums[(size_t)row * SURF_DESC_DIMS + lane] = mine;
    if (lane == 0) {
        long long lap;
        (void)surf_hessian(I, T.w, T.h, y, x, L, lap);
        sfmba_surf_keypoint k;
        k.x = (float)x;
        k.y = (float)y;
        k.size = (float)L;
        k.angle = (float)(12 * bin);
        k.response = (float)surf_key_response(key[g.begin + r]);
        k.octave = o;
        k.layer = m;
        k.laplacian = lap >= 0 ? 1 : -1;
        kp[row] = k;
        bins[row] = bin;
        moments[2 * row] = mx;
        moments[2 * row + 1] = my;
    }
}

long long align64(long long n) { return (n + 63) & ~63ll; }

// The candidates of a layer are strictly above their 8 neighbours of that layer, so no two touch: a 2 x 2 cell of the admissible grid
// positions holds at most one.
long long axis_positions(int n, int o, int m) {
    const int s = 1 << o, bt = (surf_layer_size(o, m + 1) - 1) / 2;
    const int lo = (s + bt + s - 1) / s, hi = n - 1 - s - bt;                  // grid indices lo .. floor(hi / s)
    if (hi < 0) return 0;
    return std::max(0, hi / s - lo + 1);
}
long long candidate_bound(int w, int h, int n_octaves) {
    long long b = 0;
    for (int o = 0; o < n_octaves; ++o)
        for (int m = 1; m <= 2; ++m) b += ((axis_positions(w, o, m) + 1) / 2) * ((axis_positions(h, o, m) + 1) / 2);
    return b;
}

struct ImagePlan {
    long long resp[SURF_MAX_OCTAVES];          // doubles of the response maps of octave o (0: the octave finds nothing in this image)
    long long cand;                            // upper bound on its candidates
    long long scratch;                         // bytes of the group's arrays this image accounts for
};

}  // namespace

int surf_extract(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
                 const int32_t* height, int channels, int n_features, int n_octaves, float hessian_threshold, int upright, int64_t* kp_ptr,
                 sfmba_surf_keypoint* kp, float* desc, int64_t cap, int64_t* total, int32_t* dbg_bin, int64_t* dbg_moments, int64_t* dbg_sums,
                 int32_t* dbg_candidates, double* timing) {
    for (int i = 0; i <= n_images; ++i) kp_ptr[i] = 0;
    *total = 0;
    if (timing) for (int i = 0; i < SURF_T_COUNT; ++i) timing[i] = 0.0;
    if (n_images == 0) return 0;

    std::vector<ImagePlan> plan((size_t)n_images);
    for (int i = 0; i < n_images; ++i) {
        ImagePlan& P = plan[(size_t)i];
        const int w = width[i], h = height[i];
        P.cand = candidate_bound(w, h, n_octaves);
        long long resp = 0;
        for (int o = 0; o < SURF_MAX_OCTAVES; ++o) {
            const bool live = o < n_octaves && axis_positions(w, o, 1) > 0 && axis_positions(h, o, 1) > 0;
            P.resp[o] = live ? align64((long long)SURF_LAYERS * surf_grid_len(w, o) * surf_grid_len(h, o)) : 0;
            resp += P.resp[o];
        }
        P.scratch = align64((long long)w * h * channels) + 4 * align64((long long)(w + 1) * (h + 1)) + 8 * resp + 4 * 8 * P.cand;
    }

    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    DeviceArena keep(device);
    int* d_counts;                                             // [n_images][n_octaves][2]
    const size_t n_counts = (size_t)n_images * n_octaves * 2;
    UNIT_ALLOC(keep, d_counts, int, n_counts);                 // handed out zeroed
    std::vector<int> counts(n_counts, 0);
    // the rows of the call, staged on the host: nothing reaches the caller's arrays unless the whole call fits
    std::vector<sfmba_surf_keypoint> h_kp;
    std::vector<float> h_desc;
    std::vector<int> h_bin;
    std::vector<long long> h_mom, h_sums;
    double response_bytes = 0.0;

    const long long group_bytes = group_bytes_limit(SURF_SCRATCH_BYTES);
    const int group_items = group_items_limit(SURF_MAX_GROUP_IMAGES);
    int n_groups = 0;
    for (int i0 = 0; i0 < n_images;) {
        int i1 = i0 + 1;
        long long bytes = plan[(size_t)i0].scratch;
        while (i1 < n_images && i1 - i0 < group_items && bytes + plan[(size_t)i1].scratch <= group_bytes)
            bytes += plan[(size_t)i1++].scratch;
        const int ng = i1 - i0;
        ++n_groups;

        // the image table and the region sizes of the group
        std::vector<SurfImage> tab((size_t)ng);
        long long raw_bytes = 0, int_words = 0, resp_doubles = 0, cand_cap = 0, max_rows = 0, max_cols = 0;
        long long max_plane[SURF_MAX_OCTAVES] = { 0, 0, 0, 0 };
        for (int i = 0; i < ng; ++i) {
            const ImagePlan& P = plan[(size_t)(i0 + i)];
            SurfImage& T = tab[(size_t)i];
            std::memset(&T, 0, sizeof(T));
            T.w = width[i0 + i]; T.h = height[i0 + i];
            T.poff = raw_bytes;
            T.ioff = int_words;
            raw_bytes += align64((long long)T.w * T.h * channels);
            int_words += align64((long long)(T.w + 1) * (T.h + 1));
            for (int o = 0; o < n_octaves; ++o) {
                T.roff[o] = resp_doubles;
                resp_doubles += P.resp[o];
                if (P.resp[o]) T.octaves = o + 1;
                if (P.resp[o]) max_plane[o] = std::max(max_plane[o], (long long)surf_grid_len(T.w, o) * surf_grid_len(T.h, o));
            }
            cand_cap += P.cand;
            if (P.cand) { max_rows = std::max(max_rows, (long long)T.h + 1); max_cols = std::max(max_cols, (long long)T.w + 1); }
        }
        if (cand_cap == 0) {                                   // every image of the group is too small for a key point
            for (int i = i0; i < i1; ++i) kp_ptr[i + 1] = kp_ptr[i];
            i0 = i1;
            continue;
        }
        if (cand_cap > (long long)INT32_MAX) return (int)hipErrorInvalidValue;      // unreachable below 16384^2 per group

        DeviceArena scratch(device);
        SurfImage* d_tab;
        SurfSegment* d_seg;
        unsigned char* d_raw;
        uint32_t* d_int;
        double* d_resp;
        int* d_ncand;
        uint64_t *d_key[2], *d_ent[2];
        UNIT_ALLOC(scratch, d_tab, SurfImage, (size_t)ng);
        UNIT_ALLOC(scratch, d_seg, SurfSegment, (size_t)ng);
        UNIT_ALLOC(scratch, d_raw, unsigned char, (size_t)raw_bytes);
        UNIT_ALLOC(scratch, d_int, uint32_t, (size_t)int_words);
        UNIT_ALLOC(scratch, d_resp, double, (size_t)resp_doubles);
        UNIT_ALLOC(scratch, d_ncand, int, 1);
        for (int b = 0; b < 2; ++b) {
            UNIT_ALLOC(scratch, d_key[b], uint64_t, (size_t)cand_cap);
            UNIT_ALLOC(scratch, d_ent[b], uint64_t, (size_t)cand_cap);
        }
        int img_bits = 1;
        while ((1 << img_bits) < ng) ++img_bits;
        size_t sort_a = 0, sort_b = 0, sort_c = 0;
        {
            hipcub::DoubleBuffer<uint64_t> k(d_key[0], d_key[1]), e(d_ent[0], d_ent[1]);
            UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_a, e, k, (int)cand_cap, 0, ENT_IMAGE_SHIFT + img_bits, s));
            UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, k, e, (int)cand_cap, 0, 64, s));
            UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_c, e, k, (int)cand_cap, ENT_IMAGE_SHIFT, ENT_IMAGE_SHIFT + img_bits, s));
        }
        const size_t tmp_bytes = std::max(std::max(sort_a, sort_b), std::max(sort_c, (size_t)1));
        void* d_tmp = scratch.alloc(tmp_bytes);
        if (!d_tmp) return (int)hipErrorOutOfMemory;

        tm.begin(SURF_T_UPLOAD);
        UNIT_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(SurfImage) * tab.size(), hipMemcpyHostToDevice, s));
        for (int i = 0; i < ng; ++i)
            if (plan[(size_t)(i0 + i)].cand)
                UNIT_TRY(hipMemcpyAsync(d_raw + tab[(size_t)i].poff, pixels + img_ptr[i0 + i], (size_t)tab[(size_t)i].w * tab[(size_t)i].h * channels,
                                        hipMemcpyHostToDevice, s));
        tm.end();

        tm.begin(SURF_T_INTEGRAL);
        hipLaunchKernelGGL(k_surf_rows, dim3((unsigned)((max_rows + LANES / 64 - 1) / (LANES / 64)), (unsigned)ng), dim3(LANES), 0, s, d_tab, d_raw,
                           channels, d_int);
        hipLaunchKernelGGL(k_surf_cols, dim3((unsigned)((max_cols + LANES - 1) / LANES), (unsigned)ng), dim3(LANES), 0, s, d_tab, d_int);
        UNIT_TRY(hipGetLastError());
        tm.end();
        for (int o = 0; o < n_octaves; ++o) {
            if (max_plane[o] == 0) continue;
            const unsigned gx = (unsigned)((max_plane[o] + LANES - 1) / LANES);
            tm.begin(SURF_T_RESPONSE);
            hipLaunchKernelGGL(k_surf_response, dim3(gx, (unsigned)ng, SURF_LAYERS), dim3(LANES), 0, s, d_tab, d_int, o, d_resp);
            tm.end();
            tm.begin(SURF_T_CANDIDATES);
            hipLaunchKernelGGL(k_surf_candidates, dim3(gx, (unsigned)ng, 2), dim3(LANES), 0, s, d_tab, d_resp, o, n_octaves, i0,
                               (double)hessian_threshold, (int)cand_cap, d_ncand, d_counts, d_ent[0], d_key[0]);
            UNIT_TRY(hipGetLastError());
            tm.end();
            if (timing)
                for (int i = 0; i < ng; ++i)
                    for (int layer = 0; layer < SURF_LAYERS && plan[(size_t)(i0 + i)].resp[o]; ++layer) {
                        const int b = (surf_layer_size(o, layer) - 1) / 2, st = 1 << o, w = tab[(size_t)i].w, h = tab[(size_t)i].h;
                        const long long nx = (w - 1 - b) / st - (b + st - 1) / st + 1, ny = (h - 1 - b) / st - (b + st - 1) / st + 1;
                        if (nx > 0 && ny > 0) response_bytes += 8.0 * (double)nx * (double)ny;
                    }
        }

        // the counts of the group: sizes of the sorts, kp_ptr, the segments.  The phase open at the end of this block (select when
        // nothing is described, download otherwise) is closed behind it.
        tm.begin(SURF_T_SELECT);
        int n_cand = 0;
        UNIT_TRY(hipMemcpyAsync(&n_cand, d_ncand, sizeof(int), hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipMemcpyAsync(counts.data() + (size_t)i0 * n_octaves * 2, d_counts + (size_t)i0 * n_octaves * 2, sizeof(int) * (size_t)ng * n_octaves * 2,
                                hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipStreamSynchronize(s));
        if (n_cand < 0 || n_cand > cand_cap) return (int)hipErrorUnknown;          // cannot happen: candidate_bound
        std::vector<SurfSegment> seg((size_t)ng);
        long long begin = 0, rows = 0, max_kept = 0;
        for (int i = 0; i < ng; ++i) {
            long long c = 0;
            for (int j = 0; j < n_octaves * 2; ++j) c += counts[(size_t)(i0 + i) * n_octaves * 2 + j];
            const long long kept = std::min<long long>(c, n_features);
            seg[(size_t)i].begin = (int)begin;
            seg[(size_t)i].kept = (int)kept;
            seg[(size_t)i].out = rows;
            begin += c;
            rows += kept;
            max_kept = std::max(max_kept, kept);
            kp_ptr[i0 + i + 1] = kp_ptr[i0 + i] + kept;
        }
        if (begin != n_cand) return (int)hipErrorUnknown;
        const long long row0 = kp_ptr[i0];
        if (rows > 0 && kp_ptr[i1] <= cap) {
            hipcub::DoubleBuffer<uint64_t> k(d_key[0], d_key[1]), e(d_ent[0], d_ent[1]);
            size_t ba = sort_a, bb = sort_b, bc = sort_c;
            UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, ba, e, k, n_cand, 0, ENT_IMAGE_SHIFT + img_bits, s));
            UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, bb, k, e, n_cand, 0, 64, s));
            if (ng > 1) UNIT_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, bc, e, k, n_cand, ENT_IMAGE_SHIFT, ENT_IMAGE_SHIFT + img_bits, s));
            tm.end();

            sfmba_surf_keypoint* d_kp;
            float* d_desc;
            int* d_bin;
            long long *d_mom, *d_sums;
            UNIT_ALLOC(scratch, d_kp, sfmba_surf_keypoint, (size_t)rows);
            UNIT_ALLOC(scratch, d_desc, float, (size_t)rows * SURF_DESC_DIMS);
            UNIT_ALLOC(scratch, d_bin, int, (size_t)rows);
            UNIT_ALLOC(scratch, d_mom, long long, (size_t)rows * 2);
            UNIT_ALLOC(scratch, d_sums, long long, (size_t)rows * SURF_DESC_DIMS);
            tm.begin(SURF_T_DESCRIBE);
            UNIT_TRY(hipMemcpyAsync(d_seg, seg.data(), sizeof(SurfSegment) * seg.size(), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_surf_describe, dim3((unsigned)((max_kept + LANES / 64 - 1) / (LANES / 64)), (unsigned)ng), dim3(LANES), 0, s, d_tab, d_seg,
                               d_int, e.Current(), k.Current(), upright, d_kp, d_desc, d_bin, d_mom, d_sums);
            UNIT_TRY(hipGetLastError());
            tm.end();
            tm.begin(SURF_T_DOWNLOAD);
            const size_t end = (size_t)(row0 + rows);
            h_kp.resize(end);
            h_desc.resize(end * SURF_DESC_DIMS);
            UNIT_TRY(hipMemcpyAsync(h_kp.data() + row0, d_kp, sizeof(sfmba_surf_keypoint) * (size_t)rows, hipMemcpyDeviceToHost, s));
            UNIT_TRY(hipMemcpyAsync(h_desc.data() + (size_t)row0 * SURF_DESC_DIMS, d_desc, sizeof(float) * (size_t)rows * SURF_DESC_DIMS, hipMemcpyDeviceToHost, s));
            if (dbg_bin) {
                h_bin.resize(end);
                UNIT_TRY(hipMemcpyAsync(h_bin.data() + row0, d_bin, sizeof(int) * (size_t)rows, hipMemcpyDeviceToHost, s));
            }
            if (dbg_moments) {
                h_mom.resize(end * 2);
                UNIT_TRY(hipMemcpyAsync(h_mom.data() + (size_t)row0 * 2, d_mom, sizeof(long long) * (size_t)rows * 2, hipMemcpyDeviceToHost, s));
            }
            if (dbg_sums) {
                h_sums.resize(end * SURF_DESC_DIMS);
                UNIT_TRY(hipMemcpyAsync(h_sums.data() + (size_t)row0 * SURF_DESC_DIMS, d_sums, sizeof(long long) * (size_t)rows * SURF_DESC_DIMS,
                                        hipMemcpyDeviceToHost, s));
            }
        }
        tm.end();
        UNIT_TRY(hipStreamSynchronize(s));                     // the group's arena goes back to the cache below
        i0 = i1;
    }

    const long long tot = kp_ptr[n_images];
    *total = tot;
    if (tot > cap) return UNIT_ERR_CAPACITY;
    static_assert(sizeof(long long) == sizeof(int64_t), "the debug rows leave as they are");
    if (dbg_candidates) std::memcpy(dbg_candidates, counts.data(), sizeof(int) * counts.size());
    if (tot > 0) {
        std::memcpy(kp, h_kp.data(), sizeof(sfmba_surf_keypoint) * (size_t)tot);
        std::memcpy(desc, h_desc.data(), sizeof(float) * (size_t)tot * SURF_DESC_DIMS);
        if (dbg_bin) std::memcpy(dbg_bin, h_bin.data(), sizeof(int) * (size_t)tot);
        if (dbg_moments) std::memcpy(dbg_moments, h_mom.data(), sizeof(long long) * (size_t)tot * 2);
        if (dbg_sums) std::memcpy(dbg_sums, h_sums.data(), sizeof(long long) * (size_t)tot * SURF_DESC_DIMS);
    }
    if (timing) {
        tm.collect(timing);
        timing[SURF_T_GROUPS] = n_groups;
        timing[SURF_T_RESPONSE_BYTES] = response_bytes;
    }
    return 0;
}

}  // namespace sfmba
