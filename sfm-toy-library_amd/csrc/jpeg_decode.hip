// jpeg_decode.hip -- sfmba_jpeg_decode and sfmba_resize_images for a whole list of images on the MI355X (gfx950).
//
// Reference: SfM::setImagesDirectory (SfMToyLib/SfM.cpp:125-129) calls imread and resize per image, serially.  The contract here is
// the project's own, integer-exact one (include/sfmba.h; arithmetic in jpeg_math.h): the decode equals libjpeg's default decode of
// a baseline file bit for bit, and both calls are BIT-EXACT with a CPU restatement (tests/jpeg_oracle.py).
//
// The host half (jpeg_entropy.cpp) parses and Huffman-decodes every file with at most 16 threads; the device never sees file
// bytes, and every device array is sized from validated header fields.  Images are taken in consecutive groups bounded by
// JPEG_SCRATCH_BYTES; every launch covers all images of the group:
//
//   idct      k_jpeg_idct, grid.y = component of an image: a block of 256 lanes works 32 blocks of 8 x 8 coefficients, 8 lanes each.
//             Lane j dequantises and transforms column j, the 8 x 8 intermediate goes through LDS (32 x 8 rows of 9 words: the
//             padding makes both the column-wise write and the row-wise read bank-conflict free; 9216 bytes per block), lane j
//             transforms row j and stores its 8 samples as one 64-bit word into the component's plane (8 bw bytes per row).
//   colour    k_jpeg_colour, grid.y = image: four consecutive output pixels per lane; luma read directly, chroma through the
//             triangle filter from the component's own cw x ch samples (the MCU padding is never read), fixed-point colour
//             conversion, three packed 32-bit stores (B, G, R interleaved) or one for a single component.
//   resize    k_resize, grid.y = image: four consecutive output bytes per lane, one packed store; the (index, weight) tables of both
//             axes are built on the host in double and uploaded, so no device contraction can change a weight.
//
// No atomics anywhere: every output byte has one writer.
#include "jpeg_decode.h"
#include "jpeg_math.h"
#include "device_arena.h"

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;
constexpr int BLOCKS_PER_GROUP = LANES / 8;       // 8 x 8 blocks per thread block
constexpr int WS_ROW = 9;                         // words per row of the LDS intermediate

// One component of one image of the group.
struct JpegPlane {
    long long coef;             // first coefficient of its blocks in the group's array (a multiple of 64)
    long long plane;            // first byte of its plane in the group's plane region (a multiple of 64)
    long long blocks;           // bw * bh
    int bw;
    int quant;                  // first entry of its quantiser in the group's table (a multiple of 64)
};
// One image of the group for the colour kernel.
struct JpegImage {
    long long plane[3];
    long long out;              // first byte of its pixels in the decoded region (a multiple of 4)
    int stride[3];              // bytes per plane row
    int w, h, ncomp;
    int mode;                   // chroma: 0 as large as luma, 1 doubled horizontally, 2 doubled both ways
    int cw, ch;                 // chroma samples
};
// One image of the group for the resize kernel.
struct ResizeImage {
    long long src, dst;         // first bytes in the source and destination regions (multiples of 4)
    long long xt, yt;           // first entries of its tables
    int w, h, ow, oh, channels;
};

__device__ __forceinline__ unsigned pack4(const int (&v)[4]) {
    return (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
}

__global__ __launch_bounds__(LANES) void k_jpeg_idct(const JpegPlane* __restrict__ tab, const int16_t* __restrict__ coef,
                                                     const unsigned short* __restrict__ quant, unsigned char* __restrict__ planes) {
    __shared__ int ws[BLOCKS_PER_GROUP * 8 * WS_ROW];
    const JpegPlane T = tab[blockIdx.y];
    if ((long long)blockIdx.x * BLOCKS_PER_GROUP >= T.blocks) return;          // the whole block leaves: no barrier is skipped
    const int lb = threadIdx.x >> 3, j = threadIdx.x & 7;
    const long long b = (long long)blockIdx.x * BLOCKS_PER_GROUP + lb;
    const bool live = b < T.blocks;
    int* w = ws + lb * 8 * WS_ROW;
    if (live) {
        const int16_t* c = coef + T.coef + b * 64 + j;
        const unsigned short* q = quant + T.quant + j;
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = jpeg_dequant(c[8 * k], q[8 * k]);
        jpeg_idct_column(in, out);
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k * WS_ROW + j] = out[k];
    }
    __syncthreads();
    if (!live) return;
    int in[8], sample[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = w[j * WS_ROW + k];
    jpeg_idct_row(in, sample);
    const int by = (int)(b / T.bw), bx = (int)(b - (long long)by * T.bw);
    const int lo[4] = { sample[0], sample[1], sample[2], sample[3] }, hi[4] = { sample[4], sample[5], sample[6], sample[7] };
    // 8-byte aligned: the plane starts at a multiple of 64 and a row holds 8 bw bytes
    *reinterpret_cast<uint2*>(planes + T.plane + ((size_t)by * 8 + j) * ((size_t)T.bw * 8) + (size_t)bx * 8) = make_uint2(pack4(lo), pack4(hi));
}

__global__ __launch_bounds__(LANES) void k_jpeg_colour(const JpegImage* __restrict__ tab, const unsigned char* __restrict__ planes,
                                                       unsigned char* __restrict__ dst) {
    const JpegImage T = tab[blockIdx.y];
    // 32-bit throughout: an image has at most 16384 x 16384 pixels, and the grid overshoots that by less than one block
    const unsigned n = (unsigned)T.w * (unsigned)T.h, q = (blockIdx.x * LANES + threadIdx.x) * 4u;
    if (q >= n) return;
    int y = (int)(q / (unsigned)T.w), x = (int)(q - (unsigned)y * (unsigned)T.w);     // the one division of the lane; the pixels after it step
    const unsigned char* Y = planes + T.plane[0];
    if (T.ncomp == 1) {
        int v[4] = { 0, 0, 0, 0 };
        for (int i = 0; i < 4 && q + i < n; ++i) {
            v[i] = Y[(size_t)y * T.stride[0] + x];
            if (++x == T.w) { x = 0; ++y; }
        }
        unsigned char* o = dst + T.out + q;
        if (q + 3 < n) *reinterpret_cast<unsigned*>(o) = pack4(v);
        else for (int i = 0; i < 4 && q + i < n; ++i) o[i] = (unsigned char)v[i];
        return;
    }
    const unsigned char* Cb = planes + T.plane[1];
    const unsigned char* Cr = planes + T.plane[2];
    int px[12] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    for (int i = 0; i < 4 && q + i < n; ++i) {
        int cb, cr;
        if (T.mode == 0) {
            cb = Cb[(size_t)y * T.stride[1] + x];
            cr = Cr[(size_t)y * T.stride[2] + x];
        } else if (T.mode == 1) {
            cb = jpeg_up_h2v1(Cb + (size_t)y * T.stride[1], T.cw, x);
            cr = jpeg_up_h2v1(Cr + (size_t)y * T.stride[2], T.cw, x);
        } else {
            cb = jpeg_up_h2v2(Cb, T.stride[1], T.cw, T.ch, x, y);
            cr = jpeg_up_h2v2(Cr, T.stride[2], T.cw, T.ch, x, y);
        }
        jpeg_ycc_to_bgr(Y[(size_t)y * T.stride[0] + x], cb, cr, px[3 * i], px[3 * i + 1], px[3 * i + 2]);
        if (++x == T.w) { x = 0; ++y; }
    }
    unsigned char* o = dst + T.out + 3 * (size_t)q;
    if (q + 3 < n) {
        const int a[4] = { px[0], px[1], px[2], px[3] }, b[4] = { px[4], px[5], px[6], px[7] }, c[4] = { px[8], px[9], px[10], px[11] };
        unsigned* o32 = reinterpret_cast<unsigned*>(o);          // T.out and 3 q are multiples of 4
        o32[0] = pack4(a); o32[1] = pack4(b); o32[2] = pack4(c);
    } else {
        for (unsigned i = 0; i < 12 && i < 3 * (n - q); ++i) o[i] = (unsigned char)px[i];
    }
}

__global__ __launch_bounds__(LANES) void k_resize(const ResizeImage* __restrict__ tab, const ResizeEntry* __restrict__ tables,
                                                  const unsigned char* __restrict__ src, unsigned char* __restrict__ dst) {
    const ResizeImage T = tab[blockIdx.y];
    // 32-bit throughout: an image has fewer than 2^30 bytes (16384 x 16384 x 3), and the grid overshoots that by less than one block
    const unsigned n = (unsigned)T.ow * (unsigned)T.oh * (unsigned)T.channels, q = (blockIdx.x * LANES + threadIdx.x) * 4u;
    if (q >= n) return;
    const unsigned p = q / (unsigned)T.channels;                       // the two divisions of the lane; the bytes after the first step
    int c = (int)(q - p * (unsigned)T.channels), y = (int)(p / (unsigned)T.ow), x = (int)(p - (unsigned)y * (unsigned)T.ow);
    int v[4] = { 0, 0, 0, 0 };
    for (int i = 0; i < 4 && q + i < n; ++i) {
        v[i] = resize_pixel(src + T.src, T.w, T.h, T.channels, tables + T.xt, tables + T.yt, x, y, c);
        if (++c == T.channels) { c = 0; if (++x == T.ow) { x = 0; ++y; } }
    }
    unsigned char* o = dst + T.dst + q;
    if (q + 3 < n) *reinterpret_cast<unsigned*>(o) = pack4(v);
    else for (int i = 0; i < 4 && q + i < n; ++i) o[i] = (unsigned char)v[i];
}

long long align4(long long n) { return (n + 3) & ~3ll; }
unsigned grid_quads(long long n) { return (unsigned)((n + 4 * LANES - 1) / (4 * LANES)); }

}  // namespace

long long resize_scratch(const ResizeJob& j) { return align4((long long)j.ow * j.oh * j.channels) + 8ll * (j.ow + j.oh); }

// Tables up, one launch over the jobs: *d_dst receives the destination region, dst_off [jobs] the first byte of each result.
int launch_resize(hipStream_t s, DeviceArena& arena, PhaseTimer& tm, const std::vector<ResizeJob>& jobs, float factor, const unsigned char* d_src,
                  unsigned char** d_dst, std::vector<long long>& dst_off) {
    const double inv = 1.0 / (double)factor;
    std::vector<ResizeImage> tab(jobs.size());
    std::vector<ResizeEntry> entries;
    long long off = 0, max_bytes = 0;
    dst_off.assign(jobs.size(), 0);
    for (size_t i = 0; i < jobs.size(); ++i) {
        const ResizeJob& J = jobs[i];
        ResizeImage& T = tab[i];
        T.src = J.src; T.dst = off;
        T.w = J.w; T.h = J.h; T.ow = J.ow; T.oh = J.oh; T.channels = J.channels;
        T.xt = (long long)entries.size();
        for (int x = 0; x < J.ow; ++x) entries.push_back(resize_axis_entry(x, J.w, inv));
        T.yt = (long long)entries.size();
        for (int y = 0; y < J.oh; ++y) entries.push_back(resize_axis_entry(y, J.h, inv));
        dst_off[i] = off;
        const long long bytes = (long long)J.ow * J.oh * J.channels;
        max_bytes = std::max(max_bytes, bytes);
        off += align4(bytes);
    }
    ResizeImage* d_tab;
    ResizeEntry* d_entries;
    UNIT_DRAIN_ALLOC(arena, d_tab, ResizeImage, tab.size());
    UNIT_DRAIN_ALLOC(arena, d_entries, ResizeEntry, entries.size());
    UNIT_DRAIN_ALLOC(arena, *d_dst, unsigned char, (size_t)off);
    tm.begin(JPEG_T_UPLOAD);
    UNIT_DRAIN_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(ResizeImage) * tab.size(), hipMemcpyHostToDevice, s));
    UNIT_DRAIN_TRY(hipMemcpyAsync(d_entries, entries.data(), sizeof(ResizeEntry) * entries.size(), hipMemcpyHostToDevice, s));
    tm.end();
    tm.begin(JPEG_T_RESIZE);
    hipLaunchKernelGGL(k_resize, dim3(grid_quads(max_bytes), (unsigned)jobs.size()), dim3(LANES), 0, s, d_tab, d_entries, d_src, *d_dst);
    UNIT_DRAIN_TRY(hipGetLastError());
    tm.end();
    UNIT_DRAIN_TRY(hipStreamSynchronize(s));                         // the host tables leave scope here
    return 0;
}

namespace {

double now_ms() { return 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

void jpeg_fill_info(const JpegHeader& h, sfmba_image_info* info) {
    std::memset(info, 0, sizeof(*info));
    info->status = h.status;
    if (h.status != JPEG_OK) return;
    info->width = h.width; info->height = h.height; info->channels = h.ncomp;
    info->h_samp = h.hmax; info->v_samp = h.vmax;
    info->restart_interval = h.restart_interval;
}

int jpeg_decode(hipStream_t s, int device, int n_images, const int64_t* file_ptr, const unsigned char* bytes, float factor,
                sfmba_image_info* info, int64_t* out_ptr, unsigned char* out, int64_t cap, int64_t* total, double* timing) {
    if (timing) for (int i = 0; i < JPEG_T_COUNT; ++i) timing[i] = 0.0;
    const double t0 = timing ? now_ms() : 0.0;
    std::vector<JpegHeader> hdr;
    std::vector<std::vector<int16_t> > coef;
    jpeg_parse_batch(n_images, file_ptr, bytes, hdr);
    // the sizes come from the headers alone: a refused factor is refused here, before the first write and before any scan is decoded
    const bool resize = factor != 1.0f;
    std::vector<int> ow((size_t)n_images, 0), oh((size_t)n_images, 0);
    for (int i = 0; i < n_images; ++i) {
        const JpegHeader& H = hdr[(size_t)i];
        if (H.status != JPEG_OK) continue;
        ow[(size_t)i] = resize ? resized_length(H.width, factor) : H.width;
        oh[(size_t)i] = resize ? resized_length(H.height, factor) : H.height;
        if (ow[(size_t)i] == 0 || oh[(size_t)i] == 0) return UNIT_ERR_SIZE;
    }
    if (!jpeg_scan_batch(n_images, file_ptr, bytes, 16, hdr, coef)) return UNIT_ERR_HOST_ALLOC;
    if (timing) timing[JPEG_T_ENTROPY] = now_ms() - t0;

    out_ptr[0] = 0;
    for (int i = 0; i < n_images; ++i) {
        const JpegHeader& H = hdr[(size_t)i];
        jpeg_fill_info(H, &info[i]);
        out_ptr[i + 1] = out_ptr[i] + (H.status == JPEG_OK ? (long long)ow[(size_t)i] * oh[(size_t)i] * H.ncomp : 0);
    }
    *total = out_ptr[n_images];
    if (*total > cap) return UNIT_ERR_CAPACITY;

    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    const long long group_bytes = group_bytes_limit(JPEG_SCRATCH_BYTES);
    const int group_items = group_items_limit(JPEG_MAX_GROUP_IMAGES);
    int n_groups = 0;
    auto scratch_of = [&](int i) -> long long {
        const JpegHeader& H = hdr[(size_t)i];
        if (H.status != JPEG_OK) return 0;
        ResizeJob J{ H.width, H.height, ow[(size_t)i], oh[(size_t)i], H.ncomp, 0 };
        return H.blocks * (128 + 64) + align4((long long)H.width * H.height * H.ncomp) + (resize ? resize_scratch(J) : 0);
    };
    for (int i0 = 0; i0 < n_images;) {
        int i1 = i0 + 1;
        long long budget = scratch_of(i0);
        while (i1 < n_images && i1 - i0 < group_items && budget + scratch_of(i1) <= group_bytes) budget += scratch_of(i1++);
        std::vector<int> member;                                 // the decodable images of the group
        for (int i = i0; i < i1; ++i) if (hdr[(size_t)i].status == JPEG_OK) member.push_back(i);
        i0 = i1;
        if (member.empty()) continue;
        ++n_groups;

        std::vector<JpegPlane> planes;
        std::vector<JpegImage> images(member.size());
        std::vector<unsigned short> quant;
        std::vector<ResizeJob> jobs(member.size());
        std::vector<long long> coef_off(member.size());
        long long n_coef = 0, n_plane = 0, n_out = 0, max_blocks = 0, max_px = 0;
        for (size_t g = 0; g < member.size(); ++g) {
            const JpegHeader& H = hdr[(size_t)member[g]];
            JpegImage& I = images[g];
            std::memset(&I, 0, sizeof(I));
            coef_off[g] = n_coef;
            for (int c = 0; c < H.ncomp; ++c) {
                const JpegComponent& C = H.comp[c];
                JpegPlane P;
                P.coef = n_coef + C.block0 * 64;
                P.plane = n_plane;
                P.blocks = (long long)C.bw * C.bh;
                P.bw = C.bw;
                P.quant = (int)quant.size();
                quant.insert(quant.end(), H.quant[C.tq], H.quant[C.tq] + 64);
                planes.push_back(P);
                I.plane[c] = n_plane;
                I.stride[c] = C.bw * 8;
                n_plane += P.blocks * 64;
                max_blocks = std::max(max_blocks, P.blocks);
            }
            n_coef += H.blocks * 64;
            I.w = H.width; I.h = H.height; I.ncomp = H.ncomp;
            I.mode = H.hmax == 1 ? 0 : H.vmax == 1 ? 1 : 2;
            I.cw = H.comp[H.ncomp - 1].cw; I.ch = H.comp[H.ncomp - 1].ch;
            I.out = n_out;
            jobs[g] = ResizeJob{ H.width, H.height, ow[(size_t)member[g]], oh[(size_t)member[g]], H.ncomp, n_out };
            n_out += align4((long long)H.width * H.height * H.ncomp);
            max_px = std::max(max_px, (long long)H.width * H.height);
        }

        DeviceArena scratch(device);
        JpegPlane* d_planes_tab;
        JpegImage* d_images;
        unsigned short* d_quant;
        int16_t* d_coef;
        unsigned char *d_planes, *d_full;
        UNIT_DRAIN_ALLOC(scratch, d_planes_tab, JpegPlane, planes.size());
        UNIT_DRAIN_ALLOC(scratch, d_images, JpegImage, images.size());
        UNIT_DRAIN_ALLOC(scratch, d_quant, unsigned short, quant.size());
        UNIT_DRAIN_ALLOC(scratch, d_coef, int16_t, (size_t)n_coef);
        UNIT_DRAIN_ALLOC(scratch, d_planes, unsigned char, (size_t)n_plane);
        UNIT_DRAIN_ALLOC(scratch, d_full, unsigned char, (size_t)n_out);
        tm.begin(JPEG_T_UPLOAD);
        UNIT_DRAIN_TRY(hipMemcpyAsync(d_planes_tab, planes.data(), sizeof(JpegPlane) * planes.size(), hipMemcpyHostToDevice, s));
        UNIT_DRAIN_TRY(hipMemcpyAsync(d_images, images.data(), sizeof(JpegImage) * images.size(), hipMemcpyHostToDevice, s));
        UNIT_DRAIN_TRY(hipMemcpyAsync(d_quant, quant.data(), sizeof(unsigned short) * quant.size(), hipMemcpyHostToDevice, s));
        for (size_t g = 0; g < member.size(); ++g) {
            const std::vector<int16_t>& c = coef[(size_t)member[g]];
            UNIT_DRAIN_TRY(hipMemcpyAsync(d_coef + coef_off[g], c.data(), sizeof(int16_t) * c.size(), hipMemcpyHostToDevice, s));
        }
        tm.end();
        tm.begin(JPEG_T_IDCT);
        hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)((max_blocks + BLOCKS_PER_GROUP - 1) / BLOCKS_PER_GROUP), (unsigned)planes.size()), dim3(LANES), 0, s,
                           d_planes_tab, d_coef, d_quant, d_planes);
        UNIT_DRAIN_TRY(hipGetLastError());
        tm.end();
        tm.begin(JPEG_T_COLOUR);
        hipLaunchKernelGGL(k_jpeg_colour, dim3(grid_quads(max_px), (unsigned)images.size()), dim3(LANES), 0, s, d_images, d_planes, d_full);
        UNIT_DRAIN_TRY(hipGetLastError());
        tm.end();
        const unsigned char* d_result = d_full;
        std::vector<long long> result_off(member.size());
        for (size_t g = 0; g < member.size(); ++g) result_off[g] = images[g].out;
        if (resize) {
            unsigned char* d_small = nullptr;
            const int rc = launch_resize(s, scratch, tm, jobs, factor, d_full, &d_small, result_off);
            if (rc) return rc;
            d_result = d_small;
        }
        tm.begin(JPEG_T_DOWNLOAD);
        for (size_t g = 0; g < member.size(); ++g) {
            const int i = member[g];
            UNIT_DRAIN_TRY(hipMemcpyAsync(out + out_ptr[i], d_result + result_off[g], (size_t)(out_ptr[i + 1] - out_ptr[i]), hipMemcpyDeviceToHost, s));
        }
        tm.end();
        UNIT_DRAIN_TRY(hipStreamSynchronize(s));                     // the host tables and the group's arena go away below
    }
    if (timing) {
        tm.collect(timing);
        timing[JPEG_T_GROUPS] = n_groups;
    }
    return 0;
}

int resize_images(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* px, const int32_t* width,
                  const int32_t* height, int channels, float factor, int64_t* out_ptr, unsigned char* out, int64_t cap, int64_t* total,
                  double* timing) {
    if (timing) for (int i = 0; i < JPEG_T_COUNT; ++i) timing[i] = 0.0;
    std::vector<int64_t> optr((size_t)n_images + 1, 0);
    std::vector<ResizeJob> all((size_t)n_images);
    for (int i = 0; i < n_images; ++i) {
        ResizeJob& J = all[(size_t)i];
        J = ResizeJob{ width[i], height[i], resized_length(width[i], factor), resized_length(height[i], factor), channels, 0 };
        if (J.ow == 0 || J.oh == 0) return UNIT_ERR_SIZE;                       // before the first write
        optr[(size_t)i + 1] = optr[(size_t)i] + (int64_t)J.ow * J.oh * channels;
    }
    for (int i = 0; i <= n_images; ++i) out_ptr[i] = optr[(size_t)i];
    *total = out_ptr[n_images];
    if (*total > cap) return UNIT_ERR_CAPACITY;

    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    const long long group_bytes = group_bytes_limit(JPEG_SCRATCH_BYTES);
    const int group_items = group_items_limit(JPEG_MAX_GROUP_IMAGES);
    int n_groups = 0;
    auto scratch_of = [&](int i) { return align4((long long)width[i] * height[i] * channels) + resize_scratch(all[(size_t)i]); };
    for (int i0 = 0; i0 < n_images;) {
        int i1 = i0 + 1;
        long long budget = scratch_of(i0);
        while (i1 < n_images && i1 - i0 < group_items && budget + scratch_of(i1) <= group_bytes) budget += scratch_of(i1++);
        ++n_groups;
        std::vector<ResizeJob> jobs(all.begin() + i0, all.begin() + i1);
        long long n_src = 0;
        for (ResizeJob& J : jobs) { J.src = n_src; n_src += align4((long long)J.w * J.h * channels); }
        DeviceArena scratch(device);
        unsigned char *d_src, *d_dst = nullptr;
        UNIT_DRAIN_ALLOC(scratch, d_src, unsigned char, (size_t)n_src);
        tm.begin(JPEG_T_UPLOAD);
        for (int i = i0; i < i1; ++i)
            UNIT_DRAIN_TRY(hipMemcpyAsync(d_src + jobs[(size_t)(i - i0)].src, px + img_ptr[i], (size_t)(img_ptr[i + 1] - img_ptr[i]), hipMemcpyHostToDevice, s));
        tm.end();
        std::vector<long long> dst_off;
        const int rc = launch_resize(s, scratch, tm, jobs, factor, d_src, &d_dst, dst_off);
        if (rc) return rc;
        tm.begin(JPEG_T_DOWNLOAD);
        for (int i = i0; i < i1; ++i)
            UNIT_DRAIN_TRY(hipMemcpyAsync(out + out_ptr[i], d_dst + dst_off[(size_t)(i - i0)], (size_t)(out_ptr[i + 1] - out_ptr[i]), hipMemcpyDeviceToHost, s));
        tm.end();
        UNIT_DRAIN_TRY(hipStreamSynchronize(s));
        i0 = i1;
    }
    if (timing) {
        tm.collect(timing);
        timing[JPEG_T_GROUPS] = n_groups;
    }
    return 0;
}

}  // namespace sfmba
