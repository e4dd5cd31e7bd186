// png_decode.hip -- sfmba_png_decode for a whole list of PNG files on the MI355X (gfx950).
//
// Reference: SfM::setImagesDirectory (SfMToyLib/SfM.cpp:98-139) promises jpg and png and reads them with imread, serially.  The
// contract here is the project's own, integer-exact one (include/sfmba.h; arithmetic in png_math.h), and the device is held BIT FOR
// BIT to a CPU restatement (tests/png_oracle.py).
//
// The host half (png_inflate.cpp) walks the chunks and inflates every file with at most 16 threads; the device never sees file
// bytes, and every device array is sized from validated header fields.  Images are taken in consecutive groups bounded by
// JPEG_SCRATCH_BYTES; every launch covers all images of the group:
//
//   unfilter  k_png_unfilter, ONE WAVE PER IMAGE, in place on the inflated stream.  A byte depends on its left, upper and upper-left
//             neighbours, and Paeth and Average are not associative, so the parallelism is the anti-diagonal wavefront: lane r owns
//             row r of a band of 64 rows and runs one pixel (bpp bytes, carried in one or two dwords) behind lane r - 1.  In a step
//             a lane takes the pixel lane r - 1 finished in the step before (= b) through one __shfl_up per dword, keeps the b of
//             its own previous step as c and its own previous result as a, and evaluates the predictor of its row's filter byte as
//             selects (png_predict).  The filtered bytes do not depend on the recurrence: they are staged through LDS in skewed
//             tiles of 64 rows x 64 pixels (row r of a tile starts r pixels to the left, so that in step j every lane reads
//             column j of its own row; rows are 64 W + 1 words apart, W = words per pixel: no bank conflict), loaded and written
//             back with consecutive lanes on consecutive bytes of a row.  Lane 0 of a band reads b from the last row of the band
//             before, which the same wave has written to global memory (a 65th tile row; zeros for band 0).  Bands of an image
//             run one after another in the same wave: a wave only ever depends on itself, and nothing waits on a flag.
//   pixels    k_png_pixels, grid.y = image: one lane per output pixel -- bit unpacking, gray scaling, the palette (in LDS), the high
//             byte of a 16-bit sample, alpha dropped, B, G, R order -- into the tight pixel array that k_resize reads.
//   resize    launch_resize of jpeg_decode.hip: the same kernel and tables as the JPEG path.
//
// No atomics anywhere: every output byte has one writer.
#include "png_decode.h"
#include "png_math.h"
#include "jpeg_math.h"
#include "device_arena.h"

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sfmba {

namespace {

constexpr int WAVE = 64;
constexpr int TILE = 64;                          // pixels per tile row
constexpr int TILE_WORDS = (WAVE + 1) * (TILE * 2 + 1);       // the widest form: two words per pixel
constexpr int PIXEL_LANES = 256;
constexpr int STAGE_ROWS = 8;                    // rows whose loads are in flight together while a tile is staged

// One image of the group.
struct PngImage {
    long long stream;           // first byte of its scanline stream in the group's stream region
    long long out;              // first byte of its pixels in the decoded region (a multiple of 4)
    int rowbytes;
    int w, h;
    int colour_type, depth, bpp;
    int palette;                // its table of 256 x (R, G, B) in the group's palette array
};

template <int BPP> __device__ __forceinline__ void unfilter_image(const PngImage& T, unsigned char* __restrict__ streams, unsigned* tile) {
    constexpr int W = (BPP + 3) / 4;                          // words per pixel
    constexpr int STRIDE = TILE * W + 1;                      // words per tile row: odd, so 64 lanes on one column hit 64 banks
    const int lane = (int)threadIdx.x;
    unsigned char* const base = streams + T.stream;
    const size_t stride = (size_t)T.rowbytes + 1;
    const int npix = T.rowbytes / BPP;
    unsigned char* const tb = reinterpret_cast<unsigned char*>(tile);
    unsigned a[W], c[W];
#pragma unroll
    for (int w = 0; w < W; ++w) { a[w] = 0u; c[w] = 0u; }
    for (int y0 = 0; y0 < T.h; y0 += WAVE) {
        const int rows = min(WAVE, T.h - y0);
        const bool live = lane < rows;
        const int ft = live ? (int)base[(size_t)(y0 + lane) * stride] : 0;
        const int steps = npix + rows - 1;
        for (int s0 = 0; s0 < steps; s0 += TILE) {
            // stage the filtered bytes: row r of the tile holds pixels s0 - r .. s0 - r + TILE - 1 of row y0 + r.  STAGE_ROWS rows at a
            // time: every load goes to a clamped, always valid address and none sits under a branch, so that all of them are in
            // flight together; what lies outside the row is dropped at the LDS write
            for (int r0 = 0; r0 < rows; r0 += STAGE_ROWS) {
                unsigned char v[STAGE_ROWS][BPP];
#pragma unroll
                for (int i = 0; i < STAGE_ROWS; ++i) {
                    const int r = min(r0 + i, rows - 1);
                    const unsigned char* g = base + (size_t)(y0 + r) * stride + 1;
#pragma unroll
                    for (int q = 0; q < BPP; ++q) {
                        const int e = lane + q * WAVE, j = e / BPP, k = e - j * BPP, p = min(max(s0 - r + j, 0), npix - 1);
                        v[i][q] = g[(size_t)p * BPP + k];
                    }
                }
#pragma unroll
                for (int i = 0; i < STAGE_ROWS; ++i) {
                    const int r = r0 + i;
#pragma unroll
                    for (int q = 0; q < BPP; ++q) {
                        const int e = lane + q * WAVE, j = e / BPP, k = e - j * BPP, p = s0 - r + j;
                        if (r < rows && p >= 0 && p < npix) tb[(r * STRIDE + j * W) * 4 + k] = v[i][q];
                    }
                }
            }
            // row 64 of the tile: pixels s0 .. s0 + TILE - 1 of the last row of the band before (reconstructed), zeros for band 0
            for (int e = lane; e < TILE * BPP; e += WAVE) {
                const int j = e / BPP, k = e - j * BPP, p = s0 + j;
                tb[(WAVE * STRIDE + j * W) * 4 + k] = (y0 > 0 && p < npix) ? base[(size_t)(y0 - 1) * stride + 1 + (size_t)p * BPP + k] : (unsigned char)0;
            }
            __syncthreads();
            // the wavefront: in step s0 + j lane r works pixel s0 + j - r
            unsigned xn[W];                                                 // the filtered pixel of the next step, read one step ahead
#pragma unroll
            for (int w = 0; w < W; ++w) xn[w] = tile[lane * STRIDE + w];
            for (int j = 0; j < TILE; ++j) {
                const int p = s0 + j - lane;
                unsigned x[W], b[W], res[W];
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    x[w] = xn[w];
                    b[w] = (unsigned)__shfl_up((int)a[w], 1);              // what lane r - 1 finished in the step before: the pixel above
                    xn[w] = tile[lane * STRIDE + min(j + 1, TILE - 1) * W + w];
                }
                if (lane == 0) {
#pragma unroll
                    for (int w = 0; w < W; ++w) b[w] = tile[WAVE * STRIDE + j * W + w];
                }
                if (p <= 0) {                                               // the first pixel of a row has nothing to its left
#pragma unroll
                    for (int w = 0; w < W; ++w) { a[w] = 0u; c[w] = 0u; }
                }
                png_unfilter_pixel<BPP>(ft, x, a, b, c, res);
#pragma unroll
                for (int w = 0; w < W; ++w) { c[w] = b[w]; a[w] = res[w]; }
                if (live && p >= 0 && p < npix) {
#pragma unroll
                    for (int w = 0; w < W; ++w) tile[lane * STRIDE + j * W + w] = res[w];
                }
            }
            __syncthreads();
            // the reconstructed bytes go back where the filtered ones came from
            for (int r0 = 0; r0 < rows; r0 += STAGE_ROWS) {
                unsigned char v[STAGE_ROWS][BPP];
#pragma unroll
                for (int i = 0; i < STAGE_ROWS; ++i) {
                    const int r = min(r0 + i, rows - 1);
#pragma unroll
                    for (int q = 0; q < BPP; ++q) {
                        const int e = lane + q * WAVE, j = e / BPP, k = e - j * BPP;
                        v[i][q] = tb[(r * STRIDE + j * W) * 4 + k];
                    }
                }
#pragma unroll
                for (int i = 0; i < STAGE_ROWS; ++i) {
                    const int r = r0 + i;
                    unsigned char* g = base + (size_t)(y0 + min(r, rows - 1)) * stride + 1;
#pragma unroll
                    for (int q = 0; q < BPP; ++q) {
                        const int e = lane + q * WAVE, j = e / BPP, k = e - j * BPP, p = s0 - r + j;
                        if (r < rows && p >= 0 && p < npix) g[(size_t)p * BPP + k] = v[i][q];
                    }
                }
            }
            __syncthreads();                                                // the stores above are read again as the next band's row above
        }
    }
}

// grid.x = image, one wave each.
__global__ __launch_bounds__(WAVE) void k_png_unfilter(const PngImage* __restrict__ tab, unsigned char* __restrict__ streams) {
    __shared__ unsigned tile[TILE_WORDS];
    const PngImage T = tab[blockIdx.x];
    switch (T.bpp) {                                                        // the same in every lane
        case 1: unfilter_image<1>(T, streams, tile); break;
        case 2: unfilter_image<2>(T, streams, tile); break;
        case 3: unfilter_image<3>(T, streams, tile); break;
        case 4: unfilter_image<4>(T, streams, tile); break;
        case 6: unfilter_image<6>(T, streams, tile); break;
        case 8: unfilter_image<8>(T, streams, tile); break;
        default: break;
    }
}

__global__ __launch_bounds__(PIXEL_LANES) void k_png_pixels(const PngImage* __restrict__ tab, const unsigned char* __restrict__ streams,
                                                            const unsigned char* __restrict__ palettes, unsigned char* __restrict__ dst) {
    __shared__ unsigned char pal[768];
    const PngImage T = tab[blockIdx.y];
    // 32-bit throughout: an image has at most 16384 x 16384 pixels, and the grid overshoots that by less than one block
    const unsigned n = (unsigned)T.w * (unsigned)T.h;
    if (blockIdx.x * (unsigned)PIXEL_LANES >= n) return;                    // the whole block leaves: no barrier is skipped
    if (T.colour_type == 3)
        for (int i = (int)threadIdx.x; i < 768; i += PIXEL_LANES) pal[i] = palettes[(size_t)T.palette * 768 + i];
    __syncthreads();
    const unsigned q = blockIdx.x * (unsigned)PIXEL_LANES + threadIdx.x;
    if (q >= n) return;
    const int y = (int)(q / (unsigned)T.w), x = (int)(q - (unsigned)y * (unsigned)T.w);
    const unsigned char* row = streams + T.stream + (size_t)y * ((size_t)T.rowbytes + 1) + 1;
    int px[3];
    png_pixel(row, x, T.colour_type, T.depth, pal, px);
    if (png_out_channels(T.colour_type) == 1) {
        dst[T.out + q] = (unsigned char)px[0];
    } else {
        unsigned char* o = dst + T.out + 3 * (size_t)q;
        o[0] = (unsigned char)px[0]; o[1] = (unsigned char)px[1]; o[2] = (unsigned char)px[2];
    }
}

long long align4(long long n) { return (n + 3) & ~3ll; }
double now_ms() { return 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

void png_fill_info(const PngHeader& h, struct sfmba_png_info* info) {
    std::memset(info, 0, sizeof(*info));
    info->status = h.status;
    if (h.status != PNG_OK) return;
    info->width = h.width; info->height = h.height; info->channels = h.channels;
    info->bit_depth = h.bit_depth; info->colour_type = h.colour_type; info->interlace = h.interlace;
}

int png_decode(hipStream_t s, int device, int n_images, const int64_t* file_ptr, const unsigned char* bytes, float factor,
               struct sfmba_png_info* info, int64_t* out_ptr, unsigned char* out, int64_t cap, int64_t* total, double* timing) {
    if (timing) for (int i = 0; i < PNG_T_COUNT; ++i) timing[i] = 0.0;
    const double t0 = timing ? now_ms() : 0.0;
    std::vector<PngHeader> hdr;
    std::vector<std::vector<unsigned char> > streams;
    png_parse_batch(n_images, file_ptr, bytes, hdr);
    // the sizes come from IHDR alone: a refused factor is refused here, before the first write and before anything is inflated
    const bool resize = factor != 1.0f;
    std::vector<int> ow((size_t)n_images, 0), oh((size_t)n_images, 0);
    for (int i = 0; i < n_images; ++i) {
        const PngHeader& H = hdr[(size_t)i];
        if (H.status != PNG_OK) continue;
        ow[(size_t)i] = resize ? resized_length(H.width, factor) : H.width;
        oh[(size_t)i] = resize ? resized_length(H.height, factor) : H.height;
        if (ow[(size_t)i] == 0 || oh[(size_t)i] == 0) return UNIT_ERR_SIZE;
    }
    if (!png_inflate_batch(n_images, file_ptr, bytes, 16, hdr, streams)) return UNIT_ERR_HOST_ALLOC;
    if (timing) timing[PNG_T_INFLATE] = now_ms() - t0;

    out_ptr[0] = 0;
    for (int i = 0; i < n_images; ++i) {
        const PngHeader& H = hdr[(size_t)i];
        png_fill_info(H, &info[i]);
        out_ptr[i + 1] = out_ptr[i] + (H.status == PNG_OK ? (long long)ow[(size_t)i] * oh[(size_t)i] * H.channels : 0);
    }
    *total = out_ptr[n_images];
    if (*total > cap) return UNIT_ERR_CAPACITY;

    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    const long long group_bytes = group_bytes_limit(JPEG_SCRATCH_BYTES);
    const int group_items = group_items_limit(JPEG_MAX_GROUP_IMAGES);
    int n_groups = 0;
    auto scratch_of = [&](int i) -> long long {
        const PngHeader& H = hdr[(size_t)i];
        if (H.status != PNG_OK) return 0;
        ResizeJob J{ H.width, H.height, ow[(size_t)i], oh[(size_t)i], H.channels, 0 };
        return align4(H.stream_bytes) + 768 + align4((long long)H.width * H.height * H.channels) + (resize ? resize_scratch(J) : 0);
    };
    for (int i0 = 0; i0 < n_images;) {
        int i1 = i0 + 1;
        long long budget = scratch_of(i0);
        while (i1 < n_images && i1 - i0 < group_items && budget + scratch_of(i1) <= group_bytes) budget += scratch_of(i1++);
        std::vector<int> member;                                 // the decodable images of the group
        for (int i = i0; i < i1; ++i) if (hdr[(size_t)i].status == PNG_OK) member.push_back(i);
        i0 = i1;
        if (member.empty()) continue;
        ++n_groups;

        std::vector<PngImage> images(member.size());
        std::vector<unsigned char> palettes(768 * member.size());
        std::vector<ResizeJob> jobs(member.size());
        long long n_stream = 0, n_out = 0, max_px = 0;
        for (size_t g = 0; g < member.size(); ++g) {
            const PngHeader& H = hdr[(size_t)member[g]];
            PngImage& I = images[g];
            std::memset(&I, 0, sizeof(I));
            I.stream = n_stream; I.out = n_out;
            I.rowbytes = (int)H.rowbytes; I.w = H.width; I.h = H.height;
            I.colour_type = H.colour_type; I.depth = H.bit_depth; I.bpp = H.bpp;
            I.palette = (int)g;
            std::memcpy(&palettes[768 * g], H.palette, 768);
            jobs[g] = ResizeJob{ H.width, H.height, ow[(size_t)member[g]], oh[(size_t)member[g]], H.channels, n_out };
            n_stream += align4(H.stream_bytes);
            n_out += align4((long long)H.width * H.height * H.channels);
            max_px = std::max(max_px, (long long)H.width * H.height);
        }

        DeviceArena scratch(device);
        PngImage* d_images;
        unsigned char *d_palettes, *d_streams, *d_full;
        UNIT_DRAIN_ALLOC(scratch, d_images, PngImage, images.size());
        UNIT_DRAIN_ALLOC(scratch, d_palettes, unsigned char, palettes.size());
        UNIT_DRAIN_ALLOC(scratch, d_streams, unsigned char, (size_t)n_stream);
        UNIT_DRAIN_ALLOC(scratch, d_full, unsigned char, (size_t)n_out);
        tm.begin(PNG_T_UPLOAD);
        UNIT_DRAIN_TRY(hipMemcpyAsync(d_images, images.data(), sizeof(PngImage) * images.size(), hipMemcpyHostToDevice, s));
        UNIT_DRAIN_TRY(hipMemcpyAsync(d_palettes, palettes.data(), palettes.size(), hipMemcpyHostToDevice, s));
        for (size_t g = 0; g < member.size(); ++g) {
            const std::vector<unsigned char>& st = streams[(size_t)member[g]];
            UNIT_DRAIN_TRY(hipMemcpyAsync(d_streams + images[g].stream, st.data(), st.size(), hipMemcpyHostToDevice, s));
        }
        tm.end();
        tm.begin(PNG_T_UNFILTER);
        hipLaunchKernelGGL(k_png_unfilter, dim3((unsigned)images.size()), dim3(WAVE), 0, s, d_images, d_streams);
        UNIT_DRAIN_TRY(hipGetLastError());
        tm.end();
        tm.begin(PNG_T_PIXELS);
        hipLaunchKernelGGL(k_png_pixels, dim3((unsigned)((max_px + PIXEL_LANES - 1) / PIXEL_LANES), (unsigned)images.size()), dim3(PIXEL_LANES), 0, s,
                           d_images, d_streams, d_palettes, d_full);
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
        tm.begin(PNG_T_DOWNLOAD);
        for (size_t g = 0; g < member.size(); ++g) {
            const int i = member[g];
            UNIT_DRAIN_TRY(hipMemcpyAsync(out + out_ptr[i], d_result + result_off[g], (size_t)(out_ptr[i + 1] - out_ptr[i]), hipMemcpyDeviceToHost, s));
        }
        tm.end();
        UNIT_DRAIN_TRY(hipStreamSynchronize(s));                      // the host tables and the group's arena go away below
    }
    if (timing) {
        tm.collect(timing);
        timing[PNG_T_GROUPS] = n_groups;
    }
    return 0;
}

}  // namespace sfmba
