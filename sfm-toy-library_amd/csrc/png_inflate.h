// png_inflate.h -- the host half of sfmba_png_decode: chunk walk, CRC-32, the zlib wrapper and the project's own inflate
// (png_inflate.cpp).
//
// Plain C++ with no HIP include and no zlib / libpng, so g++ builds it alone (the sanitizer program host/png_sanitize.cpp does).
// Inflating is serial and stays on the host; the device (png_decode.hip) receives the inflated scanline stream (filter bytes
// included), the palette and the geometry, never file bytes, and sizes every array from the validated fields of PngHeader.
//
// The accepted scope and the split between PNG_UNSUPPORTED and PNG_CORRUPT are those of include/sfmba.h.  No input makes these
// functions read outside [data, data + n) or write outside the arrays they are given.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace sfmba {

enum { PNG_OK = 0, PNG_UNSUPPORTED = 1, PNG_CORRUPT = 2 };         // = SFMBA_IMAGE_* of include/sfmba.h
constexpr int PNG_MAX_SIDE = 16384;

struct PngHeader {
    int status;
    int width, height;
    int bit_depth, colour_type, interlace;
    int samples;                // per pixel in the file: 1, 2, 3 or 4
    int channels;               // of the OUTPUT: 1 (colour types 0 and 4) or 3
    int bpp;                    // max(1, samples * depth / 8): the distance of the filters' left neighbour in bytes
    long long rowbytes;         // ceil(width * samples * depth / 8)
    long long stream_bytes;     // height * (1 + rowbytes): what the IDAT chunks must inflate to, exactly
    long long idat_bytes;       // of all IDAT chunks together
    int n_palette;              // entries of PLTE (0 without one)
    unsigned char palette[768]; // R, G, B per entry; entries at and past n_palette are 0
    std::vector<std::pair<size_t, size_t> > idat;   // (first byte, length) of every IDAT chunk's data, in file order
};

// The chunk walk: signature, every chunk's length and CRC, IHDR, PLTE, the IDAT list, IEND.  Returns the status, which is also
// h->status; the geometry is meaningful only with PNG_OK.  An image whose stream_bytes exceeds 1032 * idat_bytes + 64 is
// PNG_CORRUPT here already (a deflate stream cannot expand further), so no caller sizes an array from an image its file cannot hold.
int png_parse(const unsigned char* data, size_t n, PngHeader* h);

// A bare deflate stream z[0 .. zn) into out[0 .. cap): true when the stream is valid, ends with a final block and wants no more
// than cap bytes.  *produced = bytes written, *used = bytes of z consumed (the last one possibly in part).
bool png_inflate_raw(const unsigned char* z, size_t zn, unsigned char* out, size_t cap, size_t* produced, size_t* used);

// The zlib stream z[0 .. zn) into out[0 .. expect): PNG_OK when the header is deflate with a window of at most 32 K and no preset
// dictionary, the stream is valid, inflates to exactly `expect` bytes and the Adler-32 that follows it agrees.
int png_inflate_zlib(const unsigned char* z, size_t zn, unsigned char* out, size_t expect);

// The scanline stream of a file whose walk ended PNG_OK: stream receives h.stream_bytes bytes.  PNG_CORRUPT also for a filter-type
// byte above 4.
int png_inflate_image(const unsigned char* data, size_t n, const PngHeader& h, unsigned char* stream);

uint32_t png_crc32(const unsigned char* p, size_t n, uint32_t crc = 0);
uint32_t png_adler32(const unsigned char* p, size_t n);

// The walks of every file of a batch (serial), and the streams of those that ended PNG_OK with at most min(n_images, max_threads,
// 16) threads, one image each: streams[i] is filled and headers[i].status updated (streams[i] stays empty unless the status ends
// as PNG_OK).  Returns false when the host could not allocate a stream; no exception leaves a worker thread.
void png_parse_batch(int n_images, const int64_t* file_ptr, const unsigned char* bytes, std::vector<PngHeader>& headers);
bool png_inflate_batch(int n_images, const int64_t* file_ptr, const unsigned char* bytes, int max_threads, std::vector<PngHeader>& headers,
                       std::vector<std::vector<unsigned char> >& streams);

}  // namespace sfmba
