// jpeg_entropy.h -- the host half of sfmba_jpeg_decode: header parse and Huffman decode of baseline JPEG files (jpeg_entropy.cpp).
//
// Plain C++ with no HIP include, so g++ builds it alone (the sanitizer program host/jpeg_sanitize.cpp does).  Entropy decoding is
// serial inside a restart interval and stays on the host; the device (jpeg_decode.hip) receives int16 coefficients, quantisation
// tables and geometry, never file bytes, and sizes every array from the validated fields of JpegHeader.
//
// Accepted: SOF0, 8-bit samples, 8-bit quantisation tables, Huffman coding, one component or three in one interleaved scan with
// luma 1x1 / 2x1 / 2x2 and chroma 1x1, any restart interval, width and height 1..16384; APPn and COM are skipped.  Anything else
// that is well-formed is JPEG_UNSUPPORTED; a file that breaks its own syntax is JPEG_CORRUPT.  No input makes these functions
// read outside [data, data + n) or write outside the arrays they are given.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sfmba {

enum { JPEG_OK = 0, JPEG_UNSUPPORTED = 1, JPEG_CORRUPT = 2 };       // = SFMBA_IMAGE_* of include/sfmba.h

struct JpegComponent {
    int id, h, v, tq;           // as in the frame header (h = v = 1 for a single component: its scan is not interleaved)
    int td, ta;                 // Huffman tables of the scan
    int cw, ch;                 // samples: ceil(width h / hmax) x ceil(height v / vmax)
    int bw, bh;                 // 8 x 8 blocks per row and per column of the stored plane (MCU padding included)
    long long block0;           // first block of the component in the image's coefficient array
};

struct JpegHuffman {
    bool defined;
    unsigned char bits[17];     // bits[l] = codes of length l
    unsigned char vals[256];
    int mincode[17], maxcode[18], valptr[17];
    unsigned short fast[512];   // 9 leading bits -> (length << 8) | symbol, 0 when the code is longer
};

struct JpegHeader {
    int status;
    int width, height, ncomp;
    int hmax, vmax;
    int mcus_x, mcus_y;
    int restart_interval;
    JpegComponent comp[3];
    bool have_quant[4];
    unsigned short quant[4][64];    // natural (row-major) order
    JpegHuffman huff[2][4];         // [0] DC, [1] AC
    size_t scan;                    // first byte of the entropy-coded segment
    long long blocks;               // of all components
};

// Everything up to the entropy-coded segment.  Returns the status, which is also h->status; the geometry fields are meaningful
// only with JPEG_OK.  A block takes at least 2 bits of scan data (a DC code and an end-of-block code), so a frame that declares more
// than 4 blocks per remaining byte is JPEG_CORRUPT here already: no caller sizes an array from a frame its file cannot hold.
int jpeg_parse_header(const unsigned char* data, size_t n, JpegHeader* h);

// The scan of a header that parsed JPEG_OK: coef receives h.blocks * 64 coefficients in natural order, block b of component c at
// (c.block0 + b) * 64 with b = block_row * c.bw + block_column (blocks of the padding that no MCU codes stay zero).
// Returns JPEG_OK or JPEG_CORRUPT.
int jpeg_decode_scan(const unsigned char* data, size_t n, const JpegHeader& h, int16_t* coef);

// The headers of every file of a batch (serial: a header is a few hundred bytes).
void jpeg_parse_batch(int n_images, const int64_t* file_ptr, const unsigned char* bytes, std::vector<JpegHeader>& headers);

// The scans of the files whose header parsed JPEG_OK, with at most min(n_images, max_threads, 16) threads, one image each.
// coef[i] is filled and headers[i].status updated (coef[i] stays empty unless the status ends as JPEG_OK).  Returns false when
// the host could not allocate a coefficient array; no exception leaves a worker thread.
bool jpeg_scan_batch(int n_images, const int64_t* file_ptr, const unsigned char* bytes, int max_threads, std::vector<JpegHeader>& headers,
                     std::vector<std::vector<int16_t> >& coef);

}  // namespace sfmba
