// jpeg_entropy.cpp -- see jpeg_entropy.h: header parse and Huffman decode of baseline JPEG files on the host.
#include "jpeg_entropy.h"
#include "host_pool.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>

namespace sfmba {

namespace {

const unsigned char ZIGZAG[64] = { 0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };
const int MAX_SIDE = 16384;

// The canonical code of (bits, vals); false when the counts do not form a prefix code.
bool build_huffman(JpegHuffman& t) {
    int code = 0, k = 0;
    std::memset(t.fast, 0, sizeof(t.fast));
    for (int l = 1; l <= 16; ++l) {
        t.valptr[l] = k;
        t.mincode[l] = code;
        for (int i = 0; i < t.bits[l]; ++i, ++k, ++code) {
            if (l <= 9) {
                const int first = code << (9 - l), count = 1 << (9 - l);
                if (first + count > 512) return false;
                for (int j = 0; j < count; ++j) t.fast[first + j] = (unsigned short)((l << 8) | t.vals[k]);
            }
        }
        if (code > (1 << l)) return false;
        t.maxcode[l] = t.bits[l] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.defined = true;
    return true;
}

unsigned be16(const unsigned char* p) { return ((unsigned)p[0] << 8) | p[1]; }

// The bits of the entropy-coded segment: 0xFF 0x00 gives a 0xFF byte, any other marker (or the end of the file) ends the supply.
// Beyond the end zero bits are handed out for the look-ahead only: consuming one of them sets `overrun`.
struct BitReader {
    const unsigned char* data;
    size_t n, pos;
    uint64_t acc;
    int nbits, npad;
    bool overrun;
    void fill() {
        while (nbits <= 56) {
            if (npad == 0 && pos < n && !(data[pos] == 0xFF && (pos + 1 >= n || data[pos + 1] != 0x00))) {
                acc = (acc << 8) | data[pos];
                pos += data[pos] == 0xFF ? 2 : 1;
            } else {
                acc <<= 8;
                npad += 8;
            }
            nbits += 8;
        }
    }
    unsigned peek(int k) { if (nbits < k) fill(); return (unsigned)((acc >> (nbits - k)) & ((1u << k) - 1u)); }
    void skip(int k) { nbits -= k; if (nbits < npad) overrun = true; }
    unsigned get(int k) { if (k == 0) return 0; const unsigned v = peek(k); skip(k); return v; }
    void restart() { acc = 0; nbits = 0; npad = 0; }
};

// the next Huffman symbol, -1 when the bits match no code
int decode_symbol(BitReader& br, const JpegHuffman& t) {
    const unsigned look = br.peek(16);
    const unsigned short f = t.fast[look >> 7];
    if (f) { br.skip(f >> 8); return f & 0xff; }
    for (int l = 10; l <= 16; ++l) {
        const int code = (int)(look >> (16 - l));
        if (code <= t.maxcode[l] && t.maxcode[l] >= 0 && code >= t.mincode[l]) {
            br.skip(l);
            return t.vals[t.valptr[l] + code - t.mincode[l]];
        }
    }
    return -1;
}

int extend(unsigned v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

bool decode_block(BitReader& br, const JpegHuffman& dc, const JpegHuffman& ac, int& pred, int16_t* block) {
    const int s = decode_symbol(br, dc);
    if (s < 0 || s > 11) return false;
    if (s) pred += extend(br.get(s), s);
    if (pred < -32768 || pred > 32767) return false;
    block[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        const int rs = decode_symbol(br, ac);
        if (rs < 0) return false;
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            if (r != 15) break;              // end of block
            k += 16;
            if (k > 64) return false;
            continue;
        }
        k += r;
        if (k > 63) return false;            // a coefficient index past 63
        block[ZIGZAG[k++]] = (int16_t)extend(br.get(sz), sz);
    }
    return !br.overrun;
}

int fail(JpegHeader* h, int status) { h->status = status; return status; }

}  // namespace

int jpeg_parse_header(const unsigned char* data, size_t n, JpegHeader* h) {
    h->status = JPEG_CORRUPT;
    h->width = h->height = h->ncomp = 0;
    h->hmax = h->vmax = 1;
    h->mcus_x = h->mcus_y = 0;
    h->restart_interval = 0;
    h->scan = 0;
    h->blocks = 0;
    std::memset(h->comp, 0, sizeof(h->comp));
    for (int i = 0; i < 4; ++i) {
        h->have_quant[i] = false;
        h->huff[0][i].defined = h->huff[1][i].defined = false;
    }
    if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) return fail(h, JPEG_CORRUPT);
    size_t pos = 2;
    bool have_frame = false;
    for (;;) {
        if (pos >= n || data[pos] != 0xFF) return fail(h, JPEG_CORRUPT);
        while (pos < n && data[pos] == 0xFF) ++pos;                      // fill bytes
        if (pos >= n) return fail(h, JPEG_CORRUPT);
        const int m = data[pos++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return fail(h, JPEG_CORRUPT);      // no segment may stand here (D9: no scan)
        if (pos + 2 > n) return fail(h, JPEG_CORRUPT);
        const size_t len = be16(data + pos);
        if (len < 2 || pos + len > n) return fail(h, JPEG_CORRUPT);     // a segment that runs past the end of the file
        const unsigned char* p = data + pos + 2;
        const size_t body = len - 2;
        if (m == 0xC0) {
            if (have_frame || body < 6) return fail(h, JPEG_CORRUPT);
            const int precision = p[0], nc = p[5];
            h->height = (int)be16(p + 1);
            h->width = (int)be16(p + 3);
            if (body != 6 + 3 * (size_t)nc) return fail(h, JPEG_CORRUPT);
            if (h->width == 0 || h->height == 0 || nc == 0) return fail(h, JPEG_CORRUPT);
            if (precision != 8 || (nc != 1 && nc != 3) || h->width > MAX_SIDE || h->height > MAX_SIDE) return fail(h, JPEG_UNSUPPORTED);
            for (int c = 0; c < nc; ++c) {
                JpegComponent& C = h->comp[c];
                C.id = p[6 + 3 * c];
                C.h = p[7 + 3 * c] >> 4; C.v = p[7 + 3 * c] & 15;
                C.tq = p[8 + 3 * c];
                if (C.h < 1 || C.h > 4 || C.v < 1 || C.v > 4 || C.tq > 3) return fail(h, JPEG_CORRUPT);
                for (int d = 0; d < c; ++d) if (h->comp[d].id == C.id) return fail(h, JPEG_CORRUPT);
            }
            if (nc == 1) h->comp[0].h = h->comp[0].v = 1;
            else {
                const int lh = h->comp[0].h, lv = h->comp[0].v;
                const bool luma_ok = (lh == 1 && lv == 1) || (lh == 2 && lv == 1) || (lh == 2 && lv == 2);
                if (!luma_ok || h->comp[1].h != 1 || h->comp[1].v != 1 || h->comp[2].h != 1 || h->comp[2].v != 1) return fail(h, JPEG_UNSUPPORTED);
            }
            h->ncomp = nc;
            have_frame = true;
        } else if ((m >= 0xC1 && m <= 0xCF && m != 0xC4) || m == 0xDC || m == 0xDE || m == 0xDF) {
            return fail(h, JPEG_UNSUPPORTED);            // other frame types, arithmetic conditioning, DNL, hierarchical
        } else if (m == 0xDB) {
            size_t o = 0;
            while (o < body) {
                const int pq = p[o] >> 4, tq = p[o] & 15;
                if (tq > 3 || pq > 1) return fail(h, JPEG_CORRUPT);
                if (pq == 1) return fail(h, JPEG_UNSUPPORTED);                // 16-bit quantisation table
                if (o + 65 > body) return fail(h, JPEG_CORRUPT);
                for (int k = 0; k < 64; ++k) h->quant[tq][ZIGZAG[k]] = p[o + 1 + k];
                h->have_quant[tq] = true;
                o += 65;
            }
        } else if (m == 0xC4) {
            size_t o = 0;
            while (o < body) {
                const int tc = p[o] >> 4, th = p[o] & 15;
                if (tc > 1 || th > 3 || o + 17 > body) return fail(h, JPEG_CORRUPT);
                JpegHuffman& t = h->huff[tc][th];
                t.defined = false;
                int count = 0;
                t.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) { t.bits[l] = p[o + l]; count += t.bits[l]; }
                if (count > 256 || o + 17 + (size_t)count > body) return fail(h, JPEG_CORRUPT);
                std::memset(t.vals, 0, sizeof(t.vals));
                std::memcpy(t.vals, p + o + 17, (size_t)count);
                if (!build_huffman(t)) return fail(h, JPEG_CORRUPT);
                o += 17 + (size_t)count;
            }
        } else if (m == 0xDD) {
            if (body != 2) return fail(h, JPEG_CORRUPT);
            h->restart_interval = (int)be16(p);
        } else if (m == 0xDA) {
            if (!have_frame || body < 1) return fail(h, JPEG_CORRUPT);
            const int ns = p[0];
            if (ns < 1 || ns > 4 || body != 4 + 2 * (size_t)ns) return fail(h, JPEG_CORRUPT);
            if (ns != h->ncomp) return fail(h, JPEG_UNSUPPORTED);            // the frame is spread over several scans
            for (int c = 0; c < ns; ++c) {
                JpegComponent& C = h->comp[c];
                bool known = false;
                for (int d = 0; d < h->ncomp; ++d) known = known || h->comp[d].id == p[1 + 2 * c];
                if (!known) return fail(h, JPEG_CORRUPT);
                if (p[1 + 2 * c] != C.id) return fail(h, JPEG_UNSUPPORTED);   // components out of the frame's order
                C.td = p[2 + 2 * c] >> 4; C.ta = p[2 + 2 * c] & 15;
                if (C.td > 3 || C.ta > 3) return fail(h, JPEG_CORRUPT);
                if (!h->huff[0][C.td].defined || !h->huff[1][C.ta].defined || !h->have_quant[C.tq]) return fail(h, JPEG_CORRUPT);   // a missing table
            }
            const unsigned char* e = p + 1 + 2 * ns;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) return fail(h, JPEG_CORRUPT);    // spectral selection / approximation of a sequential scan
            h->scan = pos + len;
            break;
        }
        // APPn, COM and every other segment with a length: skipped
        pos += len;
    }
    h->hmax = h->comp[0].h; h->vmax = h->comp[0].v;
    h->mcus_x = (h->width + 8 * h->hmax - 1) / (8 * h->hmax);
    h->mcus_y = (h->height + 8 * h->vmax - 1) / (8 * h->vmax);
    long long blocks = 0;
    for (int c = 0; c < h->ncomp; ++c) {
        JpegComponent& C = h->comp[c];
        C.cw = (h->width * C.h + h->hmax - 1) / h->hmax;
        C.ch = (h->height * C.v + h->vmax - 1) / h->vmax;
        C.bw = h->mcus_x * C.h;
        C.bh = h->mcus_y * C.v;
        C.block0 = blocks;
        blocks += (long long)C.bw * C.bh;
    }
    h->blocks = blocks;
    if (blocks > 4 * (long long)(n - h->scan)) return fail(h, JPEG_CORRUPT);       // truncated: at least 2 bits per block
    h->status = JPEG_OK;
    return JPEG_OK;
}

int jpeg_decode_scan(const unsigned char* data, size_t n, const JpegHeader& h, int16_t* coef) {
    if (h.status != JPEG_OK || h.scan > n) return JPEG_CORRUPT;
    std::memset(coef, 0, sizeof(int16_t) * 64 * (size_t)h.blocks);
    BitReader br;
    br.data = data; br.n = n; br.pos = h.scan;
    br.overrun = false;
    br.restart();
    int pred[3] = { 0, 0, 0 };
    const long long mcus = (long long)h.mcus_x * h.mcus_y;
    int next_restart = 0;
    for (long long m = 0; m < mcus; ++m) {
        if (h.restart_interval > 0 && m > 0 && m % h.restart_interval == 0) {
            // the rest of the last byte is dropped; the marker RSTn must stand right here (fill bytes allowed before it)
            if (br.nbits - br.npad >= 8) return JPEG_CORRUPT;
            size_t p = br.pos;
            if (p >= n || data[p] != 0xFF) return JPEG_CORRUPT;
            while (p < n && data[p] == 0xFF) ++p;
            if (p >= n || data[p] != 0xD0 + next_restart) return JPEG_CORRUPT;
            br.pos = p + 1;
            br.restart();
            next_restart = (next_restart + 1) & 7;
            pred[0] = pred[1] = pred[2] = 0;
        }
        const int my = (int)(m / h.mcus_x), mx = (int)(m % h.mcus_x);
        for (int c = 0; c < h.ncomp; ++c) {
            const JpegComponent& C = h.comp[c];
            for (int v = 0; v < C.v; ++v)
                for (int u = 0; u < C.h; ++u) {
                    const long long b = C.block0 + (long long)(my * C.v + v) * C.bw + (mx * C.h + u);
                    if (!decode_block(br, h.huff[0][C.td], h.huff[1][C.ta], pred[c], coef + 64 * b)) return JPEG_CORRUPT;
                }
        }
    }
    return JPEG_OK;
}

void jpeg_parse_batch(int n_images, const int64_t* file_ptr, const unsigned char* bytes, std::vector<JpegHeader>& headers) {
    headers.resize((size_t)std::max(n_images, 0));
    for (int i = 0; i < n_images; ++i) jpeg_parse_header(bytes + file_ptr[i], (size_t)(file_ptr[i + 1] - file_ptr[i]), &headers[(size_t)i]);
}

bool jpeg_scan_batch(int n_images, const int64_t* file_ptr, const unsigned char* bytes, int max_threads, std::vector<JpegHeader>& headers,
                     std::vector<std::vector<int16_t> >& coef) {
    coef.assign((size_t)std::max(n_images, 0), std::vector<int16_t>());
    if (n_images <= 0) return true;
    std::atomic<bool> alloc_failed(false);
    host_pool_for(n_images, max_threads, [&](int i) {
        JpegHeader& h = headers[(size_t)i];
        if (h.status != JPEG_OK) return;
        std::vector<int16_t>& c = coef[(size_t)i];
        try {
            c.resize(64 * (size_t)h.blocks);
        } catch (const std::bad_alloc&) {                  // nothing may leave a worker thread
            alloc_failed = true;
            return;
        }
        h.status = jpeg_decode_scan(bytes + file_ptr[i], (size_t)(file_ptr[i + 1] - file_ptr[i]), h, c.data());
        if (h.status != JPEG_OK) std::vector<int16_t>().swap(c);
    });
    return !alloc_failed;
}

}  // namespace sfmba
