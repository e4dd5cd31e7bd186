// png_inflate.cpp -- see png_inflate.h: chunk walk, CRC-32, zlib wrapper and inflate of PNG files on the host.
#include "png_inflate.h"
#include "host_pool.h"

#include <atomic>
#include <cstring>
#include <new>

namespace sfmba {

namespace {

// ---- checksums ----------------------------------------------------------------------------------------------------------------
struct CrcTables {
    uint32_t t[8][256];
    CrcTables() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (int s = 1; s < 8; ++s)
            for (uint32_t i = 0; i < 256; ++i) t[s][i] = t[0][t[s - 1][i] & 255u] ^ (t[s - 1][i] >> 8);
    }
};
const CrcTables& crc_tables() { static const CrcTables T; return T; }

uint32_t be32(const unsigned char* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }

// ---- the bit reader: least significant bit first, never past the end -----------------------------------------------------------
struct Bits {
    const unsigned char* p;
    size_t n, pos;
    uint64_t buf;
    int cnt;                    // valid bits of buf
    void fill() { while (cnt <= 56 && pos < n) { buf |= (uint64_t)p[pos++] << cnt; cnt += 8; } }
    unsigned peek(int k) { fill(); return (unsigned)(buf & ((1ull << k) - 1ull)); }      // k <= 16; zeros stand in for bits past the end
    bool drop(int k) { if (cnt < k) return false; buf >>= k; cnt -= k; return true; }    // false: those bits were not there
    bool get(int k, unsigned* v) { *v = peek(k); return drop(k); }
    // to the next byte boundary, the buffered whole bytes handed back
    void align() { (void)drop(cnt & 7); pos -= (size_t)(cnt >> 3); buf = 0; cnt = 0; }
};

// ---- canonical Huffman codes: 9 leading bits through a table, longer codes by length -----------------------------------------------
constexpr int FAST_BITS = 9;
struct Huff {
    uint16_t fast[1 << FAST_BITS];          // (length << 9) | symbol, 0 when the code is longer or absent
    uint16_t firstcode[17], firstsymbol[17];
    int maxcode[18];                        // left-aligned to 16 bits; [16] closes the search
    unsigned char size[288];
    uint16_t value[288];
    int n;
};

unsigned bitrev16(unsigned v) {
    v = ((v & 0xAAAAu) >> 1) | ((v & 0x5555u) << 1);
    v = ((v & 0xCCCCu) >> 2) | ((v & 0x3333u) << 2);
    v = ((v & 0xF0F0u) >> 4) | ((v & 0x0F0Fu) << 4);
    return ((v & 0xFF00u) >> 8) | ((v & 0x00FFu) << 8);
}

enum { CODE_COMPLETE = 0, CODE_OR_SINGLE = 1, CODE_OR_SINGLE_OR_NONE = 2 };
// The code of lens[0 .. n): false when it is over-subscribed, or incomplete beyond what `rule` admits (a single code of length 1,
// as deflate encoders write for one distance; no code at all for a block of literals only).
bool build_huff(Huff& h, const unsigned char* lens, int n, int rule) {
    int count[17] = { 0 };
    std::memset(h.fast, 0, sizeof(h.fast));
    for (int i = 0; i < n; ++i) ++count[lens[i]];
    count[0] = 0;
    int left = 1, total = 0;
    for (int l = 1; l <= 15; ++l) {
        left = 2 * left - count[l];
        if (left < 0) return false;                                     // over-subscribed
        total += count[l];
    }
    if (left > 0) {
        const bool single = total == 1 && count[1] == 1;
        if (!((rule >= CODE_OR_SINGLE && single) || (rule == CODE_OR_SINGLE_OR_NONE && total == 0))) return false;
    }
    int next[17];
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 15; ++l) {
        next[l] = (int)code;
        h.firstcode[l] = (uint16_t)code;
        h.firstsymbol[l] = (uint16_t)k;
        code += (unsigned)count[l];
        h.maxcode[l] = (int)(code << (16 - l));
        code <<= 1;
        k += count[l];
    }
    h.firstcode[16] = 0; h.firstsymbol[16] = 0;
    h.maxcode[16] = 0x10000;
    h.maxcode[17] = 0x10000;
    h.n = total;
    for (int i = 0; i < n; ++i) {
        const int l = lens[i];
        if (!l) continue;
        const int c = next[l] - h.firstcode[l] + h.firstsymbol[l];
        h.size[c] = (unsigned char)l;
        h.value[c] = (uint16_t)i;
        if (l <= FAST_BITS) {
            const unsigned entry = ((unsigned)l << 9) | (unsigned)i;
            for (unsigned j = bitrev16((unsigned)next[l]) >> (16 - l); j < (1u << FAST_BITS); j += 1u << l) h.fast[j] = (uint16_t)entry;
        }
        ++next[l];
    }
    return true;
}

// The next symbol, -1 for a code that is not in the table or that runs past the end of the input.
int decode_symbol(Bits& b, const Huff& h) {
    const unsigned v = b.peek(16);
    const unsigned f = h.fast[v & ((1u << FAST_BITS) - 1u)];
    if (f) return b.drop((int)(f >> 9)) ? (int)(f & 511u) : -1;
    const int k = (int)bitrev16(v);
    int s = FAST_BITS + 1;
    while (k >= h.maxcode[s]) ++s;                                      // maxcode[16] = 0x10000 ends it
    if (s >= 16) return -1;
    const int c = (k >> (16 - s)) - h.firstcode[s] + h.firstsymbol[s];
    if (c < 0 || c >= h.n || h.size[c] != s) return -1;
    return b.drop(s) ? (int)h.value[c] : -1;
}

const uint16_t LEN_BASE[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258 };
const unsigned char LEN_EXTRA[29] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0 };
const uint16_t DIST_BASE[30] = { 1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577 };
const unsigned char DIST_EXTRA[30] = { 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13 };
const unsigned char CLEN_ORDER[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };

struct FixedCodes {
    Huff lit, dist;
    FixedCodes() {
        unsigned char l[288], d[32];
        for (int i = 0; i < 288; ++i) l[i] = (unsigned char)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        for (int i = 0; i < 32; ++i) d[i] = 5;                          // 32 codes of 5 bits; 30 and 31 are refused where they are met
        (void)build_huff(lit, l, 288, CODE_COMPLETE);
        (void)build_huff(dist, d, 32, CODE_COMPLETE);
    }
};
const FixedCodes& fixed_codes() { static const FixedCodes F; return F; }

bool read_dynamic(Bits& b, Huff& lit, Huff& dist) {
    unsigned hlit, hdist, hclen;
    if (!b.get(5, &hlit) || !b.get(5, &hdist) || !b.get(4, &hclen)) return false;
    hlit += 257; hdist += 1; hclen += 4;
    if (hlit > 286 || hdist > 30) return false;
    unsigned char cl[19] = { 0 };
    for (unsigned i = 0; i < hclen; ++i) {
        unsigned v;
        if (!b.get(3, &v)) return false;
        cl[CLEN_ORDER[i]] = (unsigned char)v;
    }
    Huff clen;
    if (!build_huff(clen, cl, 19, CODE_COMPLETE)) return false;
    unsigned char lens[286 + 30];
    const unsigned total = hlit + hdist;
    for (unsigned i = 0; i < total;) {
        const int sym = decode_symbol(b, clen);
        if (sym < 0 || sym > 18) return false;
        if (sym < 16) { lens[i++] = (unsigned char)sym; continue; }
        unsigned rep, fill = 0;
        if (sym == 16) {
            if (i == 0 || !b.get(2, &rep)) return false;
            rep += 3; fill = lens[i - 1];
        } else if (sym == 17) {
            if (!b.get(3, &rep)) return false;
            rep += 3;
        } else {
            if (!b.get(7, &rep)) return false;
            rep += 11;
        }
        if (i + rep > total) return false;
        std::memset(lens + i, (int)fill, rep);
        i += rep;
    }
    if (lens[256] == 0) return false;                                   // a block cannot end
    return build_huff(lit, lens, (int)hlit, CODE_OR_SINGLE) && build_huff(dist, lens + hlit, (int)hdist, CODE_OR_SINGLE_OR_NONE);
}

}  // namespace

uint32_t png_crc32(const unsigned char* p, size_t n, uint32_t crc) {
    const CrcTables& T = crc_tables();
    uint32_t c = ~crc;
    while (n >= 8) {
        const uint32_t lo = c ^ ((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
        c = T.t[7][lo & 255u] ^ T.t[6][(lo >> 8) & 255u] ^ T.t[5][(lo >> 16) & 255u] ^ T.t[4][lo >> 24] ^ T.t[3][p[4]] ^ T.t[2][p[5]] ^ T.t[1][p[6]] ^ T.t[0][p[7]];
        p += 8; n -= 8;
    }
    for (; n; --n, ++p) c = T.t[0][(c ^ *p) & 255u] ^ (c >> 8);
    return ~c;
}

uint32_t png_adler32(const unsigned char* p, size_t n) {
    uint32_t a = 1, b = 0;
    while (n) {
        const size_t run = n < 5552 ? n : 5552;                         // the largest run whose sums fit 32 bits
        for (size_t i = 0; i < run; ++i) { a += p[i]; b += a; }
        a %= 65521u; b %= 65521u;
        p += run; n -= run;
    }
    return (b << 16) | a;
}

bool png_inflate_raw(const unsigned char* z, size_t zn, unsigned char* out, size_t cap, size_t* produced, size_t* used) {
    Bits b;
    b.p = z; b.n = zn; b.pos = 0; b.buf = 0; b.cnt = 0;
    size_t op = 0;
    bool ok = false;
    Huff dyn_lit, dyn_dist;
    for (;;) {
        unsigned final_block, type;
        if (!b.get(1, &final_block) || !b.get(2, &type)) break;
        if (type == 3) break;                                           // reserved
        if (type == 0) {
            b.align();
            if (zn - b.pos < 4) break;
            const unsigned len = (unsigned)z[b.pos] | ((unsigned)z[b.pos + 1] << 8), nlen = (unsigned)z[b.pos + 2] | ((unsigned)z[b.pos + 3] << 8);
            b.pos += 4;
            if ((len ^ nlen) != 0xFFFFu) break;
            if (zn - b.pos < len || cap - op < len) break;
            if (len) std::memcpy(out + op, z + b.pos, len);
            op += len; b.pos += len;
        } else {
            const Huff *lit, *dist;
            if (type == 1) {
                lit = &fixed_codes().lit; dist = &fixed_codes().dist;
            } else {
                if (!read_dynamic(b, dyn_lit, dyn_dist)) break;
                lit = &dyn_lit; dist = &dyn_dist;
            }
            bool block_ok = false;
            for (;;) {
                int sym = decode_symbol(b, *lit);
                if (sym < 0) break;
                if (sym < 256) {
                    if (op >= cap) break;                               // the stream wants more than the image holds
                    out[op++] = (unsigned char)sym;
                    continue;
                }
                if (sym == 256) { block_ok = true; break; }
                sym -= 257;
                if (sym >= 29) break;
                unsigned extra;
                if (!b.get(LEN_EXTRA[sym], &extra)) break;
                const size_t len = (size_t)LEN_BASE[sym] + extra;
                const int d = decode_symbol(b, *dist);
                if (d < 0 || d >= 30) break;
                if (!b.get(DIST_EXTRA[d], &extra)) break;
                const size_t distance = (size_t)DIST_BASE[d] + extra;
                if (distance > op) break;                               // before the start of the output
                if (cap - op < len) break;
                const unsigned char* from = out + op - distance;
                for (size_t i = 0; i < len; ++i) out[op + i] = from[i];  // byte by byte: the ranges may overlap
                op += len;
            }
            if (!block_ok) break;
        }
        if (final_block) { ok = true; break; }
    }
    *produced = op;
    *used = b.pos - (size_t)(b.cnt >> 3);
    return ok;
}

int png_inflate_zlib(const unsigned char* z, size_t zn, unsigned char* out, size_t expect) {
    if (zn < 2) return PNG_CORRUPT;
    const unsigned cmf = z[0], flg = z[1];
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 0x20u) || ((cmf << 8) | flg) % 31u != 0u) return PNG_CORRUPT;
    size_t produced = 0, used = 0;
    if (!png_inflate_raw(z + 2, zn - 2, out, expect, &produced, &used)) return PNG_CORRUPT;
    if (produced != expect) return PNG_CORRUPT;
    if (zn - 2 - used < 4) return PNG_CORRUPT;
    if (be32(z + 2 + used) != png_adler32(out, expect)) return PNG_CORRUPT;
    return PNG_OK;                                                      // bytes after the Adler-32 are ignored
}

namespace {
int refuse(PngHeader* h, int status) {
    h->status = status;
    h->width = h->height = h->bit_depth = h->colour_type = h->interlace = h->samples = h->channels = h->bpp = h->n_palette = 0;
    h->rowbytes = h->stream_bytes = h->idat_bytes = 0;
    h->idat.clear();
    return status;
}
uint32_t chunk_name(const char* s) { return be32(reinterpret_cast<const unsigned char*>(s)); }
}  // namespace

int png_parse(const unsigned char* data, size_t n, PngHeader* h) {
    static const unsigned char SIGNATURE[8] = { 0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A };
    h->status = PNG_CORRUPT;
    h->width = h->height = h->bit_depth = h->colour_type = h->interlace = h->samples = h->channels = h->bpp = h->n_palette = 0;
    h->rowbytes = h->stream_bytes = h->idat_bytes = 0;
    std::memset(h->palette, 0, sizeof(h->palette));
    h->idat.clear();
    if (n < 8 || std::memcmp(data, SIGNATURE, 8) != 0) return refuse(h, PNG_CORRUPT);
    const uint32_t IHDR = chunk_name("IHDR"), PLTE = chunk_name("PLTE"), IDAT = chunk_name("IDAT"), IEND = chunk_name("IEND");
    size_t at = 8;
    bool first = true, have_plte = false, idat_open = false, idat_closed = false, ended = false, unsupported = false;
    while (!ended) {
        if (n - at < 12) return refuse(h, PNG_CORRUPT);                 // IEND missing, or a chunk cut short
        const uint32_t len = be32(data + at), type = be32(data + at + 4);
        if (len > 0x7FFFFFFFu || (size_t)len > n - at - 12) return refuse(h, PNG_CORRUPT);
        const unsigned char* body = data + at + 8;
        if (png_crc32(data + at + 4, (size_t)len + 4) != be32(body + len)) return refuse(h, PNG_CORRUPT);
        if (first != (type == IHDR)) return refuse(h, PNG_CORRUPT);     // IHDR missing, not first, or met again
        if (type != IDAT && idat_open) { idat_open = false; idat_closed = true; }
        if (type == IHDR) {
            if (len != 13) return refuse(h, PNG_CORRUPT);
            const uint32_t w = be32(body), ht = be32(body + 4);
            const int depth = body[8], ct = body[9];
            if (w == 0 || ht == 0 || w > 0x7FFFFFFFu || ht > 0x7FFFFFFFu) return refuse(h, PNG_CORRUPT);
            bool pair_ok;
            switch (ct) {
                case 0: pair_ok = depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16; break;
                case 3: pair_ok = depth == 1 || depth == 2 || depth == 4 || depth == 8; break;
                case 2: case 4: case 6: pair_ok = depth == 8 || depth == 16; break;
                default: pair_ok = false;
            }
            if (!pair_ok || body[10] != 0 || body[11] != 0 || body[12] > 1) return refuse(h, PNG_CORRUPT);
            if (body[12] == 1 || w > (uint32_t)PNG_MAX_SIDE || ht > (uint32_t)PNG_MAX_SIDE) {
                unsupported = true;                                     // well-formed so far; the rest of the walk still has to hold
            } else {
                h->width = (int)w; h->height = (int)ht;
                h->bit_depth = depth; h->colour_type = ct; h->interlace = 0;
                h->samples = ct == 0 || ct == 3 ? 1 : ct == 4 ? 2 : ct == 2 ? 3 : 4;
                h->channels = ct == 0 || ct == 4 ? 1 : 3;
                h->bpp = h->samples * depth >= 8 ? h->samples * depth / 8 : 1;
                h->rowbytes = ((long long)w * h->samples * depth + 7) / 8;
                h->stream_bytes = (long long)ht * (1 + h->rowbytes);
            }
            first = false;
        } else if (type == PLTE) {
            if (have_plte || idat_closed || !h->idat.empty() || len == 0 || len % 3 != 0 || len > 768) return refuse(h, PNG_CORRUPT);
            have_plte = true;
            h->n_palette = (int)(len / 3);
            std::memcpy(h->palette, body, len);
        } else if (type == IDAT) {
            if (idat_closed) return refuse(h, PNG_CORRUPT);             // IDAT chunks must be consecutive
            idat_open = true;
            h->idat.push_back(std::make_pair((size_t)(body - data), (size_t)len));
            h->idat_bytes += (long long)len;
        } else if (type == IEND) {
            ended = true;
        } else if (!(data[at + 4] & 0x20u)) {
            unsupported = true;                                         // a critical chunk this reader does not know
        }
        at += (size_t)len + 12;
    }
    if (h->idat.empty()) return refuse(h, PNG_CORRUPT);
    if (unsupported) return refuse(h, PNG_UNSUPPORTED);
    if (h->colour_type == 3 && !have_plte) return refuse(h, PNG_CORRUPT);
    if (h->colour_type != 3) { h->n_palette = 0; std::memset(h->palette, 0, sizeof(h->palette)); }      // a suggested palette is not used
    if (h->stream_bytes > 1032ll * h->idat_bytes + 64) return refuse(h, PNG_CORRUPT);                   // an image its file cannot hold
    h->status = PNG_OK;
    return PNG_OK;
}

int png_inflate_image(const unsigned char* data, size_t n, const PngHeader& h, unsigned char* stream) {
    if (h.status != PNG_OK) return PNG_CORRUPT;
    const unsigned char* z = nullptr;
    size_t zn = 0;
    std::vector<unsigned char> joined;
    if (h.idat.size() == 1) {
        if (h.idat[0].first > n || h.idat[0].second > n - h.idat[0].first) return PNG_CORRUPT;
        z = data + h.idat[0].first; zn = h.idat[0].second;
    } else {
        joined.reserve((size_t)h.idat_bytes);
        for (const std::pair<size_t, size_t>& c : h.idat) {
            if (c.first > n || c.second > n - c.first) return PNG_CORRUPT;
            joined.insert(joined.end(), data + c.first, data + c.first + c.second);
        }
        z = joined.data(); zn = joined.size();
    }
    if (png_inflate_zlib(z, zn, stream, (size_t)h.stream_bytes) != PNG_OK) return PNG_CORRUPT;
    const size_t stride = (size_t)h.rowbytes + 1;
    for (int y = 0; y < h.height; ++y)
        if (stream[(size_t)y * stride] > 4) return PNG_CORRUPT;
    return PNG_OK;
}

void png_parse_batch(int n_images, const int64_t* file_ptr, const unsigned char* bytes, std::vector<PngHeader>& headers) {
    headers.resize((size_t)(n_images > 0 ? n_images : 0));
    for (int i = 0; i < n_images; ++i) png_parse(bytes + file_ptr[i], (size_t)(file_ptr[i + 1] - file_ptr[i]), &headers[(size_t)i]);
}

bool png_inflate_batch(int n_images, const int64_t* file_ptr, const unsigned char* bytes, int max_threads, std::vector<PngHeader>& headers,
                       std::vector<std::vector<unsigned char> >& streams) {
    streams.assign((size_t)(n_images > 0 ? n_images : 0), std::vector<unsigned char>());
    std::atomic<bool> alloc_failed(false);
    host_pool_for(n_images, max_threads, [&](int i) {
        PngHeader& h = headers[(size_t)i];
        if (h.status != PNG_OK) return;
        std::vector<unsigned char>& s = streams[(size_t)i];
        int status;
        try {
            s.resize((size_t)h.stream_bytes);
            status = png_inflate_image(bytes + file_ptr[i], (size_t)(file_ptr[i + 1] - file_ptr[i]), h, s.data());
        } catch (const std::bad_alloc&) {                               // nothing may leave a worker thread
            alloc_failed = true;
            return;
        }
        if (status != PNG_OK) {
            std::vector<unsigned char>().swap(s);
            refuse(&h, status);
        }
    });
    return !alloc_failed;
}

}  // namespace sfmba
