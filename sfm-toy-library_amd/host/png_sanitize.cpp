// png_sanitize.cpp -- the host half of sfmba_png_decode (csrc/png_inflate.cpp: chunk walk, CRC-32, zlib wrapper, inflate) under
// AddressSanitizer + UBSan: `make -C sfm-toy-library_amd/host png_asan`.  Host code only, no device involved.
//   png_sanitize_asan DIR...        every *.png of the directories is walked and inflated as it is; the two files named below are
//                                   decoded at every prefix length; every one of the first 700 bytes of a third is replaced by 0x00,
//                                   by 0xFF and by itself with the top bit flipped; and the bare deflate streams of two more go to
//                                   the inflate DIRECTLY (no CRC, no Adler-32 in the way, which would refuse nearly every mutation
//                                   before the decoder saw it) with each of their first 350 bytes replaced in the same three ways.
// Every outcome must be PNG_OK, PNG_UNSUPPORTED or PNG_CORRUPT, and the sanitizers must stay silent.
#include <dirent.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../csrc/png_inflate.h"

using namespace sfmba;

static long counts[3];

// the decode of a heap copy of exactly n bytes into a heap array of exactly the expected size, so that a read or a write past
// either end is a report
static int decode(const unsigned char* data, size_t n) {
    std::vector<unsigned char> copy(data, data + n);
    PngHeader h;
    int status = png_parse(copy.data(), copy.size(), &h);
    if (status == PNG_OK) {
        std::vector<unsigned char> stream((size_t)h.stream_bytes);
        status = png_inflate_image(copy.data(), copy.size(), h, stream.data());
    }
    if (status < 0 || status > 2) { std::printf("png_sanitize: status %d\n", status); std::exit(1); }
    ++counts[status];
    return status;
}

// the bare deflate stream z into exactly `expect` bytes
static bool inflate_raw(const std::vector<unsigned char>& z, size_t expect) {
    std::vector<unsigned char> copy(z), out(expect);
    size_t produced = 0, used = 0;
    const bool ok = png_inflate_raw(copy.data(), copy.size(), out.data(), out.size(), &produced, &used);
    if (produced > expect || used > copy.size()) { std::printf("png_sanitize: inflate reports %zu bytes out, %zu in\n", produced, used); std::exit(1); }
    return ok && produced == expect;
}

int main(int argc, char** argv) {
    const char* const TRUNCATE[2] = { "t3_d4_37x20.png", "dynamic_t2_d8_40x30.png" };
    const char* const MUTATE = "shortplte_t3_d8_30x20.png";
    const char* const RAW[2] = { "dynamic_t2_d8_40x30.png", "fixed_t2_d8_40x30.png" };
    long files = 0, truncations = 0, mutations = 0, raw_mutations = 0, raw_ok = 0, intact_ok = 0;
    for (int a = 1; a < argc; ++a) {
        DIR* dir = opendir(argv[a]);
        if (!dir) { std::printf("png_sanitize: cannot read %s\n", argv[a]); return 1; }
        while (const dirent* entry = readdir(dir)) {
            const std::string name = entry->d_name;
            if (name.size() < 4 || name.substr(name.size() - 4) != ".png") continue;
            std::ifstream in((std::string(argv[a]) + "/" + name).c_str(), std::ios::binary);
            std::vector<unsigned char> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            ++files;
            if (decode(data.data(), data.size()) == PNG_OK) ++intact_ok;
            if (name == TRUNCATE[0] || name == TRUNCATE[1])
                for (size_t n = 0; n < data.size(); ++n, ++truncations) decode(data.data(), n);
            if (name == MUTATE)
                for (size_t i = 0; i < 700 && i < data.size(); ++i) {
                    const unsigned char keep = data[i], with[3] = { 0x00, 0xFF, (unsigned char)(keep ^ 0x80) };
                    for (int k = 0; k < 3; ++k, ++mutations) { data[i] = with[k]; decode(data.data(), data.size()); }
                    data[i] = keep;
                }
            if (name == RAW[0] || name == RAW[1]) {
                PngHeader h;
                if (png_parse(data.data(), data.size(), &h) != PNG_OK || h.idat.size() != 1 || h.idat[0].second < 6) { std::printf("png_sanitize: %s\n", name.c_str()); return 1; }
                // without the two bytes of the zlib header and the four of the Adler-32
                std::vector<unsigned char> z(data.begin() + (long)h.idat[0].first + 2, data.begin() + (long)(h.idat[0].first + h.idat[0].second) - 4);
                if (!inflate_raw(z, (size_t)h.stream_bytes)) { std::printf("png_sanitize: the intact stream of %s does not inflate\n", name.c_str()); return 1; }
                for (size_t i = 0; i < 350 && i < z.size(); ++i) {
                    const unsigned char keep = z[i], with[3] = { 0x00, 0xFF, (unsigned char)(keep ^ 0x80) };
                    for (int k = 0; k < 3; ++k, ++raw_mutations) { z[i] = with[k]; if (inflate_raw(z, (size_t)h.stream_bytes)) ++raw_ok; }
                    z[i] = keep;
                }
            }
        }
        closedir(dir);
    }
    std::printf("png_sanitize: %ld files (%ld decodable), %ld truncations, %ld mutations: %ld ok, %ld unsupported, %ld corrupt; %ld raw mutations (%ld inflate)\n",
                files, intact_ok, truncations, mutations, counts[0], counts[1], counts[2], raw_mutations, raw_ok);
    return 0;
}
