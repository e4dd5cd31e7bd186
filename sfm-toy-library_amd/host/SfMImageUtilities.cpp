// SfMImageUtilities.cpp -- host side of the image reader: flattens the files / images, calls the C ABI (include/sfmba.h,
// sfmba_jpeg_decode, sfmba_png_decode, sfmba_resize_images) and rebuilds the reference's list of cv::Mat.  See SfMImageUtilities.h.
#include "SfMImageUtilities.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

#include "../../include/sfmba.h"

namespace sfmtoylib {

namespace {

cv::Mat imageFromBytes(int w, int h, int channels, const unsigned char* px) {
    cv::Mat m(h, w, channels == 3 ? CV_8UC3 : CV_8U);
    for (int r = 0; r < h; ++r) std::memcpy(m.ptr<unsigned char>(r), px + (size_t)r * w * channels, (size_t)w * channels);
    return m;
}

const char* const statusNames[] = { "ok", "outside the scope of this reader (baseline JPEG, non-interlaced PNG)", "corrupt" };

bool isPng(const std::vector<unsigned char>& f) {
    static const unsigned char SIGNATURE[8] = { 0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A };
    return f.size() >= 8 && std::memcmp(f.data(), SIGNATURE, 8) == 0;
}
bool isJpeg(const std::vector<unsigned char>& f) { return f.size() >= 2 && f[0] == 0xFF && f[1] == 0xD8; }

// The files `which` of one format in ONE decode call (sfmba_jpeg_* or sfmba_png_*: both info structs begin with status, width,
// height, channels); images[which[k]] receives file k.
template <typename Info, typename InfoFn, typename DecodeFn>
bool decodeFiles(const std::vector<std::string>& paths, const std::vector<std::vector<unsigned char> >& files, const std::vector<size_t>& which,
                 float downscale, InfoFn infoFn, DecodeFn decodeFn, std::vector<cv::Mat>& images) {
    const size_t n = which.size();
    if (n == 0) return true;
    std::vector<int64_t> ptr(n + 1, 0), out_ptr(n + 1, 0);
    std::vector<unsigned char> bytes;
    for (size_t k = 0; k < n; ++k) {
        bytes.insert(bytes.end(), files[which[k]].begin(), files[which[k]].end());
        ptr[k + 1] = (int64_t)bytes.size();
    }
    std::vector<Info> info(n);
    std::vector<unsigned char> px;
    int64_t cap = 0, total = 0;
    if (infoFn((int)n, ptr.data(), bytes.data(), info.data()) == SFMBA_OK)          // sizes the output: one device call in the usual case
        for (size_t k = 0; k < n; ++k) {
            int32_t ow = info[k].width, oh = info[k].height;
            if (info[k].status == SFMBA_IMAGE_OK && (downscale == 1.0f || sfmba_resized_size(info[k].width, info[k].height, downscale, &ow, &oh) == SFMBA_OK))
                cap += (int64_t)ow * oh * info[k].channels;
        }
    int rc = SFMBA_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        px.resize((size_t)cap + 1);
        rc = decodeFn(0, (int)n, ptr.data(), bytes.data(), downscale, info.data(), out_ptr.data(), px.data(), cap, &total);
        if (rc == SFMBA_ERR_CAPACITY && attempt == 0) { cap = total; continue; }
        break;
    }
    if (rc != SFMBA_OK) {
        std::fprintf(stderr, "readImages failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return false;
    }
    for (size_t k = 0; k < n; ++k)
        if (info[k].status != SFMBA_IMAGE_OK) {
            std::fprintf(stderr, "readImages: %s is %s\n", paths[which[k]].c_str(), statusNames[info[k].status == SFMBA_IMAGE_UNSUPPORTED ? 1 : 2]);
            return false;
        }
    for (size_t k = 0; k < n; ++k) {
        int32_t ow = info[k].width, oh = info[k].height;
        if (downscale != 1.0f && sfmba_resized_size(info[k].width, info[k].height, downscale, &ow, &oh) != SFMBA_OK) return false;
        if (out_ptr[k + 1] - out_ptr[k] != (int64_t)ow * oh * info[k].channels) return false;
        images[which[k]] = imageFromBytes(ow, oh, info[k].channels, px.data() + out_ptr[k]);
    }
    return true;
}

}  // namespace

bool SfMImageUtilities::readImages(const std::vector<std::string>& paths, float downscale, std::vector<cv::Mat>& images) {
    images.clear();
    const size_t n = paths.size();
    if (n == 0) return true;
    // the signature decides, not the name: 89 50 4E 47 0D 0A 1A 0A is PNG, FF D8 is JPEG
    std::vector<std::vector<unsigned char> > files(n);
    std::vector<size_t> jpeg, png;
    for (size_t i = 0; i < n; ++i) {
        std::ifstream in(paths[i].c_str(), std::ios::binary);
        if (!in) { std::fprintf(stderr, "readImages: %s cannot be read\n", paths[i].c_str()); return false; }
        files[i].assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
        if (isPng(files[i])) png.push_back(i);
        else if (isJpeg(files[i])) jpeg.push_back(i);
        else { std::fprintf(stderr, "readImages: %s is neither a JPEG nor a PNG file\n", paths[i].c_str()); return false; }
    }
    // one call per format; the results go back in path order
    std::vector<cv::Mat> out(n);
    if (!decodeFiles<sfmba_image_info>(paths, files, jpeg, downscale, sfmba_jpeg_info, sfmba_jpeg_decode, out) ||
        !decodeFiles<struct sfmba_png_info>(paths, files, png, downscale, sfmba_png_info, sfmba_png_decode, out))
        return false;
    images.swap(out);
    return true;
}

bool SfMImageUtilities::resizeImages(const std::vector<cv::Mat>& images, float downscale, std::vector<cv::Mat>& out) {
    out.clear();
    const size_t n = images.size();
    if (n == 0) return true;
    const int type = images[0].type();
    if (type != CV_8U && type != CV_8UC3) { std::fprintf(stderr, "resizeImages: images must be CV_8U or CV_8UC3\n"); return false; }
    const int channels = type == CV_8UC3 ? 3 : 1;
    std::vector<int64_t> ptr(n + 1, 0), out_ptr(n + 1, 0);
    std::vector<int32_t> width(n), height(n), ow(n), oh(n);
    int64_t cap = 0, total = 0;
    for (size_t i = 0; i < n; ++i) {
        if (images[i].empty() || images[i].type() != type) { std::fprintf(stderr, "resizeImages: empty image or image types differ\n"); return false; }
        width[i] = images[i].cols; height[i] = images[i].rows;
        ptr[i + 1] = ptr[i] + (int64_t)images[i].cols * images[i].rows * channels;
        if (sfmba_resized_size(width[i], height[i], downscale, &ow[i], &oh[i]) != SFMBA_OK) {
            std::fprintf(stderr, "resizeImages: factor %g is refused (%s)\n", (double)downscale, sfmba_last_error());
            return false;
        }
        cap += (int64_t)ow[i] * oh[i] * channels;
    }
    std::vector<unsigned char> src((size_t)ptr[n]), px((size_t)cap + 1);
    for (size_t i = 0; i < n; ++i)
        for (int r = 0; r < images[i].rows; ++r)                           // row by row: an OpenCV matrix need not be continuous
            std::memcpy(&src[(size_t)ptr[i] + (size_t)r * width[i] * channels], images[i].ptr<unsigned char>(r), (size_t)width[i] * channels);
    const int rc = sfmba_resize_images(0, (int)n, ptr.data(), src.data(), width.data(), height.data(), channels, downscale, out_ptr.data(), px.data(), cap,
                                       &total);
    if (rc != SFMBA_OK) {
        std::fprintf(stderr, "resizeImages failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return false;
    }
    out.reserve(n);
    for (size_t i = 0; i < n; ++i) out.push_back(imageFromBytes(ow[i], oh[i], channels, px.data() + out_ptr[i]));
    return true;
}

}  // namespace sfmtoylib
