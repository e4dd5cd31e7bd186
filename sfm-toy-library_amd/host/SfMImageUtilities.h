// SfMImageUtilities.h -- the two lines of SfM::setImagesDirectory that read and shrink the photographs (SfMToyLib/SfM.cpp:125-129:
// imread, then resize(..., Size(), f, f)), as free-standing functions over whole lists, backed by the MI355X decoder and resize
// (include/sfmba.h: sfmba_jpeg_decode, sfmba_png_decode, sfmba_resize_images).  A maintainer replaces the loop body by one call after the loop:
//
//   SfMImageUtilities::readImages(mImagesFilenames, mDownscaleFactor, mImages);
//
// The pixels are libjpeg's default decode of a baseline file bit for bit (so imread's, for such a file), and of a PNG file the
// samples themselves (16-bit ones reduced to their high byte, alpha dropped, no gamma: IMREAD_COLOR's, for such a file, except that a
// gray PNG stays one channel as a gray JPEG does); the resize samples where
// cv::resize(..., INTER_LINEAR) samples, with the project's own integer rounding (within one level of the exact bilinear value).
// EXIF orientation is ignored.
#pragma once
#include <string>
#include <vector>

#include "SfMCommon.h"

namespace sfmtoylib {

class SfMImageUtilities {
public:
    /**
     * images[i] = the JPEG or PNG file paths[i] (its first bytes decide which, not its name), decoded (one component -> CV_8U, three
     * -> CV_8UC3 stored B, G, R) and, with downscale != 1, resized by that factor on the device: ONE device call for the JPEG files
     * of the list and ONE for the PNG files.  Returns false (images is then empty; a line is written to stderr) when a file cannot
     * be read, is neither, is not a decodable baseline JPEG / non-interlaced PNG, or on a device error.
     */
    static bool readImages(
            const std::vector<std::string>& paths,
            float                           downscale,
            std::vector<cv::Mat>&           images);

    /**
     * out[i] = images[i] resized by downscale: ONE device call.  All images must be of one type (CV_8U or CV_8UC3).  Returns false
     * (out is then empty; a line is written to stderr) on a refused factor or a device error.
     */
    static bool resizeImages(
            const std::vector<cv::Mat>& images,
            float                       downscale,
            std::vector<cv::Mat>&       out);
};

}  // namespace sfmtoylib
