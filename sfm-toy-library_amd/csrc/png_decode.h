// png_decode.h -- batched PNG decode behind sfmba_png_decode (png_decode.hip; host half in png_inflate.cpp, arithmetic in
// png_math.h).  Groups, scratch bound, return values and the resize are those of the JPEG unit (jpeg_decode.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sfmba.h"
#include "jpeg_decode.h"
#include "png_inflate.h"

namespace sfmba {

// phases of the timing array: the slots of the JPEG unit, so that launch_resize files its two phases in the right ones
enum { PNG_T_INFLATE = JPEG_T_ENTROPY, PNG_T_UPLOAD = JPEG_T_UPLOAD, PNG_T_UNFILTER = JPEG_T_IDCT, PNG_T_PIXELS = JPEG_T_COLOUR,
       PNG_T_RESIZE = JPEG_T_RESIZE, PNG_T_DOWNLOAD = JPEG_T_DOWNLOAD, PNG_T_GROUPS = JPEG_T_GROUPS, PNG_T_COUNT = JPEG_T_COUNT };

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  Returns 0, a UNIT_ERR_* value or a
// positive hipError_t.  timing (may be NULL): [PNG_T_COUNT] = host wall milliseconds of the chunk walk + inflate, then HIP-event
// milliseconds on `s` summed over groups -- upload, unfilter kernel, pixel kernel, resize kernel, download -- and the number of groups.
int png_decode(hipStream_t s, int device, int n_images, const int64_t* file_ptr, const unsigned char* bytes, float factor,
               struct sfmba_png_info* info, int64_t* out_ptr, unsigned char* out, int64_t cap, int64_t* total, double* timing);

// the header fields of sfmba_png_info (host only)
void png_fill_info(const PngHeader& h, struct sfmba_png_info* info);

}  // namespace sfmba
