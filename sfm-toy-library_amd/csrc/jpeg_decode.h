// jpeg_decode.h -- batched baseline-JPEG decode and bilinear resize behind sfmba_jpeg_decode / sfmba_resize_images
// (jpeg_decode.hip; host half in jpeg_entropy.cpp, arithmetic in jpeg_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/sfmba.h"
#include "jpeg_entropy.h"
#include "unit_common.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h

// Images go to the device in consecutive groups.  A group's arrays (coefficients, component planes, decoded pixels, resize tables
// and resized pixels) stay within this bound; an image that exceeds it alone forms a group of its own.
constexpr size_t JPEG_SCRATCH_BYTES = (size_t)512 << 20;
constexpr int JPEG_MAX_GROUP_IMAGES = 1024;      // grid.y of the per-image launches (three times that for the per-component one)

// phases of the timing array
enum { JPEG_T_ENTROPY = 0, JPEG_T_UPLOAD, JPEG_T_IDCT, JPEG_T_COLOUR, JPEG_T_RESIZE, JPEG_T_DOWNLOAD, JPEG_T_GROUPS, JPEG_T_COUNT };

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// [JPEG_T_COUNT] = host wall milliseconds of the parse + entropy decode, then HIP-event milliseconds on `s` summed over groups --
// upload, dequantise + inverse DCT kernel, upsample + colour kernel, resize kernel, download -- and the number of groups.
int jpeg_decode(hipStream_t s, int device, int n_images, const int64_t* file_ptr, const unsigned char* bytes, float factor,
                sfmba_image_info* info, int64_t* out_ptr, unsigned char* out, int64_t cap, int64_t* total, double* timing);

int resize_images(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* px, const int32_t* width,
                  const int32_t* height, int channels, float factor, int64_t* out_ptr, unsigned char* out, int64_t cap, int64_t* total,
                  double* timing);

// ---- shared with the PNG reader (png_decode.hip), which ends in the same resize ------------------------------------------------------
// What the resize of one image of a group needs.
struct ResizeJob {
    int w, h, ow, oh, channels;
    long long src;              // first byte in the device source region (a multiple of 4)
};

// device bytes launch_resize allocates for one job
long long resize_scratch(const ResizeJob& j);
// Tables up, one k_resize launch over the jobs (the upload goes to phase JPEG_T_UPLOAD, the kernel to JPEG_T_RESIZE): *d_dst
// receives the destination region, dst_off [jobs] the first byte of each result.  Returns 0 or a hipError_t; `s` is drained.
class DeviceArena;
int launch_resize(hipStream_t s, DeviceArena& arena, PhaseTimer& tm, const std::vector<ResizeJob>& jobs, float factor, const unsigned char* d_src,
                  unsigned char** d_dst, std::vector<long long>& dst_off);

// the header fields of sfmba_image_info (host only)
void jpeg_fill_info(const JpegHeader& h, sfmba_image_info* info);

}  // namespace sfmba
