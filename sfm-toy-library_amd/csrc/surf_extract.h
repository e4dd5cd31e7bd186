// surf_extract.h -- batched Fast-Hessian detect and SURF-style describe behind sfmba_surf_extract (surf_extract.hip; arithmetic in
// surf_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h

// Images go to the device in consecutive groups.  A group's arrays (the input bytes, the integral images, the response maps of
// every octave, the four candidate sort buffers) stay within this bound; an image that exceeds it alone forms a group of its own.
// hipCUB's temporaries (a few MiB) and the group's output rows come on top.
constexpr size_t SURF_SCRATCH_BYTES = (size_t)512 << 20;
constexpr int SURF_MAX_GROUP_IMAGES = 1024;   // grid.y of the launches, and the image bits of the last sort pass

// phases of the timing array
enum { SURF_T_UPLOAD = 0, SURF_T_INTEGRAL, SURF_T_RESPONSE, SURF_T_CANDIDATES, SURF_T_SELECT, SURF_T_DESCRIBE, SURF_T_DOWNLOAD, SURF_T_GROUPS,
       SURF_T_RESPONSE_BYTES, SURF_T_COUNT };

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// [SURF_T_COUNT] = HIP-event milliseconds on `s` summed over groups and octaves -- upload, gray + integral kernels, response
// kernel, candidate kernel, the sort passes, orientation + descriptor kernel, download -- then the number of groups and the bytes
// the response kernel wrote (8 per sample it computes).
int surf_extract(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
                 const int32_t* height, int channels, int n_features, int n_octaves, float hessian_threshold, int upright, int64_t* kp_ptr,
                 sfmba_surf_keypoint* kp, float* desc, int64_t cap, int64_t* total, int32_t* dbg_bin, int64_t* dbg_moments, int64_t* dbg_sums,
                 int32_t* dbg_candidates, double* timing);

}  // namespace sfmba
