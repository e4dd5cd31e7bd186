// orb_extract.h -- batched ORB-style detect and describe behind sfmba_orb_extract (orb_extract.hip; arithmetic in orb_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h

// The score and the smoothing kernels work on tiles of this many pixels of a level (plus a 3-pixel halo), one block of 256 lanes
// per tile, four pixels per lane.
constexpr int ORB_TILE_W = 64;
constexpr int ORB_TILE_H = 16;

// Images go to the device in consecutive groups.  A group's per-level arrays (two pyramid levels, score map, smoothed level,
// flags, scan positions, the four candidate sort buffers, and the BGR input when there is one) stay within this bound; an image
// that exceeds it alone forms a group of its own.  hipCUB's temporaries (a few MiB) come on top.
constexpr size_t ORB_SCRATCH_BYTES = (size_t)512 << 20;
constexpr int ORB_MAX_GROUP_IMAGES = 1024;   // grid.y of the per-level launches, and the image bits of the second sort pass

// phases of the timing array
enum { ORB_T_UPLOAD = 0, ORB_T_PYRAMID, ORB_T_SCORE, ORB_T_CANDIDATES, ORB_T_HARRIS, ORB_T_SELECT, ORB_T_SMOOTH, ORB_T_DESCRIBE,
       ORB_T_DOWNLOAD, ORB_T_GROUPS, ORB_T_COUNT };

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// [ORB_T_COUNT] = HIP-event milliseconds on `s` summed over groups and levels -- upload, gray + resample kernels, score kernel,
// flags + scan + compaction, response kernel, the sort passes, smoothing kernel, orientation + descriptor kernel, pack +
// download -- and the number of groups.
int orb_extract(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
                const int32_t* height, int channels, int n_features, float scale_factor, int n_levels, int fast_threshold,
                int64_t* kp_ptr, sfmba_orb_keypoint* kp, unsigned char* desc, int64_t cap, int64_t* total, int32_t* dbg_level_xy,
                int32_t* dbg_bin, int64_t* dbg_harris, int32_t* dbg_candidates, double* timing);

}  // namespace sfmba
