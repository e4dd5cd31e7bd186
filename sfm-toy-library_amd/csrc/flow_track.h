// flow_track.h -- batched pyramidal Lucas-Kanade tracking and the snap of its end points to key points behind sfmba_flow_track /
// sfmba_flow_match (flow_track.hip; arithmetic in flow_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h

// Pairs go to the device in consecutive groups.  A group's arrays (the pixels of the images its pairs name, their pyramids, the
// points and what is written per point) stay within this bound; a pair that exceeds it alone forms a group of its own.  The unit
// caps the images of a group (65535, grid.y), not its pairs; the test hook SFMBA_GROUP_ITEMS (unit_common.h) counts pairs here.
constexpr size_t FLOW_SCRATCH_BYTES = (size_t)512 << 20;
constexpr int FLOW_MATCH_TILE = 256;           // key points of an LDS stage of the matcher
constexpr int FLOW_MATCH_QUERIES = 64;         // queries of a workgroup: one lane each

// phases of the timing arrays
enum { FLOW_T_UPLOAD = 0, FLOW_T_GRAY, FLOW_T_PYRAMID, FLOW_T_TRACK, FLOW_T_DOWNLOAD, FLOW_T_GROUPS, FLOW_T_COUNT };
enum { FLOWM_T_UPLOAD = 0, FLOWM_T_NEAR, FLOWM_T_COMPACT, FLOWM_T_DOWNLOAD, FLOWM_T_COUNT };

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// [FLOW_T_COUNT] = HIP-event milliseconds on `s` summed over groups, then the number of groups.
int flow_track(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
               const int32_t* height, int channels, int n_pairs, const int32_t* pair_src, const int32_t* pair_dst, const int64_t* pt_ptr,
               const float* pts, int n_levels, int radius, int max_iters, float min_eig, float* next, unsigned char* status, float* err,
               int64_t* dbg_G, int32_t* dbg_state, unsigned char* dbg_pyramid, double* timing);

// timing (may be NULL): [FLOWM_T_COUNT] = milliseconds of upload, the nearest-two and winner kernels, scan and scatter, download.
int flow_match(hipStream_t s, int device, int n_images, const int64_t* kp_ptr, const float* kp_xy, int n_pairs, const int32_t* pair_dst,
               const int64_t* pt_ptr, const float* next, const unsigned char* status, const float* err, float max_err, float radius,
               double ratio, int64_t* pair_ptr, int32_t* query_idx, int32_t* train_idx, float* distance, int64_t cap, int64_t* total,
               double* timing);

}  // namespace sfmba
