// essential_ransac.h -- batched five-point essential-matrix RANSAC + recoverPose behind sfmba_essential_ransac (essential_ransac.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h

constexpr int ESS_HYP_THREADS = 64;          // hypotheses: one lane each, one wave per block; the lanes' work areas fill 100 KiB of LDS
constexpr int ESS_TILE = 64;                 // hypotheses per score block: one per lane of a wave
constexpr int ESS_CHUNK = 1024;              // correspondences a score block stages in LDS at a time (one float4 each)
constexpr int ESS_SCORE_THREADS = 256;       // 4 waves share the tile's 64 hypotheses and interleave the chunk's correspondences
constexpr int ESS_MAX_CHUNK_BLOCKS = 64;     // grid.y of the score kernel, at most: a block then walks several chunks
constexpr int ESS_SELECT_THREADS = 256;      // select + pose: one block per pair

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// { upload, k_ess_hypotheses, k_ess_score, k_ess_select, download } in ms from HIP events on `s`.
int essential_ransac(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const float* pts, int n_pairs, const int32_t* pair_left,
                     const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx, const float* K,
                     int n_hyp, float threshold_px, uint64_t seed, double* E, double* pose, unsigned char* inlier,
                     sfmba_essential_result* result, double* hyp_E, int32_t* hyp_count, int32_t* hyp_nsol, double* timing);

}  // namespace sfmba
