// homography_ransac.h -- batched four-point homography RANSAC behind sfmba_homography_ransac (homography_ransac.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h

constexpr int HOM_TILE = 64;                 // hypotheses per score block: one per lane of a wave
constexpr int HOM_CHUNK = 1024;              // correspondences a score block stages in LDS at a time (one float4 each)
constexpr int HOM_SCORE_THREADS = 256;       // 4 waves share the tile's 64 hypotheses and interleave the chunk's correspondences
constexpr int HOM_MAX_CHUNK_BLOCKS = 64;     // grid.y of the score kernel, at most: a block then walks several chunks
constexpr int HOM_SELECT_THREADS = 256;      // select: one block per pair
constexpr int HOM_HF_STRIDE = 12;            // floats per hypothesis in the fp32 copy the score reads: 9 + 3 of padding = three float4

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// { upload, k_hom_hypotheses, k_hom_score, k_hom_select, download } in ms from HIP events on `s`.
int homography_ransac(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const float* pts, int n_pairs, const int32_t* pair_left,
                      const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx, int n_hyp,
                      float threshold_px, uint64_t seed, double* H, unsigned char* inlier, sfmba_homography_result* result, double* hyp_H,
                      int32_t* hyp_count, double* timing);

}  // namespace sfmba
