// pnp_ransac.h -- batched P3P RANSAC + Gauss-Newton refinement behind sfmba_pnp_ransac (pnp_ransac.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h

constexpr int PNP_TILE = 64;                 // hypotheses per score block: one per lane of a wave
constexpr int PNP_CHUNK = 1024;              // points a score block stages in LDS at a time (20 B each)
constexpr int PNP_SCORE_THREADS = 256;       // 4 waves share the tile's 64 hypotheses and interleave the chunk's points
constexpr int PNP_MAX_CHUNK_BLOCKS = 64;     // grid.y of the score kernel, at most: a block then walks several chunks
constexpr int PNP_REFINE_THREADS = 256;      // select + refine: one block per problem

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// { upload ms, the three kernels ms, download ms } from HIP events on `s`.
int pnp_ransac(hipStream_t s, int device, int n_prob, const int64_t* prob_ptr, const float* xyz, const float* uv, const float* K,
               int n_hyp, float threshold_px, uint64_t seed, int max_refine_iters, double* pose, unsigned char* inlier,
               sfmba_pnp_result* result, double* hyp_pose, int32_t* hyp_count, double* timing);

}  // namespace sfmba
