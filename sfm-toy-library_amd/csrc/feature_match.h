// feature_match.h -- brute-force Hamming 2-NN + ratio test behind sfmba_match_features (feature_match.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unit_common.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h

// Scratch for the per-slice top-2 keys of one batch (8 bytes per query row and slice): the pair list is cut into batches of
// query tiles so that this bound holds whatever the number of pairs (feature matching).
constexpr size_t MATCH_SCRATCH_BYTES = (size_t)64 << 20;
constexpr int MATCH_TILE = 512;              // query rows per block: 256 lanes x 2 queries
constexpr int MATCH_MAX_SLICES = 32;         // train slices per query tile, at most
constexpr int MATCH_MIN_SLICE_ROWS = 256;    // a slice is not made shorter than this many train rows (when the image has them)
constexpr int MATCH_TARGET_BLOCKS = 4096;    // slices are added until a batch launches about this many blocks
constexpr int MATCH_BATCH_TILES = (int)(MATCH_SCRATCH_BYTES / (8 * (size_t)MATCH_MAX_SLICES * MATCH_TILE));

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// { upload ms, top-2 + merge kernels ms, compaction ms, download ms, batches } from HIP events on `s`.
int match_features(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* desc, int desc_bytes,
                   int n_pairs, const int32_t* pair_left, const int32_t* pair_right, double ratio, int64_t* pair_ptr,
                   int32_t* query_idx, int32_t* train_idx, float* distance, int64_t cap, int64_t* total, double* timing);

}  // namespace sfmba
