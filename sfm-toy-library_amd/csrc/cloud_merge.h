// cloud_merge.h -- a normal per depth pixel and the voxel merge of a dense cloud, behind sfmba_depth_normals / sfmba_cloud_merge
// (cloud_merge.hip; arithmetic in cloud_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h

// a run of the sorted order with more members than this is reduced by a whole wave, a shorter one by a single lane
constexpr int CLOUD_SHORT_RUN = 32;

// phases of the timing arrays
enum { NORMALS_T_UPLOAD = 0, NORMALS_T_KERNEL, NORMALS_T_DOWNLOAD, NORMALS_T_COUNT };
enum { MERGE_T_UPLOAD = 0, MERGE_T_QUANTISE, MERGE_T_SORT, MERGE_T_RUNS, MERGE_T_REDUCE, MERGE_T_COMPACT, MERGE_T_FINALISE, MERGE_T_DOWNLOAD,
       MERGE_T_COUNT };

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// [NORMALS_T_COUNT] = HIP-event milliseconds on `s` of upload, kernel, download.
int depth_normals(hipStream_t s, int device, int n_images, const int32_t* width, const int32_t* height, const float* K, const float* P,
                  const float* const* depth, float max_rel_step, float* const* normal, double* timing);

// timing (may be NULL): [MERGE_T_COUNT] = milliseconds of upload, quantise kernel, sort, head flags + scan + run starts, the two
// reduction kernels, flags + scan + voxel_of, finalise kernel, download.
int cloud_merge(hipStream_t s, int device, int n, const float* xyz, const unsigned char* bgr, const float* normal, float voxel, int min_count,
                float* xyz_out, unsigned char* bgr_out, float* normal_out, int32_t* count, int32_t* first, int32_t* voxel_of, int64_t cap,
                int64_t* total, int64_t* n_skipped, double* timing);

}  // namespace sfmba
