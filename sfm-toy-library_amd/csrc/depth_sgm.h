// depth_sgm.h -- semi-global matching over the sweep's cost volume, behind sfmba_depth_cost_volume / sfmba_sgm_aggregate /
// sfmba_depth_sweep_sgm (depth_sgm.hip; arithmetic in sgm_math.h; the volume itself is stored by depth_sweep.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "depth_sweep.h"
#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// phases of the timing array: the three kernels of the aggregation, HIP-event milliseconds summed over groups; the aggregation also
// per direction (SGM_T_PATH0 + i, in the contract's order)
enum { SGM_T_AGGREGATE = 0, SGM_T_SELECT, SGM_T_FINISH, SGM_T_PATH0, SGM_T_COUNT = SGM_T_PATH0 + 8 };

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  The first and the last are
// depth_sweep() with a sink: sweep_timing is its array [DEPTH_T_COUNT], sgm_timing [SGM_T_COUNT]; both may be NULL.
int depth_cost_volume(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
                      const int32_t* height, int channels, const float* K, const float* P, int n_jobs, const int32_t* job_ref,
                      const int64_t* job_src_ptr, const int32_t* job_src, const float* z_near, const float* z_far, int n_planes, int radius,
                      int min_std, int min_sources, unsigned char* cost, double* sweep_timing);

int sgm_aggregate(hipStream_t s, int device, int n_jobs, const unsigned char* const* cost, const int32_t* width, const int32_t* height, int D,
                  int p1, int p2, int n_paths, int invalid_cost, int16_t* const* plane, uint16_t* const* best, uint16_t* const* second,
                  uint16_t* const* sums, double* sgm_timing);

int depth_sweep_sgm(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
                    const int32_t* height, int channels, const float* K, const float* P, int n_jobs, const int32_t* job_ref,
                    const int64_t* job_src_ptr, const int32_t* job_src, const float* z_near, const float* z_far, int n_planes, int radius,
                    int min_std, int min_sources, int p1, int p2, int n_paths, int invalid_cost, int uniqueness, float* depth, float* score,
                    int16_t* plane, double* sweep_timing, double* sgm_timing);

}  // namespace sfmba
