// depth_sweep.h -- batched plane-sweep stereo and the consistency filter behind sfmba_depth_sweep / sfmba_depth_fuse
// (depth_sweep.hip; arithmetic in depth_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h

// Jobs go to the device in consecutive groups.  A group's arrays (the pixels of the images its jobs name, their gray planes, the
// three output maps) stay within this bound; a job that exceeds it alone forms a group of its own.
constexpr size_t DEPTH_SCRATCH_BYTES = (size_t)512 << 20;
constexpr int DEPTH_MAX_GROUP_JOBS = 4096;     // grid.y of the sweep

// phases of the timing arrays
enum { DEPTH_T_UPLOAD = 0, DEPTH_T_GRAY, DEPTH_T_SWEEP, DEPTH_T_DOWNLOAD, DEPTH_T_GROUPS, DEPTH_T_COUNT };
enum { FUSE_T_UPLOAD = 0, FUSE_T_FLAG, FUSE_T_SCAN, FUSE_T_EMIT, FUSE_T_DOWNLOAD, FUSE_T_COUNT };

// What the units behind sfmba_depth_cost_volume / sfmba_depth_sweep_sgm (depth_sgm.hip) see of one group when the sweep stores its
// cost volume instead of choosing a winner: the group's jobs and its device arrays, all on the sweep's stream.
struct DepthCostJob { int w, h; long long px_off; double wf, step; };   // px_off: the job's first pixel in the group's arrays
class DeviceArena;
struct DepthCostGroup {
    int first_job, n_jobs, D;
    const DepthCostJob* jobs;        // host, [n_jobs]
    long long first_px, n_px;        // the group's pixels in the call's concatenated outputs
    const unsigned char* d_cost;     // [n_px][D], as sfmba_depth_cost_volume defines it
    float *d_depth, *d_score;        // [n_px]: filled by a sink with `maps`, downloaded by the sweep
    int16_t* d_plane;
};
struct DepthCostSink {
    int extra_bytes_per_entry = 0;   // device bytes the sink needs per volume entry besides the entry itself (the scratch bound counts them)
    bool maps = false;               // the sink fills the three maps of the group
    virtual int group(hipStream_t s, DeviceArena& scratch, const DepthCostGroup& g) = 0;
    virtual ~DepthCostSink() = default;
};

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// [DEPTH_T_COUNT] = HIP-event milliseconds on `s` summed over groups -- upload, gray kernel, sweep kernel, download -- then the
// number of groups.  sink = NULL: sfmba_depth_sweep.  Otherwise the sweep kernel's other instantiation stores the quantised cost of
// every (pixel, plane) (`invalid_cost` is not read by it), the sink is handed every group, and min_score is not read.
int depth_sweep(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
                const int32_t* height, int channels, const float* K, const float* P, int n_jobs, const int32_t* job_ref,
                const int64_t* job_src_ptr, const int32_t* job_src, const float* z_near, const float* z_far, int n_planes, int radius,
                int min_std, float min_score, int min_sources, float* depth, float* score, int16_t* plane, double* timing,
                DepthCostSink* sink = nullptr);

// timing (may be NULL): [FUSE_T_COUNT] = milliseconds of upload, flag kernel, scan, emit kernel, download.
int depth_fuse(hipStream_t s, int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
               const int32_t* height, int channels, const float* K, const float* P, const float* const* depth, const int64_t* chk_ptr,
               const int32_t* chk, float rel_tol, int min_consistent, int64_t* pt_ptr, float* xyz, unsigned char* bgr, int32_t* src_image,
               int32_t* src_pixel, int64_t cap, int64_t* total, double* timing);

}  // namespace sfmba
