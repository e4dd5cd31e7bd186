// tsdf_mesh.h -- a truncated signed distance grid from depth maps and its surface by marching tetrahedra, behind
// sfmba_tsdf_integrate / sfmba_tsdf_extract / sfmba_tsdf_mesh (tsdf_mesh.hip; arithmetic in mesh_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h, and
constexpr int TSDF_ERR_GRID = -16;          // the grid handed to the extraction breaks its bounds (found on the device; nothing was written)

// images of the table a workgroup of the integration keeps in LDS at a time
constexpr int TSDF_TABLE_CHUNK = 64;

// phases of the timing array
enum { TSDF_T_UPLOAD = 0, TSDF_T_INTEGRATE, TSDF_T_CHECK, TSDF_T_COUNT_TRI, TSDF_T_SCAN, TSDF_T_FLAGS, TSDF_T_EMIT, TSDF_T_VERTICES, TSDF_T_DOWNLOAD,
       TSDF_T_COUNT };

struct TsdfGrid {
    const float* origin;     // [3]
    float voxel;
    int nx, ny, nz;
};
// the images of an integration, as sfmba_depth_fuse takes them; pixels may be NULL (img_ptr and channels are then not read)
struct TsdfViews {
    int n_images;
    const int64_t* img_ptr;
    const unsigned char* pixels;
    const int32_t *width, *height;
    int channels;
    const float *K, *P;
    const float* const* depth;
    float trunc;
};
// the outputs of an extraction (bgr is written only where the grid has colour sums)
struct TsdfMeshOut {
    float* xyz;
    unsigned char* bgr;
    int32_t* vkey;
    int64_t vcap;
    int32_t* tri;
    int64_t tcap;
    int64_t *n_vertices, *n_triangles;
};

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// [TSDF_T_COUNT] = HIP-event milliseconds on `s` of the phases above; a call leaves the phases it does not run at 0.
// colour: csum and cweight are written (both given) or left alone (both NULL, or views.pixels NULL).
int tsdf_integrate(hipStream_t s, int device, const TsdfViews& views, const TsdfGrid& grid, int32_t* sum, int32_t* weight, int32_t* csum,
                   int32_t* cweight, double* timing);
int tsdf_extract(hipStream_t s, int device, const TsdfGrid& grid, const int32_t* sum, const int32_t* weight, const int32_t* csum,
                 const int32_t* cweight, int min_weight, const TsdfMeshOut& out, double* timing);
// integrate, then extract, the grid never leaving the device; colour iff views.pixels is given
int tsdf_mesh(hipStream_t s, int device, const TsdfViews& views, const TsdfGrid& grid, int min_weight, const TsdfMeshOut& out, double* timing);

}  // namespace sfmba
