// tsdf_mesh.h -- a truncated signed distance grid from depth maps and its surface by marching tetrahedra, behind
// sfmba_tsdf_integrate / sfmba_tsdf_extract / sfmba_tsdf_mesh (tsdf_mesh.hip; arithmetic in mesh_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_arena.h"
#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h, and
constexpr int TSDF_ERR_GRID = -16;          // the grid handed to the extraction breaks its bounds (found on the device; nothing was written)

// images of the table a workgroup of the integration keeps in LDS at a time
constexpr int TSDF_TABLE_CHUNK = 64;

// phases of the timing array
enum { TSDF_T_UPLOAD = 0, TSDF_T_INTEGRATE, TSDF_T_CHECK, TSDF_T_COUNT_TRI, TSDF_T_SCAN, TSDF_T_FLAGS, TSDF_T_EMIT, TSDF_T_VERTICES, TSDF_T_DOWNLOAD,
       TSDF_T_FILL,          // the hole filling of tsdf_fill.hip (0 in the three calls of tsdf_mesh.hip)
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
    unsigned char* vfilled = nullptr;    // [vcap] or NULL: sfmba_tsdf_mesh_fill only
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


// ---- the pieces on a DEVICE-RESIDENT grid, for tsdf_fill.hip: one copy of the validation, the integration and the extraction ----------
struct TsdfGridDev {
    double origin[3];
    double voxel;
    int nx, ny, nz, nvox;
};
struct TsdfGridArrays { int *sum, *weight, *csum, *cweight; };       // device pointers; csum and cweight NULL without colour

TsdfGridDev tsdf_grid_dev(const TsdfGrid& grid);
int tsdf_alloc_grid(DeviceArena& scratch, const TsdfGridDev& g, bool colour, TsdfGridArrays& a);
void tsdf_zero_timing(double* timing);
// *d_bad (zeroed by the caller) becomes 1 iff the grid breaks the bounds an integration guarantees; enqueued on s
int tsdf_check_device(hipStream_t s, const TsdfGridDev& g, const TsdfGridArrays& a, int* d_bad);
int tsdf_integrate_device(hipStream_t s, DeviceArena& scratch, PhaseTimer& tm, const TsdfViews& v, const TsdfGridDev& g, bool colour,
                          const TsdfGridArrays& a);
// check: hold the grid to its bounds first.  fill_state (device, [nvox], or NULL): the state bytes of a hole filling, from which
// out.vfilled is made; with out.vfilled given and fill_state NULL it is zeroed.
int tsdf_extract_device(hipStream_t s, DeviceArena& scratch, PhaseTimer& tm, const TsdfGridDev& g, const TsdfGridArrays& a, int min_weight, bool check,
                        const TsdfMeshOut& out, const unsigned char* fill_state);

}  // namespace sfmba
