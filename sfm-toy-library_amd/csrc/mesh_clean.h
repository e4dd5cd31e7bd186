// mesh_clean.h -- connected components, small-island removal, Taubin smoothing in integers and vertex normals of a triangle mesh,
// behind sfmba_mesh_components / sfmba_mesh_filter / sfmba_mesh_smooth / sfmba_mesh_clean (mesh_clean.hip; arithmetic in
// mesh_clean_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h, and
constexpr int CLEAN_ERR_INDEX = -17;        // a triangle index lies outside the vertex list (found on the device; nothing was written)
constexpr int CLEAN_ERR_COORD = -18;        // a coordinate is not finite or quantises to |P| >= 2^25 (found on the device; nothing was written)

// phases of the timing array
enum { CLEAN_T_UPLOAD = 0, CLEAN_T_CHECK, CLEAN_T_COMPONENTS, CLEAN_T_FILTER, CLEAN_T_QUANTISE, CLEAN_T_SMOOTH, CLEAN_T_NORMALS, CLEAN_T_DOWNLOAD,
       CLEAN_T_COUNT };

struct CleanMesh {
    int nv, nt;
    const float* xyz;             // [nv][3]
    const unsigned char* bgr;     // [nv][3] or NULL
    const int32_t* tri;           // [nt][3]
};
struct CleanFilterParams { int min_triangles, keep_largest; };
// origin and quantum as doubles of the floats given; L and M are the quantised factors (clean_factor)
struct CleanSmoothParams { double origin[3], quantum; int iterations, L, M; };
struct CleanFilterOut {
    float* xyz;
    unsigned char* bgr;
    float* normal;                // sfmba_mesh_clean only
    int64_t vcap;
    int32_t* tri;
    int64_t tcap;
    int32_t* vertex_of;
    int64_t *n_vertices, *n_triangles;
};

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// [CLEAN_T_COUNT] = HIP-event milliseconds on `s` of the phases above; a call leaves the phases it does not run at 0.
int mesh_components(hipStream_t s, int device, const CleanMesh& m, int32_t* label, int32_t* comp_triangles, int64_t* n_components, int64_t* largest,
                    double* timing);
int mesh_filter(hipStream_t s, int device, const CleanMesh& m, const CleanFilterParams& f, const CleanFilterOut& out, double* timing);
int mesh_smooth(hipStream_t s, int device, const CleanMesh& m, const CleanSmoothParams& p, float* xyz_out, float* normal, double* timing);
// filter, then smooth, the mesh never leaving the device
int mesh_clean(hipStream_t s, int device, const CleanMesh& m, const CleanFilterParams& f, const CleanSmoothParams& p, const CleanFilterOut& out,
               double* timing);

}  // namespace sfmba
