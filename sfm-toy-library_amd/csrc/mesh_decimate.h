// mesh_decimate.h -- vertex clustering with quadric placement of a triangle mesh, behind sfmba_mesh_decimate (mesh_decimate.hip;
// arithmetic in decimate_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_clean.h"      // CleanMesh, CLEAN_ERR_INDEX, CLEAN_ERR_COORD

namespace sfmba {

// phases of the timing array
enum { DEC_T_UPLOAD = 0, DEC_T_KEYS, DEC_T_SORT, DEC_T_RUNS, DEC_T_MEMBERS, DEC_T_QUADRICS, DEC_T_SOLVE, DEC_T_MAP, DEC_T_DEDUP, DEC_T_COMPACT,
       DEC_T_EMIT, DEC_T_DOWNLOAD, DEC_T_COUNT };

// origin and quantum as doubles of the floats given
struct DecimateParams { double origin[3], quantum; int cell, placement, reg; };
struct DecimateOut {
    float* xyz;
    unsigned char* bgr;
    int32_t* members;             // or NULL
    int64_t vcap;
    int32_t* tri;
    int32_t* triangle_of;         // or NULL
    int64_t tcap;
    int32_t* vertex_of;           // or NULL
    int64_t *n_vertices, *n_triangles;
    int64_t* stats;               // [4] or NULL
};

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  Returns 0, UNIT_ERR_CAPACITY (the
// totals valid, nothing else written), CLEAN_ERR_INDEX / CLEAN_ERR_COORD (nothing written) or a positive hipError_t.  timing (may be
// NULL): [DEC_T_COUNT] = HIP-event milliseconds on `s` of the phases above.
int mesh_decimate(hipStream_t s, int device, const CleanMesh& m, const DecimateParams& p, const DecimateOut& out, double* timing);

}  // namespace sfmba
