// mesh_texture.h -- a view per triangle and a texture atlas of fixed-size patches for a triangle mesh, behind sfmba_mesh_texture
// (mesh_texture.hip; arithmetic in texture_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h, and
constexpr int TEX_ERR_INDEX = -19;          // a triangle index lies outside the vertex list (found on the device; nothing was written)

// phases of the timing array
enum { TEX_T_UPLOAD = 0, TEX_T_CHECK, TEX_T_VIEWS, TEX_T_RASTER, TEX_T_DOWNLOAD, TEX_T_COUNT };

struct TexMesh {
    int nv, nt;
    const float* xyz;             // [nv][3]
    const unsigned char* bgr;     // [nv][3] or NULL
    const int32_t* tri;           // [nt][3]
};
// the images as sfmba_depth_fuse takes them; depth[i] may be NULL
struct TexViews {
    int n_images;
    const int64_t* img_ptr;
    const unsigned char* pixels;
    const int32_t *width, *height;
    int channels;
    const float *K, *P;
    const float* const* depth;
};
struct TexParams {
    float occl_tol;
    int64_t min_area;
    int patch, blocks_per_row;    // S, B
    int W, H;                     // of the atlas (tex_atlas_size)
};
struct TexOut {
    unsigned char* atlas;         // [H][W][3]
    float* uv;                    // [nt][3][2]
    int32_t* view;                // [nt]
    int64_t* score;               // [nt] or NULL
    int64_t* n_textured;
};

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// [TEX_T_COUNT] = HIP-event milliseconds on `s` of the phases above.
int mesh_texture(hipStream_t s, int device, const TexMesh& m, const TexViews& v, const TexParams& p, const TexOut& out, double* timing);

}  // namespace sfmba
