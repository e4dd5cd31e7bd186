// mesh_texture.h -- a view per triangle and a texture atlas of fixed-size patches for a triangle mesh, behind sfmba_mesh_texture
// (mesh_texture.hip; arithmetic in texture_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "texture_math.h"
#include "unit_common.h"

#include "../../include/sfmba.h"

namespace sfmba {

// return values besides 0 (ok) and positive hipError_t codes: UNIT_ERR_* of unit_common.h, and
constexpr int TEX_ERR_INDEX = -19;          // a triangle index lies outside the vertex list (found on the device; nothing was written)
constexpr int TEX_ERR_VIEW = -20;           // a given view label lies outside -1 .. n_images-1 (found on the device; nothing was written)

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

// how the labels of a call come about when it is not the plain largest-score rule (mesh_labels.h): GIVEN (view_in, the device holds
// them to -1 .. n_images-1) or SMOOTHED (candidates, adjacency, diffusion and relaxation, everything staying on the device)
struct TexLabels {
    const int32_t* view_in;       // [nt]: the labels are given; out.view and out.score are not written
    int K, rings, penalty, max_passes;      // view_in == NULL: the smoothing
    int64_t* stats;               // [LABEL_STATS] of the smoothing
    double* timing;               // [LAB_T_COUNT] of the smoothing's phases (mesh_labels.h), or NULL
};

// the levelling of the colours across seams (mesh_colour.h), off unless a caller asks: the offsets are GIVEN (node_of_in, g_in) or come
// from nodes, colours and passes on the call's final labels, everything staying on the device
struct TexLevel {
    const int32_t* node_of_in;    // [nt][3], each row -1 -1 -1 or nodes in 0 .. n_nodes-1: the offsets are given
    const int32_t* g_in;          // [n_nodes][3] in 1/256 grey level
    int n_nodes;
    int radius, weight, passes;   // node_of_in == NULL: the sample radius of the node colours, the seam weight, the Jacobi passes
    int64_t* stats;               // [COLOUR_STATS] (colour_math.h), or NULL
    int64_t* n_clamped;           // the texels whose clamp changed a channel, or NULL
    double* timing;               // [COL_T_COUNT] of the levelling's phases (mesh_colour.h), or NULL
};

// one view and the parameters as the kernels of mesh_texture.hip and mesh_labels.hip take them
struct TexImage {
    double P[12];
    long long map_off;       // first float of its depth map among the maps on the device, -1 without a map
    long long raw_off;       // first byte of its pixels among the pixels on the device
    int w, h;
    long long pad;           // 128 bytes
};
static_assert(sizeof(TexImage) == 128, "TexImage is 16 words");

struct TexKernelParams {
    double k4[4];
    double occl_tol;
    long long min_area;
    int nv, nt, n_images, channels;
    int S, B, W, H;          // B: blocks per row of the atlas as laid out (1 for an empty mesh)
    int slots, group;        // block slots of the atlas (rows x B), blocks per workgroup of the raster
};

__device__ __forceinline__ TexView view_of(const TexImage& T, const float* __restrict__ maps, const unsigned char* __restrict__ raw) {
    return TexView{ T.P, T.map_off >= 0 ? maps + T.map_off : nullptr, raw + T.raw_off, T.w, T.h };
}
__device__ __forceinline__ void load_vertex(const float* __restrict__ xyz, int v, double* X) {
    for (int a = 0; a < 3; ++a) X[a] = (double)xyz[3 * (size_t)v + a];
}

// pieces of mesh_texture that the label calls share (mesh_labels.hip): the view table with its map and pixel offsets, the camera part of
// the kernel parameters, and the index check (enqueue only; raises d_flag[0])
void tex_view_table(const TexViews& v, std::vector<TexImage>& tab, long long& n_map, long long& n_raw);
void tex_camera_params(const TexViews& v, float occl_tol, int64_t min_area, TexKernelParams& prm);
int tex_check_indices(hipStream_t s, int nt, int nv, const int* d_tri, int* d_flag);

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing (may be NULL):
// [TEX_T_COUNT] = HIP-event milliseconds on `s` of the phases above.
int mesh_texture(hipStream_t s, int device, const TexMesh& m, const TexViews& v, const TexParams& p, const TexOut& out, double* timing,
                 const TexLabels* labels = nullptr, const TexLevel* level = nullptr);

}  // namespace sfmba
