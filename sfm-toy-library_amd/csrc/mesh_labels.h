// mesh_labels.h -- smoothing the view labels of a textured mesh: the K best views per triangle, the triangle adjacency, score diffusion
// and a parallel Potts relaxation, behind sfmba_mesh_view_candidates / _adjacency / _view_smooth and, through mesh_texture.hip,
// sfmba_mesh_texture_smooth (mesh_labels.hip; the rules are in label_math.h, the contract in include/sfmba.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_arena.h"
#include "label_math.h"
#include "mesh_texture.h"
#include "unit_common.h"

namespace sfmba {

// phases of the timing array of the three calls and of the smoothing inside mesh_texture
enum { LAB_T_UPLOAD = 0, LAB_T_CANDIDATES, LAB_T_KEYS, LAB_T_SORT, LAB_T_LINK, LAB_T_RINGS, LAB_T_START, LAB_T_GAIN, LAB_T_MOVE, LAB_T_STATS,
       LAB_T_DOWNLOAD, LAB_T_COUNT };

struct LabelParams { int K, rings, penalty, max_passes; };

// ---- on device arrays (mesh_texture.hip calls these between its view kernel and its raster) -----------------------------------------
// Enqueue only.  flag: the index flag of k_tex_check (nothing is read when it is set).  cand_view [nt][K], cand_score [nt][K].
int labels_candidates_dev(hipStream_t s, const TexKernelParams& prm, const int* d_flag, const float* d_xyz, const int* d_tri, const TexImage* d_tab,
                          const float* d_maps, const unsigned char* d_raw, int K, int* d_cand_view, long long* d_cand_score);
// Enqueue only; temporaries from `raw`, which the caller keeps until the stream has drained.  `raw` here and below is an arena that
// does NOT zero what it hands out (set_zeroing(false)): every array taken from it is written in full before it is read, and a zeroing
// arena would clear each new chunk whole and wait for it.  d_tri holds indices >= 0.
// d_counts [3]: pairs, open edges, non-manifold edges (zero on entry).
int labels_adjacency_dev(hipStream_t s, DeviceArena& raw, int nt, const int* d_tri, int* d_adj, unsigned long long* d_counts, PhaseTimer* tm);
// Waits for the stream (the mover counts come back in batches of passes).  d_view [nt] and d_score [nt] (or NULL: the original score of
// the final label) are written; stats is a HOST array [LABEL_STATS].  The counters come from `scratch` (zeroed), the rest from `raw`.
int labels_smooth_dev(hipStream_t s, DeviceArena& scratch, DeviceArena& raw, int nt, const LabelParams& p, const int* d_cand_view, const long long* d_cand_score,
                      const int* d_adj, int* d_view, long long* d_score, int64_t* stats, PhaseTimer* tm);

// ---- host pointers in and out; arguments already validated ---------------------------------------------------------------------------
// returns 0, TEX_ERR_INDEX, a UNIT_ERR_* or a hipError_t; timing (may be NULL): [LAB_T_COUNT] HIP-event milliseconds
int mesh_view_candidates(hipStream_t s, int device, const TexMesh& m, const TexViews& v, float occl_tol, int64_t min_area, int K, int32_t* cand_view,
                         int64_t* cand_score, double* timing);
int mesh_adjacency(hipStream_t s, int device, int nt, const int32_t* tri, int32_t* adj, int64_t* counts /*[3]*/, double* timing);
int mesh_view_smooth(hipStream_t s, int device, int nt, const LabelParams& p, const int32_t* cand_view, const int64_t* cand_score, const int32_t* adj,
                     int32_t* view, int64_t* stats, double* timing);

}  // namespace sfmba
