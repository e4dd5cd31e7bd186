// mesh_colour.h -- levelling the colours across the seams of a textured mesh: a node per (vertex, view), its colour in the photograph, and
// additive per-node offsets by integer Jacobi passes, behind sfmba_mesh_colour_nodes / _colour_level and, through mesh_texture.hip,
// sfmba_mesh_texture_levelled / _adjust (mesh_colour.hip; the rules are in colour_math.h, the contract in include/sfmba.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "colour_math.h"
#include "device_arena.h"
#include "mesh_texture.h"
#include "unit_common.h"

namespace sfmba {

// phases of the levelling's timing array
enum { COL_T_KEYS = 0, COL_T_SORT, COL_T_NODES, COL_T_COLOURS, COL_T_PASSES, COL_T_STATS, COL_T_COUNT };

// the nodes of a mesh on the device.  F and the offsets are 16-byte records: x, y, z the three channels, w the node's `seen`.
struct ColourNodes {
    int* node_of = nullptr;        // [nt][3]
    int* node_vertex = nullptr;    // [3 nt], the first n_nodes written
    int* node_view = nullptr;      // [3 nt], likewise
    int4* F = nullptr;             // [3 nt], likewise
    int* entry = nullptr;          // [3 nt]: the entries 3 t + q in node order; node n owns entry[run[n] .. run[n + 1])
    int* run = nullptr;            // [3 nt + 1]
};

// ---- on device arrays (mesh_texture.hip calls these between its labels and its raster) ------------------------------------------------
// d_tri holds indices inside the vertex list and d_view labels in -1 .. n_images-1: the caller has read the flags of its checks.
// Temporaries from `raw`, an arena that does not zero (mesh_labels.h).  Waits for the stream once, for n_nodes.
int colour_nodes_dev(hipStream_t s, DeviceArena& raw, const TexKernelParams& prm, const float* d_xyz, const int* d_tri, const TexImage* d_tab,
                     const unsigned char* d_raw, const int* d_view, int radius, ColourNodes& out, int& n_nodes, PhaseTimer* tm);
// N Jacobi passes, no wait between them; waits once at the end for the statistics.  *d_g: [n_nodes] records (NULL without a node).
// stats is a HOST array [COLOUR_STATS]; [COLOUR_S_CLAMPED] is left 0.
int colour_level_dev(hipStream_t s, DeviceArena& raw, int n_nodes, const int* d_node_vertex, const int4* d_F, const int* d_node_of, const int* d_entry,
                     const int* d_run, int weight, int passes, const int4** d_g, int64_t* stats, PhaseTimer* tm);

// ---- host pointers in and out; arguments already validated ---------------------------------------------------------------------------
// returns 0, TEX_ERR_INDEX, TEX_ERR_VIEW, a UNIT_ERR_* or a hipError_t
int mesh_colour_nodes(hipStream_t s, int device, const TexMesh& m, const TexViews& v, const int32_t* view, int radius, int64_t* n_nodes,
                      int32_t* node_vertex, int32_t* node_view, int32_t* node_of, unsigned char* seen, int32_t* F);
int mesh_colour_level(hipStream_t s, int device, int n_nodes, const int32_t* node_vertex, const unsigned char* seen, const int32_t* F, int nt,
                      const int32_t* node_of, int weight, int passes, int32_t* g, int64_t* stats);

}  // namespace sfmba
