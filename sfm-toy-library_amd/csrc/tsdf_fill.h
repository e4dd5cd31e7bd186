// tsdf_fill.h -- hole filling by volumetric diffusion of the signed distance into the undefined vertices of a TSDF grid, behind
// sfmba_tsdf_fill / sfmba_tsdf_mesh_fill (tsdf_fill.hip; arithmetic in tsdf_fill_math.h; the grid, its validation, the integration
// and the extraction are tsdf_mesh.hip's).
#pragma once
#include "tsdf_mesh.h"

namespace sfmba {

struct TsdfFillParams { int min_weight, iterations, min_neighbours; };

// Host pointers in and out; arguments already validated (see include/sfmba.h for the contract).  timing as in tsdf_mesh.h;
// the passes and the write-back go to TSDF_T_FILL.  TSDF_ERR_GRID: the grid breaks its bounds, nothing was written.
int tsdf_fill(hipStream_t s, int device, int nx, int ny, int nz, const int32_t* sum, const int32_t* weight, const int32_t* csum, const int32_t* cweight,
              const TsdfFillParams& prm, int32_t* sum_out, int32_t* weight_out, int32_t* csum_out, int32_t* cweight_out, unsigned char* state,
              int64_t* n_filled, double* timing);
// integrate, fill, extract, the grid never leaving the device; colour iff views.pixels is given; out.vfilled may be given
int tsdf_mesh_fill(hipStream_t s, int device, const TsdfViews& views, const TsdfGrid& grid, const TsdfFillParams& prm, const TsdfMeshOut& out,
                   double* timing);

}  // namespace sfmba
