// ba_eval.hip -- outside the LM iteration: the kernel-level entry points of the parity tests and debug tools (C ABI: sfmba_problem_eval_*,
// sfmba_problem_build_reduced).
//   reads   camtab[cur], pts[cur], the observations; the reduced system a linearisation left in S
//   leaves  residuals / cost, the Jacobian blocks per observation, a full symmetric unpadded copy of S with the scale vector -- in caller buffers
#include "ba_common.h"

namespace sfmba {

// ------------------------------------------------------------------------------------------
// kernel-level entry points used by the parity tests (C ABI: sfmba_problem_eval_*)
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(BLK) void k_eval_residuals(DeviceStructure ds, DeviceBuffers db, const int* __restrict__ obs_pt,
                                                        const int* __restrict__ perm, double* __restrict__ res_out, double* cost_out) {
    __shared__ double scratch[BLK / 64];
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const int cur = db.st->cur;
    double c = 0.0;
    if (q < ds.nobs) {
        const int i = obs_pt[q];
        const CamRow ct = { db.camtab[cur] + 4 * (size_t)(ds.obs_cam[q]), ds.ncam };
        const double X[3] = { db.pts[cur][3 * i], db.pts[cur][3 * i + 1], db.pts[cur][3 * i + 2] };
        double ox, oy;
        load_obs<T>(ds.obs_xy, q, ox, oy);
        const Proj pr = project_point(ct, CT_R, CT_T, X);
        const double f = db.st->focal[cur];
        const double r0 = f * pr.xp - ox, r1 = f * pr.yp - oy;
        if (res_out) { res_out[2 * (size_t)perm[q]] = r0; res_out[2 * (size_t)perm[q] + 1] = r1; }
        c = r0 * r0 + r1 * r1;
    }
    c = block_sum(c, scratch);
    if (threadIdx.x == 0 && cost_out) atomicAdd(cost_out, 0.5 * c);
}

template <typename T>
__global__ __launch_bounds__(BLK) void k_eval_jacobian(DeviceStructure ds, DeviceBuffers db, const int* __restrict__ obs_pt,
                                                       const int* __restrict__ perm, double* jc, double* jp, double* jf) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ds.nobs) return;
    const int cur = db.st->cur;
    const int i = obs_pt[q];
    const CamRow ct = { db.camtab[cur] + 4 * (size_t)(ds.obs_cam[q]), ds.ncam };
    const double X[3] = { db.pts[cur][3 * i], db.pts[cur][3 * i + 1], db.pts[cur][3 * i + 2] };
    const Proj pr = project_point(ct, CT_R, CT_T, X);
    const double f = db.st->focal[cur];
    T B[6], A[12];
    point_block<T>(ct, pr, f, B);
    camera_block<T>(ct, pr, f, X, B, A);
    const size_t k = (size_t)perm[q];
    if (jc) for (int e = 0; e < 12; ++e) jc[12 * k + e] = (double)A[e];
    if (jp) for (int e = 0; e < 6; ++e) jp[6 * k + e] = (double)B[e];
    if (jf) { jf[2 * k] = pr.xp; jf[2 * k + 1] = pr.yp; }
}

template <typename T>
void launch_eval_residuals(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db, const int* obs_pt_and_perm,
                           double* res_out, double* cost_out) {
    // obs_pt_and_perm: [2*nobs] = point slot per point-major obs, then perm (point-major position -> caller index)
    hipLaunchKernelGGL(k_eval_residuals<T>, dim3((ds.nobs + BLK - 1) / BLK), dim3(BLK), 0, s, ds, db,
                       obs_pt_and_perm, obs_pt_and_perm + ds.nobs, res_out, cost_out);
}
template void launch_eval_residuals<float>(hipStream_t, const DeviceStructure&, const DeviceBuffers&, const int*, double*, double*);
template void launch_eval_residuals<double>(hipStream_t, const DeviceStructure&, const DeviceBuffers&, const int*, double*, double*);

template <typename T>
void launch_eval_jacobian(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db, const int* obs_pt, const int* perm,
                          double* jc, double* jp, double* jf) {
    hipLaunchKernelGGL(k_eval_jacobian<T>, dim3((ds.nobs + BLK - 1) / BLK), dim3(BLK), 0, s, ds, db, obs_pt, perm, jc, jp, jf);
}
template void launch_eval_jacobian<float>(hipStream_t, const DeviceStructure&, const DeviceBuffers&, const int*, const int*, double*, double*, double*);
template void launch_eval_jacobian<double>(hipStream_t, const DeviceStructure&, const DeviceBuffers&, const int*, const int*, double*, double*, double*);

// full symmetric unpadded copy of the reduced system + the scale vector (sfmba_problem_build_reduced)
__global__ void k_mirror_scale(DeviceStructure ds, DeviceBuffers db, double* S_full, double* scale_out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (c >= ds.d || r >= ds.d) return;
    const double v = c >= r ? db.S[(size_t)r * ds.ld + c] : db.S[(size_t)c * ds.ld + r];
    S_full[(size_t)r * ds.d + c] = v;
    if (r == 0 && scale_out) scale_out[c] = c < ds.d - 1 ? db.cscale[c] : db.st->fscale;
}

void launch_mirror_scale(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db, double* S_full, double* scale_out) {
    hipLaunchKernelGGL(k_mirror_scale, dim3((ds.d + 255) / 256, ds.d), dim3(256), 0, s, ds, db, S_full, scale_out);
}

}  // namespace sfmba
