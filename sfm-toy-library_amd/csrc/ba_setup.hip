// ba_setup.hip -- what runs once per solve, in front of the first LM iteration: the per-camera tables, the clearing first launch, ||x|| of
// the starting point and the Jacobi column scaling.
//   reads   the camera / point parameters of the current buffer (or the initial ones behind a pending reset), the LM state as an argument
//   leaves  camtab[cur], cscale / pscale / fscale, x_norm, cleared slots, status words and column-norm accumulators
// Every later pass (ba_points.hip onwards) starts from the camera table this unit builds (make_cam_table, ba_common.h).
#include "ba_common.h"
#include <algorithm>

namespace sfmba {

__global__ void k_cam_setup(int ncam, const double* __restrict__ cam, const double* __restrict__ cscale, double* __restrict__ camtab) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ncam) return;
    double c6[6], ct[CT_STRIDE];
    for (int e = 0; e < 6; ++e) c6[e] = cam[6 * j + e];
    make_cam_table(c6, cscale + 6 * j, ct);
    for (int e = 0; e < CT_STRIDE; ++e) camtab[cam_tab_index(e, j, ncam)] = ct[e];
}

template <typename T>
void launch_cam_setup(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db, int which) {
    hipLaunchKernelGGL(k_cam_setup, dim3((ds.ncam + 63) / 64), dim3(64), 0, s, ds.ncam, db.cam[which], db.cscale, db.camtab[which]);
}
template void launch_cam_setup<float>(hipStream_t, const DeviceStructure&, const DeviceBuffers&, int);
template void launch_cam_setup<double>(hipStream_t, const DeviceStructure&, const DeviceBuffers&, int);

// First launch of a solve: the LM state arrives as a kernel argument (no H2D copy); the same launch clears the linear-solver
// status word, the Jacobi scales, the column-norm accumulators and the slotted accumulators and builds the camera tables
// (instead of a copy, two memsets, a fill kernel, k_cam_setup and k_iter0).
// cam_src / pts_src non-null: a pending sfmba_problem_reset() -- the initial parameters are copied into the current buffers by this
// launch (instead of two device-to-device copies and a state upload enqueued ahead of it: three more host calls in front of a solve
// whose first kernels are all a few microseconds long)
__global__ void k_begin(LMState st, DeviceStructure ds, DeviceBuffers db, const double* __restrict__ cam_src, const double* __restrict__ pts_src) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) { *db.st = st; *db.lin_info = 0; *db.fin_counter = 0; }
    if (e < 6 * ds.ncam) db.cscale[e] = 1.0;
    if (e < ds.ld) db.udiag[e] = 0.0;
    for (int k = e; k < db.nslot * SLOT_W; k += gridDim.x * blockDim.x) db.slots[k] = 0.0;
    if (pts_src) { for (size_t k = e; k < (size_t)3 * ds.npt; k += (size_t)gridDim.x * blockDim.x) db.pts[st.cur][k] = pts_src[k]; }
    if (e < ds.ncam) {
        double c6[6], ct[CT_STRIDE];
        for (int k = 0; k < 6; ++k) c6[k] = cam_src ? cam_src[6 * e + k] : db.cam[st.cur][6 * e + k];
        if (cam_src) { for (int k = 0; k < 6; ++k) db.cam[st.cur][6 * e + k] = c6[k]; }
        make_cam_table(c6, nullptr, ct);
        for (int k = 0; k < CT_STRIDE; ++k) db.camtab[st.cur][cam_tab_index(k, e, ds.ncam)] = ct[k];
    }
}
void launch_begin(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db, const LMState& st, const double* cam_src, const double* pts_src) {
    int nb = std::max(std::max(6 * ds.ncam, ds.ld), NSLOT * SLOT_W);      // (a larger slot array is cleared by a strided loop)
    if (pts_src) nb = std::max(nb, std::min(3 * ds.npt, 1 << 20));         // one point coordinate per thread up to 4096 workgroups
    hipLaunchKernelGGL(k_begin, dim3((nb + 255) / 256), dim3(256), 0, s, st, ds, db, cam_src, pts_src);
}

// ||x||^2 of the current parameters -> acc[ACC_XNEW2]
__global__ void k_xnorm(DeviceStructure ds, DeviceBuffers db) {
    __shared__ double scratch[BLK / 64];
    const int cur = db.st->cur;
    const double* cam = db.cam[cur];
    const double* pts = db.pts[cur];
    const int nc = 6 * ds.ncam, np = 3 * ds.npt;
    double s = 0.0;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nc + np; e += gridDim.x * blockDim.x) {
        const double v = e < nc ? cam[e] : pts[(size_t)3 * ds.pt_base + (e - nc)];
        s += (e < nc ? db.shared_weight : 1.0) * v * v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { const double f = db.st->focal[cur]; s += db.shared_weight * f * f; }
    s = block_sum(s, scratch);
    if (threadIdx.x == 0) atomicAdd(slot_ptr(db, ACC_XNEW2), s);
}

void launch_xnorm(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db) {
    int blocks = (6 * ds.ncam + 3 * ds.npt + BLK - 1) / BLK;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_xnorm, dim3(blocks), dim3(BLK), 0, s, ds, db);
}

// ------------------------------------------------------------------------------------------
// Jacobi column scaling (iteration 0): s = 1 / (1 + ||J_col||)   [Ceres-upstream EstimateScale]
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(BLK) void k_colnorm_points(DeviceStructure ds, DeviceBuffers db, int jacobi) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ds.npt) return;
    const int cur = db.st->cur;
    const double* tab = db.camtab[cur];
    const double focal = db.st->focal[cur];
    const double X[3] = { db.pts[cur][3 * i], db.pts[cur][3 * i + 1], db.pts[cur][3 * i + 2] };
    double n0 = 0, n1 = 0, n2 = 0;
    if (jacobi) {
        for (int q = ds.pt_ptr[i]; q < ds.pt_ptr[i + 1]; ++q) {
            const CamRow ct = { tab + 4 * (size_t)(ds.obs_cam[q]), ds.ncam };
            const Proj pr = project_point(ct, CT_R, CT_T, X);
            T B[6];
            point_block<T>(ct, pr, focal, B);
            n0 += (double)B[0] * (double)B[0] + (double)B[3] * (double)B[3];
            n1 += (double)B[1] * (double)B[1] + (double)B[4] * (double)B[4];
            n2 += (double)B[2] * (double)B[2] + (double)B[5] * (double)B[5];
        }
        db.pscale[3 * i] = 1.0 / (1.0 + sqrt(n0));
        db.pscale[3 * i + 1] = 1.0 / (1.0 + sqrt(n1));
        db.pscale[3 * i + 2] = 1.0 / (1.0 + sqrt(n2));
    } else {
        db.pscale[3 * i] = db.pscale[3 * i + 1] = db.pscale[3 * i + 2] = 1.0;
    }
}

// squared column norms of the camera / focal columns -> udiag (atomics), one block per chunk
// with_xnorm: the launch also sums ||x||^2 of the current parameters (k_xnorm's job: a launch of its own, 4.6 us per solve, for one strided pass
// over 2.4 MB) -- every workgroup takes a stride of the parameter arrays beside its chunk
template <typename T>
__global__ __launch_bounds__(BLK) void k_colnorm_cams(DeviceStructure ds, DeviceBuffers db, int with_xnorm) {
    __shared__ double scratch[(BLK / 64) * 8];
    const int4 ch = ds.chunks_coarse[ds.coarse_order[blockIdx.x]];
    const int j = ch.x;
    const int cur = db.st->cur;
    const CamRow ct = { db.camtab[cur] + 4 * (size_t)(j), ds.ncam };
    const double focal = db.st->focal[cur];
    const typename ObsXY<T>::type* oxy = reinterpret_cast<const typename ObsXY<T>::type*>(ds.obs_xy);
    (void)oxy;
    double n[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (with_xnorm) {
        const double* cam = db.cam[cur];
        const double* pts = db.pts[cur];
        const int nc = 6 * ds.ncam, np = 3 * ds.npt;
        double s = 0.0;
        for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nc + np; e += gridDim.x * blockDim.x) {
            const double v = e < nc ? cam[e] : pts[(size_t)3 * ds.pt_base + (e - nc)];
            s += (e < nc ? db.shared_weight : 1.0) * v * v;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) s += db.shared_weight * focal * focal;
        n[7] = s;
    }
    for (int e = ch.y + threadIdx.x; e < ch.z; e += blockDim.x) {
        const int i = ds.cam_obs_pt[e];
        const double X[3] = { db.pts[cur][3 * i], db.pts[cur][3 * i + 1], db.pts[cur][3 * i + 2] };
        const Proj pr = project_point(ct, CT_R, CT_T, X);
        T B[6], A[12];
        point_block<T>(ct, pr, focal, B);
        camera_block<T>(ct, pr, focal, X, B, A);
#pragma unroll
        for (int c = 0; c < 6; ++c) n[c] += (double)A[c] * (double)A[c] + (double)A[6 + c] * (double)A[6 + c];
        n[6] += pr.xp * pr.xp + pr.yp * pr.yp;
    }
    const double tot = block_sums<8>(n, scratch);            // (one barrier instead of eight pairs of them)
    if (threadIdx.x < 7) atomicAdd(threadIdx.x < 6 ? &db.udiag[6 * j + threadIdx.x] : slot_ptr(db, ACC_UDF), tot);
    if (with_xnorm && threadIdx.x == 7) atomicAdd(slot_ptr(db, ACC_XNEW2), tot);
}

__global__ void k_colnorm_finish(DeviceStructure ds, DeviceBuffers db, int jacobi, int finish_xnorm) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 64) {      // focal column: summed over the slots by one wave
        const double n2 = slots_take(db, ACC_UDF);
        if (threadIdx.x == 0) db.st->fscale = jacobi ? 1.0 / (1.0 + sqrt(n2)) : 1.0;
        if (finish_xnorm) {                          // ||x|| of the starting point (k_iter0's job outside a solve)
            const double x2 = slots_take(db, ACC_XNEW2);
            if (threadIdx.x == 0) db.st->x_norm = sqrt(x2);
        }
    }
    if (e >= ds.d - 1) return;
    db.cscale[e] = jacobi ? 1.0 / (1.0 + sqrt(db.udiag[e])) : 1.0;
}

void launch_colnorm_points_only(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db, int jacobi, int f32) {
    if (f32) hipLaunchKernelGGL(k_colnorm_points<float>, dim3((ds.npt + BLK - 1) / BLK), dim3(BLK), 0, s, ds, db, jacobi);
    else hipLaunchKernelGGL(k_colnorm_points<double>, dim3((ds.npt + BLK - 1) / BLK), dim3(BLK), 0, s, ds, db, jacobi);
}
void launch_colnorm_cams_only(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db, int jacobi, int f32, bool clear_udiag) {
    if (clear_udiag) (void)hipMemsetAsync(db.udiag, 0, sizeof(double) * ds.ld, s);
    if (!jacobi || ds.nchunk_coarse <= 0) return;
    if (f32) hipLaunchKernelGGL(k_colnorm_cams<float>, dim3(ds.nchunk_coarse), dim3(BLK), 0, s, ds, db, 0);
    else hipLaunchKernelGGL(k_colnorm_cams<double>, dim3(ds.nchunk_coarse), dim3(BLK), 0, s, ds, db, 0);
}
void launch_colnorm_finish(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db, int jacobi) {
    hipLaunchKernelGGL(k_colnorm_finish, dim3((ds.d + 255) / 256), dim3(256), 0, s, ds, db, jacobi, 0);
}

// with_xnorm: ||x||^2 is summed by the camera pass itself (launch_colnorm_sums_xnorm says whether that pass runs: else launch_xnorm first)
template <typename T>
void launch_colnorm(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db, int jacobi, bool clear_udiag, bool points, bool finish_xnorm, bool with_xnorm) {
    if (clear_udiag) (void)hipMemsetAsync(db.udiag, 0, sizeof(double) * ds.ld, s);
    if (points) hipLaunchKernelGGL(k_colnorm_points<T>, dim3((ds.npt + BLK - 1) / BLK), dim3(BLK), 0, s, ds, db, jacobi);
    if (jacobi && ds.nchunk_coarse > 0) hipLaunchKernelGGL(k_colnorm_cams<T>, dim3(ds.nchunk_coarse), dim3(BLK), 0, s, ds, db, with_xnorm ? 1 : 0);
    hipLaunchKernelGGL(k_colnorm_finish, dim3((ds.d + 255) / 256), dim3(256), 0, s, ds, db, jacobi, finish_xnorm ? 1 : 0);
}
template void launch_colnorm<float>(hipStream_t, const DeviceStructure&, const DeviceBuffers&, int, bool, bool, bool, bool);
template void launch_colnorm<double>(hipStream_t, const DeviceStructure&, const DeviceBuffers&, int, bool, bool, bool, bool);

// iteration 0 bookkeeping: x_norm from the accumulated ||x||^2
__global__ void k_iter0(DeviceBuffers db) {
    LMState* st = db.st;
    const double x2 = slots_take(db, ACC_XNEW2);
    for (int e = 0; e < SLOT_W; ++e) if (e != ACC_XNEW2) (void)slots_take(db, e);
    if (threadIdx.x == 0) { st->x_norm = sqrt(x2); *db.fin_counter = 0; }
}
void launch_iter0(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db) {
    (void)ds;
    hipLaunchKernelGGL(k_iter0, dim3(1), dim3(64), 0, s, db);
}

}  // namespace sfmba
