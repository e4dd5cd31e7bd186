// ba_cams.hip -- stage 2 of the linearisation: the camera-diagonal pass (camera-major), behind the point pass (ba_points.hip).
//   reads   camtab[cur], the per-point table (PA, PB), the observations in camera-major order, cscale / fscale
//   leaves  per camera: S_jj (upper part, minus the self terms), S_jf, the undamped diagonal, b_c and the reduced right-hand side --
//           added with atomics, or (deterministic handles) one row of cd_part per chunk that ba_finalize.hip adds in chunk order;
//           the focal-focal sums in the slots
#include "ba_common.h"

namespace sfmba {

// ------------------------------------------------------------------------------------------
// K2b: camera-diagonal pass.  One lane per observation of the camera (no loop, two dependent memory
// levels), SFMBA_CAM_CHUNK (256) lanes per workgroup = one chunk of one camera.  Each lane forms its 47 terms in T;
// the sums over lanes are carried in fp64: halving butterfly inside the wave, LDS across the waves,
// one atomic per value per workgroup.
//   S_jj += A~^T (I - C C^T) A~   (U_jj minus the self term Y_a Y_a^T), undamped diagonal, S_jf, b_c, rhs
// ------------------------------------------------------------------------------------------
// the 47 terms (ACCUM: added to v, else stored) one observation contributes to its camera's diagonal block, focal column, gradient and right-hand side, from its packed
// record and side values z = {C t (2), C y_f (2), residual (2)} -- shared by the record-gathering and the re-evaluating camera pass
template <typename T, bool ACCUM>
__device__ __forceinline__ void cam_diag_terms(const T (&rec)[YREC], const T (&z)[8], const double* __restrict__ cscale6, T fscale, T (&v)[CD_N]) {
        T A[12];
        rec_camera_block<T>(rec, A);
#pragma unroll
        for (int c = 0; c < 6; ++c) { const T s = (T)cscale6[c]; A[c] *= s; A[6 + c] *= s; }
        const T r0 = z[4], r1 = z[5];
        const T g0 = rec[7] * fscale, g1 = rec[8] * fscale;
        // N = I - C C^T
        const T n00 = (T)1 - (rec[9] * rec[9] + rec[10] * rec[10] + rec[11] * rec[11]);
        const T n01 = -(rec[9] * rec[12] + rec[10] * rec[13] + rec[11] * rec[14]);
        const T n11 = (T)1 - (rec[12] * rec[12] + rec[13] * rec[13] + rec[14] * rec[14]);
        // Y v = A~^T (C v): C t and C y_f come from the side record
        const T ct0 = z[0], ct1 = z[1], cy0 = z[2], cy1 = z[3];
        int u = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const T p0 = n00 * A[a] + n01 * A[6 + a], p1 = n01 * A[a] + n11 * A[6 + a];
#pragma unroll
            for (int b = a; b < 6; ++b) { const T t_ = p0 * A[b] + p1 * A[6 + b]; if (ACCUM) v[u] += t_; else v[u] = t_; ++u; }
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const T ar = A[a] * r0 + A[6 + a] * r1;
            { const T t_ = A[a] * A[a] + A[6 + a] * A[6 + a]; if (ACCUM) v[21 + a] += t_; else v[21 + a] = t_; }                               // undamped diagonal
            { const T t_ = (A[a] * g0 + A[6 + a] * g1) - (A[a] * cy0 + A[6 + a] * cy1); if (ACCUM) v[27 + a] += t_; else v[27 + a] = t_; }     // S[j,f]
            { const T t_ = ar; if (ACCUM) v[33 + a] += t_; else v[33 + a] = t_; }                                                              // b_c (scaled gradient)
            { const T t_ = ar - (A[a] * ct0 + A[6 + a] * ct1); if (ACCUM) v[39 + a] += t_; else v[39 + a] = t_; }                              // reduced rhs
        }
        { const T t_ = g0 * g0 + g1 * g1; if (ACCUM) v[45] += t_; else v[45] = t_; }
        { const T t_ = g0 * r0 + g1 * r1; if (ACCUM) v[46] += t_; else v[46] = t_; }
}

// sums of the 47 terms over the workgroup (fp64: halving butterfly inside the wave, LDS across the waves) and one atomic per value
// per workgroup -- or, deterministic mode, the per-chunk slot that k_finalize / k_cd_fold add in chunk order
template <typename T>
__device__ __forceinline__ void cam_diag_finish(const DeviceStructure& ds, const DeviceBuffers& db, int j, int chunk_id, T (&v)[CD_N], double (*red)[CD_N]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // first halving step on the T values (one 32-bit shuffle each), the rest in fp64
    double acc[CD_N / 2];
    {
        const bool up = (lane & 32) != 0;
#pragma unroll
        for (int k = 0; k < CD_N / 2; ++k) {
            const T lo = v[k], hi = v[CD_N / 2 + k];
            const T send = up ? lo : hi, keep = up ? hi : lo;
            acc[k] = (double)keep + (double)__shfl_xor(send, 32, 64);        // (LDS pipe: see HalvingReduceT, fp64)
        }
    }
    int base = (lane & 32) ? CD_N / 2 : 0, len = CD_N / 2;
    HalvingReduce<CD_N / 2, 16>::run(acc, lane, base, len);
    if (len >= 1) red[w][base] = acc[0];
    __syncthreads();
    if (threadIdx.x < 47) {
        const int k = threadIdx.x;
        double s = 0.0;
#pragma unroll
        for (int ww = 0; ww < CD_BLK / 64; ++ww) s += red[ww][k];
        const int row0 = 6 * j, fo = ds.d - 1;
        if (db.cd_part && k < 45) { db.cd_part[(size_t)chunk_id * 48 + k] = s; return; }      // deterministic mode: k_finalize adds the chunks in order
        if (k < 21) {
            int a = 0, rem = k;
            while (rem >= 6 - a) { rem -= 6 - a; ++a; }
            atomicAdd(&db.S[(size_t)(row0 + a) * ds.ld + row0 + a + rem], s);
        } else if (k < 27) {
            atomicAdd(&db.udiag[row0 + k - 21], s);
        } else if (k < 33) {
            atomicAdd(&db.S[(size_t)(row0 + k - 27) * ds.ld + fo], s);
        } else if (k < 39) {
            atomicAdd(&db.bc[row0 + k - 33], s);
        } else if (k < 45) {
            atomicAdd(&db.rhs[row0 + k - 39], s);
        } else if (k == 45) {
            atomicAdd(slot_ptr(db, ACC_SFF), s);
            atomicAdd(slot_ptr(db, ACC_UDF), s);
        } else {
            atomicAdd(slot_ptr(db, ACC_RHSF), s);
            atomicAdd(slot_ptr(db, ACC_BCF), s);
        }
    }
}

// Nothing is stored per observation: the camera's table row sits in scalar registers (one camera per workgroup), a lane gathers its
// observation's point-table entries (64 + 24 bytes from a table that stays in L2), reads the observation's coordinates from the
// camera-major copy (coalesced), and re-evaluates blocks and residual with the expressions of the point pass (obs_record).
template <typename T>
__global__ __launch_bounds__(CD_BLK) void k_cam_diag_f(DeviceStructure ds, DeviceBuffers db) {
    __shared__ double red[CD_BLK / 64][CD_N];
    const int chunk_id = ds.chunk_order[blockIdx.x];
    const int4 ch = ds.chunks[chunk_id];
    const int j = ch.x;
    const LMState* st = db.st;
    const int cur = st->cur;
    const double focal = st->focal[cur];
    const T fscale = (T)st->fscale;
    CamRegs ct;
    load_cam_regs(db.camtab[cur], j, ds.ncam, ct);
    T v[CD_N];
#pragma unroll
    for (int k = 0; k < CD_N; ++k) v[k] = (T)0;
    const typename ObsXY<T>::type* xy = reinterpret_cast<const typename ObsXY<T>::type*>(ds.cam_obs_xy);
    const PtRecA<T>* PA = reinterpret_cast<const PtRecA<T>*>(db.PA);
    const PtRecB<T>* PB = reinterpret_cast<const PtRecB<T>*>(db.PB);
    // SFMBA_CAM_CHUNK / CD_BLK observations per lane (1 by default).  With several, the loop is software-pipelined: the point slot is fetched
    // two rounds ahead and the point-table entries one round ahead, so that a round's arithmetic runs under the next round's gathers.
    int e = ch.y + threadIdx.x;
    int i_nn = 0;
    PtRecA<T> pa_n = PA[0]; PtRecB<T> pb_n = PB[0];
    typename ObsXY<T>::type oxy_n = xy[e < ch.z ? e : ch.y];
    if (e < ch.z) { const int i0 = ds.cam_obs_pt[e]; pa_n = PA[i0]; pb_n = PB[i0]; }
    if (CD_OBS > 1 && e + CD_BLK < ch.z) i_nn = ds.cam_obs_pt[e + CD_BLK];
#pragma unroll 1
    for (; e < ch.z; e += CD_BLK) {
        const PtRecA<T> pa = pa_n;
        const PtRecB<T> pb = pb_n;
        const typename ObsXY<T>::type oxy = oxy_n;
        if (CD_OBS > 1) {
            if (e + CD_BLK < ch.z) { pa_n = PA[i_nn]; pb_n = PB[i_nn]; oxy_n = xy[e + CD_BLK]; }
            if (e + 2 * CD_BLK < ch.z) i_nn = ds.cam_obs_pt[e + 2 * CD_BLK];
        }
        T rec[YREC], z[8];
        obs_record<T>(ct, focal, pa.X, pa.L, rec);
        // the residual as the point pass forms it: fp64 projection, fp64 subtraction, then rounded to T
        typename ObsXY<T>::type rr;
        { const Proj pr = project_point(ct, CT_R, CT_T, pa.X); rr.x = (T)(focal * pr.xp - (double)oxy.x); rr.y = (T)(focal * pr.yp - (double)oxy.y); }
        // side values: C t, C y_f, residual
        z[0] = rec[9] * pb.t[0] + rec[10] * pb.t[1] + rec[11] * pb.t[2];
        z[1] = rec[12] * pb.t[0] + rec[13] * pb.t[1] + rec[14] * pb.t[2];
        z[2] = rec[9] * pb.yf[0] + rec[10] * pb.yf[1] + rec[11] * pb.yf[2];
        z[3] = rec[12] * pb.yf[0] + rec[13] * pb.yf[1] + rec[14] * pb.yf[2];
        z[4] = rr.x; z[5] = rr.y; z[6] = (T)0; z[7] = (T)0;
        cam_diag_terms<T, (CD_OBS > 1)>(rec, z, db.cscale + 6 * j, fscale, v);
    }
    cam_diag_finish<T>(ds, db, j, chunk_id, v, red);
}

template <typename T>
void launch_cam_diag(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db) {
    if (ds.nchunk > 0) hipLaunchKernelGGL(k_cam_diag_f<T>, dim3(ds.nchunk), dim3(CD_BLK), 0, s, ds, db);
}
template void launch_cam_diag<float>(hipStream_t, const DeviceStructure&, const DeviceBuffers&);
template void launch_cam_diag<double>(hipStream_t, const DeviceStructure&, const DeviceBuffers&);

}  // namespace sfmba
