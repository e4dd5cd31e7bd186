// ba_finalize.hip -- stage 3 of the linearisation: finalize, between the camera pass (ba_cams.hip) and the pair pass (ba_pairs.hip, mode 1).
//   reads   the undamped diagonal blocks, focal column, gradient and right-hand side the passes before it summed (and cd_part), the slots'
//           focal-focal sums, the LM state (radius, clamps)
//   leaves  the damped diagonal of S, the camera / focal part of the gradient max-norm, the padding rows; PCG: Linv of every damped 6x6
//           block (pcg_binv), the pair pass's per-camera factor (pair_G) and the eight gauge vectors (pcg_W); exact solver: the
//           post-linearisation bookkeeping (PCG leaves it to the launch that follows)
// k_cd_fold and k_gauge are the two pieces of k_finalize a sharded solve runs on their own, in front of and behind its exchange.
#include "ba_common.h"

namespace sfmba {

// ------------------------------------------------------------------------------------------
// finalize: damping of the reduced diagonal, camera/focal part of the gradient max-norm, padding
// ------------------------------------------------------------------------------------------
// Rows of camera j in the 8 gauge vectors of the problem, in the unknowns of the block-Jacobi transformed reduced system
// (coarse space of the two-level CG preconditioner, pcg_common.h "Coarse space").  adjustBundle() holds no block constant
// (BA.cpp:160-164), so the undamped problem does not change under a similarity transform of the scene; in camera
// parameters (p = R X + t), to first order:
//   world translation a   (X -> X + a):        dt = -R a,  dw = 0
//   world rotation phi    (X -> Exp(phi) X):   R -> R Exp(-phi)  =>  dw = -Jr(w)^-1 phi,  dt = 0
//                         Jr^-1 = I + [w]x / 2 + (1/theta^2 - (1 + cos theta) / (2 theta sin theta)) [w]x^2
//   scale s               (X -> s X):          dt = t
// plus the weakly determined focal / depth direction (df = f, dt_z = t_z: a longer lens further away).  Unknowns are
// Jacobi-scaled (x = s x_s) and transformed by the block factor (x~ = Lb^T x_s, Lb^-1 = Li): w~ solves Li^T w~ = w / s.
// Values are rounded to fp32 so that every consumer (LDS copies included) sees the same numbers; any vectors are a valid
// coarse space, they only have to be close to the slow directions.
// (the camera's parameters, the rows of R and the Jacobi scales arrive preloaded: k_finalize issues every global load of a camera
// before its first dependent instruction -- read where they are used they were one more L2 round trip each on a kernel of 200 lanes)
// (Sibling: gauge_vector_k below, ONE vector for a runtime k.  Two, because this one computes cq and takes its reciprocals once for all
// eight vectors, that one reads CT_CQ from the table and takes them per vector: merging them would change results.)
__device__ __forceinline__ void gauge_vectors_pre(const DeviceStructure& ds, const DeviceBuffers& db, int j, const double (&Li)[6][6],
                                                  const double (&cam)[6], const double (&Rm)[9], const double (&cs6)[6]) {
    const double w0 = cam[0], w1 = cam[1], w2 = cam[2];
    const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
    double cq = 1.0 / 12.0;                              // limit of the [w]x^2 coefficient for theta -> 0
    if (th2 > 1e-8) {
        const double th = sqrt(th2);
        double sn, cs;
        sincos(th, &sn, &cs);
        const double den = 2.0 * th * sn;
        cq = fabs(den) > 1e-12 ? 1.0 / th2 - (1.0 + cs) / den : 0.0;     // theta near pi: drop the term, any vector will do
    }
    const double K[3][3] = { { 0.0, -w2, w1 }, { w2, 0.0, -w0 }, { -w1, w0, 0.0 } };
    double Ji[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double k2 = 0.0;
#pragma unroll
            for (int m = 0; m < 3; ++m) k2 += K[r][m] * K[m][c];
            Ji[r][c] = (r == c ? 1.0 : 0.0) + 0.5 * K[r][c] + cq * k2;
        }
    double s6[6], ild[6];       // 1 / Jacobi scale; 1 / Li[r][r]: reciprocals once, not a division per back-substitution step
#pragma unroll
    for (int e = 0; e < 6; ++e) { s6[e] = fast_rcp(cs6[e]); ild[e] = fast_rcp(Li[e][e]); }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        double wv[6] = { 0, 0, 0, 0, 0, 0 };
        if (k < 3) { for (int r = 0; r < 3; ++r) wv[3 + r] = -Rm[3 * r + k]; }
        else if (k < 6) { for (int r = 0; r < 3; ++r) wv[r] = -Ji[r][k - 3]; }
        else if (k == 6) { for (int r = 0; r < 3; ++r) wv[3 + r] = cam[3 + r]; }
        else wv[5] = cam[5];
#pragma unroll
        for (int e = 0; e < 6; ++e) wv[e] *= s6[e];
        // back substitution with the upper triangular Li^T
        double wt[6];
#pragma unroll
        for (int r = 5; r >= 0; --r) {
            double v = wv[r];
#pragma unroll
            for (int t = 5; t > r; --t) v -= Li[t][r] * wt[t];
            wt[r] = v * ild[r];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) db.pcg_W[(size_t)k * ds.ld + 6 * j + r] = (double)(float)wt[r];
    }
}
__device__ void gauge_vectors(const DeviceStructure& ds, const DeviceBuffers& db, int j, const double (&Li)[6][6]) {
    const int cur = db.st->cur;
    double cam[6], Rm[9], cs6[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) { cam[e] = db.cam[cur][6 * (size_t)j + e]; cs6[e] = db.cscale[6 * j + e]; }
#pragma unroll
    for (int e = 0; e < 9; ++e) Rm[e] = db.camtab[cur][cam_tab_index(CT_R + e, j, ds.ncam)];
    gauge_vectors_pre(ds, db, j, Li, cam, Rm, cs6);
}

// Focal row of the gauge vectors and their padding [d, ld): only the focal / depth vector (7) touches the focal; x~_f = lf x_f, lf = sqrt(S_ff)
__device__ __forceinline__ void gauge_focal_row(const DeviceStructure& ds, const DeviceBuffers& db, double lf) {
    const LMState* st = db.st;
    const int fo = ds.d - 1;
    for (int k = 0; k < 8; ++k) {
        db.pcg_W[(size_t)k * ds.ld + fo] = k == 7 ? (double)(float)(lf * st->focal[st->cur] / st->fscale) : 0.0;
        for (int e = ds.d; e < ds.ld; ++e) db.pcg_W[(size_t)k * ds.ld + e] = 0.0;
    }
}

// The gauge vectors for a reduced system whose block factors were formed outside k_finalize (sharded solve: the factors come
// from the all-reduced system, dense_pcg_transform): Linv of every camera block from db.pcg_binv, focal row from its last entry.
__global__ __launch_bounds__(64) void k_gauge(DeviceStructure ds, DeviceBuffers db) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < ds.ncam) {
        double Li[6][6];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) Li[r][c] = db.pcg_binv[(size_t)j * 36 + r * 6 + c];
        gauge_vectors(ds, db, j, Li);
    }
    if (j == 0) gauge_focal_row(ds, db, 1.0 / db.pcg_binv[(size_t)ds.ncam * 36]);        // sqrt(S_ff)
}
void launch_gauge(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db) {
    if (db.pcg_W) hipLaunchKernelGGL(k_gauge, dim3((ds.ncam + 63) / 64), dim3(64), 0, s, ds, db);
}

// ONE gauge vector (k = 0 .. 7, a per-lane value) of camera j: the body of gauge_vectors_pre for a runtime k -- the vector's entries are
// picked by selects (no dynamically indexed registers), the back substitution with Li^T is the same for every k.
// (Sibling: gauge_vectors_pre above; cq comes from the table here and the reciprocals sit elsewhere, so the two stay two.)
__device__ __forceinline__ void gauge_vector_k(const DeviceStructure& ds, const DeviceBuffers& db, int j, int k, const double (&Li)[6][6], const double (&cam)[6],
                                               const double (&Rm)[9], const double (&cs6)[6], double cq) {
    const double w0 = cam[0], w1 = cam[1], w2 = cam[2];
    const double K[3][3] = { { 0.0, -w2, w1 }, { w2, 0.0, -w0 }, { -w1, w0, 0.0 } };
    double wv[6];
    const int c3 = k - 3;                                     // world rotation: column k - 3 of -Jr^-1
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double k2c[3], ji[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            k2c[c] = 0.0;
#pragma unroll
            for (int m = 0; m < 3; ++m) k2c[c] += K[r][m] * K[m][c];
            ji[c] = (r == c ? 1.0 : 0.0) + 0.5 * K[r][c] + cq * k2c[c];
        }
        // (0 / 1 weights instead of select chains: the compiler turns a chain of selects over array elements into a dynamically indexed
        // array -- in scratch memory)
        const double jsel = (c3 == 0 ? 1.0 : 0.0) * ji[0] + (c3 == 1 ? 1.0 : 0.0) * ji[1] + (c3 == 2 ? 1.0 : 0.0) * ji[2];
        wv[r] = -jsel;
        const double rsel = (k == 0 ? 1.0 : 0.0) * Rm[3 * r] + (k == 1 ? 1.0 : 0.0) * Rm[3 * r + 1] + (k == 2 ? 1.0 : 0.0) * Rm[3 * r + 2];
        wv[3 + r] = -rsel + (k == 6 ? 1.0 : 0.0) * cam[3 + r] + ((k == 7 && r == 2) ? 1.0 : 0.0) * cam[5];
    }
    double wt[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) wv[e] *= fast_rcp(cs6[e]);
#pragma unroll
    for (int r = 5; r >= 0; --r) {                            // back substitution with the upper triangular Li^T
        double v = wv[r];
#pragma unroll
        for (int t = 5; t > r; --t) v -= Li[t][r] * wt[t];
        wt[r] = v * fast_rcp(Li[r][r]);
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) db.pcg_W[(size_t)k * ds.ld + 6 * j + r] = (double)(float)wt[r];
}

// Deterministic mode: the 45 per-camera sums of camera g's k_cam_diag_f chunks (cd_part), added in chunk order.  What is done with them
// differs: k_finalize adds them in registers on top of what it loaded, k_cd_fold adds them to memory.
__device__ __forceinline__ void cd_chunk_sums(const DeviceStructure& ds, const DeviceBuffers& db, int g, double (&acc)[45]) {
#pragma unroll
    for (int k = 0; k < 45; ++k) acc[k] = 0.0;
    for (int c = ds.cam_chunk_ptr[g]; c < ds.cam_chunk_ptr[g + 1]; ++c) {
#pragma unroll
        for (int k = 0; k < 45; ++k) acc[k] += db.cd_part[(size_t)c * 48 + k];
    }
}

// damping of the reduced diagonal, camera/focal part of the gradient max-norm, padding; in PCG mode also Linv of every damped 6x6
// diagonal block (the block-Jacobi preconditioner), the pair pass's per-camera factor and the gauge vectors.  EIGHT LANES PER CAMERA
// (round 4; one lane per camera made this kernel a 1000-deep dependent fp64 chain on 200 lanes: 14 us): every lane of a camera's group
// loads the block and factors it (the same instructions, no divergence), then lane t writes row t of the pair factor (rows picked by
// selects), gauge vector t and its share of Linv.  The focal entries are owned by the last wave of the last workgroup.  pcg = 0: the last
// workgroup to arrive (agent-scope release/acquire around an arrival counter) runs post_linearisation.
constexpr int FIN_LANES = 8;
__global__ __launch_bounds__(256) void k_finalize(DeviceStructure ds, DeviceBuffers db, int pcg) {
    __shared__ int is_last;
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    const LMState* st = db.st;
    // what the launch reads of the LM state, once and in front of its first store: read where they are used, the clamps and the radius came
    // back after every store of a damped diagonal entry (six round trips in a row on the writer lane of every camera), and the
    // accepted buffer's index was a vector load that the second half of a camera's loads waited for, each behind a pointer load of its own
    const int cur = st->cur;
    const double min_diag = st->min_diag, max_diag = st->max_diag, radius = st->radius, fscale = st->fscale;
    const double* const cam_c = cur ? db.cam[1] : db.cam[0];
    const double* const tab = cur ? db.camtab[1] : db.camtab[0];
    if (pcg && db.pcg_zero) { for (int i = gt; i < db.pcg_zero_n; i += gridDim.x * blockDim.x) db.pcg_zero[i] = 0.0; }      // (the symmetric CG's S~ W~ is accumulated with atomics)
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x >= 192) {
        // focal-focal entries were accumulated in the slotted buffer: the last wave of the last block owns them
        const int foc_acc[4] = { ACC_SFF, ACC_RHSF, ACC_UDF, ACC_BCF };
        double foc[4];
        slots_take_n<4>(db, foc_acc, foc);
        const double sff = foc[0], rhsf = foc[1], udf = foc[2], bcf = foc[3];
        if (threadIdx.x == 192) {
            const int fo = ds.d - 1;
            const double dd = fmin(fmax(udf, min_diag), max_diag) / radius;
            db.S[(size_t)fo * ds.ld + fo] = sff + dd;
            db.rhs[fo] = rhsf; db.udiag[fo] = udf; db.bc[fo] = bcf;
            const double gg = fabs(bcf / fscale);
            if (gg > 0.0) atomic_max_nonneg(slot_ptr(db, ACC_GMAX), gg);
            if (!finite_d(sff + dd) || !finite_d(rhsf)) atomicAdd(slot_ptr(db, ACC_BAD_LIN), 1.0);
            if (pcg && !(sff + dd > 0.0)) atomicCAS(db.lin_info, 0, ds.d);
            if (pcg && db.pcg_W) gauge_focal_row(ds, db, sqrt(sff + dd > 0.0 ? sff + dd : 1.0));
        }
    }
    double gm = 0.0;
    const int g = gt / FIN_LANES, t = gt % FIN_LANES;         // camera, lane of its group
    if (g < ds.ncam) {
        const int row0 = 6 * g, fo = ds.d - 1;
        const bool writer = t == 0;
        // every global load of this camera first (one L2 round trip): diagonal block, focal column, undamped diagonal, gradient, scales,
        // and what the gauge vectors and the pair pass's camera factor need
        double Sb[6][6], ud[6], bcv[6], csv[6], rhv[6], sjf[6], camv[6], Rm[9], Q9[9], cq = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            ud[a] = db.udiag[row0 + a]; bcv[a] = db.bc[row0 + a]; csv[a] = db.cscale[row0 + a]; rhv[a] = db.rhs[row0 + a];
            sjf[a] = db.cd_part ? db.S[(size_t)(row0 + a) * ds.ld + fo] : 0.0;
#pragma unroll
            for (int b = 0; b < 6; ++b) Sb[a][b] = (b >= a) ? db.S[(size_t)(row0 + a) * ds.ld + row0 + b] : 0.0;
        }
        if (pcg) {
#pragma unroll
            for (int e = 0; e < 6; ++e) camv[e] = db.pcg_W ? cam_c[6 * (size_t)g + e] : 0.0;
#pragma unroll
            for (int e = 0; e < 9; ++e) { Rm[e] = db.pcg_W ? tab[cam_tab_index(CT_R + e, g, ds.ncam)] : 0.0; Q9[e] = db.pair_G ? tab[cam_tab_index(CT_QD + e, g, ds.ncam)] : 0.0; }
            cq = db.pcg_W ? tab[cam_tab_index(CT_CQ, g, ds.ncam)] : 0.0;
        }
        if (db.cd_part) {
            // deterministic mode: this camera's k_cam_diag_f chunks, in chunk order, on top of what the (single-writer) passes left -- added in
            // registers by every lane of the group, written back by one (the exact solver and the AUTO fallback read the block from memory)
            double acc[45];
            cd_chunk_sums(ds, db, g, acc);
            int u = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b) Sb[a][b] += acc[u++];
#pragma unroll
            for (int a = 0; a < 6; ++a) { ud[a] += acc[21 + a]; sjf[a] += acc[27 + a]; bcv[a] += acc[33 + a]; rhv[a] += acc[39 + a]; }
            if (writer) {
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    db.udiag[row0 + a] = ud[a]; db.S[(size_t)(row0 + a) * ds.ld + fo] = sjf[a]; db.bc[row0 + a] = bcv[a]; db.rhs[row0 + a] = rhv[a];
#pragma unroll
                    for (int b = a + 1; b < 6; ++b) db.S[(size_t)(row0 + a) * ds.ld + row0 + b] = Sb[a][b];
                }
            }
        }
        bool bad = false;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const int e = row0 + a;
            const double dd = fmin(fmax(ud[a], min_diag), max_diag) / radius;
            const double v = Sb[a][a] + dd;
            Sb[a][a] = v;
            if (writer) db.S[(size_t)e * ds.ld + e] = v;
            gm = fmax(gm, fabs(bcv[a] / csv[a]));
            bad = bad || !finite_d(v) || !finite_d(rhv[a]);
        }
        if (bad && writer) atomicAdd(slot_ptr(db, ACC_BAD_LIN), 1.0);
        if (pcg) {
            // Linv of the damped block (row-major lower, zeros above).  (Sibling: k_pcg_blockchol, dense_solver.hip -- sqrt and divisions
            // there, fast_rsq and reciprocal pivots here: different arithmetic, so the two stay two.)
            double L[6][6], Li[6][6];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) L[r][c] = (c <= r) ? Sb[c][r] : 0.0;
            bool ok = true;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double dj = L[j][j];
#pragma unroll
                for (int tt = 0; tt < 6; ++tt) if (tt < j) dj -= L[j][tt] * L[j][tt];
                ok = ok && (dj > 0.0);
                const double lji = fast_rsq(dj > 0.0 ? dj : 1.0);
                L[j][j] = lji;              // the RECIPROCAL of the pivot is what the inverse needs
#pragma unroll
                for (int i = 0; i < 6; ++i) if (i > j) {
                    double v = L[i][j];
#pragma unroll
                    for (int tt = 0; tt < 6; ++tt) if (tt < j) v -= L[i][tt] * L[j][tt];
                    L[i][j] = v * lji;
                }
            }
            if (!ok && writer) atomicCAS(db.lin_info, 0, row0 + 1);
#pragma unroll
            for (int c = 0; c < 6; ++c)
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    double v = (r == c) ? 1.0 : 0.0;
#pragma unroll
                    for (int tt = 0; tt < 6; ++tt) if (tt >= c && tt < r) v -= L[r][tt] * Li[tt][c];
                    Li[r][c] = (r < c) ? 0.0 : v * L[r][r];
                }
            // lane t < 6 owns row t of Linv (store) and of the pair factor G = Linv D E^T: the row by selects.  (Sibling: pair_factor<true>,
            // ba_pairs.hip, all 36 entries on one lane; this is its row form for eight lanes per camera.)
            double lrow[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < 6; ++r) v += (t == r ? 1.0 : 0.0) * Li[r][c];      // (weights, not selects: see gauge_vector_k)
                lrow[c] = v;
            }
            if (t < 6) {
#pragma unroll
                for (int c = 0; c < 6; ++c) db.pcg_binv[(size_t)g * 36 + t * 6 + c] = lrow[c];
                if (db.pair_G) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
                        double v;
                        if (c < 3) {            // sum_{a < 3} Lw[r][a] (D E^T)[a][c],  (D E^T)[a][c] = cs[a] Q[c][a]
                            v = 0.0;
#pragma unroll
                            for (int a = 0; a < 3; ++a) v += lrow[a] * (csv[a] * Q9[3 * c + a]);
                        } else {
                            v = lrow[c] * csv[c];
                        }
                        db.pair_G[(size_t)g * 36 + 6 * t + c] = v;
                    }
                }
            }
            if (db.pcg_W) gauge_vector_k(ds, db, g, t, Li, camv, Rm, csv, cq);
        }
        if (!writer) gm = 0.0;
    } else if (gt - ds.ncam * FIN_LANES < ds.ld - ds.d) {
        const int e = ds.d + (gt - ds.ncam * FIN_LANES);
        db.S[(size_t)e * ds.ld + e] = 1.0;
        db.rhs[e] = 0.0;
    }
    gm = wave_max(gm);
    if ((threadIdx.x & 63) == 0 && gm > 0.0) atomic_max_nonneg(slot_ptr(db, ACC_GMAX), gm);
    if (pcg == 1) return;        // post_linearisation runs in the pair pass that follows (see k_schur_pairs, MODE 1)
    // ---- arrival: every wave drains its stores, one lane releases and takes a ticket ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int ticket = __hip_atomic_fetch_add(db.fin_counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = (ticket == (int)gridDim.x - 1);
        if (is_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __hip_atomic_store(db.fin_counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (is_last && threadIdx.x < 64) post_linearisation(ds, db);
}

// Deterministic mode, sharded solve: the per-chunk sums of k_cam_diag are folded into the reduced system (in chunk order, one thread
// per camera) BEFORE the partial system is packed for the exchange; k_finalize, which does this on one GPU, runs behind the all-reduce
// there and is then called with cd_part = null.
__global__ __launch_bounds__(64) void k_cd_fold(DeviceStructure ds, DeviceBuffers db) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ds.ncam || !db.cd_part) return;
    const int row0 = 6 * g, fo = ds.d - 1;
    double acc[45];
    cd_chunk_sums(ds, db, g, acc);
    int u = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) db.S[(size_t)(row0 + a) * ds.ld + row0 + b] += acc[u++];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        db.udiag[row0 + a] += acc[21 + a];
        db.S[(size_t)(row0 + a) * ds.ld + fo] += acc[27 + a];
        db.bc[row0 + a] += acc[33 + a];
        db.rhs[row0 + a] += acc[39 + a];
    }
}
void launch_cd_fold(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db) {
    if (db.cd_part) hipLaunchKernelGGL(k_cd_fold, dim3((ds.ncam + 63) / 64), dim3(64), 0, s, ds, db);
}

void launch_finalize(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db, int pcg) {
    const int work = ds.ncam * FIN_LANES + (ds.ld - ds.d) + 64;     // eight lanes per camera, padding rows, room for the focal wave
    hipLaunchKernelGGL(k_finalize, dim3((work + 255) / 256), dim3(256), 0, s, ds, db, pcg);
}

}  // namespace sfmba
