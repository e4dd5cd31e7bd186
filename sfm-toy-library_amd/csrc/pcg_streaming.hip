// pcg_streaming.hip -- the streaming CG family: any d, both triangles of S~ read once per iteration, one launch per iteration (k_pcg_iter), the
// 8-vector coarse set-up in two (k_pcg_coarse, then k_pcg_coarse_invert of pcg_fast.hip).  What deterministic handles and the sharded replicated form run above d = 1280.
#include "pcg_common.h"

namespace sfmba {

// NR: rows per wave held at a time (2 for rows_per_wg <= 8 -- BASELINE config 5 --, else NR)
template <typename FT, int NR>
__global__ __launch_bounds__(256) void k_pcg_coarse(int d, int ld, const FT* __restrict__ F, const double* __restrict__ W, const double* __restrict__ bt,
                                                    double* __restrict__ AW, double* __restrict__ epart, int rows_per_wg) {
    __shared__ __align__(16) float wt[PCG_NW][CO_TILE];
    __shared__ double awrow[4][PCG_NW];
    __shared__ double esum[4][PCG_NW * PCG_NW + PCG_NW];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row0 = blockIdx.x * rows_per_wg, row1 = min(d, row0 + rows_per_wg);
    double acc[NR][PCG_NW];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) acc[r][k] = 0.0;
    for (int t0 = 0; t0 < d; t0 += CO_TILE) {
        // The wave's rows of this tile first, 16 bytes per load and ALL of them in flight before anything waits (a lane takes four consecutive
        // columns of each 256-column chunk): with one 4-byte load per row and chunk, as this loop used to be written, a wave of cfg 5 (two rows)
        // had 32 bytes per lane in flight and the pass ran at 1.3 TB/s (112 us for the 144 MB of the fp32 matrix).  They do not depend on the
        // staging of W~ below and overlap it.
        Quad<FT> f[NR][CO_TILE / 256];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int row = row0 + w + 4 * r;
            const FT* Fr = F + (size_t)(row < row1 ? row : row0) * ld + t0;
#pragma unroll
            for (int q = 0; q < CO_TILE / 256; ++q) {
                const int c = 256 * q + 4 * lane;
                f[r][q].load(Fr + ((row < row1 && t0 + c < d) ? c : 0));
            }
        }
        __syncthreads();
        // (eight loads in flight per thread: left as one load per loop iteration the staging was a chain of L2 round trips per tile and
        // cost more than the pass over the matrix it serves)
#pragma unroll
        for (int b = 0; b < CO_TILE / 256; ++b) {
            double wv[PCG_NW];
            const int c = tid + 256 * b;
#pragma unroll
            for (int k = 0; k < PCG_NW; ++k) wv[k] = W[(size_t)k * ld + (t0 + c < d ? t0 + c : 0)];
#pragma unroll
            for (int k = 0; k < PCG_NW; ++k) wt[k][c] = (t0 + c < d) ? (float)wv[k] : 0.0f;       // W~ holds fp32-representable values: lossless
        }
        __syncthreads();
        // a lane's W~ values of its four columns are read from LDS (and widened) ONCE per chunk and used by all of the wave's rows
#pragma unroll
        for (int q = 0; q < CO_TILE / 256; ++q) {
            const int c = 256 * q + 4 * lane;
            if (t0 + 256 * q >= d) break;                            // wave-uniform
            float4 wq[PCG_NW];
#pragma unroll
            for (int k = 0; k < PCG_NW; ++k) wq[k] = *reinterpret_cast<const float4*>(&wt[k][c]);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                if (row0 + w + 4 * r >= row1) continue;              // wave-uniform
                // columns beyond d hold padding: never multiply garbage (W~ is zero there, 0 x NaN is not)
                const double f0 = t0 + c + 0 < d ? f[r][q].get(0) : 0.0, f1 = t0 + c + 1 < d ? f[r][q].get(1) : 0.0;
                const double f2 = t0 + c + 2 < d ? f[r][q].get(2) : 0.0, f3 = t0 + c + 3 < d ? f[r][q].get(3) : 0.0;
#pragma unroll
                for (int k = 0; k < PCG_NW; ++k)
                    acc[r][k] = fma(f0, (double)wq[k].x, fma(f1, (double)wq[k].y, fma(f2, (double)wq[k].z, fma(f3, (double)wq[k].w, acc[r][k]))));
            }
        }
    }
    double e_acc = 0.0, c_acc = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int row = row0 + w + 4 * r;
        if (row >= row1) continue;                        // wave-uniform
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) {
            double v = acc[r][k];
            v = wave_allsum(v);
            if (lane == k) { AW[(size_t)row * PCG_NW + k] = v; awrow[w][k] = v; }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        e_acc = fma(W[(size_t)(lane >> 3) * ld + row], awrow[w][lane & 7], e_acc);
        if (lane < PCG_NW) c_acc = fma(W[(size_t)lane * ld + row], bt[row], c_acc);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    esum[w][lane] = e_acc;
    if (lane < PCG_NW) esum[w][PCG_NW * PCG_NW + lane] = c_acc;
    __syncthreads();
    if (tid < PCG_NW * PCG_NW + PCG_NW) epart[(size_t)tid * PCG_PART + blockIdx.x] = esum[0][tid] + esum[1][tid] + esum[2][tid] + esum[3][tid];
}

// Generic path of one CG iteration (any d).  Vector phase as in the fast path but looped; the matvec streams two rows
// of S~ per wave with 16-byte loads, four deep, so that a wave keeps 128 B per lane in flight (the rows are HBM/MALL
// traffic: d*ld*8 bytes per iteration, 289 MB at d = 6001).  Up to PCG_MAXWG_BIG workgroups.
template <bool INIT, typename FT, bool COARSE>
__global__ __launch_bounds__(256) void k_pcg_iter(int d, int ld, const FT* __restrict__ F, double* __restrict__ vec,
                                                  const double* __restrict__ bt, double* __restrict__ part, double* scal,
                                                  int* flags, int rows_per_wg, double tol2, int in, int* info, int* mailbox, int anchor, double cap,
                                                  const double* __restrict__ W, const double* __restrict__ AW, const double* __restrict__ coarse) {
    extern __shared__ __align__(16) double sm[];
    double* pl = sm;            // [ld] new search direction (p_r)
    double* red = sm + ld;      // [PCG_RED]
    // `in` = (launch number << 1) | parity.  PF_DONE holds the first launch number that has nothing left to do: a launch must not act
    // on the flag its own workgroup 0 raises (workgroups that start late, e.g. behind another process's kernels, would skip the
    // converging iteration's x update).
    const int seq = in >> 1;
    in &= 1;
    if (!INIT) { const int dn = flags[PF_DONE]; if (dn != 0 && seq >= dn) return; }
    constexpr int NV = COARSE ? PCG_NPART : 1;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, out = in ^ 1;
    const int row0 = blockIdx.x * rows_per_wg;
    const int row1 = min(d, row0 + rows_per_wg);
    const int nwg = (int)gridDim.x;
    double* x_out = pcg_vec(vec, 0, out, ld); double* r_out = pcg_vec(vec, 1, out, ld);
    double* p_out = pcg_vec(vec, 2, out, ld); double* q_out = pcg_vec(vec, 3, out, ld);
    const double* x_in = pcg_vec(vec, 0, in, ld); const double* r_in = INIT ? bt : pcg_vec(vec, 1, in, ld);
    const double* p_in = pcg_vec(vec, 2, in, ld); const double* q_in = pcg_vec(vec, 3, in, ld);
    const double* st_in = scal + PS_STATE + PS_STATE_LEN * in;
    double* st_out = scal + PS_STATE + PS_STATE_LEN * out;
    if (COARSE && tid < PCG_NW * PCG_NW) red[80 + tid] = coarse[tid];
    // fp32 matrix: the first 16-byte batch of this wave's first two rows is requested NOW -- the vector phase below (three syncs, the
    // vectors from L2) then runs under the matrix's first memory round trip instead of in front of it
    float4 pre_a[4], pre_b[4];
    const bool pre = sizeof(FT) == 4 && row0 + w < row1 && lane + 192 < (d >> 2);
    if (sizeof(FT) == 4) {
        const int rowa = row0 + w < row1 ? row0 + w : row0, rowb = rowa + 4 < row1 ? rowa + 4 : rowa;
        const float4* Fa = reinterpret_cast<const float4*>(F + (size_t)rowa * ld);
        const float4* Fb = reinterpret_cast<const float4*>(F + (size_t)rowb * ld);
#pragma unroll
        for (int m = 0; m < 4; ++m) { pre_a[m] = Fa[pre ? lane + 64 * m : 0]; pre_b[m] = Fb[pre ? lane + 64 * m : 0]; }
    }
    double c_new[PCG_NW], mu_new[PCG_NW], pmu_new[PCG_NW], pmu_in[PCG_NW];
    double rz_new = 0.0;
    if (INIT) {
        double rr = 0.0;
        for (int e0 = tid; e0 < d; e0 += 256 * 8) {
            double bv8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; bv8[u] = bt[e < d ? e : d - 1]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; if (e < d) { pl[e] = bv8[u]; rr += bv8[u] * bv8[u]; } }
        }
        rr = wave_allsum(rr);
        if (lane == 0) red[16 + w] = rr;
        __syncthreads();
        rr = red[16] + red[17] + red[18] + red[19];
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) { c_new[k] = COARSE ? coarse[PCG_NW * PCG_NW + k] : 0.0; mu_new[k] = 0.0; pmu_in[k] = 0.0; }
        if (COARSE) einv_apply(red + 80, c_new, mu_new);
        rz_new = rr + (COARSE ? dot8(c_new, mu_new) : 0.0);
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) pmu_new[k] = mu_new[k];
        for (int e = row0 + tid; e < row1; e += 256) { x_out[e] = 0.0; r_out[e] = pl[e]; p_out[e] = pl[e]; }
        if (blockIdx.x == 0 && tid == 0) {
            scal[PS_RR0] = pcg_threshold_base(rr, scal, anchor, cap); flags[PF_DONE] = (rr == 0.0); flags[PF_ITERS] = 0; flags[PF_XBUF] = out;
            if (mailbox && rr == 0.0) pcg_post(mailbox, 0, 1);
        }
    } else {
        double mine[3] = { 0.0, 0.0, 0.0 };
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int v = w + 4 * j;
            if (4 * j < NV) {
                const double* pp = pcg_part(part, in, v < NV ? v : 0);
                for (int i0 = 0; i0 < nwg; i0 += 256) {       // four loads in flight per value, never a `+= load` chain
                    double t[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) { const int wg = i0 + lane + 64 * i; t[i] = pp[wg < nwg ? wg : nwg - 1]; }
#pragma unroll
                    for (int i = 0; i < 4; ++i) mine[j] += (i0 + lane + 64 * i < nwg && v < NV) ? t[i] : 0.0;
                }
            }
        }
        reduce_partials<NV>(mine, red);
        __syncthreads();
        double g[PCG_NW], Eg[PCG_NW], c_in[PCG_NW], mu_in[PCG_NW];
        const double rz_in = st_in[PS_RZ];
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) {
            g[k] = COARSE ? red[1 + k] : 0.0;
            pmu_in[k] = COARSE ? st_in[PS_PMU + k] : 0.0;
            c_in[k] = COARSE ? st_in[PS_C + k] : 0.0;
            mu_in[k] = COARSE ? st_in[PS_MU + k] : 0.0;
            Eg[k] = 0.0;
        }
        if (COARSE) einv_apply(red + 80, g, Eg);
        const double pq = red[0] + (COARSE ? dot8(pmu_in, g) : 0.0);
        const double alpha = rz_in / pq;
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) { c_new[k] = fma(-alpha, g[k], c_in[k]); mu_new[k] = fma(-alpha, Eg[k], mu_in[k]); }
        const double cmu = COARSE ? dot8(c_new, mu_new) : 0.0;
        double rrn = 0.0;
        // (eight elements' loads in flight: one load / use pair per loop iteration is a chain of d / 256 cache round trips)
        for (int e0 = tid; e0 < d; e0 += 256 * 8) {
            double rv8[8], qv8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u, ec = e < d ? e : d - 1; rv8[u] = r_in[ec]; qv8[u] = q_in[ec]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; if (e < d) { const double v = rv8[u] - alpha * qv8[u]; pl[e] = v; rrn += v * v; } }
        }
        rrn = wave_allsum(rrn);
        if (lane == 0) red[16 + w] = rrn;
        // x += alpha p  with p = p_r + W~ p_mu, own rows
        for (int e = row0 + tid; e < row1; e += 256) {
            double pe = p_in[e];
            if (COARSE) {
#pragma unroll
                for (int k = 0; k < PCG_NW; ++k) pe = fma(W[(size_t)k * ld + e], pmu_in[k], pe);
            }
            x_out[e] = x_in[e] + alpha * pe;
        }
        __syncthreads();
        rrn = red[16] + red[17] + red[18] + red[19];
        rz_new = rrn + cmu;
        const bool broke = !(pq > 0.0) || !(rrn == rrn);
        if (rrn <= tol2 * scal[PS_RR0] || broke) {
            if (blockIdx.x == 0 && tid == 0) {
                flags[PF_DONE] = seq + 1; flags[PF_XBUF] = out; const int it = flags[PF_ITERS] + 1; flags[PF_ITERS] = it;
                if (broke) atomicCAS(info, 0, d + 1);
                if (mailbox) pcg_post(mailbox, it, 1);
            }
            return;
        }
        const double beta = rz_new / rz_in;
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) pmu_new[k] = fma(beta, pmu_in[k], mu_new[k]);
        for (int e = row0 + tid; e < row1; e += 256) r_out[e] = pl[e];      // pl holds r_new
        __syncthreads();
        for (int e0 = tid; e0 < d; e0 += 256 * 8) {
            double pv8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; pv8[u] = p_in[e < d ? e : d - 1]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; if (e < d) pl[e] = pl[e] + beta * pv8[u]; }
        }
        __syncthreads();
        for (int e = row0 + tid; e < row1; e += 256) p_out[e] = pl[e];
        if (blockIdx.x == 0 && tid == 0) { const int it = flags[PF_ITERS] + 1; flags[PF_ITERS] = it; flags[PF_XBUF] = out; if (mailbox) pcg_post(mailbox, it, 0); }
    }
    if (blockIdx.x == 0 && tid == 0) {
        st_out[PS_RZ] = rz_new;
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) { st_out[PS_C + k] = c_new[k]; st_out[PS_MU + k] = mu_new[k]; st_out[PS_PMU + k] = pmu_new[k]; }
    }
    if (COARSE && tid < PCG_NW) red[32 + tid] = pmu_new[tid];
    __syncthreads();
    // q = S~ p_r + AW p_mu for the rows this workgroup owns: each wave takes rows (row0 + w + 4k), two at a time
    double pqp = 0.0, gacc = 0.0;
    const int nd2 = d >> 1, nd4 = d >> 2;
    for (int row = row0 + w; row < row1; row += 8) {
        const int rowb = (row + 4 < row1) ? row + 4 : row;
        double sa = 0.0, sb = 0.0;
        if (COARSE && lane < PCG_NW) {
            sa = AW[(size_t)row * PCG_NW + lane] * red[32 + lane];
            sb = AW[(size_t)rowb * PCG_NW + lane] * red[32 + lane];
        }
        if (sizeof(FT) == 8) {
            const double2* pl2 = reinterpret_cast<const double2*>(pl);
            const double2* Fa = reinterpret_cast<const double2*>(F + (size_t)row * ld);
            const double2* Fb = reinterpret_cast<const double2*>(F + (size_t)rowb * ld);
            int c = lane;
            for (; c + 192 < nd2; c += 256) {
                double2 a[4], b[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) { a[m] = Fa[c + 64 * m]; b[m] = Fb[c + 64 * m]; }
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const double2 pv = pl2[c + 64 * m];
                    sa += a[m].x * pv.x + a[m].y * pv.y;
                    sb += b[m].x * pv.x + b[m].y * pv.y;
                }
            }
            for (; c < nd2; c += 64) {
                const double2 a = Fa[c], b = Fb[c], pv = pl2[c];
                sa += a.x * pv.x + a.y * pv.y;
                sb += b.x * pv.x + b.y * pv.y;
            }
            if ((d & 1) && lane == 0) {
                sa += (double)F[(size_t)row * ld + d - 1] * pl[d - 1];
                sb += (double)F[(size_t)rowb * ld + d - 1] * pl[d - 1];
            }
        } else {
            // fp32 matrix: 16-byte loads of four columns, products and sums in fp64
            const float4* Fa = reinterpret_cast<const float4*>(F + (size_t)row * ld);
            const float4* Fb = reinterpret_cast<const float4*>(F + (size_t)rowb * ld);
            int c = lane;
            for (; c + 192 < nd4; c += 256) {
                float4 a[4], b[4];
                const bool first = pre && row == row0 + w && c == lane;       // (wave-uniform) the batch requested before the vector phase
                if (first) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) { a[m] = pre_a[m]; b[m] = pre_b[m]; }
                } else {
#pragma unroll
                    for (int m = 0; m < 4; ++m) { a[m] = Fa[c + 64 * m]; b[m] = Fb[c + 64 * m]; }
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const double2 p0 = reinterpret_cast<const double2*>(pl)[2 * (c + 64 * m)], p1 = reinterpret_cast<const double2*>(pl)[2 * (c + 64 * m) + 1];
                    sa += (double)a[m].x * p0.x + (double)a[m].y * p0.y + (double)a[m].z * p1.x + (double)a[m].w * p1.y;
                    sb += (double)b[m].x * p0.x + (double)b[m].y * p0.y + (double)b[m].z * p1.x + (double)b[m].w * p1.y;
                }
            }
            for (; c < nd4; c += 64) {
                const float4 a = Fa[c], b = Fb[c];
                const double2 p0 = reinterpret_cast<const double2*>(pl)[2 * c], p1 = reinterpret_cast<const double2*>(pl)[2 * c + 1];
                sa += (double)a.x * p0.x + (double)a.y * p0.y + (double)a.z * p1.x + (double)a.w * p1.y;
                sb += (double)b.x * p0.x + (double)b.y * p0.y + (double)b.z * p1.x + (double)b.w * p1.y;
            }
            if (lane == 0) {
                for (int cc = 4 * nd4; cc < d; ++cc) {
                    sa += (double)F[(size_t)row * ld + cc] * pl[cc];
                    sb += (double)F[(size_t)rowb * ld + cc] * pl[cc];
                }
            }
        }
        { sa = wave_allsum(sa); sb = wave_allsum(sb); }
        if (lane == 0) {
            q_out[row] = sa; pqp += pl[row] * sa;
            if (rowb != row) { q_out[rowb] = sb; pqp += pl[rowb] * sb; }
        }
        if (COARSE && lane >= 8 && lane < 8 + PCG_NW) {
            gacc = fma(W[(size_t)(lane - 8) * ld + row], sa, gacc);
            if (rowb != row) gacc = fma(W[(size_t)(lane - 8) * ld + rowb], sb, gacc);
        }
    }
    if (lane == 0) red[40 + 9 * w] = pqp;
    if (COARSE && lane >= 8 && lane < 8 + PCG_NW) red[40 + 9 * w + 1 + (lane - 8)] = gacc;
    __syncthreads();
    if (tid < NV) pcg_part(part, out, tid)[blockIdx.x] = red[40 + tid] + red[49 + tid] + red[58 + tid] + red[67 + tid];
}

// AW, the partials of E and c_0 (one extra pass over S~ per linear solve), then the 8 x 8 inverse (k_pcg_coarse_invert, pcg_fast.hip)
void pcg_streaming_setup(hipStream_t s, const DenseSolver* ws, Profiler* prof) {
    const CgPath& r = ws->run.path;
    if (!r.coarse) return;
    ProfScope ps(prof, KID_PCG_SETUP, s, 2);
#define SFMBA_CO(FT, NR, Fptr) hipLaunchKernelGGL((k_pcg_coarse<FT, NR>), dim3(r.nwg), dim3(256), 0, s, ws->d, ws->ld, Fptr, ws->W, pcg_btilde(ws), ws->AW, ws->epart, r.rows_per_wg)
    if (r.f32) { if (r.rows_per_wg <= 8) SFMBA_CO(float, 2, ws->Sfull32); else SFMBA_CO(float, CO_MAXROWS, ws->Sfull32); }
    else { if (r.rows_per_wg <= 8) SFMBA_CO(double, 2, ws->Sfull); else SFMBA_CO(double, CO_MAXROWS, ws->Sfull); }
#undef SFMBA_CO
    pcg_coarse_invert(s, r.nwg, ws->epart, ws->coarse);
}

void pcg_streaming_iterate(hipStream_t s, const DenseSolver* ws, bool init, int in, int anchor, double cap) {
    const DenseSolver::CgRun& run = ws->run;
    const CgPath& r = run.path;
    // (above 64 KiB of dynamic LDS -- ld > 7 840 -- the instantiation's limit is raised once, to what dense_pcg_path admits at the most)
#define SFMBA_IT(INIT, FT, C, Fptr) do { \
        static bool attr_set = false; \
        if (r.lds > PCG_LDS_DEFAULT && !attr_set) { (void)hipFuncSetAttribute((const void*)k_pcg_iter<INIT, FT, C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PCG_LDS_GFX950); attr_set = true; } \
        hipLaunchKernelGGL((k_pcg_iter<INIT, FT, C>), dim3(r.nwg), dim3(256), r.lds, s, ws->d, ws->ld, Fptr, ws->vec, pcg_btilde(ws), ws->part, ws->scal, \
        ws->flags, r.rows_per_wg, run.tol2, in, run.info, ws->d_mailbox, anchor, cap, ws->W, ws->AW, ws->coarse); } while (0)
    if (r.f32) {
        if (r.coarse) { if (init) SFMBA_IT(true, float, true, ws->Sfull32); else SFMBA_IT(false, float, true, ws->Sfull32); }
        else { if (init) SFMBA_IT(true, float, false, ws->Sfull32); else SFMBA_IT(false, float, false, ws->Sfull32); }
    } else {
        if (r.coarse) { if (init) SFMBA_IT(true, double, true, ws->Sfull); else SFMBA_IT(false, double, true, ws->Sfull); }
        else { if (init) SFMBA_IT(true, double, false, ws->Sfull); else SFMBA_IT(false, double, false, ws->Sfull); }
    }
#undef SFMBA_IT
}

}  // namespace sfmba
