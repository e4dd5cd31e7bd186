// pcg_segments_streaming.hip -- the streaming segmented CG family (1280 < d <= 8192, camera paths): classical PCG with up to 141 hat-restricted gauge
// vectors, three launches per iteration (k_sg_q or k_sg_q_sparse, k_sg_u, k_sg_p), set-up k_sg_v, k_sg_e, k_sg_invert.
#include "pcg_common.h"
#include "../../include/sfmba.h"

namespace sfmba {

// ---------------------------------------------------------------------------------------------------------------------
// Segmented coarse space on the STREAMING path (d > 1280: long camera paths -- 600 cameras of a path need 314 .. 396 CG iterations per
// linearisation with the eight global vectors, tools/large_banded_check.py).  Same coarse space as above with G = cameras / 25 hats (at most 20:
// 7 G + 1 <= 141 vectors), but a coarse operator of that size cannot ride in every workgroup of a fused launch (E^-1 is 166 KB), and the search
// direction need not be kept split: classical PCG with M^-1 = I + W~ E^-1 W~^T in THREE launches per iteration --
//   k_sg_q   q = S~ p for the rows of a workgroup (the streaming product of k_pcg_iter), per-workgroup partials of p . q
//   k_sg_u   alpha; x += alpha p, r -= alpha q on the rows of a workgroup's cameras; per camera t_k = sum of W~_k[row] r[row]; partials of |r|^2
//   k_sg_p   |r|^2 (the stopping test), c = W~^T r from the t_k per hat, mu = E^-1 c, r . z = |r|^2 + c . mu, beta, p = r + W~ mu + beta p
// (the coarse solve is formed by each of the SG_UWG workgroups of k_sg_p for itself).  Set-up per linear solve: k_sg_v (per camera: the pieces of E
// and c_0, AW is never stored), k_sg_e (E, hat sums), k_sg_invert (Gauss-Jordan in the registers of one workgroup -- what limits the hats to 20,
// see there).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SG_CB = 36;                   // columns per part of the E^-1 c product (SG_NCP / 4)
constexpr int SG_UT = 1024;                 // ... and their threads
constexpr int SG_TC = 64;                   // cameras per column tile of k_sg_v

__device__ __forceinline__ int sg_first_cam(int a, int nc, int G) { return (a * nc + G - 1) / G; }
__device__ __forceinline__ double sg_frac(int j, int a, int nc, int G, double inv_nc) { return (double)(j * G - a * nc) * inv_nc; }

// per camera j (workgroup; the last one: the focal row): V[j][8][SG_NCP] = sum over the camera's rows of W~_k[row] (S~ W~)[row][:].  Column tiles of
// SG_TC cameras, two phases per tile through LDS: (1) T[row][camera][k] = the 6-term product of the camera's row entries with W~_k, one item per thread
// and step -- k = 7 is the global vector's share --, (2) lane + 64 pass = coarse vector (g, k) adds hat_g(camera) T over the cameras of its hat inside the
// tile.  (With the 6-term products inside phase 2, every wave ran as long as its busiest lane's hat: 187 us.)
template <typename FT>
__global__ __launch_bounds__(256) void k_sg_v(int d, int ld, int G, const FT* __restrict__ F, const double* __restrict__ W,
                                              double* __restrict__ V) {
    constexpr int TW = 6 * SG_TC;
    __shared__ __align__(16) double rows[6 * TW];               // [6][TW]
    __shared__ __align__(16) float wt[PCG_NW * TW];             // [8][TW]
    __shared__ double T[6 * SG_TC * PCG_NW];                    // [6][SG_TC][8]
    __shared__ double vbuf[4 * SG_NCP];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nc = (d - 1) / 6, NC = 7 * G + 1;
    const double inv_nc = 1.0 / (double)nc;
    const int row0 = 6 * blockIdx.x, row1 = min(d, row0 + 6);
    const int ra = w, rb = w + 4;
    const bool have_a = row0 + ra < row1, have_b = row0 + rb < row1;
    double acc[2][3], gs[2] = { 0.0, 0.0 };
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int p = 0; p < 3; ++p) acc[r][p] = 0.0;
    for (int c0 = 0; c0 < nc; c0 += SG_TC) {
        const int col0 = 6 * c0, ncol = min(6 * nc - col0, TW);
        // all loads of the tile first (9 + 12 per thread, clamped, branch-free), then the LDS stores
        FT fr_[6 * TW / 256];
        double wr_[PCG_NW * TW / 256];
#pragma unroll
        for (int u = 0; u < 6 * TW / 256; ++u) {
            const int e = tid + 256 * u, r = e / TW, c = e - TW * r;
            const bool ok = row0 + r < row1 && c < ncol;
            fr_[u] = F[(size_t)(ok ? row0 + r : row0) * ld + col0 + (ok ? c : 0)];
        }
#pragma unroll
        for (int u = 0; u < PCG_NW * TW / 256; ++u) {
            const int e = tid + 256 * u, k = e / TW, c = e - TW * k;
            wr_[u] = W[(size_t)k * ld + col0 + (c < ncol ? c : 0)];
        }
        __syncthreads();                                         // (the previous tile's phase 2 is done with T, rows, wt)
#pragma unroll
        for (int u = 0; u < 6 * TW / 256; ++u) {
            const int e = tid + 256 * u, r = e / TW, c = e - TW * r;
            rows[e] = (row0 + r < row1 && c < ncol) ? (double)fr_[u] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < PCG_NW * TW / 256; ++u) {
            const int e = tid + 256 * u, c = e % TW;
            wt[e] = c < ncol ? (float)wr_[u] : 0.0f;
        }
        __syncthreads();
        // (1) T[r][camera][k]
#pragma unroll
        for (int u = 0; u < 6 * SG_TC * PCG_NW / 256; ++u) {
            const int item = tid + 256 * u, r = item / (SG_TC * PCG_NW), rem = item - (SG_TC * PCG_NW) * r, cam = rem / PCG_NW, k = rem - PCG_NW * cam;
            const double* rp = rows + r * TW + 6 * cam;
            const float* wk = wt + k * TW + 6 * cam;
            double t = 0.0;
#pragma unroll
            for (int e = 0; e < 6; ++e) t = fma(rp[e], (double)wk[e], t);
            T[item] = t;
        }
        __syncthreads();
        // (2) hat sums
        const int c1 = min(nc, c0 + SG_TC);
        const double* Ta = T + (size_t)ra * SG_TC * PCG_NW;
        const double* Tb = T + (size_t)(have_b ? rb : ra) * SG_TC * PCG_NW;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int v = lane + 64 * p;
            if (v < NC - 1) {
                const int g = v / 7, k = v - 7 * g;
                for (int range = 0; range < 2; ++range) {
                    const int a = range == 0 ? (g + G - 1) % G : g;
                    const int lo = max(sg_first_cam(a, nc, G), c0), hi = min(sg_first_cam(a + 1, nc, G), c1);
                    for (int j = lo; j < hi; ++j) {
                        const double fr = sg_frac(j, a, nc, G, inv_nc);
                        const double wgt = range == 0 ? fr : 1.0 - fr;
                        acc[0][p] = fma(wgt, Ta[(j - c0) * PCG_NW + k], acc[0][p]);
                        acc[1][p] = fma(wgt, Tb[(j - c0) * PCG_NW + k], acc[1][p]);
                    }
                }
            }
        }
        if (c0 + lane < c1) { gs[0] += Ta[lane * PCG_NW + (PCG_NW - 1)]; gs[1] += Tb[lane * PCG_NW + (PCG_NW - 1)]; }     // the global (focal / depth) vector
    }
    gs[0] = wave_allsum(gs[0]); gs[1] = wave_allsum(gs[1]);
    {   // the focal column
        const double wf = W[(size_t)(PCG_NW - 1) * ld + d - 1];
        if (have_a) gs[0] = fma((double)F[(size_t)(row0 + ra) * ld + d - 1], wf, gs[0]);
        if (have_b) gs[1] = fma((double)F[(size_t)(row0 + rb) * ld + d - 1], wf, gs[1]);
    }
    if (!have_a) { gs[0] = 0.0; acc[0][0] = acc[0][1] = acc[0][2] = 0.0; }
    if (!have_b) { gs[1] = 0.0; acc[1][0] = acc[1][1] = acc[1][2] = 0.0; }
    if (lane + 128 == NC - 1) { acc[0][2] = gs[0]; acc[1][2] = gs[1]; }
    if (lane + 64 == NC - 1) { acc[0][1] = gs[0]; acc[1][1] = gs[1]; }
    if (lane == NC - 1) { acc[0][0] = gs[0]; acc[1][0] = gs[1]; }
    // V[k][:] = sum over the camera's rows of W~_k[row] AW[row][:], wave partials summed through LDS, one k at a time
    double wab[PCG_NW][2];
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k) { wab[k][0] = have_a ? W[(size_t)k * ld + row0 + ra] : 0.0; wab[k][1] = have_b ? W[(size_t)k * ld + row0 + rb] : 0.0; }
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k) {
        const double wa = wab[k][0], wb = wab[k][1];
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 3; ++p) if (lane + 64 * p < SG_NCP) vbuf[w * SG_NCP + lane + 64 * p] = fma(wa, acc[0][p], wb * acc[1][p]);
        __syncthreads();
        if (tid < SG_NCP) V[((size_t)blockIdx.x * PCG_NW + k) * SG_NCP + tid] = (vbuf[tid] + vbuf[SG_NCP + tid]) + (vbuf[2 * SG_NCP + tid] + vbuf[3 * SG_NCP + tid]);
    }
}

// E[i][:]: one workgroup per coarse vector, 3 x SG_NCP threads (a third of the terms each)
__global__ __launch_bounds__(3 * SG_NCP) void k_sg_e(int d, int G, const double* __restrict__ V, double* __restrict__ E) {
    __shared__ double eq[3][SG_NCP];
    const int i = blockIdx.x, tid = threadIdx.x, v = tid % SG_NCP, part = tid / SG_NCP;
    const int nc = (d - 1) / 6, NC = 7 * G + 1;
    const double inv_nc = 1.0 / (double)nc;
    double e = 0.0;
    if (i < NC - 1) {
        const int g = i / 7, k = i - 7 * g;
        for (int range = 0; range < 2; ++range) {
            const int a = range == 0 ? (g + G - 1) % G : g;
            const int lo = sg_first_cam(a, nc, G), hi = sg_first_cam(a + 1, nc, G);
            for (int jb = lo + part; jb < hi; jb += 3 * 8) {               // eight loads in flight (clamped, branch-free)
                double val[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) { const int j = jb + 3 * t; val[t] = V[((size_t)(j < hi ? j : lo) * PCG_NW + k) * SG_NCP + v]; }
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const int j = jb + 3 * t;
                    const double fr = sg_frac(j, a, nc, G, inv_nc);
                    e = fma(j < hi ? (range == 0 ? fr : 1.0 - fr) : 0.0, val[t], e);
                }
            }
        }
    } else {
        for (int jb = part; jb <= nc; jb += 3 * 16) {                       // the plain sum over all workgroups: sixteen loads in flight
            double val[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) { const int j = jb + 3 * t; val[t] = V[((size_t)(j <= nc ? j : nc) * PCG_NW + (PCG_NW - 1)) * SG_NCP + v]; }
#pragma unroll
            for (int t = 0; t < 16; ++t) e += (jb + 3 * t <= nc) ? val[t] : 0.0;
        }
    }
    eq[part][v] = e;
    __syncthreads();
    if (tid < SG_NCP) E[(size_t)i * SG_NCP + tid] = (eq[0][tid] + eq[1][tid]) + eq[2][tid];
}

// E^-1 (SG_NCP x SG_NCP): gj_invert_tiled with 6 x 4 tiles on 864 threads (24 entries per thread).  (History: 27 hats -- 192 rows, a slice of 48 or 40
// columns per thread -- spilled two dozen doubles per thread in every step whatever the scheduling hints: 1.3 ms; hence the limit of 20 hats.  21
// columns per thread on 1008 threads: 219 us, bound by the LDS reads of the pivot row.)
constexpr int SG_ITR = 6, SG_ITC = 4, SG_ITHREADS = (SG_NCP / SG_ITR) * (SG_NCP / SG_ITC);
__global__ __launch_bounds__(SG_ITHREADS) void k_sg_invert(int NC, const double* __restrict__ E, double* __restrict__ einv) {
    __shared__ double rowbuf[2 * SG_NCP], colbuf[2 * SG_NCP], sc[SG_NCP], diagbuf[2];
    __shared__ unsigned char drop[SG_NCP + 1];
    gj_invert_tiled<SG_NCP, SG_ITR, SG_ITC, 12>(NC, E, einv, rowbuf, colbuf, sc, diagbuf, drop);
}

// q = S~ p for the rows of this workgroup (eight; two per wave at a time), partial of p . q
template <typename FT>
__global__ __launch_bounds__(256) void k_sg_q(int d, int ld, const FT* __restrict__ F, const double* __restrict__ p, double* __restrict__ q,
                                              double* __restrict__ pqpart, const int* __restrict__ flags, int rows_per_wg) {
    extern __shared__ __align__(16) double sm[];
    double* pl = sm;
    __shared__ double red[4];
    if (flags[PF_DONE] != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row0 = blockIdx.x * rows_per_wg, row1 = min(d, row0 + rows_per_wg);
    for (int e0 = tid; e0 < ld; e0 += 256 * 8) {
        double pv8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; pv8[u] = p[e < d ? e : d - 1]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; if (e < ld) pl[e] = e < d ? pv8[u] : 0.0; }
    }
    __syncthreads();
    double pqp = 0.0;
    const int nd2 = d >> 1, nd4 = d >> 2;
    for (int row = row0 + w; row < row1; row += 8) {
        const int rowb = (row + 4 < row1) ? row + 4 : row;
        double sa = 0.0, sb = 0.0;
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
                for (int m = 0; m < 4; ++m) { const double2 pv = pl2[c + 64 * m]; sa += a[m].x * pv.x + a[m].y * pv.y; sb += b[m].x * pv.x + b[m].y * pv.y; }
            }
            for (; c < nd2; c += 64) { const double2 a = Fa[c], b = Fb[c], pv = pl2[c]; sa += a.x * pv.x + a.y * pv.y; sb += b.x * pv.x + b.y * pv.y; }
            if ((d & 1) && lane == 0) { sa += (double)F[(size_t)row * ld + d - 1] * pl[d - 1]; sb += (double)F[(size_t)rowb * ld + d - 1] * pl[d - 1]; }
        } else {
            const float4* Fa = reinterpret_cast<const float4*>(F + (size_t)row * ld);
            const float4* Fb = reinterpret_cast<const float4*>(F + (size_t)rowb * ld);
            int c = lane;
            for (; c + 192 < nd4; c += 256) {
                float4 a[4], b[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) { a[m] = Fa[c + 64 * m]; b[m] = Fb[c + 64 * m]; }
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
            if (lane == 0) for (int cc = 4 * nd4; cc < d; ++cc) { sa += (double)F[(size_t)row * ld + cc] * pl[cc]; sb += (double)F[(size_t)rowb * ld + cc] * pl[cc]; }
        }
        sa = wave_allsum(sa); sb = wave_allsum(sb);
        if (lane == 0) {
            q[row] = sa; pqp += pl[row] * sa;
            if (rowb != row) { q[rowb] = sb; pqp += pl[rowb] * sb; }
        }
    }
    if (lane == 0) red[w] = pqp;
    __syncthreads();
    if (tid == 0) pqpart[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The same product for a SPARSELY FILLED S~ (a long camera path: 6 % of the blocks hold anything): workgroup = camera (six rows; the last workgroup: the
// focal row, dense), the cameras it shares a non-empty block with come from the structure build's bit mask (k_block_mask; the camera itself included:
// S~_jj = I), compacted into LDS; lanes walk (neighbour, entry) pairs -- six consecutive lanes read the 24 / 48 contiguous bytes of a block row -- and
// read p from L2.  Empty blocks of S~ are exact zeros (the pair pass writes them), so this IS the dense product.
template <typename FT>
__global__ __launch_bounds__(256) void k_sg_q_sparse(int d, int ld, const FT* __restrict__ F, const double* __restrict__ p, double* __restrict__ q,
                                                     double* __restrict__ pqpart, const int* __restrict__ flags, const unsigned* __restrict__ mask) {
    __shared__ int list[1024];
    __shared__ int wcount[4], nn_s;
    __shared__ double red[4];
    if (flags[PF_DONE] != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nc = (d - 1) / 6, words = (nc + 31) / 32, ja = blockIdx.x;
    double pqp = 0.0;
    if (ja < nc) {
        // compact the set bits of mask[ja] into list (ascending): ballot + popcount per wave, wave offsets through LDS
        int base = 0;
        for (int c0 = 0; c0 < nc; c0 += 256) {
            const int c = c0 + tid;
            const bool on = c < nc && ((mask[(size_t)ja * words + (c >> 5)] >> (c & 31)) & 1u);
            const unsigned long long bal = __ballot(on);
            if (lane == 0) wcount[w] = __popcll(bal);
            __syncthreads();
            int off = base;
            for (int k = 0; k < w; ++k) off += wcount[k];
            if (on) list[off + __popcll(bal & ((1ull << lane) - 1ull))] = c;
            base += wcount[0] + wcount[1] + wcount[2] + wcount[3];
            __syncthreads();
        }
        if (tid == 0) nn_s = base;
        __syncthreads();
        const int nn = nn_s;
        const double pf = p[d - 1];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int r = w + 4 * rr;
            if (r < 6) {
                const int row = 6 * ja + r;
                const FT* Fr = F + (size_t)row * ld;
                double s = 0.0;
                for (int idx0 = lane; idx0 < 6 * nn; idx0 += 64 * 4) {          // four gathers in flight
                    double fv[4], pv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int idx = idx0 + 64 * u, ic = idx < 6 * nn ? idx : 0;
                        const int col = 6 * list[ic / 6] + ic % 6;
                        fv[u] = (double)Fr[col]; pv[u] = p[col];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) s = fma(idx0 + 64 * u < 6 * nn ? fv[u] : 0.0, pv[u], s);
                }
                if (lane == 0) s = fma((double)Fr[d - 1], pf, s);
                s = wave_allsum(s);
                if (lane == 0) { q[row] = s; pqp += p[row] * s; }
            }
        }
    } else if (w == 0) {                             // the focal row: dense
        const FT* Fr = F + (size_t)(d - 1) * ld;
        double s = 0.0;
        for (int c = lane; c < d; c += 64) s = fma((double)Fr[c], p[c], s);
        s = wave_allsum(s);
        if (lane == 0) { q[d - 1] = s; pqp = p[d - 1] * s; }
    }
    if (lane == 0) red[w] = pqp;
    __syncthreads();
    if (tid == 0) pqpart[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// block sum over SG_UT threads (every thread gets the total); scratch: 16 doubles
__device__ __forceinline__ double sg_block_sum(double v, double* scratch) {
    v = wave_allsum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < SG_UT / 64; ++k) s += scratch[k];
    return s;
}
// cameras (and the focal pseudo-camera nc) of vector workgroup g: [sg_cam0(g), sg_cam0(g + 1)) of nc + 1
__device__ __forceinline__ int sg_cam0(int g, int nc) { return (int)(((long long)g * (nc + 1)) / SG_UWG); }

// INIT: x = 0, r = b~.  Else: alpha = r.z / p.q; x += alpha p; r -= alpha q.  Both: t_k per camera, the workgroup's share of |r|^2.
template <bool INIT>
__global__ __launch_bounds__(SG_UT) void k_sg_u(int d, int ld, int nwgq, const double* __restrict__ bt, double* __restrict__ x, double* __restrict__ r,
                                                const double* __restrict__ p, const double* __restrict__ q, const double* __restrict__ W,
                                                const double* __restrict__ pqpart, double* __restrict__ tcam, double* __restrict__ rrpart,
                                                double* __restrict__ state, const int* __restrict__ flags, int in) {
    __shared__ double scratch[16];
    __shared__ double rl[6 * 64 + 8];                 // the workgroup's rows of the new r (at most ceil(1001 / 16) = 63 cameras)
    if (!INIT && flags[PF_DONE] != 0) return;
    const int tid = threadIdx.x;
    const int nc = (d - 1) / 6;
    const int j0 = sg_cam0(blockIdx.x, nc), j1 = sg_cam0(blockIdx.x + 1, nc);
    const int r0 = 6 * j0, r1 = min(d, 6 * j1), nrows = r1 - r0;
    double alpha = 0.0;
    if (!INIT) {
        double s = 0.0;
        for (int wg = tid; wg < nwgq; wg += SG_UT) s += pqpart[wg];
        const double pq = sg_block_sum(s, scratch);
        alpha = state[SGS_LEN * in + SGS_RZ] / pq;
        if (blockIdx.x == 0 && tid == 0) state[SGS_LEN * in + SGS_PQ] = pq;
    }
    double rr = 0.0;
    if (tid < nrows) {
        const int row = r0 + tid;
        double rn;
        if (INIT) { rn = bt[row]; x[row] = 0.0; }
        else { x[row] += alpha * p[row]; rn = r[row] - alpha * q[row]; }
        r[row] = rn;
        rl[tid] = rn;
        rr = rn * rn;
    }
    rr = sg_block_sum(rr, scratch);                   // (also the barrier behind rl)
    if (tid == 0) rrpart[blockIdx.x] = rr;
    if (tid < PCG_NW * (j1 - j0)) {
        const int jl = tid / PCG_NW, k = tid - PCG_NW * jl, j = j0 + jl;
        double t = 0.0;
        if (j < nc) {
#pragma unroll
            for (int e = 0; e < 6; ++e) t = fma(W[(size_t)k * ld + 6 * j + e], rl[6 * jl + e], t);
        } else t = W[(size_t)k * ld + d - 1] * rl[6 * jl];          // the focal row
        tcam[(size_t)j * PCG_NW + k] = t;
    }
}

// |r|^2 and the stopping test; c = W~^T r (hat sums of the t_k), mu = E^-1 c, r . z = |r|^2 + c . mu, beta; p = r + W~ mu + beta p on the workgroup's rows
template <bool INIT>
__global__ __launch_bounds__(SG_UT) void k_sg_p(int d, int ld, int G, const double* __restrict__ r, double* __restrict__ p, const double* __restrict__ W,
                                                const double* __restrict__ tcam, const double* __restrict__ rrpart, const double* __restrict__ einv,
                                                double* __restrict__ state, double* __restrict__ scal, int* __restrict__ flags, int* info, int* mailbox,
                                                double tol2, int in, int anchor, double cap) {
    __shared__ double scratch[16];
    __shared__ double cl[SG_NCP], ml[SG_NCP], mp[4][SG_NCP];
    if (!INIT && flags[PF_DONE] != 0) return;
    const int tid = threadIdx.x, out = in ^ 1;
    const int nc = (d - 1) / 6, NC = 7 * G + 1;
    const double inv_nc = 1.0 / (double)nc;
    double rr = 0.0;
#pragma unroll
    for (int k = 0; k < SG_UWG; ++k) rr += rrpart[k];
    if (INIT) {
        if (blockIdx.x == 0 && tid == 0) {
            scal[PS_RR0] = pcg_threshold_base(rr, scal, anchor, cap); flags[PF_DONE] = (rr == 0.0); flags[PF_ITERS] = 0; flags[PF_XBUF] = 0;
            if (mailbox && rr == 0.0) pcg_post(mailbox, 0, 1);
        }
        if (rr == 0.0) return;
    } else {
        const double pq = state[SGS_LEN * in + SGS_PQ];
        const bool broke = !(pq > 0.0) || !(rr == rr);
        if (rr <= tol2 * scal[PS_RR0] || broke) {
            if (blockIdx.x == 0 && tid == 0) {
                flags[PF_XBUF] = 0; const int it = flags[PF_ITERS] + 1; flags[PF_ITERS] = it;
                if (broke) atomicCAS(info, 0, d + 1);
                __threadfence();
                flags[PF_DONE] = 1;
                if (mailbox) pcg_post(mailbox, it, 1);
            }
            return;
        }
    }
    // c: vector i = tid % SG_NCP, a quarter of its hat's cameras per part = tid / SG_NCP (eight loads in flight); the global vector by a block sum
    {
        double t7 = 0.0;
        for (int j = tid; j <= nc; j += SG_UT) t7 += tcam[(size_t)j * PCG_NW + (PCG_NW - 1)];
        t7 = sg_block_sum(t7, scratch);
        double c = 0.0;
        const int i = tid % SG_NCP, part = tid / SG_NCP;
        if (part < 4 && i < NC - 1) {
            const int g = i / 7, k = i - 7 * g;
            const int a = (part >> 1) == 0 ? (g + G - 1) % G : g;
            const int lo = sg_first_cam(a, nc, G), hi = sg_first_cam(a + 1, nc, G);
            const int half = (hi - lo + 1) >> 1;
            const int jb0 = (part & 1) ? lo + half : lo, jb1 = (part & 1) ? hi : min(hi, lo + half);
            for (int jb = jb0; jb < jb1; jb += 8) {
                double val[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) val[t] = tcam[(size_t)(jb + t < jb1 ? jb + t : jb1 - 1) * PCG_NW + k];
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const double fr = sg_frac(jb + t, a, nc, G, inv_nc);
                    c = fma(jb + t < jb1 ? ((part >> 1) == 0 ? fr : 1.0 - fr) : 0.0, val[t], c);
                }
            }
        }
        if (part < 4) mp[part][i] = c;
        __syncthreads();
        if (tid < SG_NCP) cl[tid] = tid < NC - 1 ? (mp[0][tid] + mp[1][tid]) + (mp[2][tid] + mp[3][tid]) : tid == NC - 1 ? t7 : 0.0;
    }
    __syncthreads();
    if (tid < 4 * SG_NCP) {
        const int i = tid % SG_NCP, part = tid / SG_NCP;
        double s = 0.0;
#pragma unroll 8
        for (int jj = 0; jj < SG_CB; ++jj) { const int j = SG_CB * part + jj; s = fma(einv[(size_t)j * SG_NCP + i], cl[j], s); }
        mp[part][i] = s;
    }
    __syncthreads();
    if (tid < SG_NCP) ml[tid] = (mp[0][tid] + mp[1][tid]) + (mp[2][tid] + mp[3][tid]);
    __syncthreads();
    const double cmu = sg_block_sum(tid < SG_NCP ? cl[tid] * ml[tid] : 0.0, scratch);
    const double rz_new = rr + cmu;
    const double beta = INIT ? 0.0 : rz_new / state[SGS_LEN * in + SGS_RZ];
    // p on the rows of this workgroup's cameras
    const int j0 = sg_cam0(blockIdx.x, nc), j1 = sg_cam0(blockIdx.x + 1, nc);
    const int r0 = 6 * j0, r1 = min(d, 6 * j1);
    if (r0 + tid < r1) {
        const int row = r0 + tid;
        const int j = min(row / 6, nc - 1);           // (the focal row: W~_0..6 are zero there)
        const int gl = (j * G) / nc, gh = gl + 1 == G ? 0 : gl + 1;
        const double fr = sg_frac(j, gl, nc, G, inv_nc);
        double z = fma(W[(size_t)(PCG_NW - 1) * ld + row], ml[NC - 1], r[row]);
#pragma unroll
        for (int k = 0; k < 7; ++k) z = fma(W[(size_t)k * ld + row], fma(fr, ml[7 * gh + k], (1.0 - fr) * ml[7 * gl + k]), z);
        p[row] = INIT ? z : fma(beta, p[row], z);
    }
    if (blockIdx.x == 0 && tid == 0) {
        state[SGS_LEN * out + SGS_RZ] = rz_new;
        if (!INIT) { const int it = flags[PF_ITERS] + 1; flags[PF_ITERS] = it; if (mailbox) pcg_post(mailbox, it, 0); }
    }
}

void pcg_segments_streaming_setup(hipStream_t s, const DenseSolver* ws, Profiler* prof) {
    const CgPath& r = ws->run.path;
    const int d = ws->d, ld = ws->ld;
    ProfScope ps(prof, KID_PCG_SETUP, s, 3);
    const int nc = (d - 1) / 6, G = sg_hats(nc), NC = 7 * G + 1;
    if (r.f32) hipLaunchKernelGGL((k_sg_v<float>), dim3(nc + 1), dim3(256), 0, s, d, ld, G, ws->Sfull32, ws->W, ws->sgV);
    else hipLaunchKernelGGL((k_sg_v<double>), dim3(nc + 1), dim3(256), 0, s, d, ld, G, ws->Sfull, ws->W, ws->sgV);
    hipLaunchKernelGGL(k_sg_e, dim3(NC), dim3(3 * SG_NCP), 0, s, d, G, ws->sgV, ws->sgE);
    hipLaunchKernelGGL(k_sg_invert, dim3(1), dim3(SG_ITHREADS), 0, s, NC, ws->sgE, ws->sgEinv);
}

// the first launch pair initialises (x = 0, r = b~, p = z); an iteration is the product -- block-sparse for SFMBA_FAMILY_PCG_SEGMENTS_STREAMING_SPARSE
// (a reduced matrix filled below a quarter: one workgroup per camera), dense otherwise -- then k_sg_u and k_sg_p
void pcg_segments_streaming_iterate(hipStream_t s, const DenseSolver* ws, bool init, int in, int anchor, double cap) {
    const DenseSolver::CgRun& run = ws->run;
    const CgPath& r = run.path;
    const int d = ws->d, ld = ws->ld;
    const int G = sg_hats((d - 1) / 6);
    double* bt = pcg_btilde(ws);
    double *x = ws->vec, *rv = ws->vec + (size_t)2 * ld, *pv = ws->vec + (size_t)4 * ld, *qv = ws->vec + (size_t)6 * ld;      // the parity-0 buffers of pcg_vec
    const int par = in & 1;
    if (init) {
        hipLaunchKernelGGL((k_sg_u<true>), dim3(SG_UWG), dim3(SG_UT), 0, s, d, ld, r.nwg, bt, x, rv, pv, qv, ws->W, ws->part, ws->sgT, ws->sgRR, ws->sgState, ws->flags, par);
        hipLaunchKernelGGL((k_sg_p<true>), dim3(SG_UWG), dim3(SG_UT), 0, s, d, ld, G, rv, pv, ws->W, ws->sgT, ws->sgRR, ws->sgEinv, ws->sgState, ws->scal, ws->flags, run.info, ws->d_mailbox, run.tol2, par, anchor, cap);
        return;
    }
    const bool sparse = r.family == SFMBA_FAMILY_PCG_SEGMENTS_STREAMING_SPARSE;
    const int nwgq = sparse ? (d - 1) / 6 + 1 : r.nwg;
    if (sparse) {
        if (r.f32) hipLaunchKernelGGL((k_sg_q_sparse<float>), dim3(nwgq), dim3(256), 0, s, d, ld, ws->Sfull32, pv, qv, ws->part, ws->flags, ws->blk_mask);
        else hipLaunchKernelGGL((k_sg_q_sparse<double>), dim3(nwgq), dim3(256), 0, s, d, ld, ws->Sfull, pv, qv, ws->part, ws->flags, ws->blk_mask);
    } else if (r.f32) hipLaunchKernelGGL((k_sg_q<float>), dim3(r.nwg), dim3(256), r.lds, s, d, ld, ws->Sfull32, pv, qv, ws->part, ws->flags, r.rows_per_wg);
    else hipLaunchKernelGGL((k_sg_q<double>), dim3(r.nwg), dim3(256), r.lds, s, d, ld, ws->Sfull, pv, qv, ws->part, ws->flags, r.rows_per_wg);
    hipLaunchKernelGGL((k_sg_u<false>), dim3(SG_UWG), dim3(SG_UT), 0, s, d, ld, nwgq, bt, x, rv, pv, qv, ws->W, ws->part, ws->sgT, ws->sgRR, ws->sgState, ws->flags, par);
    hipLaunchKernelGGL((k_sg_p<false>), dim3(SG_UWG), dim3(SG_UT), 0, s, d, ld, G, rv, pv, ws->W, ws->sgT, ws->sgRR, ws->sgEinv, ws->sgState, ws->scal, ws->flags, run.info, ws->d_mailbox, run.tol2, par, anchor, cap);
}

}  // namespace sfmba
