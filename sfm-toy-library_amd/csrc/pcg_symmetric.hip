// pcg_symmetric.hip -- the symmetric streaming CG family (d > 1280, not for deterministic handles): ONE triangle of S~ read per iteration, two
// launches per iteration (k_sy_vec, k_sy_prod), the 8-vector coarse set-up on the same triangle (k_sy_coarse, k_sy_e, then k_pcg_coarse_invert of pcg_fast.hip).
#include "pcg_common.h"

namespace sfmba {

// ---------------------------------------------------------------------------------------------------------------------
// Symmetric streaming path (round 6).  S~ is symmetric: the CG reads ONE triangle of it per iteration -- 72 MB instead of
// 144 MB at d = 6001 -- and uses every entry twice from the one 16-byte load that brought it in:
//     q_i += U_ij p_j      (row use: summed across the wave by a halving butterfly)
//     q_j += U_ij p_i      (column use, j > i: kept per lane, summed across the four waves of the tile in LDS)
// over TILES of SY_R rows x SY_C columns of the scalar upper triangle (diagonal included; the lower triangle and the padding are never multiplied),
// ONE TILE PER WORKGROUP: every load of the product is in flight as soon as the launch starts (2 396 workgroups at d = 6001).  A row of q collects
// sums from every tile of its row strip and of its column chunk: fp64 device-scope atomics on a zeroed q buffer, every atomic instruction on
// CONSECUTIVE addresses (tools/micro/symv_bench.hip: the memory side retires ~6 G line-sized atomic transactions per second whatever they carry;
// 48 k of them per product cost nothing next to the stream -- 14.7 us = 4.9 TB/s of the 72 MB under rocprofv3, against 27 - 32 us for both triangles --,
// the 2 M of a form with one flush per wave and strided lanes cost 100 us).  In the solve: 17.9 us per launch, of which 15.0 the bare product and 1.8 the
// epilogue below (profiles/r06_ab_sy_prod_bisect.txt: occupancy, the prologue's scalar round trips, an unmasked path for interior tiles do not move it).
// What does NOT survive a grid of 2 396 workgroups is the vector phase of k_pcg_iter (every workgroup forms alpha, |r - alpha q|^2, beta from the
// whole vectors: 96 KB from L2 per workgroup -- measured +5 ... +10 us at 512 ... 1 024 workgroups in the same micro-benchmark, fused forms of the
// iteration land at 20 - 26 us).  So an iteration is TWO launches here:
//   k_sy_vec   (SY_VEC_WG workgroups) the scalars of the iteration, x, r, the new search direction p = p_r (its own slice of each), the stopping test;
//              zeroes its slice of the q buffer and of the partial sums the product is about to add into
//   k_sy_prod  (one workgroup per tile) the product; the slotted partial sums p_r . q; its first workgroups also add (S~ W~) p_mu to their slice of q
//              and form the partials of W~^T q = (S~ W~)^T p_r (+ E p_mu in k_sy_vec): S~ is symmetric, so W~^T S~ p_r needs no pass over W~ per tile
// q and the partial sums are double-buffered by iteration parity like the other vectors.  Not for deterministic handles (the order the atomics
// arrive in is not fixed): those keep k_pcg_iter.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SY_VEC_WG = 64;         // workgroups of the vector kernel (each forms the scalars for itself and updates its slice)

// sums of eight per-lane values over the wave: afterwards every lane of the group lane / 8 holds the total of value lane / 8
__device__ __forceinline__ double rows8_reduce(const double (&v)[8], int lane) {
    double a[4], b[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = xlane_pairsum<32>(v[k], v[4 + k]);
#pragma unroll
    for (int k = 0; k < 2; ++k) b[k] = xlane_pairsum<16>(a[k], a[2 + k]);
    const bool up = (lane & 8) != 0;
    const double send = up ? b[0] : b[1], keep = up ? b[1] : b[0];
    double c = keep + xlane_get<8>(send);
    c = xlane_add<4>(c); c = xlane_add<2>(c); c = xlane_add<1>(c);
    return c;
}
__device__ __forceinline__ double* sy_slot(double* part, int parity, int v, int slot) { return part + ((size_t)(parity * PCG_NPART + v) * SY_SLOTS + slot) * SY_SLOT_STRIDE; }

// the vector half of an iteration (see above).  q2: [2][ld] the products by parity; part: [2][9][SY_SLOTS] accumulators, one line each
// EPT > 0: the whole of r and q in registers (EPT entries per thread, 256 EPT >= d), requested together with everything else the launch reads BEFORE
// the first reduction -- one memory round trip per launch instead of one per phase; EPT = 0: looped (any d)
template <bool INIT, bool COARSE, int EPT>
__global__ __launch_bounds__(256) void k_sy_vec(int d, int ld, double* __restrict__ vec, double* __restrict__ q2, const double* __restrict__ bt,
                                                double* __restrict__ part, double* scal, int* flags, double tol2, int in, int* info, int* mailbox,
                                                int anchor, double cap, const double* __restrict__ W, const double* __restrict__ coarse) {
    __shared__ double red[PCG_RED];
    const int seq = in >> 1;
    in &= 1;
    if (!INIT) { const int dn = flags[PF_DONE]; if (dn != 0 && seq >= dn) return; }
    constexpr int NV = COARSE ? PCG_NPART : 1;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, out = in ^ 1;
    const int nwg = (int)gridDim.x;
    const int per = (d + nwg - 1) / nwg;
    const int row0 = min(d, (int)blockIdx.x * per), row1 = min(d, row0 + per);
    double* x_out = pcg_vec(vec, 0, out, ld); double* r_out = pcg_vec(vec, 1, out, ld); double* p_out = pcg_vec(vec, 2, out, ld);
    const double* x_in = pcg_vec(vec, 0, in, ld); const double* r_in = INIT ? bt : pcg_vec(vec, 1, in, ld);
    const double* p_in = pcg_vec(vec, 2, in, ld);
    const double* q_in = q2 + (size_t)in * ld;
    double* q_next = q2 + (size_t)out * ld;         // the product of THIS iteration is added into it
    const double* st_in = scal + PS_STATE + PS_STATE_LEN * in;
    double* st_out = scal + PS_STATE + PS_STATE_LEN * out;
    if (COARSE && tid < PCG_NW * PCG_NW) { red[80 + tid] = coarse[tid]; red[144 + tid] = coarse[PCG_NW * PCG_NW + PCG_NW + tid]; }      // E^-1, E
    // the buffers the product adds into: zero (this workgroup's slice of q, its share of the accumulators)
    for (int e = row0 + tid; e < row1; e += 256) q_next[e] = 0.0;
    for (int i = blockIdx.x * 256 + tid; i < NV * SY_SLOTS; i += nwg * 256) sy_slot(part, out, 0, 0)[(size_t)i * SY_SLOT_STRIDE] = 0.0;
    double c_new[PCG_NW], mu_new[PCG_NW], pmu_new[PCG_NW], pmu_in[PCG_NW];
    double rz_new = 0.0;
    if (INIT) {
        double rr = 0.0;
        for (int e0 = tid; e0 < d; e0 += 256 * 8) {
            double bv8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; bv8[u] = bt[e < d ? e : d - 1]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; if (e < d) rr += bv8[u] * bv8[u]; }
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
        for (int e = row0 + tid; e < row1; e += 256) { const double b = bt[e]; x_out[e] = 0.0; r_out[e] = b; p_out[e] = b; }
        if (blockIdx.x == 0 && tid == 0) {
            scal[PS_RR0] = pcg_threshold_base(rr, scal, anchor, cap); flags[PF_DONE] = (rr == 0.0); flags[PF_ITERS] = 0; flags[PF_XBUF] = out;
            if (mailbox && rr == 0.0) pcg_post(mailbox, 0, 1);
        }
    } else {
        // the slotted sums of the previous product: wave w owns values w, w + 4, w + 8; one slot per lane
        double mine[3] = { 0.0, 0.0, 0.0 };
#pragma unroll
        for (int j = 0; j < 3; ++j) { const int v = w + 4 * j; mine[j] = (4 * j < NV && v < NV) ? *sy_slot(part, in, v, lane) : 0.0; }
        // ... and every other load of the launch, before anything waits: r and q (whole), this thread's entry of the slice
        double rv[EPT > 0 ? EPT : 1], qv[EPT > 0 ? EPT : 1];
        if (EPT > 0) {
#pragma unroll
            for (int m = 0; m < EPT; ++m) { const int e = tid + 256 * m, ec = e < d ? e : d - 1; rv[m] = r_in[ec]; qv[m] = q_in[ec]; }
        }
        const int eo = row0 + tid;
        const bool own = eo < row1;                      // (per <= 256: one entry per thread; longer slices loop below)
        const int eoc = own ? eo : 0;
        const double xo = x_in[eoc], po = p_in[eoc], ro = r_in[eoc], qo = q_in[eoc];
        double wo[PCG_NW];
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) wo[k] = COARSE ? W[(size_t)k * ld + eoc] : 0.0;
        const double rz_in = st_in[PS_RZ], rr0 = scal[PS_RR0];
        double g[PCG_NW], Eg[PCG_NW], c_in[PCG_NW], mu_in[PCG_NW];
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) {
            pmu_in[k] = COARSE ? st_in[PS_PMU + k] : 0.0;
            c_in[k] = COARSE ? st_in[PS_C + k] : 0.0;
            mu_in[k] = COARSE ? st_in[PS_MU + k] : 0.0;
            Eg[k] = 0.0;
        }
        reduce_partials<NV>(mine, red);
        __syncthreads();
        // W~^T q = (S~ W~)^T p_r (the partials) + E p_mu
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) {
            double erow[PCG_NW];
#pragma unroll
            for (int j = 0; j < PCG_NW; ++j) erow[j] = COARSE ? red[144 + PCG_NW * k + j] : 0.0;
            g[k] = COARSE ? red[1 + k] + dot8(erow, pmu_in) : 0.0;
        }
        const double pq = red[0] + (COARSE ? dot8(pmu_in, g) : 0.0);
        const double alpha = rz_in * fast_rcp(pq);
        if (COARSE) einv_apply(red + 80, g, Eg);         // independent of alpha: overlaps the reciprocal
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) { c_new[k] = fma(-alpha, g[k], c_in[k]); mu_new[k] = fma(-alpha, Eg[k], mu_in[k]); }
        const double cmu = COARSE ? dot8(c_new, mu_new) : 0.0;
        double rrn = 0.0;
        if (EPT > 0) {
#pragma unroll
            for (int m = 0; m < EPT; ++m) { const double v = fma(-alpha, qv[m], rv[m]); rrn = (tid + 256 * m < d) ? fma(v, v, rrn) : rrn; }
        } else {
            for (int e0 = tid; e0 < d; e0 += 256 * 8) {
                double rv8[8], qv8[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u, ec = e < d ? e : d - 1; rv8[u] = r_in[ec]; qv8[u] = q_in[ec]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int e = e0 + 256 * u; if (e < d) { const double v = fma(-alpha, qv8[u], rv8[u]); rrn = fma(v, v, rrn); } }
            }
        }
        rrn = wave_allsum(rrn);
        if (lane == 0) red[16 + w] = rrn;
        // x += alpha p  with p = p_r + W~ p_mu, own slice
        if (own) x_out[eo] = xo + alpha * (po + (COARSE ? dot8(wo, pmu_in) : 0.0));
        for (int e = eo + 256; e < row1; e += 256) {
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
        if (rrn <= tol2 * rr0 || broke) {
            if (blockIdx.x == 0 && tid == 0) {
                flags[PF_DONE] = seq + 1; flags[PF_XBUF] = out; const int it = flags[PF_ITERS] + 1; flags[PF_ITERS] = it;
                if (broke) atomicCAS(info, 0, d + 1);
                if (mailbox) pcg_post(mailbox, it, 1);
            }
            return;
        }
        const double beta = rz_new * fast_rcp(rz_in);
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) pmu_new[k] = fma(beta, pmu_in[k], mu_new[k]);
        if (own) { const double rn = fma(-alpha, qo, ro); r_out[eo] = rn; p_out[eo] = fma(beta, po, rn); }
        for (int e = eo + 256; e < row1; e += 256) {
            const double rn = fma(-alpha, q_in[e], r_in[e]);
            r_out[e] = rn;
            p_out[e] = fma(beta, p_in[e], rn);
        }
        if (blockIdx.x == 0 && tid == 0) { const int it = flags[PF_ITERS] + 1; flags[PF_ITERS] = it; flags[PF_XBUF] = out; if (mailbox) pcg_post(mailbox, it, 0); }
    }
    if (blockIdx.x == 0 && tid == 0) {
        st_out[PS_RZ] = rz_new;
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) { st_out[PS_C + k] = c_new[k]; st_out[PS_MU + k] = mu_new[k]; st_out[PS_PMU + k] = pmu_new[k]; }
    }
}

// the product half: tiles[blockIdx.x] = {first row, first column (a multiple of SY_C), rows, 1 if the tile overlaps the diagonal}.  `in` as k_sy_vec's
// (the launch pair of one iteration shares it): p_r and the state of parity out = in ^ 1 are what k_sy_vec just wrote.
template <typename FT, bool COARSE>
__global__ __launch_bounds__(256) void k_sy_prod(int d, int ld, const FT* __restrict__ F, const double* __restrict__ vec, double* __restrict__ q2,
                                                 double* __restrict__ part, const double* __restrict__ scal, const int* __restrict__ flags,
                                                 const int4* __restrict__ tiles, int in, int nslice, const double* __restrict__ AW) {
    __shared__ __align__(16) double colsh[4 * SY_C];
    __shared__ double red[4 * PCG_NPART];
    const int seq = in >> 1;
    in &= 1;
    { const int dn = flags[PF_DONE]; if (dn != 0 && seq + 1 >= dn) return; }       // (k_sy_vec of this iteration has raised it: nothing left to multiply)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, out = in ^ 1;
    const double* p = vec + (size_t)(2 * 2 + out) * ld;        // pcg_vec(vec, 2, out, ld)
    double* q = q2 + (size_t)out * ld;
    const int4 tl = tiles[blockIdx.x];
    const int r0 = tl.x, c0 = tl.y, rend = tl.x + tl.z;
    const bool diag = tl.w != 0;
    const int j0 = c0 + 4 * lane, rw0 = r0 + 8 * w;
    Quad<FT> f[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int row = rw0 + u; f[u].load(F + (size_t)(row < rend ? row : r0) * ld + j0); }
    double pj[4];
    {
        const double2 a = reinterpret_cast<const double2*>(p + j0)[0], b = reinterpret_cast<const double2*>(p + j0)[1];      // (j0 + 3 < ld + pcg_tile_slack(d, ld), inside vec: what lies at columns >= d is selected away)
        pj[0] = j0 + 0 < d ? a.x : 0.0; pj[1] = j0 + 1 < d ? a.y : 0.0; pj[2] = j0 + 2 < d ? b.x : 0.0; pj[3] = j0 + 3 < d ? b.y : 0.0;
    }
    const int myrow = rw0 + (lane >> 3);              // the row whose total this lane group publishes
    const double prow = myrow < rend ? p[myrow] : 0.0;
    double pq_acc = 0.0;
    double racc[8], colacc[4] = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int row = rw0 + u;                      // wave-uniform
        const double pi = lane_bcast(prow, 8 * u);    // (0 for a row beyond the tile)
        const bool live = row < rend;
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + e;
            double x = f[u].get(e);
            if (!live || j >= d || (diag && j < row)) x = 0.0;
            s = fma(x, pj[e], s);
            colacc[e] = fma((diag && j == row) ? 0.0 : x, pi, colacc[e]);       // the diagonal entry is used once
        }
        racc[u] = s;
    }
    const double tot = rows8_reduce(racc, lane);
    if ((lane & 7) == 0 && myrow < rend) { atomicAdd(q + myrow, tot); pq_acc = prow * tot; }
#pragma unroll
    for (int e = 0; e < 4; ++e) colsh[w * SY_C + 4 * lane + e] = colacc[e];
    __syncthreads();
    if (c0 + tid < d) {
        const double cs = (colsh[tid] + colsh[SY_C + tid]) + (colsh[2 * SY_C + tid] + colsh[3 * SY_C + tid]);
        atomicAdd(q + c0 + tid, cs);
        pq_acc = fma(p[c0 + tid], cs, pq_acc);
    }
    // ---- the first nslice workgroups: q += (S~ W~) p_mu on their slice, and the partials of (S~ W~)^T p_r ----
    double gpart[PCG_NW];
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k) gpart[k] = 0.0;
    const bool slice = COARSE && (int)blockIdx.x < nslice;
    if (slice) {
        const int per = (d + nslice - 1) / nslice;
        const int e0 = min(d, (int)blockIdx.x * per), e1 = min(d, e0 + per);
        const double* st = scal + PS_STATE + PS_STATE_LEN * out;
        double pmu[PCG_NW];
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) pmu[k] = st[PS_PMU + k];
        for (int e = e0 + tid; e < e1; e += 256) {
            const double pe = p[e];
            double aw[PCG_NW];
#pragma unroll
            for (int k = 0; k < PCG_NW; ++k) aw[k] = AW[(size_t)k * ld + e];        // (AWt: vector-major)
            const double a = dot8(aw, pmu);
            atomicAdd(q + e, a);
            pq_acc = fma(pe, a, pq_acc);
#pragma unroll
            for (int k = 0; k < PCG_NW; ++k) gpart[k] = fma(aw[k], pe, gpart[k]);
        }
    }
    pq_acc = wave_allsum(pq_acc);
    if (slice) {
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) gpart[k] = wave_allsum(gpart[k]);
    }
    if (lane == 0) {
        red[PCG_NPART * w] = pq_acc;
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) red[PCG_NPART * w + 1 + k] = gpart[k];
    }
    __syncthreads();
    if (tid == 0 || (slice && tid < PCG_NPART)) {
        const double v = (red[tid] + red[PCG_NPART + tid]) + (red[2 * PCG_NPART + tid] + red[3 * PCG_NPART + tid]);
        atomicAdd(sy_slot(part, out, tid, (int)(blockIdx.x % SY_SLOTS)), v);
    }
}

// The coarse set-up on the same triangle: AW = S~ W~ for the eight gauge vectors at once, every entry of the triangle used sixteen times from its
// one load.  With eight vectors the atomics are what has to be budgeted (the memory side retires ~6 G line-sized atomic transactions per second,
// see above): TALL tiles, SY_CR rows x SY_C columns -- the eight column sums of a lane's four columns stay in registers over the wave's 32 rows
// and leave through LDS (ds_add_f64 across the four waves), the row sums of a wave's rows are parked in LDS until the tile is done -- so a tile
// issues 8 x (256 + 128) atomics as 192 instructions on consecutive addresses (~115 k lines per pass at d = 6001).  The result is vector-major,
// AWt[k][i] (consecutive lanes = consecutive entries), zeroed by the linearisation (k_finalize: DeviceBuffers::pcg_zero).
// (Measured and not kept, profiles/r06_ab_sy_coarse.txt: the batch specialised on the diagonal flag with the prefetch peeled -- four copies of the loop,
// 86 spilled registers, 86 us --; W~ of the lane's columns held as floats with the widening kept opaque -- 18 spills, 58 us; this form, one spill: 51 us.
// The pass is bound by its instruction count, ~1 800 per eight rows of 256 columns -- 512 fp64 FMAs, 330 v_readlane for W~ of the rows, ~300 for the
// eight halving reductions, the masks -- at two waves per SIMD: the 72 MB stream at 1.4 TB/s.)
template <typename FT>
__global__ __launch_bounds__(256, 2) void k_sy_coarse(int d, int ld, const FT* __restrict__ F, const double* __restrict__ W, double* __restrict__ AWt,
                                                      const int4* __restrict__ tiles) {
    __shared__ double colsh[PCG_NW * SY_C];      // [k][column]
    __shared__ double rowsh[PCG_NW * SY_CR];     // [k][row]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int4 tl = tiles[blockIdx.x];
    const int r0 = tl.x, c0 = tl.y, rend = tl.x + tl.z;
    const bool diag = tl.w != 0;
    const int j0 = c0 + 4 * lane;
    for (int i = tid; i < PCG_NW * SY_C; i += 256) colsh[i] = 0.0;
    double wj[4][PCG_NW], colacc[4][PCG_NW];
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k) {
        const double2 a = reinterpret_cast<const double2*>(W + (size_t)k * ld + j0)[0], b = reinterpret_cast<const double2*>(W + (size_t)k * ld + j0)[1];
        wj[0][k] = j0 + 0 < d ? a.x : 0.0; wj[1][k] = j0 + 1 < d ? a.y : 0.0; wj[2][k] = j0 + 2 < d ? b.x : 0.0; wj[3][k] = j0 + 3 < d ? b.y : 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) colacc[e][k] = 0.0;
    }
    constexpr int RPWV = SY_CR / 4, NBATCH = RPWV / 8;
    const int rw = r0 + RPWV * w;                     // this wave's rows, eight at a time
    Quad<FT> f[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int row = rw + u; f[u].load(F + (size_t)(row < rend ? row : r0) * ld + j0); }
#pragma unroll 1
    for (int b = 0; b < NBATCH; ++b) {
        const int rb = rw + 8 * b;
        // W~ of the batch's rows: lane l holds vector l % 8 of row l / 8; a row's eight values reach the FMAs as scalar operands (v_readlane)
        const int wr = rb + (lane >> 3);
        const double wrow = wr < rend ? W[(size_t)(lane & 7) * ld + wr] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int row = rb + u;
            const bool live = row < rend;
            double x[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { const int j = j0 + e; x[e] = (!live || j >= d || (diag && j < row)) ? 0.0 : f[u].get(e); }
            if (b < NBATCH - 1) { const int nrow = rb + 8 + u; f[u].load(F + (size_t)(nrow < rend ? nrow : r0) * ld + j0); }      // the next batch's load of this slot goes out at once
            double sacc[PCG_NW];
#pragma unroll
            for (int k = 0; k < PCG_NW; ++k) {
                const double wi = lane_bcast(wrow, 8 * u + k);
                double sk = 0.0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    sk = fma(x[e], wj[e][k], sk);
                    colacc[e][k] = fma((diag && j0 + e == row) ? 0.0 : x[e], wi, colacc[e][k]);       // the diagonal entry is used once
                }
                sacc[k] = sk;
            }
            const double tot = rows8_reduce(sacc, lane);          // lanes of group g: vector g of this row
            if ((lane & 7) == 0) rowsh[(lane >> 3) * SY_CR + RPWV * w + 8 * b + u] = tot;
        }
    }
    __syncthreads();                                  // colsh zeroed, rowsh complete
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(&colsh[k * SY_C + 4 * lane + e], colacc[e][k]);
    // the row sums: consecutive threads = consecutive rows of one vector
#pragma unroll
    for (int m = 0; m < PCG_NW * SY_CR / 256; ++m) {
        const int v = tid + 256 * m, k = v / SY_CR, row = r0 + (v % SY_CR);
        if (row < rend) atomicAdd(AWt + (size_t)k * ld + row, rowsh[v]);
    }
    __syncthreads();
    if (c0 + tid < d) {
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) atomicAdd(AWt + (size_t)k * ld + c0 + tid, colsh[k * SY_C + tid]);
    }
}

// E = W~^T (S~ W~) and c_0 = W~^T b~ from the finished AWt: partials per workgroup into epart (the layout k_pcg_coarse_invert sums)
__global__ __launch_bounds__(256) void k_sy_e(int d, int ld, const double* __restrict__ W, const double* __restrict__ AWt, const double* __restrict__ bt,
                                              double* __restrict__ epart) {
    __shared__ double sh[4][PCG_NW * PCG_NW + PCG_NW];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = (d + gridDim.x - 1) / gridDim.x, i0 = blockIdx.x * per, i1 = min(d, i0 + per);
    double e[PCG_NW][PCG_NW], c[PCG_NW];
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k) { c[k] = 0.0;
#pragma unroll
        for (int l = 0; l < PCG_NW; ++l) e[k][l] = 0.0; }
    for (int i = i0 + tid; i < i1; i += 256) {
        double wv[PCG_NW], av[PCG_NW];
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) { wv[k] = W[(size_t)k * ld + i]; av[k] = AWt[(size_t)k * ld + i]; }
        const double b = bt[i];
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) { c[k] = fma(wv[k], b, c[k]);
#pragma unroll
            for (int l = 0; l < PCG_NW; ++l) e[k][l] = fma(wv[k], av[l], e[k][l]); }
    }
#pragma unroll
    for (int k = 0; k < PCG_NW; ++k) { c[k] = wave_allsum(c[k]);
#pragma unroll
        for (int l = 0; l < PCG_NW; ++l) e[k][l] = wave_allsum(e[k][l]); }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < PCG_NW; ++k) { sh[w][PCG_NW * PCG_NW + k] = c[k];
#pragma unroll
            for (int l = 0; l < PCG_NW; ++l) sh[w][k * PCG_NW + l] = e[k][l]; }
    }
    __syncthreads();
    if (tid < PCG_NW * PCG_NW + PCG_NW) epart[(size_t)tid * PCG_PART + blockIdx.x] = (sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid]);
}

// the set-up on the one triangle as well: AWt = S~ W~ (zeroed by the linearisation), then E and c_0 from it, then the 8 x 8 inverse
void pcg_symmetric_setup(hipStream_t s, const DenseSolver* ws, Profiler* prof) {
    const CgPath& r = ws->run.path;
    if (!r.coarse) return;
    ProfScope ps(prof, KID_PCG_SETUP, s, 3);
    if (r.f32) hipLaunchKernelGGL((k_sy_coarse<float>), dim3(ws->sym_nctiles), dim3(256), 0, s, ws->d, ws->ld, ws->Sfull32, ws->W, ws->AWt, ws->sym_ctiles);
    else hipLaunchKernelGGL((k_sy_coarse<double>), dim3(ws->sym_nctiles), dim3(256), 0, s, ws->d, ws->ld, ws->Sfull, ws->W, ws->AWt, ws->sym_ctiles);
    hipLaunchKernelGGL(k_sy_e, dim3(SY_VEC_WG), dim3(256), 0, s, ws->d, ws->ld, ws->W, ws->AWt, pcg_btilde(ws), ws->epart);
    pcg_coarse_invert(s, SY_VEC_WG, ws->epart, ws->coarse);
}

// two launches per iteration: the vector half, then one workgroup per tile of the upper triangle.  (ONE launch per iteration was built and measured --
// the Chronopoulos - Gear form of the CG, whose inner products are all sums of per-workgroup partials, so that no launch needs a pass over the vectors:
// correct, and 27 us per iteration against 17.9 + 7.5 here: profiles/r06_ab_sy_one_launch.txt, commit "k_sy_cg".)
template <bool INIT>
static void sy_iterate(hipStream_t s, const DenseSolver* ws, int in, int anchor, double cap) {
    const DenseSolver::CgRun& run = ws->run;
    const CgPath& r = run.path;
    const int d = ws->d, ld = ws->ld;
    const int nvec = std::max(1, std::min(SY_VEC_WG, (d + 63) / 64)), nslice = std::min(ws->sym_ntiles, 256);
#define SYV_ARGS d, ld, ws->vec, ws->q3, pcg_btilde(ws), ws->sym_part, ws->scal, ws->flags, run.tol2, in, run.info, ws->d_mailbox, anchor, cap, ws->W, ws->coarse
#define SYV(C, E) hipLaunchKernelGGL((k_sy_vec<INIT, C, E>), dim3(nvec), dim3(256), 0, s, SYV_ARGS)
    const int ept = INIT ? 0 : (d <= 256 * 8 ? 8 : d <= 256 * 16 ? 16 : d <= 256 * 24 ? 24 : d <= 256 * 32 ? 32 : 0);
    if (r.coarse) { if (ept == 8) SYV(true, 8); else if (ept == 16) SYV(true, 16); else if (ept == 24) SYV(true, 24); else if (ept == 32) SYV(true, 32); else SYV(true, 0); }
    else { if (ept == 8) SYV(false, 8); else if (ept == 16) SYV(false, 16); else if (ept == 24) SYV(false, 24); else if (ept == 32) SYV(false, 32); else SYV(false, 0); }
#undef SYV
#undef SYV_ARGS
#define SY_ARGS(Fptr) d, ld, Fptr, ws->vec, ws->q3, ws->sym_part, ws->scal, ws->flags, ws->sym_tiles, in, nslice, ws->AWt
    if (r.f32) { if (r.coarse) hipLaunchKernelGGL((k_sy_prod<float, true>), dim3(ws->sym_ntiles), dim3(256), 0, s, SY_ARGS(ws->Sfull32));
                 else hipLaunchKernelGGL((k_sy_prod<float, false>), dim3(ws->sym_ntiles), dim3(256), 0, s, SY_ARGS(ws->Sfull32)); }
    else { if (r.coarse) hipLaunchKernelGGL((k_sy_prod<double, true>), dim3(ws->sym_ntiles), dim3(256), 0, s, SY_ARGS(ws->Sfull));
           else hipLaunchKernelGGL((k_sy_prod<double, false>), dim3(ws->sym_ntiles), dim3(256), 0, s, SY_ARGS(ws->Sfull)); }
#undef SY_ARGS
}

void pcg_symmetric_iterate(hipStream_t s, const DenseSolver* ws, bool init, int in, int anchor, double cap) {
    if (init) sy_iterate<true>(s, ws, in, anchor, cap); else sy_iterate<false>(s, ws, in, anchor, cap);
}

}  // namespace sfmba
