// ba_pairs.hip -- stage 4 of the linearisation: the reduced-system pass over camera pairs (the off-diagonal 6x6 blocks), behind
// k_finalize (ba_finalize.hip) on the PCG path, behind the camera pass on the exact solver's; mode 2 (duplicate pairs) runs before k_finalize.
//   reads   camtab[cur], the per-point table (PA), the pair lists and descriptors of structure_build.hip, the per-camera factor pair_G
//           (k_finalize, or k_pair_factors here), PCG: pcg_binv, the focal column and right-hand side for the glue
//   leaves  every off-diagonal block exactly once: in S (mode 0, upper triangle) or straight in S~ = Lb^-1 S Lb^-T (mode 1: the CG's matrix
//           or the exchange buffer of a sharded solve) with the per-camera glue of the block-Jacobi transform (pcg_bt, focal row / column)
//           and the post-linearisation bookkeeping; mode 2 adds the duplicate pairs into the diagonal blocks
#include "ba_common.h"

namespace sfmba {

// ------------------------------------------------------------------------------------------
// K2a: reduced-system pass over camera pairs.  One wave per 6x6 block (ja < jb): the pairs of observations (one of camera ja,
// one of camera jb, same point) were listed once at build time (structure_build.hip: per pair its POINT, grouped by block),
// so the block is the plain sum
//   -S_a [ sum_pairs A_a^T (C_a C_b^T) A_b ] S_b
// -- no atomics, every block written exactly once per iteration (empty blocks are written as zero:
// the in-place Cholesky destroyed the previous contents).  Workgroups are grouped so that all
// blocks of one block-row run on one XCD (blockIdx % 8).  Nothing is stored per observation (rounds 1 / 2 gathered two 64-byte
// records per pair: 19x the algorithmic traffic): both observations of a pair are RE-EVALUATED from the two camera rows (scalar
// registers) and one 64-byte point-table entry, in the FACTORED form of sfmba_device.h (obs_factored).
// ------------------------------------------------------------------------------------------
// The block sums of the pair passes: the lane's own sums in T (at most eight pair products each in the wave-per-chunk pass) are WIDENED to
// fp64 before the first cross-lane step, so that everything summed across lanes, chunks and ranks is summed in fp64 ("fp32 Jacobian blocks,
// fp64 accumulation", BASELINE config 3).  The first halving level over the lanes that differ in bit OFF converts on the fly: only 18
// doubles are ever live.  On return this lane owns the sums of entries base .. base + len - 1 in own[0 .. len): at most one with the
// whole wave on a block (OFF = 32), up to three with a group of sixteen lanes (OFF = 8).  (Measured and not kept, DESIGN_HISTORY.md
// "Pair-pass block sums": the butterfly in fp32 as well -- every entry a sum of up to 512 fp32 products; fp64 lane sums too -- 72 more
// registers, a wave of occupancy at config 3, spills at config 5.)
template <typename T, int OFF>
__device__ __forceinline__ void pair_reduce(T (&acc)[36], int lane, int& base, int& len, double (&own)[3]) {
    if constexpr (sizeof(T) == 8) {
        HalvingReduceT<T, 36, OFF>::run(acc, lane, base, len);
#pragma unroll
        for (int k = 0; k < 3; ++k) own[k] = acc[k];
    } else {
        constexpr int H = 18;
        const bool up = (lane & OFF) != 0;
        double w[H];
#pragma unroll
        for (int k = 0; k < H; ++k) {
            const double lo = (double)acc[k], hi = (double)acc[H + k];
            if constexpr (OFF >= 16) w[k] = xlane_pairsum<OFF>(lo, hi);
            else { const double send = up ? lo : hi, keep = up ? hi : lo; w[k] = keep + xlane_get<OFF>(send); }
        }
        base += up ? H : 0;
        len = up ? len - H : (len < H ? len : H);
        HalvingReduceT<double, H, OFF / 2, true>::run(w, lane, base, len);
#pragma unroll
        for (int k = 0; k < 3; ++k) own[k] = w[k];
    }
}

// {ja, jb} of a pair-pass descriptor {block, row camera ja, ...}: block b is entry jb - ja of row ja of the upper triangle
__device__ __forceinline__ int2 pair_block_cams(const int4& dsc, int ncam) {
    int2 cj;
    cj.x = dsc.y;
    cj.y = dsc.y + (dsc.x - (int)((long long)dsc.y * ncam - (long long)dsc.y * (dsc.y - 1) / 2));
    return cj;
}

// one pair of observations: acc += A_a^T (C_a C_b^T) A_b   (unscaled; the camera scales are applied once at the end)
template <typename T>
__device__ __forceinline__ void pair_product(const T ra[YREC], const T rb[YREC], bool diag, T acc[36]) {
    const T m00 = ra[9] * rb[9] + ra[10] * rb[10] + ra[11] * rb[11];
    const T m01 = ra[9] * rb[12] + ra[10] * rb[13] + ra[11] * rb[14];
    const T m10 = ra[12] * rb[9] + ra[13] * rb[10] + ra[14] * rb[11];
    const T m11 = ra[12] * rb[12] + ra[13] * rb[13] + ra[14] * rb[14];
    T Aa[12], Ab[12], Tm[12];
    rec_camera_block<T>(ra, Aa);
    rec_camera_block<T>(rb, Ab);
#pragma unroll
    for (int c = 0; c < 6; ++c) { Tm[c] = m00 * Ab[c] + m01 * Ab[6 + c]; Tm[6 + c] = m10 * Ab[c] + m11 * Ab[6 + c]; }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const T v = Aa[r] * Tm[c] + Aa[6 + r] * Tm[6 + c];
            acc[6 * r + c] += v;
            if (diag) acc[6 * c + r] += v;   // same camera twice: Y_a Y_b^T + Y_b Y_a^T
        }
}

// the two-sided transform of one block's sums (factored coordinates, sfmba_device.h): S_IJ = G_I [sum] G_J^T with the per-camera
// G = Lw D E^T that k_finalize (PCG: Lw = Linv, so this IS the preconditioned block) or k_pair_factors (exact solver: Lw = I) left in
// pair_G.  tile: the 36 sums (negated) in LDS; lanes 0..35 write one entry each.
template <int MODE>
__device__ __forceinline__ void pair_epilogue(const DeviceStructure& ds, const DeviceBuffers& db, int b, int2 cj, const double* tile, int lane) {
    if (lane < 36) {
        const int r = lane / 6, c = lane - 6 * r;
        double Gi[6], Gj[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) { Gi[a] = db.pair_G[(size_t)cj.x * 36 + 6 * r + a]; Gj[a] = db.pair_G[(size_t)cj.y * 36 + 6 * c + a]; }
        double v = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double u = 0.0;
#pragma unroll
            for (int bb = 0; bb < 6; ++bb) u += tile[6 * a + bb] * Gj[bb];
            v += Gi[a] * u;
        }
        if (MODE == 0) db.S[(size_t)(6 * cj.x + r) * ds.ld + 6 * cj.y + c] = v;
        else store_block_entry(ds, db, b, cj, r, c, v);
    }
}

// One wave per CHUNK of a block: at most SFMBA_PAIR_CHUNK pairs (eight rounds of 64), so lane-local sums in T never pile up more than eight
// terms and no wave runs longer than eight rounds whatever the co-visibility (structure_build.hip, build_pair_chunks).  The per-camera
// factor diag(R K', I) of the camera blocks is applied once per block in the epilogue (pair_G), the pair loop works on [ -[R X]x | I ], the
// projection Jacobian and C.  In fp32 mode both observations of a pair are evaluated at once as packed fp32 halves and the 6x6 update is
// summed in its rank-2 form (sfmba_device.h: obs_factored_ab, pair_product_ab): 139 wave instructions per 64 pairs, 96 registers (five
// waves per SIMD; tools/pair_isa_count.py counts them from the compiler's output).  A block of several chunks leaves its partial sums in
// pair_partial; k_schur_combine (the next launch) adds them and runs the epilogue.
// QUAD (fp32 mode, the default): the round's 64 point-table entries are fetched by quads -- four loads in which the four lanes of a quad
// read one contiguous 64-byte entry, 16 lines per load where a per-lane gather walks 64 (three such gathers per round without it) -- and
// transposed through 4 144 bytes of LDS private to the wave (sfmba_device.h: ptrec_quad_fetch / ptrec_quad_take): 162 instructions per
// round, 7 of them LDS, 94 registers.  Measured at BASELINE config 3 (profiles/pair_coop_loads_ab.txt): cache accesses per wave 1 178 -> 481,
// the texture addresser 68 % -> 50 % busy, 48.9 -> 46.0 us per launch.  Every lane ends up with the bytes its own loads would bring.
template <typename T, int MODE, bool QUAD>
__device__ __forceinline__ void schur_pairs_wave(const DeviceStructure& ds, const DeviceBuffers& db) {
    static_assert(!QUAD || sizeof(T) == 4, "the quad fetch is that of the 64-byte entry");
    __shared__ double tile[36];
    const int lane = threadIdx.x & 63;
    const int4 dsc = ds.pwg_desc[blockIdx.x];       // one load: block, row camera, pair range of the chunk
    const int2 chunk = ds.pwg_chunk[blockIdx.x];    // {row of pair_partial (blocks of several chunks), chunks of the block}
    const int b = dsc.x, pbeg = dsc.z, p1 = dsc.w;
    const int2 cj = pair_block_cams(dsc, ds.ncam);
    if (cj.x == cj.y) {
        if (MODE == 1) {
            // k_finalize(pcg = 1) left the post-linearisation bookkeeping (gradient tolerance, cost of iteration 0, failed
            // evaluation) to this launch, which starts after it in stream order: no arrival counter, no fences there
            if (cj.x == 0) post_linearisation(ds, db);
            // glue of the block-Jacobi transform for camera j (ba_common.h: pcg_glue_row / pcg_glue_focal), and S~_jj = I
            const int j = cj.x, row0 = 6 * j;
            const double linv_f = pcg_glue_linv_f(ds, db);
            if (lane < 36) {
                const int r = lane / 6, c = lane - 6 * r;
                store_F(db, (size_t)(row0 + r) * ds.ld + row0 + c, (r == c) ? 1.0 : 0.0);
            }
            if (lane < 6) pcg_glue_row(ds, db, j, lane, linv_f);
            if (j == 0 && lane == 63) pcg_glue_focal(ds, db, linv_f);
        }
        return;     // pairs inside diagonal blocks (duplicates) were added by k_schur_dups before k_finalize
    }
    const int s = lane & 3, g = lane >> 2;
    T acc[36];
#pragma unroll
    for (int e = 0; e < 36; ++e) acc[e] = (T)0;
    {
        const LMState* st = db.st;
        const int cur = st->cur;
        const double focal = st->focal[cur];
        const PtRecA<T>* PA = reinterpret_cast<const PtRecA<T>*>(db.PA);
        // lane (s, g) owns pair p0 + 16 s + g of a round.  A round issues the loads of its own point-table entry and of the NEXT round's point
        // slot together, and the next entry's address is formed from that slot at the round's end: one dependent memory level per round (the
        // entry), the slot's latency behind the round's arithmetic.  (Carried as a bare slot the load is moved by the compiler to the top of
        // the round that uses it -- a phi of loads becomes a load of a phi -- and the round waits for two dependent loads; the address is
        // arithmetic on the loaded value and stays in the round that loaded it.)  Rounds past the end re-read the chunk's last pair.
        const int mine = 16 * s + g;
        const int plast = pbeg < p1 ? p1 - 1 : 0;
        const PtRecA<T>* ent_next = PA + ds.pair_pt[pbeg + mine < p1 ? pbeg + mine : plast];
        // QUAD: the entry's byte offset is carried instead (arithmetic on the loaded slot as well), and the entry comes through LDS: the four
        // lanes of a quad fetch the entries of the quad's four pairs piece by piece (sfmba_device.h, ptrec_quad_fetch) -- 64 lines per round
        // instead of 192, the same bytes in every lane.
        auto rounds = [&](auto&& body) {
            if constexpr (QUAD) {
                __shared__ int4 coop[PTQ_PIECES];
                unsigned off_next = (unsigned)(ent_next - PA) * 64u;
                for (int p0 = pbeg; p0 < p1; p0 += 64) {
                    unsigned w = 16u * (unsigned)lane;
                    asm volatile("" : "+v"(w));         // the LDS addresses and the piece offset are formed anew every round (five instructions): carried, they cost the fifth wave (98 registers)
                    ptrec_quad_fetch(PA, off_next, w, coop);
                    wave_lds_fence();
                    const PtRecA<T> pa = ptrec_quad_take(w, coop);
                    const int p = p0 + 64 + mine;
                    const int pt = ds.pair_pt[p < p1 ? p : plast];
                    body(pa, p0 + mine < p1);
                    off_next = (unsigned)pt * 64u;
                }
            } else {
                for (int p0 = pbeg; p0 < p1; p0 += 64) {
                    const PtRecA<T> pa = load_ptrec(ent_next);
                    const int p = p0 + 64 + mine;
                    const int pt = ds.pair_pt[p < p1 ? p : plast];
                    body(pa, p0 + mine < p1);               // (pair inside the chunk?)
                    ent_next = PA + pt;
                }
            }
        };
        if constexpr (sizeof(T) == 4) {
            // fp32-Jacobian mode: both observations of a pair as the halves of packed fp32 values (obs_factored_ab).  Lane k < 12 fetches
            // value k (R, t) of camera a, lane 12 + k that of camera b: one load and one conversion, then 24 lane reads into uniform pairs.
            const double* tab = db.camtab[cur];
            const int ja = __builtin_amdgcn_readfirstlane(cj.x), jb = __builtin_amdgcn_readfirstlane(cj.y);
            const int kk = lane < 12 ? lane : (lane < 24 ? lane - 12 : 0);
            const int rv = __float_as_int((float)tab[cam_tab_index(kk, lane < 12 ? ja : jb, ds.ncam)]);
            v2f R[12];
#pragma unroll
            for (int k = 0; k < 12; ++k)
                R[k] = v2f{__int_as_float(__builtin_amdgcn_readlane(rv, k)), __int_as_float(__builtin_amdgcn_readlane(rv, 12 + k))};
            const bool fo_a = tab[cam_tab_index(CT_SMALL, ja, ds.ncam)] != 0.0, fo_b = tab[cam_tab_index(CT_SMALL, jb, ds.ncam)] != 0.0;   // wave-uniform
            const float focal_t = (float)focal;
            PairAccAB accp;
            accp.clear();
            rounds([&](const PtRecA<T>& pa, bool live) {
                v2f gab[GREC];
                obs_factored_ab(R, fo_a, fo_b, focal_t, (float)pa.X[0], (float)pa.X[1], (float)pa.X[2], pa.L, gab);
                pair_product_ab(gab, live, accp);
            });
            accp.unpack(acc);
        } else {
            CamG<T> ca, cb;
            load_cam_g<T>(db.camtab[cur], __builtin_amdgcn_readfirstlane(cj.x), ds.ncam, ca);
            load_cam_g<T>(db.camtab[cur], __builtin_amdgcn_readfirstlane(cj.y), ds.ncam, cb);
            rounds([&](const PtRecA<T>& pa, bool live) {
                T ga[GREC], gb[GREC];
                obs_factored<T>(ca, focal, pa.X, pa.L, ga);
                obs_factored<T>(cb, focal, pa.X, pa.L, gb);
                if (!live) ga[3] = (T)0;                // this lane's pair lies beyond the chunk: contribute nothing (N carries f_a / p_z)
                pair_product_factored<T>(ga, gb, acc);
            });
        }
    }
    // Sum of the 36 entries over the 64 lanes by a halving butterfly: afterwards lane `base` -- 36 of the 64 lanes -- owns ONE
    // entry of the 6x6 block.
    int base = 0, len = 36;
    double own[3];
    pair_reduce<T, 32>(acc, lane, base, len, own);
    if (chunk.y > 1) {                              // one of several chunks: the partial sums of this one
        if (len >= 1) db.pair_partial[(size_t)chunk.x * 36 + base] = -own[0];
        return;
    }
    if (len >= 1) tile[base] = -own[0];
    wave_lds_fence();
    pair_epilogue<MODE>(ds, db, b, cj, tile, lane);
}
// fp32: the quad fetch.  The per-lane loads stay selectable (SFMBA_PAIR_LOADS=lane when the problem is built; DeviceStructure::pair_quad) as the
// kernel below: the reference of tests/test_gpu_pair_coop_loads.py and the other side of an A/B measurement.
template <typename T, int MODE>
__global__ __launch_bounds__(64, (sizeof(T) == 4 ? 4 : 2)) void k_schur_pairs(DeviceStructure ds, DeviceBuffers db) {
    schur_pairs_wave<T, MODE, sizeof(T) == 4>(ds, db);
}
template <typename T, int MODE>
__global__ __launch_bounds__(64, 4) void k_schur_pairs_lane(DeviceStructure ds, DeviceBuffers db) {
    schur_pairs_wave<T, MODE, false>(ds, db);
}

// the blocks of several chunks: their partial sums added in chunk order, then the epilogue of k_schur_pairs
template <int MODE>
__global__ __launch_bounds__(64) void k_schur_combine(DeviceStructure ds, DeviceBuffers db) {
    __shared__ double tile[36];
    const int lane = threadIdx.x & 63;
    const int slot0 = ds.multi_slots[blockIdx.x];
    const int4 dsc = ds.pwg_desc[slot0];
    const int2 rows = ds.pwg_chunk[slot0];          // {first row of pair_partial, chunks}
    const int nch = rows.y;
    const int b = dsc.x;
    const int2 cj = pair_block_cams(dsc, ds.ncam);
    if (lane < 36) {
        double v = 0.0;
        for (int c = 0; c < nch; ++c) v += db.pair_partial[(size_t)(rows.x + c) * 36 + lane];
        tile[lane] = v;
    }
    wave_lds_fence();
    pair_epilogue<MODE>(ds, db, b, cj, tile, lane);
}

// Pairs INSIDE a diagonal block: one camera observing a point twice (two features matched to the same 3D point).  Both observations
// of such a pair have the same camera and the same point, hence the same Jacobian blocks (only their coordinates differ):
// Y_a Y_b^T + Y_b Y_a^T = 2 Y Y^T, one evaluation per pair.  One wave per diagonal block that has pairs (usually none); added to the
// upper part of the block with atomics BEFORE k_finalize damps and factors it.
template <typename T>
__global__ __launch_bounds__(64) void k_schur_dups(DeviceStructure ds, DeviceBuffers db) {
    const int lane = threadIdx.x & 63;
    const int b = ds.dup_blocks[blockIdx.x].x;
    const int j = ds.blk_cams[b].x;
    const int pbeg = ds.blk_ptr[b], p1 = ds.blk_ptr[b + 1];
    const LMState* st = db.st;
    const int cur = st->cur;
    const double focal = st->focal[cur];
    CamRegs ct;
    load_cam_regs(db.camtab[cur], __builtin_amdgcn_readfirstlane(j), ds.ncam, ct);
    const PtRecA<T>* PA = reinterpret_cast<const PtRecA<T>*>(db.PA);
    double total[36];
#pragma unroll
    for (int e = 0; e < 36; ++e) total[e] = 0.0;
    for (int p0 = pbeg; p0 < p1; p0 += 64) {
        const int p = p0 + lane;
        const PtRecA<T> pa = load_ptrec(PA + ds.pair_pt[p < p1 ? p : p1 - 1]);
        T rec[YREC], acc[36];
        obs_record<T>(ct, focal, pa.X, pa.L, rec);
        if (p >= p1) {
#pragma unroll
            for (int e = 9; e < 15; ++e) rec[e] = (T)0;
        }
#pragma unroll
        for (int e = 0; e < 36; ++e) acc[e] = (T)0;
        pair_product<T>(rec, rec, true, acc);
#pragma unroll
        for (int e = 0; e < 36; ++e) total[e] += (double)acc[e];
    }
#pragma unroll
    for (int e = 0; e < 36; ++e) {
        const double v = wave_allsum(total[e]);
        const int r = e / 6, c = e - 6 * r;
        if (lane == e && c >= r) atomicAdd(db.S + (size_t)(6 * j + r) * ds.ld + 6 * j + c, -v * db.cscale[6 * j + r] * db.cscale[6 * j + c]);
    }
}

// The pair pass for SMALL blocks, LPB = 16 lanes per 6x6 block and 64 / LPB blocks per wave -- BASELINE config 5's 500k blocks of ~45
// pairs, every problem with more than ~210 cameras, and every rank of a sharded solve (which owns every block with 1/N of its pairs).
// Nothing is gathered per observation and there is no (qa, qb) pair list: per pair a lane reads the pair's point slot (pair_pt, coalesced
// inside its lane group), ONE 64-byte point-table entry, and re-evaluates both observations (obs_factored).  The blocks of a wave are
// consecutive blocks of ONE block row (build_structure), so the row camera sits in scalar registers for the whole wave; the column
// camera differs per lane group and is held per lane.  The 36 sums are reduced over the LPB lanes of a group by the VALU-only halving
// butterfly (DPP row operations never leave a row of 16 lanes), and the per-camera factors G = Lw D E^T (pair_G) are applied from both
// sides in the epilogue of all NG blocks side by side.
constexpr int SUBF_WPS = 3;      // waves per SIMD the fp32 form is compiled for
template <typename T, int MODE, int LPB>
__global__ __launch_bounds__(64, (sizeof(T) == 4 ? SUBF_WPS : 2)) void k_schur_pairs_sub_f(DeviceStructure ds, DeviceBuffers db) {
    static_assert(LPB == 16, "one DPP row per block");
    constexpr int NG = 64 / LPB;
    __shared__ double tile[NG][36];
    const int lane = threadIdx.x & 63;
    if (MODE == 1 && blockIdx.x == 0) post_linearisation(ds, db);        // block (0,0) is in the first workgroup; all 64 lanes here
    const int sub = lane / LPB, li = lane % LPB;
    const int4 dsc = ds.pwg_desc[(size_t)blockIdx.x * NG + sub];         // one load: block, row camera, pair range
    const bool have = dsc.x >= 0;
    const int b = have ? dsc.x : 0;
    const int2 cj = pair_block_cams(dsc, ds.ncam);                       // (read under `have` only)
    const bool diag = cj.x == cj.y;
    if (MODE == 1 && have && diag) {
        // glue of the block-Jacobi transform for camera j (see k_schur_pairs).  This kernel's OWN copy of pcg_glue_row / pcg_glue_focal
        // (ba_common.h): through the shared helpers the compiler allocates the pair loop below differently -- fp32 loop body 269 -> 284
        // instructions (tools/pair_isa_count.py) -- and that loop is all of BASELINE config 5's pair pass.
        const int j = cj.x, row0 = 6 * j, fo = ds.d - 1;
        const double* Li = db.pcg_binv + (size_t)j * 36;
        const double linv_f = 1.0 / sqrt(db.S[(size_t)fo * ds.ld + fo]);
        for (int e = li; e < 36; e += LPB) {
            const int r = e / 6, c = e - 6 * r;
            store_F(db, (size_t)(row0 + r) * ds.ld + row0 + c, (r == c) ? 1.0 : 0.0);
        }
        for (int l = li; l < 6; l += LPB) {
            double vf = 0.0, vb = 0.0;
            for (int a = 0; a <= l; ++a) { vf += Li[l * 6 + a] * db.S[(size_t)(row0 + a) * ds.ld + fo]; vb += Li[l * 6 + a] * db.rhs[row0 + a]; }
            vf *= linv_f;
            store_F(db, (size_t)(row0 + l) * ds.ld + fo, vf);
            store_F(db, (size_t)fo * ds.ld + row0 + l, vf);
            db.pcg_bt[row0 + l] = vb;
        }
        if (j == 0 && li == LPB - 1) {
            store_F(db, (size_t)fo * ds.ld + fo, 1.0);
            db.pcg_bt[fo] = db.rhs[fo] * linv_f;
            db.pcg_binv[(size_t)ds.ncam * 36] = linv_f;
        }
    }
    const bool work = have && !diag;
    if (!__any(work)) return;
    const LMState* st = db.st;
    const int cur = st->cur;
    const double focal = st->focal[cur];
    const double* tab = db.camtab[cur];
    // lane group 0 always holds a block of the workgroup's row (the descriptors of a workgroup are filled from the front).  Both rows in
    // the precision of the Jacobian blocks (obs_factored_t): the row camera's wave-uniform, the column camera's per lane.
    T Ra[12], Rb[12];
    {
        const int ja = __builtin_amdgcn_readfirstlane(dsc.y), jb = work ? cj.y : 0;
#pragma unroll
        for (int k = 0; k < 12; ++k) { Ra[k] = to_uniform((T)tab[cam_tab_index(k, ja, ds.ncam)]); Rb[k] = (T)tab[cam_tab_index(k, jb, ds.ncam)]; }
    }
    const bool fo_a = tab[cam_tab_index(CT_SMALL, __builtin_amdgcn_readfirstlane(dsc.y), ds.ncam)] != 0.0;
    const bool fo_b = tab[cam_tab_index(CT_SMALL, work ? cj.y : 0, ds.ncam)] != 0.0;
    const T focal_t = (T)focal;
    const PtRecA<T>* PA = reinterpret_cast<const PtRecA<T>*>(db.PA);
    T acc[36];
#pragma unroll
    for (int e = 0; e < 36; ++e) acc[e] = (T)0;
    int p0 = work ? dsc.z : 0;
    const int p1 = work ? dsc.w : 0;
    // the point slot of a round's pair is fetched one round ahead (a round then costs one dependent memory level: the point-table entry);
    // lanes beyond the block's last pair re-read it and contribute nothing
    const bool nonempty = p0 < p1;
    int pt_next = nonempty ? ds.pair_pt[p0 + li < p1 ? p0 + li : p1 - 1] : 0;
    // No branch around the body: a lane group whose block is finished (or empty) keeps evaluating its last pair (point 0 if it never had
    // one) and adds zeros -- a divergent `if` here costs a register copy of all 36 sums per round.
    while (__any(p0 < p1)) {
        const PtRecA<T> pa = load_ptrec(PA + pt_next);
        const bool mine = p0 + li < p1;
        if (nonempty) { const int p = p0 + LPB + li; pt_next = ds.pair_pt[p < p1 ? p : p1 - 1]; }
        T ga[GREC], gb[GREC];
        const T X0 = (T)pa.X[0], X1 = (T)pa.X[1], X2 = (T)pa.X[2];
        obs_factored_t<T>(Ra, fo_a, focal_t, X0, X1, X2, pa.L, ga);
        obs_factored_t<T>(Rb, fo_b, focal_t, X0, X1, X2, pa.L, gb);
        if (!mine) ga[3] = (T)0;                       // (N carries f_a / p_z)
        pair_product_factored<T>(ga, gb, acc);
        p0 += LPB;
    }
    if (!nonempty) {                                   // never had a pair: whatever point 0 gave under these two cameras (0 x inf) is not a sum
#pragma unroll
        for (int e = 0; e < 36; ++e) acc[e] = (T)0;
    }
    int base = 0, len = 36;
    double own[3];                                     // afterwards lane li owns entries base .. base + len - 1 (len <= 3)
    pair_reduce<T, LPB / 2>(acc, lane, base, len, own);
    if (work) {
#pragma unroll
        for (int k = 0; k < 3; ++k) if (k < len) tile[sub][base + k] = -own[k];
    }
    wave_lds_fence();
    if (work) {
        // S_IJ = G_I [sum] G_J^T: pair_epilogue's arithmetic, sixteen lanes over the 36 entries.  Its OWN copy: with one entry of the
        // transform as a helper shared with pair_epilogue the fp32 pair loop above grows from 283 / 269 to 312 / 313 instructions
        // (MODE 0 / 1, tools/pair_isa_count.py; the source of the loop is the same, its register allocation is not).
        for (int e = li; e < 36; e += LPB) {
            const int r = e / 6, c = e - 6 * r;
            double Gi[6], Gj[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) { Gi[a] = db.pair_G[(size_t)cj.x * 36 + 6 * r + a]; Gj[a] = db.pair_G[(size_t)cj.y * 36 + 6 * c + a]; }
            double v = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double u = 0.0;
#pragma unroll
                for (int bb = 0; bb < 6; ++bb) u += tile[sub][6 * a + bb] * Gj[bb];
                v += Gi[a] * u;
            }
            if (MODE == 0) db.S[(size_t)(6 * cj.x + r) * ds.ld + 6 * cj.y + c] = v;
            else store_block_entry(ds, db, b, cj, r, c, v);
        }
    }
}

// Per-camera factor of the factored pair pass (sfmba_device.h, obs_factored): G = Lw D E^T, E = diag(Q, I), Q = R K' (I for a camera on
// the first-order branch), D the Jacobi scales, Lw = Linv (PCG: the block-Jacobi transform) or I.  The rotation part of D E^T is in the
// camera table (CT_QD, make_cam_table).  Row-major 6 x 6 per camera: pair_G[36 j + 6 r + c] (entry-major would let k_finalize's lanes
// store side by side, -1 us there, but costs the pair pass's epilogue +5 us: measured).
// (Sibling: the per-lane row form inside k_finalize, ba_finalize.hip -- lane t forms row t alone from a row picked by 0 / 1 weights; two, because here one lane owns all 36 entries.)
template <bool HAVE_L>
__device__ __forceinline__ void pair_factor(const DeviceBuffers& db, int j, const double (&Lw)[6][6], const double (&Q9)[9], const double (&cs)[6]) {
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double v;
            if (c < 3) {            // sum_{a < 3} Lw[r][a] (D E^T)[a][c],  (D E^T)[a][c] = cs[a] Q[c][a]
                v = 0.0;
#pragma unroll
                for (int a = 0; a < 3; ++a) v += (HAVE_L ? Lw[r][a] : (r == a ? 1.0 : 0.0)) * (cs[a] * Q9[3 * c + a]);
            } else {
                v = (HAVE_L ? Lw[r][c] : (r == c ? 1.0 : 0.0)) * cs[c];
            }
            db.pair_G[(size_t)j * 36 + 6 * r + c] = v;
        }
}
__global__ void k_pair_factors(DeviceStructure ds, DeviceBuffers db) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ds.ncam) return;
    const double none[6][6] = {};
    double Q9[9], cs[6];
#pragma unroll
    for (int e = 0; e < 9; ++e) Q9[e] = db.camtab[db.st->cur][cam_tab_index(CT_QD + e, j, ds.ncam)];
#pragma unroll
    for (int e = 0; e < 6; ++e) cs[e] = db.cscale[6 * j + e];       // (not the table's copy: the first linearisation's table predates the scales)
    pair_factor<false>(db, j, none, Q9, cs);
}

// mode 0: off-diagonal blocks of S (upper triangle; exact solver);  mode 1: the same blocks written straight into S~ = Lb^-1 S Lb^-T
// (both triangles, or the exchange buffer of a sharded solve) + the per-camera glue of the block-Jacobi transform;  mode 2: the
// duplicate pairs inside diagonal blocks.  One wave per block, or -- small blocks (ds.pair_lpb == 16) -- 16 lanes per block.
template <typename T>
void launch_schur_pairs(hipStream_t s, const DeviceStructure& ds, const DeviceBuffers& db, int mode) {
    const dim3 grid(ds.npairwg);
    if (mode != 2 && ds.npairwg <= 0) return;      // (a row-sharded rank without a block row)
    if (mode == 2) {
        if (ds.ndupwg > 0) hipLaunchKernelGGL(k_schur_dups<T>, dim3(ds.ndupwg), dim3(64), 0, s, ds, db);
        return;
    }
    if (mode == 0) hipLaunchKernelGGL(k_pair_factors, dim3((ds.ncam + 63) / 64), dim3(64), 0, s, ds, db);      // D E^T per camera (PCG: k_finalize wrote Linv D E^T)
    if (ds.pair_lpb == 16) {
        if (mode == 1) hipLaunchKernelGGL((k_schur_pairs_sub_f<T, 1, 16>), grid, dim3(64), 0, s, ds, db);
        else hipLaunchKernelGGL((k_schur_pairs_sub_f<T, 0, 16>), grid, dim3(64), 0, s, ds, db);
    } else {
        if (sizeof(T) == 4 && !ds.pair_quad) {
            if (mode == 1) hipLaunchKernelGGL((k_schur_pairs_lane<float, 1>), grid, dim3(64), 0, s, ds, db);
            else hipLaunchKernelGGL((k_schur_pairs_lane<float, 0>), grid, dim3(64), 0, s, ds, db);
        } else if (mode == 1) hipLaunchKernelGGL((k_schur_pairs<T, 1>), grid, dim3(64), 0, s, ds, db);
        else hipLaunchKernelGGL((k_schur_pairs<T, 0>), grid, dim3(64), 0, s, ds, db);
        if (ds.nmulti > 0) {
            if (mode == 1) hipLaunchKernelGGL(k_schur_combine<1>, dim3(ds.nmulti), dim3(64), 0, s, ds, db);
            else hipLaunchKernelGGL(k_schur_combine<0>, dim3(ds.nmulti), dim3(64), 0, s, ds, db);
        }
    }
}
template void launch_schur_pairs<float>(hipStream_t, const DeviceStructure&, const DeviceBuffers&, int);
template void launch_schur_pairs<double>(hipStream_t, const DeviceStructure&, const DeviceBuffers&, int);

}  // namespace sfmba
