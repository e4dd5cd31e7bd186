// tsdf_fill.hip -- hole filling on the MI355X (gfx950): volumetric diffusion of the signed distance into the undefined vertices of
// a TSDF grid (Davis et al., "Filling holes in complex surfaces using volumetric diffusion"), so that the extraction of tsdf_mesh.hip,
// unchanged, closes the surface behind what was seen, at grazing angles and across the holes of a depth map.
//
// The contract is the project's own (include/sfmba.h, sfmba_tsdf_fill / sfmba_tsdf_mesh_fill; arithmetic in tsdf_fill_math.h):
// NOTHING BUT INTEGERS, every pass a JACOBI step that reads the state from before the pass, so the result is BIT-EXACT with a CPU
// restatement and does not depend on how the grid is cut into workgroups.
//
//   quantise      k_fill_quantise: a lane per grid vertex packs (V, known, state, colour, hasC) into ONE 64-BIT WORD and writes it to
//                 BOTH buffers of the ping-pong; the observed vertices are never written again.
//   a pass        k_fill_pass: a lane per grid vertex, x fastest.  A lane whose vertex is observed reads its own word and stops.  Every
//                 other lane gathers its up to six face neighbours (one 8-byte load each; the x neighbours lie in the cache lines the
//                 wave reads anyway, the y and z neighbours are coalesced rows that the wave of the next row reads again out of L2)
//                 and runs fill_update.  A vertex that stays unknown writes nothing (the other buffer holds "unknown" already); a
//                 filled vertex is written in every pass.  NO ATOMIC, no LDS.
//   write back    k_fill_finish: a filled vertex gets W = FW, S = V (FW / 64) and its colour IN PLACE on the device grid; every
//                 other vertex keeps its bits.  The state byte leaves for every vertex; where the count is asked for, every
//                 workgroup writes the number of its filled vertices and the host adds them up (an atomic per wave on one
//                 counter was measured first: the same address from 126 000 waves cost about a millisecond).
//
// DENSE SWEEPS, NO LIST OF ACTIVE BRICKS ("hole filling", has the arithmetic and the measurements): a pass moves 16 bytes per
// vertex at most, so a grid of 8 M vertices is a pass of 75 - 80 us, the order of the launches and scans a compaction of the front would
// add per pass.  Handing every XCD a contiguous eighth of the grid (so that neighbouring rows share an L2) was measured and changed
// nothing: the two buffers fit the Infinity Cache (profiles/tsdf_fill.txt).
//
// SCRATCH beyond the grid: 16 V bytes for the two buffers and V for the state bytes.
#include "tsdf_fill.h"
#include "tsdf_fill_math.h"

#include <cstdint>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;

unsigned blocks_for(long long n) { return (unsigned)((n + LANES - 1) / LANES); }

__global__ __launch_bounds__(LANES) void k_fill_quantise(int nvox, const int* __restrict__ sum, const int* __restrict__ weight,
                                                         const int* __restrict__ csum, const int* __restrict__ cweight, int min_weight,
                                                         unsigned long long* __restrict__ b0, unsigned long long* __restrict__ b1) {
    const int lin = blockIdx.x * LANES + threadIdx.x;
    if (lin >= nvox) return;
    int cs[3] = { 0, 0, 0 }, Wc = 0;                             // (Wc == 0: no colour)
    if (csum) {
        for (int a = 0; a < 3; ++a) cs[a] = csum[3 * (size_t)lin + a];
        Wc = cweight[lin];
    }
    const uint64_t w = fill_quantise(sum[lin], weight[lin], cs, Wc, min_weight);
    b0[lin] = w;
    b1[lin] = w;
}

__global__ __launch_bounds__(LANES) void k_fill_pass(int nx, int ny, int nz, int nvox, int min_neighbours, int pass,
                                                     const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst) {
    const int lin = blockIdx.x * LANES + threadIdx.x;
    if (lin >= nvox) return;
    const uint64_t self = src[lin];
    if (fill_state(self) == 0) return;                           // observed: both buffers hold it
    const int i = lin % nx, j = (lin / nx) % ny, k = lin / (nx * ny);
    const int sy = nx, sz = nx * ny;
    uint64_t nb[6];
    int n = 0;
    if (i > 0) nb[n++] = src[lin - 1];
    if (i < nx - 1) nb[n++] = src[lin + 1];
    if (j > 0) nb[n++] = src[lin - sy];
    if (j < ny - 1) nb[n++] = src[lin + sy];
    if (k > 0) nb[n++] = src[lin - sz];
    if (k < nz - 1) nb[n++] = src[lin + sz];
    const uint64_t w = fill_update(self, nb, n, min_neighbours, pass);
    if (fill_known(w)) dst[lin] = w;                             // (still unknown: dst says so since the quantisation)
}

__global__ __launch_bounds__(LANES) void k_fill_finish(int nvox, const unsigned long long* __restrict__ buf, int FW, int* __restrict__ sum,
                                                       int* __restrict__ weight, int* __restrict__ csum, int* __restrict__ cweight,
                                                       unsigned char* __restrict__ state, int* __restrict__ block_filled) {
    __shared__ int s_count[LANES / 64];
    const int lin = blockIdx.x * LANES + threadIdx.x;
    bool filled = false;
    if (lin < nvox) {
        const uint64_t w = buf[lin];
        state[lin] = (unsigned char)fill_state(w);
        filled = fill_is_filled(w);
        if (filled) {
            int S, W, cs[3], Wc;
            fill_write_back(w, FW, S, W, cs, Wc);
            sum[lin] = S;
            weight[lin] = W;
            if (csum) {
                for (int a = 0; a < 3; ++a) csum[3 * (size_t)lin + a] = cs[a];
                cweight[lin] = Wc;
            }
        }
    }
    if (!block_filled) return;                                   // (uniform: nobody asked for the count)
    const unsigned long long m = __ballot(filled);
    if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int q = 0; q < LANES / 64; ++q) n += s_count[q];
        block_filled[blockIdx.x] = n;                            // its owner writes it: no atomic
    }
}

// fills the device grid in place; *d_state ([nvox]) stays on the device, and so does, if asked for, *d_block_filled (the filled vertices
// of every workgroup of LANES vertices, [blocks_for(nvox)])
int fill_device(hipStream_t s, DeviceArena& scratch, PhaseTimer& tm, const TsdfGridDev& g, const TsdfGridArrays& a, const TsdfFillParams& prm,
                unsigned char** d_state, int** d_block_filled) {
    const size_t V = (size_t)g.nvox;
    const unsigned blocks = blocks_for(g.nvox);
    unsigned long long* buf[2];
    UNIT_ALLOC(scratch, buf[0], unsigned long long, V);
    UNIT_ALLOC(scratch, buf[1], unsigned long long, V);
    UNIT_ALLOC(scratch, *d_state, unsigned char, V);
    int* d_counts = nullptr;
    if (d_block_filled) {
        UNIT_ALLOC(scratch, d_counts, int, blocks);
        *d_block_filled = d_counts;
    }
    tm.begin(TSDF_T_FILL);
    hipLaunchKernelGGL(k_fill_quantise, dim3(blocks), dim3(LANES), 0, s, g.nvox, a.sum, a.weight, a.csum, a.cweight, prm.min_weight, buf[0], buf[1]);
    UNIT_TRY(hipGetLastError());
    for (int p = 1; p <= prm.iterations; ++p) {
        hipLaunchKernelGGL(k_fill_pass, dim3(blocks), dim3(LANES), 0, s, g.nx, g.ny, g.nz, g.nvox, prm.min_neighbours, p, buf[(p - 1) & 1], buf[p & 1]);
        UNIT_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_fill_finish, dim3(blocks), dim3(LANES), 0, s, g.nvox, buf[prm.iterations & 1], fill_weight(prm.min_weight), a.sum, a.weight,
                       a.csum, a.cweight, *d_state, d_counts);
    UNIT_TRY(hipGetLastError());
    tm.end();
    return 0;
}

}  // namespace

int tsdf_fill(hipStream_t s, int device, int nx, int ny, int nz, const int32_t* sum, const int32_t* weight, const int32_t* csum, const int32_t* cweight,
              const TsdfFillParams& prm, int32_t* sum_out, int32_t* weight_out, int32_t* csum_out, int32_t* cweight_out, unsigned char* state,
              int64_t* n_filled, double* timing) {
    tsdf_zero_timing(timing);
    TsdfGridDev g{};
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.nvox = nx * ny * nz;
    const bool colour = csum && cweight;
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    DeviceArena scratch(device);
    TsdfGridArrays a;
    if (int rc = tsdf_alloc_grid(scratch, g, colour, a)) return rc;
    const size_t V = (size_t)g.nvox;
    int* d_bad;
    UNIT_ALLOC(scratch, d_bad, int, 1);
    tm.begin(TSDF_T_UPLOAD);
    UNIT_TRY(hipMemcpyAsync(a.sum, sum, sizeof(int) * V, hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(a.weight, weight, sizeof(int) * V, hipMemcpyHostToDevice, s));
    if (colour) {
        UNIT_TRY(hipMemcpyAsync(a.csum, csum, sizeof(int) * V * 3, hipMemcpyHostToDevice, s));
        UNIT_TRY(hipMemcpyAsync(a.cweight, cweight, sizeof(int) * V, hipMemcpyHostToDevice, s));
    }
    tm.end();
    tm.begin(TSDF_T_CHECK);
    if (int rc = tsdf_check_device(s, g, a, d_bad)) return rc;
    int bad = 0;
    UNIT_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    tm.end();
    if (bad) return TSDF_ERR_GRID;                               // before anything is written, and before a pass reads the grid
    unsigned char* d_state;
    int* d_counts;
    if (int rc = fill_device(s, scratch, tm, g, a, prm, &d_state, &d_counts)) { (void)hipStreamSynchronize(s); return rc; }
    std::vector<int> counts(blocks_for(g.nvox));
    tm.begin(TSDF_T_DOWNLOAD);
    UNIT_TRY(hipMemcpyAsync(counts.data(), d_counts, sizeof(int) * counts.size(), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(sum_out, a.sum, sizeof(int) * V, hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(weight_out, a.weight, sizeof(int) * V, hipMemcpyDeviceToHost, s));
    if (colour) {
        UNIT_TRY(hipMemcpyAsync(csum_out, a.csum, sizeof(int) * V * 3, hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipMemcpyAsync(cweight_out, a.cweight, sizeof(int) * V, hipMemcpyDeviceToHost, s));
    }
    if (state) UNIT_TRY(hipMemcpyAsync(state, d_state, V, hipMemcpyDeviceToHost, s));
    tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    int64_t count = 0;
    for (int c : counts) count += c;
    *n_filled = count;
    if (timing) tm.collect(timing);
    return 0;
}

int tsdf_mesh_fill(hipStream_t s, int device, const TsdfViews& views, const TsdfGrid& grid, const TsdfFillParams& prm, const TsdfMeshOut& out,
                   double* timing) {
    tsdf_zero_timing(timing);
    const TsdfGridDev g = tsdf_grid_dev(grid);
    const bool colour = views.pixels != nullptr;
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    DeviceArena scratch(device);
    TsdfGridArrays a;
    if (int rc = tsdf_alloc_grid(scratch, g, colour, a)) return rc;
    if (int rc = tsdf_integrate_device(s, scratch, tm, views, g, colour, a)) return rc;
    unsigned char* d_state = nullptr;
    if (prm.iterations > 0)                                      // 0 passes: the call sfmba_tsdf_mesh makes
        if (int rc = fill_device(s, scratch, tm, g, a, prm, &d_state, nullptr)) { (void)hipStreamSynchronize(s); return rc; }
    const int rc = tsdf_extract_device(s, scratch, tm, g, a, prm.min_weight, false, out, d_state);
    if (timing) tm.collect(timing);
    return rc;
}

}  // namespace sfmba
