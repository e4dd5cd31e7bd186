// tsdf_mesh.hip -- from depth maps to a surface on the MI355X (gfx950): the depth maps are averaged along the viewing rays in a
// truncated signed distance grid, and the zero set of the grid leaves as a triangle mesh by marching tetrahedra.
//
// The contract is the project's own (include/sfmba.h, sfmba_tsdf_integrate / sfmba_tsdf_extract / sfmba_tsdf_mesh; arithmetic in
// mesh_math.h): fp64 with every operation rounded on its own per element, and NOTHING BUT INTEGERS is summed per voxel -- so the
// result does not depend on the order of the images and is BIT-EXACT with a CPU restatement.
//
//   integrate     k_tsdf_integrate: a GATHER, one lane per grid vertex, x fastest, so that the lanes of a wave project into
//                 neighbouring pixels of a depth map.  The table of the images with a map (pose, size, offsets; 128 bytes each) goes
//                 through LDS TSDF_TABLE_CHUNK images at a time; every lane reads the same entry (a broadcast).  The lane loops over
//                 the images, keeps its six sums in registers and writes them once.  NO ATOMIC.  (A scatter -- a lane per depth pixel
//                 walking its ray through the band -- would need an atomic per (pixel, voxel) pair and would visit a voxel once per
//                 pixel whose ray crosses it, not once per image: the contract's "the pixel the voxel projects to" is a gather.)
//   check         k_mesh_check (extract only): a grid from the host is held to the bounds the integration guarantees.
//   triangles     k_mesh_count: a lane per cell -> its activity, the inside bits of its corners and its number of triangles
//                 (6 tetrahedra, the case table of mesh_math.h); a hipCUB exclusive sum -> the first triangle of every cell.
//   vertex set    k_mesh_flags: a lane per grid vertex A flags which of its 7 edges (A, A + d) carry a vertex: the ends differ in
//                 sign and an active cell holds the edge (every such edge is used by a triangle: Kuhn's six tetrahedra cover all 19
//                 edges of the cell, and a tetrahedron puts a vertex on each of its edges between an inside and an outside end).
//                 The flags of a vertex are ONE BYTE, its owner writes it: a gather again, no atomic.  A hipCUB exclusive sum of
//                 the counts gives the rank of a key: first[lin] + the number of flagged codes below it.  Ascending key order is
//                 ascending (lin, code) order, so no sort is needed.
//   emit          k_mesh_emit: a lane per cell with triangles writes them in table order; every edge goes to its rank directly
//                 (mesh_rank, the step a separate key -> rank pass would take), so the keys of the triangles never exist in memory.
//   vertices      k_mesh_vertices: a lane per grid vertex with a flag writes its 1..7 vertices (position, colour, key), always from
//                 the lower end A.
//   vfilled       k_mesh_vfilled (sfmba_tsdf_mesh_fill only): a lane per mesh vertex reads the hole filling's state bytes of the two
//                 ends of its edge.  The pieces that work on a device-resident grid (tsdf_alloc_grid, tsdf_check_device,
//                 tsdf_integrate_device, tsdf_extract_device; tsdf_mesh.h) are what tsdf_fill.hip calls: one copy of each.
//
// SCRATCH, for V = nx ny nz voxels (V <= 2^26), T triangles and N vertices: the grid 8 V bytes (24 V with colour), cell bits 2 V,
// triangle counts and offsets 8 V, vertex flags V, vertex counts and offsets 8 V, the scan's temporary (a few KB), 12 T for the
// triangles and 16 N (19 N with colour) for the vertices: at most 43 V + 12 T + 19 N, T <= 12 V, N <= 7 V.
#include "tsdf_mesh.h"
#include "mesh_math.h"
#include "device_arena.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;

struct TsdfImage {
    double P[12];
    long long map_off;       // first float of its depth map among the maps on the device
    long long raw_off;       // first byte of its pixels among the pixels on the device
    int w, h;
    long long pad;           // 128 bytes: the LDS copy moves whole 8-byte words
};
static_assert(sizeof(TsdfImage) == 128, "TsdfImage is copied to LDS as 16 words");

struct IntegrateParams { double k4[4]; double trunc; int n_tab, channels; };

__global__ __launch_bounds__(LANES) void k_tsdf_integrate(TsdfGridDev g, IntegrateParams prm, const TsdfImage* __restrict__ tab,
                                                          const float* __restrict__ maps, const unsigned char* __restrict__ raw,
                                                          int* __restrict__ sum, int* __restrict__ weight, int* __restrict__ csum,
                                                          int* __restrict__ cweight) {
    __shared__ TsdfImage s_tab[TSDF_TABLE_CHUNK];
    const int lin = blockIdx.x * LANES + threadIdx.x;
    const bool live = lin < g.nvox;
    const int i = lin % g.nx, j = (lin / g.nx) % g.ny, k = lin / (g.nx * g.ny);
    const double X[3] = { mesh_grid_coord(g.origin[0], i, g.voxel), mesh_grid_coord(g.origin[1], j, g.voxel), mesh_grid_coord(g.origin[2], k, g.voxel) };
    int S = 0, W = 0, Sc[3] = { 0, 0, 0 }, Wc = 0;
    for (int base = 0; base < prm.n_tab; base += TSDF_TABLE_CHUNK) {
        const int n = min(TSDF_TABLE_CHUNK, prm.n_tab - base);
        __syncthreads();                                         // the previous chunk is spent
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(tab + base);
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(s_tab);
        for (int q = threadIdx.x; q < n * (int)(sizeof(TsdfImage) / 8); q += LANES) dst[q] = src[q];
        __syncthreads();
        if (!live) continue;
        for (int c = 0; c < n; ++c) {
            const TsdfImage& T = s_tab[c];
            int e = 0, px = 0, py = 0;
            bool colour = false;
            double qz, sdf;
            if (!mesh_observe(prm.k4, T.P, X, maps + T.map_off, T.w, T.h, prm.trunc, e, colour, px, py, qz, sdf)) continue;
            S += e;
            ++W;
            if (colour && raw) {
                const unsigned char* p = raw + T.raw_off + ((size_t)py * (size_t)T.w + (size_t)px) * (size_t)prm.channels;
                for (int a = 0; a < 3; ++a) Sc[a] += prm.channels == 3 ? (int)p[a] : (int)p[0];
                ++Wc;
            }
        }
    }
    if (!live) return;
    sum[lin] = S;
    weight[lin] = W;
    if (csum) {
        for (int a = 0; a < 3; ++a) csum[3 * (size_t)lin + a] = Sc[a];
        cweight[lin] = Wc;
    }
}

// ---- extraction ------------------------------------------------------------------------------------------------------------------
// the bounds an integration guarantees: 0 <= W, |S| <= 1024 W, 0 <= Wc, 0 <= a colour sum <= 255 Wc.  Every lane that finds a
// breach stores the same 1.
__global__ __launch_bounds__(LANES) void k_mesh_check(int nvox, const int* __restrict__ sum, const int* __restrict__ weight,
                                                      const int* __restrict__ csum, const int* __restrict__ cweight, int* __restrict__ bad) {
    const int lin = blockIdx.x * LANES + threadIdx.x;
    if (lin >= nvox) return;
    const long long S = sum[lin], W = weight[lin];
    bool b = W < 0 || S > 1024 * W || -S > 1024 * W;
    if (csum) {
        const long long Wc = cweight[lin];
        b = b || Wc < 0;
        for (int a = 0; a < 3; ++a) {
            const long long c = csum[3 * (size_t)lin + a];
            b = b || c < 0 || c > 255 * Wc;
        }
    }
    if (b) *bad = 1;
}

constexpr int CELL_ACTIVE = 0x100;         // cell bits: the inside bits of the eight corners, and this

__global__ __launch_bounds__(LANES) void k_mesh_count(TsdfGridDev g, const int* __restrict__ sum, const int* __restrict__ weight, int min_weight,
                                                      unsigned short* __restrict__ cell_bits, int* __restrict__ tcount) {
    const int lin = blockIdx.x * LANES + threadIdx.x;
    if (lin >= g.nvox) return;
    const int i = lin % g.nx, j = (lin / g.nx) % g.ny, k = lin / (g.nx * g.ny);
    int bits = 0, n = 0;
    if (i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1) {
        bool active = true;
        for (int c = 0; c < 8; ++c) {
            const int at = lin + (c & 1) + ((c >> 1) & 1) * g.nx + ((c >> 2) & 1) * g.nx * g.ny;
            active = active && weight[at] >= min_weight;
            bits |= (sum[at] < 0 ? 1 : 0) << c;
        }
        if (active) {
            bits |= CELL_ACTIVE;
            n = mesh_cell_triangles(bits & 0xff);
        } else {
            bits = 0;
        }
    }
    cell_bits[lin] = (unsigned short)bits;
    tcount[lin] = n;
}

__global__ __launch_bounds__(LANES) void k_mesh_flags(TsdfGridDev g, const int* __restrict__ sum, const unsigned short* __restrict__ cell_bits,
                                                      unsigned char* __restrict__ vmask, int* __restrict__ vcount) {
    const int lin = blockIdx.x * LANES + threadIdx.x;
    if (lin >= g.nvox) return;
    const int A[3] = { lin % g.nx, (lin / g.nx) % g.ny, lin / (g.nx * g.ny) };
    const int n[3] = { g.nx, g.ny, g.nz };
    const int stride[3] = { 1, g.nx, g.nx * g.ny };
    // act bit o (o_x + 2 o_y + 4 o_z): the cell with corner A - o exists and is active
    int act = 0;
    for (int o = 0; o < 8; ++o) {
        bool ok = true;
        int at = lin;
        for (int a = 0; a < 3; ++a) {
            const int c = A[a] - ((o >> a) & 1);
            ok = ok && c >= 0 && c <= n[a] - 2;
            at -= ((o >> a) & 1) * stride[a];
        }
        if (ok && (cell_bits[at] & CELL_ACTIVE)) act |= 1 << o;
    }
    int mask = 0;
    if (act) {
        const bool inA = sum[lin] < 0;
        for (int code = 0; code < 7; ++code) {
            const int d = code + 1;
            // the cells that hold the edge: along an axis with d_a = 1 the corner is A_a, otherwise A_a or A_a - 1
            int holds = 0;
            for (int o = 0; o < 8; ++o)
                if ((o & d) == 0) holds |= 1 << o;
            if (!(act & holds)) continue;                        // (an active cell holds it: B = A + d lies inside the grid)
            const int at = lin + (d & 1) * stride[0] + ((d >> 1) & 1) * stride[1] + ((d >> 2) & 1) * stride[2];
            if ((sum[at] < 0) != inA) mask |= 1 << code;
        }
    }
    vmask[lin] = (unsigned char)mask;
    vcount[lin] = __popc((unsigned)mask);
}

// the rank of key linA * 8 + code among the keys in use
__device__ __forceinline__ int mesh_rank(const int* __restrict__ voff, const unsigned char* __restrict__ vmask, int linA, int code) {
    return voff[linA] + __popc((unsigned)vmask[linA] & ((1u << code) - 1u));
}

__global__ __launch_bounds__(LANES) void k_mesh_emit(TsdfGridDev g, const unsigned short* __restrict__ cell_bits, const int* __restrict__ tcount,
                                                     const int* __restrict__ toff, const int* __restrict__ voff,
                                                     const unsigned char* __restrict__ vmask, int* __restrict__ tri) {
    const int lin = blockIdx.x * LANES + threadIdx.x;
    if (lin >= g.nvox || tcount[lin] == 0) return;
    const int bits = cell_bits[lin] & 0xff;
    size_t o = 3 * (size_t)toff[lin];
    for (int p = 0; p < 6; ++p) {
        const unsigned char* row = mesh_table_row(p, mesh_tet_mask(p, bits));
        for (int q = 0; q < 3 * (int)row[0]; ++q) {
            const int e = row[1 + q], corner = e >> 3;
            const int linA = lin + (corner & 1) + ((corner >> 1) & 1) * g.nx + ((corner >> 2) & 1) * g.nx * g.ny;
            tri[o++] = mesh_rank(voff, vmask, linA, e & 7);
        }
    }
}

__global__ __launch_bounds__(LANES) void k_mesh_vertices(TsdfGridDev g, const int* __restrict__ sum, const int* __restrict__ weight,
                                                         const int* __restrict__ csum, const int* __restrict__ cweight,
                                                         const unsigned char* __restrict__ vmask, const int* __restrict__ voff,
                                                         float* __restrict__ xyz, unsigned char* __restrict__ bgr, int* __restrict__ vkey) {
    const int lin = blockIdx.x * LANES + threadIdx.x;
    if (lin >= g.nvox) return;
    const int mask = vmask[lin];
    if (!mask) return;
    const int A[3] = { lin % g.nx, (lin / g.nx) % g.ny, lin / (g.nx * g.ny) };
    const int SA = sum[lin], WA = weight[lin];
    size_t r = (size_t)voff[lin];
    for (int code = 0; code < 7; ++code) {
        if (!((mask >> code) & 1)) continue;
        const int d[3] = { (code + 1) & 1, ((code + 1) >> 1) & 1, ((code + 1) >> 2) & 1 };
        const int at = lin + d[0] + d[1] * g.nx + d[2] * g.nx * g.ny;
        const double t = mesh_edge_t(SA, WA, sum[at], weight[at]);
        for (int a = 0; a < 3; ++a) xyz[3 * r + a] = mesh_vertex_coord(g.origin[a], A[a], d[a], t, g.voxel);
        if (csum)
            for (int a = 0; a < 3; ++a)
                bgr[3 * r + a] = mesh_vertex_colour(csum[3 * (size_t)lin + a], csum[3 * (size_t)at + a], cweight[lin], cweight[at]);
        vkey[r] = lin * 8 + code;
        ++r;
    }
}

// vfilled of a mesh vertex: 1 iff either end of its edge is a grid vertex the hole filling made (state 1..254; tsdf_fill.hip)
__global__ __launch_bounds__(LANES) void k_mesh_vfilled(TsdfGridDev g, int nv, const int* __restrict__ vkey, const unsigned char* __restrict__ state,
                                                        unsigned char* __restrict__ vfilled) {
    const int r = blockIdx.x * LANES + threadIdx.x;
    if (r >= nv) return;
    const int lin = vkey[r] >> 3, d = (vkey[r] & 7) + 1;
    const int at = lin + (d & 1) + ((d >> 1) & 1) * g.nx + ((d >> 2) & 1) * g.nx * g.ny;
    const int sa = state[lin], sb = state[at];
    vfilled[r] = (unsigned char)(((sa >= 1 && sa <= 254) || (sb >= 1 && sb <= 254)) ? 1 : 0);
}

unsigned blocks_for(long long n) { return (unsigned)((n + LANES - 1) / LANES); }

}  // namespace

int tsdf_check_device(hipStream_t s, const TsdfGridDev& g, const TsdfGridArrays& a, int* d_bad) {
    hipLaunchKernelGGL(k_mesh_check, dim3(blocks_for(g.nvox)), dim3(LANES), 0, s, g.nvox, a.sum, a.weight, a.csum, a.cweight, d_bad);
    UNIT_TRY(hipGetLastError());
    return 0;
}

TsdfGridDev tsdf_grid_dev(const TsdfGrid& grid) {
    TsdfGridDev g;
    for (int a = 0; a < 3; ++a) g.origin[a] = (double)grid.origin[a];
    g.voxel = (double)grid.voxel;
    g.nx = grid.nx; g.ny = grid.ny; g.nz = grid.nz;
    g.nvox = grid.nx * grid.ny * grid.nz;
    return g;
}

int tsdf_alloc_grid(DeviceArena& scratch, const TsdfGridDev& g, bool colour, TsdfGridArrays& a) {
    const size_t V = (size_t)g.nvox;
    a.csum = a.cweight = nullptr;
    UNIT_ALLOC(scratch, a.sum, int, V);
    UNIT_ALLOC(scratch, a.weight, int, V);
    if (colour) {
        UNIT_ALLOC(scratch, a.csum, int, V * 3);
        UNIT_ALLOC(scratch, a.cweight, int, V);
    }
    return 0;
}

// uploads the maps (and, with colour, the pixels) of the images that have a map and fills the device grid
int tsdf_integrate_device(hipStream_t s, DeviceArena& scratch, PhaseTimer& tm, const TsdfViews& v, const TsdfGridDev& g, bool colour, const TsdfGridArrays& a) {
    std::vector<TsdfImage> tab;
    long long n_map = 0, n_raw = 0;
    std::vector<int> image_of;
    for (int i = 0; i < v.n_images; ++i) {
        if (!v.depth[i]) continue;
        TsdfImage T;
        std::memset(&T, 0, sizeof(T));
        for (int q = 0; q < 12; ++q) T.P[q] = (double)v.P[(size_t)i * 12 + q];
        T.w = v.width[i]; T.h = v.height[i];
        T.map_off = n_map;
        T.raw_off = n_raw;
        n_map += (long long)T.w * T.h;
        if (colour) n_raw += (long long)T.w * T.h * v.channels;
        tab.push_back(T);
        image_of.push_back(i);
    }
    TsdfImage* d_tab;
    float* d_maps;
    unsigned char* d_raw = nullptr;
    UNIT_ALLOC(scratch, d_tab, TsdfImage, tab.size());
    UNIT_ALLOC(scratch, d_maps, float, (size_t)n_map);
    if (colour) UNIT_ALLOC(scratch, d_raw, unsigned char, (size_t)n_raw);

    tm.begin(TSDF_T_UPLOAD);
    if (!tab.empty()) UNIT_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(TsdfImage) * tab.size(), hipMemcpyHostToDevice, s));
    for (size_t c = 0; c < tab.size(); ++c) {
        const int i = image_of[c];
        const size_t px = (size_t)tab[c].w * tab[c].h;
        UNIT_TRY(hipMemcpyAsync(d_maps + tab[c].map_off, v.depth[i], sizeof(float) * px, hipMemcpyHostToDevice, s));
        if (colour) UNIT_TRY(hipMemcpyAsync(d_raw + tab[c].raw_off, v.pixels + v.img_ptr[i], px * v.channels, hipMemcpyHostToDevice, s));
    }
    tm.end();

    IntegrateParams prm;
    prm.k4[0] = (double)v.K[0]; prm.k4[1] = (double)v.K[4]; prm.k4[2] = (double)v.K[2]; prm.k4[3] = (double)v.K[5];
    prm.trunc = (double)v.trunc;
    prm.n_tab = (int)tab.size();
    prm.channels = colour ? v.channels : 1;
    tm.begin(TSDF_T_INTEGRATE);
    hipLaunchKernelGGL(k_tsdf_integrate, dim3(blocks_for(g.nvox)), dim3(LANES), 0, s, g, prm, d_tab, d_maps, d_raw, a.sum, a.weight, a.csum, a.cweight);
    UNIT_TRY(hipGetLastError());
    tm.end();
    UNIT_TRY(hipStreamSynchronize(s));                           // `tab` goes out of scope
    return 0;
}

// the mesh of a device grid; check: hold the grid to its bounds first
int tsdf_extract_device(hipStream_t s, DeviceArena& scratch, PhaseTimer& tm, const TsdfGridDev& g, const TsdfGridArrays& a, int min_weight, bool check,
                        const TsdfMeshOut& out, const unsigned char* fill_state) {
    const size_t V = (size_t)g.nvox;
    const unsigned blocks = blocks_for(g.nvox);
    unsigned short* d_cell;
    unsigned char* d_vmask;
    int *d_tcount, *d_toff, *d_vcount, *d_voff, *d_bad;
    UNIT_ALLOC(scratch, d_cell, unsigned short, V);
    UNIT_ALLOC(scratch, d_vmask, unsigned char, V);
    UNIT_ALLOC(scratch, d_tcount, int, V + 1);                   // zeroed: the last count stays 0
    UNIT_ALLOC(scratch, d_toff, int, V + 1);
    UNIT_ALLOC(scratch, d_vcount, int, V + 1);
    UNIT_ALLOC(scratch, d_voff, int, V + 1);
    UNIT_ALLOC(scratch, d_bad, int, 1);
    size_t scan_bytes = 0;
    UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, d_tcount, d_toff, g.nvox + 1, s));
    void* d_tmp = scratch.alloc(std::max(scan_bytes, (size_t)1));
    if (!d_tmp) return (int)hipErrorOutOfMemory;

    if (check) {
        tm.begin(TSDF_T_CHECK);
        if (int rc = tsdf_check_device(s, g, a, d_bad)) return rc;
        tm.end();
    }
    tm.begin(TSDF_T_COUNT_TRI);
    hipLaunchKernelGGL(k_mesh_count, dim3(blocks), dim3(LANES), 0, s, g, a.sum, a.weight, min_weight, d_cell, d_tcount);
    UNIT_TRY(hipGetLastError());
    tm.end();
    tm.begin(TSDF_T_SCAN);
    {
        size_t bytes = scan_bytes;
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, bytes, d_tcount, d_toff, g.nvox + 1, s));
    }
    tm.end();
    tm.begin(TSDF_T_FLAGS);
    hipLaunchKernelGGL(k_mesh_flags, dim3(blocks), dim3(LANES), 0, s, g, a.sum, d_cell, d_vmask, d_vcount);
    UNIT_TRY(hipGetLastError());
    tm.end();
    tm.begin(TSDF_T_SCAN);
    {
        size_t bytes = scan_bytes;
        UNIT_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, bytes, d_vcount, d_voff, g.nvox + 1, s));
    }
    int bad = 0, nt = 0, nv = 0;
    UNIT_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(&nt, d_toff + V, sizeof(int), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(&nv, d_voff + V, sizeof(int), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));
    tm.end();
    if (bad) return TSDF_ERR_GRID;
    *out.n_vertices = nv;
    *out.n_triangles = nt;
    if (nv > out.vcap || nt > out.tcap) return UNIT_ERR_CAPACITY;
    if (nt == 0) return 0;                                       // (then nv == 0 too: a vertex belongs to a triangle)

    const size_t NV = (size_t)nv, NT = (size_t)nt;
    float* d_xyz;
    unsigned char* d_bgr = nullptr;
    int *d_vkey, *d_tri;
    UNIT_ALLOC(scratch, d_xyz, float, NV * 3);
    if (a.csum) UNIT_ALLOC(scratch, d_bgr, unsigned char, NV * 3);
    UNIT_ALLOC(scratch, d_vkey, int, NV);
    UNIT_ALLOC(scratch, d_tri, int, NT * 3);
    tm.begin(TSDF_T_EMIT);
    hipLaunchKernelGGL(k_mesh_emit, dim3(blocks), dim3(LANES), 0, s, g, d_cell, d_tcount, d_toff, d_voff, d_vmask, d_tri);
    UNIT_TRY(hipGetLastError());
    tm.end();
    tm.begin(TSDF_T_VERTICES);
    hipLaunchKernelGGL(k_mesh_vertices, dim3(blocks), dim3(LANES), 0, s, g, a.sum, a.weight, a.csum, a.cweight, d_vmask, d_voff, d_xyz, d_bgr, d_vkey);
    UNIT_TRY(hipGetLastError());
    tm.end();
    tm.begin(TSDF_T_DOWNLOAD);
    UNIT_TRY(hipMemcpyAsync(out.xyz, d_xyz, sizeof(float) * NV * 3, hipMemcpyDeviceToHost, s));
    if (a.csum && out.bgr) UNIT_TRY(hipMemcpyAsync(out.bgr, d_bgr, NV * 3, hipMemcpyDeviceToHost, s));
    if (out.vkey) UNIT_TRY(hipMemcpyAsync(out.vkey, d_vkey, sizeof(int) * NV, hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(out.tri, d_tri, sizeof(int) * NT * 3, hipMemcpyDeviceToHost, s));
    tm.end();
    if (out.vfilled && fill_state) {
        unsigned char* d_vfilled;
        UNIT_ALLOC(scratch, d_vfilled, unsigned char, NV);
        tm.begin(TSDF_T_VERTICES);
        hipLaunchKernelGGL(k_mesh_vfilled, dim3(blocks_for(nv)), dim3(LANES), 0, s, g, nv, d_vkey, fill_state, d_vfilled);
        UNIT_TRY(hipGetLastError());
        tm.next(TSDF_T_DOWNLOAD);
        UNIT_TRY(hipMemcpyAsync(out.vfilled, d_vfilled, NV, hipMemcpyDeviceToHost, s));
        tm.end();
    } else if (out.vfilled) {
        std::memset(out.vfilled, 0, NV);                         // no pass ran: nothing was made up
    }
    UNIT_TRY(hipStreamSynchronize(s));
    return 0;
}

void tsdf_zero_timing(double* timing) {
    if (timing) for (int i = 0; i < TSDF_T_COUNT; ++i) timing[i] = 0.0;
}

int tsdf_integrate(hipStream_t s, int device, const TsdfViews& views, const TsdfGrid& grid, int32_t* sum, int32_t* weight, int32_t* csum,
                   int32_t* cweight, double* timing) {
    tsdf_zero_timing(timing);
    const TsdfGridDev g = tsdf_grid_dev(grid);
    const bool colour = views.pixels && csum && cweight;
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    DeviceArena scratch(device);
    TsdfGridArrays a;
    if (int rc = tsdf_alloc_grid(scratch, g, colour, a)) return rc;
    if (int rc = tsdf_integrate_device(s, scratch, tm, views, g, colour, a)) return rc;
    const size_t V = (size_t)g.nvox;
    tm.begin(TSDF_T_DOWNLOAD);
    UNIT_TRY(hipMemcpyAsync(sum, a.sum, sizeof(int) * V, hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipMemcpyAsync(weight, a.weight, sizeof(int) * V, hipMemcpyDeviceToHost, s));
    if (colour) {
        UNIT_TRY(hipMemcpyAsync(csum, a.csum, sizeof(int) * V * 3, hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipMemcpyAsync(cweight, a.cweight, sizeof(int) * V, hipMemcpyDeviceToHost, s));
    }
    tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    if (timing) tm.collect(timing);
    return 0;
}

int tsdf_extract(hipStream_t s, int device, const TsdfGrid& grid, const int32_t* sum, const int32_t* weight, const int32_t* csum,
                 const int32_t* cweight, int min_weight, const TsdfMeshOut& out, double* timing) {
    tsdf_zero_timing(timing);
    const TsdfGridDev g = tsdf_grid_dev(grid);
    const bool colour = csum && cweight;
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    DeviceArena scratch(device);
    TsdfGridArrays a;
    if (int rc = tsdf_alloc_grid(scratch, g, colour, a)) return rc;
    const size_t V = (size_t)g.nvox;
    tm.begin(TSDF_T_UPLOAD);
    UNIT_TRY(hipMemcpyAsync(a.sum, sum, sizeof(int) * V, hipMemcpyHostToDevice, s));
    UNIT_TRY(hipMemcpyAsync(a.weight, weight, sizeof(int) * V, hipMemcpyHostToDevice, s));
    if (colour) {
        UNIT_TRY(hipMemcpyAsync(a.csum, csum, sizeof(int) * V * 3, hipMemcpyHostToDevice, s));
        UNIT_TRY(hipMemcpyAsync(a.cweight, cweight, sizeof(int) * V, hipMemcpyHostToDevice, s));
    }
    tm.end();
    const int rc = tsdf_extract_device(s, scratch, tm, g, a, min_weight, true, out, nullptr);
    if (timing) tm.collect(timing);
    return rc;
}

int tsdf_mesh(hipStream_t s, int device, const TsdfViews& views, const TsdfGrid& grid, int min_weight, const TsdfMeshOut& out, double* timing) {
    tsdf_zero_timing(timing);
    const TsdfGridDev g = tsdf_grid_dev(grid);
    const bool colour = views.pixels != nullptr;
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    DeviceArena scratch(device);
    TsdfGridArrays a;
    if (int rc = tsdf_alloc_grid(scratch, g, colour, a)) return rc;
    if (int rc = tsdf_integrate_device(s, scratch, tm, views, g, colour, a)) return rc;
    const int rc = tsdf_extract_device(s, scratch, tm, g, a, min_weight, false, out, nullptr);
    if (timing) tm.collect(timing);
    return rc;
}

}  // namespace sfmba
