// mesh_texture.hip -- the photographs on the mesh, on the MI355X (gfx950, wave64): a view per triangle and a texture atlas with one
// fixed-size patch per triangle.
//
// The contract is the project's own (include/sfmba.h, sfmba_mesh_texture; arithmetic in texture_math.h): fp64 per element with every
// operation rounded on its own, integers from the 1/16 px image coordinate to the texel, no sum across triangles or texels and NO
// ATOMIC ANYWHERE -- so the result is BIT-EXACT with a CPU restatement (tests/texture_oracle.py) however the work is cut.
//
//   check         k_tex_check: a lane per triangle holds its indices to 0 .. nv-1 and raises a device flag.  The two kernels below
//                 read the flag first and do nothing when it is set, so a bad list is never dereferenced and the host waits once.
//   views         k_tex_views: a lane per triangle, looping over the views in ascending index: three projections, the depth-map test
//                 and the doubled image area per view; keeps the largest score (a later view must be strictly better, so ties go to
//                 the lower index).  The view table is read with a uniform index (scalar loads).  Also writes the three corner uv.
//   raster        k_tex_raster: THE HOT PATH.  A workgroup owns G consecutive blocks of the atlas (2 G triangles; G = 1024 texels'
//                 worth of blocks, 1..32, a run-time value: S and B are never template parameters).  Its first 2 G lanes SET THE
//                 TRIANGLES UP ONCE IN LDS: corners as doubles, corner colours, the chosen view's pose, size and pixel pointer.  Then
//                 the 256 lanes walk the group's texels: one 3-vector blend, one projection with two fp64 divisions, four byte loads
//                 per channel, three byte stores.  A texel nobody owns is written as 0, so the atlas needs no clear.
//
// SCRATCH, for V vertices, T triangles, an atlas of A texels, n images with p pixels and m depth-map pixels: the mesh 15 V + 12 T, the
// outputs 3 A + 36 T, the views 128 n + channels p + 4 m.
#include "mesh_texture.h"
#include "texture_math.h"
#include "device_arena.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;
constexpr int TEX_GROUP_TEXELS = 1024;         // a workgroup takes about this many texels ...
constexpr int TEX_GROUP_MAX_BLOCKS = 32;       // ... in at most this many blocks (64 triangles in LDS)

struct TexImage {
    double P[12];
    long long map_off;       // first float of its depth map among the maps on the device, -1 without a map
    long long raw_off;       // first byte of its pixels among the pixels on the device
    int w, h;
    long long pad;           // 128 bytes
};
static_assert(sizeof(TexImage) == 128, "TexImage is 16 words");

struct TexKernelParams {
    double k4[4];
    double occl_tol;
    long long min_area;
    int nv, nt, n_images, channels;
    int S, B, W, H;          // B: blocks per row of the atlas as laid out (1 for an empty mesh)
    int slots, group;        // block slots of the atlas (rows x B), blocks per workgroup of the raster
};

__device__ __forceinline__ TexView view_of(const TexImage& T, const float* __restrict__ maps, const unsigned char* __restrict__ raw) {
    return TexView{ T.P, T.map_off >= 0 ? maps + T.map_off : nullptr, raw + T.raw_off, T.w, T.h };
}

__global__ __launch_bounds__(LANES) void k_tex_check(int nt, int nv, const int* __restrict__ tri, int* __restrict__ flag) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    if (t >= nt) return;
    bool b = false;
    for (int q = 0; q < 3; ++q) {
        const int v = tri[3 * (size_t)t + q];
        b = b || v < 0 || v >= nv;
    }
    if (b) flag[0] = 1;
}

__device__ __forceinline__ void load_vertex(const float* __restrict__ xyz, int v, double* X) {
    for (int a = 0; a < 3; ++a) X[a] = (double)xyz[3 * (size_t)v + a];
}

__global__ __launch_bounds__(LANES) void k_tex_views(TexKernelParams prm, const int* __restrict__ flag, const float* __restrict__ xyz,
                                                     const int* __restrict__ tri, const TexImage* __restrict__ tab, const float* __restrict__ maps,
                                                     const unsigned char* __restrict__ raw, int* __restrict__ view, long long* __restrict__ score,
                                                     float* __restrict__ uv) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    if (t >= prm.nt || flag[0]) return;
    const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
    double A[3], Bv[3], C[3];
    load_vertex(xyz, a, A);
    load_vertex(xyz, b, Bv);
    load_vertex(xyz, c, C);
    int best_view = -1;
    long long best = 0;
    if (a != b && a != c && b != c && tex_finite3(A) && tex_finite3(Bv) && tex_finite3(C)) {
        for (int i = 0; i < prm.n_images; ++i) {
            const TexView V = view_of(tab[i], maps, raw);
            long long a2;
            const bool cand = tex_candidate(prm.k4, V, A, Bv, C, prm.occl_tol, a2);
            if (tex_eligible(cand, a2, prm.min_area) && -a2 > best) { best = -a2; best_view = i; }
        }
    }
    view[t] = best_view;
    score[t] = best;
    float corner[6];
    tex_corner_uv(t, prm.S, prm.B, corner);
    for (int q = 0; q < 6; ++q) uv[6 * (size_t)t + q] = corner[q];
}

// a triangle as the raster keeps it in LDS
struct TexTri {
    double A[3], B[3], C[3];
    double P[12];                // of its view
    const unsigned char* pixels;
    int w, h, view;
    int colour[3][3];            // [corner][channel]
};

__global__ __launch_bounds__(LANES) void k_tex_raster(TexKernelParams prm, const int* __restrict__ flag, const float* __restrict__ xyz,
                                                      const unsigned char* __restrict__ bgr, const int* __restrict__ tri,
                                                      const TexImage* __restrict__ tab, const float* __restrict__ maps,
                                                      const unsigned char* __restrict__ raw, const int* __restrict__ view,
                                                      unsigned char* __restrict__ atlas) {
    __shared__ TexTri s_tri[2 * TEX_GROUP_MAX_BLOCKS];
    if (flag[0]) return;
    const int S = prm.S, per = (S + 1) * S;
    const long long slot0 = (long long)blockIdx.x * prm.group;
    const int n_slots = (int)min((long long)prm.group, (long long)prm.slots - slot0);
    // ---- the group's triangles, once ----
    if ((int)threadIdx.x < 2 * n_slots) {
        const long long t = 2 * slot0 + threadIdx.x;
        TexTri& R = s_tri[threadIdx.x];
        R.view = -1;
        if (t < prm.nt) {
            const int idx[3] = { tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2] };
            load_vertex(xyz, idx[0], R.A);
            load_vertex(xyz, idx[1], R.B);
            load_vertex(xyz, idx[2], R.C);
            for (int c = 0; c < 3; ++c)
                for (int ch = 0; ch < 3; ++ch) R.colour[c][ch] = bgr ? (int)bgr[3 * (size_t)idx[c] + ch] : 0;
            const int v = view[t];
            R.view = v;
            if (v >= 0) {
                const TexImage& T = tab[v];
                for (int q = 0; q < 12; ++q) R.P[q] = T.P[q];
                R.pixels = raw + T.raw_off;
                R.w = T.w;
                R.h = T.h;
            }
        }
    }
    __syncthreads();
    // ---- the group's texels ----
    const int total = n_slots * per;
    for (int e = threadIdx.x; e < total; e += LANES) {
        const int blk = e / per, r = e - blk * per, y = r / (S + 1), x = r - y * (S + 1);
        const long long slot = slot0 + blk;
        const long long X = (slot % prm.B) * (S + 1) + x, Y = (slot / prm.B) * S + y;
        int i, j;
        const int half = tex_half_of(S, x, y, i, j);
        unsigned char out[3] = { 0, 0, 0 };
        if (2 * slot + half < prm.nt) {
            const TexTri& R = s_tri[2 * blk + half];
            bool sampled = false;
            if (R.view >= 0) {
                const TexView V{ R.P, nullptr, R.pixels, R.w, R.h };
                double P3[3], q[3], u, v;
                int su, sv;
                tex_point(S, i, j, R.A, R.B, R.C, P3);
                if (tex_texel_coord(prm.k4, V, P3, q, u, v, su, sv)) {
                    sampled = true;
                    if (prm.channels == 3) {
                        for (int ch = 0; ch < 3; ++ch) out[ch] = tex_texel(tex_sample12(V, 3, ch, su, sv));
                    } else {
                        out[0] = out[1] = out[2] = tex_texel(tex_sample12(V, 1, 0, su, sv));
                    }
                }
            }
            if (!sampled)
                for (int ch = 0; ch < 3; ++ch) out[ch] = tex_fallback(S, i, j, R.colour[0][ch], R.colour[1][ch], R.colour[2][ch]);
        }
        unsigned char* dst = atlas + ((size_t)Y * (size_t)prm.W + (size_t)X) * 3;
        dst[0] = out[0];
        dst[1] = out[1];
        dst[2] = out[2];
    }
}

unsigned blocks_for(long long n) { return (unsigned)((n + LANES - 1) / LANES); }

#define TEX_COPY(dst, src, bytes, kind) do { if ((bytes) > 0) UNIT_TRY(hipMemcpyAsync(dst, src, bytes, kind, s)); } while (0)

}  // namespace

int mesh_texture(hipStream_t s, int device, const TexMesh& m, const TexViews& v, const TexParams& p, const TexOut& out, double* timing) {
    if (timing) for (int i = 0; i < TEX_T_COUNT; ++i) timing[i] = 0.0;
    DeviceArena scratch(device);
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    const size_t NV = (size_t)m.nv, NT = (size_t)m.nt, texels = (size_t)p.W * (size_t)p.H;

    // the view table
    std::vector<TexImage> tab((size_t)v.n_images);
    long long n_map = 0, n_raw = 0;
    for (int i = 0; i < v.n_images; ++i) {
        TexImage& T = tab[(size_t)i];
        std::memset(&T, 0, sizeof(T));
        for (int q = 0; q < 12; ++q) T.P[q] = (double)v.P[(size_t)i * 12 + q];
        T.w = v.width[i]; T.h = v.height[i];
        const long long px = (long long)T.w * T.h;
        T.map_off = v.depth[i] ? n_map : -1;
        if (v.depth[i]) n_map += px;
        T.raw_off = n_raw;
        n_raw += px * v.channels;
    }

    int *d_flag, *d_tri, *d_view;
    float *d_xyz, *d_maps, *d_uv;
    unsigned char *d_bgr = nullptr, *d_raw, *d_atlas;
    long long* d_score;
    TexImage* d_tab;
    UNIT_ALLOC(scratch, d_flag, int, 1);                         // zeroed
    UNIT_ALLOC(scratch, d_tri, int, NT * 3);
    UNIT_ALLOC(scratch, d_xyz, float, NV * 3);
    if (m.bgr) UNIT_ALLOC(scratch, d_bgr, unsigned char, NV * 3);
    UNIT_ALLOC(scratch, d_tab, TexImage, tab.size());
    UNIT_ALLOC(scratch, d_maps, float, (size_t)n_map);
    UNIT_ALLOC(scratch, d_raw, unsigned char, (size_t)n_raw);
    UNIT_ALLOC(scratch, d_view, int, NT);
    UNIT_ALLOC(scratch, d_score, long long, NT);
    UNIT_ALLOC(scratch, d_uv, float, NT * 6);
    UNIT_ALLOC(scratch, d_atlas, unsigned char, texels * 3);

    tm.begin(TEX_T_UPLOAD);
    TEX_COPY(d_tri, m.tri, sizeof(int) * NT * 3, hipMemcpyHostToDevice);
    TEX_COPY(d_xyz, m.xyz, sizeof(float) * NV * 3, hipMemcpyHostToDevice);
    if (d_bgr) TEX_COPY(d_bgr, m.bgr, NV * 3, hipMemcpyHostToDevice);
    TEX_COPY(d_tab, tab.data(), sizeof(TexImage) * tab.size(), hipMemcpyHostToDevice);
    for (int i = 0; i < v.n_images; ++i) {
        const TexImage& T = tab[(size_t)i];
        const size_t px = (size_t)T.w * T.h;
        if (v.depth[i]) TEX_COPY(d_maps + T.map_off, v.depth[i], sizeof(float) * px, hipMemcpyHostToDevice);
        TEX_COPY(d_raw + T.raw_off, v.pixels + v.img_ptr[i], px * v.channels, hipMemcpyHostToDevice);
    }
    tm.end();

    TexKernelParams prm;
    prm.k4[0] = (double)v.K[0]; prm.k4[1] = (double)v.K[4]; prm.k4[2] = (double)v.K[2]; prm.k4[3] = (double)v.K[5];
    prm.occl_tol = (double)p.occl_tol;
    prm.min_area = (long long)p.min_area;
    prm.nv = m.nv; prm.nt = m.nt; prm.n_images = v.n_images; prm.channels = v.channels;
    prm.S = p.patch; prm.W = p.W; prm.H = p.H;
    prm.B = p.W / (p.patch + 1);
    prm.slots = prm.B * (p.H / p.patch);
    const int per = (p.patch + 1) * p.patch;
    prm.group = std::max(1, std::min(TEX_GROUP_MAX_BLOCKS, TEX_GROUP_TEXELS / per));

    tm.begin(TEX_T_CHECK);
    if (m.nt > 0) {
        hipLaunchKernelGGL(k_tex_check, dim3(blocks_for(m.nt)), dim3(LANES), 0, s, m.nt, m.nv, d_tri, d_flag);
        UNIT_TRY(hipGetLastError());
    }
    tm.next(TEX_T_VIEWS);
    if (m.nt > 0) {
        hipLaunchKernelGGL(k_tex_views, dim3(blocks_for(m.nt)), dim3(LANES), 0, s, prm, d_flag, d_xyz, d_tri, d_tab, d_maps, d_raw, d_view, d_score, d_uv);
        UNIT_TRY(hipGetLastError());
    }
    tm.next(TEX_T_RASTER);
    hipLaunchKernelGGL(k_tex_raster, dim3((unsigned)((prm.slots + prm.group - 1) / prm.group)), dim3(LANES), 0, s, prm, d_flag, d_xyz, d_bgr, d_tri, d_tab,
                       d_maps, d_raw, d_view, d_atlas);
    UNIT_TRY(hipGetLastError());
    tm.end();

    int flag = 0;
    UNIT_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));                           // also: `tab` is spent
    if (flag) return TEX_ERR_INDEX;

    tm.begin(TEX_T_DOWNLOAD);
    TEX_COPY(out.atlas, d_atlas, texels * 3, hipMemcpyDeviceToHost);
    TEX_COPY(out.uv, d_uv, sizeof(float) * NT * 6, hipMemcpyDeviceToHost);
    TEX_COPY(out.view, d_view, sizeof(int) * NT, hipMemcpyDeviceToHost);
    if (out.score) TEX_COPY(out.score, d_score, sizeof(long long) * NT, hipMemcpyDeviceToHost);
    tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    int64_t textured = 0;
    for (size_t t = 0; t < NT; ++t) textured += out.view[t] >= 0;
    *out.n_textured = textured;
    if (timing) tm.collect(timing);
    return 0;
}

}  // namespace sfmba
