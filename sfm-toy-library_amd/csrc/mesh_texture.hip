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
//   labels        (TexLabels, off unless a caller asks) GIVEN: k_tex_given holds the caller's labels to -1 .. n_images-1 (its own flag
//                 word) and writes the corner uv in place of k_tex_views.  SMOOTHED: the same kernel writes uv alone, then the
//                 candidates, the adjacency and the smoothing of mesh_labels.hip write the labels and the scores on the device, so
//                 the views are projected once.  The raster is the same.
//   levelling     (TexLevel, off unless a caller asks; the contract is "levelling the colours across seams", the stages are in
//                 mesh_colour.hip) k_tex_raster<true> keeps the offsets of the triangle's three nodes in its LDS record, blends them
//                 with the texel's own integer weights and adds them to the sample before the texel is rounded (colour_texel); the
//                 texels that the clamp changed are counted: one LDS add per texel that clamps, one global add per workgroup.  The
//                 offsets are GIVEN (sfmba_mesh_texture_levelled) or come from the nodes, colours and passes of mesh_colour.hip on the
//                 final labels, everything staying on the device (sfmba_mesh_texture_adjust).  k_tex_raster<false> is the raster above.
//
// SCRATCH, for V vertices, T triangles, an atlas of A texels, n images with p pixels and m depth-map pixels: the mesh 15 V + 12 T, the
// outputs 3 A + 36 T, the views 128 n + channels p + 4 m.
#include "mesh_texture.h"
#include "mesh_labels.h"
#include "mesh_colour.h"
#include "texture_math.h"
#include "device_arena.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

namespace sfmba {

namespace {

constexpr int LANES = 256;
constexpr int TEX_GROUP_TEXELS = 1024;         // a workgroup takes about this many texels ...
constexpr int TEX_GROUP_MAX_BLOCKS = 32;       // ... in at most this many blocks (64 triangles in LDS)

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

// Labels that k_tex_views does not choose: a lane per triangle writes the corner uv, which k_tex_views writes otherwise.  GIVEN labels
// (sfmba_mesh_texture_from_views; view != NULL) are held to -1 .. n_images-1, raising flag[0], which stops the raster, and flag[1],
// which names the reason.  SMOOTHED labels (view == NULL) come later, from mesh_labels.hip, and need no check.
__global__ __launch_bounds__(LANES) void k_tex_given(TexKernelParams prm, const int* __restrict__ view, int* __restrict__ flag, float* __restrict__ uv) {
    const long long t = (long long)blockIdx.x * LANES + threadIdx.x;
    if (t >= prm.nt) return;
    if (view) {
        const int v = view[t];
        if (v < -1 || v >= prm.n_images) { flag[0] = 1; flag[1] = 1; }
    }
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
// and with the offsets of its three nodes
struct TexTriLevel : TexTri {
    int offset[3][3];            // [corner][channel], 1/256 grey level
};

template <bool LEVEL>
__global__ __launch_bounds__(LANES) void k_tex_raster(TexKernelParams prm, const int* __restrict__ flag, const float* __restrict__ xyz,
                                                      const unsigned char* __restrict__ bgr, const int* __restrict__ tri,
                                                      const TexImage* __restrict__ tab, const float* __restrict__ maps,
                                                      const unsigned char* __restrict__ raw, const int* __restrict__ view,
                                                      unsigned char* __restrict__ atlas, const int* __restrict__ node_of,
                                                      const int4* __restrict__ offsets, unsigned long long* __restrict__ n_clamped) {
    using Record = typename std::conditional<LEVEL, TexTriLevel, TexTri>::type;
    __shared__ Record s_tri[2 * TEX_GROUP_MAX_BLOCKS];
    __shared__ unsigned s_clamped;
    if (flag[0]) return;
    if (LEVEL && threadIdx.x == 0) s_clamped = 0;
    const int S = prm.S, per = (S + 1) * S;
    const long long slot0 = (long long)blockIdx.x * prm.group;
    const int n_slots = (int)min((long long)prm.group, (long long)prm.slots - slot0);
    // ---- the group's triangles, once ----
    if ((int)threadIdx.x < 2 * n_slots) {
        const long long t = 2 * slot0 + threadIdx.x;
        Record& R = s_tri[threadIdx.x];
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
            if constexpr (LEVEL) {
                for (int c = 0; c < 3; ++c) {
                    const int n = node_of[3 * (size_t)t + c];
                    const int4 g = n >= 0 ? offsets[n] : make_int4(0, 0, 0, 0);
                    R.offset[c][0] = g.x; R.offset[c][1] = g.y; R.offset[c][2] = g.z;
                }
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
            const Record& R = s_tri[2 * blk + half];
            bool sampled = false;
            if (R.view >= 0) {
                const TexView V{ R.P, nullptr, R.pixels, R.w, R.h };
                double P3[3], q[3], u, v;
                int su, sv;
                tex_point(S, i, j, R.A, R.B, R.C, P3);
                if (tex_texel_coord(prm.k4, V, P3, q, u, v, su, sv)) {
                    sampled = true;
                    if constexpr (LEVEL) {
                        bool clamped = false;
                        for (int ch = 0; ch < 3; ++ch) {
                            const int s12 = tex_sample12(V, prm.channels, ch, su, sv);
                            out[ch] = colour_texel(S, s12, colour_blend(S, i, j, R.offset[0][ch], R.offset[1][ch], R.offset[2][ch]), clamped);
                        }
                        if (clamped) atomicAdd(&s_clamped, 1u);
                    } else if (prm.channels == 3) {
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
    if constexpr (LEVEL) {
        __syncthreads();
        if (threadIdx.x == 0 && s_clamped) atomicAdd(n_clamped, (unsigned long long)s_clamped);
    }
}

unsigned blocks_for(long long n) { return (unsigned)((n + LANES - 1) / LANES); }

#define TEX_COPY(dst, src, bytes, kind) do { if ((bytes) > 0) UNIT_TRY(hipMemcpyAsync(dst, src, bytes, kind, s)); } while (0)

}  // namespace

void tex_view_table(const TexViews& v, std::vector<TexImage>& tab, long long& n_map, long long& n_raw) {
    tab.assign((size_t)v.n_images, TexImage{});
    n_map = n_raw = 0;
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
}
void tex_camera_params(const TexViews& v, float occl_tol, int64_t min_area, TexKernelParams& prm) {
    prm.k4[0] = (double)v.K[0]; prm.k4[1] = (double)v.K[4]; prm.k4[2] = (double)v.K[2]; prm.k4[3] = (double)v.K[5];
    prm.occl_tol = (double)occl_tol;
    prm.min_area = (long long)min_area;
    prm.n_images = v.n_images; prm.channels = v.channels;
}
int tex_check_indices(hipStream_t s, int nt, int nv, const int* d_tri, int* d_flag) {
    if (nt > 0) {
        hipLaunchKernelGGL(k_tex_check, dim3(blocks_for(nt)), dim3(LANES), 0, s, nt, nv, d_tri, d_flag);
        UNIT_TRY(hipGetLastError());
    }
    return 0;
}

int mesh_texture(hipStream_t s, int device, const TexMesh& m, const TexViews& v, const TexParams& p, const TexOut& out, double* timing,
                 const TexLabels* labels, const TexLevel* level) {
    if (timing) for (int i = 0; i < TEX_T_COUNT; ++i) timing[i] = 0.0;
    DeviceArena scratch(device), raw(device);                    // raw: the label stage's temporaries, not zeroed (mesh_labels.h)
    PhaseTimer tm{ s, timing != nullptr, {}, {} };
    const size_t NV = (size_t)m.nv, NT = (size_t)m.nt, texels = (size_t)p.W * (size_t)p.H;
    const bool given = labels && labels->view_in, smooth = labels && !labels->view_in;
    int64_t st[LABEL_STATS] = { 0 };
    PhaseTimer ltm{ s, smooth && labels->timing != nullptr, {}, {} };
    if (ltm.on) for (int i = 0; i < LAB_T_COUNT; ++i) labels->timing[i] = 0.0;
    const bool offsets_given = level && level->node_of_in;
    int64_t cst[COLOUR_STATS] = { 0 };
    PhaseTimer ctm{ s, level && level->timing != nullptr, {}, {} };
    if (ctm.on) for (int i = 0; i < COL_T_COUNT; ++i) level->timing[i] = 0.0;

    // the view table
    std::vector<TexImage> tab;
    long long n_map = 0, n_raw = 0;
    tex_view_table(v, tab, n_map, n_raw);

    int *d_flag, *d_tri, *d_view;
    float *d_xyz, *d_maps, *d_uv;
    unsigned char *d_bgr = nullptr, *d_raw, *d_atlas;
    long long* d_score;
    TexImage* d_tab;
    UNIT_ALLOC(scratch, d_flag, int, 2);                         // zeroed
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
    // the levelling: the node of every corner, the offset of every node, the count of the texels that clamp
    const int* d_node_of = nullptr;
    const int4* d_g = nullptr;
    unsigned long long* d_clamped = nullptr;
    std::vector<int4> g_rec;
    if (level) UNIT_ALLOC(scratch, d_clamped, unsigned long long, 1);       // zeroed
    if (offsets_given) {
        int* node_of;
        int4* g;
        UNIT_ALLOC(scratch, node_of, int, NT * 3);
        UNIT_ALLOC(scratch, g, int4, (size_t)level->n_nodes);
        g_rec.resize((size_t)level->n_nodes);
        for (size_t n = 0; n < g_rec.size(); ++n) g_rec[n] = make_int4(level->g_in[3 * n], level->g_in[3 * n + 1], level->g_in[3 * n + 2], 1);
        d_node_of = node_of;
        d_g = g;
    }

    tm.begin(TEX_T_UPLOAD);
    if (offsets_given) {
        TEX_COPY(const_cast<int*>(d_node_of), level->node_of_in, sizeof(int) * NT * 3, hipMemcpyHostToDevice);
        TEX_COPY(const_cast<int4*>(d_g), g_rec.data(), sizeof(int4) * g_rec.size(), hipMemcpyHostToDevice);
    }
    TEX_COPY(d_tri, m.tri, sizeof(int) * NT * 3, hipMemcpyHostToDevice);
    TEX_COPY(d_xyz, m.xyz, sizeof(float) * NV * 3, hipMemcpyHostToDevice);
    if (d_bgr) TEX_COPY(d_bgr, m.bgr, NV * 3, hipMemcpyHostToDevice);
    if (given) TEX_COPY(d_view, labels->view_in, sizeof(int) * NT, hipMemcpyHostToDevice);
    TEX_COPY(d_tab, tab.data(), sizeof(TexImage) * tab.size(), hipMemcpyHostToDevice);
    for (int i = 0; i < v.n_images; ++i) {
        const TexImage& T = tab[(size_t)i];
        const size_t px = (size_t)T.w * T.h;
        if (v.depth[i]) TEX_COPY(d_maps + T.map_off, v.depth[i], sizeof(float) * px, hipMemcpyHostToDevice);
        TEX_COPY(d_raw + T.raw_off, v.pixels + v.img_ptr[i], px * v.channels, hipMemcpyHostToDevice);
    }
    tm.end();

    TexKernelParams prm;
    tex_camera_params(v, p.occl_tol, p.min_area, prm);
    prm.nv = m.nv; prm.nt = m.nt;
    prm.S = p.patch; prm.W = p.W; prm.H = p.H;
    prm.B = p.W / (p.patch + 1);
    prm.slots = prm.B * (p.H / p.patch);
    const int per = (p.patch + 1) * p.patch;
    prm.group = std::max(1, std::min(TEX_GROUP_MAX_BLOCKS, TEX_GROUP_TEXELS / per));

    tm.begin(TEX_T_CHECK);
    if (int rc = tex_check_indices(s, m.nt, m.nv, d_tri, d_flag)) return rc;
    tm.next(TEX_T_VIEWS);
    if (m.nt > 0 && (given || smooth)) {
        hipLaunchKernelGGL(k_tex_given, dim3(blocks_for(m.nt)), dim3(LANES), 0, s, prm, given ? d_view : (const int*)nullptr, d_flag, d_uv);
        UNIT_TRY(hipGetLastError());
    } else if (m.nt > 0) {
        hipLaunchKernelGGL(k_tex_views, dim3(blocks_for(m.nt)), dim3(LANES), 0, s, prm, d_flag, d_xyz, d_tri, d_tab, d_maps, d_raw, d_view, d_score, d_uv);
        UNIT_TRY(hipGetLastError());
    }
    if (smooth) {
        // the K best views, the adjacency, the smoothing: they write d_view and d_score.  The smoothing waits for the stream,
        // so the index flag is read first: a list with a bad index goes no further.
        int bad = 0;
        UNIT_TRY(hipMemcpyAsync(&bad, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
        UNIT_TRY(hipStreamSynchronize(s));
        if (bad) return TEX_ERR_INDEX;
        const LabelParams lp{ labels->K, labels->rings, labels->penalty, labels->max_passes };
        raw.set_zeroing(false);                                  // what the label stage takes is written in full before it is read
        int *d_cv = nullptr, *d_adj = nullptr;
        long long* d_cs = nullptr;
        unsigned long long* d_counts = nullptr;
        UNIT_ALLOC(raw, d_cv, int, NT * (size_t)lp.K);
        UNIT_ALLOC(raw, d_cs, long long, NT * (size_t)lp.K);
        UNIT_ALLOC(raw, d_adj, int, NT * 3);
        UNIT_ALLOC(scratch, d_counts, unsigned long long, 3);
        ltm.begin(LAB_T_CANDIDATES);
        if (int rc = labels_candidates_dev(s, prm, d_flag, d_xyz, d_tri, d_tab, d_maps, d_raw, lp.K, d_cv, d_cs)) return rc;
        ltm.end();
        if (int rc = labels_adjacency_dev(s, raw, m.nt, d_tri, d_adj, d_counts, &ltm)) return rc;
        if (int rc = labels_smooth_dev(s, scratch, raw, m.nt, lp, d_cv, d_cs, d_adj, d_view, d_score, st, &ltm)) return rc;
    }
    if (level && !offsets_given) {
        // nodes, colours and passes on the final labels (the smoothing has waited for the stream and the index flag has been read)
        ColourNodes nodes;
        int n_nodes = 0;
        if (int rc = colour_nodes_dev(s, raw, prm, d_xyz, d_tri, d_tab, d_raw, d_view, level->radius, nodes, n_nodes, &ctm)) return rc;
        if (int rc = colour_level_dev(s, raw, n_nodes, nodes.node_vertex, nodes.F, nodes.node_of, nodes.entry, nodes.run, level->weight, level->passes, &d_g, cst,
                                      &ctm))
            return rc;
        d_node_of = nodes.node_of;
    }
    tm.next(TEX_T_RASTER);
    const dim3 raster_grid((unsigned)((prm.slots + prm.group - 1) / prm.group));
    if (level && m.nt > 0) {
        hipLaunchKernelGGL(k_tex_raster<true>, raster_grid, dim3(LANES), 0, s, prm, d_flag, d_xyz, d_bgr, d_tri, d_tab, d_maps, d_raw, d_view, d_atlas, d_node_of,
                           d_g, d_clamped);
    } else {
        hipLaunchKernelGGL(k_tex_raster<false>, raster_grid, dim3(LANES), 0, s, prm, d_flag, d_xyz, d_bgr, d_tri, d_tab, d_maps, d_raw, d_view, d_atlas,
                           (const int*)nullptr, (const int4*)nullptr, (unsigned long long*)nullptr);
    }
    UNIT_TRY(hipGetLastError());
    tm.end();

    int flag[2] = { 0, 0 };
    unsigned long long clamped = 0;
    UNIT_TRY(hipMemcpyAsync(flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, s));
    if (level) UNIT_TRY(hipMemcpyAsync(&clamped, d_clamped, sizeof(clamped), hipMemcpyDeviceToHost, s));
    UNIT_TRY(hipStreamSynchronize(s));                           // also: `tab` and `g_rec` are spent
    if (flag[1]) return TEX_ERR_VIEW;
    if (flag[0]) return TEX_ERR_INDEX;

    tm.begin(TEX_T_DOWNLOAD);
    TEX_COPY(out.atlas, d_atlas, texels * 3, hipMemcpyDeviceToHost);
    TEX_COPY(out.uv, d_uv, sizeof(float) * NT * 6, hipMemcpyDeviceToHost);
    if (out.view) TEX_COPY(out.view, d_view, sizeof(int) * NT, hipMemcpyDeviceToHost);
    if (out.score) TEX_COPY(out.score, d_score, sizeof(long long) * NT, hipMemcpyDeviceToHost);
    tm.end();
    UNIT_TRY(hipStreamSynchronize(s));
    const int32_t* final_view = given ? labels->view_in : out.view;
    int64_t textured = 0;
    for (size_t t = 0; t < NT; ++t) textured += final_view[t] >= 0;
    *out.n_textured = textured;
    if (smooth) for (int i = 0; i < LABEL_STATS; ++i) labels->stats[i] = st[i];
    if (level) {
        cst[COLOUR_S_CLAMPED] = (int64_t)clamped;
        if (level->stats) for (int i = 0; i < COLOUR_STATS; ++i) level->stats[i] = cst[i];
        if (level->n_clamped) *level->n_clamped = (int64_t)clamped;
        if (ctm.on) ctm.collect(level->timing);
    }
    if (timing) tm.collect(timing);
    if (ltm.on) ltm.collect(labels->timing);
    return 0;
}
}  // namespace sfmba
