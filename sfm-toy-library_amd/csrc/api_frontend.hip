// api_frontend.hip -- C ABI of include/sfmba.h, the front-end entry points (everything in front of bundle adjustment: image files,
// features, matches, RANSAC, triangulation, association, dense depth, flow, cloud merge, mesh, mesh cleaning, texturing, label smoothing): argument checks and dispatch.  The work
// is in the unit each wrapper names; the error state, the device checks and the problem / solver entry points are in sfmba_api.hip.
//
// Every wrapper reads: checks, open, call, timing line, mapped result.  Every check comes before the first write: a refused call
// leaves the outputs as they were.  What several entry points refuse in the same words is one check_* function below.
#include "association.h"
#include "cloud_merge.h"
#include "depth_sgm.h"
#include "depth_sweep.h"
#include "essential_ransac.h"
#include "feature_match.h"
#include "flow_math.h"
#include "flow_track.h"
#include "homography_ransac.h"
#include "jpeg_decode.h"
#include "jpeg_math.h"
#include "match_l2.h"
#include "mesh_clean.h"
#include "mesh_clean_math.h"
#include "mesh_decimate.h"
#include "decimate_math.h"
#include "mesh_math.h"
#include "mesh_colour.h"
#include "mesh_labels.h"
#include "mesh_texture.h"
#include "texture_math.h"
#include "orb_extract.h"
#include "png_decode.h"
#include "pnp_ransac.h"
#include "problem.h"
#include "sgm_math.h"
#include "surf_extract.h"
#include "tsdf_fill.h"
#include "tsdf_fill_math.h"
#include "tsdf_mesh.h"
#include <climits>
#include <cmath>

using namespace sfmba;

namespace {
// A CallKit and the unit's timing array: tm() is the array when the environment switch `env` is set (one stderr line per call with
// the HIP-event times of its phases, parsed by tools/*_bench.py), NULL otherwise
template <int N> struct TimedCall : CallKit {
    double t[N];
    const bool on;
    explicit TimedCall(const char* env) : on(std::getenv(env) != nullptr) {}
    double* tm() { return on ? t : nullptr; }
};

// what a unit returned -> SFMBA_OK or the failure; too_large is the unit's own text for UNIT_ERR_TOO_LARGE
int unit_result(int rc, const char* who, const char* too_large = "") {
    if (rc == 0) return SFMBA_OK;
    const std::string w = std::string(who) + ": ";
    if (rc == UNIT_ERR_CAPACITY) return fail(SFMBA_ERR_CAPACITY, w + "output capacity too small");
    if (rc == UNIT_ERR_TOO_LARGE) return fail(SFMBA_ERR_INVALID_ARG, w + too_large);
    if (rc == UNIT_ERR_SIZE) return fail(SFMBA_ERR_INVALID_ARG, w + "the factor gives an image a side outside 1..16384");
    if (rc == UNIT_ERR_HOST_ALLOC) return fail(SFMBA_ERR_ALLOC, w + "host allocation failed");
    if (rc == (int)hipErrorOutOfMemory) return fail(SFMBA_ERR_ALLOC, w + "device allocation failed");
    return fail(SFMBA_ERR_HIP, w + hipGetErrorString((hipError_t)rc));
}

// ---- one function per argument shape that several entry points share; each returns 0 or the failure ----------------------------
// a batch of 8-bit images (n_images >= 0, img_ptr and, for n_images > 0, width and height are not NULL)
int check_images(const char* who, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                 int channels) {
    const std::string w(who);
    if (channels != 1 && channels != 3) return fail(SFMBA_ERR_INVALID_ARG, w + ": channels must be 1 or 3");
    if (img_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr must start at 0");
    for (int i = 0; i < n_images; ++i) {
        if (width[i] < 1 || width[i] > 16384 || height[i] < 1 || height[i] > 16384)
            return fail(SFMBA_ERR_INVALID_ARG, w + ": an image dimension lies outside 1..16384");
        if (img_ptr[i + 1] - img_ptr[i] != (int64_t)width[i] * height[i] * channels)
            return fail(SFMBA_ERR_INVALID_ARG, w + ": img_ptr does not agree with width * height * channels");
    }
    if (n_images > 0 && !pixels) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    return 0;
}
// a match list over the points of n_images images (n_images, n_pairs >= 0, img_ptr and pair_ptr and, for n_pairs > 0, pair_left and
// pair_right are not NULL)
int check_match_list(const char* who, int n_images, const int64_t* img_ptr, const float* pts, int n_pairs, const int32_t* pair_left,
                     const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx) {
    const std::string w(who);
    if (img_ptr[0] < 0 || pair_ptr[0] < 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr and pair_ptr must not be negative");
    for (int i = 0; i < n_images; ++i)
        if (img_ptr[i + 1] < img_ptr[i]) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr not monotone");
    for (int p = 0; p < n_pairs; ++p) {
        if (pair_ptr[p + 1] < pair_ptr[p]) return fail(SFMBA_ERR_INVALID_ARG, "pair_ptr not monotone");
        if (pair_ptr[p + 1] - pair_ptr[p] > (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, w + ": a pair has 2^31 or more matches");
        if (pair_left[p] < 0 || pair_left[p] >= n_images || pair_right[p] < 0 || pair_right[p] >= n_images)
            return fail(SFMBA_ERR_INVALID_ARG, "pair index out of range");
    }
    if (pair_ptr[n_pairs] > pair_ptr[0] && (!query_idx || !train_idx || !pts)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    for (int p = 0; p < n_pairs; ++p) {
        const int64_t nl = img_ptr[pair_left[p] + 1] - img_ptr[pair_left[p]], nr = img_ptr[pair_right[p] + 1] - img_ptr[pair_right[p]];
        for (int64_t e = pair_ptr[p]; e < pair_ptr[p + 1]; ++e)
            if (query_idx[e] < 0 || query_idx[e] >= nl || train_idx[e] < 0 || train_idx[e] >= nr)
                return fail(SFMBA_ERR_INVALID_ARG, w + ": a query_idx / train_idx lies outside its image");
    }
    return 0;
}
// the descriptor rows of n_images images and the pairs to match (the same preconditions); the limit on the rows of one image is
// worded per matcher and stays with it
int check_desc_rows(const char* who, int n_images, const int64_t* img_ptr, const void* desc, int n_pairs, const int32_t* pair_left,
                    const int32_t* pair_right) {
    if (img_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr must start at 0");
    for (int i = 0; i < n_images; ++i)
        if (img_ptr[i + 1] < img_ptr[i]) return fail(SFMBA_ERR_INVALID_ARG, "img_ptr not monotone");
    if (img_ptr[n_images] > 0 && !desc) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    int64_t rows = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int l = pair_left[p], r = pair_right[p];
        if (l < 0 || l >= n_images || r < 0 || r >= n_images) return fail(SFMBA_ERR_INVALID_ARG, "pair index out of range");
        if (img_ptr[r + 1] - img_ptr[r] >= 2) rows += img_ptr[l + 1] - img_ptr[l];
    }
    if (rows >= (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": too many query rows in one call (2^31)");
    return 0;
}
bool too_many_rows(int n_images, const int64_t* img_ptr) {
    for (int i = 0; i < n_images; ++i)
        if (img_ptr[i + 1] - img_ptr[i] >= ((int64_t)1 << 22)) return true;
    return false;
}
int check_ransac(int n_hyp, float threshold_px) {
    if (n_hyp < 1 || n_hyp > 65536) return fail(SFMBA_ERR_INVALID_ARG, "n_hyp must be in 1..65536");
    if (!std::isfinite(threshold_px) || !(threshold_px > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "threshold_px must be finite and > 0");
    return 0;
}
int check_focal(const float* K) {
    if (!std::isfinite(K[0]) || !(K[0] > 0.0f) || !std::isfinite(K[4]) || !(K[4] > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "fx and fy must be finite and > 0");
    return 0;
}
// what every dense call refuses about the sizes, K and P
int depth_check_cameras(const char* who, int n_images, const int32_t* width, const int32_t* height, const float* K, const float* P) {
    const std::string w(who);
    if (n_images < 0 || !K || (n_images > 0 && (!width || !height || !P))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    for (int i = 0; i < n_images; ++i) {
        if (width[i] < 1 || width[i] > 16384 || height[i] < 1 || height[i] > 16384)
            return fail(SFMBA_ERR_INVALID_ARG, w + ": an image dimension lies outside 1..16384");
        for (int q = 0; q < 12; ++q)
            if (!std::isfinite(P[(size_t)i * 12 + q])) return fail(SFMBA_ERR_INVALID_ARG, w + ": non-finite pose of image " + std::to_string(i));
    }
    for (int q : { 0, 4, 2, 5 })
        if (!std::isfinite(K[q])) return fail(SFMBA_ERR_INVALID_ARG, w + ": fx, fy, cx and cy must be finite");
    if (!(K[0] > 0.0f) || !(K[4] > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, w + ": fx and fy must be > 0");
    return 0;
}
// what the sweep and the fuse refuse about the images, K and P
int depth_check_images(const char* who, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                       int channels, const float* K, const float* P) {
    if (n_images < 0 || !img_ptr || !K || (n_images > 0 && (!width || !height || !P || !pixels))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (const int rc = check_images(who, n_images, img_ptr, pixels, width, height, channels)) return rc;
    return depth_check_cameras(who, n_images, width, height, K, P);
}
// a CSR list of 0 / 1 .. 4 other images per row
int depth_check_lists(const char* who, const char* what, int n_images, int n_rows, const int32_t* row_image, const int64_t* ptr, const int32_t* idx,
                      int min_len) {
    const std::string w(who);
    if (!ptr || ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, w + ": " + what + " pointer array must start at 0");
    for (int j = 0; j < n_rows; ++j) {
        const int64_t n = ptr[j + 1] - ptr[j];
        if (n < min_len || n > 4) return fail(SFMBA_ERR_INVALID_ARG, w + ": a row has " + std::to_string((long long)n) + " " + what + " images, outside " +
                                                                       std::to_string(min_len) + "..4");
        if (n > 0 && !idx) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
        const int own = row_image ? row_image[j] : j;
        for (int64_t a = ptr[j]; a < ptr[j + 1]; ++a) {
            if (idx[a] < 0 || idx[a] >= n_images) return fail(SFMBA_ERR_INVALID_ARG, w + ": " + what + " image index out of range");
            if (idx[a] == own) return fail(SFMBA_ERR_INVALID_ARG, w + ": a " + what + " image equals the image it belongs to");
            for (int64_t c = ptr[j]; c < a; ++c)
                if (idx[c] == idx[a]) return fail(SFMBA_ERR_INVALID_ARG, w + ": a " + what + " image is listed twice");
        }
    }
    return 0;
}
// what both flow calls refuse about the pair list and the points' CSR
int flow_check_pairs(const char* who, int n_images, int n_pairs, const int32_t* pair_a, const int32_t* pair_b, const int64_t* pt_ptr) {
    const std::string w(who);
    if (n_images < 0 || n_pairs < 0 || !pt_ptr || (n_pairs > 0 && !pair_b)) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (pt_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, w + ": pt_ptr must start at 0");
    for (int p = 0; p < n_pairs; ++p) {
        if ((pair_a && (pair_a[p] < 0 || pair_a[p] >= n_images)) || pair_b[p] < 0 || pair_b[p] >= n_images)
            return fail(SFMBA_ERR_INVALID_ARG, w + ": pair index out of range");
        if (pt_ptr[p + 1] < pt_ptr[p]) return fail(SFMBA_ERR_INVALID_ARG, w + ": pt_ptr not monotone");
    }
    if (pt_ptr[n_pairs] >= (int64_t)1 << 31) return fail(SFMBA_ERR_INVALID_ARG, w + ": 2^31 or more points in one call");
    return 0;
}
// the files of a batch, back to back in `bytes`
int check_file_ptr(int n_images, const int64_t* file_ptr, const unsigned char* bytes) {
    if (n_images < 0 || !file_ptr) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (file_ptr[0] < 0) return fail(SFMBA_ERR_INVALID_ARG, "file_ptr must not be negative");
    for (int i = 0; i < n_images; ++i)
        if (file_ptr[i + 1] < file_ptr[i]) return fail(SFMBA_ERR_INVALID_ARG, "file_ptr not monotone");
    if (file_ptr[n_images] > file_ptr[0] && !bytes) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    return 0;
}
// the timing line of the two calls that end in jpeg_decode.hip
void image_timing_line(const char* what, const double* tm) {
    std::fprintf(stderr, "[sfmba %s] entropy_ms %.6f upload_ms %.6f idct_ms %.6f colour_ms %.6f resize_ms %.6f download_ms %.6f groups %d\n", what,
                 tm[JPEG_T_ENTROPY], tm[JPEG_T_UPLOAD], tm[JPEG_T_IDCT], tm[JPEG_T_COLOUR], tm[JPEG_T_RESIZE], tm[JPEG_T_DOWNLOAD], (int)tm[JPEG_T_GROUPS]);
}
// what the three mesh calls refuse about the grid, the views and the outputs; their failure text and their timing line
int tsdf_check_dims(const char* who, int nx, int ny, int nz) {
    const std::string w(who);
    if (nx < 1 || nx > MESH_MAX_DIM || ny < 1 || ny > MESH_MAX_DIM || nz < 1 || nz > MESH_MAX_DIM)
        return fail(SFMBA_ERR_INVALID_ARG, w + ": a grid dimension lies outside 1..1024");
    if ((int64_t)nx * ny * nz > (int64_t)MESH_MAX_VOXELS) return fail(SFMBA_ERR_INVALID_ARG, w + ": more than 2^26 voxels");
    return 0;
}
int tsdf_check_min_weight(const char* who, int min_weight) {
    if (min_weight < 1 || min_weight > MESH_MAX_WEIGHT) return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": min_weight must be in 1..65535");
    return 0;
}
// what the two hole-filling calls refuse about the passes and the rule
int tsdf_check_fill(const char* who, int iterations, int min_neighbours) {
    const std::string w(who);
    if (iterations < 0 || iterations > FILL_MAX_ITERATIONS) return fail(SFMBA_ERR_INVALID_ARG, w + ": iterations must be in 0..254");
    if (min_neighbours < 1 || min_neighbours > 6) return fail(SFMBA_ERR_INVALID_ARG, w + ": min_neighbours must be in 1..6");
    return 0;
}
int tsdf_check_grid(const char* who, const float* origin, float voxel, int nx, int ny, int nz) {
    const std::string w(who);
    if (!origin) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(origin[a])) return fail(SFMBA_ERR_INVALID_ARG, w + ": origin must be finite");
    if (!std::isfinite(voxel) || !(voxel > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, w + ": voxel must be finite and > 0");
    return tsdf_check_dims(who, nx, ny, nz);
}
// what the fuse refuses about images, sizes, K and P (the pixels may be missing here), and trunc
int tsdf_check_views(const char* who, const TsdfViews& v) {
    const std::string w(who);
    if (v.n_images > 0 && !v.depth) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (v.pixels) {
        if (const int rc = depth_check_images(who, v.n_images, v.img_ptr, v.pixels, v.width, v.height, v.channels, v.K, v.P)) return rc;
    } else if (const int rc = depth_check_cameras(who, v.n_images, v.width, v.height, v.K, v.P)) {
        return rc;
    }
    if (v.n_images > MESH_MAX_WEIGHT) return fail(SFMBA_ERR_INVALID_ARG, w + ": more than 65535 images in one call");
    if (!std::isfinite(v.trunc) || !(v.trunc > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, w + ": trunc must be finite and > 0");
    int64_t px = 0;
    for (int i = 0; i < v.n_images; ++i)
        if (v.depth[i]) px += (int64_t)v.width[i] * v.height[i];
    if (px >= (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, w + ": too many pixels with a depth map in one call (2^31)");
    return 0;
}
int tsdf_check_out(const char* who, int min_weight, bool colour, const TsdfMeshOut& o) {
    if (o.vcap < 0 || o.tcap < 0 || !o.n_vertices || !o.n_triangles || (o.vcap > 0 && (!o.xyz || (colour && !o.bgr))) || (o.tcap > 0 && !o.tri))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    return tsdf_check_min_weight(who, min_weight);
}
int tsdf_result(int rc, const char* who) {
    if (rc == TSDF_ERR_GRID)
        return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": the grid breaks 0 <= W, |S| <= 1024 W, 0 <= Wc or 0 <= colour sum <= 255 Wc");
    return unit_result(rc, who);
}
void tsdf_fill_timing_line(const char* what, const double* t, const TsdfGrid& g, int iterations, long long filled, long long nv, long long nt) {
    std::fprintf(stderr,
                 "[sfmba %s] upload_ms %.6f integrate_ms %.6f check_ms %.6f fill_ms %.6f count_ms %.6f scan_ms %.6f flags_ms %.6f emit_ms %.6f "
                 "vertices_ms %.6f download_ms %.6f voxels %lld passes %d filled %lld vertices %lld triangles %lld\n",
                 what, t[TSDF_T_UPLOAD], t[TSDF_T_INTEGRATE], t[TSDF_T_CHECK], t[TSDF_T_FILL], t[TSDF_T_COUNT_TRI], t[TSDF_T_SCAN], t[TSDF_T_FLAGS],
                 t[TSDF_T_EMIT], t[TSDF_T_VERTICES], t[TSDF_T_DOWNLOAD], (long long)g.nx * g.ny * g.nz, iterations, filled, nv, nt);
}
void tsdf_timing_line(const char* what, const double* t, const TsdfGrid& g, long long nv, long long nt) {
    std::fprintf(stderr,
                 "[sfmba %s] upload_ms %.6f integrate_ms %.6f check_ms %.6f count_ms %.6f scan_ms %.6f flags_ms %.6f emit_ms %.6f vertices_ms %.6f "
                 "download_ms %.6f voxels %lld vertices %lld triangles %lld\n",
                 what, t[TSDF_T_UPLOAD], t[TSDF_T_INTEGRATE], t[TSDF_T_CHECK], t[TSDF_T_COUNT_TRI], t[TSDF_T_SCAN], t[TSDF_T_FLAGS], t[TSDF_T_EMIT],
                 t[TSDF_T_VERTICES], t[TSDF_T_DOWNLOAD], (long long)g.nx * g.ny * g.nz, nv, nt);
}
// what the four mesh-cleaning calls refuse about the mesh, the filter's rule, the smoothing's parameters and the capacities; their
// failure text and their timing line
int clean_check_mesh(const char* who, int64_t n_vertices, const float* xyz, bool want_xyz, int64_t n_triangles, const int32_t* tri) {
    const std::string w(who);
    if (n_vertices < 0 || n_vertices > (int64_t)INT_MAX || n_triangles < 0 || n_triangles > (int64_t)INT_MAX)
        return fail(SFMBA_ERR_INVALID_ARG, w + ": n_vertices and n_triangles must lie in 0 .. 2^31 - 1");
    if ((n_triangles > 0 && !tri) || (want_xyz && n_vertices > 0 && !xyz)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    return 0;
}
int clean_check_filter(const char* who, int min_triangles, int keep_largest) {
    if (min_triangles < 1) return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": min_triangles must be >= 1");
    if (keep_largest != 0 && keep_largest != 1) return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": keep_largest must be 0 or 1");
    return 0;
}
int clean_check_smooth(const char* who, const float* origin, float quantum, int iterations, float lambda, float mu, CleanSmoothParams& p) {
    const std::string w(who);
    if (!origin) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(origin[a])) return fail(SFMBA_ERR_INVALID_ARG, w + ": origin must be finite");
        p.origin[a] = (double)origin[a];
    }
    if (!std::isfinite(quantum) || !(quantum > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, w + ": quantum must be finite and > 0");
    p.quantum = (double)quantum;
    if (iterations < 0 || iterations > CLEAN_MAX_ITERATIONS) return fail(SFMBA_ERR_INVALID_ARG, w + ": iterations must be in 0..100");
    p.iterations = iterations;
    if (!clean_factor(lambda, 1, 65536, p.L)) return fail(SFMBA_ERR_INVALID_ARG, w + ": lambda must quantise to 1..65536 / 65536");
    if (!clean_factor(mu, -131072, -1, p.M)) return fail(SFMBA_ERR_INVALID_ARG, w + ": mu must quantise to -131072..-1 / 65536");
    return 0;
}
int clean_check_out(const CleanFilterOut& o, bool colour) {
    if (o.vcap < 0 || o.tcap < 0 || !o.n_vertices || !o.n_triangles || (o.vcap > 0 && (!o.xyz || (colour && !o.bgr))) || (o.tcap > 0 && !o.tri))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    return 0;
}
int clean_result(int rc, const char* who) {
    if (rc == CLEAN_ERR_INDEX) return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": a triangle index lies outside the vertex list");
    if (rc == CLEAN_ERR_COORD) return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": a coordinate is not finite or lies 2^25 quanta or more from the origin");
    return unit_result(rc, who);
}
void clean_timing_line(const char* what, const double* t, long long nv, long long nt, long long nv_out, long long nt_out) {
    std::fprintf(stderr,
                 "[sfmba %s] upload_ms %.6f check_ms %.6f components_ms %.6f filter_ms %.6f quantise_ms %.6f smooth_ms %.6f normals_ms %.6f "
                 "download_ms %.6f vertices %lld triangles %lld vertices_out %lld triangles_out %lld\n",
                 what, t[CLEAN_T_UPLOAD], t[CLEAN_T_CHECK], t[CLEAN_T_COMPONENTS], t[CLEAN_T_FILTER], t[CLEAN_T_QUANTISE], t[CLEAN_T_SMOOTH],
                 t[CLEAN_T_NORMALS], t[CLEAN_T_DOWNLOAD], nv, nt, nv_out, nt_out);
}
// what the two texturing calls refuse about the layout; W and H of the atlas
int texture_check_layout(const char* who, int64_t n_triangles, int patch, int blocks_per_row, long long& W, long long& H) {
    const std::string w(who);
    if (n_triangles < 0 || n_triangles > (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, w + ": n_triangles must lie in 0 .. 2^31 - 1");
    if (patch < TEX_MIN_PATCH || patch > TEX_MAX_PATCH) return fail(SFMBA_ERR_INVALID_ARG, w + ": patch must be in 3..64");
    if (blocks_per_row < 1) return fail(SFMBA_ERR_INVALID_ARG, w + ": blocks_per_row must be >= 1");
    if (!tex_atlas_size((long long)n_triangles, patch, blocks_per_row, W, H))
        return fail(SFMBA_ERR_INVALID_ARG, w + ": the atlas has a side above 16384");
    return 0;
}
// what the texturing calls refuse about the view rule
int texture_check_rule(const char* who, float occl_tol, int64_t min_area) {
    const std::string w(who);
    if (!std::isfinite(occl_tol) || occl_tol < 0.0f) return fail(SFMBA_ERR_INVALID_ARG, w + ": occl_tol must be finite and >= 0");
    if (min_area < 0) return fail(SFMBA_ERR_INVALID_ARG, w + ": min_area must be >= 0");
    return 0;
}
// ---- what the label calls refuse ------------------------------------------------------------------------------------------------
int label_check_count(const char* who, int64_t n_triangles) {
    if (n_triangles < 0 || n_triangles > (int64_t)(INT_MAX / 3))
        return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": 3 n_triangles must lie in 0 .. 2^31 - 1");
    return 0;
}
int label_check_k(const char* who, int n_candidates) {
    if (n_candidates < 1 || n_candidates > LABEL_MAX_K) return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": n_candidates must be in 1..8");
    return 0;
}
int label_check_params(const char* who, int rings, int penalty, int max_passes) {
    const std::string w(who);
    if (rings < 0 || rings > LABEL_MAX_RINGS) return fail(SFMBA_ERR_INVALID_ARG, w + ": rings must be in 0..8");
    if (penalty < 0 || penalty > LABEL_MAX_PENALTY) return fail(SFMBA_ERR_INVALID_ARG, w + ": penalty must be in 0..65535");
    if (max_passes < 0 || max_passes > LABEL_MAX_PASSES) return fail(SFMBA_ERR_INVALID_ARG, w + ": max_passes must be in 0..10000");
    return 0;
}
// the lists as sfmba_mesh_view_candidates writes them and an adjacency within the mesh
int label_check_lists(const char* who, int64_t nt, int n_images, int K, const int32_t* cand_view, const int64_t* cand_score, const int32_t* adj) {
    const std::string w(who);
    for (int64_t t = 0; t < nt; ++t) {
        for (int q = 0; q < 3; ++q)
            if (adj[3 * t + q] < -1 || adj[3 * t + q] >= nt) return fail(SFMBA_ERR_INVALID_ARG, w + ": an adj entry lies outside -1 .. n_triangles-1");
        for (int k = 0; k < K; ++k) {
            const int32_t v = cand_view[t * K + k];
            const int64_t s = cand_score[t * K + k];
            if (v < -1 || v >= n_images) return fail(SFMBA_ERR_INVALID_ARG, w + ": a cand_view lies outside -1 .. n_images-1");
            const bool ordered = v < 0 ? s == 0 : (s > 0 && s < LABEL_SCORE_LIMIT && (k == 0 || (cand_view[t * K + k - 1] >= 0 && cand_score[t * K + k - 1] >= s)));
            if (!ordered) return fail(SFMBA_ERR_INVALID_ARG, w + ": a row is not a list of sfmba_mesh_view_candidates (scores in 1 .. 2^37-1, descending, then -1 and 0)");
        }
    }
    return 0;
}
// ---- what the levelling calls refuse ---------------------------------------------------------------------------------------------
int colour_check_params(const char* who, int sample_radius, int seam_weight, int passes) {
    const std::string w(who);
    if (sample_radius < 0 || sample_radius > COLOUR_MAX_RADIUS) return fail(SFMBA_ERR_INVALID_ARG, w + ": sample_radius must be in 0..2");
    if (seam_weight < 1 || seam_weight > COLOUR_MAX_WEIGHT) return fail(SFMBA_ERR_INVALID_ARG, w + ": seam_weight must be in 1..256");
    if (passes < 0 || passes > COLOUR_MAX_PASSES) return fail(SFMBA_ERR_INVALID_ARG, w + ": passes must be in 0..1024");
    return 0;
}
// every row of node_of is -1 -1 -1 or three nodes in 0 .. n_nodes-1
int colour_check_rows(const char* who, int64_t nt, const int32_t* node_of, int64_t n_nodes) {
    const std::string w(who);
    for (int64_t t = 0; t < nt; ++t) {
        int none = 0;
        for (int q = 0; q < 3; ++q) {
            const int32_t n = node_of[3 * t + q];
            if (n < -1 || n >= n_nodes) return fail(SFMBA_ERR_INVALID_ARG, w + ": a node_of entry lies outside -1 .. n_nodes-1");
            none += n < 0;
        }
        if (none != 0 && none != 3) return fail(SFMBA_ERR_INVALID_ARG, w + ": a node_of row is partly -1");
    }
    return 0;
}
int texture_result(int rc, const char* who) {
    if (rc == TEX_ERR_INDEX) return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": a triangle index lies outside the vertex list");
    if (rc == TEX_ERR_VIEW) return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": a view lies outside -1 .. n_images-1");
    return unit_result(rc, who);
}
void label_timing_line(const char* what, const double* t, long long nt) {
    std::fprintf(stderr, "[sfmba %s] upload_ms %.6f candidates_ms %.6f keys_ms %.6f sort_ms %.6f link_ms %.6f rings_ms %.6f start_ms %.6f gain_ms %.6f "
                         "move_ms %.6f stats_ms %.6f download_ms %.6f triangles %lld\n",
                 what, t[LAB_T_UPLOAD], t[LAB_T_CANDIDATES], t[LAB_T_KEYS], t[LAB_T_SORT], t[LAB_T_LINK], t[LAB_T_RINGS], t[LAB_T_START], t[LAB_T_GAIN],
                 t[LAB_T_MOVE], t[LAB_T_STATS], t[LAB_T_DOWNLOAD], nt);
}
}  // namespace

extern "C" {
// ---- triangulation (SfMStereoUtilities::triangulateViews) --------------------------------------------------------------------------
int sfmba_triangulate(int device, int64_t n, const float* left_xy, const float* right_xy, const float* K, const float* P_left,
                      const float* P_right, float max_reproj_px, float* points3d, unsigned char* keep, float* reproj_err) {
    if (n < 0 || !K || !P_left || !P_right || (n > 0 && (!left_xy || !right_xy || !points3d || !keep)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (n == 0) return check_device(device);
    DeviceArena arena(device);
    CallKit ck;
    if (const int rc = ck.open(device)) return rc;
    const HostKit& kit = ck.kit;
    float* d_l = arena.alloc_n<float>((size_t)2 * n);
    float* d_r = arena.alloc_n<float>((size_t)2 * n);
    float* d_x = arena.alloc_n<float>((size_t)3 * n);
    float* d_e = reproj_err ? arena.alloc_n<float>((size_t)2 * n) : nullptr;
    unsigned char* d_k = arena.alloc_n<unsigned char>((size_t)n);
    if (!d_l || !d_r || !d_x || !d_k || (reproj_err && !d_e)) return fail(SFMBA_ERR_ALLOC, "device allocation failed");
    HIP_TRY(hipMemcpyAsync(d_l, left_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, kit.stream));
    HIP_TRY(hipMemcpyAsync(d_r, right_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, kit.stream));
    launch_triangulate(kit.stream, (long long)n, d_l, d_r, K, P_left, P_right, max_reproj_px, d_x, d_k, d_e);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(points3d, d_x, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, kit.stream));
    HIP_TRY(hipMemcpyAsync(keep, d_k, (size_t)n, hipMemcpyDeviceToHost, kit.stream));
    if (reproj_err) HIP_TRY(hipMemcpyAsync(reproj_err, d_e, sizeof(float) * 2 * (size_t)n, hipMemcpyDeviceToHost, kit.stream));
    HIP_TRY(hipStreamSynchronize(kit.stream));
    return SFMBA_OK;
}

int sfmba_triangulate_pairs(int device, int n_images, const int64_t* img_ptr, const float* pts, const float* K, int n_pairs, const int32_t* pair_left,
                            const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx,
                            const unsigned char* mask, const float* P_left, const float* P_right, float max_reproj_px, float* points3d,
                            unsigned char* keep, float* reproj_err, int64_t* kept_ptr, int64_t* kept_idx) {
    if (n_images < 0 || n_pairs < 0 || !img_ptr || !pair_ptr || !K || !kept_ptr || (n_pairs > 0 && (!pair_left || !pair_right || !P_left || !P_right)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (!std::isfinite(max_reproj_px) || max_reproj_px < 0.0f) return fail(SFMBA_ERR_INVALID_ARG, "max_reproj_px must be finite and >= 0");
    if (const int rc = check_match_list("triangulate_pairs", n_images, img_ptr, pts, n_pairs, pair_left, pair_right, pair_ptr, query_idx, train_idx)) return rc;
    const int64_t total = pair_ptr[n_pairs];
    if (total > 0 && (!points3d || !keep || !kept_idx)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (total >= (int64_t)INT_MAX - 256) return fail(SFMBA_ERR_INVALID_ARG, "triangulate_pairs: too many entries for one call (2^31)");
    if (total == pair_ptr[0]) {                                       // no entry belongs to a pair: nothing runs on the device
        if (const int rc = check_device(device)) return rc;
        for (int64_t e = 0; e < total; ++e) {
            points3d[3 * e] = points3d[3 * e + 1] = points3d[3 * e + 2] = 0.0f;
            keep[e] = 0;
            if (reproj_err) reproj_err[2 * e] = reproj_err[2 * e + 1] = 0.0f;
        }
        for (int p = 0; p <= n_pairs; ++p) kept_ptr[p] = 0;
        return SFMBA_OK;
    }
    CallKit ck;
    if (const int rc = ck.open(device)) return rc;
    return unit_result(triangulate_pairs(ck.kit.stream, device, n_images, img_ptr, pts, K, n_pairs, pair_left, pair_right, pair_ptr, query_idx, train_idx,
                                         mask, P_left, P_right, max_reproj_px, points3d, keep, reproj_err, kept_ptr, kept_idx), "triangulate_pairs");
}

// ---- association joins -----------------------------------------------------------------------
int sfmba_find_2d3d_matches(int device, int n_views, const unsigned char* view_done, int n_pt, const int64_t* view_ptr,
                            const int32_t* view_idx, const int32_t* feat_idx, int n_pairs, const int32_t* pair_left,
                            const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx,
                            int64_t* out_ptr, int32_t* out_point, int32_t* out_feature, int64_t cap, int64_t* total) {
    if (n_views < 0 || n_pt < 0 || n_pairs < 0 || cap < 0 || !out_ptr || !total || (n_views > 0 && !view_done) || !view_ptr ||
        (n_pairs > 0 && (!pair_left || !pair_right || !pair_ptr)) || (cap > 0 && (!out_point || !out_feature)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (view_ptr[0] != 0 || (n_pairs > 0 && pair_ptr[0] != 0)) return fail(SFMBA_ERR_INVALID_ARG, "CSR pointers must start at 0");
    for (int i = 0; i < n_pt; ++i) if (view_ptr[i + 1] < view_ptr[i]) return fail(SFMBA_ERR_INVALID_ARG, "view_ptr not monotone");
    for (int p = 0; p < n_pairs; ++p) if (pair_ptr[p + 1] < pair_ptr[p]) return fail(SFMBA_ERR_INVALID_ARG, "pair_ptr not monotone");
    if ((view_ptr[n_pt] > 0 && (!view_idx || !feat_idx)) || (n_pairs > 0 && pair_ptr[n_pairs] > 0 && (!query_idx || !train_idx)))
        return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    CallKit ck;
    if (const int rc = ck.open(device)) return rc;
    return unit_result(assoc_find_2d3d(ck.kit.stream, device, n_views, view_done, n_pt, view_ptr, view_idx, feat_idx, n_pairs, pair_left, pair_right,
                                       pair_ptr, query_idx, train_idx, out_ptr, out_point, out_feature, cap, total),
                       "find_2d3d_matches", "problem too large for 32-bit indices");
}

int sfmba_merge_candidates(int device, int n_exist, const float* exist_xyz, int n_new, const float* new_xyz, float max_dist,
                           int64_t* cand_ptr, int32_t* cand_idx, int64_t cap, int64_t* total) {
    if (n_exist < 0 || n_new < 0 || cap < 0 || !cand_ptr || !total || (n_exist > 0 && !exist_xyz) || (n_new > 0 && !new_xyz) || (cap > 0 && !cand_idx))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    CallKit ck;
    if (const int rc = ck.open(device)) return rc;
    return unit_result(assoc_radius_candidates(ck.kit.stream, device, n_exist, exist_xyz, n_new, new_xyz, max_dist, cand_ptr, cand_idx, cap, total),
                       "merge_candidates", "problem too large for 32-bit indices");
}

// ---- feature match matrix (SfM::createFeatureMatchMatrix) ---------------------------------------------------------
int sfmba_match_features(int device, int n_images, const int64_t* img_ptr, const unsigned char* desc, int desc_bytes, int n_pairs,
                         const int32_t* pair_left, const int32_t* pair_right, double ratio, int64_t* pair_ptr, int32_t* query_idx,
                         int32_t* train_idx, float* distance, int64_t cap, int64_t* total) {
    if (n_images < 0 || n_pairs < 0 || cap < 0 || !img_ptr || !pair_ptr || !total || (n_pairs > 0 && (!pair_left || !pair_right)) ||
        (cap > 0 && (!query_idx || !train_idx)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (desc_bytes < 1 || desc_bytes > 64) return fail(SFMBA_ERR_INVALID_ARG, "desc_bytes must be in 1..64");
    if (!std::isfinite(ratio) || !(ratio > 0.0)) return fail(SFMBA_ERR_INVALID_ARG, "ratio must be finite and > 0");
    if (const int rc = check_desc_rows("match_features", n_images, img_ptr, desc, n_pairs, pair_left, pair_right)) return rc;
    if (too_many_rows(n_images, img_ptr))
        return fail(SFMBA_ERR_INVALID_ARG, "an image has 2^22 or more descriptor rows (the train index is packed in 22 bits)");
    TimedCall<5> c("SFMBA_MATCH_TIMING");          // (tools/match_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = match_features(c.kit.stream, device, n_images, img_ptr, desc, desc_bytes, n_pairs, pair_left, pair_right, ratio, pair_ptr, query_idx,
                                  train_idx, distance, cap, total, c.tm());
    if (rc == 0 && c.on)
        std::fprintf(stderr, "[sfmba match] upload_ms %.6f top2_ms %.6f compact_ms %.6f download_ms %.6f batches %d\n", c.t[0], c.t[1], c.t[2], c.t[3],
                     (int)c.t[4]);
    return unit_result(rc, "match_features");
}
// ---- the same for float descriptors: exact L2 2-NN (cv::BFMatcher with NORM_L2) ---------------------------------------------
int sfmba_match_features_l2(int device, int n_images, const int64_t* img_ptr, const float* desc, int dims, int n_pairs,
                            const int32_t* pair_left, const int32_t* pair_right, double ratio, int64_t* pair_ptr, int32_t* query_idx,
                            int32_t* train_idx, float* distance, int64_t cap, int64_t* total) {
    if (n_images < 0 || n_pairs < 0 || cap < 0 || !img_ptr || !pair_ptr || !total || (n_pairs > 0 && (!pair_left || !pair_right)) ||
        (cap > 0 && (!query_idx || !train_idx)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (dims < 1 || dims > MATCH_L2_MAX_DIMS) return fail(SFMBA_ERR_INVALID_ARG, "dims must be in 1..512");
    if (!std::isfinite(ratio) || !(ratio > 0.0)) return fail(SFMBA_ERR_INVALID_ARG, "ratio must be finite and > 0");
    if (const int rc = check_desc_rows("match_features_l2", n_images, img_ptr, desc, n_pairs, pair_left, pair_right)) return rc;
    if (too_many_rows(n_images, img_ptr)) return fail(SFMBA_ERR_INVALID_ARG, "an image has 2^22 or more descriptor rows");
    for (int i = 0; i < n_images; ++i)                      // the contract is stated for finite values only
        for (int64_t r = img_ptr[i]; r < img_ptr[i + 1]; ++r) {
            const float* row = desc + (size_t)r * (size_t)dims;
            for (int k = 0; k < dims; ++k)
                if (!std::isfinite(row[k]))
                    return fail(SFMBA_ERR_INVALID_ARG, "match_features_l2: non-finite descriptor value in image " + std::to_string(i) + ", row " +
                                                           std::to_string((long long)(r - img_ptr[i])));
        }
    TimedCall<5> c("SFMBA_MATCH_TIMING");          // (tools/match_l2_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = match_features_l2(c.kit.stream, device, n_images, img_ptr, desc, dims, n_pairs, pair_left, pair_right, ratio, pair_ptr, query_idx,
                                     train_idx, distance, cap, total, c.tm());
    if (rc == 0 && c.on)
        std::fprintf(stderr, "[sfmba match_l2] upload_ms %.6f top2_ms %.6f compact_ms %.6f download_ms %.6f batches %d\n", c.t[0], c.t[1], c.t[2], c.t[3],
                     (int)c.t[4]);
    return unit_result(rc, "match_features_l2");
}
// ---- feature extraction (SfM::extractFeatures) ------------------------------------------------------------------------
int sfmba_orb_extract(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                      int channels, int n_features, float scale_factor, int n_levels, int fast_threshold, int64_t* kp_ptr, sfmba_orb_keypoint* kp,
                      unsigned char* desc, int64_t cap, int64_t* total, int32_t* dbg_level_xy, int32_t* dbg_bin, int64_t* dbg_harris,
                      int32_t* dbg_candidates) {
    if (n_images < 0 || cap < 0 || !img_ptr || !kp_ptr || !total || (n_images > 0 && (!width || !height)) || (cap > 0 && (!kp || !desc)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (const int rc = check_images("orb_extract", n_images, img_ptr, pixels, width, height, channels)) return rc;
    if (n_features < 1) return fail(SFMBA_ERR_INVALID_ARG, "orb_extract: n_features must be >= 1");
    if (n_levels < 1 || n_levels > 12) return fail(SFMBA_ERR_INVALID_ARG, "orb_extract: n_levels must be in 1..12");
    if (!std::isfinite(scale_factor) || !(scale_factor > 1.0f) || scale_factor > 2.0f)
        return fail(SFMBA_ERR_INVALID_ARG, "orb_extract: scale_factor must be finite and in (1, 2]");
    if (fast_threshold < 1 || fast_threshold > 254) return fail(SFMBA_ERR_INVALID_ARG, "orb_extract: fast_threshold must be in 1..254");
    TimedCall<ORB_T_COUNT> c("SFMBA_ORB_TIMING");          // (tools/orb_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = orb_extract(c.kit.stream, device, n_images, img_ptr, pixels, width, height, channels, n_features, scale_factor, n_levels,
                               fast_threshold, kp_ptr, kp, desc, cap, total, dbg_level_xy, dbg_bin, dbg_harris, dbg_candidates, c.tm());
    if (rc == 0 && c.on)
        std::fprintf(stderr, "[sfmba orb] upload_ms %.6f pyramid_ms %.6f score_ms %.6f candidates_ms %.6f response_ms %.6f select_ms %.6f smooth_ms %.6f "
                     "describe_ms %.6f download_ms %.6f groups %d\n", c.t[ORB_T_UPLOAD], c.t[ORB_T_PYRAMID], c.t[ORB_T_SCORE], c.t[ORB_T_CANDIDATES],
                     c.t[ORB_T_HARRIS], c.t[ORB_T_SELECT], c.t[ORB_T_SMOOTH], c.t[ORB_T_DESCRIBE], c.t[ORB_T_DOWNLOAD], (int)c.t[ORB_T_GROUPS]);
    return unit_result(rc, "orb_extract");
}
// ---- float descriptors: Fast-Hessian detect and SURF-style describe, the extractor in front of sfmba_match_features_l2 ---------
int sfmba_surf_extract(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                       int channels, int n_features, int n_octaves, float hessian_threshold, int upright, int64_t* kp_ptr, sfmba_surf_keypoint* kp,
                       float* desc, int64_t cap, int64_t* total, int32_t* dbg_bin, int64_t* dbg_moments, int64_t* dbg_sums, int32_t* dbg_candidates) {
    if (n_images < 0 || cap < 0 || !img_ptr || !kp_ptr || !total || (n_images > 0 && (!width || !height)) || (cap > 0 && (!kp || !desc)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (const int rc = check_images("surf_extract", n_images, img_ptr, pixels, width, height, channels)) return rc;
    if (n_features < 1) return fail(SFMBA_ERR_INVALID_ARG, "surf_extract: n_features must be >= 1");
    if (n_octaves < 1 || n_octaves > 4) return fail(SFMBA_ERR_INVALID_ARG, "surf_extract: n_octaves must be in 1..4");
    if (!std::isfinite(hessian_threshold) || hessian_threshold < 0.0f)
        return fail(SFMBA_ERR_INVALID_ARG, "surf_extract: hessian_threshold must be finite and >= 0");
    if (upright != 0 && upright != 1) return fail(SFMBA_ERR_INVALID_ARG, "surf_extract: upright must be 0 or 1");
    TimedCall<SURF_T_COUNT> c("SFMBA_SURF_TIMING");          // (tools/surf_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = surf_extract(c.kit.stream, device, n_images, img_ptr, pixels, width, height, channels, n_features, n_octaves, hessian_threshold,
                                upright, kp_ptr, kp, desc, cap, total, dbg_bin, dbg_moments, dbg_sums, dbg_candidates, c.tm());
    if (rc == 0 && c.on)
        std::fprintf(stderr, "[sfmba surf] upload_ms %.6f integral_ms %.6f response_ms %.6f candidates_ms %.6f select_ms %.6f describe_ms %.6f "
                     "download_ms %.6f groups %d response_bytes %.0f\n", c.t[SURF_T_UPLOAD], c.t[SURF_T_INTEGRAL], c.t[SURF_T_RESPONSE],
                     c.t[SURF_T_CANDIDATES], c.t[SURF_T_SELECT], c.t[SURF_T_DESCRIBE], c.t[SURF_T_DOWNLOAD], (int)c.t[SURF_T_GROUPS],
                     c.t[SURF_T_RESPONSE_BYTES]);
    return unit_result(rc, "surf_extract");
}
// ---- dense depth maps and a dense cloud: plane-sweep stereo and the consistency filter (SfM::densify) ---------------------------
namespace {
// what sfmba_depth_sweep and the two calls that store its cost volume refuse about the images, the cameras, the jobs and the shared
// parameters; *out_px receives the pixels of all reference images
int depth_check_sweep(const char* who, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                      int channels, const float* K, const float* P, int n_jobs, const int32_t* job_ref, const int64_t* job_src_ptr,
                      const int32_t* job_src, const float* z_near, const float* z_far, int n_planes, int radius, int min_std,
                      const float* min_score /*NULL: the call has none*/, int min_sources, int64_t* out_px) {
    const std::string w(who);
    if (n_jobs < 0 || (n_jobs > 0 && (!job_ref || !job_src_ptr || !job_src || !z_near || !z_far))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (const int rc = depth_check_images(who, n_images, img_ptr, pixels, width, height, channels, K, P)) return rc;
    if (n_planes < 2 || n_planes > 256) return fail(SFMBA_ERR_INVALID_ARG, w + ": n_planes must be in 2..256");
    if (radius < 1 || radius > 4) return fail(SFMBA_ERR_INVALID_ARG, w + ": radius must be in 1..4");
    if (min_std < 0 || min_std > 127) return fail(SFMBA_ERR_INVALID_ARG, w + ": min_std must be in 0..127");
    if (min_score && (!(*min_score >= -1.0f) || !(*min_score <= 1.0f))) return fail(SFMBA_ERR_INVALID_ARG, w + ": min_score must be in [-1, 1]");
    if (min_sources < 1 || min_sources > 4) return fail(SFMBA_ERR_INVALID_ARG, w + ": min_sources must be in 1..4");
    *out_px = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (job_ref[j] < 0 || job_ref[j] >= n_images) return fail(SFMBA_ERR_INVALID_ARG, w + ": reference image index out of range");
        if (!std::isfinite(z_near[j]) || !std::isfinite(z_far[j]) || !(z_near[j] > 0.0f) || !(z_near[j] < z_far[j]))
            return fail(SFMBA_ERR_INVALID_ARG, w + ": a job needs 0 < z_near < z_far, both finite");
        *out_px += (int64_t)width[job_ref[j]] * height[job_ref[j]];
    }
    if (n_jobs > 0)
        if (const int rc = depth_check_lists(who, "source", n_images, n_jobs, job_ref, job_src_ptr, job_src, 1)) return rc;
    return 0;
}
int sgm_check_params(const char* who, int p1, int p2, int n_paths, int invalid_cost) {
    const std::string w(who);
    if (p1 < 0 || p2 < p1 || p2 > SGM_MAX_PENALTY) return fail(SFMBA_ERR_INVALID_ARG, w + ": the penalties must satisfy 0 <= p1 <= p2 <= 1023");
    if (n_paths != 4 && n_paths != 8) return fail(SFMBA_ERR_INVALID_ARG, w + ": n_paths must be 4 or 8");
    if (invalid_cost < 0 || invalid_cost > SGM_MAX_COST) return fail(SFMBA_ERR_INVALID_ARG, w + ": invalid_cost must be in 0..254");
    return 0;
}
void sweep_timing_line(const char* what, const double* t) {
    std::fprintf(stderr, "[sfmba %s] upload_ms %.6f gray_ms %.6f sweep_ms %.6f download_ms %.6f groups %d\n", what, t[DEPTH_T_UPLOAD], t[DEPTH_T_GRAY],
                 t[DEPTH_T_SWEEP], t[DEPTH_T_DOWNLOAD], (int)t[DEPTH_T_GROUPS]);
}
void sgm_timing_line(const char* what, const double* t) {
    std::fprintf(stderr, "[sfmba %s] aggregate_ms %.6f select_ms %.6f finish_ms %.6f path_ms", what, t[SGM_T_AGGREGATE], t[SGM_T_SELECT], t[SGM_T_FINISH]);
    for (int i = 0; i < 8; ++i) std::fprintf(stderr, " %.6f", t[SGM_T_PATH0 + i]);
    std::fprintf(stderr, "\n");
}
}  // namespace
int sfmba_depth_sweep(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                      int channels, const float* K, const float* P, int n_jobs, const int32_t* job_ref, const int64_t* job_src_ptr,
                      const int32_t* job_src, const float* z_near, const float* z_far, int n_planes, int radius, int min_std, float min_score,
                      int min_sources, float* depth, float* score, int16_t* plane) {
    int64_t out_px = 0;
    if (const int rc = depth_check_sweep("depth_sweep", n_images, img_ptr, pixels, width, height, channels, K, P, n_jobs, job_ref, job_src_ptr, job_src,
                                         z_near, z_far, n_planes, radius, min_std, &min_score, min_sources, &out_px))
        return rc;
    if (out_px > 0 && (!depth || !score)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (n_jobs == 0) return check_device(device);
    TimedCall<DEPTH_T_COUNT> c("SFMBA_DEPTH_TIMING");          // (tools/dense_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = depth_sweep(c.kit.stream, device, n_images, img_ptr, pixels, width, height, channels, K, P, n_jobs, job_ref, job_src_ptr, job_src,
                               z_near, z_far, n_planes, radius, min_std, min_score, min_sources, depth, score, plane, c.tm());
    if (rc == 0 && c.on) sweep_timing_line("depth_sweep", c.t);
    return unit_result(rc, "depth_sweep");
}
// ---- semi-global matching over the sweep's cost volume (DenseParams::sgm) -----------------------------------------------------------
int sfmba_depth_cost_volume(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width,
                            const int32_t* height, int channels, const float* K, const float* P, int n_jobs, const int32_t* job_ref,
                            const int64_t* job_src_ptr, const int32_t* job_src, const float* z_near, const float* z_far, int n_planes, int radius,
                            int min_std, int min_sources, int invalid_cost, unsigned char* cost) {
    int64_t out_px = 0;
    if (const int rc = depth_check_sweep("depth_cost_volume", n_images, img_ptr, pixels, width, height, channels, K, P, n_jobs, job_ref, job_src_ptr,
                                         job_src, z_near, z_far, n_planes, radius, min_std, nullptr, min_sources, &out_px))
        return rc;
    if (invalid_cost < 0 || invalid_cost > SGM_MAX_COST) return fail(SFMBA_ERR_INVALID_ARG, "depth_cost_volume: invalid_cost must be in 0..254");
    if (out_px > 0 && !cost) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (n_jobs == 0) return check_device(device);
    TimedCall<DEPTH_T_COUNT> c("SFMBA_DEPTH_TIMING");          // (tools/sgm_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = depth_cost_volume(c.kit.stream, device, n_images, img_ptr, pixels, width, height, channels, K, P, n_jobs, job_ref, job_src_ptr,
                                     job_src, z_near, z_far, n_planes, radius, min_std, min_sources, cost, c.tm());
    if (rc == 0 && c.on) sweep_timing_line("depth_cost_volume", c.t);
    return unit_result(rc, "depth_cost_volume");
}
int sfmba_sgm_aggregate(int device, int n_jobs, const unsigned char* const* cost, const int32_t* width, const int32_t* height, int n_planes, int p1,
                        int p2, int n_paths, int invalid_cost, int16_t* const* plane, uint16_t* const* best, uint16_t* const* second,
                        uint16_t* const* sums) {
    if (n_jobs < 0 || (n_jobs > 0 && (!cost || !width || !height || !plane || !best || !second))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (n_planes < 2 || n_planes > 256) return fail(SFMBA_ERR_INVALID_ARG, "sgm_aggregate: n_planes must be in 2..256");
    if (const int rc = sgm_check_params("sgm_aggregate", p1, p2, n_paths, invalid_cost)) return rc;
    for (int j = 0; j < n_jobs; ++j) {
        if (width[j] < 1 || width[j] > 16384 || height[j] < 1 || height[j] > 16384)
            return fail(SFMBA_ERR_INVALID_ARG, "sgm_aggregate: a volume's width or height lies outside 1..16384");
        if (!cost[j] || !plane[j] || !best[j] || !second[j]) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    }
    if (n_jobs == 0) return check_device(device);
    TimedCall<SGM_T_COUNT> c("SFMBA_DEPTH_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = sgm_aggregate(c.kit.stream, device, n_jobs, cost, width, height, n_planes, p1, p2, n_paths, invalid_cost, plane, best, second, sums,
                                 c.tm());
    if (rc == 0 && c.on) sgm_timing_line("sgm_aggregate", c.t);
    return unit_result(rc, "sgm_aggregate");
}
int sfmba_depth_sweep_sgm(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                          int channels, const float* K, const float* P, int n_jobs, const int32_t* job_ref, const int64_t* job_src_ptr,
                          const int32_t* job_src, const float* z_near, const float* z_far, int n_planes, int radius, int min_std, int min_sources,
                          int p1, int p2, int n_paths, int invalid_cost, int uniqueness, float* depth, float* score, int16_t* plane) {
    int64_t out_px = 0;
    if (const int rc = depth_check_sweep("depth_sweep_sgm", n_images, img_ptr, pixels, width, height, channels, K, P, n_jobs, job_ref, job_src_ptr,
                                         job_src, z_near, z_far, n_planes, radius, min_std, nullptr, min_sources, &out_px))
        return rc;
    if (const int rc = sgm_check_params("depth_sweep_sgm", p1, p2, n_paths, invalid_cost)) return rc;
    if (uniqueness < 0 || uniqueness > 100) return fail(SFMBA_ERR_INVALID_ARG, "depth_sweep_sgm: uniqueness must be in 0..100");
    if (out_px > 0 && (!depth || !score)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (n_jobs == 0) return check_device(device);
    TimedCall<DEPTH_T_COUNT> c("SFMBA_DEPTH_TIMING");
    if (const int rc = c.open(device)) return rc;
    double sgm_t[SGM_T_COUNT];
    const int rc = depth_sweep_sgm(c.kit.stream, device, n_images, img_ptr, pixels, width, height, channels, K, P, n_jobs, job_ref, job_src_ptr, job_src,
                                   z_near, z_far, n_planes, radius, min_std, min_sources, p1, p2, n_paths, invalid_cost, uniqueness, depth, score, plane,
                                   c.tm(), c.on ? sgm_t : nullptr);
    if (rc == 0 && c.on) {
        sweep_timing_line("depth_sweep_sgm", c.t);
        sgm_timing_line("depth_sweep_sgm", sgm_t);
    }
    return unit_result(rc, "depth_sweep_sgm");
}
int sfmba_depth_fuse(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                     int channels, const float* K, const float* P, const float* const* depth, const int64_t* chk_ptr, const int32_t* chk,
                     float rel_tol, int min_consistent, int64_t* pt_ptr, float* xyz, unsigned char* bgr, int32_t* src_image, int32_t* src_pixel,
                     int64_t cap, int64_t* total) {
    if (cap < 0 || !pt_ptr || !total || (n_images > 0 && !depth) || (cap > 0 && (!xyz || !bgr || !src_image || !src_pixel)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (const int rc = depth_check_images("depth_fuse", n_images, img_ptr, pixels, width, height, channels, K, P)) return rc;
    if (n_images > 65535) return fail(SFMBA_ERR_INVALID_ARG, "depth_fuse: more than 65535 images in one call");
    if (!std::isfinite(rel_tol) || rel_tol < 0.0f) return fail(SFMBA_ERR_INVALID_ARG, "depth_fuse: rel_tol must be finite and >= 0");
    if (min_consistent < 0 || min_consistent > 4) return fail(SFMBA_ERR_INVALID_ARG, "depth_fuse: min_consistent must be in 0..4");
    if (const int rc = depth_check_lists("depth_fuse", "check", n_images, n_images, nullptr, chk_ptr, chk, 0)) return rc;
    int64_t px = 0;
    for (int i = 0; i < n_images; ++i)
        if (depth[i]) px += (int64_t)width[i] * height[i];
    if (px >= (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "depth_fuse: too many pixels with a depth map in one call (2^31)");
    if (px == 0) {
        for (int i = 0; i <= n_images; ++i) pt_ptr[i] = 0;
        *total = 0;
        return check_device(device);
    }
    TimedCall<FUSE_T_COUNT> c("SFMBA_DEPTH_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = depth_fuse(c.kit.stream, device, n_images, img_ptr, pixels, width, height, channels, K, P, depth, chk_ptr, chk, rel_tol, min_consistent,
                              pt_ptr, xyz, bgr, src_image, src_pixel, cap, total, c.tm());
    if (rc == 0 && c.on)
        std::fprintf(stderr, "[sfmba depth_fuse] upload_ms %.6f flag_ms %.6f scan_ms %.6f emit_ms %.6f download_ms %.6f\n", c.t[FUSE_T_UPLOAD],
                     c.t[FUSE_T_FLAG], c.t[FUSE_T_SCAN], c.t[FUSE_T_EMIT], c.t[FUSE_T_DOWNLOAD]);
    return unit_result(rc, "depth_fuse");
}
// ---- matching by optical flow: pyramidal Lucas-Kanade and the snap to key points (SfMFeatureMatching::createFlowMatchMatrix) -----
int sfmba_flow_track(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                     int channels, int n_pairs, const int32_t* pair_src, const int32_t* pair_dst, const int64_t* pt_ptr, const float* pts,
                     int n_levels, int radius, int max_iters, float min_eig, float* next, unsigned char* status, float* err, int64_t* dbg_G,
                     int32_t* dbg_state, unsigned char* dbg_pyramid) {
    if (n_images < 0 || !img_ptr || (n_images > 0 && (!width || !height)) || (n_pairs > 0 && !pair_src))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (const int rc = check_images("flow_track", n_images, img_ptr, pixels, width, height, channels)) return rc;
    if (n_levels < 1 || n_levels > FLOW_MAX_LEVELS) return fail(SFMBA_ERR_INVALID_ARG, "flow_track: n_levels must be in 1..8");
    if (radius < 1 || radius > FLOW_MAX_RADIUS) return fail(SFMBA_ERR_INVALID_ARG, "flow_track: radius must be in 1..10");
    if (max_iters < 1 || max_iters > FLOW_MAX_ITERS) return fail(SFMBA_ERR_INVALID_ARG, "flow_track: max_iters must be in 1..64");
    if (!std::isfinite(min_eig) || min_eig < 0.0f) return fail(SFMBA_ERR_INVALID_ARG, "flow_track: min_eig must be finite and >= 0");
    if (const int rc = flow_check_pairs("flow_track", n_images, n_pairs, pair_src, pair_dst, pt_ptr)) return rc;
    const int64_t n_pts = pt_ptr[n_pairs];
    if (n_pts > 0 && (!pts || !next || !status || !err)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    for (int64_t q = 0; q < 2 * n_pts; ++q)
        if (!std::isfinite(pts[q])) return fail(SFMBA_ERR_INVALID_ARG, "flow_track: non-finite coordinate of point " + std::to_string((long long)(q / 2)));
    if (n_pairs == 0) return check_device(device);
    TimedCall<FLOW_T_COUNT> c("SFMBA_FLOW_TIMING");          // (tools/flow_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = flow_track(c.kit.stream, device, n_images, img_ptr, pixels, width, height, channels, n_pairs, pair_src, pair_dst, pt_ptr, pts, n_levels,
                              radius, max_iters, min_eig, next, status, err, dbg_G, dbg_state, dbg_pyramid, c.tm());
    if (rc == 0 && c.on)
        std::fprintf(stderr, "[sfmba flow_track] upload_ms %.6f gray_ms %.6f pyramid_ms %.6f track_ms %.6f download_ms %.6f groups %d\n",
                     c.t[FLOW_T_UPLOAD], c.t[FLOW_T_GRAY], c.t[FLOW_T_PYRAMID], c.t[FLOW_T_TRACK], c.t[FLOW_T_DOWNLOAD], (int)c.t[FLOW_T_GROUPS]);
    return unit_result(rc, "flow_track");
}
int sfmba_flow_match(int device, int n_images, const int64_t* kp_ptr, const float* kp_xy, int n_pairs, const int32_t* pair_dst,
                     const int64_t* pt_ptr, const float* next, const unsigned char* status, const float* err, float max_err, float radius,
                     double ratio, int64_t* pair_ptr, int32_t* query_idx, int32_t* train_idx, float* distance, int64_t cap, int64_t* total) {
    if (cap < 0 || !kp_ptr || !pair_ptr || !total || (cap > 0 && (!query_idx || !train_idx))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (!std::isfinite(max_err)) return fail(SFMBA_ERR_INVALID_ARG, "flow_match: max_err must be finite");
    if (!std::isfinite(radius) || !(radius > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "flow_match: radius must be finite and > 0");
    if (!std::isfinite(ratio) || !(ratio > 0.0)) return fail(SFMBA_ERR_INVALID_ARG, "flow_match: ratio must be finite and > 0");
    if (const int rc = flow_check_pairs("flow_match", n_images, n_pairs, nullptr, pair_dst, pt_ptr)) return rc;
    if (kp_ptr[0] != 0) return fail(SFMBA_ERR_INVALID_ARG, "flow_match: kp_ptr must start at 0");
    for (int i = 0; i < n_images; ++i) {
        const int64_t n = kp_ptr[i + 1] - kp_ptr[i];
        if (n < 0) return fail(SFMBA_ERR_INVALID_ARG, "flow_match: kp_ptr not monotone");
        if (n >= ((int64_t)1 << 22)) return fail(SFMBA_ERR_INVALID_ARG, "flow_match: an image has 2^22 or more key points");
    }
    const int64_t n_pts = pt_ptr[n_pairs];
    if ((n_pts > 0 && (!next || !status || !err)) || (kp_ptr[n_images] > 0 && !kp_xy)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (n_pts == 0) {
        for (int p = 0; p <= n_pairs; ++p) pair_ptr[p] = 0;
        *total = 0;
        return check_device(device);
    }
    TimedCall<FLOWM_T_COUNT> c("SFMBA_FLOW_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = flow_match(c.kit.stream, device, n_images, kp_ptr, kp_xy, n_pairs, pair_dst, pt_ptr, next, status, err, max_err, radius, ratio, pair_ptr,
                              query_idx, train_idx, distance, cap, total, c.tm());
    if (rc == 0 && c.on)
        std::fprintf(stderr, "[sfmba flow_match] upload_ms %.6f near_ms %.6f compact_ms %.6f download_ms %.6f\n", c.t[FLOWM_T_UPLOAD], c.t[FLOWM_T_NEAR],
                     c.t[FLOWM_T_COMPACT], c.t[FLOWM_T_DOWNLOAD]);
    return unit_result(rc, "flow_match");
}
// ---- one oriented point per surface element: a normal per depth pixel and the voxel merge (SfM::mergeDenseCloud) ------------------
int sfmba_depth_normals(int device, int n_images, const int32_t* width, const int32_t* height, const float* K, const float* P,
                        const float* const* depth, float max_rel_step, float* const* normal) {
    if ((n_images > 0 && (!depth || !normal))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (const int rc = depth_check_cameras("depth_normals", n_images, width, height, K, P)) return rc;
    if (n_images > 65535) return fail(SFMBA_ERR_INVALID_ARG, "depth_normals: more than 65535 images in one call");
    if (!std::isfinite(max_rel_step) || max_rel_step < 0.0f) return fail(SFMBA_ERR_INVALID_ARG, "depth_normals: max_rel_step must be finite and >= 0");
    int64_t px = 0;
    for (int i = 0; i < n_images; ++i) {
        if (!depth[i]) continue;
        if (!normal[i]) return fail(SFMBA_ERR_INVALID_ARG, "depth_normals: an image with a depth map needs an output map");
        px += (int64_t)width[i] * height[i];
    }
    if (px >= (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "depth_normals: too many pixels with a depth map in one call (2^31)");
    if (px == 0) return check_device(device);
    TimedCall<NORMALS_T_COUNT> c("SFMBA_CLOUD_TIMING");          // (tools/cloud_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = depth_normals(c.kit.stream, device, n_images, width, height, K, P, depth, max_rel_step, normal, c.tm());
    if (rc == 0 && c.on)
        std::fprintf(stderr, "[sfmba depth_normals] upload_ms %.6f kernel_ms %.6f download_ms %.6f\n", c.t[NORMALS_T_UPLOAD], c.t[NORMALS_T_KERNEL],
                     c.t[NORMALS_T_DOWNLOAD]);
    return unit_result(rc, "depth_normals");
}
int sfmba_cloud_merge(int device, int64_t n, const float* xyz, const unsigned char* bgr, const float* normal, float voxel, int min_count,
                      float* xyz_out, unsigned char* bgr_out, float* normal_out, int32_t* count, int32_t* first, int32_t* voxel_of, int64_t cap,
                      int64_t* total, int64_t* n_skipped) {
    if (n < 0 || cap < 0 || !total || !n_skipped || (n > 0 && !xyz) ||
        (cap > 0 && (!xyz_out || !count || !first || (bgr && !bgr_out) || (normal && !normal_out))))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (n >= (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "cloud_merge: too many points in one call (2^31)");
    if (!std::isfinite(voxel) || !(voxel > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "cloud_merge: voxel must be finite and > 0");
    if (min_count < 1) return fail(SFMBA_ERR_INVALID_ARG, "cloud_merge: min_count must be >= 1");
    if (n == 0) {
        *total = 0;
        *n_skipped = 0;
        return check_device(device);
    }
    TimedCall<MERGE_T_COUNT> c("SFMBA_CLOUD_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = cloud_merge(c.kit.stream, device, (int)n, xyz, bgr, normal, voxel, min_count, xyz_out, bgr_out, normal_out, count, first, voxel_of, cap,
                               total, n_skipped, c.tm());
    if ((rc == 0 || rc == UNIT_ERR_CAPACITY) && c.on)          // (a capacity failure has run every phase but the download)
        std::fprintf(stderr,
                     "[sfmba cloud_merge] upload_ms %.6f quantise_ms %.6f sort_ms %.6f runs_ms %.6f reduce_ms %.6f compact_ms %.6f finalise_ms %.6f "
                     "download_ms %.6f points %lld voxels %lld\n",
                     c.t[MERGE_T_UPLOAD], c.t[MERGE_T_QUANTISE], c.t[MERGE_T_SORT], c.t[MERGE_T_RUNS], c.t[MERGE_T_REDUCE], c.t[MERGE_T_COMPACT],
                     c.t[MERGE_T_FINALISE], c.t[MERGE_T_DOWNLOAD], (long long)n, (long long)*total);
    return unit_result(rc, "cloud_merge");
}
// ---- a surface from the depth maps: TSDF fusion and marching tetrahedra (SfM::meshDenseCloud) -------------------------------------
int sfmba_tsdf_integrate(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                         int channels, const float* K, const float* P, const float* const* depth, const float* origin, float voxel, int nx, int ny,
                         int nz, float trunc, int32_t* sum, int32_t* weight, int32_t* csum, int32_t* cweight) {
    if (!sum || !weight || (csum == nullptr) != (cweight == nullptr)) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    const TsdfViews views{ n_images, img_ptr, pixels, width, height, channels, K, P, depth, trunc };
    const TsdfGrid grid{ origin, voxel, nx, ny, nz };
    if (const int rc = tsdf_check_views("tsdf_integrate", views)) return rc;
    if (const int rc = tsdf_check_grid("tsdf_integrate", origin, voxel, nx, ny, nz)) return rc;
    TimedCall<TSDF_T_COUNT> c("SFMBA_MESH_TIMING");          // (tools/mesh_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = tsdf_integrate(c.kit.stream, device, views, grid, sum, weight, csum, cweight, c.tm());
    if (rc == 0 && c.on) tsdf_timing_line("tsdf_integrate", c.t, grid, 0, 0);
    return tsdf_result(rc, "tsdf_integrate");
}
int sfmba_tsdf_extract(int device, const float* origin, float voxel, int nx, int ny, int nz, const int32_t* sum, const int32_t* weight,
                       const int32_t* csum, const int32_t* cweight, int min_weight, float* xyz, unsigned char* bgr, int32_t* vkey, int64_t vcap,
                       int32_t* tri, int64_t tcap, int64_t* n_vertices, int64_t* n_triangles) {
    if (!sum || !weight || (csum == nullptr) != (cweight == nullptr)) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    const TsdfGrid grid{ origin, voxel, nx, ny, nz };
    const TsdfMeshOut out{ xyz, bgr, vkey, vcap, tri, tcap, n_vertices, n_triangles };
    if (const int rc = tsdf_check_out("tsdf_extract", min_weight, csum != nullptr, out)) return rc;
    if (const int rc = tsdf_check_grid("tsdf_extract", origin, voxel, nx, ny, nz)) return rc;
    TimedCall<TSDF_T_COUNT> c("SFMBA_MESH_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = tsdf_extract(c.kit.stream, device, grid, sum, weight, csum, cweight, min_weight, out, c.tm());
    if ((rc == 0 || rc == UNIT_ERR_CAPACITY) && c.on) tsdf_timing_line("tsdf_extract", c.t, grid, (long long)*n_vertices, (long long)*n_triangles);
    return tsdf_result(rc, "tsdf_extract");
}
int sfmba_tsdf_mesh(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                    int channels, const float* K, const float* P, const float* const* depth, const float* origin, float voxel, int nx, int ny, int nz,
                    float trunc, int min_weight, float* xyz, unsigned char* bgr, int32_t* vkey, int64_t vcap, int32_t* tri, int64_t tcap,
                    int64_t* n_vertices, int64_t* n_triangles) {
    const TsdfViews views{ n_images, img_ptr, pixels, width, height, channels, K, P, depth, trunc };
    const TsdfGrid grid{ origin, voxel, nx, ny, nz };
    const TsdfMeshOut out{ xyz, bgr, vkey, vcap, tri, tcap, n_vertices, n_triangles };
    if (const int rc = tsdf_check_out("tsdf_mesh", min_weight, pixels != nullptr, out)) return rc;
    if (const int rc = tsdf_check_views("tsdf_mesh", views)) return rc;
    if (const int rc = tsdf_check_grid("tsdf_mesh", origin, voxel, nx, ny, nz)) return rc;
    TimedCall<TSDF_T_COUNT> c("SFMBA_MESH_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = tsdf_mesh(c.kit.stream, device, views, grid, min_weight, out, c.tm());
    if ((rc == 0 || rc == UNIT_ERR_CAPACITY) && c.on) tsdf_timing_line("tsdf_mesh", c.t, grid, (long long)*n_vertices, (long long)*n_triangles);
    return tsdf_result(rc, "tsdf_mesh");
}
// ---- filling the holes of the surface: volumetric diffusion of the TSDF grid (MeshParams::fillIterations) -------------------------
int sfmba_tsdf_fill(int device, int nx, int ny, int nz, const int32_t* sum, const int32_t* weight, const int32_t* csum, const int32_t* cweight,
                    int min_weight, int iterations, int min_neighbours, int32_t* sum_out, int32_t* weight_out, int32_t* csum_out, int32_t* cweight_out,
                    unsigned char* state, int64_t* n_filled) {
    if (!sum || !weight || !sum_out || !weight_out || !n_filled || (csum == nullptr) != (cweight == nullptr) || (csum && (!csum_out || !cweight_out)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (const int rc = tsdf_check_min_weight("tsdf_fill", min_weight)) return rc;
    if (const int rc = tsdf_check_fill("tsdf_fill", iterations, min_neighbours)) return rc;
    if (const int rc = tsdf_check_dims("tsdf_fill", nx, ny, nz)) return rc;
    const TsdfFillParams prm{ min_weight, iterations, min_neighbours };
    const TsdfGrid grid{ nullptr, 0.0f, nx, ny, nz };
    TimedCall<TSDF_T_COUNT> c("SFMBA_MESH_TIMING");          // (tools/tsdf_fill_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = tsdf_fill(c.kit.stream, device, nx, ny, nz, sum, weight, csum, cweight, prm, sum_out, weight_out, csum_out, cweight_out, state,
                             n_filled, c.tm());
    if (rc == 0 && c.on) tsdf_fill_timing_line("tsdf_fill", c.t, grid, iterations, (long long)*n_filled, 0, 0);
    return tsdf_result(rc, "tsdf_fill");
}
int sfmba_tsdf_mesh_fill(int device, int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                         int channels, const float* K, const float* P, const float* const* depth, const float* origin, float voxel, int nx, int ny,
                         int nz, float trunc, int min_weight, int fill_iterations, int min_neighbours, float* xyz, unsigned char* bgr, int32_t* vkey,
                         unsigned char* vfilled, int64_t vcap, int32_t* tri, int64_t tcap, int64_t* n_vertices, int64_t* n_triangles) {
    const TsdfViews views{ n_images, img_ptr, pixels, width, height, channels, K, P, depth, trunc };
    const TsdfGrid grid{ origin, voxel, nx, ny, nz };
    const TsdfMeshOut out{ xyz, bgr, vkey, vcap, tri, tcap, n_vertices, n_triangles, vfilled };
    if (const int rc = tsdf_check_out("tsdf_mesh_fill", min_weight, pixels != nullptr, out)) return rc;
    if (const int rc = tsdf_check_fill("tsdf_mesh_fill", fill_iterations, min_neighbours)) return rc;
    if (const int rc = tsdf_check_views("tsdf_mesh_fill", views)) return rc;
    if (const int rc = tsdf_check_grid("tsdf_mesh_fill", origin, voxel, nx, ny, nz)) return rc;
    const TsdfFillParams prm{ min_weight, fill_iterations, min_neighbours };
    TimedCall<TSDF_T_COUNT> c("SFMBA_MESH_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = tsdf_mesh_fill(c.kit.stream, device, views, grid, prm, out, c.tm());
    if ((rc == 0 || rc == UNIT_ERR_CAPACITY) && c.on)
        tsdf_fill_timing_line("tsdf_mesh_fill", c.t, grid, fill_iterations, -1, (long long)*n_vertices, (long long)*n_triangles);
    return tsdf_result(rc, "tsdf_mesh_fill");
}
// ---- cleaning a mesh: components, small-island removal, Taubin smoothing, vertex normals (SfM::cleanMesh) -------------------------
int sfmba_mesh_components(int device, int64_t n_vertices, int64_t n_triangles, const int32_t* tri, int32_t* label, int32_t* comp_triangles,
                          int64_t* n_components, int64_t* largest) {
    if (const int rc = clean_check_mesh("mesh_components", n_vertices, nullptr, false, n_triangles, tri)) return rc;
    if (!n_components || !largest || (n_vertices > 0 && !label)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    const CleanMesh m{ (int)n_vertices, (int)n_triangles, nullptr, nullptr, tri };
    TimedCall<CLEAN_T_COUNT> c("SFMBA_MESH_CLEAN_TIMING");       // (tools/mesh_clean_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = mesh_components(c.kit.stream, device, m, label, comp_triangles, n_components, largest, c.tm());
    if (rc == 0 && c.on) clean_timing_line("mesh_components", c.t, n_vertices, n_triangles, n_vertices, n_triangles);
    return clean_result(rc, "mesh_components");
}
int sfmba_mesh_filter(int device, int64_t n_vertices, const float* xyz, const unsigned char* bgr, int64_t n_triangles, const int32_t* tri,
                      int min_triangles, int keep_largest, float* xyz_out, unsigned char* bgr_out, int64_t vcap, int32_t* tri_out, int64_t tcap,
                      int32_t* vertex_of, int64_t* n_vertices_out, int64_t* n_triangles_out) {
    if (const int rc = clean_check_mesh("mesh_filter", n_vertices, xyz, true, n_triangles, tri)) return rc;
    const CleanFilterOut out{ xyz_out, bgr_out, nullptr, vcap, tri_out, tcap, vertex_of, n_vertices_out, n_triangles_out };
    if (const int rc = clean_check_out(out, bgr != nullptr)) return rc;
    if (const int rc = clean_check_filter("mesh_filter", min_triangles, keep_largest)) return rc;
    const CleanMesh m{ (int)n_vertices, (int)n_triangles, xyz, bgr, tri };
    const CleanFilterParams f{ min_triangles, keep_largest };
    TimedCall<CLEAN_T_COUNT> c("SFMBA_MESH_CLEAN_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = mesh_filter(c.kit.stream, device, m, f, out, c.tm());
    if ((rc == 0 || rc == UNIT_ERR_CAPACITY) && c.on)
        clean_timing_line("mesh_filter", c.t, n_vertices, n_triangles, (long long)*n_vertices_out, (long long)*n_triangles_out);
    return clean_result(rc, "mesh_filter");
}
int sfmba_mesh_smooth(int device, int64_t n_vertices, const float* xyz, int64_t n_triangles, const int32_t* tri, const float* origin, float quantum,
                      int iterations, float lambda, float mu, float* xyz_out, float* normal) {
    if (const int rc = clean_check_mesh("mesh_smooth", n_vertices, xyz, true, n_triangles, tri)) return rc;
    if (n_vertices > 0 && !xyz_out) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    CleanSmoothParams p;
    if (const int rc = clean_check_smooth("mesh_smooth", origin, quantum, iterations, lambda, mu, p)) return rc;
    const CleanMesh m{ (int)n_vertices, (int)n_triangles, xyz, nullptr, tri };
    TimedCall<CLEAN_T_COUNT> c("SFMBA_MESH_CLEAN_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = mesh_smooth(c.kit.stream, device, m, p, xyz_out, normal, c.tm());
    if (rc == 0 && c.on) clean_timing_line("mesh_smooth", c.t, n_vertices, n_triangles, n_vertices, n_triangles);
    return clean_result(rc, "mesh_smooth");
}
int sfmba_mesh_clean(int device, int64_t n_vertices, const float* xyz, const unsigned char* bgr, int64_t n_triangles, const int32_t* tri,
                     int min_triangles, int keep_largest, const float* origin, float quantum, int iterations, float lambda, float mu, float* xyz_out,
                     unsigned char* bgr_out, float* normal, int64_t vcap, int32_t* tri_out, int64_t tcap, int32_t* vertex_of, int64_t* n_vertices_out,
                     int64_t* n_triangles_out) {
    if (const int rc = clean_check_mesh("mesh_clean", n_vertices, xyz, true, n_triangles, tri)) return rc;
    const CleanFilterOut out{ xyz_out, bgr_out, normal, vcap, tri_out, tcap, vertex_of, n_vertices_out, n_triangles_out };
    if (const int rc = clean_check_out(out, bgr != nullptr)) return rc;
    if (const int rc = clean_check_filter("mesh_clean", min_triangles, keep_largest)) return rc;
    CleanSmoothParams p;
    if (const int rc = clean_check_smooth("mesh_clean", origin, quantum, iterations, lambda, mu, p)) return rc;
    const CleanMesh m{ (int)n_vertices, (int)n_triangles, xyz, bgr, tri };
    const CleanFilterParams f{ min_triangles, keep_largest };
    TimedCall<CLEAN_T_COUNT> c("SFMBA_MESH_CLEAN_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = mesh_clean(c.kit.stream, device, m, f, p, out, c.tm());
    if ((rc == 0 || rc == UNIT_ERR_CAPACITY) && c.on)
        clean_timing_line("mesh_clean", c.t, n_vertices, n_triangles, (long long)*n_vertices_out, (long long)*n_triangles_out);
    return clean_result(rc, "mesh_clean");
}
// ---- decimating a mesh: vertex clustering with quadric placement (SfM::decimateMesh) ----------------------------------------------
int sfmba_mesh_decimate(int device, int64_t n_vertices, const float* xyz, const unsigned char* bgr, int64_t n_triangles, const int32_t* tri,
                        const float* origin, float quantum, int cell, int placement, int reg, float* xyz_out, unsigned char* bgr_out, int32_t* members,
                        int64_t vcap, int32_t* tri_out, int32_t* triangle_of, int64_t tcap, int32_t* vertex_of, int64_t* n_vertices_out,
                        int64_t* n_triangles_out, int64_t* stats) {
    const char* who = "mesh_decimate";
    if (const int rc = clean_check_mesh(who, n_vertices, xyz, true, n_triangles, tri)) return rc;
    const CleanFilterOut shape{ xyz_out, bgr_out, nullptr, vcap, tri_out, tcap, vertex_of, n_vertices_out, n_triangles_out };
    if (const int rc = clean_check_out(shape, bgr != nullptr)) return rc;
    CleanSmoothParams q;                                          // the smooth's rules for origin and quantum
    if (const int rc = clean_check_smooth(who, origin, quantum, 0, 0.5f, -0.5f, q)) return rc;
    if (cell < DEC_MIN_CELL || cell > DEC_MAX_CELL) return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": cell must be in 32..2^20 quanta");
    if (placement != 0 && placement != 1) return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": placement must be 0 (mean) or 1 (quadric)");
    if (placement == 1 && (reg < 1 || reg > DEC_MAX_REG)) return fail(SFMBA_ERR_INVALID_ARG, std::string(who) + ": reg must be in 1..2^20");
    const CleanMesh m{ (int)n_vertices, (int)n_triangles, xyz, bgr, tri };
    const DecimateParams p{ { q.origin[0], q.origin[1], q.origin[2] }, q.quantum, cell, placement, placement == 1 ? reg : 1 };
    const DecimateOut out{ xyz_out, bgr_out, members, vcap, tri_out, triangle_of, tcap, vertex_of, n_vertices_out, n_triangles_out, stats };
    TimedCall<DEC_T_COUNT> c("SFMBA_MESH_DECIMATE_TIMING");      // (tools/mesh_decimate_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = mesh_decimate(c.kit.stream, device, m, p, out, c.tm());
    if ((rc == 0 || rc == UNIT_ERR_CAPACITY) && c.on)
        std::fprintf(stderr,
                     "[sfmba mesh_decimate] upload_ms %.6f keys_ms %.6f sort_ms %.6f runs_ms %.6f members_ms %.6f quadrics_ms %.6f solve_ms %.6f "
                     "map_ms %.6f dedup_ms %.6f compact_ms %.6f emit_ms %.6f download_ms %.6f vertices %lld triangles %lld vertices_out %lld "
                     "triangles_out %lld\n",
                     c.t[DEC_T_UPLOAD], c.t[DEC_T_KEYS], c.t[DEC_T_SORT], c.t[DEC_T_RUNS], c.t[DEC_T_MEMBERS], c.t[DEC_T_QUADRICS], c.t[DEC_T_SOLVE],
                     c.t[DEC_T_MAP], c.t[DEC_T_DEDUP], c.t[DEC_T_COMPACT], c.t[DEC_T_EMIT], c.t[DEC_T_DOWNLOAD], (long long)n_vertices,
                     (long long)n_triangles, (long long)*n_vertices_out, (long long)*n_triangles_out);
    return clean_result(rc, who);
}
// ---- texturing a mesh: a view per triangle and a texture atlas (SfM::textureMesh) -------------------------------------------------
int sfmba_mesh_texture_size(int64_t n_triangles, int patch, int blocks_per_row, int32_t* width, int32_t* height) {
    if (!width || !height) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    long long W, H;
    if (const int rc = texture_check_layout("mesh_texture_size", n_triangles, patch, blocks_per_row, W, H)) return rc;
    *width = (int32_t)W;
    *height = (int32_t)H;
    return SFMBA_OK;
}
int sfmba_mesh_texture(int device, int64_t n_vertices, const float* xyz, const unsigned char* bgr, int64_t n_triangles, const int32_t* tri,
                       int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels,
                       const float* K, const float* P, const float* const* depth, float occl_tol, int64_t min_area, int patch, int blocks_per_row,
                       unsigned char* atlas, float* uv, int32_t* view, int64_t* score, int64_t* n_textured) {
    if (const int rc = clean_check_mesh("mesh_texture", n_vertices, xyz, true, n_triangles, tri)) return rc;
    if (!atlas || !uv || !view || !n_textured || (n_images > 0 && !depth)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (const int rc = depth_check_images("mesh_texture", n_images, img_ptr, pixels, width, height, channels, K, P)) return rc;
    if (const int rc = texture_check_rule("mesh_texture", occl_tol, min_area)) return rc;
    long long W, H;
    if (const int rc = texture_check_layout("mesh_texture", n_triangles, patch, blocks_per_row, W, H)) return rc;
    const TexMesh m{ (int)n_vertices, (int)n_triangles, xyz, bgr, tri };
    const TexViews views{ n_images, img_ptr, pixels, width, height, channels, K, P, depth };
    const TexParams prm{ occl_tol, min_area, patch, blocks_per_row, (int)W, (int)H };
    const TexOut out{ atlas, uv, view, score, n_textured };
    TimedCall<TEX_T_COUNT> c("SFMBA_MESH_TEXTURE_TIMING");       // (tools/texture_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = mesh_texture(c.kit.stream, device, m, views, prm, out, c.tm());
    if (rc == 0 && c.on)
        std::fprintf(stderr, "[sfmba mesh_texture] upload_ms %.6f check_ms %.6f views_ms %.6f raster_ms %.6f download_ms %.6f vertices %lld "
                             "triangles %lld images %d width %lld height %lld textured %lld\n",
                     c.t[TEX_T_UPLOAD], c.t[TEX_T_CHECK], c.t[TEX_T_VIEWS], c.t[TEX_T_RASTER], c.t[TEX_T_DOWNLOAD], (long long)n_vertices,
                     (long long)n_triangles, n_images, W, H, (long long)*n_textured);
    return texture_result(rc, "mesh_texture");
}
// ---- smoothing the view labels (SfM::textureMesh with TextureParams::smoothRings / smoothPasses) ------------------------------------
int sfmba_mesh_view_candidates(int device, int64_t n_vertices, const float* xyz, int64_t n_triangles, const int32_t* tri, int n_images,
                               const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels,
                               const float* K, const float* P, const float* const* depth, float occl_tol, int64_t min_area, int n_candidates,
                               int32_t* cand_view, int64_t* cand_score) {
    if (const int rc = clean_check_mesh("mesh_view_candidates", n_vertices, xyz, true, n_triangles, tri)) return rc;
    if ((n_triangles > 0 && (!cand_view || !cand_score)) || (n_images > 0 && !depth)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (const int rc = depth_check_images("mesh_view_candidates", n_images, img_ptr, pixels, width, height, channels, K, P)) return rc;
    if (const int rc = texture_check_rule("mesh_view_candidates", occl_tol, min_area)) return rc;
    if (const int rc = label_check_k("mesh_view_candidates", n_candidates)) return rc;
    const TexMesh m{ (int)n_vertices, (int)n_triangles, xyz, nullptr, tri };
    const TexViews views{ n_images, img_ptr, pixels, width, height, channels, K, P, depth };
    TimedCall<LAB_T_COUNT> c("SFMBA_MESH_LABELS_TIMING");        // (tools/texture_smooth_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = mesh_view_candidates(c.kit.stream, device, m, views, occl_tol, min_area, n_candidates, cand_view, cand_score, c.tm());
    if (rc == 0 && c.on) label_timing_line("mesh_view_candidates", c.t, (long long)n_triangles);
    return texture_result(rc, "mesh_view_candidates");
}
int sfmba_mesh_adjacency(int device, int64_t n_triangles, const int32_t* tri, int32_t* adj, int64_t* n_pairs, int64_t* n_open_edges,
                         int64_t* n_nonmanifold_edges) {
    if (const int rc = label_check_count("mesh_adjacency", n_triangles)) return rc;
    if (!n_pairs || !n_open_edges || !n_nonmanifold_edges || (n_triangles > 0 && (!tri || !adj))) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    for (int64_t i = 0; i < 3 * n_triangles; ++i)
        if (tri[i] < 0) return fail(SFMBA_ERR_INVALID_ARG, "mesh_adjacency: a triangle index is negative");
    TimedCall<LAB_T_COUNT> c("SFMBA_MESH_LABELS_TIMING");
    if (const int rc = c.open(device)) return rc;
    int64_t counts[3] = { 0, 0, 0 };
    const int rc = mesh_adjacency(c.kit.stream, device, (int)n_triangles, tri, adj, counts, c.tm());
    if (rc == 0) { *n_pairs = counts[0]; *n_open_edges = counts[1]; *n_nonmanifold_edges = counts[2]; }
    if (rc == 0 && c.on) label_timing_line("mesh_adjacency", c.t, (long long)n_triangles);
    return unit_result(rc, "mesh_adjacency");
}
int sfmba_mesh_view_smooth(int device, int64_t n_triangles, int n_images, int n_candidates, const int32_t* cand_view, const int64_t* cand_score,
                           const int32_t* adj, int rings, int penalty, int max_passes, int32_t* view, int64_t* stats) {
    if (const int rc = label_check_count("mesh_view_smooth", n_triangles)) return rc;
    if (n_images < 0) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (!stats || (n_triangles > 0 && (!cand_view || !cand_score || !adj || !view))) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (const int rc = label_check_k("mesh_view_smooth", n_candidates)) return rc;
    if (const int rc = label_check_params("mesh_view_smooth", rings, penalty, max_passes)) return rc;
    if (const int rc = label_check_lists("mesh_view_smooth", n_triangles, n_images, n_candidates, cand_view, cand_score, adj)) return rc;
    const LabelParams p{ n_candidates, rings, penalty, max_passes };
    TimedCall<LAB_T_COUNT> c("SFMBA_MESH_LABELS_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = mesh_view_smooth(c.kit.stream, device, (int)n_triangles, p, cand_view, cand_score, adj, view, stats, c.tm());
    if (rc == 0 && c.on) label_timing_line("mesh_view_smooth", c.t, (long long)n_triangles);
    return unit_result(rc, "mesh_view_smooth");
}
int sfmba_mesh_texture_from_views(int device, int64_t n_vertices, const float* xyz, const unsigned char* bgr, int64_t n_triangles, const int32_t* tri,
                                  int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                                  int channels, const float* K, const float* P, int patch, int blocks_per_row, const int32_t* view, unsigned char* atlas,
                                  float* uv, int64_t* n_textured) {
    if (const int rc = clean_check_mesh("mesh_texture_from_views", n_vertices, xyz, true, n_triangles, tri)) return rc;
    if (!atlas || !uv || !n_textured || (n_triangles > 0 && !view)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (const int rc = depth_check_images("mesh_texture_from_views", n_images, img_ptr, pixels, width, height, channels, K, P)) return rc;
    long long W, H;
    if (const int rc = texture_check_layout("mesh_texture_from_views", n_triangles, patch, blocks_per_row, W, H)) return rc;
    const std::vector<const float*> no_maps((size_t)std::max(n_images, 1), nullptr);       // the labels are given: nothing is tested
    const TexMesh m{ (int)n_vertices, (int)n_triangles, xyz, bgr, tri };
    const TexViews views{ n_images, img_ptr, pixels, width, height, channels, K, P, no_maps.data() };
    const TexParams prm{ 0.0f, 0, patch, blocks_per_row, (int)W, (int)H };
    const TexOut out{ atlas, uv, nullptr, nullptr, n_textured };
    const int32_t none = -1;
    const TexLabels labels{ n_triangles > 0 ? view : &none, 0, 0, 0, 0, nullptr, nullptr };
    TimedCall<TEX_T_COUNT> c("SFMBA_MESH_TEXTURE_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = mesh_texture(c.kit.stream, device, m, views, prm, out, c.tm(), &labels);
    return texture_result(rc, "mesh_texture_from_views");
}
int sfmba_mesh_texture_smooth(int device, int64_t n_vertices, const float* xyz, const unsigned char* bgr, int64_t n_triangles, const int32_t* tri,
                              int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                              int channels, const float* K, const float* P, const float* const* depth, float occl_tol, int64_t min_area, int patch,
                              int blocks_per_row, int n_candidates, int rings, int penalty, int max_passes, unsigned char* atlas, float* uv,
                              int32_t* view, int64_t* score, int64_t* n_textured, int64_t* stats) {
    if (const int rc = clean_check_mesh("mesh_texture_smooth", n_vertices, xyz, true, n_triangles, tri)) return rc;
    if (!atlas || !uv || !view || !n_textured || !stats || (n_images > 0 && !depth)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (const int rc = depth_check_images("mesh_texture_smooth", n_images, img_ptr, pixels, width, height, channels, K, P)) return rc;
    if (const int rc = texture_check_rule("mesh_texture_smooth", occl_tol, min_area)) return rc;
    long long W, H;
    if (const int rc = texture_check_layout("mesh_texture_smooth", n_triangles, patch, blocks_per_row, W, H)) return rc;
    if (const int rc = label_check_count("mesh_texture_smooth", n_triangles)) return rc;
    if (const int rc = label_check_k("mesh_texture_smooth", n_candidates)) return rc;
    if (const int rc = label_check_params("mesh_texture_smooth", rings, penalty, max_passes)) return rc;
    const TexMesh m{ (int)n_vertices, (int)n_triangles, xyz, bgr, tri };
    const TexViews views{ n_images, img_ptr, pixels, width, height, channels, K, P, depth };
    const TexParams prm{ occl_tol, min_area, patch, blocks_per_row, (int)W, (int)H };
    const TexOut out{ atlas, uv, view, score, n_textured };
    TimedCall<TEX_T_COUNT> c("SFMBA_MESH_TEXTURE_TIMING");
    double lt[LAB_T_COUNT];
    const TexLabels labels{ nullptr, n_candidates, rings, penalty, max_passes, stats, c.on ? lt : nullptr };
    if (const int rc = c.open(device)) return rc;
    const int rc = mesh_texture(c.kit.stream, device, m, views, prm, out, c.tm(), &labels);
    if (rc == 0 && c.on) {
        std::fprintf(stderr, "[sfmba mesh_texture_smooth] upload_ms %.6f check_ms %.6f views_ms %.6f raster_ms %.6f download_ms %.6f triangles %lld\n",
                     c.t[TEX_T_UPLOAD], c.t[TEX_T_CHECK], c.t[TEX_T_VIEWS], c.t[TEX_T_RASTER], c.t[TEX_T_DOWNLOAD], (long long)n_triangles);
        label_timing_line("mesh_texture_smooth", lt, (long long)n_triangles);
    }
    return texture_result(rc, "mesh_texture_smooth");
}
// ---- levelling the colours across seams (SfM::textureMesh with TextureParams::levelPasses) ----------------------------------------------
int sfmba_mesh_colour_nodes(int device, int64_t n_vertices, const float* xyz, int64_t n_triangles, const int32_t* tri, int n_images,
                            const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels,
                            const float* K, const float* P, const int32_t* view, int sample_radius, int64_t* n_nodes, int32_t* node_vertex,
                            int32_t* node_view, int32_t* node_of, unsigned char* seen, int32_t* F) {
    if (const int rc = clean_check_mesh("mesh_colour_nodes", n_vertices, xyz, true, n_triangles, tri)) return rc;
    if (!n_nodes || (n_triangles > 0 && (!view || !node_vertex || !node_view || !node_of || !seen || !F))) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (const int rc = depth_check_images("mesh_colour_nodes", n_images, img_ptr, pixels, width, height, channels, K, P)) return rc;
    if (const int rc = label_check_count("mesh_colour_nodes", n_triangles)) return rc;
    if (const int rc = colour_check_params("mesh_colour_nodes", sample_radius, 1, 0)) return rc;
    const TexMesh m{ (int)n_vertices, (int)n_triangles, xyz, nullptr, tri };
    const TexViews views{ n_images, img_ptr, pixels, width, height, channels, K, P, nullptr };
    CallKit ck;
    if (const int rc = ck.open(device)) return rc;
    const int rc = mesh_colour_nodes(ck.kit.stream, device, m, views, view, sample_radius, n_nodes, node_vertex, node_view, node_of, seen, F);
    return texture_result(rc, "mesh_colour_nodes");
}
int sfmba_mesh_colour_level(int device, int64_t n_nodes, const int32_t* node_vertex, const unsigned char* seen, const int32_t* F, int64_t n_triangles,
                            const int32_t* node_of, int seam_weight, int passes, int32_t* g, int64_t* stats) {
    if (const int rc = label_check_count("mesh_colour_level", n_triangles)) return rc;
    if (n_nodes < 0 || n_nodes > (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "mesh_colour_level: n_nodes must lie in 0 .. 2^31 - 1");
    if (!stats || (n_nodes > 0 && (!node_vertex || !seen || !F || !g)) || (n_triangles > 0 && !node_of)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (const int rc = colour_check_params("mesh_colour_level", 0, seam_weight, passes)) return rc;
    if (const int rc = colour_check_rows("mesh_colour_level", n_triangles, node_of, n_nodes)) return rc;
    for (int64_t n = 0; n < n_nodes; ++n) {
        if (n > 0 && node_vertex[n] < node_vertex[n - 1]) return fail(SFMBA_ERR_INVALID_ARG, "mesh_colour_level: node_vertex decreases");
        for (int c = 0; c < 3; ++c)
            if (F[3 * n + c] < 0 || F[3 * n + c] > COLOUR_F_MAX) return fail(SFMBA_ERR_INVALID_ARG, "mesh_colour_level: an F lies outside 0..65280");
    }
    CallKit ck;
    if (const int rc = ck.open(device)) return rc;
    const int rc = mesh_colour_level(ck.kit.stream, device, (int)n_nodes, node_vertex, seen, F, (int)n_triangles, node_of, seam_weight, passes, g, stats);
    return unit_result(rc, "mesh_colour_level");
}
int sfmba_mesh_texture_levelled(int device, int64_t n_vertices, const float* xyz, const unsigned char* bgr, int64_t n_triangles, const int32_t* tri,
                                int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                                int channels, const float* K, const float* P, int patch, int blocks_per_row, const int32_t* view, const int32_t* node_of,
                                const int32_t* g, int64_t n_nodes, unsigned char* atlas, float* uv, int64_t* n_textured, int64_t* n_clamped) {
    if (const int rc = clean_check_mesh("mesh_texture_levelled", n_vertices, xyz, true, n_triangles, tri)) return rc;
    if (n_nodes < 0 || n_nodes > (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "mesh_texture_levelled: n_nodes must lie in 0 .. 2^31 - 1");
    if (!atlas || !uv || !n_textured || !n_clamped || (n_triangles > 0 && (!view || !node_of)) || (n_nodes > 0 && !g)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (const int rc = depth_check_images("mesh_texture_levelled", n_images, img_ptr, pixels, width, height, channels, K, P)) return rc;
    long long W, H;
    if (const int rc = texture_check_layout("mesh_texture_levelled", n_triangles, patch, blocks_per_row, W, H)) return rc;
    if (const int rc = label_check_count("mesh_texture_levelled", n_triangles)) return rc;
    if (const int rc = colour_check_rows("mesh_texture_levelled", n_triangles, node_of, n_nodes)) return rc;
    for (int64_t i = 0; i < 3 * n_nodes; ++i)
        if (g[i] < -COLOUR_F_MAX || g[i] > COLOUR_F_MAX) return fail(SFMBA_ERR_INVALID_ARG, "mesh_texture_levelled: a g lies outside -65280..65280");
    const std::vector<const float*> no_maps((size_t)std::max(n_images, 1), nullptr);       // the labels are given: nothing is tested
    const TexMesh m{ (int)n_vertices, (int)n_triangles, xyz, bgr, tri };
    const TexViews views{ n_images, img_ptr, pixels, width, height, channels, K, P, no_maps.data() };
    const TexParams prm{ 0.0f, 0, patch, blocks_per_row, (int)W, (int)H };
    const TexOut out{ atlas, uv, nullptr, nullptr, n_textured };
    const int32_t none = -1;
    const TexLabels labels{ n_triangles > 0 ? view : &none, 0, 0, 0, 0, nullptr, nullptr };
    const int32_t no_row[3] = { -1, -1, -1 };
    const TexLevel level{ n_triangles > 0 ? node_of : no_row, g, (int)n_nodes, 0, 0, 0, nullptr, n_clamped, nullptr };
    TimedCall<TEX_T_COUNT> c("SFMBA_MESH_TEXTURE_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = mesh_texture(c.kit.stream, device, m, views, prm, out, c.tm(), &labels, &level);
    return texture_result(rc, "mesh_texture_levelled");
}
int sfmba_mesh_texture_adjust(int device, int64_t n_vertices, const float* xyz, const unsigned char* bgr, int64_t n_triangles, const int32_t* tri,
                              int n_images, const int64_t* img_ptr, const unsigned char* pixels, const int32_t* width, const int32_t* height,
                              int channels, const float* K, const float* P, const float* const* depth, float occl_tol, int64_t min_area, int patch,
                              int blocks_per_row, int n_candidates, int rings, int penalty, int max_passes, unsigned char* atlas, float* uv,
                              int32_t* view, int64_t* score, int64_t* n_textured, int64_t* stats, int sample_radius, int seam_weight, int level_passes,
                              int64_t* level_stats) {
    if (const int rc = clean_check_mesh("mesh_texture_adjust", n_vertices, xyz, true, n_triangles, tri)) return rc;
    if (!atlas || !uv || !view || !n_textured || !stats || !level_stats || (n_images > 0 && !depth)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (const int rc = depth_check_images("mesh_texture_adjust", n_images, img_ptr, pixels, width, height, channels, K, P)) return rc;
    if (const int rc = texture_check_rule("mesh_texture_adjust", occl_tol, min_area)) return rc;
    long long W, H;
    if (const int rc = texture_check_layout("mesh_texture_adjust", n_triangles, patch, blocks_per_row, W, H)) return rc;
    if (const int rc = label_check_count("mesh_texture_adjust", n_triangles)) return rc;
    if (const int rc = label_check_k("mesh_texture_adjust", n_candidates)) return rc;
    if (const int rc = label_check_params("mesh_texture_adjust", rings, penalty, max_passes)) return rc;
    if (const int rc = colour_check_params("mesh_texture_adjust", sample_radius, seam_weight, level_passes)) return rc;
    const TexMesh m{ (int)n_vertices, (int)n_triangles, xyz, bgr, tri };
    const TexViews views{ n_images, img_ptr, pixels, width, height, channels, K, P, depth };
    const TexParams prm{ occl_tol, min_area, patch, blocks_per_row, (int)W, (int)H };
    const TexOut out{ atlas, uv, view, score, n_textured };
    TimedCall<TEX_T_COUNT> c("SFMBA_MESH_TEXTURE_TIMING");       // (tools/texture_level_bench.py)
    double lt[LAB_T_COUNT], ct[COL_T_COUNT];
    const TexLabels labels{ nullptr, n_candidates, rings, penalty, max_passes, stats, c.on ? lt : nullptr };
    const TexLevel level{ nullptr, nullptr, 0, sample_radius, seam_weight, level_passes, level_stats, nullptr, c.on ? ct : nullptr };
    if (const int rc = c.open(device)) return rc;
    const int rc = mesh_texture(c.kit.stream, device, m, views, prm, out, c.tm(), &labels, &level);
    if (rc == 0 && c.on) {
        std::fprintf(stderr, "[sfmba mesh_texture_adjust] upload_ms %.6f check_ms %.6f views_ms %.6f raster_ms %.6f download_ms %.6f triangles %lld\n",
                     c.t[TEX_T_UPLOAD], c.t[TEX_T_CHECK], c.t[TEX_T_VIEWS], c.t[TEX_T_RASTER], c.t[TEX_T_DOWNLOAD], (long long)n_triangles);
        label_timing_line("mesh_texture_adjust", lt, (long long)n_triangles);
        std::fprintf(stderr, "[sfmba mesh_texture_adjust level] keys_ms %.6f sort_ms %.6f nodes_ms %.6f colours_ms %.6f passes_ms %.6f stats_ms %.6f nodes %lld "
                             "passes %d\n",
                     ct[COL_T_KEYS], ct[COL_T_SORT], ct[COL_T_NODES], ct[COL_T_COLOURS], ct[COL_T_PASSES], ct[COL_T_STATS], (long long)level_stats[0], level_passes);
    }
    return texture_result(rc, "mesh_texture_adjust");
}
// ---- pose of a new view (SfMStereoUtilities::findCameraPoseFrom2D3DMatch) -------------------------------------------
int sfmba_pnp_ransac(int device, int n_prob, const int64_t* prob_ptr, const float* xyz, const float* uv, const float* K, int n_hyp,
                     float threshold_px, uint64_t seed, int max_refine_iters, double* pose, unsigned char* inlier,
                     sfmba_pnp_result* result, double* hyp_pose, int32_t* hyp_count) {
    if (n_prob < 0 || !prob_ptr || !K || (n_prob > 0 && (!pose || !result))) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (const int rc = check_ransac(n_hyp, threshold_px)) return rc;
    if (const int rc = check_focal(K)) return rc;
    if (max_refine_iters < 0) return fail(SFMBA_ERR_INVALID_ARG, "max_refine_iters must be >= 0");
    if (prob_ptr[0] < 0) return fail(SFMBA_ERR_INVALID_ARG, "prob_ptr must not be negative");
    for (int p = 0; p < n_prob; ++p) {
        if (prob_ptr[p + 1] < prob_ptr[p]) return fail(SFMBA_ERR_INVALID_ARG, "prob_ptr not monotone");
        if (prob_ptr[p + 1] - prob_ptr[p] >= (int64_t)INT_MAX) return fail(SFMBA_ERR_INVALID_ARG, "pnp_ransac: a problem has 2^31 or more points");
    }
    if (prob_ptr[n_prob] > 0 && (!xyz || !uv || !inlier)) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (n_prob == 0) return check_device(device);
    TimedCall<3> c("SFMBA_PNP_TIMING");          // (tools/pnp_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = pnp_ransac(c.kit.stream, device, n_prob, prob_ptr, xyz, uv, K, n_hyp, threshold_px, seed, max_refine_iters, pose, inlier, result,
                              hyp_pose, hyp_count, c.tm());
    if (rc == 0 && c.on) std::fprintf(stderr, "[sfmba pnp] upload_ms %.6f kernels_ms %.6f download_ms %.6f\n", c.t[0], c.t[1], c.t[2]);
    return unit_result(rc, "pnp_ransac", "too many problems x hypotheses for one call");
}
// ---- baseline pair ranking (SfMStereoUtilities::findHomographyInliers) ------------------------------------------------
int sfmba_homography_ransac(int device, int n_images, const int64_t* img_ptr, const float* pts, int n_pairs, const int32_t* pair_left,
                            const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx, int n_hyp,
                            float threshold_px, uint64_t seed, double* H, unsigned char* inlier, sfmba_homography_result* result, double* hyp_H,
                            int32_t* hyp_count) {
    if (n_images < 0 || n_pairs < 0 || !img_ptr || !pair_ptr || (n_pairs > 0 && (!pair_left || !pair_right || !H || !result)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (const int rc = check_ransac(n_hyp, threshold_px)) return rc;
    if (const int rc = check_match_list("homography_ransac", n_images, img_ptr, pts, n_pairs, pair_left, pair_right, pair_ptr, query_idx, train_idx)) return rc;
    if (pair_ptr[n_pairs] > pair_ptr[0] && !inlier) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (n_pairs == 0) return check_device(device);
    TimedCall<5> c("SFMBA_HOMOGRAPHY_TIMING");          // (tools/homography_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = homography_ransac(c.kit.stream, device, n_images, img_ptr, pts, n_pairs, pair_left, pair_right, pair_ptr, query_idx, train_idx, n_hyp,
                                     threshold_px, seed, H, inlier, result, hyp_H, hyp_count, c.tm());
    if (rc == 0 && c.on)
        std::fprintf(stderr, "[sfmba homography] upload_ms %.6f hypotheses_ms %.6f score_ms %.6f select_ms %.6f download_ms %.6f\n", c.t[0], c.t[1], c.t[2],
                     c.t[3], c.t[4]);
    return unit_result(rc, "homography_ransac", "too many pairs x hypotheses for one call");
}
// ---- pose of an image pair (SfMStereoUtilities::findCameraMatricesFromMatch): same checks, same refusals, and K ---------------------
int sfmba_essential_ransac(int device, int n_images, const int64_t* img_ptr, const float* pts, int n_pairs, const int32_t* pair_left,
                           const int32_t* pair_right, const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx, const float* K,
                           int n_hyp, float threshold_px, uint64_t seed, double* E, double* pose, unsigned char* inlier,
                           sfmba_essential_result* result, double* hyp_E, int32_t* hyp_count, int32_t* hyp_nsol) {
    if (n_images < 0 || n_pairs < 0 || !img_ptr || !pair_ptr || !K || (n_pairs > 0 && (!pair_left || !pair_right || !E || !pose || !result)))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (const int rc = check_ransac(n_hyp, threshold_px)) return rc;
    if (const int rc = check_focal(K)) return rc;
    if (const int rc = check_match_list("essential_ransac", n_images, img_ptr, pts, n_pairs, pair_left, pair_right, pair_ptr, query_idx, train_idx)) return rc;
    if (pair_ptr[n_pairs] > pair_ptr[0] && !inlier) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    if (n_pairs == 0) return check_device(device);
    TimedCall<5> c("SFMBA_ESSENTIAL_TIMING");          // (tools/essential_bench.py)
    if (const int rc = c.open(device)) return rc;
    const int rc = essential_ransac(c.kit.stream, device, n_images, img_ptr, pts, n_pairs, pair_left, pair_right, pair_ptr, query_idx, train_idx, K, n_hyp,
                                    threshold_px, seed, E, pose, inlier, result, hyp_E, hyp_count, hyp_nsol, c.tm());
    if (rc == 0 && c.on)
        std::fprintf(stderr, "[sfmba essential] upload_ms %.6f hypotheses_ms %.6f score_ms %.6f select_ms %.6f download_ms %.6f\n", c.t[0], c.t[1], c.t[2],
                     c.t[3], c.t[4]);
    return unit_result(rc, "essential_ransac", "too many pairs x hypotheses for one call");
}
// ---- reading photographs (SfM::setImagesDirectory: imread + resize) ---------------------------------------------------
int sfmba_jpeg_info(int n_images, const int64_t* file_ptr, const unsigned char* bytes, sfmba_image_info* info) {
    if (const int rc = check_file_ptr(n_images, file_ptr, bytes)) return rc;
    if (n_images > 0 && !info) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    std::vector<JpegHeader> hdr;
    jpeg_parse_batch(n_images, file_ptr, bytes, hdr);
    for (int i = 0; i < n_images; ++i) jpeg_fill_info(hdr[(size_t)i], &info[i]);
    return SFMBA_OK;
}

int sfmba_resized_size(int width, int height, float factor, int32_t* out_width, int32_t* out_height) {
    if (!out_width || !out_height) return fail(SFMBA_ERR_INVALID_ARG, "NULL argument");
    if (!std::isfinite(factor) || !(factor > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "factor must be finite and > 0");
    if (width < 1 || width > JPEG_MAX_SIDE || height < 1 || height > JPEG_MAX_SIDE) return fail(SFMBA_ERR_INVALID_ARG, "an image dimension lies outside 1..16384");
    const int ow = resized_length(width, factor), oh = resized_length(height, factor);
    if (ow == 0 || oh == 0) return fail(SFMBA_ERR_INVALID_ARG, "the factor gives the image a side outside 1..16384");
    *out_width = ow; *out_height = oh;
    return SFMBA_OK;
}

int sfmba_jpeg_decode(int device, int n_images, const int64_t* file_ptr, const unsigned char* bytes, float factor, sfmba_image_info* info,
                      int64_t* out_ptr, unsigned char* out, int64_t cap, int64_t* total) {
    if (const int rc = check_file_ptr(n_images, file_ptr, bytes)) return rc;
    if (cap < 0 || !out_ptr || !total || (n_images > 0 && !info) || (cap > 0 && !out)) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (!std::isfinite(factor) || !(factor > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "jpeg_decode: factor must be finite and > 0");
    // the entropy decode runs on the host: its line has that time in front of the HIP-event times (tools/image_io_bench.py)
    TimedCall<JPEG_T_COUNT> c("SFMBA_JPEG_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = jpeg_decode(c.kit.stream, device, n_images, file_ptr, bytes, factor, info, out_ptr, out, cap, total, c.tm());
    if (rc == 0 && c.on) image_timing_line("jpeg_decode", c.t);
    return unit_result(rc, "jpeg_decode");
}

int sfmba_resize_images(int device, int n_images, const int64_t* img_ptr, const unsigned char* px, const int32_t* width, const int32_t* height,
                        int channels, float factor, int64_t* out_ptr, unsigned char* out, int64_t cap, int64_t* total) {
    if (n_images < 0 || cap < 0 || !img_ptr || !out_ptr || !total || (n_images > 0 && (!width || !height)) || (cap > 0 && !out))
        return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (!std::isfinite(factor) || !(factor > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "resize_images: factor must be finite and > 0");
    if (const int rc = check_images("resize_images", n_images, img_ptr, px, width, height, channels)) return rc;
    for (int i = 0; i < n_images; ++i)
        if (resized_length(width[i], factor) == 0 || resized_length(height[i], factor) == 0)
            return fail(SFMBA_ERR_INVALID_ARG, "resize_images: the factor gives an image a side outside 1..16384");
    TimedCall<JPEG_T_COUNT> c("SFMBA_JPEG_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = resize_images(c.kit.stream, device, n_images, img_ptr, px, width, height, channels, factor, out_ptr, out, cap, total, c.tm());
    if (rc == 0 && c.on) image_timing_line("resize_images", c.t);
    return unit_result(rc, "resize_images");
}

int sfmba_png_info(int n_images, const int64_t* file_ptr, const unsigned char* bytes, struct sfmba_png_info* info) {
    if (const int rc = check_file_ptr(n_images, file_ptr, bytes)) return rc;
    if (n_images > 0 && !info) return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    std::vector<PngHeader> hdr;
    png_parse_batch(n_images, file_ptr, bytes, hdr);
    for (int i = 0; i < n_images; ++i) png_fill_info(hdr[(size_t)i], &info[i]);
    return SFMBA_OK;
}

int sfmba_png_decode(int device, int n_images, const int64_t* file_ptr, const unsigned char* bytes, float factor, struct sfmba_png_info* info,
                     int64_t* out_ptr, unsigned char* out, int64_t cap, int64_t* total) {
    if (const int rc = check_file_ptr(n_images, file_ptr, bytes)) return rc;
    if (cap < 0 || !out_ptr || !total || (n_images > 0 && !info) || (cap > 0 && !out)) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    if (!std::isfinite(factor) || !(factor > 0.0f)) return fail(SFMBA_ERR_INVALID_ARG, "png_decode: factor must be finite and > 0");
    // the inflate runs on the host: its line has that time in front of the HIP-event times (tools/image_io_bench.py)
    TimedCall<PNG_T_COUNT> c("SFMBA_PNG_TIMING");
    if (const int rc = c.open(device)) return rc;
    const int rc = png_decode(c.kit.stream, device, n_images, file_ptr, bytes, factor, info, out_ptr, out, cap, total, c.tm());
    if (rc == 0 && c.on)
        std::fprintf(stderr, "[sfmba png_decode] inflate_ms %.6f upload_ms %.6f unfilter_ms %.6f pixels_ms %.6f resize_ms %.6f download_ms %.6f groups %d\n",
                     c.t[PNG_T_INFLATE], c.t[PNG_T_UPLOAD], c.t[PNG_T_UNFILTER], c.t[PNG_T_PIXELS], c.t[PNG_T_RESIZE], c.t[PNG_T_DOWNLOAD], (int)c.t[PNG_T_GROUPS]);
    return unit_result(rc, "png_decode");
}
}  // extern "C"
