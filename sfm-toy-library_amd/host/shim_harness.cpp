// shim_harness.cpp -- flat-array entry points used by the tests to drive the C++ shim, e.g. for tests/test_gpu_shim.py:
// builds the reference's containers (PointCloud / vector<Matx34f> / Intrinsics / vector<Features>),
// calls sfmtoylib::SfMBundleAdjustmentUtils::adjustBundle() and copies the containers back.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "SfMBundleAdjustmentUtils.h"
#include "SfMStereoUtilities.h"
#include "SfMAssociation.h"
#include "SfMExport.h"
#include "SfM2DFeatureUtilities.h"
#include "SfM.h"
#include "SfMImageUtilities.h"

extern "C" __attribute__((visibility("default")))
void sfmba_shim_adjust_bundle(int n_views, float* poses /*[n_views][12]*/, float* K /*[9]*/, int n_pts, float* points /*[n_pts][3]*/,
                              const int64_t* view_ptr, const int32_t* view_idx, const int32_t* feat_idx,
                              const int64_t* feat_ptr, const float* feat_xy) {
    using namespace sfmtoylib;
    std::vector<Pose> cams((size_t)n_views);
    for (int v = 0; v < n_views; ++v) for (int e = 0; e < 12; ++e) cams[v].val[e] = poses[12 * v + e];
    Intrinsics intr;
    intr.K = cv::Mat(3, 3);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) intr.K.at<float>(r, c) = K[3 * r + c];
    std::vector<Features> feats((size_t)n_views);
    for (int v = 0; v < n_views; ++v)
        for (int64_t f = feat_ptr[v]; f < feat_ptr[v + 1]; ++f) feats[v].points.push_back(cv::Point2f(feat_xy[2 * f], feat_xy[2 * f + 1]));
    PointCloud cloud((size_t)n_pts);
    for (int i = 0; i < n_pts; ++i) {
        cloud[i].p = cv::Point3f(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
        for (int64_t q = view_ptr[i]; q < view_ptr[i + 1]; ++q) cloud[i].originatingViews[view_idx[q]] = feat_idx[q];
    }
    const auto t0 = std::chrono::steady_clock::now();
    SfMBundleAdjustmentUtils::adjustBundle(cloud, cams, intr, feats);
    if (std::getenv("SFMBA_SHIM_TIMING"))
        std::fprintf(stderr, "[sfmba shim] adjustBundle() wall time %.3f ms\n",
                     1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    for (int v = 0; v < n_views; ++v) for (int e = 0; e < 12; ++e) poses[12 * v + e] = cams[v].val[e];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) K[3 * r + c] = intr.K.at<float>(r, c);
    for (int i = 0; i < n_pts; ++i) { points[3 * i] = cloud[i].p.x; points[3 * i + 1] = cloud[i].p.y; points[3 * i + 2] = cloud[i].p.z; }
}

// Flat-array driver of sfmtoylib::SfMStereoUtilities::triangulateViews (tests/test_gpu_triangulate.py): builds Features /
// Matching, calls the reference-signature function and flattens the resulting PointCloud.  Returns the number of points
// written (<= cap), or -1 when the call reported failure.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_triangulate_views(const float* K /*[9]*/, int left_view, int right_view, int n_left, const float* left_xy, int n_right,
                                 const float* right_xy, int n_match, const int32_t* query_idx, const int32_t* train_idx,
                                 const float* P_left /*[12]*/, const float* P_right /*[12]*/, int cap, float* points3d /*[cap][3]*/,
                                 int32_t* left_ref /*[cap]*/, int32_t* right_ref /*[cap]*/) {
    using namespace sfmtoylib;
    Intrinsics intr;
    intr.K = cv::Mat(3, 3);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) intr.K.at<float>(r, c) = K[3 * r + c];
    Features fl, fr;
    for (int i = 0; i < n_left; ++i) { cv::KeyPoint kp; kp.pt = cv::Point2f(left_xy[2 * i], left_xy[2 * i + 1]); fl.keyPoints.push_back(kp); fl.points.push_back(kp.pt); }
    for (int i = 0; i < n_right; ++i) { cv::KeyPoint kp; kp.pt = cv::Point2f(right_xy[2 * i], right_xy[2 * i + 1]); fr.keyPoints.push_back(kp); fr.points.push_back(kp.pt); }
    Matching matches;
    for (int i = 0; i < n_match; ++i) matches.push_back(cv::DMatch(query_idx[i], train_idx[i], 0.0f));
    cv::Matx34f Pl, Pr;
    for (int e = 0; e < 12; ++e) { Pl.val[e] = P_left[e]; Pr.val[e] = P_right[e]; }
    PointCloud cloud;
    ImagePair pair; pair.left = (size_t)left_view; pair.right = (size_t)right_view;
    if (!SfMStereoUtilities::triangulateViews(intr, pair, matches, fl, fr, Pl, Pr, cloud)) return -1;
    int n = 0;
    for (const Point3DInMap& p : cloud) {
        if (n >= cap) break;
        points3d[3 * n] = p.p.x; points3d[3 * n + 1] = p.p.y; points3d[3 * n + 2] = p.p.z;
        left_ref[n] = p.originatingViews.at(left_view);
        right_ref[n] = p.originatingViews.at(right_view);
        ++n;
    }
    return n;
}

// Flat-array driver of sfmtoylib::SfMStereoUtilities::findCameraPoseFrom2D3DMatch (tests/test_gpu_pnp_ransac.py).  pose [12] goes
// in and comes back (untouched when the call reports failure).  Returns 1 / 0 = the call's true / false.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_find_camera_pose(const float* K /*[9]*/, int n, const float* xyz /*[n][3]*/, const float* uv /*[n][2]*/, float* pose /*[12]*/) {
    using namespace sfmtoylib;
    Intrinsics intr;
    intr.K = cv::Mat(3, 3);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) intr.K.at<float>(r, c) = K[3 * r + c];
    Image2D3DMatch match;
    for (int i = 0; i < n; ++i) {
        match.points2D.push_back(cv::Point2f(uv[2 * i], uv[2 * i + 1]));
        match.points3D.push_back(cv::Point3f(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
    }
    cv::Matx34f P;
    for (int e = 0; e < 12; ++e) P.val[e] = pose[e];
    const bool ok = SfMStereoUtilities::findCameraPoseFrom2D3DMatch(intr, match, P);
    for (int e = 0; e < 12; ++e) pose[e] = P.val[e];
    return ok ? 1 : 0;
}

namespace {
std::vector<sfmtoylib::Features> buildKeyPoints(int n_images, const int64_t* img_ptr, const float* xy) {
    std::vector<sfmtoylib::Features> feats((size_t)n_images);
    for (int v = 0; v < n_images; ++v)
        for (int64_t f = img_ptr[v]; f < img_ptr[v + 1]; ++f) {
            cv::KeyPoint kp; kp.pt = cv::Point2f(xy[2 * f], xy[2 * f + 1]);
            feats[v].keyPoints.push_back(kp); feats[v].points.push_back(kp.pt);
        }
    return feats;
}
}  // namespace

// Flat-array driver of sfmtoylib::SfMStereoUtilities::findHomographyInliers (tests/test_gpu_homography_ransac.py): img_ptr [3] / xy
// hold the key points of the left (image 0) and the right image.  Returns the call's count.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_find_homography_inliers(const int64_t* img_ptr /*[3]*/, const float* xy, int n_match, const int32_t* query_idx, const int32_t* train_idx) {
    using namespace sfmtoylib;
    const std::vector<Features> feats = buildKeyPoints(2, img_ptr, xy);
    Matching matches;
    for (int i = 0; i < n_match; ++i) matches.push_back(cv::DMatch(query_idx[i], train_idx[i], 0.0f));
    return SfMStereoUtilities::findHomographyInliers(feats[0], feats[1], matches);
}

namespace {
sfmtoylib::Intrinsics buildIntrinsics(const float* K) {
    sfmtoylib::Intrinsics intr;
    if (K) {
        intr.K = cv::Mat(3, 3);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) intr.K.at<float>(r, c) = K[3 * r + c];
    }
    return intr;
}
}  // namespace

// Flat-array driver of sfmtoylib::SfMStereoUtilities::findCameraMatricesFromMatch (tests/test_gpu_essential_ransac.py): img_ptr [3] /
// xy hold the key points of the left (image 0) and the right image; K == NULL leaves the intrinsics empty.  P_left / P_right [12] and
// pruned [n_match][2] (query, train) go in and come back (untouched when the call reports failure); *n_pruned likewise.  Returns
// 1 / 0 = the call's true / false.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_find_camera_matrices(const float* K /*[9] or NULL*/, const int64_t* img_ptr /*[3]*/, const float* xy, int n_match,
                                    const int32_t* query_idx, const int32_t* train_idx, float* P_left, float* P_right, int32_t* pruned,
                                    int* n_pruned) {
    using namespace sfmtoylib;
    const std::vector<Features> feats = buildKeyPoints(2, img_ptr, xy);
    Matching matches, kept;
    for (int i = 0; i < n_match; ++i) matches.push_back(cv::DMatch(query_idx[i], train_idx[i], 0.0f));
    for (int i = 0; i < *n_pruned; ++i) kept.push_back(cv::DMatch(pruned[2 * i], pruned[2 * i + 1], 0.0f));
    cv::Matx34f Pl, Pr;
    for (int e = 0; e < 12; ++e) { Pl.val[e] = P_left[e]; Pr.val[e] = P_right[e]; }
    const bool ok = SfMStereoUtilities::findCameraMatricesFromMatch(buildIntrinsics(K), matches, feats[0], feats[1], kept, Pl, Pr);
    for (int e = 0; e < 12; ++e) { P_left[e] = Pl.val[e]; P_right[e] = Pr.val[e]; }
    *n_pruned = (int)kept.size();
    for (size_t i = 0; i < kept.size(); ++i) { pruned[2 * i] = kept[i].queryIdx; pruned[2 * i + 1] = kept[i].trainIdx; }
    return ok ? 1 : 0;
}

// Flat-array driver of sfmtoylib::SfMStereoUtilities::findCameraMatricesFromMatchBatch: ok [n_pairs], P_left / P_right [n_pairs][12],
// pruned_ptr [n_pairs + 1] and pruned [pair_ptr[n_pairs]][2] (query, train) come back.  Returns 1 / 0 = the call's true / false.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_find_camera_matrices_batch(const float* K /*[9] or NULL*/, int n_images, const int64_t* img_ptr, const float* xy, int n_pairs,
                                          const int32_t* left, const int32_t* right, const int64_t* pair_ptr, const int32_t* query,
                                          const int32_t* train, unsigned char* ok, float* P_left, float* P_right, int64_t* pruned_ptr,
                                          int32_t* pruned) {
    using namespace sfmtoylib;
    const std::vector<Features> feats = buildKeyPoints(n_images, img_ptr, xy);
    std::vector<const Features*> images;
    for (const Features& f : feats) images.push_back(&f);
    std::vector<Matching> lists((size_t)n_pairs);
    std::vector<const Matching*> matches;
    for (int p = 0; p < n_pairs; ++p) {
        for (int64_t e = pair_ptr[p]; e < pair_ptr[p + 1]; ++e) lists[p].push_back(cv::DMatch(query[e], train[e], 0.0f));
        matches.push_back(&lists[p]);
    }
    std::vector<unsigned char> good;
    std::vector<Matching> kept;
    std::vector<cv::Matx34f> Pl, Pr;
    const bool all = SfMStereoUtilities::findCameraMatricesFromMatchBatch(buildIntrinsics(K), images, std::vector<int>(left, left + n_pairs),
                                                                          std::vector<int>(right, right + n_pairs), matches, good, kept, Pl, Pr);
    int64_t n = 0;
    for (int p = 0; p < n_pairs; ++p) {
        ok[p] = good[p];
        for (int e = 0; e < 12; ++e) { P_left[12 * p + e] = Pl[p].val[e]; P_right[12 * p + e] = Pr[p].val[e]; }
        pruned_ptr[p] = n;
        for (const cv::DMatch& d : kept[p]) { pruned[2 * n] = d.queryIdx; pruned[2 * n + 1] = d.trainIdx; ++n; }
    }
    pruned_ptr[n_pairs] = n;
    return all ? 1 : 0;
}

// Flat-array driver of sfmtoylib::SfMStereoUtilities::triangulateViewsBatch (tests/test_gpu_triangulate_pairs.py): the clouds come
// back one after the other, cloud_ptr [n_pairs + 1] cutting points3d / left_ref / right_ref (points beyond cap are not written);
// ok [n_pairs].  Returns 1 / 0 = the call's true / false.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_triangulate_views_batch(const float* K /*[9] or NULL*/, int n_images, const int64_t* img_ptr, const float* xy, int n_pairs,
                                       const int32_t* left, const int32_t* right, const int64_t* pair_ptr, const int32_t* query,
                                       const int32_t* train, const float* P_left /*[n_pairs][12]*/, const float* P_right, unsigned char* ok,
                                       int64_t* cloud_ptr, int64_t cap, float* points3d, int32_t* left_ref, int32_t* right_ref) {
    using namespace sfmtoylib;
    const std::vector<Features> feats = buildKeyPoints(n_images, img_ptr, xy);
    std::vector<const Features*> images;
    for (const Features& f : feats) images.push_back(&f);
    std::vector<Matching> lists((size_t)n_pairs);
    std::vector<const Matching*> matches;
    std::vector<cv::Matx34f> Pl((size_t)n_pairs), Pr((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        for (int64_t e = pair_ptr[p]; e < pair_ptr[p + 1]; ++e) lists[p].push_back(cv::DMatch(query[e], train[e], 0.0f));
        matches.push_back(&lists[p]);
        for (int e = 0; e < 12; ++e) { Pl[p].val[e] = P_left[12 * p + e]; Pr[p].val[e] = P_right[12 * p + e]; }
    }
    std::vector<unsigned char> good;
    std::vector<PointCloud> clouds;
    const bool all = SfMStereoUtilities::triangulateViewsBatch(buildIntrinsics(K), images, std::vector<int>(left, left + n_pairs),
                                                               std::vector<int>(right, right + n_pairs), matches, Pl, Pr, good, clouds);
    int64_t n = 0;
    for (int p = 0; p < n_pairs; ++p) {
        ok[p] = good[p];
        cloud_ptr[p] = n;
        for (const Point3DInMap& pt : clouds[p]) {
            if (n < cap) {
                points3d[3 * n] = pt.p.x; points3d[3 * n + 1] = pt.p.y; points3d[3 * n + 2] = pt.p.z;
                left_ref[n] = pt.originatingViews.at(left[p]);
                right_ref[n] = pt.originatingViews.at(right[p]);
            }
            ++n;
        }
    }
    cloud_ptr[n_pairs] = n;
    return all ? 1 : 0;
}

namespace {
using namespace sfmtoylib;
PointCloud buildCloud(int n, const float* xyz, const int64_t* view_ptr, const int32_t* view_idx, const int32_t* feat_idx) {
    PointCloud cloud((size_t)n);
    for (int i = 0; i < n; ++i) {
        cloud[i].p = cv::Point3f(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        for (int64_t q = view_ptr[i]; q < view_ptr[i + 1]; ++q) cloud[i].originatingViews[view_idx[q]] = feat_idx[q];
    }
    return cloud;
}
MatchMatrix buildMatchMatrix(int n_views, int n_pairs, const int32_t* left, const int32_t* right, const int64_t* ptr, const int32_t* query,
                             const int32_t* train, const float* dist) {
    MatchMatrix mm((size_t)n_views, std::vector<Matching>((size_t)n_views));
    for (int p = 0; p < n_pairs; ++p)
        for (int64_t e = ptr[p]; e < ptr[p + 1]; ++e) mm[left[p]][right[p]].push_back(cv::DMatch(query[e], train[e], dist ? dist[e] : 0.0f));
    return mm;
}
}  // namespace

// Flat-array driver of sfmtoylib::SfMAssociation::find2D3DMatches (tests/test_gpu_association.py).  Returns the total number of
// 2D-3D pairs (entries beyond cap are not written), -1 if a not-done view has no entry in the result.
extern "C" __attribute__((visibility("default")))
int64_t sfmba_shim_find_2d3d(int n_views, const unsigned char* done, int n_pt, const float* xyz, const int64_t* view_ptr, const int32_t* view_idx,
                             const int32_t* feat_idx, int n_pairs, const int32_t* left, const int32_t* right, const int64_t* pair_ptr,
                             const int32_t* query, const int32_t* train, const int64_t* feat_ptr, const float* feat_xy,
                             int64_t* out_ptr /*[n_views+1]*/, float* out_2d /*[cap][2]*/, float* out_3d /*[cap][3]*/, int64_t cap) {
    using namespace sfmtoylib;
    const PointCloud cloud = buildCloud(n_pt, xyz, view_ptr, view_idx, feat_idx);
    const MatchMatrix mm = buildMatchMatrix(n_views, n_pairs, left, right, pair_ptr, query, train, nullptr);
    std::vector<Features> feats((size_t)n_views);
    for (int v = 0; v < n_views; ++v)
        for (int64_t f = feat_ptr[v]; f < feat_ptr[v + 1]; ++f) feats[v].points.push_back(cv::Point2f(feat_xy[2 * f], feat_xy[2 * f + 1]));
    std::set<int> doneViews;
    for (int v = 0; v < n_views; ++v) if (done[v]) doneViews.insert(v);
    const Images2D3DMatches res = SfMAssociation::find2D3DMatches((size_t)n_views, doneViews, cloud, mm, feats);
    int64_t n = 0;
    for (int v = 0; v < n_views; ++v) {
        out_ptr[v] = n;
        const auto it = res.find(v);
        if (done[v]) { if (it != res.end()) return -1; continue; }
        if (it == res.end()) return -1;
        for (size_t e = 0; e < it->second.points2D.size(); ++e, ++n) {
            if (n >= cap) continue;
            out_2d[2 * n] = it->second.points2D[e].x; out_2d[2 * n + 1] = it->second.points2D[e].y;
            out_3d[3 * n] = it->second.points3D[e].x; out_3d[3 * n + 1] = it->second.points3D[e].y; out_3d[3 * n + 2] = it->second.points3D[e].z;
        }
    }
    out_ptr[n_views] = n;
    return n;
}

// Flat-array driver of sfmtoylib::SfMAssociation::mergeNewPointCloud.  The merged reconstruction cloud comes back flattened
// (out_n points, views CSR); counts[0..1] = new / merged points; merge_pairs = (left, right, query, train) of the matches pushed to
// the merge match matrix, row-major over the matrix.  Returns 0, -1 on device failure, -2 if an output capacity is too small.
// sfmba_shim_merge_ex takes the feature-match distance below which a match confirms; sfmba_shim_merge is the default (20).
extern "C" __attribute__((visibility("default")))
int sfmba_shim_merge_ex(int n_views, int n_exist, const float* ex_xyz, const int64_t* ex_view_ptr, const int32_t* ex_view_idx, const int32_t* ex_feat_idx,
                        int n_new, const float* nw_xyz, const int64_t* nw_view_ptr, const int32_t* nw_view_idx, const int32_t* nw_feat_idx,
                        int n_pairs, const int32_t* left, const int32_t* right, const int64_t* pair_ptr, const int32_t* query, const int32_t* train,
                        const float* dist, int cap_pts, int64_t cap_views, int* out_n, float* out_xyz, int64_t* out_view_ptr, int32_t* out_view_idx,
                        int32_t* out_feat_idx, int64_t* counts, int64_t cap_merge, int32_t* merge_pairs /*[cap_merge][4]*/, int64_t* n_merge,
                        float max_feature_match_distance) {
    using namespace sfmtoylib;
    PointCloud recon = buildCloud(n_exist, ex_xyz, ex_view_ptr, ex_view_idx, ex_feat_idx);
    const PointCloud fresh = buildCloud(n_new, nw_xyz, nw_view_ptr, nw_view_idx, nw_feat_idx);
    const MatchMatrix mm = buildMatchMatrix(n_views, n_pairs, left, right, pair_ptr, query, train, dist);
    MatchMatrix merged;
    size_t np = 0, nm = 0;
    if (!SfMAssociation::mergeNewPointCloud(recon, fresh, mm, &merged, &np, &nm, max_feature_match_distance)) return -1;
    counts[0] = (int64_t)np; counts[1] = (int64_t)nm;
    if ((int)recon.size() > cap_pts) return -2;
    *out_n = (int)recon.size();
    int64_t o = 0;
    for (size_t i = 0; i < recon.size(); ++i) {
        out_xyz[3 * i] = recon[i].p.x; out_xyz[3 * i + 1] = recon[i].p.y; out_xyz[3 * i + 2] = recon[i].p.z;
        out_view_ptr[i] = o;
        for (const auto& kv : recon[i].originatingViews) { if (o >= cap_views) return -2; out_view_idx[o] = kv.first; out_feat_idx[o] = kv.second; ++o; }
    }
    out_view_ptr[recon.size()] = o;
    int64_t m = 0;
    for (size_t l = 0; l < merged.size(); ++l)
        for (size_t r = 0; r < merged[l].size(); ++r)
            for (const cv::DMatch& d : merged[l][r]) {
                if (m < cap_merge) { merge_pairs[4 * m] = (int32_t)l; merge_pairs[4 * m + 1] = (int32_t)r; merge_pairs[4 * m + 2] = d.queryIdx; merge_pairs[4 * m + 3] = d.trainIdx; }
                ++m;
            }
    *n_merge = m;
    return 0;
}

extern "C" __attribute__((visibility("default")))
int sfmba_shim_merge(int n_views, int n_exist, const float* ex_xyz, const int64_t* ex_view_ptr, const int32_t* ex_view_idx, const int32_t* ex_feat_idx,
                     int n_new, const float* nw_xyz, const int64_t* nw_view_ptr, const int32_t* nw_view_idx, const int32_t* nw_feat_idx,
                     int n_pairs, const int32_t* left, const int32_t* right, const int64_t* pair_ptr, const int32_t* query, const int32_t* train,
                     const float* dist, int cap_pts, int64_t cap_views, int* out_n, float* out_xyz, int64_t* out_view_ptr, int32_t* out_view_idx,
                     int32_t* out_feat_idx, int64_t* counts, int64_t cap_merge, int32_t* merge_pairs /*[cap_merge][4]*/, int64_t* n_merge) {
    return sfmba_shim_merge_ex(n_views, n_exist, ex_xyz, ex_view_ptr, ex_view_idx, ex_feat_idx, n_new, nw_xyz, nw_view_ptr, nw_view_idx, nw_feat_idx,
                               n_pairs, left, right, pair_ptr, query, train, dist, cap_pts, cap_views, out_n, out_xyz, out_view_ptr, out_view_idx,
                               out_feat_idx, counts, cap_merge, merge_pairs, n_merge, 20.0f);
}

// Flat-array driver of sfmtoylib::SfMExport::saveCloudAndCamerasToPLY (tests/test_ply_export.py).  images: n_views images of
// img_rows x img_cols BGR bytes, concatenated.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_save_ply(const char* prefix, int n_views, const float* poses /*[n_views][12]*/, int n_pt, const float* xyz, const int64_t* view_ptr,
                        const int32_t* view_idx, const int32_t* feat_idx, const int64_t* feat_ptr, const float* feat_xy, int img_rows, int img_cols,
                        const unsigned char* images) {
    using namespace sfmtoylib;
    const PointCloud cloud = buildCloud(n_pt, xyz, view_ptr, view_idx, feat_idx);
    std::vector<cv::Matx34f> cams((size_t)n_views);
    for (int v = 0; v < n_views; ++v) for (int e = 0; e < 12; ++e) cams[v].val[e] = poses[12 * v + e];
    std::vector<Features> feats((size_t)n_views);
    std::vector<ImageBGR> imgs((size_t)n_views);
    for (int v = 0; v < n_views; ++v) {
        for (int64_t f = feat_ptr[v]; f < feat_ptr[v + 1]; ++f) feats[v].points.push_back(cv::Point2f(feat_xy[2 * f], feat_xy[2 * f + 1]));
#ifndef SFMBA_HAVE_OPENCV
        imgs[v].rows = img_rows; imgs[v].cols = img_cols;
        imgs[v].data.assign(images + (size_t)v * img_rows * img_cols * 3, images + (size_t)(v + 1) * img_rows * img_cols * 3);
#endif
    }
    return SfMExport::saveCloudAndCamerasToPLY(prefix, cloud, cams, feats, imgs) ? 0 : -1;
}

namespace {
std::vector<Features> buildDescriptors(int n_images, const int64_t* img_ptr, const unsigned char* desc, int desc_bytes) {
    std::vector<Features> feats((size_t)n_images);
    for (int i = 0; i < n_images; ++i) {
        const int rows = (int)(img_ptr[i + 1] - img_ptr[i]);
        if (rows == 0) continue;                                  // an image without key points: an empty matrix
        feats[i].descriptors = cv::Mat(rows, desc_bytes, CV_8U);
        for (int r = 0; r < rows; ++r)
            for (int b = 0; b < desc_bytes; ++b) feats[i].descriptors.at<unsigned char>(r, b) = desc[(size_t)(img_ptr[i] + r) * desc_bytes + b];
    }
    return feats;
}
std::vector<Features> buildFloatDescriptors(int n_images, const int64_t* img_ptr, const float* desc, int dims) {
    std::vector<Features> feats((size_t)n_images);
    for (int i = 0; i < n_images; ++i) {
        const int rows = (int)(img_ptr[i + 1] - img_ptr[i]);
        if (rows == 0) continue;                                  // an image without key points: an empty matrix
        feats[i].descriptors = cv::Mat(rows, dims, CV_32F);
        for (int r = 0; r < rows; ++r) std::memcpy(feats[i].descriptors.ptr<float>(r), desc + (size_t)(img_ptr[i] + r) * dims, sizeof(float) * (size_t)dims);
    }
    return feats;
}
int64_t flattenMatching(const Matching& m, int64_t at, int64_t cap, int32_t* query, int32_t* train, int32_t* img, float* dist) {
    for (const cv::DMatch& d : m) {
        if (at < cap) { query[at] = d.queryIdx; train[at] = d.trainIdx; img[at] = d.imgIdx; dist[at] = d.distance; }
        ++at;
    }
    return at;
}
// createFeatureMatchMatrix flattened: sizes [n_images * n_images] (row-major) and the entries in that order; -1 if the call reported
// failure, -2 if the matrix is not n_images x n_images
int64_t flattenMatchMatrix(const std::vector<sfmtoylib::Features>& feats, int n_images, int64_t* sizes, int64_t cap, int32_t* query, int32_t* train,
                           int32_t* img_idx, float* dist) {
    using namespace sfmtoylib;
    MatchMatrix mm;
    if (!SfMFeatureMatching::createFeatureMatchMatrix(feats, mm)) return -1;
    if (mm.size() != (size_t)n_images) return -2;
    int64_t n = 0;
    for (int l = 0; l < n_images; ++l) {
        if (mm[l].size() != (size_t)n_images) return -2;
        for (int r = 0; r < n_images; ++r) {
            sizes[(size_t)l * n_images + r] = (int64_t)mm[l][r].size();
            n = flattenMatching(mm[l][r], n, cap, query, train, img_idx, dist);
        }
    }
    return n;
}
}  // namespace

// Flat-array driver of sfmtoylib::SfM2DFeatureUtilities::matchFeatures (tests/test_gpu_feature_match.py): image 0 of the
// descriptor CSR is the left one, image 1 the right one.  Returns the number of matches (entries beyond cap are not written).
extern "C" __attribute__((visibility("default")))
int64_t sfmba_shim_match_features(const int64_t* img_ptr /*[3]*/, const unsigned char* desc, int desc_bytes, int64_t cap, int32_t* query,
                                  int32_t* train, int32_t* img_idx, float* dist) {
    using namespace sfmtoylib;
    const std::vector<Features> feats = buildDescriptors(2, img_ptr, desc, desc_bytes);
    return flattenMatching(SfM2DFeatureUtilities::matchFeatures(feats[0], feats[1]), 0, cap, query, train, img_idx, dist);
}

// Flat-array driver of sfmtoylib::SfMFeatureMatching::createFeatureMatchMatrix.  sizes [n_images * n_images] receives the length
// of every entry [l][r] (row-major), the entries are flattened in that order.  Returns the number of matches, -1 if the call
// reported failure, -2 if the matrix is not n_images x n_images.
extern "C" __attribute__((visibility("default")))
int64_t sfmba_shim_feature_match_matrix(int n_images, const int64_t* img_ptr, const unsigned char* desc, int desc_bytes, int64_t* sizes,
                                        int64_t cap, int32_t* query, int32_t* train, int32_t* img_idx, float* dist) {
    using namespace sfmtoylib;
    return flattenMatchMatrix(buildDescriptors(n_images, img_ptr, desc, desc_bytes), n_images, sizes, cap, query, train, img_idx, dist);
}

// The same two drivers for CV_32F descriptors of `dims` columns (tests/test_gpu_match_l2.py).
extern "C" __attribute__((visibility("default")))
int64_t sfmba_shim_match_features_f32(const int64_t* img_ptr /*[3]*/, const float* desc, int dims, int64_t cap, int32_t* query, int32_t* train,
                                      int32_t* img_idx, float* dist) {
    using namespace sfmtoylib;
    const std::vector<Features> feats = buildFloatDescriptors(2, img_ptr, desc, dims);
    return flattenMatching(SfM2DFeatureUtilities::matchFeatures(feats[0], feats[1]), 0, cap, query, train, img_idx, dist);
}

extern "C" __attribute__((visibility("default")))
int64_t sfmba_shim_feature_match_matrix_f32(int n_images, const int64_t* img_ptr, const float* desc, int dims, int64_t* sizes, int64_t cap,
                                            int32_t* query, int32_t* train, int32_t* img_idx, float* dist) {
    return flattenMatchMatrix(buildFloatDescriptors(n_images, img_ptr, desc, dims), n_images, sizes, cap, query, train, img_idx, dist);
}

// createFeatureMatchMatrix over images whose descriptor matrices are of BOTH kinds: image i has rows[i] rows, CV_32F where is_f32[i],
// CV_8U otherwise (all zero, 32 columns).  The shim must refuse before any device call (tests/test_match_l2_oracle_cpu.py): -1.
extern "C" __attribute__((visibility("default")))
int64_t sfmba_shim_feature_match_matrix_mixed(int n_images, const int32_t* rows, const unsigned char* is_f32) {
    using namespace sfmtoylib;
    std::vector<Features> feats((size_t)n_images);
    for (int i = 0; i < n_images; ++i)
        if (rows[i] > 0) feats[i].descriptors = cv::Mat(rows[i], 32, is_f32[i] ? CV_32F : CV_8U);
    MatchMatrix mm;
    return SfMFeatureMatching::createFeatureMatchMatrix(feats, mm) ? 0 : -1;
}

// Flat-array driver of sfmtoylib::SfMFeatureMatching::sortViewsForBaseline: the map comes back in key order as keys [cap] and
// pairs [cap][2] (left, right).  Returns the number of map entries (entries beyond cap are not written).
extern "C" __attribute__((visibility("default")))
int sfmba_shim_sort_views_for_baseline(int n_images, const int64_t* img_ptr, const float* xy, int n_pairs, const int32_t* left, const int32_t* right,
                                       const int64_t* pair_ptr, const int32_t* query, const int32_t* train, int cap, float* keys, int32_t* pairs) {
    using namespace sfmtoylib;
    const std::vector<Features> feats = buildKeyPoints(n_images, img_ptr, xy);
    const MatchMatrix mm = buildMatchMatrix(n_images, n_pairs, left, right, pair_ptr, query, train, nullptr);
    const std::map<float, ImagePair> sorted = SfMFeatureMatching::sortViewsForBaseline(feats, mm);
    int n = 0;
    for (const auto& kv : sorted) {
        if (n < cap) { keys[n] = kv.first; pairs[2 * n] = (int32_t)kv.second.left; pairs[2 * n + 1] = (int32_t)kv.second.right; }
        ++n;
    }
    return n;
}

namespace {
cv::Mat buildImage(int w, int h, int channels, const unsigned char* px) {
    cv::Mat m(h, w, channels == 3 ? CV_8UC3 : CV_8U);
    for (int r = 0; r < h; ++r) std::memcpy(m.ptr<unsigned char>(r), px + (size_t)r * w * channels, (size_t)w * channels);
    return m;
}
// kp [cap][7] = pt.x pt.y size angle response octave class_id, points [cap][2], desc [cap][32]; -2 if the members disagree
int64_t flattenFeatures(const sfmtoylib::Features& f, int64_t at, int64_t cap, float* kp, float* points, unsigned char* desc) {
    const size_t n = f.keyPoints.size();
    if (f.points.size() != n || (n > 0 && (f.descriptors.rows != (int)n || f.descriptors.cols != 32 || f.descriptors.type() != CV_8U))) return -2;
    if (n == 0 && !f.descriptors.empty()) return -2;
    for (size_t r = 0; r < n; ++r, ++at) {
        if (at >= cap) continue;
        const cv::KeyPoint& k = f.keyPoints[r];
        float* o = kp + 7 * at;
        o[0] = k.pt.x; o[1] = k.pt.y; o[2] = k.size; o[3] = k.angle; o[4] = k.response; o[5] = (float)k.octave; o[6] = (float)k.class_id;
        points[2 * at] = f.points[r].x; points[2 * at + 1] = f.points[r].y;
        std::memcpy(desc + 32 * at, f.descriptors.ptr<unsigned char>((int)r), 32);
    }
    return at;
}
}  // namespace

// Flat-array driver of sfmtoylib::SfM2DFeatureUtilities::extractFeatures (tests/test_gpu_orb_extract.py): one w x h image of 1 (gray)
// or 3 (BGR) channels, rows tight.  Returns the number of key points (rows beyond cap are not written), -2 if the members of the
// Features disagree.
extern "C" __attribute__((visibility("default")))
int64_t sfmba_shim_extract_features(int w, int h, int channels, const unsigned char* px, int64_t cap, float* kp, float* points, unsigned char* desc) {
    using namespace sfmtoylib;
    SfM2DFeatureUtilities util;
    return flattenFeatures(util.extractFeatures(buildImage(w, h, channels, px)), 0, cap, kp, points, desc);
}

// Flat-array driver of sfmtoylib::SfMFeatureExtraction::extractFeatures: image i owns bytes img_ptr[i] .. img_ptr[i+1]-1 of px;
// kp_ptr [n_images + 1] receives the CSR of the flattened rows.  Returns the number of key points, -1 if the call reported failure,
// -2 on an inconsistent result.
extern "C" __attribute__((visibility("default")))
int64_t sfmba_shim_extract_features_batch(int n_images, const int64_t* img_ptr, const unsigned char* px, const int32_t* w, const int32_t* h,
                                          int channels, int64_t* kp_ptr, int64_t cap, float* kp, float* points, unsigned char* desc) {
    using namespace sfmtoylib;
    std::vector<cv::Mat> images;
    for (int i = 0; i < n_images; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
    std::vector<Features> feats;
    if (!SfMFeatureExtraction::extractFeatures(images, feats)) return -1;
    if (feats.size() != (size_t)n_images) return -2;
    int64_t at = 0;
    kp_ptr[0] = 0;
    for (int i = 0; i < n_images; ++i) {
        at = flattenFeatures(feats[(size_t)i], at, cap, kp, points, desc);
        if (at < 0) return -2;
        kp_ptr[i + 1] = at;
    }
    return at;
}

namespace {
// flattenFeatures for the float rows of FEATURES_SURF: desc [cap][64] floats
int64_t flattenFloatFeatures(const sfmtoylib::Features& f, int64_t at, int64_t cap, float* kp, float* points, float* desc) {
    const size_t n = f.keyPoints.size();
    if (f.points.size() != n || (n > 0 && (f.descriptors.rows != (int)n || f.descriptors.cols != 64 || f.descriptors.type() != CV_32F))) return -2;
    if (n == 0 && !f.descriptors.empty()) return -2;
    for (size_t r = 0; r < n; ++r, ++at) {
        if (at >= cap) continue;
        const cv::KeyPoint& k = f.keyPoints[r];
        float* o = kp + 7 * at;
        o[0] = k.pt.x; o[1] = k.pt.y; o[2] = k.size; o[3] = k.angle; o[4] = k.response; o[5] = (float)k.octave; o[6] = (float)k.class_id;
        points[2 * at] = f.points[r].x; points[2 * at + 1] = f.points[r].y;
        std::memcpy(desc + 64 * at, f.descriptors.ptr<unsigned char>((int)r), 64 * sizeof(float));
    }
    return at;
}
}  // namespace

// sfmba_shim_extract_features through extractFeatures(image, FEATURES_SURF) (tests/test_gpu_surf_extract.py): desc [cap][64] floats,
// kp [cap][7] with class_id = the sign of the Laplacian.
extern "C" __attribute__((visibility("default")))
int64_t sfmba_shim_extract_features_surf(int w, int h, int channels, const unsigned char* px, int64_t cap, float* kp, float* points, float* desc) {
    using namespace sfmtoylib;
    SfM2DFeatureUtilities util;
    return flattenFloatFeatures(util.extractFeatures(buildImage(w, h, channels, px), FEATURES_SURF), 0, cap, kp, points, desc);
}

// sfmba_shim_extract_features_batch through extractFeatures(images, imageFeatures, FEATURES_SURF).
extern "C" __attribute__((visibility("default")))
int64_t sfmba_shim_extract_features_surf_batch(int n_images, const int64_t* img_ptr, const unsigned char* px, const int32_t* w, const int32_t* h,
                                               int channels, int64_t* kp_ptr, int64_t cap, float* kp, float* points, float* desc) {
    using namespace sfmtoylib;
    std::vector<cv::Mat> images;
    for (int i = 0; i < n_images; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
    std::vector<Features> feats;
    if (!SfMFeatureExtraction::extractFeatures(images, feats, FEATURES_SURF)) return -1;
    if (feats.size() != (size_t)n_images) return -2;
    int64_t at = 0;
    kp_ptr[0] = 0;
    for (int i = 0; i < n_images; ++i) {
        at = flattenFloatFeatures(feats[(size_t)i], at, cap, kp, points, desc);
        if (at < 0) return -2;
        kp_ptr[i + 1] = at;
    }
    return at;
}

namespace {
// the key points (+ points) of view v: rows kp_ptr[v] .. kp_ptr[v+1]-1 of kp_xy [..][2]
void addKeyPoints(std::vector<sfmtoylib::Features>& feats, const int64_t* kp_ptr, const float* kp_xy) {
    for (size_t v = 0; v < feats.size(); ++v)
        for (int64_t f = kp_ptr[v]; f < kp_ptr[v + 1]; ++f) {
            cv::KeyPoint kp; kp.pt = cv::Point2f(kp_xy[2 * f], kp_xy[2 * f + 1]);
            feats[v].keyPoints.push_back(kp); feats[v].points.push_back(kp.pt);
        }
}
// What a finished run leaves, flattened as sfmba_shim_run_sfm documents it.
int flattenRun(sfmtoylib::SfM& sfm, sfmtoylib::ErrorCode code, int n_views, float* poses, float* K, unsigned char* done, unsigned char* good, int* n_added,
               int32_t* added_view, unsigned char* added_posed, int64_t* added_cloud, int64_t cap_pts, int64_t cap_views, int64_t* n_pts, float* xyz,
               int64_t* view_ptr, int32_t* view_idx, int32_t* feat_idx, const char* ply_prefix) {
    using namespace sfmtoylib;
    *n_added = 0;
    *n_pts = 0;
    if (code != OKAY) return (int)code;
    for (int v = 0; v < n_views; ++v) {
        for (int e = 0; e < 12; ++e) poses[12 * v + e] = sfm.getCameraPoses()[v].val[e];
        done[v] = sfm.getDoneViews().count(v) ? 1 : 0;
        good[v] = sfm.getGoodViews().count(v) ? 1 : 0;
    }
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) K[3 * r + c] = sfm.getIntrinsics().K.at<float>(r, c);
    for (const SfM::AddedView& a : sfm.getAddedViews()) {
        if (*n_added >= n_views) return -2;
        added_view[*n_added] = a.view; added_posed[*n_added] = a.posed ? 1 : 0; added_cloud[*n_added] = (int64_t)a.cloudSize;
        ++*n_added;
    }
    const PointCloud& cloud = sfm.getPointCloud();
    if ((int64_t)cloud.size() > cap_pts) return -2;
    *n_pts = (int64_t)cloud.size();
    int64_t o = 0;
    for (size_t i = 0; i < cloud.size(); ++i) {
        xyz[3 * i] = cloud[i].p.x; xyz[3 * i + 1] = cloud[i].p.y; xyz[3 * i + 2] = cloud[i].p.z;
        view_ptr[i] = o;
        for (const auto& kv : cloud[i].originatingViews) { if (o >= cap_views) return -2; view_idx[o] = kv.first; feat_idx[o] = kv.second; ++o; }
    }
    view_ptr[cloud.size()] = o;
    if (ply_prefix && !sfm.saveCloudAndCamerasToPLY(ply_prefix)) return -3;
    return 0;
}
}  // namespace

// Flat-array driver of sfmtoylib::SfM (tests/test_gpu_sfm_pipeline.py): one run from images (channels = 1 or 3: image i owns bytes
// img_ptr[i] .. img_ptr[i+1]-1 of px, w / h per image) or from features (channels = 0: view i owns rows kp_ptr[i] .. kp_ptr[i+1]-1 of
// kp_xy [..][2] and desc [..][32]; cols / rows = the image size).  Back come the poses [n_views][12], K [9], the done / good flags
// [n_views], the turns of the add-more-views loop (added_view / added_posed / added_cloud [n_views], *n_added of them) and the
// cloud flattened with its views CSR.  ply_prefix != NULL: saveCloudAndCamerasToPLY(ply_prefix) after the run.
// Returns runSfM's code (0 = OKAY, 1 = ERROR), -2 if an output capacity is too small, -3 if the PLY files could not be written.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm(float downscale, int n_views, int channels, const int64_t* img_ptr, const unsigned char* px, const int32_t* w, const int32_t* h,
                       const int64_t* kp_ptr, const float* kp_xy, const unsigned char* desc, int cols, int rows, int debug_level, float* poses,
                       float* K, unsigned char* done, unsigned char* good, int* n_added, int32_t* added_view, unsigned char* added_posed,
                       int64_t* added_cloud, int64_t cap_pts, int64_t cap_views, int64_t* n_pts, float* xyz, int64_t* view_ptr, int32_t* view_idx,
                       int32_t* feat_idx, const char* ply_prefix) {
    using namespace sfmtoylib;
    SfM sfm(downscale);
    sfm.setConsoleDebugLevel((unsigned)debug_level);
    if (channels == 0) {
        std::vector<Features> feats = buildDescriptors(n_views, kp_ptr, desc, 32);
        addKeyPoints(feats, kp_ptr, kp_xy);
        sfm.setFeatures(feats, cols, rows);
    } else {
        std::vector<cv::Mat> images;
        for (int i = 0; i < n_views; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
        sfm.setImages(images);
    }
    return flattenRun(sfm, sfm.runSfM(), n_views, poses, K, done, good, n_added, added_view, added_posed, added_cloud, cap_pts, cap_views, n_pts, xyz,
                      view_ptr, view_idx, feat_idx, ply_prefix);
}

// sfmba_shim_run_sfm from features with CV_32F descriptors of `dims` columns (desc [..][dims]) and the merge distance of
// SfM::setMergeFeatureMatchDistance (tests/test_gpu_match_l2_pipeline.py).  Outputs and return value as sfmba_shim_run_sfm.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm_f32(int n_views, const int64_t* kp_ptr, const float* kp_xy, const float* desc, int dims, float merge_distance, int cols, int rows,
                           int debug_level, float* poses, float* K, unsigned char* done, unsigned char* good, int* n_added, int32_t* added_view,
                           unsigned char* added_posed, int64_t* added_cloud, int64_t cap_pts, int64_t cap_views, int64_t* n_pts, float* xyz,
                           int64_t* view_ptr, int32_t* view_idx, int32_t* feat_idx) {
    using namespace sfmtoylib;
    SfM sfm(1.0f);
    sfm.setConsoleDebugLevel((unsigned)debug_level);
    sfm.setMergeFeatureMatchDistance(merge_distance);
    std::vector<Features> feats = buildFloatDescriptors(n_views, kp_ptr, desc, dims);
    addKeyPoints(feats, kp_ptr, kp_xy);
    sfm.setFeatures(feats, cols, rows);
    return flattenRun(sfm, sfm.runSfM(), n_views, poses, K, done, good, n_added, added_view, added_posed, added_cloud, cap_pts, cap_views, n_pts, xyz,
                      view_ptr, view_idx, feat_idx, nullptr);
}

// sfmba_shim_run_sfm from images with the extractor of SfM::setFeatureType (0 = FEATURES_ORB, 1 = FEATURES_SURF) and the merge
// distance of SfM::setMergeFeatureMatchDistance (tests/test_gpu_surf_pipeline.py).  Outputs and return value as sfmba_shim_run_sfm.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm_typed(int feature_type, float merge_distance, int n_views, int channels, const int64_t* img_ptr, const unsigned char* px,
                             const int32_t* w, const int32_t* h, int debug_level, float* poses, float* K, unsigned char* done, unsigned char* good,
                             int* n_added, int32_t* added_view, unsigned char* added_posed, int64_t* added_cloud, int64_t cap_pts, int64_t cap_views,
                             int64_t* n_pts, float* xyz, int64_t* view_ptr, int32_t* view_idx, int32_t* feat_idx, const char* ply_prefix) {
    using namespace sfmtoylib;
    SfM sfm(1.0f);
    sfm.setConsoleDebugLevel((unsigned)debug_level);
    sfm.setFeatureType((FeatureType)feature_type);
    sfm.setMergeFeatureMatchDistance(merge_distance);
    std::vector<cv::Mat> images;
    for (int i = 0; i < n_views; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
    sfm.setImages(images);
    return flattenRun(sfm, sfm.runSfM(), n_views, poses, K, done, good, n_added, added_view, added_posed, added_cloud, cap_pts, cap_views, n_pts, xyz,
                      view_ptr, view_idx, feat_idx, ply_prefix);
}

// sfmba_shim_run_sfm_typed followed by SfM::densify() with the default DenseParams (tests/test_gpu_depth_pipeline.py).  On top of
// sfmba_shim_run_sfm's outputs: the jobs densify made (*n_jobs of them: job_ref / z_near / z_far [n_views], job_src_ptr [n_views + 1],
// job_src [4 n_views]), has_map [n_views], the depth maps of ALL views one after the other in view order (depth [sum of w h]; zeros
// where a view has none) and the dense cloud (cap_dense rows: dense_xyz [..][3], dense_bgr [..][3], dense_view, dense_pixel).
// ply_prefix != NULL: saveCloudAndCamerasToPLY and saveDenseCloudToPLY.  Returns as sfmba_shim_run_sfm; 10 + densify's code when the
// run was OKAY and densify was not.
// the body of sfmba_shim_run_sfm_dense and sfmba_shim_run_sfm_dense_sgm: `dense` goes to densify; mesh_resolution > 0 also runs
// meshDenseCloud at that resolution and *n_triangles receives its triangle count
static int runDense(const sfmtoylib::DenseParams& dense, int mesh_resolution, int64_t* n_triangles, int feature_type, float merge_distance, int n_views,
                    int channels, const int64_t* img_ptr, const unsigned char* px, const int32_t* w, const int32_t* h, int debug_level, float* poses,
                    float* K, unsigned char* done, unsigned char* good, int* n_added, int32_t* added_view, unsigned char* added_posed,
                    int64_t* added_cloud, int64_t cap_pts, int64_t cap_views, int64_t* n_pts, float* xyz, int64_t* view_ptr, int32_t* view_idx,
                    int32_t* feat_idx, const char* ply_prefix, int* n_jobs, int32_t* job_ref, int64_t* job_src_ptr, int32_t* job_src, float* z_near,
                    float* z_far, unsigned char* has_map, float* depth, int64_t cap_dense, int64_t* n_dense, float* dense_xyz, unsigned char* dense_bgr,
                    int32_t* dense_view, int32_t* dense_pixel) {
    using namespace sfmtoylib;
    SfM sfm(1.0f);
    sfm.setConsoleDebugLevel((unsigned)debug_level);
    sfm.setFeatureType((FeatureType)feature_type);
    sfm.setMergeFeatureMatchDistance(merge_distance);
    std::vector<cv::Mat> images;
    for (int i = 0; i < n_views; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
    sfm.setImages(images);
    *n_jobs = 0;
    *n_dense = 0;
    const int rc = flattenRun(sfm, sfm.runSfM(), n_views, poses, K, done, good, n_added, added_view, added_posed, added_cloud, cap_pts, cap_views, n_pts,
                              xyz, view_ptr, view_idx, feat_idx, ply_prefix);
    if (rc != 0) return rc;
    const ErrorCode code = sfm.densify(dense);
    if (code != OKAY) return 10 + (int)code;
    job_src_ptr[0] = 0;
    for (const DenseJob& j : sfm.getDenseJobs()) {
        const int at = (*n_jobs)++;
        job_ref[at] = j.reference; z_near[at] = j.zNear; z_far[at] = j.zFar;
        job_src_ptr[at + 1] = job_src_ptr[at];
        for (int s : j.sources) job_src[job_src_ptr[at + 1]++] = s;
    }
    size_t at = 0;
    for (int v = 0; v < n_views; ++v) {
        const size_t n = (size_t)w[v] * h[v];
        const cv::Mat& m = sfm.getDepthMaps()[(size_t)v];
        has_map[v] = m.empty() ? 0 : 1;
        if (m.empty()) std::memset(depth + at, 0, n * sizeof(float));
        else std::memcpy(depth + at, m.ptr<float>(0), n * sizeof(float));
        at += n;
    }
    const DenseCloud& cloud = sfm.getDenseCloud();
    *n_dense = (int64_t)cloud.points.size();
    if (*n_dense > cap_dense) return -2;
    for (size_t i = 0; i < cloud.points.size(); ++i) {
        dense_xyz[3 * i] = cloud.points[i].x; dense_xyz[3 * i + 1] = cloud.points[i].y; dense_xyz[3 * i + 2] = cloud.points[i].z;
        for (int k = 0; k < 3; ++k) dense_bgr[3 * i + k] = cloud.bgr[3 * i + k];
        dense_view[i] = cloud.views[i]; dense_pixel[i] = cloud.pixels[i];
    }
    if (ply_prefix && !sfm.saveDenseCloudToPLY(ply_prefix)) return -3;
    if (mesh_resolution > 0) {
        MeshParams mesh;
        mesh.resolution = mesh_resolution;
        const ErrorCode meshed = sfm.meshDenseCloud(mesh);
        if (meshed != OKAY) return 20 + (int)meshed;
        *n_triangles = (int64_t)sfm.getMesh().triangles.size() / 3;
    }
    return 0;
}

extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm_dense(int feature_type, float merge_distance, int n_views, int channels, const int64_t* img_ptr, const unsigned char* px,
                             const int32_t* w, const int32_t* h, int debug_level, float* poses, float* K, unsigned char* done, unsigned char* good,
                             int* n_added, int32_t* added_view, unsigned char* added_posed, int64_t* added_cloud, int64_t cap_pts, int64_t cap_views,
                             int64_t* n_pts, float* xyz, int64_t* view_ptr, int32_t* view_idx, int32_t* feat_idx, const char* ply_prefix, int* n_jobs,
                             int32_t* job_ref, int64_t* job_src_ptr, int32_t* job_src, float* z_near, float* z_far, unsigned char* has_map, float* depth,
                             int64_t cap_dense, int64_t* n_dense, float* dense_xyz, unsigned char* dense_bgr, int32_t* dense_view, int32_t* dense_pixel) {
    return runDense(sfmtoylib::DenseParams(), 0, nullptr, feature_type, merge_distance, n_views, channels, img_ptr, px, w, h, debug_level, poses, K, done,
                    good, n_added, added_view, added_posed, added_cloud, cap_pts, cap_views, n_pts, xyz, view_ptr, view_idx, feat_idx, ply_prefix, n_jobs,
                    job_ref, job_src_ptr, job_src, z_near, z_far, has_map, depth, cap_dense, n_dense, dense_xyz, dense_bgr, dense_view, dense_pixel);
}

// sfmba_shim_run_sfm_dense with the semi-global matching fields of DenseParams set from sgm [6] = sgm (0 / 1), sgmP1, sgmP2, sgmPaths,
// sgmInvalidCost, sgmUniqueness (tests/test_gpu_sgm_pipeline.py); mesh_resolution > 0 also runs meshDenseCloud on the depth maps
// (*n_triangles: the mesh's triangles; 20 + its code when it fails).
extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm_dense_sgm(const int32_t* sgm, int mesh_resolution, int64_t* n_triangles, int feature_type, float merge_distance, int n_views,
                                 int channels, const int64_t* img_ptr, const unsigned char* px, const int32_t* w, const int32_t* h, int debug_level,
                                 float* poses, float* K, unsigned char* done, unsigned char* good, int* n_added, int32_t* added_view,
                                 unsigned char* added_posed, int64_t* added_cloud, int64_t cap_pts, int64_t cap_views, int64_t* n_pts, float* xyz,
                                 int64_t* view_ptr, int32_t* view_idx, int32_t* feat_idx, const char* ply_prefix, int* n_jobs, int32_t* job_ref,
                                 int64_t* job_src_ptr, int32_t* job_src, float* z_near, float* z_far, unsigned char* has_map, float* depth,
                                 int64_t cap_dense, int64_t* n_dense, float* dense_xyz, unsigned char* dense_bgr, int32_t* dense_view,
                                 int32_t* dense_pixel) {
    sfmtoylib::DenseParams dense;
    dense.sgm = sgm[0] != 0;
    dense.sgmP1 = sgm[1]; dense.sgmP2 = sgm[2]; dense.sgmPaths = sgm[3]; dense.sgmInvalidCost = sgm[4]; dense.sgmUniqueness = sgm[5];
    *n_triangles = 0;
    return runDense(dense, mesh_resolution, n_triangles, feature_type, merge_distance, n_views, channels, img_ptr, px, w, h, debug_level, poses, K, done,
                    good, n_added, added_view, added_posed, added_cloud, cap_pts, cap_views, n_pts, xyz, view_ptr, view_idx, feat_idx, ply_prefix, n_jobs,
                    job_ref, job_src_ptr, job_src, z_near, z_far, has_map, depth, cap_dense, n_dense, dense_xyz, dense_bgr, dense_view, dense_pixel);
}

// setImages, runSfM, densify() and mergeDenseCloud(voxel, min_count, max_rel_step) in one call (tests/test_gpu_cloud_pipeline.py).
// Back come the poses [n_views][12], K [9], the jobs densify made (*n_jobs of them: job_ref / z_near / z_far [n_views], job_src_ptr
// [n_views + 1], job_src [4 n_views]),
// has_map [n_views], the depth maps of ALL views in view order (depth [sum of w h]; zeros where a view has none), the dense cloud as
// it stands AFTER the merge (cap_dense rows) with *dense_unchanged = 1 iff it equals, byte for byte, the copy taken before the merge,
// and the merged cloud (cap_dense rows: merged_xyz / merged_normal [..][3] floats, merged_bgr [..][3], merged_count, merged_first;
// *voxel_used, *n_skipped).  ply_prefix != NULL: all four PLY files.  Returns runSfM's code, 10 + densify's code, 20 +
// mergeDenseCloud's code, -2 if a capacity is too small, -3 if a PLY file could not be written.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm_merged(int n_views, int channels, const int64_t* img_ptr, const unsigned char* px, const int32_t* w, const int32_t* h,
                              int debug_level, float voxel, int min_count, float max_rel_step, const char* ply_prefix, float* poses, float* K, int* n_jobs,
                              int32_t* job_ref, int64_t* job_src_ptr, int32_t* job_src, float* z_near, float* z_far, unsigned char* has_map, float* depth, int64_t cap_dense, int64_t* n_dense, float* dense_xyz,
                              unsigned char* dense_bgr, int32_t* dense_view, int32_t* dense_pixel, int* dense_unchanged, int64_t* n_merged,
                              float* merged_xyz, unsigned char* merged_bgr, float* merged_normal, int32_t* merged_count, int32_t* merged_first,
                              float* voxel_used, int64_t* n_skipped) {
    using namespace sfmtoylib;
    SfM sfm(1.0f);
    sfm.setConsoleDebugLevel((unsigned)debug_level);
    std::vector<cv::Mat> images;
    for (int i = 0; i < n_views; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
    sfm.setImages(images);
    *n_jobs = 0; *n_dense = 0; *n_merged = 0; *dense_unchanged = 0; *n_skipped = 0; *voxel_used = 0.0f;
    ErrorCode code = sfm.runSfM();
    if (code != OKAY) return (int)code;
    for (int v = 0; v < n_views; ++v)
        for (int e = 0; e < 12; ++e) poses[12 * v + e] = sfm.getCameraPoses()[v].val[e];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) K[3 * r + c] = sfm.getIntrinsics().K.at<float>(r, c);
    if (ply_prefix && !sfm.saveCloudAndCamerasToPLY(ply_prefix)) return -3;
    if ((code = sfm.densify()) != OKAY) return 10 + (int)code;
    job_src_ptr[0] = 0;
    for (const DenseJob& j : sfm.getDenseJobs()) {
        const int at = (*n_jobs)++;
        job_ref[at] = j.reference; z_near[at] = j.zNear; z_far[at] = j.zFar;
        job_src_ptr[at + 1] = job_src_ptr[at];
        for (int s : j.sources) job_src[job_src_ptr[at + 1]++] = s;
    }
    const DenseCloud before = sfm.getDenseCloud();
    if ((code = sfm.mergeDenseCloud(voxel, min_count, max_rel_step)) != OKAY) return 20 + (int)code;
    size_t at = 0;
    for (int v = 0; v < n_views; ++v) {
        const size_t n = (size_t)w[v] * h[v];
        const cv::Mat& m = sfm.getDepthMaps()[(size_t)v];
        has_map[v] = m.empty() ? 0 : 1;
        if (m.empty()) std::memset(depth + at, 0, n * sizeof(float));
        else std::memcpy(depth + at, m.ptr<float>(0), n * sizeof(float));
        at += n;
    }
    const DenseCloud& cloud = sfm.getDenseCloud();
    const MergedCloud& merged = sfm.getMergedDenseCloud();
    *n_dense = (int64_t)cloud.points.size();
    *n_merged = (int64_t)merged.points.size();
    if (*n_dense > cap_dense || *n_merged > cap_dense) return -2;
    bool same = cloud.points.size() == before.points.size() && cloud.bgr == before.bgr && cloud.views == before.views && cloud.pixels == before.pixels;
    for (size_t i = 0; i < cloud.points.size(); ++i) {
        dense_xyz[3 * i] = cloud.points[i].x; dense_xyz[3 * i + 1] = cloud.points[i].y; dense_xyz[3 * i + 2] = cloud.points[i].z;
        for (int k = 0; k < 3; ++k) dense_bgr[3 * i + k] = cloud.bgr[3 * i + k];
        dense_view[i] = cloud.views[i]; dense_pixel[i] = cloud.pixels[i];
        same = same && std::memcmp(&cloud.points[i], &before.points[i], sizeof(cv::Point3f)) == 0;
    }
    *dense_unchanged = same ? 1 : 0;
    for (size_t i = 0; i < merged.points.size(); ++i) {
        merged_xyz[3 * i] = merged.points[i].x; merged_xyz[3 * i + 1] = merged.points[i].y; merged_xyz[3 * i + 2] = merged.points[i].z;
        merged_normal[3 * i] = merged.normals[i].x; merged_normal[3 * i + 1] = merged.normals[i].y; merged_normal[3 * i + 2] = merged.normals[i].z;
        for (int k = 0; k < 3; ++k) merged_bgr[3 * i + k] = merged.bgr[3 * i + k];
        merged_count[i] = merged.counts[i]; merged_first[i] = merged.first[i];
    }
    *voxel_used = merged.voxel;
    *n_skipped = (int64_t)merged.skipped;
    if (ply_prefix && (!sfm.saveDenseCloudToPLY(ply_prefix) || !sfm.saveMergedDenseCloudToPLY(ply_prefix))) return -3;
    return 0;
}

// setImages, runSfM, densify() and meshDenseCloud({voxel, resolution, trunc_voxels, min_weight}) in one call
// (tests/test_gpu_mesh_pipeline.py).  Back come the poses [n_views][12], K [9], has_map [n_views], the depth maps of ALL views in view
// order (depth [sum of w h]; zeros where a view has none) and the dense cloud's points (cap_dense rows of dense_xyz), both as they
// stand AFTER the mesh call with *unchanged = 1 iff the dense cloud and every depth map equal, byte for byte, the copies taken before
// it; the grid the class chose (grid [8] floats: origin x y z, voxel, trunc, then nx ny nz as floats) and the mesh (cap_vertices rows of
// mesh_xyz / mesh_bgr, cap_triangles rows of mesh_tri).  ply_prefix != NULL: saveMeshToPLY.  what == 1: no run at all, only
// meshDenseCloud on a fresh object with images (it has to refuse; no device involved).  Returns runSfM's code, 10 + densify's code, 20 + meshDenseCloud's code (120 + it if a refusing call left a mesh behind),
// -2 if a capacity is too small, -3 if the PLY file could not be written.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm_mesh(int what, int n_views, int channels, const int64_t* img_ptr, const unsigned char* px, const int32_t* w, const int32_t* h,
                            int debug_level, float voxel, int resolution, float trunc_voxels, int min_weight, const char* ply_prefix, float* poses,
                            float* K, unsigned char* has_map, float* depth, int64_t cap_dense, int64_t* n_dense, float* dense_xyz, int* unchanged,
                            float* grid, int64_t cap_vertices, int64_t cap_triangles, int64_t* n_vertices, int64_t* n_triangles, float* mesh_xyz,
                            unsigned char* mesh_bgr, int32_t* mesh_tri) {
    using namespace sfmtoylib;
    SfM sfm(1.0f);
    sfm.setConsoleDebugLevel((unsigned)debug_level);
    std::vector<cv::Mat> images;
    for (int i = 0; i < n_views; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
    sfm.setImages(images);
    *n_dense = 0; *unchanged = 0; *n_vertices = 0; *n_triangles = 0;
    MeshParams params;
    params.voxel = voxel; params.resolution = resolution; params.truncVoxels = trunc_voxels; params.minWeight = min_weight;
    ErrorCode code;
    if (what == 1) {
        code = sfm.meshDenseCloud(params);
        return (code == OKAY || !sfm.getMesh().vertices.empty() ? 120 : 20) + (int)code;
    }
    if ((code = sfm.runSfM()) != OKAY) return (int)code;
    for (int v = 0; v < n_views; ++v)
        for (int e = 0; e < 12; ++e) poses[12 * v + e] = sfm.getCameraPoses()[v].val[e];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) K[3 * r + c] = sfm.getIntrinsics().K.at<float>(r, c);
    if ((code = sfm.densify()) != OKAY) return 10 + (int)code;
    const DenseCloud before = sfm.getDenseCloud();
    std::vector<std::vector<float> > mapsBefore;             // a view without a map: empty
    for (const cv::Mat& m : sfm.getDepthMaps())
        mapsBefore.push_back(m.empty() ? std::vector<float>() : std::vector<float>(m.ptr<float>(0), m.ptr<float>(0) + (size_t)m.rows * m.cols));
    code = sfm.meshDenseCloud(params);
    if (code != OKAY) return (!sfm.getMesh().vertices.empty() || !sfm.getMesh().triangles.empty() ? 120 : 20) + (int)code;
    const DenseCloud& cloud = sfm.getDenseCloud();
    bool same = cloud.points.size() == before.points.size() && cloud.bgr == before.bgr && cloud.views == before.views && cloud.pixels == before.pixels &&
                sfm.getDepthMaps().size() == mapsBefore.size();
    size_t at = 0;
    for (int v = 0; v < n_views; ++v) {
        const size_t n = (size_t)w[v] * h[v];
        const cv::Mat& m = sfm.getDepthMaps()[(size_t)v];
        has_map[v] = m.empty() ? 0 : 1;
        if (m.empty()) std::memset(depth + at, 0, n * sizeof(float));
        else std::memcpy(depth + at, m.ptr<float>(0), n * sizeof(float));
        same = same && (m.empty() ? mapsBefore[(size_t)v].empty()
                                  : mapsBefore[(size_t)v].size() == n && std::memcmp(m.ptr<float>(0), mapsBefore[(size_t)v].data(), n * sizeof(float)) == 0);
        at += n;
    }
    const Mesh& mesh = sfm.getMesh();
    *n_dense = (int64_t)cloud.points.size();
    *n_vertices = (int64_t)mesh.vertices.size();
    *n_triangles = (int64_t)(mesh.triangles.size() / 3);
    if (*n_dense > cap_dense || *n_vertices > cap_vertices || *n_triangles > cap_triangles) return -2;
    for (size_t i = 0; i < cloud.points.size(); ++i) {
        dense_xyz[3 * i] = cloud.points[i].x; dense_xyz[3 * i + 1] = cloud.points[i].y; dense_xyz[3 * i + 2] = cloud.points[i].z;
        same = same && std::memcmp(&cloud.points[i], &before.points[i], sizeof(cv::Point3f)) == 0;
    }
    *unchanged = same ? 1 : 0;
    grid[0] = mesh.grid.origin.x; grid[1] = mesh.grid.origin.y; grid[2] = mesh.grid.origin.z; grid[3] = mesh.grid.voxel; grid[4] = mesh.grid.trunc;
    grid[5] = (float)mesh.grid.nx; grid[6] = (float)mesh.grid.ny; grid[7] = (float)mesh.grid.nz;
    for (size_t i = 0; i < mesh.vertices.size(); ++i) {
        mesh_xyz[3 * i] = mesh.vertices[i].x; mesh_xyz[3 * i + 1] = mesh.vertices[i].y; mesh_xyz[3 * i + 2] = mesh.vertices[i].z;
        for (int k = 0; k < 3; ++k) mesh_bgr[3 * i + k] = mesh.bgr[3 * i + k];
    }
    for (size_t i = 0; i < mesh.triangles.size(); ++i) mesh_tri[i] = mesh.triangles[i];
    if (ply_prefix && !sfm.saveMeshToPLY(ply_prefix)) return -3;
    return 0;
}

// setImages, runSfM, densify(), then meshDenseCloud twice -- with fillIterations 0 and with {fill_iterations, fill_min_neighbours} -- and
// cleanMesh() with its defaults on the filled mesh, in one call (tests/test_gpu_tsdf_fill_pipeline.py).  Back come the poses, K, has_map,
// the depth maps and the dense cloud as in sfmba_shim_run_sfm_mesh, with *unchanged = 1 iff the dense cloud and every depth map equal,
// byte for byte, the copies taken before the first mesh call; the grid of the first and of the second call (grid [16]: twice origin x y z,
// voxel, trunc, nx ny nz as floats); the mesh without the fill (mesh0_*, *filled0_size = its filled.size()) and the mesh with it (mesh_*,
// mesh_filled, *filled_size) under the same capacities; *clean_code = cleanMesh's code.  ply_prefix != NULL: saveMeshToPLY of the filled
// mesh.  what == 1: no run at all, only meshDenseCloud with these fill parameters on a fresh object (it has to refuse).  Returns runSfM's
// code, 10 + densify's code, 20 + the first meshDenseCloud's code, 40 + the second's, -2 if a capacity is too small, -3 if the PLY file
// could not be written.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm_mesh_fill(int what, int n_views, int channels, const int64_t* img_ptr, const unsigned char* px, const int32_t* w, const int32_t* h,
                                 int debug_level, int resolution, int min_weight, int fill_iterations, int fill_min_neighbours, const char* ply_prefix,
                                 float* poses, float* K, unsigned char* has_map, float* depth, int64_t cap_dense, int64_t* n_dense, float* dense_xyz,
                                 int* unchanged, float* grid, int64_t cap_vertices, int64_t cap_triangles, int64_t* n_vertices0, int64_t* n_triangles0,
                                 float* mesh0_xyz, unsigned char* mesh0_bgr, int32_t* mesh0_tri, int64_t* filled0_size, int64_t* n_vertices,
                                 int64_t* n_triangles, float* mesh_xyz, unsigned char* mesh_bgr, int32_t* mesh_tri, unsigned char* mesh_filled,
                                 int64_t* filled_size, int* clean_code) {
    using namespace sfmtoylib;
    SfM sfm(1.0f);
    sfm.setConsoleDebugLevel((unsigned)debug_level);
    std::vector<cv::Mat> images;
    for (int i = 0; i < n_views; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
    sfm.setImages(images);
    *n_dense = 0; *unchanged = 0; *n_vertices0 = 0; *n_triangles0 = 0; *n_vertices = 0; *n_triangles = 0; *filled0_size = -1; *filled_size = -1;
    *clean_code = -1;
    MeshParams params;
    params.resolution = resolution; params.minWeight = min_weight;
    MeshParams fill = params;
    fill.fillIterations = fill_iterations; fill.fillMinNeighbours = fill_min_neighbours;
    ErrorCode code;
    if (what == 1) {
        code = sfm.meshDenseCloud(fill);
        return (code == OKAY || !sfm.getMesh().vertices.empty() ? 140 : 40) + (int)code;
    }
    if ((code = sfm.runSfM()) != OKAY) return (int)code;
    for (int v = 0; v < n_views; ++v)
        for (int e = 0; e < 12; ++e) poses[12 * v + e] = sfm.getCameraPoses()[v].val[e];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) K[3 * r + c] = sfm.getIntrinsics().K.at<float>(r, c);
    if ((code = sfm.densify()) != OKAY) return 10 + (int)code;
    const DenseCloud before = sfm.getDenseCloud();
    std::vector<std::vector<float> > mapsBefore;             // a view without a map: empty
    for (const cv::Mat& m : sfm.getDepthMaps())
        mapsBefore.push_back(m.empty() ? std::vector<float>() : std::vector<float>(m.ptr<float>(0), m.ptr<float>(0) + (size_t)m.rows * m.cols));
    auto put = [&](const Mesh& mesh, float* g, int64_t* nv, int64_t* nt, float* xyz, unsigned char* bgr, int32_t* tri) {
        *nv = (int64_t)mesh.vertices.size();
        *nt = (int64_t)(mesh.triangles.size() / 3);
        if (*nv > cap_vertices || *nt > cap_triangles) return false;
        g[0] = mesh.grid.origin.x; g[1] = mesh.grid.origin.y; g[2] = mesh.grid.origin.z; g[3] = mesh.grid.voxel; g[4] = mesh.grid.trunc;
        g[5] = (float)mesh.grid.nx; g[6] = (float)mesh.grid.ny; g[7] = (float)mesh.grid.nz;
        for (size_t i = 0; i < mesh.vertices.size(); ++i) {
            xyz[3 * i] = mesh.vertices[i].x; xyz[3 * i + 1] = mesh.vertices[i].y; xyz[3 * i + 2] = mesh.vertices[i].z;
            for (int k = 0; k < 3; ++k) bgr[3 * i + k] = mesh.bgr[3 * i + k];
        }
        for (size_t i = 0; i < mesh.triangles.size(); ++i) tri[i] = mesh.triangles[i];
        return true;
    };
    if ((code = sfm.meshDenseCloud(params)) != OKAY) return 20 + (int)code;
    *filled0_size = (int64_t)sfm.getMesh().filled.size();
    if (!put(sfm.getMesh(), grid, n_vertices0, n_triangles0, mesh0_xyz, mesh0_bgr, mesh0_tri)) return -2;
    if ((code = sfm.meshDenseCloud(fill)) != OKAY) return 40 + (int)code;
    const Mesh& mesh = sfm.getMesh();
    *filled_size = (int64_t)mesh.filled.size();
    if (!put(mesh, grid + 8, n_vertices, n_triangles, mesh_xyz, mesh_bgr, mesh_tri)) return -2;
    for (size_t i = 0; i < mesh.filled.size() && i < mesh.vertices.size(); ++i) mesh_filled[i] = mesh.filled[i];
    const DenseCloud& cloud = sfm.getDenseCloud();
    bool same = cloud.points.size() == before.points.size() && cloud.bgr == before.bgr && cloud.views == before.views && cloud.pixels == before.pixels &&
                sfm.getDepthMaps().size() == mapsBefore.size();
    size_t at = 0;
    for (int v = 0; v < n_views; ++v) {
        const size_t n = (size_t)w[v] * h[v];
        const cv::Mat& m = sfm.getDepthMaps()[(size_t)v];
        has_map[v] = m.empty() ? 0 : 1;
        if (m.empty()) std::memset(depth + at, 0, n * sizeof(float));
        else std::memcpy(depth + at, m.ptr<float>(0), n * sizeof(float));
        same = same && (m.empty() ? mapsBefore[(size_t)v].empty()
                                  : mapsBefore[(size_t)v].size() == n && std::memcmp(m.ptr<float>(0), mapsBefore[(size_t)v].data(), n * sizeof(float)) == 0);
        at += n;
    }
    *n_dense = (int64_t)cloud.points.size();
    if (*n_dense > cap_dense) return -2;
    for (size_t i = 0; i < cloud.points.size(); ++i) {
        dense_xyz[3 * i] = cloud.points[i].x; dense_xyz[3 * i + 1] = cloud.points[i].y; dense_xyz[3 * i + 2] = cloud.points[i].z;
        same = same && std::memcmp(&cloud.points[i], &before.points[i], sizeof(cv::Point3f)) == 0;
    }
    *unchanged = same ? 1 : 0;
    if (ply_prefix && !sfm.saveMeshToPLY(ply_prefix)) return -3;
    *clean_code = (int)sfm.cleanMesh();
    return 0;
}

// setImages, runSfM, densify(), meshDenseCloud() with its defaults and cleanMesh({min_component, keep_largest, iterations, lambda, mu})
// in one call (tests/test_gpu_mesh_clean_pipeline.py).  Back come the grid the class chose (grid [8], as above), the mesh of
// meshDenseCloud as it stands AFTER cleanMesh (cap_vertices rows of mesh_xyz / mesh_bgr, cap_triangles rows of mesh_tri) and the clean
// mesh (clean_xyz / clean_bgr / clean_normal, clean_tri, under the same capacities), with *unchanged = 1 iff the mesh, the dense cloud
// and every depth map equal, byte for byte, the copies taken before cleanMesh.  ply_prefix != NULL: saveMeshToPLY and
// saveCleanMeshToPLY.  what == 1: no run at all, only cleanMesh on a fresh object with images (it has to refuse; no device involved).
// Returns runSfM's code, 10 + densify's code, 20 + meshDenseCloud's code, 30 + cleanMesh's code (130 + it if a refusing call left a
// clean mesh behind), -2 if a capacity is too small, -3 if a PLY file could not be written.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm_mesh_clean(int what, int n_views, int channels, const int64_t* img_ptr, const unsigned char* px, const int32_t* w,
                                  const int32_t* h, int debug_level, int min_component, int keep_largest, int iterations, float lambda, float mu,
                                  const char* ply_prefix, int* unchanged, float* grid, int64_t cap_vertices, int64_t cap_triangles,
                                  int64_t* n_vertices, int64_t* n_triangles, float* mesh_xyz, unsigned char* mesh_bgr, int32_t* mesh_tri,
                                  int64_t* n_clean_vertices, int64_t* n_clean_triangles, float* clean_xyz, unsigned char* clean_bgr,
                                  float* clean_normal, int32_t* clean_tri) {
    using namespace sfmtoylib;
    SfM sfm(1.0f);
    sfm.setConsoleDebugLevel((unsigned)debug_level);
    std::vector<cv::Mat> images;
    for (int i = 0; i < n_views; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
    sfm.setImages(images);
    *unchanged = 0; *n_vertices = 0; *n_triangles = 0; *n_clean_vertices = 0; *n_clean_triangles = 0;
    MeshCleanParams params;
    params.minComponentTriangles = min_component; params.keepLargest = keep_largest != 0; params.smoothIterations = iterations;
    params.lambda = lambda; params.mu = mu;
    const auto left_behind = [&]() { return !sfm.getCleanMesh().vertices.empty() || !sfm.getCleanMesh().triangles.empty(); };
    ErrorCode code;
    if (what == 1) {
        code = sfm.cleanMesh(params);
        return (code == OKAY || left_behind() ? 130 : 30) + (int)code;
    }
    if ((code = sfm.runSfM()) != OKAY) return (int)code;
    if ((code = sfm.densify()) != OKAY) return 10 + (int)code;
    if ((code = sfm.meshDenseCloud()) != OKAY) return 20 + (int)code;
    const Mesh before = sfm.getMesh();
    const DenseCloud cloudBefore = sfm.getDenseCloud();
    std::vector<std::vector<float> > mapsBefore;             // a view without a map: empty
    for (const cv::Mat& m : sfm.getDepthMaps())
        mapsBefore.push_back(m.empty() ? std::vector<float>() : std::vector<float>(m.ptr<float>(0), m.ptr<float>(0) + (size_t)m.rows * m.cols));
    code = sfm.cleanMesh(params);
    if (code != OKAY) return (left_behind() ? 130 : 30) + (int)code;
    const Mesh& mesh = sfm.getMesh();
    const Mesh& clean = sfm.getCleanMesh();
    const DenseCloud& cloud = sfm.getDenseCloud();
    bool same = mesh.vertices.size() == before.vertices.size() && mesh.bgr == before.bgr && mesh.triangles == before.triangles && mesh.normals.empty() &&
                cloud.points.size() == cloudBefore.points.size() && cloud.bgr == cloudBefore.bgr && sfm.getDepthMaps().size() == mapsBefore.size();
    for (size_t i = 0; same && i < mesh.vertices.size(); ++i) same = std::memcmp(&mesh.vertices[i], &before.vertices[i], sizeof(cv::Point3f)) == 0;
    for (size_t i = 0; same && i < cloud.points.size(); ++i) same = std::memcmp(&cloud.points[i], &cloudBefore.points[i], sizeof(cv::Point3f)) == 0;
    for (size_t v = 0; same && v < mapsBefore.size(); ++v) {
        const cv::Mat& m = sfm.getDepthMaps()[v];
        const size_t n = m.empty() ? 0 : (size_t)m.rows * m.cols;
        same = mapsBefore[v].size() == n && (n == 0 || std::memcmp(m.ptr<float>(0), mapsBefore[v].data(), n * sizeof(float)) == 0);
    }
    *unchanged = same ? 1 : 0;
    *n_vertices = (int64_t)mesh.vertices.size();
    *n_triangles = (int64_t)(mesh.triangles.size() / 3);
    *n_clean_vertices = (int64_t)clean.vertices.size();
    *n_clean_triangles = (int64_t)(clean.triangles.size() / 3);
    if (*n_vertices > cap_vertices || *n_triangles > cap_triangles) return -2;
    if (clean.bgr.size() != 3 * clean.vertices.size() || clean.normals.size() != 3 * clean.vertices.size()) return -4;
    grid[0] = mesh.grid.origin.x; grid[1] = mesh.grid.origin.y; grid[2] = mesh.grid.origin.z; grid[3] = mesh.grid.voxel; grid[4] = mesh.grid.trunc;
    grid[5] = (float)mesh.grid.nx; grid[6] = (float)mesh.grid.ny; grid[7] = (float)mesh.grid.nz;
    for (size_t i = 0; i < mesh.vertices.size(); ++i) {
        mesh_xyz[3 * i] = mesh.vertices[i].x; mesh_xyz[3 * i + 1] = mesh.vertices[i].y; mesh_xyz[3 * i + 2] = mesh.vertices[i].z;
        for (int k = 0; k < 3; ++k) mesh_bgr[3 * i + k] = mesh.bgr[3 * i + k];
    }
    for (size_t i = 0; i < mesh.triangles.size(); ++i) mesh_tri[i] = mesh.triangles[i];
    for (size_t i = 0; i < clean.vertices.size(); ++i) {
        clean_xyz[3 * i] = clean.vertices[i].x; clean_xyz[3 * i + 1] = clean.vertices[i].y; clean_xyz[3 * i + 2] = clean.vertices[i].z;
        for (int k = 0; k < 3; ++k) { clean_bgr[3 * i + k] = clean.bgr[3 * i + k]; clean_normal[3 * i + k] = clean.normals[3 * i + k]; }
    }
    for (size_t i = 0; i < clean.triangles.size(); ++i) clean_tri[i] = clean.triangles[i];
    if (ply_prefix && (!sfm.saveMeshToPLY(ply_prefix) || !sfm.saveCleanMeshToPLY(ply_prefix))) return -3;
    return 0;
}

// setImages, runSfM, densify(), meshDenseCloud() with its defaults, textureMesh({patch}) on the mesh, cleanMesh() with its defaults and
// textureMesh({patch}) again, now on the clean mesh, in one call (tests/test_gpu_texture_pipeline.py).  Back come the poses
// [n_views][12], K [9], has_map [n_views], the depth maps of ALL views in view order (zeros where a view has none), the grid's voxel, the
// mesh and the clean mesh (cap_vertices rows of *_xyz / *_bgr, cap_triangles rows of *_tri) and the two textured meshes, k = 0 on the
// mesh and k = 1 on the clean mesh: atlas_wh [2 k .. 2 k + 1], cap_atlas bytes of atlas at k cap_atlas, cap_triangles rows of uv
// [.][6] and of view at k cap_triangles, textured [k], and same_source [k] = 1 iff its vertices and triangles are those of the mesh it
// was made from.  *unchanged = 1 iff the mesh, the clean mesh, the dense cloud and every depth map equal, byte for byte, the copies
// taken before the texturing calls.  obj_prefix != NULL: saveTexturedMeshToOBJ after the first call, and under obj_prefix + "_clean"
// after the second.  what == 1: no run at all, only textureMesh on a fresh object with images (it has to refuse; no device involved).
// Returns runSfM's code, 10 + densify's code, 20 + meshDenseCloud's code, 30 + cleanMesh's code, 50 + textureMesh's code (150 + it if a
// refusing call left a textured mesh behind), -2 if a capacity is too small, -3 if a file could not be written.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm_texture(int what, int n_views, int channels, const int64_t* img_ptr, const unsigned char* px, const int32_t* w, const int32_t* h,
                               int debug_level, int patch, const char* obj_prefix, float* poses, float* K, unsigned char* has_map, float* depth,
                               float* voxel, int* unchanged, int64_t cap_vertices, int64_t cap_triangles, int64_t* n_vertices, int64_t* n_triangles,
                               float* mesh_xyz, unsigned char* mesh_bgr, int32_t* mesh_tri, int64_t* n_clean_vertices, int64_t* n_clean_triangles,
                               float* clean_xyz, unsigned char* clean_bgr, int32_t* clean_tri, int64_t cap_atlas, int32_t* atlas_wh, unsigned char* atlas,
                               float* uv, int32_t* view, int64_t* textured, int* same_source) {
    using namespace sfmtoylib;
    SfM sfm(1.0f);
    sfm.setConsoleDebugLevel((unsigned)debug_level);
    std::vector<cv::Mat> images;
    for (int i = 0; i < n_views; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
    sfm.setImages(images);
    *unchanged = 0; *n_vertices = 0; *n_triangles = 0; *n_clean_vertices = 0; *n_clean_triangles = 0;
    TextureParams params;
    params.patch = patch;
    const auto left_behind = [&]() { return !sfm.getTexturedMesh().atlas.empty() || !sfm.getTexturedMesh().triangles.empty(); };
    ErrorCode code;
    if (what == 1) {
        code = sfm.textureMesh(params);
        return (code == OKAY || left_behind() ? 150 : 50) + (int)code;
    }
    if ((code = sfm.runSfM()) != OKAY) return (int)code;
    for (int v = 0; v < n_views; ++v)
        for (int e = 0; e < 12; ++e) poses[12 * v + e] = sfm.getCameraPoses()[v].val[e];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) K[3 * r + c] = sfm.getIntrinsics().K.at<float>(r, c);
    if ((code = sfm.densify()) != OKAY) return 10 + (int)code;
    if ((code = sfm.meshDenseCloud()) != OKAY) return 20 + (int)code;
    const auto same_mesh = [](const Mesh& a, const Mesh& b) {
        bool same = a.vertices.size() == b.vertices.size() && a.bgr == b.bgr && a.triangles == b.triangles && a.normals.size() == b.normals.size();
        for (size_t i = 0; same && i < a.vertices.size(); ++i) same = std::memcmp(&a.vertices[i], &b.vertices[i], sizeof(cv::Point3f)) == 0;
        return same && (a.normals.empty() || std::memcmp(a.normals.data(), b.normals.data(), a.normals.size() * sizeof(float)) == 0);
    };
    const auto put_textured = [&](int k, const Mesh& source) {
        const TexturedMesh& t = sfm.getTexturedMesh();
        const int64_t bytes = (int64_t)t.atlas.rows * t.atlas.cols * 3, nt = (int64_t)(t.triangles.size() / 3);
        if (bytes > cap_atlas || nt > cap_triangles || (int64_t)t.uv.size() != 6 * nt || (int64_t)t.view.size() != nt) return false;
        atlas_wh[2 * k] = t.atlas.cols; atlas_wh[2 * k + 1] = t.atlas.rows;
        std::memcpy(atlas + (size_t)k * (size_t)cap_atlas, t.atlas.ptr<unsigned char>(0), (size_t)bytes);
        std::memcpy(uv + (size_t)k * (size_t)cap_triangles * 6, t.uv.data(), t.uv.size() * sizeof(float));
        std::memcpy(view + (size_t)k * (size_t)cap_triangles, t.view.data(), t.view.size() * sizeof(int32_t));
        textured[k] = (int64_t)t.textured;
        bool same = t.triangles == source.triangles && t.vertices.size() == source.vertices.size();
        for (size_t i = 0; same && i < t.vertices.size(); ++i) same = std::memcmp(&t.vertices[i], &source.vertices[i], sizeof(cv::Point3f)) == 0;
        same_source[k] = same ? 1 : 0;
        return true;
    };
    const auto put_mesh = [](const Mesh& m, float* xyz, unsigned char* bgr, int32_t* tri) {
        for (size_t i = 0; i < m.vertices.size(); ++i) {
            xyz[3 * i] = m.vertices[i].x; xyz[3 * i + 1] = m.vertices[i].y; xyz[3 * i + 2] = m.vertices[i].z;
            for (int k = 0; k < 3; ++k) bgr[3 * i + k] = m.bgr[3 * i + k];
        }
        for (size_t i = 0; i < m.triangles.size(); ++i) tri[i] = m.triangles[i];
    };
    const Mesh meshBefore = sfm.getMesh();
    const DenseCloud cloudBefore = sfm.getDenseCloud();
    std::vector<std::vector<float> > mapsBefore;             // a view without a map: empty
    for (const cv::Mat& m : sfm.getDepthMaps())
        mapsBefore.push_back(m.empty() ? std::vector<float>() : std::vector<float>(m.ptr<float>(0), m.ptr<float>(0) + (size_t)m.rows * m.cols));
    *voxel = meshBefore.grid.voxel;
    *n_vertices = (int64_t)meshBefore.vertices.size();
    *n_triangles = (int64_t)(meshBefore.triangles.size() / 3);
    if (*n_vertices > cap_vertices || *n_triangles > cap_triangles || meshBefore.bgr.size() != 3 * meshBefore.vertices.size()) return -2;
    // on the mesh
    code = sfm.textureMesh(params);
    if (code != OKAY) return (left_behind() ? 150 : 50) + (int)code;
    if (!put_textured(0, sfm.getMesh())) return -2;
    if (obj_prefix && !sfm.saveTexturedMeshToOBJ(obj_prefix)) return -3;
    // on the clean mesh
    if ((code = sfm.cleanMesh()) != OKAY) return 30 + (int)code;
    if (left_behind()) return 150;                           // cleanMesh clears what was made from the mesh before it
    const Mesh cleanBefore = sfm.getCleanMesh();
    *n_clean_vertices = (int64_t)cleanBefore.vertices.size();
    *n_clean_triangles = (int64_t)(cleanBefore.triangles.size() / 3);
    if (cleanBefore.bgr.size() != 3 * cleanBefore.vertices.size()) return -2;
    code = sfm.textureMesh(params);
    if (code != OKAY) return (left_behind() ? 150 : 50) + (int)code;
    if (!put_textured(1, sfm.getCleanMesh())) return -2;
    if (obj_prefix && !sfm.saveTexturedMeshToOBJ(std::string(obj_prefix) + "_clean")) return -3;
    // nothing else moved
    const DenseCloud& cloud = sfm.getDenseCloud();
    bool same = same_mesh(sfm.getMesh(), meshBefore) && same_mesh(sfm.getCleanMesh(), cleanBefore) && cloud.points.size() == cloudBefore.points.size() &&
                cloud.bgr == cloudBefore.bgr && sfm.getDepthMaps().size() == mapsBefore.size();
    for (size_t i = 0; same && i < cloud.points.size(); ++i) same = std::memcmp(&cloud.points[i], &cloudBefore.points[i], sizeof(cv::Point3f)) == 0;
    size_t at = 0;
    for (int v = 0; v < n_views; ++v) {
        const size_t n = (size_t)w[v] * h[v];
        const cv::Mat& m = sfm.getDepthMaps()[(size_t)v];
        has_map[v] = m.empty() ? 0 : 1;
        if (m.empty()) std::memset(depth + at, 0, n * sizeof(float));
        else std::memcpy(depth + at, m.ptr<float>(0), n * sizeof(float));
        same = same && (m.empty() ? mapsBefore[(size_t)v].empty()
                                  : mapsBefore[(size_t)v].size() == n && std::memcmp(m.ptr<float>(0), mapsBefore[(size_t)v].data(), n * sizeof(float)) == 0);
        at += n;
    }
    *unchanged = same ? 1 : 0;
    put_mesh(meshBefore, mesh_xyz, mesh_bgr, mesh_tri);
    put_mesh(cleanBefore, clean_xyz, clean_bgr, clean_tri);
    return 0;
}

// setImages, runSfM, densify(), meshDenseCloud() with its defaults, textureMesh({patch}) on the mesh, decimateMesh({cell_voxels, placement,
// reg}) on the mesh, textureMesh({patch}) again, now on the decimated mesh, cleanMesh() with its defaults and decimateMesh again, now on
// the clean mesh, in one call (tests/test_gpu_mesh_decimate_pipeline.py).  Back come the poses [n_views][12], K [9], has_map [n_views],
// the depth maps of ALL views in view order (zeros where a view has none), the grid the class chose (grid [8]: origin, voxel, trunc,
// dims), four meshes under the capacities cap_vertices and cap_triangles -- k = 0 the mesh, 1 the clean mesh, 2 the decimated mesh, 3 the
// decimated clean mesh: counts [2 k .. 2 k + 1], xyz / bgr / normal at k cap_vertices rows, tri at k cap_triangles rows (the mesh has no
// normals: zeros) -- and the two textured meshes as sfmba_shim_run_sfm_texture returns them, k = 0 on the mesh and k = 1 on the decimated
// mesh.  *unchanged = 1 iff the mesh, the clean mesh, the dense cloud and every depth map equal, byte for byte, the copies taken when
// they were made.  ply_prefix != NULL: saveDecimatedMeshToPLY after the first decimateMesh.  what == 1: no run at all, only decimateMesh
// on a fresh object with images (it has to refuse; no device involved).  Returns runSfM's code, 10 + densify's code, 20 +
// meshDenseCloud's code, 30 + cleanMesh's code, 50 + textureMesh's code, 60 + decimateMesh's code (160 + it if a refusing call left a
// decimated mesh behind), 150 if decimateMesh left the textured mesh standing, 170 if cleanMesh left the decimated mesh standing, -2 if
// a capacity is too small, -3 if a file could not be written.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm_mesh_decimate(int what, int n_views, int channels, const int64_t* img_ptr, const unsigned char* px, const int32_t* w,
                                     const int32_t* h, int debug_level, float cell_voxels, int placement, int reg, int patch, const char* ply_prefix,
                                     float* poses, float* K, unsigned char* has_map, float* depth, float* grid, int* unchanged, int64_t cap_vertices,
                                     int64_t cap_triangles, int64_t* counts, float* xyz, unsigned char* bgr, float* normal, int32_t* tri,
                                     int64_t cap_atlas, int32_t* atlas_wh, unsigned char* atlas, float* uv, int32_t* view, int64_t* textured,
                                     int* same_source) {
    using namespace sfmtoylib;
    SfM sfm(1.0f);
    sfm.setConsoleDebugLevel((unsigned)debug_level);
    std::vector<cv::Mat> images;
    for (int i = 0; i < n_views; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
    sfm.setImages(images);
    *unchanged = 0;
    for (int k = 0; k < 8; ++k) counts[k] = 0;
    MeshDecimateParams params;
    params.cellVoxels = cell_voxels; params.placement = placement; params.reg = reg;
    TextureParams texture;
    texture.patch = patch;
    const auto left_behind = [&]() { return !sfm.getDecimatedMesh().vertices.empty() || !sfm.getDecimatedMesh().triangles.empty(); };
    const auto texture_left = [&]() { return !sfm.getTexturedMesh().atlas.empty() || !sfm.getTexturedMesh().triangles.empty(); };
    ErrorCode code;
    if (what == 1) {
        code = sfm.decimateMesh(params);
        return (code == OKAY || left_behind() ? 160 : 60) + (int)code;
    }
    if ((code = sfm.runSfM()) != OKAY) return (int)code;
    for (int v = 0; v < n_views; ++v)
        for (int e = 0; e < 12; ++e) poses[12 * v + e] = sfm.getCameraPoses()[v].val[e];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) K[3 * r + c] = sfm.getIntrinsics().K.at<float>(r, c);
    if ((code = sfm.densify()) != OKAY) return 10 + (int)code;
    if ((code = sfm.meshDenseCloud()) != OKAY) return 20 + (int)code;
    const auto same_mesh = [](const Mesh& a, const Mesh& b) {
        bool same = a.vertices.size() == b.vertices.size() && a.bgr == b.bgr && a.triangles == b.triangles && a.normals.size() == b.normals.size();
        for (size_t i = 0; same && i < a.vertices.size(); ++i) same = std::memcmp(&a.vertices[i], &b.vertices[i], sizeof(cv::Point3f)) == 0;
        return same && (a.normals.empty() || std::memcmp(a.normals.data(), b.normals.data(), a.normals.size() * sizeof(float)) == 0);
    };
    const auto put_mesh = [&](int k, const Mesh& m) {
        const int64_t nv = (int64_t)m.vertices.size(), nt = (int64_t)(m.triangles.size() / 3);
        counts[2 * k] = nv; counts[2 * k + 1] = nt;
        if (nv > cap_vertices || nt > cap_triangles || m.bgr.size() != 3 * m.vertices.size() || (!m.normals.empty() && m.normals.size() != 3 * m.vertices.size()))
            return false;
        float* X = xyz + (size_t)k * (size_t)cap_vertices * 3;
        float* N = normal + (size_t)k * (size_t)cap_vertices * 3;
        unsigned char* C = bgr + (size_t)k * (size_t)cap_vertices * 3;
        for (size_t i = 0; i < m.vertices.size(); ++i) {
            X[3 * i] = m.vertices[i].x; X[3 * i + 1] = m.vertices[i].y; X[3 * i + 2] = m.vertices[i].z;
            for (int q = 0; q < 3; ++q) { C[3 * i + q] = m.bgr[3 * i + q]; N[3 * i + q] = m.normals.empty() ? 0.0f : m.normals[3 * i + q]; }
        }
        std::memcpy(tri + (size_t)k * (size_t)cap_triangles * 3, m.triangles.data(), m.triangles.size() * sizeof(int32_t));
        return true;
    };
    const auto put_textured = [&](int k, const Mesh& source) {
        const TexturedMesh& t = sfm.getTexturedMesh();
        const int64_t bytes = (int64_t)t.atlas.rows * t.atlas.cols * 3, nt = (int64_t)(t.triangles.size() / 3);
        if (bytes > cap_atlas || nt > cap_triangles || (int64_t)t.uv.size() != 6 * nt || (int64_t)t.view.size() != nt) return false;
        atlas_wh[2 * k] = t.atlas.cols; atlas_wh[2 * k + 1] = t.atlas.rows;
        std::memcpy(atlas + (size_t)k * (size_t)cap_atlas, t.atlas.ptr<unsigned char>(0), (size_t)bytes);
        std::memcpy(uv + (size_t)k * (size_t)cap_triangles * 6, t.uv.data(), t.uv.size() * sizeof(float));
        std::memcpy(view + (size_t)k * (size_t)cap_triangles, t.view.data(), t.view.size() * sizeof(int32_t));
        textured[k] = (int64_t)t.textured;
        bool same = t.triangles == source.triangles && t.vertices.size() == source.vertices.size();
        for (size_t i = 0; same && i < t.vertices.size(); ++i) same = std::memcmp(&t.vertices[i], &source.vertices[i], sizeof(cv::Point3f)) == 0;
        same_source[k] = same ? 1 : 0;
        return true;
    };
    const Mesh meshBefore = sfm.getMesh();
    const DenseCloud cloudBefore = sfm.getDenseCloud();
    std::vector<std::vector<float> > mapsBefore;             // a view without a map: empty
    for (const cv::Mat& m : sfm.getDepthMaps())
        mapsBefore.push_back(m.empty() ? std::vector<float>() : std::vector<float>(m.ptr<float>(0), m.ptr<float>(0) + (size_t)m.rows * m.cols));
    const MeshGrid& g = meshBefore.grid;
    grid[0] = g.origin.x; grid[1] = g.origin.y; grid[2] = g.origin.z; grid[3] = g.voxel; grid[4] = g.trunc;
    grid[5] = (float)g.nx; grid[6] = (float)g.ny; grid[7] = (float)g.nz;
    // without decimateMesh: the texture of the mesh
    code = sfm.textureMesh(texture);
    if (code != OKAY) return 50 + (int)code;
    if (!put_textured(0, sfm.getMesh())) return -2;
    // on the mesh
    code = sfm.decimateMesh(params);
    if (code != OKAY) return (left_behind() ? 160 : 60) + (int)code;
    if (texture_left()) return 150;                          // decimateMesh clears what was made from the mesh before it
    if (!put_mesh(2, sfm.getDecimatedMesh())) return -2;
    if (ply_prefix && !sfm.saveDecimatedMeshToPLY(ply_prefix)) return -3;
    code = sfm.textureMesh(texture);
    if (code != OKAY) return 50 + (int)code;
    if (!put_textured(1, sfm.getDecimatedMesh())) return -2;
    // on the clean mesh
    if ((code = sfm.cleanMesh()) != OKAY) return 30 + (int)code;
    if (left_behind()) return 170;                           // cleanMesh clears the decimated mesh
    const Mesh cleanBefore = sfm.getCleanMesh();
    code = sfm.decimateMesh(params);
    if (code != OKAY) return (left_behind() ? 160 : 60) + (int)code;
    if (!put_mesh(3, sfm.getDecimatedMesh())) return -2;
    // nothing else moved
    const DenseCloud& cloud = sfm.getDenseCloud();
    bool same = same_mesh(sfm.getMesh(), meshBefore) && same_mesh(sfm.getCleanMesh(), cleanBefore) && cloud.points.size() == cloudBefore.points.size() &&
                cloud.bgr == cloudBefore.bgr && sfm.getDepthMaps().size() == mapsBefore.size();
    for (size_t i = 0; same && i < cloud.points.size(); ++i) same = std::memcmp(&cloud.points[i], &cloudBefore.points[i], sizeof(cv::Point3f)) == 0;
    size_t at = 0;
    for (int v = 0; v < n_views; ++v) {
        const size_t n = (size_t)w[v] * h[v];
        const cv::Mat& m = sfm.getDepthMaps()[(size_t)v];
        has_map[v] = m.empty() ? 0 : 1;
        if (m.empty()) std::memset(depth + at, 0, n * sizeof(float));
        else std::memcpy(depth + at, m.ptr<float>(0), n * sizeof(float));
        same = same && (m.empty() ? mapsBefore[(size_t)v].empty()
                                  : mapsBefore[(size_t)v].size() == n && std::memcmp(m.ptr<float>(0), mapsBefore[(size_t)v].data(), n * sizeof(float)) == 0);
        at += n;
    }
    *unchanged = same ? 1 : 0;
    if (!put_mesh(0, meshBefore) || !put_mesh(1, cleanBefore)) return -2;
    return 0;
}

// SfM::densify() where it has to refuse (tests/test_depth_oracle_cpu.py; no device involved): what = 0 after setFeatures (there are
// no pixels), 1 on images without a run, 2 on a fresh object.  Returns densify's code.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_densify_refusal(int what) {
    using namespace sfmtoylib;
    SfM sfm(1.0f);
    sfm.setConsoleDebugLevel(LOG_ERROR);
    if (what == 0) sfm.setFeatures(std::vector<Features>(2), 640, 480);
    if (what == 1) sfm.setImages(std::vector<cv::Mat>(2, cv::Mat(8, 8, CV_8U)));
    const int code = (int)sfm.densify();
    return code == 0 || !sfm.getDepthMaps().empty() || !sfm.getDenseCloud().points.empty() ? 100 + code : code;
}

// Flat-array driver of sfmtoylib::SfMFeatureMatching::createFlowMatchMatrix (tests/test_gpu_flow_pipeline.py): the images as
// sfmba_shim_run_sfm takes them, view i's key points in rows kp_ptr[i] .. kp_ptr[i+1]-1 of kp_xy [..][2], the pair window.  Outputs as
// sfmba_shim_feature_match_matrix.  Returns the number of matches, -1 if the call reported failure, -2 if the matrix is not
// n_images x n_images.
extern "C" __attribute__((visibility("default")))
int64_t sfmba_shim_flow_match_matrix(int n_images, int channels, const int64_t* img_ptr, const unsigned char* px, const int32_t* w, const int32_t* h,
                                     const int64_t* kp_ptr, const float* kp_xy, int window, int64_t* sizes, int64_t cap, int32_t* query, int32_t* train,
                                     int32_t* img_idx, float* dist) {
    using namespace sfmtoylib;
    std::vector<cv::Mat> images;
    for (int i = 0; i < n_images; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
    std::vector<Features> feats((size_t)n_images);
    addKeyPoints(feats, kp_ptr, kp_xy);
    MatchMatrix mm;
    if (!SfMFeatureMatching::createFlowMatchMatrix(images, feats, mm, window)) return -1;
    if (mm.size() != (size_t)n_images) return -2;
    int64_t n = 0;
    for (int l = 0; l < n_images; ++l) {
        if (mm[l].size() != (size_t)n_images) return -2;
        for (int r = 0; r < n_images; ++r) {
            sizes[(size_t)l * n_images + r] = (int64_t)mm[l][r].size();
            n = flattenMatching(mm[l][r], n, cap, query, train, img_idx, dist);
        }
    }
    return n;
}

// sfmba_shim_run_sfm_typed with the matcher of SfM::setMatcherType (0 = MATCHER_DESCRIPTORS, 1 = MATCHER_FLOW) and the window of
// SfM::setFlowPairWindow (tests/test_gpu_flow_pipeline.py).  Outputs and return value as sfmba_shim_run_sfm.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm_matcher(int feature_type, int matcher_type, int flow_window, float merge_distance, int n_views, int channels,
                               const int64_t* img_ptr, const unsigned char* px, const int32_t* w, const int32_t* h, int debug_level, float* poses, float* K,
                               unsigned char* done, unsigned char* good, int* n_added, int32_t* added_view, unsigned char* added_posed,
                               int64_t* added_cloud, int64_t cap_pts, int64_t cap_views, int64_t* n_pts, float* xyz, int64_t* view_ptr,
                               int32_t* view_idx, int32_t* feat_idx, const char* ply_prefix) {
    using namespace sfmtoylib;
    SfM sfm(1.0f);
    sfm.setConsoleDebugLevel((unsigned)debug_level);
    sfm.setFeatureType((FeatureType)feature_type);
    sfm.setMatcherType((MatcherType)matcher_type);
    sfm.setFlowPairWindow(flow_window);
    sfm.setMergeFeatureMatchDistance(merge_distance);
    std::vector<cv::Mat> images;
    for (int i = 0; i < n_views; ++i) images.push_back(buildImage(w[i], h[i], channels, px + img_ptr[i]));
    sfm.setImages(images);
    return flattenRun(sfm, sfm.runSfM(), n_views, poses, K, done, good, n_added, added_view, added_posed, added_cloud, cap_pts, cap_views, n_pts, xyz,
                      view_ptr, view_idx, feat_idx, ply_prefix);
}

// SfM::runSfM with MATCHER_FLOW where it has to refuse (tests/test_flow_oracle_cpu.py; no device involved): what = 0 after setFeatures
// (there are no pixels to track in), 1 on images with a negative pair window.  Returns runSfM's code.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_flow_refusal(int what) {
    using namespace sfmtoylib;
    SfM sfm(1.0f);
    sfm.setConsoleDebugLevel(LOG_ERROR);
    sfm.setMatcherType(MATCHER_FLOW);
    if (what == 0) sfm.setFeatures(std::vector<Features>(2), 640, 480);
    if (what == 1) { sfm.setImages(std::vector<cv::Mat>(2, cv::Mat(8, 8, CV_8U))); sfm.setFlowPairWindow(-1); }
    return (int)sfm.runSfM();
}

// Flat-array driver of sfmtoylib::SfM::setImagesDirectory (tests/test_sfm_scene_cpu.py; no device involved): the images come back
// one after the other in px (cap bytes), w / h [cap_images], *channels = 1 or 3.  Returns the number of images, -1 when the call
// reported failure, -2 if a capacity is too small.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_read_images_directory(const char* path, int cap_images, int64_t cap, int32_t* w, int32_t* h, int* channels, unsigned char* px) {
    using namespace sfmtoylib;
    SfM sfm;
    sfm.setConsoleDebugLevel(LOG_ERROR);
    if (!sfm.setImagesDirectory(path)) return -1;
    const std::vector<cv::Mat>& images = sfm.getImages();
    if ((int)images.size() > cap_images) return -2;
    int64_t at = 0;
    for (size_t i = 0; i < images.size(); ++i) {
        const int ch = images[i].type() == CV_8UC3 ? 3 : 1;
        const int64_t row = (int64_t)images[i].cols * ch;
        if (at + row * images[i].rows > cap) return -2;
        *channels = ch;
        w[i] = images[i].cols; h[i] = images[i].rows;
        for (int r = 0; r < images[i].rows; ++r, at += row) std::memcpy(px + at, images[i].ptr<unsigned char>(r), (size_t)row);
    }
    return (int)images.size();
}

namespace {
// images one after the other in px (cap bytes), w / h [cap_images]; the number of images, -2 if a capacity is too small
int flattenImages(const std::vector<cv::Mat>& images, int cap_images, int64_t cap, int32_t* w, int32_t* h, int* channels, unsigned char* px) {
    if ((int)images.size() > cap_images) return -2;
    int64_t at = 0;
    for (size_t i = 0; i < images.size(); ++i) {
        const int ch = images[i].type() == CV_8UC3 ? 3 : 1;
        const int64_t row = (int64_t)images[i].cols * ch;
        if (at + row * images[i].rows > cap) return -2;
        *channels = ch;
        w[i] = images[i].cols; h[i] = images[i].rows;
        for (int r = 0; r < images[i].rows; ++r, at += row) std::memcpy(px + at, images[i].ptr<unsigned char>(r), (size_t)row);
    }
    return (int)images.size();
}
}  // namespace

// Flat-array driver of sfmtoylib::SfMImageUtilities::readImages (tests/test_gpu_image_io.py): n_paths file paths, one downscale
// factor.  The images come back as sfmba_shim_read_images_directory returns them.  Returns the number of images, -1 when the call
// reported failure, -2 if a capacity is too small.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_read_images(int n_paths, const char* const* paths, float downscale, int cap_images, int64_t cap, int32_t* w, int32_t* h, int* channels,
                           unsigned char* px) {
    using namespace sfmtoylib;
    std::vector<cv::Mat> images;
    if (!SfMImageUtilities::readImages(std::vector<std::string>(paths, paths + n_paths), downscale, images)) return -1;
    return flattenImages(images, cap_images, cap, w, h, channels, px);
}

// Flat-array driver of sfmtoylib::SfMImageUtilities::resizeImages: image i owns bytes img_ptr[i] .. img_ptr[i+1]-1 of src.  Returns as
// sfmba_shim_read_images.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_resize_images(int n_images, const int64_t* img_ptr, const unsigned char* src, const int32_t* sw, const int32_t* sh, int src_channels,
                             float downscale, int cap_images, int64_t cap, int32_t* w, int32_t* h, int* channels, unsigned char* px) {
    using namespace sfmtoylib;
    std::vector<cv::Mat> images, out;
    for (int i = 0; i < n_images; ++i) images.push_back(buildImage(sw[i], sh[i], src_channels, src + img_ptr[i]));
    if (!SfMImageUtilities::resizeImages(images, downscale, out)) return -1;
    return flattenImages(out, cap_images, cap, w, h, channels, px);
}

// sfmba_shim_read_images_directory with the downscale factor of the constructor: SfM(downscale).setImagesDirectory(path).
extern "C" __attribute__((visibility("default")))
int sfmba_shim_read_images_directory_scaled(const char* path, float downscale, int cap_images, int64_t cap, int32_t* w, int32_t* h, int* channels,
                                            unsigned char* px) {
    using namespace sfmtoylib;
    SfM sfm(downscale);
    sfm.setConsoleDebugLevel(LOG_ERROR);
    if (!sfm.setImagesDirectory(path)) return -1;
    return flattenImages(sfm.getImages(), cap_images, cap, w, h, channels, px);
}

// sfmba_shim_run_sfm starting from a directory: SfM(downscale), setImagesDirectory(path), runSfM().  *n_views_out receives the number
// of images read (the per-view outputs hold cap_view_count entries).  Returns as sfmba_shim_run_sfm, -1 when the directory could
// not be read, -2 also when it holds more than cap_view_count images.
extern "C" __attribute__((visibility("default")))
int sfmba_shim_run_sfm_directory(const char* path, float downscale, int debug_level, int cap_view_count, int* n_views_out, float* poses, float* K,
                                 unsigned char* done, unsigned char* good, int* n_added, int32_t* added_view, unsigned char* added_posed,
                                 int64_t* added_cloud, int64_t cap_pts, int64_t cap_views, int64_t* n_pts, float* xyz, int64_t* view_ptr,
                                 int32_t* view_idx, int32_t* feat_idx, const char* ply_prefix) {
    using namespace sfmtoylib;
    SfM sfm(downscale);
    sfm.setConsoleDebugLevel((unsigned)debug_level);
    *n_views_out = 0;
    if (!sfm.setImagesDirectory(path)) return -1;
    const int n_views = (int)sfm.getImages().size();
    *n_views_out = n_views;
    if (n_views > cap_view_count) return -2;
    return flattenRun(sfm, sfm.runSfM(), n_views, poses, K, done, good, n_added, added_view, added_posed, added_cloud, cap_pts, cap_views, n_pts, xyz,
                      view_ptr, view_idx, feat_idx, ply_prefix);
}
