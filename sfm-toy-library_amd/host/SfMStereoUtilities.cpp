// SfMStereoUtilities.cpp -- drop-in for SfMStereoUtilities::triangulateViews (SfMToyLib/SfMStereoUtilities.cpp:120-206).
//
// Marshalling mirrors the reference: matches are aligned through queryIdx / trainIdx with back references to the original
// feature indices (GetAlignedPointsFromMatch, SfMCommon.cpp:63-87; the 2D points are the key points' pt, :85-86), the
// triangulation + 10 px reprojection filter runs on the GPU (sfmba_triangulate), and every surviving point is appended to
// pointCloud with originatingViews[left] / [right] = those back references (:192-203).  Points are appended in match order.
//
// triangulateViewsBatch: the same for the pairs (good view, new view) of one added view (SfM.cpp:413-444) in ONE device call
// (sfmba_triangulate_pairs): the match lists go as they are, the alignment happens on the device, and the kept entries come back as
// a list per pair, in match order.
//
// findCameraPoseFrom2D3DMatch (SfMToyLib/SfMStereoUtilities.cpp:208-243): the reference calls cv::solvePnPRansac with
// iterationsCount = 100, reprojectionError = RANSAC_THRESHOLD = 10 and confidence 0.99, then rejects the pose when fewer than
// POSE_INLIERS_MINIMAL_RATIO of the matches are inliers.  Here sfmba_pnp_ransac evaluates all 100 hypotheses at once -- the
// confidence-based early stop has no meaning in a parallel evaluation, so 0.99 has no counterpart -- with threshold 10, seed 0
// and 20 refinement steps; the gate and its message are the reference's.
//
// findHomographyInliers (SfMToyLib/SfMStereoUtilities.cpp:51-72): the reference aligns the matched key points
// (GetAlignedPointsFromMatch, SfMCommon.cpp:63-87), calls cv::findHomography(RANSAC, RANSAC_THRESHOLD = 10) and counts the mask.
// Here the key points of the images and the match lists go to sfmba_homography_ransac as they are -- the alignment happens on the
// device -- with threshold 10, seed 0 and 2000 hypotheses (OpenCV's default maxIters: where its loop stops at the latest).
//
// findCameraMatricesFromMatch (SfMToyLib/SfMStereoUtilities.cpp:74-118): the reference aligns the matched key points, calls
// cv::findEssentialMat(RANSAC, 0.999, 1.0) and cv::recoverPose, sets Pleft = I and Pright = [R|t] and keeps the matches of the final
// mask.  Here the key points and the match lists go to sfmba_essential_ransac as they are, with threshold 1, seed 0 and 1000
// hypotheses (cv::findEssentialMat's maxIters: where its loop stops at the latest); fx and fy are both read from K (the reference
// assumes fx = fy).
#include "SfMStereoUtilities.h"

#include <iostream>
#include <vector>

#include "../../include/sfmba.h"

namespace sfmtoylib {

bool SfMStereoUtilities::findHomographyInliersBatch(
        const std::vector<const Features*>& images,
        const std::vector<int>&             left,
        const std::vector<int>&             right,
        const std::vector<const Matching*>& matches,
        std::vector<int>&                   inliers) {
    const int    HOMOGRAPHY_HYPOTHESES = 2000;      // cv::findHomography's default maxIters (all are evaluated)
    const float  RANSAC_THRESHOLD      = 10.0f;     // SfMStereoUtilities.cpp:41
    const size_t n_pairs = left.size();
    inliers.assign(n_pairs, 0);
    if (n_pairs == 0) return true;
    std::vector<int64_t> img_ptr(images.size() + 1, 0);
    for (size_t i = 0; i < images.size(); i++) img_ptr[i + 1] = img_ptr[i] + (int64_t)images[i]->keyPoints.size();
    std::vector<float> pts(2 * (size_t)img_ptr.back() + 2);
    for (size_t i = 0; i < images.size(); i++)
        for (size_t k = 0; k < images[i]->keyPoints.size(); k++) {
            pts[2 * ((size_t)img_ptr[i] + k)]     = images[i]->keyPoints[k].pt.x;
            pts[2 * ((size_t)img_ptr[i] + k) + 1] = images[i]->keyPoints[k].pt.y;
        }
    std::vector<int64_t> pair_ptr(n_pairs + 1, 0);
    for (size_t p = 0; p < n_pairs; p++) pair_ptr[p + 1] = pair_ptr[p] + (int64_t)matches[p]->size();
    std::vector<int32_t> pl(left.begin(), left.end()), pr(right.begin(), right.end());
    std::vector<int32_t> query((size_t)pair_ptr.back() + 1), train((size_t)pair_ptr.back() + 1);
    for (size_t p = 0; p < n_pairs; p++)
        for (size_t e = 0; e < matches[p]->size(); e++) {
            query[(size_t)pair_ptr[p] + e] = (*matches[p])[e].queryIdx;
            train[(size_t)pair_ptr[p] + e] = (*matches[p])[e].trainIdx;
        }
    std::vector<double> H(9 * n_pairs);
    std::vector<unsigned char> mask((size_t)pair_ptr.back() + 1);
    std::vector<sfmba_homography_result> res(n_pairs);
    const int rc = sfmba_homography_ransac(0, (int)images.size(), img_ptr.data(), pts.data(), (int)n_pairs, pl.data(), pr.data(), pair_ptr.data(),
                                           query.data(), train.data(), HOMOGRAPHY_HYPOTHESES, RANSAC_THRESHOLD, 0, H.data(), mask.data(),
                                           res.data(), nullptr, nullptr);
    if (rc != SFMBA_OK) {
        std::cerr << "findHomographyInliers failed. (sfmba rc=" << rc << ": " << sfmba_last_error() << ")" << std::endl;
        return false;
    }
    for (size_t p = 0; p < n_pairs; p++) inliers[p] = res[p].status == 0 ? res[p].n_inliers : 0;
    return true;
}

int SfMStereoUtilities::findHomographyInliers(
        const Features& left,
        const Features& right,
        const Matching& matches) {
    if (matches.size() < 4) return 0;               // SfMStereoUtilities.cpp:67
    std::vector<int> inliers;
    findHomographyInliersBatch({ &left, &right }, { 0 }, { 1 }, { &matches }, inliers);
    return inliers[0];
}

bool SfMStereoUtilities::findCameraMatricesFromMatchBatch(
        const Intrinsics&                   intrinsics,
        const std::vector<const Features*>& images,
        const std::vector<int>&             left,
        const std::vector<int>&             right,
        const std::vector<const Matching*>& matches,
        std::vector<unsigned char>&         ok,
        std::vector<Matching>&              prunedMatches,
        std::vector<cv::Matx34f>&           Pleft,
        std::vector<cv::Matx34f>&           Pright) {
    const int    ESSENTIAL_HYPOTHESES = 1000;       // cv::findEssentialMat's maxIters (all are evaluated)
    const float  ESSENTIAL_THRESHOLD  = 1.0f;       // SfMStereoUtilities.cpp:97
    const size_t n_pairs = left.size();
    ok.assign(n_pairs, 0);
    prunedMatches.assign(n_pairs, Matching());
    Pleft.assign(n_pairs, cv::Matx34f::eye());
    Pright.assign(n_pairs, cv::Matx34f::eye());
    if (intrinsics.K.empty()) {
        std::cerr << "Intrinsics matrix (K) must be initialized." << std::endl;
        return false;
    }
    if (n_pairs == 0) return true;
    float K[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) K[3 * r + c] = intrinsics.K.at<float>(r, c);
    std::vector<int64_t> img_ptr(images.size() + 1, 0);
    for (size_t i = 0; i < images.size(); i++) img_ptr[i + 1] = img_ptr[i] + (int64_t)images[i]->keyPoints.size();
    std::vector<float> pts(2 * (size_t)img_ptr.back() + 2);
    for (size_t i = 0; i < images.size(); i++)
        for (size_t k = 0; k < images[i]->keyPoints.size(); k++) {
            pts[2 * ((size_t)img_ptr[i] + k)]     = images[i]->keyPoints[k].pt.x;
            pts[2 * ((size_t)img_ptr[i] + k) + 1] = images[i]->keyPoints[k].pt.y;
        }
    std::vector<int64_t> pair_ptr(n_pairs + 1, 0);
    for (size_t p = 0; p < n_pairs; p++) pair_ptr[p + 1] = pair_ptr[p] + (int64_t)matches[p]->size();
    std::vector<int32_t> pl(left.begin(), left.end()), pr(right.begin(), right.end());
    std::vector<int32_t> query((size_t)pair_ptr.back() + 1), train((size_t)pair_ptr.back() + 1);
    for (size_t p = 0; p < n_pairs; p++)
        for (size_t e = 0; e < matches[p]->size(); e++) {
            query[(size_t)pair_ptr[p] + e] = (*matches[p])[e].queryIdx;
            train[(size_t)pair_ptr[p] + e] = (*matches[p])[e].trainIdx;
        }
    std::vector<double> E(9 * n_pairs), pose(12 * n_pairs);
    std::vector<unsigned char> mask((size_t)pair_ptr.back() + 1);
    std::vector<sfmba_essential_result> res(n_pairs);
    const int rc = sfmba_essential_ransac(0, (int)images.size(), img_ptr.data(), pts.data(), (int)n_pairs, pl.data(), pr.data(), pair_ptr.data(),
                                          query.data(), train.data(), K, ESSENTIAL_HYPOTHESES, ESSENTIAL_THRESHOLD, 0, E.data(), pose.data(),
                                          mask.data(), res.data(), nullptr, nullptr, nullptr);
    if (rc != SFMBA_OK) {
        std::cerr << "findCameraMatricesFromMatch failed. (sfmba rc=" << rc << ": " << sfmba_last_error() << ")" << std::endl;
        return false;
    }
    for (size_t p = 0; p < n_pairs; p++) {
        if (res[p].status != 0) continue;
        ok[p] = 1;
        for (int e = 0; e < 12; e++) Pright[p].val[e] = (float)pose[12 * p + e];
        for (size_t e = 0; e < matches[p]->size(); e++)
            if (mask[(size_t)pair_ptr[p] + e]) prunedMatches[p].push_back((*matches[p])[e]);
    }
    return true;
}

bool SfMStereoUtilities::findCameraMatricesFromMatch(
        const Intrinsics& intrinsics,
        const Matching&   matches,
        const Features&   featuresLeft,
        const Features&   featuresRight,
        Matching&         prunedMatches,
        cv::Matx34f&      Pleft,
        cv::Matx34f&      Pright) {
    std::vector<unsigned char> ok;
    std::vector<Matching> pruned;
    std::vector<cv::Matx34f> Pl, Pr;
    if (!findCameraMatricesFromMatchBatch(intrinsics, { &featuresLeft, &featuresRight }, { 0 }, { 1 }, { &matches }, ok, pruned, Pl, Pr) || !ok[0])
        return false;
    Pleft = Pl[0];
    Pright = Pr[0];
    prunedMatches = pruned[0];
    return true;
}

bool SfMStereoUtilities::triangulateViews(
        const Intrinsics&  intrinsics,
        const ImagePair    imagePair,
        const Matching&    matches,
        const Features&    featuresLeft,
        const Features&    featuresRight,
        const cv::Matx34f& Pleft,
        const cv::Matx34f& Pright,
        PointCloud&        pointCloud) {
    const size_t n = matches.size();
    std::vector<float> left(2 * n), right(2 * n);
    std::vector<int> leftBackReference(n), rightBackReference(n);
    for (size_t i = 0; i < n; i++) {
        const cv::Point2f& pl = featuresLeft.keyPoints[matches[i].queryIdx].pt;
        const cv::Point2f& pr = featuresRight.keyPoints[matches[i].trainIdx].pt;
        left[2 * i] = pl.x;  left[2 * i + 1] = pl.y;
        right[2 * i] = pr.x; right[2 * i + 1] = pr.y;
        leftBackReference[i] = matches[i].queryIdx;
        rightBackReference[i] = matches[i].trainIdx;
    }
    float K[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) K[3 * r + c] = intrinsics.K.at<float>(r, c);

    std::vector<float> points3d(3 * n);
    std::vector<unsigned char> keep(n);
    const float MIN_REPROJECTION_ERROR = 10.0f;     // SfMStereoUtilities.cpp:42
    const int rc = sfmba_triangulate(0, (int64_t)n, left.data(), right.data(), K, Pleft.val, Pright.val, MIN_REPROJECTION_ERROR,
                                     points3d.data(), keep.data(), nullptr);
    if (rc != SFMBA_OK) {
        std::cerr << "triangulateViews failed. (sfmba rc=" << rc << ": " << sfmba_last_error() << ")" << std::endl;
        return false;
    }
    for (size_t i = 0; i < n; i++) {
        if (!keep[i]) continue;
        Point3DInMap p;
        p.p = cv::Point3f(points3d[3 * i], points3d[3 * i + 1], points3d[3 * i + 2]);
        p.originatingViews[(int)imagePair.left]  = leftBackReference[i];
        p.originatingViews[(int)imagePair.right] = rightBackReference[i];
        pointCloud.push_back(p);
    }
    return true;
}

bool SfMStereoUtilities::triangulateViewsBatch(
        const Intrinsics&                   intrinsics,
        const std::vector<const Features*>& images,
        const std::vector<int>&             left,
        const std::vector<int>&             right,
        const std::vector<const Matching*>& matches,
        const std::vector<cv::Matx34f>&     Pleft,
        const std::vector<cv::Matx34f>&     Pright,
        std::vector<unsigned char>&         ok,
        std::vector<PointCloud>&            pointClouds) {
    const float  MIN_REPROJECTION_ERROR = 10.0f;    // SfMStereoUtilities.cpp:42
    const size_t n_pairs = left.size();
    ok.assign(n_pairs, 0);
    pointClouds.assign(n_pairs, PointCloud());
    if (intrinsics.K.empty()) {
        std::cerr << "Intrinsics matrix (K) must be initialized." << std::endl;
        return false;
    }
    if (right.size() != n_pairs || matches.size() != n_pairs || Pleft.size() != n_pairs || Pright.size() != n_pairs) {
        std::cerr << "triangulateViews failed. (the lists of a batch differ in length)" << std::endl;
        return false;
    }
    if (n_pairs == 0) return true;
    float K[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) K[3 * r + c] = intrinsics.K.at<float>(r, c);
    std::vector<int64_t> img_ptr(images.size() + 1, 0);
    for (size_t i = 0; i < images.size(); i++) img_ptr[i + 1] = img_ptr[i] + (int64_t)images[i]->keyPoints.size();
    std::vector<float> pts(2 * (size_t)img_ptr.back() + 2);
    for (size_t i = 0; i < images.size(); i++)
        for (size_t k = 0; k < images[i]->keyPoints.size(); k++) {
            pts[2 * ((size_t)img_ptr[i] + k)]     = images[i]->keyPoints[k].pt.x;
            pts[2 * ((size_t)img_ptr[i] + k) + 1] = images[i]->keyPoints[k].pt.y;
        }
    std::vector<int64_t> pair_ptr(n_pairs + 1, 0);
    for (size_t p = 0; p < n_pairs; p++) pair_ptr[p + 1] = pair_ptr[p] + (int64_t)matches[p]->size();
    const size_t total = (size_t)pair_ptr.back();
    std::vector<int32_t> pl(left.begin(), left.end()), pr(right.begin(), right.end());
    std::vector<int32_t> query(total + 1), train(total + 1);
    std::vector<float> Pl(12 * n_pairs), Pr(12 * n_pairs);
    for (size_t p = 0; p < n_pairs; p++) {
        for (size_t e = 0; e < matches[p]->size(); e++) {
            query[(size_t)pair_ptr[p] + e] = (*matches[p])[e].queryIdx;
            train[(size_t)pair_ptr[p] + e] = (*matches[p])[e].trainIdx;
        }
        for (int e = 0; e < 12; e++) { Pl[12 * p + e] = Pleft[p].val[e]; Pr[12 * p + e] = Pright[p].val[e]; }
    }
    std::vector<float> points3d(3 * total + 3);
    std::vector<unsigned char> keep(total + 1);
    std::vector<int64_t> kept_ptr(n_pairs + 1), kept_idx(total + 1);
    const int rc = sfmba_triangulate_pairs(0, (int)images.size(), img_ptr.data(), pts.data(), K, (int)n_pairs, pl.data(), pr.data(), pair_ptr.data(),
                                           query.data(), train.data(), nullptr, Pl.data(), Pr.data(), MIN_REPROJECTION_ERROR, points3d.data(),
                                           keep.data(), nullptr, kept_ptr.data(), kept_idx.data());
    if (rc != SFMBA_OK) {
        std::cerr << "triangulateViews failed. (sfmba rc=" << rc << ": " << sfmba_last_error() << ")" << std::endl;
        return false;
    }
    for (size_t p = 0; p < n_pairs; p++) {
        ok[p] = 1;
        pointClouds[p].reserve((size_t)(kept_ptr[p + 1] - kept_ptr[p]));
        for (int64_t k = kept_ptr[p]; k < kept_ptr[p + 1]; k++) {
            const size_t i = (size_t)kept_idx[k];
            Point3DInMap pt;
            pt.p = cv::Point3f(points3d[3 * i], points3d[3 * i + 1], points3d[3 * i + 2]);
            pt.originatingViews[left[p]]  = query[i];
            pt.originatingViews[right[p]] = train[i];
            pointClouds[p].push_back(pt);
        }
    }
    return true;
}

bool SfMStereoUtilities::findCameraPoseFrom2D3DMatch(
        const Intrinsics&     intrinsics,
        const Image2D3DMatch& match,
        cv::Matx34f&          cameraPose) {
    const size_t n = match.points2D.size();
    if (match.points3D.size() != n) {
        std::cerr << "findCameraPoseFrom2D3DMatch failed. (" << n << " 2D points, " << match.points3D.size() << " 3D points)" << std::endl;
        return false;
    }
    std::vector<float> xyz(3 * n), uv(2 * n);
    for (size_t i = 0; i < n; i++) {
        xyz[3 * i] = match.points3D[i].x; xyz[3 * i + 1] = match.points3D[i].y; xyz[3 * i + 2] = match.points3D[i].z;
        uv[2 * i] = match.points2D[i].x;  uv[2 * i + 1] = match.points2D[i].y;
    }
    float K[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) K[3 * r + c] = intrinsics.K.at<float>(r, c);

    const int    ITERATIONS_COUNT = 100;            // SfMStereoUtilities.cpp:224 (all are evaluated)
    const float  RANSAC_THRESHOLD = 10.0f;          // SfMStereoUtilities.cpp:41
    const int    REFINE_STEPS     = 20;
    const int64_t prob_ptr[2] = { 0, (int64_t)n };
    double pose[12];
    std::vector<unsigned char> inliers(n ? n : 1);
    sfmba_pnp_result res;
    const int rc = sfmba_pnp_ransac(0, 1, prob_ptr, xyz.data(), uv.data(), K, ITERATIONS_COUNT, RANSAC_THRESHOLD, 0, REFINE_STEPS,
                                    pose, inliers.data(), &res, nullptr, nullptr);
    if (rc != SFMBA_OK) {
        std::cerr << "findCameraPoseFrom2D3DMatch failed. (sfmba rc=" << rc << ": " << sfmba_last_error() << ")" << std::endl;
        return false;
    }
    //check inliers ratio and reject if too small
    if (res.status != 0 || n == 0 || ((float)res.n_inliers / (float)n) < POSE_INLIERS_MINIMAL_RATIO) {
        std::cerr << "Inliers ratio is too small: " << res.n_inliers << " / " << n << std::endl;
        return false;
    }
    for (int e = 0; e < 12; e++) cameraPose.val[e] = (float)pose[e];
    return true;
}

}  // namespace sfmtoylib
