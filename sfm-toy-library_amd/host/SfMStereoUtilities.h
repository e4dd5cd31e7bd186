// SfMStereoUtilities.h -- the homography-inlier count, the relative pose of a pair, the triangulation and the 2D-3D pose entry
// points of the reference with their own signatures (SfMToyLib/SfMStereoUtilities.h:53-105), backed by the MI355X kernels
// (include/sfmba.h: sfmba_homography_ransac, sfmba_essential_ransac, sfmba_triangulate, sfmba_triangulate_pairs,
// sfmba_pnp_ransac).  Every member of the reference class has its counterpart here.
#pragma once
#include <vector>

#include "SfMCommon.h"

namespace sfmtoylib {

class SfMStereoUtilities {
public:
    /**
     * Number of matches that agree with one homography (four-point RANSAC on the GPU, threshold RANSAC_THRESHOLD = 10 px).
     * The reference runs cv::findHomography on OpenCV's global RNG with a confidence-based early stop; this runs the project's
     * own deterministic contract (include/sfmba.h, sfmba_homography_ransac) with all 2000 hypotheses -- OpenCV's default
     * maxIters, where its loop stops at the latest -- and seed 0: the same call always gives the same count.
     * @return the inlier count; 0 for fewer than 4 matches, no valid hypothesis, no HIP device or a device error.
     */
    static int findHomographyInliers(
            const Features& left,
            const Features& right,
            const Matching& matches);

    /**
     * The same for a list of pairs in ONE device call: pair p = images[left[p]] -> images[right[p]] with matches[p];
     * inliers[p] receives its count.  Pair p draws the sample stream of seed 0 + p (include/sfmba.h), so only pair 0 of a batch
     * counts exactly what findHomographyInliers counts for it.
     * @return false (every count 0; a line is written to stderr) when there is no HIP device or on a device error.
     */
    static bool findHomographyInliersBatch(
            const std::vector<const Features*>& images,
            const std::vector<int>&             left,
            const std::vector<int>&             right,
            const std::vector<const Matching*>& matches,
            std::vector<int>&                   inliers);

    /**
     * Find the camera matrices of a pair from its matches: Pleft = I, Pright = [R|t] with |t| = 1, prunedMatches = the matches
     * that agree with the essential matrix AND lie in front of both cameras, in their order (five-point RANSAC + recoverPose on
     * the GPU, threshold 1 px).  The reference runs cv::findEssentialMat on OpenCV's global RNG with a confidence-based early stop;
     * this runs the project's own deterministic contract (include/sfmba.h, sfmba_essential_ransac) with all 1000 hypotheses --
     * cv::findEssentialMat's maxIters, where its loop stops at the latest -- and seed 0: the same call always gives the same pose.
     * @return true on success; false (prunedMatches, Pleft and Pright untouched) when K is empty, the pair is degenerate (fewer
     *         than 6 matches, no valid hypothesis, no point in front), or there is no HIP device / a device error.
     */
    static bool findCameraMatricesFromMatch(
            const Intrinsics& intrinsics,
            const Matching&   featureMatching,
            const Features&   featuresLeft,
            const Features&   featuresRight,
            Matching&         prunedMatches,
            cv::Matx34f&      Pleft,
            cv::Matx34f&      Pright);

    /**
     * The same for a list of pairs in ONE device call -- the pairs (good view, new view) of one added view (SfM.cpp:413-431):
     * pair p = images[left[p]] -> images[right[p]] with matches[p]; ok[p], prunedMatches[p], Pleft[p], Pright[p] receive what
     * findCameraMatricesFromMatch returns for it (Pleft / Pright / prunedMatches of a pair with ok[p] == 0 are [I|0] / [I|0] /
     * empty).  Pair p draws the sample stream of seed 0 + p (include/sfmba.h), so only pair 0 of a batch gets exactly what
     * findCameraMatricesFromMatch gives it.
     * @return false (every ok 0; a line is written to stderr) when K is empty, there is no HIP device or on a device error.
     */
    static bool findCameraMatricesFromMatchBatch(
            const Intrinsics&                   intrinsics,
            const std::vector<const Features*>& images,
            const std::vector<int>&             left,
            const std::vector<int>&             right,
            const std::vector<const Matching*>& matches,
            std::vector<unsigned char>&         ok,
            std::vector<Matching>&              prunedMatches,
            std::vector<cv::Matx34f>&           Pleft,
            std::vector<cv::Matx34f>&           Pright);

    /**
     * Triangulate (recover 3D locations) from point matching.
     * @return true on success (false: no HIP device / device error; pointCloud untouched).
     */
    static bool triangulateViews(
            const Intrinsics&  intrinsics,
            const ImagePair    imagePair,
            const Matching&    matches,
            const Features&    leftFeatures,
            const Features&    rightFeatures,
            const cv::Matx34f& Pleft,
            const cv::Matx34f& Pright,
            PointCloud&        pointCloud);

    /**
     * The same for a list of pairs in ONE device call -- the pairs (good view, new view) of one added view (SfM.cpp:413-444):
     * pair p = images[left[p]] -> images[right[p]] with matches[p] under Pleft[p] / Pright[p]; pointClouds[p] receives exactly
     * the points triangulateViews appends for that pair (same floats, same back references, same order), with
     * originatingViews keyed by left[p] / right[p]; ok[p] = 1.
     * @return false (every ok 0, every cloud empty; a line is written to stderr) when K is empty, the lists differ in length,
     *         there is no HIP device or on a device error.
     */
    static bool triangulateViewsBatch(
            const Intrinsics&                   intrinsics,
            const std::vector<const Features*>& images,
            const std::vector<int>&             left,
            const std::vector<int>&             right,
            const std::vector<const Matching*>& matches,
            const std::vector<cv::Matx34f>&     Pleft,
            const std::vector<cv::Matx34f>&     Pright,
            std::vector<unsigned char>&         ok,
            std::vector<PointCloud>&            pointClouds);

    /**
     * Find the camera pose of a new view from its 2D-3D matches (P3P RANSAC + refinement on the GPU).
     * The reference runs cv::solvePnPRansac on OpenCV's global RNG; this runs the project's own deterministic contract
     * (include/sfmba.h, sfmba_pnp_ransac): the same call always gives the same pose.
     * @return true on success; false (cameraPose untouched) when the inlier ratio is below POSE_INLIERS_MINIMAL_RATIO, the
     *         problem is degenerate, or there is no HIP device / a device error.
     */
    static bool findCameraPoseFrom2D3DMatch(
            const Intrinsics&     intrinsics,
            const Image2D3DMatch& match,
            cv::Matx34f&          cameraPose);
};

}  // namespace sfmtoylib
