// SfMStereoUtilities.h -- the triangulation and the 2D-3D pose entry points of the reference with their own signatures
// (SfMToyLib/SfMStereoUtilities.h:72-105), backed by the MI355X kernels (include/sfmba.h: sfmba_triangulate, sfmba_pnp_ransac).
// The other members of the reference class (homography inliers, essential-matrix pose) stay on the reference's OpenCV path
// (out of scope).
#pragma once
#include "SfMCommon.h"

namespace sfmtoylib {

class SfMStereoUtilities {
public:
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
