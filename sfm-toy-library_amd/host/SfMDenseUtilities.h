// SfMDenseUtilities.h -- dense depth maps and a dense cloud over the C ABI's sfmba_depth_sweep / sfmba_depth_fuse (include/sfmba.h
// holds the contract): plane-sweep stereo for a list of jobs in ONE device call, and the consistency filter that turns the depth maps
// of a set of views into coloured points in ONE device call.  The reference stops at the sparse cloud; this is the stage between
// "camera poses" and "a model" (SfM::densify drives it).  Both functions are thin: they flatten, call and rebuild.
#pragma once
#include <vector>

#include "SfMCommon.h"

namespace sfmtoylib {

// One sweep: a reference view, 1..4 source views, the depth range searched.
struct DenseJob {
    int              reference;
    std::vector<int> sources;
    float            zNear, zFar;
};

// First choices; nobody has tuned them (see SfM.h).
struct DenseParams {
    int   planes;           // inverse-depth planes per job, 2..256
    int   radius;           // the window is (2 radius + 1)^2 pixels, radius 1..4
    int   minStd;           // a reference window takes part if its standard deviation is at least this, 0..127
    float minScore;         // the winning plane's mean correlation must reach this, [-1, 1]
    int   minSources;       // sources that must count for a plane to be valid, 1..4
    float relTol;           // fuse: relative depth difference that still agrees, >= 0
    int   minConsistent;    // fuse: agreeing check views a pixel needs, 0..4
    int   maxSources;       // SfM::densify: the nearest other good views swept against, 1..4
    DenseParams() : planes(64), radius(3), minStd(2), minScore(0.6f), minSources(1), relTol(0.01f), minConsistent(1), maxSources(2) {}
};

// The fused points in (view, row, column) order.  A surface point seen by three views appears three times: nothing is de-duplicated.
struct DenseCloud {
    Points3f                   points;
    std::vector<unsigned char> bgr;      // 3 per point: the pixel's own colour (a gray image gives g, g, g)
    std::vector<int>           views;    // the view a point comes from
    std::vector<int>           pixels;   // ... and its pixel there, row * cols + column
};

class SfMDenseUtilities {
public:
    /**
     * One depth map (CV_32F, the reference view's size, 0 = no depth) and one score map (CV_32F, the winning plane's mean
     * correlation) per job, in job order.  images: all CV_8U or all CV_8UC3; poses: [R | t] per image.
     * @return false (outputs empty) when the device call fails or refuses an argument; the reason goes to stderr.
     */
    static bool computeDepthMaps(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses,
                                 const std::vector<DenseJob>& jobs, const DenseParams& params, std::vector<cv::Mat>& depthMaps,
                                 std::vector<cv::Mat>& scores);

    /**
     * depthMaps: one per image, an empty Mat for "none"; checks: per image the views its depths are checked against (0..4).
     * @param ok  if not null, receives false when the device call fails or refuses an argument (the cloud is then empty).
     */
    static DenseCloud fuseDepthMaps(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses,
                                    const std::vector<cv::Mat>& depthMaps, const std::vector<std::vector<int> >& checks,
                                    const DenseParams& params, bool* ok = nullptr);
};

}  // namespace sfmtoylib
