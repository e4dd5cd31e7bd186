// SfM2DFeatureUtilities.h -- the two entry points of the reference with their own signatures
// (SfMToyLib/SfM2DFeatureUtilities.h:42-46), backed by the MI355X extractor and matchers (include/sfmba.h: sfmba_orb_extract,
// sfmba_match_features, sfmba_match_features_l2, sfmba_flow_track, sfmba_flow_match), and the bodies of SfM::extractFeatures (SfMToyLib/SfM.cpp:141-154) and SfM::createFeatureMatchMatrix
// (SfM.cpp:157-212) as free-standing functions over the members they read and write.
// In the reference createFeatureMatchMatrix is a private member function; a maintainer replaces its body by one call
// (INTEGRATION.md section 5):
//
//   void SfM::createFeatureMatchMatrix() {
//       SfMFeatureMatching::createFeatureMatchMatrix(mImageFeatures, mFeatureMatchMatrix);
//   }
//
// Results are identical to the reference's: the same DMatch entries in the same order (queryIdx, trainIdx, imgIdx = 0,
// distance), for descriptors of type CV_8U.  Descriptors a caller brings through SfM::setFeatures may also be CV_32F (SIFT, SURF,
// RootSIFT, learned ones): they are matched by exact L2 distance, as cv::BFMatcher does with NORM_L2 (the contract is
// sfmba_match_features_l2's).  All non-empty descriptor matrices of a call must be of one type and one length.
//
// SfM::extractFeatures is replaced the same way, its loop over the images becoming one device call:
//
//   void SfM::extractFeatures() {
//       SfMFeatureExtraction::extractFeatures(mImages, mImageFeatures);
//   }
//
// The features are NOT cv::ORB's: the extractor runs the project's own deterministic ORB-style contract (include/sfmba.h,
// sfmba_orb_extract: its own steered-BRIEF pattern, 30 orientation bins, Harris ranking of all suppressed FAST corners,
// fixed-point resampling and smoothing, no mask) with the reference's parameters: 5000 features, scale 1.2, 8 levels, FAST
// threshold 20.
//
// FLOAT DESCRIPTORS: extractFeatures takes an extractor choice, FeatureType.  FEATURES_ORB (the default everywhere) is the unit
// above; FEATURES_SURF runs the project's Fast-Hessian / SURF-style contract (include/sfmba.h, sfmba_surf_extract -- not
// cv::xfeatures2d::SURF: no sub-pixel or sub-scale interpolation, one Gaussian over the descriptor window, 30 orientation bins)
// with 5000 features, 4 octaves, threshold 100, oriented.  Its descriptors are CV_32F rows of 64 of unit length, which matchFeatures
// and createFeatureMatchMatrix take through their L2 branch.
//
// The consumer of the whole matrix, SfM::sortViewsForBaseline (SfMToyLib/SfM.cpp:333-364), is restated the same way:
//
//   map<float, ImagePair> SfM::sortViewsForBaseline() {
//       return SfMFeatureMatching::sortViewsForBaseline(mImageFeatures, mFeatureMatchMatrix);
//   }
#pragma once
#include <map>
#include <vector>

#include "SfMCommon.h"

namespace sfmtoylib {

enum FeatureType { FEATURES_ORB = 0, FEATURES_SURF = 1 };
enum MatcherType { MATCHER_DESCRIPTORS = 0, MATCHER_FLOW = 1 };

class SfM2DFeatureUtilities {
public:
    /**
     * Key points, their coordinates (KeyPointsToPoints) and a CV_8U n x 32 descriptor matrix of one CV_8U (gray) or CV_8UC3 (BGR)
     * image (SfM2DFeatureUtilities.cpp:46-51).  On a device error the features are empty and a line is written to stderr.
     */
    Features extractFeatures(const cv::Mat& image);                          // a member function in the reference too (its detector is a member)

    /**
     * The same with the extractor named: FEATURES_ORB is the call above; FEATURES_SURF gives a CV_32F n x 64 descriptor matrix
     * (key point: size = the filter size L, octave = the octave, class_id = the sign of the Laplacian, as OpenCV's SURF stores it).
     */
    Features extractFeatures(const cv::Mat& image, FeatureType type);

    /**
     * Brute-force 2-NN (Hamming for CV_8U descriptors, L2 for CV_32F ones) of every left descriptor among the right ones, pruned
     * by the ratio test (NN_MATCH_RATIO = 0.8f, SfM2DFeatureUtilities.cpp:53-71).  Mixed types are refused (empty result).  Fewer than 2 right descriptors give no matches (the
     * reference's behaviour is undefined there).  On a device error the result is empty and a line is written to stderr.
     */
    static Matching matchFeatures(
            const Features& featuresLeft,
            const Features& featuresRight);
};

class SfMFeatureExtraction {
public:
    /**
     * SfM::extractFeatures: imageFeatures[i] = extractFeatures(images[i]) for every image, in ONE device call instead of the
     * reference's serial loop.  All images must be of one type (CV_8U or CV_8UC3).  Returns false on a device error
     * (imageFeatures is then sized but every entry is empty; a line is written to stderr).
     */
    static bool extractFeatures(
            const std::vector<cv::Mat>& images,
            std::vector<Features>&      imageFeatures);

    /** The same with the extractor named (FEATURES_ORB: the call above).  An unknown type is refused (false, a stderr line). */
    static bool extractFeatures(
            const std::vector<cv::Mat>& images,
            std::vector<Features>&      imageFeatures,
            FeatureType                 type);
};

class SfMFeatureMatching {
public:
    /**
     * SfM::createFeatureMatchMatrix: featureMatchMatrix becomes numImages x numImages with entry [i][j] = matchFeatures(i, j)
     * for every i < j and every other entry empty -- one batched device call instead of the reference's thread pool.
     * Returns false on a device error (the matrix is then sized but empty; a line is written to stderr).
     */
    static bool createFeatureMatchMatrix(
            const std::vector<Features>& imageFeatures,
            MatchMatrix&                 featureMatchMatrix);

    /**
     * MATCHING BY OPTICAL FLOW, for video-like input (what the reference's legacy tree did in OFFeatureMatcher.cpp with
     * gpu::PyrLKOpticalFlow::sparse): the same matrix without descriptors.  Entry [i][j], i < j, comes from tracking image i's key
     * points (imageFeatures[i].points) into image j with the pyramidal Lucas-Kanade tracker of include/sfmba.h (sfmba_flow_track),
     * snapping every end point to a key point of j within 2 px, a 0.7 ratio test among the key points in range and first come first
     * served per key point of j (sfmba_flow_match; tracking error below 12) -- ONE track call and ONE match call for the whole pair
     * list.  pairWindow k > 0 restricts the list to j - i <= k and leaves the other entries empty; 0 means all pairs.  A match's
     * distance is the snap distance in pixels (<= 2).  The tracker runs at 4 levels, radius 7, at most 20 iterations, min_eig 1:
     * first choices that nobody has tuned.  The images are all CV_8U or all CV_8UC3, one per feature set; the descriptors are not read.
     * Returns false on a refusal or a device error (the matrix is then sized but empty; a line is written to stderr).
     */
    static bool createFlowMatchMatrix(
            const std::vector<cv::Mat>&  images,
            const std::vector<Features>& imageFeatures,
            MatchMatrix&                 featureMatchMatrix,
            int                          pairWindow = 0);

    /**
     * SfM::sortViewsForBaseline: every pair i < j keyed by its homography-inlier ratio (float)inliers / (float)matches, pairs with
     * fewer than MIN_POINT_COUNT_FOR_HOMOGRAPHY = 100 matches under key 1.0; a later pair with an equal key overwrites the earlier
     * one, as in the reference's std::map.  All qualifying pairs go to the device in ONE call
     * (SfMStereoUtilities::findHomographyInliersBatch) instead of one cv::findHomography each.  On a device error the qualifying
     * pairs count 0 inliers (a line is written to stderr).
     */
    static std::map<float, ImagePair> sortViewsForBaseline(
            const std::vector<Features>& imageFeatures,
            const MatchMatrix&           featureMatchMatrix);
};

}  // namespace sfmtoylib
