// SfM2DFeatureUtilities.h -- the matching entry point of the reference with its own signature
// (SfMToyLib/SfM2DFeatureUtilities.h:44-46), backed by the MI355X matcher (include/sfmba.h: sfmba_match_features), and the
// body of SfM::createFeatureMatchMatrix (SfMToyLib/SfM.cpp:157-212) as a free-standing function over the members it reads
// and writes.  Only matchFeatures is provided: extractFeatures (ORB detection) stays on the reference's OpenCV path.
// In the reference createFeatureMatchMatrix is a private member function; a maintainer replaces its body by one call
// (INTEGRATION.md section 5):
//
//   void SfM::createFeatureMatchMatrix() {
//       SfMFeatureMatching::createFeatureMatchMatrix(mImageFeatures, mFeatureMatchMatrix);
//   }
//
// Results are identical to the reference's: the same DMatch entries in the same order (queryIdx, trainIdx, imgIdx = 0,
// distance), for descriptors of type CV_8U.
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

class SfM2DFeatureUtilities {
public:
    /**
     * Brute-force Hamming 2-NN of every left descriptor among the right ones, pruned by the ratio test
     * (NN_MATCH_RATIO = 0.8f, SfM2DFeatureUtilities.cpp:53-71).  Fewer than 2 right descriptors give no matches (the
     * reference's behaviour is undefined there).  On a device error the result is empty and a line is written to stderr.
     */
    static Matching matchFeatures(
            const Features& featuresLeft,
            const Features& featuresRight);
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
