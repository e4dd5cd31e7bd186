// SfM2DFeatureUtilities.cpp -- host side of the feature extractor and matcher: flattens the images / descriptor matrices, calls
// the C ABI (include/sfmba.h, sfmba_orb_extract, sfmba_surf_extract, sfmba_match_features, sfmba_match_features_l2, sfmba_flow_track, sfmba_flow_match) and rebuilds the reference's Features and Matching lists.
// See SfM2DFeatureUtilities.h.
#include "SfM2DFeatureUtilities.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sfmba.h"
#include "SfMStereoUtilities.h"

namespace sfmtoylib {

namespace {

const double NN_MATCH_RATIO = 0.8f;     // SfM2DFeatureUtilities.cpp:35 -- a float literal widened to double

// the tracker's parameters: first choices that nobody has tuned
const int FLOW_LEVELS = 4, FLOW_RADIUS = 7, FLOW_MAX_ITERS = 20;
const float FLOW_MIN_EIG = 1.0f;
// the snap's are the reference's (legacy/SfMToyLib_Old/OFFeatureMatcher.cpp): error below 12, a key point within 2 px, ratio 0.7
const float FLOW_MAX_ERR = 12.0f, FLOW_SNAP_RADIUS = 2.0f;
const double FLOW_RATIO = 0.7;

struct FlatDescriptors {
    std::vector<int64_t> ptr;
    std::vector<unsigned char> bytes;       // the rows back to back: rowBytes bytes each (CV_8U) or rowBytes / 4 floats each (CV_32F)
    int rowBytes = 32;
    int type = CV_8U;
};

// The descriptors of images[0..n-1] back to back; false (with a stderr line) if one is neither CV_8U nor CV_32F, the types are
// mixed or the row lengths differ.  Decided before any device call.
bool flatten(const std::vector<const Features*>& images, FlatDescriptors& f) {
    f.ptr.assign(images.size() + 1, 0);
    int cols = -1, type = -1;
    for (size_t i = 0; i < images.size(); ++i) {
        const cv::Mat& d = images[i]->descriptors;
        const int rows = d.empty() ? 0 : d.rows;
        if (rows > 0) {
            if (d.type() != CV_8U && d.type() != CV_32F) { std::fprintf(stderr, "matchFeatures: descriptors must be CV_8U or CV_32F\n"); return false; }
            if (type >= 0 && d.type() != type) { std::fprintf(stderr, "matchFeatures: descriptor types differ (CV_8U and CV_32F mixed)\n"); return false; }
            if (cols >= 0 && d.cols != cols) { std::fprintf(stderr, "matchFeatures: descriptor lengths differ\n"); return false; }
            cols = d.cols; type = d.type();
        }
        f.ptr[i + 1] = f.ptr[i] + rows;
    }
    if (type >= 0) f.type = type;
    if (cols >= 0) f.rowBytes = cols * (f.type == CV_32F ? (int)sizeof(float) : 1);
    f.bytes.resize((size_t)f.ptr.back() * (size_t)f.rowBytes);
    for (size_t i = 0; i < images.size(); ++i) {
        const cv::Mat& d = images[i]->descriptors;
        for (int64_t r = 0; r < f.ptr[i + 1] - f.ptr[i]; ++r)           // row by row: an OpenCV matrix need not be continuous
            std::memcpy(&f.bytes[(size_t)(f.ptr[i] + r) * (size_t)f.rowBytes], d.ptr<unsigned char>((int)r), (size_t)f.rowBytes);
    }
    return true;
}

// One device call for the pair list; out[p] receives the Matching of pair p.  CV_8U rows: Hamming (sfmba_match_features);
// CV_32F rows: L2, what cv::BFMatcher does with NORM_L2 (sfmba_match_features_l2).
bool matchPairs(const std::vector<const Features*>& images, const std::vector<int32_t>& left, const std::vector<int32_t>& right,
                std::vector<Matching>& out) {
    out.assign(left.size(), Matching());
    FlatDescriptors f;
    if (!flatten(images, f)) return false;
    const int n_pairs = (int)left.size();
    std::vector<int64_t> ptr((size_t)n_pairs + 1, 0);
    std::vector<int32_t> query, train;
    std::vector<float> dist;
    int64_t cap = 0, total = 0;
    for (int p = 0; p < n_pairs; ++p)                     // at most one match per query row of a pair with >= 2 train rows
        if (f.ptr[right[p] + 1] - f.ptr[right[p]] >= 2) cap += f.ptr[left[p] + 1] - f.ptr[left[p]];
    int rc = SFMBA_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        query.resize((size_t)cap + 1); train.resize((size_t)cap + 1); dist.resize((size_t)cap + 1);
        if (f.type == CV_32F)
            rc = sfmba_match_features_l2(0, (int)images.size(), f.ptr.data(), reinterpret_cast<const float*>(f.bytes.data()),
                                         f.rowBytes / (int)sizeof(float), n_pairs, left.data(), right.data(), NN_MATCH_RATIO, ptr.data(),
                                         query.data(), train.data(), dist.data(), cap, &total);
        else
            rc = sfmba_match_features(0, (int)images.size(), f.ptr.data(), f.bytes.data(), f.rowBytes, n_pairs, left.data(), right.data(),
                                      NN_MATCH_RATIO, ptr.data(), query.data(), train.data(), dist.data(), cap, &total);
        if (rc == SFMBA_ERR_CAPACITY && attempt == 0) { cap = total; continue; }
        break;
    }
    if (rc != SFMBA_OK) {
        std::fprintf(stderr, "matchFeatures failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return false;
    }
    for (int p = 0; p < n_pairs; ++p) {
        Matching& m = out[(size_t)p];
        m.reserve((size_t)(ptr[p + 1] - ptr[p]));
        for (int64_t e = ptr[p]; e < ptr[p + 1]; ++e) {
            cv::DMatch d(query[(size_t)e], train[(size_t)e], dist[(size_t)e]);
            d.imgIdx = 0;                                                  // what OpenCV sets for a single train set
            m.push_back(d);
        }
    }
    return true;
}

// The pixels of images[0..n-1] back to back, as the image calls of include/sfmba.h take them; false (with a stderr line) unless all
// are non-empty and of one type, CV_8U or CV_8UC3.
bool flattenImages(const std::vector<cv::Mat>& images, const char* who, std::vector<int64_t>& ptr, std::vector<int32_t>& width,
                   std::vector<int32_t>& height, int& channels, std::vector<unsigned char>& pixels) {
    const size_t n = images.size();
    ptr.assign(n + 1, 0);
    width.assign(n, 0);
    height.assign(n, 0);
    const int type = images[0].type();
    if (type != CV_8U && type != CV_8UC3) { std::fprintf(stderr, "%s: images must be CV_8U or CV_8UC3\n", who); return false; }
    channels = type == CV_8UC3 ? 3 : 1;
    for (size_t i = 0; i < n; ++i) {
        if (images[i].empty() || images[i].type() != type) { std::fprintf(stderr, "%s: empty image or image types differ\n", who); return false; }
        width[i] = images[i].cols; height[i] = images[i].rows;
        ptr[i + 1] = ptr[i] + (int64_t)images[i].cols * images[i].rows * channels;
    }
    pixels.resize((size_t)ptr[n]);
    for (size_t i = 0; i < n; ++i) {
        const size_t row = (size_t)width[i] * (size_t)channels;
        for (int r = 0; r < height[i]; ++r)                                   // row by row: an OpenCV matrix need not be continuous
            std::memcpy(&pixels[(size_t)ptr[i] + (size_t)r * row], images[i].ptr<unsigned char>(r), row);
    }
    return true;
}

}  // namespace

Features SfM2DFeatureUtilities::extractFeatures(const cv::Mat& image) {
    std::vector<Features> out;
    if (!SfMFeatureExtraction::extractFeatures(std::vector<cv::Mat>(1, image), out)) return Features();
    return out[0];
}

Features SfM2DFeatureUtilities::extractFeatures(const cv::Mat& image, FeatureType type) {
    std::vector<Features> out;
    if (!SfMFeatureExtraction::extractFeatures(std::vector<cv::Mat>(1, image), out, type)) return Features();
    return out[0];
}

bool SfMFeatureExtraction::extractFeatures(const std::vector<cv::Mat>& images, std::vector<Features>& imageFeatures) {
    return extractFeatures(images, imageFeatures, FEATURES_ORB);
}

bool SfMFeatureExtraction::extractFeatures(const std::vector<cv::Mat>& images, std::vector<Features>& imageFeatures, FeatureType featureType) {
    const int ORB_FEATURES = 5000;                                            // ORB::create(5000), SfM2DFeatureUtilities.cpp:40
    const float ORB_SCALE = 1.2f;                                             // OpenCV's defaults for the rest
    const int ORB_LEVELS = 8, ORB_FAST_THRESHOLD = 20;
    const int SURF_FEATURES = 5000, SURF_OCTAVES = 4, SURF_UPRIGHT = 0;       // the float-descriptor unit's defaults
    const float SURF_THRESHOLD = 100.0f;
    const size_t n = images.size();
    imageFeatures.assign(n, Features());
    if (featureType != FEATURES_ORB && featureType != FEATURES_SURF) { std::fprintf(stderr, "extractFeatures: unknown feature type\n"); return false; }
    if (n == 0) return true;
    const bool surf = featureType == FEATURES_SURF;
    std::vector<int64_t> ptr, kp_ptr(n + 1, 0);
    std::vector<int32_t> width, height;
    std::vector<unsigned char> pixels;
    int channels = 1;
    if (!flattenImages(images, "extractFeatures", ptr, width, height, channels, pixels)) return false;
    std::vector<sfmba_orb_keypoint> kp;
    std::vector<sfmba_surf_keypoint> skp;
    std::vector<unsigned char> desc;
    std::vector<float> sdesc;
    int64_t cap = (int64_t)n * (surf ? SURF_FEATURES : ORB_FEATURES), total = 0;
    int rc = SFMBA_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (surf) {
            skp.resize((size_t)cap + 1); sdesc.resize(((size_t)cap + 1) * 64);
            rc = sfmba_surf_extract(0, (int)n, ptr.data(), pixels.data(), width.data(), height.data(), channels, SURF_FEATURES, SURF_OCTAVES,
                                    SURF_THRESHOLD, SURF_UPRIGHT, kp_ptr.data(), skp.data(), sdesc.data(), cap, &total, nullptr, nullptr, nullptr, nullptr);
        } else {
            kp.resize((size_t)cap + 1); desc.resize(((size_t)cap + 1) * 32);
            rc = sfmba_orb_extract(0, (int)n, ptr.data(), pixels.data(), width.data(), height.data(), channels, ORB_FEATURES, ORB_SCALE, ORB_LEVELS,
                                   ORB_FAST_THRESHOLD, kp_ptr.data(), kp.data(), desc.data(), cap, &total, nullptr, nullptr, nullptr, nullptr);
        }
        if (rc == SFMBA_ERR_CAPACITY && attempt == 0) { cap = total; continue; }
        break;
    }
    if (rc != SFMBA_OK) {
        std::fprintf(stderr, "extractFeatures failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return false;
    }
    for (size_t i = 0; i < n; ++i) {
        Features& f = imageFeatures[i];
        const int rows = (int)(kp_ptr[i + 1] - kp_ptr[i]);
        f.keyPoints.reserve((size_t)rows);
        f.points.reserve((size_t)rows);
        if (rows > 0) f.descriptors = surf ? cv::Mat(rows, 64, CV_32F) : cv::Mat(rows, 32, CV_8U);
        for (int r = 0; r < rows; ++r) {
            const size_t at = (size_t)kp_ptr[i] + (size_t)r;
            cv::KeyPoint c;
            if (surf) {
                const sfmba_surf_keypoint& k = skp[at];
                c.pt = cv::Point2f(k.x, k.y); c.size = k.size; c.angle = k.angle; c.response = k.response; c.octave = k.octave; c.class_id = k.laplacian;
                std::memcpy(f.descriptors.ptr<unsigned char>(r), &sdesc[at * 64], 64 * sizeof(float));
            } else {
                const sfmba_orb_keypoint& k = kp[at];
                c.pt = cv::Point2f(k.x, k.y); c.size = k.size; c.angle = k.angle; c.response = k.response; c.octave = k.octave; c.class_id = -1;
                std::memcpy(f.descriptors.ptr<unsigned char>(r), &desc[at * 32], 32);
            }
            f.keyPoints.push_back(c);
            f.points.push_back(c.pt);                                         // KeyPointsToPoints, SfMCommon.h
        }
    }
    return true;
}

Matching SfM2DFeatureUtilities::matchFeatures(const Features& featuresLeft, const Features& featuresRight) {
    std::vector<Matching> out;
    if (!matchPairs({ &featuresLeft, &featuresRight }, { 0 }, { 1 }, out)) return Matching();
    return out[0];
}

bool SfMFeatureMatching::createFeatureMatchMatrix(const std::vector<Features>& imageFeatures, MatchMatrix& featureMatchMatrix) {
    const size_t numImages = imageFeatures.size();
    featureMatchMatrix.resize(numImages, std::vector<Matching>(numImages));     // SfM.cpp:163
    std::vector<const Features*> images;
    for (const Features& f : imageFeatures) images.push_back(&f);
    std::vector<int32_t> left, right;
    for (size_t i = 0; i < numImages; i++)
        for (size_t j = i + 1; j < numImages; j++) { left.push_back((int32_t)i); right.push_back((int32_t)j); }
    std::vector<Matching> out;
    if (!matchPairs(images, left, right, out)) return false;
    for (size_t p = 0; p < left.size(); ++p) featureMatchMatrix[(size_t)left[p]][(size_t)right[p]].swap(out[p]);
    return true;
}

bool SfMFeatureMatching::createFlowMatchMatrix(const std::vector<cv::Mat>& images, const std::vector<Features>& imageFeatures,
                                               MatchMatrix& featureMatchMatrix, int pairWindow) {
    const size_t numImages = imageFeatures.size();
    featureMatchMatrix.assign(numImages, std::vector<Matching>(numImages));
    if (images.size() != numImages) { std::fprintf(stderr, "createFlowMatchMatrix: %zu images but %zu feature sets\n", images.size(), numImages); return false; }
    if (pairWindow < 0) { std::fprintf(stderr, "createFlowMatchMatrix: the pair window must be >= 0\n"); return false; }
    if (numImages == 0) return true;
    std::vector<int64_t> ptr, kp_ptr(numImages + 1, 0);
    std::vector<int32_t> width, height;
    std::vector<unsigned char> pixels;
    int channels = 1;
    if (!flattenImages(images, "createFlowMatchMatrix", ptr, width, height, channels, pixels)) return false;
    std::vector<float> kp;
    for (size_t i = 0; i < numImages; ++i) {
        kp_ptr[i + 1] = kp_ptr[i] + (int64_t)imageFeatures[i].points.size();
        for (const cv::Point2f& p : imageFeatures[i].points) { kp.push_back(p.x); kp.push_back(p.y); }
    }
    // pair (i, j), i < j, tracks i's key points into j; a window k > 0 keeps j - i <= k
    std::vector<int32_t> src, dst;
    std::vector<int64_t> pt_ptr(1, 0);
    std::vector<float> pts;
    for (size_t i = 0; i < numImages; i++)
        for (size_t j = i + 1; j < numImages && (pairWindow == 0 || j - i <= (size_t)pairWindow); j++) {
            src.push_back((int32_t)i); dst.push_back((int32_t)j);
            pts.insert(pts.end(), kp.begin() + 2 * kp_ptr[i], kp.begin() + 2 * kp_ptr[i + 1]);
            pt_ptr.push_back(pt_ptr.back() + (kp_ptr[i + 1] - kp_ptr[i]));
        }
    const int n_pairs = (int)src.size();
    const size_t n_pts = (size_t)pt_ptr.back();
    std::vector<float> next(2 * n_pts + 2), err(n_pts + 1), dist(n_pts + 1);
    std::vector<unsigned char> status(n_pts + 1);
    std::vector<int64_t> pair_ptr((size_t)n_pairs + 1, 0);
    std::vector<int32_t> query(n_pts + 1), train(n_pts + 1);
    int64_t total = 0;
    kp.resize(kp.size() + 2);
    pts.resize(pts.size() + 2);
    int rc = sfmba_flow_track(0, (int)numImages, ptr.data(), pixels.data(), width.data(), height.data(), channels, n_pairs, src.data(), dst.data(),
                              pt_ptr.data(), pts.data(), FLOW_LEVELS, FLOW_RADIUS, FLOW_MAX_ITERS, FLOW_MIN_EIG, next.data(), status.data(), err.data(),
                              nullptr, nullptr, nullptr);
    if (rc == SFMBA_OK)                                   // at most one match per query: the capacity always suffices
        rc = sfmba_flow_match(0, (int)numImages, kp_ptr.data(), kp.data(), n_pairs, dst.data(), pt_ptr.data(), next.data(), status.data(), err.data(),
                              FLOW_MAX_ERR, FLOW_SNAP_RADIUS, FLOW_RATIO, pair_ptr.data(), query.data(), train.data(), dist.data(), (int64_t)n_pts, &total);
    if (rc != SFMBA_OK) {
        std::fprintf(stderr, "createFlowMatchMatrix failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return false;
    }
    for (int p = 0; p < n_pairs; ++p) {
        Matching& m = featureMatchMatrix[(size_t)src[(size_t)p]][(size_t)dst[(size_t)p]];
        m.reserve((size_t)(pair_ptr[(size_t)p + 1] - pair_ptr[(size_t)p]));
        for (int64_t e = pair_ptr[(size_t)p]; e < pair_ptr[(size_t)p + 1]; ++e) {
            cv::DMatch d(query[(size_t)e], train[(size_t)e], dist[(size_t)e]);
            d.imgIdx = 0;
            m.push_back(d);
        }
    }
    return true;
}

std::map<float, ImagePair> SfMFeatureMatching::sortViewsForBaseline(const std::vector<Features>& imageFeatures, const MatchMatrix& featureMatchMatrix) {
    const size_t MIN_POINT_COUNT_FOR_HOMOGRAPHY = 100;                          // SfM.cpp:47
    const size_t numImages = imageFeatures.size();
    std::vector<const Features*> images;
    for (const Features& f : imageFeatures) images.push_back(&f);
    std::vector<int> left, right, inliers;
    std::vector<const Matching*> matches;
    for (size_t i = 0; i + 1 < numImages; i++)
        for (size_t j = i + 1; j < numImages; j++)
            if (featureMatchMatrix[i][j].size() >= MIN_POINT_COUNT_FOR_HOMOGRAPHY) {
                left.push_back((int)i); right.push_back((int)j); matches.push_back(&featureMatchMatrix[i][j]);
            }
    SfMStereoUtilities::findHomographyInliersBatch(images, left, right, matches, inliers);
    // the reference's loop and its insertion order (SfM.cpp:341-361): the map keeps the LAST pair of every key
    std::map<float, ImagePair> matchesSizes;
    size_t q = 0;
    for (size_t i = 0; i + 1 < numImages; i++)
        for (size_t j = i + 1; j < numImages; j++) {
            if (featureMatchMatrix[i][j].size() < MIN_POINT_COUNT_FOR_HOMOGRAPHY) {
                matchesSizes[1.0] = { i, j };
                continue;
            }
            const float inliersRatio = (float)inliers[q++] / (float)(featureMatchMatrix[i][j].size());
            matchesSizes[inliersRatio] = { i, j };
        }
    return matchesSizes;
}

}  // namespace sfmtoylib
