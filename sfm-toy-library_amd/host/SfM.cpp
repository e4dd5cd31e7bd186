// SfM.cpp -- see SfM.h: the reference's orchestration (SfMToyLib/SfM.cpp:63-469) restated over the shim members of this directory.
#include "SfM.h"

#include <dirent.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <chrono>
#include <cstdlib>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <utility>

#include "SfM2DFeatureUtilities.h"
#include "SfMBundleAdjustmentUtils.h"
#include "SfMExport.h"
#include "SfMImageUtilities.h"
#include "SfMStereoUtilities.h"
#include "../csrc/png_inflate.h"        // the CRC-32 and the Adler-32 of the PNG reader, for the atlas writer

namespace sfmtoylib {

namespace {

// the next header token of a PNM file: white space and '#' comments skipped; empty at the end of the file
std::string pnmToken(std::istream& in) {
    std::string tok;
    int c = in.get();
    while (c != EOF && (std::isspace(c) || c == '#')) {
        if (c == '#') while (c != EOF && c != '\n') c = in.get();
        else c = in.get();
    }
    while (c != EOF && !std::isspace(c)) { tok.push_back((char)c); c = in.get(); }
    return tok;                                        // the single white-space byte behind the token has been consumed
}

bool pnmNumber(const std::string& tok, long& value) {
    if (tok.empty() || tok.size() > 9) return false;
    for (char ch : tok) if (ch < '0' || ch > '9') return false;
    value = std::atol(tok.c_str());
    return true;
}

// P5 -> CV_8U, P6 -> CV_8UC3 with the bytes of a pixel turned from R, G, B into OpenCV's B, G, R
bool readPnm(const std::string& path, cv::Mat& image) {
    std::ifstream in(path.c_str(), std::ios::binary);
    if (!in) return false;
    const std::string magic = pnmToken(in);
    if (magic != "P5" && magic != "P6") return false;
    long w = 0, h = 0, maxval = 0;
    if (!pnmNumber(pnmToken(in), w) || !pnmNumber(pnmToken(in), h) || !pnmNumber(pnmToken(in), maxval)) return false;
    if (w < 1 || h < 1 || w > 16384 || h > 16384 || maxval != 255) return false;
    const int channels = magic == "P6" ? 3 : 1;
    image = cv::Mat((int)h, (int)w, channels == 3 ? CV_8UC3 : CV_8U);
    for (int r = 0; r < (int)h; ++r) {
        unsigned char* row = image.ptr<unsigned char>(r);
        in.read(reinterpret_cast<char*>(row), (std::streamsize)(w * channels));
        if (in.gcount() != (std::streamsize)(w * channels)) return false;
        if (channels == 3)
            for (long x = 0; x < w; ++x) std::swap(row[3 * x], row[3 * x + 2]);
    }
    return true;
}

// Adds the wall time of its scope to one entry of SfM::mStageMs; does nothing (no clock is read) when `sums` is null, which is the
// case unless SFMBA_SFM_TIMING is set.
struct StageClock {
    double* sum;
    std::chrono::steady_clock::time_point t0;
    StageClock(double* sums, int stage) : sum(sums ? sums + stage : nullptr) { if (sum) t0 = std::chrono::steady_clock::now(); }
    ~StageClock() { if (sum) *sum += 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
const char* const stageNames[] = { "extract", "match", "rank", "baseline_pose", "baseline_triangulate", "associate", "pnp", "pair_poses",
                                   "triangulate", "merge", "adjust" };

std::string lowerExtension(const std::string& name) {
    const size_t dot = name.rfind('.');
    std::string ext = dot == std::string::npos ? std::string() : name.substr(dot);
    for (char& ch : ext) ch = (char)std::tolower((unsigned char)ch);
    return ext;
}

}  // namespace

SfM::SfM(const float downscale) :
        mConsoleDebugLevel(LOG_INFO),
        mDownscaleFactor(downscale),
        mMergeFeatureMatchDistance(20.0f),                 // MERGE_CLOUD_FEATURE_MIN_MATCH_DISTANCE, SfM.cpp:51
        mFeatureType(FEATURES_ORB),
        mMatcherType(MATCHER_DESCRIPTORS),
        mFlowPairWindow(0),
        mFeaturesGiven(false),
        mDownscaleApplied(false),
        mCols(0), mRows(0),
        mMeshOkay(false),
        mCleanOkay(false),
        mDecimateOkay(false),
        mRunOkay(false),
        mTiming(false) {
    for (double& ms : mStageMs) ms = 0.0;
}

SfM::~SfM() {
}

bool SfM::setImagesDirectory(const std::string& directoryPath) {
    DIR* dir = opendir(directoryPath.c_str());
    if (!dir) {
        std::cerr << "setImagesDirectory: " << directoryPath << " cannot be read as a directory" << std::endl;
        return false;
    }
    std::vector<std::string> names;
    while (const dirent* entry = readdir(dir)) {
        const std::string ext = lowerExtension(entry->d_name);
        if (ext == ".pgm" || ext == ".ppm" || ext == ".jpg" || ext == ".jpeg" || ext == ".png") names.push_back(entry->d_name);
    }
    closedir(dir);
    std::sort(names.begin(), names.end());
    if (names.empty()) {
        std::cerr << "setImagesDirectory: no .pgm / .ppm / .jpg / .jpeg / .png file in " << directoryPath << std::endl;
        return false;
    }
    // the PNM files are read here; the JPEG and the PNG files go to the device in ONE decode call each, which also applies the
    // downscale factor
    std::vector<cv::Mat> images(names.size());
    std::vector<size_t> pnm, jpeg;
    std::vector<std::string> jpegPaths;
    for (size_t i = 0; i < names.size(); i++) {
        const std::string path = directoryPath + "/" + names[i];
        const std::string ext = lowerExtension(names[i]);
        if (ext == ".jpg" || ext == ".jpeg" || ext == ".png") {
            jpeg.push_back(i);
            jpegPaths.push_back(path);
            continue;
        }
        pnm.push_back(i);
        if (!readPnm(path, images[i])) {
            std::cerr << "setImagesDirectory: " << path << " is not a complete binary PGM / PPM file of maxval 255" << std::endl;
            return false;
        }
    }
    if (!jpeg.empty()) {
        std::vector<cv::Mat> decoded;
        if (!SfMImageUtilities::readImages(jpegPaths, mDownscaleFactor, decoded)) return false;
        for (size_t k = 0; k < jpeg.size(); k++) images[jpeg[k]] = decoded[k];
    }
    for (size_t i = 0; i < names.size(); i++)
        if (images[i].type() != images[0].type()) {
            std::cerr << "setImagesDirectory: " << directoryPath << "/" << names[i] << " is not of the kind (gray / colour) of the files before it" << std::endl;
            return false;
        }
    // the PNM images in ONE resize call; at factor 1 they touch no device
    if (!pnm.empty() && mDownscaleFactor != 1.0f) {
        std::vector<cv::Mat> full, resized;
        for (size_t k = 0; k < pnm.size(); k++) full.push_back(images[pnm[k]]);
        if (!SfMImageUtilities::resizeImages(full, mDownscaleFactor, resized)) return false;
        for (size_t k = 0; k < pnm.size(); k++) images[pnm[k]] = resized[k];
    }
    if (mConsoleDebugLevel <= LOG_DEBUG) std::cout << "[sfm] " << names.size() << " images read from " << directoryPath << std::endl;
    setImages(images);
    mDownscaleApplied = true;
    return true;
}

void SfM::setImages(const std::vector<cv::Mat>& images) {
    mImages = images;
    mImageFeatures.clear();
    mRunOkay = false;
    mFeaturesGiven = false;
    mDownscaleApplied = false;
    mCols = images.empty() ? 0 : images[0].cols;
    mRows = images.empty() ? 0 : images[0].rows;
}

void SfM::setFeatures(const std::vector<Features>& imageFeatures, int cols, int rows) {
    mImages.clear();
    mImageFeatures = imageFeatures;
    mRunOkay = false;
    mFeaturesGiven = true;
    mDownscaleApplied = false;
    mCols = cols;
    mRows = rows;
}

void SfM::say(unsigned int level, const std::string& line) const {
    if (mConsoleDebugLevel > level) return;
    (level >= LOG_WARN ? std::cerr : std::cout) << "[sfm] " << line << std::endl;
}

// K of the contract in SfM.h (integer halves of the image size), its inverse in closed form, no distortion; empty reconstruction
void SfM::startRun(size_t n_views) {
    const float focal = 2500.0f;
    const float centre[2] = { (float)(mCols / 2), (float)(mRows / 2) };
    cv::Mat K(3, 3, CV_32F), Kinv(3, 3, CV_32F);
    for (int d = 0; d < 2; d++) {
        K.at<float>(d, d) = focal;
        K.at<float>(d, 2) = centre[d];
        Kinv.at<float>(d, d) = 1.0f / focal;
        Kinv.at<float>(d, 2) = -centre[d] / focal;
    }
    K.at<float>(2, 2) = Kinv.at<float>(2, 2) = 1.0f;
    mIntrinsics.K = K;
    mIntrinsics.Kinv = Kinv;
    mIntrinsics.distortion = cv::Mat(1, 4, CV_32F);
    mCameraPoses.assign(n_views, cv::Matx34f());
    mDoneViews.clear();
    mGoodViews.clear();
    mReconstructionCloud.clear();
    mAddedViews.clear();
    mFeatureMatchMatrix.clear();
    mDepthMaps.clear();
    mDenseCloud = DenseCloud();
    mMergedCloud = MergedCloud();
    mMesh = Mesh();
    mCleanMesh = Mesh();
    mDecimatedMesh = Mesh();
    mTexturedMesh = TexturedMesh();
    mCleanOkay = false;
    mDecimateOkay = false;
    mMeshOkay = false;
    mDenseJobs.clear();
    mRunOkay = false;
    mTiming = std::getenv("SFMBA_SFM_TIMING") != nullptr;
    for (double& ms : mStageMs) ms = 0.0;
}

ErrorCode SfM::runSfM() {
    const size_t n_views = mFeaturesGiven ? mImageFeatures.size() : mImages.size();
    if (n_views == 0) {
        std::cerr << "runSfM: there are no images and no features" << std::endl;
        return ERROR;
    }
    if (mDownscaleFactor != 1.0f && !mDownscaleApplied) {
        std::cerr << "runSfM: downscale " << mDownscaleFactor << " is refused: only setImagesDirectory applies a factor, images given through setImages "
                  << "and features are taken as they are" << std::endl;
        return ERROR;
    }
    if (mMatcherType == MATCHER_FLOW && mFeaturesGiven) {
        std::cerr << "runSfM: MATCHER_FLOW tracks the key points through the images, and setFeatures gave none" << std::endl;
        return ERROR;
    }
    if (mMatcherType == MATCHER_FLOW && mFlowPairWindow < 0) {
        std::cerr << "runSfM: the flow pair window must be >= 0" << std::endl;
        return ERROR;
    }
    startRun(n_views);
    double* const sums = mTiming ? mStageMs : nullptr;

    if (!mFeaturesGiven) {
        say(LOG_INFO, "stage 1: features of " + std::to_string(n_views) + " images");
        StageClock clock(sums, T_EXTRACT);
        if (!SfMFeatureExtraction::extractFeatures(mImages, mImageFeatures, mFeatureType)) return ERROR;
    }
    say(LOG_INFO, "stage 2: match matrix");
    {
        StageClock clock(sums, T_MATCH);
        if (mMatcherType == MATCHER_FLOW) {
            if (!SfMFeatureMatching::createFlowMatchMatrix(mImages, mImageFeatures, mFeatureMatchMatrix, mFlowPairWindow)) return ERROR;
        } else if (!SfMFeatureMatching::createFeatureMatchMatrix(mImageFeatures, mFeatureMatchMatrix)) return ERROR;
    }
    say(LOG_INFO, "stage 3: baseline pair");
    if (!findBaselineTriangulation()) {
        std::cerr << "runSfM: no pair of views could start the reconstruction" << std::endl;
        return ERROR;
    }
    say(LOG_INFO, "stage 4: remaining views");
    addMoreViewsToReconstruction();
    say(LOG_INFO, "finished: " + std::to_string(mGoodViews.size()) + " of " + std::to_string(n_views) + " views registered, " +
                  std::to_string(mReconstructionCloud.size()) + " points");

    if (mTiming) {
        std::fprintf(stderr, "[sfmba sfm] views %d", (int)n_views);
        for (int stage = 0; stage < T_COUNT; stage++) std::fprintf(stderr, " %s_ms %.3f", stageNames[stage], mStageMs[stage]);
        std::fprintf(stderr, "\n");
    }
    mRunOkay = true;
    return OKAY;
}

// The ranked pairs in key order (lowest homography-inlier ratio first); the first one that has a pose with enough inliers AND
// triangulates becomes the reconstruction.  Pose and cloud outlive a turn of the loop as they do in the reference: a failed pose call
// leaves them untouched, so nothing of an abandoned candidate is carried along.
bool SfM::findBaselineTriangulation() {
    double* const sums = mTiming ? mStageMs : nullptr;
    std::map<float, ImagePair> ranked;
    {
        StageClock clock(sums, T_RANK);
        ranked = SfMFeatureMatching::sortViewsForBaseline(mImageFeatures, mFeatureMatchMatrix);
    }
    cv::Matx34f poseA = cv::Matx34f::eye(), poseB = cv::Matx34f::eye();
    PointCloud seed;
    for (std::map<float, ImagePair>::const_iterator it = ranked.begin(); it != ranked.end(); ++it) {
        const int a = (int)it->second.left, b = (int)it->second.right;
        const std::string name = "pair (" + std::to_string(a) + ", " + std::to_string(b) + ")";
        Matching& entry = mFeatureMatchMatrix[a][b];
        Matching inliers;
        bool ok;
        {
            StageClock clock(sums, T_BASELINE_POSE);
            ok = SfMStereoUtilities::findCameraMatricesFromMatch(mIntrinsics, entry, mImageFeatures[a], mImageFeatures[b], inliers, poseA, poseB);
        }
        if (!ok) {
            say(LOG_WARN, name + " has no relative pose");
            continue;
        }
        // the gate of the reference on the share of matches that survive the pose (float division, as there)
        if ((float)inliers.size() / (float)entry.size() < POSE_INLIERS_MINIMAL_RATIO) {
            say(LOG_TRACE, name + " keeps " + std::to_string(inliers.size()) + " of " + std::to_string(entry.size()) + " matches: too few");
            continue;
        }
        entry.swap(inliers);                           // the match matrix holds the pruned list from here on
        {
            StageClock clock(sums, T_BASELINE_TRIANGULATE);
            ok = SfMStereoUtilities::triangulateViews(mIntrinsics, it->second, entry, mImageFeatures[a], mImageFeatures[b], poseA, poseB, seed);
        }
        if (!ok) {
            say(LOG_WARN, name + " could not be triangulated");
            continue;
        }
        say(LOG_DEBUG, name + " starts the reconstruction with " + std::to_string(seed.size()) + " points");
        mReconstructionCloud.swap(seed);
        mCameraPoses[a] = poseA;
        mCameraPoses[b] = poseB;
        const int both[2] = { a, b };
        mDoneViews.insert(both, both + 2);
        mGoodViews.insert(both, both + 2);
        adjustCurrentBundle();
        return true;
    }
    return false;
}

void SfM::adjustCurrentBundle() {
    StageClock clock(mTiming ? mStageMs : nullptr, T_ADJUST);
    SfMBundleAdjustmentUtils::adjustBundle(mReconstructionCloud, mCameraPoses, mIntrinsics, mImageFeatures);
}

// The view to add next: most 2D-3D matches, the lowest index among equals (the map is walked in ascending view order and only a
// strictly larger count replaces the candidate); when no view has a match, the lowest view that is not done.
int SfM::nextView(const Images2D3DMatches& candidates) const {
    int view = -1;
    size_t most = 0;
    for (Images2D3DMatches::const_iterator it = candidates.begin(); it != candidates.end(); ++it)
        if (it->second.points2D.size() > most) {
            most = it->second.points2D.size();
            view = it->first;
        }
    for (int v = 0; view < 0 && v < (int)mCameraPoses.size(); v++)
        if (mDoneViews.find(v) == mDoneViews.end()) view = v;
    return view;
}

// New points of a freshly posed view: its pairs with every good view (ascending; the lower index is the left image, because only
// the upper triangle of the match matrix is filled) go through ONE pose call, whose pruned lists replace the matrix entries -- an
// empty list for a pair without a pose --, then through ONE triangulation call under the reconstruction's poses; the clouds are
// merged in pair order.  Returns whether the triangulation call succeeded.
bool SfM::triangulateAgainstGoodViews(int view) {
    double* const sums = mTiming ? mStageMs : nullptr;
    std::vector<const Features*> images;
    for (size_t v = 0; v < mImageFeatures.size(); v++) images.push_back(&mImageFeatures[v]);
    std::vector<int> left, right;
    std::vector<const Matching*> lists;
    std::vector<cv::Matx34f> poseLeft, poseRight;
    for (std::set<int>::const_iterator g = mGoodViews.begin(); g != mGoodViews.end(); ++g) {
        left.push_back(std::min(*g, view));
        right.push_back(std::max(*g, view));
        lists.push_back(&mFeatureMatchMatrix[left.back()][right.back()]);
        poseLeft.push_back(mCameraPoses[left.back()]);
        poseRight.push_back(mCameraPoses[right.back()]);
    }
    const size_t n_pairs = left.size();
    std::vector<unsigned char> ok;
    {
        std::vector<Matching> pruned;
        std::vector<cv::Matx34f> relLeft, relRight;    // the pairs' own relative poses: only their inlier sets are used
        StageClock clock(sums, T_PAIR_POSES);
        SfMStereoUtilities::findCameraMatricesFromMatchBatch(mIntrinsics, images, left, right, lists, ok, pruned, relLeft, relRight);
        for (size_t p = 0; p < n_pairs; p++) mFeatureMatchMatrix[left[p]][right[p]].swap(pruned[p]);
    }
    std::vector<PointCloud> clouds;
    bool triangulated;
    {
        StageClock clock(sums, T_TRIANGULATE);
        triangulated = SfMStereoUtilities::triangulateViewsBatch(mIntrinsics, images, left, right, lists, poseLeft, poseRight, ok, clouds);
    }
    if (!triangulated) {
        say(LOG_WARN, "view " + std::to_string(view) + ": the triangulation against the good views failed");
        return false;
    }
    StageClock clock(sums, T_MERGE);
    for (size_t p = 0; p < n_pairs; p++) {
        SfMAssociation::mergeNewPointCloud(mReconstructionCloud, clouds[p], mFeatureMatchMatrix, nullptr, nullptr, nullptr, mMergeFeatureMatchDistance);
        say(LOG_DEBUG, "views " + std::to_string(left[p]) + " / " + std::to_string(right[p]) + ": " + std::to_string(clouds[p].size()) +
                       " points triangulated, cloud now " + std::to_string(mReconstructionCloud.size()));
    }
    return true;
}

void SfM::addMoreViewsToReconstruction() {
    double* const sums = mTiming ? mStageMs : nullptr;
    const size_t n_views = mCameraPoses.size();
    while (mDoneViews.size() < n_views) {
        Images2D3DMatches candidates;
        {
            StageClock clock(sums, T_ASSOCIATE);
            candidates = SfMAssociation::find2D3DMatches(n_views, mDoneViews, mReconstructionCloud, mFeatureMatchMatrix, mImageFeatures);
        }
        const int view = nextView(candidates);
        mDoneViews.insert(view);                       // done whatever follows: a view is tried once

        AddedView turn = { view, false, 0 };
        cv::Matx34f pose;
        {
            StageClock clock(sums, T_PNP);
            turn.posed = SfMStereoUtilities::findCameraPoseFrom2D3DMatch(mIntrinsics, candidates[view], pose);
        }
        say(turn.posed ? LOG_DEBUG : LOG_WARN, "view " + std::to_string(view) + " with " + std::to_string(candidates[view].points2D.size()) +
                                               " 2D-3D matches: " + (turn.posed ? "posed" : "no pose, left out"));
        if (turn.posed) {
            mCameraPoses[view] = pose;
            const bool grown = triangulateAgainstGoodViews(view);
            turn.cloudSize = mReconstructionCloud.size();
            if (grown) adjustCurrentBundle();
            mGoodViews.insert(view);
        } else {
            turn.cloudSize = mReconstructionCloud.size();
        }
        mAddedViews.push_back(turn);
    }
}

ErrorCode SfM::densify(const DenseParams& params) {
    mDepthMaps.clear();
    mDenseCloud = DenseCloud();
    mMergedCloud = MergedCloud();
    mMesh = Mesh();
    mCleanMesh = Mesh();
    mDecimatedMesh = Mesh();
    mTexturedMesh = TexturedMesh();
    mCleanOkay = false;
    mDecimateOkay = false;
    mMeshOkay = false;
    mDenseJobs.clear();
    if (mFeaturesGiven || mImages.empty()) {
        std::cerr << "densify: there are no pixels: the run started from setFeatures, and depth maps need the images" << std::endl;
        return ERROR;
    }
    if (!mRunOkay || mCameraPoses.size() != mImages.size()) {
        std::cerr << "densify: needs a runSfM on these images that returned OKAY" << std::endl;
        return ERROR;
    }
    if (params.maxSources < 1 || params.maxSources > 4) {
        std::cerr << "densify: maxSources must be in 1..4" << std::endl;
        return ERROR;
    }
    const std::vector<int> good(mGoodViews.begin(), mGoodViews.end());
    // camera centres and the sorted depths of every good view's own cloud points, in double
    std::map<int, std::vector<double> > centre, depths;
    for (int v : good) {
        const cv::Matx34f& P = mCameraPoses[(size_t)v];
        std::vector<double>& C = centre[v];
        for (int j = 0; j < 3; j++) C.push_back(-(((double)P(0, j) * (double)P(0, 3) + (double)P(1, j) * (double)P(1, 3)) + (double)P(2, j) * (double)P(2, 3)));
        depths[v];
    }
    for (const Point3DInMap& point : mReconstructionCloud)
        for (const auto& origin : point.originatingViews) {
            if (!depths.count(origin.first)) continue;
            const cv::Matx34f& P = mCameraPoses[(size_t)origin.first];
            const double z = (((double)P(2, 0) * (double)point.p.x + (double)P(2, 1) * (double)point.p.y) + (double)P(2, 2) * (double)point.p.z) + (double)P(2, 3);
            if (std::isfinite(z) && z > 0.0) depths[origin.first].push_back(z);
        }
    for (int v : good) {
        std::vector<double>& z = depths[v];
        std::sort(z.begin(), z.end());
        const size_t m = z.size();
        if (m < 8) continue;
        std::vector<std::pair<double, int> > others;
        for (int o : good) {
            if (o == v) continue;
            const double dx = centre[o][0] - centre[v][0], dy = centre[o][1] - centre[v][1], dz = centre[o][2] - centre[v][2];
            others.push_back(std::make_pair((dx * dx + dy * dy) + dz * dz, o));
        }
        if (others.empty()) continue;
        std::sort(others.begin(), others.end());           // ascending distance, then index
        DenseJob job;
        job.reference = v;
        for (size_t k = 0; k < others.size() && (int)k < params.maxSources; k++) job.sources.push_back(others[k].second);
        job.zNear = (float)(z[(5 * m) / 100] / 1.25);
        job.zFar = (float)(z[std::min(m - 1, (95 * m) / 100)] * 1.25);
        mDenseJobs.push_back(job);
    }
    say(LOG_INFO, "dense: " + std::to_string(mDenseJobs.size()) + " sweep jobs over " + std::to_string(good.size()) + " good views");

    const bool timing = std::getenv("SFMBA_SFM_TIMING") != nullptr;
    double ms[2] = { 0.0, 0.0 };
    std::vector<cv::Mat> depthMaps, scores;
    {
        StageClock clock(timing ? ms : nullptr, 0);
        if (!SfMDenseUtilities::computeDepthMaps(mImages, mIntrinsics, mCameraPoses, mDenseJobs, params, depthMaps, scores)) {
            mDenseJobs.clear();
            return ERROR;
        }
    }
    std::vector<cv::Mat> perView(mImages.size());
    std::vector<std::vector<int> > checks(mImages.size());
    for (size_t j = 0; j < mDenseJobs.size(); j++) {
        perView[(size_t)mDenseJobs[j].reference] = depthMaps[j];
        checks[(size_t)mDenseJobs[j].reference] = mDenseJobs[j].sources;
    }
    bool ok = true;
    DenseCloud cloud;
    if (!mDenseJobs.empty()) {
        StageClock clock(timing ? ms : nullptr, 1);
        cloud = SfMDenseUtilities::fuseDepthMaps(mImages, mIntrinsics, mCameraPoses, perView, checks, params, &ok);
    }
    if (!ok) {
        mDenseJobs.clear();
        return ERROR;
    }
    mDepthMaps = perView;
    mDenseCloud = cloud;
    say(LOG_INFO, "dense: " + std::to_string(mDenseCloud.points.size()) + " points");
    if (timing)
        std::fprintf(stderr, "[sfmba sfm dense] jobs %d dense_sweep_ms %.3f dense_fuse_ms %.3f points %lld\n", (int)mDenseJobs.size(), ms[0], ms[1],
                     (long long)mDenseCloud.points.size());
    return OKAY;
}

bool SfM::saveDenseCloudToPLY(const std::string& prefix) {
    std::ofstream file(prefix + "_dense.ply");
    // the header of the points file (SfMExport.cpp), padding included
    file << "ply                 " << std::endl
         << "format ascii 1.0    " << std::endl
         << "element vertex " << mDenseCloud.points.size() << std::endl
         << "property float x    " << std::endl
         << "property float y    " << std::endl
         << "property float z    " << std::endl
         << "property uchar red  " << std::endl
         << "property uchar green" << std::endl
         << "property uchar blue " << std::endl
         << "end_header          " << std::endl;
    for (size_t i = 0; i < mDenseCloud.points.size(); i++) {
        const cv::Point3f& p = mDenseCloud.points[i];
        const unsigned char* bgr = &mDenseCloud.bgr[3 * i];
        file << p.x << " " << p.y << " " << p.z << " " << (int)bgr[2] << " " << (int)bgr[1] << " " << (int)bgr[0] << " " << std::endl;
    }
    file.close();
    return !file.fail();
}

ErrorCode SfM::mergeDenseCloud(float voxel, int minCount, float maxRelStep) {
    mMergedCloud = MergedCloud();
    if (mDenseJobs.empty() || mDepthMaps.size() != mImages.size()) {
        std::cerr << "mergeDenseCloud: needs a densify on these images that returned OKAY" << std::endl;
        return ERROR;
    }
    if (!std::isfinite(voxel) || voxel < 0.0f || minCount < 1) {
        std::cerr << "mergeDenseCloud: voxel must be finite and >= 0 (0 = auto), minCount >= 1" << std::endl;
        return ERROR;
    }
    if (voxel == 0.0f) {
        // the footprint of a pixel at the typical depth: the median over the jobs of the geometric mean of a job's depth range
        std::vector<double> g;
        for (const DenseJob& job : mDenseJobs) g.push_back(std::sqrt((double)job.zNear * (double)job.zFar));
        std::sort(g.begin(), g.end());
        voxel = (float)(g[g.size() / 2] / (double)mIntrinsics.K.at<float>(0, 0));
    }
    const bool timing = std::getenv("SFMBA_SFM_TIMING") != nullptr;
    double ms[2] = { 0.0, 0.0 };
    std::vector<cv::Mat> normalMaps;
    {
        StageClock clock(timing ? ms : nullptr, 0);
        if (!SfMDenseUtilities::computeNormals(mImages, mIntrinsics, mCameraPoses, mDepthMaps, maxRelStep, normalMaps)) return ERROR;
    }
    Points3f normals;
    normals.reserve(mDenseCloud.points.size());
    for (size_t i = 0; i < mDenseCloud.points.size(); i++) {
        const float* n = normalMaps[(size_t)mDenseCloud.views[i]].ptr<float>(0) + 3 * (size_t)mDenseCloud.pixels[i];
        normals.push_back(cv::Point3f(n[0], n[1], n[2]));
    }
    bool ok = true;
    MergedCloud merged;
    {
        StageClock clock(timing ? ms : nullptr, 1);
        merged = SfMDenseUtilities::mergeCloud(mDenseCloud, normals, voxel, minCount, &ok);
    }
    if (!ok) return ERROR;
    mMergedCloud = merged;
    say(LOG_INFO, "dense: " + std::to_string(mDenseCloud.points.size()) + " points merged into " + std::to_string(mMergedCloud.points.size()) +
                      " at voxel " + std::to_string(voxel));
    if (timing)
        std::fprintf(stderr, "[sfmba sfm merge] voxel %.9g merge_normals_ms %.3f merge_cloud_ms %.3f points %lld merged %lld\n", (double)voxel, ms[0],
                     ms[1], (long long)mDenseCloud.points.size(), (long long)mMergedCloud.points.size());
    return OKAY;
}

bool SfM::saveMergedDenseCloudToPLY(const std::string& prefix) {
    std::ofstream file(prefix + "_dense_merged.ply");
    const bool haveNormals = mMergedCloud.normals.size() == mMergedCloud.points.size();
    const bool haveBgr = mMergedCloud.bgr.size() == 3 * mMergedCloud.points.size();
    // the header of the points file (SfMExport.cpp), padding included, with the normal between position and colour
    file << "ply                 " << std::endl
         << "format ascii 1.0    " << std::endl
         << "element vertex " << mMergedCloud.points.size() << std::endl
         << "property float x    " << std::endl
         << "property float y    " << std::endl
         << "property float z    " << std::endl
         << "property float nx   " << std::endl
         << "property float ny   " << std::endl
         << "property float nz   " << std::endl
         << "property uchar red  " << std::endl
         << "property uchar green" << std::endl
         << "property uchar blue " << std::endl
         << "end_header          " << std::endl;
    for (size_t i = 0; i < mMergedCloud.points.size(); i++) {
        const cv::Point3f& p = mMergedCloud.points[i];
        const cv::Point3f n = haveNormals ? mMergedCloud.normals[i] : cv::Point3f(0.0f, 0.0f, 0.0f);
        const unsigned char none[3] = { 0, 0, 0 };
        const unsigned char* bgr = haveBgr ? &mMergedCloud.bgr[3 * i] : none;
        file << p.x << " " << p.y << " " << p.z << " " << n.x << " " << n.y << " " << n.z << " " << (int)bgr[2] << " " << (int)bgr[1] << " "
             << (int)bgr[0] << " " << std::endl;
    }
    file.close();
    return !file.fail();
}

ErrorCode SfM::meshDenseCloud(const MeshParams& params) {
    mMesh = Mesh();
    mCleanMesh = Mesh();
    mDecimatedMesh = Mesh();
    mTexturedMesh = TexturedMesh();
    mCleanOkay = false;
    mDecimateOkay = false;
    mMeshOkay = false;
    if (mDenseJobs.empty() || mDepthMaps.size() != mImages.size()) {
        std::cerr << "meshDenseCloud: needs a densify on these images that returned OKAY" << std::endl;
        return ERROR;
    }
    if (!std::isfinite(params.voxel) || params.voxel < 0.0f || params.resolution < 2 || !std::isfinite(params.truncVoxels) ||
        !(params.truncVoxels > 0.0f) || params.minWeight < 1 || params.minWeight > 65535) {
        std::cerr << "meshDenseCloud: voxel must be finite and >= 0 (0 = from resolution), resolution >= 2, truncVoxels finite and > 0, "
                     "minWeight in 1..65535" << std::endl;
        return ERROR;
    }
    if (params.fillIterations < 0 || params.fillIterations > 254 || params.fillMinNeighbours < 1 || params.fillMinNeighbours > 6) {
        std::cerr << "meshDenseCloud: fillIterations must be in 0..254 (0 = no hole filling) and fillMinNeighbours in 1..6" << std::endl;
        return ERROR;
    }
    // the box of the dense cloud without its outermost hundredths (the rule is at the top of SfM.h)
    float lo[3], hi[3];
    double side[3], longest = 0.0;
    for (int a = 0; a < 3; a++) {
        std::vector<float> c;
        c.reserve(mDenseCloud.points.size());
        for (const cv::Point3f& p : mDenseCloud.points) {
            const float v = a == 0 ? p.x : a == 1 ? p.y : p.z;
            if (std::isfinite(v)) c.push_back(v);
        }
        if (c.empty()) {
            std::cerr << "meshDenseCloud: the dense cloud has no finite point" << std::endl;
            return ERROR;
        }
        std::sort(c.begin(), c.end());
        lo[a] = c[c.size() / 100];
        hi[a] = c[(99 * c.size()) / 100];
        side[a] = (double)hi[a] - (double)lo[a];
        longest = std::max(longest, side[a]);
    }
    MeshGrid grid;
    grid.voxel = params.voxel == 0.0f ? (float)(longest / (double)(params.resolution - 1)) : params.voxel;
    if (!std::isfinite(grid.voxel) || !(grid.voxel > 0.0f)) {
        std::cerr << "meshDenseCloud: the dense cloud's box is empty: give a voxel" << std::endl;
        return ERROR;
    }
    grid.trunc = params.truncVoxels * grid.voxel;
    const double pad = (double)grid.trunc + (double)grid.voxel;
    int dims[3];
    float origin[3];
    for (int a = 0; a < 3; a++) {
        origin[a] = (float)((double)lo[a] - pad);
        const double cells = std::floor((side[a] + (pad + pad)) / (double)grid.voxel) + 2.0;
        dims[a] = cells < 1024.0 ? (int)cells : 1024;
    }
    grid.origin = cv::Point3f(origin[0], origin[1], origin[2]);
    grid.nx = dims[0]; grid.ny = dims[1]; grid.nz = dims[2];
    const bool timing = std::getenv("SFMBA_SFM_TIMING") != nullptr;
    double ms[1] = { 0.0 };
    bool ok = true;
    Mesh mesh;
    {
        StageClock clock(timing ? ms : nullptr, 0);
        if (params.fillIterations == 0)
            mesh = SfMDenseUtilities::meshDepthMaps(mImages, mIntrinsics, mCameraPoses, mDepthMaps, grid, params.minWeight, &ok);
        else                                                     // ONE sfmba_tsdf_mesh_fill call; mesh.filled is set
            mesh = SfMDenseUtilities::meshDepthMaps(mImages, mIntrinsics, mCameraPoses, mDepthMaps, grid, params.minWeight, params.fillIterations,
                                                    params.fillMinNeighbours, &ok);
    }
    if (!ok) return ERROR;
    mMesh = mesh;
    mMeshOkay = true;
    say(LOG_INFO, "mesh: " + std::to_string(mMesh.vertices.size()) + " vertices, " + std::to_string(mMesh.triangles.size() / 3) + " triangles on a " +
                      std::to_string(grid.nx) + " x " + std::to_string(grid.ny) + " x " + std::to_string(grid.nz) + " grid at voxel " +
                      std::to_string(grid.voxel));
    if (!mMesh.filled.empty())
        say(LOG_INFO, "mesh: " + std::to_string(std::count(mMesh.filled.begin(), mMesh.filled.end(), (unsigned char)1)) +
                          " vertices made by the hole filling (" + std::to_string(params.fillIterations) + " passes)");
    if (timing)
        std::fprintf(stderr, "[sfmba sfm mesh] voxel %.9g trunc %.9g grid %d %d %d mesh_ms %.3f vertices %lld triangles %lld\n", (double)grid.voxel,
                     (double)grid.trunc, grid.nx, grid.ny, grid.nz, ms[0], (long long)mMesh.vertices.size(), (long long)(mMesh.triangles.size() / 3));
    return OKAY;
}

const Mesh& SfM::getMesh() const { return mMesh; }

bool SfM::saveMeshToPLY(const std::string& prefix) {
    std::ofstream file(prefix + "_mesh.ply");
    const bool haveBgr = mMesh.bgr.size() == 3 * mMesh.vertices.size();
    // the header of the points file (SfMExport.cpp), padding included, then the faces
    file << "ply                 " << std::endl
         << "format ascii 1.0    " << std::endl
         << "element vertex " << mMesh.vertices.size() << std::endl
         << "property float x    " << std::endl
         << "property float y    " << std::endl
         << "property float z    " << std::endl
         << "property uchar red  " << std::endl
         << "property uchar green" << std::endl
         << "property uchar blue " << std::endl
         << "element face " << mMesh.triangles.size() / 3 << std::endl
         << "property list uchar int vertex_indices" << std::endl
         << "end_header          " << std::endl;
    for (size_t i = 0; i < mMesh.vertices.size(); i++) {
        const cv::Point3f& p = mMesh.vertices[i];
        const unsigned char none[3] = { 0, 0, 0 };
        const unsigned char* bgr = haveBgr ? &mMesh.bgr[3 * i] : none;
        file << p.x << " " << p.y << " " << p.z << " " << (int)bgr[2] << " " << (int)bgr[1] << " " << (int)bgr[0] << " " << std::endl;
    }
    for (size_t t = 0; t + 2 < mMesh.triangles.size(); t += 3)
        file << "3 " << mMesh.triangles[t] << " " << mMesh.triangles[t + 1] << " " << mMesh.triangles[t + 2] << std::endl;
    file.close();
    return !file.fail();
}

ErrorCode SfM::cleanMesh(const MeshCleanParams& params) {
    mCleanMesh = Mesh();
    mDecimatedMesh = Mesh();
    mTexturedMesh = TexturedMesh();
    mCleanOkay = false;
    mDecimateOkay = false;
    if (!mMeshOkay) {
        std::cerr << "cleanMesh: needs a meshDenseCloud that returned OKAY" << std::endl;
        return ERROR;
    }
    const bool timing = std::getenv("SFMBA_SFM_TIMING") != nullptr;
    double ms[1] = { 0.0 };
    bool ok = true;
    Mesh mesh;
    {
        StageClock clock(timing ? ms : nullptr, 0);
        mesh = SfMDenseUtilities::cleanMesh(mMesh, params, &ok);
    }
    if (!ok) return ERROR;
    mCleanMesh = mesh;
    mCleanOkay = true;
    say(LOG_INFO, "clean mesh: " + std::to_string(mCleanMesh.vertices.size()) + " of " + std::to_string(mMesh.vertices.size()) + " vertices, " +
                      std::to_string(mCleanMesh.triangles.size() / 3) + " of " + std::to_string(mMesh.triangles.size() / 3) + " triangles");
    if (timing)
        std::fprintf(stderr, "[sfmba sfm mesh_clean] clean_ms %.3f vertices %lld triangles %lld\n", ms[0], (long long)mCleanMesh.vertices.size(),
                     (long long)(mCleanMesh.triangles.size() / 3));
    return OKAY;
}

const Mesh& SfM::getCleanMesh() const { return mCleanMesh; }

// a mesh with normals, ASCII: x y z, nx ny nz, red green blue per vertex, then the faces
static bool writeMeshWithNormalsToPLY(const std::string& path, const Mesh& m) {
    std::ofstream file(path);
    const bool haveBgr = m.bgr.size() == 3 * m.vertices.size(), haveNormals = m.normals.size() == 3 * m.vertices.size();
    // the header of the mesh file with the normals of the merged cloud's file between the position and the colour
    file << "ply                 " << std::endl
         << "format ascii 1.0    " << std::endl
         << "element vertex " << m.vertices.size() << std::endl
         << "property float x    " << std::endl
         << "property float y    " << std::endl
         << "property float z    " << std::endl
         << "property float nx   " << std::endl
         << "property float ny   " << std::endl
         << "property float nz   " << std::endl
         << "property uchar red  " << std::endl
         << "property uchar green" << std::endl
         << "property uchar blue " << std::endl
         << "element face " << m.triangles.size() / 3 << std::endl
         << "property list uchar int vertex_indices" << std::endl
         << "end_header          " << std::endl;
    for (size_t i = 0; i < m.vertices.size(); i++) {
        const cv::Point3f& p = m.vertices[i];
        const unsigned char none[3] = { 0, 0, 0 };
        const float flat[3] = { 0.0f, 0.0f, 0.0f };
        const unsigned char* bgr = haveBgr ? &m.bgr[3 * i] : none;
        const float* n = haveNormals ? &m.normals[3 * i] : flat;
        file << p.x << " " << p.y << " " << p.z << " " << n[0] << " " << n[1] << " " << n[2] << " " << (int)bgr[2] << " " << (int)bgr[1] << " "
             << (int)bgr[0] << " " << std::endl;
    }
    for (size_t t = 0; t + 2 < m.triangles.size(); t += 3)
        file << "3 " << m.triangles[t] << " " << m.triangles[t + 1] << " " << m.triangles[t + 2] << std::endl;
    file.close();
    return !file.fail();
}

bool SfM::saveCleanMeshToPLY(const std::string& prefix) { return writeMeshWithNormalsToPLY(prefix + "_mesh_clean.ply", mCleanMesh); }

ErrorCode SfM::decimateMesh(const MeshDecimateParams& params) {
    mDecimatedMesh = Mesh();
    mTexturedMesh = TexturedMesh();
    mDecimateOkay = false;
    if (!mMeshOkay) {
        std::cerr << "decimateMesh: needs a meshDenseCloud that returned OKAY" << std::endl;
        return ERROR;
    }
    const Mesh& source = mCleanOkay ? mCleanMesh : mMesh;
    const bool timing = std::getenv("SFMBA_SFM_TIMING") != nullptr;
    double ms[1] = { 0.0 };
    long long stats[4] = { 0, 0, 0, 0 };
    bool ok = true;
    Mesh mesh;
    {
        StageClock clock(timing ? ms : nullptr, 0);
        mesh = SfMDenseUtilities::decimateMesh(source, params, &ok, stats);
    }
    if (!ok) return ERROR;
    mDecimatedMesh = mesh;
    mDecimateOkay = true;
    say(LOG_INFO, "decimated mesh: " + std::to_string(mDecimatedMesh.vertices.size()) + " of " + std::to_string(source.vertices.size()) + " vertices, " +
                      std::to_string(mDecimatedMesh.triangles.size() / 3) + " of " + std::to_string(source.triangles.size() / 3) + " triangles (" +
                      (mCleanOkay ? "the clean mesh" : "the mesh") + "); " + std::to_string(stats[0]) + " clusters, " + std::to_string(stats[1]) +
                      " triangles collapsed, " + std::to_string(stats[2]) + " duplicates, " + std::to_string(stats[3]) + " clusters took the mean");
    if (timing)
        std::fprintf(stderr, "[sfmba sfm mesh_decimate] decimate_ms %.3f vertices %lld triangles %lld\n", ms[0], (long long)mDecimatedMesh.vertices.size(),
                     (long long)(mDecimatedMesh.triangles.size() / 3));
    return OKAY;
}

const Mesh& SfM::getDecimatedMesh() const { return mDecimatedMesh; }

bool SfM::saveDecimatedMeshToPLY(const std::string& prefix) { return writeMeshWithNormalsToPLY(prefix + "_mesh_decimated.ply", mDecimatedMesh); }

ErrorCode SfM::textureMesh(const TextureParams& params) {
    mTexturedMesh = TexturedMesh();
    if (!mMeshOkay) {
        std::cerr << "textureMesh: needs a meshDenseCloud that returned OKAY" << std::endl;
        return ERROR;
    }
    if (!std::isfinite(params.occlTolVoxels) || params.occlTolVoxels < 0.0f) {
        std::cerr << "textureMesh: occlTolVoxels must be finite and >= 0" << std::endl;
        return ERROR;
    }
    const Mesh& source = mDecimateOkay ? mDecimatedMesh : mCleanOkay ? mCleanMesh : mMesh;
    const bool timing = std::getenv("SFMBA_SFM_TIMING") != nullptr;
    double ms[1] = { 0.0 };
    bool ok = true;
    TexturedMesh textured;
    {
        StageClock clock(timing ? ms : nullptr, 0);
        textured = SfMDenseUtilities::textureMesh(source, mImages, mIntrinsics, mCameraPoses, mDepthMaps, params, &ok);
    }
    if (!ok) return ERROR;
    mTexturedMesh = textured;
    say(LOG_INFO, "textured mesh: " + std::to_string(mTexturedMesh.textured) + " of " + std::to_string(mTexturedMesh.triangles.size() / 3) +
                      " triangles have a view (" + (mDecimateOkay ? "the decimated mesh" : mCleanOkay ? "the clean mesh" : "the mesh") + "), atlas " + std::to_string(mTexturedMesh.atlas.cols) +
                      " x " + std::to_string(mTexturedMesh.atlas.rows));
    if (mTexturedMesh.smoothed) {
        const long long* st = mTexturedMesh.smoothStats;
        say(LOG_INFO, "smoothed view labels: pairs of neighbours with different views " + std::to_string(st[2]) + " plain, " + std::to_string(st[3]) +
                          " after the diffusion, " + std::to_string(st[4]) + " at the end (" + std::to_string(st[5]) +
                          " more pairs have one side without a view); energy " + std::to_string(st[0]) + " -> " + std::to_string(st[1]) + "; " +
                          std::to_string(st[6]) + " moves in " + std::to_string(st[7]) + " passes");
    }
    if (mTexturedMesh.levelled) {
        const long long* st = mTexturedMesh.levelStats;
        say(LOG_INFO, "levelled colours: " + std::to_string(st[0]) + " nodes (" + std::to_string(st[1]) + " blind), " + std::to_string(st[2]) +
                          " seam vertices; summed spread at the seams " + std::to_string(st[3]) + " -> " + std::to_string(st[4]) +
                          " (1/256 grey level) in " + std::to_string(st[7]) + " passes; largest offset " + std::to_string(st[5]) + "; " +
                          std::to_string(st[6]) + " texels clamped");
    }
    if (timing)
        std::fprintf(stderr, "[sfmba sfm mesh_texture] texture_ms %.3f triangles %lld textured %lld width %d height %d\n", ms[0],
                     (long long)(mTexturedMesh.triangles.size() / 3), mTexturedMesh.textured, mTexturedMesh.atlas.cols, mTexturedMesh.atlas.rows);
    return OKAY;
}

const TexturedMesh& SfM::getTexturedMesh() const { return mTexturedMesh; }

namespace {
void be32(std::vector<unsigned char>& out, uint32_t v) {
    for (int s = 24; s >= 0; s -= 8) out.push_back((unsigned char)(v >> s));
}
void pngChunk(std::vector<unsigned char>& file, const char* type, const std::vector<unsigned char>& data) {
    be32(file, (uint32_t)data.size());
    const size_t at = file.size();
    file.insert(file.end(), type, type + 4);
    file.insert(file.end(), data.begin(), data.end());
    be32(file, sfmba::png_crc32(file.data() + at, data.size() + 4));
}
// a BGR image as an 8-bit RGB PNG: filter 0 on every row, the zlib stream made of STORED blocks (no compression), one IDAT chunk
bool writeStoredPNG(const std::string& path, const cv::Mat& bgr) {
    const size_t w = (size_t)bgr.cols, h = (size_t)bgr.rows;
    std::vector<unsigned char> raw;
    raw.reserve(h * (1 + 3 * w));
    for (size_t y = 0; y < h; ++y) {
        const unsigned char* row = bgr.ptr<unsigned char>((int)y);
        raw.push_back(0);
        for (size_t x = 0; x < w; ++x)
            for (int c = 2; c >= 0; --c) raw.push_back(row[3 * x + c]);
    }
    std::vector<unsigned char> z;
    z.reserve(raw.size() + 5 * (raw.size() / 65535 + 1) + 6);
    z.push_back(0x78);
    z.push_back(0x01);
    for (size_t at = 0; at < raw.size(); at += 65535) {               // (an atlas has at least one row, so there is at least one block)
        const size_t n = std::min<size_t>(65535, raw.size() - at);
        z.push_back(at + n >= raw.size() ? 1 : 0);
        z.push_back((unsigned char)(n & 255)); z.push_back((unsigned char)(n >> 8));
        z.push_back((unsigned char)(~n & 255)); z.push_back((unsigned char)((~n >> 8) & 255));
        z.insert(z.end(), raw.begin() + (std::ptrdiff_t)at, raw.begin() + (std::ptrdiff_t)(at + n));
    }
    be32(z, sfmba::png_adler32(raw.data(), raw.size()));
    std::vector<unsigned char> file = { 0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n' }, ihdr;
    be32(ihdr, (uint32_t)w);
    be32(ihdr, (uint32_t)h);
    const unsigned char kind[5] = { 8, 2, 0, 0, 0 };             // 8 bits, RGB, deflate, adaptive filters, no interlace
    ihdr.insert(ihdr.end(), kind, kind + 5);
    pngChunk(file, "IHDR", ihdr);
    pngChunk(file, "IDAT", z);
    pngChunk(file, "IEND", std::vector<unsigned char>());
    std::ofstream out(path, std::ios::binary);
    out.write(reinterpret_cast<const char*>(file.data()), (std::streamsize)file.size());
    out.close();
    return !out.fail();
}
}  // namespace

bool SfM::saveTexturedMeshToOBJ(const std::string& prefix) {
    const TexturedMesh& m = mTexturedMesh;
    if (m.atlas.empty() || m.uv.size() != 2 * m.triangles.size()) return false;
    const std::string base = prefix.substr(prefix.find_last_of('/') == std::string::npos ? 0 : prefix.find_last_of('/') + 1);
    if (!writeStoredPNG(prefix + "_textured.png", m.atlas)) return false;
    std::ofstream mtl(prefix + "_textured.mtl");
    mtl << "newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd " << base << "_textured.png\n";
    mtl.close();
    if (mtl.fail()) return false;
    FILE* obj = std::fopen((prefix + "_textured.obj").c_str(), "w");
    if (!obj) return false;
    std::fprintf(obj, "mtllib %s_textured.mtl\nusemtl atlas\n", base.c_str());
    for (const cv::Point3f& p : m.vertices) std::fprintf(obj, "v %.9g %.9g %.9g\n", (double)p.x, (double)p.y, (double)p.z);
    const double W = (double)m.atlas.cols, H = (double)m.atlas.rows;
    for (size_t q = 0; q + 1 < m.uv.size(); q += 2) std::fprintf(obj, "vt %.9g %.9g\n", (double)m.uv[q] / W, 1.0 - (double)m.uv[q + 1] / H);
    for (size_t t = 0; t + 2 < m.triangles.size(); t += 3)
        std::fprintf(obj, "f %d/%lld %d/%lld %d/%lld\n", m.triangles[t] + 1, (long long)t + 1, m.triangles[t + 1] + 1, (long long)t + 2, m.triangles[t + 2] + 1,
                     (long long)t + 3);
    const bool bad = std::ferror(obj) != 0;
    return std::fclose(obj) == 0 && !bad;
}

bool SfM::saveCloudAndCamerasToPLY(const std::string& prefix) {
#ifdef SFMBA_HAVE_OPENCV
    return SfMExport::saveCloudAndCamerasToPLY(prefix, mReconstructionCloud, mCameraPoses, mImageFeatures, mImages);
#else
    // B, G, R bytes of every view: a colour image as it is, a gray one with its value in all three, gray 128 without images.  One
    // row and one pixel of slack behind the last row: SfMExport rounds a feature to the nearest pixel without a bounds check.
    std::vector<ImageBGR> images(mCameraPoses.size());
    for (size_t v = 0; v < images.size(); v++) {
        ImageBGR& out = images[v];
        const cv::Mat* src = v < mImages.size() ? &mImages[v] : nullptr;
        out.rows = src ? src->rows : mRows;
        out.cols = src ? src->cols : mCols;
        out.data.assign(((size_t)out.rows * out.cols + out.cols + 1) * 3, 128);
        if (!src) continue;
        for (int r = 0; r < out.rows; r++) {
            const unsigned char* row = src->ptr<unsigned char>(r);
            unsigned char* dst = out.data.data() + (size_t)r * out.cols * 3;
            for (int c = 0; c < out.cols; c++)
                for (int k = 0; k < 3; k++) dst[3 * c + k] = src->type() == CV_8UC3 ? row[3 * c + k] : row[c];
        }
    }
    return SfMExport::saveCloudAndCamerasToPLY(prefix, mReconstructionCloud, mCameraPoses, mImageFeatures, images);
#endif
}

}  // namespace sfmtoylib
