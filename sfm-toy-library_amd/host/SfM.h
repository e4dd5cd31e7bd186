// SfM.h -- sfmtoylib::SfM, the orchestrator of the reference (SfMToyLib/SfM.h:45-149, SfM.cpp:63-469), over the shim members of this
// directory: from images (or features) to camera poses and a point cloud in one call, every stage on the MI355X.
//
// The control flow is the reference's, member for member.  Where the reference is undefined, or where a batched stage changes which
// sample stream a pair draws, the behaviour is fixed here -- tests/sfm_loop.py restates it and tests/test_gpu_sfm_pipeline.py pins it:
//
//   K             f = 2500, centre = (cols / 2, rows / 2) of image 0 in integer division (SfM.cpp:70-72); with setFeatures the cols /
//                 rows given there.  Kinv is the closed form, distortion 1 x 4 zeros.
//   front end     SfMFeatureExtraction::extractFeatures (skipped after setFeatures), SfMFeatureMatching::createFeatureMatchMatrix and
//                 sortViewsForBaseline.  A device failure in any of them makes runSfM return ERROR: the first two report it themselves;
//                 sortViewsForBaseline returns a map and cannot, so its failure shows one step later -- every qualifying pair ranks
//                 with 0 inliers, the pose calls of the baseline fail on the same device, and the ERROR is the baseline's
//                 ("no pair of views could start the reconstruction").
//   baseline      the map of sortViewsForBaseline in key order, each pair through the SINGLE-pair findCameraMatricesFromMatch (seed 0;
//                 the loop leaves at the first pair that works, so it is serial by nature), the POSE_INLIERS_MINIMAL_RATIO gate, the
//                 pruned matches written back to the match matrix, triangulateViews, adjustBundle.  No pair works: runSfM returns
//                 ERROR (the reference goes on with an empty cloud).
//   next view     the not-done view with the most 2D-3D matches, ties to the lowest index; every count 0: the lowest not-done view
//                 (the reference reads an uninitialised variable).  It is marked done; findCameraPoseFrom2D3DMatch; on failure the
//                 loop goes on: the view stays done and not good.
//   new points    the good views in ascending order as ONE findCameraMatricesFromMatchBatch call (pair p draws seed p; left = the
//                 lower view index).  EVERY pair's pruned list replaces its match-matrix entry, an empty list for a failed pair
//                 (the reference's unconditional assignment, SfM.cpp:431).  Then ONE triangulateViewsBatch call with the GLOBAL
//                 poses, SfMAssociation::mergeNewPointCloud pair by pair in that order, adjustBundle if the batch triangulated,
//                 and the view becomes good.
//   merge         a match confirms a merge only if its distance is below setMergeFeatureMatchDistance's value, by default 20, the
//                 reference's MERGE_CLOUD_FEATURE_MIN_MATCH_DISTANCE (SfM.cpp:51).  That constant is on the Hamming scale of ORB.
//                 FLOAT descriptors given through setFeatures (CV_32F: matched by L2 distance) need a value on their own scale --
//                 SIFT-scale distances are 100 to 300, and with 20 no new point would ever be confirmed into a track.
//                 The other way round for setFeatureType(FEATURES_SURF): its descriptors are of unit length, their distances are
//                 <= 2, so the default 20 CONFIRMS EVERY MATCH.  A better default is not chosen here: nobody has measured one.
//   features      setFeatureType chooses the extractor of a run from images: FEATURES_ORB (the default; binary rows, Hamming) or
//                 FEATURES_SURF (sfmba_surf_extract: 64 floats, the L2 branch of the matcher).  It has no effect after setFeatures.
//   matcher       setMatcherType chooses stage 2 of a run from images: MATCHER_DESCRIPTORS (the default: the 2-NN ratio-test matcher over
//                 the descriptors) or MATCHER_FLOW (SfMFeatureMatching::createFlowMatchMatrix: the key points of whichever extractor
//                 is selected, tracked from image i into image j by pyramidal Lucas-Kanade and snapped to j's key points), for
//                 video-like input.  setFlowPairWindow(k), k > 0, matches only views at most k apart; the other entries of the
//                 matrix stay empty and everything downstream reads the matrix as it is.  A flow match's distance is its snap
//                 distance in pixels, at most 2, so the default merge distance 20 CONFIRMS EVERY FLOW MATCH.  After setFeatures
//                 there are no pixels to track in: runSfM returns ERROR for MATCHER_FLOW.
//   end           every view is done.
//   downscale     the factor of the constructor is applied by setImagesDirectory at load time, as in the reference (SfM.cpp:125-129): the
//                 JPEG files and the PNG files in ONE decode call each that also resizes (SfMImageUtilities::readImages), the PNM
//                 images in ONE resize call;
//                 K then comes from the resized image 0.  Images given through setImages and features given through setFeatures are
//                 taken as they are: runSfM refuses downscale != 1 for them (there is nothing to resize in the second case).
//   dense         densify() after a runSfM that returned OKAY on images: one plane-sweep job per good view (include/sfmba.h,
//                 sfmba_depth_sweep), ALL jobs in ONE sweep call, then ONE sfmba_depth_fuse call over the depth maps.
//                 Sources: the up-to-maxSources (default 2) other good views whose camera centres are nearest, listed by ascending
//                 distance, ties to the lower index; centres C_j = -((R_0j t_0 + R_1j t_1) + R_2j t_2) and squared distances
//                 (dx^2 + dy^2) + dz^2 in double.  Depth range: the camera-space z = ((R_20 X + R_21 Y) + R_22 Z) + t_2 (double) of
//                 every cloud point that lists the view in originatingViews, the non-positive and non-finite ones dropped, sorted;
//                 with m values z_near = (float)(z[(5 m) / 100] / 1.25), z_far = (float)(z[min(m - 1, (95 m) / 100)] * 1.25)
//                 (integer division); a view with m < 8, or without another good view, gets no job and no depth map.  The check
//                 views of the fuse are the job's sources.  The defaults of DenseParams (64 planes, radius 3, min_std 2,
//                 min_score 0.6, min_sources 1, rel_tol 0.01, min_consistent 1) are first choices like the merge distance above:
//                 nobody has tuned them.  Nothing is de-duplicated: a surface point seen by three views appears three times.
//                 With DenseParams::sgm set (OFF by default) the ONE sweep call is sfmba_depth_sweep_sgm with sgmP1, sgmP2, sgmPaths,
//                 sgmInvalidCost and sgmUniqueness (8, 64, 8, 127, 5: untuned too): semi-global matching over the cost volume, a
//                 plane for every pixel, min_score not read; the jobs, the fuse and everything after it are the same.
//   merged        mergeDenseCloud(voxel, minCount, maxRelStep) after a densify that returned OKAY: ONE sfmba_depth_normals call over
//                 the depth maps, every dense point takes the normal of its own pixel (through views / pixels of the dense cloud),
//                 then ONE sfmba_cloud_merge (include/sfmba.h): one oriented point per occupied voxel.  voxel == 0 means AUTO, the
//                 footprint of a pixel at the typical depth: g_j = sqrt((double)zNear_j * (double)zFar_j) over the jobs of the
//                 densify, sorted ascending, voxel = (float)(g[n / 2] / (double)fx) (integer division).  The dense cloud itself is
//                 not changed.
//   mesh          meshDenseCloud(params) after a densify that returned OKAY: ONE sfmba_tsdf_mesh call (include/sfmba.h) over the
//                 images and the depth maps of the views that have one: the maps are averaged along the viewing rays in a truncated
//                 signed distance grid, whose zero set leaves as a coloured triangle mesh.  THE GRID: per axis a the finite
//                 coordinates of the dense cloud, sorted ascending, n of them: lo_a = c[n / 100], hi_a = c[(99 n) / 100] (integer
//                 division: floor(0.01 n), floor(0.99 n)), side_a = (double)hi_a - (double)lo_a.  voxel == 0 means
//                 (float)(max side / (double)(resolution - 1)), resolution default 256.  trunc = truncVoxels * voxel (float),
//                 truncVoxels default 4.  The box is padded by pad = (double)trunc + (double)voxel on every side:
//                 origin_a = (float)((double)lo_a - pad), n_a = floor((side_a + (pad + pad)) / (double)voxel) + 2, capped at 1024.
//                 minWeight (the views a grid vertex needs) defaults to 1.  These defaults are first choices like the ones above:
//                 nobody has tuned them.  The dense cloud and the depth maps are not changed.
//   hole filling  params.fillIterations > 0 (default 0: OFF, the call above exactly): ONE sfmba_tsdf_mesh_fill call instead, which
//                 diffuses the signed distance into the undefined grid vertices for that many passes between the integration and
//                 the extraction (an unknown vertex is filled once fillMinNeighbours, default 2, of its face neighbours are
//                 known); getMesh().filled then says per vertex what the fill made up.  AT AN OPEN BORDER THE SURFACE CONTINUES AS
//                 A SKIRT UP TO fillIterations VOXELS WIDE; neither parameter has been tuned.  The grid rule does not change.
//   clean mesh   cleanMesh(params) after a meshDenseCloud that returned OKAY: ONE sfmba_mesh_clean call (include/sfmba.h) over the
//                 mesh: the connected components with fewer than minComponentTriangles triangles go (or, with keepLargest, all but
//                 the largest), the rest is smoothed by smoothIterations iterations of Taubin's lambda | mu in integers, and every
//                 vertex gets a normal (every triangle of a vertex has equal weight: NOT area weighted).  THE HOST RULES:
//                 origin = the mesh grid's origin; quantum = voxel / 1024 (float), the unit the TSDF already uses;
//                 minComponentTriangles == 0 means max(1, triangles / 1000) (integer division).  These defaults, and lambda 0.5 /
//                 mu -0.53 (Taubin's usual pair) at 10 iterations, are first choices like the ones above: nobody has tuned them.
//                 The mesh of meshDenseCloud, the dense cloud and the depth maps are not changed.
//   decimate     decimateMesh(params) after a meshDenseCloud that returned OKAY: ONE sfmba_mesh_decimate call (include/sfmba.h) over the
//                 clean mesh when cleanMesh has returned OKAY since, otherwise over the mesh: every cell of cellVoxels voxels becomes
//                 one vertex (the minimiser of the cell's quadric, kept inside the cell, or the rounded mean), and the triangles that
//                 still span three cells survive, once each; then ONE sfmba_mesh_smooth call with 0 iterations gives the normals.
//                 THE HOST RULES: origin = the mesh grid's origin; quantum = voxel / 1024 (float); cell = round(cellVoxels * 1024),
//                 refused outside 32..2^20.  cellVoxels 2, the quadric placement and reg 1024 are first choices that NOBODY HAS
//                 TUNED.  NOT DONE: no edge-collapse simplification, no topology guarantee (sheets closer than a cell fuse, a few
//                 non-manifold edges appear), no area weighting, no boundary-preserving quadrics.  The mesh, the clean mesh, the dense
//                 cloud and the depth maps are not changed; a later meshDenseCloud or cleanMesh clears the decimated mesh.
//   texture       textureMesh(params) after a meshDenseCloud that returned OKAY: ONE sfmba_mesh_texture call (include/sfmba.h) over
//                 the decimated mesh when decimateMesh has returned OKAY since, otherwise over
//                 the clean mesh when cleanMesh has returned OKAY since, otherwise over the mesh, with all images, the poses and the
//                 depth maps: every triangle takes the view that sees it largest among those that see all three vertices
//                 unoccluded, and a patch of S (S + 1) / 2 texels in an atlas, filled from that view perspective-correctly; a
//                 triangle no view sees keeps its blended vertex colours.  THE HOST RULES: patch S = 6; blocksPerRow 0 means
//                 B = ceil(sqrt(ceil(triangles / 2))), at least 1 (a square atlas); occl_tol = occlTolVoxels * the grid's voxel
//                 (float), occlTolVoxels default 2; min_area = round(2 * 256 * minAreaPx), minAreaPx default 0.5.  These are first
//                 choices that NOBODY HAS TUNED.  NO COLOUR ADJUSTMENT ACROSS VIEWS unless asked for (off by default), see
//                 params.levelPasses below (seams where exposures differ stay visible), NO
//                 SMOOTHING OF THE VIEW LABELS BY DEFAULT, NO CHART MERGING (every triangle costs (S + 1) S / 2 texels, however small).
//                 The mesh, the clean mesh, the dense cloud and the depth maps are not changed.
//                 With params.smoothRings or params.smoothPasses not 0 the labels are chosen TOGETHER, by ONE
//                 sfmba_mesh_texture_smooth call in place of the plain one (include/sfmba.h, "smoothing the view labels"): the
//                 params.candidates best views per triangle, their scores summed over smoothRings rings of neighbours, then at most
//                 smoothPasses passes of a Potts relaxation with the penalty smoothPenalty; the textured mesh then carries the call's
//                 eight statistics, and an INFO line reports them.  The defaults (off; 256; 4 candidates) and sfmtoy's 4 rings, 256
//                 and 100 passes are first choices that nobody has tuned.
//                 With params.levelPasses not 0 the colours are LEVELLED ACROSS SEAMS, by ONE sfmba_mesh_texture_adjust call in place
//                 of the two above (include/sfmba.h, "levelling the colours across seams"): the labels as above, then an additive
//                 colour offset per (vertex, view) by levelPasses integer Jacobi passes with the seam weight levelSeamWeight, from
//                 colours sampled with the radius levelSampleRadius, blended into every sampled texel; the textured mesh then
//                 carries the call's eight statistics, and an INFO line reports them.  The defaults (off; 16; 1) and sfmtoy's 16
//                 passes are first choices that NOBODY HAS TUNED.
// There is no visual debugging.
// An object holds all of a run's state (the stage times of SFMBA_SFM_TIMING included): different objects may run in different
// threads; one object is not re-entrant.
#pragma once
#include <set>
#include <string>
#include <vector>

#include "SfMCommon.h"
#include "SfMAssociation.h"
#include "SfM2DFeatureUtilities.h"
#include "SfMDenseUtilities.h"

namespace sfmtoylib {

enum ErrorCode {
    OKAY = 0,
    ERROR
};

enum { LOG_TRACE = 0, LOG_DEBUG, LOG_INFO, LOG_WARN, LOG_ERROR };      // SfMCommon.h:38-44 of the reference

class SfM {
public:
    // one turn of the add-more-views loop
    struct AddedView {
        int    view;            // the view that was marked done
        bool   posed;           // findCameraPoseFrom2D3DMatch's verdict
        size_t cloudSize;       // the reconstruction cloud after the view's merges (as before them when posed is false)
    };

    SfM(const float downscale = 1.0);
    virtual ~SfM();

    /**
     * Binary .pgm (P5 -> CV_8U) / .ppm (P6 -> CV_8UC3, stored B, G, R) files of maxval 255 and baseline .jpg / .jpeg files (one
     * component -> CV_8U, three -> CV_8UC3; the scope is that of sfmba_jpeg_decode, EXIF orientation is ignored) and non-interlaced
     * .png files (gray with or without alpha -> CV_8U, colour and palette -> CV_8UC3; the scope is that of sfmba_png_decode: 16-bit
     * samples keep their high byte, alpha is dropped, no gamma) of the directory, in
     * ascending file-name order across all extensions (the extension decides which files are read, in either letter case).  The
     * downscale factor of the constructor is applied here, on the device; PNM files at factor 1 touch no device.
     * @return true on success; false (no image kept) when the directory cannot be read, holds no such file, a file is not a P5 / P6
     *         file of maxval 255 with all its bytes or not a decodable baseline JPEG / PNG, the files are not all of one kind, or the
     *         device fails.
     */
    bool setImagesDirectory(const std::string& directoryPath);

    /** The images themselves, all CV_8U or all CV_8UC3, taken as they are (no downscale).  Forgets features given by setFeatures. */
    void setImages(const std::vector<cv::Mat>& images);

    /**
     * Key points (+ points) and descriptors of every view and the image size: runSfM then skips the extraction.  The descriptors
     * are all CV_8U (Hamming) or all CV_32F (L2; see setMergeFeatureMatchDistance).
     */
    void setFeatures(const std::vector<Features>& imageFeatures, int cols, int rows);

    /**
     * The distance below which a feature match confirms a merge in SfMAssociation::mergeNewPointCloud.  Default 20, the reference's
     * constant for ORB's Hamming distances; float descriptors need a value on the scale of their own L2 distances.  With
     * MATCHER_FLOW a match's distance is its snap distance in pixels (<= 2): the default 20 confirms every flow match.
     */
    void setMergeFeatureMatchDistance(float maxDistance) { mMergeFeatureMatchDistance = maxDistance; }

    /**
     * The extractor runSfM uses on images: FEATURES_ORB (default) or FEATURES_SURF (float rows of unit length, matched by L2).  The
     * merge distance stays what setMergeFeatureMatchDistance says; its default 20 confirms every match of unit-length descriptors
     * (their distances are <= 2).
     */
    void setFeatureType(FeatureType type) { mFeatureType = type; }

    /**
     * The matcher of stage 2: MATCHER_DESCRIPTORS (default) or MATCHER_FLOW (optical flow between the images, for frame sequences;
     * see `matcher` at the top of this file).  MATCHER_FLOW needs the images: after setFeatures runSfM returns ERROR.
     */
    void setMatcherType(MatcherType type) { mMatcherType = type; }

    /** MATCHER_FLOW only: k > 0 matches view i with views i+1 .. i+k only; 0 (default) matches all pairs.  Negative: runSfM returns ERROR. */
    void setFlowPairWindow(int window) { mFlowPairWindow = window; }

    /** Run the pipeline (the contract is at the top of this file); every call starts from the images / features again. */
    ErrorCode runSfM();

    /**
     * <prefix>_points.ply and <prefix>_cameras.ply through SfMExport.  Gray images colour a point with its gray value; after
     * setFeatures every point is gray 128.
     */
    bool saveCloudAndCamerasToPLY(const std::string& prefix);

    /**
     * Dense depth maps of the good views and the fused dense cloud (the contract is at the top of this file).  Valid after a runSfM
     * that returned OKAY on images; after setFeatures there are no pixels.  With SFMBA_SFM_TIMING set, one stderr line reports
     * dense_sweep_ms and dense_fuse_ms.
     * @return ERROR (nothing kept) without such a run, for maxSources outside 1..4, or when a device call fails or refuses.
     */
    ErrorCode densify(const DenseParams& params = DenseParams());

    /**
     * <prefix>_dense.ply: the dense cloud, ASCII, with the header and the number formatting of <prefix>_points.ply, colours R G B.
     */
    bool saveDenseCloudToPLY(const std::string& prefix);

    /**
     * One oriented point per occupied voxel of the dense cloud (the contract is at the top of this file).  Valid after a densify
     * that returned OKAY.  voxel: the edge length, 0 = auto; minCount: a voxel needs this many dense points.  maxRelStep (a
     * neighbouring pixel takes part in a normal if its depth differs by at most this share) defaults to 0.05: a first choice that
     * nobody has tuned.  With SFMBA_SFM_TIMING set, one stderr line reports merge_normals_ms and merge_cloud_ms.
     * @return ERROR (nothing kept) without such a densify, for voxel < 0 or not finite, minCount < 1, or when a device call fails.
     */
    ErrorCode mergeDenseCloud(float voxel = 0.0f, int minCount = 1, float maxRelStep = 0.05f);

    /**
     * <prefix>_dense_merged.ply: the merged cloud, ASCII, in the style of the other writers: x y z, nx ny nz, red green blue.
     */
    bool saveMergedDenseCloudToPLY(const std::string& prefix);

    /**
     * A triangle mesh of the scene from the depth maps (the contract is at the top of this file).  Valid after a densify that returned
     * OKAY.  With SFMBA_SFM_TIMING set, one stderr line reports mesh_ms.
     * @return ERROR (nothing kept) without such a densify, for voxel < 0 or not finite, resolution < 2, truncVoxels not finite or
     *         <= 0, minWeight outside 1..65535, a dense cloud without a finite point, or when the device call fails or refuses.
     */
    ErrorCode meshDenseCloud(const MeshParams& params = MeshParams());

    /**
     * <prefix>_mesh.ply: the mesh, ASCII, in the style of the other writers: x y z red green blue per vertex, then element face with
     * property list uchar int vertex_indices.
     */
    bool saveMeshToPLY(const std::string& prefix);

    /**
     * The mesh without its small components, smoothed, with a normal per vertex (the contract is at the top of this file).  Valid after
     * a meshDenseCloud that returned OKAY; cleared wherever that mesh is cleared.  With SFMBA_SFM_TIMING set, one stderr line reports
     * clean_ms.
     * @return ERROR (no clean mesh kept) without such a meshDenseCloud, or when the device call fails or refuses (minComponentTriangles
     *         < 0, smoothIterations outside 0..100, lambda or mu outside their ranges).
     */
    ErrorCode cleanMesh(const MeshCleanParams& params = MeshCleanParams());

    /**
     * <prefix>_mesh_clean.ply: the clean mesh, ASCII, in the style of the other writers: x y z, nx ny nz, red green blue per vertex,
     * then element face with property list uchar int vertex_indices.
     */
    bool saveCleanMeshToPLY(const std::string& prefix);

    /**
     * Fewer, larger triangles: vertex clustering with the quadric (or the mean) placement and a normal per vertex (the contract is at the
     * top of this file).  Valid after a meshDenseCloud that returned OKAY; works on the clean mesh when cleanMesh has returned OKAY since,
     * otherwise on the mesh; cleared by a later meshDenseCloud or cleanMesh, and wherever the mesh is cleared.  With SFMBA_SFM_TIMING set,
     * one stderr line reports decimate_ms.
     * @return ERROR (no decimated mesh kept) without such a meshDenseCloud, when cellVoxels * 1024 rounds outside 32..2^20, or when a
     *         device call fails or refuses (placement outside {0, 1}, reg outside 1..2^20 with the quadric placement).
     */
    ErrorCode decimateMesh(const MeshDecimateParams& params = MeshDecimateParams());

    /**
     * <prefix>_mesh_decimated.ply: the decimated mesh, in the clean mesh's layout.
     */
    bool saveDecimatedMeshToPLY(const std::string& prefix);

    /**
     * The photographs on the mesh: a view per triangle and a texture atlas (the contract is at the top of this file).  Valid after a
     * meshDenseCloud that returned OKAY; works on the decimated mesh when decimateMesh has returned OKAY since, otherwise
     * on the clean mesh when cleanMesh has returned OKAY since, otherwise on the mesh; cleared
     * wherever those are cleared.  ONE C-ABI call.  With SFMBA_SFM_TIMING set, one stderr line reports texture_ms.
     * @return ERROR (no textured mesh kept) without such a meshDenseCloud, or when the device call fails or refuses (patch outside
     *         3..64, an atlas side above 16384, occlTolVoxels or minAreaPx negative or not finite).
     */
    ErrorCode textureMesh(const TextureParams& params = TextureParams());

    /**
     * <prefix>_textured.obj (v, then three vt per triangle: u / W and 1 - v / H, printed with %.9g, then f a/1 b/2 c/3 ...),
     * <prefix>_textured.mtl (one material whose map_Kd names the PNG) and <prefix>_textured.png (the atlas, 8-bit RGB, filter 0 on
     * every row, STORED deflate blocks: NO COMPRESSION).
     */
    bool saveTexturedMeshToOBJ(const std::string& prefix);

    void setConsoleDebugLevel(unsigned int consoleDebugLevel) { mConsoleDebugLevel = consoleDebugLevel < (unsigned int)LOG_ERROR ? consoleDebugLevel : (unsigned int)LOG_ERROR; }

    const std::vector<cv::Mat>&     getImages() const { return mImages; }
    const std::vector<Features>&    getImageFeatures() const { return mImageFeatures; }
    const std::vector<cv::Matx34f>& getCameraPoses() const { return mCameraPoses; }
    const PointCloud&               getPointCloud() const { return mReconstructionCloud; }
    const Intrinsics&               getIntrinsics() const { return mIntrinsics; }
    const std::set<int>&            getDoneViews() const { return mDoneViews; }
    const std::set<int>&            getGoodViews() const { return mGoodViews; }
    const std::vector<AddedView>&   getAddedViews() const { return mAddedViews; }
    const std::vector<cv::Mat>&     getDepthMaps() const { return mDepthMaps; }       // per view; an empty Mat where densify made no job
    const DenseCloud&               getDenseCloud() const { return mDenseCloud; }
    const std::vector<DenseJob>&    getDenseJobs() const { return mDenseJobs; }       // the jobs of the last densify, ascending view
    const MergedCloud&              getMergedDenseCloud() const { return mMergedCloud; }
    const Mesh&                     getMesh() const;                                  // of the last meshDenseCloud; empty without one
    const Mesh&                     getCleanMesh() const;                             // of the last cleanMesh; empty without one
    const Mesh&                     getDecimatedMesh() const;                         // of the last decimateMesh; empty without one
    const TexturedMesh&             getTexturedMesh() const;                          // of the last textureMesh; empty without one

private:
    enum { T_EXTRACT, T_MATCH, T_RANK, T_BASELINE_POSE, T_BASELINE_TRIANGULATE, T_ASSOCIATE, T_PNP, T_PAIR_POSES, T_TRIANGULATE, T_MERGE,
           T_ADJUST, T_COUNT };                  // the stages SFMBA_SFM_TIMING reports

    void say(unsigned int level, const std::string& line) const;      // one console line if the debug level admits it
    void startRun(size_t n_views);
    bool findBaselineTriangulation();
    void adjustCurrentBundle();
    void addMoreViewsToReconstruction();
    int  nextView(const Images2D3DMatches& candidates) const;
    bool triangulateAgainstGoodViews(int view);

    std::vector<cv::Mat>      mImages;
    std::vector<Features>     mImageFeatures;
    std::vector<cv::Matx34f>  mCameraPoses;
    std::set<int>             mDoneViews;
    std::set<int>             mGoodViews;
    MatchMatrix               mFeatureMatchMatrix;
    Intrinsics                mIntrinsics;
    PointCloud                mReconstructionCloud;
    std::vector<AddedView>    mAddedViews;
    unsigned int              mConsoleDebugLevel;
    float                     mDownscaleFactor;
    float                     mMergeFeatureMatchDistance;
    FeatureType               mFeatureType;
    MatcherType               mMatcherType;
    int                       mFlowPairWindow;
    bool                      mFeaturesGiven;
    bool                      mDownscaleApplied; // the images came from setImagesDirectory, which applied mDownscaleFactor
    int                       mCols, mRows;      // of image 0, or as given to setFeatures
    std::vector<cv::Mat>      mDepthMaps;
    DenseCloud                mDenseCloud;
    std::vector<DenseJob>     mDenseJobs;
    MergedCloud               mMergedCloud;
    Mesh                      mMesh;
    Mesh                      mCleanMesh;
    Mesh                      mDecimatedMesh;
    TexturedMesh              mTexturedMesh;
    bool                      mMeshOkay;        // the last meshDenseCloud returned OKAY and nothing was set since
    bool                      mCleanOkay;       // a cleanMesh returned OKAY since that meshDenseCloud
    bool                      mDecimateOkay;    // a decimateMesh returned OKAY since that meshDenseCloud and since the last cleanMesh
    bool                      mRunOkay;         // the last runSfM returned OKAY and nothing was set since
    bool                      mTiming;           // SFMBA_SFM_TIMING was set when the run began
    double                    mStageMs[T_COUNT]; // wall time per stage of the current run (all zero unless mTiming)
};

}  // namespace sfmtoylib
