// SfMDenseUtilities.h -- dense depth maps and a dense cloud over the C ABI's sfmba_depth_sweep / sfmba_depth_fuse (include/sfmba.h
// holds the contract): plane-sweep stereo for a list of jobs in ONE device call, and the consistency filter that turns the depth maps
// of a set of views into coloured points in ONE device call.  The reference stops at the sparse cloud; this is the stage between
// "camera poses" and "a model" (SfM::densify drives it).  Both functions are thin: they flatten, call and rebuild.  So are the two
// that follow them, over sfmba_depth_normals / sfmba_cloud_merge: a normal per depth pixel, and one oriented point per occupied voxel
// of the fused cloud (SfM::mergeDenseCloud drives them).  The last three, over sfmba_tsdf_integrate / sfmba_tsdf_extract /
// sfmba_tsdf_mesh, turn the depth maps into a surface: a truncated signed distance grid and its triangle mesh (SfM::meshDenseCloud);
// sfmba_tsdf_fill / sfmba_tsdf_mesh_fill fill the grid's holes in between (MeshParams::fillIterations, off by default).
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
    // Semi-global matching over the sweep's cost volume (include/sfmba.h, sfmba_depth_sweep_sgm), OFF by default: with `sgm` unset
    // computeDepthMaps makes the sfmba_depth_sweep call it always made and none of the fields below is read.  With it set every pixel
    // of a reference view gets a plane -- one without texture takes what its neighbours agree on -- minScore is not read, and the
    // score map holds 0 where the depth came from the neighbours alone.
    bool  sgm;
    int   sgmP1, sgmP2;     // the penalty for a change of one plane and for any other change, 0 <= sgmP1 <= sgmP2 <= 1023
    int   sgmPaths;         // path directions, 4 or 8
    int   sgmInvalidCost;   // what a plane without a cost reads as, 0..254
    int   sgmUniqueness;    // accepted iff 100 (second - best) >= sgmUniqueness * second, 0..100
    DenseParams() : planes(64), radius(3), minStd(2), minScore(0.6f), minSources(1), relTol(0.01f), minConsistent(1), maxSources(2), sgm(false),
                    sgmP1(8), sgmP2(64), sgmPaths(8), sgmInvalidCost(127), sgmUniqueness(5) {}
};

// The fused points in (view, row, column) order.  A surface point seen by three views appears three times: nothing is de-duplicated
// (mergeCloud below, over sfmba_cloud_merge, makes one point per occupied voxel of such a cloud).
struct DenseCloud {
    Points3f                   points;
    std::vector<unsigned char> bgr;      // 3 per point: the pixel's own colour (a gray image gives g, g, g)
    std::vector<int>           views;    // the view a point comes from
    std::vector<int>           pixels;   // ... and its pixel there, row * cols + column
};

// One point per occupied voxel, in ascending voxel key order (include/sfmba.h, sfmba_cloud_merge).
struct MergedCloud {
    Points3f                   points;   // the mean of the voxel's members, on a grid of 1/1024 voxel
    std::vector<unsigned char> bgr;      // 3 per point: the rounded mean colour; empty if the input had none
    Points3f                   normals;  // unit length, or (0, 0, 0) where the members' normals cancel or none had one; empty if none given
    std::vector<int>           counts;   // members per point
    std::vector<int>           first;    // the lowest input index among the members
    float                      voxel;    // the edge length merged with
    long long                  skipped;  // input points outside the grid or not finite
    MergedCloud() : voxel(0.0f), skipped(0) {}
};

// The grid of a truncated signed distance field (include/sfmba.h, "the grid"): vertex (i, j, k) lies at origin + (i, j, k) voxel.
struct MeshGrid {
    cv::Point3f origin;
    float       voxel;       // > 0
    int         nx, ny, nz;  // each 1..1024, nx ny nz <= 2^26
    float       trunc;       // the distance is clamped to [-trunc, trunc]; a view behind -trunc does not count
    MeshGrid() : origin(0.0f, 0.0f, 0.0f), voxel(0.0f), nx(0), ny(0), nz(0), trunc(0.0f) {}
};

// What sfmba_tsdf_integrate leaves per grid vertex, in (z, y, x) order: integers only.
struct TsdfVolume {
    MeshGrid         grid;
    std::vector<int> sum, weight;        // the summed distance quanta (1024 per trunc) and the number of views that count
    std::vector<int> csum, cweight;      // 3 colour sums per vertex and their number of views; both empty without colour
};

// A triangle mesh: the vertices in ascending key order, the triangles in (cell, tetrahedron) order (include/sfmba.h, sfmba_tsdf_extract).
// Normals face the outside, towards the cameras.
struct Mesh {
    Points3f                   vertices;
    std::vector<unsigned char> bgr;        // 3 per vertex; empty if the grid had no colour
    std::vector<int>           triangles;  // 3 vertex indices per triangle
    MeshGrid                   grid;       // the grid it was taken from
    std::vector<float>         normals;    // 3 per vertex, unit length or (0, 0, 0); empty on a raw mesh (cleanMesh fills them)
    std::vector<unsigned char> filled;     // 1 per vertex that lies on an edge with an end the hole filling made; EMPTY when nothing was filled
};

// SfM::meshDenseCloud: how the grid is laid over the dense cloud (the rule is at the top of SfM.h).  First choices; nobody has tuned them.
struct MeshParams {
    float voxel;            // the grid's edge length, 0 = from resolution
    int   resolution;       // grid vertices along the longest side of the cloud's box, >= 2
    float truncVoxels;      // trunc in voxels, > 0
    int   minWeight;        // views a grid vertex needs to count, 1..65535
    int   fillIterations;   // hole filling (include/sfmba.h, sfmba_tsdf_fill): passes, 0..254; 0 = OFF, THE DEFAULT.  AT AN OPEN BORDER THE FILL
                            // CONTINUES THE SURFACE AS A SKIRT UP TO THIS MANY VOXELS WIDE
    int   fillMinNeighbours;  // known face neighbours an unknown grid vertex needs to be filled, 1..6; NOT TUNED
    MeshParams() : voxel(0.0f), resolution(256), truncVoxels(4.0f), minWeight(1), fillIterations(0), fillMinNeighbours(2) {}
};

// SfMDenseUtilities::cleanMesh / SfM::cleanMesh: which components go and how the rest is smoothed (include/sfmba.h, sfmba_mesh_clean; the
// host rules are at the top of SfM.h).  lambda 0.5 / mu -0.53 is Taubin's usual pair; with 10 iterations and the island rule below they
// are first choices; nobody has tuned them.
struct MeshCleanParams {
    int   minComponentTriangles;  // a component with fewer triangles goes; 0 = max(1, triangles / 1000)
    bool  keepLargest;            // keep only the component with the most triangles
    int   smoothIterations;       // 0..100, each a lambda pass and a mu pass
    float lambda, mu;
    MeshCleanParams() : minComponentTriangles(0), keepLargest(false), smoothIterations(10), lambda(0.5f), mu(-0.53f) {}
};

// SfMDenseUtilities::decimateMesh / SfM::decimateMesh: the size of a cell and where its representative goes (include/sfmba.h,
// sfmba_mesh_decimate; the host rules are at the top of SfM.h).  Two voxels a cell, the quadric placement and reg 1024 are first choices;
// NOBODY HAS TUNED THEM.
struct MeshDecimateParams {
    enum { MEAN = 0, QUADRIC = 1 };
    float cellVoxels;       // the edge of a cell in voxels of the mesh's grid; cell = round(cellVoxels * 1024) quanta must lie in 32..2^20
    int   placement;        // MEAN: the rounded mean of a cell's vertices; QUADRIC: the minimiser of the cell's quadric, kept inside the cell
    int   reg;              // 1..2^20, read with QUADRIC only: pulls towards the mean with weight reg / 2^20 relative to a unit normal
    MeshDecimateParams() : cellVoxels(2.0f), placement(QUADRIC), reg(1024) {}
};

// SfMDenseUtilities::textureMesh / SfM::textureMesh: the size of a triangle's patch and which views count (include/sfmba.h,
// sfmba_mesh_texture; the host rules are at the top of SfM.h).  First choices; NOBODY HAS TUNED THEM.
// SMOOTHING THE VIEW LABELS IS OFF BY DEFAULT: with smoothRings = 0 and smoothPasses = 0 the call is the plain sfmba_mesh_texture call and
// the other three smoothing fields are not read.  Otherwise ONE sfmba_mesh_texture_smooth call chooses the labels together (the K =
// candidates best views per triangle, their scores summed over smoothRings rings of neighbours, then at most smoothPasses passes of a
// Potts relaxation with the penalty smoothPenalty, in 1/1024 of the best view's area).  sfmtoy's --texture-smooth switches 4, 256 and
// 100 passes on; those too are first choices that nobody has tuned.
// LEVELLING THE COLOURS ACROSS SEAMS IS OFF BY DEFAULT: with levelPasses = 0 the call is the one above and the other two levelling fields
// are not read.  Otherwise ONE sfmba_mesh_texture_adjust call chooses the labels as above (the plain rule with smoothRings = 0 and
// smoothPasses = 0), gives every (vertex, view) pair an additive colour offset by levelPasses integer Jacobi passes and blends the
// offsets into the sampled texels (include/sfmba.h, "levelling the colours across seams").  The defaults 16 and 1, and the 16 passes
// that sfmtoy's --texture-level switches on, are first choices that NOBODY HAS TUNED.
struct TextureParams {
    int   patch;            // S: a triangle gets S (S + 1) / 2 texels, 3..64
    int   blocksPerRow;     // B: blocks (pairs of triangles) per atlas row; 0 = ceil(sqrt(blocks)), at least 1
    float occlTolVoxels;    // a vertex may lie this many voxels of the mesh's grid behind a view's depth map
    float minAreaPx;        // a view counts for a triangle from this image area, in square pixels
    int   smoothRings;      // r, 0..8: rings of neighbours whose scores a triangle hears before it chooses
    int   smoothPenalty;    // p, 0..65535: what a pair of neighbours with different views costs
    int   smoothPasses;     // 0..10000: the most relaxation passes
    int   candidates;       // K, 1..8: views a triangle may choose among
    int   levelPasses;      // N, 0..1024: Jacobi passes of the seam levelling; 0 = off
    int   levelSeamWeight;  // w, 1..256: what closing the gap at a seam counts against smoothness within a view
    int   levelSampleRadius;  // r, 0..2: a node's colour is the mean over (2 r + 1)^2 samples about its vertex
    TextureParams() : patch(6), blocksPerRow(0), occlTolVoxels(2.0f), minAreaPx(0.5f), smoothRings(0), smoothPenalty(256), smoothPasses(0), candidates(4),
                      levelPasses(0), levelSeamWeight(16), levelSampleRadius(1) {}
};

// A mesh that carries the photographs: triangle t has the corners uv[6 t .. 6 t + 5] (u, v per corner, in atlas pixels, origin top-left)
// in the atlas and took its texels from view[t] (-1: none saw it; its patch holds the blended vertex colours).  NO COLOUR ADJUSTMENT
// ACROSS VIEWS unless asked for (off by default), see TextureParams::levelPasses, NO SMOOTHING OF THE VIEW LABELS unless TextureParams asks
// for it (off by default), NO CHART MERGING (include/sfmba.h).
// smoothed: the labels came from sfmba_mesh_texture_smooth, and smoothStats holds its eight statistics (include/sfmba.h: the energy after
// the start and at the end; the pairs of neighbours with different views under the plain rule, after the start and at the end; the pairs
// with one side without a view; the moves; the passes that moved something); all zero otherwise.
// levelled: the atlas came from sfmba_mesh_texture_adjust, and levelStats holds its eight statistics (nodes; blind nodes; seam vertices; the
// summed spread of the colours at the seam vertices before and after, in 1/256 grey level; the largest offset; the texels that clamped; the
// passes); all zero otherwise.
struct TexturedMesh {
    Points3f           vertices;
    std::vector<int>   triangles;  // 3 vertex indices per triangle
    std::vector<float> uv;         // 6 per triangle
    std::vector<int>   view;       // 1 per triangle
    cv::Mat            atlas;      // CV_8UC3, BGR
    long long          textured;   // triangles with a view
    bool               smoothed;
    long long          smoothStats[8];
    bool               levelled;
    long long          levelStats[8];
    TexturedMesh() : textured(0), smoothed(false), smoothStats{ 0, 0, 0, 0, 0, 0, 0, 0 }, levelled(false), levelStats{ 0, 0, 0, 0, 0, 0, 0, 0 } {}
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

    /**
     * One normal map (CV_32FC3, world coordinates, (0, 0, 0) where a pixel has none) per view with a depth map, an empty Mat for the
     * others: ONE sfmba_depth_normals call.  images give the sizes only (their pixels are not read); depthMaps as fuseDepthMaps takes
     * them.  maxRelStep: a neighbour takes part in a pixel's differences if its depth differs by at most this share.
     * @return false (normals empty) when the device call fails or refuses an argument; the reason goes to stderr.
     */
    static bool computeNormals(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses,
                               const std::vector<cv::Mat>& depthMaps, float maxRelStep, std::vector<cv::Mat>& normals);

    /**
     * One point per voxel of edge `voxel` that holds at least minCount points of the cloud: ONE sfmba_cloud_merge call (two when the
     * first reports the size).  normals: one per point of the cloud, or empty.
     * @param ok  if not null, receives false when the device call fails or refuses an argument (the result is then empty).
     */
    static MergedCloud mergeCloud(const DenseCloud& cloud, const Points3f& normals, float voxel, int minCount, bool* ok = nullptr);

    /**
     * The depth maps averaged along the viewing rays into the grid: ONE sfmba_tsdf_integrate call.  images, poses and depthMaps as
     * fuseDepthMaps takes them; colour: sum the pixels' colours too.
     * @return false (volume empty) when the device call fails or refuses an argument; the reason goes to stderr.
     */
    static bool integrateTSDF(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses,
                              const std::vector<cv::Mat>& depthMaps, const MeshGrid& grid, bool colour, TsdfVolume& volume);

    /**
     * The zero set of the volume over the cells whose eight corners were seen by at least minWeight views, by marching tetrahedra:
     * ONE sfmba_tsdf_extract call (two when the first reports the sizes).
     * @param ok  if not null, receives false when the device call fails or refuses an argument (the mesh is then empty).
     */
    static Mesh extractMesh(const TsdfVolume& volume, int minWeight, bool* ok = nullptr);

    /**
     * integrateTSDF with colour, then extractMesh, the grid never leaving the device: ONE sfmba_tsdf_mesh call (two when the first
     * reports the sizes).  The result equals the two calls' byte for byte.
     */
    static Mesh meshDepthMaps(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses,
                              const std::vector<cv::Mat>& depthMaps, const MeshGrid& grid, int minWeight, bool* ok = nullptr);

    /**
     * meshDepthMaps with the holes of the grid filled between the integration and the extraction: ONE sfmba_tsdf_mesh_fill call (two
     * when the first reports the sizes); mesh.filled says per vertex what the fill made up.  With fillIterations == 0 it is the call
     * above and mesh.filled stays empty.
     */
    static Mesh meshDepthMaps(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses,
                              const std::vector<cv::Mat>& depthMaps, const MeshGrid& grid, int minWeight, int fillIterations, int fillMinNeighbours,
                              bool* ok = nullptr);

    /**
     * The volume with the signed distance diffused into its undefined vertices (volumetric diffusion; the rule is in include/sfmba.h):
     * ONE sfmba_tsdf_fill call.  state (may be null): per vertex 0 observed, p the pass in which it became known, 255 still unknown.
     * A filled vertex lies within `iterations` voxels (L1) of an observed one: THE SKIRT AT AN OPEN BORDER IS THAT WIDE.
     * @return false (out empty) when the device call fails or refuses an argument; the reason goes to stderr.
     */
    static bool fillTSDF(const TsdfVolume& volume, int minWeight, int iterations, int minNeighbours, TsdfVolume& out,
                         std::vector<unsigned char>* state = nullptr);

    /**
     * Per vertex the lowest vertex index of its connected component (a vertex no triangle names is its own): ONE sfmba_mesh_components
     * call.
     * @param ok  if not null, receives false when the device call fails or refuses an argument (the result is then empty).
     */
    static std::vector<int> meshComponents(const Mesh& mesh, bool* ok = nullptr);

    /**
     * The mesh without its small components (or with its largest only), smoothed by Taubin's lambda | mu passes in integers of
     * mesh.grid.voxel / 1024 about mesh.grid.origin, with a normal per vertex (every triangle of a vertex has equal weight: NOT area
     * weighted): ONE sfmba_mesh_clean call (two when the first reports the sizes).  The grid is carried over.
     * @param ok  if not null, receives false when the device call fails or refuses an argument (the mesh is then empty).
     */
    static Mesh cleanMesh(const Mesh& mesh, const MeshCleanParams& params, bool* ok = nullptr);

    /**
     * The mesh with every cell of params.cellVoxels voxels collapsed to one vertex (vertex clustering; the mean or the quadric
     * placement) and the triangles that still span three cells, without duplicates: ONE sfmba_mesh_decimate call (two when the first
     * reports the sizes) in integers of mesh.grid.voxel / 1024 about mesh.grid.origin, then ONE sfmba_mesh_smooth call with 0 iterations
     * on the result for its normals (NOT area weighted).  The grid is carried over; `filled` is not.  NO TOPOLOGY GUARANTEE: sheets closer
     * than a cell fuse and a few non-manifold edges appear.
     * @param ok     if not null, receives false when cell = round(cellVoxels * 1024) lies outside 32..2^20 or a device call fails or
     *               refuses an argument (the mesh is then empty).
     * @param stats  if not null, receives the call's four statistics: clusters, collapsed triangles, duplicates dropped, clusters that
     *               the quadric placement left to the mean.
     */
    static Mesh decimateMesh(const Mesh& mesh, const MeshDecimateParams& params, bool* ok = nullptr, long long* stats = nullptr);

    /**
     * A view per triangle and a texture atlas with one patch per triangle: ONE sfmba_mesh_texture call, or, when params.smoothRings or
     * params.smoothPasses is not 0, ONE sfmba_mesh_texture_smooth call, or, when params.levelPasses is not 0, ONE sfmba_mesh_texture_adjust call.  images, poses and depthMaps as
     * fuseDepthMaps takes them (a view without a map has no visibility test).  THE HOST RULES: B = params.blocksPerRow, or
     * ceil(sqrt(ceil(triangles / 2))) (at least 1) when that is 0; occl_tol = params.occlTolVoxels * mesh.grid.voxel (float);
     * min_area = round(2 * 256 * params.minAreaPx).
     * @param ok  if not null, receives false when the device call fails or refuses an argument (the result is then empty).
     */
    static TexturedMesh textureMesh(const Mesh& mesh, const std::vector<cv::Mat>& images, const Intrinsics& intrinsics,
                                    const std::vector<cv::Matx34f>& poses, const std::vector<cv::Mat>& depthMaps, const TextureParams& params,
                                    bool* ok = nullptr);
};

}  // namespace sfmtoylib
