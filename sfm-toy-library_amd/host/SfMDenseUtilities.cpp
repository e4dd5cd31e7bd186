// SfMDenseUtilities.cpp -- host side of the dense stage: flattens the containers, calls the C ABI (include/sfmba.h), rebuilds the
// results.  See SfMDenseUtilities.h.
#include "SfMDenseUtilities.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sfmba.h"

namespace sfmtoylib {

namespace {

struct FlatScene {
    std::vector<int64_t>       ptr;
    std::vector<unsigned char> px;
    std::vector<int32_t>       w, h;
    std::vector<float>         P;
    float                      K[9];
    int                        channels;
};

bool flattenScene(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses, FlatScene& f) {
    if (images.empty() || poses.size() != images.size()) return false;
    f.channels = images[0].type() == CV_8UC3 ? 3 : 1;
    f.ptr.assign(1, 0);
    for (const cv::Mat& m : images) {
        if (m.type() != images[0].type() || (m.type() != CV_8U && m.type() != CV_8UC3)) return false;
        f.ptr.push_back(f.ptr.back() + (int64_t)m.rows * m.cols * f.channels);
        f.w.push_back(m.cols);
        f.h.push_back(m.rows);
    }
    f.px.resize((size_t)f.ptr.back());
    for (size_t i = 0; i < images.size(); ++i)
        for (int r = 0; r < images[i].rows; ++r)
            std::memcpy(f.px.data() + f.ptr[i] + (size_t)r * images[i].cols * f.channels, images[i].ptr<unsigned char>(r),
                        (size_t)images[i].cols * f.channels);
    for (const cv::Matx34f& p : poses)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) f.P.push_back(p(r, c));
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) f.K[3 * r + c] = intrinsics.K.at<float>(r, c);
    return true;
}

}  // namespace

bool SfMDenseUtilities::computeDepthMaps(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses,
                                         const std::vector<DenseJob>& jobs, const DenseParams& params, std::vector<cv::Mat>& depthMaps,
                                         std::vector<cv::Mat>& scores) {
    depthMaps.clear();
    scores.clear();
    FlatScene f;
    if (!flattenScene(images, intrinsics, poses, f)) {
        std::fprintf(stderr, "computeDepthMaps: one pose per image and images of one kind (CV_8U or CV_8UC3) are needed\n");
        return false;
    }
    std::vector<int32_t> ref, src;
    std::vector<int64_t> srcPtr(1, 0);
    std::vector<float> zNear, zFar;
    int64_t pixels = 0;
    for (const DenseJob& j : jobs) {
        if (j.reference < 0 || j.reference >= (int)images.size()) {
            std::fprintf(stderr, "computeDepthMaps: a job's reference view is out of range\n");
            return false;
        }
        ref.push_back(j.reference);
        for (int s : j.sources) src.push_back(s);
        srcPtr.push_back((int64_t)src.size());
        zNear.push_back(j.zNear);
        zFar.push_back(j.zFar);
        pixels += (int64_t)images[(size_t)j.reference].rows * images[(size_t)j.reference].cols;
    }
    if (jobs.empty()) return true;
    src.push_back(0);                                      // never read: keeps data() non-null
    std::vector<float> depth((size_t)pixels), score((size_t)pixels);
    const int rc = params.sgm
        ? sfmba_depth_sweep_sgm(0, (int)images.size(), f.ptr.data(), f.px.data(), f.w.data(), f.h.data(), f.channels, f.K, f.P.data(),
                                (int)jobs.size(), ref.data(), srcPtr.data(), src.data(), zNear.data(), zFar.data(), params.planes, params.radius,
                                params.minStd, params.minSources, params.sgmP1, params.sgmP2, params.sgmPaths, params.sgmInvalidCost,
                                params.sgmUniqueness, depth.data(), score.data(), nullptr)
        : sfmba_depth_sweep(0, (int)images.size(), f.ptr.data(), f.px.data(), f.w.data(), f.h.data(), f.channels, f.K, f.P.data(),
                            (int)jobs.size(), ref.data(), srcPtr.data(), src.data(), zNear.data(), zFar.data(), params.planes, params.radius,
                            params.minStd, params.minScore, params.minSources, depth.data(), score.data(), nullptr);
    if (rc != SFMBA_OK) {
        std::fprintf(stderr, "computeDepthMaps failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return false;
    }
    size_t at = 0;
    for (const DenseJob& j : jobs) {
        const cv::Mat& image = images[(size_t)j.reference];
        const size_t n = (size_t)image.rows * image.cols;
        cv::Mat d(image.rows, image.cols, CV_32F), s(image.rows, image.cols, CV_32F);
        std::memcpy(d.ptr<float>(0), depth.data() + at, n * sizeof(float));
        std::memcpy(s.ptr<float>(0), score.data() + at, n * sizeof(float));
        depthMaps.push_back(d);
        scores.push_back(s);
        at += n;
    }
    return true;
}

DenseCloud SfMDenseUtilities::fuseDepthMaps(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses,
                                            const std::vector<cv::Mat>& depthMaps, const std::vector<std::vector<int> >& checks,
                                            const DenseParams& params, bool* ok) {
    DenseCloud cloud;
    if (ok) *ok = false;
    FlatScene f;
    if (!flattenScene(images, intrinsics, poses, f) || depthMaps.size() != images.size() || checks.size() != images.size()) {
        std::fprintf(stderr, "fuseDepthMaps: one pose, one depth map (or an empty Mat) and one check list per image are needed\n");
        return cloud;
    }
    std::vector<const float*> maps(images.size(), nullptr);
    std::vector<int64_t> chkPtr(1, 0);
    std::vector<int32_t> chk;
    for (size_t i = 0; i < images.size(); ++i) {
        const cv::Mat& m = depthMaps[i];
        if (!m.empty()) {
            if (m.type() != CV_32F || m.rows != images[i].rows || m.cols != images[i].cols) {
                std::fprintf(stderr, "fuseDepthMaps: a depth map is not CV_32F of its image's size\n");
                return cloud;
            }
            maps[i] = m.ptr<float>(0);
        }
        for (int s : checks[i]) chk.push_back(s);
        chkPtr.push_back((int64_t)chk.size());
    }
    chk.push_back(0);                                      // never read: keeps data() non-null
    std::vector<int64_t> ptPtr(images.size() + 1, 0);
    std::vector<float> xyz;
    std::vector<int32_t> view, pixel;
    int64_t total = 0, cap = 0;                            // the first call reports the size
    for (int attempt = 0; attempt < 2; ++attempt) {
        xyz.resize((size_t)cap * 3 + 1); cloud.bgr.resize((size_t)cap * 3 + 1); view.resize((size_t)cap + 1); pixel.resize((size_t)cap + 1);
        const int rc = sfmba_depth_fuse(0, (int)images.size(), f.ptr.data(), f.px.data(), f.w.data(), f.h.data(), f.channels, f.K, f.P.data(),
                                        maps.data(), chkPtr.data(), chk.data(), params.relTol, params.minConsistent, ptPtr.data(), xyz.data(),
                                        cloud.bgr.data(), view.data(), pixel.data(), cap, &total);
        if (rc == SFMBA_OK) break;
        if (rc == SFMBA_ERR_CAPACITY && attempt == 0) { cap = total; continue; }
        std::fprintf(stderr, "fuseDepthMaps failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        cloud.bgr.clear();
        return cloud;
    }
    cloud.bgr.resize((size_t)total * 3);
    cloud.points.reserve((size_t)total);
    for (int64_t i = 0; i < total; ++i) cloud.points.push_back(cv::Point3f(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
    cloud.views.assign(view.begin(), view.begin() + total);
    cloud.pixels.assign(pixel.begin(), pixel.begin() + total);
    if (ok) *ok = true;
    return cloud;
}

bool SfMDenseUtilities::computeNormals(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses,
                                       const std::vector<cv::Mat>& depthMaps, float maxRelStep, std::vector<cv::Mat>& normals) {
    normals.clear();
    if (images.empty() || poses.size() != images.size() || depthMaps.size() != images.size()) {
        std::fprintf(stderr, "computeNormals: one pose and one depth map (or an empty Mat) per image are needed\n");
        return false;
    }
    std::vector<int32_t> w, h;
    std::vector<float> P;
    float K[9];
    for (size_t i = 0; i < images.size(); ++i) {
        w.push_back(images[i].cols);
        h.push_back(images[i].rows);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) P.push_back(poses[i](r, c));
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) K[3 * r + c] = intrinsics.K.at<float>(r, c);
    std::vector<cv::Mat> out(images.size());
    std::vector<const float*> maps(images.size(), nullptr);
    std::vector<float*> outs(images.size(), nullptr);
    for (size_t i = 0; i < images.size(); ++i) {
        const cv::Mat& m = depthMaps[i];
        if (m.empty()) continue;
        if (m.type() != CV_32F || m.rows != images[i].rows || m.cols != images[i].cols) {
            std::fprintf(stderr, "computeNormals: a depth map is not CV_32F of its image's size\n");
            return false;
        }
        out[i] = cv::Mat(m.rows, m.cols, CV_32FC3);
        maps[i] = m.ptr<float>(0);
        outs[i] = out[i].ptr<float>(0);
    }
    const int rc = sfmba_depth_normals(0, (int)images.size(), w.data(), h.data(), K, P.data(), maps.data(), maxRelStep, outs.data());
    if (rc != SFMBA_OK) {
        std::fprintf(stderr, "computeNormals failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return false;
    }
    normals.swap(out);
    return true;
}

MergedCloud SfMDenseUtilities::mergeCloud(const DenseCloud& cloud, const Points3f& normals, float voxel, int minCount, bool* ok) {
    MergedCloud merged;
    if (ok) *ok = false;
    const size_t n = cloud.points.size();
    const bool haveBgr = !cloud.bgr.empty() || n == 0, haveNormals = !normals.empty();
    if ((haveBgr && cloud.bgr.size() != 3 * n) || (haveNormals && normals.size() != n)) {
        std::fprintf(stderr, "mergeCloud: three colour bytes per point (or none at all) and one normal per point (or none at all) are needed\n");
        return merged;
    }
    std::vector<float> xyz(3 * n + 1), nrm(haveNormals ? 3 * n + 1 : 0);
    for (size_t i = 0; i < n; ++i) {
        xyz[3 * i] = cloud.points[i].x; xyz[3 * i + 1] = cloud.points[i].y; xyz[3 * i + 2] = cloud.points[i].z;
        if (haveNormals) { nrm[3 * i] = normals[i].x; nrm[3 * i + 1] = normals[i].y; nrm[3 * i + 2] = normals[i].z; }
    }
    std::vector<unsigned char> bgrIn(cloud.bgr);
    bgrIn.push_back(0);                                    // never read: keeps data() non-null
    std::vector<float> oxyz, onrm;
    std::vector<unsigned char> obgr;
    std::vector<int32_t> count, first;
    int64_t total = 0, skipped = 0, cap = 0;               // the first call reports the size
    for (int attempt = 0; attempt < 2; ++attempt) {
        oxyz.resize((size_t)cap * 3 + 1); onrm.resize((size_t)cap * 3 + 1); obgr.resize((size_t)cap * 3 + 1);
        count.resize((size_t)cap + 1); first.resize((size_t)cap + 1);
        const int rc = sfmba_cloud_merge(0, (int64_t)n, xyz.data(), haveBgr ? bgrIn.data() : nullptr, haveNormals ? nrm.data() : nullptr, voxel,
                                         minCount, oxyz.data(), obgr.data(), onrm.data(), count.data(), first.data(), nullptr, cap, &total,
                                         &skipped);
        if (rc == SFMBA_OK) break;
        if (rc == SFMBA_ERR_CAPACITY && attempt == 0) { cap = total; continue; }
        std::fprintf(stderr, "mergeCloud failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return merged;
    }
    merged.voxel = voxel;
    merged.skipped = (long long)skipped;
    merged.points.reserve((size_t)total);
    for (int64_t i = 0; i < total; ++i) merged.points.push_back(cv::Point3f(oxyz[3 * i], oxyz[3 * i + 1], oxyz[3 * i + 2]));
    if (haveBgr) merged.bgr.assign(obgr.begin(), obgr.begin() + 3 * total);
    if (haveNormals)
        for (int64_t i = 0; i < total; ++i) merged.normals.push_back(cv::Point3f(onrm[3 * i], onrm[3 * i + 1], onrm[3 * i + 2]));
    merged.counts.assign(count.begin(), count.begin() + total);
    merged.first.assign(first.begin(), first.begin() + total);
    if (ok) *ok = true;
    return merged;
}

namespace {

// the depth map pointers of a scene, one per image (NULL for an empty Mat); false if a map does not fit its image
bool mapPointers(const char* who, const std::vector<cv::Mat>& images, const std::vector<cv::Mat>& depthMaps, std::vector<const float*>& maps) {
    maps.assign(images.size(), nullptr);
    for (size_t i = 0; i < images.size(); ++i) {
        const cv::Mat& m = depthMaps[i];
        if (m.empty()) continue;
        if (m.type() != CV_32F || m.rows != images[i].rows || m.cols != images[i].cols) {
            std::fprintf(stderr, "%s: a depth map is not CV_32F of its image's size\n", who);
            return false;
        }
        maps[i] = m.ptr<float>(0);
    }
    return true;
}

// runs call(xyz, bgr, vcap, tri, tcap, &nv, &nt), a second time with the sizes the first reports, and rebuilds the mesh
template <typename Call>
bool runMeshCall(const char* who, bool colour, const MeshGrid& grid, Call call, Mesh& mesh) {
    std::vector<float> xyz;
    std::vector<unsigned char> bgr;
    std::vector<int32_t> tri;
    int64_t nv = 0, nt = 0, vcap = 0, tcap = 0;            // the first call reports the sizes
    for (int attempt = 0; attempt < 2; ++attempt) {
        xyz.resize((size_t)vcap * 3 + 1); bgr.resize((size_t)vcap * 3 + 1); tri.resize((size_t)tcap * 3 + 1);
        const int rc = call(xyz.data(), bgr.data(), vcap, tri.data(), tcap, &nv, &nt);
        if (rc == SFMBA_OK) break;
        if (rc == SFMBA_ERR_CAPACITY && attempt == 0) { vcap = nv; tcap = nt; continue; }
        std::fprintf(stderr, "%s failed (sfmba rc=%d: %s)\n", who, rc, sfmba_last_error());
        return false;
    }
    mesh.grid = grid;
    mesh.vertices.reserve((size_t)nv);
    for (int64_t i = 0; i < nv; ++i) mesh.vertices.push_back(cv::Point3f(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
    if (colour) mesh.bgr.assign(bgr.begin(), bgr.begin() + 3 * nv);
    mesh.triangles.assign(tri.begin(), tri.begin() + 3 * nt);
    return true;
}

}  // namespace

bool SfMDenseUtilities::integrateTSDF(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses,
                                      const std::vector<cv::Mat>& depthMaps, const MeshGrid& grid, bool colour, TsdfVolume& volume) {
    volume = TsdfVolume();
    FlatScene f;
    std::vector<const float*> maps;
    if (!flattenScene(images, intrinsics, poses, f) || depthMaps.size() != images.size()) {
        std::fprintf(stderr, "integrateTSDF: one pose and one depth map (or an empty Mat) per image are needed\n");
        return false;
    }
    if (!mapPointers("integrateTSDF", images, depthMaps, maps)) return false;
    const int64_t cells = (int64_t)grid.nx * grid.ny * grid.nz;
    const bool sized = grid.nx >= 1 && grid.nx <= 1024 && grid.ny >= 1 && grid.ny <= 1024 && grid.nz >= 1 && grid.nz <= 1024 && cells <= ((int64_t)1 << 26);
    TsdfVolume v;
    v.grid = grid;
    if (sized) {
        v.sum.resize((size_t)cells); v.weight.resize((size_t)cells);
        if (colour) { v.csum.resize((size_t)cells * 3); v.cweight.resize((size_t)cells); }
    }
    const float origin[3] = { grid.origin.x, grid.origin.y, grid.origin.z };
    // (an unsized grid is refused by the call before it touches the outputs)
    const int rc = sfmba_tsdf_integrate(0, (int)images.size(), f.ptr.data(), f.px.data(), f.w.data(), f.h.data(), f.channels, f.K, f.P.data(), maps.data(),
                                        origin, grid.voxel, grid.nx, grid.ny, grid.nz, grid.trunc, sized ? v.sum.data() : nullptr,
                                        sized ? v.weight.data() : nullptr, colour && sized ? v.csum.data() : nullptr,
                                        colour && sized ? v.cweight.data() : nullptr);
    if (rc != SFMBA_OK) {
        std::fprintf(stderr, "integrateTSDF failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return false;
    }
    volume = v;
    return true;
}

Mesh SfMDenseUtilities::extractMesh(const TsdfVolume& volume, int minWeight, bool* ok) {
    Mesh mesh;
    if (ok) *ok = false;
    const MeshGrid& g = volume.grid;
    const int64_t cells = (int64_t)g.nx * g.ny * g.nz;
    const bool colour = !volume.csum.empty();
    if (g.nx < 1 || g.ny < 1 || g.nz < 1 || cells > ((int64_t)1 << 26) || (int64_t)volume.sum.size() != cells || (int64_t)volume.weight.size() != cells ||
        (colour && ((int64_t)volume.csum.size() != 3 * cells || (int64_t)volume.cweight.size() != cells))) {
        std::fprintf(stderr, "extractMesh: the volume's arrays do not fit its grid\n");
        return mesh;
    }
    const float origin[3] = { g.origin.x, g.origin.y, g.origin.z };
    const bool done = runMeshCall("extractMesh", colour, g, [&](float* xyz, unsigned char* bgr, int64_t vcap, int32_t* tri, int64_t tcap, int64_t* nv, int64_t* nt) {
        return sfmba_tsdf_extract(0, origin, g.voxel, g.nx, g.ny, g.nz, volume.sum.data(), volume.weight.data(), colour ? volume.csum.data() : nullptr,
                                  colour ? volume.cweight.data() : nullptr, minWeight, xyz, bgr, nullptr, vcap, tri, tcap, nv, nt);
    }, mesh);
    if (!done) return Mesh();
    if (ok) *ok = true;
    return mesh;
}

Mesh SfMDenseUtilities::meshDepthMaps(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses,
                                      const std::vector<cv::Mat>& depthMaps, const MeshGrid& grid, int minWeight, bool* ok) {
    Mesh mesh;
    if (ok) *ok = false;
    FlatScene f;
    std::vector<const float*> maps;
    if (!flattenScene(images, intrinsics, poses, f) || depthMaps.size() != images.size()) {
        std::fprintf(stderr, "meshDepthMaps: one pose and one depth map (or an empty Mat) per image are needed\n");
        return mesh;
    }
    if (!mapPointers("meshDepthMaps", images, depthMaps, maps)) return mesh;
    const float origin[3] = { grid.origin.x, grid.origin.y, grid.origin.z };
    const bool done = runMeshCall("meshDepthMaps", true, grid, [&](float* xyz, unsigned char* bgr, int64_t vcap, int32_t* tri, int64_t tcap, int64_t* nv, int64_t* nt) {
        return sfmba_tsdf_mesh(0, (int)images.size(), f.ptr.data(), f.px.data(), f.w.data(), f.h.data(), f.channels, f.K, f.P.data(), maps.data(), origin,
                               grid.voxel, grid.nx, grid.ny, grid.nz, grid.trunc, minWeight, xyz, bgr, nullptr, vcap, tri, tcap, nv, nt);
    }, mesh);
    if (!done) return Mesh();
    if (ok) *ok = true;
    return mesh;
}

Mesh SfMDenseUtilities::meshDepthMaps(const std::vector<cv::Mat>& images, const Intrinsics& intrinsics, const std::vector<cv::Matx34f>& poses,
                                      const std::vector<cv::Mat>& depthMaps, const MeshGrid& grid, int minWeight, int fillIterations,
                                      int fillMinNeighbours, bool* ok) {
    if (fillIterations == 0) return meshDepthMaps(images, intrinsics, poses, depthMaps, grid, minWeight, ok);      // the call made without the fill
    Mesh mesh;
    if (ok) *ok = false;
    FlatScene f;
    std::vector<const float*> maps;
    if (!flattenScene(images, intrinsics, poses, f) || depthMaps.size() != images.size()) {
        std::fprintf(stderr, "meshDepthMaps: one pose and one depth map (or an empty Mat) per image are needed\n");
        return mesh;
    }
    if (!mapPointers("meshDepthMaps", images, depthMaps, maps)) return mesh;
    const float origin[3] = { grid.origin.x, grid.origin.y, grid.origin.z };
    std::vector<unsigned char> filled;
    const bool done = runMeshCall("meshDepthMaps", true, grid, [&](float* xyz, unsigned char* bgr, int64_t vcap, int32_t* tri, int64_t tcap, int64_t* nv, int64_t* nt) {
        filled.assign((size_t)vcap + 1, 0);
        return sfmba_tsdf_mesh_fill(0, (int)images.size(), f.ptr.data(), f.px.data(), f.w.data(), f.h.data(), f.channels, f.K, f.P.data(), maps.data(),
                                    origin, grid.voxel, grid.nx, grid.ny, grid.nz, grid.trunc, minWeight, fillIterations, fillMinNeighbours, xyz, bgr,
                                    nullptr, filled.data(), vcap, tri, tcap, nv, nt);
    }, mesh);
    if (!done) return Mesh();
    filled.resize(mesh.vertices.size());
    mesh.filled.swap(filled);
    if (ok) *ok = true;
    return mesh;
}

bool SfMDenseUtilities::fillTSDF(const TsdfVolume& volume, int minWeight, int iterations, int minNeighbours, TsdfVolume& out,
                                 std::vector<unsigned char>* state) {
    out = TsdfVolume();
    if (state) state->clear();
    const MeshGrid& g = volume.grid;
    const int64_t cells = (int64_t)g.nx * g.ny * g.nz;
    const bool colour = !volume.csum.empty();
    if (g.nx < 1 || g.ny < 1 || g.nz < 1 || cells > ((int64_t)1 << 26) || (int64_t)volume.sum.size() != cells || (int64_t)volume.weight.size() != cells ||
        (colour && ((int64_t)volume.csum.size() != 3 * cells || (int64_t)volume.cweight.size() != cells))) {
        std::fprintf(stderr, "fillTSDF: the volume's arrays do not fit its grid\n");
        return false;
    }
    TsdfVolume v;
    v.grid = g;
    v.sum.resize((size_t)cells); v.weight.resize((size_t)cells);
    if (colour) { v.csum.resize((size_t)cells * 3); v.cweight.resize((size_t)cells); }
    std::vector<unsigned char> st(state ? (size_t)cells : 0);
    int64_t filled = 0;
    const int rc = sfmba_tsdf_fill(0, g.nx, g.ny, g.nz, volume.sum.data(), volume.weight.data(), colour ? volume.csum.data() : nullptr,
                                   colour ? volume.cweight.data() : nullptr, minWeight, iterations, minNeighbours, v.sum.data(), v.weight.data(),
                                   colour ? v.csum.data() : nullptr, colour ? v.cweight.data() : nullptr, state ? st.data() : nullptr, &filled);
    if (rc != SFMBA_OK) {
        std::fprintf(stderr, "fillTSDF failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return false;
    }
    out = v;
    if (state) state->swap(st);
    return true;
}

namespace {
// the vertices as the C ABI takes them; false if the mesh's arrays do not fit together
bool flattenMesh(const char* who, const Mesh& mesh, std::vector<float>& xyz) {
    if (mesh.triangles.size() % 3 != 0 || (!mesh.bgr.empty() && mesh.bgr.size() != 3 * mesh.vertices.size())) {
        std::fprintf(stderr, "%s: the mesh's arrays do not fit together\n", who);
        return false;
    }
    xyz.resize(3 * mesh.vertices.size() + 1);
    for (size_t i = 0; i < mesh.vertices.size(); ++i) {
        xyz[3 * i] = mesh.vertices[i].x; xyz[3 * i + 1] = mesh.vertices[i].y; xyz[3 * i + 2] = mesh.vertices[i].z;
    }
    return true;
}
}  // namespace

std::vector<int> SfMDenseUtilities::meshComponents(const Mesh& mesh, bool* ok) {
    if (ok) *ok = false;
    std::vector<float> xyz;
    if (!flattenMesh("meshComponents", mesh, xyz)) return std::vector<int>();
    std::vector<int32_t> label(mesh.vertices.size() + 1);
    int64_t components = 0, largest = 0;
    const int rc = sfmba_mesh_components(0, (int64_t)mesh.vertices.size(), (int64_t)(mesh.triangles.size() / 3), mesh.triangles.data(), label.data(),
                                         nullptr, &components, &largest);
    if (rc != SFMBA_OK) {
        std::fprintf(stderr, "meshComponents failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return std::vector<int>();
    }
    if (ok) *ok = true;
    return std::vector<int>(label.begin(), label.begin() + mesh.vertices.size());
}

Mesh SfMDenseUtilities::cleanMesh(const Mesh& mesh, const MeshCleanParams& params, bool* ok) {
    if (ok) *ok = false;
    std::vector<float> xyz;
    if (!flattenMesh("cleanMesh", mesh, xyz)) return Mesh();
    const bool colour = !mesh.bgr.empty();
    const int64_t nv = (int64_t)mesh.vertices.size(), nt = (int64_t)(mesh.triangles.size() / 3);
    // the host rules (SfM.h): the quantum is the unit the TSDF already uses, and 0 stands for a thousandth of the triangles
    const float origin[3] = { mesh.grid.origin.x, mesh.grid.origin.y, mesh.grid.origin.z };
    const float quantum = mesh.grid.voxel / 1024.0f;
    const int minTriangles = params.minComponentTriangles == 0 ? (int)std::max<int64_t>(1, nt / 1000) : params.minComponentTriangles;
    std::vector<float> normal;
    Mesh out;
    const bool done = runMeshCall("cleanMesh", colour, mesh.grid, [&](float* oxyz, unsigned char* obgr, int64_t vcap, int32_t* otri, int64_t tcap, int64_t* onv, int64_t* ont) {
        normal.assign((size_t)vcap * 3 + 1, 0.0f);
        return sfmba_mesh_clean(0, nv, xyz.data(), colour ? mesh.bgr.data() : nullptr, nt, mesh.triangles.data(), minTriangles, params.keepLargest ? 1 : 0,
                                origin, quantum, params.smoothIterations, params.lambda, params.mu, oxyz, obgr, normal.data(), vcap, otri, tcap, nullptr,
                                onv, ont);
    }, out);
    if (!done) return Mesh();
    out.normals.assign(normal.begin(), normal.begin() + 3 * out.vertices.size());
    if (ok) *ok = true;
    return out;
}

Mesh SfMDenseUtilities::decimateMesh(const Mesh& mesh, const MeshDecimateParams& params, bool* ok, long long* stats) {
    if (ok) *ok = false;
    std::vector<float> xyz;
    if (!flattenMesh("decimateMesh", mesh, xyz)) return Mesh();
    const bool colour = !mesh.bgr.empty();
    const int64_t nv = (int64_t)mesh.vertices.size(), nt = (int64_t)(mesh.triangles.size() / 3);
    // the host rules (SfM.h): the quantum is the unit the TSDF already uses, and a cell is given in voxels
    const float origin[3] = { mesh.grid.origin.x, mesh.grid.origin.y, mesh.grid.origin.z };
    const float quantum = mesh.grid.voxel / 1024.0f;
    const double cellQuanta = std::round((double)params.cellVoxels * 1024.0);
    if (!(cellQuanta >= 32.0 && cellQuanta <= 1048576.0)) {
        std::fprintf(stderr, "decimateMesh: cellVoxels * 1024 must round to 32..2^20 quanta\n");
        return Mesh();
    }
    const int cell = (int)cellQuanta;
    int64_t st[4] = { 0, 0, 0, 0 };
    Mesh out;
    const bool done = runMeshCall("decimateMesh", colour, mesh.grid, [&](float* oxyz, unsigned char* obgr, int64_t vcap, int32_t* otri, int64_t tcap, int64_t* onv, int64_t* ont) {
        return sfmba_mesh_decimate(0, nv, xyz.data(), colour ? mesh.bgr.data() : nullptr, nt, mesh.triangles.data(), origin, quantum, cell, params.placement,
                                   params.reg, oxyz, obgr, nullptr, vcap, otri, nullptr, tcap, nullptr, onv, ont, st);
    }, out);
    if (!done) return Mesh();
    // the normals: the smooth's, with no iteration, on the decimated mesh
    std::vector<float> oxyz, same, normal;
    if (!flattenMesh("decimateMesh", out, oxyz)) return Mesh();
    same.assign(oxyz.size() + 1, 0.0f);
    normal.assign(oxyz.size() + 1, 0.0f);
    const int rc = sfmba_mesh_smooth(0, (int64_t)out.vertices.size(), oxyz.data(), (int64_t)(out.triangles.size() / 3), out.triangles.data(), origin, quantum, 0,
                                     0.5f, -0.53f, same.data(), normal.data());
    if (rc != SFMBA_OK) {
        std::fprintf(stderr, "decimateMesh: the normals failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return Mesh();
    }
    out.normals.assign(normal.begin(), normal.begin() + 3 * out.vertices.size());
    if (stats) for (int i = 0; i < 4; ++i) stats[i] = (long long)st[i];
    if (ok) *ok = true;
    return out;
}

TexturedMesh SfMDenseUtilities::textureMesh(const Mesh& mesh, const std::vector<cv::Mat>& images, const Intrinsics& intrinsics,
                                            const std::vector<cv::Matx34f>& poses, const std::vector<cv::Mat>& depthMaps, const TextureParams& params,
                                            bool* ok) {
    if (ok) *ok = false;
    std::vector<float> xyz;
    FlatScene f;
    std::vector<const float*> maps;
    if (!flattenMesh("textureMesh", mesh, xyz)) return TexturedMesh();
    if (!flattenScene(images, intrinsics, poses, f) || depthMaps.size() != images.size()) {
        std::fprintf(stderr, "textureMesh: one pose and one depth map (or an empty Mat) per image are needed\n");
        return TexturedMesh();
    }
    if (!mapPointers("textureMesh", images, depthMaps, maps)) return TexturedMesh();
    if (!std::isfinite(params.minAreaPx) || params.minAreaPx < 0.0f || params.minAreaPx > 1.0e9f || params.blocksPerRow < 0) {
        std::fprintf(stderr, "textureMesh: minAreaPx must be finite and in 0..1e9, blocksPerRow >= 0 (0 = a square atlas)\n");
        return TexturedMesh();
    }
    const int64_t nv = (int64_t)mesh.vertices.size(), nt = (int64_t)(mesh.triangles.size() / 3);
    // the host rules (SfM.h)
    int B = params.blocksPerRow;
    if (B == 0)
        for (B = 1; (int64_t)B * B < (nt + 1) / 2; ++B) {}
    const float occlTol = params.occlTolVoxels * mesh.grid.voxel;
    const int64_t minArea = (int64_t)std::llround(2.0 * 256.0 * (double)params.minAreaPx);
    // the atlas of include/sfmba.h's layout (an empty mesh has one empty block); a layout the call refuses gets no atlas: the call
    // refuses before it writes
    const int64_t S = params.patch, blocks = (nt + 1) / 2;
    const int64_t W = blocks ? B * (S + 1) : S + 1, H = blocks ? ((blocks + B - 1) / B) * S : S;
    const bool sized = S >= 3 && S <= 64 && W <= 16384 && H <= 16384;
    TexturedMesh out;
    out.atlas = sized ? cv::Mat((int)H, (int)W, CV_8UC3) : cv::Mat(1, 1, CV_8UC3);
    out.uv.resize((size_t)nt * 6 + 1);
    std::vector<int32_t> view((size_t)nt + 1);
    int64_t textured = 0, stats[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, levelStats[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    // smoothing and levelling are off by default: the call is then exactly the plain one
    out.smoothed = params.smoothRings != 0 || params.smoothPasses != 0;
    out.levelled = params.levelPasses != 0;
    const unsigned char* bgr = mesh.bgr.empty() ? nullptr : mesh.bgr.data();
    const int rc = out.levelled
        ? sfmba_mesh_texture_adjust(0, nv, xyz.data(), bgr, nt, mesh.triangles.data(), (int)images.size(), f.ptr.data(), f.px.data(), f.w.data(), f.h.data(),
                                    f.channels, f.K, f.P.data(), maps.data(), occlTol, minArea, params.patch, B, params.candidates, params.smoothRings,
                                    params.smoothPenalty, params.smoothPasses, out.atlas.ptr<unsigned char>(0), out.uv.data(), view.data(), nullptr,
                                    &textured, stats, params.levelSampleRadius, params.levelSeamWeight, params.levelPasses, levelStats)
        : out.smoothed
        ? sfmba_mesh_texture_smooth(0, nv, xyz.data(), bgr, nt, mesh.triangles.data(), (int)images.size(), f.ptr.data(), f.px.data(), f.w.data(), f.h.data(),
                                    f.channels, f.K, f.P.data(), maps.data(), occlTol, minArea, params.patch, B, params.candidates, params.smoothRings,
                                    params.smoothPenalty, params.smoothPasses, out.atlas.ptr<unsigned char>(0), out.uv.data(), view.data(), nullptr,
                                    &textured, stats)
        : sfmba_mesh_texture(0, nv, xyz.data(), bgr, nt, mesh.triangles.data(), (int)images.size(), f.ptr.data(), f.px.data(), f.w.data(), f.h.data(),
                             f.channels, f.K, f.P.data(), maps.data(), occlTol, minArea, params.patch, B, out.atlas.ptr<unsigned char>(0), out.uv.data(),
                             view.data(), nullptr, &textured);
    if (rc != SFMBA_OK) {
        std::fprintf(stderr, "textureMesh failed (sfmba rc=%d: %s)\n", rc, sfmba_last_error());
        return TexturedMesh();
    }
    out.vertices = mesh.vertices;
    out.triangles = mesh.triangles;
    out.uv.resize((size_t)nt * 6);
    out.view.assign(view.begin(), view.begin() + nt);
    out.textured = (long long)textured;
    for (int i = 0; i < 8; ++i) out.smoothStats[i] = out.smoothed ? (long long)stats[i] : 0;
    for (int i = 0; i < 8; ++i) out.levelStats[i] = (long long)levelStats[i];
    if (ok) *ok = true;
    return out;
}

}  // namespace sfmtoylib
