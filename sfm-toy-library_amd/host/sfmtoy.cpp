// sfmtoy.cpp -- the command-line program of the reference (main.cpp) over sfmtoylib::SfM of this directory: read the images of a
// directory, run the pipeline on the MI355X (-M flow: with the optical-flow matcher), write <prefix>_points.ply and <prefix>_cameras.ply -- and, with -D, densify and write
// <prefix>_dense.ply; with --voxel on top of -D, merge that cloud and write <prefix>_dense_merged.ply; with --mesh on top of -D, mesh
// the depth maps and write <prefix>_mesh.ply (--mesh-fill N: with the grid's holes filled by N passes first); with --mesh-clean on top of --mesh, drop the mesh's small components, smooth it and write
// <prefix>_mesh_clean.ply; with --mesh-decimate on top of --mesh, cluster the vertices of the mesh (the clean one with --mesh-clean) into cells and
// write <prefix>_mesh_decimated.ply; with --texture on top of --mesh, put the photographs on the mesh (the decimated one with --mesh-decimate, else the clean one with --mesh-clean) and write
// <prefix>_textured.obj, .mtl and .png (--texture-smooth: with the views of neighbouring triangles chosen together; --texture-level: with the colours levelled across the seams).  The arguments are parsed here
// (no boost).  Exit status: 0 when runSfM returned OKAY and the files were written, 1 on ERROR, 2 on a usage error.
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "SfM.h"

using namespace sfmtoylib;

namespace {

void usage(std::ostream& os, const char* program) {
    os << "usage: " << program << " [options] <input-directory>\n"
       << "  -h, --help                   this text\n"
       << "  -p, --input-directory DIR    directory of .jpg / .jpeg / .png / .pgm / .ppm images (also as the positional argument)\n"
       << "  -s, --downscale F            factor applied to every image at load time (default 1)\n"
       << "  -d, --console-debug N        console log level, 0 = trace .. 4 = error (default 2)\n"
       << "  -o, --output-prefix PREFIX   PREFIX_points.ply and PREFIX_cameras.ply (default output)\n"
       << "  -f, --features orb|surf      the extractor: orb (binary rows, Hamming; the default) or surf (64 floats, L2)\n"
       << "  -m, --merge-distance F       distance below which a match confirms a merge (default 20: ORB's Hamming scale; unit-length\n"
       << "                               float rows never lie further than 2 apart, so 20 confirms every match of theirs)\n"
       << "  -M, --matcher NAME           stage 2: descriptors (2-NN ratio test; the default) or flow (pyramidal Lucas-Kanade between\n"
       << "                               the images and a snap to key points, for frame sequences; a match's distance is <= 2 px)\n"
       << "  -w, --flow-window N          with -M flow: match view i with views i+1 .. i+N only (default 0: all pairs)\n"
       << "  -D, --dense                  also densify (plane-sweep depth maps of the registered views, fused) and write PREFIX_dense.ply\n"
       << "      --sgm [P1,P2]            with -D: regularise the depth maps by semi-global matching over the sweep's cost volume, with the\n"
       << "                               penalties P1 <= P2 in 0..1023 (default 8,64); every pixel then gets a plane, one without texture\n"
       << "                               from its neighbours; NO LEFT-RIGHT CHECK, the fuse is the cross-check\n"
       << "      --sgm-paths 4|8          with --sgm: path directions (default 8)\n"
       << "      --sgm-uniqueness U       with --sgm: a pixel needs 100 (second - best) >= U * second, 0..100 (default 5)\n"
       << "      --voxel SIZE             with -D: also merge the dense cloud into one oriented point per voxel of edge SIZE (0 = the\n"
       << "                               footprint of a pixel at the typical depth) and write PREFIX_dense_merged.ply\n"
       << "      --mesh RES               with -D: also mesh the depth maps (TSDF fusion and marching tetrahedra on a grid of RES vertices\n"
       << "                               along the longest side of the dense cloud's box, 2..1024) and write PREFIX_mesh.ply\n"
       << "      --mesh-fill N            with --mesh: fill the holes of the grid by N passes of volumetric diffusion, 0..254 (default 0: off);\n"
       << "                               PAST AN OPEN BORDER THE SURFACE CONTINUES AS A SKIRT UP TO N VOXELS WIDE\n"
       << "      --mesh-fill-neighbours K with --mesh-fill: known face neighbours a grid vertex needs to be filled, 1..6 (default 2)\n"
       << "      --mesh-clean             with --mesh: also drop the mesh's small components, smooth the rest (Taubin, 10 iterations) and\n"
       << "                               write PREFIX_mesh_clean.ply with a normal per vertex; the other files are as without it\n"
       << "      --mesh-min-component N   with --mesh-clean: a component with fewer than N triangles goes (default 0: a thousandth of the\n"
       << "                               mesh's triangles, at least 1)\n"
       << "      --mesh-keep-largest      with --mesh-clean: keep only the component with the most triangles\n"
       << "      --mesh-smooth ITERS      with --mesh-clean: smoothing iterations, 0..100 (default 10)\n"
       << "      --mesh-decimate [C]      with --mesh: also collapse every cell of C voxels (default 2; C * 1024 must round to 32..1048576) of the\n"
       << "                               mesh (the clean one with --mesh-clean) to one vertex, placed by the cell's quadric, and write\n"
       << "                               PREFIX_mesh_decimated.ply with a normal per vertex; --texture then works on this mesh; first choices\n"
       << "                               that nobody has tuned; NO TOPOLOGY GUARANTEE; the other files are as without it\n"
       << "      --mesh-decimate-mean     with --mesh-decimate: place a cell's vertex at the rounded mean of its vertices instead\n"
       << "      --texture [S]            with --mesh: also choose a view per triangle, fill a texture atlas with a patch of S (S + 1) / 2 texels\n"
       << "                               per triangle (S in 3..64, default 6) and write PREFIX_textured.obj, .mtl and .png (the clean mesh\n"
       << "                               with --mesh-clean); NO COLOUR ADJUSTMENT ACROSS VIEWS unless --texture-level asks for it; the other\n"
       << "                               files are as without it\n"
       << "      --texture-smooth [R,P]   with --texture: choose the views of neighbouring triangles together: every view's score summed over R\n"
       << "                               rings of neighbours (0..8) before the choice, then a Potts relaxation in which a pair of neighbours\n"
       << "                               with different views costs P (0..65535, in 1/1024 of the best view's area); default 4,256, first\n"
       << "                               choices that nobody has tuned; the other files are as without it\n"
       << "      --texture-smooth-passes N  with --texture-smooth: the most relaxation passes, 0..10000 (default 100)\n"
       << "      --texture-level [N[,W]]  with --texture: level the colours across the seams between photographs: an additive offset per vertex\n"
       << "                               and view by N integer Jacobi passes (1..1024) with the seam weight W (1..256); default 16,16, first\n"
       << "                               choices that nobody has tuned; only PREFIX_textured.png changes\n"
       << "      --texture-level-radius R with --texture-level: a vertex's colour in a view is the mean over (2 R + 1)^2 samples, 0..2 (default 1)\n"
       << "  -v, --visual-debug N         accepted and ignored: there is no visual debugging\n";
}

// "--name=value" or "-n value" / "--name value": true when argv[i] is this option, with the value in `value` (i then stands on
// the last argument consumed); `missing` is set when the value is absent
bool option(int argc, char** argv, int& i, const char* brief, const char* full, std::string& value, bool& missing) {
    const std::string arg = argv[i], prefix = std::string(full) + "=";
    if (arg.compare(0, prefix.size(), prefix) == 0) { value = arg.substr(prefix.size()); return true; }
    if (arg != brief && arg != full) return false;
    if (i + 1 >= argc) { missing = true; return true; }
    value = argv[++i];
    return true;
}

bool number(const std::string& text, double& value) {
    char* end = nullptr;
    value = std::strtod(text.c_str(), &end);
    return !text.empty() && end && *end == '\0';
}

}  // namespace

int main(int argc, char** argv) {
    std::string directory, prefix = "output", text;
    double downscale = 1.0, level = LOG_INFO, ignored = 0.0, merge = 20.0, window = 0.0, voxel = 0.0, resolution = 256.0,
           min_component = 0.0, smooth = 10.0, fill = 0.0, fill_neighbours = 2.0, patch = 6.0, sgm_p1 = 8.0, sgm_p2 = 64.0, sgm_paths = 8.0,
           sgm_uniqueness = 5.0, smooth_rings = 4.0, smooth_penalty = 256.0, smooth_passes = 100.0, level_passes = 16.0, level_weight = 16.0,
           level_radius = 1.0, decimate_cell = 2.0;
    FeatureType features = FEATURES_ORB;
    MatcherType matcher = MATCHER_DESCRIPTORS;
    bool have_directory = false, dense = false, merged = false, meshed = false, cleaned = false, clean_option = false, keep_largest = false,
         filled = false, fill_option = false, textured = false, sgm = false, sgm_option = false, texture_smooth = false, smooth_option = false, texture_level = false,
         level_option = false, decimated = false, decimate_mean = false;
    for (int i = 1; i < argc; ++i) {
        bool missing = false, bad = false;
        const std::string arg = argv[i];
        if (arg == "-h" || arg == "--help") { usage(std::cout, argv[0]); return 0; }
        if (arg == "-D" || arg == "--dense") { dense = true; continue; }
        if (arg == "--mesh-clean") { cleaned = true; continue; }
        if (arg == "--mesh-keep-largest") { keep_largest = clean_option = true; continue; }
        if (arg == "--mesh-decimate-mean") { decimate_mean = true; continue; }
        if (arg == "--mesh-decimate" || arg.compare(0, 16, "--mesh-decimate=") == 0) {
            // the value is optional: "--mesh-decimate=C", or a next argument made of digits and a point only
            decimated = true;
            text = arg.size() > 16 ? arg.substr(16) : "";
            if (arg == "--mesh-decimate" && i + 1 < argc && argv[i + 1][0] != '\0' && std::string(argv[i + 1]).find_first_not_of("0123456789.") == std::string::npos)
                text = argv[++i];
            else if (arg == "--mesh-decimate")
                continue;
            if (!number(text, decimate_cell) || !(decimate_cell * 1024.0 >= 31.5) || !(decimate_cell * 1024.0 < 1048576.5)) {
                std::cerr << argv[0] << ": --mesh-decimate has a value that cannot be used\n"; usage(std::cerr, argv[0]); return 2;
            }
            continue;
        }
        if (arg == "--texture" || arg.compare(0, 10, "--texture=") == 0) {
            // the value is optional: "--texture=S", or a next argument made of digits only
            textured = true;
            text = arg.size() > 10 ? arg.substr(10) : "";
            if (arg == "--texture" && i + 1 < argc && argv[i + 1][0] != '\0' && std::string(argv[i + 1]).find_first_not_of("0123456789") == std::string::npos)
                text = argv[++i];
            else if (arg == "--texture")
                continue;
            if (!number(text, patch) || !(patch >= 3.0) || !(patch <= 64.0) || patch != (double)(int)patch) {
                std::cerr << argv[0] << ": --texture has a value that cannot be used\n"; usage(std::cerr, argv[0]); return 2;
            }
            continue;
        }
        if (arg == "--texture-smooth" || arg.compare(0, 17, "--texture-smooth=") == 0) {
            // the value is optional: "--texture-smooth=R,P", or a next argument made of digits around a comma
            texture_smooth = true;
            text = arg.size() > 17 ? arg.substr(17) : "";
            if (arg == "--texture-smooth" && i + 1 < argc && std::isdigit((unsigned char)argv[i + 1][0]) &&
                std::string(argv[i + 1]).find(',') != std::string::npos && std::string(argv[i + 1]).find_first_not_of("0123456789,") == std::string::npos)
                text = argv[++i];
            else if (arg == "--texture-smooth")
                continue;
            const size_t comma = text.find(',');
            if (comma == std::string::npos || !number(text.substr(0, comma), smooth_rings) || !number(text.substr(comma + 1), smooth_penalty) ||
                !(smooth_rings >= 0.0) || !(smooth_rings <= 8.0) || !(smooth_penalty >= 0.0) || !(smooth_penalty <= 65535.0) ||
                smooth_rings != (double)(int)smooth_rings || smooth_penalty != (double)(int)smooth_penalty) {
                std::cerr << argv[0] << ": --texture-smooth has a value that cannot be used\n"; usage(std::cerr, argv[0]); return 2;
            }
            continue;
        }
        if (arg == "--texture-level" || arg.compare(0, 16, "--texture-level=") == 0) {
            // the value is optional: "--texture-level=N[,W]", or a next argument made of digits with at most one comma among them
            texture_level = true;
            text = arg.size() > 16 ? arg.substr(16) : "";
            if (arg == "--texture-level" && i + 1 < argc && std::isdigit((unsigned char)argv[i + 1][0]) &&
                std::string(argv[i + 1]).find_first_not_of("0123456789,") == std::string::npos)
                text = argv[++i];
            else if (arg == "--texture-level")
                continue;
            const size_t comma = text.find(',');
            const bool weighted = comma != std::string::npos;
            if (!number(text.substr(0, comma), level_passes) || (weighted && !number(text.substr(comma + 1), level_weight)) || !(level_passes >= 1.0) ||
                !(level_passes <= 1024.0) || !(level_weight >= 1.0) || !(level_weight <= 256.0) || level_passes != (double)(int)level_passes ||
                level_weight != (double)(int)level_weight) {
                std::cerr << argv[0] << ": --texture-level has a value that cannot be used\n"; usage(std::cerr, argv[0]); return 2;
            }
            continue;
        }
        if (arg == "--sgm" || arg.compare(0, 6, "--sgm=") == 0) {
            // the value is optional: "--sgm=P1,P2", or a next argument made of digits around a comma (a directory named 2024 is none)
            sgm = true;
            text = arg.size() > 6 ? arg.substr(6) : "";
            if (arg == "--sgm" && i + 1 < argc && std::isdigit((unsigned char)argv[i + 1][0]) &&
                std::string(argv[i + 1]).find(',') != std::string::npos && std::string(argv[i + 1]).find_first_not_of("0123456789,") == std::string::npos)
                text = argv[++i];
            else if (arg == "--sgm")
                continue;
            const size_t comma = text.find(',');
            if (comma == std::string::npos || !number(text.substr(0, comma), sgm_p1) || !number(text.substr(comma + 1), sgm_p2) || !(sgm_p1 >= 0.0) ||
                !(sgm_p1 <= sgm_p2) || !(sgm_p2 <= 1023.0) || sgm_p1 != (double)(int)sgm_p1 || sgm_p2 != (double)(int)sgm_p2) {
                std::cerr << argv[0] << ": --sgm has a value that cannot be used\n"; usage(std::cerr, argv[0]); return 2;
            }
            continue;
        }
        if (option(argc, argv, i, "-p", "--input-directory", text, missing)) { directory = text; have_directory = !missing; }
        else if (option(argc, argv, i, "-o", "--output-prefix", text, missing)) prefix = text;
        else if (option(argc, argv, i, "-s", "--downscale", text, missing)) bad = !missing && (!number(text, downscale) || !(downscale > 0.0));
        else if (option(argc, argv, i, "-d", "--console-debug", text, missing)) bad = !missing && (!number(text, level) || level < 0.0 || level > 4.0);
        else if (option(argc, argv, i, "-f", "--features", text, missing)) {
            bad = !missing && text != "orb" && text != "surf";
            features = text == "surf" ? FEATURES_SURF : FEATURES_ORB;
        }
        else if (option(argc, argv, i, "-M", "--matcher", text, missing)) {
            bad = !missing && text != "descriptors" && text != "flow";
            matcher = text == "flow" ? MATCHER_FLOW : MATCHER_DESCRIPTORS;
        }
        else if (option(argc, argv, i, "-w", "--flow-window", text, missing))
            bad = !missing && (!number(text, window) || !(window >= 0.0) || !(window <= 1.0e6) || window != (double)(int)window);
        else if (option(argc, argv, i, "-m", "--merge-distance", text, missing)) bad = !missing && (!number(text, merge) || !(merge >= 0.0) || !(merge <= 3.0e38));
        else if (option(argc, argv, i, "--sgm-paths", "--sgm-paths", text, missing)) {
            bad = !missing && (!number(text, sgm_paths) || (sgm_paths != 4.0 && sgm_paths != 8.0));
            sgm_option = true;
        }
        else if (option(argc, argv, i, "--sgm-uniqueness", "--sgm-uniqueness", text, missing)) {
            bad = !missing && (!number(text, sgm_uniqueness) || !(sgm_uniqueness >= 0.0) || !(sgm_uniqueness <= 100.0) || sgm_uniqueness != (double)(int)sgm_uniqueness);
            sgm_option = true;
        }
        else if (option(argc, argv, i, "--voxel", "--voxel", text, missing)) {
            bad = !missing && (!number(text, voxel) || !(voxel >= 0.0) || !(voxel <= 3.0e38));
            merged = true;
        }
        else if (option(argc, argv, i, "--mesh", "--mesh", text, missing)) {
            bad = !missing && (!number(text, resolution) || !(resolution >= 2.0) || !(resolution <= 1024.0) || resolution != (double)(int)resolution);
            meshed = true;
        }
        else if (option(argc, argv, i, "--mesh-fill", "--mesh-fill", text, missing)) {
            bad = !missing && (!number(text, fill) || !(fill >= 0.0) || !(fill <= 254.0) || fill != (double)(int)fill);
            filled = true;
        }
        else if (option(argc, argv, i, "--mesh-fill-neighbours", "--mesh-fill-neighbours", text, missing)) {
            bad = !missing && (!number(text, fill_neighbours) || !(fill_neighbours >= 1.0) || !(fill_neighbours <= 6.0) || fill_neighbours != (double)(int)fill_neighbours);
            fill_option = true;
        }
        else if (option(argc, argv, i, "--mesh-min-component", "--mesh-min-component", text, missing)) {
            bad = !missing && (!number(text, min_component) || !(min_component >= 0.0) || !(min_component <= 2147483647.0) || min_component != (double)(int)min_component);
            clean_option = true;
        }
        else if (option(argc, argv, i, "--mesh-smooth", "--mesh-smooth", text, missing)) {
            bad = !missing && (!number(text, smooth) || !(smooth >= 0.0) || !(smooth <= 100.0) || smooth != (double)(int)smooth);
            clean_option = true;
        }
        else if (option(argc, argv, i, "--texture-smooth-passes", "--texture-smooth-passes", text, missing)) {
            bad = !missing && (!number(text, smooth_passes) || !(smooth_passes >= 0.0) || !(smooth_passes <= 10000.0) || smooth_passes != (double)(int)smooth_passes);
            smooth_option = true;
        }
        else if (option(argc, argv, i, "--texture-level-radius", "--texture-level-radius", text, missing)) {
            bad = !missing && (!number(text, level_radius) || !(level_radius >= 0.0) || !(level_radius <= 2.0) || level_radius != (double)(int)level_radius);
            level_option = true;
        }
        else if (option(argc, argv, i, "-v", "--visual-debug", text, missing)) bad = !missing && !number(text, ignored);
        else if (arg.size() > 1 && arg[0] == '-') { std::cerr << argv[0] << ": unknown option " << arg << "\n"; usage(std::cerr, argv[0]); return 2; }
        else if (!have_directory) { directory = arg; have_directory = true; }
        else { std::cerr << argv[0] << ": more than one input directory\n"; usage(std::cerr, argv[0]); return 2; }
        if (missing || bad) { std::cerr << argv[0] << ": " << arg << (missing ? " needs a value\n" : " has a value that cannot be used\n"); usage(std::cerr, argv[0]); return 2; }
    }
    if (sgm && !dense) { std::cerr << argv[0] << ": --sgm needs -D\n"; usage(std::cerr, argv[0]); return 2; }
    if (sgm_option && !sgm) { std::cerr << argv[0] << ": --sgm-paths and --sgm-uniqueness need --sgm\n"; usage(std::cerr, argv[0]); return 2; }
    if (merged && !dense) { std::cerr << argv[0] << ": --voxel needs -D\n"; usage(std::cerr, argv[0]); return 2; }
    if (meshed && !dense) { std::cerr << argv[0] << ": --mesh needs -D\n"; usage(std::cerr, argv[0]); return 2; }
    if (filled && !meshed) { std::cerr << argv[0] << ": --mesh-fill needs --mesh\n"; usage(std::cerr, argv[0]); return 2; }
    if (fill_option && !filled) { std::cerr << argv[0] << ": --mesh-fill-neighbours needs --mesh-fill\n"; usage(std::cerr, argv[0]); return 2; }
    if (cleaned && !meshed) { std::cerr << argv[0] << ": --mesh-clean needs --mesh\n"; usage(std::cerr, argv[0]); return 2; }
    if (clean_option && !cleaned) { std::cerr << argv[0] << ": --mesh-min-component, --mesh-keep-largest and --mesh-smooth need --mesh-clean\n"; usage(std::cerr, argv[0]); return 2; }
    if (decimated && !meshed) { std::cerr << argv[0] << ": --mesh-decimate needs --mesh\n"; usage(std::cerr, argv[0]); return 2; }
    if (decimate_mean && !decimated) { std::cerr << argv[0] << ": --mesh-decimate-mean needs --mesh-decimate\n"; usage(std::cerr, argv[0]); return 2; }
    if (textured && !meshed) { std::cerr << argv[0] << ": --texture needs --mesh\n"; usage(std::cerr, argv[0]); return 2; }
    if (texture_smooth && !textured) { std::cerr << argv[0] << ": --texture-smooth needs --texture\n"; usage(std::cerr, argv[0]); return 2; }
    if (smooth_option && !texture_smooth) { std::cerr << argv[0] << ": --texture-smooth-passes needs --texture-smooth\n"; usage(std::cerr, argv[0]); return 2; }
    if (texture_level && !textured) { std::cerr << argv[0] << ": --texture-level needs --texture\n"; usage(std::cerr, argv[0]); return 2; }
    if (level_option && !texture_level) { std::cerr << argv[0] << ": --texture-level-radius needs --texture-level\n"; usage(std::cerr, argv[0]); return 2; }
    if (!have_directory || directory.empty()) { std::cerr << argv[0] << ": no input directory\n"; usage(std::cerr, argv[0]); return 2; }

    SfM sfm((float)downscale);
    sfm.setConsoleDebugLevel((unsigned int)level);
    sfm.setFeatureType(features);
    sfm.setMatcherType(matcher);
    sfm.setFlowPairWindow((int)window);
    sfm.setMergeFeatureMatchDistance((float)merge);
    if (!sfm.setImagesDirectory(directory)) return 1;
    if (sfm.runSfM() != OKAY) return 1;
    if (!sfm.saveCloudAndCamerasToPLY(prefix)) return 1;
    if (!dense) return 0;
    DenseParams dense_params;
    dense_params.sgm = sgm;
    dense_params.sgmP1 = (int)sgm_p1;
    dense_params.sgmP2 = (int)sgm_p2;
    dense_params.sgmPaths = (int)sgm_paths;
    dense_params.sgmUniqueness = (int)sgm_uniqueness;
    if (sfm.densify(dense_params) != OKAY) return 1;
    if (!sfm.saveDenseCloudToPLY(prefix)) return 1;
    if (merged) {
        if (sfm.mergeDenseCloud((float)voxel) != OKAY) return 1;
        if (!sfm.saveMergedDenseCloudToPLY(prefix)) return 1;
    }
    if (meshed) {
        MeshParams params;
        params.resolution = (int)resolution;
        params.fillIterations = (int)fill;
        params.fillMinNeighbours = (int)fill_neighbours;
        if (sfm.meshDenseCloud(params) != OKAY) return 1;
        if (!sfm.saveMeshToPLY(prefix)) return 1;
        if (cleaned) {
            MeshCleanParams clean;
            clean.minComponentTriangles = (int)min_component;
            clean.keepLargest = keep_largest;
            clean.smoothIterations = (int)smooth;
            if (sfm.cleanMesh(clean) != OKAY) return 1;
            if (!sfm.saveCleanMeshToPLY(prefix)) return 1;
        }
        if (decimated) {
            MeshDecimateParams decimate;
            decimate.cellVoxels = (float)decimate_cell;
            if (decimate_mean) decimate.placement = MeshDecimateParams::MEAN;
            if (sfm.decimateMesh(decimate) != OKAY) return 1;
            if (!sfm.saveDecimatedMeshToPLY(prefix)) return 1;
        }
        if (textured) {
            TextureParams texture;
            texture.patch = (int)patch;
            if (texture_smooth) {
                texture.smoothRings = (int)smooth_rings;
                texture.smoothPenalty = (int)smooth_penalty;
                texture.smoothPasses = (int)smooth_passes;
            }
            if (texture_level) {
                texture.levelPasses = (int)level_passes;
                texture.levelSeamWeight = (int)level_weight;
                texture.levelSampleRadius = (int)level_radius;
            }
            if (sfm.textureMesh(texture) != OKAY) return 1;
            if (!sfm.saveTexturedMeshToOBJ(prefix)) return 1;
        }
    }
    return 0;
}
