"""Calls every timed front-end entry point once, with every SFMBA_*_TIMING switch set by the caller: each call leaves one
"[sfmba <tag>] name value ..." line on stderr.  Run as a child process by tests/test_gpu_timing_lines.py.

Each unit gets the smallest case of its tests/*_cases.py that still gives every phase something to do; the units without such a
file (the Hamming matcher and the three RANSAC units) get the valid call of tests/frontend_refusal_cases.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

SWITCHES = ("SFMBA_MATCH_TIMING", "SFMBA_ORB_TIMING", "SFMBA_SURF_TIMING", "SFMBA_DEPTH_TIMING", "SFMBA_FLOW_TIMING", "SFMBA_CLOUD_TIMING",
            "SFMBA_PNP_TIMING", "SFMBA_HOMOGRAPHY_TIMING", "SFMBA_ESSENTIAL_TIMING", "SFMBA_JPEG_TIMING", "SFMBA_PNG_TIMING")


def main():
    from sfm_toy_library_amd import capi
    import cloud_cases
    import depth_cases
    import flow_cases
    import frontend_refusal_cases as frc
    import jpeg_cases
    import match_l2_cases
    import orb_cases
    import png_cases
    import surf_cases

    for name in ("sfmba_match_features", "sfmba_pnp_ransac", "sfmba_homography_ransac", "sfmba_essential_ransac"):
        e = frc.BY_NAME[name]
        rc, msg, _ = frc.invoke(capi.lib(), e, e.args())
        assert rc == 0, (name, msg)

    index = min((i for i, (q, t, d) in enumerate(match_l2_cases.CASES) if q > 0 and t >= 2), key=lambda i: np.prod(match_l2_cases.CASES[i]))
    capi.match_features_l2(match_l2_cases.case_rows(index))

    name = min((n for n in orb_cases.CASES if n.startswith("noise")), key=lambda n: orb_cases.image(n).size)
    capi.orb_extract([orb_cases.image(name)], **orb_cases.params(name))
    name = min((n for n in surf_cases.CASES if n.startswith("noise") and min(surf_cases.image(n).shape[:2]) >= 40), key=lambda n: surf_cases.image(n).size)
    capi.surf_extract([surf_cases.image(name)], **surf_cases.params(name))

    c = depth_cases.case(next(iter(depth_cases.CASES)))
    capi.depth_sweep(c["images"], c["K"], c["P"], c["jobs"], **c["params"])
    images, K, P, maps = depth_cases.fuse_scene()
    capi.depth_fuse(images, K, P, maps, [[1, 2], [0], [0]])

    c = flow_cases.case(next(iter(flow_cases.TRACK_CASES)))
    capi.flow_track(c["images"], c["pairs"], c["points"], **c["params"])
    c = flow_cases.match_case(next(iter(flow_cases.MATCH_CASES)))
    capi.flow_match(c["keypoints"], c["pairs"], c["tracked"], **c["params"])

    c = cloud_cases.normals_case(next(iter(cloud_cases.NORMAL_CASES)))
    capi.depth_normals(c["K"], c["P"][None], [c["depth"]], max_rel_step=float(c["max_rel_step"]))
    c = cloud_cases.case(next(iter(cloud_cases.CASES)))
    capi.cloud_merge(c["xyz"], c["bgr"], c["normal"], voxel=float(c["voxel"]), min_count=c["min_count"])

    capi.jpeg_decode([min((jpeg_cases.small_file(n) for n in jpeg_cases.decodable_names()), key=len)])
    capi.resize_images([jpeg_cases.resize_sources()["67x43x1"]], 0.5)
    capi.png_decode([min((png_cases.small_file(n) for n in png_cases.decodable_names()), key=len)])


if __name__ == "__main__":
    missing = [s for s in SWITCHES if not os.environ.get(s)]
    assert not missing, missing
    main()
