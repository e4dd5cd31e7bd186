"""The argument refusals of the front-end entry points (csrc/api_frontend.hip), as small ctypes calls.

For every entry point: its signature, one valid smallest call, and a list of (defect, overrides) -- the valid call with the named
arguments replaced so that exactly one thing is wrong.  tests/golden/make_frontend_refusals.py records what a library answers to each
(rc and sfmba_last_error()); tests/test_frontend_refusals_cpu.py replays the table.  Every refusal comes back before the device
check, so none of this needs a GPU.  No input array is larger than a few KB: where a limit (2^22 rows, 2^31 entries) is reached, it is
reached through the pointer arrays alone, and the data pointer the library never gets to read is DUMMY.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

I32, I64, F32, F64, U8 = np.int32, np.int64, np.float32, np.float64, np.uint8
SENTINEL = 0xA5
INT_MAX = 2 ** 31 - 1
NAN = float("nan")
DUMMY = np.zeros(64, U8)          # a non-NULL pointer for an array that a refused call never reads

_SCALARS = {"i": C.c_int, "q": C.c_int64, "f": C.c_float, "d": C.c_double, "Q": C.c_uint64}


def a(values, dtype):
    return np.ascontiguousarray(values, dtype=dtype)


def out(dtype, n):
    """An output array; invoke() prefills it with the sentinel."""
    return np.zeros(n, dtype=dtype)


def ptr(*values):
    return a(values, I64)


def idx(*values):
    return a(values, I32)


class Entry:
    def __init__(self, name, sig, outputs, valid, cases):
        self.name = name
        self.sig = [s.split(":") for s in sig.split()]          # (argument, kind): i q f d Q scalars, p array, P array of arrays
        self.outputs = outputs.split()
        self.valid = valid                                        # () -> dict of every argument
        self.cases = cases                                        # [(defect, overrides or callable(args) -> overrides)]

    def args(self, overrides=None):
        args = self.valid()
        if callable(overrides):
            overrides = overrides(args)
        args.update(overrides or {})
        return args


def _arrays(value):
    if isinstance(value, np.ndarray):
        return [value]
    if isinstance(value, (list, tuple)):
        return [v for v in value if isinstance(v, np.ndarray)]
    return []


def invoke(lib, entry, args):
    """Call `entry` with `args`; returns (rc, message, outputs_untouched)."""
    outs = [arr for name in entry.outputs for arr in _arrays(args[name]) if arr is not DUMMY]
    for arr in outs:
        arr.view(U8).reshape(-1)[:] = SENTINEL
    keep, cargs = [], []
    for name, kind in entry.sig:
        v = args[name]
        if kind in _SCALARS:
            cargs.append(_SCALARS[kind](v))
        elif kind == "p":
            cargs.append(None if v is None else C.c_void_p(v.ctypes.data))
        else:
            if v is None:
                cargs.append(None)
            else:
                table = (C.c_void_p * max(len(v), 1))(*[None if x is None else x.ctypes.data for x in v])
                keep.append(table)
                cargs.append(table)
    fn = getattr(lib, entry.name)
    fn.restype = C.c_int
    rc = fn(*cargs)
    lib.sfmba_last_error.restype = C.c_char_p
    msg = (lib.sfmba_last_error() or b"").decode()
    untouched = all(bool((arr.view(U8) == SENTINEL).all()) for arr in outs)
    return int(rc), msg, untouched


# ---- shared pieces of the valid calls -----------------------------------------------------------------------------------------
K33 = a([100, 0, 16, 0, 100, 16, 0, 0, 1], F32)
P_EYE = a([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)
P_SIDE = a([1, 0, 0, -1, 0, 1, 0, 0, 0, 0, 1, 0], F32)


def noise(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=w * h, dtype=np.uint8)


def _match_list():
    """two images of 4 points each, one pair with 4 matches (the RANSAC entries and triangulate_pairs)"""
    pts = a([[4, 4], [20, 6], [8, 22], [25, 25], [5, 4], [21, 7], [9, 21], [27, 26]], F32)
    return dict(n_images=2, img_ptr=ptr(0, 4, 8), pts=pts, n_pairs=1, pair_left=idx(0), pair_right=idx(1), pair_ptr=ptr(0, 4),
                query_idx=idx(0, 1, 2, 3), train_idx=idx(0, 1, 2, 3))


MATCH_LIST_CASES = [
    ("n_pairs < 0", dict(n_pairs=-1)),
    ("img_ptr NULL", dict(img_ptr=None)),
    ("img_ptr[0] < 0", dict(img_ptr=ptr(-1, 4, 8))),
    ("pair_ptr[0] < 0", dict(pair_ptr=ptr(-1, 3))),
    ("img_ptr not monotone", dict(img_ptr=ptr(0, 8, 4))),
    ("pair_ptr not monotone", dict(pair_ptr=ptr(4, 0))),
    ("a pair with 2^31 matches, through pair_ptr alone", dict(pair_ptr=ptr(0, 2 ** 31), query_idx=DUMMY, train_idx=DUMMY)),
    ("pair_left out of range", dict(pair_left=idx(2))),
    ("pair_right negative", dict(pair_right=idx(-1))),
    ("query_idx NULL", dict(query_idx=None)),
    ("pts NULL", dict(pts=None)),
    ("a query_idx past its image", dict(query_idx=idx(0, 1, 2, 4))),
    ("a train_idx negative", dict(train_idx=idx(0, -1, 2, 3))),
]
RANSAC_CASES = [
    ("n_hyp 0", dict(n_hyp=0)),
    ("n_hyp 65537", dict(n_hyp=65537)),
    ("threshold_px 0", dict(threshold_px=0.0)),
    ("threshold_px NaN", dict(threshold_px=NAN)),
]
FOCAL_CASES = [
    ("fx 0", dict(K=a([0, 0, 16, 0, 100, 16, 0, 0, 1], F32))),
    ("fy infinite", dict(K=a([100, 0, 16, 0, np.inf, 16, 0, 0, 1], F32))),
]


def _images(n=1, w=48, h=40, channels=1):
    px = np.concatenate([noise(w * channels, h, seed=i) for i in range(n)])
    return dict(n_images=n, img_ptr=a(np.arange(n + 1) * w * h * channels, I64), pixels=px, width=a([w] * n, I32), height=a([h] * n, I32),
                channels=channels)


def image_cases(pixels="pixels", n=1):
    """defects of a batch of n 48 x 40 gray images, always in the last image"""
    size, first = 48 * 40, [48 * 40 * i for i in range(n)]

    def sides(last, others=48):
        return idx(*([others] * (n - 1) + [last]))

    def ends(last):
        return ptr(*(first + [first[-1] + last]))
    return [
        ("channels 2", dict(channels=2)),
        ("img_ptr[0] != 0", dict(img_ptr=ptr(*[1 + size * i for i in range(n + 1)]))),
        ("width 0", dict(width=sides(0), img_ptr=ends(0))),
        ("height 16385", dict(height=sides(16385, 40), img_ptr=ends(48 * 16385))),
        ("img_ptr one byte short", dict(img_ptr=ends(size - 1))),
        ("pixels NULL", {pixels: None}),
        ("width NULL", dict(width=None)),
        ("n_images < 0", dict(n_images=-1)),
    ]


def _big_images(args, n=8):
    """n images of 16384 x 16384 gray: 2^31 pixels for n = 8, described by the pointer arrays alone"""
    side = 16384
    return dict(n_images=n, img_ptr=a(np.arange(n + 1) * side * side, I64), width=a([side] * n, I32), height=a([side] * n, I32),
                P=a(np.tile(P_EYE, n), F32))


ENTRIES = []


def entry(name, sig, outputs, cases):
    def wrap(valid):
        ENTRIES.append(Entry(name, sig, outputs, valid, cases))
        return valid
    return wrap


# ---- triangulation ----------------------------------------------------------------------------------------------------------------
@entry("sfmba_triangulate", "device:i n:q left_xy:p right_xy:p K:p P_left:p P_right:p max_reproj_px:f points3d:p keep:p reproj_err:p",
       "points3d keep reproj_err",
       [("n < 0", dict(n=-1)), ("K NULL", dict(K=None)), ("left_xy NULL", dict(left_xy=None)), ("keep NULL", dict(keep=None))])
def _triangulate():
    return dict(device=0, n=1, left_xy=a([16, 16], F32), right_xy=a([6, 16], F32), K=K33, P_left=P_EYE, P_right=P_SIDE, max_reproj_px=10.0,
                points3d=out(F32, 3), keep=out(U8, 1), reproj_err=out(F32, 2))


@entry("sfmba_triangulate_pairs",
       "device:i n_images:i img_ptr:p pts:p K:p n_pairs:i pair_left:p pair_right:p pair_ptr:p query_idx:p train_idx:p mask:p P_left:p "
       "P_right:p max_reproj_px:f points3d:p keep:p reproj_err:p kept_ptr:p kept_idx:p",
       "points3d keep reproj_err kept_ptr kept_idx",
       MATCH_LIST_CASES + [
           ("kept_ptr NULL", dict(kept_ptr=None)),
           ("max_reproj_px negative", dict(max_reproj_px=-1.0)),
           ("max_reproj_px NaN", dict(max_reproj_px=NAN)),
           ("points3d NULL", dict(points3d=None)),
           ("2^31 - 11 entries in front of the first pair, through pair_ptr alone",
            dict(pair_ptr=ptr(INT_MAX - 10, INT_MAX - 10), points3d=DUMMY, keep=DUMMY, kept_idx=DUMMY, reproj_err=None)),
       ])
def _triangulate_pairs():
    m = _match_list()
    m["pts"] = a([[16, 16], [20, 16], [16, 20], [20, 20], [6, 16], [10, 16], [6, 20], [10, 20]], F32)
    return dict(device=0, K=K33, mask=None, P_left=P_EYE, P_right=P_SIDE, max_reproj_px=10.0, points3d=out(F32, 12), keep=out(U8, 4),
                reproj_err=out(F32, 8), kept_ptr=out(I64, 2), kept_idx=out(I64, 4), **m)


# ---- association ------------------------------------------------------------------------------------------------------------------
@entry("sfmba_find_2d3d_matches",
       "device:i n_views:i view_done:p n_pt:i view_ptr:p view_idx:p feat_idx:p n_pairs:i pair_left:p pair_right:p pair_ptr:p query_idx:p "
       "train_idx:p out_ptr:p out_point:p out_feature:p cap:q total:p",
       "out_ptr out_point out_feature total",
       [("cap < 0", dict(cap=-1)),
        ("view_done NULL", dict(view_done=None)),
        ("view_ptr[0] != 0", dict(view_ptr=ptr(1, 1))),
        ("pair_ptr[0] != 0", dict(pair_ptr=ptr(1, 1))),
        ("view_ptr not monotone", dict(n_pt=2, view_ptr=ptr(0, 1, 0))),
        ("pair_ptr not monotone", dict(n_pairs=2, pair_left=idx(0, 0), pair_right=idx(1, 1), pair_ptr=ptr(0, 1, 0))),
        ("view_idx NULL", dict(view_idx=None)),
        ("train_idx NULL", dict(train_idx=None))])
def _find_2d3d():
    return dict(device=0, n_views=2, view_done=a([1, 0], U8), n_pt=1, view_ptr=ptr(0, 1), view_idx=idx(0), feat_idx=idx(0), n_pairs=1,
                pair_left=idx(0), pair_right=idx(1), pair_ptr=ptr(0, 1), query_idx=idx(0), train_idx=idx(0), out_ptr=out(I64, 3),
                out_point=out(I32, 4), out_feature=out(I32, 4), cap=4, total=out(I64, 1))


@entry("sfmba_merge_candidates", "device:i n_exist:i exist_xyz:p n_new:i new_xyz:p max_dist:f cand_ptr:p cand_idx:p cap:q total:p",
       "cand_ptr cand_idx total",
       [("n_new < 0", dict(n_new=-1)), ("exist_xyz NULL", dict(exist_xyz=None)), ("cand_idx NULL with cap > 0", dict(cand_idx=None))])
def _merge_candidates():
    return dict(device=0, n_exist=1, exist_xyz=a([0, 0, 1], F32), n_new=1, new_xyz=a([0, 0, 1.001], F32), max_dist=0.01,
                cand_ptr=out(I64, 2), cand_idx=out(I32, 4), cap=4, total=out(I64, 1))


# ---- matching ---------------------------------------------------------------------------------------------------------------------
ROWS_22 = 2 ** 22 - 1
DESC_ROW_CASES = [
    ("cap < 0", dict(cap=-1)),
    ("pair_ptr NULL", dict(pair_ptr=None)),
    ("ratio 0", dict(ratio=0.0)),
    ("ratio NaN", dict(ratio=NAN)),
    ("img_ptr[0] != 0", dict(img_ptr=ptr(1, 3, 5))),
    ("img_ptr not monotone", dict(img_ptr=ptr(0, 2, 1))),
    ("an image with 2^22 rows, through img_ptr alone", dict(img_ptr=ptr(0, 2, 2 + 2 ** 22), desc=DUMMY)),
    ("desc NULL", dict(desc=None)),
    ("pair_right out of range", dict(pair_right=idx(2))),
    ("513 pairs of 2^22 - 1 query rows each, through img_ptr and the pair list alone",
     dict(img_ptr=ptr(0, ROWS_22, 2 * ROWS_22), desc=DUMMY, n_pairs=513, pair_left=a([0] * 513, I32), pair_right=a([1] * 513, I32),
          pair_ptr=out(I64, 514))),
]


def _match(desc):
    return dict(device=0, n_images=2, img_ptr=ptr(0, 2, 4), desc=desc, n_pairs=1, pair_left=idx(0), pair_right=idx(1),
                ratio=float(np.float32(0.8)), pair_ptr=out(I64, 2), query_idx=out(I32, 4), train_idx=out(I32, 4), distance=out(F32, 4), cap=4,
                total=out(I64, 1))


MATCH_SIG = ("device:i n_images:i img_ptr:p desc:p %s:i n_pairs:i pair_left:p pair_right:p ratio:d pair_ptr:p query_idx:p train_idx:p "
             "distance:p cap:q total:p")
MATCH_OUT = "pair_ptr query_idx train_idx distance total"


@entry("sfmba_match_features", MATCH_SIG % "desc_bytes", MATCH_OUT,
       DESC_ROW_CASES + [("desc_bytes 0", dict(desc_bytes=0)), ("desc_bytes 65", dict(desc_bytes=65))])
def _match_features():
    return dict(desc_bytes=32, **_match(np.random.default_rng(3).integers(0, 256, size=4 * 32, dtype=np.uint8)))


def _l2_desc(bad=None):
    d = np.random.default_rng(4).random(4 * 8).astype(F32)
    if bad is not None:
        d[3 * 8 + 5] = bad
    return d


@entry("sfmba_match_features_l2", MATCH_SIG % "dims", MATCH_OUT,
       DESC_ROW_CASES + [("dims 0", dict(dims=0)), ("dims 513", dict(dims=513)),
                         ("a NaN in image 1, row 1", dict(desc=_l2_desc(NAN))), ("an infinity in image 1, row 1", dict(desc=_l2_desc(np.inf)))])
def _match_features_l2():
    return dict(dims=8, **_match(_l2_desc()))


# ---- feature extraction -----------------------------------------------------------------------------------------------------------
@entry("sfmba_orb_extract",
       "device:i n_images:i img_ptr:p pixels:p width:p height:p channels:i n_features:i scale_factor:f n_levels:i fast_threshold:i kp_ptr:p "
       "kp:p desc:p cap:q total:p dbg_level_xy:p dbg_bin:p dbg_harris:p dbg_candidates:p",
       "kp_ptr kp desc total",
       image_cases() + [
           ("kp NULL with cap > 0", dict(kp=None)),
           ("n_features 0", dict(n_features=0)),
           ("n_levels 0", dict(n_levels=0)),
           ("n_levels 13", dict(n_levels=13)),
           ("scale_factor 1", dict(scale_factor=1.0)),
           ("scale_factor 2.5", dict(scale_factor=2.5)),
           ("scale_factor NaN", dict(scale_factor=NAN)),
           ("fast_threshold 0", dict(fast_threshold=0)),
           ("fast_threshold 255", dict(fast_threshold=255)),
       ])
def _orb_extract():
    return dict(device=0, n_features=8, scale_factor=1.2, n_levels=2, fast_threshold=20, kp_ptr=out(I64, 2), kp=out(U8, 8 * 24),
                desc=out(U8, 8 * 32), cap=8, total=out(I64, 1), dbg_level_xy=None, dbg_bin=None, dbg_harris=None, dbg_candidates=None, **_images())


@entry("sfmba_surf_extract",
       "device:i n_images:i img_ptr:p pixels:p width:p height:p channels:i n_features:i n_octaves:i hessian_threshold:f upright:i kp_ptr:p "
       "kp:p desc:p cap:q total:p dbg_bin:p dbg_moments:p dbg_sums:p dbg_candidates:p",
       "kp_ptr kp desc total",
       image_cases() + [
           ("desc NULL with cap > 0", dict(desc=None)),
           ("n_features 0", dict(n_features=0)),
           ("n_octaves 0", dict(n_octaves=0)),
           ("n_octaves 5", dict(n_octaves=5)),
           ("hessian_threshold negative", dict(hessian_threshold=-1.0)),
           ("hessian_threshold infinite", dict(hessian_threshold=float("inf"))),
           ("upright 2", dict(upright=2)),
       ])
def _surf_extract():
    return dict(device=0, n_features=8, n_octaves=1, hessian_threshold=2.0, upright=0, kp_ptr=out(I64, 2), kp=out(U8, 8 * 32),
                desc=out(F32, 8 * 64), cap=8, total=out(I64, 1), dbg_bin=None, dbg_moments=None, dbg_sums=None, dbg_candidates=None, **_images())


# ---- dense depth ------------------------------------------------------------------------------------------------------------------
def _two_cameras():
    return dict(K=a([60, 0, 24, 0, 60, 20, 0, 0, 1], F32), P=a(np.concatenate([P_EYE, a([1, 0, 0, -0.2, 0, 1, 0, 0, 0, 0, 1, 0], F32)]), F32))


def _p_with(value, image=1):
    p = _two_cameras()["P"].copy()
    p[12 * image + 7] = value
    return p


def _k_with(slot, value):
    k = _two_cameras()["K"].copy()
    k[slot] = value
    return k


CAMERA_CASES = [
    ("K NULL", dict(K=None)),
    ("P NULL", dict(P=None)),
    ("width 0 in image 1", dict(width=idx(48, 0))),
    ("height 16385 in image 0", dict(height=idx(16385, 40), img_ptr=ptr(0, 48 * 16385, 48 * 16385 + 1920))),
    ("a NaN in the pose of image 1", dict(P=_p_with(NAN))),
    ("an infinity in the pose of image 0", dict(P=_p_with(np.inf, 0))),
    ("cx NaN", dict(K=_k_with(2, NAN))),
    ("fy infinite", dict(K=_k_with(4, np.inf))),
    ("fx 0", dict(K=_k_with(0, 0.0))),
    ("fy negative", dict(K=_k_with(4, -60.0))),
]
DEPTH_IMAGE_CASES = [
    ("img_ptr NULL", dict(img_ptr=None)),
    ("pixels NULL", dict(pixels=None)),
    ("channels 4", dict(channels=4)),
    ("img_ptr[0] != 0", dict(img_ptr=ptr(1, 1921, 3841))),
    ("img_ptr one byte long in image 1", dict(img_ptr=ptr(0, 1920, 3841))),
]


@entry("sfmba_depth_sweep",
       "device:i n_images:i img_ptr:p pixels:p width:p height:p channels:i K:p P:p n_jobs:i job_ref:p job_src_ptr:p job_src:p z_near:p z_far:p "
       "n_planes:i radius:i min_std:i min_score:f min_sources:i depth:p score:p plane:p",
       "depth score plane",
       DEPTH_IMAGE_CASES + CAMERA_CASES + [
           ("n_jobs < 0", dict(n_jobs=-1)),
           ("z_far NULL", dict(z_far=None)),
           ("n_planes 1", dict(n_planes=1)),
           ("n_planes 257", dict(n_planes=257)),
           ("radius 0", dict(radius=0)),
           ("radius 5", dict(radius=5)),
           ("min_std 128", dict(min_std=128)),
           ("min_score 1.5", dict(min_score=1.5)),
           ("min_score NaN", dict(min_score=NAN)),
           ("min_sources 0", dict(min_sources=0)),
           ("min_sources 5", dict(min_sources=5)),
           ("job_ref out of range", dict(job_ref=idx(2))),
           ("z_near 0", dict(z_near=a([0], F32))),
           ("z_near above z_far", dict(z_near=a([9], F32))),
           ("z_far infinite", dict(z_far=a([np.inf], F32))),
           ("job_src_ptr[0] != 0", dict(job_src_ptr=ptr(1, 2))),
           ("job_src_ptr NULL", dict(job_src_ptr=None)),
           ("a job without a source", dict(job_src_ptr=ptr(0, 0))),
           ("a job with five sources", dict(job_src_ptr=ptr(0, 5), job_src=idx(1, 1, 1, 1, 1))),
           ("a source index out of range", dict(job_src=idx(2))),
           ("a source that is the reference", dict(job_src=idx(0))),
           ("a source listed twice", dict(job_src_ptr=ptr(0, 2), job_src=idx(1, 1))),
           ("depth NULL", dict(depth=None)),
       ])
def _depth_sweep():
    return dict(device=0, n_jobs=1, job_ref=idx(0), job_src_ptr=ptr(0, 1), job_src=idx(1), z_near=a([2], F32), z_far=a([6], F32), n_planes=4,
                radius=1, min_std=2, min_score=0.6, min_sources=1, depth=out(F32, 48 * 40), score=out(F32, 48 * 40), plane=out(np.int16, 48 * 40),
                **_images(2), **_two_cameras())


def _depth_maps():
    return [np.full(48 * 40, 4.0, F32), np.full(48 * 40, 4.0, F32)]


def _too_many_pixels(args):
    big = _big_images(args)
    return dict(pixels=DUMMY, depth=[DUMMY] * 8, chk_ptr=a([0] * 9, I64), pt_ptr=out(I64, 9), **big)


@entry("sfmba_depth_fuse",
       "device:i n_images:i img_ptr:p pixels:p width:p height:p channels:i K:p P:p depth:P chk_ptr:p chk:p rel_tol:f min_consistent:i pt_ptr:p "
       "xyz:p bgr:p src_image:p src_pixel:p cap:q total:p",
       "pt_ptr xyz bgr src_image src_pixel total",
       DEPTH_IMAGE_CASES + CAMERA_CASES + [
           ("cap < 0", dict(cap=-1)),
           ("depth NULL", dict(depth=None)),
           ("xyz NULL with cap > 0", dict(xyz=None)),
           ("rel_tol negative", dict(rel_tol=-0.5)),
           ("rel_tol NaN", dict(rel_tol=NAN)),
           ("min_consistent 5", dict(min_consistent=5)),
           ("chk_ptr NULL", dict(chk_ptr=None)),
           ("chk_ptr[0] != 0", dict(chk_ptr=ptr(1, 2, 3))),
           ("chk_ptr not monotone", dict(chk_ptr=ptr(0, 1, 0))),
           ("chk NULL", dict(chk=None)),
           ("a check image out of range", dict(chk=idx(1, 7))),
           ("a check image that is its own", dict(chk=idx(0, 0))),
           ("a check image listed twice", dict(chk_ptr=ptr(0, 2, 2), chk=idx(1, 1))),
           ("8 images of 16384 x 16384 with a depth map: 2^31 pixels, through the pointer arrays alone", _too_many_pixels),
       ])
def _depth_fuse():
    n = 2 * 48 * 40
    return dict(device=0, depth=_depth_maps(), chk_ptr=ptr(0, 1, 2), chk=idx(1, 0), rel_tol=0.01, min_consistent=1, pt_ptr=out(I64, 3),
                xyz=out(F32, 3 * n), bgr=out(U8, 3 * n), src_image=out(I32, n), src_pixel=out(I32, n), cap=n, total=out(I64, 1),
                **_images(2), **_two_cameras())


def _normals_too_many_pixels(args):
    big = _big_images(args)
    del big["img_ptr"]
    return dict(depth=[DUMMY] * 8, normal=[DUMMY] * 8, **big)


@entry("sfmba_depth_normals", "device:i n_images:i width:p height:p K:p P:p depth:P max_rel_step:f normal:P", "normal",
       CAMERA_CASES + [
           ("n_images < 0", dict(n_images=-1)),
           ("normal NULL", dict(normal=None)),
           ("max_rel_step negative", dict(max_rel_step=-0.1)),
           ("max_rel_step NaN", dict(max_rel_step=NAN)),
           ("a depth map without an output map", lambda args: dict(normal=[args["normal"][0], None])),
           ("8 images of 16384 x 16384 with a depth map: 2^31 pixels, through the size arrays alone", _normals_too_many_pixels),
       ])
def _depth_normals():
    return dict(device=0, n_images=2, width=idx(48, 48), height=idx(40, 40), depth=_depth_maps(), max_rel_step=0.05,
                normal=[out(F32, 3 * 48 * 40), out(F32, 3 * 48 * 40)], **_two_cameras())


@entry("sfmba_cloud_merge",
       "device:i n:q xyz:p bgr:p normal:p voxel:f min_count:i xyz_out:p bgr_out:p normal_out:p count:p first:p voxel_of:p cap:q total:p "
       "n_skipped:p",
       "xyz_out bgr_out normal_out count first voxel_of total n_skipped",
       [("n < 0", dict(n=-1)),
        ("xyz NULL", dict(xyz=None)),
        ("n_skipped NULL", dict(n_skipped=None)),
        ("bgr without bgr_out", dict(bgr_out=None)),
        ("2^31 - 1 points, through n alone", dict(n=INT_MAX, xyz=DUMMY, bgr=None, normal=None)),
        ("voxel 0", dict(voxel=0.0)),
        ("voxel infinite", dict(voxel=float("inf"))),
        ("min_count 0", dict(min_count=0))])
def _cloud_merge():
    xyz = a([[0.1, 0.1, 0.1], [0.2, 0.1, 0.1], [1.5, 0.2, 0.3], [-0.4, 2.2, 0.9]], F32)
    return dict(device=0, n=4, xyz=xyz, bgr=a(np.arange(12), U8), normal=a([[0, 0, 1]] * 4, F32), voxel=1.0, min_count=1, xyz_out=out(F32, 12),
                bgr_out=out(U8, 12), normal_out=out(F32, 12), count=out(I32, 4), first=out(I32, 4), voxel_of=out(I32, 4), cap=4,
                total=out(I64, 1), n_skipped=out(I64, 1))


# ---- optical flow -----------------------------------------------------------------------------------------------------------------
FLOW_PAIR_CASES = [
    ("pt_ptr NULL", dict(pt_ptr=None)),
    ("pair_dst NULL", dict(pair_dst=None)),
    ("pt_ptr[0] != 0", dict(pt_ptr=ptr(1, 3))),
    ("pair_dst out of range", dict(pair_dst=idx(2))),
    ("pt_ptr not monotone", dict(pt_ptr=ptr(0, -1))),
    ("2^31 points, through pt_ptr alone", dict(pt_ptr=ptr(0, 2 ** 31))),
]


@entry("sfmba_flow_track",
       "device:i n_images:i img_ptr:p pixels:p width:p height:p channels:i n_pairs:i pair_src:p pair_dst:p pt_ptr:p pts:p n_levels:i radius:i "
       "max_iters:i min_eig:f next:p status:p err:p dbg_G:p dbg_state:p dbg_pyramid:p",
       "next status err",
       image_cases(n=2) + FLOW_PAIR_CASES + [
           ("pair_src NULL", dict(pair_src=None)),
           ("pair_src out of range", dict(pair_src=idx(-1))),
           ("n_levels 0", dict(n_levels=0)),
           ("n_levels 9", dict(n_levels=9)),
           ("radius 0", dict(radius=0)),
           ("radius 11", dict(radius=11)),
           ("max_iters 0", dict(max_iters=0)),
           ("max_iters 65", dict(max_iters=65)),
           ("min_eig negative", dict(min_eig=-1.0)),
           ("min_eig NaN", dict(min_eig=NAN)),
           ("pts NULL", dict(pts=None)),
           ("status NULL", dict(status=None)),
           ("an infinite coordinate in point 1", dict(pts=a([10, 10, np.inf, 20], F32))),
       ])
def _flow_track():
    return dict(device=0, n_pairs=1, pair_src=idx(0), pair_dst=idx(1), pt_ptr=ptr(0, 2), pts=a([10, 10, 30, 20], F32), n_levels=2, radius=2,
                max_iters=4, min_eig=0.5, next=out(F32, 4), status=out(U8, 2), err=out(F32, 2), dbg_G=None, dbg_state=None, dbg_pyramid=None,
                **_images(2))


@entry("sfmba_flow_match",
       "device:i n_images:i kp_ptr:p kp_xy:p n_pairs:i pair_dst:p pt_ptr:p next:p status:p err:p max_err:f radius:f ratio:d pair_ptr:p "
       "query_idx:p train_idx:p distance:p cap:q total:p",
       "pair_ptr query_idx train_idx distance total",
       FLOW_PAIR_CASES + [
           ("cap < 0", dict(cap=-1)),
           ("kp_ptr NULL", dict(kp_ptr=None)),
           ("n_images < 0", dict(n_images=-1)),
           ("max_err NaN", dict(max_err=NAN)),
           ("radius 0", dict(radius=0.0)),
           ("radius infinite", dict(radius=float("inf"))),
           ("ratio 0", dict(ratio=0.0)),
           ("ratio NaN", dict(ratio=NAN)),
           ("kp_ptr[0] != 0", dict(kp_ptr=ptr(1, 3, 5))),
           ("kp_ptr not monotone", dict(kp_ptr=ptr(0, 2, 1))),
           ("an image with 2^22 key points, through kp_ptr alone", dict(kp_ptr=ptr(0, 2, 2 + 2 ** 22), kp_xy=DUMMY)),
           ("status NULL", dict(status=None)),
           ("kp_xy NULL", dict(kp_xy=None)),
       ])
def _flow_match():
    return dict(device=0, n_images=2, kp_ptr=ptr(0, 2, 4), kp_xy=a([10, 10, 30, 20, 11, 10, 31, 21], F32), n_pairs=1, pair_dst=idx(1),
                pt_ptr=ptr(0, 2), next=a([11, 10, 31, 21], F32), status=a([1, 1], U8), err=a([1, 1], F32), max_err=12.0, radius=2.0, ratio=0.7,
                pair_ptr=out(I64, 2), query_idx=out(I32, 4), train_idx=out(I32, 4), distance=out(F32, 4), cap=4, total=out(I64, 1))


# ---- RANSAC -----------------------------------------------------------------------------------------------------------------------
@entry("sfmba_pnp_ransac",
       "device:i n_prob:i prob_ptr:p xyz:p uv:p K:p n_hyp:i threshold_px:f seed:Q max_refine_iters:i pose:p inlier:p result:p hyp_pose:p "
       "hyp_count:p",
       "pose inlier result",
       RANSAC_CASES + FOCAL_CASES + [
           ("n_prob < 0", dict(n_prob=-1)),
           ("pose NULL", dict(pose=None)),
           ("max_refine_iters < 0", dict(max_refine_iters=-1)),
           ("prob_ptr[0] < 0", dict(prob_ptr=ptr(-1, 5))),
           ("prob_ptr not monotone", dict(prob_ptr=ptr(6, 0))),
           ("a problem with 2^31 - 1 points, through prob_ptr alone", dict(prob_ptr=ptr(0, INT_MAX))),
           ("uv NULL", dict(uv=None)),
           ("inlier NULL", dict(inlier=None)),
       ])
def _pnp_ransac():
    xyz = a([[0, 0, 4], [1, 0, 5], [0, 1, 6], [1, 1, 4], [-1, 0.5, 5], [0.5, -1, 6]], F32)
    uv = a(np.stack([100 * xyz[:, 0] / xyz[:, 2] + 16, 100 * xyz[:, 1] / xyz[:, 2] + 16], axis=1), F32)
    return dict(device=0, n_prob=1, prob_ptr=ptr(0, 6), xyz=xyz, uv=uv, K=K33, n_hyp=8, threshold_px=2.0, seed=1, max_refine_iters=2,
                pose=out(F64, 12), inlier=out(U8, 6), result=out(U8, 24), hyp_pose=None, hyp_count=None)


@entry("sfmba_homography_ransac",
       "device:i n_images:i img_ptr:p pts:p n_pairs:i pair_left:p pair_right:p pair_ptr:p query_idx:p train_idx:p n_hyp:i threshold_px:f seed:Q "
       "H:p inlier:p result:p hyp_H:p hyp_count:p",
       "H inlier result",
       MATCH_LIST_CASES + RANSAC_CASES + [("H NULL", dict(H=None)), ("inlier NULL", dict(inlier=None))])
def _homography_ransac():
    return dict(device=0, n_hyp=8, threshold_px=2.0, seed=1, H=out(F64, 9), inlier=out(U8, 4), result=out(U8, 16), hyp_H=None, hyp_count=None,
                **_match_list())


# the match-list cases above are written for 4 points per image; the essential call needs 6
def _essential_cases(cases):
    swap = {"a query_idx past its image": dict(query_idx=idx(0, 1, 2, 3, 4, 6)), "a train_idx negative": dict(train_idx=idx(0, -1, 2, 3, 4, 5)),
            "img_ptr[0] < 0": dict(img_ptr=ptr(-1, 6, 12)), "img_ptr not monotone": dict(img_ptr=ptr(0, 12, 6)),
            "pair_ptr not monotone": dict(pair_ptr=ptr(6, 0)),
            "pair_ptr[0] < 0": dict(pair_ptr=ptr(-1, 5))}
    return [(d, swap.get(d, o)) for d, o in cases]


@entry("sfmba_essential_ransac",
       "device:i n_images:i img_ptr:p pts:p n_pairs:i pair_left:p pair_right:p pair_ptr:p query_idx:p train_idx:p K:p n_hyp:i threshold_px:f "
       "seed:Q E:p pose:p inlier:p result:p hyp_E:p hyp_count:p hyp_nsol:p",
       "E pose inlier result",
       _essential_cases(MATCH_LIST_CASES) + RANSAC_CASES + FOCAL_CASES +
       [("K NULL", dict(K=None)), ("pose NULL", dict(pose=None)), ("inlier NULL", dict(inlier=None))])
def _essential_ransac():
    m = _match_list()
    rng = np.random.default_rng(2)
    X = np.concatenate([rng.uniform(-1, 1, (6, 2)), rng.uniform(4, 6, (6, 1))], axis=1)
    left = 100 * X[:, :2] / X[:, 2:] + 16
    Xr = X + np.array([-0.5, 0.05, 0.1])
    right = 100 * Xr[:, :2] / Xr[:, 2:] + 16
    m.update(img_ptr=ptr(0, 6, 12), pts=a(np.concatenate([left, right]), F32), pair_ptr=ptr(0, 6), query_idx=a(np.arange(6), I32),
             train_idx=a(np.arange(6), I32))
    return dict(device=0, K=K33, n_hyp=8, threshold_px=1.0, seed=1, E=out(F64, 9), pose=out(F64, 12), inlier=out(U8, 6), result=out(U8, 24),
                hyp_E=None, hyp_count=None, hyp_nsol=None, **m)


# ---- image files ------------------------------------------------------------------------------------------------------------------
def _smallest(cases):
    files = [cases.small_file(n) for n in cases.decodable_names()]
    return np.frombuffer(min(files, key=len), dtype=U8).copy()


def _jpeg_bytes():
    import jpeg_cases
    return _smallest(jpeg_cases)


def _png_bytes():
    import png_cases
    return _smallest(png_cases)


FILE_CASES = [
    ("n_images < 0", dict(n_images=-1)),
    ("file_ptr NULL", dict(file_ptr=None)),
    ("file_ptr[0] < 0", dict(file_ptr=ptr(-1, 10))),
    ("file_ptr not monotone", dict(file_ptr=ptr(10, 0))),
    ("bytes NULL", dict(bytes=None)),
]
DECODE_CASES = FILE_CASES + [
    ("cap < 0", dict(cap=-1)),
    ("info NULL", dict(info=None)),
    ("out NULL with cap > 0", dict(out=None)),
    ("factor 0", dict(factor=0.0)),
    ("factor NaN", dict(factor=NAN)),
]
MAX_DECODED = 64 * 64 * 3          # every file under tests/golden/*_small decodes to fewer bytes


def _file(data):
    return dict(n_images=1, file_ptr=ptr(0, len(data)), bytes=data)


@entry("sfmba_jpeg_info", "n_images:i file_ptr:p bytes:p info:p", "info", FILE_CASES + [("info NULL", dict(info=None))])
def _jpeg_info():
    return dict(info=out(I32, 7), **_file(_jpeg_bytes()))


@entry("sfmba_resized_size", "width:i height:i factor:f out_width:p out_height:p", "out_width out_height",
       [("out_width NULL", dict(out_width=None)),
        ("factor 0", dict(factor=0.0)),
        ("factor NaN", dict(factor=NAN)),
        ("width 0", dict(width=0)),
        ("height 16385", dict(height=16385)),
        ("a factor that gives a side of 0", dict(factor=0.001)),
        ("a factor that gives a side above 16384", dict(width=16384, factor=1.5))])
def _resized_size():
    return dict(width=48, height=40, factor=0.5, out_width=out(I32, 1), out_height=out(I32, 1))


@entry("sfmba_jpeg_decode", "device:i n_images:i file_ptr:p bytes:p factor:f info:p out_ptr:p out:p cap:q total:p", "info out_ptr out total",
       DECODE_CASES)
def _jpeg_decode():
    return dict(device=0, factor=1.0, info=out(I32, 7), out_ptr=out(I64, 2), out=out(U8, MAX_DECODED), cap=MAX_DECODED, total=out(I64, 1),
                **_file(_jpeg_bytes()))


@entry("sfmba_resize_images", "device:i n_images:i img_ptr:p px:p width:p height:p channels:i factor:f out_ptr:p out:p cap:q total:p",
       "out_ptr out total",
       image_cases("px") + [
           ("cap < 0", dict(cap=-1)),
           ("out NULL with cap > 0", dict(out=None)),
           ("factor 0", dict(factor=0.0)),
           ("factor infinite", dict(factor=float("inf"))),
           ("a factor that gives a side of 0", dict(factor=0.001)),
       ])
def _resize_images():
    im = _images()
    im["px"] = im.pop("pixels")
    return dict(device=0, factor=0.5, out_ptr=out(I64, 2), out=out(U8, 48 * 40), cap=48 * 40, total=out(I64, 1), **im)


@entry("sfmba_png_info", "n_images:i file_ptr:p bytes:p info:p", "info", FILE_CASES + [("info NULL", dict(info=None))])
def _png_info():
    return dict(info=out(I32, 7), **_file(_png_bytes()))


@entry("sfmba_png_decode", "device:i n_images:i file_ptr:p bytes:p factor:f info:p out_ptr:p out:p cap:q total:p", "info out_ptr out total",
       DECODE_CASES)
def _png_decode():
    return dict(device=0, factor=1.0, info=out(I32, 7), out_ptr=out(I64, 2), out=out(U8, MAX_DECODED), cap=MAX_DECODED, total=out(I64, 1),
                **_file(_png_bytes()))


BY_NAME = {e.name: e for e in ENTRIES}


# ---- refusals for the arguments that a unit finds only after the device is open: they need a GPU --------------------------------
def _many_pairs(args, n=16385):
    """16385 empty pairs x 65536 hypotheses: more score threads than one grid dimension holds"""
    return dict(n_pairs=n, pair_left=a([0] * n, I32), pair_right=a([1] * n, I32), pair_ptr=a([0] * (n + 1), I64), n_hyp=65536,
                result=out(U8, n * len(args["result"])), **{k: out(F64, n * len(args[k])) for k in ("H", "E", "pose") if k in args})


def _many_problems(args, n=16385):
    return dict(n_prob=n, prob_ptr=a([0] * (n + 1), I64), n_hyp=65536, pose=out(F64, 12 * n), result=out(U8, 24 * n))


def _many_views(args, n=46341):
    """46341 views, one of them done: the [left][right] pair table would have 2^31 entries"""
    return dict(n_views=n, view_done=a([1] + [0] * (n - 1), U8), out_ptr=out(I64, n + 1))


DEVICE_CASES = [
    ("sfmba_find_2d3d_matches", "46341 views: a pair table of 2^31 entries", _many_views),
    ("sfmba_merge_candidates", "2^26 - 1 existing points, through n_exist alone", dict(n_exist=2 ** 26 - 1, exist_xyz=DUMMY)),
    ("sfmba_pnp_ransac", "16385 empty problems x 65536 hypotheses", _many_problems),
    ("sfmba_homography_ransac", "16385 empty pairs x 65536 hypotheses", _many_pairs),
    ("sfmba_essential_ransac", "16385 empty pairs x 65536 hypotheses", _many_pairs),
    ("sfmba_jpeg_decode", "a factor that gives a side of 0", dict(factor=0.001)),
    ("sfmba_png_decode", "a factor that gives a side of 0", dict(factor=0.001)),
]
# entry points that never touch the device: their valid call is SFMBA_OK with or without a GPU
HOST_ONLY = ("sfmba_jpeg_info", "sfmba_resized_size", "sfmba_png_info")
