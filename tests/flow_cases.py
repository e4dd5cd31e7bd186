"""The inputs of the optical-flow tests (tests/test_flow_oracle_cpu.py, tests/test_gpu_flow_track.py) and their restated results,
computed once per process (tests/flow_oracle.py) and shared.  TEST INFRASTRUCTURE ONLY.

A texture is the sum of Gaussian-filtered noise at sigma = 1.5, 4 and 10, weighted by sigma and scaled to 0..255: it has content at
every pyramid scale (single-scale fine noise leaves the coarse levels without signal and about a fifth of the points diverge).  The
second view of a pair is the first one shifted through a cubic warp."""
import ctypes as C
import functools

import numpy as np
from scipy import ndimage

import flow_oracle as fo


@functools.lru_cache(maxsize=None)
def _field(w, h, seed):
    rng = np.random.default_rng(seed)
    acc = np.zeros((h, w))
    for sigma in (1.5, 4.0, 10.0):
        acc += sigma * ndimage.gaussian_filter(rng.normal(size=(h, w)), sigma, mode="wrap")
    return acc


def texture_pair(w, h, shift=(0.0, 0.0), seed=0, margin=40):
    """(first, second) uint8 h x w: a point at p of the first view lies at p + shift in the second."""
    f = _field(w + 2 * margin, h + 2 * margin, seed)
    lo, hi = f.min(), f.max()
    moved = ndimage.shift(f, (shift[1], shift[0]), order=3, mode="wrap")
    to8 = lambda a: np.clip(np.rint((a - lo) / (hi - lo) * 255.0), 0, 255).astype(np.uint8)[margin:margin + h, margin:margin + w]
    return to8(f), to8(moved)


def texture(w, h, seed=0):
    return texture_pair(w, h, seed=seed)[0]


def inner_points(w, h, n, border, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(border, w - 1 - border, n), rng.uniform(border, h - 1 - border, n)], axis=1).astype(np.float32)


def floor_scene(shift):
    """The 200 x 160 scene of the contract's floors: 60 points at least 25 px from the border."""
    a, b = texture_pair(200, 160, shift, seed=7)
    return [a, b], inner_points(200, 160, 60, 25, seed=8)


def bgr_of(img, seed=5):
    """A BGR image whose gray reduction is `img` exactly where b = g = r; elsewhere a true colour image."""
    rng = np.random.default_rng(seed)
    out = np.repeat(img[:, :, None], 3, axis=2).astype(np.int64)
    out = np.clip(out + rng.integers(-20, 21, size=out.shape), 0, 255)
    return out.astype(np.uint8)


def eig_ramp():
    """I = 2 |x - 20| + y on 40 x 30: at (20, 15) with r = 4 and L = 1, gx sums to 0 over the window, so Gxy = 0 exactly,
    Gyy = 81 * 32^2 < Gxx = 9 * 8 * 64^2 and lam = Gyy = (1.0 * 81) * 1024 exactly: min_eig = 1 lies ON the point's value."""
    ys, xs = np.mgrid[0:30, 0:40]
    return (2 * np.abs(xs - 20) + ys).astype(np.uint8)


def _tracked(w, h, shift, n, seed, border=0, **params):
    a, b = texture_pair(w, h, shift, seed=seed)
    return dict(images=[a, b], pairs=[(0, 1)], points=[inner_points(w, h, n, border, seed + 100)], params=params)


def _case_edges():
    a, b = texture_pair(40, 30, (1.25, -0.75), seed=3)
    pts = [(0, 0), (39, 0), (0, 29), (39, 29), (-5.5, 3), (45.25, 12), (7, -9), (11, 36.5), (-0.03125, -0.03125), (39.03125, 29.03125),
           (1e6, -1e6), (3e38, 3e38), (-3e38, 5), (20, 15)]
    return dict(images=[a, b], pairs=[(0, 1)], points=[np.asarray(pts, np.float32)], params=dict(n_levels=3, radius=4, max_iters=10, min_eig=0.0))


def _case_leaves():
    a = texture(48, 40, seed=4)
    return dict(images=[a, np.ascontiguousarray(a[:24, :30])], pairs=[(0, 1), (1, 0)],
                points=[np.asarray([(40, 30), (10, 10), (29, 23), (31, 12)], np.float32), np.asarray([(10, 10), (29, 23)], np.float32)],
                params=dict(n_levels=2, radius=4, max_iters=8, min_eig=0.5))


def _case_counts():
    imgs = [texture(33, 17, seed=20), texture_pair(33, 17, (0.8, 0.4), seed=20)[1], texture(45, 70, seed=21)]
    pairs = [(0, 1), (1, 0), (0, 1), (2, 2), (0, 2)]
    pts = [inner_points(33, 17, n, 0, 30 + n) for n in (0, 1, 63)] + [inner_points(45, 70, 64, 0, 40), inner_points(33, 17, 65, 0, 41)]
    return dict(images=imgs, pairs=pairs, points=pts, params=dict(n_levels=2, radius=2, max_iters=6, min_eig=0.25))


def _case_eig(min_eig):
    img = eig_ramp()
    return dict(images=[img, img], pairs=[(0, 1)], points=[np.asarray([(20, 15)], np.float32)],
                params=dict(n_levels=1, radius=4, max_iters=3, min_eig=min_eig))


def _small(w, h, L, r, pts):
    rng = np.random.default_rng(w * 100 + h)
    a, b = (rng.integers(0, 256, size=(h, w)).astype(np.uint8) for _ in range(2))
    return dict(images=[a, b], pairs=[(0, 1)], points=[np.asarray(pts, np.float32)], params=dict(n_levels=L, radius=r, max_iters=5, min_eig=0.0))


def _case_bgr():
    c = _tracked(37, 23, (1.5, 0.5), 12, seed=9, n_levels=2, radius=3, max_iters=10, min_eig=0.5)
    c["images"] = [bgr_of(im, seed=5 + k) for k, im in enumerate(c["images"])]
    return c


TRACK_CASES = {
    "size_1x1": lambda: _small(1, 1, 1, 1, [(0, 0), (0.5, -0.5)]),
    "size_1x7": lambda: _small(1, 7, 2, 1, [(0, 3), (0, 0), (0, 6.5)]),
    "size_2x2": lambda: _small(2, 2, 2, 1, [(0, 0), (1, 1), (0.5, 0.5)]),
    "levels_8_on_5x3": lambda: _small(5, 3, 8, 1, [(2, 1), (0, 0), (4, 2), (3.25, 1.5)]),
    "size_33x17_r1_l1": lambda: _tracked(33, 17, (0.4, -0.3), 20, seed=1, n_levels=1, radius=1, max_iters=20, min_eig=0.0),
    "size_33x17_r4_l3": lambda: _tracked(33, 17, (2.3, -1.6), 20, seed=1, n_levels=3, radius=4, max_iters=20, min_eig=1.0),
    "size_70x45_r10_l4": lambda: _tracked(70, 45, (5.5, 3.25), 16, seed=2, n_levels=4, radius=10, max_iters=20, min_eig=1.0),
    "size_64x48_r7_defaults": lambda: _tracked(64, 48, (3.3, -2.6), 16, seed=6, border=8, **fo.DEFAULTS),
    "edges": _case_edges,
    "leaves_dst": _case_leaves,
    "constant_src": lambda: dict(images=[np.full((20, 24), 77, np.uint8), texture(24, 20, seed=5)], pairs=[(0, 1), (1, 0)],
                                 points=[inner_points(24, 20, 5, 0, 1)] * 2, params=dict(n_levels=2, radius=3, max_iters=4, min_eig=0.0)),
    "min_eig_on": lambda: _case_eig(1.0),
    "min_eig_above": lambda: _case_eig(float(np.nextafter(np.float32(1.0), np.float32(2.0)))),
    "max_iters_1": lambda: _tracked(48, 36, (2.0, 1.0), 12, seed=11, n_levels=3, radius=5, max_iters=1, min_eig=0.5),
    "max_iters_64": lambda: _tracked(40, 28, (1.3, 0.6), 6, seed=12, n_levels=1, radius=3, max_iters=64, min_eig=0.0),
    "src_is_dst": lambda: dict(images=[texture(40, 30, seed=13)], pairs=[(0, 0)], points=[inner_points(40, 30, 10, 0, 2)],
                               params=dict(n_levels=3, radius=4, max_iters=10, min_eig=0.5)),
    "bgr": _case_bgr,
    "counts": _case_counts,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return TRACK_CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(per pair (next, status, err, G, state), per image its levels) of a case -- shared, treat as read-only."""
    c = case(name)
    return fo.track_vec(c["images"], c["pairs"], c["points"], **c["params"])


# ---- matcher -------------------------------------------------------------------------------------------------------------------
def _m(kps, pairs, queries, **params):
    """queries: per pair a list of (x, y, status, err)."""
    tracked = []
    for rows in queries:
        a = np.asarray(rows, np.float64).reshape(-1, 4)
        tracked.append((a[:, :2].astype(np.float32), a[:, 2].astype(np.uint8), a[:, 3].astype(np.float32)))
    return dict(keypoints=[np.asarray(k, np.float32).reshape(-1, 2) for k in kps], pairs=pairs, tracked=tracked, params=dict(fo.MATCH_DEFAULTS, **params))


def _case_tile(n_kp, seed):
    rng = np.random.default_rng(seed)
    kp = rng.uniform(0, 120, size=(n_kp, 2)).astype(np.float32)
    kp[-1] = kp[0] + np.float32(0.5)                                     # the last key point of the last stage decides a ratio test
    pick = rng.integers(0, n_kp, size=300)
    q = kp[pick] + rng.normal(scale=0.6, size=(300, 2)).astype(np.float32)
    q[0], q[1] = kp[-1], kp[0]
    rows = np.concatenate([q, (rng.uniform(size=(300, 1)) < 0.9), rng.uniform(0, 14, size=(300, 1))], axis=1)
    return _m([np.zeros((0, 2)), kp], [(0, 1)], [rows])


MATCH_CASES = {
    # s = 4 = radius^2 exactly is in range; one ulp further is not
    "on_radius": lambda: _m([[], [(10, 10)]], [(0, 1)], [[(12, 10, 1, 0), (float(np.nextafter(np.float32(12), np.float32(13))), 10, 1, 0), (10, 8, 1, 0)]]),
    "one_two_three_in_range": lambda: _m([[], [(10, 10), (11.5, 10), (10, 11.75), (50, 50), (50.5, 50), (80, 80)]], [(0, 1)],
                                         [[(10.1, 10.1, 1, 0), (50.1, 50, 1, 0), (80.5, 80.5, 1, 0), (30, 30, 1, 0), (50.25, 50, 1, 0)]]),
    # equal s: dropped at ratio 0.7 (1 < 0.7 fails); at ratio 1.5 the lower j is the best
    "tie_dropped": lambda: _m([[], [(10, 11), (10, 9)]], [(0, 1)], [[(10, 10, 1, 0)]]),
    "tie_lower_j": lambda: _m([[], [(10, 11), (10, 9), (11, 10)]], [(0, 1)], [[(10, 10, 1, 0)]], ratio=1.5),
    "coincident": lambda: _m([[], [(10, 10), (10, 10), (30, 30)]], [(0, 1)], [[(10, 10, 1, 0), (30.5, 30, 1, 0)]], ratio=5.0),
    "three_on_one": lambda: _m([[], [(10, 10), (40, 40)]], [(0, 1)], [[(40.1, 40, 1, 0), (10.5, 10, 1, 0), (10.1, 10, 1, 0), (10, 10, 1, 0), (40, 40, 1, 0)]]),
    "err_on_max": lambda: _m([[], [(10, 10), (20, 20), (30, 30)]], [(0, 1)],
                             [[(10, 10, 1, 12.0), (20, 20, 1, float(np.nextafter(np.float32(12), np.float32(0)))), (30, 30, 1, 12.5)]]),
    "status_0": lambda: _m([[], [(10, 10), (20, 20)]], [(0, 1)], [[(10, 10, 0, 0), (20, 20, 1, 0), (20, 20, 2, 0)]]),
    "empty_train": lambda: _m([[(1, 1)], []], [(0, 1), (1, 0)], [[(1, 1, 1, 0)], [(1, 1, 1, 0), (1.5, 1, 1, 0)]]),
    "empty_queries": lambda: _m([[(1, 1)], [(2, 2)]], [(0, 1), (1, 0), (0, 0)], [[], [(1, 1, 1, 0)], []]),
    "several_pairs": lambda: _m([[(5, 5), (9, 9)], [(5.5, 5), (9, 9.5), (70, 70)], [(5, 5.5)]], [(0, 1), (1, 2), (0, 2), (2, 1), (0, 1)],
                                [[(5.4, 5, 1, 1), (9, 9.4, 1, 2)], [(5, 5.4, 1, 0), (70, 70, 1, 0)], [(5, 5, 1, 0), (5, 5.6, 1, 0)],
                                 [(70.5, 70.5, 1, 3)], [(9, 9, 0, 0), (9, 9.6, 1, 11.9)]]),
    "kp_255": lambda: _case_tile(255, 1),
    "kp_256": lambda: _case_tile(256, 2),
    "kp_257": lambda: _case_tile(257, 3),
    "kp_600": lambda: _case_tile(600, 4),
}


@functools.lru_cache(maxsize=None)
def match_case(name):
    return MATCH_CASES[name]()


@functools.lru_cache(maxsize=None)
def match_oracle(name):
    c = match_case(name)
    return fo.match_vec(c["keypoints"], c["pairs"], c["tracked"], **c["params"])


# ---- the two calls with the arrays as given (refusals, the capacity protocol) ---------------------------------------------------
def raw_track(capi, images, pair_src, pair_dst, pt_ptr, pts, n_levels=2, radius=2, max_iters=4, min_eig=0.5, channels=None, img_ptr=None):
    """sfmba_flow_track with the arrays as given: (rc, next, status, err), the outputs prefilled with a pattern."""
    imgs, ch, iptr, flat, wd, ht = capi._flat_images(images)
    iptr = iptr if img_ptr is None else np.asarray(img_ptr, np.int64)
    ps, pd, pp = (np.asarray(list(a) or [0], t) for a, t in ((pair_src, np.int32), (pair_dst, np.int32), (pt_ptr, np.int64)))
    pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 2))
    n = max(len(pts), 1)
    nxt, status, err = np.full((n, 2), 7.0, np.float32), np.full(n, 9, np.uint8), np.full(n, 7.0, np.float32)
    lp, bp, fp, ip = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rc = capi.lib().sfmba_flow_track(C.c_int(0), C.c_int(len(imgs)), iptr.ctypes.data_as(lp), flat.ctypes.data_as(bp), wd.ctypes.data_as(ip),
                                     ht.ctypes.data_as(ip), C.c_int(ch if channels is None else channels), C.c_int(len(pair_src)),
                                     ps.ctypes.data_as(ip), pd.ctypes.data_as(ip), pp.ctypes.data_as(lp),
                                     (pts if len(pts) else np.zeros((1, 2), np.float32)).ctypes.data_as(fp), C.c_int(n_levels), C.c_int(radius),
                                     C.c_int(max_iters), C.c_float(min_eig), nxt.ctypes.data_as(fp), status.ctypes.data_as(bp),
                                     err.ctypes.data_as(fp), None, None, None)
    return rc, nxt, status, err


def raw_match(capi, kp_ptr, kp, pair_dst, pt_ptr, nxt, status, err, max_err=12.0, radius=2.0, ratio=0.7, cap=8):
    """sfmba_flow_match with the arrays as given: (rc, pair_ptr, query_idx, train_idx, distance, total), prefilled with a pattern."""
    kp_ptr, pp, pd = np.asarray(kp_ptr, np.int64), np.asarray(pt_ptr, np.int64), np.asarray(list(pair_dst) or [0], np.int32)
    kp = np.ascontiguousarray(np.asarray(list(kp) or [(0, 0)], np.float32).reshape(-1, 2))
    nxt = np.ascontiguousarray(np.asarray(list(nxt) or [(0, 0)], np.float32).reshape(-1, 2))
    status, err = np.asarray(list(status) or [0], np.uint8), np.asarray(list(err) or [0], np.float32)
    ptr = np.full(len(pair_dst) + 1, -7, np.int64)
    q, t, d = np.full(max(cap, 1), -7, np.int32), np.full(max(cap, 1), -7, np.int32), np.full(max(cap, 1), -7.0, np.float32)
    total = C.c_int64(-7)
    lp, bp, fp, ip = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rc = capi.lib().sfmba_flow_match(C.c_int(0), C.c_int(len(kp_ptr) - 1), kp_ptr.ctypes.data_as(lp), kp.ctypes.data_as(fp), C.c_int(len(pair_dst)),
                                     pd.ctypes.data_as(ip), pp.ctypes.data_as(lp), nxt.ctypes.data_as(fp), status.ctypes.data_as(bp),
                                     err.ctypes.data_as(fp), C.c_float(max_err), C.c_float(radius), C.c_double(ratio), ptr.ctypes.data_as(lp),
                                     q.ctypes.data_as(ip), t.ctypes.data_as(ip), d.ctypes.data_as(fp), C.c_int64(cap), C.byref(total))
    return rc, ptr, q, t, d, total.value
