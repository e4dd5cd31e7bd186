"""The control flow of sfmtoylib::SfM::runSfM (host/SfM.h) restated in Python over the shim harness's PER-STAGE drivers -- TEST
INFRASTRUCTURE ONLY.  restated_loop() follows the same seeds and the same order as the class: the single-pair
sfmba_shim_find_camera_matrices for the baseline, ONE sfmba_shim_find_camera_matrices_batch per added view, then
sfmba_shim_triangulate_views pair by pair, sfmba_shim_merge pair by pair and sfmba_shim_adjust_bundle.  It calls neither
sfmba_shim_run_sfm nor the batched triangulation; run_class() is the one call of sfmba_shim_run_sfm it is compared with.

Both return the same dict: code (0 = OKAY, 1 = ERROR), poses [v,12] f32, K [9] f32, done / good [v] bool, added_view / added_posed /
added_cloud (one entry per turn of the add-more-views loop), xyz [n,3] f32, view_ptr / view_idx / feat_idx (the cloud's views CSR).

As a program (a fresh process per run, which the tests start with SFMBA_DETERMINISTIC=1 and SFMBA_SHIM_CACHE=0):
    python tests/sfm_loop.py class|loop [--ply PREFIX] INPUT.npz OUTPUT.npz [INPUT.npz OUTPUT.npz ...]
INPUT.npz holds either kp_ptr / kp_xy / desc / cols / rows (features) or images [v,h,w] (gray) / [v,h,w,3] (B, G, R) uint8 (pixels), and optionally downscale.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "sfm-toy-library_amd", "host", "libsfmba_shim.so")
POSE_INLIERS_MINIMAL_RATIO = np.float32(0.5)
lp, ip, fp, bp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(SHIM)
        _lib.sfmba_shim_find_2d3d.restype = C.c_int64
        _lib.sfmba_shim_feature_match_matrix.restype = C.c_int64
        _lib.sfmba_shim_extract_features_batch.restype = C.c_int64
    return _lib


def _a(x, dtype):
    return np.ascontiguousarray(x, dtype=dtype)


def _p(x, t):
    return x.ctypes.data_as(t)


def features_input(views, cols, rows):
    """views: list of dict(xy [m,2], desc [m,32]) -> the arrays of an INPUT.npz."""
    ptr = np.zeros(len(views) + 1, np.int64)
    ptr[1:] = np.cumsum([len(v["xy"]) for v in views])
    xy = np.concatenate([v["xy"] for v in views]) if views else np.zeros((0, 2))
    desc = np.concatenate([v["desc"] for v in views]) if views else np.zeros((0, 32))
    return dict(kp_ptr=ptr, kp_xy=_a(xy, np.float32).reshape(-1, 2), desc=_a(desc, np.uint8).reshape(-1, 32), cols=cols, rows=rows)


# ---- the class: one call ---------------------------------------------------------------------------------------------------
def run_class(inp, ply_prefix=None, debug_level=4):
    images = inp.get("images")
    downscale = float(inp.get("downscale", 1.0))
    if images is not None:
        images = _a(images, np.uint8)
        n, h, w = images.shape[0], (images.shape[1] if images.ndim > 1 else 0), (images.shape[2] if images.ndim > 2 else 0)
        channels = 3 if images.ndim == 4 else 1                    # [v,h,w] gray or [v,h,w,3] B, G, R
        img_ptr = (np.arange(n + 1, dtype=np.int64) * h * w * channels)
        wd, ht = np.full(max(n, 1), w, np.int32), np.full(max(n, 1), h, np.int32)
        kp_ptr, kp_xy, desc, cols, rows = np.zeros(1, np.int64), np.zeros((1, 2), np.float32), np.zeros((1, 32), np.uint8), 0, 0
        cap_pts = 8 * 5000 * max(n, 1)
    else:
        kp_ptr, kp_xy, desc = _a(inp["kp_ptr"], np.int64), _a(inp["kp_xy"], np.float32), _a(inp["desc"], np.uint8)
        n, cols, rows = len(kp_ptr) - 1, int(inp["cols"]), int(inp["rows"])
        channels, img_ptr, images, wd, ht = 0, np.zeros(1, np.int64), np.zeros(1, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.int32)
        cap_pts = 8 * max(len(kp_xy), 1)
    m = max(n, 1)
    cap_views = cap_pts * m
    poses, K = np.zeros((m, 12), np.float32), np.zeros(9, np.float32)
    done, good = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    n_added, n_pts = C.c_int(0), C.c_int64(0)
    av, ap, ac = np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros(m, np.int64)
    xyz, view_ptr = np.zeros((cap_pts, 3), np.float32), np.zeros(cap_pts + 1, np.int64)
    vi, fi = np.zeros(cap_views, np.int32), np.zeros(cap_views, np.int32)
    code = lib().sfmba_shim_run_sfm(C.c_float(downscale), C.c_int(n), C.c_int(channels), _p(img_ptr, lp), _p(images, bp), _p(wd, ip), _p(ht, ip),
                                    _p(kp_ptr, lp), _p(kp_xy, fp), _p(desc, bp), C.c_int(cols), C.c_int(rows), C.c_int(debug_level), _p(poses, fp),
                                    _p(K, fp), _p(done, bp), _p(good, bp), C.byref(n_added), _p(av, ip), _p(ap, bp), _p(ac, lp),
                                    C.c_int64(cap_pts), C.c_int64(cap_views), C.byref(n_pts), _p(xyz, fp), _p(view_ptr, lp), _p(vi, ip), _p(fi, ip),
                                    ply_prefix.encode() if ply_prefix else None)
    assert code in (0, 1), "sfmba_shim_run_sfm returned %d" % code
    na, npt = n_added.value, n_pts.value
    nv = int(view_ptr[npt])
    return dict(code=code, poses=poses[:n], K=K, done=done[:n].astype(bool), good=good[:n].astype(bool), added_view=av[:na], added_posed=ap[:na].astype(bool),
                added_cloud=ac[:na], xyz=xyz[:npt], view_ptr=view_ptr[:npt + 1], view_idx=vi[:nv], feat_idx=fi[:nv])


# ---- the per-stage drivers ------------------------------------------------------------------------------------------------
def extract_features(images):
    images = _a(images, np.uint8)
    n, h, w = images.shape[:3]
    channels = 3 if images.ndim == 4 else 1
    img_ptr = np.arange(n + 1, dtype=np.int64) * h * w * channels
    wd, ht = np.full(n, w, np.int32), np.full(n, h, np.int32)
    cap = 5000 * n
    kp_ptr, kp = np.zeros(n + 1, np.int64), np.zeros((cap, 7), np.float32)
    pts, desc = np.zeros((cap, 2), np.float32), np.zeros((cap, 32), np.uint8)
    tot = lib().sfmba_shim_extract_features_batch(C.c_int(n), _p(img_ptr, lp), _p(images, bp), _p(wd, ip), _p(ht, ip), C.c_int(channels), _p(kp_ptr, lp),
                                                  C.c_int64(cap), _p(kp, fp), _p(pts, fp), _p(desc, bp))
    if tot < 0:
        return None
    return dict(kp_ptr=kp_ptr, kp_xy=_a(kp[:tot, :2], np.float32), desc=desc[:tot].copy(), cols=w, rows=h)


def match_matrix(kp_ptr, desc):
    """{(l, r): [q, t, dist]} for l < r, or None on failure."""
    n = len(kp_ptr) - 1
    cap = int(kp_ptr[-1]) * max(n, 1)
    sizes = np.zeros(n * n, np.int64)
    q, t, im, d = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32)
    tot = lib().sfmba_shim_feature_match_matrix(C.c_int(n), _p(kp_ptr, lp), _p(desc, bp), C.c_int(32), _p(sizes, lp), C.c_int64(cap), _p(q, ip),
                                                _p(t, ip), _p(im, ip), _p(d, fp))
    if tot < 0:
        return None
    assert tot <= cap
    mm, at = {}, 0
    for l in range(n):
        for r in range(n):
            s = int(sizes[l * n + r])
            if l < r:
                mm[(l, r)] = [q[at:at + s].copy(), t[at:at + s].copy(), d[at:at + s].copy()]
            else:
                assert s == 0
            at += s
    return mm


def flat_matrix(mm):
    keys = sorted(mm)
    ptr = np.zeros(len(keys) + 1, np.int64)
    ptr[1:] = np.cumsum([len(mm[k][0]) for k in keys])
    cat = lambda j, dt: _a(np.concatenate([mm[k][j] for k in keys]) if keys else np.zeros(0), dt)
    left, right = _a([k[0] for k in keys], np.int32), _a([k[1] for k in keys], np.int32)
    return left, right, ptr, cat(0, np.int32), cat(1, np.int32), cat(2, np.float32)


def sort_views_for_baseline(kp_ptr, kp_xy, mm):
    n = len(kp_ptr) - 1
    left, right, ptr, q, t, _ = flat_matrix(mm)
    cap = max(len(left), 1)
    keys, pairs = np.zeros(cap, np.float32), np.zeros((cap, 2), np.int32)
    m = lib().sfmba_shim_sort_views_for_baseline(C.c_int(n), _p(kp_ptr, lp), _p(kp_xy, fp), C.c_int(len(left)), _p(left, ip), _p(right, ip), _p(ptr, lp),
                                                 _p(q, ip), _p(t, ip), C.c_int(cap), _p(keys, fp), _p(pairs, ip))
    return [(float(keys[i]), int(pairs[i, 0]), int(pairs[i, 1])) for i in range(m)]


def _keep_distances(entry, pruned):
    """The pruned (query, train) rows are a sub-list of the entry, in order: the entry's rows of those matches (distances kept)."""
    q, t, d = entry
    where = {(int(a), int(b)): i for i, (a, b) in reversed(list(enumerate(zip(q, t))))}
    idx = np.array([where[(int(a), int(b))] for a, b in pruned], dtype=np.int64)
    assert np.all(np.diff(idx) > 0)
    return [q[idx].copy(), t[idx].copy(), d[idx].copy()] if len(idx) else [np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)]


def find_camera_matrices(K, kp_ptr, kp_xy, l, r, entry):
    a, b, c, d = int(kp_ptr[l]), int(kp_ptr[l + 1]), int(kp_ptr[r]), int(kp_ptr[r + 1])
    img_ptr = np.array([0, b - a, b - a + d - c], np.int64)
    xy = _a(np.concatenate([kp_xy[a:b], kp_xy[c:d]]), np.float32)
    q, t = _a(entry[0], np.int32), _a(entry[1], np.int32)
    Pl, Pr = np.zeros(12, np.float32), np.zeros(12, np.float32)
    Pl[[0, 5, 10]] = 1; Pr[[0, 5, 10]] = 1
    pruned = np.zeros((max(len(q), 1), 2), np.int32)
    n_pruned = C.c_int(0)
    ok = lib().sfmba_shim_find_camera_matrices(_p(K, fp), _p(img_ptr, lp), _p(xy, fp), C.c_int(len(q)), _p(q, ip), _p(t, ip), _p(Pl, fp), _p(Pr, fp),
                                               _p(pruned, ip), C.byref(n_pruned))
    return bool(ok), Pl, Pr, pruned[:n_pruned.value]


def find_camera_matrices_batch(K, kp_ptr, kp_xy, lefts, rights, entries):
    n_pairs = len(lefts)
    ptr = np.zeros(n_pairs + 1, np.int64)
    ptr[1:] = np.cumsum([len(e[0]) for e in entries])
    q = _a(np.concatenate([e[0] for e in entries]), np.int32)
    t = _a(np.concatenate([e[1] for e in entries]), np.int32)
    left, right = _a(lefts, np.int32), _a(rights, np.int32)
    ok = np.zeros(n_pairs, np.uint8)
    Pl, Pr = np.zeros((n_pairs, 12), np.float32), np.zeros((n_pairs, 12), np.float32)
    pruned_ptr, pruned = np.zeros(n_pairs + 1, np.int64), np.zeros((max(len(q), 1), 2), np.int32)
    lib().sfmba_shim_find_camera_matrices_batch(_p(K, fp), C.c_int(len(kp_ptr) - 1), _p(kp_ptr, lp), _p(kp_xy, fp), C.c_int(n_pairs), _p(left, ip),
                                                _p(right, ip), _p(ptr, lp), _p(q, ip), _p(t, ip), _p(ok, bp), _p(Pl, fp), _p(Pr, fp),
                                                _p(pruned_ptr, lp), _p(pruned, ip))
    return ok.astype(bool), [pruned[pruned_ptr[p]:pruned_ptr[p + 1]] for p in range(n_pairs)]


def triangulate_views(K, kp_ptr, kp_xy, l, r, entry, Pl, Pr):
    """(ok, xyz [m,3], left_ref [m], right_ref [m])."""
    a, b, c, d = int(kp_ptr[l]), int(kp_ptr[l + 1]), int(kp_ptr[r]), int(kp_ptr[r + 1])
    xl, xr = _a(kp_xy[a:b], np.float32), _a(kp_xy[c:d], np.float32)
    q, t = _a(entry[0], np.int32), _a(entry[1], np.int32)
    cap = max(len(q), 1)
    X, lr, rr = np.zeros((cap, 3), np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    Pl, Pr = _a(Pl, np.float32), _a(Pr, np.float32)
    n = lib().sfmba_shim_triangulate_views(_p(K, fp), C.c_int(l), C.c_int(r), C.c_int(b - a), _p(xl, fp), C.c_int(d - c), _p(xr, fp), C.c_int(len(q)),
                                           _p(q, ip), _p(t, ip), _p(Pl, fp), _p(Pr, fp), C.c_int(cap), _p(X, fp), _p(lr, ip), _p(rr, ip))
    if n < 0:
        return False, None, None, None
    return True, X[:n].copy(), lr[:n].copy(), rr[:n].copy()


class Cloud:
    """xyz [n,3] f32 and the views CSR (ascending view per point)."""

    def __init__(self, xyz=None, view_ptr=None, view_idx=None, feat_idx=None):
        self.xyz = np.zeros((0, 3), np.float32) if xyz is None else _a(xyz, np.float32).reshape(-1, 3)
        self.view_ptr = np.zeros(1, np.int64) if view_ptr is None else _a(view_ptr, np.int64)
        self.view_idx = np.zeros(0, np.int32) if view_idx is None else _a(view_idx, np.int32)
        self.feat_idx = np.zeros(0, np.int32) if feat_idx is None else _a(feat_idx, np.int32)

    @staticmethod
    def from_pair(l, r, xyz, lref, rref):
        n = len(xyz)
        vi = np.tile(np.array([l, r], np.int32), n)
        fi = np.stack([lref, rref], axis=1).reshape(-1).astype(np.int32) if n else np.zeros(0, np.int32)
        return Cloud(xyz, 2 * np.arange(n + 1, dtype=np.int64), vi, fi)

    def __len__(self):
        return len(self.xyz)


def _pad(a):
    return a if len(a) else np.zeros(1, a.dtype)


def find_2d3d_counts(n_views, done, cloud, mm, kp_ptr, kp_xy):
    """(counts per view (0 for done views), out_ptr, out_2d, out_3d), or None on a device error."""
    left, right, ptr, q, t, _ = flat_matrix(mm)
    cap = max(len(cloud), 1) * n_views
    out_ptr, o2, o3 = np.zeros(n_views + 1, np.int64), np.zeros((cap, 2), np.float32), np.zeros((cap, 3), np.float32)
    d8 = _a(done, np.uint8)
    tot = lib().sfmba_shim_find_2d3d(C.c_int(n_views), _p(d8, bp), C.c_int(len(cloud)), _p(_pad(cloud.xyz.reshape(-1)), fp), _p(cloud.view_ptr, lp),
                                     _p(_pad(cloud.view_idx), ip), _p(_pad(cloud.feat_idx), ip), C.c_int(len(left)), _p(left, ip), _p(right, ip),
                                     _p(ptr, lp), _p(_pad(q), ip), _p(_pad(t), ip), _p(kp_ptr, lp), _p(kp_xy, fp), _p(out_ptr, lp), _p(o2, fp),
                                     _p(o3, fp), C.c_int64(cap))
    if tot < 0:
        return None
    return np.diff(out_ptr), out_ptr, o2, o3


def find_camera_pose(K, uv, xyz):
    uv, xyz = _a(uv, np.float32), _a(xyz, np.float32)
    pose = np.zeros(12, np.float32)
    ok = lib().sfmba_shim_find_camera_pose(_p(K, fp), C.c_int(len(uv)), _p(_pad(xyz.reshape(-1)), fp), _p(_pad(uv.reshape(-1)), fp), _p(pose, fp))
    return bool(ok), pose


def merge(n_views, recon, fresh, mm):
    left, right, ptr, q, t, d = flat_matrix(mm)
    cap_pts = len(recon) + len(fresh) + 1
    cap_views = len(recon.view_idx) + len(fresh.view_idx) + 2 * len(fresh) + 1
    out_n = C.c_int(0)
    xyz, vp = np.zeros((cap_pts, 3), np.float32), np.zeros(cap_pts + 1, np.int64)
    vi, fi = np.zeros(cap_views, np.int32), np.zeros(cap_views, np.int32)
    counts, n_merge = np.zeros(2, np.int64), C.c_int64(0)
    mp = np.zeros((1, 4), np.int32)
    rc = lib().sfmba_shim_merge(C.c_int(n_views), C.c_int(len(recon)), _p(_pad(recon.xyz.reshape(-1)), fp), _p(recon.view_ptr, lp), _p(_pad(recon.view_idx), ip),
                                _p(_pad(recon.feat_idx), ip), C.c_int(len(fresh)), _p(_pad(fresh.xyz.reshape(-1)), fp), _p(fresh.view_ptr, lp),
                                _p(_pad(fresh.view_idx), ip), _p(_pad(fresh.feat_idx), ip), C.c_int(len(left)), _p(left, ip), _p(right, ip), _p(ptr, lp),
                                _p(_pad(q), ip), _p(_pad(t), ip), _p(_pad(d), fp), C.c_int(cap_pts), C.c_int64(cap_views), C.byref(out_n), _p(xyz, fp),
                                _p(vp, lp), _p(vi, ip), _p(fi, ip), _p(counts, lp), C.c_int64(1), _p(mp, ip), C.byref(n_merge))
    assert rc in (0, -1), "sfmba_shim_merge: capacity"
    if rc == -1:
        return recon
    n = out_n.value
    return Cloud(xyz[:n], vp[:n + 1], vi[:vp[n]], fi[:vp[n]])


def adjust_bundle(poses, K, cloud, kp_ptr, kp_xy):
    """In place on poses [v,12], K [9] and cloud.xyz."""
    xyz = _a(cloud.xyz, np.float32)
    lib().sfmba_shim_adjust_bundle(C.c_int(len(poses)), _p(poses, fp), _p(K, fp), C.c_int(len(cloud)), _p(_pad(xyz.reshape(-1)), fp), _p(cloud.view_ptr, lp),
                                   _p(_pad(cloud.view_idx), ip), _p(_pad(cloud.feat_idx), ip), _p(kp_ptr, lp), _p(kp_xy, fp))
    cloud.xyz = xyz


# ---- the loop ---------------------------------------------------------------------------------------------------------------
def restated_loop(inp):
    downscale = float(inp.get("downscale", 1.0))
    images = inp.get("images")
    n = len(images) if images is not None else len(inp["kp_ptr"]) - 1
    err = dict(code=1)
    if n <= 0 or downscale != 1.0:
        return err
    if images is not None:
        feats = extract_features(images)
        if feats is None:
            return err
    else:
        feats = inp
    kp_ptr, kp_xy, desc = _a(feats["kp_ptr"], np.int64), _a(feats["kp_xy"], np.float32), _a(feats["desc"], np.uint8)
    cols, rows = int(feats["cols"]), int(feats["rows"])
    K = np.array([2500, 0, cols // 2, 0, 2500, rows // 2, 0, 0, 1], np.float32)
    poses = np.zeros((n, 12), np.float32)
    done, good = np.zeros(n, bool), np.zeros(n, bool)
    mm = match_matrix(kp_ptr, desc)
    if mm is None:
        return err

    # baseline: the ranked pairs in key order, the single-pair pose call (seed 0), the first pair that works
    cloud = None
    for _, i, j in sort_views_for_baseline(kp_ptr, kp_xy, mm):
        ok, Pl, Pr, pruned = find_camera_matrices(K, kp_ptr, kp_xy, i, j, mm[(i, j)])
        if not ok:
            continue
        if np.float32(len(pruned)) / np.float32(len(mm[(i, j)][0])) < POSE_INLIERS_MINIMAL_RATIO:
            continue
        mm[(i, j)] = _keep_distances(mm[(i, j)], pruned)
        ok, X, lref, rref = triangulate_views(K, kp_ptr, kp_xy, i, j, mm[(i, j)], Pl, Pr)
        if not ok:
            continue
        cloud = Cloud.from_pair(i, j, X, lref, rref)
        poses[i], poses[j] = Pl, Pr
        done[[i, j]] = True
        good[[i, j]] = True
        adjust_bundle(poses, K, cloud, kp_ptr, kp_xy)
        break
    if cloud is None:
        return err

    added_view, added_posed, added_cloud = [], [], []
    while not done.all():
        found = find_2d3d_counts(n, done, cloud, mm, kp_ptr, kp_xy)
        best, best_n = -1, 0
        if found is not None:
            for v in range(n):
                if not done[v] and found[0][v] > best_n:
                    best, best_n = v, int(found[0][v])
        if best < 0:
            best = int(np.flatnonzero(~done)[0])
        done[best] = True
        if found is not None:
            a, b = int(found[1][best]), int(found[1][best + 1])
            posed, pose = find_camera_pose(K, found[2][a:b], found[3][a:b])
        else:
            posed, pose = find_camera_pose(K, np.zeros((0, 2)), np.zeros((0, 3)))
        if not posed:
            added_view.append(best); added_posed.append(False); added_cloud.append(len(cloud))
            continue
        poses[best] = pose
        goods = [int(g) for g in np.flatnonzero(good)]
        lefts, rights = [min(g, best) for g in goods], [max(g, best) for g in goods]
        _, pruned = find_camera_matrices_batch(K, kp_ptr, kp_xy, lefts, rights, [mm[(l, r)] for l, r in zip(lefts, rights)])
        for l, r, pr in zip(lefts, rights, pruned):
            mm[(l, r)] = _keep_distances(mm[(l, r)], pr)
        any_ok = False
        for l, r in zip(lefts, rights):                              # pair by pair: what the class does in one batched call
            ok, X, lref, rref = triangulate_views(K, kp_ptr, kp_xy, l, r, mm[(l, r)], poses[l], poses[r])
            if ok:
                cloud = merge(n, cloud, Cloud.from_pair(l, r, X, lref, rref), mm)
                any_ok = True
        added_view.append(best); added_posed.append(True); added_cloud.append(len(cloud))
        if any_ok:
            adjust_bundle(poses, K, cloud, kp_ptr, kp_xy)
        good[best] = True
    return dict(code=0, poses=poses, K=K, done=done, good=good, added_view=np.array(added_view, np.int32), added_posed=np.array(added_posed, bool),
                added_cloud=np.array(added_cloud, np.int64), xyz=cloud.xyz, view_ptr=cloud.view_ptr, view_idx=cloud.view_idx, feat_idx=cloud.feat_idx)


def main(argv):
    """MODE then IN OUT pairs; --ply PREFIX (class mode) makes the FIRST run write its PLY files there."""
    args = list(argv[1:])
    ply = None
    if "--ply" in args:
        at = args.index("--ply")
        ply = args[at + 1]
        del args[at:at + 2]
    mode, rest = args[0], args[1:]
    for k in range(0, len(rest), 2):
        inp = dict(np.load(rest[k]))
        out = run_class(inp, ply_prefix=ply if k == 0 else None) if mode == "class" else restated_loop(inp)
        np.savez(rest[k + 1], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
