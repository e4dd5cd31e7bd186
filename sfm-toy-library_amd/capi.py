"""ctypes binding of the C ABI in include/sfmba.h (libsfmba_hip.so, built from csrc/).

This is the only way Python code (tests, bench.py, the sharded driver) reaches the product: through
the same extern "C" entry points the C++ shim in host/ calls.  If the shared library has not been
built, or no HIP device is present, calls fail loudly -- there is no CPU fallback.
"""
import ctypes as C
import os
import numpy as np

from .structs import SfmbaOptions, SfmbaSummary, SfmbaIteration

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsfmba_hip.so")
if os.environ.get("SFMBA_LIB"):          # development aid: A/B a library built from another commit (tools/ab/) through the same binding
    LIB_PATH = os.path.abspath(os.environ["SFMBA_LIB"])
_lib = None

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)

# every extern "C" symbol include/sfmba.h declares (tests check the library exports all of them)
SYMBOLS = [
    "sfmba_options_default", "sfmba_abi_version", "sfmba_last_error", "sfmba_device_count", "sfmba_solve",
    "sfmba_problem_create", "sfmba_problem_reset", "sfmba_problem_set_params", "sfmba_problem_solve",
    "sfmba_problem_get_params", "sfmba_problem_destroy", "sfmba_problem_stream", "sfmba_problem_reduced_dim",
    "sfmba_problem_eval_residuals", "sfmba_problem_eval_jacobian", "sfmba_problem_build_reduced",
    "sfmba_dense_spd_solve", "sfmba_dense_pcg_probe", "sfmba_dist_cg_probe", "sfmba_shard_begin", "sfmba_shard_reduce_len", "sfmba_shard_reduce_buf",
    "sfmba_shard_scalars_buf", "sfmba_shard_partial_build", "sfmba_shard_solve_update", "sfmba_shard_finish",
    "sfmba_shard_end", "sfmba_problem_set_profiling", "sfmba_problem_get_profile",
    "sfmba_problem_create_sharded", "sfmba_shard_setup_finish", "sfmba_shard_setup_len", "sfmba_shard_setup_buf", "sfmba_release_cache", "sfmba_triangulate",
    "sfmba_find_2d3d_matches", "sfmba_merge_candidates", "sfmba_problem_append",
    "sfmba_comm_unique_id", "sfmba_comm_create", "sfmba_comm_destroy", "sfmba_comm_allreduce", "sfmba_problem_solve_sharded",
    "sfmba_comm_allreduce_f32", "sfmba_problem_set_allreduce_f32", "sfmba_shard_last_exchange",
    "sfmba_problem_create_ex", "sfmba_comm_abort", "sfmba_comm_reduce_scatter", "sfmba_problem_set_reduce_scatter",
    "sfmba_comm_allgather", "sfmba_problem_set_allgather", "sfmba_comm_size", "sfmba_device_warmup",
    "sfmba_match_features", "sfmba_problem_set_step_probe", "sfmba_problem_get_step_probe", "sfmba_pnp_ransac",
    "sfmba_homography_ransac", "sfmba_essential_ransac", "sfmba_orb_extract", "sfmba_triangulate_pairs",
    "sfmba_jpeg_info", "sfmba_resized_size", "sfmba_jpeg_decode", "sfmba_resize_images",
    "sfmba_png_info", "sfmba_png_decode", "sfmba_match_features_l2", "sfmba_surf_extract",
    "sfmba_depth_sweep", "sfmba_depth_fuse", "sfmba_flow_track", "sfmba_flow_match",
    "sfmba_depth_normals", "sfmba_cloud_merge", "sfmba_tsdf_integrate", "sfmba_tsdf_extract", "sfmba_tsdf_mesh",
    "sfmba_tsdf_fill", "sfmba_tsdf_mesh_fill",
    "sfmba_mesh_components", "sfmba_mesh_filter", "sfmba_mesh_smooth", "sfmba_mesh_clean", "sfmba_mesh_decimate",
    "sfmba_mesh_texture_size", "sfmba_mesh_texture",
    "sfmba_mesh_view_candidates", "sfmba_mesh_adjacency", "sfmba_mesh_view_smooth", "sfmba_mesh_texture_from_views", "sfmba_mesh_texture_smooth",
    "sfmba_mesh_colour_nodes", "sfmba_mesh_colour_level", "sfmba_mesh_texture_levelled", "sfmba_mesh_texture_adjust",
    "sfmba_depth_cost_volume", "sfmba_sgm_aggregate", "sfmba_depth_sweep_sgm",
]

# reduced-system solver families of the step probe (SFMBA_FAMILY_* in include/sfmba.h), by value
FAMILIES = ("NONE", "CHOL_SMALL", "CHOL_FUSED", "CHOL_PANEL", "PCG_FAST", "PCG_SEGMENTS", "PCG_SYMMETRIC", "PCG_STREAMING",
            "PCG_SEGMENTS_STREAMING", "PCG_SEGMENTS_STREAMING_SPARSE", "DIST_BLOCKS", "DIST_ROWS", "IMPLICIT")


class _StepProbe(C.Structure):
    _fields_ = [("family", C.c_int), ("f32_matrix", C.c_int), ("coarse_vectors", C.c_int), ("cg_iters", C.c_int), ("cholesky_fallback", C.c_int)]


def get_step_probe(handle, dim, n_pt):
    """What the last back-substitution on `handle` consumed (include/sfmba.h, sfmba_problem_get_step_probe): (z [dim], dpt [n_pt][3], info dict)."""
    z, dpt, info = np.zeros(max(dim, 1)), np.zeros(3 * max(n_pt, 1)), _StepProbe()
    _check(lib().sfmba_problem_get_step_probe(handle, _p(z, _dp), _p(dpt, _dp), C.byref(info)))
    out = {k: int(getattr(info, k)) for k, _ in _StepProbe._fields_}
    out["family_name"] = FAMILIES[out["family"]] if 0 <= out["family"] < len(FAMILIES) else str(out["family"])
    return z[:dim], dpt[:3 * n_pt].reshape(n_pt, 3), out


def triangulate(K, P_left, P_right, left_xy, right_xy, max_reproj_px=10.0, device=0, reproj_err=True):
    """SfMStereoUtilities::triangulateViews for aligned matches on the GPU: (points3d [n,3] float32, keep [n] bool, err [n,2]).
    reproj_err=False passes NULL for the optional error output: err is then None."""
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    Pl = np.ascontiguousarray(P_left, dtype=np.float32).reshape(12)
    Pr = np.ascontiguousarray(P_right, dtype=np.float32).reshape(12)
    l = np.ascontiguousarray(left_xy, dtype=np.float32).reshape(-1, 2)
    r = np.ascontiguousarray(right_xy, dtype=np.float32).reshape(-1, 2)
    n = l.shape[0]
    X = np.zeros((n, 3), dtype=np.float32); keep = np.zeros(n, dtype=np.uint8)
    err = np.zeros((n, 2), dtype=np.float32) if reproj_err else None
    fp = C.POINTER(C.c_float)
    _check(lib().sfmba_triangulate(C.c_int(device), C.c_int64(n), l.ctypes.data_as(fp), r.ctypes.data_as(fp), K.ctypes.data_as(fp),
                                   Pl.ctypes.data_as(fp), Pr.ctypes.data_as(fp), C.c_float(max_reproj_px), X.ctypes.data_as(fp),
                                   keep.ctypes.data_as(C.POINTER(C.c_ubyte)), err.ctypes.data_as(fp) if reproj_err else None))
    return X, keep.astype(bool), err


def triangulate_pairs(pts_per_image, pairs, matches, K, P_left, P_right, mask=None, max_reproj_px=10.0, reproj_err=True, device=0):
    """sfmba_triangulate_pairs: triangulateViews for the match lists of many pairs in one call (the contract is in include/sfmba.h).

    pts_per_image, pairs, matches: as homography_ransac takes them.  K [3, 3]; P_left / P_right [n_pairs, 3, 4], one camera pair per
    pair.  mask: None or [total] (the concatenated `inlier` arrays of essential_ransac); total = pair_ptr[-1].  Returns a dict:
    points3d [total, 3] float32, keep [total] bool, err [total, 2] float32 (None with reproj_err=False), kept_ptr [n_pairs + 1]
    int64, kept_idx [kept_ptr[-1]] int64, pair_ptr (as given)."""
    ps = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 2) for x in pts_per_image]
    if len(matches) == 6:
        pl, pr, ptr, q, t = matches[:5]
    else:
        if pairs is None:
            pairs = [(i, j) for i in range(len(ps)) for j in range(i + 1, len(ps))]
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        pl, pr = pairs[:, 0], pairs[:, 1]
        ptr, q, t = matches
    pl, pr, q, t = _i(pl), _i(pr), _i(q), _i(t)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    n_pairs = len(pl)
    if len(pr) != n_pairs or len(ptr) != n_pairs + 1 or len(q) != len(t) or (n_pairs and len(q) < ptr[-1]):
        raise ValueError("pair_left / pair_right / pair_ptr / query_idx / train_idx do not fit together")
    total = int(ptr[-1])
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    Pl = np.ascontiguousarray(P_left, dtype=np.float32).reshape(-1)
    Pr = np.ascontiguousarray(P_right, dtype=np.float32).reshape(-1)
    if len(Pl) != 12 * n_pairs or len(Pr) != 12 * n_pairs:
        raise ValueError("P_left / P_right must hold one 3 x 4 matrix per pair")
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
        if len(mask) < total:
            raise ValueError("mask must hold one entry per match")
    img_ptr = np.zeros(len(ps) + 1, dtype=np.int64)
    img_ptr[1:] = np.cumsum([len(x) for x in ps])
    pts = np.ascontiguousarray(np.concatenate(ps, axis=0) if ps else np.zeros((0, 2), np.float32))
    X = np.zeros((max(total, 1), 3), dtype=np.float32)
    keep = np.zeros(max(total, 1), dtype=np.uint8)
    err = np.zeros((max(total, 1), 2), dtype=np.float32) if reproj_err else None
    kept_ptr = np.zeros(n_pairs + 1, dtype=np.int64)
    kept_idx = np.zeros(max(total, 1), dtype=np.int64)
    lp, fp, bp = C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    _check(lib().sfmba_triangulate_pairs(C.c_int(device), C.c_int(len(ps)), _p(img_ptr, lp), _p(pts, fp), _p(K, fp), C.c_int(n_pairs), _p(pl, _ip),
                                         _p(pr, _ip), _p(ptr, lp), _p(q, _ip), _p(t, _ip), _p(mask, bp) if mask is not None else None,
                                         _p(Pl, fp), _p(Pr, fp), C.c_float(max_reproj_px), _p(X, fp), _p(keep, bp),
                                         _p(err, fp) if reproj_err else None, _p(kept_ptr, lp), _p(kept_idx, lp)))
    return dict(points3d=X[:total], keep=keep[:total].astype(bool), err=err[:total] if reproj_err else None, kept_ptr=kept_ptr,
                kept_idx=kept_idx[:int(kept_ptr[-1])].copy(), pair_ptr=ptr)


SFMBA_ERR_CAPACITY = 5


def _flat_views(views):
    """list of {view: feature} per cloud point -> CSR arrays in ascending view order (std::map iteration order)."""
    ptr = np.zeros(len(views) + 1, dtype=np.int64)
    vi, fi = [], []
    for i, m in enumerate(views):
        for v in sorted(m):
            vi.append(v)
            fi.append(m[v])
        ptr[i + 1] = len(vi)
    return ptr, np.asarray(vi, dtype=np.int32), np.asarray(fi, dtype=np.int32)


def _flat_matches(match_matrix):
    """{(left, right): [(query, train, distance), ...]} -> flattened pair arrays (any key order, every key kept)."""
    left, right, ptr, q, t, d = [], [], [0], [], [], []
    for (l, r), lst in match_matrix.items():
        left.append(l)
        right.append(r)
        for m in lst:
            q.append(m[0]); t.append(m[1]); d.append(m[2] if len(m) > 2 else 0.0)
        ptr.append(len(q))
    return (np.asarray(left, np.int32), np.asarray(right, np.int32), np.asarray(ptr, np.int64), np.asarray(q, np.int32),
            np.asarray(t, np.int32), np.asarray(d, np.float32))


def find_2d3d_matches(n_views, done_views, view_ptr, view_idx, feat_idx, pair_left, pair_right, pair_ptr, query_idx, train_idx,
                      cap=None, device=0):
    """sfmba_find_2d3d_matches on flat arrays: (out_ptr [n_views+1], out_point, out_feature)."""
    done = np.zeros(n_views, dtype=np.uint8)
    done[np.asarray(list(done_views), dtype=np.int64)] = 1
    view_ptr = np.ascontiguousarray(view_ptr, np.int64); view_idx = _i(view_idx); feat_idx = _i(feat_idx)
    pair_left = _i(pair_left); pair_right = _i(pair_right); pair_ptr = np.ascontiguousarray(pair_ptr, np.int64)
    query_idx = _i(query_idx); train_idx = _i(train_idx)
    n_pt = len(view_ptr) - 1
    cap = int(n_pt if cap is None else cap)
    lp = C.POINTER(C.c_int64)
    out_ptr = np.zeros(n_views + 1, dtype=np.int64)
    total = C.c_int64(0)
    for _ in range(2):
        op, of = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
        rc = lib().sfmba_find_2d3d_matches(
            C.c_int(device), C.c_int(n_views), done.ctypes.data_as(C.POINTER(C.c_ubyte)), C.c_int(n_pt), _p(view_ptr, lp), _p(view_idx, _ip),
            _p(feat_idx, _ip), C.c_int(len(pair_left)), _p(pair_left, _ip), _p(pair_right, _ip), _p(pair_ptr, lp), _p(query_idx, _ip),
            _p(train_idx, _ip), _p(out_ptr, lp), _p(op, _ip), _p(of, _ip), C.c_int64(cap), C.byref(total))
        if rc != SFMBA_ERR_CAPACITY:
            break
        cap = int(total.value)
    _check(rc)
    return out_ptr, op[:total.value].copy(), of[:total.value].copy()


def merge_candidates(exist_xyz, new_xyz, max_dist=0.01, cap=None, device=0):
    """sfmba_merge_candidates: (cand_ptr [n_new+1], cand_idx) -- see include/sfmba.h."""
    ex = np.ascontiguousarray(exist_xyz, np.float32).reshape(-1, 3)
    nw = np.ascontiguousarray(new_xyz, np.float32).reshape(-1, 3)
    cap = int(4 * len(nw) + 1024 if cap is None else cap)
    lp, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    ptr = np.zeros(len(nw) + 1, dtype=np.int64)
    total = C.c_int64(0)
    for _ in range(2):
        idx = np.zeros(max(cap, 1), np.int32)
        rc = lib().sfmba_merge_candidates(C.c_int(device), C.c_int(len(ex)), _p(ex, fp), C.c_int(len(nw)), _p(nw, fp), C.c_float(max_dist),
                                          _p(ptr, lp), _p(idx, _ip), C.c_int64(cap), C.byref(total))
        if rc != SFMBA_ERR_CAPACITY:
            break
        cap = int(total.value)
    _check(rc)
    return ptr, idx[:total.value].copy()


def match_features(descs, pairs=None, ratio=float(np.float32(0.8)), cap=None, device=0):
    """sfmba_match_features: brute-force Hamming 2-NN + ratio test for every pair (see include/sfmba.h).

    descs: list of uint8 arrays [n_i, B] (one per image, the same B for all).  pairs: list of (left, right) image indices, None = all
    i < j in row-major order (SfM::createFeatureMatchMatrix).  ratio defaults to the reference's (double)0.8f.
    Returns (pair_left, pair_right, pair_ptr [n_pairs+1], query_idx, train_idx, distance float32)."""
    descs = [np.asarray(d, dtype=np.uint8) for d in descs]
    nb = {d.shape[1] for d in descs if d.ndim == 2}
    if any(d.ndim != 2 for d in descs) or len(nb) > 1:
        raise ValueError("descs must be 2-D uint8 arrays with one row length")
    B = nb.pop() if nb else 32
    if pairs is None:
        pairs = [(i, j) for i in range(len(descs)) for j in range(i + 1, len(descs))]
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    pl, pr = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    img_ptr = np.zeros(len(descs) + 1, dtype=np.int64)
    img_ptr[1:] = np.cumsum([d.shape[0] for d in descs])
    flat = np.ascontiguousarray(np.concatenate(descs, axis=0) if descs else np.zeros((0, B), np.uint8))
    if cap is None:                      # at most one entry per query row of a pair with >= 2 train rows: one call, no retry
        cap = int(sum(descs[l].shape[0] for l, r in zip(pl, pr) if 0 <= r < len(descs) and descs[r].shape[0] >= 2 and 0 <= l < len(descs)))
    lp, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    ptr = np.zeros(len(pl) + 1, dtype=np.int64)
    total = C.c_int64(0)
    for _ in range(2):
        q, t, d = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32)
        rc = lib().sfmba_match_features(C.c_int(device), C.c_int(len(descs)), _p(img_ptr, lp), flat.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                        C.c_int(B), C.c_int(len(pl)), _p(pl, _ip), _p(pr, _ip), C.c_double(ratio), _p(ptr, lp), _p(q, _ip),
                                        _p(t, _ip), _p(d, fp), C.c_int64(cap), C.byref(total))
        if rc != SFMBA_ERR_CAPACITY:
            break
        cap = int(total.value)
    _check(rc)
    n = total.value
    return pl, pr, ptr, q[:n].copy(), t[:n].copy(), d[:n].copy()


def match_features_l2(descs, pairs=None, ratio=float(np.float32(0.8)), cap=None, device=0):
    """sfmba_match_features_l2: brute-force exact L2 2-NN + ratio test over float descriptors (see include/sfmba.h).

    descs: list of float32 arrays [n_i, dims] (one per image, the same dims for all).  pairs, ratio and the return value are those of
    match_features: (pair_left, pair_right, pair_ptr [n_pairs+1], query_idx, train_idx, distance float32)."""
    descs = [np.asarray(d, dtype=np.float32) for d in descs]
    nd = {d.shape[1] for d in descs if d.ndim == 2}
    if any(d.ndim != 2 for d in descs) or len(nd) > 1:
        raise ValueError("descs must be 2-D float32 arrays with one row length")
    D = nd.pop() if nd else 128
    if pairs is None:
        pairs = [(i, j) for i in range(len(descs)) for j in range(i + 1, len(descs))]
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    pl, pr = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    img_ptr = np.zeros(len(descs) + 1, dtype=np.int64)
    img_ptr[1:] = np.cumsum([d.shape[0] for d in descs])
    flat = np.ascontiguousarray(np.concatenate(descs, axis=0) if descs else np.zeros((0, D), np.float32))
    if cap is None:                      # at most one entry per query row of a pair with >= 2 train rows: one call, no retry
        cap = int(sum(descs[l].shape[0] for l, r in zip(pl, pr) if 0 <= r < len(descs) and descs[r].shape[0] >= 2 and 0 <= l < len(descs)))
    lp, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    ptr = np.zeros(len(pl) + 1, dtype=np.int64)
    total = C.c_int64(0)
    for _ in range(2):
        q, t, d = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32)
        rc = lib().sfmba_match_features_l2(C.c_int(device), C.c_int(len(descs)), _p(img_ptr, lp), flat.ctypes.data_as(fp),
                                           C.c_int(D), C.c_int(len(pl)), _p(pl, _ip), _p(pr, _ip), C.c_double(ratio), _p(ptr, lp), _p(q, _ip),
                                           _p(t, _ip), _p(d, fp), C.c_int64(cap), C.byref(total))
        if rc != SFMBA_ERR_CAPACITY:
            break
        cap = int(total.value)
    _check(rc)
    n = total.value
    return pl, pr, ptr, q[:n].copy(), t[:n].copy(), d[:n].copy()


ORB_KEYPOINT = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32), ("response", np.float32),
                         ("octave", np.int32)])          # sfmba_orb_keypoint


def orb_extract(images, n_features=5000, scale_factor=1.2, n_levels=8, fast_threshold=20, cap=None, debug=False, device=0):
    """sfmba_orb_extract: ORB-style key points and 32-byte descriptors of every image of a batch (the contract is in include/sfmba.h).

    images: list of uint8 arrays, h x w (gray) or h x w x 3 (BGR), all of one kind.  Returns one tuple per image: (kp, desc) with kp a
    record array of ORB_KEYPOINT and desc uint8 [n, 32]; with debug=True (kp, desc, level_xy int32 [n, 2], bin int32 [n], harris
    int64 [n], candidates int32 [n_levels]).  cap=None sizes the outputs for n_features per image; a smaller cap is retried once
    with the size the library reports."""
    imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
    kinds = {(im.ndim, im.shape[2] if im.ndim == 3 else 1) for im in imgs}
    if len(kinds) > 1 or any(k not in ((2, 1), (3, 3)) for k in kinds):
        raise ValueError("images must all be h x w or all be h x w x 3 uint8 arrays")
    channels = kinds.pop()[1] if kinds else 1
    n = len(imgs)
    img_ptr = np.zeros(n + 1, dtype=np.int64)
    img_ptr[1:] = np.cumsum([im.size for im in imgs])
    flat = np.ascontiguousarray(np.concatenate([im.reshape(-1) for im in imgs]) if imgs else np.zeros(0, np.uint8))
    wd = np.asarray([im.shape[1] for im in imgs], dtype=np.int32)
    ht = np.asarray([im.shape[0] for im in imgs], dtype=np.int32)
    cap = int(n * max(n_features, 0) if cap is None else cap)
    lp, bp = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)
    kp_ptr = np.zeros(n + 1, dtype=np.int64)
    total = C.c_int64(0)
    cand = np.zeros((max(n, 1), max(n_levels, 1)), np.int32)
    for _ in range(2):
        kp = np.zeros(max(cap, 1), ORB_KEYPOINT)
        desc = np.zeros((max(cap, 1), 32), np.uint8)
        lxy, bn, hr = np.zeros((max(cap, 1), 2), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int64)
        rc = lib().sfmba_orb_extract(C.c_int(device), C.c_int(n), _p(img_ptr, lp), flat.ctypes.data_as(bp), _p(wd, _ip), _p(ht, _ip),
                                     C.c_int(channels), C.c_int(n_features), C.c_float(scale_factor), C.c_int(n_levels),
                                     C.c_int(fast_threshold), _p(kp_ptr, lp), kp.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(bp),
                                     C.c_int64(cap), C.byref(total), _p(lxy, _ip) if debug else None, _p(bn, _ip) if debug else None,
                                     _p(hr, lp) if debug else None, _p(cand, _ip) if debug else None)
        if rc != SFMBA_ERR_CAPACITY:
            break
        cap = int(total.value)
    _check(rc)
    out = []
    for i in range(n):
        a, b = int(kp_ptr[i]), int(kp_ptr[i + 1])
        if debug:
            out.append((kp[a:b].copy(), desc[a:b].copy(), lxy[a:b].copy(), bn[a:b].copy(), hr[a:b].copy(), cand[i].copy()))
        else:
            out.append((kp[a:b].copy(), desc[a:b].copy()))
    return out


SURF_KEYPOINT = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32), ("response", np.float32),
                          ("octave", np.int32), ("layer", np.int32), ("laplacian", np.int32)])          # sfmba_surf_keypoint


def surf_extract(images, n_features=5000, n_octaves=4, hessian_threshold=100.0, upright=0, cap=None, debug=False, device=0):
    """sfmba_surf_extract: Fast-Hessian key points and 64-float descriptors of every image of a batch (the contract is in include/sfmba.h).

    images: as orb_extract.  Returns one tuple per image: (kp, desc) with kp a record array of SURF_KEYPOINT and desc float32 [n, 64];
    with debug=True (kp, desc, bin int32 [n], moments int64 [n, 2], sums int64 [n, 64], candidates int32 [n_octaves, 2]).  cap=None
    sizes the outputs for n_features per image; a smaller cap is retried once with the size the library reports."""
    imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
    kinds = {(im.ndim, im.shape[2] if im.ndim == 3 else 1) for im in imgs}
    if len(kinds) > 1 or any(k not in ((2, 1), (3, 3)) for k in kinds):
        raise ValueError("images must all be h x w or all be h x w x 3 uint8 arrays")
    channels = kinds.pop()[1] if kinds else 1
    n = len(imgs)
    img_ptr = np.zeros(n + 1, dtype=np.int64)
    img_ptr[1:] = np.cumsum([im.size for im in imgs])
    flat = np.ascontiguousarray(np.concatenate([im.reshape(-1) for im in imgs]) if imgs else np.zeros(0, np.uint8))
    wd = np.asarray([im.shape[1] for im in imgs], dtype=np.int32)
    ht = np.asarray([im.shape[0] for im in imgs], dtype=np.int32)
    cap = int(n * max(n_features, 0) if cap is None else cap)
    lp, bp, fp = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte), C.POINTER(C.c_float)
    kp_ptr = np.zeros(n + 1, dtype=np.int64)
    total = C.c_int64(0)
    cand = np.zeros((max(n, 1), max(n_octaves, 1), 2), np.int32)
    for _ in range(2):
        kp = np.zeros(max(cap, 1), SURF_KEYPOINT)
        desc = np.zeros((max(cap, 1), 64), np.float32)
        bn, mom, sm = np.zeros(max(cap, 1), np.int32), np.zeros((max(cap, 1), 2), np.int64), np.zeros((max(cap, 1), 64), np.int64)
        rc = lib().sfmba_surf_extract(C.c_int(device), C.c_int(n), _p(img_ptr, lp), flat.ctypes.data_as(bp), _p(wd, _ip), _p(ht, _ip),
                                      C.c_int(channels), C.c_int(n_features), C.c_int(n_octaves), C.c_float(hessian_threshold),
                                      C.c_int(upright), _p(kp_ptr, lp), kp.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(fp),
                                      C.c_int64(cap), C.byref(total), _p(bn, _ip) if debug else None, _p(mom, lp) if debug else None,
                                      _p(sm, lp) if debug else None, _p(cand, _ip) if debug else None)
        if rc != SFMBA_ERR_CAPACITY:
            break
        cap = int(total.value)
    _check(rc)
    out = []
    for i in range(n):
        a, b = int(kp_ptr[i]), int(kp_ptr[i + 1])
        if debug:
            out.append((kp[a:b].copy(), desc[a:b].copy(), bn[a:b].copy(), mom[a:b].copy(), sm[a:b].copy(), cand[i].copy()))
        else:
            out.append((kp[a:b].copy(), desc[a:b].copy()))
    return out


def _flat_images(images):
    imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
    kinds = {(im.ndim, im.shape[2] if im.ndim == 3 else 1) for im in imgs}
    if len(kinds) > 1 or any(k not in ((2, 1), (3, 3)) for k in kinds):
        raise ValueError("images must all be h x w or all be h x w x 3 uint8 arrays")
    channels = kinds.pop()[1] if kinds else 1
    img_ptr = np.zeros(len(imgs) + 1, dtype=np.int64)
    img_ptr[1:] = np.cumsum([im.size for im in imgs])
    flat = np.ascontiguousarray(np.concatenate([im.reshape(-1) for im in imgs]) if imgs else np.zeros(1, np.uint8))
    wd = np.asarray([im.shape[1] for im in imgs], dtype=np.int32)
    ht = np.asarray([im.shape[0] for im in imgs], dtype=np.int32)
    return imgs, channels, img_ptr, flat, wd, ht


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    flat = np.asarray([v for x in lists for v in x] or [0], dtype=np.int32)
    return ptr, flat


def depth_sweep(images, K, P, jobs, n_planes=64, radius=3, min_std=2, min_score=0.6, min_sources=1, want_plane=True, device=0):
    """sfmba_depth_sweep: plane-sweep stereo for a list of jobs in one call (the contract is in include/sfmba.h).

    images: as orb_extract.  K [3, 3]; P [n_images, 3, 4].  jobs: list of (ref, sources, z_near, z_far).  Returns one tuple per job:
    (depth float32 [h, w], score float32 [h, w], plane int16 [h, w]); plane is None with want_plane=False (NULL is passed)."""
    imgs, channels, img_ptr, flat, wd, ht = _flat_images(images)
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1)
    if len(P) != 12 * len(imgs):
        raise ValueError("P must hold one 3 x 4 matrix per image")
    ref = np.asarray([j[0] for j in jobs] or [0], dtype=np.int32)
    src_ptr, src = _csr([list(j[1]) for j in jobs])
    zn = np.asarray([j[2] for j in jobs] or [0], dtype=np.float32)
    zf = np.asarray([j[3] for j in jobs] or [0], dtype=np.float32)
    sizes = [(int(ht[r]), int(wd[r])) if 0 <= r < len(imgs) else (0, 0) for r in ref[:len(jobs)]]
    n_px = sum(h * w for h, w in sizes)
    depth, score, plane = np.zeros(max(n_px, 1), np.float32), np.zeros(max(n_px, 1), np.float32), np.zeros(max(n_px, 1), np.int16)
    lp, bp, fp = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte), C.POINTER(C.c_float)
    _check(lib().sfmba_depth_sweep(C.c_int(device), C.c_int(len(imgs)), _p(img_ptr, lp), flat.ctypes.data_as(bp), _p(wd, _ip), _p(ht, _ip),
                                   C.c_int(channels), K.ctypes.data_as(fp), P.ctypes.data_as(fp), C.c_int(len(jobs)), _p(ref, _ip),
                                   _p(src_ptr, lp), _p(src, _ip), zn.ctypes.data_as(fp), zf.ctypes.data_as(fp), C.c_int(n_planes),
                                   C.c_int(radius), C.c_int(min_std), C.c_float(min_score), C.c_int(min_sources), depth.ctypes.data_as(fp),
                                   score.ctypes.data_as(fp), plane.ctypes.data_as(C.POINTER(C.c_int16)) if want_plane else None))
    out, at = [], 0
    for h, w in sizes:
        n = h * w
        out.append((depth[at:at + n].reshape(h, w).copy(), score[at:at + n].reshape(h, w).copy(),
                    plane[at:at + n].reshape(h, w).copy() if want_plane else None))
        at += n
    return out


def _sweep_inputs(images, K, P, jobs, device):
    """The arguments sfmba_depth_sweep and the calls that store its cost volume share, up to z_far; and the (h, w) of every job."""
    imgs, channels, img_ptr, flat, wd, ht = _flat_images(images)
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1)
    if len(P) != 12 * len(imgs):
        raise ValueError("P must hold one 3 x 4 matrix per image")
    ref = np.asarray([j[0] for j in jobs] or [0], dtype=np.int32)
    src_ptr, src = _csr([list(j[1]) for j in jobs])
    zn = np.asarray([j[2] for j in jobs] or [0], dtype=np.float32)
    zf = np.asarray([j[3] for j in jobs] or [0], dtype=np.float32)
    sizes = [(int(ht[r]), int(wd[r])) if 0 <= r < len(imgs) else (0, 0) for r in ref[:len(jobs)]]
    lp, bp, fp = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte), C.POINTER(C.c_float)
    keep = (img_ptr, flat, wd, ht, K, P, ref, src_ptr, src, zn, zf)
    args = [C.c_int(device), C.c_int(len(imgs)), _p(img_ptr, lp), flat.ctypes.data_as(bp), _p(wd, _ip), _p(ht, _ip), C.c_int(channels),
            K.ctypes.data_as(fp), P.ctypes.data_as(fp), C.c_int(len(jobs)), _p(ref, _ip), _p(src_ptr, lp), _p(src, _ip), zn.ctypes.data_as(fp),
            zf.ctypes.data_as(fp)]
    return args, sizes, keep


def depth_cost_volume(images, K, P, jobs, n_planes=64, radius=3, min_std=2, min_sources=1, invalid_cost=127, device=0):
    """sfmba_depth_cost_volume: the quantised cost of every (pixel, plane) of a list of sweep jobs (the contract is in include/sfmba.h).
    Inputs as depth_sweep.  Returns one uint8 [h, w, n_planes] array per job (255 = no cost)."""
    args, sizes, keep = _sweep_inputs(images, K, P, jobs, device)
    cost = np.zeros(max(sum(h * w for h, w in sizes) * max(n_planes, 0), 1), np.uint8)
    _check(lib().sfmba_depth_cost_volume(*args, C.c_int(n_planes), C.c_int(radius), C.c_int(min_std), C.c_int(min_sources), C.c_int(invalid_cost),
                                         cost.ctypes.data_as(C.POINTER(C.c_ubyte))))
    out, at = [], 0
    for h, w in sizes:
        out.append(cost[at:at + h * w * n_planes].reshape(h, w, n_planes).copy())
        at += h * w * n_planes
    return out


def sgm_aggregate(volumes, p1=8, p2=64, n_paths=8, invalid_cost=127, want_sums=True, n_planes=None, device=0):
    """sfmba_sgm_aggregate: semi-global aggregation and selection over cost volumes (the contract is in include/sfmba.h).

    volumes: uint8 [h, w, D] arrays with one D (n_planes overrides the D that is passed).  Returns one dict per volume: plane int16
    [h, w], best and second uint16 [h, w], sums uint16 [h, w, D] (None with want_sums=False: NULL is passed; want_sums may also be a
    list of one flag per volume: an entry of the pointer array is then NULL)."""
    vols = [np.ascontiguousarray(v, dtype=np.uint8) for v in volumes]
    if any(v.ndim != 3 for v in vols) or len({v.shape[2] for v in vols}) > 1:
        raise ValueError("volumes must be h x w x D uint8 arrays with one D")
    D = (vols[0].shape[2] if vols else 2) if n_planes is None else n_planes
    wd = np.asarray([v.shape[1] for v in vols] or [0], dtype=np.int32)
    ht = np.asarray([v.shape[0] for v in vols] or [0], dtype=np.int32)
    n = len(vols)
    plane = [np.zeros(v.shape[:2], np.int16) for v in vols]
    best = [np.zeros(v.shape[:2], np.uint16) for v in vols]
    second = [np.zeros(v.shape[:2], np.uint16) for v in vols]
    each = list(want_sums) if isinstance(want_sums, (list, tuple)) else [bool(want_sums)] * len(vols)
    want_sums = bool(want_sums) and any(each)
    sums = [np.zeros(v.shape, np.uint16) if e else None for v, e in zip(vols, each)] if want_sums else None
    bp, sp, up = C.POINTER(C.c_ubyte), C.POINTER(C.c_int16), C.POINTER(C.c_uint16)
    arr = lambda t, xs: (t * max(n, 1))(*[None if x is None else x.ctypes.data_as(t) for x in xs])
    _check(lib().sfmba_sgm_aggregate(C.c_int(device), C.c_int(n), arr(bp, vols), _p(wd, _ip), _p(ht, _ip), C.c_int(D), C.c_int(p1), C.c_int(p2),
                                     C.c_int(n_paths), C.c_int(invalid_cost), arr(sp, plane), arr(up, best), arr(up, second),
                                     arr(up, sums) if want_sums else None))
    return [dict(plane=plane[j], best=best[j], second=second[j], sums=sums[j] if want_sums else None) for j in range(n)]


def depth_sweep_sgm(images, K, P, jobs, n_planes=64, radius=3, min_std=2, min_sources=1, p1=8, p2=64, n_paths=8, invalid_cost=127,
                    uniqueness=5, want_plane=True, device=0):
    """sfmba_depth_sweep_sgm: plane sweep, semi-global aggregation and selection in one call (the contract is in include/sfmba.h).
    Inputs as depth_sweep (there is no min_score); returns what depth_sweep returns."""
    args, sizes, keep = _sweep_inputs(images, K, P, jobs, device)
    n_px = max(sum(h * w for h, w in sizes), 1)
    depth, score, plane = np.zeros(n_px, np.float32), np.zeros(n_px, np.float32), np.zeros(n_px, np.int16)
    fp = C.POINTER(C.c_float)
    _check(lib().sfmba_depth_sweep_sgm(*args, C.c_int(n_planes), C.c_int(radius), C.c_int(min_std), C.c_int(min_sources), C.c_int(p1), C.c_int(p2),
                                       C.c_int(n_paths), C.c_int(invalid_cost), C.c_int(uniqueness), depth.ctypes.data_as(fp),
                                       score.ctypes.data_as(fp), plane.ctypes.data_as(C.POINTER(C.c_int16)) if want_plane else None))
    out, at = [], 0
    for h, w in sizes:
        n = h * w
        out.append((depth[at:at + n].reshape(h, w).copy(), score[at:at + n].reshape(h, w).copy(),
                    plane[at:at + n].reshape(h, w).copy() if want_plane else None))
        at += n
    return out


def depth_fuse(images, K, P, depth_maps, checks, rel_tol=0.01, min_consistent=1, cap=None, device=0):
    """sfmba_depth_fuse: the depth maps of a set of images -> one coloured cloud (the contract is in include/sfmba.h).

    depth_maps: per image None or float32 [h, w]; checks: per image the list of its check images.  Returns a dict: xyz float32 [n, 3],
    bgr uint8 [n, 3], src_image int32 [n], src_pixel int32 [n], pt_ptr int64 [n_images + 1].  cap=None asks for the size first (cap 0);
    a short cap is retried once with the size the library reports."""
    imgs, channels, img_ptr, flat, wd, ht = _flat_images(images)
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1)
    if len(P) != 12 * len(imgs) or len(depth_maps) != len(imgs) or len(checks) != len(imgs):
        raise ValueError("P, depth_maps and checks must hold one entry per image")
    maps = [None if m is None else np.ascontiguousarray(m, dtype=np.float32) for m in depth_maps]
    for m, im in zip(maps, imgs):
        if m is not None and m.shape != im.shape[:2]:
            raise ValueError("a depth map must have its image's size")
    fp, lp, bp = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)
    ptrs = (fp * max(len(imgs), 1))(*[None if m is None else m.ctypes.data_as(fp) for m in maps])
    chk_ptr, chk = _csr([list(c) for c in checks])
    pt_ptr = np.zeros(len(imgs) + 1, dtype=np.int64)
    total = C.c_int64(0)
    cap = 0 if cap is None else int(cap)
    for _ in range(2):
        xyz, bgr = np.zeros((max(cap, 1), 3), np.float32), np.zeros((max(cap, 1), 3), np.uint8)
        si, sp = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
        rc = lib().sfmba_depth_fuse(C.c_int(device), C.c_int(len(imgs)), _p(img_ptr, lp), flat.ctypes.data_as(bp), _p(wd, _ip), _p(ht, _ip),
                                    C.c_int(channels), K.ctypes.data_as(fp), P.ctypes.data_as(fp), ptrs, _p(chk_ptr, lp), _p(chk, _ip),
                                    C.c_float(rel_tol), C.c_int(min_consistent), _p(pt_ptr, lp), xyz.ctypes.data_as(fp), bgr.ctypes.data_as(bp),
                                    _p(si, _ip), _p(sp, _ip), C.c_int64(cap), C.byref(total))
        if rc != SFMBA_ERR_CAPACITY:
            break
        cap = int(total.value)
    _check(rc)
    n = int(total.value)
    return {"xyz": xyz[:n].copy(), "bgr": bgr[:n].copy(), "src_image": si[:n].copy(), "src_pixel": sp[:n].copy(), "pt_ptr": pt_ptr.copy()}


def _flow_pairs(pairs, lists, width):
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    if len(lists) != len(pairs):
        raise ValueError("one point list per pair")
    rows = [np.asarray(x, dtype=np.float32).reshape(-1, width) for x in lists]
    ptr = np.zeros(len(pairs) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    flat = np.ascontiguousarray(np.concatenate(rows, axis=0) if rows else np.zeros((0, width), np.float32))
    if not len(flat):
        flat = np.zeros((1, width), np.float32)
    return np.ascontiguousarray(pairs[:, 0]) if len(pairs) else np.zeros(1, np.int32), \
        np.ascontiguousarray(pairs[:, 1]) if len(pairs) else np.zeros(1, np.int32), ptr, flat, len(pairs)


def flow_pyramid_sizes(w, h, n_levels):
    """(w, h) of the n_levels pyramid levels of a w x h image (sfmba_flow_track)."""
    out = []
    for _ in range(n_levels):
        out.append((w, h))
        w, h = (w + 1) >> 1, (h + 1) >> 1
    return out


def flow_track(images, pairs, points, n_levels=4, radius=7, max_iters=20, min_eig=1.0, debug=False, device=0):
    """sfmba_flow_track: pyramidal Lucas-Kanade tracking of the points of a list of image pairs (the contract is in include/sfmba.h).

    images: as orb_extract.  pairs: list of (src, dst) image indices; points: per pair a float32 array [n, 2] of (x, y) in the source
    image.  Returns one tuple per pair: (next float32 [n, 2], status uint8 [n], err float32 [n]); with debug=True a pair of lists:
    per pair (next, status, err, G int64 [n, L, 3], state int32 [n, L, 4]) and per image its L pyramid levels (uint8 [h_l, w_l]; of
    an image that no pair names, zeros)."""
    imgs, channels, img_ptr, flat, wd, ht = _flat_images(images)
    ps, pd, pt_ptr, pts, n_pairs = _flow_pairs(pairs, points, 2)
    n = int(pt_ptr[-1])
    L = max(int(n_levels), 1)
    nxt, status, err = np.zeros((max(n, 1), 2), np.float32), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.float32)
    G, state = np.zeros((max(n, 1), L, 3), np.int64), np.zeros((max(n, 1), L, 4), np.int32)
    in_range = 1 <= n_levels <= 8
    sizes = [flow_pyramid_sizes(int(w), int(h), L if in_range else 1) for w, h in zip(wd, ht)]
    pyr = np.zeros(max(sum(w * h for s in sizes for w, h in s), 1), np.uint8)
    lp, bp, fp = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte), C.POINTER(C.c_float)
    _check(lib().sfmba_flow_track(C.c_int(device), C.c_int(len(imgs)), _p(img_ptr, lp), flat.ctypes.data_as(bp), _p(wd, _ip), _p(ht, _ip),
                                  C.c_int(channels), C.c_int(n_pairs), _p(ps, _ip), _p(pd, _ip), _p(pt_ptr, lp), pts.ctypes.data_as(fp),
                                  C.c_int(n_levels), C.c_int(radius), C.c_int(max_iters), C.c_float(min_eig), nxt.ctypes.data_as(fp),
                                  status.ctypes.data_as(bp), err.ctypes.data_as(fp), _p(G, lp) if debug else None,
                                  _p(state, _ip) if debug else None, pyr.ctypes.data_as(bp) if debug else None))
    out = []
    for p in range(n_pairs):
        a, b = int(pt_ptr[p]), int(pt_ptr[p + 1])
        row = (nxt[a:b].copy(), status[a:b].copy(), err[a:b].copy())
        out.append(row + (G[a:b].copy(), state[a:b].copy()) if debug else row)
    if not debug:
        return out
    levels, at = [], 0
    for s in sizes:
        levels.append([])
        for w, h in s:
            levels[-1].append(pyr[at:at + w * h].reshape(h, w).copy())
            at += w * h
    return out, levels


def flow_match(keypoints, pairs, tracked, max_err=12.0, radius=2.0, ratio=0.7, cap=None, device=0):
    """sfmba_flow_match: snap the tracker's end points to the key points of the destination image, ratio test, first come first served
    (the contract is in include/sfmba.h).

    keypoints: per image a float32 array [n_i, 2]; pairs: the (src, dst) list the tracker was given; tracked: per pair (next, status,
    err, ...) as flow_track returns it.  Returns (pair_ptr int64 [n_pairs+1], query_idx, train_idx, distance float32).  cap=None sizes
    the outputs for one entry per query; a smaller cap is retried once with the size the library reports."""
    kps = [np.asarray(k, dtype=np.float32).reshape(-1, 2) for k in keypoints]
    kp_ptr = np.zeros(len(kps) + 1, dtype=np.int64)
    kp_ptr[1:] = np.cumsum([len(k) for k in kps])
    kp = np.ascontiguousarray(np.concatenate(kps, axis=0) if kps else np.zeros((0, 2), np.float32))
    if not len(kp):
        kp = np.zeros((1, 2), np.float32)
    _, pd, pt_ptr, nxt, n_pairs = _flow_pairs(pairs, [t[0] for t in tracked], 2)
    n = int(pt_ptr[-1])
    status = np.ascontiguousarray(np.concatenate([np.asarray(t[1], np.uint8).reshape(-1) for t in tracked] + [np.zeros(0, np.uint8)]))
    err = np.ascontiguousarray(np.concatenate([np.asarray(t[2], np.float32).reshape(-1) for t in tracked] + [np.zeros(0, np.float32)]))
    if len(status) != n or len(err) != n:
        raise ValueError("next, status and err of a pair must have one length")
    if not n:
        status, err = np.zeros(1, np.uint8), np.zeros(1, np.float32)
    cap = n if cap is None else int(cap)
    lp, bp, fp = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte), C.POINTER(C.c_float)
    ptr = np.zeros(n_pairs + 1, dtype=np.int64)
    total = C.c_int64(0)
    for _ in range(2):
        q, t, d = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32)
        rc = lib().sfmba_flow_match(C.c_int(device), C.c_int(len(kps)), _p(kp_ptr, lp), kp.ctypes.data_as(fp), C.c_int(n_pairs), _p(pd, _ip),
                                    _p(pt_ptr, lp), nxt.ctypes.data_as(fp), status.ctypes.data_as(bp), err.ctypes.data_as(fp),
                                    C.c_float(max_err), C.c_float(radius), C.c_double(ratio), _p(ptr, lp), _p(q, _ip), _p(t, _ip), _p(d, fp),
                                    C.c_int64(cap), C.byref(total))
        if rc != SFMBA_ERR_CAPACITY:
            break
        cap = int(total.value)
    _check(rc)
    m = int(total.value)
    return ptr, q[:m].copy(), t[:m].copy(), d[:m].copy()


def depth_normals(K, P, depth_maps, max_rel_step=0.05, device=0):
    """sfmba_depth_normals: a normal per depth pixel (the contract is in include/sfmba.h).

    K [3, 3]; P [n_images, 3, 4]; depth_maps: per image None or float32 [h, w] (a None entry counts as a 1 x 1 image without a map).
    Returns per image None or float32 [h, w, 3]; (0, 0, 0) where a pixel has no normal."""
    maps = [None if m is None else np.ascontiguousarray(m, dtype=np.float32) for m in depth_maps]
    n = len(maps)
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1)
    if len(P) != 12 * n or any(m is not None and m.ndim != 2 for m in maps):
        raise ValueError("P must hold one 3 x 4 matrix per image, and a depth map is h x w")
    wd = np.asarray([1 if m is None else m.shape[1] for m in maps] or [1], dtype=np.int32)
    ht = np.asarray([1 if m is None else m.shape[0] for m in maps] or [1], dtype=np.int32)
    out = [None if m is None else np.zeros(m.shape + (3,), np.float32) for m in maps]
    fp = C.POINTER(C.c_float)
    dptr = (fp * max(n, 1))(*[None if m is None else m.ctypes.data_as(fp) for m in maps])
    optr = (fp * max(n, 1))(*[None if o is None else o.ctypes.data_as(fp) for o in out])
    _check(lib().sfmba_depth_normals(C.c_int(device), C.c_int(n), _p(wd, _ip), _p(ht, _ip), K.ctypes.data_as(fp), P.ctypes.data_as(fp), dptr,
                                     C.c_float(max_rel_step), optr))
    return out


def cloud_merge(xyz, bgr=None, normal=None, voxel=1.0, min_count=1, cap=None, want_voxel_of=True, device=0):
    """sfmba_cloud_merge: one point per occupied voxel of a cloud (the contract is in include/sfmba.h).

    xyz float32 [n, 3]; bgr uint8 [n, 3] or None; normal float32 [n, 3] or None.  Returns a dict: xyz float32 [m, 3], bgr uint8 [m, 3] or
    None, normal float32 [m, 3] or None, count int32 [m], first int32 [m], voxel_of int32 [n] or None, n_skipped.  cap=None asks for the
    size first (cap 0); a short cap is retried once with the size the library reports."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = len(xyz)
    bgr = None if bgr is None else np.ascontiguousarray(bgr, dtype=np.uint8).reshape(-1, 3)
    normal = None if normal is None else np.ascontiguousarray(normal, dtype=np.float32).reshape(-1, 3)
    if (bgr is not None and len(bgr) != n) or (normal is not None and len(normal) != n):
        raise ValueError("bgr and normal must hold one row per point")
    fp, bp, lp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte), C.POINTER(C.c_int64)
    voxel_of = np.zeros(max(n, 1), np.int32) if want_voxel_of else None
    total, skipped = C.c_int64(0), C.c_int64(0)
    cap = 0 if cap is None else int(cap)
    for _ in range(2):
        oxyz, obgr, onrm = np.zeros((max(cap, 1), 3), np.float32), np.zeros((max(cap, 1), 3), np.uint8), np.zeros((max(cap, 1), 3), np.float32)
        cnt, first = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
        rc = lib().sfmba_cloud_merge(C.c_int(device), C.c_int64(n), xyz.ctypes.data_as(fp), None if bgr is None else bgr.ctypes.data_as(bp),
                                     None if normal is None else normal.ctypes.data_as(fp), C.c_float(voxel), C.c_int(min_count),
                                     oxyz.ctypes.data_as(fp), None if bgr is None else obgr.ctypes.data_as(bp),
                                     None if normal is None else onrm.ctypes.data_as(fp), _p(cnt, _ip), _p(first, _ip),
                                     _p(voxel_of, _ip) if want_voxel_of else None, C.c_int64(cap), C.byref(total), C.byref(skipped))
        if rc != SFMBA_ERR_CAPACITY:
            break
        cap = int(total.value)
    _check(rc)
    m = int(total.value)
    return {"xyz": oxyz[:m].copy(), "bgr": None if bgr is None else obgr[:m].copy(), "normal": None if normal is None else onrm[:m].copy(),
            "count": cnt[:m].copy(), "first": first[:m].copy(), "voxel_of": voxel_of[:n].copy() if want_voxel_of else None,
            "n_skipped": int(skipped.value)}


def _tsdf_views(images, K, P, depth_maps):
    """The image arguments of sfmba_tsdf_integrate / sfmba_tsdf_mesh, in order, and what must stay alive beside them.  images None:
    no colour (pixels NULL); the sizes then come from the maps, and an image without a map counts as 1 x 1."""
    maps = [None if m is None else np.ascontiguousarray(m, dtype=np.float32) for m in depth_maps]
    n = len(maps)
    fp, lp, bp = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)
    if images is None:
        channels, img_ptr, flat = 1, None, None
        wd = np.asarray([1 if m is None else m.shape[1] for m in maps] or [1], dtype=np.int32)
        ht = np.asarray([1 if m is None else m.shape[0] for m in maps] or [1], dtype=np.int32)
    else:
        imgs, channels, img_ptr, flat, wd, ht = _flat_images(images)
        if len(imgs) != n or any(m is not None and m.shape != im.shape[:2] for m, im in zip(maps, imgs)):
            raise ValueError("one depth map (or None) per image, of its image's size")
        if not n:
            wd, ht = np.ones(1, np.int32), np.ones(1, np.int32)
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1)
    if len(P) != 12 * n:
        raise ValueError("P must hold one 3 x 4 matrix per image")
    if not n:
        P = np.zeros(12, np.float32)
    ptrs = (fp * max(n, 1))(*[None if m is None else m.ctypes.data_as(fp) for m in maps])
    args = [C.c_int(n), None if img_ptr is None else _p(img_ptr, lp), None if flat is None else _p(flat, bp), _p(wd, _ip), _p(ht, _ip),
            C.c_int(channels), _p(K, fp), _p(P, fp), ptrs]
    return args, (maps, img_ptr, flat, wd, ht, K, P)


def _tsdf_grid(origin, voxel, dims):
    origin = np.ascontiguousarray(origin, dtype=np.float32).reshape(3)
    nx, ny, nz = (int(v) for v in dims)
    return [_p(origin, C.POINTER(C.c_float)), C.c_float(voxel), C.c_int(nx), C.c_int(ny), C.c_int(nz)], origin, (nz, ny, nx)


def tsdf_integrate(images, K, P, depth_maps, origin, voxel, dims, trunc, colour=True, device=0):
    """sfmba_tsdf_integrate: depth maps -> a truncated signed distance grid (the contract is in include/sfmba.h).

    images: as orb_extract, or None (no colour); K [3, 3]; P [n_images, 3, 4]; depth_maps: per image None or float32 [h, w]; origin [3];
    dims = (nx, ny, nz).  Returns a dict: sum, weight int32 [nz, ny, nx]; csum int32 [nz, ny, nx, 3] and cweight int32 [nz, ny, nx], both
    None without images or with colour=False (NULL is passed)."""
    views, keep = _tsdf_views(images, K, P, depth_maps)
    grid, origin, shape = _tsdf_grid(origin, voxel, dims)
    S, W = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    with_colour = images is not None and colour
    CS, CW = (np.zeros(shape + (3,), np.int32), np.zeros(shape, np.int32)) if with_colour else (None, None)
    _check(lib().sfmba_tsdf_integrate(C.c_int(device), *views, *grid, C.c_float(trunc), _p(S, _ip), _p(W, _ip),
                                      _p(CS, _ip) if with_colour else None, _p(CW, _ip) if with_colour else None))
    return {"sum": S, "weight": W, "csum": CS, "cweight": CW}


def _tsdf_mesh_call(call, colour, want_vkey, vcap, tcap):
    """Runs call(xyz, bgr, vkey, vcap, tri, tcap, n_vertices, n_triangles) with the size-first protocol of depth_fuse."""
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    nv, nt = C.c_int64(0), C.c_int64(0)
    vcap, tcap = 0 if vcap is None else int(vcap), 0 if tcap is None else int(tcap)
    for _ in range(2):
        xyz, bgr = np.zeros((max(vcap, 1), 3), np.float32), np.zeros((max(vcap, 1), 3), np.uint8)
        vkey, tri = np.zeros(max(vcap, 1), np.int32), np.zeros((max(tcap, 1), 3), np.int32)
        rc = call(_p(xyz, fp), _p(bgr, bp) if colour else None, _p(vkey, _ip) if want_vkey else None, C.c_int64(vcap), _p(tri, _ip),
                  C.c_int64(tcap), C.byref(nv), C.byref(nt))
        if rc != SFMBA_ERR_CAPACITY:
            break
        vcap, tcap = int(nv.value), int(nt.value)
    _check(rc)
    v, t = int(nv.value), int(nt.value)
    return {"xyz": xyz[:v].copy(), "bgr": bgr[:v].copy() if colour else None, "vkey": vkey[:v].copy() if want_vkey else None,
            "tri": tri[:t].copy()}


def tsdf_extract(origin, voxel, grid_sum, grid_weight, csum=None, cweight=None, min_weight=1, want_vkey=True, vcap=None, tcap=None, device=0):
    """sfmba_tsdf_extract: the surface of a truncated signed distance grid by marching tetrahedra (the contract is in include/sfmba.h).

    grid_sum, grid_weight int32 [nz, ny, nx]; csum int32 [nz, ny, nx, 3] and cweight int32 [nz, ny, nx] or both None.  Returns a dict:
    xyz float32 [n, 3], bgr uint8 [n, 3] or None, vkey int32 [n] or None, tri int32 [m, 3].  vcap / tcap None asks for the sizes first
    (capacity 0); short capacities are retried once with the sizes the library reports."""
    S, W = np.ascontiguousarray(grid_sum, dtype=np.int32), np.ascontiguousarray(grid_weight, dtype=np.int32)
    if S.ndim != 3 or W.shape != S.shape or (csum is None) != (cweight is None):
        raise ValueError("sum and weight are [nz, ny, nx]; csum and cweight come together")
    nz, ny, nx = S.shape
    grid, origin, _ = _tsdf_grid(origin, voxel, (nx, ny, nz))
    colour = csum is not None
    if colour:
        csum, cweight = np.ascontiguousarray(csum, dtype=np.int32), np.ascontiguousarray(cweight, dtype=np.int32)
        if csum.shape != S.shape + (3,) or cweight.shape != S.shape:
            raise ValueError("csum is [nz, ny, nx, 3] and cweight [nz, ny, nx]")

    def call(*out):
        return lib().sfmba_tsdf_extract(C.c_int(device), *grid, _p(S, _ip), _p(W, _ip), _p(csum, _ip) if colour else None,
                                        _p(cweight, _ip) if colour else None, C.c_int(min_weight), *out)
    return _tsdf_mesh_call(call, colour, want_vkey, vcap, tcap)


def tsdf_mesh(images, K, P, depth_maps, origin, voxel, dims, trunc, min_weight=1, want_vkey=True, vcap=None, tcap=None, device=0):
    """sfmba_tsdf_mesh: depth maps -> a triangle mesh, the grid never leaving the device; equals tsdf_integrate followed by
    tsdf_extract byte for byte (the contract is in include/sfmba.h).  Arguments as tsdf_integrate takes them, the result as
    tsdf_extract gives it; bgr is None when images is None."""
    views, keep = _tsdf_views(images, K, P, depth_maps)
    grid, origin, _ = _tsdf_grid(origin, voxel, dims)

    def call(*out):
        return lib().sfmba_tsdf_mesh(C.c_int(device), *views, *grid, C.c_float(trunc), C.c_int(min_weight), *out)
    return _tsdf_mesh_call(call, images is not None, want_vkey, vcap, tcap)


def tsdf_fill(grid_sum, grid_weight, csum=None, cweight=None, min_weight=1, iterations=3, min_neighbours=2, want_state=True, device=0):
    """sfmba_tsdf_fill: volumetric diffusion of the signed distance into the undefined vertices of a grid, so that the extraction closes
    the holes (the contract is in include/sfmba.h; THE FILL CONTINUES THE SURFACE PAST AN OPEN BORDER AS A SKIRT UP TO `iterations`
    VOXELS WIDE).

    grid_sum, grid_weight int32 [nz, ny, nx]; csum int32 [nz, ny, nx, 3] and cweight int32 [nz, ny, nx] or both None.  Returns a dict:
    sum, weight, csum, cweight (None without colour) of the filled grid; state uint8 [nz, ny, nx] (0 observed, p the pass in which the
    vertex became known, 255 still unknown) or None; n_filled."""
    S, W = np.ascontiguousarray(grid_sum, dtype=np.int32), np.ascontiguousarray(grid_weight, dtype=np.int32)
    if S.ndim != 3 or W.shape != S.shape or (csum is None) != (cweight is None):
        raise ValueError("sum and weight are [nz, ny, nx]; csum and cweight come together")
    nz, ny, nx = S.shape
    colour = csum is not None
    if colour:
        csum, cweight = np.ascontiguousarray(csum, dtype=np.int32), np.ascontiguousarray(cweight, dtype=np.int32)
        if csum.shape != S.shape + (3,) or cweight.shape != S.shape:
            raise ValueError("csum is [nz, ny, nx, 3] and cweight [nz, ny, nx]")
    So, Wo = np.zeros_like(S), np.zeros_like(W)
    CSo, CWo = (np.zeros_like(csum), np.zeros_like(cweight)) if colour else (None, None)
    state = np.zeros(S.shape, np.uint8) if want_state else None
    n_filled = C.c_int64(0)
    bp = C.POINTER(C.c_ubyte)
    _check(lib().sfmba_tsdf_fill(C.c_int(device), C.c_int(nx), C.c_int(ny), C.c_int(nz), _p(S, _ip), _p(W, _ip), _p(csum, _ip) if colour else None,
                                 _p(cweight, _ip) if colour else None, C.c_int(min_weight), C.c_int(iterations), C.c_int(min_neighbours),
                                 _p(So, _ip), _p(Wo, _ip), _p(CSo, _ip) if colour else None, _p(CWo, _ip) if colour else None,
                                 _p(state, bp) if want_state else None, C.byref(n_filled)))
    return {"sum": So, "weight": Wo, "csum": CSo, "cweight": CWo, "state": state, "n_filled": int(n_filled.value)}


def tsdf_mesh_fill(images, K, P, depth_maps, origin, voxel, dims, trunc, min_weight=1, fill_iterations=3, min_neighbours=2, want_vkey=True,
                   want_vfilled=True, vcap=None, tcap=None, device=0):
    """sfmba_tsdf_mesh_fill: depth maps -> a triangle mesh with its holes filled, the grid never leaving the device; equals
    tsdf_integrate, tsdf_fill and tsdf_extract byte for byte, and tsdf_mesh with fill_iterations 0 (the contract is in include/sfmba.h).
    Arguments as tsdf_mesh takes them; the result has vfilled uint8 [n] (1 iff either end of the vertex's edge is a filled grid vertex)
    or None beside what tsdf_mesh gives."""
    views, keep = _tsdf_views(images, K, P, depth_maps)
    grid, origin, _ = _tsdf_grid(origin, voxel, dims)
    bp = C.POINTER(C.c_ubyte)
    box = {}

    def call(xyz, bgr, vkey, cap, *rest):
        box["vfilled"] = np.zeros(max(int(cap.value), 1), np.uint8)
        return lib().sfmba_tsdf_mesh_fill(C.c_int(device), *views, *grid, C.c_float(trunc), C.c_int(min_weight), C.c_int(fill_iterations),
                                          C.c_int(min_neighbours), xyz, bgr, vkey, _p(box["vfilled"], bp) if want_vfilled else None, cap, *rest)
    out = _tsdf_mesh_call(call, images is not None, want_vkey, vcap, tcap)
    out["vfilled"] = box["vfilled"][:len(out["xyz"])].copy() if want_vfilled else None
    return out


def _clean_mesh(xyz, bgr, tri):
    """The mesh arguments of the mesh-cleaning calls: xyz float32 [n, 3] (or a vertex count), bgr uint8 [n, 3] or None, tri int32 [m, 3]."""
    tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    if isinstance(xyz, (int, np.integer)):
        return int(xyz), None, None, tri
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    if bgr is not None:
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8).reshape(-1, 3)
        if len(bgr) != len(xyz):
            raise ValueError("one colour per vertex")
    return len(xyz), xyz, bgr, tri


def _opt(a, t):
    return None if a is None or a.size == 0 else _p(a, t)


def mesh_components(n_vertices, tri, want_comp_triangles=True, device=0):
    """sfmba_mesh_components: the connected components of a triangle list (the contract is in include/sfmba.h).

    Returns a dict: label int32 [n_vertices], comp_triangles int32 [n_vertices] or None (NULL is passed), n_components, largest."""
    nv, _, _, tri = _clean_mesh(int(n_vertices), None, tri)
    label, comp = np.zeros(max(nv, 1), np.int32), np.zeros(max(nv, 1), np.int32)
    nc, largest = C.c_int64(0), C.c_int64(0)
    _check(lib().sfmba_mesh_components(C.c_int(device), C.c_int64(nv), C.c_int64(len(tri)), _opt(tri, _ip), _p(label, _ip),
                                       _p(comp, _ip) if want_comp_triangles else None, C.byref(nc), C.byref(largest)))
    return {"label": label[:nv].copy(), "comp_triangles": comp[:nv].copy() if want_comp_triangles else None, "n_components": int(nc.value),
            "largest": int(largest.value)}


def _mesh_clean_call(call, nv, colour, want_normal, want_vertex_of, vcap, tcap):
    """Runs call(xyz_out, bgr_out, normal, vcap, tri_out, tcap, vertex_of, n_vertices_out, n_triangles_out) with the size-first
    protocol of tsdf_extract."""
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    n_v, n_t = C.c_int64(0), C.c_int64(0)
    vcap, tcap = 0 if vcap is None else int(vcap), 0 if tcap is None else int(tcap)
    vertex_of = np.zeros(max(nv, 1), np.int32)
    for _ in range(2):
        xyz, bgr, nrm = np.zeros((max(vcap, 1), 3), np.float32), np.zeros((max(vcap, 1), 3), np.uint8), np.zeros((max(vcap, 1), 3), np.float32)
        tri = np.zeros((max(tcap, 1), 3), np.int32)
        rc = call(_p(xyz, fp), _p(bgr, bp) if colour else None, _p(nrm, fp) if want_normal else None, C.c_int64(vcap), _p(tri, _ip),
                  C.c_int64(tcap), _p(vertex_of, _ip) if want_vertex_of else None, C.byref(n_v), C.byref(n_t))
        if rc != SFMBA_ERR_CAPACITY:
            break
        vcap, tcap = int(n_v.value), int(n_t.value)
    _check(rc)
    v, t = int(n_v.value), int(n_t.value)
    return {"xyz": xyz[:v].copy(), "bgr": bgr[:v].copy() if colour else None, "normal": nrm[:v].copy() if want_normal else None,
            "tri": tri[:t].copy(), "vertex_of": vertex_of[:nv].copy() if want_vertex_of else None}


def mesh_filter(xyz, bgr, tri, min_triangles=1, keep_largest=False, want_vertex_of=True, vcap=None, tcap=None, device=0):
    """sfmba_mesh_filter: drop the components with fewer than min_triangles triangles (or all but the largest) and compact (the
    contract is in include/sfmba.h).

    Returns a dict: xyz float32 [n, 3], bgr uint8 [n, 3] or None, tri int32 [m, 3], vertex_of int32 [n_vertices] or None.  vcap / tcap
    None asks for the sizes first (capacity 0); short capacities are retried once with the sizes the library reports."""
    nv, xyz, bgr, tri = _clean_mesh(xyz, bgr, tri)
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte)

    def call(oxyz, obgr, onrm, vcap, otri, tcap, vof, n_v, n_t):
        return lib().sfmba_mesh_filter(C.c_int(device), C.c_int64(nv), _opt(xyz, fp), _opt(bgr, bp), C.c_int64(len(tri)), _opt(tri, _ip),
                                       C.c_int(min_triangles), C.c_int(int(keep_largest)), oxyz, obgr, vcap, otri, tcap, vof, n_v, n_t)
    out = _mesh_clean_call(call, nv, bgr is not None, False, want_vertex_of, vcap, tcap)
    del out["normal"]
    return out


def mesh_smooth(xyz, tri, origin, quantum, iterations=10, lam=0.5, mu=-0.53, want_normal=True, device=0):
    """sfmba_mesh_smooth: Taubin's lambda | mu smoothing in integers and a normal per vertex (the contract is in include/sfmba.h).

    Returns a dict: xyz float32 [n, 3], normal float32 [n, 3] or None (NULL is passed)."""
    nv, xyz, _, tri = _clean_mesh(xyz, None, tri)
    fp = C.POINTER(C.c_float)
    origin = np.ascontiguousarray(origin, dtype=np.float32).reshape(3)
    out, nrm = np.zeros((max(nv, 1), 3), np.float32), np.zeros((max(nv, 1), 3), np.float32)
    _check(lib().sfmba_mesh_smooth(C.c_int(device), C.c_int64(nv), _opt(xyz, fp), C.c_int64(len(tri)), _opt(tri, _ip), _p(origin, fp),
                                   C.c_float(quantum), C.c_int(iterations), C.c_float(lam), C.c_float(mu), _p(out, fp),
                                   _p(nrm, fp) if want_normal else None))
    return {"xyz": out[:nv].copy(), "normal": nrm[:nv].copy() if want_normal else None}


def mesh_clean(xyz, bgr, tri, origin, quantum, min_triangles=1, keep_largest=False, iterations=10, lam=0.5, mu=-0.53, want_normal=True,
               want_vertex_of=True, vcap=None, tcap=None, device=0):
    """sfmba_mesh_clean: mesh_filter followed by mesh_smooth with the mesh staying on the device; equals the two calls byte for byte
    (the contract is in include/sfmba.h).  Returns a dict: xyz, bgr (or None), normal (or None), tri, vertex_of (or None)."""
    nv, xyz, bgr, tri = _clean_mesh(xyz, bgr, tri)
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    origin = np.ascontiguousarray(origin, dtype=np.float32).reshape(3)

    def call(oxyz, obgr, onrm, vcap, otri, tcap, vof, n_v, n_t):
        return lib().sfmba_mesh_clean(C.c_int(device), C.c_int64(nv), _opt(xyz, fp), _opt(bgr, bp), C.c_int64(len(tri)), _opt(tri, _ip),
                                      C.c_int(min_triangles), C.c_int(int(keep_largest)), _p(origin, fp), C.c_float(quantum), C.c_int(iterations),
                                      C.c_float(lam), C.c_float(mu), oxyz, obgr, onrm, vcap, otri, tcap, vof, n_v, n_t)
    return _mesh_clean_call(call, nv, bgr is not None, want_normal, want_vertex_of, vcap, tcap)


def mesh_decimate(xyz, bgr, tri, origin, quantum, cell, placement=1, reg=1024, want_members=True, want_triangle_of=True, want_vertex_of=True,
                  want_stats=True, vcap=None, tcap=None, device=0):
    """sfmba_mesh_decimate: vertex clustering with the mean (placement 0) or the quadric (1) placement (the contract is in
    include/sfmba.h).

    Returns a dict: xyz float32 [n, 3], bgr uint8 [n, 3] or None, members int32 [n] or None, tri int32 [m, 3], triangle_of int32 [m] or
    None, vertex_of int32 [n_vertices] or None, stats (a list of four) or None; None where NULL is passed.  vcap / tcap None asks for
    the sizes first (capacity 0); short capacities are retried once with the sizes the library reports."""
    nv, xyz, bgr, tri = _clean_mesh(xyz, bgr, tri)
    fp, bp, lp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte), C.POINTER(C.c_int64)
    origin = np.ascontiguousarray(origin, dtype=np.float32).reshape(3)
    colour = bgr is not None
    n_v, n_t = C.c_int64(0), C.c_int64(0)
    vcap, tcap = 0 if vcap is None else int(vcap), 0 if tcap is None else int(tcap)
    vertex_of, stats = np.zeros(max(nv, 1), np.int32), np.zeros(4, np.int64)
    for _ in range(2):
        oxyz, obgr, mem = np.zeros((max(vcap, 1), 3), np.float32), np.zeros((max(vcap, 1), 3), np.uint8), np.zeros(max(vcap, 1), np.int32)
        otri, tof = np.zeros((max(tcap, 1), 3), np.int32), np.zeros(max(tcap, 1), np.int32)
        rc = lib().sfmba_mesh_decimate(C.c_int(device), C.c_int64(nv), _opt(xyz, fp), _opt(bgr, bp), C.c_int64(len(tri)), _opt(tri, _ip),
                                       _p(origin, fp), C.c_float(quantum), C.c_int(cell), C.c_int(placement), C.c_int(reg), _p(oxyz, fp),
                                       _p(obgr, bp) if colour else None, _p(mem, _ip) if want_members else None, C.c_int64(vcap), _p(otri, _ip),
                                       _p(tof, _ip) if want_triangle_of else None, C.c_int64(tcap), _p(vertex_of, _ip) if want_vertex_of else None,
                                       C.byref(n_v), C.byref(n_t), _p(stats, lp) if want_stats else None)
        if rc != SFMBA_ERR_CAPACITY:
            break
        vcap, tcap = int(n_v.value), int(n_t.value)
    _check(rc)
    v, t = int(n_v.value), int(n_t.value)
    return {"xyz": oxyz[:v].copy(), "bgr": obgr[:v].copy() if colour else None, "members": mem[:v].copy() if want_members else None,
            "tri": otri[:t].copy(), "triangle_of": tof[:t].copy() if want_triangle_of else None,
            "vertex_of": vertex_of[:nv].copy() if want_vertex_of else None, "stats": [int(x) for x in stats] if want_stats else None}


def mesh_texture_size(n_triangles, patch=6, blocks_per_row=1):
    """sfmba_mesh_texture_size: (W, H) of the atlas of sfmba_mesh_texture (the contract is in include/sfmba.h)."""
    w, h = C.c_int32(0), C.c_int32(0)
    _check(lib().sfmba_mesh_texture_size(C.c_int64(n_triangles), C.c_int(patch), C.c_int(blocks_per_row), C.byref(w), C.byref(h)))
    return int(w.value), int(h.value)


def mesh_texture(xyz, bgr, tri, images, K, P, depth_maps, occl_tol, min_area=0, patch=6, blocks_per_row=None, want_score=True, device=0):
    """sfmba_mesh_texture: a view per triangle and a texture atlas with one fixed-size patch per triangle (the contract is in
    include/sfmba.h; NO COLOUR ADJUSTMENT ACROSS VIEWS unless asked for (off by default), see mesh_texture_adjust, NO SMOOTHING OF THE VIEW
    LABELS, NO CHART MERGING).

    The mesh as mesh_clean takes it; images, K, P, depth_maps as tsdf_integrate takes them (images are required; a map may be None).
    blocks_per_row None: ceil(sqrt(n_blocks)), at least 1.  Returns a dict: atlas uint8 [H, W, 3] (BGR), uv float32 [m, 3, 2] in atlas
    pixels, view int32 [m], score int64 [m] or None (NULL is passed), n_textured."""
    nv, xyz, bgr, tri = _clean_mesh(xyz, bgr, tri)
    nt = len(tri)
    if blocks_per_row is None:
        blocks_per_row = max(1, int(np.ceil(np.sqrt((nt + 1) // 2))))
        while blocks_per_row * blocks_per_row < (nt + 1) // 2:
            blocks_per_row += 1
    views, keep = _tsdf_views(images, K, P, depth_maps)
    W, H = mesh_texture_size(nt, patch, blocks_per_row)
    fp, bp, lp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte), C.POINTER(C.c_int64)
    atlas, uv = np.zeros((H, W, 3), np.uint8), np.zeros((max(nt, 1), 3, 2), np.float32)
    view, score = np.zeros(max(nt, 1), np.int32), np.zeros(max(nt, 1), np.int64)
    n_textured = C.c_int64(0)
    _check(lib().sfmba_mesh_texture(C.c_int(device), C.c_int64(nv), _opt(xyz, fp), _opt(bgr, bp), C.c_int64(nt), _opt(tri, _ip), *views,
                                    C.c_float(occl_tol), C.c_int64(min_area), C.c_int(patch), C.c_int(blocks_per_row), _p(atlas, bp), _p(uv, fp),
                                    _p(view, _ip), _p(score, lp) if want_score else None, C.byref(n_textured)))
    return {"atlas": atlas, "uv": uv[:nt].copy(), "view": view[:nt].copy(), "score": score[:nt].copy() if want_score else None,
            "n_textured": int(n_textured.value)}


LABEL_STATS = ("energy_start", "energy_end", "diff_rank0", "diff_start", "diff_end", "frontier", "moves", "n_passes")    # stats[0..7]


def _default_blocks_per_row(nt):
    b = max(1, int(np.ceil(np.sqrt((nt + 1) // 2))))
    while b * b < (nt + 1) // 2:
        b += 1
    return b


def mesh_view_candidates(xyz, tri, images, K, P, depth_maps, occl_tol, min_area=0, n_candidates=4, device=0):
    """sfmba_mesh_view_candidates: the n_candidates eligible views of largest score per triangle (the contract is in include/sfmba.h).
    Returns (cand_view int32 [m, k], cand_score int64 [m, k]); unused entries are -1 and 0."""
    nv, xyz, _, tri = _clean_mesh(xyz, None, tri)
    nt, k = len(tri), int(n_candidates)
    views, keep = _tsdf_views(images, K, P, depth_maps)
    fp, lp = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    cv, cs = np.zeros((max(nt, 1), max(k, 1)), np.int32), np.zeros((max(nt, 1), max(k, 1)), np.int64)
    _check(lib().sfmba_mesh_view_candidates(C.c_int(device), C.c_int64(nv), _opt(xyz, fp), C.c_int64(nt), _opt(tri, _ip), *views, C.c_float(occl_tol),
                                            C.c_int64(min_area), C.c_int(k), _p(cv, _ip), _p(cs, lp)))
    return cv[:nt].copy(), cs[:nt].copy()


def mesh_adjacency(tri, device=0):
    """sfmba_mesh_adjacency: the triangle across each edge (the contract is in include/sfmba.h).  Returns a dict: adj int32 [m, 3],
    n_pairs, n_open_edges, n_nonmanifold_edges."""
    tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    nt = len(tri)
    adj = np.zeros((max(nt, 1), 3), np.int32)
    n = [C.c_int64(0) for _ in range(3)]
    _check(lib().sfmba_mesh_adjacency(C.c_int(device), C.c_int64(nt), _opt(tri, _ip), _p(adj, _ip), *[C.byref(c) for c in n]))
    return {"adj": adj[:nt].copy(), "n_pairs": int(n[0].value), "n_open_edges": int(n[1].value), "n_nonmanifold_edges": int(n[2].value)}


def mesh_view_smooth(cand_view, cand_score, adj, n_images, rings=0, penalty=256, max_passes=0, device=0):
    """sfmba_mesh_view_smooth: score diffusion over `rings` rings and a parallel Potts relaxation of at most max_passes passes (the
    contract is in include/sfmba.h).  Returns (view int32 [m], stats int64 [8], named by LABEL_STATS)."""
    cv = np.ascontiguousarray(cand_view, dtype=np.int32)
    cs = np.ascontiguousarray(cand_score, dtype=np.int64)
    adj = np.ascontiguousarray(adj, dtype=np.int32).reshape(-1, 3)
    if cv.ndim != 2 or cv.shape != cs.shape or len(adj) != len(cv):
        raise ValueError("cand_view and cand_score [m, k] and adj [m, 3]")
    nt, k = cv.shape
    view, stats = np.zeros(max(nt, 1), np.int32), np.zeros(8, np.int64)
    lp = C.POINTER(C.c_int64)
    _check(lib().sfmba_mesh_view_smooth(C.c_int(device), C.c_int64(nt), C.c_int(n_images), C.c_int(k), _opt(cv, _ip), _opt(cs, lp), _opt(adj, _ip),
                                        C.c_int(rings), C.c_int(penalty), C.c_int(max_passes), _p(view, _ip), _p(stats, lp)))
    return view[:nt].copy(), stats


def mesh_texture_from_views(xyz, bgr, tri, images, K, P, view, patch=6, blocks_per_row=None, device=0):
    """sfmba_mesh_texture_from_views: the atlas of mesh_texture for GIVEN labels (each -1 or an image index; the contract is in
    include/sfmba.h).  Returns a dict: atlas, uv, n_textured."""
    nv, xyz, bgr, tri = _clean_mesh(xyz, bgr, tri)
    nt = len(tri)
    if blocks_per_row is None:
        blocks_per_row = _default_blocks_per_row(nt)
    view = np.ascontiguousarray(view, dtype=np.int32).reshape(-1)
    if len(view) != nt:
        raise ValueError("one view per triangle")
    views, keep = _tsdf_views(images, K, P, [None] * len(images))
    W, H = mesh_texture_size(nt, patch, blocks_per_row)
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    atlas, uv = np.zeros((H, W, 3), np.uint8), np.zeros((max(nt, 1), 3, 2), np.float32)
    n_textured = C.c_int64(0)
    _check(lib().sfmba_mesh_texture_from_views(C.c_int(device), C.c_int64(nv), _opt(xyz, fp), _opt(bgr, bp), C.c_int64(nt), _opt(tri, _ip), *views[:8],
                                               C.c_int(patch), C.c_int(blocks_per_row), _opt(view, _ip), _p(atlas, bp), _p(uv, fp),
                                               C.byref(n_textured)))
    return {"atlas": atlas, "uv": uv[:nt].copy(), "n_textured": int(n_textured.value)}


def mesh_texture_smooth(xyz, bgr, tri, images, K, P, depth_maps, occl_tol, min_area=0, patch=6, blocks_per_row=None, n_candidates=4, rings=4,
                        penalty=256, max_passes=100, want_score=True, device=0):
    """sfmba_mesh_texture_smooth: mesh_texture with smoothed view labels -- candidates, adjacency, diffusion, relaxation and the raster
    in one call, everything staying on the device (the contract is in include/sfmba.h).  Returns mesh_texture's dict and stats int64 [8]
    (named by LABEL_STATS)."""
    nv, xyz, bgr, tri = _clean_mesh(xyz, bgr, tri)
    nt = len(tri)
    if blocks_per_row is None:
        blocks_per_row = _default_blocks_per_row(nt)
    views, keep = _tsdf_views(images, K, P, depth_maps)
    W, H = mesh_texture_size(nt, patch, blocks_per_row)
    fp, bp, lp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte), C.POINTER(C.c_int64)
    atlas, uv = np.zeros((H, W, 3), np.uint8), np.zeros((max(nt, 1), 3, 2), np.float32)
    view, score, stats = np.zeros(max(nt, 1), np.int32), np.zeros(max(nt, 1), np.int64), np.zeros(8, np.int64)
    n_textured = C.c_int64(0)
    _check(lib().sfmba_mesh_texture_smooth(C.c_int(device), C.c_int64(nv), _opt(xyz, fp), _opt(bgr, bp), C.c_int64(nt), _opt(tri, _ip), *views,
                                           C.c_float(occl_tol), C.c_int64(min_area), C.c_int(patch), C.c_int(blocks_per_row), C.c_int(n_candidates),
                                           C.c_int(rings), C.c_int(penalty), C.c_int(max_passes), _p(atlas, bp), _p(uv, fp), _p(view, _ip),
                                           _p(score, lp) if want_score else None, C.byref(n_textured), _p(stats, lp)))
    return {"atlas": atlas, "uv": uv[:nt].copy(), "view": view[:nt].copy(), "score": score[:nt].copy() if want_score else None,
            "n_textured": int(n_textured.value), "stats": stats}


COLOUR_STATS = ("nodes", "blind", "seam_vertices", "spread_before", "spread_after", "max_offset", "n_clamped", "n_passes")    # stats[0..7]


def mesh_colour_nodes(xyz, tri, images, K, P, view, sample_radius=1, device=0):
    """sfmba_mesh_colour_nodes: a node per distinct (vertex, view) of the contributing triangles and its colour in 1/256 grey level (the
    contract is in include/sfmba.h, "levelling the colours across seams").  Returns a dict: n_nodes, node_vertex int32 [n], node_view
    int32 [n], node_of int32 [m, 3], seen uint8 [n], F int32 [n, 3]."""
    nv, xyz, _, tri = _clean_mesh(xyz, None, tri)
    nt = len(tri)
    view = np.ascontiguousarray(view, dtype=np.int32).reshape(-1)
    if len(view) != nt:
        raise ValueError("one view per triangle")
    views, keep = _tsdf_views(images, K, P, [None] * len(images))
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    cap = max(3 * nt, 1)
    node_vertex, node_view, node_of = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros((max(nt, 1), 3), np.int32)
    seen, F = np.zeros(cap, np.uint8), np.zeros((cap, 3), np.int32)
    n = C.c_int64(0)
    _check(lib().sfmba_mesh_colour_nodes(C.c_int(device), C.c_int64(nv), _opt(xyz, fp), C.c_int64(nt), _opt(tri, _ip), *views[:8], _opt(view, _ip),
                                         C.c_int(sample_radius), C.byref(n), _p(node_vertex, _ip), _p(node_view, _ip), _p(node_of, _ip), _p(seen, bp),
                                         _p(F, _ip)))
    n = int(n.value)
    return {"n_nodes": n, "node_vertex": node_vertex[:n].copy(), "node_view": node_view[:n].copy(), "node_of": node_of[:nt].copy(),
            "seen": seen[:n].copy(), "F": F[:n].copy()}


def mesh_colour_level(node_vertex, seen, F, node_of, seam_weight=16, passes=16, device=0):
    """sfmba_mesh_colour_level: the additive offset of every node after `passes` integer Jacobi passes (the contract is in
    include/sfmba.h).  Returns (g int32 [n, 3] in 1/256 grey level, stats int64 [8], named by COLOUR_STATS)."""
    node_vertex = np.ascontiguousarray(node_vertex, dtype=np.int32).reshape(-1)
    seen = np.ascontiguousarray(seen, dtype=np.uint8).reshape(-1)
    F = np.ascontiguousarray(F, dtype=np.int32).reshape(-1, 3)
    node_of = np.ascontiguousarray(node_of, dtype=np.int32).reshape(-1, 3)
    n = len(node_vertex)
    if len(seen) != n or len(F) != n:
        raise ValueError("node_vertex [n], seen [n] and F [n, 3]")
    g, stats = np.zeros((max(n, 1), 3), np.int32), np.zeros(8, np.int64)
    bp, lp = C.POINTER(C.c_ubyte), C.POINTER(C.c_int64)
    _check(lib().sfmba_mesh_colour_level(C.c_int(device), C.c_int64(n), _opt(node_vertex, _ip), _opt(seen, bp), _opt(F, _ip), C.c_int64(len(node_of)),
                                         _opt(node_of, _ip), C.c_int(seam_weight), C.c_int(passes), _p(g, _ip), _p(stats, lp)))
    return g[:n].copy(), stats


def mesh_texture_levelled(xyz, bgr, tri, images, K, P, view, node_of, g, patch=6, blocks_per_row=None, device=0):
    """sfmba_mesh_texture_levelled: mesh_texture_from_views with the offsets g [n, 3] of the nodes node_of [m, 3] blended into every
    sampled texel (the contract is in include/sfmba.h).  Returns a dict: atlas, uv, n_textured, n_clamped."""
    nv, xyz, bgr, tri = _clean_mesh(xyz, bgr, tri)
    nt = len(tri)
    if blocks_per_row is None:
        blocks_per_row = _default_blocks_per_row(nt)
    view = np.ascontiguousarray(view, dtype=np.int32).reshape(-1)
    node_of = np.ascontiguousarray(node_of, dtype=np.int32).reshape(-1, 3)
    g = np.ascontiguousarray(g, dtype=np.int32).reshape(-1, 3)
    if len(view) != nt or len(node_of) != nt:
        raise ValueError("one view and one row of nodes per triangle")
    views, keep = _tsdf_views(images, K, P, [None] * len(images))
    W, H = mesh_texture_size(nt, patch, blocks_per_row)
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    atlas, uv = np.zeros((H, W, 3), np.uint8), np.zeros((max(nt, 1), 3, 2), np.float32)
    n_textured, n_clamped = C.c_int64(0), C.c_int64(0)
    _check(lib().sfmba_mesh_texture_levelled(C.c_int(device), C.c_int64(nv), _opt(xyz, fp), _opt(bgr, bp), C.c_int64(nt), _opt(tri, _ip), *views[:8],
                                             C.c_int(patch), C.c_int(blocks_per_row), _opt(view, _ip), _opt(node_of, _ip), _opt(g, _ip), C.c_int64(len(g)),
                                             _p(atlas, bp), _p(uv, fp), C.byref(n_textured), C.byref(n_clamped)))
    return {"atlas": atlas, "uv": uv[:nt].copy(), "n_textured": int(n_textured.value), "n_clamped": int(n_clamped.value)}


def mesh_texture_adjust(xyz, bgr, tri, images, K, P, depth_maps, occl_tol, min_area=0, patch=6, blocks_per_row=None, n_candidates=4, rings=4,
                        penalty=256, max_passes=100, sample_radius=1, seam_weight=16, level_passes=16, want_score=True, device=0):
    """sfmba_mesh_texture_adjust: mesh_texture_smooth followed by the seam levelling -- nodes, offsets and the levelled raster in one call,
    everything staying on the device (the contract is in include/sfmba.h).  The defaults 1 / 16 / 16 are first choices that nobody has
    tuned.  Returns mesh_texture_smooth's dict and level_stats int64 [8] (named by COLOUR_STATS)."""
    nv, xyz, bgr, tri = _clean_mesh(xyz, bgr, tri)
    nt = len(tri)
    if blocks_per_row is None:
        blocks_per_row = _default_blocks_per_row(nt)
    views, keep = _tsdf_views(images, K, P, depth_maps)
    W, H = mesh_texture_size(nt, patch, blocks_per_row)
    fp, bp, lp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte), C.POINTER(C.c_int64)
    atlas, uv = np.zeros((H, W, 3), np.uint8), np.zeros((max(nt, 1), 3, 2), np.float32)
    view, score, stats, level_stats = np.zeros(max(nt, 1), np.int32), np.zeros(max(nt, 1), np.int64), np.zeros(8, np.int64), np.zeros(8, np.int64)
    n_textured = C.c_int64(0)
    _check(lib().sfmba_mesh_texture_adjust(C.c_int(device), C.c_int64(nv), _opt(xyz, fp), _opt(bgr, bp), C.c_int64(nt), _opt(tri, _ip), *views,
                                           C.c_float(occl_tol), C.c_int64(min_area), C.c_int(patch), C.c_int(blocks_per_row), C.c_int(n_candidates),
                                           C.c_int(rings), C.c_int(penalty), C.c_int(max_passes), _p(atlas, bp), _p(uv, fp), _p(view, _ip),
                                           _p(score, lp) if want_score else None, C.byref(n_textured), _p(stats, lp), C.c_int(sample_radius),
                                           C.c_int(seam_weight), C.c_int(level_passes), _p(level_stats, lp)))
    return {"atlas": atlas, "uv": uv[:nt].copy(), "view": view[:nt].copy(), "score": score[:nt].copy() if want_score else None,
            "n_textured": int(n_textured.value), "stats": stats, "level_stats": level_stats}


class _ImageInfo(C.Structure):
    _fields_ = [("status", C.c_int), ("width", C.c_int), ("height", C.c_int), ("channels", C.c_int), ("h_samp", C.c_int), ("v_samp", C.c_int),
                ("restart_interval", C.c_int)]


IMAGE_STATUS = ("OK", "UNSUPPORTED", "CORRUPT")          # SFMBA_IMAGE_* by value


def _flat_files(files):
    blobs = [bytes(f) for f in files]
    ptr = np.zeros(len(blobs) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(b) for b in blobs])
    flat = np.frombuffer(b"".join(blobs) or b"\0", dtype=np.uint8).copy()
    return ptr, flat


def _info_dicts(info):
    return [{k: int(getattr(i, k)) for k, _ in _ImageInfo._fields_} for i in info]


def jpeg_info(files):
    """sfmba_jpeg_info: the header fields of every file (bytes objects) as dicts; host only, no device needed."""
    ptr, flat = _flat_files(files)
    info = (_ImageInfo * max(len(files), 1))()
    _check(lib().sfmba_jpeg_info(C.c_int(len(files)), _p(ptr, C.POINTER(C.c_int64)), flat.ctypes.data_as(C.POINTER(C.c_ubyte)), info))
    return _info_dicts(info)[:len(files)]


def resized_size(width, height, factor):
    """sfmba_resized_size: (ow, oh) of the resize rule; host only."""
    ow, oh = C.c_int32(0), C.c_int32(0)
    _check(lib().sfmba_resized_size(C.c_int(width), C.c_int(height), C.c_float(factor), C.byref(ow), C.byref(oh)))
    return ow.value, oh.value


def _split_images(out, out_ptr, shapes):
    return [None if s is None else out[int(out_ptr[i]):int(out_ptr[i + 1])].reshape(s).copy() for i, s in enumerate(shapes)]


def jpeg_decode(files, factor=1.0, cap=None, device=0):
    """sfmba_jpeg_decode: (info dicts, images) for a list of JPEG files (bytes objects).  An image is a uint8 array h x w (gray) or
    h x w x 3 (B, G, R), None where the status is not OK.  cap=None asks for the size first (a call with cap 0)."""
    n = len(files)
    ptr, flat = _flat_files(files)
    lp, bp = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)
    info = (_ImageInfo * max(n, 1))()
    out_ptr = np.zeros(n + 1, dtype=np.int64)
    total = C.c_int64(0)
    cap = 0 if cap is None else int(cap)
    for _ in range(2):
        out = np.zeros(max(cap, 1), np.uint8)
        rc = lib().sfmba_jpeg_decode(C.c_int(device), C.c_int(n), _p(ptr, lp), flat.ctypes.data_as(bp), C.c_float(factor), info, _p(out_ptr, lp),
                                     out.ctypes.data_as(bp), C.c_int64(cap), C.byref(total))
        if rc != SFMBA_ERR_CAPACITY:
            break
        cap = int(total.value)
    _check(rc)
    infos = _info_dicts(info)[:n]
    shapes = []
    for i, d in enumerate(infos):
        if d["status"] != 0:
            shapes.append(None)
            continue
        ow, oh = (d["width"], d["height"]) if factor == 1.0 else resized_size(d["width"], d["height"], factor)
        shapes.append((oh, ow) if d["channels"] == 1 else (oh, ow, 3))
    return infos, _split_images(out, out_ptr, shapes)


def resize_images(images, factor, cap=None, device=0):
    """sfmba_resize_images: the resized uint8 images (all h x w or all h x w x 3) of a batch."""
    imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
    kinds = {(im.ndim, im.shape[2] if im.ndim == 3 else 1) for im in imgs}
    if len(kinds) > 1 or any(k not in ((2, 1), (3, 3)) for k in kinds):
        raise ValueError("images must all be h x w or all be h x w x 3 uint8 arrays")
    channels = kinds.pop()[1] if kinds else 1
    n = len(imgs)
    img_ptr = np.zeros(n + 1, dtype=np.int64)
    img_ptr[1:] = np.cumsum([im.size for im in imgs])
    flat = np.ascontiguousarray(np.concatenate([im.reshape(-1) for im in imgs]) if imgs else np.zeros(1, np.uint8))
    wd = np.asarray([im.shape[1] for im in imgs], dtype=np.int32)
    ht = np.asarray([im.shape[0] for im in imgs], dtype=np.int32)
    lp, bp = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)
    out_ptr = np.zeros(n + 1, dtype=np.int64)
    total = C.c_int64(0)
    cap = 0 if cap is None else int(cap)
    for _ in range(2):
        out = np.zeros(max(cap, 1), np.uint8)
        rc = lib().sfmba_resize_images(C.c_int(device), C.c_int(n), _p(img_ptr, lp), flat.ctypes.data_as(bp), _p(wd, _ip), _p(ht, _ip), C.c_int(channels),
                                       C.c_float(factor), _p(out_ptr, lp), out.ctypes.data_as(bp), C.c_int64(cap), C.byref(total))
        if rc != SFMBA_ERR_CAPACITY:
            break
        cap = int(total.value)
    _check(rc)
    shapes = []
    for im in imgs:
        ow, oh = resized_size(im.shape[1], im.shape[0], factor)
        shapes.append((oh, ow) if channels == 1 else (oh, ow, 3))
    return _split_images(out, out_ptr, shapes)


class _PngInfo(C.Structure):
    _fields_ = [("status", C.c_int), ("width", C.c_int), ("height", C.c_int), ("channels", C.c_int), ("bit_depth", C.c_int), ("colour_type", C.c_int),
                ("interlace", C.c_int)]


def _png_info_dicts(info):
    return [{k: int(getattr(i, k)) for k, _ in _PngInfo._fields_} for i in info]


def png_info(files):
    """sfmba_png_info: the chunk walk of every file (bytes objects) as dicts; host only, no device needed."""
    ptr, flat = _flat_files(files)
    info = (_PngInfo * max(len(files), 1))()
    _check(lib().sfmba_png_info(C.c_int(len(files)), _p(ptr, C.POINTER(C.c_int64)), flat.ctypes.data_as(C.POINTER(C.c_ubyte)), info))
    return _png_info_dicts(info)[:len(files)]


def png_decode(files, factor=1.0, cap=None, device=0):
    """sfmba_png_decode: (info dicts, images) for a list of PNG files (bytes objects).  An image is a uint8 array h x w (colour types 0
    and 4) or h x w x 3 (B, G, R), None where the status is not OK.  cap=None asks for the size first (a call with cap 0)."""
    n = len(files)
    ptr, flat = _flat_files(files)
    lp, bp = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)
    info = (_PngInfo * max(n, 1))()
    out_ptr = np.zeros(n + 1, dtype=np.int64)
    total = C.c_int64(0)
    cap = 0 if cap is None else int(cap)
    for _ in range(2):
        out = np.zeros(max(cap, 1), np.uint8)
        rc = lib().sfmba_png_decode(C.c_int(device), C.c_int(n), _p(ptr, lp), flat.ctypes.data_as(bp), C.c_float(factor), info, _p(out_ptr, lp),
                                    out.ctypes.data_as(bp), C.c_int64(cap), C.byref(total))
        if rc != SFMBA_ERR_CAPACITY:
            break
        cap = int(total.value)
    _check(rc)
    infos = _png_info_dicts(info)[:n]
    shapes = []
    for d in infos:
        if d["status"] != 0:
            shapes.append(None)
            continue
        ow, oh = (d["width"], d["height"]) if factor == 1.0 else resized_size(d["width"], d["height"], factor)
        shapes.append((oh, ow) if d["channels"] == 1 else (oh, ow, 3))
    return infos, _split_images(out, out_ptr, shapes)


class _PnpResult(C.Structure):
    _fields_ = [("status", C.c_int), ("best_hypothesis", C.c_int), ("n_inliers", C.c_int), ("refine_iters", C.c_int), ("refine_cost", C.c_double)]


def pnp_ransac(problems, K, n_hyp=100, threshold_px=10.0, seed=0, max_refine_iters=20, debug=False, device=0):
    """sfmba_pnp_ransac: pose every problem of a batch from its 2D-3D matches (the contract is in include/sfmba.h).

    problems: list of (xyz [n_i, 3], uv [n_i, 2]) -- one per view to register.  K [3, 3].  Returns one dict per problem: status,
    best_hypothesis, n_inliers, refine_iters, refine_cost, pose [3, 4] float64, inlier [n_i] bool; with debug=True also
    hyp_pose [n_hyp, 3, 4] and hyp_count [n_hyp] (every hypothesis' unrefined pose and count, -1 = invalid)."""
    xs = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 3) for x, _ in problems]
    us = [np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 2) for _, u in problems]
    if any(len(x) != len(u) for x, u in zip(xs, us)):
        raise ValueError("xyz and uv of a problem must have the same number of rows")
    n_prob = len(xs)
    ptr = np.zeros(n_prob + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in xs])
    total = int(ptr[-1])
    xyz = np.ascontiguousarray(np.concatenate(xs, axis=0) if xs else np.zeros((0, 3), np.float32))
    uv = np.ascontiguousarray(np.concatenate(us, axis=0) if us else np.zeros((0, 2), np.float32))
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    pose = np.zeros((max(n_prob, 1), 12))
    inl = np.zeros(max(total, 1), dtype=np.uint8)
    res = (_PnpResult * max(n_prob, 1))()
    n_dbg = max(n_prob, 1) * max(int(n_hyp), 1) if debug else 0
    hp = np.zeros((n_dbg, 12)) if debug else None
    hc = np.zeros(n_dbg, dtype=np.int32) if debug else None
    lp, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    _check(lib().sfmba_pnp_ransac(C.c_int(device), C.c_int(n_prob), _p(ptr, lp), _p(xyz, fp), _p(uv, fp), _p(K, fp), C.c_int(n_hyp),
                                  C.c_float(threshold_px), C.c_uint64(seed), C.c_int(max_refine_iters), _p(pose, _dp),
                                  inl.ctypes.data_as(C.POINTER(C.c_ubyte)), res, _p(hp, _dp) if debug else None,
                                  _p(hc, _ip) if debug else None))
    out = []
    for p in range(n_prob):
        d = {k: getattr(res[p], k) for k, _ in _PnpResult._fields_}
        d["pose"] = pose[p].reshape(3, 4).copy()
        d["inlier"] = inl[ptr[p]:ptr[p + 1]].astype(bool)
        if debug:
            d["hyp_pose"] = hp[p * n_hyp:(p + 1) * n_hyp].reshape(n_hyp, 3, 4).copy()
            d["hyp_count"] = hc[p * n_hyp:(p + 1) * n_hyp].copy()
        out.append(d)
    return out


class _HomographyResult(C.Structure):
    _fields_ = [("status", C.c_int), ("best_hypothesis", C.c_int), ("n_inliers", C.c_int), ("n_matches", C.c_int)]


def homography_ransac(pts_per_image, pairs, matches, n_hyp=2000, threshold_px=10.0, seed=0, debug=False, device=0):
    """sfmba_homography_ransac: four-point homography RANSAC for every image pair of a batch (the contract is in include/sfmba.h).

    pts_per_image: list of float32 arrays [n_i, 2] (the key points of every image, pixels).  pairs: list of (left, right) image
    indices, None = all i < j in row-major order.  matches: either the tuple capi.match_features returns as it comes
    (pair_left, pair_right, pair_ptr, query_idx, train_idx, distance) -- `pairs` is then ignored -- or (pair_ptr, query_idx,
    train_idx) for `pairs`.  Returns one dict per pair: status, best_hypothesis, n_inliers, n_matches, H [3, 3] float64,
    inlier [n_p] bool; with debug=True also hyp_H [n_hyp, 3, 3] and hyp_count [n_hyp] (every hypothesis' H and count, -1 = invalid)."""
    ps = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 2) for x in pts_per_image]
    if len(matches) == 6:
        pl, pr, ptr, q, t = matches[:5]
    else:
        if pairs is None:
            pairs = [(i, j) for i in range(len(ps)) for j in range(i + 1, len(ps))]
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        pl, pr = pairs[:, 0], pairs[:, 1]
        ptr, q, t = matches
    pl, pr, q, t = _i(pl), _i(pr), _i(q), _i(t)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    n_pairs = len(pl)
    if len(pr) != n_pairs or len(ptr) != n_pairs + 1 or len(q) != len(t) or (n_pairs and len(q) < ptr[-1]):
        raise ValueError("pair_left / pair_right / pair_ptr / query_idx / train_idx do not fit together")
    img_ptr = np.zeros(len(ps) + 1, dtype=np.int64)
    img_ptr[1:] = np.cumsum([len(x) for x in ps])
    pts = np.ascontiguousarray(np.concatenate(ps, axis=0) if ps else np.zeros((0, 2), np.float32))
    total = int(ptr[-1]) if n_pairs else 0
    H = np.zeros((max(n_pairs, 1), 9))
    inl = np.zeros(max(total, 1), dtype=np.uint8)
    res = (_HomographyResult * max(n_pairs, 1))()
    n_dbg = max(n_pairs, 1) * max(int(n_hyp), 1) if debug else 0
    hh = np.zeros((n_dbg, 9)) if debug else None
    hc = np.zeros(n_dbg, dtype=np.int32) if debug else None
    lp, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    _check(lib().sfmba_homography_ransac(C.c_int(device), C.c_int(len(ps)), _p(img_ptr, lp), _p(pts, fp), C.c_int(n_pairs), _p(pl, _ip),
                                         _p(pr, _ip), _p(ptr, lp), _p(q, _ip), _p(t, _ip), C.c_int(n_hyp), C.c_float(threshold_px),
                                         C.c_uint64(seed), _p(H, _dp), inl.ctypes.data_as(C.POINTER(C.c_ubyte)), res,
                                         _p(hh, _dp) if debug else None, _p(hc, _ip) if debug else None))
    out = []
    for p in range(n_pairs):
        d = {k: getattr(res[p], k) for k, _ in _HomographyResult._fields_}
        d["H"] = H[p].reshape(3, 3).copy()
        d["inlier"] = inl[ptr[p]:ptr[p + 1]].astype(bool)
        if debug:
            d["hyp_H"] = hh[p * n_hyp:(p + 1) * n_hyp].reshape(n_hyp, 3, 3).copy()
            d["hyp_count"] = hc[p * n_hyp:(p + 1) * n_hyp].copy()
        out.append(d)
    return out


class _EssentialResult(C.Structure):
    _fields_ = [("status", C.c_int), ("best_hypothesis", C.c_int), ("n_inliers", C.c_int), ("n_pose_inliers", C.c_int),
                ("pose_candidate", C.c_int), ("n_matches", C.c_int)]


def essential_ransac(pts_per_image, pairs, matches, K, n_hyp=1000, threshold_px=1.0, seed=0, debug=False, device=0):
    """sfmba_essential_ransac: five-point essential-matrix RANSAC + recoverPose for every image pair of a batch (the contract is in
    include/sfmba.h).

    pts_per_image, pairs, matches: as homography_ransac takes them.  K [3, 3].  Returns one dict per pair: status, best_hypothesis,
    n_inliers, n_pose_inliers, pose_candidate, n_matches, E [3, 3] float64, pose [3, 4] float64 ([R|t]), inlier [n_p] bool (the
    winner's mask AND in front for the pose); with debug=True also hyp_E [n_hyp, 3, 3], hyp_count [n_hyp] (-1 = invalid) and
    hyp_nsol [n_hyp] (every hypothesis' E, count and number of real solutions)."""
    ps = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 2) for x in pts_per_image]
    if len(matches) == 6:
        pl, pr, ptr, q, t = matches[:5]
    else:
        if pairs is None:
            pairs = [(i, j) for i in range(len(ps)) for j in range(i + 1, len(ps))]
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        pl, pr = pairs[:, 0], pairs[:, 1]
        ptr, q, t = matches
    pl, pr, q, t = _i(pl), _i(pr), _i(q), _i(t)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    n_pairs = len(pl)
    if len(pr) != n_pairs or len(ptr) != n_pairs + 1 or len(q) != len(t) or (n_pairs and len(q) < ptr[-1]):
        raise ValueError("pair_left / pair_right / pair_ptr / query_idx / train_idx do not fit together")
    img_ptr = np.zeros(len(ps) + 1, dtype=np.int64)
    img_ptr[1:] = np.cumsum([len(x) for x in ps])
    pts = np.ascontiguousarray(np.concatenate(ps, axis=0) if ps else np.zeros((0, 2), np.float32))
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    total = int(ptr[-1]) if n_pairs else 0
    E = np.zeros((max(n_pairs, 1), 9))
    pose = np.zeros((max(n_pairs, 1), 12))
    inl = np.zeros(max(total, 1), dtype=np.uint8)
    res = (_EssentialResult * max(n_pairs, 1))()
    n_dbg = max(n_pairs, 1) * max(int(n_hyp), 1) if debug else 0
    he = np.zeros((n_dbg, 9)) if debug else None
    hc = np.zeros(n_dbg, dtype=np.int32) if debug else None
    hn = np.zeros(n_dbg, dtype=np.int32) if debug else None
    lp, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    _check(lib().sfmba_essential_ransac(C.c_int(device), C.c_int(len(ps)), _p(img_ptr, lp), _p(pts, fp), C.c_int(n_pairs), _p(pl, _ip),
                                        _p(pr, _ip), _p(ptr, lp), _p(q, _ip), _p(t, _ip), _p(K, fp), C.c_int(n_hyp), C.c_float(threshold_px),
                                        C.c_uint64(seed), _p(E, _dp), _p(pose, _dp), inl.ctypes.data_as(C.POINTER(C.c_ubyte)), res,
                                        _p(he, _dp) if debug else None, _p(hc, _ip) if debug else None, _p(hn, _ip) if debug else None))
    out = []
    for p in range(n_pairs):
        d = {k: getattr(res[p], k) for k, _ in _EssentialResult._fields_}
        d["E"] = E[p].reshape(3, 3).copy()
        d["pose"] = pose[p].reshape(3, 4).copy()
        d["inlier"] = inl[ptr[p]:ptr[p + 1]].astype(bool)
        if debug:
            d["hyp_E"] = he[p * n_hyp:(p + 1) * n_hyp].reshape(n_hyp, 3, 3).copy()
            d["hyp_count"] = hc[p * n_hyp:(p + 1) * n_hyp].copy()
            d["hyp_nsol"] = hn[p * n_hyp:(p + 1) * n_hyp].copy()
        out.append(d)
    return out


def release_cache():
    """Return the device memory cached from destroyed problems to HIP; bytes released."""
    return int(lib().sfmba_release_cache())


class _KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("total_us", C.c_double), ("launches", C.c_int64)]


class SfmbaError(RuntimeError):
    pass


def _let_torch_open_the_device_first():
    """A torch wheel bundles its own HIP / HSA runtime beside the system one this library links against.  One process can hold both as
    long as torch's opens the device FIRST (every bench / sharded run does: torch.cuda.set_device comes before the first solve); the
    other way round torch.cuda then reports 'No HIP GPUs are available' -- e.g. a pytest selection that runs a plain C-ABI test before
    the first sharded one.  So: when torch is installed and sees a GPU, let it initialise before libsfmba_hip.so is loaded.  Nothing
    happens without torch or without a GPU; the C ABI itself never needs torch."""
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass


def lib():
    global _lib
    if _lib is None:
        _let_torch_open_the_device_first()
        if not os.path.exists(LIB_PATH):
            raise SfmbaError("%s is missing: build it with `make -C %s` (or __graft_entry__.build()); "
                             "the MI355X back end has no CPU fallback" % (LIB_PATH, os.path.dirname(LIB_PATH)))
        L = C.CDLL(LIB_PATH)
        L.sfmba_last_error.restype = C.c_char_p
        L.sfmba_problem_stream.restype = C.c_void_p
        L.sfmba_shard_reduce_buf.restype = C.c_void_p
        L.sfmba_shard_scalars_buf.restype = C.c_void_p
        L.sfmba_shard_reduce_len.restype = C.c_int64
        L.sfmba_shard_setup_len.restype = C.c_int64
        L.sfmba_shard_setup_buf.restype = C.c_void_p
        L.sfmba_release_cache.restype = C.c_longlong
        for name in ("sfmba_problem_reset", "sfmba_problem_set_params", "sfmba_problem_solve", "sfmba_problem_get_params",
                     "sfmba_problem_destroy", "sfmba_problem_stream", "sfmba_problem_reduced_dim", "sfmba_problem_append",
                     "sfmba_problem_eval_residuals", "sfmba_problem_eval_jacobian", "sfmba_problem_build_reduced",
                     "sfmba_shard_begin", "sfmba_shard_reduce_len", "sfmba_shard_reduce_buf", "sfmba_shard_scalars_buf",
                     "sfmba_shard_partial_build", "sfmba_shard_solve_update", "sfmba_shard_finish", "sfmba_shard_end"):
            getattr(L, name).argtypes = None
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise SfmbaError("sfmba rc=%d: %s" % (rc, (lib().sfmba_last_error() or b"").decode()))


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a, t):
    return a.ctypes.data_as(t)


def device_count():
    return int(lib().sfmba_device_count())


def device_warmup(device=0, expected_obs=0):
    """sfmba_device_warmup: pay the process-wide first-call costs (HIP context, pinned pool, device chunks) now."""
    _check(lib().sfmba_device_warmup(C.c_int(device), C.c_int64(expected_obs)))


def default_options(**overrides):
    o = SfmbaOptions()
    lib().sfmba_options_default(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _trace_rows(trace, n, cap):
    return [trace[i].as_dict() for i in range(min(n, cap))]


def solve(prob, opt=None, trace_cap=1024):
    """One-shot sfmba_solve on host arrays.  Returns (cam6, pt3, focal, summary, trace); prob untouched."""
    cam6, pt3 = _d(prob.cam6).copy(), _d(prob.pt3).copy()
    oc, op, oxy = _i(prob.obs_cam), _i(prob.obs_pt), _d(prob.obs_xy)
    focal = C.c_double(prob.focal)
    opt = opt or default_options()
    summ = SfmbaSummary()
    trace = (SfmbaIteration * trace_cap)()
    tl = C.c_int(0)
    _check(lib().sfmba_solve(C.c_int(prob.n_cam), _p(cam6, _dp), C.c_int(prob.n_pt), _p(pt3, _dp), C.c_int64(prob.n_obs),
                             _p(oc, _ip), _p(op, _ip), _p(oxy, _dp), C.byref(focal), C.byref(opt), C.byref(summ),
                             trace, C.c_int(trace_cap), C.byref(tl)))
    return cam6, pt3, focal.value, summ.as_dict(), _trace_rows(trace, tl.value, trace_cap)


def dense_spd_solve(A, b, method=0, tol=1e-12, max_iters=0, device=0):
    A, b = _d(A), _d(b)
    n = b.shape[0]
    x = np.zeros(n)
    info, iters = C.c_int(0), C.c_int(0)
    _check(lib().sfmba_dense_spd_solve(C.c_int(device), C.c_int(n), _p(A, _dp), _p(b, _dp), _p(x, _dp), C.c_int(method),
                                       C.c_double(tol), C.c_int(max_iters), C.byref(info), C.byref(iters)))
    return x, info.value, iters.value


PCG_PROBE_SYMMETRIC, PCG_PROBE_F32_MATRIX, PCG_PROBE_SEGMENTS, PCG_PROBE_POISON = 1, 2, 4, 8


def dense_pcg_probe(A, B, Wt=None, flags=0, tol=1e-10, max_iters=200, device=0):
    """sfmba_dense_pcg_probe: the reduced-system CG on A [n, n] for the right-hand sides B [nrhs, n] (or [n]), one after another on one workspace.
    Wt: None or [8, n] coarse vectors in the transformed unknowns; flags: PCG_PROBE_*; max_iters: one int or one per right-hand side.
    Returns (X [nrhs, n], info, iters [nrhs], path dict: family, family_name, f32_matrix, coarse_vectors, cg_iters)."""
    A = _d(A)
    B = np.ascontiguousarray(np.atleast_2d(np.asarray(B, dtype=np.float64)))
    nrhs, n = B.shape
    if A.shape != (n, n) or (Wt is not None and np.shape(Wt) != (8, n)):
        raise ValueError("A, B and Wt do not fit together")
    W = None if Wt is None else np.ascontiguousarray(Wt, dtype=np.float64)
    mi = _i(np.broadcast_to(np.asarray(max_iters, dtype=np.int32), (nrhs,)))
    X = np.zeros((nrhs, n))
    info, iters, path = C.c_int(0), np.zeros(nrhs, dtype=np.int32), _StepProbe()
    _check(lib().sfmba_dense_pcg_probe(C.c_int(device), C.c_int(n), _p(A, _dp), C.c_int(nrhs), _p(B, _dp), None if W is None else _p(W, _dp),
                                       C.c_int(flags), C.c_double(tol), _p(mi, _ip), _p(X, _dp), C.byref(info), _p(iters, _ip), C.byref(path)))
    out = {k: int(getattr(path, k)) for k, _ in _StepProbe._fields_}
    out["family_name"] = FAMILIES[out["family"]] if 0 <= out["family"] < len(FAMILIES) else str(out["family"])
    return X, info.value, iters.copy(), out


DCG_PROBE_F32, DCG_PROBE_POISON = 1, 2


def dist_cg_probe(A, world, B, Wt=None, flags=0, tol=1e-10, max_iters=200, surplus=0, device=0):
    """sfmba_dist_cg_probe: the distributed CG on A [n, n], n = 6 ncam + 1, with every rank of a world of `world` ranks simulated in this process,
    for the right-hand sides B [nrhs, n] (or [n]) one after another.  Wt: None or [8, n] coarse vectors in the transformed unknowns; flags:
    DCG_PROBE_*; max_iters: one int or one per right-hand side; surplus: further launches behind the end of every solve.
    Returns a dict: Xt [nrhs, n] (rank 0's solution in the TRANSFORMED unknowns), info, iters [nrhs], rows [world + 1], chunk_blocks,
    replicas_differ (0, or the number of the first check at which a rank's replicated state differed from rank 0's)."""
    A = _d(A)
    B = np.ascontiguousarray(np.atleast_2d(np.asarray(B, dtype=np.float64)))
    nrhs, n = B.shape
    if A.shape != (n, n) or (Wt is not None and np.shape(Wt) != (8, n)):
        raise ValueError("A, B and Wt do not fit together")
    W = None if Wt is None else np.ascontiguousarray(Wt, dtype=np.float64)
    mi = _i(np.broadcast_to(np.asarray(max_iters, dtype=np.int32), (nrhs,)))
    Xt = np.zeros((nrhs, n))
    info, differ, chunk = C.c_int(0), C.c_int(0), C.c_longlong(0)
    iters, rows = np.zeros(nrhs, dtype=np.int32), np.zeros(max(int(world), 0) + 1, dtype=np.int32)
    _check(lib().sfmba_dist_cg_probe(C.c_int(device), C.c_int(n), _p(A, _dp), C.c_int(world), C.c_int(nrhs), _p(B, _dp), None if W is None else _p(W, _dp),
                                     C.c_int(flags), C.c_double(tol), _p(mi, _ip), C.c_int(surplus), _p(Xt, _dp), C.byref(info), _p(iters, _ip),
                                     _p(rows, _ip), C.byref(chunk), C.byref(differ)))
    return {"Xt": Xt, "info": info.value, "iters": iters.copy(), "rows": [int(r) for r in rows], "chunk_blocks": int(chunk.value),
            "replicas_differ": differ.value}


class Problem:
    """Device-resident problem (sfmba_problem_*)."""

    def __init__(self, prob, precision=0, device=0, flags=0):
        """flags: SFMBA_CREATE_* (structs.CREATE_DETERMINISTIC); 0 goes through plain sfmba_problem_create."""
        self.n_cam, self.n_pt, self.n_obs = prob.n_cam, prob.n_pt, prob.n_obs
        cam6, pt3 = _d(prob.cam6), _d(prob.pt3)
        oc, op, oxy = _i(prob.obs_cam), _i(prob.obs_pt), _d(prob.obs_xy)
        self._h = C.c_void_p()
        self._template = (cam6.copy(), pt3.copy())
        if flags:
            _check(lib().sfmba_problem_create_ex(C.c_int(device), C.c_int(precision), C.c_int(flags), C.c_int(prob.n_cam), _p(cam6, _dp),
                                                 None, C.c_int(prob.n_pt), _p(pt3, _dp), C.c_int64(prob.n_obs), _p(oc, _ip), _p(op, _ip),
                                                 _p(oxy, _dp), C.c_double(prob.focal), C.c_int(0), C.c_int(1), C.byref(self._h)))
        else:
            _check(lib().sfmba_problem_create(C.c_int(device), C.c_int(precision), C.c_int(prob.n_cam), _p(cam6, _dp),
                                              C.c_int(prob.n_pt), _p(pt3, _dp), C.c_int64(prob.n_obs), _p(oc, _ip), _p(op, _ip),
                                              _p(oxy, _dp), C.c_double(prob.focal), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().sfmba_problem_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        return lib().sfmba_problem_stream(self._h)

    @property
    def reduced_dim(self):
        return int(lib().sfmba_problem_reduced_dim(self._h))

    def reset(self):
        _check(lib().sfmba_problem_reset(self._h))

    def set_params(self, cam6, pt3, focal):
        cam6, pt3 = _d(cam6), _d(pt3)
        _check(lib().sfmba_problem_set_params(self._h, _p(cam6, _dp), _p(pt3, _dp), C.c_double(focal)))

    def append(self, cam6, pt3, focal, obs_cam, obs_pt, obs_xy):
        """sfmba_problem_append: grow the resident problem by new observations (and, at the end of the arrays, new cameras /
        points); cam6 / pt3 are the FULL current parameter arrays."""
        cam6, pt3 = _d(cam6), _d(pt3)
        oc, op, oxy = _i(obs_cam), _i(obs_pt), _d(obs_xy)
        _check(lib().sfmba_problem_append(self._h, C.c_int(cam6.shape[0]), _p(cam6, _dp), C.c_int(pt3.shape[0]), _p(pt3, _dp),
                                          C.c_int64(len(oc)), _p(oc, _ip), _p(op, _ip), _p(oxy, _dp), C.c_double(focal)))
        self.n_cam, self.n_pt, self.n_obs = cam6.shape[0], pt3.shape[0], self.n_obs + len(oc)
        self._template = (cam6.copy(), pt3.copy())

    def get_params(self):
        cam6, pt3 = self._template[0].copy(), self._template[1].copy()
        focal = C.c_double(0.0)
        _check(lib().sfmba_problem_get_params(self._h, _p(cam6, _dp), _p(pt3, _dp), C.byref(focal)))
        return cam6, pt3, focal.value

    def solve(self, opt=None, trace_cap=1024):
        opt = opt or default_options()
        summ = SfmbaSummary()
        # the trace buffer is kept with the handle: allocating (and zeroing) 64 KB of ctypes array per call is measurable
        # next to a ~1 ms solve
        if getattr(self, "_trace_cap", 0) != trace_cap:
            self._trace = (SfmbaIteration * trace_cap)()
            self._trace_cap = trace_cap
        trace = self._trace
        tl = C.c_int(0)
        _check(lib().sfmba_problem_solve(self._h, C.byref(opt), C.byref(summ), trace, C.c_int(trace_cap), C.byref(tl)))
        return summ.as_dict(), _trace_rows(trace, tl.value, trace_cap)

    def set_profiling(self, enable):
        _check(lib().sfmba_problem_set_profiling(self._h, C.c_int(1 if enable else 0)))

    def get_profile(self):
        """{kernel: {total_us, launches, avg_us}} measured with HIP events on the solver's stream."""
        buf = (_KernelTime * 64)()
        n = C.c_int(0)
        _check(lib().sfmba_problem_get_profile(self._h, buf, C.c_int(64), C.byref(n)))
        out = {}
        for i in range(min(n.value, 64)):
            k = buf[i]
            out[k.name.decode()] = dict(total_us=k.total_us, launches=int(k.launches), avg_us=k.total_us / max(1, k.launches))
        return out

    def set_step_probe(self, enable):
        """Record the step of every back-substitution (a test hook; off = nothing allocated, nothing stored)."""
        _check(lib().sfmba_problem_set_step_probe(self._h, C.c_int(1 if enable else 0)))

    def step_probe(self):
        """(z, dpt, info) of the last back-substitution: z in build_reduced's unknowns, dpt the point step in caller order."""
        return get_step_probe(self._h, self.reduced_dim, self.n_pt)

    def eval_residuals(self):
        res = np.zeros(2 * self.n_obs)
        cost = C.c_double(0.0)
        _check(lib().sfmba_problem_eval_residuals(self._h, _p(res, _dp), C.byref(cost)))
        return res.reshape(-1, 2), cost.value

    def eval_jacobian(self):
        n = self.n_obs
        jc, jp, jf = np.zeros(12 * n), np.zeros(6 * n), np.zeros(2 * n)
        _check(lib().sfmba_problem_eval_jacobian(self._h, _p(jc, _dp), _p(jp, _dp), _p(jf, _dp)))
        return jc.reshape(n, 2, 6), jp.reshape(n, 2, 3), jf.reshape(n, 2)

    def build_reduced(self, radius, opt=None):
        d = self.reduced_dim
        S, rhs, scale = np.zeros(d * d), np.zeros(d), np.zeros(d)
        opt = opt or default_options()
        _check(lib().sfmba_problem_build_reduced(self._h, C.byref(opt), C.c_double(radius), _p(S, _dp), _p(rhs, _dp), _p(scale, _dp)))
        return S.reshape(d, d), rhs, scale
