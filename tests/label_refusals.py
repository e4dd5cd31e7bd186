"""Every argument refusal of the five label calls (the contract is in include/sfmba.h, "smoothing the view labels") as a list of calls --
TEST INFRASTRUCTURE ONLY.  Each case is the valid call with exactly one thing wrong; the outputs are filled with 0xA5 bytes before the
call.  refusal_calls gives (name, call) pairs; call() returns (rc, untouched).  The refusals that the library finds before it opens the
device run in the CPU suite too; a triangle index outside the vertex list and a given view outside the images are found on the device."""
import ctypes as C

import numpy as np

import label_oracle as lo
import texture_refusals as tr

FILL = tr.FILL
VIEWS = ("n_images", "img_ptr", "pixels", "width", "height", "channels", "K", "P")
NAMES = {
    "sfmba_mesh_view_candidates": ("device", "n_vertices", "xyz", "n_triangles", "tri") + VIEWS + ("depth", "occl_tol", "min_area", "n_candidates", "cand_view",
                                                                                                  "cand_score"),
    "sfmba_mesh_adjacency": ("device", "n_triangles", "tri", "adj", "n_pairs", "n_open_edges", "n_nonmanifold_edges"),
    "sfmba_mesh_view_smooth": ("device", "n_triangles", "n_images", "n_candidates", "cand_view_in", "cand_score_in", "adj_in", "rings", "penalty", "max_passes",
                               "view", "stats"),
    "sfmba_mesh_texture_from_views": ("device", "n_vertices", "xyz", "bgr", "n_triangles", "tri") + VIEWS + ("patch", "blocks_per_row", "view_in", "atlas", "uv",
                                                                                                             "n_textured"),
    "sfmba_mesh_texture_smooth": tr.TEXTURE[:19] + ("n_candidates", "rings", "penalty", "max_passes") + tr.TEXTURE[19:] + ("stats",),
}
OUTPUTS = {
    "sfmba_mesh_view_candidates": ("cand_view", "cand_score"),
    "sfmba_mesh_adjacency": ("adj", "n_pairs", "n_open_edges", "n_nonmanifold_edges"),
    "sfmba_mesh_view_smooth": ("view", "stats"),
    "sfmba_mesh_texture_from_views": ("atlas", "uv", "n_textured"),
    "sfmba_mesh_texture_smooth": ("atlas", "uv", "view", "score", "n_textured", "stats"),
}
FLOATS, LONGS = ("occl_tol",), ("n_vertices", "n_triangles", "min_area")
K_VALID = 4


def valid(entry):
    """the arguments of a valid call by name (the texture suite's four views)"""
    a = tr.valid("sfmba_mesh_texture")
    nt, n = a["n_triangles"], a["n_images"]
    cv, cs = lo.candidates_np(a["xyz"], a["tri"], _images(a), a["K"], a["P"], a["depth"], a["occl_tol"], a["min_area"], K_VALID)
    adj = lo.adjacency_sort(a["tri"])[0]
    a.update(n_candidates=K_VALID, rings=2, penalty=256, max_passes=10, cand_view=tr._filled((nt, K_VALID), np.int32),
             cand_score=tr._filled((nt, K_VALID), np.int64), adj=tr._filled((nt, 3), np.int32), n_pairs=tr._filled(1, np.int64),
             n_open_edges=tr._filled(1, np.int64), n_nonmanifold_edges=tr._filled(1, np.int64), stats=tr._filled(8, np.int64),
             cand_view_in=cv.copy(), cand_score_in=cs.copy(), adj_in=adj.copy(), view_in=np.ascontiguousarray(cv[:, 0]).copy())
    return {k: a[k] for k in NAMES[entry]}


def _images(a):
    out = []
    for i in range(a["n_images"]):
        w, h = int(a["width"][i]), int(a["height"][i])
        out.append(a["pixels"][int(a["img_ptr"][i]):int(a["img_ptr"][i + 1])].reshape(h, w, a["channels"]))
    return out


def invoke(lib, entry, a):
    """(rc, untouched) of one call with the named arguments `a`"""
    keep, args = [], []
    for k in NAMES[entry]:
        v = a[k]
        if v is None:
            args.append(None)
        elif k == "depth":
            fp = C.POINTER(C.c_float)
            ptrs = (fp * max(len(v), 1))(*[None if m is None else m.ctypes.data_as(fp) for m in v])
            keep.append(ptrs)
            args.append(ptrs)
        elif isinstance(v, np.ndarray):
            keep.append(v)
            args.append(C.c_void_p(v.ctypes.data))
        elif k in FLOATS:
            args.append(C.c_float(v))
        elif k in LONGS:
            args.append(C.c_int64(v))
        else:
            args.append(C.c_int(v))
    rc = getattr(lib, entry)(*args)
    untouched = all(a[k] is None or (a[k].view(np.uint8) == FILL).all() for k in OUTPUTS[entry])
    return rc, untouched


_set, _at = tr._set, tr._at
T_LIMIT = ((1 << 31) + 2) // 3                                     # the least n_triangles with 3 T >= 2^31
K_DEFECTS = [("n_candidates 0", _set("n_candidates", 0)), ("n_candidates 9", _set("n_candidates", 9)), ("n_candidates negative", _set("n_candidates", -4))]
PARAM_DEFECTS = [
    ("rings negative", _set("rings", -1)), ("rings 9", _set("rings", 9)), ("penalty negative", _set("penalty", -1)), ("penalty 65536", _set("penalty", 65536)),
    ("max_passes negative", _set("max_passes", -1)), ("max_passes 10001", _set("max_passes", 10001)),
]
COUNT_DEFECTS = [("n_triangles negative", _set("n_triangles", -1)), ("3 n_triangles 2^31", _set("n_triangles", T_LIMIT)), ("n_triangles 2^31", _set("n_triangles", 1 << 31))]


def _null(*keys):
    return [("%s NULL" % k, _set(k, None)) for k in keys]


LIST_DEFECTS = [
    ("adj -2", _at("adj_in", 4, -2)), ("adj n_triangles", lambda a: _at("adj_in", 7, a["n_triangles"])(a)), ("cand_view -2", _at("cand_view_in", 0, -2)),
    ("cand_view n_images", lambda a: _at("cand_view_in", 0, a["n_images"])(a)), ("a score of 0 with a view", _at("cand_score_in", 0, 0)),
    ("a negative score", _at("cand_score_in", 0, -5)), ("a score of 2^37", _at("cand_score_in", 0, 1 << 37)),
    ("ascending scores", lambda a: _at("cand_score_in", 1, int(a["cand_score_in"].reshape(-1)[0]) + 1)(a)),
    ("a view after a gap", lambda a: (_at("cand_view_in", 0, -1)(a), _at("cand_score_in", 0, 0)(a))),
    ("a score without a view", lambda a: (_at("cand_view_in", K_VALID - 1, -1)(a), _at("cand_score_in", K_VALID - 1, 3)(a))),
    ("n_images negative", _set("n_images", -1)),
]
# found on the device
GIVEN_DEFECTS = [("a view of n_images", lambda a: _at("view_in", 3, a["n_images"])(a)), ("a view of -2", _at("view_in", -1, -2))]


def table(device_cases=False):
    index = tr.INDEX_DEFECTS if device_cases else []
    return [
        ("sfmba_mesh_view_candidates", tr.MESH_DEFECTS + tr.VIEW_DEFECTS + tr.PARAM_DEFECTS + K_DEFECTS + _null("cand_view", "cand_score") + index),
        ("sfmba_mesh_adjacency", COUNT_DEFECTS + [("a negative index", _at("tri", 7, -1))] + _null("tri", "adj", "n_pairs", "n_open_edges", "n_nonmanifold_edges")),
        ("sfmba_mesh_view_smooth", COUNT_DEFECTS + K_DEFECTS + PARAM_DEFECTS + LIST_DEFECTS + _null("cand_view_in", "cand_score_in", "adj_in", "view", "stats")),
        ("sfmba_mesh_texture_from_views", tr.LAYOUT_DEFECTS + tr.MESH_DEFECTS + [d for d in tr.VIEW_DEFECTS if d[0] != "depth NULL"] +
         _null("view_in", "atlas", "uv", "n_textured") + (index + GIVEN_DEFECTS if device_cases else [])),
        ("sfmba_mesh_texture_smooth", tr.LAYOUT_DEFECTS + tr.MESH_DEFECTS + tr.VIEW_DEFECTS + tr.PARAM_DEFECTS + tr.OUT_DEFECTS + K_DEFECTS + PARAM_DEFECTS +
         _null("stats") + index),
    ]


def refusal_calls(capi, device_cases=False):
    lib = capi.lib()
    out = []
    for entry, defects in table(device_cases):
        for what, spoil in defects:
            def call(entry=entry, spoil=spoil):
                a = valid(entry)
                spoil(a)
                return invoke(lib, entry, a)
            out.append(("%s: %s" % (entry, what), call))
    return out


def valid_call(capi, entry):
    return invoke(capi.lib(), entry, valid(entry))
