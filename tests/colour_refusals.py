"""Every argument refusal of the four levelling calls (the contract is in include/sfmba.h, "levelling the colours across seams") as a list
of calls -- TEST INFRASTRUCTURE ONLY.  Each case is the valid call with exactly one thing wrong; the outputs are filled with 0xA5 bytes
before the call.  refusal_calls gives (name, call) pairs; call() returns (rc, untouched).  The refusals that the library finds before it
opens the device run in the CPU suite too; a triangle index outside the vertex list and a view outside the images are found on the
device."""
import ctypes as C

import numpy as np

import colour_oracle as co
import label_refusals as lr
import texture_refusals as tr

FILL = tr.FILL
VIEWS = lr.VIEWS
NAMES = {
    "sfmba_mesh_colour_nodes": ("device", "n_vertices", "xyz", "n_triangles", "tri") + VIEWS + ("view_in", "sample_radius", "n_nodes_out", "node_vertex",
                                                                                              "node_view", "node_of", "seen", "F"),
    "sfmba_mesh_colour_level": ("device", "n_nodes", "node_vertex_in", "seen_in", "F_in", "n_triangles", "node_of_in", "seam_weight", "passes", "g", "stats"),
    "sfmba_mesh_texture_levelled": ("device", "n_vertices", "xyz", "bgr", "n_triangles", "tri") + VIEWS + ("patch", "blocks_per_row", "view_in", "node_of_in",
                                                                                                           "g_in", "n_nodes", "atlas", "uv", "n_textured", "n_clamped"),
    "sfmba_mesh_texture_adjust": lr.NAMES["sfmba_mesh_texture_smooth"] + ("sample_radius", "seam_weight", "level_passes", "level_stats"),
}
OUTPUTS = {
    "sfmba_mesh_colour_nodes": ("n_nodes_out", "node_vertex", "node_view", "node_of", "seen", "F"),
    "sfmba_mesh_colour_level": ("g", "stats"),
    "sfmba_mesh_texture_levelled": ("atlas", "uv", "n_textured", "n_clamped"),
    "sfmba_mesh_texture_adjust": ("atlas", "uv", "view", "score", "n_textured", "stats", "level_stats"),
}
FLOATS, LONGS = ("occl_tol",), ("n_vertices", "n_triangles", "min_area", "n_nodes")


def valid(entry):
    """the arguments of a valid call by name (the texture suite's four views, the labels of the plain rule)"""
    a = lr.valid("sfmba_mesh_texture_smooth")
    nt = a["n_triangles"]
    view = np.ascontiguousarray(lr.valid("sfmba_mesh_texture_from_views")["view_in"])
    nd = co.nodes(a["xyz"], a["tri"], lr._images(a), a["K"], a["P"], view, 1)
    g, _ = co.level(nd["node_vertex"], nd["seen"], nd["F"], nd["node_of"], 16, 4)
    n = nd["n_nodes"]
    a.update(view_in=view.copy(), sample_radius=1, seam_weight=16, passes=4, level_passes=4, n_nodes=n, n_nodes_out=tr._filled(1, np.int64),
             node_vertex=tr._filled(3 * nt, np.int32), node_view=tr._filled(3 * nt, np.int32), node_of=tr._filled((nt, 3), np.int32),
             seen=tr._filled(3 * nt, np.uint8), F=tr._filled((3 * nt, 3), np.int32), node_vertex_in=nd["node_vertex"].copy(), seen_in=nd["seen"].copy(),
             F_in=nd["F"].copy(), node_of_in=nd["node_of"].copy(), g_in=g.copy(), g=tr._filled((n, 3), np.int32), stats=tr._filled(8, np.int64),
             level_stats=tr._filled(8, np.int64), n_clamped=tr._filled(1, np.int64))
    return {k: a[k] for k in NAMES[entry]}


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


_set, _at, _null = tr._set, tr._at, lr._null


def _partly(a):
    row = int(np.argmax(a["node_of_in"][:, 0] >= 0))
    _at("node_of_in", 3 * row + 1, -1)(a)


RADIUS_DEFECTS = [("sample_radius negative", _set("sample_radius", -1)), ("sample_radius 3", _set("sample_radius", 3))]
WEIGHT_DEFECTS = [("seam_weight 0", _set("seam_weight", 0)), ("seam_weight 257", _set("seam_weight", 257)), ("seam_weight negative", _set("seam_weight", -16))]
ROW_DEFECTS = [("node_of -2", _at("node_of_in", 4, -2)), ("node_of n_nodes", lambda a: _at("node_of_in", 5, a["n_nodes"])(a)),
               ("a row partly -1", _partly)]
NO_DEPTH = [d for d in tr.VIEW_DEFECTS if d[0] != "depth NULL"]
# found on the device
GIVEN_DEFECTS = lr.GIVEN_DEFECTS


def table(device_cases=False):
    index = tr.INDEX_DEFECTS if device_cases else []
    given = GIVEN_DEFECTS if device_cases else []
    return [
        ("sfmba_mesh_colour_nodes", tr.MESH_DEFECTS + NO_DEPTH + RADIUS_DEFECTS + lr.COUNT_DEFECTS[1:2] +
         _null("view_in", "n_nodes_out", "node_vertex", "node_view", "node_of", "seen", "F") + index + given),
        ("sfmba_mesh_colour_level", lr.COUNT_DEFECTS + WEIGHT_DEFECTS + ROW_DEFECTS +
         [("passes negative", _set("passes", -1)), ("passes 1025", _set("passes", 1025)), ("n_nodes negative", _set("n_nodes", -1)),
          ("node_vertex decreases", lambda a: _at("node_vertex_in", 3, int(a["node_vertex_in"][2]) - 1)(a)), ("F negative", _at("F_in", 7, -1)),
          ("F 65281", _at("F_in", 8, 65281))] + _null("node_vertex_in", "seen_in", "F_in", "node_of_in", "g", "stats")),
        ("sfmba_mesh_texture_levelled", tr.LAYOUT_DEFECTS + tr.MESH_DEFECTS + NO_DEPTH + ROW_DEFECTS +
         [("g 65281", _at("g_in", 2, 65281)), ("g -65281", _at("g_in", 4, -65281)), ("n_nodes negative", _set("n_nodes", -1))] +
         _null("view_in", "node_of_in", "g_in", "atlas", "uv", "n_textured", "n_clamped") + index + given),
        ("sfmba_mesh_texture_adjust", tr.LAYOUT_DEFECTS + tr.MESH_DEFECTS + tr.VIEW_DEFECTS + tr.PARAM_DEFECTS + tr.OUT_DEFECTS + lr.K_DEFECTS + lr.PARAM_DEFECTS +
         RADIUS_DEFECTS + WEIGHT_DEFECTS + [("level_passes negative", _set("level_passes", -1)), ("level_passes 1025", _set("level_passes", 1025))] +
         _null("stats", "level_stats") + index),
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
