"""Every argument refusal of sfmba_mesh_components / sfmba_mesh_filter / sfmba_mesh_smooth / sfmba_mesh_clean (the contract is in
include/sfmba.h) as a list of calls -- TEST INFRASTRUCTURE ONLY.  Each case is the valid call of its entry point with exactly one
thing wrong; the outputs are filled with 0xA5 bytes before the call.  refusal_calls gives (name, call) pairs; call() returns
(rc, untouched).  The refusals that the library finds before it opens the device run in the CPU suite too; a triangle index outside
the vertex list and a coordinate out of range are found on the device."""
import ctypes as C

import numpy as np

import mesh_clean_cases as cc

FILL = 0xA5
COMPONENTS = ("device", "n_vertices", "n_triangles", "tri", "label", "comp_triangles", "n_components", "largest")
FILTER = ("device", "n_vertices", "xyz", "bgr", "n_triangles", "tri", "min_triangles", "keep_largest", "xyz_out", "bgr_out", "vcap", "tri_out", "tcap",
          "vertex_of", "n_vertices_out", "n_triangles_out")
SMOOTH = ("device", "n_vertices", "xyz", "n_triangles", "tri", "origin", "quantum", "iterations", "lam", "mu", "xyz_out", "normal")
CLEAN = FILTER[:8] + SMOOTH[5:10] + ("xyz_out", "bgr_out", "normal", "vcap", "tri_out", "tcap", "vertex_of", "n_vertices_out", "n_triangles_out")
NAMES = {"sfmba_mesh_components": COMPONENTS, "sfmba_mesh_filter": FILTER, "sfmba_mesh_smooth": SMOOTH, "sfmba_mesh_clean": CLEAN}
OUTPUTS = {"sfmba_mesh_components": COMPONENTS[4:], "sfmba_mesh_filter": ("xyz_out", "bgr_out", "tri_out", "vertex_of", "n_vertices_out", "n_triangles_out"),
           "sfmba_mesh_smooth": ("xyz_out", "normal"),
           "sfmba_mesh_clean": ("xyz_out", "bgr_out", "normal", "tri_out", "vertex_of", "n_vertices_out", "n_triangles_out")}
FLOATS, LONGS = ("quantum", "lam", "mu"), ("n_vertices", "n_triangles", "vcap", "tcap")


def _filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def valid(entry, case="islands"):
    """the arguments of a valid call by name"""
    c = cc.case(case)
    nv, nt = len(c["xyz"]), len(c["tri"])
    return dict(device=0, n_vertices=nv, n_triangles=nt, xyz=c["xyz"].copy(), bgr=c["bgr"].copy(), tri=c["tri"].copy(), min_triangles=2, keep_largest=0,
                origin=c["origin"].copy(), quantum=float(c["quantum"]), iterations=2, lam=cc.LAM, mu=cc.MU, vcap=nv, tcap=nt,
                label=_filled(nv, np.int32), comp_triangles=_filled(nv, np.int32), n_components=_filled(1, np.int64), largest=_filled(1, np.int64),
                xyz_out=_filled((nv, 3), np.float32), bgr_out=_filled((nv, 3), np.uint8), normal=_filled((nv, 3), np.float32),
                tri_out=_filled((nt, 3), np.int32), vertex_of=_filled(nv, np.int32), n_vertices_out=_filled(1, np.int64),
                n_triangles_out=_filled(1, np.int64))


def invoke(lib, entry, a):
    """(rc, untouched) of one call with the named arguments `a`"""
    keep, args = [], []
    for k in NAMES[entry]:
        v = a[k]
        if v is None:
            args.append(None)
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


def _set(key, value):
    return lambda a: a.__setitem__(key, value)


def _at(key, index, value):
    def f(a):
        a[key] = a[key].copy()
        a[key].reshape(-1)[index] = value
    return f


MESH_DEFECTS = [
    ("n_vertices negative", _set("n_vertices", -1)), ("n_vertices 2^31", _set("n_vertices", 1 << 31)), ("n_triangles negative", _set("n_triangles", -1)),
    ("n_triangles 2^31", _set("n_triangles", 1 << 31)), ("n_triangles 2^40", _set("n_triangles", 1 << 40)), ("tri NULL", _set("tri", None)),
]
XYZ_DEFECTS = [("xyz NULL", _set("xyz", None))]
COMPONENT_DEFECTS = [("label NULL", _set("label", None)), ("n_components NULL", _set("n_components", None)), ("largest NULL", _set("largest", None))]
FILTER_DEFECTS = [
    ("min_triangles 0", _set("min_triangles", 0)), ("min_triangles negative", _set("min_triangles", -3)), ("keep_largest 2", _set("keep_largest", 2)),
    ("keep_largest -1", _set("keep_largest", -1)), ("vcap negative", _set("vcap", -1)), ("tcap negative", _set("tcap", -1)),
    ("n_vertices_out NULL", _set("n_vertices_out", None)), ("n_triangles_out NULL", _set("n_triangles_out", None)),
    ("xyz_out NULL with vcap > 0", _set("xyz_out", None)), ("tri_out NULL with tcap > 0", _set("tri_out", None)),
    ("bgr_out NULL with colours", _set("bgr_out", None)),
]
SMOOTH_DEFECTS = [
    ("iterations -1", _set("iterations", -1)), ("iterations 101", _set("iterations", 101)), ("lambda 0", _set("lam", 0.0)),
    ("lambda below half a unit", _set("lam", 0.49 / 65536.0)), ("lambda above 1", _set("lam", 1.0 + 2.0 ** -16)), ("lambda negative", _set("lam", -0.5)),
    ("lambda NaN", _set("lam", float("nan"))), ("lambda infinite", _set("lam", float("inf"))), ("mu 0", _set("mu", 0.0)), ("mu positive", _set("mu", 0.53)),
    ("mu above minus half a unit", _set("mu", -0.49 / 65536.0)), ("mu below -2", _set("mu", -2.0 - 2.0 ** -15)), ("mu NaN", _set("mu", float("nan"))),
    ("mu infinite", _set("mu", float("-inf"))), ("origin NULL", _set("origin", None)), ("origin NaN", _at("origin", 1, np.nan)),
    ("origin infinite", _at("origin", 2, -np.inf)), ("quantum 0", _set("quantum", 0.0)), ("quantum negative", _set("quantum", -0.25)),
    ("quantum NaN", _set("quantum", float("nan"))), ("quantum infinite", _set("quantum", float("inf"))),
]
SMOOTH_OUT_DEFECTS = [("xyz_out NULL", _set("xyz_out", None))]
# found on the device
INDEX_DEFECTS = [("a negative index", _at("tri", 7, -1)), ("an index of n_vertices", lambda a: _at("tri", 100, a["n_vertices"])(a)),
                 ("the last index out of range", lambda a: _at("tri", -1, 1 << 30)(a))]
COORD_DEFECTS = [("a NaN coordinate", _at("xyz", 100, np.nan)), ("an infinite coordinate", _at("xyz", 5, np.inf)),
                 ("a coordinate 2^25 quanta out", lambda a: _at("xyz", 31, a["origin"][1] + np.float32(a["quantum"]) * np.float32(1 << 25))(a)),
                 ("a coordinate -2^25 quanta out", lambda a: _at("xyz", 30, a["origin"][0] - np.float32(a["quantum"]) * np.float32(1 << 25))(a))]


def refusal_calls(capi, device_cases=False):
    lib = capi.lib()
    dev = device_cases
    table = [("sfmba_mesh_components", MESH_DEFECTS + COMPONENT_DEFECTS + (INDEX_DEFECTS if dev else [])),
             ("sfmba_mesh_filter", MESH_DEFECTS + XYZ_DEFECTS + FILTER_DEFECTS + (INDEX_DEFECTS if dev else [])),
             ("sfmba_mesh_smooth", MESH_DEFECTS + XYZ_DEFECTS + SMOOTH_DEFECTS + SMOOTH_OUT_DEFECTS + (INDEX_DEFECTS + COORD_DEFECTS if dev else [])),
             ("sfmba_mesh_clean", MESH_DEFECTS + XYZ_DEFECTS + FILTER_DEFECTS + SMOOTH_DEFECTS + (INDEX_DEFECTS + COORD_DEFECTS if dev else []))]
    out = []
    for entry, defects in table:
        for what, spoil in defects:
            def call(entry=entry, spoil=spoil):
                a = valid(entry)
                spoil(a)
                return invoke(lib, entry, a)
            out.append(("%s: %s" % (entry, what), call))
    return out


def valid_call(capi, entry):
    return invoke(capi.lib(), entry, valid(entry))
