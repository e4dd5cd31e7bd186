"""Every argument refusal of sfmba_mesh_decimate (the contract is in include/sfmba.h) as a list of calls -- TEST INFRASTRUCTURE ONLY.
Each case is the valid call with exactly one thing wrong; the outputs are filled with 0xA5 bytes before the call.  refusal_calls
gives (name, call) pairs; call() returns (rc, untouched).  The refusals that the library finds before it opens the device run in the
CPU suite too; a triangle index outside the vertex list and a coordinate out of range are found on the device."""
import ctypes as C

import numpy as np

import decimate_cases as dc
from mesh_clean_refusals import COORD_DEFECTS, FILL, INDEX_DEFECTS, MESH_DEFECTS, XYZ_DEFECTS, _at, _filled, _set

ENTRY = "sfmba_mesh_decimate"
ARGS = ("device", "n_vertices", "xyz", "bgr", "n_triangles", "tri", "origin", "quantum", "cell", "placement", "reg", "xyz_out", "bgr_out", "members",
        "vcap", "tri_out", "triangle_of", "tcap", "vertex_of", "n_vertices_out", "n_triangles_out", "stats")
OUTPUTS = ("xyz_out", "bgr_out", "members", "tri_out", "triangle_of", "vertex_of", "n_vertices_out", "n_triangles_out", "stats")
ARRAYS_OUT = ("xyz_out", "bgr_out", "members", "tri_out", "triangle_of", "vertex_of", "stats")            # what a short capacity leaves alone
FLOATS, LONGS = ("quantum",), ("n_vertices", "n_triangles", "vcap", "tcap")


def valid(case="small_cube"):
    """the arguments of a valid call by name"""
    c = dc.case(case)
    nv, nt = len(c["xyz"]), len(c["tri"])
    return dict(device=0, n_vertices=nv, n_triangles=nt, xyz=c["xyz"].copy(), bgr=None if c["bgr"] is None else c["bgr"].copy(), tri=c["tri"].copy(),
                origin=c["origin"].copy(), quantum=float(c["quantum"]), cell=c["cell"], placement=c["placement"], reg=c["reg"], vcap=nv, tcap=nt,
                xyz_out=_filled((max(nv, 1), 3), np.float32), bgr_out=_filled((max(nv, 1), 3), np.uint8), members=_filled(max(nv, 1), np.int32),
                tri_out=_filled((max(nt, 1), 3), np.int32), triangle_of=_filled(max(nt, 1), np.int32), vertex_of=_filled(max(nv, 1), np.int32),
                n_vertices_out=_filled(1, np.int64), n_triangles_out=_filled(1, np.int64), stats=_filled(4, np.int64))


def invoke(lib, a):
    """(rc, untouched) of one call with the named arguments `a`"""
    keep, args = [], []
    for k in ARGS:
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
    rc = getattr(lib, ENTRY)(*args)
    untouched = all(a[k] is None or (a[k].view(np.uint8) == FILL).all() for k in OUTPUTS)
    return rc, untouched


OUT_DEFECTS = [
    ("vcap negative", _set("vcap", -1)), ("tcap negative", _set("tcap", -1)), ("n_vertices_out NULL", _set("n_vertices_out", None)),
    ("n_triangles_out NULL", _set("n_triangles_out", None)), ("xyz_out NULL with vcap > 0", _set("xyz_out", None)),
    ("tri_out NULL with tcap > 0", _set("tri_out", None)), ("bgr_out NULL with colours", _set("bgr_out", None)),
]
GRID_DEFECTS = [
    ("origin NULL", _set("origin", None)), ("origin NaN", _at("origin", 1, np.nan)), ("origin infinite", _at("origin", 2, -np.inf)),
    ("quantum 0", _set("quantum", 0.0)), ("quantum negative", _set("quantum", -0.25)), ("quantum NaN", _set("quantum", float("nan"))),
    ("quantum infinite", _set("quantum", float("inf"))),
]


def _both(**kv):
    def f(a):
        a.update(kv)
    return f


PARAM_DEFECTS = [
    ("cell 31", _set("cell", 31)), ("cell 0", _set("cell", 0)), ("cell negative", _set("cell", -256)), ("cell 2^20 + 1", _set("cell", (1 << 20) + 1)),
    ("cell 2^31 - 1", _set("cell", (1 << 31) - 1)), ("placement 2", _set("placement", 2)), ("placement -1", _set("placement", -1)),
    ("reg 0", _set("reg", 0)), ("reg negative", _set("reg", -1024)), ("reg 2^20 + 1", _set("reg", (1 << 20) + 1)),
    ("placement 2 with reg 0", _both(placement=2, reg=0)),
]
# reg is read only with placement 1: these calls are VALID
REG_IGNORED = [("reg 0 with the mean", _both(placement=0, reg=0)), ("reg 2^30 with the mean", _both(placement=0, reg=1 << 30))]


def refusal_calls(capi, device_cases=False):
    lib = capi.lib()
    defects = MESH_DEFECTS + XYZ_DEFECTS + OUT_DEFECTS + GRID_DEFECTS + PARAM_DEFECTS + (INDEX_DEFECTS + COORD_DEFECTS if device_cases else [])
    out = []
    for what, spoil in defects:
        def call(spoil=spoil):
            a = valid()
            spoil(a)
            return invoke(lib, a)
        out.append(("%s: %s" % (ENTRY, what), call))
    return out


def valid_call(capi, spoil=None):
    a = valid()
    if spoil:
        spoil(a)
    return invoke(capi.lib(), a)
