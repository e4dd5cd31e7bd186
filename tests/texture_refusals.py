"""Every argument refusal of sfmba_mesh_texture / sfmba_mesh_texture_size (the contract is in include/sfmba.h) as a list of calls -- TEST
INFRASTRUCTURE ONLY.  Each case is the valid call with exactly one thing wrong; the outputs are filled with 0xA5 bytes before the call.
refusal_calls gives (name, call) pairs; call() returns (rc, untouched).  The refusals that the library finds before it opens the device
run in the CPU suite too; a triangle index outside the vertex list is found on the device."""
import ctypes as C

import numpy as np

import texture_cases as tc
import texture_oracle as to

FILL = 0xA5
TEXTURE = ("device", "n_vertices", "xyz", "bgr", "n_triangles", "tri", "n_images", "img_ptr", "pixels", "width", "height", "channels", "K", "P", "depth",
           "occl_tol", "min_area", "patch", "blocks_per_row", "atlas", "uv", "view", "score", "n_textured")
SIZE = ("n_triangles", "patch", "blocks_per_row", "width_out", "height_out")
NAMES = {"sfmba_mesh_texture": TEXTURE, "sfmba_mesh_texture_size": SIZE}
OUTPUTS = {"sfmba_mesh_texture": ("atlas", "uv", "view", "score", "n_textured"), "sfmba_mesh_texture_size": ("width_out", "height_out")}
FLOATS, LONGS = ("occl_tol",), ("n_vertices", "n_triangles", "min_area")


def _filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def valid(entry, case="four_views"):
    """the arguments of a valid call by name"""
    c = tc.case(case)
    nv, nt, n = len(c["xyz"]), len(c["tri"]), len(c["images"])
    B = to.default_blocks_per_row(nt)
    W, H = to.atlas_size(nt, c["patch"], B)
    if entry == "sfmba_mesh_texture_size":
        return dict(n_triangles=nt, patch=c["patch"], blocks_per_row=B, width_out=_filled(1, np.int32), height_out=_filled(1, np.int32))
    maps = [None if m is None else np.ascontiguousarray(m, np.float32) for m in c["depth_maps"]]
    img_ptr = np.zeros(n + 1, np.int64)
    img_ptr[1:] = np.cumsum([im.size for im in c["images"]])
    return dict(device=0, n_vertices=nv, xyz=c["xyz"].copy(), bgr=c["bgr"].copy(), n_triangles=nt, tri=c["tri"].copy(), n_images=n, img_ptr=img_ptr,
                pixels=np.concatenate([im.reshape(-1) for im in c["images"]]), width=np.asarray([im.shape[1] for im in c["images"]], np.int32),
                height=np.asarray([im.shape[0] for im in c["images"]], np.int32), channels=3, K=np.ascontiguousarray(c["K"], np.float32).reshape(9),
                P=np.ascontiguousarray(c["P"], np.float32).reshape(-1), depth=maps, occl_tol=float(c["occl_tol"]), min_area=int(c["min_area"]),
                patch=c["patch"], blocks_per_row=B, atlas=_filled((H, W, 3), np.uint8), uv=_filled((nt, 3, 2), np.float32), view=_filled(nt, np.int32),
                score=_filled(nt, np.int64), n_textured=_filled(1, np.int64))


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


def _set(key, value):
    return lambda a: a.__setitem__(key, value)


def _at(key, index, value):
    def f(a):
        a[key] = a[key].copy()
        a[key].reshape(-1)[index] = value
    return f


def _layout(B, patch, n_triangles=None):
    def f(a):
        a["blocks_per_row"], a["patch"] = B, patch
        if n_triangles is not None:
            a["n_triangles"] = n_triangles
    return f


LAYOUT_DEFECTS = [
    ("patch 2", _set("patch", 2)), ("patch 65", _set("patch", 65)), ("patch negative", _set("patch", -6)), ("blocks_per_row 0", _set("blocks_per_row", 0)),
    ("blocks_per_row negative", _set("blocks_per_row", -1)), ("W above 16384", _layout(2731, 5)), ("H above 16384", _layout(1, 5, 6556)),
    ("n_triangles negative", _set("n_triangles", -1)), ("n_triangles 2^31", _set("n_triangles", 1 << 31)),
]
SIZE_DEFECTS = [("width NULL", _set("width_out", None)), ("height NULL", _set("height_out", None))]
MESH_DEFECTS = [
    ("n_vertices negative", _set("n_vertices", -1)), ("n_vertices 2^31", _set("n_vertices", 1 << 31)), ("tri NULL", _set("tri", None)),
    ("xyz NULL", _set("xyz", None)),
]
VIEW_DEFECTS = [
    ("n_images negative", _set("n_images", -1)), ("img_ptr NULL", _set("img_ptr", None)), ("pixels NULL", _set("pixels", None)),
    ("width NULL", _set("width", None)), ("height NULL", _set("height", None)), ("K NULL", _set("K", None)), ("P NULL", _set("P", None)),
    ("depth NULL", _set("depth", None)), ("channels 2", _set("channels", 2)), ("channels 4", _set("channels", 4)), ("img_ptr not from 0", _at("img_ptr", 0, 1)),
    ("img_ptr against the sizes", _at("img_ptr", 2, 7)), ("a width of 0", _at("width", 1, 0)), ("a height of 16385", _at("height", 0, 16385)),
    ("P NaN", _at("P", 17, np.nan)), ("P infinite", _at("P", 3, np.inf)), ("fx 0", _at("K", 0, 0.0)), ("fy negative", _at("K", 4, -36.0)),
    ("fx NaN", _at("K", 0, np.nan)), ("cx infinite", _at("K", 2, np.inf)), ("cy NaN", _at("K", 5, np.nan)),
]
PARAM_DEFECTS = [
    ("occl_tol negative", _set("occl_tol", -0.25)), ("occl_tol NaN", _set("occl_tol", float("nan"))), ("occl_tol infinite", _set("occl_tol", float("inf"))),
    ("min_area negative", _set("min_area", -1)),
]
OUT_DEFECTS = [("atlas NULL", _set("atlas", None)), ("uv NULL", _set("uv", None)), ("view NULL", _set("view", None)), ("n_textured NULL", _set("n_textured", None))]
# found on the device
INDEX_DEFECTS = [("a negative index", _at("tri", 7, -1)), ("an index of n_vertices", lambda a: _at("tri", 50, a["n_vertices"])(a)),
                 ("the last index out of range", lambda a: _at("tri", -1, 1 << 30)(a))]


def refusal_calls(capi, device_cases=False):
    lib = capi.lib()
    table = [("sfmba_mesh_texture_size", LAYOUT_DEFECTS + SIZE_DEFECTS),
             ("sfmba_mesh_texture", LAYOUT_DEFECTS + MESH_DEFECTS + VIEW_DEFECTS + PARAM_DEFECTS + OUT_DEFECTS + (INDEX_DEFECTS if device_cases else []))]
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
