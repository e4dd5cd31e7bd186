"""Every argument refusal of sfmba_tsdf_integrate / sfmba_tsdf_extract / sfmba_tsdf_mesh (the contract is in include/sfmba.h) as a list
of calls -- TEST INFRASTRUCTURE ONLY.  Each case is the valid call of its entry point with exactly one thing wrong; the outputs are
filled with 0xA5 bytes before the call.  refusal_calls gives (name, call) pairs; call() returns (rc, untouched).  The refusals that
the library finds before it opens the device run in the CPU suite too; the breaches of a grid's bounds are found on the device."""
import ctypes as C

import numpy as np

FILL = 0xA5
INTEGRATE = ("device", "n_images", "img_ptr", "pixels", "width", "height", "channels", "K", "P", "depth", "origin", "voxel", "nx", "ny", "nz", "trunc",
             "sum", "weight", "csum", "cweight")
EXTRACT = ("device", "origin", "voxel", "nx", "ny", "nz", "sum", "weight", "csum", "cweight", "min_weight", "xyz", "bgr", "vkey", "vcap", "tri", "tcap",
           "n_vertices", "n_triangles")
MESH = INTEGRATE[:16] + EXTRACT[10:]
FLOATS, LONGS = ("voxel", "trunc"), ("vcap", "tcap")
NX, NY, NZ, CAP = 4, 3, 3, 256          # 12 cells: at most 144 triangles and 252 vertices


def _filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def valid(entry):
    """the arguments of a valid call by name; arrays are numpy arrays, `depth` a list of arrays / None"""
    rng = np.random.default_rng(90)
    w, h, n = 6, 5, 2
    a = dict(device=0, n_images=n, img_ptr=np.arange(n + 1, dtype=np.int64) * (w * h * 3), pixels=rng.integers(0, 256, n * w * h * 3).astype(np.uint8),
             width=np.full(n, w, np.int32), height=np.full(n, h, np.int32), channels=3,
             K=np.array([5, 0, 2.5, 0, 5, 2, 0, 0, 1], np.float32), P=np.tile(np.eye(3, 4, dtype=np.float32).reshape(-1), n),
             depth=[(1.0 + rng.random((h, w))).astype(np.float32) for _ in range(n)],
             origin=np.array([-0.5, -0.5, 0.8], np.float32), voxel=0.25, nx=NX, ny=NY, nz=NZ, trunc=0.5, min_weight=1, vcap=CAP, tcap=CAP)
    W = rng.integers(1, 4, size=(NZ, NY, NX)).astype(np.int32)
    if entry == "sfmba_tsdf_extract":
        a.update(sum=(rng.integers(-1024, 1025, size=W.shape) * W).astype(np.int32), weight=W, cweight=W.copy(),
                 csum=(rng.integers(0, 256, size=W.shape + (3,)) * W[..., None]).astype(np.int32))
    else:
        a.update(sum=_filled(W.shape, np.int32), weight=_filled(W.shape, np.int32), csum=_filled(W.shape + (3,), np.int32), cweight=_filled(W.shape, np.int32))
    a.update(xyz=_filled((CAP, 3), np.float32), bgr=_filled((CAP, 3), np.uint8), vkey=_filled(CAP, np.int32), tri=_filled((CAP, 3), np.int32),
             n_vertices=_filled(1, np.int64), n_triangles=_filled(1, np.int64))
    return a


def outputs(entry):
    return {"sfmba_tsdf_integrate": ("sum", "weight", "csum", "cweight"), "sfmba_tsdf_extract": EXTRACT[11:14] + ("tri", "n_vertices", "n_triangles"),
            "sfmba_tsdf_mesh": EXTRACT[11:14] + ("tri", "n_vertices", "n_triangles")}[entry]


def invoke(lib, entry, a):
    """(rc, untouched) of one call with the named arguments `a`"""
    names = {"sfmba_tsdf_integrate": INTEGRATE, "sfmba_tsdf_extract": EXTRACT, "sfmba_tsdf_mesh": MESH}[entry]
    keep, args = [], []
    for k in names:
        v = a[k]
        if v is None:
            args.append(None)
        elif k == "depth":
            fp = C.POINTER(C.c_float)
            args.append((fp * max(len(v), 1))(*[None if m is None else m.ctypes.data_as(fp) for m in v]))
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
    untouched = all(a[k] is None or (a[k].view(np.uint8) == FILL).all() for k in outputs(entry))
    return rc, untouched


def _many_images(a, n):
    a.update(n_images=n, img_ptr=np.arange(n + 1, dtype=np.int64), pixels=np.zeros(n, np.uint8), width=np.ones(n, np.int32),
             height=np.ones(n, np.int32), channels=1, P=np.tile(np.eye(3, 4, dtype=np.float32).reshape(-1), n), depth=[None] * n)


def _huge_maps(a):
    # 8 images of 16384 x 16384 with a map: 2^31 pixels, through the size arrays alone (the maps are never read; no pixels)
    one = np.zeros(1, np.float32)
    a.update(n_images=8, pixels=None, img_ptr=None, width=np.full(8, 16384, np.int32), height=np.full(8, 16384, np.int32),
             P=np.tile(np.eye(3, 4, dtype=np.float32).reshape(-1), 8), depth=[one] * 8)


def _set(key, value):
    return lambda a: a.__setitem__(key, value)


def _at(key, index, value):
    def f(a):
        a[key] = a[key].copy()
        a[key].reshape(-1)[index] = value
    return f


VIEW_DEFECTS = [
    ("channels 4", _set("channels", 4)), ("img_ptr[0] != 0", _at("img_ptr", 0, 1)), ("img_ptr one byte long", _at("img_ptr", 2, 181)),
    ("img_ptr NULL with pixels", _set("img_ptr", None)), ("width 0", _at("width", 1, 0)), ("height 16385", _at("height", 0, 16385)),
    ("width NULL", _set("width", None)), ("a NaN in a pose", _at("P", 15, np.nan)), ("an infinity in a pose", _at("P", 3, np.inf)),
    ("cx NaN", _at("K", 2, np.nan)), ("fy infinite", _at("K", 4, np.inf)), ("fx 0", _at("K", 0, 0.0)), ("fy negative", _at("K", 4, -5.0)),
    ("K NULL", _set("K", None)), ("P NULL", _set("P", None)), ("depth NULL", _set("depth", None)), ("n_images < 0", _set("n_images", -1)),
    ("65536 images", lambda a: _many_images(a, 65536)), ("2^31 pixels with a map", _huge_maps),
    ("trunc 0", _set("trunc", 0.0)), ("trunc negative", _set("trunc", -0.5)), ("trunc NaN", _set("trunc", float("nan"))),
    ("trunc infinite", _set("trunc", float("inf"))),
]
GRID_DEFECTS = [
    ("origin NULL", _set("origin", None)), ("origin NaN", _at("origin", 1, np.nan)), ("origin infinite", _at("origin", 2, -np.inf)),
    ("voxel 0", _set("voxel", 0.0)), ("voxel negative", _set("voxel", -0.25)), ("voxel NaN", _set("voxel", float("nan"))),
    ("voxel infinite", _set("voxel", float("inf"))), ("nx 0", _set("nx", 0)), ("ny 1025", _set("ny", 1025)), ("nz negative", _set("nz", -1)),
    ("more than 2^26 voxels", lambda a: a.update(nx=1024, ny=1024, nz=65)),
]
GRID_POINTER_DEFECTS = [
    ("sum NULL", _set("sum", None)), ("weight NULL", _set("weight", None)), ("csum without cweight", _set("cweight", None)),
    ("cweight without csum", _set("csum", None)),
]
OUT_DEFECTS = [
    ("min_weight 0", _set("min_weight", 0)), ("min_weight 65536", _set("min_weight", 65536)), ("vcap negative", _set("vcap", -1)),
    ("tcap negative", _set("tcap", -1)), ("n_vertices NULL", _set("n_vertices", None)), ("n_triangles NULL", _set("n_triangles", None)),
    ("xyz NULL with vcap > 0", _set("xyz", None)), ("tri NULL with tcap > 0", _set("tri", None)), ("bgr NULL with colours", _set("bgr", None)),
]
# found on the device: the grid handed to extract breaks the bounds an integration guarantees
DEVICE_DEFECTS = [
    ("a negative weight", _at("weight", 7, -1)), ("a negative cweight", _at("cweight", 30, -2)), ("S above 1024 W", lambda a: (_at("weight", 35, 2)(a), _at("sum", 35, 2049)(a))),
    ("S below -1024 W", lambda a: (_at("weight", 0, 1)(a), _at("sum", 0, -1025)(a))),
    ("a colour sum above 255 Wc", lambda a: (_at("cweight", 12, 1)(a), _at("csum", 38, 256)(a))),
    ("a negative colour sum", _at("csum", 3, -1)),
]


def refusal_calls(capi, device_cases=False):
    lib = capi.lib()
    table = [("sfmba_tsdf_integrate", VIEW_DEFECTS + GRID_DEFECTS + GRID_POINTER_DEFECTS),
             ("sfmba_tsdf_extract", GRID_DEFECTS + GRID_POINTER_DEFECTS + OUT_DEFECTS + (DEVICE_DEFECTS if device_cases else [])),
             ("sfmba_tsdf_mesh", VIEW_DEFECTS + GRID_DEFECTS + OUT_DEFECTS)]
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
