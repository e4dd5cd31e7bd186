"""Every refusal that include/sfmba.h documents for sfmba_depth_cost_volume, sfmba_sgm_aggregate and sfmba_depth_sweep_sgm, as raw
calls whose outputs are filled with a pattern first (tests/test_gpu_depth_sgm.py) -- TEST INFRASTRUCTURE ONLY.

REFUSALS maps a name to a function of the capi module that returns (rc, {output name: array}); a refused call must return
SFMBA_ERR_INVALID_ARG and leave every byte of every output at FILL.

Allowed importers: tests/.
"""
import ctypes as C

import numpy as np

import depth_cases as dc

FILL = 0x5a
_lp, _bp, _fp, _ip = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte), C.POINTER(C.c_float), C.POINTER(C.c_int32)
_sp, _up = C.POINTER(C.c_int16), C.POINTER(C.c_uint16)


def _filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


# ---- sfmba_sgm_aggregate ----------------------------------------------------------------------------------------------------------
def aggregate(capi, w=5, h=4, D=6, p1=8, p2=64, n_paths=8, invalid_cost=127, n_jobs=1, null=(), width=None, height=None):
    vol = np.random.default_rng(0).integers(0, 256, size=(abs(h), abs(w), max(D, 1))).astype(np.uint8)
    out = dict(plane=_filled((abs(h), abs(w)), np.int16), best=_filled((abs(h), abs(w)), np.uint16), second=_filled((abs(h), abs(w)), np.uint16),
               sums=_filled((abs(h), abs(w), max(D, 1)), np.uint16))
    wd, ht = np.asarray([w if width is None else width], np.int32), np.asarray([h if height is None else height], np.int32)

    def arr(t, a, name):
        if name in null:
            return None
        return (t * 1)(None if name + "[0]" in null else a.ctypes.data_as(t))

    rc = capi.lib().sfmba_sgm_aggregate(0, n_jobs, arr(_bp, vol, "cost"), None if "width" in null else wd.ctypes.data_as(_ip),
                                        None if "height" in null else ht.ctypes.data_as(_ip), D, p1, p2, n_paths, invalid_cost,
                                        arr(_sp, out["plane"], "plane"), arr(_up, out["best"], "best"), arr(_up, out["second"], "second"),
                                        arr(_up, out["sums"], "sums"))
    return rc, out


# ---- the two calls that start from images -----------------------------------------------------------------------------------------
def _sweep_call(capi, symbol, tail, outputs, images=None, K=None, P=None, jobs=None, n_planes=None, radius=None, min_std=None, min_sources=None):
    c = dc.case("size_17x33_r2_d3")
    images, K, P, jobs = (c["images"] if images is None else images, c["K"] if K is None else K, c["P"] if P is None else P,
                          c["jobs"] if jobs is None else jobs)
    prm = c["params"]
    args, sizes, keep = capi._sweep_inputs(images, K, P, jobs, 0)
    rc = getattr(capi.lib(), symbol)(*args, prm["n_planes"] if n_planes is None else n_planes, prm["radius"] if radius is None else radius,
                                     prm["min_std"] if min_std is None else min_std, prm["min_sources"] if min_sources is None else min_sources, *tail)
    return rc, outputs


def cost_volume(capi, invalid_cost=127, null_cost=False, **over):
    c = dc.case("size_17x33_r2_d3")
    h, w = c["images"][0].shape
    out = dict(cost=_filled((h, w, 256), np.uint8))
    return _sweep_call(capi, "sfmba_depth_cost_volume", [invalid_cost, None if null_cost else out["cost"].ctypes.data_as(_bp)], out, **over)


def sweep_sgm(capi, p1=8, p2=64, n_paths=8, invalid_cost=127, uniqueness=5, null=(), **over):
    c = dc.case("size_17x33_r2_d3")
    h, w = c["images"][0].shape
    out = dict(depth=_filled((h, w), np.float32), score=_filled((h, w), np.float32), plane=_filled((h, w), np.int16))
    ptr = lambda name, t: None if name in null else out[name].ctypes.data_as(t)
    return _sweep_call(capi, "sfmba_depth_sweep_sgm", [p1, p2, n_paths, invalid_cost, uniqueness, ptr("depth", _fp), ptr("score", _fp), ptr("plane", _sp)],
                       out, **over)


def _bad_K(i, j, v):
    K = dc.case("size_17x33_r2_d3")["K"].copy()
    K[i, j] = v
    return K


def _bad_P():
    P = dc.case("size_17x33_r2_d3")["P"].copy()
    P[1, 2, 3] = np.inf
    return P


REFUSALS = {}
for _k, _kw in {
    "p1_negative": dict(p1=-1), "p2_below_p1": dict(p1=9, p2=8), "p2_above_1023": dict(p2=1024), "p1_above_1023": dict(p1=1024, p2=1024),
    "paths_0": dict(n_paths=0), "paths_6": dict(n_paths=6), "paths_16": dict(n_paths=16), "invalid_cost_negative": dict(invalid_cost=-1),
    "invalid_cost_255": dict(invalid_cost=255), "planes_1": dict(D=1), "planes_257": dict(D=257), "width_0": dict(width=0),
    "height_negative": dict(height=-3), "width_16385": dict(width=16385), "n_jobs_negative": dict(n_jobs=-1),
    "null_cost": dict(null=("cost",)), "null_cost_entry": dict(null=("cost[0]",)), "null_width": dict(null=("width",)),
    "null_height": dict(null=("height",)), "null_plane": dict(null=("plane",)), "null_plane_entry": dict(null=("plane[0]",)),
    "null_best": dict(null=("best",)), "null_best_entry": dict(null=("best[0]",)), "null_second": dict(null=("second",)),
    "null_second_entry": dict(null=("second[0]",)),
}.items():
    REFUSALS["aggregate_" + _k] = (lambda kw: lambda capi: aggregate(capi, **kw))(_kw)

_SWEEP = {
    "planes_1": dict(n_planes=1), "planes_257": dict(n_planes=257), "radius_0": dict(radius=0), "radius_5": dict(radius=5),
    "min_std_negative": dict(min_std=-1), "min_std_128": dict(min_std=128), "min_sources_0": dict(min_sources=0), "min_sources_5": dict(min_sources=5),
    "ref_out_of_range": dict(jobs=[(2, [1], 8.0, 12.0)]), "source_out_of_range": dict(jobs=[(0, [2], 8.0, 12.0)]),
    "source_is_reference": dict(jobs=[(0, [0], 8.0, 12.0)]), "source_twice": dict(jobs=[(0, [1, 1], 8.0, 12.0)]),
    "no_source": dict(jobs=[(0, [], 8.0, 12.0)]), "range_reversed": dict(jobs=[(0, [1], 12.0, 8.0)]), "range_zero": dict(jobs=[(0, [1], 0.0, 8.0)]),
    "range_infinite": dict(jobs=[(0, [1], 8.0, float("inf"))]), "range_nan": dict(jobs=[(0, [1], float("nan"), 8.0)]),
    "fx_zero": dict(K=_bad_K(0, 0, 0.0)), "cy_nan": dict(K=_bad_K(1, 2, np.nan)), "pose_infinite": dict(P=_bad_P()),
}
for _k, _kw in _SWEEP.items():
    REFUSALS["cost_volume_" + _k] = (lambda kw: lambda capi: cost_volume(capi, **kw))(_kw)
    REFUSALS["sweep_sgm_" + _k] = (lambda kw: lambda capi: sweep_sgm(capi, **kw))(_kw)
for _k, _kw in {"invalid_cost_negative": dict(invalid_cost=-1), "invalid_cost_255": dict(invalid_cost=255), "null_cost": dict(null_cost=True)}.items():
    REFUSALS["cost_volume_" + _k] = (lambda kw: lambda capi: cost_volume(capi, **kw))(_kw)
for _k, _kw in {
    "p1_negative": dict(p1=-1), "p2_below_p1": dict(p1=9, p2=8), "p2_above_1023": dict(p2=1024), "paths_5": dict(n_paths=5),
    "invalid_cost_negative": dict(invalid_cost=-1), "invalid_cost_255": dict(invalid_cost=255), "uniqueness_negative": dict(uniqueness=-1),
    "uniqueness_101": dict(uniqueness=101), "null_depth": dict(null=("depth",)), "null_score": dict(null=("score",)),
}.items():
    REFUSALS["sweep_sgm_" + _k] = (lambda kw: lambda capi: sweep_sgm(capi, **kw))(_kw)
