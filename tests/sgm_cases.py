"""The cases of the semi-global matching tests (tests/test_sgm_oracle_cpu.py, tests/test_gpu_depth_sgm.py) -- TEST INFRASTRUCTURE ONLY.

A volume case is dict(vol uint8 [h, w, D], p1, p2, n_paths, invalid_cost) for sgm_oracle.aggregate_* / capi.sgm_aggregate.  The sizes
are the smallest at which the kernel can still go wrong: one pixel, one row, one column, line lengths on both sides of a wave (64)
and of a workgroup of four lines, diagonals that start on every border; D on both sides of 64 and of every further slab of 64 planes.
The restatement's answer for each is computed once and shared (oracle(name)).

den = 0 is not among the volumes: k* is the LOWEST plane of the smallest sum, so S(k* - 1) > S(k*) and den >= 1 wherever k* has two
neighbours.  The rule is held on the arithmetic itself (the `delta` rows of tools/micro/sgm_math_host.hip).

Allowed importers: tests/, tools/.
"""
import functools

import numpy as np

import depth_cases as dc
import sgm_oracle as so


def _rand(w, h, D, seed, lo=0, hi=255):
    """Uniform entries lo..hi (hi = 255 includes the sentinel)."""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(h, w, D)).astype(np.uint8)


def _case(vol, p1=8, p2=64, n_paths=8, invalid_cost=127):
    return dict(vol=np.ascontiguousarray(vol, np.uint8), p1=p1, p2=p2, n_paths=n_paths, invalid_cost=invalid_cost)


def _ramp(w, h, D):
    """Plane 0 costs 0 everywhere, every other plane 254: L grows by 254 a step until it stands at 254 + p2."""
    v = np.full((h, w, D), 254, np.uint8)
    v[:, :, 0] = 0
    return v


def _valley(w, h, D, at, seed):
    """Noise 100..254 with a plane of cost 0..3 at `at` (a function of x, y): k* lands there."""
    v = _rand(w, h, D, seed, 100, 254)
    ys, xs = np.mgrid[0:h, 0:w]
    k = np.clip(at(xs, ys), 0, D - 1)
    np.put_along_axis(v, k[..., None], (np.random.default_rng(seed + 1).integers(0, 4, size=(h, w, 1))).astype(np.uint8), 2)
    return v


def _two_minima(w, h, D):
    """Two planes share the smallest cost in every pixel (a tie of the path minimum and of k*); the lower one must win."""
    v = np.full((h, w, D), 90, np.uint8)
    v[:, :, 1] = 7
    v[:, :, D - 1] = 7
    return v


CASES = {
    # sizes x D x paths x penalties
    "1x1_d2_p8": lambda: _case(_rand(1, 1, 2, 1), 3, 9, 8),
    "1x1_d256_p4": lambda: _case(_rand(1, 1, 256, 2), 0, 0, 4),
    "1x7_d64_p8": lambda: _case(_rand(1, 7, 64, 3), 5, 5, 8),
    "7x1_d256_p8": lambda: _case(_rand(7, 1, 256, 4), 0, 1023, 8),
    "7x1_d3_p4": lambda: _case(_rand(7, 1, 3, 5), 8, 64, 4),
    "2x2_d63_p8": lambda: _case(_rand(2, 2, 63, 6), 8, 64, 8),
    "2x2_d2_p4": lambda: _case(_rand(2, 2, 2, 7), 1, 1, 4),
    "17x33_d65_p8": lambda: _case(_rand(17, 33, 65, 8), 8, 64, 8),
    "17x33_d3_p4_zero": lambda: _case(_rand(17, 33, 3, 9), 0, 0, 4),
    "33x17_d129_p4": lambda: _case(_rand(33, 17, 129, 10), 20, 20, 4),
    "33x17_d64_p8_wide": lambda: _case(_rand(33, 17, 64, 11), 0, 1023, 8),
    "70x45_d3_p8": lambda: _case(_rand(70, 45, 3, 12), 8, 64, 8),
    "70x45_d64_p4": lambda: _case(_valley(70, 45, 64, lambda x, y: 5 + (x + y) // 3, 13), 8, 64, 4),
    "70x45_d2_p8_equal": lambda: _case(_rand(70, 45, 2, 14), 64, 64, 8),
    # volumes
    "all_254": lambda: _case(np.full((9, 13, 65), 254, np.uint8), 8, 1023, 8),
    "all_sentinel": lambda: _case(np.full((9, 13, 63), 255, np.uint8), 8, 64, 8),
    "invalid_cost_0": lambda: _case(_rand(13, 9, 64, 15, 200, 255), 8, 64, 8, invalid_cost=0),
    "invalid_cost_254": lambda: _case(_rand(13, 9, 64, 16, 0, 255), 0, 1023, 8, invalid_cost=254),
    "ramp_equal_1023": lambda: _case(_ramp(9, 8, 5), 1023, 1023, 8),
    "ramp_zero_1023": lambda: _case(_ramp(9, 8, 65), 0, 1023, 8),
    "ramp_equal_200": lambda: _case(_ramp(5, 3, 129), 200, 200, 4),
    "two_minima_d65": lambda: _case(_two_minima(11, 6, 65), 8, 64, 8),
    "two_minima_d256": lambda: _case(_two_minima(5, 6, 256), 0, 0, 4),
    "edge_low": lambda: _case(_valley(12, 10, 64, lambda x, y: 0 * x, 17), 8, 64, 8),
    "edge_high_d65": lambda: _case(_valley(12, 10, 65, lambda x, y: 64 + 0 * x, 18), 8, 64, 8),
    "edge_high_d256": lambda: _case(_valley(6, 5, 256, lambda x, y: 255 + 0 * x, 19), 8, 64, 4),
    "second_absent_d3": lambda: _case(_valley(8, 6, 3, lambda x, y: 1 + 0 * x, 20), 8, 64, 8),
    "second_absent_d2": lambda: _case(_valley(8, 6, 2, lambda x, y: (x + y) % 2, 21), 0, 1023, 8),
}
NO_SUMS = ("17x33_d65_p8", "2x2_d2_p4", "7x1_d256_p8")       # the cases that also run with sums = NULL on the device


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle(name):
    """sgm_oracle.sgm_aggregate's dict for the case; shared, not to be changed."""
    c = case(name)
    return so.sgm_aggregate(c["vol"], c["p1"], c["p2"], c["n_paths"], c["invalid_cost"])


# ---- scenes for the calls that start from images ------------------------------------------------------------------------------------
VOLUME_SCENES = ("blind", "const_ref", "min_sources_2", "size_17x33_r2_d3", "size_48x31_r3_d64")       # of depth_cases.CASES


@functools.lru_cache(maxsize=None)
def volume_oracle(name):
    """(vol, wf, step) of the single job of a depth_cases case."""
    c = dc.case(name)
    p = c["params"]
    return so.cost_volume(c["images"], c["K"], c["P"], c["jobs"][0], p["n_planes"], p["radius"], p["min_std"], p["min_sources"])


def sweep_params(c, **sgm):
    """The keyword arguments of capi.depth_sweep_sgm / sgm_oracle.sweep_sgm from a depth_cases case."""
    p = {k: v for k, v in c["params"].items() if k != "min_score"}
    p.update(sgm)
    return p


@functools.lru_cache(maxsize=None)
def uniqueness_case():
    """A scene, SGM parameters and a `uniqueness` u for which the restatement has a pixel EXACTLY on the ratio
    (100 (second - best) == u second), one whose best is one unit too large for it and one whose best is one unit below the bound:
    (case, sgm params without uniqueness, u, agg).  Found by search over u; the scene and the penalties are fixed."""
    c = dc.case("size_48x31_r3_d64")
    sgm = dict(p1=0, p2=0, n_paths=4, invalid_cost=127)
    vol, wf, step = volume_oracle("size_48x31_r3_d64")
    agg = so.sgm_aggregate(vol, **sgm)
    b, s = agg["best"].astype(np.int64), agg["second"].astype(np.int64)
    for u in range(1, 101):
        slack = 100 * (s - b) - u * s                        # >= 0: accepted
        on, above, below = (slack == 0), (slack >= -100) & (slack < 0), (slack > 0) & (slack <= 100)
        if on.any() and above.any() and below.any():
            return c, sgm, u, agg
    raise AssertionError("no uniqueness lies exactly on a pixel's ratio")
