"""Named inputs of sfmba_tsdf_fill for the CPU and GPU tests -- TEST INFRASTRUCTURE ONLY.

A case is a dict S, W int32 [nz, ny, nx], CS int32 [nz, ny, nx, 3] or None, CW int32 [nz, ny, nx] or None, min_weight, iterations,
min_neighbours, want_state.  expected(name) gives the restatement's answer once per process (tsdf_fill_oracle.fill_numpy); it is
shared and not to be changed.  Small on purpose: the largest grid is 65 x 4 x 3."""
import functools

import numpy as np

import tsdf_fill_oracle as fo


def _case(S, W, CS=None, CW=None, min_weight=1, iterations=3, k=2, want_state=True):
    S, W = np.ascontiguousarray(S, np.int32), np.ascontiguousarray(W, np.int32)
    if CS is not None:
        CS, CW = np.ascontiguousarray(CS, np.int32), np.ascontiguousarray(CW, np.int32)
    return dict(S=S, W=W, CS=CS, CW=CW, min_weight=min_weight, iterations=iterations, min_neighbours=k, want_state=want_state)


def _colours(W, rng):
    """colour sums inside their bounds beside W: about a third of the vertices with W > 0 have none"""
    CW = np.where(rng.random(W.shape) < 0.35, 0, rng.integers(0, W + 1))
    CS = rng.integers(0, 256, size=W.shape + (3,)) * CW[..., None]
    return np.maximum(CS - rng.integers(0, 3, size=CS.shape) * (CW[..., None] > 0), 0), CW


def _random(nx, ny, nz, seed, frac=0.4, min_weight=1, colour=True, **kw):
    """`frac` of the vertices observed (W in min_weight .. min_weight + 4); the others have W in 0 .. min_weight - 1, sums and all"""
    rng = np.random.default_rng(seed)
    obs = rng.random((nz, ny, nx)) < frac
    W = np.where(obs, rng.integers(min_weight, min_weight + 5, size=obs.shape), rng.integers(0, min_weight, size=obs.shape))
    S = rng.integers(-1024 * W, 1024 * W + 1)
    CS, CW = _colours(W, rng) if colour else (None, None)
    return _case(S, W, CS, CW, min_weight=min_weight, **kw)


def _line(values, k, iterations, axis=2):
    """a line of len(values) vertices along x (axis 2), y or z; a value is None (W = 0) or (S, W)"""
    n = len(values)
    shape = [1, 1, 1]
    shape[axis] = n
    S = np.asarray([0 if v is None else v[0] for v in values]).reshape(shape)
    W = np.asarray([0 if v is None else v[1] for v in values]).reshape(shape)
    return _case(S, W, k=k, iterations=iterations)


def _centre(iterations, k=1):
    S, W = np.zeros((5, 5, 5), np.int64), np.zeros((5, 5, 5), np.int64)
    S[2, 2, 2], W[2, 2, 2] = -700, 3
    CS, CW = np.zeros((5, 5, 5, 3), np.int64), np.zeros((5, 5, 5), np.int64)
    CS[2, 2, 2], CW[2, 2, 2] = (90, 301, 509), 2
    return _case(S, W, CS, CW, k=k, iterations=iterations)


def _below_min_weight():
    # x = 0 observed (W = 3); x = 1 has W = 1 and is reached in pass 1; x = 4 has W = 2 and is not reached; colours ride along
    S = np.asarray([1500, -700, 0, 0, 2048, 0]).reshape(1, 1, 6)
    W = np.asarray([3, 1, 0, 0, 2, 0]).reshape(1, 1, 6)
    CW = np.asarray([2, 1, 0, 0, 2, 0]).reshape(1, 1, 6)
    CS = np.asarray([[100, 200, 300], [7, 8, 9], [0, 0, 0], [0, 0, 0], [500, 1, 2], [0, 0, 0]]).reshape(1, 1, 6, 3)
    return _case(S, W, CS, CW, min_weight=3, iterations=1, k=1)


def _colour_mix():
    # the row y = 0, z = 0 is observed: with colour, without, with.  One pass at k = 1 fills its neighbours at y = 1 and at z = 1: the
    # two beside x = 1 have a colourless vertex as their only known neighbour (hasC = 0), the others take their neighbour's colour
    S, W = np.zeros((2, 2, 3), np.int64), np.zeros((2, 2, 3), np.int64)
    CS, CW = np.zeros((2, 2, 3, 3), np.int64), np.zeros((2, 2, 3), np.int64)
    W[0, 0] = (2, 4, 1)
    S[0, 0] = (-100, 3000, 77)
    CW[0, 0] = (2, 0, 1)
    CS[0, 0, 0], CS[0, 0, 2] = (255, 0, 301), (17, 200, 255)
    return _case(S, W, CS, CW, k=1, iterations=1)


def _only_colourless():
    # one observed vertex without colour: everything the fill makes has hasC = 0
    S, W = np.zeros((1, 3, 3), np.int64), np.zeros((1, 3, 3), np.int64)
    S[0, 1, 1], W[0, 1, 1] = 555, 2
    return _case(S, W, np.zeros((1, 3, 3, 3), np.int64), np.zeros((1, 3, 3), np.int64), k=1, iterations=2)


def _halves():
    # W = 128, S = +-1: 64 S / W = +-0.5 -> V = 1 and 0 (half up).  Between V = 1 and V = 2 the mean is 1.5 -> 2; between -1 and -2 it is
    # -1.5 -> -1 (floor_div of the doubled sum plus n: towards minus infinity, so halves go up on both sides of zero)
    v = [(1, 128), None, (-1, 128), None, (1, 64), None, (2, 64), None, (-1, 64), None, (-2, 64), None, (-3, 64)]
    return _line(v, k=2, iterations=1)


def _extremes():
    v = [(1024 * 5, 5), None, (1024 * 5, 5), None, (-1024 * 7, 7), None, (-1024 * 7, 7), None, (1024 * 2, 2)]
    return _line(v, k=2, iterations=2)


CASES = {
    "g_1x1x1": lambda: _random(1, 1, 1, 1, frac=1.0),
    "g_1x1x1_unknown": lambda: _random(1, 1, 1, 2, frac=0.0),
    "g_2x2x2": lambda: _random(2, 2, 2, 3),
    "line_z_k1": lambda: _line([(300, 2)] + [None] * 8, k=1, iterations=5, axis=0),
    "line_z_k2": lambda: _line([(300, 2)] + [None] * 8, k=2, iterations=5, axis=0),
    "centre_5_k1": lambda: _centre(4),
    "nx_63": lambda: _random(63, 4, 3, 10),
    "nx_64": lambda: _random(64, 4, 3, 11),
    "nx_65": lambda: _random(65, 4, 3, 12),
    "ny_63": lambda: _random(3, 63, 4, 13),
    "ny_64": lambda: _random(3, 64, 4, 14),
    "ny_65": lambda: _random(3, 65, 4, 15),
    "nz_63": lambda: _random(4, 3, 63, 16),
    "nz_64": lambda: _random(4, 3, 64, 17),
    "nz_65": lambda: _random(4, 3, 65, 18),
    "none_observed": lambda: _random(5, 4, 3, 19, frac=0.0, min_weight=3),
    "all_observed": lambda: _random(5, 4, 3, 20, frac=1.0),
    "k1_9": lambda: _random(9, 9, 9, 30, k=1, iterations=4),
    "k2_9": lambda: _random(9, 9, 9, 30, k=2, iterations=4),
    "k3_9": lambda: _random(9, 9, 9, 30, k=3, iterations=4),
    "k4_9": lambda: _random(9, 9, 9, 30, k=4, iterations=4),
    "k5_9": lambda: _random(9, 9, 9, 30, k=5, iterations=4),
    "k6_9": lambda: _random(9, 9, 9, 30, k=6, iterations=4),
    "halves": _halves,
    "extremes": _extremes,
    "below_min_weight": _below_min_weight,
    "min_weight_1": lambda: _random(7, 5, 4, 40, min_weight=1),
    "min_weight_64": lambda: _random(7, 5, 4, 41, min_weight=64),
    "min_weight_65": lambda: _random(7, 5, 4, 42, min_weight=65),
    "min_weight_65535": lambda: _random(7, 5, 4, 43, min_weight=65535),
    "colour_mix": _colour_mix,
    "only_colourless": _only_colourless,
    "no_colour": lambda: _random(6, 5, 4, 50, colour=False),
    "iterations_0": lambda: _random(6, 5, 4, 51, min_weight=2, iterations=0),
    "iterations_254": lambda: _centre(254),
    "state_null": lambda: _random(6, 5, 4, 52, want_state=False),
}
FILL_WEIGHT = {"min_weight_1": 64, "min_weight_64": 64, "min_weight_65": 128, "min_weight_65535": 65536}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def run(c, fn=fo.fill_numpy):
    return fn(c["S"], c["W"], c["CS"], c["CW"], c["min_weight"], c["iterations"], c["min_neighbours"])


@functools.lru_cache(maxsize=None)
def expected(name):
    return run(case(name))
