"""Named inputs of sfmba_mesh_components / sfmba_mesh_filter / sfmba_mesh_smooth / sfmba_mesh_clean for the CPU and GPU tests -- TEST
INFRASTRUCTURE ONLY.

A case is a dict: xyz float32 [n, 3], bgr uint8 [n, 3] or None, tri int32 [m, 3], origin float32 [3], quantum (float32), and the
parameters min_triangles, keep_largest, iterations, lam, mu.  want(name) gives the restatement's answers once per process
(mesh_clean_oracle's numpy statements): components, filter, smooth (of the whole mesh; None where the call refuses) and clean (None
likewise); they are shared and not to be changed.  The shapes are the smallest at which the kernels can still go wrong."""
import functools

import numpy as np

import mesh_cases as mc
import mesh_clean_oracle as co

LAM, MU = 0.5, -0.53


def _case(xyz, tri, bgr="random", origin=(0.0, 0.0, 0.0), quantum=2.0 ** -10, seed=0, **params):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    if isinstance(bgr, str):
        bgr = np.random.default_rng(seed + 900).integers(0, 256, size=(len(xyz), 3)).astype(np.uint8)
    c = dict(xyz=xyz, bgr=bgr, tri=tri, origin=np.asarray(origin, np.float32), quantum=np.float32(quantum), min_triangles=1, keep_largest=0,
             iterations=2, lam=LAM, mu=MU)
    c.update(params)
    return c


def with_params(name, **params):
    def make():
        c = dict(case(name))
        c.update(params)
        return c
    return make


# ---- shapes -------------------------------------------------------------------------------------------------------------------
def strip(n_vertices, seed, permute=False):
    """a zig-zag strip: vertex i at (i / 2, i % 2) with noise, triangle t on (t, t + 1, t + 2), every other one flipped to keep the
    orientation; n_vertices - 2 triangles, one component"""
    rng = np.random.default_rng(seed)
    i = np.arange(n_vertices)
    xyz = np.stack([0.5 * i, (i % 2).astype(np.float64), np.zeros(n_vertices)], axis=1) * 0.125 + rng.normal(scale=0.01, size=(n_vertices, 3))
    t = np.arange(max(n_vertices - 2, 0))
    tri = np.stack([t, np.where(t % 2 == 0, t + 1, t + 2), np.where(t % 2 == 0, t + 2, t + 1)], axis=1).reshape(-1, 3)
    if permute:
        perm = rng.permutation(n_vertices)                                              # old index -> new index
        new = np.zeros_like(xyz)
        new[perm] = xyz
        xyz, tri = new, perm[tri]
    return xyz, tri


def sheet(nx, ny, seed, at=(0.0, 0.0, 0.0), step=0.125, noise=0.01):
    """an nx x ny grid of vertices, two triangles per cell: 2 (nx - 1) (ny - 1) triangles"""
    rng = np.random.default_rng(seed)
    Y, X = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    xyz = np.stack([X * step + at[0], Y * step + at[1], np.full(X.shape, at[2])], axis=-1).reshape(-1, 3) + rng.normal(scale=noise, size=(nx * ny, 3))
    v = (Y * nx + X)[:-1, :-1].reshape(-1)
    tri = np.concatenate([np.stack([v, v + 1, v + nx + 1], axis=1), np.stack([v, v + nx + 1, v + nx], axis=1)])
    return xyz, tri


def join(*parts):
    xyz, tri, base = [], [], 0
    for p, t in parts:
        xyz.append(np.asarray(p, np.float64).reshape(-1, 3))
        tri.append(np.asarray(t, np.int64).reshape(-1, 3) + base)
        base += len(xyz[-1])
    return np.concatenate(xyz), np.concatenate(tri)


def _two_sheets(bridge):
    xyz, tri = join(sheet(9, 7, 21), sheet(8, 6, 22, at=(3.0, 0.0, 0.5)))
    if bridge:                                                                          # its indices are the first and the last of the list
        tri = np.concatenate([tri, [[0, len(xyz) - 1, 8]]])
    return _case(xyz, tri, seed=21)


def _islands():
    """sheets of 4, 24, 48, 24, 2 and 8 triangles (the two of 24 tie; the largest is neither first nor last), and three loose vertices"""
    xyz, tri = join(sheet(3, 2, 31, at=(9.0, 0.0, 0.0)), sheet(4, 5, 32, at=(2.0, 0.0, 0.0)), sheet(5, 7, 33), sheet(5, 4, 34, at=(4.0, 0.0, 0.0)),
                    (np.array([[7.0, 7.0, 7.0]] * 3), np.zeros((0, 3))), sheet(2, 2, 35, at=(6.0, 0.0, 0.0)), sheet(3, 3, 36, at=(7.0, 0.0, 0.0)))
    return _case(xyz, tri, seed=31)


def _unused_between():
    xyz, tri = sheet(6, 5, 41)
    spread = np.arange(len(xyz)) * 2 + 1                                                # used vertices at the odd places, loose ones between
    out = np.random.default_rng(41).normal(size=(2 * len(xyz) + 1, 3))
    out[spread] = xyz
    return _case(out, spread[tri], seed=41)


def _repeated_index():
    # two triangles and a third that names vertex 2 twice and vertex 3: it connects them, does not smooth and gives no normal
    xyz = [[0, 0, 0], [1, 0, 0.1], [0, 1, 0], [3, 0, 0], [4, 0, 0.2], [3, 1, 0], [9, 9, 9]]
    return _case(np.asarray(xyz) * 0.125, [[0, 1, 2], [3, 4, 5], [2, 2, 3], [6, 6, 6]], seed=42)


def _zero_area():
    # (3, 4, 5) is collinear with distinct indices: it smooths (D counts it) and gives no normal; vertex 5 has no other triangle
    xyz = [[0, 0, 0], [1, 0, 0], [0, 1, 0.25], [1, 1, 0], [2, 2, 0], [3, 3, 0]]
    return _case(np.asarray(xyz) * 0.125, [[0, 1, 2], [1, 3, 2], [3, 4, 5]], seed=43)


def fan(n_triangles):
    """n_triangles + 1 rim vertices around vertex 0, which is lifted off their plane: D_0 = 2 n_triangles"""
    a = np.arange(n_triangles + 1) * (1.5 * np.pi / n_triangles)
    rim = np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], axis=1)
    xyz = np.concatenate([[[0.0, 0.0, 0.5]], rim])
    r = np.arange(1, n_triangles + 1)
    return _case(xyz, np.stack([np.zeros_like(r), r, r + 1], axis=1), bgr=None, iterations=1)


def _halves():
    # quantum 0.25 about 0: +-0.125 and +-0.375 are quotients of +-0.5 and +-1.5; halves go up: 1, 0, 2, -1
    xyz = [[0.125, -0.125, 0.375], [-0.375, 0.125, 1.0], [1.0, -0.375, -0.125], [0.5, 0.5, 0.5]]
    return _case(xyz, [[0, 1, 2], [0, 2, 3]], quantum=0.25, iterations=0)


BIG = float((1 << 25) - 2)                 # 2^25 - 2 is a float32; about an origin of -+1 it quantises to +-(2^25 - 1)


def _rim(x0, origin_x):
    xyz = [[x0, 0, 0], [0, 100, 0], [0, 0, 100], [50, 50, 50]]
    return _case(xyz, [[0, 1, 2], [0, 2, 3], [0, 3, 1]], origin=(origin_x, 0.0, 0.0), quantum=1.0, iterations=1)


def _spike():
    # mu = -2 would carry vertex 0 from 2^25 - 1 to beyond the range: it stays where the L pass left it; vertex 1 moves
    c = _rim(BIG, -1.0)
    c.update(lam=1.0 / 65536.0, mu=-2.0, iterations=2)
    return c


def _bad_coordinate(value):
    c = dict(case("two_sheets"))
    c["xyz"] = c["xyz"].copy()
    c["xyz"][40, 1] = value
    return c


def _from_extraction(name, **params):
    e, m = mc.case(name), mc.mesh(name)
    return _case(m["xyz"], m["tri"], bgr=m["bgr"], origin=e["origin"], quantum=np.float32(e["voxel"]) / np.float32(1024.0), **params)


CASES = {
    "empty_0": lambda: _case(np.zeros((0, 3)), np.zeros((0, 3))),
    "empty_5": lambda: _case(np.random.default_rng(1).normal(size=(5, 3)), np.zeros((0, 3))),
    "one_triangle": lambda: _case([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], [[0, 1, 2]]),
    "two_sheets_bridge": lambda: _two_sheets(True),
    "two_sheets": lambda: _two_sheets(False),
    "strip_4096": lambda: _case(*strip(4098, 11, permute=True), seed=11, iterations=1),
    "all_256": lambda: _from_extraction("all_256"),
    "sphere_14": lambda: _from_extraction("sphere_14", iterations=10),
    "torus_18": lambda: _from_extraction("torus_18", iterations=10),
    "zeros_14": lambda: _from_extraction("zeros_14", iterations=10),
    "islands": _islands,
    "unused_between": _unused_between,
    "repeated_index": _repeated_index,
    "zero_area": _zero_area,
    "fan_65536": lambda: fan(65536),
    "fan_65537": lambda: fan(65537),
    "halves": _halves,
    "rim_plus": lambda: _rim(BIG, -1.0),
    "rim_minus": lambda: _rim(-BIG, 1.0),
    "spike": _spike,
    "iterations_0": with_params("two_sheets_bridge", iterations=0),
    "iterations_1": with_params("two_sheets_bridge", iterations=1),
    "iterations_10": with_params("two_sheets_bridge", iterations=10),
    "L_1": with_params("two_sheets", lam=1.0 / 65536.0),
    "L_65536": with_params("two_sheets", lam=1.0),
    "M_minus_1": with_params("two_sheets", mu=-1.0 / 65536.0),
    "M_minus_131072": with_params("two_sheets", mu=-2.0),
    "min_on_count": with_params("islands", min_triangles=24),
    "min_above_count": with_params("islands", min_triangles=25),
    "keep_largest": with_params("islands", keep_largest=1),
    "keep_largest_tie": with_params("all_256", keep_largest=1),
    "keep_largest_removed": with_params("islands", keep_largest=1, min_triangles=49),
    "no_colour": with_params("islands", bgr=None, min_triangles=8),
}
# vertex and triangle counts around a wave and a workgroup: a strip of n vertices has n - 2 triangles
for _n in (63, 64, 65, 66, 67, 255, 256, 257, 258, 259):
    CASES["strip_%d" % _n] = (lambda n: lambda: _case(*strip(n, n), seed=n))(_n)

# the calls that refuse: the coordinate is found on the device
REFUSED = {
    "rim_plus_refused": lambda: _rim(float(1 << 25), 0.0),
    "rim_minus_refused": lambda: _rim(-float(1 << 25), 0.0),
    "nan_coordinate": lambda: _bad_coordinate(np.nan),
    "inf_coordinate": lambda: _bad_coordinate(-np.inf),
}
ONE_COMPONENT = ("one_triangle", "two_sheets_bridge", "strip_4096", "sphere_14", "torus_18", "zeros_14", "fan_65536", "fan_65537")
SLOW_LOOP = ("fan_65536", "fan_65537")          # their Python loops take seconds: the CPU test runs the loop statement on one of them


@functools.lru_cache(maxsize=None)
def case(name):
    return (CASES.get(name) or REFUSED[name])()


def smooth_args(c):
    return (c["xyz"], c["tri"], c["origin"], c["quantum"], c["iterations"], c["lam"], c["mu"])


def clean_args(c):
    return (c["xyz"], c["bgr"], c["tri"], c["origin"], c["quantum"], c["min_triangles"], c["keep_largest"], c["iterations"], c["lam"], c["mu"])


@functools.lru_cache(maxsize=None)
def want(name):
    c = case(name)
    return dict(components=co.components_np(len(c["xyz"]), c["tri"]),
                filter=co.filter_np(c["xyz"], c["bgr"], c["tri"], c["min_triangles"], c["keep_largest"]),
                smooth=co.smooth_np(*smooth_args(c)), clean=co.clean(*clean_args(c)))
