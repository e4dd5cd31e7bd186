"""Named cases of the seam levelling, each the smallest shape at which its rule can go wrong (the contract is in include/sfmba.h,
"levelling the colours across seams").

A SCENE case is a dict: xyz, bgr, tri, images, K, P (the arguments of the texture call as tests/texture_cases.py states them), view int32
[T] GIVEN, radius, weight, passes, patch, blocks_per_row.  A PLANTED case is a dict of the level call's arguments alone: node_vertex, seen,
F, node_of, weight, passes -- nodes and colours that no geometry need produce.  want(name) / want_planted(name) is the restatement's
answer (the numpy statements), computed once and shared."""
import functools

import numpy as np

import colour_oracle as co
import label_cases as lc
import mesh_cases as mc
import texture_cases as tc
import texture_oracle as to


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def strip(nt):
    return lc.strip(nt)


def cameras(n_views, sizes=None, channels=3, seed=0):
    """n_views cameras on a ring in front of the plane z = 4, all looking at (0, 0, 4); images of different small sizes"""
    rng = np.random.default_rng(3000 + seed)
    sizes = sizes or [tc.SIZES[i % 4] for i in range(n_views)]
    K = mc.intrinsics(40, 30, 36.0)
    eyes = [(0.9 * np.cos(2.0 * np.pi * i / max(n_views, 1)), 0.7 * np.sin(2.0 * np.pi * i / max(n_views, 1)), 0.1 * (i % 3)) for i in range(n_views)]
    P = np.stack([mc.look_at(e, target=(0.0, 0.0, 4.0)) for e in eyes]) if n_views else np.zeros((0, 3, 4), np.float32)
    images = [rng.integers(0, 256, (h, w, 3) if channels == 3 else (h, w)).astype(np.uint8) for w, h in sizes[:n_views]]
    return images, K, P


def given(xyz, tri, images, K, P, view, bgr=None, radius=1, weight=16, passes=4, patch=4, blocks_per_row=None):
    tri = np.asarray(tri, np.int32).reshape(-1, 3)
    return dict(xyz=np.asarray(xyz, np.float32).reshape(-1, 3), bgr=bgr, tri=tri, images=images, K=K, P=P, view=np.asarray(view, np.int32).reshape(-1),
                radius=radius, weight=weight, passes=passes, patch=patch, blocks_per_row=blocks_per_row)


def plain_labels(nt, patch, radius=1, passes=4, **kw):
    """a scene of tests/texture_cases.py under the labels of the plain rule"""
    s = tc.scene(nt, patch, **kw)
    view, _ = to.views_np(s["xyz"], s["tri"], s["images"], s["K"], s["P"], s["depth_maps"], s["occl_tol"], s["min_area"])
    return given(s["xyz"], s["tri"], s["images"], s["K"], s["P"], view, bgr=s["bgr"], radius=radius, passes=passes, patch=patch,
                 blocks_per_row=s["blocks_per_row"])


def strip_scene(nt, n_views=3, run=5, seed=0, radius=1, passes=3, patch=3):
    """a strip on random points in front of the cameras; the labels change every `run` triangles and every 11th triangle has none"""
    rng = np.random.default_rng(4000 + seed + nt)
    xyz = np.concatenate([rng.uniform(-1.0, 1.0, (nt + 2, 2)), 4.0 + 0.05 * rng.uniform(-1, 1, (nt + 2, 1))], 1).astype(np.float32)
    images, K, P = cameras(n_views, seed=seed)
    t = np.arange(nt)
    view = np.where(t % 11 == 10, -1, (t // run) % n_views)
    return given(xyz, strip(nt), images, K, P, view, radius=radius, passes=passes, patch=patch)


def grid_scene(n_views, radius=1, weight=16, passes=8, patch=4):
    """the 9 x 9 vertices of an 8 x 8 sheet cut into 2 or 3 stripes or 4 quadrants: a vertex has up to n_views siblings"""
    xyz, bgr, tri = tc.sheet(128, 70 + n_views)
    images, K, P = cameras(n_views, seed=n_views)
    c = xyz[tri].mean(axis=1)
    if n_views == 4:
        view = (c[:, 0] > 0).astype(np.int32) + 2 * (c[:, 1] > 0).astype(np.int32)
    else:
        view = np.minimum(((c[:, 0] + 1.0) / 2.0 * n_views).astype(np.int32), n_views - 1)
    return given(xyz, tri, images, K, P, view, bgr=bgr, radius=radius, weight=weight, passes=passes, patch=patch)


def fan_scene(n_views, nt=300):
    """nt triangles on one vertex: its node in one view owns a run of nt entries; in nine views the vertex has nine siblings"""
    a = 2.0 * np.pi * np.arange(nt + 1) / nt
    xyz = np.concatenate([[[0.0, 0.0, 4.0]], np.stack([np.cos(a), np.sin(a), np.full(nt + 1, 4.0)], 1)]).astype(np.float32)
    tri = np.asarray([(0, 1 + t, 2 + t) for t in range(nt)], np.int32)
    images, K, P = cameras(n_views, sizes=[(20 + 2 * i, 15 + i) for i in range(n_views)], seed=50 + n_views)
    return given(xyz, tri, images, K, P, np.arange(nt) % n_views, passes=5, patch=3)


def _with(c, **kw):
    out = dict(c)
    out.update(kw)
    return out


def _spoiled():
    c = plain_labels(12, 4, seed=31)
    tri, xyz, view = c["tri"].copy(), c["xyz"].copy(), c["view"].copy()
    tri[3, 2] = tri[3, 0]                                     # a repeated index
    xyz[int(tri[8, 1]), 1] = np.nan                           # a NaN vertex: every triangle on it stops contributing
    view[:] = np.where(view < 0, 0, view)
    return _with(c, tri=tri, xyz=xyz, view=view)


def _exact(vertices, t=((0.0, 0.0, 0.0),), size=8, channels=3, radius=1, view=(0,), tri=((0, 1, 2),), patch=4, seed=5):
    s = tc.exact(vertices, tri=tri, t=t, size=size, channels=channels, patch=patch, seed=seed)
    return given(s["xyz"], s["tri"], s["images"], s["K"], s["P"], view, radius=radius, patch=patch, blocks_per_row=1)


def _sizes(channels):
    """a 1 x 1 and a 2 x 2 image beside a larger one"""
    xyz, bgr, tri = tc.sheet(8, 81)
    images, K, P = cameras(3, sizes=[(1, 1), (2, 2), (9, 7)], channels=channels, seed=81 + channels)
    return given(xyz, tri, images, K, P, np.arange(8) % 3, bgr=bgr, radius=2, patch=4)


def _disjoint(nt):
    """nt triangles that share no vertex: n_nodes = 3 T"""
    c = strip_scene(3 * nt, seed=9)
    return _with(c, tri=np.arange(3 * nt, dtype=np.int32).reshape(nt, 3), view=np.arange(nt, dtype=np.int32) % 3)


def _permuted(name, seed):
    c = case(name)
    order = np.random.default_rng(seed).permutation(len(c["tri"]))
    return _with(c, tri=c["tri"][order], view=c["view"][order])


def _sphere():
    s = lc.sphere_scene()
    view, _ = to.views_np(s["xyz"], s["tri"], s["images"], s["K"], s["P"], s["depth_maps"], s["occl_tol"], 0)
    return given(s["xyz"], s["tri"], s["images"], s["K"], s["P"], view, bgr=s["bgr"], passes=4, patch=3)


BEHIND = ((-1.0, 0.0, -1.0),) + tc.FRONT[1:]                   # q_2 = -1 for the first vertex: its node is blind
CORNER = ((5.0, -4.0, 1.0), (6.0, -4.0, 1.0), (5.0, -5.0, 1.0))  # u >= 8 > 7 and v <= -1 < 0: all three clamp to the image corner (7, 0)

CASES = {
    **{"nt_%d" % n: (lambda n=n: plain_labels(n, 4, blocks_per_row=2, n_views=4)) for n in (0, 1, 2, 3)},
    **{"strip_%d" % n: (lambda n=n: strip_scene(n)) for n in (21, 22, 43, 85, 86, 171)},
    **{"strip_%d" % n: (lambda n=n: strip_scene(n, radius=0, passes=2)) for n in (10922, 10923)},
    **{"grid_%d_views" % n: (lambda n=n: grid_scene(n)) for n in (2, 3, 4)},
    "fan_one_view": lambda: fan_scene(1),
    "fan_nine_views": lambda: fan_scene(9),
    "all_unlabelled": lambda: _with(grid_scene(2), view=np.full(128, -1, np.int32)),
    "one_labelled": lambda: _with(grid_scene(2), view=np.where(np.arange(128) == 37, 1, -1).astype(np.int32)),
    "spoiled_mesh": _spoiled,
    "blind_node": lambda: _exact(BEHIND),
    **{"corner_r%d" % r: (lambda r=r: _exact(CORNER, radius=r)) for r in (0, 1, 2)},
    "tiny_images_bgr": lambda: _sizes(3),
    "tiny_images_gray": lambda: _sizes(1),
    "gray": lambda: plain_labels(40, 4, seed=40, channels=1, n_views=4),
    "weight_1": lambda: grid_scene(3, weight=1),
    "weight_256": lambda: grid_scene(3, weight=256),
    **{"passes_%d" % n: (lambda n=n: _with(strip_scene(43, seed=2), passes=n)) for n in (0, 1, 2, 1024)},
    "disjoint": lambda: _disjoint(20),
    **{"patch_%d" % s: (lambda s=s: plain_labels(5 if s < 64 else 3, s, blocks_per_row=1, seed=s, n_views=4)) for s in (3, 4, 6, 64)},
    "grid_permuted": lambda: _permuted("grid_4_views", 7),
    "six_view_sphere": _sphere,
}
LARGE = ("strip_10922", "strip_10923", "six_view_sphere", "passes_1024")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def node_args(c):
    return (c["xyz"], c["tri"], c["images"], c["K"], c["P"], c["view"], c["radius"])


@functools.lru_cache(maxsize=None)
def want(name):
    """nodes, offsets with their statistics, and the levelled atlas of a scene case"""
    c = case(name)
    nd = co.nodes(*node_args(c))
    g, stats = co.level(nd["node_vertex"], nd["seen"], nd["F"], nd["node_of"], c["weight"], c["passes"])
    tex = co.texture_levelled(c["xyz"], c["bgr"], c["tri"], c["images"], c["K"], c["P"], c["view"], nd["node_of"], g, c["patch"], c["blocks_per_row"])
    return dict(nodes=nd, g=g, stats=stats, tex=tex)


# ---- planted nodes -------------------------------------------------------------------------------------------------------------------
def planted(node_vertex, F, node_of, seen=None, weight=16, passes=8):
    node_vertex = np.asarray(node_vertex, np.int32).reshape(-1)
    return dict(node_vertex=node_vertex, seen=np.ones(len(node_vertex), np.uint8) if seen is None else np.asarray(seen, np.uint8),
                F=np.asarray(F, np.int32).reshape(-1, 3), node_of=np.asarray(node_of, np.int32).reshape(-1, 3), weight=weight, passes=passes)


def _extremes(flip, m=40):
    """Colours at the two ends of the range, w = 1.  Vertex 0 has the nodes a (F = 0) and b (F = 65280); every vertex i >= 1 has p_i (F = 0)
    and q_i (F = 65280).  The rows (b, p_i, p_i+1) link b to the p, whose own seams push them UP, so b is pulled up although its seam
    pulls it down, and a, which wants g_b + 65280, runs into the clamp at +65280.  flip exchanges the colours: the clamp at -65280."""
    lo, hi = (65280, 0) if flip else (0, 65280)
    node_vertex = np.repeat(np.arange(m + 1), 2)
    F = np.where((np.arange(2 * (m + 1)) % 2 == 0)[:, None], lo, hi) * np.ones((1, 3), np.int64)
    return planted(node_vertex, F, [(1, 2 * i, 2 * (i + 1)) for i in range(1, m)], weight=1, passes=8)


def _halves():
    """two siblings one level apart and no link, w = 1: den = 2 and num = +1 for one, -1 for the other"""
    return planted([0, 0, 1, 1, 1], [[100, 7, 0], [101, 6, 1], [5, 5, 5], [8, 2, 5], [6, 5, 5]], np.zeros((0, 3), np.int32), weight=1, passes=3)


def _planted_grid(n=33, step=20 * 256, weight=16, passes=16):
    """the n x n grid split into two views down the middle column with a planted step: the prototype's scene"""
    at = lambda y, x: y * n + x
    tri = np.asarray([t for y in range(n - 1) for x in range(n - 1)
                      for t in ((at(y, x), at(y + 1, x), at(y, x + 1)), (at(y + 1, x + 1), at(y, x + 1), at(y + 1, x)))], np.int32)
    view = (np.asarray([min(at_ % n for at_ in t) for t in tri.tolist()]) >= n // 2).astype(np.int32)
    nd = co.nodes_np(np.zeros((n * n, 3), np.float32), tri, view)
    rng = np.random.default_rng(33)
    base = 30000 + rng.integers(-2000, 2000, (n * n, 3))
    F = base[nd["node_vertex"]] + np.where(nd["node_view"] == 1, step, 0)[:, None]
    return planted(nd["node_vertex"], F, nd["node_of"], weight=weight, passes=passes)


def _blind_among():
    c = _planted_grid(9, passes=6)
    seen = c["seen"].copy()
    seen[[3, 40, 41]] = 0
    return dict(c, seen=seen)


PLANTED = {
    "no_nodes": lambda: planted([], np.zeros((0, 3)), np.full((4, 3), -1), passes=3),
    "no_triangles": lambda: planted([0, 0, 1], [[10, 20, 30], [50, 60, 70], [1, 2, 3]], np.zeros((0, 3)), passes=3),
    "clamp_high": lambda: _extremes(False),
    "clamp_low": lambda: _extremes(True),
    "halves": _halves,
    "planted_grid": _planted_grid,
    "planted_grid_w1": lambda: _planted_grid(17, weight=1, passes=5),
    "planted_grid_w256": lambda: _planted_grid(17, weight=256, passes=5),
    "blind_among": _blind_among,
    "unused_nodes": lambda: planted([0, 0, 2, 2, 5, 7], np.arange(18).reshape(6, 3) * 1000, [[0, 2, 4], [-1, -1, -1], [1, 3, 4]], passes=4),
}


@functools.lru_cache(maxsize=None)
def planted_case(name):
    return PLANTED[name]()


def level_args(c):
    return (c["node_vertex"], c["seen"], c["F"], c["node_of"], c["weight"], c["passes"])


@functools.lru_cache(maxsize=None)
def want_planted(name):
    g, stats = co.level(*level_args(planted_case(name)))
    return dict(g=g, stats=stats)


# ---- the quality scene: the texture suite's plane under two views, the second photograph brighter by 20 levels -------------------------
QUALITY_STEP, QUALITY_AMPLITUDE = 20, 0.85


@functools.lru_cache(maxsize=None)
def quality_scene():
    """tests/texture_cases.py's plane at depth 10 under two 160 x 120 views at +-15 degrees.  The pattern's swing about 127.5 is scaled to
    0.85 of its own (27.5 .. 227.5 becomes 42.5 .. 212.5), so that the second photograph + 20 stays below 255: nothing saturates."""
    s = dict(tc.quality_scene())
    images = []
    for i, im in enumerate(s["images"]):
        v = np.floor(127.5 + QUALITY_AMPLITUDE * (im.astype(np.float64) - 127.5) + 0.5) + (QUALITY_STEP if i == 1 else 0)
        assert v.min() >= 1 and v.max() <= 254
        images.append(v.astype(np.uint8))
    s["images"] = images
    return s


# MEASURED ONCE on the restatement on this scene under the labels of the plain rule at the defaults 16 passes / seam weight 16 / sample
# radius 1: the summed spread falls from 138084 to 3356, a ratio of 0.024304, and no texel clamps (written to
# profiles/texture_level.txt).  The ratio is below 1/8, so the gate of the tests is TWICE THE MEASURED RATIO, not 1/4.
QUALITY_RATIO_MEASURED_PPM = 24304
QUALITY_PARAMS = dict(k=4, rings=0, penalty=256, max_passes=0, radius=1, weight=16, passes=16)


@functools.lru_cache(maxsize=None)
def quality_want():
    s, p = quality_scene(), QUALITY_PARAMS
    return co.texture_adjust(s["xyz"], s["bgr"], s["tri"], s["images"], s["K"], s["P"], s["depth_maps"], s["occl_tol"], s["min_area"], s["patch"],
                             s["blocks_per_row"], p["k"], p["rings"], p["penalty"], p["max_passes"], p["radius"], p["weight"], p["passes"])
