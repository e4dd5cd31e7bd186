"""Named cases of the view-label smoothing, each the smallest shape at which its rule can go wrong (the contract is in include/sfmba.h,
"smoothing the view labels").

A case is a dict: tri int32 [T, 3], n_images, k, rings, penalty, max_passes, and EITHER scene (the arguments of the texture call as
tests/texture_cases.py states them: the candidates come from the geometry, and the combined call runs too) OR cand = (cand_view,
cand_score), PLANTED lists that no geometry need produce.  want(name) is the restatement's answer (the numpy statements), computed once
and shared: cand_view, cand_score, adj with its three counts, and the smoothing's result."""
import functools

import numpy as np

import label_oracle as lo
import mesh_cases as mc
import texture_cases as tc

TOP = 1 << 37


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def strip(nt):
    """triangle t on the vertices t, t + 1, t + 2: a chain, t linked to t - 1 and t + 1, the edge (t, t + 2) open"""
    return np.asarray([(t, t + 1, t + 2) for t in range(nt)], np.int32).reshape(-1, 3)


def sheet_tri(nt, seed=7):
    return tc.sheet(nt, seed)[2]


# ---- planted lists ------------------------------------------------------------------------------------------------------------------------
def random_lists(nt, n_images, k, seed, lo_score=1, hi_score=1 << 20, empty=0.1, tie=0.2):
    """valid candidate lists: a random number of distinct views per triangle, descending scores, equal scores in ascending view index"""
    rng = np.random.default_rng(seed)
    cv, cs = np.full((nt, k), -1, np.int32), np.zeros((nt, k), np.int64)
    for t in range(nt):
        m = 0 if rng.random() < empty else int(rng.integers(1, min(k, n_images) + 1))
        views = rng.permutation(n_images)[:m]
        scores = rng.integers(lo_score, hi_score, m)
        if m > 1 and rng.random() < tie:
            scores[1] = scores[0]
        order = sorted(range(m), key=lambda i: (-int(scores[i]), int(views[i])))
        cv[t, :m], cs[t, :m] = views[order], scores[order]
    return cv, cs


def planted(tri, n_images=5, k=4, seed=0, rings=2, penalty=256, max_passes=100, **kw):
    tri = np.asarray(tri, np.int32).reshape(-1, 3)
    return dict(tri=tri, n_images=n_images, k=k, rings=rings, penalty=penalty, max_passes=max_passes, scene=None,
                cand=random_lists(len(tri), n_images, k, 100 + seed, **kw))


def with_lists(tri, cv, cs, n_images, rings, penalty, max_passes):
    cv, cs = np.asarray(cv, np.int32), np.asarray(cs, np.int64)
    return dict(tri=np.asarray(tri, np.int32).reshape(-1, 3), n_images=n_images, k=cv.shape[1], rings=rings, penalty=penalty, max_passes=max_passes,
                scene=None, cand=(cv, cs))


def from_scene(scene, k=4, rings=2, penalty=256, max_passes=100):
    return dict(tri=scene["tri"], n_images=len(scene["images"]), k=k, rings=rings, penalty=penalty, max_passes=max_passes, scene=scene, cand=None)


def _permuted_strip(nt, seed):
    order = np.random.default_rng(seed).permutation(nt)
    return strip(nt)[order]


def _hole(nt):
    """a sheet in which one triangle in the middle has no candidate"""
    c = planted(sheet_tri(nt), seed=31, empty=0.0)
    c["cand"][0][nt // 2] = -1
    c["cand"][1][nt // 2] = 0
    return c


def _repeated(nt):
    tri = strip(nt)
    tri[5, 2] = tri[5, 0]
    return planted(tri, seed=32)


def chain(max_passes, n=257, penalty=256):
    """A front that advances ONE triangle per pass with the same gain every time.  Chain triangle t = (t, t + 1, t + 2) has the anchor
    triangle n + t on its open edge.  Anchors and chain triangle 0 list only view 1.  Chain triangles 1 .. n-1 list view 0 (1000) and view
    1 (999: D = 1) and start at view 0.  With two neighbours at view 0 a chain triangle stays (e = p against 1 + 2 p); once its left
    neighbour shows view 1 it moves (e = 2 p against 1 + p: gain p - 1), and only then does its right neighbour want to."""
    tri = np.concatenate([strip(n), np.asarray([(t + 2, t, n + 2 + t) for t in range(n)], np.int32)])
    cv, cs = np.full((2 * n, 2), -1, np.int32), np.zeros((2 * n, 2), np.int64)
    cv[:, 0], cs[:, 0] = 1, 1000
    cv[1:n, 0], cv[1:n, 1], cs[1:n, 1] = 0, 1, 999
    return with_lists(tri, cv, cs, 2, 0, penalty, max_passes)


def _top_scores(rings):
    """every triangle of a sheet lists the same four views with scores just under 2^37: the diffused sums come as near 2^53 as they can"""
    tri = sheet_tri(128)
    rng = np.random.default_rng(41)
    cs = np.sort(TOP - 1 - rng.integers(0, 1000, (len(tri), 4)), axis=1)[:, ::-1]
    cs[0] = TOP - 1
    cv = np.tile(np.arange(4, dtype=np.int32), (len(tri), 1))
    return with_lists(tri, cv, cs, 4, rings, 256, 100)


def _exact_D():
    """1024 (1024 - 512) / 1024 = 512, 1024 (1000 - 375) / 1000 = 640, 1024 * 999 / 1024 = 999: quotients on an integer, and one just below"""
    tri = strip(4)
    cv = np.asarray([[0, 1, -1], [1, 0, -1], [0, 1, 2], [2, 0, 1]], np.int32)
    cs = np.asarray([[1024, 512, 0], [1000, 375, 0], [1024, 25, 24], [1 << 36, (1 << 36) - (1 << 26), 1]], np.int64)
    return with_lists(tri, cv, cs, 3, 0, 300, 10)


def _equal_scores():
    c = dict(tc.exact(tc.FRONT, t=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))))
    return from_scene(c, k=2)


@functools.lru_cache(maxsize=None)
def sphere_scene(min_area=0):
    c, m = mc.integration_case("six_view_sphere"), mc.grid_mesh("six_view_sphere")
    return dict(xyz=m["xyz"], bgr=m["bgr"], tri=m["tri"], images=c["images"], K=c["K"], P=c["P"], depth_maps=c["depth_maps"],
                occl_tol=2.0 * float(c["voxel"]), min_area=min_area, patch=3, blocks_per_row=None, want_score=True)


CASES = {
    # sizes, through the geometry
    "nt_0": lambda: from_scene(tc.scene(0, 4, 2, n_views=4)),
    "nt_1": lambda: from_scene(tc.scene(1, 4, 2, n_views=4)),
    "nt_2": lambda: from_scene(tc.scene(2, 4, 2, n_views=4)),
    **{"sheet_%d" % n: (lambda n=n: from_scene(tc.scene(n, 3, n_views=4, seed=n, null_maps=(2,)))) for n in (63, 64, 65, 255, 256, 257)},
    "no_images": lambda: from_scene(tc.scene(7, 4, seed=41, n_views=0)),
    "three_views_k8": lambda: from_scene(tc.scene(40, 4, seed=43, n_views=3), k=8),
    "k1_nothing_moves": lambda: from_scene(tc.scene(40, 4, seed=44, n_views=4), k=1, rings=3),
    "equal_scores_scene": _equal_scores,
    "spoiled_mesh": lambda: from_scene(tc.case("repeated_index")),
    "nan_coordinate": lambda: from_scene(tc.case("nan_coordinate")),
    "min_area_floor": lambda: from_scene(tc.scene(60, 4, seed=45, n_views=4, min_area=2600)),
    # strips with planted lists
    **{"strip_%d" % n: (lambda n=n: planted(strip(n), seed=n)) for n in (63, 64, 65, 255, 256, 257)},
    "strip_permuted": lambda: planted(_permuted_strip(65, 3), seed=3),
    "three_on_an_edge": lambda: planted([(0, 1, 2), (0, 1, 3), (1, 0, 4), (2, 1, 5), (5, 1, 6)], seed=4, empty=0.0),
    "four_on_an_edge": lambda: planted([(0, 1, 2), (0, 1, 3), (1, 0, 4), (0, 1, 5), (2, 1, 5)], seed=5, empty=0.0),
    "doubled_triangle": lambda: planted([(0, 1, 2), (2, 1, 0), (3, 4, 5), (4, 3, 6)], seed=6, empty=0.0),
    "repeated_index": lambda: _repeated(12),
    "hole_in_a_region": lambda: _hole(32),
    "k1_planted": lambda: planted(sheet_tri(40), k=1, seed=8),
    "equal_scores": lambda: planted(sheet_tri(40), seed=9, tie=1.0, empty=0.0),
    **{"chain_%d" % p: (lambda p=p: chain(p)) for p in (1, 2, 100)},
    "penalty_0": lambda: planted(sheet_tri(64), seed=10, penalty=0),
    "penalty_65535": lambda: planted(sheet_tri(64), seed=10, penalty=65535),
    **{"top_scores_r%d" % r: (lambda r=r: _top_scores(r)) for r in (0, 1, 8)},
    "exact_D": _exact_D,
    "rings_8_passes_0": lambda: planted(sheet_tri(200), seed=11, rings=8, max_passes=0),
    "k8_sheet": lambda: planted(sheet_tri(200), n_images=9, k=8, seed=12, rings=4),
    # the texture suite's six-view sphere, every triangle with an area
    "six_view_sphere": lambda: from_scene(sphere_scene(), rings=4),
}
SMALL = [n for n in CASES if n != "six_view_sphere"]
SCENES = ("nt_0", "nt_1", "nt_2", "sheet_63", "sheet_64", "sheet_65", "sheet_255", "sheet_256", "sheet_257", "no_images", "three_views_k8",
          "k1_nothing_moves", "equal_scores_scene", "spoiled_mesh", "nan_coordinate", "min_area_floor")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def candidate_args(c):
    s = c["scene"]
    return (s["xyz"], s["tri"], s["images"], s["K"], s["P"], s["depth_maps"], s["occl_tol"], s["min_area"], c["k"])


def lists_of(c, fn=lo.candidates_np):
    return c["cand"] if c["scene"] is None else fn(*candidate_args(c))


@functools.lru_cache(maxsize=None)
def want(name):
    c = case(name)
    cv, cs = lists_of(c)
    adj, n_pairs, n_open, n_nonmanifold = lo.adjacency_sort(c["tri"])
    sm = lo.smooth_np(cv, cs, adj, c["rings"], c["penalty"], c["max_passes"])
    return dict(cand_view=cv, cand_score=cs, adj=adj, n_pairs=n_pairs, n_open_edges=n_open, n_nonmanifold_edges=n_nonmanifold, smooth=sm)


def texture_args(c):
    s = c["scene"]
    return (s["xyz"], s["bgr"], s["tri"], s["images"], s["K"], s["P"], s["depth_maps"], s["occl_tol"], s["min_area"], s["patch"], s["blocks_per_row"])


@functools.lru_cache(maxsize=None)
def want_texture(name):
    c = case(name)
    return lo.texture_smooth(*texture_args(c), c["k"], c["rings"], c["penalty"], c["max_passes"])


# ---- the quality scene: a noisy wall under five cameras -------------------------------------------------------------------------------------
WALL_CELLS, WALL_CELL, WALL_Z, WALL_RELIEF, WALL_NOISE, WALL_F, WALL_SIZE = 96, 0.05, 10.0, 0.3, 0.01, 800.0, (1024, 512)
WALL_PARAMS = dict(k=4, rings=8, penalty=256, max_passes=100)


@functools.lru_cache(maxsize=None)
def wall():
    """96 x 96 cells of 0.05 at depth 10 with the relief 0.3 sin x and vertex noise of sigma 0.01; five cameras 1.5 apart along x, all
    looking down +z, f = 800; no depth maps, constant images; the triangles face the cameras (positive scores)"""
    rng = np.random.default_rng(2024)
    n = WALL_CELLS
    g = (np.arange(n + 1) - n / 2.0) * WALL_CELL
    X, Y = np.meshgrid(g, g)
    Z = WALL_Z + WALL_RELIEF * np.sin(X)
    xyz = (np.stack([X, Y, Z], -1) + WALL_NOISE * rng.standard_normal((n + 1, n + 1, 3))).reshape(-1, 3).astype(np.float32)
    at = lambda y, x: y * (n + 1) + x
    tri = np.asarray([t for y in range(n) for x in range(n)
                      for t in ((at(y, x), at(y + 1, x), at(y, x + 1)), (at(y + 1, x + 1), at(y, x + 1), at(y + 1, x)))], np.int32)
    w, h = WALL_SIZE
    K = np.array([[WALL_F, 0, (w - 1) / 2.0], [0, WALL_F, (h - 1) / 2.0], [0, 0, 1]], np.float32)
    P = np.zeros((5, 3, 4), np.float32)
    P[:, :, :3] = np.eye(3)
    P[:, 0, 3] = -1.5 * (np.arange(5) - 2)
    images = [np.full((h, w), 128, np.uint8) for _ in range(5)]
    return dict(xyz=xyz, bgr=None, tri=tri, images=images, K=K, P=P, depth_maps=[None] * 5, occl_tol=0.0, min_area=0, patch=3, blocks_per_row=None,
                want_score=True)


@functools.lru_cache(maxsize=None)
def wall_want():
    c = wall()
    cv, cs = lo.candidates_np(c["xyz"], c["tri"], c["images"], c["K"], c["P"], c["depth_maps"], c["occl_tol"], c["min_area"], WALL_PARAMS["k"])
    adj = lo.adjacency_sort(c["tri"])[0]
    sm = lo.smooth_np(cv, cs, adj, WALL_PARAMS["rings"], WALL_PARAMS["penalty"], WALL_PARAMS["max_passes"])
    return dict(cand_view=cv, cand_score=cs, adj=adj, smooth=sm)


def mean_area_given_up(cand_score, cand_view, view):
    """the mean of D / 1024 over the triangles with a label"""
    cs, cv = np.asarray(cand_score, np.int64), np.asarray(cand_view)
    rank = np.argmax(cv == np.asarray(view)[:, None], axis=1)
    has = np.asarray(view) >= 0
    D = (1024 * (cs[:, 0] - cs[np.arange(len(cs)), rank])) // np.maximum(cs[:, 0], 1)
    return float(D[has].mean() / 1024.0)
