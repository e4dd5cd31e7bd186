"""Named cases of sfmba_mesh_texture, each the smallest shape at which its rule can go wrong (the contract is in include/sfmba.h).

A case is a dict of the arguments of texture_oracle.texture / capi.mesh_texture: xyz, bgr, tri, images, K, P, depth_maps, occl_tol,
min_area, patch, blocks_per_row, want_score.  want(name) is the restatement's answer (numpy statements), computed once and shared."""
import functools

import numpy as np

import mesh_cases as mc
import texture_oracle as to


# ---- a generic scene: a jittered sheet in front of a few cameras ------------------------------------------------------------------
def sheet(nt, seed, jitter=0.05):
    """the first nt triangles of a c x c grid of cells over [-1, 1]^2 at z = 4, every one facing a camera at the origin that looks
    down +z (x right, y down): (v00, v01, v10) and (v11, v10, v01)"""
    rng = np.random.default_rng(seed)
    c = max(1, int(np.ceil(np.sqrt((nt + 1) // 2))))
    g = np.linspace(-1.0, 1.0, c + 1)
    xyz = np.stack([np.repeat(g[None, :], c + 1, 0), np.repeat(g[:, None], c + 1, 1), 4.0 + jitter * rng.uniform(-1, 1, (c + 1, c + 1))], -1)
    at = lambda y, x: y * (c + 1) + x
    tri = []
    for y in range(c):
        for x in range(c):
            tri += [(at(y, x), at(y + 1, x), at(y, x + 1)), (at(y + 1, x + 1), at(y, x + 1), at(y + 1, x))]
    xyz = xyz.reshape(-1, 3).astype(np.float32)
    return xyz, rng.integers(0, 256, (len(xyz), 3)).astype(np.uint8), np.asarray(tri[:nt], np.int32).reshape(-1, 3)


EYES = ((0.0, 0.0, 0.0), (1.0, 0.2, 0.0), (-0.8, -0.3, 0.3), (0.3, 0.9, -0.2))
SIZES = ((40, 30), (48, 36), (36, 40), (44, 32))


def plane_depth(K, P, w, h, z_world):
    """the z-depth at which every pixel's ray meets the plane z = z_world, float32 [h, w]"""
    K, P = np.asarray(K, np.float64), np.asarray(P, np.float64)
    R, t = P[:, :3], P[:, 3]
    eye = -R.T @ t
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1) @ R
    return ((z_world - eye[2]) / d[..., 2]).astype(np.float32)


def scene(nt, patch, blocks_per_row=None, n_views=2, channels=3, seed=1, null_maps=(), holes=0.04, min_area=0, want_score=True, bgr=True):
    rng = np.random.default_rng(1000 + seed)
    xyz, col, tri = sheet(nt, seed)
    K = mc.intrinsics(40, 30, 36.0)
    P = np.stack([mc.look_at(e, target=(0.0, 0.0, 4.0)) for e in EYES[:n_views]]) if n_views else np.zeros((0, 3, 4), np.float32)
    images, maps = [], []
    for i in range(n_views):
        w, h = SIZES[i]
        images.append(rng.integers(0, 256, (h, w, 3) if channels == 3 else (h, w)).astype(np.uint8))
        m = plane_depth(K, P[i], w, h, 4.0)
        m[rng.random(m.shape) < holes] = 0.0
        maps.append(None if i in null_maps else m)
    return dict(xyz=xyz, bgr=col if bgr else None, tri=tri, images=images, K=K, P=P, depth_maps=maps, occl_tol=0.25, min_area=min_area,
                patch=patch, blocks_per_row=blocks_per_row, want_score=want_score)


# ---- exact scenes: fx = fy = 1, cx = cy = 3, an 8 x 8 image, identity rotation, points at z = 1, so u = x + t_x + 3 exactly -------
def exact(vertices, tri=((0, 1, 2),), t=((0.0, 0.0, 0.0),), maps=None, occl_tol=0.25, min_area=0, patch=4, colours=None, channels=3, seed=5,
          blocks_per_row=1, size=8):
    rng = np.random.default_rng(2000 + seed)
    K = np.array([[1, 0, 3], [0, 1, 3], [0, 0, 1]], np.float32)
    P = np.zeros((len(t), 3, 4), np.float32)
    P[:, :, :3] = np.eye(3)
    P[:, :, 3] = np.asarray(t, np.float32).reshape(-1, 3)
    images = [rng.integers(0, 256, (size, size, 3) if channels == 3 else (size, size)).astype(np.uint8) for _ in t]
    xyz = np.asarray(vertices, np.float32).reshape(-1, 3)
    bgr = None if colours is None else np.asarray(colours, np.uint8).reshape(-1, 3)
    return dict(xyz=xyz, bgr=bgr, tri=np.asarray(tri, np.int32).reshape(-1, 3), images=images, K=K, P=P,
                depth_maps=[None] * len(t) if maps is None else maps, occl_tol=occl_tol, min_area=min_area, patch=patch,
                blocks_per_row=blocks_per_row, want_score=True)


FRONT = ((-1.0, 0.0, 1.0), (-1.0, 2.0, 1.0), (1.0, 0.0, 1.0))          # u, v = (2, 3), (2, 5), (4, 3): a2 = -32 * 32 = -1024
LEFT = ((-3.0, 0.0, 1.0), (-3.0, 2.0, 1.0), (-1.0, 0.0, 1.0))          # A and B exactly on u = 0
RIGHT = ((2.0, 0.0, 1.0), (2.0, 2.0, 1.0), (4.0, 0.0, 1.0))            # C exactly on u = w - 1 = 7
ULP_3, ULP_4 = 2.0 ** -51, 2.0 ** -50                                  # one double at 3 and at 4 .. 8
COLOURS = ((10, 200, 30), (250, 0, 90), (60, 70, 255))


def _map(value, zero_at=()):
    m = np.full((8, 8), value, np.float32)
    for y, x in zero_at:
        m[y, x] = 0.0
    return m


def _spoiled(nt, what):
    c = scene(nt, 4, seed=31)
    if what == "repeated":
        c["tri"] = c["tri"].copy()
        c["tri"][3, 2] = c["tri"][3, 0]
    else:
        c["xyz"] = c["xyz"].copy()
        c["xyz"][int(c["tri"][3, 1]), 1] = what
    return c


def permuted_views(c, order):
    out = dict(c)
    out["images"] = [c["images"][i] for i in order]
    out["depth_maps"] = [c["depth_maps"][i] for i in order]
    out["P"] = np.ascontiguousarray(c["P"][list(order)])
    return out


def bgr_of_gray(c):
    out = dict(c)
    out["images"] = [np.ascontiguousarray(np.repeat(im[..., None], 3, 2)) for im in c["images"]]
    return out


PERMUTATION = (2, 0, 3, 1)

CASES = {
    # sizes
    "nt_0": lambda: scene(0, 4, 2),
    "nt_1": lambda: scene(1, 4, 2),
    "nt_2": lambda: scene(2, 4, 2),
    "nt_3": lambda: scene(3, 4, 2),
    **{"nt_%d" % n: (lambda n=n: scene(n, 3, seed=n)) for n in (63, 64, 65, 255, 256, 257)},
    "blocks_8_of_9": lambda: scene(16, 4, 3, seed=16),
    "blocks_9_of_9": lambda: scene(18, 4, 3, seed=18),
    "blocks_9_odd": lambda: scene(17, 4, 3, seed=17),
    "blocks_10_of_9": lambda: scene(20, 4, 3, seed=20),
    "one_column_S3": lambda: scene(5, 3, 1, seed=3),
    "one_column_S4": lambda: scene(5, 4, 1, seed=4),
    "one_column_S6": lambda: scene(5, 6, 1, seed=6),
    "one_column_S64": lambda: scene(3, 64, 1, seed=64),
    # the candidate rules, exactly
    "front": lambda: exact(FRONT),
    "behind_zero": lambda: exact(((-1.0, 0.0, 0.0),) + FRONT[1:]),                               # q_2 = 0
    "behind_minus": lambda: exact(((-1.0, 0.0, -1.0),) + FRONT[1:]),
    "on_u_0": lambda: exact(LEFT),
    "outside_u_0": lambda: exact(LEFT, t=((-ULP_3, 0.0, 0.0),)),                                 # u = -2^-51
    "on_u_w1": lambda: exact(RIGHT),
    "outside_u_w1": lambda: exact(RIGHT, t=((ULP_4, 0.0, 0.0),)),                                # u = 7 + 2^-50
    "back_facing": lambda: exact((FRONT[0], FRONT[2], FRONT[1])),
    "identical_views": lambda: exact(FRONT, t=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))),
    "on_min_area": lambda: exact(FRONT, min_area=1024),
    "below_min_area": lambda: exact(FRONT, min_area=1025),
    "no_area": lambda: exact((FRONT[0], FRONT[1], (-1.0, 1.0, 1.0))),                            # three distinct points on a line
    "on_occl_tol": lambda: exact(FRONT, maps=[_map(0.75)]),                                      # q_2 - zs = 0.25
    "above_occl_tol": lambda: exact(FRONT, t=((0.0, 0.0, 2.0 ** -52),), maps=[_map(0.75)]),      # q_2 - zs = 0.25 + 2^-52
    "zs_zero": lambda: exact(FRONT, maps=[_map(1.0, zero_at=((5, 2),))]),                        # B's pixel
    "null_map_beside": lambda: exact(FRONT, t=((0.0, 0.0, 0.0),) * 3, maps=[_map(1.0, zero_at=((5, 2),)), None, _map(1.0)]),
    # images
    "gray": lambda: scene(12, 4, seed=40, channels=1),
    "gray_as_bgr": lambda: bgr_of_gray(case("gray")),
    "no_images": lambda: scene(7, 4, seed=41, n_views=0),
    "four_views": lambda: scene(40, 5, seed=42, n_views=4, null_maps=(2,)),
    "four_views_permuted": lambda: permuted_views(case("four_views"), PERMUTATION),
    # the mesh
    "nan_coordinate": lambda: _spoiled(12, np.nan),
    "inf_coordinate": lambda: _spoiled(12, np.inf),
    "repeated_index": lambda: _spoiled(12, "repeated"),
    # the fallback: S = 4, so a sum s gives floor(s / 2 + 1 / 2); the texel (3, 0) has the weights -1, 3, 0 and (1, 0) has 1, 1, 0
    "fallback_halves": lambda: exact(FRONT + ((0.0, 0.0, 1.0),) * 3, tri=((0, 1, 2), (3, 4, 5)), t=(),
                                     colours=((1, 2, 7), (0, 1, 2), (0, 0, 0), (0, 200, 255), (1, 0, 255), (9, 9, 9))),
    "fallback_no_colour": lambda: scene(5, 4, seed=43, n_views=0, bgr=False),
    "no_colour": lambda: scene(9, 4, seed=44, bgr=False),
    # the gutter: RIGHT's texel (0, 3) is (-A + 3 C) / 2 = (5, 0, 1), u = 8 > 7 (clamped); with A at z = 3 and B at z = 1 the texel
    # (3, 0) is (-A + 3 B) / 2 at z = 0 (the fallback)
    "texel_clamped": lambda: exact(RIGHT, colours=COLOURS),
    "texel_behind": lambda: exact(((0.0, 0.0, 3.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0)), colours=COLOURS),
    "score_null": lambda: dict(scene(9, 4, seed=45), want_score=False),
}

REFUSED = {
    "index_high": lambda: dict(scene(6, 4, seed=50), tri=np.asarray([[0, 1, 2], [0, 1, 16]], np.int32)),
    "index_negative": lambda: dict(scene(6, 4, seed=50), tri=np.asarray([[0, -1, 2]], np.int32)),
    "atlas_too_wide": lambda: scene(2, 64, 253, seed=51),                                        # W = 253 * 65 = 16445
    "atlas_too_high": lambda: scene(10924, 3, 1, seed=52, n_views=0),                            # H = 5462 * 3 = 16386
}


@functools.lru_cache(maxsize=None)
def case(name):
    return (CASES.get(name) or REFUSED[name])()


def args(c):
    return (c["xyz"], c["bgr"], c["tri"], c["images"], c["K"], c["P"], c["depth_maps"], c["occl_tol"], c["min_area"], c["patch"],
            c["blocks_per_row"], c["want_score"])


@functools.lru_cache(maxsize=None)
def want(name):
    return to.texture(*args(case(name)))


# ---- the quality scene: a plane at depth 10 under two views at +-15 degrees, an analytic pattern through the true homography -------
PLANE_Z, PLANE_HALF, QUALITY_SIZE, QUALITY_F = 10.0, 1.8, (160, 120), 300.0


def pattern(x, y):
    """the pattern on the plane, 0..255 as float64 [..., 3]; at f / z = 30 px per unit the shortest period, 0.8 units, is 24 px in
    a frontal view and at least 16 px under any foreshortening down to 2 / 3"""
    two_pi = 2.0 * np.pi
    b = 127.5 + 100.0 * np.sin(two_pi * x / 0.8) * np.cos(two_pi * y / 1.1)
    g = 127.5 + 100.0 * np.sin(two_pi * (x + y) / 1.3)
    r = 127.5 + 100.0 * np.cos(two_pi * (x - 0.5 * y) / 0.9)
    return np.stack([b, g, r], -1)


@functools.lru_cache(maxsize=None)
def quality_scene():
    w, h = QUALITY_SIZE
    K = mc.intrinsics(w, h, QUALITY_F)
    eyes = [(PLANE_Z * np.sin(a), 0.0, PLANE_Z - PLANE_Z * np.cos(a)) for a in np.radians((15.0, -15.0))]
    P = np.stack([mc.look_at(e, target=(0.0, 0.0, PLANE_Z)) for e in eyes])
    g = np.linspace(-PLANE_HALF, PLANE_HALF, 9)
    xyz = np.stack([np.repeat(g[None, :], 9, 0), np.repeat(g[:, None], 9, 1), np.full((9, 9), PLANE_Z)], -1).reshape(-1, 3).astype(np.float32)
    at = lambda y, x: y * 9 + x
    tri = np.asarray([t for y in range(8) for x in range(8)
                      for t in ((at(y, x), at(y + 1, x), at(y, x + 1)), (at(y + 1, x + 1), at(y, x + 1), at(y + 1, x)))], np.int32)
    images, maps = [], []
    Kd = K.astype(np.float64)
    for p in P.astype(np.float64):
        R, t = p[:, :3], p[:, 3]
        eye = -R.T @ t
        xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        d = np.stack([(xs - Kd[0, 2]) / Kd[0, 0], (ys - Kd[1, 2]) / Kd[1, 1], np.ones_like(xs)], -1) @ R
        s = (PLANE_Z - eye[2]) / d[..., 2]
        X = eye + s[..., None] * d                                                             # where each pixel's ray meets the plane
        images.append(np.clip(np.floor(pattern(X[..., 0], X[..., 1]) + 0.5), 0, 255).astype(np.uint8))
        maps.append(s.astype(np.float32))
    return dict(xyz=xyz, bgr=np.full((len(xyz), 3), 128, np.uint8), tri=tri, images=images, K=K, P=P, depth_maps=maps, occl_tol=0.05, min_area=256,
                patch=6, blocks_per_row=None, want_score=True)


def quality_error(c, out):
    """the mean absolute difference between the texels with non-negative weights and the pattern at their own point of the plane"""
    S, nt = c["patch"], len(c["tri"])
    H, W = out["atlas"].shape[:2]
    owner, i, j = to.ownership(nt, S, W // (S + 1), W, H)
    inside = (owner >= 0) & (S - 2 - i - j >= 0)
    X = c["xyz"].astype(np.float64)[c["tri"].astype(np.int64)][np.where(inside, owner, 0)]
    wA, wB, wC = ((a.astype(np.float64) / (S - 2))[..., None] for a in (S - 2 - i - j, i, j))
    Xp = wA * X[:, :, 0] + wB * X[:, :, 1] + wC * X[:, :, 2]
    diff = np.abs(out["atlas"].astype(np.float64) - pattern(Xp[..., 0], Xp[..., 1]))
    return float(diff[inside].mean())
