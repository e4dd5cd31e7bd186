"""Named inputs of sfmba_tsdf_extract and sfmba_tsdf_integrate / sfmba_tsdf_mesh for the CPU and GPU tests -- TEST INFRASTRUCTURE ONLY.

An extraction case is a dict origin [3], voxel, S, W int32 [nz, ny, nx], CS int32 [nz, ny, nx, 3], CW int32 [nz, ny, nx], min_weight;
an integration case a dict images (list of uint8 [h, w] or [h, w, 3]), K [3, 3], P [n, 3, 4], depth_maps (list of None or float32
[h, w]), origin, voxel, dims (nx, ny, nz), trunc.  mesh(name, colour) / grid(name, colour) give the restatement's answer once per
process (mesh_oracle.extract_table / integrate_maps); they are shared and not to be changed."""
import functools

import numpy as np

import mesh_oracle as mo


# ---- extraction --------------------------------------------------------------------------------------------------------------
def _grid(S, W, seed, origin=(0.125, -0.25, 0.5), voxel=0.25, min_weight=1):
    """colour sums inside their bounds beside S and W"""
    rng = np.random.default_rng(seed + 500)
    W = np.asarray(W, np.int32)
    CW = rng.integers(0, W + 1).astype(np.int32)
    CS = (rng.integers(0, 256, size=W.shape + (3,)) * CW[..., None]).astype(np.int32)
    CS = np.maximum(CS - rng.integers(0, 3, size=CS.shape) * (CW[..., None] > 0), 0).astype(np.int32)
    return dict(origin=np.asarray(origin, np.float32), voxel=np.float32(voxel), S=np.ascontiguousarray(S, np.int32), W=np.ascontiguousarray(W),
                CS=np.ascontiguousarray(CS), CW=np.ascontiguousarray(CW), min_weight=min_weight)


def _random(nx, ny, nz, seed, max_w=5):
    rng = np.random.default_rng(seed)
    W = rng.integers(1, max_w + 1, size=(nz, ny, nx))
    S = rng.integers(-1024 * W, 1024 * W + 1)
    return _grid(S, W, seed)


def _planted(n, dist, seed, band=3.0):
    """every vertex defined; f = the clamped distance in quanta, W random, S = e W plus less than one quantum"""
    rng = np.random.default_rng(seed)
    g = np.arange(n, dtype=np.float64)
    Z, Y, X = np.meshgrid(g, g, g, indexing="ij")
    e = np.floor(np.clip(dist(X, Y, Z) / band, -1.0, 1.0) * 1024.0 + 0.5).astype(np.int64)
    W = rng.integers(1, 5, size=e.shape)
    return _grid(e * W, W, seed)


def sphere_distance(c, r):
    return lambda X, Y, Z: np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r


def torus_distance(c, R, r):
    return lambda X, Y, Z: np.sqrt((np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2) - R) ** 2 + (Z - c[2]) ** 2) - r


SPHERE, TORUS, ZEROS = ((6.3, 6.6, 6.4), 4.2), ((8.5, 8.5, 8.5), 5.0, 2.0), ((6.0, 6.0, 6.0), 4.0)


def _all_256():
    """256 isolated 2 x 2 x 2 blocks along x, block b at x = 3 b, 3 b + 1 with corner c inside iff bit c of b; the layer x = 3 b + 2
    has W = 0"""
    nx = 3 * 256
    S, W = np.zeros((2, 2, nx), np.int64), np.zeros((2, 2, nx), np.int64)
    rng = np.random.default_rng(31)
    for b in range(256):
        for c in range(8):
            at = (c >> 2 & 1, c >> 1 & 1, 3 * b + (c & 1))
            W[at] = rng.integers(1, 4)
            S[at] = -rng.integers(1, 1024 * W[at] + 1) if b >> c & 1 else rng.integers(0, 1024 * W[at] + 1)
    return _grid(S, W, 31)


def _signs(value):
    c = _random(4, 5, 3, 41)
    c["S"] = np.full_like(c["S"], value)
    c["S"] *= c["W"] if value else 1
    return c


def _min_weight(m):
    c = _random(4, 4, 4, 42, max_w=1)
    c["W"] *= 3
    c["S"] *= 3
    c["CW"] *= 0
    c["CS"] *= 0
    c["min_weight"] = m
    return c


def _undefined_corner():
    c = _random(5, 5, 5, 43)
    c["W"][2, 2, 2] = 0
    c["S"][2, 2, 2] = 0
    c["CW"][2, 2, 2] = 0
    c["CS"][2, 2, 2] = 0
    return c


CASES = {
    "g_1x1x1": lambda: _random(1, 1, 1, 1),
    "g_1x5x4": lambda: _random(1, 5, 4, 2),
    "g_2x2x1": lambda: _random(2, 2, 1, 3),
    "g_2x2x2": lambda: _random(2, 2, 2, 4),
    "g_3x2x2": lambda: _random(3, 2, 2, 5),
    "all_256": _all_256,
    "nx_63": lambda: _random(63, 3, 3, 6),
    "nx_64": lambda: _random(64, 3, 3, 7),
    "nx_65": lambda: _random(65, 3, 3, 8),
    "cells_255": lambda: _random(256, 2, 2, 9),
    "cells_256": lambda: _random(257, 2, 2, 10),
    "cells_257": lambda: _random(258, 2, 2, 11),
    "sphere_14": lambda: _planted(14, sphere_distance(*SPHERE), 12),
    "torus_18": lambda: _planted(18, torus_distance(*TORUS), 13),
    "zeros_14": lambda: _planted(14, sphere_distance(*ZEROS), 14),
    "all_inside": lambda: _signs(-7),
    "all_outside": lambda: _signs(5),
    "all_zero": lambda: _signs(0),
    "min_weight_w": lambda: _min_weight(3),
    "min_weight_w1": lambda: _min_weight(4),
    "undefined_corner": _undefined_corner,
}
NO_CELL = ("g_1x1x1", "g_1x5x4", "g_2x2x1")
CLOSED = {"sphere_14": 2, "torus_18": 0, "zeros_14": 2}          # the planted solids and their Euler characteristic


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def mesh(name, colour=True):
    c = case(name)
    return mo.extract_table(c["origin"], c["voxel"], c["S"], c["W"], c["CS"] if colour else None, c["CW"] if colour else None, c["min_weight"])


# ---- integration -------------------------------------------------------------------------------------------------------------
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """[R | t] float32 [3, 4] of a camera at `eye` whose z axis points at `target` (x right, y down)"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    if abs(np.dot(z, up)) > 0.99:
        up = np.array([1.0, 0.0, 0.0])
    x = np.cross(z, -up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R, (-R @ eye)[:, None]], axis=1).astype(np.float32)


def intrinsics(w, h, f=None):
    f = float(f if f else 0.9 * max(w, h))
    return np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]], np.float32)


def sphere_depth(K, P, w, h, radius):
    """the z-depth of the sphere of `radius` about the origin by ray intersection, float32 [h, w], 0 where the ray misses"""
    K, P = np.asarray(K, np.float64), np.asarray(P, np.float64)
    R, t = P[:, :3], P[:, 3]
    eye = -R.T @ t
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1) @ R     # world ray per unit of z-depth
    a, b, c = (d * d).sum(-1), 2.0 * (d @ eye), eye @ eye - radius * radius
    disc = b * b - 4.0 * a * c
    z = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a), 0.0)
    return np.where(z > 0, z, 0.0).astype(np.float32)


def _texture(h, w, channels, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(h, w, 3) if channels == 3 else (h, w)).astype(np.uint8)


SIX_EYES = ((3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, -3, 0), (0, 0, 3), (0, 0, -3))


def _sphere_views(eyes, size, n, radius=1.0, channels=3, holes=False, seed=50):
    """the analytic sphere seen from `eyes`, a grid n^3 over [-1.3 r, 1.3 r]^3, trunc of 4 voxels"""
    w = h = size
    K = intrinsics(w, h)
    P = np.stack([look_at(e) for e in eyes])
    maps = [sphere_depth(K, p, w, h, radius) for p in P]
    if holes:
        rng = np.random.default_rng(seed)
        for m in maps:
            m[rng.random(m.shape) < 0.08] = 0.0
            m[h // 3:h // 3 + 5, w // 4:w // 4 + 9] = 0.0
    voxel = np.float32(2.6 * radius / (n - 1))
    return dict(images=[_texture(h, w, channels, seed + i) for i in range(len(eyes))], K=K, P=P, depth_maps=maps,
                origin=np.full(3, -1.3 * radius, np.float32), voxel=voxel, dims=(n, n, n), trunc=np.float32(4.0 * float(voxel)))


def _axis_camera(w, h, f, flipped=False, tz=0.0):
    K = np.array([[f, 0, (w - 1) // 2], [0, f, (h - 1) // 2], [0, 0, 1]], np.float32)
    P = np.zeros((1, 3, 4), np.float32)
    P[0, :, :3] = np.diag([1.0, -1.0, -1.0]) if flipped else np.eye(3)
    P[0, 2, 3] = tz
    return K, P


def _ramp(h, w, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return (lo + (hi - lo) * rng.random((h, w))).astype(np.float32)


def _half_pixel():
    # fx = fy = 4, cx = cy = 3, z = 2: x = -0.25, 0, 0.25 project to 2.5, 3, 3.5 and round to 3, 3, 4 (halves go up)
    K, P = _axis_camera(8, 8, 4.0)
    return dict(images=[_texture(8, 8, 3, 60)], K=K, P=P, depth_maps=[_ramp(8, 8, 1.8, 2.6, 61)], origin=np.array([-0.25, -0.25, 2.0], np.float32),
                voxel=np.float32(0.25), dims=(3, 3, 2), trunc=np.float32(0.5))


def _behind_and_outside():
    # z = -0.25 .. 1 (q_2 <= 0 for the first two layers); at z = 1 the columns land on u = -2 .. 8 of an 8 x 8 image
    K, P = _axis_camera(8, 8, 4.0)
    m = _ramp(8, 8, 0.6, 1.4, 62)
    m[2, 5] = m[6, 1] = m[0, 0] = 0.0                                        # zs == 0
    return dict(images=[_texture(8, 8, 1, 63)], K=K, P=P, depth_maps=[m], origin=np.array([-1.25, -1.25, -0.25], np.float32),
                voxel=np.float32(0.25), dims=(11, 11, 6), trunc=np.float32(0.5))


SDF_Q = 0.75 + 2.0 ** -10          # the q_2 of the first vertex of the two sdf cases; T = 0.75, the voxel is 2^-53


def _sdf_minus():
    # identity camera: q_2 = X_2 = Q, Q + 2^-53; zs = 2^-10: sdf = -0.75 exactly (kept, e = -1024), then one double below (skipped)
    K, P = _axis_camera(3, 3, 4.0)
    return dict(images=[_texture(3, 3, 3, 64)], K=K, P=P, depth_maps=[np.full((3, 3), 2.0 ** -10, np.float32)],
                origin=np.array([0.0, 0.0, SDF_Q], np.float32), voxel=np.float32(2.0 ** -53), dims=(1, 1, 2), trunc=np.float32(0.75))


def _sdf_plus():
    # a camera looking down -z with t_z = 1.5: q_2 = 1.5 - X_2 = Q, Q - 2^-53; zs = Q + 0.75: sdf = 0.75 exactly (colour kept), then one
    # double above (colour dropped); e = 1024 both times
    K, P = _axis_camera(3, 3, 4.0, flipped=True, tz=1.5)
    return dict(images=[_texture(3, 3, 3, 65)], K=K, P=P, depth_maps=[np.full((3, 3), SDF_Q + 0.75, np.float32)],
                origin=np.array([0.0, 0.0, 1.5 - SDF_Q], np.float32), voxel=np.float32(2.0 ** -53), dims=(1, 1, 2), trunc=np.float32(0.75))


def _mixed(n_images, channels, seed, null_at=None):
    """cameras around a 1.5-wide grid, images of different sizes, noisy depth maps about the distance to the centre"""
    rng = np.random.default_rng(seed)
    sizes = [(24 + 7 * (i % 3), 17 + 5 * (i % 4)) for i in range(n_images)]
    eyes = [3.0 * v / np.linalg.norm(v) for v in rng.normal(size=(n_images, 3))]
    K = intrinsics(24, 17, 20.0)
    P = np.stack([look_at(e) for e in eyes])
    maps = [_ramp(h, w, 2.6, 3.4, seed + 10 + i) for i, (w, h) in enumerate(sizes)]
    for m in maps:
        m[rng.random(m.shape) < 0.1] = 0.0
    if null_at is not None:
        maps[null_at] = None
    return dict(images=[_texture(h, w, channels, seed + 20 + i) for i, (w, h) in enumerate(sizes)], K=K, P=P, depth_maps=maps,
                origin=np.full(3, -0.75, np.float32), voxel=np.float32(0.125), dims=(13, 12, 11), trunc=np.float32(0.3))


def permuted(c, order):
    out = dict(c)
    out["images"] = [c["images"][i] for i in order]
    out["depth_maps"] = [c["depth_maps"][i] for i in order]
    out["P"] = np.ascontiguousarray(c["P"][list(order)])
    return out


def gray_of(c, channel):
    out = dict(c)
    out["images"] = [np.ascontiguousarray(im[..., channel]) for im in c["images"]]
    return out


INTEGRATION_CASES = {
    "half_pixel": _half_pixel,
    "behind_and_outside": _behind_and_outside,
    "sdf_minus": _sdf_minus,
    "sdf_plus": _sdf_plus,
    "one_image_gray": lambda: _mixed(1, 1, 70),
    "five_images_bgr": lambda: _mixed(5, 3, 71, null_at=2),
    "five_images_permuted": lambda: permuted(integration_case("five_images_bgr"), (3, 0, 4, 2, 1)),
    "six_view_sphere": lambda: _sphere_views(SIX_EYES, 64, 32),
    "two_views_holes": lambda: _sphere_views(((3, 0.4, 0.2), (-0.3, 3, 0.5)), 48, 20, holes=True, seed=80),
}


@functools.lru_cache(maxsize=None)
def integration_case(name):
    return INTEGRATION_CASES[name]()


def run_integrate(c, colour=True, fn=mo.integrate_maps):
    return fn(c["images"] if colour else None, c["K"], c["P"], c["depth_maps"], c["origin"], c["voxel"], c["dims"], c["trunc"])


@functools.lru_cache(maxsize=None)
def grid(name, colour=True):
    return run_integrate(integration_case(name), colour)


@functools.lru_cache(maxsize=None)
def grid_mesh(name, colour=True, min_weight=1):
    c, g = integration_case(name), grid(name, colour)
    return mo.extract_table(c["origin"], c["voxel"], g["sum"], g["weight"], g["csum"], g["cweight"], min_weight)
