"""Named inputs of sfmba_cloud_merge and sfmba_depth_normals for the CPU and GPU tests -- TEST INFRASTRUCTURE ONLY.

A merge case is a dict xyz float32 [n, 3], bgr uint8 [n, 3], normal float32 [n, 3], voxel, min_count; a normals case a dict K [3, 3],
P [3, 4], depth float32 [h, w], max_rel_step.  oracle(name) / normals_oracle(name) give the restatement's answer once per process
(cloud_oracle.merge_sorted / normals_shifted); they are shared and not to be changed."""
import functools

import numpy as np

import cloud_oracle as co

RUN_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257)


def _attrs(n, seed):
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-9)
    return rng.integers(0, 256, size=(n, 3)).astype(np.uint8), nrm.astype(np.float32)


def _cloud(xyz, voxel, min_count=1, seed=0, shuffle=True):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    if shuffle and len(xyz) > 1:
        xyz = xyz[np.random.default_rng(seed + 100).permutation(len(xyz))]
    bgr, nrm = _attrs(len(xyz), seed)
    return dict(xyz=np.ascontiguousarray(xyz), bgr=bgr, normal=nrm, voxel=np.float32(voxel), min_count=min_count)


def _inside(rng, n):
    """n offsets strictly inside a unit voxel, on a 1/256 grid (exact in float32 beside a small integer)"""
    return rng.integers(8, 248, size=(n, 3)) / 256.0


def _runs(lengths, seed, voxel=0.25):
    """voxels along x (the most significant field of the key) in ascending order, run k with lengths[k] members"""
    rng = np.random.default_rng(seed)
    rows = []
    for k, m in enumerate(lengths):
        cell = np.array([k - len(lengths) // 2, rng.integers(-3, 4), rng.integers(-3, 4)], np.float64)
        rows.append((cell + _inside(rng, m)) * voxel)
    return _cloud(np.concatenate(rows), voxel, seed=seed)


def _straddle():
    # 1 / 2 / 63 / 64 / 65 / 255 / 256 / 257 in several orders: run starts fall on 0, 1, 3, 66, 130, 195, 450, 706, 963, ... of the
    # sorted order, i.e. before, on and behind multiples of 64 and 256, and long runs cross several wave and block boundaries
    order = list(RUN_LENGTHS) + list(RUN_LENGTHS[::-1]) + [64, 64, 64, 64, 1, 255, 1, 256, 2, 257, 63, 63, 65, 65, 1, 1, 1]
    return _runs(order, seed=21)


def _sized(n, seed):
    rng = np.random.default_rng(seed)
    cells = rng.integers(-40, 40, size=(n, 3))               # 512 000 cells for ~32 768 points: mostly runs of 1, some of 2 and 3
    cells[: n // 4] = cells[n // 4: 2 * (n // 4)]            # ... and a quarter of the points doubled up
    return _cloud((cells + _inside(rng, n)) * 0.5, 0.5, seed=seed)


def _edges():
    v = 0.5
    pts = [[-0.5 * v, 0.25 * v, 0.25 * v],                    # i_x = -1
           [-0.25 * v, -1.75 * v, 0.5 * v],                   # i = (-1, -2, 0)
           [1.0 * v, 2.0 * v, -3.0 * v],                      # exactly on voxel faces: the point belongs to the voxel above the face
           [1023.25 / 1024 * v, 2.0 * v, -3.0 * v],           # ... q = 1023, the last quantum under the face: the voxel below
           [(7 + 0.5) / 1024 * v, (1023 + 0.5) / 1024 * v, -(0.5 / 1024) * v],          # t 1024 + 0.5 exactly an integer: 8, 1024 -> i_y = 1, 0
           [0.0, -0.0, 0.0]]
    return _cloud(pts, v, shuffle=False)


def _q_limits():
    lo, hi = -float(2 ** 20), float(2 ** 20)                  # voxel 1: q = -2^30 (kept) and 2^30 (skipped)
    pts = [[lo, 0.5, 0.5], [hi, 0.5, 0.5], [hi - 0.0625, 0.5, 0.5], [0.5, lo, hi - 0.0625], [0.5, 0.5, hi], [lo - 0.125, 0.5, 0.5],
           [lo, lo, lo], [0.5, 0.5, 0.5]]
    return _cloud(pts, 1.0, shuffle=False)


def _nonfinite():
    rng = np.random.default_rng(31)
    xyz = (rng.integers(-2, 2, size=(40, 3)) + _inside(rng, 40)).astype(np.float32)
    xyz[3, 0], xyz[7, 1], xyz[11, 2], xyz[12] = np.nan, np.inf, -np.inf, (np.nan, np.inf, 1.0)
    xyz[20, 0] = 3e38                                         # finite, but its quotient by the voxel is far outside
    return _cloud(xyz, 1.0, shuffle=False)


def _subnormal_voxel():
    rng = np.random.default_rng(32)
    xyz = (rng.integers(-2, 2, size=(30, 3)) + _inside(rng, 30)).astype(np.float32)        # no coordinate is 0: 0 / voxel would be kept
    return _cloud(xyz, np.float32(1e-40), shuffle=False)


def _opposite():
    c = _cloud([[0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [2.25, 0.25, 0.25], [2.5, 0.25, 0.25]], 1.0, shuffle=False)
    c["normal"] = np.asarray([[0, 0, 1], [0, 0, -1], [0.6, 0, 0.8], [0.6, 0, 0.8]], np.float32)
    return c


def _nan_normal():
    c = _cloud([[0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [2.25, 0.25, 0.25], [4.5, 0.25, 0.25]], 1.0, shuffle=False)
    c["normal"] = np.asarray([[np.nan, 0, 1], [0, np.nan, 1], [np.nan, np.nan, np.nan], [np.inf, -np.inf, 100.0]], np.float32)
    return c


CASES = {
    "n1": lambda: _cloud([[0.3, -0.2, 1.7]], 0.1),
    "one_voxel_5000": lambda: _cloud(3.0 + _inside(np.random.default_rng(1), 5000), 1.0, seed=1),
    "distinct_5000": lambda: _cloud(np.stack(np.unravel_index(np.random.default_rng(2).permutation(20 ** 3)[:5000], (20, 20, 20)), 1) - 10 +
                                    _inside(np.random.default_rng(2), 5000), 1.0, seed=2),
    "runs_straddle": _straddle,
    "n_32767": lambda: _sized(32767, 3),
    "n_32768": lambda: _sized(32768, 4),
    "n_32769": lambda: _sized(32769, 5),
    "edges": _edges,
    "q_limits": _q_limits,
    "nonfinite": _nonfinite,
    "subnormal_voxel": _subnormal_voxel,
    "min_count_2": lambda: dict(_runs([1, 2, 3, 1, 2, 5, 1, 1, 3, 2, 40, 1], seed=41), min_count=2),
    "min_count_3": lambda: dict(_runs([1, 2, 3, 1, 2, 5, 1, 1, 3, 2, 40, 1], seed=41), min_count=3),
    "min_count_none_left": lambda: dict(_runs([1, 2, 1, 2], seed=42), min_count=3),
    "opposite_normals": _opposite,
    "nan_normal": _nan_normal,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle(name, with_bgr=True, with_normal=True):
    c = case(name)
    return co.merge_sorted(c["xyz"], c["bgr"] if with_bgr else None, c["normal"] if with_normal else None, c["voxel"], c["min_count"])


# ---- normals ------------------------------------------------------------------------------------------------------------------
def rotation(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def camera(w, h, f=60.0, axis=(0.2, 1.0, 0.1), deg=0.0, t=(0.1, -0.2, 0.3)):
    K = np.array([[f, 0, (w - 1) / 2], [0, 1.1 * f, (h - 1) / 2], [0, 0, 1]], np.float32)
    P = np.concatenate([rotation(axis, deg), np.asarray(t, np.float64)[:, None]], axis=1).astype(np.float32)
    return K, P


def plane_depth(K, w, h, n, d):
    """depth of the camera-space plane n . X = d through every pixel"""
    K = np.asarray(K, np.float64)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    rays = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs, np.float64)], -1)
    return (d / (rays @ np.asarray(n, np.float64))).astype(np.float32)


def _surface(w, h, seed, deg=25.0, step=0.05, holes=0.0):
    rng = np.random.default_rng(seed)
    K, P = camera(w, h, deg=deg)
    n = np.array([0.3, -0.2, 1.0])
    depth = plane_depth(K, w, h, n / np.linalg.norm(n), 4.0) if w > 1 or h > 1 else np.full((1, 1), 4.0, np.float32)
    depth = (depth * (1 + 0.004 * rng.normal(size=depth.shape))).astype(np.float32)
    if holes:
        depth[rng.random(depth.shape) < holes] = 0.0
    return dict(K=K, P=P, depth=depth, max_rel_step=np.float32(step))


def _one_sided():
    # a 5 x 5 block of depth with holes placed so that the centre row meets every one-sided difference: pixel (1, 2) has no west
    # neighbour, (3, 2) no east, (2, 1) no north, (2, 3) no south; (0, 0) sits alone: no normal
    c = _surface(9, 9, seed=51, step=0.2)
    d = np.zeros_like(c["depth"])
    d[2:7, 2:7] = c["depth"][2:7, 2:7]
    d[4, 2] = d[4, 6] = d[2, 4] = d[6, 4] = 0.0
    d[0, 0] = c["depth"][0, 0]
    d[3, 3] = c["depth"][3, 3] * np.float32(1.5)              # a depth step beyond max_rel_step: not usable from its neighbours
    return dict(c, depth=d)


def _step_exact(below):
    # z0 = 2, east neighbour 2.5: |zn - z0| = 0.5 = 0.25 z0 exactly.  max_rel_step = 0.25 keeps the neighbour, one float below drops it
    K, P = camera(3, 3)
    depth = np.full((3, 3), 2.0, np.float32)
    depth[1, 2] = 2.5
    depth[1, 0] = 0.0                                         # no west neighbour: du hangs on the east one alone
    step = np.float32(0.25)
    return dict(K=K, P=P, depth=depth, max_rel_step=np.nextafter(step, np.float32(0)) if below else step)


def _flip():
    # With p = z r, r on the regular pixel grid, (dv x du) . p0 = -z0 (z_S' + z_N') (z_E' + z_W') / (fx fy) for the central and the
    # one-sided differences alike: NEGATIVE for all positive depths, so in exact arithmetic the contract's flip never fires, however
    # the camera is rotated (R enters after it).  Only rounding can make the sum positive.  This map makes rounding decide: with
    # fx = 3e10 and the principal point 1e10 pixels off the image every ray is (1/3, 0.39, 1) to one part in 1e10, du and dv are all
    # but parallel to p0, and the cross product and the dot cancel to rounding noise -- about half the pixels flip (measured 0.495).
    # The device has to take the same branch as the restatement there.
    rng = np.random.default_rng(53)
    K, P = camera(24, 18, f=3e10, deg=140.0)
    K = K.copy()
    K[0, 2], K[1, 2] = -1e10, -1.3e10
    return dict(K=K, P=P, depth=rng.uniform(1.0, 6.0, size=(18, 24)).astype(np.float32), max_rel_step=np.float32(100.0))


def _odd_values():
    c = _surface(12, 9, seed=54, step=0.1)
    d = c["depth"].copy()
    d[2, 3], d[4, 5], d[6, 7], d[1, 1] = np.nan, np.inf, -1.0, np.float32(1e-42)
    return dict(c, depth=d)


NORMAL_CASES = {
    "size_1x1": lambda: _surface(1, 1, 60),
    "size_7x1": lambda: _surface(7, 1, 61),
    "size_1x7": lambda: _surface(1, 7, 62),
    "size_33x17": lambda: _surface(33, 17, 63),
    "size_70x45": lambda: _surface(70, 45, 64, holes=0.15),
    "one_sided": _one_sided,
    "step_exact": lambda: _step_exact(False),
    "step_below": lambda: _step_exact(True),
    "flip": _flip,
    "odd_values": _odd_values,
    "step_zero": lambda: dict(_surface(9, 7, 65), depth=np.full((7, 9), 3.0, np.float32), max_rel_step=np.float32(0.0)),
}


@functools.lru_cache(maxsize=None)
def normals_case(name):
    return NORMAL_CASES[name]()


@functools.lru_cache(maxsize=None)
def normals_oracle(name):
    c = normals_case(name)
    return co.normals_shifted(c["K"], c["P"], c["depth"], c["max_rel_step"])
