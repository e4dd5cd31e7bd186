"""The cases of the dense-stereo tests (tests/test_depth_oracle_cpu.py, tests/test_gpu_depth_sweep.py) -- TEST INFRASTRUCTURE ONLY.

A scene is smoothed noise (so every window is textured) on the plane z = 0, seen by cameras of tests/sfm_scene.py's arc at radius 10
with K = (200, w / 2, h / 2) of the reference; a view is rendered through the homography the plane induces.  Every case is
dict(images, K, P, jobs, params) for depth_oracle.sweep / capi.depth_sweep; the restatement's answer is computed once per case and
shared (oracle(name)).

Allowed importers: tests/, tools/.
"""
import functools

import numpy as np

import depth_oracle as do
import sfm_scene

FOCAL, RADIUS = 200.0, 10.0
Z_NEAR, Z_FAR = 8.0, 12.5


@functools.lru_cache(maxsize=None)
def texture(seed, side=512):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, size=(side + 2, side + 2)).astype(np.float64)
    return sum(t[dy:dy + side, dx:dx + side] for dy in range(3) for dx in range(3)) / 9.0


def render(K, R, t, size, seed=0, scale=40.0):
    """uint8 [h, w]: the plane z = 0 with texture(seed), `scale` texels per world unit, through camera K [R | t]."""
    w, h = size
    tex = texture(seed, 512 if max(size) <= 256 else 2048)
    Hp = K @ np.stack([R[:, 0], R[:, 1], t], axis=1)         # (a, b, 1) on the plane -> pixel
    ys, xs = np.mgrid[0:h, 0:w]
    ab = np.stack([xs, ys, np.ones_like(xs)], axis=-1).reshape(-1, 3).astype(np.float64) @ np.linalg.inv(Hp).T
    a, b = ab[:, 0] / ab[:, 2] * scale + 0.5 * tex.shape[1], ab[:, 1] / ab[:, 2] * scale + 0.5 * tex.shape[0]
    a, b = np.clip(a, 0.0, tex.shape[1] - 1.001), np.clip(b, 0.0, tex.shape[0] - 1.001)
    x0, y0 = np.floor(a).astype(int), np.floor(b).astype(int)
    fa, fb = a - x0, b - y0
    val = (1 - fa) * (1 - fb) * tex[y0, x0] + fa * (1 - fb) * tex[y0, x0 + 1] + (1 - fa) * fb * tex[y0 + 1, x0] + fa * fb * tex[y0 + 1, x0 + 1]
    return np.clip(np.rint(val), 0, 255).astype(np.uint8).reshape(h, w)


def scene(size, n_src=1, src_size=None, step_deg=3.0, seed=0, focal=FOCAL, scale=40.0):
    """Reference = image 0 in the middle of the arc, sources on either side by turns; src_size: the size of source 1 (image 1)."""
    K = sfm_scene.k_matrix(focal, size)
    angles = [0.0] + [step_deg * (1 + i // 2) * (1 if i % 2 == 0 else -1) for i in range(n_src)]
    images, P = [], []
    for i, a in enumerate(angles):
        R, t = sfm_scene.arc_camera(a, RADIUS)
        images.append(render(K, R, t, src_size if (i == 1 and src_size) else size, seed, scale))
        P.append(np.concatenate([R, t[:, None]], axis=1))
    return images, K.astype(np.float32), np.asarray(P, dtype=np.float32)


def _case(size, n_src, radius, n_planes, src_size=None, seed=0, **params):
    images, K, P = scene(size, n_src, src_size, seed=seed)
    prm = dict(n_planes=n_planes, radius=radius, min_std=2, min_score=0.6, min_sources=1)
    prm.update(params)
    return dict(images=images, K=K, P=P, jobs=[(0, list(range(1, n_src + 1)), Z_NEAR, Z_FAR)], params=prm)


def _rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def _edge(kind):
    c = _case((40, 24), 2, 2, 8)
    images, P = list(c["images"]), c["P"].copy()
    Pr = P[0].astype(np.float64)
    if kind == "blind":                   # the only source looks the other way: q_2 < 0 everywhere, every plane is invalid
        c["jobs"] = [(0, [1], Z_NEAR, Z_FAR)]
        P[1] = np.concatenate([_rot_y(180.0) @ Pr[:, :3], (_rot_y(180.0) @ Pr[:, 3])[:, None]], axis=1)
    elif kind == "behind":                # source 1 is turned by 90 degrees about the reference's centre: q_2 changes sign at u = cx
        P[1] = np.concatenate([_rot_y(90.0) @ Pr[:, :3], (_rot_y(90.0) @ Pr[:, 3])[:, None]], axis=1)
    elif kind == "const_ref":             # varI = 0 everywhere
        images[0] = np.full_like(images[0], 77)
    elif kind == "const_src":             # varJ = 0 for source 1, source 2 still counts
        images[1] = np.full_like(images[1], 200)
    elif kind == "min_sources_2":         # source 1 is narrow: it leaves the image part-way, and a plane needs both sources
        images[1] = np.ascontiguousarray(images[1][:, :25])
        c["params"]["min_sources"] = 2
    elif kind == "tie":                   # trel = 0 and the reference's own pixels: all planes cost the same, the lowest k wins
        images[1], P[1] = images[0].copy(), P[0].copy()
        c["jobs"] = [(0, [1], Z_NEAR, Z_FAR)]
        c["params"].update(radius=1, min_score=1.0)          # ... and the cost is exactly 1.0 = (double)min_score: accepted
    else:
        raise KeyError(kind)
    c["images"], c["P"] = images, P
    return c


CASES = {
    # the smallest shapes at which the kernel can still go wrong: nothing takes part, tile edges in both directions, every radius
    "size_1x1_r1": lambda: _case((1, 1), 1, 1, 4),
    "size_4x4_r2": lambda: _case((4, 4), 1, 2, 4),
    "size_8x8_r4": lambda: _case((8, 8), 1, 4, 4),
    "size_15x16_r1_d2": lambda: _case((15, 16), 1, 1, 2),
    "size_16x16_r4_d3": lambda: _case((16, 16), 1, 4, 3),
    "size_17x33_r1_d64_s4": lambda: _case((17, 33), 4, 1, 64),
    "size_17x33_r2_d3": lambda: _case((17, 33), 1, 2, 3, src_size=(21, 30)),
    "size_48x31_r4_d64_s4": lambda: _case((48, 31), 4, 4, 64, src_size=(40, 36)),
    "size_48x31_r3_d64": lambda: _case((48, 31), 1, 3, 64, src_size=(52, 29)),
    "blind": lambda: _edge("blind"),
    "behind": lambda: _edge("behind"),
    "const_ref": lambda: _edge("const_ref"),
    "const_src": lambda: _edge("const_src"),
    "min_sources_2": lambda: _edge("min_sources_2"),
    "tie": lambda: _edge("tie"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle(name):
    """depth_oracle.sweep_integral's dict for the (single) job of the case; shared, not to be changed."""
    c = case(name)
    return do.sweep_integral(c["images"], c["K"], c["P"], c["jobs"][0], **c["params"])


def batch(extended=False):
    """Five mixed jobs over one image list: different references, source counts, ranges and sizes.

    extended: two more images and two more jobs behind the same five (tests/group_cases.py).  With two jobs to a group image 1 is the
    reference of job 1 and a source of job 2 in the next group, image 0 is named by jobs of all four groups, and job 5, the second
    of its group, names two images (4 and 5) that no job before it names."""
    images, K, P = scene((33, 20), 5 if extended else 3, src_size=(28, 25), seed=3)
    jobs = [(0, [1], Z_NEAR, Z_FAR), (1, [0, 2], 7.5, 13.0), (2, [0, 1, 3], Z_NEAR, Z_FAR), (3, [0], 9.0, 11.0), (0, [3, 2, 1], 8.5, 12.0)]
    if extended:
        jobs += [(4, [5], 8.25, 12.25), (5, [4, 0], 7.75, 12.75)]
    return dict(images=images, K=K, P=P, jobs=jobs, params=dict(n_planes=16, radius=2, min_std=2, min_score=0.6, min_sources=1))


def bgr_of(images, seed=5):
    """BGR images (distinct channels) for the list; their gray reduction is do.gray."""
    rng = np.random.default_rng(seed)
    out = []
    for im in images:
        d = rng.integers(-20, 21, size=im.shape + (3,))
        out.append(np.clip(im[..., None].astype(np.int64) + d, 0, 255).astype(np.uint8))
    return out


def fuse_scene():
    """Three views with the restatement's depth maps of a batch sweep: (images, K, P, maps)."""
    images, K, P = scene((40, 28), 2, seed=7)
    jobs = [(0, [1, 2], Z_NEAR, Z_FAR), (1, [0], Z_NEAR, Z_FAR), (2, [0], Z_NEAR, Z_FAR)]
    maps = [d for d, _, _ in do.sweep(images, K, P, jobs, n_planes=24, radius=2, min_std=2, min_score=0.6, min_sources=1)]
    return images, K, P, maps


def corner_depth(sc, v):
    """Camera-space z of every pixel of view v of a make_corner scene (inf on the background), from _plane_frames as make_corner
    computes it."""
    K, (w, h), R, t = sc["K"], sc["size"], sc["R"][v], sc["t"][v]
    Kinv, C = np.linalg.inv(K), -R.T @ t
    ys, xs = np.mgrid[0:h, 0:w]
    pix = np.stack([xs, ys, np.ones_like(xs)], -1).reshape(-1, 3).astype(np.float64)
    rays = pix @ (R.T @ Kinv).T                              # K^-1 pix has z = 1: lam along such a ray is the camera-space z
    depth = np.full(h * w, np.inf)
    for o, u, vv, nrm in sfm_scene._plane_frames():
        Hp = K @ np.stack([R @ u, R @ vv, R @ o + t], axis=1)
        ab = pix @ np.linalg.inv(Hp).T
        with np.errstate(all="ignore"):
            a, lam = ab[:, 0] / ab[:, 2], ((o - C) @ nrm) / (rays @ nrm)
        ok = np.isfinite(lam) & (lam > 0) & (a >= 0) & (lam < depth)
        depth[ok] = lam[ok]
    return depth.reshape(h, w)
