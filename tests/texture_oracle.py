"""The CPU restatement of sfmba_mesh_texture (the contract is in include/sfmba.h), every part stated TWICE:

  * the view choice as a loop per triangle and view in Python integers and floats (views_loop) and as numpy over all
    (triangle, view) pairs at once (views_np);
  * the raster as a loop per block and texel (raster_loop) and as numpy over the whole atlas with an ownership map (raster_np).

fp64 with every operation rounded on its own (neither Python nor numpy fuses a multiply and an add), integers from the 1/16 px image
coordinate to the texel.  A sum written a + b + c is ((a + b) + c)."""
import math

import numpy as np

MIN_PATCH, MAX_PATCH, MAX_SIDE = 3, 64, 16384


def k4_of(K):
    K = [float(v) for v in np.asarray(K, np.float32).reshape(-1)]
    return [K[0], K[4], K[2], K[5]]


def default_blocks_per_row(nt):
    """the host's rule: ceil(sqrt(n_blocks)), at least 1"""
    blocks = (nt + 1) // 2
    b = math.isqrt(blocks)
    return max(1, b if b * b == blocks else b + 1)


def atlas_size(nt, S, B):
    """(W, H), or None where the call refuses the layout"""
    if nt < 0 or S < MIN_PATCH or S > MAX_PATCH or B < 1:
        return None
    blocks = (nt + 1) // 2
    if blocks == 0:
        return S + 1, S
    W, H = B * (S + 1), -(-blocks // B) * S
    return (W, H) if W <= MAX_SIDE and H <= MAX_SIDE else None


# ---- layout ------------------------------------------------------------------------------------------------------------------------
def atlas_pixel(t, S, B, i, j):
    b = t >> 1
    ox, oy = (b % B) * (S + 1), (b // B) * S
    return (ox + S - i, oy + S - 1 - j) if t & 1 else (ox + i, oy + j)


def corner_uv(nt, S, B):
    uv = np.zeros((nt, 3, 2), np.float32)
    for t in range(nt):
        for c, (i, j) in enumerate(((0, 0), (S - 2, 0), (0, S - 2))):
            X, Y = atlas_pixel(t, S, B, i, j)
            uv[t, c] = (X + 0.5, Y + 0.5)
    return uv


def ownership(nt, S, B, W, H):
    """per atlas pixel: the triangle (-1: nobody) and the texel (i, j) of its frame -- int64 [H, W] each"""
    Y, X = np.mgrid[0:H, 0:W].astype(np.int64)
    bx, x, by, y = X // (S + 1), X % (S + 1), Y // S, Y % S
    half = (x + y > S - 1).astype(np.int64)
    t = 2 * (by * B + bx) + half
    i, j = np.where(half == 1, S - x, x), np.where(half == 1, S - 1 - y, y)
    return np.where(t < nt, t, -1), i, j


# ---- scalars (the loop statements) ---------------------------------------------------------------------------------------------------
def camera_point(p, X):
    return [((p[4 * i] * X[0] + p[4 * i + 1] * X[1]) + p[4 * i + 2] * X[2]) + p[4 * i + 3] for i in range(3)]


def image_point(k4, q):
    return (k4[0] * q[0]) / q[2] + k4[2], (k4[1] * q[1]) / q[2] + k4[3]


def fix(c):
    return math.floor(16.0 * c + 0.5)


def vertex(k4, p, X, w, h, dmap, occl_tol):
    """(passes, q, u, v, su, sv) of one vertex in one view; u, v, su, sv are 0 where they are not formed"""
    q = camera_point(p, X)
    if not q[2] > 0.0:
        return False, q, 0.0, 0.0, 0, 0
    u, v = image_point(k4, q)
    if not (0.0 <= u <= float(w - 1) and 0.0 <= v <= float(h - 1)):
        return False, q, u, v, 0, 0
    su, sv = fix(u), fix(v)
    if dmap is not None:
        zs = float(dmap[math.floor(v + 0.5), math.floor(u + 0.5)])
        if not (zs > 0.0 and (q[2] - zs) <= occl_tol):
            return False, q, u, v, su, sv
    return True, q, u, v, su, sv


def area2(su, sv):
    return (su[1] - su[0]) * (sv[2] - sv[0]) - (sv[1] - sv[0]) * (su[2] - su[0])


def candidate(k4, p, corners, w, h, dmap, occl_tol):
    """(candidate, a2) of a triangle in a view; a2 is 0 for a view that is no candidate"""
    res = [vertex(k4, p, X, w, h, dmap, occl_tol) for X in corners]
    if not all(r[0] for r in res):
        return False, 0
    return True, area2([r[4] for r in res], [r[5] for r in res])


def eligible(cand, a2, min_area):
    return cand and -a2 > 0 and -a2 >= min_area


def _views(images, P, depth_maps):
    P = np.asarray(P, np.float32).reshape(-1, 12).astype(np.float64)
    return [(P[i].tolist(), images[i].shape[1], images[i].shape[0], depth_maps[i]) for i in range(len(images))]


def views_loop(xyz, tri, images, K, P, depth_maps, occl_tol, min_area):
    k4, tol = k4_of(K), float(np.float32(occl_tol))
    views = _views(images, P, depth_maps)
    X = np.asarray(xyz, np.float32).astype(np.float64)
    view, score = np.full(len(tri), -1, np.int32), np.zeros(len(tri), np.int64)
    for t, idx in enumerate(np.asarray(tri).tolist()):
        if len(set(idx)) < 3 or not np.isfinite(X[idx]).all():
            continue
        corners = [X[v].tolist() for v in idx]
        for n, (p, w, h, dmap) in enumerate(views):
            cand, a2 = candidate(k4, p, corners, w, h, dmap, tol)
            if eligible(cand, a2, min_area) and -a2 > score[t]:
                view[t], score[t] = n, -a2
    return view, score


def point(S, i, j, A, B, C):
    wA, wB, wC, den = float(S - 2 - i - j), float(i), float(j), float(S - 2)
    return [((wA * A[a] + wB * B[a]) + wC * C[a]) / den for a in range(3)]


def texel_coord(k4, p, X, w, h):
    """None (the fallback) or (su, sv), and q, u, v"""
    q = camera_point(p, X)
    if not q[2] > 0.0:
        return None, q, 0.0, 0.0
    u, v = image_point(k4, q)
    if u != u or v != v:
        return None, q, u, v
    return (fix(min(max(u, 0.0), float(w - 1))), fix(min(max(v, 0.0), float(h - 1)))), q, u, v


def sample12(img, ch, su, sv):
    h, w = img.shape[:2]
    x0, fx, y0, fy = su >> 4, su & 15, sv >> 4, sv & 15
    x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
    px = (lambda y, x: int(img[y, x])) if img.ndim == 2 else (lambda y, x: int(img[y, x, ch]))
    return ((16 - fx) * (16 - fy) * px(y0, x0) + fx * (16 - fy) * px(y0, x1) + (16 - fx) * fy * px(y1, x0) + fx * fy * px(y1, x1) + 8) >> 4


def fallback(S, i, j, cA, cB, cC):
    num = 2 * ((S - 2 - i - j) * cA + i * cB + j * cC) + (S - 2)
    return min(max(num // (2 * (S - 2)), 0), 255)


def raster_loop(xyz, bgr, tri, images, K, P, view, S, B):
    nt = len(tri)
    W, H = atlas_size(nt, S, B)
    k4 = k4_of(K)
    Pd = np.asarray(P, np.float32).reshape(-1, 12).astype(np.float64)
    X = np.asarray(xyz, np.float32).astype(np.float64)
    atlas = np.zeros((H, W, 3), np.uint8)
    for t, idx in enumerate(np.asarray(tri).tolist()):
        A, Bc, C = (X[v].tolist() for v in idx)
        col = [[0, 0, 0]] * 3 if bgr is None else [[int(c) for c in bgr[v]] for v in idx]
        n = int(view[t])
        for j in range(S):
            for i in range(S - j):
                px = None
                if n >= 0:
                    img = images[n]
                    coord, _, _, _ = texel_coord(k4, Pd[n].tolist(), point(S, i, j, A, Bc, C), img.shape[1], img.shape[0])
                    if coord is not None:
                        px = [(sample12(img, ch, *coord) + 8) >> 4 for ch in range(3)]
                if px is None:
                    px = [fallback(S, i, j, col[0][ch], col[1][ch], col[2][ch]) for ch in range(3)]
                ax, ay = atlas_pixel(t, S, B, i, j)
                atlas[ay, ax] = px
    return atlas


# ---- numpy (the array statements) ------------------------------------------------------------------------------------------------------
def _flat(images, depth_maps):
    """the pixels and the maps back to back, with per-view offsets (map offset -1: no map), widths and heights"""
    n = len(images)
    w = np.asarray([im.shape[1] for im in images], np.int64).reshape(n)
    h = np.asarray([im.shape[0] for im in images], np.int64).reshape(n)
    ch = 1 if not n or images[0].ndim == 2 else 3
    raw = np.concatenate([np.asarray(im, np.uint8).reshape(-1) for im in images] + [np.zeros(1, np.uint8)]).astype(np.int64)
    raw_off = np.concatenate([[0], np.cumsum(w * h * ch)])[:n]
    maps, map_off, at = [], np.full(n, -1, np.int64), 0
    for i, m in enumerate(depth_maps):
        if m is not None:
            maps.append(np.asarray(m, np.float32).reshape(-1))
            map_off[i] = at
            at += m.size
    maps = np.concatenate(maps + [np.zeros(1, np.float32)]).astype(np.float64)
    return raw, raw_off, maps, map_off, w, h, ch


def _project_np(k4, P, X):
    """q [..., 3], u, v for poses P [..., 12] and points X [..., 3] (broadcast)"""
    q = np.stack([((P[..., 4 * i] * X[..., 0] + P[..., 4 * i + 1] * X[..., 1]) + P[..., 4 * i + 2] * X[..., 2]) + P[..., 4 * i + 3]
                  for i in range(3)], -1)
    u, v = (k4[0] * q[..., 0]) / q[..., 2] + k4[2], (k4[1] * q[..., 1]) / q[..., 2] + k4[3]
    return q, u, v


def _fix_np(c):
    return np.floor(16.0 * c + 0.5).astype(np.int64)


def views_np(xyz, tri, images, K, P, depth_maps, occl_tol, min_area):
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    nt, n = len(tri), len(images)
    view, score = np.full(nt, -1, np.int32), np.zeros(nt, np.int64)
    if nt == 0 or n == 0:
        return view, score
    k4, tol = k4_of(K), float(np.float32(occl_tol))
    raw, raw_off, maps, map_off, w, h, ch = _flat(images, depth_maps)
    Pd = np.asarray(P, np.float32).reshape(-1, 12).astype(np.float64)
    X = np.asarray(xyz, np.float32).astype(np.float64)[tri]                                  # [nt, 3 corners, 3]
    good = (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2]) & np.isfinite(X).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        q, u, v = _project_np(k4, Pd[None, :, None, :], X[:, None, :, :])                        # [nt, n, 3 corners]
        wv, hv = w[None, :, None], h[None, :, None]
        ok = (q[..., 2] > 0.0) & (u >= 0.0) & (u <= (wv - 1).astype(np.float64)) & (v >= 0.0) & (v <= (hv - 1).astype(np.float64))
        us, vs = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
        su, sv = _fix_np(us), _fix_np(vs)
        px, py = np.floor(us + 0.5).astype(np.int64), np.floor(vs + 0.5).astype(np.int64)
        has_map = (map_off >= 0)[None, :, None]
        zs = maps[np.where(has_map, map_off[None, :, None] + py * wv + px, 0)]
        ok &= ~has_map | ((zs > 0.0) & ((q[..., 2] - zs) <= tol))
    cand = ok.all(axis=2) & good[:, None]
    a2 = (su[..., 1] - su[..., 0]) * (sv[..., 2] - sv[..., 0]) - (sv[..., 1] - sv[..., 0]) * (su[..., 2] - su[..., 0])
    s = np.where(cand & (-a2 > 0) & (-a2 >= min_area), -a2, 0)                                  # [nt, n]; 0: not eligible
    best = np.argmax(s, axis=1)                                                                 # the first of the largest
    score = s[np.arange(nt), best].astype(np.int64)
    view = np.where(score > 0, best, -1).astype(np.int32)
    return view, score


def raster_np(xyz, bgr, tri, images, K, P, view, S, B):
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    nt, n = len(tri), len(images)
    W, H = atlas_size(nt, S, B)
    atlas = np.zeros((H, W, 3), np.uint8)
    if nt == 0:
        return atlas
    owner, i, j = ownership(nt, S, B, W, H)
    own = owner >= 0
    t = np.where(own, owner, 0)
    wA, wB, wC = S - 2 - i - j, i, j
    # the fallback everywhere, then the samples where there are any
    col = np.zeros((nt, 3, 3), np.int64) if bgr is None else np.asarray(bgr, np.uint8).astype(np.int64)[tri]     # [nt, corner, channel]
    c = col[t]                                                                                                  # [H, W, corner, channel]
    num = 2 * (wA[..., None] * c[:, :, 0] + wB[..., None] * c[:, :, 1] + wC[..., None] * c[:, :, 2]) + (S - 2)
    out = np.clip(num // (2 * (S - 2)), 0, 255)
    vw = np.asarray(view, np.int64)[t]
    if n > 0:
        k4 = k4_of(K)
        raw, raw_off, _, _, w, h, ch = _flat(images, [None] * n)
        Pd = np.asarray(P, np.float32).reshape(-1, 12).astype(np.float64)
        X = np.asarray(xyz, np.float32).astype(np.float64)[tri][t]                              # [H, W, 3 corners, 3]
        nv = np.where(vw >= 0, vw, 0)
        with np.errstate(all="ignore"):
            fA, fB, fC = (a.astype(np.float64)[..., None] for a in (wA, wB, wC))
            Xp = ((fA * X[:, :, 0] + fB * X[:, :, 1]) + fC * X[:, :, 2]) / float(S - 2)
            q, u, v = _project_np(k4, Pd[nv], Xp)
            ok = own & (vw >= 0) & (q[..., 2] > 0.0) & ~np.isnan(u) & ~np.isnan(v)
            wv, hv = w[nv], h[nv]
            uc = np.minimum(np.maximum(np.where(ok, u, 0.0), 0.0), (wv - 1).astype(np.float64))
            vc = np.minimum(np.maximum(np.where(ok, v, 0.0), 0.0), (hv - 1).astype(np.float64))
        su, sv = _fix_np(uc), _fix_np(vc)
        x0, fx, y0, fy = su >> 4, su & 15, sv >> 4, sv & 15
        x1, y1 = np.minimum(x0 + 1, wv - 1), np.minimum(y0 + 1, hv - 1)
        for k in range(3):
            at = lambda y, x: raw[raw_off[nv] + (y * wv + x) * ch + (k if ch == 3 else 0)]
            s12 = ((16 - fx) * (16 - fy) * at(y0, x0) + fx * (16 - fy) * at(y0, x1) + (16 - fx) * fy * at(y1, x0) + fx * fy * at(y1, x1) + 8) >> 4
            out[..., k] = np.where(ok, (s12 + 8) >> 4, out[..., k])
    atlas[own] = out[own].astype(np.uint8)
    return atlas


# ---- the call ------------------------------------------------------------------------------------------------------------------------
def texture(xyz, bgr, tri, images, K, P, depth_maps, occl_tol, min_area=0, patch=6, blocks_per_row=None, want_score=True,
            views_fn=views_np, raster_fn=raster_np):
    """what sfmba_mesh_texture writes, as capi.mesh_texture returns it, or None where the call refuses (the layout, an index)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    tri = np.asarray(tri, np.int32).reshape(-1, 3)
    B = default_blocks_per_row(len(tri)) if blocks_per_row is None else blocks_per_row
    size = atlas_size(len(tri), patch, B)
    if size is None or (len(tri) and (tri.min() < 0 or tri.max() >= len(xyz))) or min_area < 0 or not (np.isfinite(occl_tol) and occl_tol >= 0):
        return None
    Bl = B if len(tri) else 1
    view, score = views_fn(xyz, tri, images, K, P, depth_maps, occl_tol, min_area)
    atlas = raster_fn(xyz, bgr, tri, images, K, P, view, patch, Bl)
    return {"atlas": atlas, "uv": corner_uv(len(tri), patch, Bl), "view": view, "score": score if want_score else None,
            "n_textured": int((view >= 0).sum())}


def view_changes(tri, view):
    """(pairs of triangles that share an edge, those of them with different views)"""
    edges = {}
    for t, (a, b, c) in enumerate(np.asarray(tri).tolist()):
        for e in ((a, b), (b, c), (c, a)):
            edges.setdefault((min(e), max(e)), []).append(t)
    pairs = [(ts[0], ts[1]) for ts in edges.values() if len(ts) == 2]
    return len(pairs), sum(1 for s, t in pairs if view[s] != view[t])
