"""The CPU restatement of the seam levelling (the contract is in include/sfmba.h, "levelling the colours across seams"), every part stated
TWICE:

  * the nodes as a dict loop over the contributing triangles (nodes_dict) and as np.unique on the keys (nodes_np);
  * the node colours as a loop per node in Python integers (colours_loop) and as numpy over all nodes (colours_np);
  * a pass as a loop per node in Python integers (pass_loop) and as np.add.at with // on int64 (pass_np);
  * the levelled raster as a loop per texel (raster_loop) and as numpy over the whole atlas (raster_np).

The sample, the projection and the layout are tests/texture_oracle.py's.  Past the fixed-point image coordinate everything is integer
arithmetic, and every division is a floor division (Python's and numpy's // both are)."""
import numpy as np

import label_oracle as lo
import texture_oracle as to

F_MAX = 65280
MAX_RADIUS, MAX_WEIGHT, MAX_PASSES = 2, 256, 1024
STATS = ("nodes", "blind", "seam_vertices", "spread_before", "spread_after", "max_offset", "n_clamped", "n_passes")


# ---- nodes ---------------------------------------------------------------------------------------------------------------------------
def contributing(xyz, tri, view):
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    X = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])
    finite = np.isfinite(X[tri]).all(axis=(1, 2)) if len(tri) else np.zeros(0, bool)
    return (np.asarray(view, np.int64).reshape(-1) >= 0) & distinct & finite


def nodes_dict(xyz, tri, view):
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    on = contributing(xyz, tri, view)
    keys = sorted({(int(tri[t, q]), int(view[t])) for t in range(len(tri)) if on[t] for q in range(3)})
    number = {k: n for n, k in enumerate(keys)}
    node_of = np.full((len(tri), 3), -1, np.int32)
    for t in range(len(tri)):
        if on[t]:
            node_of[t] = [number[(int(tri[t, q]), int(view[t]))] for q in range(3)]
    return {"n_nodes": len(keys), "node_vertex": np.asarray([k[0] for k in keys], np.int32).reshape(-1),
            "node_view": np.asarray([k[1] for k in keys], np.int32).reshape(-1), "node_of": node_of}


def nodes_np(xyz, tri, view):
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    on = contributing(xyz, tri, view)
    key = (tri << 32) | np.asarray(view, np.int64).reshape(-1, 1)
    uniq, inverse = np.unique(key[on].reshape(-1), return_inverse=True)
    node_of = np.full((len(tri), 3), -1, np.int32)
    node_of[on] = inverse.reshape(-1, 3)
    return {"n_nodes": len(uniq), "node_vertex": (uniq >> 32).astype(np.int32), "node_view": (uniq & 0xffffffff).astype(np.int32), "node_of": node_of}


# ---- node colours ------------------------------------------------------------------------------------------------------------------------
def mean(total, n):
    return (32 * total + n) // (2 * n)


def colours_loop(xyz, images, K, P, node_vertex, node_view, r):
    """seen uint8 [n], F int32 [n, 3] and the sums int64 [n, 3]"""
    k4 = to.k4_of(K)
    Pd = np.asarray(P, np.float32).reshape(-1, 12).astype(np.float64)
    X = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(node_vertex)
    seen, F, sums = np.zeros(n, np.uint8), np.zeros((n, 3), np.int32), np.zeros((n, 3), np.int64)
    for i in range(n):
        img = images[int(node_view[i])]
        h, w = img.shape[:2]
        coord, _, _, _ = to.texel_coord(k4, Pd[int(node_view[i])].tolist(), X[int(node_vertex[i])].tolist(), w, h)
        if coord is None:
            continue
        seen[i] = 1
        for c in range(3):
            total = 0
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    total += to.sample12(img, c, min(max(coord[0] + 16 * dx, 0), 16 * (w - 1)), min(max(coord[1] + 16 * dy, 0), 16 * (h - 1)))
            sums[i, c], F[i, c] = total, mean(total, (2 * r + 1) ** 2)
    return seen, F, sums


def _sample_np(raw, off, wv, hv, ch, c, su, sv):
    x0, fx, y0, fy = su >> 4, su & 15, sv >> 4, sv & 15
    x1, y1 = np.minimum(x0 + 1, wv - 1), np.minimum(y0 + 1, hv - 1)
    at = lambda y, x: raw[off + (y * wv + x) * ch + (c if ch == 3 else 0)]
    return ((16 - fx) * (16 - fy) * at(y0, x0) + fx * (16 - fy) * at(y0, x1) + (16 - fx) * fy * at(y1, x0) + fx * fy * at(y1, x1) + 8) >> 4


def colours_np(xyz, images, K, P, node_vertex, node_view, r):
    n = len(node_vertex)
    seen, F, sums = np.zeros(n, np.uint8), np.zeros((n, 3), np.int32), np.zeros((n, 3), np.int64)
    if n == 0:
        return seen, F, sums
    k4 = to.k4_of(K)
    raw, raw_off, _, _, w, h, ch = to._flat(images, [None] * len(images))
    Pd = np.asarray(P, np.float32).reshape(-1, 12).astype(np.float64)
    X = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)[np.asarray(node_vertex, np.int64)]
    nv = np.asarray(node_view, np.int64)
    wv, hv = w[nv], h[nv]
    with np.errstate(all="ignore"):
        q, u, v = to._project_np(k4, Pd[nv], X)
        ok = (q[..., 2] > 0.0) & ~np.isnan(u) & ~np.isnan(v)
        uc = np.minimum(np.maximum(np.where(ok, u, 0.0), 0.0), (wv - 1).astype(np.float64))
        vc = np.minimum(np.maximum(np.where(ok, v, 0.0), 0.0), (hv - 1).astype(np.float64))
    su, sv = to._fix_np(uc), to._fix_np(vc)
    for c in range(3):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                sums[:, c] += _sample_np(raw, raw_off[nv], wv, hv, ch, c, np.clip(su + 16 * dx, 0, 16 * (wv - 1)), np.clip(sv + 16 * dy, 0, 16 * (hv - 1)))
    sums[~ok] = 0
    cnt = (2 * r + 1) ** 2
    F[:] = np.where(ok[:, None], (32 * sums + cnt) // (2 * cnt), 0)
    return ok.astype(np.uint8), F, sums


def nodes(xyz, tri, images, K, P, view, r, nodes_fn=nodes_np, colours_fn=colours_np):
    """what sfmba_mesh_colour_nodes writes, as capi.mesh_colour_nodes returns it (and the sums)"""
    out = nodes_fn(xyz, tri, view)
    out["seen"], out["F"], out["sums"] = colours_fn(xyz, images, K, P, out["node_vertex"], out["node_view"], r)
    return out


# ---- a pass ------------------------------------------------------------------------------------------------------------------------------
def pass_loop(node_vertex, seen, F, node_of, w, g, trace=None):
    """g^{i+1} from g^i in Python integers; trace (a list) receives (n, c, A, a, B, b, num, den) of every seeing node and channel"""
    n_nodes = len(node_vertex)
    sib, links = {}, [[] for _ in range(n_nodes)]
    for n in range(n_nodes):
        if seen[n]:
            sib.setdefault(int(node_vertex[n]), []).append(n)
    for row in np.asarray(node_of).reshape(-1, 3).tolist():
        if row[0] < 0:
            continue
        for q in range(3):
            links[row[q]] += [u for u in (row[(q + 1) % 3], row[(q + 2) % 3]) if seen[u]]
    out = np.zeros((n_nodes, 3), np.int32)
    for n in range(n_nodes):
        if not seen[n]:
            continue
        group = sib[int(node_vertex[n])]
        k = len(group)
        for c in range(3):
            A = sum((int(F[m, c]) + int(g[m, c])) - int(F[n, c]) for m in group) if k >= 2 else 0
            a = k if k >= 2 else 0
            B, b = sum(int(g[u, c]) for u in links[n]), len(links[n])
            den, num = w * a + b, w * A + B
            out[n, c] = int(g[n, c]) if den == 0 else min(max((2 * num + den) // (2 * den), -F_MAX), F_MAX)
            if trace is not None:
                trace.append((n, c, A, a, B, b, num, den))
    return out


def _structure_np(node_vertex, seen, node_of):
    see = np.asarray(seen).astype(bool)
    vert = np.asarray(node_vertex, np.int64)
    rows = np.asarray(node_of, np.int64).reshape(-1, 3)
    rows = rows[rows[:, 0] >= 0] if len(rows) else rows
    src = np.concatenate([rows[:, q] for q in range(3) for _ in range(2)]) if len(rows) else np.zeros(0, np.int64)
    dst = np.concatenate([rows[:, (q + o) % 3] for q in range(3) for o in (1, 2)]) if len(rows) else np.zeros(0, np.int64)
    keep = see[dst] if len(dst) else np.zeros(0, bool)
    return see, vert, src[keep], dst[keep]


def pass_np(node_vertex, seen, F, node_of, w, g):
    n_nodes = len(node_vertex)
    if n_nodes == 0:
        return np.zeros((0, 3), np.int32)
    see, vert, src, dst = _structure_np(node_vertex, seen, node_of)
    F, g = np.asarray(F, np.int64), np.asarray(g, np.int64)
    nvert = int(vert.max()) + 1
    k = np.zeros(nvert, np.int64)
    np.add.at(k, vert[see], 1)
    total = np.zeros((nvert, 3), np.int64)
    np.add.at(total, vert[see], (F + g)[see])
    kn = k[vert]
    seam = (kn >= 2)[:, None]
    A, a = np.where(seam, total[vert] - kn[:, None] * F, 0), np.where(seam, kn[:, None], 0)
    B, b = np.zeros((n_nodes, 3), np.int64), np.zeros(n_nodes, np.int64)
    np.add.at(B, src, g[dst])
    np.add.at(b, src, 1)
    den, num = w * a + b[:, None], w * A + B
    new = np.clip((2 * num + den) // np.maximum(2 * den, 1), -F_MAX, F_MAX)
    return np.where(see[:, None], np.where(den == 0, g, new), 0).astype(np.int32)


def spreads(node_vertex, seen, F, g):
    """(seam vertices, the summed spread of F, the summed spread of F + g)"""
    groups = {}
    for n in range(len(node_vertex)):
        if seen[n]:
            groups.setdefault(int(node_vertex[n]), []).append(n)
    seams = [np.asarray(m) for m in groups.values() if len(m) >= 2]
    F, Fg = np.asarray(F, np.int64), np.asarray(F, np.int64) + np.asarray(g, np.int64)
    return len(seams), int(sum((F[m].max(0) - F[m].min(0)).sum() for m in seams)), int(sum((Fg[m].max(0) - Fg[m].min(0)).sum() for m in seams))


def level(node_vertex, seen, F, node_of, w, passes, pass_fn=pass_np, history=None):
    """what sfmba_mesh_colour_level writes: (g int32 [n, 3], stats int64 [8]); history (a list) receives g after every pass"""
    n = len(node_vertex)
    g = np.zeros((n, 3), np.int32)
    for _ in range(passes):
        g = pass_fn(node_vertex, seen, F, node_of, w, g)
        if history is not None:
            history.append(g)
    seams, before, after = spreads(node_vertex, seen, F, g)
    stats = np.asarray([n, int((np.asarray(seen) == 0).sum()), seams, before, after, int(np.abs(g).max()) if n else 0, 0, passes], np.int64)
    return g, stats


def refused_level(node_vertex, F, node_of, n_nodes, w, passes):
    rows = np.asarray(node_of, np.int64).reshape(-1, 3)
    return (w < 1 or w > MAX_WEIGHT or passes < 0 or passes > MAX_PASSES or (len(rows) and (rows.min() < -1 or rows.max() >= n_nodes)) or
            (len(rows) and ((rows < 0).sum(1) % 3 != 0).any()) or (np.diff(np.asarray(node_vertex, np.int64)) < 0).any() or
            (len(F) and (np.min(F) < 0 or np.max(F) > F_MAX)))


# ---- the levelled raster ----------------------------------------------------------------------------------------------------------------
def levelled_texel(S, s12, G):
    """(texel, clamped)"""
    f = (16 * (S - 2) * s12 + G + 128 * (S - 2)) // (256 * (S - 2))
    return min(max(f, 0), 255), f < 0 or f > 255


def raster_loop(xyz, bgr, tri, images, K, P, view, S, B, node_of, g, trace=None):
    """(atlas, n_clamped); trace (a list) receives (t, i, j, G [3], texel [3], clamped) of every sampled texel"""
    atlas = to.raster_loop(xyz, bgr, tri, images, K, P, view, S, B)
    k4 = to.k4_of(K)
    Pd = np.asarray(P, np.float32).reshape(-1, 12).astype(np.float64)
    X = np.asarray(xyz, np.float32).astype(np.float64)
    n_clamped = 0
    for t, idx in enumerate(np.asarray(tri).tolist()):
        n = int(view[t])
        if n < 0:
            continue
        A, Bc, C = (X[v].tolist() for v in idx)
        off = [[0, 0, 0] if m < 0 else [int(x) for x in g[m]] for m in np.asarray(node_of[t]).tolist()]
        img = images[n]
        for j in range(S):
            for i in range(S - j):
                coord, _, _, _ = to.texel_coord(k4, Pd[n].tolist(), to.point(S, i, j, A, Bc, C), img.shape[1], img.shape[0])
                if coord is None:
                    continue
                px, Gs, clamped = [], [], False
                for ch in range(3):
                    G = ((S - 2 - i - j) * off[0][ch] + i * off[1][ch]) + j * off[2][ch]
                    value, c = levelled_texel(S, to.sample12(img, ch, *coord), G)
                    px.append(value)
                    Gs.append(G)
                    clamped = clamped or c
                n_clamped += clamped
                if trace is not None:
                    trace.append((t, i, j, Gs, px, clamped))
                ax, ay = to.atlas_pixel(t, S, B, i, j)
                atlas[ay, ax] = px
    return atlas, n_clamped


def raster_np(xyz, bgr, tri, images, K, P, view, S, B, node_of, g):
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    nt, n = len(tri), len(images)
    atlas = to.raster_np(xyz, bgr, tri, images, K, P, view, S, B)                  # the fallback texels and the layout
    if nt == 0 or n == 0:
        return atlas, 0
    W, H = to.atlas_size(nt, S, B)
    owner, i, j = to.ownership(nt, S, B, W, H)
    own = owner >= 0
    t = np.where(own, owner, 0)
    wA, wB, wC = S - 2 - i - j, i, j
    vw = np.asarray(view, np.int64)[t]
    k4 = to.k4_of(K)
    raw, raw_off, _, _, w, h, ch = to._flat(images, [None] * n)
    Pd = np.asarray(P, np.float32).reshape(-1, 12).astype(np.float64)
    X = np.asarray(xyz, np.float32).astype(np.float64)[tri][t]
    nv = np.where(vw >= 0, vw, 0)
    with np.errstate(all="ignore"):
        fA, fB, fC = (a.astype(np.float64)[..., None] for a in (wA, wB, wC))
        Xp = ((fA * X[:, :, 0] + fB * X[:, :, 1]) + fC * X[:, :, 2]) / float(S - 2)
        q, u, v = to._project_np(k4, Pd[nv], Xp)
        ok = own & (vw >= 0) & (q[..., 2] > 0.0) & ~np.isnan(u) & ~np.isnan(v)
        wv, hv = w[nv], h[nv]
        uc = np.minimum(np.maximum(np.where(ok, u, 0.0), 0.0), (wv - 1).astype(np.float64))
        vc = np.minimum(np.maximum(np.where(ok, v, 0.0), 0.0), (hv - 1).astype(np.float64))
    su, sv = to._fix_np(uc), to._fix_np(vc)
    rows = np.asarray(node_of, np.int64).reshape(-1, 3)[t]                           # [H, W, 3 corners]
    gz = np.concatenate([np.asarray(g, np.int64).reshape(-1, 3), np.zeros((1, 3), np.int64)])       # the last row: no node
    off = gz[np.where(rows >= 0, rows, len(gz) - 1)]                                   # [H, W, corner, channel]
    clamped = np.zeros((H, W), bool)
    out = atlas.astype(np.int64)
    for k in range(3):
        s12 = _sample_np(raw, raw_off[nv], wv, hv, ch, k, su, sv)
        G = (wA * off[:, :, 0, k] + wB * off[:, :, 1, k]) + wC * off[:, :, 2, k]
        f = (16 * (S - 2) * s12 + G + 128 * (S - 2)) // (256 * (S - 2))
        clamped |= ok & ((f < 0) | (f > 255))
        out[..., k] = np.where(ok, np.clip(f, 0, 255), out[..., k])
    return out.astype(np.uint8), int(clamped.sum())


# ---- the calls ---------------------------------------------------------------------------------------------------------------------------
def texture_levelled(xyz, bgr, tri, images, K, P, view, node_of, g, patch, blocks_per_row, raster_fn=raster_np):
    """what sfmba_mesh_texture_levelled writes, as capi.mesh_texture_levelled returns it"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    tri = np.asarray(tri, np.int32).reshape(-1, 3)
    B = to.default_blocks_per_row(len(tri)) if blocks_per_row is None else blocks_per_row
    Bl = B if len(tri) else 1
    atlas, n_clamped = raster_fn(xyz, bgr, tri, images, K, P, view, patch, Bl, node_of, g)
    return {"atlas": atlas, "uv": to.corner_uv(len(tri), patch, Bl), "n_textured": int((np.asarray(view) >= 0).sum()), "n_clamped": n_clamped}


def texture_adjust(xyz, bgr, tri, images, K, P, depth_maps, occl_tol, min_area, patch, blocks_per_row, k, rings, penalty, max_passes, radius, weight,
                   passes):
    """what sfmba_mesh_texture_adjust writes, as capi.mesh_texture_adjust returns it (and the nodes and the offsets)"""
    out = lo.texture_smooth(xyz, bgr, tri, images, K, P, depth_maps, occl_tol, min_area, patch, blocks_per_row, k, rings, penalty, max_passes)
    nd = nodes(xyz, tri, images, K, P, out["view"], radius)
    g, stats = level(nd["node_vertex"], nd["seen"], nd["F"], nd["node_of"], weight, passes)
    tex = texture_levelled(xyz, bgr, tri, images, K, P, out["view"], nd["node_of"], g, patch, blocks_per_row)
    stats[6] = tex["n_clamped"]
    out.update(atlas=tex["atlas"], level_stats=stats, nodes=nd, g=g)
    return out
