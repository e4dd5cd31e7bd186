"""The CPU restatement of the view-label smoothing (the contract is in include/sfmba.h, "smoothing the view labels"), every part stated
TWICE:

  * the candidates as a loop per triangle and view over texture_oracle.candidate / eligible (candidates_loop) and as numpy over all
    (triangle, view) pairs with a stable sort per row (candidates_np);
  * the adjacency as a dict of edges (adjacency_dict) and as a stable argsort of the 64-bit keys (adjacency_sort);
  * diffusion, start and passes as a loop per triangle in Python integers (smooth_loop), which also checks the 2^53 bound, and as numpy
    over whole arrays (smooth_np).  Both record the energy before every pass and the movers and gains of every pass.

Everything past the scores is integer arithmetic."""
import numpy as np

import texture_oracle as to

MAX_K, MAX_RINGS, MAX_PENALTY, MAX_PASSES = 8, 8, 65535, 10000
SCORE_LIMIT = 1 << 37
STATS = ("energy_start", "energy_end", "diff_rank0", "diff_start", "diff_end", "frontier", "moves", "n_passes")


# ---- candidates ----------------------------------------------------------------------------------------------------------------------
def candidates_loop(xyz, tri, images, K, P, depth_maps, occl_tol, min_area, k):
    k4, tol = to.k4_of(K), float(np.float32(occl_tol))
    views = to._views(images, P, depth_maps)
    X = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    tri = np.asarray(tri).reshape(-1, 3)
    cv, cs = np.full((len(tri), k), -1, np.int32), np.zeros((len(tri), k), np.int64)
    for t, idx in enumerate(tri.tolist()):
        if len(set(idx)) < 3 or not np.isfinite(X[idx]).all():
            continue
        corners = [X[v].tolist() for v in idx]
        row = []                                                                # (view, score), the list insertion of label_math.h
        for n, (p, w, h, dmap) in enumerate(views):
            cand, a2 = to.candidate(k4, p, corners, w, h, dmap, tol)
            if not to.eligible(cand, a2, min_area):
                continue
            at = len(row)
            for j, (_, s) in enumerate(row):
                if -a2 > s:
                    at = j
                    break
            row.insert(at, (n, -a2))
            del row[k:]
        for j, (n, s) in enumerate(row):
            cv[t, j], cs[t, j] = n, s
    return cv, cs


def scores_np(xyz, tri, images, K, P, depth_maps, occl_tol, min_area):
    """int64 [nt, n]: the score of every (triangle, view), 0 where the view is not eligible (texture_oracle.views_np's arithmetic)"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    nt, n = len(tri), len(images)
    if nt == 0 or n == 0:
        return np.zeros((nt, n), np.int64)
    k4, tol = to.k4_of(K), float(np.float32(occl_tol))
    raw, raw_off, maps, map_off, w, h, ch = to._flat(images, depth_maps)
    Pd = np.asarray(P, np.float32).reshape(-1, 12).astype(np.float64)
    X = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)[tri]
    good = (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2]) & np.isfinite(X).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        q, u, v = to._project_np(k4, Pd[None, :, None, :], X[:, None, :, :])
        wv, hv = w[None, :, None], h[None, :, None]
        ok = (q[..., 2] > 0.0) & (u >= 0.0) & (u <= (wv - 1).astype(np.float64)) & (v >= 0.0) & (v <= (hv - 1).astype(np.float64))
        us, vs = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
        su, sv = to._fix_np(us), to._fix_np(vs)
        px, py = np.floor(us + 0.5).astype(np.int64), np.floor(vs + 0.5).astype(np.int64)
        has_map = (map_off >= 0)[None, :, None]
        zs = maps[np.where(has_map, map_off[None, :, None] + py * wv + px, 0)]
        ok &= ~has_map | ((zs > 0.0) & ((q[..., 2] - zs) <= tol))
    cand = ok.all(axis=2) & good[:, None]
    a2 = (su[..., 1] - su[..., 0]) * (sv[..., 2] - sv[..., 0]) - (sv[..., 1] - sv[..., 0]) * (su[..., 2] - su[..., 0])
    return np.where(cand & (-a2 > 0) & (-a2 >= min_area), -a2, 0).astype(np.int64)


def candidates_np(xyz, tri, images, K, P, depth_maps, occl_tol, min_area, k):
    s = scores_np(xyz, tri, images, K, P, depth_maps, occl_tol, min_area)
    nt, n = s.shape
    cv, cs = np.full((nt, k), -1, np.int32), np.zeros((nt, k), np.int64)
    m = min(k, n)
    if nt and m:
        order = np.argsort(-s, axis=1, kind="stable")[:, :m]                    # descending score, the lower view first on a tie
        top = np.take_along_axis(s, order, 1)
        cv[:, :m], cs[:, :m] = np.where(top > 0, order, -1), top
    return cv, cs


# ---- adjacency -------------------------------------------------------------------------------------------------------------------------
def adjacency_dict(tri):
    """(adj int32 [nt, 3], n_pairs, n_open_edges, n_nonmanifold_edges)"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    edges = {}
    for t, idx in enumerate(tri.tolist()):
        if len(set(idx)) < 3:
            continue
        for q in range(3):
            a, b = idx[q], idx[(q + 1) % 3]
            edges.setdefault((min(a, b), max(a, b)), []).append((t, q))
    adj = np.full((len(tri), 3), -1, np.int32)
    counts = [0, 0, 0]
    for users in edges.values():
        counts[0 if len(users) == 2 else (1 if len(users) == 1 else 2)] += 1
        if len(users) == 2:
            (t0, q0), (t1, q1) = users
            adj[t0, q0], adj[t1, q1] = t1, t0
    return adj, counts[0], counts[1], counts[2]


def adjacency_sort(tri):
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    nt = len(tri)
    adj = np.full((nt, 3), -1, np.int32)
    if nt == 0:
        return adj, 0, 0, 0
    a, b = tri, np.roll(tri, -1, axis=1)
    keys = ((np.minimum(a, b).astype(np.uint64) << np.uint64(32)) | np.maximum(a, b).astype(np.uint64)).reshape(-1)
    bad = np.repeat((tri[:, 0] == tri[:, 1]) | (tri[:, 0] == tri[:, 2]) | (tri[:, 1] == tri[:, 2]), 3)
    keys[bad] = np.uint64(0xFFFFFFFFFFFFFFFF)
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    real = ks != np.uint64(0xFFFFFFFFFFFFFFFF)
    head = np.concatenate([[True], ks[1:] != ks[:-1]])
    run = np.cumsum(head) - 1
    length = np.bincount(run)[run]
    first = np.flatnonzero(head)
    n_real = real[first]
    lens = length[first]
    two = real & (length == 2)
    pos = np.flatnonzero(two)
    partner = np.where(head[pos], pos + 1, pos - 1)
    adj.reshape(-1)[order[pos]] = order[partner] // 3
    return adj, int((n_real & (lens == 2)).sum()), int((n_real & (lens == 1)).sum()), int((n_real & (lens >= 3)).sum())


# ---- smoothing: the loop statement -------------------------------------------------------------------------------------------------------
def _energy_loop(cv, D, rank, view, adj, p):
    e = diff = frontier = 0
    for t in range(len(view)):
        if rank is not None and rank[t] >= 0:
            e += D[t][rank[t]]
        for n in adj[t]:
            if n > t:
                if view[t] >= 0 and view[n] >= 0:
                    diff += view[t] != view[n]
                elif (view[t] >= 0) != (view[n] >= 0):
                    frontier += 1
    return e + p * diff, diff, frontier


def smooth_loop(cand_view, cand_score, adj, rings, penalty, max_passes):
    """dict: view int32 [nt], stats int64 [8], rank, start (the labels after the start), s (the diffused sums), D, and per pass
    energy (before it), movers (sorted), gains (all, before it)"""
    cv, cs, adj = np.asarray(cand_view).tolist(), np.asarray(cand_score).tolist(), np.asarray(adj).reshape(-1, 3).tolist()
    nt = len(cv)
    K = np.asarray(cand_view).shape[1] if np.asarray(cand_view).ndim == 2 else 0
    s = [row[:] for row in cs]
    for _ in range(rings):
        nxt = [[0] * K for _ in range(nt)]
        for t in range(nt):
            for k in range(K):
                if cv[t][k] < 0:
                    continue
                acc = s[t][k]
                for n in adj[t]:
                    if n >= 0 and cv[t][k] in cv[n]:
                        acc += s[n][cv[n].index(cv[t][k])]
                assert acc < 1 << 53
                nxt[t][k] = acc
        s = nxt
    rank = [-1] * nt
    for t in range(nt):
        for k in range(K):
            if cv[t][k] >= 0 and (rank[t] < 0 or s[t][k] > s[t][rank[t]]):
                rank[t] = k
    view = [cv[t][rank[t]] if rank[t] >= 0 else -1 for t in range(nt)]
    view0 = [cv[t][0] if K else -1 for t in range(nt)]
    D = [[(1024 * (cs[t][0] - cs[t][k])) // cs[t][0] if cv[t][0] >= 0 and cv[t][k] >= 0 else 0 for k in range(K)] for t in range(nt)]
    assert all(0 <= d <= 1023 for row in D for d in row)
    _, diff0, frontier = _energy_loop(cv, D, None, view0, adj, penalty)
    e_start, diff_start, _ = _energy_loop(cv, D, rank, view, adj, penalty)
    start = list(view)
    trace, moves, n_passes = [], 0, 0
    for _ in range(max_passes if nt else 0):
        gain, kstar = [0] * nt, list(rank)
        for t in range(nt):
            if rank[t] < 0:
                continue
            best = None
            for k in range(K):
                if cv[t][k] < 0:
                    continue
                e = D[t][k] + penalty * sum(1 for n in adj[t] if n >= 0 and view[n] >= 0 and view[n] != cv[t][k])
                if best is None or e < best:
                    best, kstar[t] = e, k
                if k == rank[t]:
                    e_rank = e
            gain[t] = e_rank - best
        movers = [t for t in range(nt) if gain[t] > 0 and
                  all(gain[t] > gain[n] or (gain[t] == gain[n] and t < n) for n in adj[t] if n >= 0)]
        trace.append({"energy": _energy_loop(cv, D, rank, view, adj, penalty)[0], "movers": movers, "gains": gain})
        if not movers:
            break
        for t in movers:
            rank[t] = kstar[t]
            view[t] = cv[t][kstar[t]]
        moves += len(movers)
        n_passes += 1
    e_end, diff_end, _ = _energy_loop(cv, D, rank, view, adj, penalty)
    stats = np.asarray([e_start, e_end, diff0, diff_start, diff_end, frontier, moves, n_passes], np.int64)
    return {"view": np.asarray(view, np.int32).reshape(nt), "stats": stats, "rank": np.asarray(rank, np.int64).reshape(nt),
            "start": np.asarray(start, np.int32).reshape(nt), "s": np.asarray(s, np.int64).reshape(nt, K),
            "D": np.asarray(D, np.int64).reshape(nt, K), "trace": trace, "energy_end": e_end}


# ---- smoothing: the array statement ------------------------------------------------------------------------------------------------------
def _look_np(cv, s, adj):
    """int64 [nt, 3, K]: per triangle, neighbour entry and own rank, the neighbour's sum for the own view (0: no neighbour, not listed)"""
    nt, K = cv.shape
    n = np.where(adj >= 0, adj, 0)
    ncv, ns = cv[n], s[n]                                                        # [nt, 3, K]
    match = (ncv[:, :, None, :] == cv[:, None, :, None]) & (cv[:, None, :, None] >= 0) & (adj >= 0)[:, :, None, None]      # [nt, 3, own k, j]
    first = match & (np.cumsum(match, axis=3) == 1)
    return (first * ns[:, :, None, :]).sum(axis=3)


def _energy_np(D, rank, view, adj, p):
    nt = len(view)
    t = np.arange(nt)[:, None]
    n = np.where(adj >= 0, adj, 0)
    pair = adj > t
    vt, vn = view[:, None], view[n]
    diff = int((pair & (vt >= 0) & (vn >= 0) & (vt != vn)).sum())
    frontier = int((pair & ((vt >= 0) != (vn >= 0))).sum())
    e = 0 if rank is None else int(D[np.arange(nt), np.maximum(rank, 0)][rank >= 0].sum())
    return e + p * diff, diff, frontier


def smooth_np(cand_view, cand_score, adj, rings, penalty, max_passes):
    cv, cs = np.asarray(cand_view, np.int64), np.asarray(cand_score, np.int64)
    adj = np.asarray(adj, np.int64).reshape(-1, 3)
    nt = len(cv)
    K = cv.shape[1] if cv.ndim == 2 else 0
    cv, cs = cv.reshape(nt, K), cs.reshape(nt, K)
    if nt == 0:
        return {"view": np.zeros(0, np.int32), "stats": np.zeros(8, np.int64), "rank": np.zeros(0, np.int64), "start": np.zeros(0, np.int32), "s": cs,
                "D": cs, "trace": [], "energy_end": 0}
    has = cv >= 0
    s = cs.copy()
    for _ in range(rings):
        s = np.where(has, s + _look_np(cv, s, adj).sum(axis=1), 0)
    big = np.where(has, s, -1)
    rank = np.where(has.any(axis=1), np.argmax(big, axis=1), -1)
    rows = np.arange(nt)
    view = np.where(rank >= 0, cv[rows, np.maximum(rank, 0)], -1)
    s0 = np.where(cs[:, :1] > 0, cs[:, :1], 1)
    D = np.where(has & has[:, :1], (1024 * (cs[:, :1] - cs)) // s0, 0)
    _, diff0, frontier = _energy_np(D, None, cv[:, 0], adj, penalty)
    e_start, diff_start, _ = _energy_np(D, rank, view, adj, penalty)
    start = view.copy()
    trace, moves, n_passes = [], 0, 0
    n = np.where(adj >= 0, adj, 0)
    for _ in range(max_passes):
        vn = np.where(adj >= 0, view[n], -1)                                      # [nt, 3]
        clash = ((vn[:, :, None] >= 0) & (vn[:, :, None] != cv[:, None, :])).sum(axis=1)
        e = np.where(has, D + penalty * clash, np.iinfo(np.int64).max)
        kstar = np.argmin(e, axis=1)
        gain = np.where(rank >= 0, e[rows, np.maximum(rank, 0)] - e[rows, kstar], 0)
        gn = gain[n]
        beats = (adj < 0) | (gain[:, None] > gn) | ((gain[:, None] == gn) & (rows[:, None] < adj))
        movers = np.flatnonzero((gain > 0) & beats.all(axis=1))
        trace.append({"energy": _energy_np(D, rank, view, adj, penalty)[0], "movers": movers.tolist(), "gains": gain.tolist()})
        if not len(movers):
            break
        rank[movers] = kstar[movers]
        view[movers] = cv[movers, kstar[movers]]
        moves += len(movers)
        n_passes += 1
    e_end, diff_end, _ = _energy_np(D, rank, view, adj, penalty)
    stats = np.asarray([e_start, e_end, diff0, diff_start, diff_end, frontier, moves, n_passes], np.int64)
    return {"view": view.astype(np.int32), "stats": stats, "rank": rank, "start": start.astype(np.int32), "s": s, "D": D, "trace": trace,
            "energy_end": e_end}


# ---- the calls -------------------------------------------------------------------------------------------------------------------------
def final_score(cand_score, rank):
    cs = np.asarray(cand_score, np.int64)
    return np.where(rank >= 0, cs[np.arange(len(cs)), np.maximum(rank, 0)], 0).astype(np.int64) if len(cs) else np.zeros(0, np.int64)


def texture_smooth(xyz, bgr, tri, images, K, P, depth_maps, occl_tol, min_area, patch, blocks_per_row, k, rings, penalty, max_passes,
                   smooth_fn=smooth_np, candidates_fn=candidates_np):
    """what sfmba_mesh_texture_smooth writes, as capi.mesh_texture_smooth returns it"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    tri = np.asarray(tri, np.int32).reshape(-1, 3)
    B = to.default_blocks_per_row(len(tri)) if blocks_per_row is None else blocks_per_row
    Bl = B if len(tri) else 1
    cv, cs = candidates_fn(xyz, tri, images, K, P, depth_maps, occl_tol, min_area, k)
    adj = adjacency_sort(tri)[0]
    sm = smooth_fn(cv, cs, adj, rings, penalty, max_passes)
    view = sm["view"]
    atlas = to.raster_np(xyz, bgr, tri, images, K, P, view, patch, Bl)
    rank = sm["rank"] if len(tri) else np.zeros(0, np.int64)
    return {"atlas": atlas, "uv": to.corner_uv(len(tri), patch, Bl), "view": view, "score": final_score(cs, np.asarray(rank)),
            "n_textured": int((view >= 0).sum()), "stats": sm["stats"], "cand_view": cv, "cand_score": cs, "adj": adj}
