"""CPU restatement of sfmba_mesh_decimate (the contract is in include/sfmba.h; csrc/decimate_math.h is the arithmetic the kernels
run) -- TEST INFRASTRUCTURE ONLY.

Every part is stated twice:
  * clusters, member sums and quadric sums: a dict of cells walked in Python integers (decimate_loop), and a stable sort of the keys
    with np.add.reduceat / np.add.at on int64 arrays (decimate_np);
  * the solve: scalar float64 operations (solve_one), and the same on arrays (solve_np);
  * the duplicate rule: a walk with a set of frozen triples (decimate_loop), and a lexicographic sort (decimate_np).
Python floats are IEEE doubles, math.sqrt and numpy's sqrt are correctly rounded and every operation below is written on its own,
so both statements, the header built for the host and the device agree BIT FOR BIT.  The quantisation, the cross product and the
position are those of tests/mesh_clean_oracle.py."""
import math

import numpy as np

import mesh_clean_oracle as co

MIN_CELL, MAX_CELL, MAX_REG = 32, 1 << 20, 1 << 20
MAX_INC = 1 << 16
BIAS = 1 << 20
UNIT = 1024.0
ROW = ((0, 1, 2), (1, 3, 4), (2, 4, 5))          # the symmetric 3 x 3 in six entries: 00 01 02 11 12 22


def _tri(tri):
    return np.ascontiguousarray(tri, np.int32).reshape(-1, 3)


def valid_params(cell, placement, reg):
    return MIN_CELL <= cell <= MAX_CELL and placement in (0, 1) and (placement == 0 or 1 <= reg <= MAX_REG)


def key_of(c):
    return ((c[2] + BIAS) << 42) | ((c[1] + BIAS) << 21) | (c[0] + BIAS)


def mean_round(S, n):
    return (2 * S + n) // (2 * n)


def unit_normal(N):
    """u [3] Python integers in units of 2^-10, or None when the triangle has no area"""
    n = [float(v) for v in N]
    length = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    if length == 0.0:
        return None
    return [int(math.floor((v / length) * UNIT + 0.5)) for v in n]


def quadric_terms(u, r):
    """what a triangle with the normal u adds to the cluster of a vertex with the remainder r: A (six), b (three), 1"""
    e = (u[0] * r[0] + u[1] * r[1]) + u[2] * r[2]
    return [u[0] * u[0], u[0] * u[1], u[0] * u[2], u[1] * u[1], u[1] * u[2], u[2] * u[2], u[0] * e, u[1] * e, u[2] * e, 1]


def solve_one(q, Sp, n, reg, cell, trace=None):
    """R [3] of a cluster from its quadric sums q [10], or None where the cluster takes the mean.  Scalar float64 operations."""
    n_inc = q[9]
    if n_inc == 0 or n_inc > MAX_INC:
        return None
    rho = float(reg) * float(n_inc)
    s = [float(v) for v in q[:6]]
    s[0] = s[0] + rho
    s[3] = s[3] + rho
    s[5] = s[5] + rho
    g = []
    for a in range(3):
        m = float(Sp[a]) / float(n)
        g.append(float(q[6 + a]) + rho * m)
    s00, s01, s02, s11, s12, s22 = s
    c = [s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11, s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01]
    det = (s00 * c[0] + s01 * c[1]) + s02 * c[2]
    x = []
    for a in range(3):
        num = (c[ROW[a][0]] * g[0] + c[ROW[a][1]] * g[1]) + c[ROW[a][2]] * g[2]
        if det == 0.0:
            x.append(math.nan if num == 0.0 or math.isnan(num) else math.copysign(math.inf, num) * math.copysign(1.0, det))
        else:
            x.append(num / det)
    if trace is not None:
        trace.update(s=s, g=g, c=c, det=det, x=x)
    if not det > 0.0 or not all(math.isfinite(v) for v in x):
        return None
    out = []
    for v in x:
        f = math.floor(v + 0.5)
        out.append(0 if f < 0 else cell - 1 if f > cell - 1 else int(f))
    return out


def solve_np(Q, Sp, n, reg, cell):
    """Q int64 [m, 10], Sp int64 [m, 3], n int64 [m] -> (R int64 [m, 3], solved bool [m]); the same operations on arrays"""
    n_inc = Q[:, 9]
    with np.errstate(all="ignore"):
        rho = float(reg) * n_inc.astype(np.float64)
        s = Q[:, :6].astype(np.float64)
        for k in (0, 3, 5):
            s[:, k] = s[:, k] + rho
        m = Sp.astype(np.float64) / n.astype(np.float64)[:, None]
        g = Q[:, 6:9].astype(np.float64) + rho[:, None] * m
        s00, s01, s02, s11, s12, s22 = (s[:, k] for k in range(6))
        c = [s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11, s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01]
        det = (s00 * c[0] + s01 * c[1]) + s02 * c[2]
        x = np.stack([((c[ROW[a][0]] * g[:, 0] + c[ROW[a][1]] * g[:, 1]) + c[ROW[a][2]] * g[:, 2]) / det for a in range(3)], axis=1)
        ok = (n_inc > 0) & (n_inc <= MAX_INC) & (det > 0.0) & np.isfinite(x).all(axis=1)
        f = np.floor(np.where(ok[:, None], x, 0.0) + 0.5)
        R = np.clip(f, 0.0, float(cell - 1)).astype(np.int64)
    return R, ok


def _empty(nv, colour):
    return dict(xyz=np.zeros((0, 3), np.float32), bgr=np.zeros((0, 3), np.uint8) if colour else None, members=np.zeros(0, np.int32),
                tri=np.zeros((0, 3), np.int32), triangle_of=np.zeros(0, np.int32), vertex_of=np.full(nv, -1, np.int32))


# ---- statement one: a dict of cells, Python integers, scalar floats, a set of triples --------------------------------------------
def decimate_loop(xyz, bgr, tri, origin, quantum, cell, placement, reg=1024):
    """dict xyz, bgr, members, tri, triangle_of, vertex_of, stats -- or None where the call refuses"""
    xyz, tri = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), _tri(tri).tolist()
    if not valid_params(cell, placement, reg):
        return None
    nv = len(xyz)
    if any(not 0 <= v < nv for t in tri for v in t):
        return None
    P = []
    for row in xyz:
        p = [co.quantise_one(row[k], origin[k], quantum) for k in range(3)]
        if any(v is None for v in p):
            return None
        P.append(p)
    cells = {}                                                                          # key -> [c, members]
    rem, key = [], []
    for v, p in enumerate(P):
        c = [p[k] // cell for k in range(3)]
        rem.append([p[k] - c[k] * cell for k in range(3)])
        key.append(key_of(c))
        cells.setdefault(key[-1], [c, []])[1].append(v)
    quad = {k: [0] * 10 for k in cells}
    if placement == 1:
        for a, b, c in tri:
            if a == b or a == c or b == c:
                continue
            u = unit_normal(co.cross(P[a], P[b], P[c]))
            if u is None:
                continue
            for v in (a, b, c):
                q = quad[key[v]]
                for i, term in enumerate(quadric_terms(u, rem[v])):
                    q[i] += term
    order = sorted(cells)
    rank = {k: i for i, k in enumerate(order)}
    rep, colour, fallback = {}, {}, 0
    for k in order:
        c, mem = cells[k]
        n = len(mem)
        Sp = [sum(rem[v][a] for v in mem) for a in range(3)]
        R = [mean_round(Sp[a], n) for a in range(3)]
        if placement == 1:
            solved = solve_one(quad[k], Sp, n, reg, cell)
            if solved is None:
                fallback += 1
            else:
                R = solved
        rep[k] = [co.position_one(origin[a], c[a] * cell + R[a], quantum) for a in range(3)]
        if bgr is not None:
            colour[k] = [mean_round(sum(int(bgr[v][a]) for v in mem), n) for a in range(3)]
    seen, kept, collapsed, dups = set(), [], 0, 0
    for t, (a, b, c) in enumerate(tri):
        ka, kb, kc = key[a], key[b], key[c]
        if ka == kb or ka == kc or kb == kc:
            collapsed += 1
            continue
        triple = frozenset((ka, kb, kc))
        if triple in seen:
            dups += 1
            continue
        seen.add(triple)
        kept.append(t)
    used = sorted({key[v] for t in kept for v in tri[t]})
    new = {k: i for i, k in enumerate(used)}
    out = _empty(nv, bgr is not None)
    out["xyz"] = np.asarray([rep[k] for k in used], np.float32).reshape(-1, 3)
    if bgr is not None:
        out["bgr"] = np.asarray([colour[k] for k in used], np.uint8).reshape(-1, 3)
    out["members"] = np.asarray([len(cells[k][1]) for k in used], np.int32).reshape(-1)
    out["tri"] = np.asarray([[new[key[v]] for v in tri[t]] for t in kept], np.int32).reshape(-1, 3)
    out["triangle_of"] = np.asarray(kept, np.int32).reshape(-1)
    out["vertex_of"] = np.asarray([new.get(key[v], -1) for v in range(nv)], np.int32).reshape(nv)
    out["stats"] = [len(rank), collapsed, dups, fallback]
    return out


# ---- statement two: a stable sort, reduceat / add.at, arrays, a lexicographic sort ------------------------------------------------
def clusters_np(P, cell):
    """c, r int64 [n, 3], key uint64 [n], order (stable), run starts, cluster rank of every vertex"""
    c = P // cell
    r = P - c * cell
    key = ((c[:, 2] + BIAS).astype(np.uint64) << np.uint64(42)) | ((c[:, 1] + BIAS).astype(np.uint64) << np.uint64(21)) | (c[:, 0] + BIAS).astype(np.uint64)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.ones(len(ks), bool)
    head[1:] = ks[1:] != ks[:-1]
    start = np.nonzero(head)[0]
    cluster = np.zeros(len(P), np.int64)
    cluster[order] = np.cumsum(head) - 1
    return c, r, key, order, start, cluster


def quadrics_np(P, r, tri, cluster, n_clusters):
    """Q int64 [n_clusters, 10] and the per-triangle u (with the rows that contribute)"""
    t = co.distinct(tri).astype(np.int64)
    e, f = P[t[:, 1]] - P[t[:, 0]], P[t[:, 2]] - P[t[:, 0]]
    N = np.stack([e[:, 1] * f[:, 2] - e[:, 2] * f[:, 1], e[:, 2] * f[:, 0] - e[:, 0] * f[:, 2], e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0]], axis=1)
    n = N.astype(np.float64)
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    ok = length > 0
    t = t[ok]
    u = np.floor((n[ok] / length[ok, None]) * UNIT + 0.5).astype(np.int64)
    Q = np.zeros((n_clusters, 10), np.int64)
    for k in range(3):
        rv = r[t[:, k]]
        e_ = (u[:, 0] * rv[:, 0] + u[:, 1] * rv[:, 1]) + u[:, 2] * rv[:, 2]
        terms = np.stack([u[:, 0] * u[:, 0], u[:, 0] * u[:, 1], u[:, 0] * u[:, 2], u[:, 1] * u[:, 1], u[:, 1] * u[:, 2], u[:, 2] * u[:, 2],
                          u[:, 0] * e_, u[:, 1] * e_, u[:, 2] * e_, np.ones(len(t), np.int64)], axis=1)
        np.add.at(Q, cluster[t[:, k]], terms)
    return Q


def decimate_np(xyz, bgr, tri, origin, quantum, cell, placement, reg=1024, want_internals=False):
    xyz, tri = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), _tri(tri)
    if not valid_params(cell, placement, reg):
        return None
    nv = len(xyz)
    if len(tri) and (tri.min() < 0 or tri.max() >= nv):
        return None
    P = co.quantise_np(xyz, origin, quantum)
    if P is None:
        return None
    out = _empty(nv, bgr is not None)
    if nv == 0:
        out["stats"] = [0, 0, 0, 0]
        return out
    c, r, key, order, start, cluster = clusters_np(P, cell)
    nc = len(start)
    n = np.diff(np.append(start, nv)).astype(np.int64)
    Sp = np.add.reduceat(r[order], start, axis=0)
    R = (2 * Sp + n[:, None]) // (2 * n[:, None])
    fallback = 0
    Q = np.zeros((nc, 10), np.int64)
    if placement == 1:
        Q = quadrics_np(P, r, tri, cluster, nc)
        Rq, ok = solve_np(Q, Sp, n, reg, cell)
        fallback = int((~ok).sum())
        R = np.where(ok[:, None], Rq, R)
    cc = c[order][start]
    rep = co.positions_np(cc * cell + R, origin, quantum)
    colour = None
    if bgr is not None:
        Sb = np.add.reduceat(np.ascontiguousarray(bgr, np.uint8).reshape(-1, 3).astype(np.int64)[order], start, axis=0)
        colour = ((2 * Sb + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    ct = cluster[tri.astype(np.int64)].reshape(-1, 3)
    collapsed = (ct[:, 0] == ct[:, 1]) | (ct[:, 0] == ct[:, 2]) | (ct[:, 1] == ct[:, 2])
    live = np.nonzero(~collapsed)[0]
    srt = np.sort(ct[live], axis=1)
    o = np.lexsort((live, srt[:, 2], srt[:, 1], srt[:, 0]))                            # by lo, mid, hi, then the input index
    s = srt[o]
    first = np.ones(len(o), bool)
    first[1:] = (s[1:] != s[:-1]).any(axis=1)
    kept = np.sort(live[o[first]])
    used = np.zeros(nc, bool)
    used[ct[kept].reshape(-1)] = True
    new = np.cumsum(used) - 1
    out["xyz"] = rep[used]
    if bgr is not None:
        out["bgr"] = colour[used]
    out["members"] = n[used].astype(np.int32)
    out["tri"] = new[ct[kept]].astype(np.int32).reshape(-1, 3)
    out["triangle_of"] = kept.astype(np.int32)
    out["vertex_of"] = np.where(used[cluster], new[cluster], -1).astype(np.int32)
    out["stats"] = [int(nc), int(collapsed.sum()), int(len(live) - len(kept)), fallback]
    if want_internals:
        out["internals"] = dict(P=P, c=c, r=r, key=key, cluster=cluster, Sp=Sp, n=n, Q=Q, R=R, cell_of_cluster=cc)
    return out


# ---- measures of the tests (not part of the contract) -----------------------------------------------------------------------------
def edge_counts(tri):
    """(boundary edges, non-manifold edges, edges) of a triangle list"""
    tri = _tri(tri).astype(np.int64)
    if not len(tri):
        return 0, 0, 0
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    e.sort(axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return int((counts == 1).sum()), int((counts > 2).sum()), int(len(counts))


def euler(tri):
    tri = _tri(tri)
    return len(np.unique(tri)) - edge_counts(tri)[2] + len(tri)
