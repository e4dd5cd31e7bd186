"""CPU restatement of sfmba_mesh_components / sfmba_mesh_filter / sfmba_mesh_smooth / sfmba_mesh_clean (the contract is in
include/sfmba.h; csrc/mesh_clean_math.h is the arithmetic the kernels run) -- TEST INFRASTRUCTURE ONLY.

Every part is stated twice:
  * components: a union-find loop in plain Python (components_loop), and scipy.sparse.csgraph.connected_components where scipy is
    importable, otherwise a numpy fixed-point iteration of label = min over each triangle run to convergence (components_np);
  * filter: a loop over triangles and vertices (filter_loop), and boolean masks with cumsum (filter_np);
  * smoothing and normals: per-triangle loops in Python integers and floats (smooth_loop), and np.add.at / // on int64 arrays
    (smooth_np).
Python floats are IEEE doubles, math.sqrt and numpy's sqrt are correctly rounded and every operation below is written on its own,
so both statements, the header built for the host and the device agree BIT FOR BIT."""
import math

import numpy as np

MAX_P = 1 << 25
MAX_D = 1 << 17
UNIT = 1048576.0
L_RANGE, M_RANGE = (1, 65536), (-131072, -1)


def _tri(tri):
    return np.ascontiguousarray(tri, np.int32).reshape(-1, 3)


# ---- components ---------------------------------------------------------------------------------------------------------------
def _summary(nv, tri, label):
    comp = np.zeros(nv, np.int64)
    if len(tri):
        np.add.at(comp, label[tri[:, 0]], 1)
    owners = np.nonzero(comp)[0]
    largest = -1 if not len(owners) else int(owners[np.argmax(comp[owners])])          # argmax takes the first: ties to the lower label
    return dict(label=label.astype(np.int32), comp_triangles=comp[label].astype(np.int32) if nv else np.zeros(0, np.int32),
                n_components=int(len(owners)), largest=largest)


def components_loop(nv, tri):
    tri = _tri(tri)
    parent = list(range(nv))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for a, b, c in tri.tolist():
        for x, y in ((a, b), (a, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    label = [find(v) for v in range(nv)]
    count = [0] * nv
    for a, _, _ in tri.tolist():
        count[label[a]] += 1
    owners = [v for v in range(nv) if count[v] > 0]
    largest = -1
    for v in owners:
        if largest < 0 or count[v] > count[largest]:
            largest = v
    return dict(label=np.asarray(label, np.int32).reshape(nv), comp_triangles=np.asarray([count[l] for l in label], np.int32).reshape(nv),
                n_components=len(owners), largest=largest)


def _labels_scipy(nv, tri):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    rows = np.concatenate([tri[:, 0], tri[:, 0]])
    cols = np.concatenate([tri[:, 1], tri[:, 2]])
    g = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(nv, nv))
    _, comp = connected_components(g, directed=False)
    lowest = np.full(nv, nv, np.int64)
    np.minimum.at(lowest, comp, np.arange(nv))
    return lowest[comp]


def _labels_fixed_point(nv, tri):
    label = np.arange(nv, dtype=np.int64)
    while True:
        m = label[tri].min(axis=1)
        new = label.copy()
        for k in range(3):
            np.minimum.at(new, tri[:, k], m)
        new = new[new]
        if (new == label).all():
            return label
        label = new


def components_np(nv, tri, use_scipy=None):
    tri = _tri(tri)
    if use_scipy is None:
        try:
            import scipy.sparse.csgraph  # noqa: F401
            use_scipy = True
        except ImportError:
            use_scipy = False
    if nv == 0 or len(tri) == 0:
        label = np.arange(nv, dtype=np.int64)
    else:
        label = _labels_scipy(nv, tri) if use_scipy else _labels_fixed_point(nv, tri)
    return _summary(nv, tri, label)


# ---- filter -------------------------------------------------------------------------------------------------------------------
def filter_np(xyz, bgr, tri, min_triangles, keep_largest, comp=None):
    xyz, tri = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), _tri(tri)
    nv = len(xyz)
    c = comp or components_np(nv, tri)
    keep_comp = c["comp_triangles"] >= min_triangles                                   # per vertex: its component's verdict
    if keep_largest:
        keep_comp &= c["label"] == c["largest"]
    tkeep = keep_comp[tri[:, 0]] if len(tri) else np.zeros(0, bool)
    vkeep = np.zeros(nv, bool)
    vkeep[tri[tkeep].reshape(-1)] = True
    new = np.cumsum(vkeep) - 1
    vertex_of = np.where(vkeep, new, -1).astype(np.int32)
    return dict(xyz=xyz[vkeep].copy(), bgr=None if bgr is None else np.ascontiguousarray(bgr, np.uint8).reshape(-1, 3)[vkeep].copy(),
                tri=vertex_of[tri[tkeep]].astype(np.int32).reshape(-1, 3), vertex_of=vertex_of)


def filter_loop(xyz, bgr, tri, min_triangles, keep_largest):
    xyz, tri = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), _tri(tri)
    nv = len(xyz)
    c = components_loop(nv, tri)
    kept = []
    for t, (a, b, cc) in enumerate(tri.tolist()):
        root = int(c["label"][a])
        if int(c["comp_triangles"][a]) >= min_triangles and (not keep_largest or root == c["largest"]):
            kept.append(t)
    used = set()
    for t in kept:
        used.update(tri[t].tolist())
    vertex_of, order = [-1] * nv, []
    for v in range(nv):
        if v in used:
            vertex_of[v] = len(order)
            order.append(v)
    out_tri = [[vertex_of[v] for v in tri[t].tolist()] for t in kept]
    return dict(xyz=xyz[order].reshape(-1, 3).copy(), bgr=None if bgr is None else np.ascontiguousarray(bgr, np.uint8).reshape(-1, 3)[order].reshape(-1, 3).copy(),
                tri=np.asarray(out_tri, np.int32).reshape(-1, 3), vertex_of=np.asarray(vertex_of, np.int32).reshape(nv))


# ---- quantisation -------------------------------------------------------------------------------------------------------------
def factor(f, lo, hi):
    """F = floor((double)f 65536 + 0.5) if it lies in lo..hi, else None (a NaN gives None)"""
    r = float(np.float32(f)) * 65536.0
    r = r + 0.5
    if not math.isfinite(r):
        return None
    r = math.floor(r)
    return int(r) if lo <= r <= hi else None


def quantise_one(x, origin, quantum):
    """P of one coordinate or None (not finite, or |P| >= 2^25); x, origin, quantum are float32 values"""
    x, o, q = float(np.float32(x)), float(np.float32(origin)), float(np.float32(quantum))
    if not math.isfinite(x):
        return None
    r = x - o
    r = r / q
    r = r + 0.5
    if not math.isfinite(r):
        return None
    r = math.floor(r)
    return int(r) if -MAX_P < r < MAX_P else None


def quantise_np(xyz, origin, quantum):
    """int64 [n, 3] or None"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        r = xyz - np.asarray(origin, np.float32).astype(np.float64)[None, :]
        r = r / float(np.float32(quantum))
        r = np.floor(r + 0.5)
    if not (np.isfinite(r).all() and (np.abs(r) < MAX_P).all()):
        return None
    return r.astype(np.int64)


def position_one(origin, P, quantum):
    s = float(P) * float(np.float32(quantum))
    return np.float32(float(np.float32(origin)) + s)


def positions_np(P, origin, quantum):
    s = P.astype(np.float64) * float(np.float32(quantum))
    return (np.asarray(origin, np.float32).astype(np.float64)[None, :] + s).astype(np.float32)


def distinct(tri):
    tri = _tri(tri)
    return tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])]


# ---- one pass -----------------------------------------------------------------------------------------------------------------
def step(P, S, D, F):
    """one axis of one vertex in Python integers (floor division)"""
    n = F * (S - D * P)
    den = D * 65536
    return P + (2 * n + den) // (2 * den)


def pass_loop(P, tri, F):
    """P: list of [x, y, z] Python integers -> the new list"""
    nv = len(P)
    S = [[0, 0, 0] for _ in range(nv)]
    D = [0] * nv
    for a, b, c in tri:
        if a == b or a == c or b == c:
            continue
        for v, (p, q) in ((a, (b, c)), (b, (a, c)), (c, (a, b))):
            for k in range(3):
                S[v][k] += P[p][k] + P[q][k]
            D[v] += 2
    out = []
    for v in range(nv):
        if D[v] == 0 or D[v] > MAX_D:
            out.append(list(P[v]))
            continue
        Q = [step(P[v][k], S[v][k], D[v], F) for k in range(3)]
        out.append(Q if all(-MAX_P < x < MAX_P for x in Q) else list(P[v]))
    return out, D


def degrees_np(nv, tri):
    D = np.zeros(nv, np.int64)
    np.add.at(D, distinct(tri).reshape(-1), 2)
    return D


def pass_np(P, tri, F, D=None):
    t = distinct(tri)
    nv = len(P)
    D = degrees_np(nv, tri) if D is None else D
    S = np.zeros((nv, 3), np.int64)
    for v, p, q in ((0, 1, 2), (1, 0, 2), (2, 0, 1)):
        np.add.at(S, t[:, v], P[t[:, p]] + P[t[:, q]])
    moves = (D > 0) & (D <= MAX_D)
    Dm = np.where(moves, D, 1)[:, None]
    n = F * (S - Dm * P)
    den = Dm * 65536
    Q = P + (2 * n + den) // (2 * den)
    moves &= (np.abs(Q) < MAX_P).all(axis=1)
    return np.where(moves[:, None], Q, P)


# ---- normals ------------------------------------------------------------------------------------------------------------------
def cross(Pa, Pb, Pc):
    e = [Pb[k] - Pa[k] for k in range(3)]
    f = [Pc[k] - Pa[k] for k in range(3)]
    return [e[1] * f[2] - e[2] * f[1], e[2] * f[0] - e[0] * f[2], e[0] * f[1] - e[1] * f[0]]


def unit_normal(N):
    """u [3] Python integers, or None when the triangle has no area"""
    n = [float(v) for v in N]
    length = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    if length == 0.0:
        return None
    return [int(math.floor((v / length) * UNIT + 0.5)) for v in n]


def vertex_normal(U):
    if U[0] == 0 and U[1] == 0 and U[2] == 0:
        return [np.float32(0.0)] * 3
    n = [float(v) for v in U]
    length = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    return [np.float32(v / length) for v in n]


def normals_loop(P, tri):
    U = [[0, 0, 0] for _ in range(len(P))]
    for a, b, c in tri:
        if a == b or a == c or b == c:
            continue
        u = unit_normal(cross(P[a], P[b], P[c]))
        if u is None:
            continue
        for v in (a, b, c):
            for k in range(3):
                U[v][k] += u[k]
    return np.asarray([vertex_normal(u) for u in U], np.float32).reshape(len(P), 3)


def normals_np(P, tri):
    t = distinct(tri)
    e, f = P[t[:, 1]] - P[t[:, 0]], P[t[:, 2]] - P[t[:, 0]]
    N = np.stack([e[:, 1] * f[:, 2] - e[:, 2] * f[:, 1], e[:, 2] * f[:, 0] - e[:, 0] * f[:, 2], e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0]], axis=1)
    n = N.astype(np.float64)
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    ok = length > 0
    u = np.floor((n[ok] / length[ok, None]) * UNIT + 0.5).astype(np.int64)
    U = np.zeros((len(P), 3), np.int64)
    for k in range(3):
        np.add.at(U, t[ok, k], u)
    Uf = U.astype(np.float64)
    ulen = np.sqrt((Uf[:, 0] * Uf[:, 0] + Uf[:, 1] * Uf[:, 1]) + Uf[:, 2] * Uf[:, 2])
    out = np.zeros((len(P), 3), np.float32)
    nz = U.any(axis=1)
    out[nz] = (Uf[nz] / ulen[nz, None]).astype(np.float32)
    return out


# ---- the calls ----------------------------------------------------------------------------------------------------------------
def smooth_np(xyz, tri, origin, quantum, iterations, lam, mu, want_P=False):
    """dict xyz, normal (and P, the final integer positions), or None where the call refuses"""
    xyz, tri = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), _tri(tri)
    L, M = factor(lam, *L_RANGE), factor(mu, *M_RANGE)
    if L is None or M is None or not 0 <= iterations <= 100:
        return None
    P = quantise_np(xyz, origin, quantum)
    if P is None:
        return None
    D = degrees_np(len(xyz), tri)
    for _ in range(iterations):
        P = pass_np(P, tri, L, D)
        P = pass_np(P, tri, M, D)
    out = dict(xyz=positions_np(P, origin, quantum) if iterations else xyz.copy(), normal=normals_np(P, tri))
    if want_P:
        out["P"] = P
    return out


def smooth_loop(xyz, tri, origin, quantum, iterations, lam, mu):
    xyz, tri = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), _tri(tri).tolist()
    L, M = factor(lam, *L_RANGE), factor(mu, *M_RANGE)
    if L is None or M is None or not 0 <= iterations <= 100:
        return None
    P = []
    for row in xyz:
        p = [quantise_one(row[k], origin[k], quantum) for k in range(3)]
        if any(v is None for v in p):
            return None
        P.append(p)
    for _ in range(iterations):
        P, _ = pass_loop(P, tri, L)
        P, _ = pass_loop(P, tri, M)
    if iterations:
        out = np.asarray([[position_one(origin[k], p[k], quantum) for k in range(3)] for p in P], np.float32).reshape(len(P), 3)
    else:
        out = xyz.copy()
    return dict(xyz=out, normal=normals_loop(P, tri))


def clean(xyz, bgr, tri, origin, quantum, min_triangles, keep_largest, iterations, lam, mu, filter_fn=filter_np, smooth_fn=smooth_np):
    """filter, then smooth: dict xyz, bgr, normal, tri, vertex_of, or None where the smoothing refuses"""
    f = filter_fn(xyz, bgr, tri, min_triangles, keep_largest)
    s = smooth_fn(f["xyz"], f["tri"], origin, quantum, iterations, lam, mu)
    if s is None:
        return None
    return dict(xyz=s["xyz"], bgr=f["bgr"], normal=s["normal"], tri=f["tri"], vertex_of=f["vertex_of"])
