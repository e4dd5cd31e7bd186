"""CPU restatement of sfmba_tsdf_integrate / sfmba_tsdf_extract / sfmba_tsdf_mesh (the contract is in include/sfmba.h) -- TEST
INFRASTRUCTURE ONLY.  Each half is stated twice:

  integration   integrate_loop: a Python loop per voxel and image with Python floats (IEEE doubles, every operation rounded on its
                own) and Python integers; integrate_maps: numpy over the whole grid, image by image.
  extraction    extract_geometric: per active cell and tetrahedron the geometric rule of the contract in Python integers (the inside
                and outside vertices, the edges, the orientation from the doubled midpoints, the rotation by key), vertices from a
                dict of keys; extract_table: the 6 x 16 case table (TABLE below, built once from the same rule and held equal to the
                constants of csrc/mesh_math.h by tests/test_mesh_oracle_cpu.py), numpy over all cells, a sort-unique of the keys.

Nothing here is imported by the product."""
import math

import numpy as np

QUANTA = 1024
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
NO_EDGE = 255


def f32(v):
    return float(np.float32(v))


# ---- the grid ---------------------------------------------------------------------------------------------------------------
def lin(i, j, k, nx, ny):
    return (k * ny + j) * nx + i


def grid_coord(origin_a, i_a, voxel):
    return f32(origin_a) + (float(i_a) * f32(voxel))


# ---- integration, stated once per voxel and image ---------------------------------------------------------------------------------
def project(k4, P, X):
    """(q, px, py) of world point X in the image with pose P [12] (Python floats); px = py = None unless q_2 > 0.  px and py are the
    rounded pixel as Python floats (they may lie outside any image, or be infinite or NaN)."""
    q = [((P[4 * i] * X[0] + P[4 * i + 1] * X[1]) + P[4 * i + 2] * X[2]) + P[4 * i + 3] for i in range(3)]
    if not q[2] > 0.0:
        return q, None, None
    out = []
    for f, c, v in ((k4[0], k4[2], q[0]), (k4[1], k4[3], q[1])):
        s = ((f * v) / q[2] + c) + 0.5
        out.append(float(math.floor(s)) if math.isfinite(s) else s)
    return q, out[0], out[1]


def quantum(sdf, T):
    return int(math.floor((min(sdf, T) / T) * 1024.0 + 0.5))


def observe(k4, P, X, depth, T):
    """None, or (e, with_colour, py, px): what the image with pose P and depth map `depth` adds to the voxel at X."""
    h, w = depth.shape
    q, x, y = project(k4, P, X)
    if x is None or not (0.0 <= x <= float(w - 1) and 0.0 <= y <= float(h - 1)):
        return None
    px, py = int(x), int(y)
    zs = float(depth[py, px])
    if not zs > 0.0:
        return None
    sdf = zs - q[2]
    if not sdf >= -T:
        return None
    return quantum(sdf, T), sdf <= T, py, px


def as_k4(K):
    K = np.asarray(K, np.float32).reshape(3, 3)
    return [float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])]


def integrate_loop(images, K, P, depth_maps, origin, voxel, dims, trunc):
    nx, ny, nz = dims
    k4, T = as_k4(K), f32(trunc)
    Ps = [[float(v) for v in np.asarray(p, np.float32).reshape(12)] for p in P]
    S, W = np.zeros((nz, ny, nx), np.int32), np.zeros((nz, ny, nx), np.int32)
    CS, CW = np.zeros((nz, ny, nx, 3), np.int32), np.zeros((nz, ny, nx), np.int32)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                X = [grid_coord(origin[0], i, voxel), grid_coord(origin[1], j, voxel), grid_coord(origin[2], k, voxel)]
                s = w = cw = 0
                cs = [0, 0, 0]
                for n, m in enumerate(depth_maps):
                    if m is None:
                        continue
                    o = observe(k4, Ps[n], X, m, T)
                    if o is None:
                        continue
                    s += o[0]
                    w += 1
                    if o[1] and images is not None:
                        px = images[n][o[2], o[3]]
                        for c in range(3):
                            cs[c] += int(px[c]) if np.ndim(px) else int(px)
                        cw += 1
                S[k, j, i], W[k, j, i], CW[k, j, i] = s, w, cw
                CS[k, j, i] = cs
    return {"sum": S, "weight": W, "csum": CS if images is not None else None, "cweight": CW if images is not None else None}


# ---- integration, stated over whole maps ------------------------------------------------------------------------------------------
def integrate_maps(images, K, P, depth_maps, origin, voxel, dims, trunc):
    nx, ny, nz = dims
    k4, T = as_k4(K), f32(trunc)
    vox = f32(voxel)
    gx = f32(origin[0]) + np.arange(nx, dtype=np.float64) * vox
    gy = f32(origin[1]) + np.arange(ny, dtype=np.float64) * vox
    gz = f32(origin[2]) + np.arange(nz, dtype=np.float64) * vox
    X2, X1, X0 = np.meshgrid(gz, gy, gx, indexing="ij")
    S, W = np.zeros((nz, ny, nx), np.int64), np.zeros((nz, ny, nx), np.int64)
    CS, CW = np.zeros((nz, ny, nx, 3), np.int64), np.zeros((nz, ny, nx), np.int64)
    with np.errstate(all="ignore"):
        for n, m in enumerate(depth_maps):
            if m is None:
                continue
            m = np.asarray(m, np.float32)
            h, w = m.shape
            p = np.asarray(P[n], np.float32).reshape(12).astype(np.float64)
            q = [((p[4 * i] * X0 + p[4 * i + 1] * X1) + p[4 * i + 2] * X2) + p[4 * i + 3] for i in range(3)]
            x = np.floor(((k4[0] * q[0]) / q[2] + k4[2]) + 0.5)
            y = np.floor(((k4[1] * q[1]) / q[2] + k4[3]) + 0.5)
            ok = (q[2] > 0.0) & (x >= 0.0) & (x <= float(w - 1)) & (y >= 0.0) & (y <= float(h - 1))
            px, py = np.where(ok, x, 0.0).astype(np.int64), np.where(ok, y, 0.0).astype(np.int64)
            zs = m[py, px].astype(np.float64)
            sdf = zs - q[2]
            ok = ok & (zs > 0.0) & (sdf >= -T)
            e = np.floor((np.minimum(np.where(ok, sdf, 0.0), T) / T) * 1024.0 + 0.5).astype(np.int64)
            S += np.where(ok, e, 0)
            W += ok
            if images is not None:
                col = ok & (sdf <= T)
                im = np.asarray(images[n])
                rgb = im[py, px].astype(np.int64)
                if rgb.ndim == 3:
                    rgb = np.repeat(rgb[..., None], 3, axis=-1)
                CS += np.where(col[..., None], rgb, 0)
                CW += col
    i32 = lambda a: a.astype(np.int32)
    return {"sum": i32(S), "weight": i32(W), "csum": i32(CS) if images is not None else None, "cweight": i32(CW) if images is not None else None}


# ---- extraction: the geometric rule ------------------------------------------------------------------------------------------------
def tet_vertices(p):
    a, b, _ = PERMS[p]
    v1 = [0, 0, 0]
    v1[a] = 1
    v2 = list(v1)
    v2[b] = 1
    return [(0, 0, 0), tuple(v1), tuple(v2), (1, 1, 1)]


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def tet_triangles(p, mask, key_of):
    """The triangles of tetrahedron p whose local vertex l is inside iff bit l of mask is set: a list of triples of local vertex pairs
    (lo, hi), oriented and rotated.  key_of(lo, hi) gives the key of the edge between the local vertices lo < hi."""
    v = tet_vertices(p)
    I = [l for l in range(4) if mask >> l & 1]
    O = [l for l in range(4) if not mask >> l & 1]
    if not I or not O:
        return []
    if len(I) == 1:
        tris = [[(I[0], O[0]), (I[0], O[1]), (I[0], O[2])]]
    elif len(I) == 3:
        tris = [[(I[0], O[0]), (I[1], O[0]), (I[2], O[0])]]
    else:
        c = [(I[0], O[0]), (I[0], O[1]), (I[1], O[1]), (I[1], O[0])]
        tris = [[c[0], c[1], c[2]], [c[0], c[2], c[3]]]
    d = tuple(len(I) * sum(v[o][a] for o in O) - len(O) * sum(v[i][a] for i in I) for a in range(3))
    out = []
    for tri in tris:
        m = [tuple(v[x][a] + v[y][a] for a in range(3)) for x, y in tri]
        n = cross(tuple(m[1][a] - m[0][a] for a in range(3)), tuple(m[2][a] - m[0][a] for a in range(3)))
        dot = sum(n[a] * d[a] for a in range(3))
        assert dot != 0
        e = [(min(x, y), max(x, y)) for x, y in tri]
        if dot < 0:
            e = [e[0], e[2], e[1]]
        keys = [key_of(*x) for x in e]
        r = keys.index(min(keys))
        out.append(e[r:] + e[:r])
    return out


def local_edge(p, lo, hi):
    """The edge between local vertices lo < hi of tetrahedron p as corner (0..7, x + 2 y + 4 z of its lower end) * 8 + code."""
    v = tet_vertices(p)
    A, d = v[lo], tuple(v[hi][a] - v[lo][a] for a in range(3))
    return (A[0] + 2 * A[1] + 4 * A[2]) * 8 + (d[0] + 2 * d[1] + 4 * d[2] - 1)


def build_table():
    """[6][16] rows (n, e0 .. e5): n triangles over local edges; NO_EDGE pads.  Inside one cell the order of the keys is the order of
    the local edges for every nx, ny >= 2: lin grows with x + nx y + nx ny z, which orders the eight corners as x + 2 y + 4 z does."""
    rows = []
    for p in range(6):
        for mask in range(16):
            tris = tet_triangles(p, mask, lambda lo, hi: local_edge(p, lo, hi))
            e = [local_edge(p, lo, hi) for t in tris for lo, hi in t]
            rows.append([len(tris)] + e + [NO_EDGE] * (6 - len(e)))
    return np.asarray(rows, np.int32).reshape(6, 16, 7)


TABLE = build_table()
# corner bit (x + 2 y + 4 z) of the four local vertices of every tetrahedron
TET_CORNERS = np.asarray([[v[0] + 2 * v[1] + 4 * v[2] for v in tet_vertices(p)] for p in range(6)], np.int32)


def vertex(A, code, origin, voxel, S, W, CS, CW):
    """(xyz float32 [3], bgr [3] or None) of the vertex on the edge from grid vertex A = (i, j, k) along code."""
    d = ((code + 1) & 1, (code + 1) >> 1 & 1, (code + 1) >> 2 & 1)
    a, b = (A[2], A[1], A[0]), (A[2] + d[2], A[1] + d[1], A[0] + d[0])
    fA, fB = float(S[a]) / float(W[a]), float(S[b]) / float(W[b])
    t = fA / (fA - fB)
    pos = [np.float32(f32(origin[c]) + ((float(A[c]) + (t * float(d[c]))) * f32(voxel))) for c in range(3)]
    col = None
    if CS is not None:
        w = int(CW[a]) + int(CW[b])
        col = [(2 * (int(CS[a][c]) + int(CS[b][c])) + w) // (2 * w) if w else 0 for c in range(3)]
    return pos, col


def check_grid(S, W, CS, CW):
    """False where sfmba_tsdf_extract refuses the grid."""
    S, W = S.astype(np.int64), W.astype(np.int64)
    if (W < 0).any() or (np.abs(S) > 1024 * W).any():
        return False
    if CS is not None:
        CS, CW = CS.astype(np.int64), CW.astype(np.int64)
        if (CW < 0).any() or (CS < 0).any() or (CS > 255 * CW[..., None]).any():
            return False
    return True


def finish(tris, origin, voxel, S, W, CS, CW, nx, ny):
    vkey = np.asarray(sorted(set(k for t in tris for k in t)), np.int64)
    xyz = np.zeros((len(vkey), 3), np.float32)
    bgr = np.zeros((len(vkey), 3), np.uint8) if CS is not None else None
    for r, key in enumerate(vkey):
        l, code = divmod(int(key), 8)
        A = (l % nx, l // nx % ny, l // (nx * ny))
        pos, col = vertex(A, code, origin, voxel, S, W, CS, CW)
        xyz[r] = pos
        if bgr is not None:
            bgr[r] = col
    tri = np.searchsorted(vkey, np.asarray(tris, np.int64).reshape(-1, 3)).astype(np.int32)
    return {"xyz": xyz, "bgr": bgr, "vkey": vkey.astype(np.int32), "tri": tri}


def extract_geometric(origin, voxel, S, W, CS, CW, min_weight):
    nz, ny, nx = S.shape
    tris = []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                if not all(W[k + c, j + b, i + a] >= min_weight for a in (0, 1) for b in (0, 1) for c in (0, 1)):
                    continue
                for p in range(6):
                    v = tet_vertices(p)
                    mask = sum(1 << l for l in range(4) if S[k + v[l][2], j + v[l][1], i + v[l][0]] < 0)

                    def key_of(lo, hi):
                        A, d = v[lo], tuple(v[hi][a] - v[lo][a] for a in range(3))
                        return lin(i + A[0], j + A[1], k + A[2], nx, ny) * 8 + (d[0] + 2 * d[1] + 4 * d[2] - 1)
                    for t in tet_triangles(p, mask, key_of):
                        tris.append([key_of(lo, hi) for lo, hi in t])
    return finish(tris, origin, voxel, S, W, CS, CW, nx, ny)


# ---- extraction: the case table, all cells at once -----------------------------------------------------------------------------------
def corner_bits(flag):
    """per cell [nz-1, ny-1, nx-1] the flags of its eight corners, bit x + 2 y + 4 z (every dimension >= 2)"""
    nz, ny, nx = flag.shape
    bits = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        a, b, cz = c & 1, c >> 1 & 1, c >> 2 & 1
        bits |= flag[cz:nz - 1 + cz, b:ny - 1 + b, a:nx - 1 + a].astype(np.int64) << c
    return bits


def active_cells(W, min_weight):
    return corner_bits(W >= min_weight) == 255



def extract_table(origin, voxel, S, W, CS, CW, min_weight):
    nz, ny, nx = S.shape
    if min(nx, ny, nz) < 2:
        return finish([], origin, voxel, S, W, CS, CW, nx, ny)
    active, bits = active_cells(W, min_weight), corner_bits(S < 0)
    kk, jj, ii = np.nonzero(active)                                   # ascending lin of the corner
    base = (kk * ny + jj) * nx + ii
    cell_bits = bits[kk, jj, ii]
    corner_lin = np.asarray([(c & 1) + (c >> 1 & 1) * nx + (c >> 2 & 1) * nx * ny for c in range(8)], np.int64)
    rows = []                                                         # (cell order, p, triangle) -> keys
    for p in range(6):
        mask = np.zeros(len(base), np.int64)
        for l in range(4):
            mask |= (cell_bits >> TET_CORNERS[p, l] & 1) << l
        row = TABLE[p][mask]                                          # [cells, 7]
        for t in range(2):
            has = row[:, 0] > t
            e = row[:, 1 + 3 * t:4 + 3 * t].astype(np.int64)
            keys = (base[:, None] + corner_lin[np.where(has[:, None], e >> 3, 0)]) * 8 + (e & 7)
            rows.append((np.nonzero(has)[0], np.full(int(has.sum()), 2 * p + t), keys[has]))
    cell = np.concatenate([r[0] for r in rows])
    slot = np.concatenate([r[1] for r in rows])
    keys = np.concatenate([r[2] for r in rows]).reshape(-1, 3)
    order = np.lexsort((slot, cell))
    keys = keys[order]
    vkey = np.unique(keys)
    out = finish([], origin, voxel, S, W, CS, CW, nx, ny)
    l, code = vkey // 8, vkey % 8 + 1
    A = np.stack([l % nx, l // nx % ny, l // (nx * ny)], -1)
    d = np.stack([code & 1, code >> 1 & 1, code >> 2 & 1], -1)
    B = A + d
    ia, ib = (A[:, 2], A[:, 1], A[:, 0]), (B[:, 2], B[:, 1], B[:, 0])
    with np.errstate(all="ignore"):
        fA, fB = S[ia].astype(np.float64) / W[ia].astype(np.float64), S[ib].astype(np.float64) / W[ib].astype(np.float64)
        t = fA / (fA - fB)
        o = np.asarray([f32(v) for v in origin], np.float64)
        out["xyz"] = (o[None] + ((A.astype(np.float64) + (t[:, None] * d.astype(np.float64))) * f32(voxel))).astype(np.float32)
    if CS is not None:
        w = (CW[ia].astype(np.int64) + CW[ib].astype(np.int64))[:, None]
        s = CS[ia].astype(np.int64) + CS[ib].astype(np.int64)
        out["bgr"] = np.where(w > 0, (2 * s + w) // np.maximum(2 * w, 1), 0).astype(np.uint8)
    out["vkey"] = vkey.astype(np.int32)
    out["tri"] = np.searchsorted(vkey, keys).astype(np.int32).reshape(-1, 3)
    return out


MESH_FIELDS = ("xyz", "bgr", "vkey", "tri")


# ---- what the tests ask of a mesh ------------------------------------------------------------------------------------------------------
def topology(tri):
    """(closed, euler, boundary_edges, n_edges): closed iff every directed edge occurs once and its reverse once."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    directed = {}
    for a, b, c in tri.tolist():
        for e in ((a, b), (b, c), (c, a)):
            directed[e] = directed.get(e, 0) + 1
    undirected = {}
    for (a, b), n in directed.items():
        k = (min(a, b), max(a, b))
        undirected[k] = undirected.get(k, 0) + n
    closed = all(n == 1 and directed.get((b, a), 0) == 1 for (a, b), n in directed.items())
    boundary = sum(1 for n in undirected.values() if n == 1)
    n_vert = len(np.unique(tri))
    return closed, n_vert - len(undirected) + len(tri), boundary, len(undirected)


def signed_volume(xyz, tri):
    p = np.asarray(xyz, np.float64)[np.asarray(tri, np.int64).reshape(-1, 3)]
    return float(np.einsum("ni,ni->n", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
