"""CPU restatement of sfmba_tsdf_fill (the contract is in include/sfmba.h) -- TEST INFRASTRUCTURE ONLY.  The rule is stated twice:

  fill_loop    a Python loop per vertex and pass in Python integers (floor_div is Python's //);
  fill_numpy   numpy over shifted copies of the whole grid.

Both return the dict sum, weight int32 [nz, ny, nx]; csum int32 [nz, ny, nx, 3] and cweight int32 [nz, ny, nx] or None; state uint8
[nz, ny, nx]; n_filled.  vfilled(vkey, state) restates the per-vertex flag of sfmba_tsdf_mesh_fill.

Nothing here is imported by the product."""
import numpy as np

UNKNOWN = 255


def fill_weight(min_weight):
    return 64 * ((min_weight + 63) // 64)


# ---- stated once per vertex ---------------------------------------------------------------------------------------------------
def fill_loop(S, W, CS, CW, min_weight, iterations, min_neighbours):
    nz, ny, nx = S.shape
    colour = CS is not None
    n_vox = nx * ny * nz
    s, w = [int(v) for v in S.reshape(-1)], [int(v) for v in W.reshape(-1)]
    cs = [[int(v) for v in row] for row in CS.reshape(-1, 3)] if colour else None
    cw = [int(v) for v in CW.reshape(-1)] if colour else None
    # the working state: (known, V, state, hasC, c)
    cur = []
    for l in range(n_vox):
        if w[l] >= min_weight:
            V = (128 * s[l] + w[l]) // (2 * w[l])
            has_c = colour and cw[l] > 0
            c = tuple((2 * cs[l][a] + cw[l]) // (2 * cw[l]) for a in range(3)) if has_c else (0, 0, 0)
            cur.append((True, V, 0, has_c, c))
        else:
            cur.append((False, 0, UNKNOWN, False, (0, 0, 0)))
    for p in range(1, iterations + 1):
        nxt = list(cur)
        for l in range(n_vox):
            known, V, st, has_c, c = cur[l]
            if st == 0:
                continue
            i, j, k = l % nx, l // nx % ny, l // (nx * ny)
            at = []
            if i > 0:
                at.append(l - 1)
            if i < nx - 1:
                at.append(l + 1)
            if j > 0:
                at.append(l - nx)
            if j < ny - 1:
                at.append(l + nx)
            if k > 0:
                at.append(l - nx * ny)
            if k < nz - 1:
                at.append(l + nx * ny)
            terms = [cur[q] for q in at if cur[q][0]]
            if not known and len(terms) < min_neighbours:
                continue
            if known:
                terms.append(cur[l])
            n = len(terms)
            V2 = (2 * sum(t[1] for t in terms) + n) // (2 * n)
            col = [t[4] for t in terms if t[3]]
            m = len(col)
            c2 = tuple((2 * sum(q[a] for q in col) + m) // (2 * m) for a in range(3)) if m else (0, 0, 0)
            nxt[l] = (True, V2, st if known else p, m > 0, c2)
        cur = nxt
    FW = fill_weight(min_weight)
    out_s, out_w = np.array(S, np.int32).reshape(-1), np.array(W, np.int32).reshape(-1)
    out_cs = np.array(CS, np.int32).reshape(-1, 3) if colour else None
    out_cw = np.array(CW, np.int32).reshape(-1) if colour else None
    state = np.zeros(n_vox, np.uint8)
    filled = 0
    for l in range(n_vox):
        known, V, st, has_c, c = cur[l]
        state[l] = st
        if 1 <= st <= 254:
            filled += 1
            out_s[l], out_w[l] = V * (FW // 64), FW
            if colour:
                out_cs[l] = c if has_c else (0, 0, 0)
                out_cw[l] = 1 if has_c else 0
    return {"sum": out_s.reshape(S.shape), "weight": out_w.reshape(S.shape), "csum": out_cs.reshape(S.shape + (3,)) if colour else None,
            "cweight": out_cw.reshape(S.shape) if colour else None, "state": state.reshape(S.shape), "n_filled": filled}


# ---- stated over shifted copies of the grid ---------------------------------------------------------------------------------------
def _neighbour_sums(a):
    """the sum of `a` over the six face neighbours that exist; a is [nz, ny, nx] or [nz, ny, nx, 3]"""
    p = np.pad(a, [(1, 1)] * 3 + [(0, 0)] * (a.ndim - 3))
    nz, ny, nx = a.shape[:3]
    c = (slice(1, nz + 1), slice(1, ny + 1), slice(1, nx + 1))
    out = np.zeros_like(a)
    for axis in range(3):
        for d in (-1, 1):
            sl = list(c)
            sl[axis] = slice(1 + d, a.shape[axis] + 1 + d)
            out = out + p[tuple(sl)]
    return out


def fill_numpy(S, W, CS, CW, min_weight, iterations, min_neighbours):
    colour = CS is not None
    S64, W64 = S.astype(np.int64), W.astype(np.int64)
    obs = W64 >= min_weight
    V = np.where(obs, (128 * S64 + W64) // np.maximum(2 * W64, 1), 0)
    if colour:
        CW64 = CW.astype(np.int64)
        has_c = obs & (CW64 > 0)
        c = np.where(has_c[..., None], (2 * CS.astype(np.int64) + CW64[..., None]) // np.maximum(2 * CW64, 1)[..., None], 0)
    else:
        has_c, c = np.zeros(S.shape, bool), np.zeros(S.shape + (3,), np.int64)
    known = obs.copy()
    state = np.where(obs, 0, UNKNOWN).astype(np.int64)
    for p in range(1, iterations + 1):
        k64, hc64 = known.astype(np.int64), (known & has_c).astype(np.int64)
        n6 = _neighbour_sums(k64)
        was = known & ~obs
        upd = was | (~known & (n6 >= min_neighbours))
        n = n6 + was
        sv = _neighbour_sums(V * k64) + np.where(was, V, 0)
        m = _neighbour_sums(hc64) + (was & has_c)
        sc = _neighbour_sums(c * hc64[..., None]) + np.where((was & has_c)[..., None], c, 0)
        V2 = (2 * sv + n) // np.maximum(2 * n, 1)
        c2 = np.where((m > 0)[..., None], (2 * sc + m[..., None]) // np.maximum(2 * m, 1)[..., None], 0)
        V = np.where(upd, V2, V)
        c = np.where(upd[..., None], c2, c)
        has_c = np.where(upd, m > 0, has_c)
        state = np.where(upd & ~known, p, state)
        known = known | upd
    FW = fill_weight(min_weight)
    filled = (state >= 1) & (state <= 254)
    i32 = lambda a: np.ascontiguousarray(a.astype(np.int32))
    out = {"sum": i32(np.where(filled, V * (FW // 64), S64)), "weight": i32(np.where(filled, FW, W64)), "csum": None, "cweight": None,
           "state": np.ascontiguousarray(state.astype(np.uint8)), "n_filled": int(filled.sum())}
    if colour:
        out["csum"] = i32(np.where(filled[..., None], np.where(has_c[..., None], c, 0), CS.astype(np.int64)))
        out["cweight"] = i32(np.where(filled, has_c.astype(np.int64), CW.astype(np.int64)))
    return out


GRID_FIELDS = ("sum", "weight", "csum", "cweight", "state")


def same(a, b):
    """the first field in which two results differ, or None"""
    for f in GRID_FIELDS:
        if (a[f] is None) != (b[f] is None) or (a[f] is not None and (a[f].dtype != b[f].dtype or not np.array_equal(a[f], b[f]))):
            return f
    return None if a["n_filled"] == b["n_filled"] else "n_filled"


def vfilled(vkey, state):
    """per mesh vertex 1 iff either end of its edge is a filled grid vertex"""
    nz, ny, nx = state.shape
    st = state.reshape(-1).astype(np.int64)
    vkey = np.asarray(vkey, np.int64)
    lin, d = vkey >> 3, (vkey & 7) + 1
    at = lin + (d & 1) + (d >> 1 & 1) * nx + (d >> 2 & 1) * nx * ny
    made = (st >= 1) & (st <= 254)
    return (made[lin] | made[at]).astype(np.uint8)


def observed_within(state, p_max):
    """per vertex the L1 distance to the nearest observed vertex, capped at p_max + 1 (a breadth-first sweep over face neighbours)"""
    dist = np.where(state == 0, 0, p_max + 1).astype(np.int64)
    for _ in range(p_max):
        pad = np.pad(dist, 1, constant_values=p_max + 1)
        nz, ny, nx = dist.shape
        best = dist
        for axis in range(3):
            for d in (-1, 1):
                sl = [slice(1, nz + 1), slice(1, ny + 1), slice(1, nx + 1)]
                sl[axis] = slice(1 + d, dist.shape[axis] + 1 + d)
                best = np.minimum(best, pad[tuple(sl)] + 1)
        dist = best
    return dist
