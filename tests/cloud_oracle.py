"""CPU restatement of sfmba_depth_normals and sfmba_cloud_merge (the contract is in include/sfmba.h) -- TEST INFRASTRUCTURE ONLY.

Each call is stated twice, by two routes that share no code beyond the scalar rounding rules:
  * merge_loop      a Python dict over the points, Python integers for the sums;
    merge_sorted    numpy: vectorised quantisation, a stable argsort of the keys, np.add.reduceat over the runs;
  * normals_loop    one pixel at a time in Python floats;
    normals_shifted shifted copies of the back-projected map with masks.
Python floats and numpy float64 are IEEE doubles with every operation rounded on its own, which is what the contract asks for."""
import math

import numpy as np

Q_LIMIT = 1 << 30
BIAS = 1 << 20
N_LIMIT = 1 << 20
SKIPPED = (1 << 64) - 1


# ---- merge: scalars ---------------------------------------------------------------------------------------------------------------
def quantise(x, voxel):
    """x, voxel: Python floats holding float32 values.  Returns q (int) or None when the axis is skipped."""
    with np.errstate(all="ignore"):
        r = np.floor(np.float64(x) / np.float64(voxel) * np.float64(1024.0) + np.float64(0.5))
    if not math.isfinite(x) or not (r >= -Q_LIMIT and r < Q_LIMIT):
        return None
    return int(r)


def key_of(q):
    return (((q[0] >> 10) + BIAS) << 42) | (((q[1] >> 10) + BIAS) << 21) | ((q[2] >> 10) + BIAS)


def normal_quantum(n):
    r = math.floor(float(n) * 16384.0 + 0.5) if math.isfinite(n) else (0 if math.isnan(n) else math.copysign(float(2 * N_LIMIT), n))
    return int(min(max(r, -N_LIMIT), N_LIMIT))


def final_coord(Sq, c, voxel):
    return np.float32(((float(Sq) / float(c)) / 1024.0) * voxel)


def final_colour(S, c):
    return (2 * S + c) // (2 * c)


def final_normal(Sm):
    a, b, c = float(Sm[0]), float(Sm[1]), float(Sm[2])
    L = math.sqrt((a * a + b * b) + c * c)
    if L == 0.0:
        return [np.float32(0.0)] * 3
    return [np.float32(a / L), np.float32(b / L), np.float32(c / L)]


def _pack(rows, n, voxel_of, n_skipped, have_bgr, have_normal):
    m = len(rows)
    out = dict(xyz=np.zeros((m, 3), np.float32), count=np.zeros(m, np.int32), first=np.zeros(m, np.int32), key=np.zeros(m, np.uint64),
               voxel_of=np.asarray(voxel_of, np.int32).reshape(n), n_skipped=int(n_skipped),
               bgr=np.zeros((m, 3), np.uint8) if have_bgr else None, normal=np.zeros((m, 3), np.float32) if have_normal else None)
    for o, (key, xyz, bgr, nrm, c, first) in enumerate(rows):
        out["key"][o], out["xyz"][o], out["count"][o], out["first"][o] = key, xyz, c, first
        if have_bgr:
            out["bgr"][o] = bgr
        if have_normal:
            out["normal"][o] = nrm
    return out


def merge_loop(xyz, bgr, normal, voxel, min_count):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n, vox = len(xyz), float(np.float32(voxel))
    table, key_of_point, n_skipped = {}, [None] * n, 0
    for i in range(n):
        q = [quantise(float(xyz[i, a]), vox) for a in range(3)]
        if None in q:
            n_skipped += 1
            continue
        k = key_of(q)
        key_of_point[i] = k
        e = table.setdefault(k, dict(c=0, q=[0, 0, 0], b=[0, 0, 0], m=[0, 0, 0], first=i))
        e["c"] += 1
        e["first"] = min(e["first"], i)
        for a in range(3):
            e["q"][a] += q[a]
            if bgr is not None:
                e["b"][a] += int(bgr[i][a])
            if normal is not None:
                e["m"][a] += normal_quantum(float(normal[i][a]))
    rows, index = [], {}
    for k in sorted(table):
        e = table[k]
        if e["c"] < min_count:
            continue
        index[k] = len(rows)
        rows.append((k, [final_coord(e["q"][a], e["c"], vox) for a in range(3)], [final_colour(e["b"][a], e["c"]) for a in range(3)],
                     final_normal(e["m"]), e["c"], e["first"]))
    voxel_of = [index.get(k, -1) if k is not None else -1 for k in key_of_point]
    return _pack(rows, n, voxel_of, n_skipped, bgr is not None, normal is not None)


def quantise_array(xyz, voxel):
    """-> q int64 [n, 3] (0 where skipped), valid bool [n], key uint64 [n] (SKIPPED where not valid)"""
    x = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        r = np.floor(x / np.float64(np.float32(voxel)) * 1024.0 + 0.5)
        valid = (np.isfinite(x) & (r >= -float(Q_LIMIT)) & (r < float(Q_LIMIT))).all(axis=1)
    q = np.where(valid[:, None], r, 0.0).astype(np.int64)
    i = ((q >> 10) + BIAS).astype(np.uint64)
    key = (i[:, 0] << np.uint64(42)) | (i[:, 1] << np.uint64(21)) | i[:, 2]
    return q, valid, np.where(valid, key, np.uint64(SKIPPED))


def normal_quanta_array(normal):
    x = np.asarray(normal, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        r = np.floor(x * 16384.0 + 0.5)
    r = np.where(np.isnan(r), 0.0, np.clip(r, -float(N_LIMIT), float(N_LIMIT)))
    return r.astype(np.int64)


def merge_sorted(xyz, bgr, normal, voxel, min_count):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n, vox = len(xyz), np.float64(np.float32(voxel))
    q, valid, key = quantise_array(xyz, voxel)
    order = np.argsort(key, kind="stable")
    order = order[: int(valid.sum())]                         # the skipped ones sort last
    voxel_of = np.full(n, -1, np.int32)
    have_bgr, have_normal = bgr is not None, normal is not None
    if len(order) == 0:
        return _pack([], n, voxel_of, n - int(valid.sum()), have_bgr, have_normal)
    ks = key[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    c = np.diff(np.concatenate([starts, [len(ks)]])).astype(np.int64)
    Sq = np.add.reduceat(q[order], starts, axis=0)
    keep = c >= min_count
    pos = np.cumsum(keep) - 1
    run_of = np.repeat(np.arange(len(starts)), c)
    voxel_of[order] = np.where(keep[run_of], pos[run_of], -1)
    cf = c.astype(np.float64)[:, None]
    out = dict(key=ks[starts][keep], xyz=(((Sq.astype(np.float64) / cf) / 1024.0) * vox).astype(np.float32)[keep], count=c[keep].astype(np.int32),
               first=np.minimum.reduceat(order, starts)[keep].astype(np.int32), voxel_of=voxel_of, n_skipped=n - int(valid.sum()), bgr=None,
               normal=None)
    if have_bgr:
        Sb = np.add.reduceat(np.asarray(bgr, np.uint8).reshape(-1, 3)[order].astype(np.int64), starts, axis=0)
        out["bgr"] = ((2 * Sb + c[:, None]) // (2 * c[:, None])).astype(np.uint8)[keep]
    if have_normal:
        Sm = np.add.reduceat(normal_quanta_array(np.asarray(normal, np.float32).reshape(-1, 3))[order], starts, axis=0).astype(np.float64)
        L = np.sqrt((Sm[:, 0] * Sm[:, 0] + Sm[:, 1] * Sm[:, 1]) + Sm[:, 2] * Sm[:, 2])
        with np.errstate(all="ignore"):
            out["normal"] = np.where(L[:, None] == 0.0, 0.0, Sm / L[:, None]).astype(np.float32)[keep]
    return out


MERGE_FIELDS = ("key", "xyz", "bgr", "normal", "count", "first", "voxel_of")


# ---- normals ------------------------------------------------------------------------------------------------------------------
def cam_point(k4, u, v, z):
    xn, yn = (float(u) - k4[2]) / k4[0], (float(v) - k4[3]) / k4[1]
    return [z * xn, z * yn, z]


def usable(zn, z0, step):
    return zn > 0.0 and abs(zn - z0) <= step * z0


def normals_loop(K, P, depth, max_rel_step):
    """One image.  K [3, 3], P [3, 4] (float32 values), depth float32 [h, w].  Returns normal float32 [h, w, 3], has bool [h, w],
    flipped bool [h, w] and mid float64 [h, w, 13] = c (after the flip), len, n_cam, du, dv -- filled as far as the pixel got."""
    K, P = np.asarray(K, np.float32).reshape(3, 3), np.asarray(P, np.float32).reshape(3, 4)
    k4 = [float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])]
    R = [[float(P[i, j]) for j in range(3)] for i in range(3)]
    depth = np.asarray(depth, np.float32)
    h, w = depth.shape
    step = float(np.float32(max_rel_step))
    normal, has, flipped, mid = np.zeros((h, w, 3), np.float32), np.zeros((h, w), bool), np.zeros((h, w), bool), np.zeros((h, w, 13))
    for v in range(h):
        for u in range(w):
            z0 = float(depth[v, u])
            if not z0 > 0.0:
                continue
            p0 = cam_point(k4, u, v, z0)
            side = {}
            for name, (uu, vv) in (("E", (u + 1, v)), ("W", (u - 1, v)), ("S", (u, v + 1)), ("N", (u, v - 1))):
                if 0 <= uu < w and 0 <= vv < h:
                    zn = float(depth[vv, uu])
                    if usable(zn, z0, step):              # Python floats: inf - inf is a quiet NaN, and a NaN fails the test
                        side[name] = cam_point(k4, uu, vv, zn)
            diffs = []
            for plus, minus in (("E", "W"), ("S", "N")):
                if plus not in side and minus not in side:
                    break
                hi, lo = side.get(plus, p0), side.get(minus, p0)
                with np.errstate(all="ignore"):
                    diffs.append([float(np.float64(hi[j]) - np.float64(lo[j])) for j in range(3)])
            if len(diffs) < 2:
                continue
            du, dv = diffs
            mid[v, u, 7:10], mid[v, u, 10:13] = du, dv
            with np.errstate(all="ignore"):
                du_, dv_, p_ = np.asarray(du), np.asarray(dv), np.asarray(p0)
                c = [float(dv_[(j + 1) % 3] * du_[(j + 2) % 3] - dv_[(j + 2) % 3] * du_[(j + 1) % 3]) for j in range(3)]
                if float((np.float64(c[0]) * p_[0] + np.float64(c[1]) * p_[1]) + np.float64(c[2]) * p_[2]) > 0.0:
                    c = [-x for x in c]
                    flipped[v, u] = True
                length = float(np.sqrt((np.float64(c[0]) * c[0] + np.float64(c[1]) * c[1]) + np.float64(c[2]) * c[2]))
            mid[v, u, 0:3], mid[v, u, 3] = c, length
            if not (length > 0.0 and math.isfinite(length)):
                continue
            nc = [x / length for x in c]
            mid[v, u, 4:7] = nc
            normal[v, u] = [np.float32((R[0][j] * nc[0] + R[1][j] * nc[1]) + R[2][j] * nc[2]) for j in range(3)]
            has[v, u] = True
    return dict(normal=normal, has=has, flipped=flipped, mid=mid)


def normals_shifted(K, P, depth, max_rel_step):
    K, P = np.asarray(K, np.float32).reshape(3, 3).astype(np.float64), np.asarray(P, np.float32).reshape(3, 4).astype(np.float64)
    z = np.asarray(depth, np.float32).astype(np.float64)
    h, w = z.shape
    step = np.float64(np.float32(max_rel_step))
    with np.errstate(all="ignore"):
        xn = (np.arange(w, dtype=np.float64) - K[0, 2]) / K[0, 0]
        yn = (np.arange(h, dtype=np.float64) - K[1, 2]) / K[1, 1]
        p = np.stack([z * xn[None, :], z * yn[:, None], z], axis=-1)

        def shifted(a, dy, dx, fill):
            out = np.full_like(a, fill)
            ys, yd = (slice(dy, None), slice(None, h - dy)) if dy >= 0 else (slice(None, dy), slice(-dy, None))
            xs, xd = (slice(dx, None), slice(None, w - dx)) if dx >= 0 else (slice(None, dx), slice(-dx, None))
            out[yd, xd] = a[ys, xs]
            return out

        def axis_diff(dy, dx):
            zp, zm = shifted(z, dy, dx, 0.0), shifted(z, -dy, -dx, 0.0)          # a neighbour outside the image: depth 0, never usable
            up, um = (zp > 0.0) & (np.abs(zp - z) <= step * z), (zm > 0.0) & (np.abs(zm - z) <= step * z)
            pp, pm = shifted(p, dy, dx, 0.0), shifted(p, -dy, -dx, 0.0)
            hi = np.where(up[..., None], pp, p)
            lo = np.where(um[..., None], pm, p)
            return hi - lo, up | um

        du, ok_u = axis_diff(0, 1)
        dv, ok_v = axis_diff(1, 0)
        c = np.stack([dv[..., 1] * du[..., 2] - dv[..., 2] * du[..., 1], dv[..., 2] * du[..., 0] - dv[..., 0] * du[..., 2],
                      dv[..., 0] * du[..., 1] - dv[..., 1] * du[..., 0]], axis=-1)
        dot = (c[..., 0] * p[..., 0] + c[..., 1] * p[..., 1]) + c[..., 2] * p[..., 2]
        flip = dot > 0.0
        c = np.where(flip[..., None], -c, c)
        length = np.sqrt((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2])
        has = (z > 0.0) & ok_u & ok_v & (length > 0.0) & np.isfinite(length)
        nc = c / length[..., None]
        world = np.stack([(P[0, j] * nc[..., 0] + P[1, j] * nc[..., 1]) + P[2, j] * nc[..., 2] for j in range(3)], axis=-1)
    normal = np.where(has[..., None], world, 0.0).astype(np.float32)
    return dict(normal=normal, has=has, flipped=flip & (z > 0.0) & ok_u & ok_v)
