"""CPU restatement of sfmba_flow_track and sfmba_flow_match (the contract is in include/sfmba.h) -- TEST INFRASTRUCTURE ONLY (numpy).

The device is held to this file bit for bit (tests/test_gpu_flow_track.py), and so is csrc/flow_math.h compiled for the host
(tests/test_flow_oracle_cpu.py).  Samples and window sums are exact integers (Python ints or int64); the fp64 operations of a level are
Python float operations, one rounding each (Python never fuses a product with a sum; math.sqrt is correctly rounded).  Both calls are
stated twice:

  track_loops     per-pixel Python loops over the window, a scalar sampler, a pyramid built pixel by pixel, b = sum (T - J) g;
  track_vec       the window as shifted copies of one sampled (2r+3)^2 block, the pyramid from clamped index arrays,
                  b = sum T g - sum J g;
  match_serial    a sort per query and a serial set of taken train indices, as the reference's loop walks them;
  match_vec       a vectorised 2-NN over the whole distance matrix and a per-train minimum over the candidates.

Allowed importers: tests/, tools/.
"""
import math

import numpy as np

from depth_oracle import gray, sample

CENTRE_LIMIT = 1 << 28
KERNEL = (1, 4, 6, 4, 1)
DEFAULTS = dict(n_levels=4, radius=7, max_iters=20, min_eig=1.0)          # first choices nobody has tuned
MATCH_DEFAULTS = dict(max_err=12.0, radius=2.0, ratio=0.7)                 # the reference's


# ---- pyramid -----------------------------------------------------------------------------------------------------------------
def pyr_down_vec(I):
    h, w = I.shape
    nh, nw = (h + 1) >> 1, (w + 1) >> 1
    ys = [np.clip(2 * np.arange(nh) + j - 2, 0, h - 1) for j in range(5)]
    xs = [np.clip(2 * np.arange(nw) + i - 2, 0, w - 1) for i in range(5)]
    s = np.zeros((nh, nw), np.int64)
    for j in range(5):
        for i in range(5):
            s += KERNEL[i] * KERNEL[j] * I[np.ix_(ys[j], xs[i])]
    return (s + 128) >> 8


def pyr_down_loops(I):
    h, w = I.shape
    rows = I.tolist()
    out = []
    for y in range((h + 1) >> 1):
        out.append([])
        for x in range((w + 1) >> 1):
            s = 0
            for j in range(5):
                row = rows[min(max(2 * y + j - 2, 0), h - 1)]
                for i in range(5):
                    s += KERNEL[i] * KERNEL[j] * row[min(max(2 * x + i - 2, 0), w - 1)]
            out[-1].append((s + 128) >> 8)
    return np.asarray(out, dtype=np.int64).reshape((h + 1) >> 1, (w + 1) >> 1)


def pyramid(img, n_levels, down=pyr_down_vec):
    """The n_levels levels of an image (h x w gray or h x w x 3 BGR) as int64 arrays."""
    levels = [gray(img)]
    for _ in range(n_levels - 1):
        levels.append(down(levels[-1]))
    return levels


# ---- the scalar pieces of a level ----------------------------------------------------------------------------------------------
def centre(x, level):
    c = math.floor(16.0 * (float(np.float32(x)) / float(1 << level)) + 0.5)
    return max(-CENTRE_LIMIT, min(CENTRE_LIMIT, c))


def trackable(Gxx, Gyy, Gxy, min_eig, n):
    """(flag, det) of a level from its exact sums (Python ints)."""
    xx, yy, xy = float(Gxx), float(Gyy), float(Gxy)
    q = xy * xy
    det = xx * yy - q
    df = float(Gxx - Gyy)
    lam = (float(Gxx + Gyy) - math.sqrt(df * df + 4.0 * q)) * 0.5
    return det > 0.0 and lam >= (float(np.float32(min_eig)) * float(n)) * 1024.0, det


def lam_of(Gxx, Gyy, Gxy):
    df, xy = float(Gxx - Gyy), float(Gxy)
    return (float(Gxx + Gyy) - math.sqrt(df * df + 4.0 * (xy * xy))) * 0.5


def step(Gxx, Gyy, Gxy, det, bx, by, r):
    xx, yy, xy, bx, by = float(Gxx), float(Gyy), float(Gxy), float(bx), float(by)
    nx = yy * bx - xy * by
    ny = xx * by - xy * bx
    sx = math.floor((32.0 * nx) / det + 0.5)
    sy = math.floor((32.0 * ny) / det + 0.5)
    lim = 16 * r
    return int(max(-lim, min(lim, sx))), int(max(-lim, min(lim, sy)))


def next_of(x, dq):
    return np.float32(float(np.float32(x)) + float(dq) / 16.0)


def err_of(sad, n):
    return np.float32(float(sad) / (16.0 * float(n)))


def inside(c, dq, n):
    return 0 <= c + dq <= 16 * (n - 1)


def sample1(rows, w, h, su, sv):
    """The clamped sampler on one coordinate, Python ints; rows = the level as a list of lists."""
    su, sv = min(max(su, 0), 16 * (w - 1)), min(max(sv, 0), 16 * (h - 1))
    x0, fx, y0, fy = su >> 4, su & 15, sv >> 4, sv & 15
    x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
    return ((16 - fx) * (16 - fy) * rows[y0][x0] + fx * (16 - fy) * rows[y0][x1] + (16 - fx) * fy * rows[y1][x0]
            + fx * fy * rows[y1][x1] + 8) >> 4


def sample_block(I, cx, cy, half):
    """S(I, (cx, cy) + 16 (i, j)) for i, j in -half .. half: int64 [2 half + 1, 2 half + 1], [j, i]."""
    h, w = I.shape
    o = 16 * np.arange(-half, half + 1, dtype=np.int64)
    su, sv = np.clip(cx + o, 0, 16 * (w - 1)), np.clip(cy + o, 0, 16 * (h - 1))
    return sample(I, su[None, :], sv[:, None])


# ---- one point -----------------------------------------------------------------------------------------------------------------
def _point_vec(S, D, x, y, L, r, max_iters, min_eig):
    n = (2 * r + 1) ** 2
    dqx = dqy = 0
    G, state = np.zeros((L, 3), np.int64), np.zeros((L, 4), np.int32)
    for l in range(L - 1, -1, -1):
        if l < L - 1:
            dqx, dqy = 2 * dqx, 2 * dqy
        cx, cy = centre(x, l), centre(y, l)
        T = sample_block(S[l], cx, cy, r + 1)
        gx, gy, Tc = T[1:-1, 2:] - T[1:-1, :-2], T[2:, 1:-1] - T[:-2, 1:-1], T[1:-1, 1:-1]
        Gxx, Gyy, Gxy = int((gx * gx).sum()), int((gy * gy).sum()), int((gx * gy).sum())
        Tgx, Tgy = int((Tc * gx).sum()), int((Tc * gy).sum())
        ok, det = trackable(Gxx, Gyy, Gxy, min_eig, n)
        it = 0
        while ok and it < max_iters:
            J = sample_block(D[l], cx + dqx, cy + dqy, r)
            sx, sy = step(Gxx, Gyy, Gxy, det, Tgx - int((J * gx).sum()), Tgy - int((J * gy).sum()), r)
            it += 1
            if sx == 0 and sy == 0:
                break
            dqx, dqy = dqx + sx, dqy + sy
        G[l] = (Gxx, Gyy, Gxy)
        state[l] = (int(ok), it, dqx, dqy)
    sad = int(np.abs(Tc - sample_block(D[0], cx + dqx, cy + dqy, r)).sum()) if ok else 0
    hd, wd = D[0].shape
    status = 1 if ok and inside(cx, dqx, wd) and inside(cy, dqy, hd) else 0
    return (next_of(x, dqx), next_of(y, dqy)), status, (err_of(sad, n) if ok else np.float32(0.0)), G, state


def _point_loops(S, D, x, y, L, r, max_iters, min_eig):
    """S, D: per level (rows as a list of lists, w, h)."""
    n = (2 * r + 1) ** 2
    dqx = dqy = 0
    G, state = np.zeros((L, 3), np.int64), np.zeros((L, 4), np.int32)
    for l in range(L - 1, -1, -1):
        if l < L - 1:
            dqx, dqy = 2 * dqx, 2 * dqy
        cx, cy = centre(x, l), centre(y, l)
        (srows, sw, sh), (drows, dw, dh) = S[l], D[l]
        T = {(i, j): sample1(srows, sw, sh, cx + 16 * i, cy + 16 * j) for j in range(-r - 1, r + 2) for i in range(-r - 1, r + 2)}
        win = [(i, j) for j in range(-r, r + 1) for i in range(-r, r + 1)]
        gx = {(i, j): T[i + 1, j] - T[i - 1, j] for i, j in win}
        gy = {(i, j): T[i, j + 1] - T[i, j - 1] for i, j in win}
        Gxx, Gyy, Gxy = sum(gx[k] ** 2 for k in win), sum(gy[k] ** 2 for k in win), sum(gx[k] * gy[k] for k in win)
        ok, det = trackable(Gxx, Gyy, Gxy, min_eig, n)
        it = 0
        while ok and it < max_iters:
            bx = by = 0
            for i, j in win:
                d = T[i, j] - sample1(drows, dw, dh, cx + dqx + 16 * i, cy + dqy + 16 * j)
                bx += d * gx[i, j]
                by += d * gy[i, j]
            sx, sy = step(Gxx, Gyy, Gxy, det, bx, by, r)
            it += 1
            if sx == 0 and sy == 0:
                break
            dqx, dqy = dqx + sx, dqy + sy
        G[l] = (Gxx, Gyy, Gxy)
        state[l] = (int(ok), it, dqx, dqy)
    sad = sum(abs(T[i, j] - sample1(drows, dw, dh, cx + dqx + 16 * i, cy + dqy + 16 * j)) for i, j in win) if ok else 0
    status = 1 if ok and inside(cx, dqx, dw) and inside(cy, dqy, dh) else 0
    return (next_of(x, dqx), next_of(y, dqy)), status, (err_of(sad, n) if ok else np.float32(0.0)), G, state


def _track(images, pairs, points, L, r, max_iters, min_eig, down, point, wrap):
    named = sorted({int(i) for p in pairs for i in p})
    pyr = {i: pyramid(images[i], L, down) for i in named}
    lv = {i: [wrap(a) for a in pyr[i]] for i in named}
    out = []
    for (s, d), pts in zip(pairs, points):
        pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
        m = len(pts)
        nxt, status, err = np.zeros((m, 2), np.float32), np.zeros(m, np.uint8), np.zeros(m, np.float32)
        G, state = np.zeros((m, L, 3), np.int64), np.zeros((m, L, 4), np.int32)
        for q, (x, y) in enumerate(pts):
            nxt[q], status[q], err[q], G[q], state[q] = point(lv[int(s)], lv[int(d)], x, y, L, r, max_iters, min_eig)
        out.append((nxt, status, err, G, state))
    levels = [[a.astype(np.uint8) for a in pyr[i]] if i in pyr else None for i in range(len(images))]
    return out, levels


def track_vec(images, pairs, points, n_levels=4, radius=7, max_iters=20, min_eig=1.0):
    """Per pair (next float32 [n, 2], status uint8 [n], err float32 [n], G int64 [n, L, 3], state int32 [n, L, 4]) and per image its
    pyramid levels (uint8; None for an image that no pair names)."""
    return _track(images, pairs, points, n_levels, radius, max_iters, min_eig, pyr_down_vec, _point_vec, lambda a: a)


def track_loops(images, pairs, points, n_levels=4, radius=7, max_iters=20, min_eig=1.0):
    return _track(images, pairs, points, n_levels, radius, max_iters, min_eig, pyr_down_loops, _point_loops,
                  lambda a: (a.tolist(), a.shape[1], a.shape[0]))


track = track_vec


# ---- match ---------------------------------------------------------------------------------------------------------------------
def dist2(qx, qy, kx, ky):
    dx, dy = float(np.float32(qx)) - float(np.float32(kx)), float(np.float32(qy)) - float(np.float32(ky))
    return dx * dx + dy * dy


def match_serial_pair(kp, nxt, status, err, max_err=12.0, radius=2.0, ratio=0.7):
    """One pair: (query_idx int32, train_idx int32, distance float32)."""
    kp, nxt = np.asarray(kp, np.float32).reshape(-1, 2), np.asarray(nxt, np.float32).reshape(-1, 2)
    r2 = float(np.float32(radius)) * float(np.float32(radius))
    taken, out = set(), []
    for q in range(len(nxt)):
        if status[q] == 0 or not (np.float32(err[q]) < np.float32(max_err)):
            continue
        near = sorted((s, j) for j, s in ((j, dist2(nxt[q, 0], nxt[q, 1], kp[j, 0], kp[j, 1])) for j in range(len(kp))) if s <= r2)
        if not near:
            continue
        if len(near) >= 2 and not (math.sqrt(near[0][0]) < float(ratio) * math.sqrt(near[1][0])):
            continue
        s, j = near[0]
        if j in taken:
            continue
        taken.add(j)
        out.append((q, j, np.float32(math.sqrt(s))))
    return (np.asarray([o[0] for o in out], np.int32), np.asarray([o[1] for o in out], np.int32), np.asarray([o[2] for o in out], np.float32))


def match_vec_pair(kp, nxt, status, err, max_err=12.0, radius=2.0, ratio=0.7):
    kp, nxt = np.asarray(kp, np.float32).reshape(-1, 2), np.asarray(nxt, np.float32).reshape(-1, 2)
    nq, nt = len(nxt), len(kp)
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    if nq == 0 or nt == 0:
        return empty
    r2 = float(np.float32(radius)) * float(np.float32(radius))
    eligible = (np.asarray(status) != 0) & (np.asarray(err, np.float32) < np.float32(max_err))
    with np.errstate(all="ignore"):
        dx = nxt[:, 0].astype(np.float64)[:, None] - kp[:, 0].astype(np.float64)[None, :]
        dy = nxt[:, 1].astype(np.float64)[:, None] - kp[:, 1].astype(np.float64)[None, :]
        s = dx * dx + dy * dy
        near = s <= r2
    count = near.sum(axis=1)
    masked = np.where(near, s, np.inf)
    order = np.argsort(masked, axis=1, kind="stable")                      # a tie on s keeps the lower j first
    j1 = order[:, 0]
    s1 = masked[np.arange(nq), j1]
    s2 = masked[np.arange(nq), order[:, 1]] if nt >= 2 else np.full(nq, np.inf)
    with np.errstate(all="ignore"):
        passes = np.sqrt(s1) < float(ratio) * np.sqrt(s2)
    cand = eligible & ((count == 1) | ((count >= 2) & passes))
    first = np.full(nt, nq, np.int64)
    np.minimum.at(first, j1[cand], np.nonzero(cand)[0])
    keep = cand & (first[j1] == np.arange(nq))
    q = np.nonzero(keep)[0]
    return q.astype(np.int32), j1[q].astype(np.int32), np.sqrt(s1[q]).astype(np.float32)


def _match(pair_fn, keypoints, pairs, tracked, **params):
    ptr, qs, ts, ds = [0], [], [], []
    for (_, d), t in zip(pairs, tracked):
        q, j, dist = pair_fn(keypoints[int(d)], t[0], t[1], t[2], **params)
        ptr.append(ptr[-1] + len(q))
        qs.append(q); ts.append(j); ds.append(dist)
    cat = lambda xs, dt: np.concatenate(xs + [np.zeros(0, dt)]).astype(dt)
    return np.asarray(ptr, np.int64), cat(qs, np.int32), cat(ts, np.int32), cat(ds, np.float32)


def match_serial(keypoints, pairs, tracked, **params):
    """(pair_ptr int64 [n_pairs + 1], query_idx, train_idx, distance float32) as capi.flow_match returns them."""
    return _match(match_serial_pair, keypoints, pairs, tracked, **params)


def match_vec(keypoints, pairs, tracked, **params):
    return _match(match_vec_pair, keypoints, pairs, tracked, **params)


match = match_vec
