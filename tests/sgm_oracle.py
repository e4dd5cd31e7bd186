"""CPU restatement of sfmba_depth_cost_volume, sfmba_sgm_aggregate and sfmba_depth_sweep_sgm (the contract is in include/sfmba.h) --
TEST INFRASTRUCTURE ONLY (numpy).

The device is held to this file bit for bit (tests/test_gpu_depth_sgm.py), and so is csrc/sgm_math.h compiled for the host
(tests/test_sgm_oracle_cpu.py).  Every stage is stated twice and the two statements are held equal on every named case:

  volume      cost_volume         the costs of all planes from depth_oracle's integral-image window sums;
              cost_volume_direct  the same from its shifted-copy window sums, plane after plane;
  aggregate   aggregate_loop      Python integers: every path line is walked from its first pixel, pixel after pixel;
              aggregate_lines     numpy: a direction advances over ALL its lines at once, a column (or a row) of pixels per step;
  select      select_loop         a loop over the planes of every pixel;
              select              argmin and a masked min;
  finish      finish_loop         Python floats and integers per pixel;
              finish              numpy element-wise operations, which never fuse a product with a sum.

Allowed importers: tests/, tools/.
"""
import numpy as np

import depth_oracle as do

SENTINEL, NO_SECOND, MAX_COST, MAX_PENALTY = 255, 0xffff, 254, 1023
DIRECTIONS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]        # (dx, dy), y down
DEFAULTS = dict(p1=8, p2=64, n_paths=8, invalid_cost=127, uniqueness=5)


# ---- the volume -----------------------------------------------------------------------------------------------------------------
def quantise(C):
    """q = (int)floor((1.0 - C) * 127.0 + 0.5), every operation on its own."""
    return np.floor((1.0 - np.asarray(C, np.float64)) * 127.0 + 0.5).astype(np.int64)


def _volume(images, K, P, job, n_planes, radius, min_std, min_sources, box):
    I, Js, ABs = do._setup(images, K, P, job)
    h, w = I.shape
    wf, step = do.planes(job[2], job[3], n_planes)
    n, SI, SII, varI, part = do._reference(I, radius, min_std, box)
    vol = np.full((h, w, n_planes), SENTINEL, np.uint8)
    for k in range(n_planes):
        C, valid = do._plane_cost(I, Js, ABs, do.plane_w(wf, step, k), radius, n, SI, varI, part, min_sources, box)
        vol[:, :, k] = np.where(valid & part, quantise(np.where(valid, C, 0.0)), SENTINEL).astype(np.uint8)
    return vol, wf, step


def cost_volume(images, K, P, job, n_planes=64, radius=3, min_std=2, min_sources=1):
    """(uint8 [h, w, D], wf, step) of one job."""
    return _volume(images, K, P, job, n_planes, radius, min_std, min_sources, do.box_integral)


def cost_volume_direct(images, K, P, job, n_planes=64, radius=3, min_std=2, min_sources=1):
    return _volume(images, K, P, job, n_planes, radius, min_std, min_sources, do.box_direct)


def costs(vol, invalid_cost):
    """c(p, d): the volume with the sentinel read as invalid_cost, int64."""
    v = np.asarray(vol).astype(np.int64)
    return np.where(v == SENTINEL, invalid_cost, v)


# ---- aggregation ----------------------------------------------------------------------------------------------------------------
def path_loop(c, dx, dy, p1, p2):
    """L_r of one direction, int64 [h, w, D]: every line from its first pixel, Python integers.  Also returns m [h, w] (the minimum
    over the previous pixel's planes, -1 at a first pixel)."""
    h, w, D = c.shape
    L = np.zeros((h, w, D), np.int64)
    M = np.full((h, w), -1, np.int64)
    starts = [(x, y) for y in range(h) for x in range(w) if not (0 <= x - dx < w and 0 <= y - dy < h)]
    for x, y in starts:
        prev = None
        while 0 <= x < w and 0 <= y < h:
            cc = [int(v) for v in c[y, x]]
            if prev is None:
                cur = cc
            else:
                m = min(prev)
                cur = []
                for d in range(D):
                    terms = [prev[d], m + p2]
                    if d - 1 >= 0:
                        terms.append(prev[d - 1] + p1)
                    if d + 1 <= D - 1:
                        terms.append(prev[d + 1] + p1)
                    cur.append(cc[d] + min(terms) - m)
                M[y, x] = m
            L[y, x] = cur
            prev = cur
            x, y = x + dx, y + dy
    return L, M


def path_lines(c, dx, dy, p1, p2):
    """The same with numpy: the direction advances a column (dx != 0) or a row of pixels per step, all its lines at once."""
    h, w, D = c.shape
    L = np.zeros((h, w, D), np.int64)
    M = np.full((h, w), -1, np.int64)
    FAR = 1 << 40
    if dx != 0:
        ys = np.arange(h)
        for x in (range(w) if dx > 0 else range(w - 1, -1, -1)):
            xq, yq = x - dx, ys - dy
            inside = (0 <= xq < w) & (yq >= 0) & (yq < h)
            if not inside.any():
                L[:, x] = c[:, x]
                continue
            prev = L[np.clip(yq, 0, h - 1), min(max(xq, 0), w - 1)]               # [h, D]
            m = prev.min(1, keepdims=True)
            lo = np.concatenate([np.full((h, 1), FAR), prev[:, :-1]], 1) + p1
            hi = np.concatenate([prev[:, 1:], np.full((h, 1), FAR)], 1) + p1
            step = c[:, x] + np.minimum(np.minimum(prev, m + p2), np.minimum(lo, hi)) - m
            L[:, x] = np.where(inside[:, None], step, c[:, x])
            M[:, x] = np.where(inside, m[:, 0], -1)
    else:
        for y in (range(h) if dy > 0 else range(h - 1, -1, -1)):
            yq = y - dy
            if not 0 <= yq < h:
                L[y] = c[y]
                continue
            prev = L[yq]                                                           # [w, D]
            m = prev.min(1, keepdims=True)
            lo = np.concatenate([np.full((w, 1), FAR), prev[:, :-1]], 1) + p1
            hi = np.concatenate([prev[:, 1:], np.full((w, 1), FAR)], 1) + p1
            L[y] = c[y] + np.minimum(np.minimum(prev, m + p2), np.minimum(lo, hi)) - m
            M[y] = m[:, 0]
    return L, M


def _aggregate(vol, p1, p2, n_paths, invalid_cost, path):
    c = costs(vol, invalid_cost)
    Ls = [path(c, dx, dy, p1, p2) for dx, dy in DIRECTIONS[:n_paths]]
    S = sum(L for L, _ in Ls)
    assert S.max() <= n_paths * (MAX_COST + p2) <= 10216
    return dict(c=c, L=[L for L, _ in Ls], m=[M for _, M in Ls], sums=S.astype(np.uint16))


def aggregate_loop(vol, p1=8, p2=64, n_paths=8, invalid_cost=127):
    return _aggregate(vol, p1, p2, n_paths, invalid_cost, path_loop)


def aggregate_lines(vol, p1=8, p2=64, n_paths=8, invalid_cost=127):
    return _aggregate(vol, p1, p2, n_paths, invalid_cost, path_lines)


# ---- selection ------------------------------------------------------------------------------------------------------------------
def select_loop(sums):
    S = np.asarray(sums)
    h, w, D = S.shape
    plane, best, second = np.zeros((h, w), np.int16), np.zeros((h, w), np.uint16), np.zeros((h, w), np.uint16)
    for y in range(h):
        for x in range(w):
            s = [int(v) for v in S[y, x]]
            k = 0
            for d in range(1, D):
                if s[d] < s[k]:
                    k = d
            sec = NO_SECOND
            for d in range(D):
                if abs(d - k) > 1 and s[d] < sec:
                    sec = s[d]
            plane[y, x], best[y, x], second[y, x] = k, s[k], sec
    return plane, best, second


def select(sums):
    S = np.asarray(sums).astype(np.int64)
    D = S.shape[2]
    k = S.argmin(2)                                          # the first of equal minima: the lowest d
    best = np.take_along_axis(S, k[..., None], 2)[..., 0]
    far = np.abs(np.arange(D)[None, None, :] - k[..., None]) > 1
    second = np.where(far, S, NO_SECOND).min(2)
    return k.astype(np.int16), best.astype(np.uint16), second.astype(np.uint16)


# ---- the three maps -------------------------------------------------------------------------------------------------------------
def accepted(best, second, uniqueness):
    b, s = np.asarray(best).astype(np.int64), np.asarray(second).astype(np.int64)
    return (s == NO_SECOND) | (100 * (s - b) >= uniqueness * s)


def finish(vol, sums, plane, best, second, wf, step, uniqueness=5):
    """dict(depth, score, plane, accepted, den, delta) from the selection, the sums and the pixel's own volume entries."""
    S = np.asarray(sums).astype(np.int64)
    D = S.shape[2]
    k = np.asarray(plane).astype(np.int64)
    take = lambda a, kk: np.take_along_axis(a, np.clip(kk, 0, D - 1)[..., None], 2)[..., 0]
    sm, s0, sp = take(S, k - 1), take(S, k), take(S, k + 1)
    inner = (k > 0) & (k < D - 1)
    den = np.where(inner, (sm - 2 * s0) + sp, 0)
    use = inner & (den > 0)
    delta = np.where(use, (0.5 * (sm - sp).astype(np.float64)) / np.where(use, den, 1).astype(np.float64), 0.0)
    acc = accepted(best, second, uniqueness)
    wv = (wf + k.astype(np.float64) * step) + delta * step
    with np.errstate(all="ignore"):
        depth = np.where(acc, (1.0 / wv).astype(np.float32), np.float32(0.0)).astype(np.float32)
    q = take(np.asarray(vol).astype(np.int64), k)
    score = np.where(q != SENTINEL, (1.0 - q.astype(np.float64) / 127.0).astype(np.float32), np.float32(0.0)).astype(np.float32)
    return dict(depth=depth, score=score, plane=k.astype(np.int16), accepted=acc, den=den, delta=delta, q=q)


def finish_loop(vol, sums, plane, best, second, wf, step, uniqueness=5):
    S, V = np.asarray(sums), np.asarray(vol)
    h, w, D = S.shape
    out = dict(depth=np.zeros((h, w), np.float32), score=np.zeros((h, w), np.float32), plane=np.asarray(plane).astype(np.int16),
               accepted=np.zeros((h, w), bool), den=np.zeros((h, w), np.int64), delta=np.zeros((h, w)), q=np.zeros((h, w), np.int64))
    for y in range(h):
        for x in range(w):
            k, b, s = int(plane[y, x]), int(best[y, x]), int(second[y, x])
            delta = 0.0
            if 0 < k < D - 1:
                sm, sp = int(S[y, x, k - 1]), int(S[y, x, k + 1])
                den = (sm - 2 * b) + sp
                out["den"][y, x] = den
                if den > 0:
                    delta = (0.5 * float(sm - sp)) / float(den)
            out["delta"][y, x] = delta
            if s == NO_SECOND or 100 * (s - b) >= uniqueness * s:
                out["accepted"][y, x] = True
                out["depth"][y, x] = np.float32(1.0 / ((wf + float(k) * step) + delta * step))
            q = int(V[y, x, k])
            out["q"][y, x] = q
            if q != SENTINEL:
                out["score"][y, x] = np.float32(1.0 - float(q) / 127.0)
    return out


# ---- whole calls ----------------------------------------------------------------------------------------------------------------
def sgm_aggregate(vol, p1=8, p2=64, n_paths=8, invalid_cost=127):
    """What capi.sgm_aggregate returns for one volume."""
    a = aggregate_lines(vol, p1, p2, n_paths, invalid_cost)
    plane, best, second = select(a["sums"])
    return dict(plane=plane, best=best, second=second, sums=a["sums"])


def maps_of(vol, agg, wf, step, uniqueness=5):
    """(depth, score, plane) from a volume and what sgm_aggregate (this one or the device's) returned for it."""
    f = finish(vol, agg["sums"], agg["plane"], agg["best"], agg["second"], wf, step, uniqueness)
    return f["depth"], f["score"], f["plane"]


def sweep_sgm(images, K, P, jobs, n_planes=64, radius=3, min_std=2, min_sources=1, p1=8, p2=64, n_paths=8, invalid_cost=127, uniqueness=5):
    """What capi.depth_sweep_sgm returns: one (depth, score, plane) per job."""
    out = []
    for job in jobs:
        vol, wf, step = cost_volume(images, K, P, job, n_planes, radius, min_std, min_sources)
        out.append(maps_of(vol, sgm_aggregate(vol, p1, p2, n_paths, invalid_cost), wf, step, uniqueness))
    return out
