"""CPU restatement of the feature extractor's contract (include/sfmba.h, sfmba_orb_extract) -- TEST INFRASTRUCTURE ONLY.

Every stage is integer arithmetic (the pyramid scales, the quotas and the key point coordinates are the only doubles), so the
device is held to this file bit for bit.  Each stage is stated twice and the two are held equal by tests/test_orb_oracle_cpu.py:

  vectorised   whole-array numpy (gray, resample_level, score_map, candidates, harris, orientation_bins, smooth, describe):
               what extract() runs, about half a second per 640 x 480 image
  plain        the contract's formula per pixel / per key point in Python ints (the *_plain functions), for tiny inputs

Allowed importers: tests/ and tools/.
"""
import math

import numpy as np

EDGE = 31                 # a key point lies at least this far from every edge of its level
MIN_SIDE = 62             # a level this wide or high (or less) has no key points
DISC = 15                 # orientation disc: u^2 + v^2 <= 225
CIRCLE = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
          (-2, -2), (-1, -3)]
TAPS = [18, 34, 49, 54, 49, 34, 18]
N_BINS = 30
COS = [int(math.floor(16384 * math.cos(2 * math.pi * k / N_BINS) + 0.5)) for k in range(N_BINS)]
SIN = [int(math.floor(16384 * math.sin(2 * math.pi * k / N_BINS) + 0.5)) for k in range(N_BINS)]
M64 = (1 << 64) - 1

KP_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32), ("response", np.float32),
                     ("octave", np.int32)])


def mix(z):
    """splitmix64's output function with its increment (pnp_mix of csrc/ransac_common.h)."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


# ---- pattern ---------------------------------------------------------------------------------------------------------
def base_pattern():
    """The first 256 accepted pairs (x0, y0, x1, y1) of the stream mix(k) % 13 + mix(k + 1) % 13 - 12."""
    out, k = [], 0
    while len(out) < 256:
        c = []
        for _ in range(4):
            c.append(mix(k) % 13 + mix(k + 1) % 13 - 12)
            k += 2
        x0, y0, x1, y1 = c
        if x0 * x0 + y0 * y0 > 169 or x1 * x1 + y1 * y1 > 169 or (x0 == x1 and y0 == y1):
            continue
        out.append((x0, y0, x1, y1))
    return out


def rotate(k, x, y):
    return (COS[k] * x - SIN[k] * y + 8192) >> 14, (SIN[k] * x + COS[k] * y + 8192) >> 14


_TABLE = None


def pattern_table():
    """[30][256][4] int8: the pattern rotated into every bin."""
    global _TABLE
    if _TABLE is None:
        base = base_pattern()
        t = np.zeros((N_BINS, 256, 4), np.int8)
        for k in range(N_BINS):
            for i, (x0, y0, x1, y1) in enumerate(base):
                t[k, i] = (*rotate(k, x0, y0), *rotate(k, x1, y1))
        _TABLE = t
    return _TABLE


# ---- pyramid and quotas ------------------------------------------------------------------------------------------------
def level_scales(scale_factor, n_levels):
    s, out = 1.0, []
    sf = float(np.float32(scale_factor))
    for _ in range(n_levels):
        out.append(s)
        s = s * sf
    return out


def level_sizes(w, h, scale_factor, n_levels):
    """[(w_l, h_l)]: floor(w / s_l + 0.5); the list ends in front of the first level of size 0."""
    out = []
    for s in level_scales(scale_factor, n_levels):
        wl, hl = int(math.floor(w / s + 0.5)), int(math.floor(h / s + 0.5))
        if wl <= 0 or hl <= 0:
            break
        out.append((wl, hl))
    return out


def quotas(n_features, scale_factor, n_levels):
    f = 1.0 / float(np.float32(scale_factor))
    fn = 1.0
    for _ in range(n_levels):
        fn = fn * f
    q, total = [], 0
    want = n_features * (1.0 - f) / (1.0 - fn)
    for _ in range(n_levels - 1):
        q.append(int(np.rint(want)))
        total += q[-1]
        want = want * f
    q.append(max(n_features - total, 0))
    return q


def gray(img):
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.copy()
    b, g, r = (img[:, :, c].astype(np.int64) for c in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def gray_plain(img):
    h, w = img.shape[:2]
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            b, g, r = (int(v) for v in img[y, x])
            out[y, x] = (1868 * b + 9617 * g + 4899 * r + 8192) >> 14
    return out


def _axis(n, m):
    d = np.arange(m, dtype=np.int64)
    num, den = (2 * d + 1) * n - m, 2 * m
    i0 = num // den
    f = ((num - i0 * den) * 2048 + den // 2) // den
    return i0, np.minimum(i0 + 1, n - 1), f


def resample_level(src, wl, hl):
    h, w = src.shape
    x0, x1, fx = _axis(w, wl)
    y0, y1, fy = _axis(h, hl)
    s = src.astype(np.int64)
    fx, fy = fx[None, :], fy[:, None]
    top = s[y0][:, x0] * (2048 - fx) + s[y0][:, x1] * fx
    bot = s[y1][:, x0] * (2048 - fx) + s[y1][:, x1] * fx
    return ((top * (2048 - fy) + bot * fy + (1 << 21)) >> 22).astype(np.uint8)


def resample_plain(src, wl, hl):
    h, w = src.shape
    out = np.zeros((hl, wl), np.uint8)

    def axis(d, n, m):
        num, den = (2 * d + 1) * n - m, 2 * m
        i0 = num // den
        return i0, min(i0 + 1, n - 1), ((num - i0 * den) * 2048 + den // 2) // den
    for y in range(hl):
        y0, y1, fy = axis(y, h, hl)
        for x in range(wl):
            x0, x1, fx = axis(x, w, wl)
            top = int(src[y0, x0]) * (2048 - fx) + int(src[y0, x1]) * fx
            bot = int(src[y1, x0]) * (2048 - fx) + int(src[y1, x1]) * fx
            out[y, x] = (top * (2048 - fy) + bot * fy + (1 << 21)) >> 22
    return out


def pyramid(g, scale_factor, n_levels):
    out = [g]
    for wl, hl in level_sizes(g.shape[1], g.shape[0], scale_factor, n_levels)[1:]:
        out.append(resample_level(out[-1], wl, hl))
    return out


# ---- FAST score, candidates ----------------------------------------------------------------------------------------------
def score_map(I, threshold):
    """S per pixel (0 within 3 of an edge): sliding minima of length 9 over the doubled circle, by doubling."""
    h, w = I.shape
    S = np.zeros((h, w), np.int64)
    if h < 7 or w < 7:
        return S
    p = I[3:h - 3, 3:w - 3].astype(np.int64)
    d = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx].astype(np.int64) - p for dx, dy in CIRCLE])
    best = None
    for sign in (1, -1):
        e = np.concatenate([sign * d, sign * d[:8]])                 # 24 entries: every arc of 9 is contiguous
        m2 = np.minimum(e[:-1], e[1:])
        m4 = np.minimum(m2[:-2], m2[2:])
        m8 = np.minimum(m4[:-4], m4[4:])
        m9 = np.minimum(m8[:16], e[8:24])
        v = m9.max(axis=0)
        best = v if best is None else np.maximum(best, v)
    best = np.where(best <= threshold, 0, best)
    S[3:h - 3, 3:w - 3] = best
    return S


def score_plain(I, x, y, threshold):
    p = int(I[y, x])
    d = [int(I[y + dy, x + dx]) - p for dx, dy in CIRCLE]
    S = max(max(min(d[(s + k) % 16] for k in range(9)), min(-d[(s + k) % 16] for k in range(9))) for s in range(16))
    return 0 if S <= threshold else S


def candidates(S, edge=EDGE):
    """(ys, xs) in raster order: S > 0, strictly above all 8 neighbours, at least `edge` from every edge."""
    h, w = S.shape
    if h <= 2 * edge or w <= 2 * edge:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    c = S[edge:h - edge, edge:w - edge]
    ok = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                ok &= c > S[edge + dy:h - edge + dy, edge + dx:w - edge + dx]
    ys, xs = np.nonzero(ok)
    return ys + edge, xs + edge


def candidates_plain(S, edge=EDGE):
    h, w = S.shape
    out = []
    for y in range(edge, h - edge):
        for x in range(edge, w - edge):
            s = int(S[y, x])
            if s > 0 and all(s > int(S[y + dy, x + dx]) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy):
                out.append((y, x))
    return (np.array([p[0] for p in out], np.int64), np.array([p[1] for p in out], np.int64))


# ---- Harris ------------------------------------------------------------------------------------------------------------
def harris(I, ys, xs):
    """R = 25 (a b - c^2) - (a + b)^2 in exact int64 at every (y, x), each at least 4 from the edges."""
    if len(ys) == 0:
        return np.zeros(0, np.int64)
    J = I.astype(np.int64)
    Ix = np.zeros_like(J); Iy = np.zeros_like(J)
    Ix[1:-1, 1:-1] = (J[:-2, 2:] + 2 * J[1:-1, 2:] + J[2:, 2:]) - (J[:-2, :-2] + 2 * J[1:-1, :-2] + J[2:, :-2])
    Iy[1:-1, 1:-1] = (J[2:, :-2] + 2 * J[2:, 1:-1] + J[2:, 2:]) - (J[:-2, :-2] + 2 * J[:-2, 1:-1] + J[:-2, 2:])
    o = np.arange(-3, 4)
    yy = ys[:, None, None] + o[None, :, None]
    xx = xs[:, None, None] + o[None, None, :]
    gx, gy = Ix[yy, xx], Iy[yy, xx]
    a, b, c = (gx * gx).sum(axis=(1, 2)), (gy * gy).sum(axis=(1, 2)), (gx * gy).sum(axis=(1, 2))
    return 25 * (a * b - c * c) - (a + b) * (a + b)


def harris_plain(I, x, y):
    a = b = c = 0
    for v in range(-3, 4):
        for u in range(-3, 4):
            P = lambda dx, dy: int(I[y + v + dy, x + u + dx])
            ix = (P(1, -1) + 2 * P(1, 0) + P(1, 1)) - (P(-1, -1) + 2 * P(-1, 0) + P(-1, 1))
            iy = (P(-1, 1) + 2 * P(0, 1) + P(1, 1)) - (P(-1, -1) + 2 * P(0, -1) + P(1, -1))
            a += ix * ix; b += iy * iy; c += ix * iy
    return 25 * (a * b - c * c) - (a + b) ** 2


def select(R, ys, xs, quota):
    """Indices of the first `quota` candidates in the order (R descending, y ascending, x ascending)."""
    return np.lexsort((xs, ys, -R))[:quota]


# ---- orientation ---------------------------------------------------------------------------------------------------------
def moments(I, ys, xs):
    o = np.arange(-DISC, DISC + 1)
    vv, uu = np.meshgrid(o, o, indexing="ij")
    inside = (uu * uu + vv * vv) <= DISC * DISC
    m10, m01 = np.zeros(len(ys), np.int64), np.zeros(len(ys), np.int64)
    for c0 in range(0, len(ys), 1024):
        y, x = ys[c0:c0 + 1024], xs[c0:c0 + 1024]
        P = I[y[:, None, None] + vv[None], x[:, None, None] + uu[None]].astype(np.int64) * inside[None]
        m10[c0:c0 + 1024] = (P * uu[None]).sum(axis=(1, 2))
        m01[c0:c0 + 1024] = (P * vv[None]).sum(axis=(1, 2))
    return m10, m01


def bins(m10, m01):
    C, Sn = np.array(COS, np.int64), np.array(SIN, np.int64)
    return np.argmax(m10[:, None] * C[None, :] + m01[:, None] * Sn[None, :], axis=1).astype(np.int64)   # argmax: the first maximum


def orientation_plain(I, x, y):
    m10 = m01 = 0
    for v in range(-DISC, DISC + 1):
        for u in range(-DISC, DISC + 1):
            if u * u + v * v <= DISC * DISC:
                m10 += u * int(I[y + v, x + u]); m01 += v * int(I[y + v, x + u])
    best, bk = None, 0
    for k in range(N_BINS):
        v = m10 * COS[k] + m01 * SIN[k]
        if best is None or v > best:
            best, bk = v, k
    return m10, m01, bk


# ---- smoothing and descriptor --------------------------------------------------------------------------------------------
def smooth(I):
    """The separable 7-tap filter; 0 within 3 of an edge (never read)."""
    h, w = I.shape
    B = np.zeros((h, w), np.uint8)
    if h < 7 or w < 7:
        return B
    J = I.astype(np.int64)
    H = sum(TAPS[k] * J[:, k:w - 6 + k] for k in range(7))
    V = sum(TAPS[k] * H[k:h - 6 + k, :] for k in range(7))
    B[3:h - 3, 3:w - 3] = (V + 32768) >> 16
    return B


def smooth_plain(I, x, y):
    v = sum(TAPS[j] * sum(TAPS[i] * int(I[y + j - 3, x + i - 3]) for i in range(7)) for j in range(7))
    return (v + 32768) >> 16


def describe(B, ys, xs, bn):
    T = pattern_table().astype(np.int64)[bn]                 # [n, 256, 4]
    a = B[ys[:, None] + T[:, :, 1], xs[:, None] + T[:, :, 0]]
    b = B[ys[:, None] + T[:, :, 3], xs[:, None] + T[:, :, 2]]
    return np.packbits((a < b).astype(np.uint8), axis=1, bitorder="little")


def describe_plain(I, x, y, k):
    out = np.zeros(32, np.uint8)
    for i, (x0, y0, x1, y1) in enumerate(base_pattern()):
        ax, ay = rotate(k, x0, y0)
        bx, by = rotate(k, x1, y1)
        if smooth_plain(I, x + ax, y + ay) < smooth_plain(I, x + bx, y + by):
            out[i // 8] |= 1 << (i % 8)
    return out


# ---- the whole contract ----------------------------------------------------------------------------------------------------
def extract(img, n_features=5000, scale_factor=1.2, n_levels=8, fast_threshold=20):
    """dict: kp (KP_DTYPE records), desc [n, 32] uint8, level_xy [n, 2] int32, bin [n] int32, harris [n] int64,
    candidates [n_levels] int32."""
    g = gray(img)
    scales = level_scales(scale_factor, n_levels)
    q = quotas(n_features, scale_factor, n_levels)
    kps, descs, lxy, bns, Rs = [], [], [], [], []
    ncand = np.zeros(n_levels, np.int32)
    for l, I in enumerate(pyramid(g, scale_factor, n_levels)):
        h, w = I.shape
        if w <= MIN_SIDE or h <= MIN_SIDE:
            break
        ys, xs = candidates(score_map(I, fast_threshold))
        ncand[l] = len(ys)
        R = harris(I, ys, xs)
        keep = select(R, ys, xs, q[l])
        ys, xs, R = ys[keep], xs[keep], R[keep]
        if len(ys) == 0:
            continue
        bn = bins(*moments(I, ys, xs))
        descs.append(describe(smooth(I), ys, xs, bn))
        kp = np.zeros(len(ys), KP_DTYPE)
        kp["x"] = (xs.astype(np.float64) * scales[l]).astype(np.float32)
        kp["y"] = (ys.astype(np.float64) * scales[l]).astype(np.float32)
        kp["size"] = np.float32(31.0 * scales[l])
        kp["angle"] = (12 * bn).astype(np.float32)
        kp["response"] = R.astype(np.float32)                  # one rounding, as (float)R of an int64
        kp["octave"] = l
        kps.append(kp); lxy.append(np.stack([xs, ys], axis=1).astype(np.int32)); bns.append(bn.astype(np.int32)); Rs.append(R)
    cat = lambda parts, empty: np.concatenate(parts) if parts else empty
    return {"kp": cat(kps, np.zeros(0, KP_DTYPE)), "desc": cat(descs, np.zeros((0, 32), np.uint8)),
            "level_xy": cat(lxy, np.zeros((0, 2), np.int32)), "bin": cat(bns, np.zeros(0, np.int32)),
            "harris": cat(Rs, np.zeros(0, np.int64)), "candidates": ncand}
