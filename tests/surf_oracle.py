"""CPU restatement of the float-descriptor extractor's contract (include/sfmba.h, sfmba_surf_extract) -- TEST INFRASTRUCTURE ONLY.

Everything up to the normalisation is integer arithmetic (H is one IEEE division of two exactly representable integers), so the
device is held to this file bit for bit.  The detector, the orientation and the descriptor are each stated twice, by different
routes, and tests/test_surf_oracle_cpu.py holds the two equal:

  vectorised   box sums as four look-ups in an int64 integral image (numpy cumsum) with clamped coordinates, whole grids and whole
               key point lists at a time (response_maps, candidates, moments, sums, normalise): what extract() runs
  plain        box sums as direct pixel sums over a zero-padded copy of the image, Python integers, one position / key point at a
               time, the weights from their formulas, H as Python's correctly rounded int / int, the normalisation through exact
               rationals (the *_plain functions): for tiny inputs

Allowed importers: tests/ and tools/.
"""
import math
from fractions import Fraction

import numpy as np

import orb_oracle as oo

DESC_HALF = 5 * 16384
COS, SIN = oo.COS, oo.SIN
WG = [[int(math.floor(65536 * math.exp(-(i * i + j * j) / 12.5) + 0.5)) for i in range(6)] for j in range(6)]                 # [|j|][|i|]
WD = [[int(math.floor(4096 * math.exp(-(a * a + b * b) / 87.12) + 0.5)) for a in range(1, 20, 2)] for b in range(1, 20, 2)]   # [(|b|-1)/2][(|a|-1)/2]
ORI = [(i, j) for j in range(-5, 6) for i in range(-5, 6) if i * i + j * j < 36]
assert len(ORI) == 109

KP_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32), ("response", np.float32),
                     ("octave", np.int32), ("layer", np.int32), ("laplacian", np.int32)])


def layer_size(o, i):
    return 3 * (2 ** (o + 1) * (i + 1) + 1)


# ---- box sums ------------------------------------------------------------------------------------------------------------
def integral(g):
    I = np.zeros((g.shape[0] + 1, g.shape[1] + 1), np.int64)
    I[1:, 1:] = g.astype(np.int64).cumsum(axis=0).cumsum(axis=1)
    return I


def box(I, y0, x0, bh, bw):
    """Box(y0, x0, bh, bw) for arrays (or scalars) of coordinates: the four corners clamped into the integral image."""
    h, w = I.shape[0] - 1, I.shape[1] - 1
    ya, yb = np.clip(y0, 0, h), np.clip(y0 + bh, 0, h)
    xa, xb = np.clip(x0, 0, w), np.clip(x0 + bw, 0, w)
    return I[yb, xb] - I[ya, xb] - I[yb, xa] + I[ya, xa]


PAD = 400     # more than any box of the contract reaches from a key point (descriptor window of L = 195: 350 + 26)


def padded(g):
    P = np.zeros((g.shape[0] + 2 * PAD, g.shape[1] + 2 * PAD), np.int64)
    P[PAD:PAD + g.shape[0], PAD:PAD + g.shape[1]] = g
    return P


def box_plain(P, y0, x0, bh, bw):
    """The same sum from the pixels of the zero-padded image."""
    assert y0 + PAD >= 0 and x0 + PAD >= 0 and y0 + bh + PAD <= P.shape[0] and x0 + bw + PAD <= P.shape[1]
    return int(P[y0 + PAD:y0 + bh + PAD, x0 + PAD:x0 + bw + PAD].sum())


# ---- detector --------------------------------------------------------------------------------------------------------------
def hessian(I, y, x, L):
    """(H float64, Dxx + Dyy) at arrays of positions."""
    l, b = L // 3, (L - 1) // 2
    Dyy = box(I, y - b, x - l + 1, L, 2 * l - 1) - 3 * box(I, y - (l - 1) // 2, x - l + 1, l, 2 * l - 1)
    Dxx = box(I, y - l + 1, x - b, 2 * l - 1, L) - 3 * box(I, y - l + 1, x - (l - 1) // 2, 2 * l - 1, l)
    Dxy = box(I, y - l, x + 1, l, l) + box(I, y + 1, x - l, l, l) - box(I, y - l, x - l, l, l) - box(I, y + 1, x + 1, l, l)
    N = 100 * Dxx * Dyy - 81 * Dxy * Dxy
    return N.astype(np.float64) / np.float64(100 * L ** 4), Dxx + Dyy


def hessian_plain(P, y, x, L):
    l, b = L // 3, (L - 1) // 2
    B = lambda *a: box_plain(P, *a)
    Dyy = B(y - b, x - l + 1, L, 2 * l - 1) - 3 * B(y - (l - 1) // 2, x - l + 1, l, 2 * l - 1)
    Dxx = B(y - l + 1, x - b, 2 * l - 1, L) - 3 * B(y - l + 1, x - (l - 1) // 2, 2 * l - 1, l)
    Dxy = B(y - l, x + 1, l, l) + B(y + 1, x - l, l, l) - B(y - l, x - l, l, l) - B(y + 1, x + 1, l, l)
    N = 100 * Dxx * Dyy - 81 * Dxy * Dxy
    assert abs(N) < 2 ** 53
    return N / (100 * L ** 4), Dxx + Dyy            # int / int: correctly rounded, as the one IEEE division is


def response_maps(I, o):
    """[4][gh][gw] float64: H of every layer of octave o at every grid position (clipped filters included; never consulted)."""
    h, w = I.shape[0] - 1, I.shape[1] - 1
    s = 2 ** o
    ys, xs = np.meshgrid(np.arange(0, h, s), np.arange(0, w, s), indexing="ij")
    return np.stack([hessian(I, ys, xs, layer_size(o, i))[0] for i in range(4)])


def _span(n, o, m):
    """Grid indices lo .. hi (inclusive) along an axis of n pixels at which a candidate of (o, m) may lie."""
    s, bt = 2 ** o, (layer_size(o, m + 1) - 1) // 2
    return -((-(s + bt)) // s), (n - 1 - s - bt) // s if n - 1 - s - bt >= 0 else -1


def candidates(R, o, m, w, h, threshold):
    """(ys, xs, H) of the candidates of layer m of octave o, in raster order."""
    s = 2 ** o
    (x0, x1), (y0, y1) = _span(w, o, m), _span(h, o, m)
    if x1 < x0 or y1 < y0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)
    c = R[m, y0:y1 + 1, x0:x1 + 1]
    ok = c > np.float64(np.float32(threshold))
    for dl in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dl or dy or dx:
                    ok &= c > R[m + dl, y0 + dy:y1 + 1 + dy, x0 + dx:x1 + 1 + dx]
    gy, gx = np.nonzero(ok)
    return (gy + y0) * s, (gx + x0) * s, c[gy, gx]


def candidates_plain(P, o, m, w, h, threshold):
    s, bt = 2 ** o, (layer_size(o, m + 1) - 1) // 2
    thr = float(np.float32(threshold))
    out = []
    for y in range(0, h, s):
        for x in range(0, w, s):
            if not (x - s - bt >= 0 and x + s + bt <= w - 1 and y - s - bt >= 0 and y + s + bt <= h - 1):
                continue
            v = hessian_plain(P, y, x, layer_size(o, m))[0]
            if v > thr and all(v > hessian_plain(P, y + dy * s, x + dx * s, layer_size(o, m + dl))[0]
                               for dl in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dl or dy or dx):
                out.append((y, x, v))
    return out


# ---- Haar, orientation -------------------------------------------------------------------------------------------------------
def haar_x(I, y, x, p):
    return box(I, y - p, x, 2 * p, p) - box(I, y - p, x - p, 2 * p, p)


def haar_y(I, y, x, p):
    return box(I, y, x - p, p, 2 * p) - box(I, y - p, x - p, p, 2 * p)


def moments(I, ys, xs, ls):
    """(mx, my) int64 for key points at (ys, xs) with lobes ls."""
    r = (4 * ls + 5) // 10
    mx, my = np.zeros(len(ys), np.int64), np.zeros(len(ys), np.int64)
    for i, j in ORI:
        yy, xx = ys + (4 * ls * j + 5) // 10, xs + (4 * ls * i + 5) // 10
        mx += WG[abs(j)][abs(i)] * haar_x(I, yy, xx, 2 * r)
        my += WG[abs(j)][abs(i)] * haar_y(I, yy, xx, 2 * r)
    return mx, my


def orientation_plain(P, y, x, l):
    r = (4 * l + 5) // 10
    mx = my = 0
    for j in range(-5, 6):
        for i in range(-5, 6):
            if i * i + j * j >= 36:
                continue
            wg = int(math.floor(65536 * math.exp(-(i * i + j * j) / 12.5) + 0.5))
            yy, xx, p = y + (4 * l * j + 5) // 10, x + (4 * l * i + 5) // 10, 2 * r
            mx += wg * (box_plain(P, yy - p, xx, 2 * p, p) - box_plain(P, yy - p, xx - p, 2 * p, p))
            my += wg * (box_plain(P, yy, xx - p, p, 2 * p) - box_plain(P, yy - p, xx - p, p, 2 * p))
    best, bk = None, 0
    for k in range(30):
        v = mx * COS[k] + my * SIN[k]
        if best is None or v > best:
            best, bk = v, k
    return mx, my, bk


# ---- descriptor ----------------------------------------------------------------------------------------------------------------
def sums(I, ys, xs, ls, bn):
    """[n][64] int64: the sums v of every key point."""
    C, S = np.array(COS, np.int64)[bn], np.array(SIN, np.int64)[bn]
    r = (4 * ls + 5) // 10
    v = np.zeros((len(ys), 64), np.int64)
    d = DESC_HALF
    for j in range(-10, 10):
        for i in range(-10, 10):
            a, b = 2 * i + 1, 2 * j + 1
            ox = (2 * ls * (C * a - S * b) + d) // (2 * d)
            oy = (2 * ls * (S * a + C * b) + d) // (2 * d)
            hx, hy = haar_x(I, ys + oy, xs + ox, r), haar_y(I, ys + oy, xs + ox, r)
            dx, dy = C * hx + S * hy, -S * hx + C * hy
            wd = WD[(abs(b) - 1) // 2][(abs(a) - 1) // 2]
            base = (4 * ((j + 10) // 5) + (i + 10) // 5) * 4
            v[:, base] += wd * dx
            v[:, base + 1] += wd * dy
            v[:, base + 2] += wd * np.abs(dx)
            v[:, base + 3] += wd * np.abs(dy)
    return v


def sums_plain(P, y, x, l, k):
    C, S, d, r = COS[k], SIN[k], DESC_HALF, (4 * l + 5) // 10
    v = [0] * 64
    for i in range(-10, 10):
        for j in range(-10, 10):
            a, b = 2 * i + 1, 2 * j + 1
            yy, xx = y + (2 * l * (S * a + C * b) + d) // (2 * d), x + (2 * l * (C * a - S * b) + d) // (2 * d)
            hx = box_plain(P, yy - r, xx, 2 * r, r) - box_plain(P, yy - r, xx - r, 2 * r, r)
            hy = box_plain(P, yy, xx - r, r, 2 * r) - box_plain(P, yy - r, xx - r, r, 2 * r)
            dx, dy = C * hx + S * hy, -S * hx + C * hy
            wd = int(math.floor(4096 * math.exp(-(a * a + b * b) / 87.12) + 0.5))
            base = (4 * ((j + 10) // 5) + (i + 10) // 5) * 4
            v[base] += wd * dx; v[base + 1] += wd * dy; v[base + 2] += wd * abs(dx); v[base + 3] += wd * abs(dy)
    return v


def shifted(v):
    """(t, n2): t_d = v_d >> sh with sh = max(0, bitlength(max |v|) - 23), n2 = sum t_d^2 -- per row of an [n][64] int64 array."""
    M = np.abs(v).max(axis=1)
    sh = np.array([max(0, int(m).bit_length() - 23) for m in M], np.int64)
    t = v >> sh[:, None]
    return t, (t * t).sum(axis=1)


def normalise(v):
    """[n][64] float32."""
    t, n2 = shifted(v)
    root = np.sqrt(n2.astype(np.float64))                      # IEEE: correctly rounded
    out = np.zeros(v.shape, np.float32)
    nz = n2 > 0
    out[nz] = (t[nz].astype(np.float64) / root[nz, None]).astype(np.float32)
    return out


def sqrt_rounded(n):
    """The double nearest to sqrt(n) for an int n > 0, established in exact arithmetic."""
    s = math.sqrt(n)
    lo, hi = (Fraction(s) + Fraction(np.nextafter(s, 0.0))) / 2, (Fraction(s) + Fraction(np.nextafter(s, math.inf))) / 2
    assert lo * lo <= n <= hi * hi
    return s


def normalise_plain(v):
    M = max(abs(c) for c in v)
    sh = max(0, M.bit_length() - 23)
    t = [c >> sh for c in v]
    n2 = sum(c * c for c in t)
    if n2 == 0:
        return [np.float32(0)] * 64
    root = Fraction(sqrt_rounded(n2))
    return [np.float32(float(Fraction(c) / root)) for c in t]          # float(Fraction): correctly rounded; then one rounding to float


# ---- the whole contract ----------------------------------------------------------------------------------------------------
def extract(img, n_features=5000, n_octaves=4, hessian_threshold=100.0, upright=0):
    """dict: kp (KP_DTYPE records), desc [n, 64] float32, H [n] float64, bin [n] int32, moments [n, 2] int64, sums [n, 64] int64,
    candidates [n_octaves, 2] int32."""
    g = oo.gray(img)
    h, w = g.shape
    I = integral(g)
    ncand = np.zeros((n_octaves, 2), np.int32)
    parts = []
    for o in range(n_octaves):
        if _span(w, o, 1)[1] < _span(w, o, 1)[0] or _span(h, o, 1)[1] < _span(h, o, 1)[0]:
            break
        R = response_maps(I, o)
        for m in (1, 2):
            ys, xs, H = candidates(R, o, m, w, h, hessian_threshold)
            ncand[o, m - 1] = len(ys)
            parts.append((H, np.full(len(ys), o, np.int64), np.full(len(ys), m, np.int64), ys.astype(np.int64), xs.astype(np.int64)))
    cat = lambda k, dt: np.concatenate([p[k] for p in parts]).astype(dt) if parts else np.zeros(0, dt)
    H, oc, ly, ys, xs = cat(0, np.float64), cat(1, np.int64), cat(2, np.int64), cat(3, np.int64), cat(4, np.int64)
    keep = np.lexsort((xs, ys, ly, oc, -H))[:n_features]
    H, oc, ly, ys, xs = H[keep], oc[keep], ly[keep], ys[keep], xs[keep]
    n = len(keep)
    L = 3 * (2 ** (oc + 1) * (ly + 1) + 1)
    ls = L // 3
    lap = np.zeros(n, np.int64)
    for size in np.unique(L):
        k = L == size
        lap[k] = hessian(I, ys[k], xs[k], int(size))[1]
    if upright or n == 0:
        mx, my, bn = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    else:
        mx, my = moments(I, ys, xs, ls)
        bn = oo.bins(mx, my)
    v = sums(I, ys, xs, ls, bn) if n else np.zeros((0, 64), np.int64)
    kp = np.zeros(n, KP_DTYPE)
    kp["x"], kp["y"], kp["size"], kp["angle"], kp["response"] = xs, ys, L, 12 * bn, H.astype(np.float32)
    kp["octave"], kp["layer"], kp["laplacian"] = oc, ly, np.where(lap >= 0, 1, -1)
    return {"kp": kp, "desc": normalise(v) if n else np.zeros((0, 64), np.float32), "H": H, "bin": bn.astype(np.int32),
            "moments": np.stack([mx, my], axis=1), "sums": v, "candidates": ncand}
