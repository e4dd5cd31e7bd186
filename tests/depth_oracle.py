"""CPU restatement of sfmba_depth_sweep and sfmba_depth_fuse (the contract is in include/sfmba.h) -- TEST INFRASTRUCTURE ONLY (numpy).

The device is held to this file bit for bit (tests/test_gpu_depth_sweep.py), and so is csrc/depth_math.h compiled for the host
(tests/test_depth_oracle_cpu.py).  Coordinates are IEEE doubles with every operation on its own: the 3 x 3 products are written out
with Python floats (no `@`, no BLAS), the per-pixel expressions are numpy element-wise operations, which never fuse a product with a
sum.  The sweep is stated twice:

  sweep_direct    the window sums are sums over the (2r+1)^2 shifted copies of the sample image, and the winner is found the way a
                  lane of the kernel finds it: plane after plane, keeping the best cost, the cost before it and the cost after it;
  sweep_integral  the window sums come from integral images of whole warped images, the costs of all planes are kept, and the
                  winner is an argmax over the cost volume.

Allowed importers: tests/, tools/.
"""
import numpy as np

NO_SAMPLE = -1


def gray(img):
    img = np.asarray(img)
    if img.ndim == 2:
        return img.astype(np.int64)
    b, g, r = (img[..., i].astype(np.int64) for i in range(3))
    return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14


def _f32(a):
    """float32 values as Python floats (exact)."""
    return [float(v) for v in np.asarray(a, dtype=np.float32).reshape(-1)]


def k4_of(K):
    K = _f32(K)
    return [K[0], K[4], K[2], K[5]]


def mat3_mul(a, b):
    return [(a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)]


def mat3_vec(a, x):
    return [(a[3 * i] * x[0] + a[3 * i + 1] * x[1]) + a[3 * i + 2] * x[2] for i in range(3)]


def warp(k4, pr, ps):
    """A [9], b [3] of the contract's `warp` paragraph; k4 = fx, fy, cx, cy; pr, ps = 12 floats each."""
    fx, fy, cx, cy = k4
    RrT = [pr[4 * j + i] for i in range(3) for j in range(3)]
    Rs = [ps[4 * i + j] for i in range(3) for j in range(3)]
    tr, ts = [pr[3], pr[7], pr[11]], [ps[3], ps[7], ps[11]]
    Rrel = mat3_mul(Rs, RrT)
    Rt = mat3_vec(Rrel, tr)
    trel = [ts[i] - Rt[i] for i in range(3)]
    K = [fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0]
    Ki = [1.0 / fx, 0.0, -(cx / fx), 0.0, 1.0 / fy, -(cy / fy), 0.0, 0.0, 1.0]
    return mat3_mul(mat3_mul(K, Rrel), Ki), mat3_vec(K, trel)


def planes(z_near, z_far, D):
    wn, wf = 1.0 / float(np.float32(z_near)), 1.0 / float(np.float32(z_far))
    return wf, (wn - wf) / float(D - 1)


def plane_w(wf, step, k):
    return wf + float(k) * step


def project(A, b, us, vs, wk, ws, hs):
    """(valid, u', v') for arrays of reference pixel coordinates (float64)."""
    with np.errstate(all="ignore"):
        q = [((A[3 * i] * us + A[3 * i + 1] * vs) + A[3 * i + 2]) + wk * b[i] for i in range(3)]
        up, vp = q[0] / q[2], q[1] / q[2]
        valid = (q[2] > 0.0) & (up >= 0.0) & (up <= float(ws - 1)) & (vp >= 0.0) & (vp <= float(hs - 1))
    return valid, up, vp


def fix(c):
    return np.floor(16.0 * c + 0.5).astype(np.int64)


def sample(J, su, sv):
    hs, ws = J.shape
    x0, fx, y0, fy = su >> 4, su & 15, sv >> 4, sv & 15
    x1, y1 = np.minimum(x0 + 1, ws - 1), np.minimum(y0 + 1, hs - 1)
    return ((16 - fx) * (16 - fy) * J[y0, x0] + fx * (16 - fy) * J[y0, x1] + (16 - fx) * fy * J[y1, x0] + fx * fy * J[y1, x1] + 8) >> 4


def warped(J, A, b, wk, h, w):
    """The samples of source J (int64 gray) for every pixel of an h x w reference on the plane wk: int64 [h, w], NO_SAMPLE = invalid."""
    vs, us = np.mgrid[0:h, 0:w].astype(np.float64)
    valid, up, vp = project(A, b, us, vs, wk, J.shape[1], J.shape[0])
    su, sv = fix(np.where(valid, up, 0.0)), fix(np.where(valid, vp, 0.0))
    return np.where(valid, sample(J, su, sv), NO_SAMPLE)


def box_integral(a, r):
    h, w = a.shape
    n = 2 * r + 1
    out = np.zeros((h, w), np.int64)
    if h < n or w < n:
        return out
    S = np.zeros((h + 1, w + 1), np.int64)
    S[1:, 1:] = a.cumsum(0).cumsum(1)
    out[r:h - r, r:w - r] = S[n:, n:] - S[:-n, n:] - S[n:, :-n] + S[:-n, :-n]
    return out


def box_direct(a, r):
    h, w = a.shape
    n = 2 * r + 1
    out = np.zeros((h, w), np.int64)
    if h < n or w < n:
        return out
    for dy in range(n):
        for dx in range(n):
            out[r:h - r, r:w - r] += a[dy:dy + h - 2 * r, dx:dx + w - 2 * r]
    return out


def _reference(I, r, min_std, box):
    h, w = I.shape
    n = (2 * r + 1) ** 2
    inner = np.zeros((h, w), bool)
    if h > 2 * r and w > 2 * r:
        inner[r:h - r, r:w - r] = True
    SI, SII = box(I, r), box(I * I, r)
    varI = n * SII - SI * SI
    part = inner & (varI >= n * n * min_std * min_std) & (varI > 0)
    return n, SI, SII, varI, part


def _plane_cost(I, Js, ABs, wk, r, n, SI, varI, part, min_sources, box, debug=None):
    """(C float64 [h, w], valid bool [h, w]) of one plane; the scores are summed in list order starting from the first."""
    h, w = I.shape
    acc, cnt = np.zeros((h, w)), np.zeros((h, w), np.int64)
    for s, (J, (A, b)) in enumerate(zip(Js, ABs)):
        Jw = warped(J, A, b, wk, h, w)
        bad = box((Jw == NO_SAMPLE).astype(np.int64), r)
        Jz = np.where(Jw == NO_SAMPLE, 0, Jw)
        SJ, SJJ, SIJ = box(Jz, r), box(Jz * Jz, r), box(I * Jz, r)
        varJ = n * SJJ - SJ * SJ
        counts = part & (bad == 0) & (varJ > 0)
        with np.errstate(all="ignore"):
            sc = (n * SIJ - SI * SJ).astype(np.float64) / np.sqrt(varI.astype(np.float64) * varJ.astype(np.float64))
        acc = np.where(counts, np.where(cnt > 0, acc + sc, sc), acc)
        cnt = cnt + counts
        if debug is not None:
            debug.append(dict(s=s, J=Jw, all_valid=part & (bad == 0), counts=counts, SJ=SJ, SJJ=SJJ, SIJ=SIJ, score=np.where(counts, sc, 0.0)))
    valid = cnt >= min_sources
    with np.errstate(all="ignore"):
        C = np.where(valid, acc / np.maximum(cnt, 1).astype(np.float64), 0.0)
    return C, valid


def refine(cm, c0, cp):
    with np.errstate(all="ignore"):
        den = (cm - 2.0 * c0) + cp
        return np.where(den < 0.0, (0.5 * (cm - cp)) / np.where(den < 0.0, den, 1.0), 0.0)


def _finish(h, w, D, wf, step, have, best, best_k, use, cm, cp, min_score):
    delta = np.where(use, refine(cm, best, cp), 0.0)
    wv = (wf + best_k.astype(np.float64) * step) + delta * step
    accepted = have & (best >= float(np.float32(min_score)))
    with np.errstate(all="ignore"):
        depth = np.where(accepted, (1.0 / wv).astype(np.float32), np.float32(0.0)).astype(np.float32)
    score = np.where(have, best.astype(np.float32), np.float32(0.0)).astype(np.float32)
    plane = np.where(have, best_k, -1).astype(np.int16)
    return dict(depth=depth, score=score, plane=plane, cost=np.where(have, best, 0.0), delta=delta, accepted=accepted)


def _setup(images, K, P, job):
    ref, srcs, zn, zf = job
    k4 = k4_of(K)
    P = np.asarray(P, dtype=np.float32).reshape(-1, 12)
    I = gray(images[ref])
    Js = [gray(images[s]) for s in srcs]
    ABs = [warp(k4, _f32(P[ref]), _f32(P[s])) for s in srcs]
    return I, Js, ABs


def sweep_integral(images, K, P, job, n_planes=64, radius=3, min_std=2, min_score=0.6, min_sources=1, debug=False):
    I, Js, ABs = _setup(images, K, P, job)
    h, w = I.shape
    D, r = n_planes, radius
    wf, step = planes(job[2], job[3], D)
    n, SI, SII, varI, part = _reference(I, r, min_std, box_integral)
    C = np.full((D, h, w), -np.inf)
    ok = np.zeros((D, h, w), bool)
    dbg = []
    for k in range(D):
        rows = [] if debug else None
        c, v = _plane_cost(I, Js, ABs, plane_w(wf, step, k), r, n, SI, varI, part, min_sources, box_integral, rows)
        C[k], ok[k] = np.where(v, c, -np.inf), v
        if debug:
            dbg.append(rows)
    have = ok.any(0)
    best_k = C.argmax(0)                                   # the first of equal maxima: the lowest k
    take = lambda kk: np.take_along_axis(C, np.clip(kk, 0, D - 1)[None], 0)[0]
    best, cm, cp = take(best_k), take(best_k - 1), take(best_k + 1)
    use = have & (best_k > 0) & (best_k < D - 1) & np.isfinite(cm) & np.isfinite(cp)
    out = _finish(h, w, D, wf, step, have, np.where(have, best, 0.0), best_k, use, np.where(use, cm, 0.0), np.where(use, cp, 0.0), min_score)
    out.update(part=part, SI=SI, SII=SII, AB=ABs, wf=wf, step=step)
    if debug:
        out["planes"] = dbg
    return out


def sweep_direct(images, K, P, job, n_planes=64, radius=3, min_std=2, min_score=0.6, min_sources=1):
    I, Js, ABs = _setup(images, K, P, job)
    h, w = I.shape
    D, r = n_planes, radius
    wf, step = planes(job[2], job[3], D)
    n, SI, SII, varI, part = _reference(I, r, min_std, box_direct)
    have, take_next = np.zeros((h, w), bool), np.zeros((h, w), bool)
    pred_ok, succ_ok, prev_ok = (np.zeros((h, w), bool) for _ in range(3))
    best, pred, succ, prev = (np.zeros((h, w)) for _ in range(4))
    best_k = np.zeros((h, w), np.int64)
    for k in range(D):
        C, valid = _plane_cost(I, Js, ABs, plane_w(wf, step, k), r, n, SI, varI, part, min_sources, box_direct)
        succ, succ_ok = np.where(take_next, C, succ), np.where(take_next, valid, succ_ok)
        take_next = np.zeros((h, w), bool)
        new = valid & (~have | (C > best))
        have = have | new
        best, best_k = np.where(new, C, best), np.where(new, k, best_k)
        pred, pred_ok = np.where(new, prev, pred), np.where(new, prev_ok, pred_ok)
        take_next = new
        succ_ok = succ_ok & ~new
        prev, prev_ok = C, valid
    use = have & (best_k > 0) & (best_k < D - 1) & pred_ok & succ_ok
    out = _finish(h, w, D, wf, step, have, best, best_k, use, pred, succ, min_score)
    out.update(part=part)
    return out


def sweep(images, K, P, jobs, **params):
    """What capi.depth_sweep returns: one (depth, score, plane) per job."""
    outs = [sweep_integral(images, K, P, j, **params) for j in jobs]
    return [(o["depth"], o["score"], o["plane"]) for o in outs]


# ---- fuse -------------------------------------------------------------------------------------------------------------------
def unproject(k4, p, us, vs, z):
    fx, fy, cx, cy = k4
    xn, yn = (us - cx) / fx, (vs - cy) / fy
    d = [z * xn - p[3], z * yn - p[7], z - p[11]]
    return [(p[j] * d[0] + p[4 + j] * d[1]) + p[8 + j] * d[2] for j in range(3)]


def reproject(k4, p, X, ws, hs):
    """(inside, px, py, qz) for arrays of world points."""
    fx, fy, cx, cy = k4
    q = [((p[4 * i] * X[0] + p[4 * i + 1] * X[1]) + p[4 * i + 2] * X[2]) + p[4 * i + 3] for i in range(3)]
    with np.errstate(all="ignore"):
        x = np.floor(((fx * q[0]) / q[2] + cx) + 0.5)
        y = np.floor(((fy * q[1]) / q[2] + cy) + 0.5)
        inside = (q[2] > 0.0) & (x >= 0.0) & (x <= float(ws - 1)) & (y >= 0.0) & (y <= float(hs - 1))
    px, py = np.where(inside, x, 0.0).astype(np.int64), np.where(inside, y, 0.0).astype(np.int64)
    return inside, px, py, q[2]


def fuse(images, K, P, depth_maps, checks, rel_tol=0.01, min_consistent=1):
    """What capi.depth_fuse returns."""
    k4 = k4_of(K)
    P = np.asarray(P, dtype=np.float32).reshape(-1, 12)
    tol = float(np.float32(rel_tol))
    xyz, bgr, si, sp, pt_ptr = [], [], [], [], [0]
    for i, img in enumerate(images):
        img = np.asarray(img)
        m = depth_maps[i]
        if m is None:
            pt_ptr.append(pt_ptr[-1])
            continue
        h, w = img.shape[:2]
        z = np.asarray(m, dtype=np.float32).astype(np.float64)
        vs, us = np.mgrid[0:h, 0:w].astype(np.float64)
        has = z > 0.0
        X = unproject(k4, _f32(P[i]), us, vs, z)
        agree = np.zeros((h, w), np.int64)
        for s in checks[i]:
            if depth_maps[s] is None:
                continue
            ms = np.asarray(depth_maps[s], dtype=np.float32).astype(np.float64)
            inside, px, py, qz = reproject(k4, _f32(P[s]), X, ms.shape[1], ms.shape[0])
            zs = ms[py, px]
            with np.errstate(all="ignore"):
                agree += has & inside & (zs > 0.0) & (np.abs(zs - qz) <= tol * qz)
        keep = has & (agree >= min_consistent)
        yy, xx = np.nonzero(keep)                           # row-major: (row, column) order
        xyz.append(np.stack([X[j][yy, xx] for j in range(3)], axis=1).astype(np.float32))
        px_ = img[yy, xx]
        bgr.append(px_.astype(np.uint8) if img.ndim == 3 else np.repeat(px_[:, None], 3, axis=1).astype(np.uint8))
        si.append(np.full(len(yy), i, np.int32))
        sp.append((yy * w + xx).astype(np.int32))
        pt_ptr.append(pt_ptr[-1] + len(yy))
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)
    return {"xyz": cat(xyz, (0, 3), np.float32), "bgr": cat(bgr, (0, 3), np.uint8), "src_image": cat(si, (0,), np.int32),
            "src_pixel": cat(sp, (0,), np.int32), "pt_ptr": np.asarray(pt_ptr, np.int64)}


# ---- the host rules of SfM::densify (host/SfM.h) ----------------------------------------------------------------------------
def dense_jobs(poses, xyz, view_ptr, view_idx, good, max_sources=2):
    """[(ref, sources, z_near, z_far)] as SfM::densify makes them from its own poses [v, 12] (float32) and cloud."""
    P = [[float(x) for x in p] for p in np.asarray(poses, np.float32).reshape(-1, 12)]
    good = [int(v) for v in np.nonzero(np.asarray(good))[0]]
    centre = {v: [-((P[v][j] * P[v][3] + P[v][4 + j] * P[v][7]) + P[v][8 + j] * P[v][11]) for j in range(3)] for v in good}
    depths = {v: [] for v in good}
    pts = np.asarray(xyz, np.float32)
    for i in range(len(pts)):
        X = [float(c) for c in pts[i]]
        for v in view_idx[view_ptr[i]:view_ptr[i + 1]]:
            v = int(v)
            if v in depths:
                z = ((P[v][8] * X[0] + P[v][9] * X[1]) + P[v][10] * X[2]) + P[v][11]
                if np.isfinite(z) and z > 0.0:
                    depths[v].append(z)
    jobs = []
    for v in good:
        z = sorted(depths[v])
        m = len(z)
        others = []
        for o in good:
            if o != v:
                d = [centre[o][k] - centre[v][k] for k in range(3)]
                others.append(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], o))
        if m < 8 or not others:
            continue
        others.sort()
        jobs.append((v, [o for _, o in others[:max_sources]], float(np.float32(z[(5 * m) // 100] / 1.25)),
                     float(np.float32(z[min(m - 1, (95 * m) // 100)] * 1.25))))
    return jobs
