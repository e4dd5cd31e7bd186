"""CPU restatement of the baseline-pose contract (include/sfmba.h, sfmba_essential_ransac) -- TEST INFRASTRUCTURE ONLY.

The contract is this project's own (the seeded splitmix64 sample stream of sfmba_pnp_ransac with six entries, a five-point
essential matrix chosen by the sixth, an all-hypotheses consensus on the squared Sampson distance, recoverPose in closed form on the
winner's inliers, no refit); it is NOT the sample stream of cv::findEssentialMat.  Everything here is fp64 numpy and takes a different
route from the device where there is a choice:

  sample        Python ints, masked to 64 bits
  null space    numpy.linalg.svd of the 5 x 9 epipolar system (the device: Gauss-Jordan with complete pivoting + Gram-Schmidt)
  constraints   polynomial products by numpy.convolve on a Kronecker packing of the exponents (the device: unrolled index tables)
  solutions     the eigenvectors of the 10 x 10 action matrix for multiplication by x, monomial order x^3 x^2y xy^2 y^3 x^2z xyz
                y^2z xz^2 yz^2 z^3 | x^2 xy y^2 xz yz z^2 x y z 1 (the device: Nister's order, the degree-10 polynomial in z,
                Sturm's sequence and bisection); each real one polished by Newton on the 10 x 20 coefficient matrix with a
                least-squares step (the device: Gauss-Newton on the matrix form of the constraints, in its own chart)
  pose          the four candidates from numpy.linalg.svd, put into the contract's order by their defining property
                [t]x R(+t) = E = [-t]x R(-t) (the device: Horn's closed form, restated here as horn_candidates and held to the SVD
                set by tests/test_essential_oracle_cpu.py); depths by the 2 x 2 normal equations (the device: cross products)

Allowed importers: tests/ and tools/.
"""
import numpy as np

import pnp_oracle

M64 = (1 << 64) - 1
MAX_DEPTH = 50.0
# exponents (i, j, k) of x^i y^j z^k in the action-matrix order
MONOMIALS = [(3, 0, 0), (2, 1, 0), (1, 2, 0), (0, 3, 0), (2, 0, 1), (1, 1, 1), (0, 2, 1), (1, 0, 2), (0, 1, 2), (0, 0, 3),
             (2, 0, 0), (1, 1, 0), (0, 2, 0), (1, 0, 1), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
PACK = np.array([i + 4 * j + 16 * k for i, j, k in MONOMIALS])          # Kronecker packing: x -> s, y -> s^4, z -> s^16


def sample(seed, p, h, n):
    """The six sample indices of hypothesis h of pair p (None: invalid -- no six distinct indices in 64 draws)."""
    if n < 6:
        return None
    key = pnp_oracle.mix((seed + p) & M64)
    got = []
    for k in range(64):
        i = pnp_oracle.mix(key ^ ((h << 8) | k)) % n
        if i not in got:
            got.append(i)
            if len(got) == 6:
                return got
    return None


def intrinsics(K):
    K = np.asarray(K, np.float64).reshape(3, 3)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def normalise(pts, K):
    fx, fy, cx, cy = intrinsics(K)
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    return np.stack([(pts[:, 0] - cx) / fx, (pts[:, 1] - cy) / fy], axis=1)


def _lin(c):
    """The packed polynomial c[0] x + c[1] y + c[2] z + c[3]."""
    out = np.zeros(17)
    out[1], out[4], out[16], out[0] = c[0], c[1], c[2], c[3]
    return out


def constraint_matrix(basis):
    """The 10 x 20 system of det E = 0 and 2 E E^T E - tr(E E^T) E = 0 on E = x B0 + y B1 + z B2 + B3 (basis [4, 9])."""
    e = [[_lin(basis[:, 3 * r + c]) for c in range(3)] for r in range(3)]
    mul = np.convolve
    det = (mul(e[0][0], mul(e[1][1], e[2][2]) - mul(e[1][2], e[2][1])) - mul(e[0][1], mul(e[1][0], e[2][2]) - mul(e[1][2], e[2][0]))
           + mul(e[0][2], mul(e[1][0], e[2][1]) - mul(e[1][1], e[2][0])))
    eet = [[sum(mul(e[i][k], e[j][k]) for k in range(3)) for j in range(3)] for i in range(3)]
    tr = eet[0][0] + eet[1][1] + eet[2][2]
    rows = [det]
    for i in range(3):
        for j in range(3):
            rows.append(2.0 * sum(mul(eet[i][k], e[k][j]) for k in range(3)) - mul(tr, e[i][j]))
    return np.stack([r[PACK] for r in rows])


EXPONENTS = np.array(MONOMIALS, float)


def polish(M, xyz, steps=3):
    """Newton on the ten constraints M m(x, y, z) = 0 from the eigenvector's solution, by least squares on the 10 x 3 Jacobian: the
    eigenvector carries the conditioning of the action matrix, the constraints themselves only that of the solution."""
    xyz = np.array(xyz, float)
    for _ in range(steps):
        with np.errstate(all="ignore"):
            mono = np.prod(xyz ** EXPONENTS, axis=1)
            J = np.zeros((20, 3))
            for v in range(3):
                e = EXPONENTS.copy()
                e[:, v] = np.maximum(e[:, v] - 1, 0)
                J[:, v] = EXPONENTS[:, v] * np.prod(xyz ** e, axis=1)
        if not (np.all(np.isfinite(mono)) and np.all(np.isfinite(J))):
            break
        step = np.linalg.lstsq(M @ J, -(M @ mono), rcond=None)[0]
        if not np.all(np.isfinite(step)):
            break
        xyz = xyz + step
    return xyz


def sampson2(E, xl, xr):
    """Squared Sampson distance of xl -> xr ([n, 2] each) under E, in the units of the points."""
    xl, xr = np.asarray(xl, np.float64).reshape(-1, 2), np.asarray(xr, np.float64).reshape(-1, 2)
    E = np.asarray(E, np.float64).reshape(3, 3)
    pl = np.concatenate([xl, np.ones((len(xl), 1))], axis=1)
    pr = np.concatenate([xr, np.ones((len(xr), 1))], axis=1)
    a, b = pl @ E.T, pr @ E
    e = (pr * a).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return e * e / (a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)


def fix_sign(E):
    E = np.asarray(E, np.float64).reshape(3, 3)
    v = E.ravel()[np.argmax(np.abs(E.ravel()))]
    return -E if v < 0 else E


def hypothesis(xl6, xr6):
    """The contract's hypothesis from six NORMALISED correspondences: (E [3,3] or None, nsol, info).  info: cond (of the eliminated
    10 x 10 block), gap (relative, between the best and the second-best sixth-point distance), imag (the smallest distance from
    real among the solutions not taken as real, on the unit-norm E), sep (the smallest distance between two real solutions' E)."""
    xl6, xr6 = np.asarray(xl6, np.float64).reshape(6, 2), np.asarray(xr6, np.float64).reshape(6, 2)
    info = dict(cond=np.inf, gap=np.inf, imag=np.inf, sep=np.inf)
    A = np.stack([np.kron([u, v, 1.0], [x, y, 1.0]) for (x, y), (u, v) in zip(xl6[:5], xr6[:5])])
    if not np.all(np.isfinite(A)):
        return None, 0, info
    _, sv, vt = np.linalg.svd(A)
    if not sv[4] > 1e-12 * sv[0]:
        info["cond"] = np.inf
        return None, 0, info
    basis = vt[5:9]
    M = constraint_matrix(basis)
    info["cond"] = np.linalg.cond(M[:, :10])
    if not info["cond"] < 1e15:
        return None, 0, info
    B = np.linalg.solve(M[:, :10], M[:, 10:])
    act = np.zeros((10, 10))
    for row, src in ((0, 0), (1, 1), (2, 2), (3, 4), (4, 5), (5, 7)):      # x * (x^2 xy y^2 xz yz z^2) = a cubic monomial
        act[row] = -B[src]
    act[6, 0] = act[7, 1] = act[8, 3] = act[9, 6] = 1.0                      # x * (x y z 1) = x^2 xy xz x
    lam, vec = np.linalg.eig(act)
    sols, imag = [], []
    for k in range(10):
        v = vec[:, k]
        with np.errstate(divide="ignore", invalid="ignore"):
            xyz = v[6:9] / v[9]
            if lam[k].imag == 0.0 and np.all(np.isfinite(xyz)):
                xyz = polish(M, xyz.real)
            Ec = (xyz[0] * basis[0] + xyz[1] * basis[1] + xyz[2] * basis[2] + basis[3])
            Ec = Ec * (np.sqrt(2.0) / np.linalg.norm(Ec))
        if not np.all(np.isfinite(Ec)):
            continue
        if lam[k].imag == 0.0 and np.abs(Ec.imag).max() == 0.0:
            sols.append(fix_sign(Ec.real))
        else:
            ph = Ec.ravel()[np.argmax(np.abs(Ec.ravel()))]
            imag.append(np.abs((Ec * (abs(ph) / ph)).imag).max())
    if imag:
        info["imag"] = float(min(imag))
    if len(sols) > 1:
        info["sep"] = float(min(np.abs(a - b).max() for i, a in enumerate(sols) for b in sols[i + 1:]))
    d = np.array([sampson2(E, xl6[5], xr6[5])[0] for E in sols])
    keep = np.isfinite(d)
    sols, d = [E for E, k in zip(sols, keep) if k], d[keep]
    if not sols:
        return None, 0, info
    order = np.argsort(d, kind="stable")
    if len(d) > 1:
        info["gap"] = float((d[order[1]] - d[order[0]]) / max(d[order[1]], 1e-300))
    return sols[order[0]], len(sols), info


def ill_conditioned(info):
    """The rule of tests/test_gpu_essential_ransac.py: the verdict then hangs on the last bits of an intermediate."""
    return bool(info["cond"] > 1e10 or info["gap"] < 1e-6 or info["imag"] < 1e-6 or info["sep"] < 1e-6)


def hypotheses(left, right, K, n_hyp, seed=0, p=0):
    """[(sample or None, E or None, nsol, info)] for h = 0 .. n_hyp - 1 over the aligned correspondences left -> right (pixels)."""
    xl, xr = normalise(left, K), normalise(right, K)
    out = []
    for h in range(n_hyp):
        s = sample(seed, p, h, len(xl))
        if s is None:
            out.append((None, None, 0, dict(cond=np.inf, gap=np.inf, imag=np.inf, sep=np.inf)))
            continue
        E, nsol, info = hypothesis(xl[s], xr[s])
        out.append((s, E, nsol, info))
    return out


def pixel_matrix(E, K):
    """F on centred pixels: diag(1/fx, 1/fy, 1) E diag(1/fx, 1/fy, 1)."""
    fx, fy, _, _ = intrinsics(K)
    D = np.diag([1.0 / fx, 1.0 / fy, 1.0])
    return D @ np.asarray(E, np.float64).reshape(3, 3) @ D


def sampson_px(E, left, right, K):
    """Sampson distance in pixels [n] (fp64)."""
    _, _, cx, cy = intrinsics(K)
    c = np.array([cx, cy])
    with np.errstate(invalid="ignore"):
        return np.sqrt(sampson2(pixel_matrix(E, K), np.asarray(left, np.float64) - c, np.asarray(right, np.float64) - c))


def inlier_mask(E, left, right, K, threshold_px):
    with np.errstate(invalid="ignore"):
        return sampson_px(E, left, right, K) <= float(threshold_px)


def border_points(E, left, right, K, threshold_px, margin=5e-3):
    """The correspondences [n] bool whose fp64 Sampson distance lies within `margin` px of the threshold (a float decision may
    differ there)."""
    with np.errstate(invalid="ignore"):
        return np.abs(sampson_px(E, left, right, K) - float(threshold_px)) <= margin


def inlier_mask_device(E, left, right, K, threshold_px):
    """The device's decision (csrc/essential_math.h, ess_inlier) emulated in numpy without fused multiply-adds: centred pixels as
    float32 hold them, the residual in fp64, the gradient sum in float32."""
    fx, fy, cx, cy = intrinsics(K)
    E = np.asarray(E, np.float64).reshape(3, 3)
    G = E * np.array([[fy / fx, 1.0, fy], [1.0, fx / fy, fx], [fy, fx, fx * fy]])
    g = G.astype(np.float32)
    f = np.float32
    L, R = np.asarray(left, np.float32), np.asarray(right, np.float32)
    x, y, u, v = L[:, 0] - f(cx), L[:, 1] - f(cy), R[:, 0] - f(cx), R[:, 1] - f(cy)
    xd, yd, ud, vd = (a.astype(np.float64) for a in (x, y, u, v))
    a0, a1, a2 = G[0, 0] * xd + (G[0, 1] * yd + G[0, 2]), G[1, 0] * xd + (G[1, 1] * yd + G[1, 2]), G[2, 0] * xd + (G[2, 1] * yd + G[2, 2])
    e = ud * a0 + (vd * a1 + a2)
    a0f, a1f = a0.astype(np.float32), a1.astype(np.float32)
    b0, b1 = g[0, 0] * u + (g[1, 0] * v + g[2, 0]), g[0, 1] * u + (g[1, 1] * v + g[2, 1])
    s = a0f * a0f + (a1f * a1f + (b0 * b0 + b1 * b1))
    return (s > 0) & (e * e <= (f(threshold_px) * f(threshold_px) * s).astype(np.float64))


def cross_matrix(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def horn_candidates(E, transposed_cofactor=False):
    """Horn 1990 in closed form, as the contract states it: [(R, t)] x 4 in the contract's order, or None."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    A = E @ E.T
    T = 0.5 * np.trace(A) * np.eye(3) - A
    c = int(np.argmax(np.diag(T)))                                           # the first maximum
    if not T[c, c] > 0:
        return None
    t = T[:, c] / np.sqrt(T[c, c])
    cof = np.stack([np.cross(E[1], E[2]), np.cross(E[2], E[0]), np.cross(E[0], E[1])])
    if transposed_cofactor:
        cof = cof.T
    Rp, Rm = cof - cross_matrix(t) @ E, cof + cross_matrix(t) @ E
    return [(Rp, t), (Rm, -t), (Rm, t), (Rp, -t)]


def svd_candidates(E):
    """The textbook decomposition: [(R, t)] x 4 in the contract's order, t's sign and the order fixed by the contract's defining
    properties (t = the column of 1/2 tr(E E^T) I - E E^T with the largest diagonal, normalised; [t]x R(+t) = E = [-t]x R(-t))."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    Rs = [U @ W @ Vt, U @ W.T @ Vt]
    t = U[:, 2]
    T = 0.5 * np.trace(E @ E.T) * np.eye(3) - E @ E.T
    c = int(np.argmax(np.diag(T)))
    if t[c] < 0:
        t = -t
    scale = np.linalg.norm(E) / np.sqrt(2.0)
    Rp = min(Rs, key=lambda R: np.abs(cross_matrix(t) @ R * scale - E).max())
    Rm = min(Rs, key=lambda R: np.abs(cross_matrix(-t) @ R * scale - E).max())
    return [(Rp, t), (Rm, -t), (Rm, t), (Rp, -t)]


def depths(R, t, xl, xr):
    """Least-squares depths (lambda, lambda', determinant of the 2 x 2 normal equations) of lambda' x' = lambda R x + t [n each]."""
    xl, xr = np.asarray(xl, np.float64).reshape(-1, 2), np.asarray(xr, np.float64).reshape(-1, 2)
    a = np.concatenate([xl, np.ones((len(xl), 1))], axis=1) @ np.asarray(R).T
    b = np.concatenate([xr, np.ones((len(xr), 1))], axis=1)
    # minimise |lambda' b - lambda a - t|^2 over (lambda, lambda')
    aa, ab, bb = (a * a).sum(1), (a * b).sum(1), (b * b).sum(1)
    at, bt = a @ t, b @ t
    det = aa * bb - ab * ab
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = (-at * bb + ab * bt) / det
        lamp = (aa * bt - ab * at) / det
    return lam, lamp, det


def in_front(R, t, xl, xr):
    lam, lamp, det = depths(R, t, xl, xr)
    with np.errstate(invalid="ignore"):
        return (det > 0) & (lam > 0) & (lam < MAX_DEPTH) & (lamp > 0) & (lamp < MAX_DEPTH)


def depth_border(R, t, xl, xr):
    """[n] bool: a depth within 1e-9 relative of 0 or 50, or a determinant below 1e-12 (the verdict may differ there)."""
    lam, lamp, det = depths(R, t, xl, xr)
    with np.errstate(invalid="ignore"):
        near = lambda v: (np.abs(v) <= 1e-9) | (np.abs(v - MAX_DEPTH) <= 1e-9 * MAX_DEPTH)
        return ~(det >= 1e-12) | near(lam) | near(lamp) | ~np.isfinite(lam) | ~np.isfinite(lamp)


def recover_pose(E, left, right, K, mask, candidates=svd_candidates):
    """recoverPose of the contract on the correspondences of `mask`: dict(pose_candidate, pose [3,4], counts [4], front [n] bool for
    the chosen candidate, border [n] bool = points of the mask on a depth border for ANY candidate), or None when there are no
    candidates."""
    cands = candidates(E)
    if cands is None:
        return None
    xl, xr = normalise(left, K), normalise(right, K)
    fronts = [in_front(R, t, xl, xr) & mask for R, t in cands]
    border = np.zeros(len(xl), bool)
    for R, t in cands:
        border |= depth_border(R, t, xl, xr) & mask
    counts = np.array([int(f.sum()) for f in fronts])
    k = int(np.argmax(counts))                                               # the first maximum
    R, t = cands[k]
    return dict(pose_candidate=k, pose=np.concatenate([R, t[:, None]], axis=1), counts=counts, front=fronts[k], fronts=fronts, border=border)


def scene_arrays(scene, seed, extra=7):
    """A scene of make_essential_scene as the C ABI takes a pair: (pts_left, pts_right, query_idx, train_idx).  The key points of
    each image are the scene's points in a shuffled order, with `extra` unmatched key points mixed in, so that
    pts_left[query_idx[i]] == scene["left"][i] and pts_right[train_idx[i]] == scene["right"][i] only through the index arrays."""
    rng = np.random.default_rng([int(seed), 78])
    out = []
    for side in ("left", "right"):
        pts = scene[side]
        n = len(pts)
        slot = rng.permutation(n + extra)[:n]
        img = rng.uniform(0, 700, (n + extra, 2)).astype(np.float32)
        img[slot] = pts
        out += [img, slot.astype(np.int32)]
    return out[0], out[2], out[1], out[3]


def essential_ransac(left, right, K, n_hyp=128, threshold_px=1.0, seed=0, p=0):
    """The whole contract for one pair of aligned correspondences: dict(status, best_hypothesis, n_inliers, n_pose_inliers,
    pose_candidate, n_matches, E, pose, inlier (the final mask), winner_mask (before the pose), hyp (the list of hypotheses()),
    hyp_count, hyp_nsol)."""
    left = np.asarray(left, np.float64).reshape(-1, 2)
    right = np.asarray(right, np.float64).reshape(-1, 2)
    n = len(left)
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    out = dict(status=1, best_hypothesis=-1, n_inliers=0, n_pose_inliers=0, pose_candidate=-1, n_matches=n, E=np.zeros((3, 3)), pose=eye,
               inlier=np.zeros(n, bool), winner_mask=np.zeros(n, bool), hyp=[], hyp_count=np.full(n_hyp, -1, np.int64),
               hyp_nsol=np.zeros(n_hyp, np.int64))
    if n < 6:
        return out
    hyp = hypotheses(left, right, K, n_hyp, seed, p)
    counts = np.array([-1 if E is None else int(inlier_mask(E, left, right, K, threshold_px).sum()) for _, E, _, _ in hyp], np.int64)
    out.update(hyp=hyp, hyp_count=counts, hyp_nsol=np.array([ns for _, _, ns, _ in hyp], np.int64))
    if counts.max() < 0:
        out["status"] = 2
        return out
    best = int(np.argmax(counts))                                            # the first maximum: ties go to the lowest h
    E = hyp[best][1]
    mask = inlier_mask(E, left, right, K, threshold_px)
    out.update(status=3, best_hypothesis=best, n_inliers=int(mask.sum()), E=E, winner_mask=mask)
    rp = recover_pose(E, left, right, K, mask)
    if rp is None or rp["counts"].max() == 0:
        return out
    out.update(status=0, pose_candidate=rp["pose_candidate"], pose=rp["pose"], inlier=rp["front"], n_pose_inliers=int(rp["front"].sum()))
    return out
