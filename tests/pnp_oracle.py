"""CPU restatement of the pose contract (include/sfmba.h, sfmba_pnp_ransac) -- TEST INFRASTRUCTURE ONLY.

The contract is this project's own (a seeded splitmix64 sample stream, P3P + fourth-point disambiguation, an all-hypotheses
consensus, Gauss-Newton on the winner's inliers); it is NOT the sample stream of cv::solvePnPRansac.  Everything here is
fp64 numpy and takes a different route from the device where there is a choice:

  sample       the same integer arithmetic (Python ints, masked to 64 bits)
  P3P          Grunert's quartic in v = s3 / s1 -- the resultant of the two quadratics in u = s2 / s1 that the three distance
               equations leave -- built with numpy polynomial arithmetic and solved with numpy.roots (companion-matrix eigenvalues;
               the device solves it in closed form), each real root polished by Newton on the quartic
  pose         Kabsch / SVD alignment of the three camera-frame points with the three world points (the device builds two
               orthonormal triads)
  refine       Gauss-Newton with numpy.linalg.solve on the normal equations (the device: fixed-order sums + 6x6 Cholesky)

Allowed importers: tests/ and tools/.
"""
import numpy as np

M64 = (1 << 64) - 1
REAL_ROOT_TOL = 1e-7          # a root of numpy.roots counts as real when |imag| <= this * max(1, |real|)


def mix(z):
    """splitmix64's output function (with its increment), mod 2^64."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample(seed, p, h, n):
    """The four sample indices of hypothesis h of problem p (None: invalid -- no four distinct indices in 64 draws)."""
    if n < 4:
        return None
    key = mix((seed + p) & M64)
    got = []
    for k in range(64):
        i = mix(key ^ ((h << 8) | k)) % n
        if i not in got:
            got.append(i)
            if len(got) == 4:
                return got
    return None


def intrinsics(K):
    K = np.asarray(K, np.float64).reshape(3, 3)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def project(pose, X, K):
    """(uv [n,2], depth [n]) of world points X under pose [3,4] = [R|t]."""
    fx, fy, cx, cy = intrinsics(K)
    pose = np.asarray(pose, np.float64).reshape(3, 4)
    pc = np.asarray(X, np.float64) @ pose[:, :3].T + pose[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], axis=1)
    return uv, pc[:, 2]


def pixel_errors(pose, X, uv, K):
    """(error in px [n], depth [n]) in fp64."""
    proj, z = project(pose, X, K)
    return np.sqrt(((proj - np.asarray(uv, np.float64)) ** 2).sum(axis=1)), z


def inlier_mask(pose, X, uv, K, threshold_px):
    err, z = pixel_errors(pose, X, uv, K)
    with np.errstate(invalid="ignore"):
        return (z > 0) & (err * err <= float(threshold_px) ** 2)


def border_points(pose, X, uv, K, threshold_px, margin=5e-3):
    """Number of points whose fp64 pixel error lies within `margin` px of the threshold (a float decision may differ there)."""
    err, z = pixel_errors(pose, X, uv, K)
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero((np.abs(err - threshold_px) <= margin) | (np.abs(z) <= 1e-6)))


def _kabsch(Xw, Yc):
    """R, t with Yc ~ R Xw + t (three points: an exact fit when the triangles are congruent)."""
    mx, my = Xw.mean(axis=0), Yc.mean(axis=0)
    H = (Yc - my).T @ (Xw - mx)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, my - R @ mx


def p3p(X3, uv3, K):
    """All P3P solutions [R|t] (a list of [3,4]) for three correspondences, through Grunert's quartic and numpy.roots."""
    fx, fy, cx, cy = intrinsics(K)
    X3 = np.asarray(X3, np.float64)
    uv3 = np.asarray(uv3, np.float64)
    f = np.stack([(uv3[:, 0] - cx) / fx, (uv3[:, 1] - cy) / fy, np.ones(3)], axis=1)
    f /= np.linalg.norm(f, axis=1)[:, None]
    c12, c13, c23 = f[0] @ f[1], f[0] @ f[2], f[1] @ f[2]
    d12, d13, d23 = ((X3[0] - X3[1]) ** 2).sum(), ((X3[0] - X3[2]) ** 2).sum(), ((X3[1] - X3[2]) ** 2).sum()
    if d12 == 0 or d13 == 0 or d23 == 0:
        return []
    P = np.polynomial.polynomial
    A, B = d12 / d13, d23 / d13
    w = np.array([1.0, -2 * c13, 1.0])                      # s1^2 w(v) = d13
    # u^2 + p1 u + p0 = 0 and u^2 + q1 u + q0 = 0, coefficients polynomials in v (low -> high)
    p1, p0 = np.array([-2 * c12]), P.polysub([1.0], A * w)
    q1, q0 = np.array([0.0, -2 * c23]), P.polysub([0.0, 0.0, 1.0], B * w)
    E, F, G = P.polysub(q0, p0), P.polysub(q1, p1), P.polysub(P.polymul(p1, q0), P.polymul(p0, q1))
    quartic = P.polysub(P.polymul(E, E), P.polymul(F, G))
    quartic = np.concatenate([quartic, np.zeros(5 - len(quartic))])
    if not np.all(np.isfinite(quartic)) or quartic[4] == 0:
        return []
    dq = P.polyder(quartic)
    out = []
    for r in np.roots(quartic[::-1]):
        if abs(r.imag) > REAL_ROOT_TOL * max(1.0, abs(r.real)):
            continue
        v = r.real
        for _ in range(3):
            d = P.polyval(v, dq)
            if d == 0:
                break
            v -= P.polyval(v, quartic) / d
        Fv = P.polyval(v, F)
        wv = P.polyval(v, w)
        if Fv == 0 or not wv > 0:
            continue
        u = -P.polyval(v, E) / Fv
        s1 = np.sqrt(d13 / wv)
        Y = np.stack([s1 * f[0], u * s1 * f[1], v * s1 * f[2]])
        R, t = _kabsch(X3, Y)
        pose = np.concatenate([R, t[:, None]], axis=1)
        if np.all(np.isfinite(pose)):
            out.append(pose)
    return out


def hypothesis(X4, uv4, K):
    """The contract's hypothesis from four correspondences: (pose [3,4] or None, info).  info: fourth-point errors of the
    admissible solutions (ascending), the worst reprojection error of the kept pose on its three sample points."""
    X4 = np.asarray(X4, np.float64)
    uv4 = np.asarray(uv4, np.float64)
    cands = []
    for pose in p3p(X4[:3], uv4[:3], K):
        err, z = pixel_errors(pose, X4, uv4, K)
        if np.all(z > 0) and np.isfinite(err[3]):
            cands.append((err[3], err[:3].max(), pose))
    if not cands:
        return None, dict(e4=[], residual=np.inf)
    cands.sort(key=lambda c: c[0])
    return cands[0][2], dict(e4=[c[0] for c in cands], residual=cands[0][1])


def ill_conditioned(info):
    """The rule of tests/test_gpu_pnp_ransac.py: the oracle's own residual is above 1e-4 px, or its two best fourth-point
    errors are closer than 0.01 px."""
    e4 = info["e4"]
    return bool(e4) and (info["residual"] > 1e-4 or (len(e4) > 1 and e4[1] - e4[0] < 0.01))


def hypotheses(X, uv, K, n_hyp, seed=0, p=0):
    """[(sample or None, pose or None, info)] for h = 0 .. n_hyp - 1."""
    X = np.asarray(X, np.float64)
    uv = np.asarray(uv, np.float64)
    out = []
    for h in range(n_hyp):
        s = sample(seed, p, h, len(X))
        if s is None:
            out.append((None, None, dict(e4=[], residual=np.inf)))
            continue
        pose, info = hypothesis(X[s], uv[s], K)
        out.append((s, pose, info))
    return out


def _exp_so3(w):
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-8:
        return np.eye(3) + W + 0.5 * W @ W
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W


def residuals(pose, X, uv, K):
    proj, _ = project(pose, X, K)
    return (proj - np.asarray(uv, np.float64)).reshape(-1)


def cost(pose, X, uv, K):
    r = residuals(pose, X, uv, K)
    return 0.5 * float(r @ r)


def jacobian(pose, X, K):
    """d(residual) / d(omega, t) for the update R <- exp([omega]x) R, t <- t + dt: [2n, 6]."""
    fx, fy, _, _ = intrinsics(K)
    pose = np.asarray(pose, np.float64).reshape(3, 4)
    q = np.asarray(X, np.float64) @ pose[:, :3].T            # R X
    pc = q + pose[:, 3]
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    n = len(q)
    dp = np.zeros((n, 2, 3))
    dp[:, 0, 0] = fx / z; dp[:, 0, 2] = -fx * x / z ** 2
    dp[:, 1, 1] = fy / z; dp[:, 1, 2] = -fy * y / z ** 2
    skew = np.zeros((n, 3, 3))                              # d(omega x q)/d omega = -[q]x
    skew[:, 0, 1] = q[:, 2]; skew[:, 0, 2] = -q[:, 1]
    skew[:, 1, 0] = -q[:, 2]; skew[:, 1, 2] = q[:, 0]
    skew[:, 2, 0] = q[:, 1]; skew[:, 2, 1] = -q[:, 0]
    J = np.concatenate([dp @ skew, dp], axis=2)
    return J.reshape(2 * n, 6)


def refine(pose0, X, uv, K, max_iters=20):
    """Gauss-Newton on pixel reprojection: (pose [3,4], cost, iters, status 0 / 3).  Stops when |delta| < 1e-12."""
    pose0 = np.asarray(pose0, np.float64).reshape(3, 4)
    X = np.asarray(X, np.float64)
    uv = np.asarray(uv, np.float64)
    pose, iters = pose0.copy(), 0
    if len(X) >= 4:
        while iters < max_iters:
            r, J = residuals(pose, X, uv, K), jacobian(pose, X, K)
            try:
                delta = np.linalg.solve(J.T @ J, -J.T @ r)
            except np.linalg.LinAlgError:
                return pose0, cost(pose0, X, uv, K), 0, 3
            if not np.all(np.isfinite(delta)):
                return pose0, cost(pose0, X, uv, K), 0, 3
            pose = np.concatenate([_exp_so3(delta[:3]) @ pose[:, :3], (pose[:, 3] + delta[3:])[:, None]], axis=1)
            iters += 1
            if np.linalg.norm(delta) < 1e-12:
                break
    return pose, cost(pose, X, uv, K), iters, 0


def pnp_ransac(X, uv, K, n_hyp=100, threshold_px=10.0, seed=0, p=0, max_refine_iters=20):
    """The whole contract for one problem: dict(status, best_hypothesis, n_inliers, refine_iters, refine_cost, pose,
    inlier, hyp (the list of hypotheses()), hyp_count)."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    n = len(X)
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    out = dict(status=1, best_hypothesis=-1, n_inliers=0, refine_iters=0, refine_cost=0.0, pose=ident,
               inlier=np.zeros(n, bool), hyp=[], hyp_count=np.full(n_hyp, -1, np.int64))
    if n < 4:
        return out
    hyp = hypotheses(X, uv, K, n_hyp, seed, p)
    counts = np.array([-1 if pose is None else int(inlier_mask(pose, X, uv, K, threshold_px).sum()) for _, pose, _ in hyp], np.int64)
    out.update(hyp=hyp, hyp_count=counts)
    if counts.max() < 0:
        out["status"] = 2
        return out
    best = int(np.argmax(counts))                           # the first maximum: ties go to the lowest h
    mask = inlier_mask(hyp[best][1], X, uv, K, threshold_px)
    pose, status, iters = hyp[best][1], 0, 0
    if max_refine_iters > 0 and mask.sum() >= 4:
        pose, _, iters, status = refine(pose, X[mask], uv[mask], K, max_refine_iters)
    out.update(status=status, best_hypothesis=best, n_inliers=int(mask.sum()), refine_iters=iters,
               refine_cost=cost(pose, X[mask], uv[mask], K), pose=pose, inlier=mask)
    return out
