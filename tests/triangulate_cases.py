"""Named two-view geometries for sfmba_triangulate and a long-double reference of triangulateViews -- TEST INFRASTRUCTURE ONLY.

The reference follows oracle/triangulate_oracle.py step by step (the same float containers: normalised pixels, the homogeneous
vector, the point, the projected pixels) and differs in ONE step: the null vector of the 4 x 4 DLT matrix comes from a one-sided
(Hestenes) Jacobi iteration in np.longdouble that runs until no column pair is left to rotate, not from LAPACK in fp64 and not for a
fixed number of sweeps.  It also hands back what the tests need to decide where a comparison of points is meaningful: the four
singular values and the float homogeneous vector of every match.

A match is CONDITIONED when (sigma_3 - sigma_4) / sigma_1 >= 1e-6 (the null vector is determined: below that, fp64 rounding of the
matrix alone turns it by more than a float ulp) and |w| >= 1e-6 |X_h| (the division by w does not amplify the float rounding of w
into the point).  Points are compared on conditioned matches only; errors and keep decisions are checked on every match.

Every case has N = 4159 matches (16 blocks of 256 lanes and 63: the last block of k_triangulate is partial), 0.5 px of noise on
both pixels and 10 % planted mismatches (40 px on the right pixel), from a fixed seed.

Allowed importers: tests/.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not the 80-bit extended type here: the reference would be no better than the device"

N = 16 * 256 + 63
K_DEFAULT = (2500.0, 2500.0, 512.0, 384.0)
K_BIG = (3500.0, 3400.0, 2048.0, 1536.0)                 # 4096 x 3072 pixels, fx != fy
ROTVEC = np.array([0.02, -0.15, 0.01])                   # the pair of tests/test_gpu_triangulate.py: 0.15 rad, unit baseline
TRANS = np.array([-1.0, 0.02, 0.1])
GAP_MIN = 1e-6
W_MIN = 1e-6
MAX_LEFT_OUT = 0.01
# general_far_origin: sigma_1 of the DLT matrix grows with the distance of the origin (its fourth column is the translation) while
# sigma_3 does not, so (sigma_3 - sigma_4) / sigma_1 falls with it: at 10^4 x the rule above leaves out EVERY match (the largest ratio
# is 5e-8), at 10^3 x 73 %, at 10^2 x none (the smallest ratio is 4.7e-6).  The origin is about 10^4 units away then, a float ulp of
# a coordinate is 1e-3 units = 0.4 px at these depths, which a 1 px threshold feels.
FAR_ORIGIN = 1e2
SEEDS = {name: 100 + i for i, name in enumerate(
    ("base1", "base1e-2", "base1e-3", "base1e-4", "forward", "rot90", "rot180", "general", "general_far_origin", "far",
     "pure_rotation", "big_image", "behind"))}
CASES = tuple(SEEDS)


def rotvec_to_matrix(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th == 0:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W


def k_matrix(k):
    fx, fy, cx, cy = k
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def project64(K, P, X):
    """Pixels of X [n,3] under P [3,4] and K [3,3], everything taken to fp64 as it stands."""
    K, P, X = np.asarray(K).astype(np.float64), np.asarray(P).astype(np.float64), np.asarray(X).astype(np.float64)
    p = X @ P[:, :3].T + P[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]], axis=1)


def make_case(name):
    """dict(name, K [3,3] f32, P_left / P_right [3,4] f32, left / right [N,2] f32, bad [N] bool, X [N,3] f64 world points).
    The pixels are the projections under the float matrices the device is given, plus noise."""
    rng = np.random.default_rng(SEEDS[name])
    k = K_BIG if name == "big_image" else K_DEFAULT
    K = k_matrix(k)
    Rl, tl = np.eye(3), np.zeros(3)
    Rr, tr = rotvec_to_matrix(ROTVEC), TRANS.copy()
    depth = rng.uniform(4.0, 8.0, N)
    if name.startswith("base"):
        b = float(name[4:])                              # baseline length, the rotation shrunk with it
        Rr, tr = rotvec_to_matrix(ROTVEC * b), TRANS * b
    elif name == "forward":
        Rr, tr = np.eye(3), np.array([0.0, 0.0, -1.0])   # the epipole is the principal point
    elif name in ("rot90", "rot180"):
        th = np.pi / 2 if name == "rot90" else np.pi     # turned about y around the middle of the points, which stays 6 in front
        Rr = rotvec_to_matrix([0.0, th, 0.0])
        centre = np.array([0.0, 0.0, 6.0])
        tr = np.array([0.0, 0.0, 6.0]) - Rr @ centre
    elif name == "far":
        depth = 10.0 ** rng.uniform(3.0, 5.0, N)
    elif name == "pure_rotation":
        tr = np.zeros(3)
    elif name == "behind":
        tr = np.array([-1.0, 0.02, -10.0])               # depth in the right camera: about z - 10 < 0 for z in 4 .. 8
    # the points: inside the left image, at `depth`
    ax, ay = 0.95 * k[2] / k[0], 0.95 * k[3] / k[1]
    X = np.stack([rng.uniform(-ax, ax, N) * depth, rng.uniform(-ay, ay, N) * depth, depth], axis=1)
    if name.startswith("general"):
        Q = rotvec_to_matrix(np.array([0.7, -1.1, 0.4]))
        o = np.array([30.0, -50.0, 80.0]) * (FAR_ORIGIN if name == "general_far_origin" else 1.0)
        X = X @ Q.T + o                                  # X_w = Q X + o, and a camera [R|t] becomes [R Q^T | t - R Q^T o]
        Rl, tl = Rl @ Q.T, tl - Rl @ Q.T @ o
        Rr, tr = Rr @ Q.T, tr - Rr @ Q.T @ o
    Pl = np.concatenate([Rl, tl[:, None]], axis=1).astype(np.float32)
    Pr = np.concatenate([Rr, tr[:, None]], axis=1).astype(np.float32)
    left = (project64(K, Pl, X) + rng.normal(0, 0.5, (N, 2))).astype(np.float32)
    right = project64(K, Pr, X) + rng.normal(0, 0.5, (N, 2))
    bad = rng.random(N) < 0.1
    right[bad] += rng.normal(0, 40.0, (int(bad.sum()), 2))
    return dict(name=name, K=K, P_left=Pl, P_right=Pr, left=left, right=right.astype(np.float32), bad=bad, X=X)


def jacobi_null_vectors(A, max_sweeps=60):
    """One-sided Jacobi on the columns of A [n,4,4] (np.longdouble), every match at once, until no pair of columns of any match is
    left to rotate: (V[:, :, argmin] [n,4], singular values descending [n,4], sweeps that rotated something).  A pair is rotated
    while |a_p . a_q| > 8 eps |a_p| |a_q| (a few roundings of the dot product itself)."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    V = np.zeros((n, 4, 4), LD)
    V[:, np.arange(4), np.arange(4)] = 1
    tol = 8 * np.finfo(LD).eps
    sweeps = 0
    for _ in range(max_sweeps):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                ap, aq = A[:, :, p].copy(), A[:, :, q].copy()
                app, aqq, apq = (ap * ap).sum(1), (aq * aq).sum(1), (ap * aq).sum(1)
                go = np.abs(apq) > tol * np.sqrt(app * aqq)
                if not go.any():
                    continue
                rotated = True
                safe = np.where(go, apq, LD(1))
                zeta = (aqq - app) / (2 * safe)
                t = np.where(zeta >= 0, LD(1), LD(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                c, s = np.where(go, c, LD(1))[:, None], np.where(go, s, LD(0))[:, None]
                A[:, :, p], A[:, :, q] = c * ap - s * aq, s * ap + c * aq
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p], V[:, :, q] = c * vp - s * vq, s * vp + c * vq
        if not rotated:
            break
        sweeps += 1
    else:
        raise AssertionError("the long-double Jacobi did not converge in %d sweeps" % max_sweeps)
    sigma = np.sqrt((A * A).sum(1))
    last = np.argmin(sigma, axis=1)
    v = V[np.arange(n), :, last]
    return v, -np.sort(-sigma, axis=1), sweeps


def reference(K, P_left, P_right, left_xy, right_xy, max_err=10.0):
    """triangulateViews for aligned matches with the DLT null vector in long double.  dict(points3d f32 [n,3], keep bool [n],
    err_left / err_right f64 [n] (at the reference's own points), sigma f64 [n,4] descending, Xh f32 [n,4], sweeps)."""
    K = np.asarray(K, dtype=np.float32).reshape(3, 3).astype(np.float64)
    Pl = np.asarray(P_left, dtype=np.float32).reshape(3, 4)
    Pr = np.asarray(P_right, dtype=np.float32).reshape(3, 4)
    l = np.asarray(left_xy, dtype=np.float32).reshape(-1, 2)
    r = np.asarray(right_xy, dtype=np.float32).reshape(-1, 2)
    n = l.shape[0]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]

    def normalise(p):
        q = np.stack([(p[:, 0].astype(np.float64) - cx) / fx, (p[:, 1].astype(np.float64) - cy) / fy], axis=1)
        q[~np.isfinite(q).all(axis=1)] = np.nan      # as oracle/triangulate_oracle.py: a pixel that is not finite normalises to NaN
        return q.astype(np.float32).astype(LD)

    nl, nr = normalise(l), normalise(r)
    Pl_, Pr_ = Pl.astype(LD), Pr.astype(LD)
    A = np.empty((n, 4, 4), LD)
    A[:, 0] = nl[:, 0:1] * Pl_[2] - Pl_[0]
    A[:, 1] = nl[:, 1:2] * Pl_[2] - Pl_[1]
    A[:, 2] = nr[:, 0:1] * Pr_[2] - Pr_[0]
    A[:, 3] = nr[:, 1:2] * Pr_[2] - Pr_[1]
    v, sigma, sweeps = jacobi_null_vectors(A)
    Xh = v.astype(np.float32)
    w = Xh[:, 3:4]
    scale = np.where(w != 0, np.float32(1.0) / np.where(w != 0, w, np.float32(1.0)), np.float32(1.0)).astype(np.float32)
    X = (Xh[:, :3] * scale).astype(np.float32)
    el, er = reprojection_errors(K, Pl, Pr, l, r, X)
    keep = ~((el > max_err) | (er > max_err))            # a NaN error compares False: kept (SfMStereoUtilities.cpp:186)
    return dict(points3d=X, keep=keep, err_left=el, err_right=er, sigma=sigma.astype(np.float64), Xh=Xh, sweeps=sweeps)


def reprojection_errors(K, P_left, P_right, left_xy, right_xy, X):
    """The reference's two errors at the float points X: projected in fp64, stored as float pixels, the norm in fp64."""
    l, r = np.asarray(left_xy, np.float32), np.asarray(right_xy, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        el = np.linalg.norm((project64(K, P_left, X).astype(np.float32) - l).astype(np.float64), axis=1)
        er = np.linalg.norm((project64(K, P_right, X).astype(np.float32) - r).astype(np.float64), axis=1)
    return el, er


def conditioned(ref):
    """bool [n]: where the point of a match is determined well enough to be compared (the rule in this module's header)."""
    s, Xh = ref["sigma"], ref["Xh"].astype(np.float64)
    return ((s[:, 2] - s[:, 3]) >= GAP_MIN * s[:, 0]) & (np.abs(Xh[:, 3]) >= W_MIN * np.linalg.norm(Xh, axis=1))


def ulp_distance(X, X_ref):
    """|X - X_ref| in float ulps of |X_ref|, per coordinate (fp64 arithmetic on the float values)."""
    X_ref = np.asarray(X_ref, np.float32)
    return np.abs(np.asarray(X, np.float32).astype(np.float64) - X_ref.astype(np.float64)) / np.spacing(np.abs(X_ref)).astype(np.float64)


def error_check(K, P_left, P_right, left_xy, right_xy, X, max_err):
    """What the error and keep tests hold a device run to, from the device's OWN float points X: (errors recomputed in fp64 [n,2],
    tolerance [n,2] = 4 float ulps of the largest pixel coordinate involved, observed or projected, band [n] = a recomputed error
    lies within its tolerance of max_err, keep_expected [n])."""
    l, r = np.asarray(left_xy, np.float32).astype(np.float64), np.asarray(right_xy, np.float32).astype(np.float64)
    out_e, out_t = [], []
    for P, obs in ((P_left, l), (P_right, r)):
        proj = project64(K, P, X)
        with np.errstate(invalid="ignore"):
            out_e.append(np.sqrt(((proj - obs) ** 2).sum(axis=1)))
            big = np.maximum(np.abs(proj).max(axis=1), np.abs(obs).max(axis=1))
            out_t.append(4.0 * np.spacing(big.astype(np.float32)).astype(np.float64))
    e, tol = np.stack(out_e, axis=1), np.stack(out_t, axis=1)
    with np.errstate(invalid="ignore"):
        band = (np.abs(e - max_err) <= tol).any(axis=1)
        keep = ~(e > max_err).any(axis=1)
    return e, tol, band, keep
