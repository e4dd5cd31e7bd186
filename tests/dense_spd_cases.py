"""Dense SPD systems for the three forms of the exact solve (csrc/dense_cholesky.hip + chol_tile.h), with their references.

Plain numpy / scipy, no GPU: generators, the LAPACK and long-double references, and the case tables shared by
tests/test_dense_spd_cases_cpu.py (which proves every declared property on the CPU) and tests/test_gpu_dense_cholesky.py
(which holds the device to them).  Arrays handed out by the cached generators are read-only: they are shared between tests.

Forms, by the padded dimension ld = 64 ceil((n + 1) / 64):  1 block column "small" (n <= 63), 2..40 "fused" (n <= 2559),
beyond "panel".
"""
import functools

import numpy as np
from scipy.linalg.lapack import dpotrf, dpotrs

U = 1.1e-16             # unit roundoff of fp64
ETA_FACTOR = 16.0       # eta_device <= ETA_FACTOR * max(eta_reference, U): see tests/test_gpu_dense_cholesky.py


def form_of(n):
    nblk = (n + 1 + 63) // 64
    return "small" if nblk == 1 else "fused" if nblk <= 40 else "panel"


def _frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------
def low_rank_factor(n, seed, rank=16):
    return np.random.default_rng(seed).normal(size=(n, rank)) * np.sqrt(n / (4.0 * rank))


def low_rank_spd(n, seed, rank=16):
    """G G^T + 0.05 n I with G n x rank, entries N(0, n / (4 rank)): the diagonal is ~0.3 n while the Schur pivots fall to ~0.05 n once the
    column index is well past `rank` (pivot_p ~ 0.05 n + 0.25 n / (1 + 5 p / rank)), at every n."""
    G = low_rank_factor(n, seed, rank)
    return G @ G.T + 0.05 * n * np.eye(n)


@functools.lru_cache(maxsize=4)
def base_matrix(n, kind="S"):
    """The SPD matrix every info case of size n and this kind starts from (shared, read-only).  Kind D takes rank = n: the pivots then stay
    near the diagonal (~0.25 (n - p) + 0.05 n against ~0.3 n), and breaking one of the first 0.4 n makes the diagonal entry itself negative."""
    return _frozen(low_rank_spd(n, 1000 + n, rank=16 if kind == "S" else n))


def break_minor(A, p):
    """Copy of A whose leading minor of order p is the first that is not positive definite: A[p-1, p-1] -= 1.5 L[p-1, p-1]^2, so pivot p
    becomes -0.5 x its old value (no rounding question) and the minors of order < p are untouched.  Only the leading p x p block of A has
    to be positive definite, so a second, earlier break can be applied to the result.  Returns (B, frac): frac = new diagonal / old."""
    L = np.linalg.cholesky(A[:p, :p])
    B = np.array(A, dtype=np.float64, copy=True)
    old = B[p - 1, p - 1]
    B[p - 1, p - 1] = old - 1.5 * L[p - 1, p - 1] ** 2
    return B, B[p - 1, p - 1] / old


def first_bad_minor(A):
    """Unblocked Cholesky in long double: 1-based order of the first leading minor that is not positive definite (pivot not positive or
    not finite), or 0.  Independent of LAPACK; ~1.4 s at n = 640, not meant for more."""
    A = np.asarray(A)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=np.longdouble)
    Al = np.tril(A).astype(np.longdouble)
    for j in range(n):
        row = L[j, :j]
        d = Al[j, j] - row @ row
        if not (d > 0) or not np.isfinite(d):
            return j + 1
        d = np.sqrt(d)
        L[j, j] = d
        if j + 1 < n:
            L[j + 1:, j] = (Al[j + 1:, j] - L[j + 1:, :j] @ row) / d
    return 0


def norm2(A):
    """||A||_2 of a symmetric matrix (Lanczos on the large ones: a full eigenvalue decomposition of 2600^2 takes seconds)."""
    if A.shape[0] > 700:
        from scipy.sparse.linalg import eigsh
        return float(np.abs(eigsh(A, k=1, which="LM", return_eigenvectors=False, v0=np.ones(A.shape[0]))).max())    # fixed start: reproducible
    return float(np.abs(np.linalg.eigvalsh(A)).max())


def eta(A, b, x, normA=None):
    """Normwise backward error ||b - A x||_2 / (||A||_2 ||x||_2 + ||b||_2), the residual formed in long double."""
    Al = A if A.dtype == np.longdouble else np.asarray(A).astype(np.longdouble)
    r = np.asarray(b).astype(np.longdouble) - Al @ np.asarray(x).astype(np.longdouble)
    if normA is None:
        normA = norm2(np.asarray(A, dtype=np.float64))
    den = normA * np.linalg.norm(x) + np.linalg.norm(b)
    return float(np.sqrt(r @ r) / den)


def lapack_info(A):
    return int(dpotrf(np.asarray(A, dtype=np.float64), lower=1, clean=0)[1])


def lapack_solve(A, b, normA=None):
    """dpotrf + dpotrs: (x, info, eta); x and eta are None when info != 0."""
    c, info = dpotrf(np.asarray(A, dtype=np.float64), lower=1, clean=0)
    if info != 0:
        return None, int(info), None
    x, info2 = dpotrs(c, b, lower=1)
    assert info2 == 0
    return x, 0, eta(A, b, x, normA)


def spectrum_spd(n, kappa, seed):
    """Q diag(logspace(0, -log10 kappa, n)) Q^T with Q from a QR: cond_2 = kappa exactly (in exact arithmetic).  For n <= 640."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = np.logspace(0, -np.log10(kappa), n) if n > 1 else np.ones(1)
    A = (Q * ev) @ Q.T
    return 0.5 * (A + A.T)


def graded_spd(n, kappa, seed, rank=16):
    """D B D with B = G G^T / rank + delta I and D a permuted logspace(0, -4, n) on the diagonal; cheap at any n.
    kappa is the condition of B, the matrix a symmetric scaling cannot improve: with rank < n the smallest eigenvalue of B is delta and the
    largest lambda_1(G^T G / rank) + delta, so delta = lambda_1 / (kappa - 1).  The grading multiplies cond_2 of the product by up to 1e8
    on top of that, which a Cholesky factorisation (invariant under symmetric diagonal scaling up to rounding) does not feel."""
    rng = np.random.default_rng(seed)
    rank = max(1, min(rank, n - 1))
    G = rng.normal(size=(n, rank))
    lam1 = float(np.linalg.eigvalsh(G.T @ G / rank).max())
    delta = lam1 / (kappa - 1.0)
    B = G @ G.T / rank + delta * np.eye(n)
    dvec = rng.permutation(np.logspace(0, -4, n)) if n > 1 else np.ones(1)
    A = dvec[:, None] * B * dvec[None, :]
    return 0.5 * (A + A.T)


# ---------------------------------------------------------------------------------------------
# info cases: (n, p, kind).  kind "D": the broken diagonal entry itself is negative; "S": it stays positive (>= 0.25 x its old value) and
# the pivot turns negative only after the updates of the earlier columns.  S wherever the low-rank matrix allows it (everywhere but p = 1);
# D besides at column 65, the first of the second tile, of the larger sizes.
# ---------------------------------------------------------------------------------------------
INFO_CASES = [
    # small: one tile.  16 | 17: last column of a 16-column panel | first of the next; 40 = d
    (40, 1, "D"), (40, 16, "S"), (40, 17, "S"), (40, 38, "S"), (40, 40, "S"),
    (63, 48, "S"), (63, 49, "S"), (63, 63, "S"),            # 63 = d: last column of the tile, before the augmented row
    # fused: tiles after the first
    (64, 64, "S"),                                          # = d; the augmented row alone in tile 1
    (200, 1, "D"), (200, 64, "S"), (200, 65, "S"), (200, 100, "S"), (200, 128, "S"), (200, 129, "S"),
    (200, 193, "S"),                                        # first column of the last, partial tile
    (200, 199, "S"), (200, 200, "S"),                       # = d: 8 true columns in its panel
    (209, 209, "S"), (193, 193, "S"), (207, 207, "S"),      # p = d with d mod 16 = 1, 1, 15
    (640, 65, "D"), (640, 577, "S"), (640, 640, "S"),
    # panel: the two-kernel form
    (2560, 65, "D"), (2560, 1300, "S"), (2560, 2497, "S"), (2560, 2560, "S"),   # 2560 = d: the augmented row in a tile of its own
    (2600, 2561, "S"), (2600, 2600, "S"),
]
# two failures: (n, p1, p2) with p1 < p2, p2 broken first and p1 on the result; the first one wins
TWO_FAILURE_CASES = [(200, 70, 150), (200, 10, 70), (2600, 1300, 2000)]
# a NaN / +inf on the diagonal at p, SPD otherwise: (n, p)
NONFINITE_CASES = [(200, 100), (2600, 1300)]


def info_id(case):
    return "n%d-p%d-%s" % case


def info_matrix(n, p, kind):
    """(B, frac) of an info case; asserts the declared kind."""
    B, frac = break_minor(base_matrix(n, kind), p)
    if kind == "S":
        assert frac >= 0.25, (n, p, frac)
    else:
        assert frac < 0, (n, p, frac)
    return B, frac


def two_failure_matrix(n, p1, p2):
    B, _ = break_minor(base_matrix(n), p2)
    B, _ = break_minor(B, p1)
    return B


def nonfinite_matrix(n, p, value):
    B = np.array(base_matrix(n), copy=True)
    B[p - 1, p - 1] = value
    return B


def info_rhs(n):
    return np.random.default_rng(7000 + n).normal(size=n)


# ---------------------------------------------------------------------------------------------
# accuracy cases: (class, n, kappa)
# ---------------------------------------------------------------------------------------------
ACCURACY_SIZES = (5, 63, 64, 129, 640)
ACCURACY_CASES = [("spectrum", n, k) for n in ACCURACY_SIZES for k in (1e4, 1e8, 1e11)] + \
                 [("graded", n, 1e8) for n in ACCURACY_SIZES + (1281, 2559, 2560, 2600)]


def accuracy_id(case):
    return "%s-n%d-k1e%d" % (case[0], case[1], round(np.log10(case[2])))


@functools.lru_cache(maxsize=2)
def accuracy_system(cls, n, kappa):
    """(A, b, ||A||_2) of an accuracy case, read-only.  b = A x0 with x0 ~ N(0, 1): a solution that is not confined to the directions of the small
    eigenvalues, so an error in any column of the factor shows in the residual."""
    seed = 100 * n + int(round(np.log10(kappa)))
    A = spectrum_spd(n, kappa, seed) if cls == "spectrum" else graded_spd(n, kappa, seed)
    b = A @ np.random.default_rng(seed + 1).normal(size=n)
    return _frozen(A), _frozen(b), norm2(A)


def eta_bar(eta_ref):
    return ETA_FACTOR * max(eta_ref, U)


# ---------------------------------------------------------------------------------------------
# tile-edge sizes: info == 0 and the backward error, with the augmented pivot 1 - |L^-1 b|^2 on both sides of zero
# ---------------------------------------------------------------------------------------------
def _r(a, b):
    return tuple(range(a, b + 1))


EDGE_GROUPS = [
    ("n1-257", _r(1, 5) + _r(60, 69) + _r(124, 132) + _r(188, 196) + _r(255, 257)),
    ("n511-513_640", _r(511, 513) + (640,)),
    ("n1023-1025", _r(1023, 1025)),
    ("n1279-1281", _r(1279, 1281)),
] + [("n%d" % n, (n,)) for n in _r(2555, 2564) + _r(2623, 2625) + (3000,)]
# |L^-1 b|^2 = b^T A^-1 b ~ 15 scale^2 for low_rank_spd and b = scale N(0, 1): the augmented pivot is positive, negative, hugely negative
EDGE_SCALES = (1e-6, 1.0, 1e6)


def edge_system(n):
    """(A, b at scale 1, ||A||_2); ||A||_2 = ||G^T G||_2 + 0.05 n from the small Gram matrix."""
    seed = 2000 + n
    A = low_rank_spd(n, seed)
    G = low_rank_factor(n, seed)
    normA = float(np.linalg.eigvalsh(G.T @ G).max()) + 0.05 * n
    b = np.random.default_rng(seed + 1).normal(size=n)
    return A, b, normA
