"""Reference check of ONE linear solve of an LM step (numpy only): is the reduced step z that a back-substitution consumed a solution
of the damped reduced camera system S z = rhs as accurate as its solver family promises, and is the point step the one that z implies?

The CG families iterate in the block-Jacobi transformed unknowns (pcg_common.h, "Block-Jacobi preconditioned conjugate gradients"): B is the Cholesky factor of
every 6x6 diagonal camera block of S plus the square root of the focal diagonal entry, S~ = B^-1 S B^-T, b~ = B^-1 rhs, x~ = B^T z, and
k_cam_update forms z = B^-T x~.  Their stopping test is on the 2-norm of the recursively updated residual of THAT system, relative to
|b~| (`rrn <= tol2 * rr0` in k_pcg_iter of pcg_streaming.hip, k_sy_vec of pcg_symmetric.hip, k_pcg_iter_fast of pcg_fast.hip, k_pcg_iter_ml of
pcg_segments.hip, `rr <= tol2 * scal[PS_RR0]` in k_sg_p of pcg_segments_streaming.hip; rr0 = |b~|^2 from pcg_threshold_base, anchored -- max(|b~|, |b~_first|) capped -- only from the
second solve of an LM run, which a one-iteration solve never reaches).  So the residual checked here is

    rho = |b~ - S~ x~| / |b~| = |B^-1 (rhs - S z)| / |B^-1 rhs|,      evaluated in np.longdouble,

and the bars are derived, not fitted (unit roundoff u, CG iterations k, the measured matrix deviation delta):

    CG        rho <= 2 tol + 10 (k + 1) (u + delta) |S~|_2 |x~| / |b~|      (true vs recursive residual drift of k steps)
    Cholesky  |S z - rhs| / (|S|_2 |z|) <= 10 d u                             (backward error of a Cholesky solve)
    step      |x~ - x~_o| / |x~_o| <= kappa~ (bar + delta)                    (forward error from the backward one)
    points    |dX_i - dX_o,i| <= 10 (m_i + 3) u_p cond(V_i) mag_i + u |X_i|     (m_i observations; mag_i = |(|V_i^-1| (|b_p| + sum |E^T u|))|,
                                                                             the terms that cancel into dX_i -- oracle.lm_step's dmag; below
                                                                             u |X_i| the trial point cannot tell)
"""
import numpy as np

U64 = 2.0 ** -53
U32 = 2.0 ** -24


def block_factor(S):
    """Lower block-Jacobi factors: L [nc][6][6] (Cholesky of each diagonal camera block) and the focal factor lf."""
    d = S.shape[0]
    nc = (d - 1) // 6
    blocks = np.stack([S[6 * j:6 * j + 6, 6 * j:6 * j + 6] for j in range(nc)]) if nc else np.zeros((0, 6, 6))
    L = np.linalg.cholesky(blocks) if nc else blocks
    return L, np.sqrt(S[d - 1, d - 1])


def apply_binv(L, lf, v):
    """B^-1 v for the block-diagonal lower B, by forward substitution in the precision of v (vectorised over the cameras and over
    the columns of a 2-D v)."""
    nc = L.shape[0]
    Lq = L.astype(v.dtype)
    y = np.zeros_like(v)
    V = v[:6 * nc].reshape((nc, 6) + v.shape[1:])
    Y = y[:6 * nc].reshape((nc, 6) + v.shape[1:])
    ex = (slice(None),) + (None,) * (v.ndim - 1)
    for a in range(6):
        acc = V[:, a].copy()
        for b in range(a):
            acc -= Lq[:, a, b][ex] * Y[:, b]
        Y[:, a] = acc / Lq[:, a, a][ex]
    y[-1] = v[-1] / v.dtype.type(lf)
    return y


def apply_bt(L, lf, z):
    """x~ = B^T z."""
    nc = L.shape[0]
    x = np.empty_like(z)
    x[:6 * nc] = np.einsum("jba,jb->ja", L, z[:6 * nc].reshape(nc, 6)).ravel()
    x[-1] = lf * z[-1]
    return x


def apply_binv_t(L, lf, x):
    """z = B^-T x~ (back substitution with the transposed factors)."""
    nc = L.shape[0]
    z = np.zeros_like(x)
    X = x[:6 * nc].reshape(nc, 6)
    Z = z[:6 * nc].reshape(nc, 6)
    for a in range(5, -1, -1):
        acc = X[:, a].copy()
        for b in range(a + 1, 6):
            acc -= L[:, b, a] * Z[:, b]
        Z[:, a] = acc / L[:, a, a]
    z[-1] = x[-1] / lf
    return z


def transformed_matrix(S, L, lf):
    """S~ = B^-1 S B^-T (float64)."""
    Y = apply_binv(L, lf, np.array(S, np.float64))
    return apply_binv(L, lf, np.ascontiguousarray(Y.T)).T


class System:
    """One damped reduced system (S, rhs) and its block-Jacobi transform; `ref` (optional) is the oracle's system of the same step,
    which fixes B for the step comparison and gives delta = |S~ - S~_o|_2 / |S~_o|_2."""

    def __init__(self, S, rhs, ref=None):
        self.S = np.asarray(S, np.float64)
        self.rhs = np.asarray(rhs, np.float64)
        self.d = self.S.shape[0]
        self.L, self.lf = block_factor(self.S)
        self.St = transformed_matrix(self.S, self.L, self.lf)
        ev = np.linalg.eigvalsh(0.5 * (self.St + self.St.T))
        self.St_norm = float(np.max(np.abs(ev)))
        self.kappa = float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf
        self.S_norm = float(np.max(np.abs(np.linalg.eigvalsh(self.S))))
        self.bt = apply_binv(self.L, self.lf, self.rhs)
        self.delta = 0.0
        self.ref = ref
        if ref is not None:
            Sto = ref.St
            Sdt = transformed_matrix(self.S, ref.L, ref.lf)
            self.delta = float(np.max(np.abs(np.linalg.eigvalsh(0.5 * ((Sdt - Sto) + (Sdt - Sto).T))))) / ref.St_norm

    def rho(self, z):
        """|b~ - S~ x~| / |b~| in long double (= |B^-1 (rhs - S z)| / |B^-1 rhs|)."""
        q = np.longdouble
        r = self.rhs.astype(q) - self.S.astype(q) @ np.asarray(z, np.float64).astype(q)
        rt = apply_binv(self.L, self.lf, r)
        bt = apply_binv(self.L, self.lf, self.rhs.astype(q))
        return float(np.sqrt(np.sum(rt * rt)) / np.sqrt(np.sum(bt * bt)))

    def xt(self, z):
        return apply_bt(self.L, self.lf, np.asarray(z, np.float64))

    def cg_bar(self, z, tol, k, u=U64, delta=None):
        delta = self.delta if delta is None else delta
        xt = self.xt(z)
        return 2.0 * tol + 10.0 * (k + 1) * (u + delta) * self.St_norm * np.linalg.norm(xt) / np.linalg.norm(self.bt)

    def chol_residual(self, z):
        q = np.longdouble
        z = np.asarray(z, np.float64)
        r = self.S.astype(q) @ z.astype(q) - self.rhs.astype(q)
        return float(np.sqrt(np.sum(r * r)) / (self.S_norm * np.linalg.norm(z)))

    def chol_bar(self, u=U64):
        return 10.0 * self.d * u

    def step_error(self, z, z_ref):
        """|x~ - x~_o| / |x~_o| with the transform of `self` (the oracle's system when called on it)."""
        a, b = self.xt(z), self.xt(z_ref)
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def check_cg(sys_, z, tol, k, u=U64, delta=None):
    """(rho, bar) of a CG family's step."""
    return sys_.rho(z), sys_.cg_bar(z, tol, k, u, delta)


def check_cholesky(sys_, z, u=U64):
    return sys_.chol_residual(z), sys_.chol_bar(u)


def check_step(oracle_sys, z, z_oracle, bar, delta):
    """(error, bar) of the step against the oracle's exact step, in the oracle's transformed unknowns."""
    return oracle_sys.step_error(z, z_oracle), oracle_sys.kappa * (bar + delta)


def check_points(dpt, dpt_ref, vcond, dmag, nobs, pts, u=U64):
    """Per point: (largest measured / bar ratio, index).  dpt_ref, vcond, dmag: the oracle's back-substitution of the SAME z."""
    dpt, dpt_ref = np.asarray(dpt, np.float64), np.asarray(dpt_ref, np.float64)
    err = np.linalg.norm(dpt - dpt_ref, axis=1)
    seen = nobs > 0
    bar = 10.0 * (nobs + 3) * u * vcond * dmag + U64 * np.linalg.norm(pts, axis=1)
    ratio = np.where(seen, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(ratio)) if ratio.size else 0
    return float(ratio[i]) if ratio.size else 0.0, i


def numpy_pcg(sys_, tol, max_iters=10000):
    """Block-Jacobi CG in the transformed unknowns, stopped at |r~| <= tol |b~| (the CG families' test): (z, iterations)."""
    St, bt = sys_.St, sys_.bt
    x = np.zeros_like(bt)
    r = bt.copy()
    p = r.copy()
    rr = r @ r
    b2 = bt @ bt
    k = 0
    while rr > tol * tol * b2 and k < max_iters:
        q = St @ p
        a = rr / (p @ q)
        x += a * p
        r -= a * q
        rrn = r @ r
        p = r + (rrn / rr) * p
        rr = rrn
        k += 1
    return apply_binv_t(sys_.L, sys_.lf, x), k
