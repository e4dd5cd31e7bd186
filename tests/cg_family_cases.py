"""Cases, systems, references and bars of tests/test_gpu_cg_families.py (numpy / scipy only; proved on the CPU by tests/test_cg_family_cases_cpu.py).

What is held: every reduced-system CG family, at the smallest dimension of each of its size classes, against a numpy restatement of the
method of csrc/pcg_common.h -- CG on the block-Jacobi transformed matrix S~ with the additive two-level preconditioner
M^-1 = I + W~ E^-1 W~^T, E = W~^T S~ W~, stopped at |r| <= tol |b~| on the recursively updated residual -- through sfmba_dense_pcg_probe,
which goes through the library's own transform, path choice and family launches.

SYSTEMS.  d = 6 nc + 1, built in O(d^2 r), no d^3 product:
    A = I + U diag(c) U^T,   U = [w_0 .. w_7 | g_0 .. g_(r-1)] orthonormal (QR of a normal matrix),   c = (lambda_k - 1 | D_m)
so A is SPD with the eigenvalues lambda_k (eight small ones, eigenvectors w_k), 1 + D_m (the band) and 1, every entry non-zero;
    S = B A B^T,             B = blockdiag(B_j), B_j a random lower 6 x 6 (the camera blocks) and a scalar (the focal),
so the diagonal blocks of S are far from the identity and the library's transform has work to do.  With L = blockdiag(chol(S_jj)) -- what the
library factors -- and Q = L^-1 B,
    S~ = L^-1 S L^-T = Q A Q^T
is applied in O(d r) in any precision (StructuredOp): that is what lets the long-double restatement run at d = 8197.  S~ has the spectrum of the
block-Jacobi preconditioned A: eight small eigenvalues along Q^-T w_k = L^T B^-T w_k (the coarse vectors Wt are an invertible mix of those, rounded
to fp32), the rest in a band.  |S~|_2 and kappa~ come from Lanczos on the structured operator (scipy eigsh), never from a dense eigenvalue
decomposition.  The matrix the DEVICE gets is the dense fp64 S: the true residual (rho) is evaluated against that one, in long double.

The structured S~ and the S~ the device forms from the rounded dense S differ by a relative O(u cond(B_j)^2) <= 1e-14 (cond(B_j) <= 8): two
decades below the forced-iterate bar kappa~ 10 (k + 1) u |S~|_2 |x~_k| / |b~| (kappa~ = 170, |x~_1| / |b~| >= 0.5: 3e-13 and more).

fp32 matrix: the library rounds the transformed matrix to fp32.  The reference operator is then StructuredOp + Delta, Delta = fp32(S~) - S~ a dense
fp64 array applied with a BLAS product (its entries are 1e-8 of the matrix's: fp64 is more than long double needs there).
"""
import functools

import numpy as np

import linear_step_check as lsc

U64, U32 = lsc.U64, lsc.U32
TOL = 1e-10
MAX_ITERS = 200            # every probe call of the tests passes it explicitly
NW = 8                     # PCG_NW

# ---- the header constants the routing table is written from (csrc/pcg_common.h, csrc/dense_solver.hip) ----
FAST_MAX_D = 1280          # 256 PCG_EPT = 64 PCG_CPL: the fast family's geometry
PCG_MAXWG = 256            # segments (fast): one workgroup per camera + the focal row
PCG_MAXWG_BIG = 1024       # streaming: rows_per_wg = 8 up to d = 8192, 16 above
PCG_PART = 1024
ML_G, ML_MIN_CAMS, SG_MAXG, SG_UWG = 8, 32, 20, 16
SY_EPT_BOUNDS = ((8, 2048), (16, 4096), (24, 6144), (32, 8192))       # k_sy_vec<.., EPT>: d <= 256 EPT; looped (EPT 0) above
CHOL_NB = 64


def padded_dim(d):
    return (d + 1 + CHOL_NB - 1) // CHOL_NB * CHOL_NB


def sg_hats(nc):
    return min(max(nc // 25, ML_G), SG_MAXG)


def sy_ept(d):
    for ept, bound in SY_EPT_BOUNDS:
        if d <= bound:
            return ept
    return 0


def streaming_rows_per_wg(d):
    return max(8, (-(-d // PCG_MAXWG_BIG) + 7) // 8 * 8)


def route(nc, symmetric, f32, coarse, segments):
    """(family name, f32_matrix, coarse_vectors) of dense_pcg_path, restated from the constants above."""
    d = 6 * nc + 1
    fast = d <= FAST_MAX_D
    ml = segments and coarse and fast and nc >= ML_MIN_CAMS and nc + 1 <= PCG_MAXWG
    sg = segments and coarse and not fast and nc >= ML_MIN_CAMS and (d + 7) // 8 <= PCG_PART and nc + 1 <= 64 * SG_UWG - SG_UWG
    family = ("PCG_SEGMENTS" if ml else "PCG_FAST" if fast else "PCG_SEGMENTS_STREAMING" if sg else "PCG_SYMMETRIC" if symmetric else "PCG_STREAMING")
    rows = 6 if ml else 8 if sg else -(-d // PCG_MAXWG) if fast else streaming_rows_per_wg(d)
    cv = 7 * ML_G + 1 if ml else 7 * sg_hats(nc) + 1 if sg else NW if coarse and rows <= 16 else 0
    return family, int(f32 and not fast), cv


# ---- variants: (symmetric, f32 matrix, coarse, segments) as the probe's flags and Wt ----
VARIANTS = {
    "sy64c": (1, 0, 1, 0), "sy64n": (1, 0, 0, 0), "sy32c": (1, 1, 1, 0), "sy32n": (1, 1, 0, 0),
    "st64c": (0, 0, 1, 0), "st64n": (0, 0, 0, 0), "st32c": (0, 1, 1, 0), "st32n": (0, 1, 0, 0),
    "seg": (1, 0, 1, 1),
}
CROSS = ("sy64c", "sy64n", "sy32c", "sy32n", "st64c", "st64n", "st32c", "st32n")

# (nc, variant, what the probe must report: family, f32_matrix, coarse_vectors) -- written out, never read back from the device;
# test_cg_family_cases_cpu.py holds every row against route() above.
_SIZES = [
    # nc, d, ld % 256: what the size is
    (32, ("seg",)),                                   # d = 193: first size of the segmented fast family
    (43, ("sy64c", "sy64n")),                         # d = 259: fast family, 2 rows per workgroup
    (213, ("sy64c", "sy64n", "seg")),                 # d = 1279: last fast size, 5 rows per workgroup; last segmented fast size
    (214, CROSS + ("seg",)),                          # d = 1285, ld 1344 (64): first streaming size; last strip 5 rows, last chunk 5 columns
    (224, ("sy64c",)),                                # d = 1345, ld 1408 (128)
    (235, ("sy64c",)),                                # d = 1411, ld 1472 (192)
    (256, CROSS),                                     # d = 1537, ld 1600 (64): d = 1 mod 256 / 128 / 32, the last tile is one diagonal entry
    (341, ("sy64c",)),                                # d = 2047, ld 2048 (0): last EPT 8, d = 255 mod 256
    (342, CROSS),                                     # d = 2053, ld 2112 (64): first EPT 16
    (682, ("sy64c",)),                                # d = 4093, ld 4096 (0): last EPT 16
    (683, CROSS),                                     # d = 4099, ld 4160 (64): first EPT 24
    (1007, ("seg",)),                                 # d = 6043: last size of the streaming segmented family (nc + 1 <= 64 SG_UWG - SG_UWG), 20 hats
    (1023, ("sy64c",)),                               # d = 6139, ld 6144 (0): last EPT 24
    (1024, ("sy64c", "sy32c")),                       # d = 6145, ld 6208 (64): first EPT 32
    (1365, ("sy64c", "sy32c", "st64c", "seg")),       # d = 8191, ld 8192 (0): last EPT 32; streaming rows_per_wg 8; segments: back to eight vectors
    (1366, ("sy64c", "sy32c", "st64c", "seg")),       # d = 8197, ld 8256 (64): looped k_sy_vec; streaming rows_per_wg 16 (CO_MAXROWS set-up, 67 KB of LDS)
]
_EXPECT = {
    "fast": {"sy64c": ("PCG_FAST", 0, 8), "sy64n": ("PCG_FAST", 0, 0)},
    "stream": {"sy64c": ("PCG_SYMMETRIC", 0, 8), "sy64n": ("PCG_SYMMETRIC", 0, 0), "sy32c": ("PCG_SYMMETRIC", 1, 8), "sy32n": ("PCG_SYMMETRIC", 1, 0),
               "st64c": ("PCG_STREAMING", 0, 8), "st64n": ("PCG_STREAMING", 0, 0), "st32c": ("PCG_STREAMING", 1, 8), "st32n": ("PCG_STREAMING", 1, 0)},
}
_SEG_EXPECT = {32: ("PCG_SEGMENTS", 0, 57), 213: ("PCG_SEGMENTS", 0, 57), 214: ("PCG_SEGMENTS_STREAMING", 0, 57), 1007: ("PCG_SEGMENTS_STREAMING", 0, 141),
               1365: ("PCG_SYMMETRIC", 0, 8), 1366: ("PCG_SYMMETRIC", 0, 8)}
CASES = [(nc, v, _SEG_EXPECT[nc] if v == "seg" else _EXPECT["fast" if 6 * nc + 1 <= FAST_MAX_D else "stream"][v]) for nc, vs in _SIZES for v in vs]


def case_id(case):
    return "nc%d-%s" % (case[0], case[1])


# ---------------------------------------------------------------------------------------------
# block-diagonal helpers: blocks [nc][6][6] + a scalar for the trailing unknown
# ---------------------------------------------------------------------------------------------
def blk_mul(Mb, mf, V, transpose=False):
    """blockdiag(Mb, mf) V (or its transpose times V) for V [d] or [d, m], in V's precision."""
    nc = Mb.shape[0]
    Mq = Mb.astype(V.dtype)
    out = np.empty_like(V)
    Vc = V[:6 * nc].reshape((nc, 6) + V.shape[1:])
    sub = ("jba" if transpose else "jab") + (",jbm->jam" if V.ndim == 2 else ",jb->ja")
    out[:6 * nc] = np.einsum(sub, Mq, Vc).reshape((6 * nc,) + V.shape[1:])
    out[6 * nc] = V.dtype.type(mf) * V[6 * nc]
    return out


class StructuredOp:
    """v -> S~ v = Q (I + U diag(c) U^T) Q^T v (+ Delta v) in precision q."""

    def __init__(self, Qb, qf, U, c, q=np.float64, delta=None):
        self.q, self.Qb, self.qf, self.U, self.c, self.delta = q, Qb.astype(q), q(qf), U.astype(q), c.astype(q), delta

    def __call__(self, V):
        V = np.asarray(V, self.q)
        Vp = blk_mul(self.Qb, self.qf, V, transpose=True)
        t = self.U.T @ Vp
        Y = Vp + self.U @ (t * (self.c if V.ndim == 1 else self.c[:, None]))
        out = blk_mul(self.Qb, self.qf, Y)
        if self.delta is not None:
            out = out + (self.delta @ V.astype(np.float64)).astype(self.q)
        return out


# ---------------------------------------------------------------------------------------------
# the systems
# ---------------------------------------------------------------------------------------------
SMALL_EIGS = np.array([1e-2, 1.2e-2, 1.5e-2, 1.8e-2, 2.2e-2, 2.6e-2, 3e-2, 8e-2])      # seven gauge-like directions and one focal/depth-like (pcg_common.h, "Coarse space")
# (a decade and a half above the 2.5e-4 of a real problem at radius 1e4: with those, plain CG -- the variants without the coarse space -- loses
# orthogonality early enough that its float64 and long-double runs end three and four iterations apart, and the iteration check would hold nothing)
MIX_COND = 200.0           # largest condition number of the 8 x 8 mix of the coarse vectors (CgSystem)
BAND = 0.72           # D_m uniform in [-BAND, BAND]: the band [0.28, 1.72], kappa 6.1 -> CG to 1e-10 in ~ sqrt(kappa) / 2 * ln(2e10) = 29 iterations


class CgSystem:
    def __init__(self, nc, want_f32=False):
        self.nc, self.d = nc, 6 * nc + 1
        d = self.d
        rng = np.random.default_rng(7000 + nc)
        r = 40 if nc >= 100 else 28
        Uo, _ = np.linalg.qr(rng.normal(size=(d, NW + r)))
        # (d < NW + r -- fewer than six cameras, the rows of dist_cg_cases.py --: the QR has d columns; the small eigenvalues first, what is left is
        # band.  One camera, d = 7: three small eigenvalues and four in the band, so that the coarse space does not span everything -- the bars model
        # the CG on S~, not the conditioning of an E that carries the whole solve -- and the eight vectors have rank three)
        ns = NW if d >= NW + 4 else d // 2
        r = max(min(r, d - ns), 0)
        self.coarse_rank = ns
        self.U = Uo
        self.c = np.concatenate([SMALL_EIGS[:ns] - 1.0, np.linspace(-BAND, BAND, r)])
        # B: lower 6 x 6 blocks, diagonal in [0.6, 1.6] times a per-camera scale over a decade, off-diagonal N(0, 0.15); focal scalar 3
        Bb = np.tril(rng.normal(scale=0.15, size=(nc, 6, 6)), -1)
        Bb[:, np.arange(6), np.arange(6)] = rng.uniform(0.6, 1.6, size=(nc, 6))
        Bb *= 10.0 ** rng.uniform(-0.5, 0.5, size=(nc, 1, 1))
        self.Bb, self.bf = Bb, 3.0
        A = (Uo * self.c) @ Uo.T
        A[np.arange(d), np.arange(d)] += 1.0
        S = blk_mul(Bb, self.bf, np.ascontiguousarray(blk_mul(Bb, self.bf, A).T)).T
        del A
        S = np.triu(S)
        S = S + np.triu(S, 1).T                      # exactly symmetric: the device reads the upper triangle
        self.S = np.ascontiguousarray(S)
        self.L, self.lf = lsc.block_factor(self.S)
        self.Qb = np.linalg.solve(self.L, Bb)        # Q_j = L_j^-1 B_j
        self.qf = self.bf / self.lf
        self.op64 = StructuredOp(self.Qb, self.qf, Uo, self.c, np.float64)
        self.opld = StructuredOp(self.Qb, self.qf, Uo, self.c, np.longdouble)
        # coarse vectors: an invertible mix of the near-null vectors L^T B^-T w_k of S~, fp32-representable
        Z = np.stack([self._binv_t_B(Uo[:, k]) for k in range(ns)])
        # (the mix is drawn again while its condition number is above MIX_COND: the forced-iterate bar models the CG on S~ with an exact coarse
        # solve, and a mix conditioned 1.5e3 -- the first draw at nc = 171 -- gives an E conditioned 2e6, at which the float64 restatement itself
        # misses the bar by 19 x.  Every size of CASES passes on its first draw, 136 at nc = 682 the largest: their systems are what they were.)
        mix8 = np.eye(NW) + 0.3 * rng.normal(size=(NW, NW))
        while np.linalg.cond(mix8) > MIX_COND:
            mix8 = np.eye(NW) + 0.3 * rng.normal(size=(NW, NW))
        mix = mix8[:, :ns]
        V = np.stack([lsc.apply_bt(self.L, self.lf, z) for z in Z])
        self.Wt = (mix @ V).astype(np.float32).astype(np.float64) * np.float64(2.0 ** 3)
        # the segmented families take vectors 0 .. 6 on the camera rows only (pcg_segments.hip: "the focal row: only W~_7 is non-zero there" -- a
        # similarity transform does not move the focal length): their Wt has zeros there, and the mix leaves vector 7 alone
        mix7 = mix.copy()
        mix7[:NW - 1, ns - 1] = 0.0
        mix7[NW - 1, :ns - 1] = 0.0
        self.Wt_seg = (mix7 @ V).astype(np.float32).astype(np.float64) * np.float64(2.0 ** 3)
        self.Wt_seg[:NW - 1, d - 1] = 0.0
        # right-hand sides (original unknowns)
        self.rhs = rng.normal(size=d)
        self.rhs2 = rng.normal(size=d)
        self.delta32 = None
        if want_f32:
            St = lsc.transformed_matrix(self.S, self.L, self.lf)
            St = np.triu(St)
            St = St + np.triu(St, 1).T
            self.delta32 = St.astype(np.float32).astype(np.float64) - St
            del St
        self._spectrum()

    def _binv_t_B(self, w):
        """B^-T w (back substitution with the blocks of B)."""
        nc = self.nc
        z = np.empty_like(w)
        z[:6 * nc] = np.linalg.solve(np.swapaxes(self.Bb, 1, 2), w[:6 * nc].reshape(nc, 6, 1)).reshape(-1)
        z[-1] = w[-1] / self.bf
        return z

    def _spectrum(self):
        if self.d <= 64:                              # too small for Lanczos with NW + 1 wanted values: the dense spectrum of the structured operator
            ev = np.linalg.eigvalsh(self.op64(np.eye(self.d)))
            ns = self.coarse_rank
            self.St_norm, self.small_eigs, self.band_lo = float(ev[-1]), ev[:ns], float(ev[ns])
            self.kappa = self.St_norm / float(ev[0])
            return
        from scipy.sparse.linalg import LinearOperator, eigsh
        lo = LinearOperator((self.d, self.d), matvec=self.op64, dtype=np.float64)
        v0 = np.ones(self.d)
        self.St_norm = float(eigsh(lo, k=1, which="LA", v0=v0, tol=1e-6, return_eigenvectors=False)[0])
        small = np.sort(eigsh(lo, k=NW + 1, which="SA", v0=v0, ncv=min(self.d - 1, 64), tol=1e-6, return_eigenvectors=False))
        self.small_eigs, self.band_lo = small[:NW], float(small[NW])
        self.kappa = self.St_norm / float(small[0])

    def op(self, f32, q):
        if not f32:
            return self.op64 if q is np.float64 else self.opld
        assert self.delta32 is not None
        return StructuredOp(self.Qb, self.qf, self.U, self.c, q, self.delta32)

    def bt(self, rhs, q=np.float64):
        return lsc.apply_binv(self.L, self.lf, np.asarray(rhs, np.float64).astype(q))

    def xt(self, Z):
        return lsc.apply_bt(self.L, self.lf, np.asarray(Z, np.float64))

    def z_of(self, xt):
        return lsc.apply_binv_t(self.L, self.lf, np.asarray(xt, np.float64))

    def rho(self, Zs, rhss):
        """|b~ - S~ x~| / |b~| = |L^-1 (rhs - S z)| / |L^-1 rhs| per pair, against the dense S the device was given, in long double
        (rows of S are widened a strip at a time)."""
        q = np.longdouble
        Zq = np.stack([np.asarray(z, np.float64) for z in Zs], axis=1).astype(q)
        R = np.stack([np.asarray(b, np.float64) for b in rhss], axis=1).astype(q)
        Bq = R.copy()
        for i0 in range(0, self.d, 512):
            R[i0:i0 + 512] -= self.S[i0:i0 + 512].astype(q) @ Zq
        rt = lsc.apply_binv(self.L, self.lf, R)
        bt = lsc.apply_binv(self.L, self.lf, Bq)
        return [float(np.sqrt(np.sum(rt[:, i] ** 2)) / np.sqrt(np.sum(bt[:, i] ** 2))) for i in range(Zq.shape[1])]

    def drift(self, xt, bt, k, u):
        """10 (k + 1) u |S~|_2 |x~| / |b~|: the drift term of linear_step_check.cg_bar (delta = 0)."""
        return 10.0 * (k + 1) * u * self.St_norm * float(np.linalg.norm(xt)) / float(np.linalg.norm(bt))


@functools.lru_cache(maxsize=2)
def _system(nc, want_f32):
    return CgSystem(nc, want_f32=want_f32)


def system(nc, want_f32=None):
    """The system of `nc` cameras (the last two are kept).  want_f32: whether the fp32 matrix's rounding is needed; None: as CASES says."""
    if want_f32 is None:
        want_f32 = any(VARIANTS[v][1] for n, v, _ in CASES if n == nc)
    return _system(nc, bool(want_f32))


# ---------------------------------------------------------------------------------------------
# coarse spaces
# ---------------------------------------------------------------------------------------------
def hat_vectors(Wt, nc, G):
    """The segmented coarse space (csrc/pcg_segments.hip): (g, k) -> hat_g(camera) W~_k for k < 7 on the camera rows, the global vector 7 last.
    Cameras whose LOWER hat is a: [ceil(a nc / G), ceil((a + 1) nc / G)); camera j there has weight 1 - frac in hat a and frac in hat
    (a + 1) mod G, frac = (j G - a nc) / nc."""
    d = 6 * nc + 1
    hat = np.zeros((G, nc))
    for a in range(G):
        lo, hi = -(-a * nc // G), -(-(a + 1) * nc // G)
        j = np.arange(lo, hi)
        fr = (j * G - a * nc) / nc
        hat[a, j] += 1.0 - fr
        hat[(a + 1) % G, j] += fr
    rows = []
    for g in range(G):
        m = np.zeros(d)
        m[:6 * nc] = np.repeat(hat[g], 6)
        for k in range(NW - 1):
            rows.append(Wt[k] * m)
    rows.append(Wt[NW - 1].copy())
    return np.array(rows)


def probe_vectors(sys_, variant):
    """Wt of the probe call: None without the coarse space, the vectors with an empty focal entry in 0 .. 6 where the segmented space is asked for."""
    sym, f32, coarse, seg = VARIANTS[variant]
    return None if not coarse else sys_.Wt_seg if seg else sys_.Wt


def coarse_basis(sys_, variant):
    sym, f32, coarse, seg = VARIANTS[variant]
    if not coarse:
        return None
    fam, _, cv = route(sys_.nc, sym, f32, coarse, seg)
    W = probe_vectors(sys_, variant)
    if fam == "PCG_SEGMENTS":
        return hat_vectors(W, sys_.nc, ML_G)
    if fam == "PCG_SEGMENTS_STREAMING":
        return hat_vectors(W, sys_.nc, sg_hats(sys_.nc))
    if cv and sys_.coarse_rank < NW:          # eight vectors of lower rank: the kernels drop the dependent ones by a pivot test (coarse_inverse.h); the same span here
        return W[:sys_.coarse_rank]
    return W if cv else None


def spd_inverse(E):
    """Inverse of a small SPD matrix by Gauss-Jordan without pivot search on the Jacobi-scaled matrix, in E's precision (long double has no LAPACK)."""
    n = E.shape[0]
    s = 1.0 / np.sqrt(np.diag(E))
    a = np.concatenate([E * s[:, None] * s[None, :], np.eye(n, dtype=E.dtype)], axis=1)
    for p in range(n):
        a[p] = a[p] / a[p, p]
        col = a[:, p].copy()
        col[p] = 0
        a -= col[:, None] * a[p][None, :]
    return a[:, n:] * s[:, None] * s[None, :]


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
def pcg(op, bt, W=None, tol=TOL, max_iters=MAX_ITERS, q=np.float64, keep=(), einv_edit=None):
    """Two-level preconditioned CG of pcg_common.h in precision q on the operator `op`: (x~, iterations, {k: x~_k for k in keep}).
    einv_edit: a function applied to E^-1 (the CPU proof plants a defect there)."""
    bt = np.asarray(bt).astype(q)
    x = np.zeros_like(bt)
    r = bt.copy()
    if W is not None:
        Wq = np.asarray(W).astype(q)
        AW = op(np.ascontiguousarray(Wq.T))
        E = Wq @ AW
        Einv = spd_inverse(0.5 * (E + E.T))
        if einv_edit is not None:
            Einv = einv_edit(Einv)
        prec = lambda v: v + Wq.T @ (Einv @ (Wq @ v))
    else:
        prec = lambda v: v
    rr0 = r @ r
    kept = {}
    k = 0
    if rr0 == 0:
        return x, 0, kept
    z = prec(r)
    p = z.copy()
    rz = r @ z
    while k < max_iters:
        qv = op(p)
        alpha = rz / (p @ qv)
        x = x + alpha * p
        r = r - alpha * qv
        k += 1
        if k in keep:
            kept[k] = x.copy()
        rrn = r @ r
        if not (rrn > q(tol) * q(tol) * rr0):          # (a NaN ends the solve, as the kernels' `broke` does)
            break
        z = prec(r)
        rz2 = r @ z
        p = z + (rz2 / rz) * p
        rz = rz2
    return x, k, kept


FORCED = (1, 2, 3)


@functools.lru_cache(maxsize=64)
def reference(nc, variant, which=0):
    """(iterations in float64, iterations in long double, {k: x~_k} of the long-double run) for right-hand side `which` (0: rhs, 1: rhs2)."""
    s = system(nc)
    f32 = bool(VARIANTS[variant][1]) and 6 * nc + 1 > FAST_MAX_D
    W = coarse_basis(s, variant)
    rhs = s.rhs if which == 0 else s.rhs2
    _, k64, _ = pcg(s.op(f32, np.float64), s.bt(rhs), W, q=np.float64)
    _, kld, kept = pcg(s.op(f32, np.longdouble), s.bt(rhs, np.longdouble), W, q=np.longdouble, keep=FORCED)
    return k64, kld, kept


# ---------------------------------------------------------------------------------------------
# the verdicts (shared by the GPU test and by the CPU proof that they bite)
# ---------------------------------------------------------------------------------------------
def unit_roundoff(nc, variant):
    return U32 if VARIANTS[variant][1] and 6 * nc + 1 > FAST_MAX_D else U64


def residual_ratios(s, nc, variant, Zs, rhss, ks):
    """measured / bar of check (2) per solve: rho <= 2 tol + 10 (k + 1) u |S~|_2 |x~| / |b~|."""
    u = unit_roundoff(nc, variant)
    out = []
    for z, b, k, rho in zip(Zs, rhss, ks, s.rho(Zs, rhss)):
        bar = 2.0 * TOL + s.drift(s.xt(z), s.bt(b), k, u)
        out.append(rho / bar if np.isfinite(rho) else np.inf)
    return out


def forced_ratios(s, nc, variant, Zk, which=0):
    """measured / bar of check (4) for the iterates z_k (original unknowns) of max_iters = 1, 2, 3:
    |x~_k - x~_k,ref| / |x~_k,ref| <= kappa~ 10 (k + 1) u |S~|_2 |x~_k,ref| / |b~|  (check_step's forward-from-backward bound on the drift term)."""
    u = unit_roundoff(nc, variant)
    kept = reference(nc, variant, which)[2]
    bt = s.bt(s.rhs if which == 0 else s.rhs2)
    out = []
    for k, z in zip(FORCED, Zk):
        ref = kept[k].astype(np.float64) if k in kept else kept[max(kept)].astype(np.float64)
        err = float(np.linalg.norm(s.xt(z) - ref) / np.linalg.norm(ref))
        bar = s.kappa * s.drift(ref, bt, k, u)
        out.append(err / bar if np.isfinite(err) else np.inf)
    return out
