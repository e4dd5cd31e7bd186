"""Cases, partition, emulation and verdicts of tests/test_gpu_dist_cg_ranks.py (numpy only; proved on the CPU by tests/test_dist_cg_cases_cpu.py).

What is held: the distributed CG of the sharded forms (csrc/dist_cg.hip: k_dcg_prod8, k_dcg_start, k_dcg_prod, k_dcg_upd behind dcg_begin /
dcg_iterate) at every rank count from 1 to 8, through sfmba_dist_cg_probe: every rank of a world simulated in one process, each with the chunk of
the reduce-scatter layout the library's partition gives it, the all-reduce a sum over the ranks' buffers.  Systems, the long-double reference CG and
the bars are those of tests/cg_family_cases.py (`cf`), unchanged: the coarse basis is the eight vectors, the matrix is fp32 where d > 1280 and the
case asks for it -- which is what the distributed CG does.

The table: every row is the smallest shape that reaches one trip boundary of the kernels (the constants below are held to the source by the CPU
test).  The emulation: the PARTITIONED algorithm in float64 -- row part and transposed part per rank from that rank's rows only, identity and focal
border on rank 0 only, the partial dots p . q and W~^T q riding in the same sum, c = W~^T r updated recursively, surplus launches handing in zeros --
which shows that the bars can be met by a float64 implementation of exactly this method, and, with one defect planted, that they bite."""
import functools

import numpy as np

import cg_family_cases as cf
import linear_step_check as lsc

TOL, FORCED, MAX_ITERS = cf.TOL, cf.FORCED, cf.MAX_ITERS
SURPLUS = 6

# ---- the constants of csrc/dist_cg.hip the table is written from ----
CPW = 4                    # cameras per product workgroup (a wave each); np = ceil(ncam / CPW) + 1 rows of partial dots
LIN_STRIDE, LIN8_STRIDE = 16, 64
UPD_MAXWG = 32             # workgroups of k_dcg_start / k_dcg_upd: min(UPD_MAXWG, ceil(d / 256)), a slice of ceil(d / grid) entries each
START_ROWS_PER_PASS = 32   # k_dcg_start: `i0 += 32` over the np rows of E partials
START_STRIDE, UPD_STRIDE = 1024, 2048
MAX_WORLD = 16


def n_partial_rows(ncam):
    return -(-ncam // CPW) + 1


def upd_grid(d):
    return max(1, min(UPD_MAXWG, -(-d // 256)))


def first_of_row(I, ncam):
    """Off-diagonal upper blocks in front of block row I."""
    return I * ncam - I * (I + 1) // 2


def partition(ncam, world):
    """dcg_partition restated: (rows [world + 1], chunk_blocks).  Row I closes rank r - 1 once r / world of the blocks are reached."""
    total = ncam * (ncam - 1) // 2
    rows = [0] + [ncam] * world
    acc, r = 0, 1
    for I in range(ncam):
        if r >= world:
            break
        acc += ncam - 1 - I
        while r < world and acc * world >= total * r:
            rows[r] = I + 1
            r += 1
    big = max(first_of_row(rows[k + 1], ncam) - first_of_row(rows[k], ncam) for k in range(world))
    return rows, max(big, 1)


# (ncam, worlds, variants, what the row sits on).  Variants: 64 / 32 = blocks and focal row in fp64 / fp32, c / n = with / without the coarse space.
_ROWS = [
    (1, (1, 3), ("64c",), "d = 7: no off-diagonal block, np = 2, eight coarse vectors of rank three; world 3: ranks without rows"),
    (2, (8,), ("64c", "64n"), "d = 13: one block; seven ranks own no block, six of them no row"),
    (5, (4,), ("64c",), "d = 31: ncam % CPW = 1 (a product workgroup with one live wave); rows 0 .. 4 split over 4 ranks"),
    (66, (1, 3), ("64c", "64n"), "d = 397: second 64-lane trip in the row part (row 0: 65 blocks) and, at world 1, in the transposed part (column 65: 65 rows)"),
    (124, (8,), ("64c",), "d = 745: np = 32, one pass of k_dcg_start's sum of the E partials"),
    (125, (8,), ("64c",), "d = 751: np = 33, two passes of it"),
    (171, (2,), ("64c",), "d = 1027: second 1024-stride pass of k_dcg_start"),
    (214, (4,), ("64c", "32c", "32n"), "d = 1285: first size with fp32 blocks and focal row"),
    (252, (8,), ("64c",), "d = 1513: np = 64, one lane trip of k_dcg_upd's sum of the partial dots"),
    (253, (8,), ("64c",), "d = 1519: np = 65, two lane trips of it"),
    (342, (5,), ("64c", "32c"), "d = 2053: second 2048-stride pass of k_dcg_upd; a world that divides nothing"),
    (1366, (8,), ("64c", "32c"), "d = 8197: update grid capped at UPD_MAXWG, slices of 257 entries; the system cg_family_cases already builds"),
]
CASES = [(nc, w, v) for nc, worlds, vs, _ in _ROWS for w in worlds for v in vs]
WHY = {nc: why for nc, _, _, why in _ROWS}
STRUCTURED_FROM = 1000     # the emulation runs the structured operator only from here (no dense S~ of 8197^2 on the CPU): the partition is then not emulated


def case_id(case):
    return "nc%d-w%d-%s" % case


def cf_variant(v):
    """The row of cf.VARIANTS with this matrix type and coarse space (the streaming family's: the eight vectors, fp32 where d > 1280)."""
    return "st" + v


def wants_f32(nc):
    return any(v.startswith("32") for n, _, v in CASES if n == nc)


def system(nc):
    return cf.system(nc, wants_f32(nc))


def is_f32(nc, v):
    return v.startswith("32") and 6 * nc + 1 > cf.FAST_MAX_D


def coarse(s, v):
    """Wt of the probe call (all eight vectors) and the basis of the restatements (cf.coarse_basis: a basis of their span)."""
    return (s.Wt, cf.coarse_basis(s, cf_variant(v))) if v.endswith("c") else (None, None)


@functools.lru_cache(maxsize=64)
def reference(nc, v, which=0):
    """cf.reference for the table's systems (cf.system keeps two: asked for again with the fp32 rounding where this table needs it)."""
    system(nc)
    return cf.reference(nc, cf_variant(v), which)


# ---------------------------------------------------------------------------------------------
# the partitioned product
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _dense(nc, f32_blocks, f32_focal):
    """(U: the strictly upper off-diagonal camera blocks of S~ as a [d - 1, d - 1] array, zero elsewhere; focal row [d - 1]) as the device holds them:
    the library's transform of the dense S, then rounded to fp32 where asked."""
    s = system(nc)
    St = np.triu(lsc.transformed_matrix(s.S, s.L, s.lf))
    fo = s.d - 1
    focal = St[:fo, fo].copy()
    U = St[:fo, :fo]
    for j in range(nc):
        U[6 * j:6 * j + 6, 6 * j:6 * j + 6] = 0.0          # the diagonal blocks are the identity, added as such
    if f32_blocks:
        U = U.astype(np.float32).astype(np.float64)
    if f32_focal:
        focal = focal.astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(U), focal


def partial_products(nc, v, world, defect=None):
    """V [d] or [d, m] -> the list over ranks of their partial S~ V, as k_dcg_prod / k_dcg_prod8 form them.  defect: None or
    'identity' (rank 1 adds the identity too), 'transposed' (the transposed part stops one row early), 'focal' (every rank adds the focal entry),
    'mixed32' (fp32 blocks with an fp64 focal row)."""
    s = system(nc)
    d, fo = s.d, s.d - 1
    rows, _ = partition(nc, world)
    if nc >= STRUCTURED_FROM:
        assert defect is None
        op = s.op(is_f32(nc, v), np.float64)
        return lambda V: [op(V)] + [np.zeros_like(np.asarray(V, np.float64))] * (world - 1)
    f32 = is_f32(nc, v)
    U, focal = _dense(nc, f32 or defect == "mixed32", f32 and defect != "mixed32")

    def prod(V):
        V = np.asarray(V, np.float64)
        ex = (slice(None),) + (None,) * (V.ndim - 1)
        out = []
        for k in range(world):
            r0, r1 = rows[k], rows[k + 1]
            y = np.zeros_like(V)
            y[6 * r0:6 * r1] += U[6 * r0:6 * r1] @ V[:fo]                         # row part: blocks (c, J > c) of the owned rows
            Ut = U[6 * r0:6 * r1]
            if defect == "transposed":                                               # ... runs to min(row1, c) - 1: the last owned row above c is left out
                Ut = Ut.copy()
                for c in range(r0 + 1, nc):
                    last = min(r1, c) - 1
                    Ut[6 * (last - r0):6 * (last - r0) + 6, 6 * c:6 * c + 6] = 0.0
            y[:fo] += Ut.T @ V[6 * r0:6 * r1]                                      # transposed part: blocks (I, c), I owned and < c
            if k == 0 or (defect == "identity" and k == 1):
                y[:fo] += V[:fo]
            if k == 0:
                y[:fo] += focal[ex] * V[fo]
            if k == 0 or defect == "focal":
                y[fo] += V[fo] + focal @ V[:fo]
            out.append(y)
        return out

    return prod


# ---------------------------------------------------------------------------------------------
# the emulation of dcg_begin / dcg_iterate over all ranks
# ---------------------------------------------------------------------------------------------
def emulate(prod, world, bt, W, max_iters, surplus=0, tol=TOL, stale=False):
    """The distributed CG in float64: (x~, iterations, finite).  prod: partial_products(...); W: the coarse basis or None.
    The replicated part is computed once (the replicas are identical by construction here; the device is checked for it).
    stale: a surplus launch's product leaves its buffer as the previous all-reduce left it -- the sum, which the in-place all-reduce then multiplies
    by the world size -- and the update's gate is one launch late (it acts on a flag raised by the launch in front of it only from the second surplus
    launch on).  With the update's gate intact the iterate cannot see the stale buffer at all; this is the form in which it could."""
    bt = np.asarray(bt, np.float64)
    d = bt.shape[0]
    x, r = np.zeros(d), bt.copy()
    rr = float(bt @ bt)
    c = mu = Einv = None
    rz = rr
    p = bt.copy()
    if W is not None:
        parts = prod(np.ascontiguousarray(W.T))                      # k_dcg_prod8: S~ W~ per rank, with the rank's part of E behind it
        E = np.zeros((W.shape[0], W.shape[0]))
        for y in parts:                                              # the all-reduce: rank order
            E = E + W @ y
        Einv = cf.spd_inverse(0.5 * (E + E.T))
        c = W @ bt
        mu = Einv @ c
        rz = rr + float(c @ mu)
        p = bt + W.T @ mu
    base = rr
    dn = 1 if rr == 0.0 else 0                                        # PF_DONE: the number of the first launch with nothing left to do
    iters = 0
    q, lin = np.zeros(d), np.zeros(1 + (0 if W is None else W.shape[0]))

    def launch(no):
        nonlocal x, r, p, c, mu, rz, dn, iters, q, lin
        done = dn != 0 and dn <= no
        if done:
            if stale:
                q, lin = world * q, world * lin
            else:
                q, lin = np.zeros(d), np.zeros_like(lin)             # zeros from every rank
        else:
            q, lin = np.zeros(d), np.zeros_like(lin)
            for y in prod(p):                                         # the partial products and, LINEAR in them, the partial dots: one sum
                q = q + y
                lin = lin + np.concatenate([[p @ y], W @ y if W is not None else []])
        if (dn != 0 and dn < no) if stale else done:
            return
        pq = lin[0]
        broke = not (pq > 0.0)
        alpha = 0.0 if broke else rz / pq
        rn = r - alpha * q
        rrn = float(rn @ rn)
        rzn = rrn
        if W is not None:
            c = c - alpha * lin[1:]
            mu = Einv @ c
            rzn = rrn + float(c @ mu)
        fin = broke or not (rrn == rrn) or rrn <= tol * tol * base
        x = x + alpha * p
        r = rn
        if not fin:
            p = rn + (W.T @ mu if W is not None else 0.0) + (rzn / rz) * p
        rz = rzn
        iters = no
        if fin:
            dn = no + 1

    launched = 0
    while launched < max_iters and dn == 0:
        launched += 1
        launch(launched)
    if dn == 0:
        dn = launched + 1                                             # the probe ends a solve stopped by its cap as a converging launch would
    for no in range(launched + 1, launched + 1 + surplus):
        launch(no)
    return x, iters, bool(np.all(np.isfinite(x)) and np.all(np.isfinite(q)))


# ---------------------------------------------------------------------------------------------
# the verdicts (shared by the GPU test and by the CPU proof that they bite)
# ---------------------------------------------------------------------------------------------
def verdicts(s, nc, v, runs):
    """runs: dict of what the three calls (and the forced call again with surplus = 0) returned, transformed unknowns:
        reuse    (Xt [3, d], iters [3])                 b, 0, b2                          max_iters 200
        forced   (Xt [4, d], iters [4]), forced0, poison   b2, then b after 1, 2, 3 iterations (forced / poison: SURPLUS launches behind each)
    Returns (dict of measured / bar ratios and counts for the report line, list of failed verdicts)."""
    cv = cf_variant(v)
    k_ref, k_ld, _ = reference(nc, v, 0)
    k2_ref = reference(nc, v, 1)[0]
    (X, it), (Xf, it_f), (Xf0, it_f0), (Xp, it_p) = runs["reuse"], runs["forced"], runs["forced0"], runs["poison"]
    z = lambda xt: s.z_of(xt)
    rr = cf.residual_ratios(s, nc, cv, [z(X[0]), z(X[2]), z(Xf[0]), z(Xp[0])], [s.rhs, s.rhs2, s.rhs2, s.rhs2], [it[0], it[2], it_f[0], it_p[0]])
    fr = cf.forced_ratios(s, nc, cv, [z(x) for x in Xf[1:4]])
    fp = cf.forced_ratios(s, nc, cv, [z(x) for x in Xp[1:4]])
    finite = bool(np.all(np.isfinite(X)) and np.all(np.isfinite(Xf)) and np.all(np.isfinite(Xp)))
    failed = []
    if not max(rr) <= 1.0:
        failed.append("2 true residual %s" % rr)
    if not (abs(int(it[0]) - k_ref) <= 2 and abs(int(it_f[0]) - k2_ref) <= 2):
        failed.append("3 iterations %d / %d, %d / %d" % (it[0], k_ref, it_f[0], k2_ref))
    if not (list(it_f[1:]) == list(FORCED) and max(fr) <= 1.0):
        failed.append("4 forced iterates %s %s" % (list(it_f), fr))
    if not (np.array_equal(Xf, Xf0) and list(it_f) == list(it_f0) and finite):
        failed.append("5 surplus launches moved the iterate (or left something non-finite)")
    if not (it[1] == 0 and not np.any(X[1]) and abs(int(it[2]) - int(it_f[0])) <= 1):
        failed.append("7 reuse: zero rhs %d iterations, b2 behind it %d / alone %d" % (it[1], it[2], it_f[0]))
    if not (list(it_p) == list(it_f) and np.array_equal(Xp, Xf) and max(fp) <= 1.0):
        failed.append("8 poison: iterations %s / %s, forced %s" % (list(it_p), list(it_f), fp))
    report = dict(it=int(it[0]), k_ref=k_ref, k_ld=k_ld, it2=int(it[2]), k2_ref=k2_ref, alone=int(it_f[0]), rr=rr, fr=fr, fp=fp)
    return report, failed


def report_line(tag, case, rows, rep, extra=""):
    nc, w, v = case
    return "%s %-14s d %4d world %d rows %s  iters %2d/%2d (ld %2d)  b2 %2d/%2d alone %2d  rho %s  forced %s  poison %s%s" % (
        tag, case_id(case), 6 * nc + 1, w, ",".join(str(r) for r in rows), rep["it"], rep["k_ref"], rep["k_ld"], rep["it2"], rep["k2_ref"], rep["alone"],
        " ".join("%.1e" % x for x in rep["rr"]), " ".join("%.1e" % x for x in rep["fr"]), " ".join("%.1e" % x for x in rep["fp"]), extra)


def emulated_runs(nc, w, v, defect=None):
    """The calls of the device test made with the emulation (the poison call is the forced call: there is no padding to poison here)."""
    s = system(nc)
    _, W = coarse(s, v)
    stale = defect == "stale"
    prod = partial_products(nc, v, w, None if stale else defect)
    b, b2, zero = s.bt(s.rhs), s.bt(s.rhs2), np.zeros(s.d)

    def call(rhss, caps, surplus):
        out = [emulate(prod, w, r, W, k, surplus, stale=stale) for r, k in zip(rhss, caps)]
        return np.stack([o[0] for o in out]), np.array([o[1] for o in out])

    full = MAX_ITERS
    runs = {"reuse": call([b, zero, b2], [full] * 3, 0),
            "forced": call([b2, b, b, b], [full] + list(FORCED), SURPLUS),
            "forced0": call([b2, b, b, b], [full] + list(FORCED), 0)}
    runs["poison"] = runs["forced"]
    return s, runs
