"""CPU restatement of the float matcher's contract (include/sfmba.h, sfmba_match_features_l2) -- TEST INFRASTRUCTURE ONLY.

cv::BFMatcher with NORM_L2, knnMatch with K = 2, then the ratio test `best.distance < NN_MATCH_RATIO * second.distance`, over
a squared distance that the contract defines operation by operation:

    acc = 0.0f;  for k ascending:  t = a[k] - b[k] (fp32);  acc = fmaf(t, t, acc);   dist = sqrt(acc) correctly rounded in fp32

Stated twice, independently, and held equal bit for bit by tests/test_match_l2_oracle_cpu.py:

  route A  sq_distances (numpy): t as float32; the fma as the EXACT double product (two 24-bit significands: 48 bits) plus acc, the
           double sum ROUNDED TO ODD (TwoSum error term; if it is non-zero and the sum's last bit is even, one ulp towards the
           error), then cast to float32 -- rounding to odd at 53 >= 24 + 2 bits makes the second rounding the only one that counts
  route B  csrc/match_l2_math.h compiled for the host (tools/micro/match_l2_math_host.hip): the code the kernel runs, through
           the C library's fmaf

The top-2 is stated twice as well (knn_lexsort on (bits of s, j); knn_insertion with a strict <), plus a fast form on combined keys
for the large GPU comparisons.  Allowed importers: tests/ and tools/.
"""
import numpy as np

RATIO_F32 = float(np.float32(0.8))       # NN_MATCH_RATIO = 0.8f widened to double: 0.800000011920929
CHUNK = 128


def fma_sq(t, acc):
    """float32 fmaf(t, t, acc), elementwise, for float32 arrays t and acc >= 0 (or +inf)."""
    t64 = t.astype(np.float64)
    p = t64 * t64                                            # exact: 48 significant bits, exponent well inside double
    a = acc.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + a
        bb = s - p
        err = (p - (s - bb)) + (a - bb)                      # TwoSum: p + a = s + err exactly (finite operands)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.uint64) & np.uint64(1)) == 0)
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)        # round to odd
        return s.astype(np.float32)


def sq_distances_chain(dq, dt):
    """[len(dq), len(dt)] float32 squared distances s(q, j) of float32 rows, by the contract's chain (route A)."""
    dq = np.ascontiguousarray(dq, np.float32)
    dt = np.ascontiguousarray(dt, np.float32)
    acc = np.zeros((len(dq), len(dt)), np.float32)
    for k in range(dq.shape[1]):
        t = dq[:, k][:, None] - dt[:, k][None, :]            # one fp32 subtraction
        acc = fma_sq(t, acc)
    return acc


def small_integers(dq, dt):
    """True if every value is an integer and no partial sum of any chain can reach 2^24: then every t, every t * t and every acc is
    an integer below 2^24, NOTHING in the chain rounds, and s is the exact sum of squares."""
    dq = np.asarray(dq, np.float64); dt = np.asarray(dt, np.float64)
    if dq.size == 0 or dt.size == 0:
        return False
    if not (np.all(dq == np.floor(dq)) and np.all(dt == np.floor(dt))):
        return False
    span = max(dq.max(), dt.max()) - min(dq.min(), dt.min())
    return span * span * dq.shape[1] < 2.0 ** 24


def sq_distances(dq, dt, shortcut=True):
    """The chain; rows of small integers (0 / 1 rows, SIFT-like 0..255 rows of up to 257 columns) go through the exact sum of squares
    |a|^2 + |b|^2 - 2 a.b in float64 instead, which is the same number (small_integers; held equal to the chain by
    tests/test_match_l2_oracle_cpu.py).  Nothing but integers below 2^53 occurs in it."""
    if shortcut and small_integers(dq, dt):
        a = np.asarray(dq, np.float64); b = np.asarray(dt, np.float64)
        s = (a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :] - 2.0 * (a @ b.T)
        return s.astype(np.float32)
    return sq_distances_chain(dq, dt)


def row_sq(a, b):
    """s of row i of a against row i of b (float32 [n])."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    acc = np.zeros(len(a), np.float32)
    for k in range(a.shape[1]):
        acc = fma_sq(a[:, k] - b[:, k], acc)
    return acc


def bits(s):
    """The order of s >= +0 is the order of its bit pattern as an unsigned integer (+inf last)."""
    return np.ascontiguousarray(s, np.float32).view(np.uint32)


def dist(s):
    """The correctly rounded fp32 square root (numpy's float32 sqrt is the hardware's, which is)."""
    return np.sqrt(np.asarray(s, np.float32))


def _empty(nq):
    return np.full(nq, -1, np.int64), np.full(nq, np.inf, np.float32), np.full(nq, -1, np.int64), np.full(nq, np.inf, np.float32)


def knn_lexsort(dq, dt):
    """best / second (index, s) per query from a lexsort on (bits of s, j).  -1 / inf where there is none."""
    nq, nt = len(dq), len(dt)
    i1, s1, i2, s2 = _empty(nq)
    if nt == 0:
        return i1, s1, i2, s2
    j = np.arange(nt)
    for q0 in range(0, nq, CHUNK):
        S = sq_distances(dq[q0:q0 + CHUNK], dt)
        B = bits(S)
        for r in range(len(S)):
            order = np.lexsort((j, B[r]))                    # primary key the bits of s, then j
            i1[q0 + r] = order[0]; s1[q0 + r] = S[r, order[0]]
            if nt >= 2:
                i2[q0 + r] = order[1]; s2[q0 + r] = S[r, order[1]]
    return i1, s1, i2, s2


def knn_insertion(dq, dt):
    """The same by the K = 2 insertion loop over train rows in ascending index with a strict < on s (floats, +inf compares last;
    the first of equal distances stays ahead), as OpenCV's batchDistance does."""
    nq, nt = len(dq), len(dt)
    i1, s1, i2, s2 = _empty(nq)
    have1 = np.zeros(nq, bool); have2 = np.zeros(nq, bool)
    for q0 in range(0, nq, CHUNK):
        S = sq_distances(dq[q0:q0 + CHUNK], dt)
        sl = slice(q0, q0 + CHUNK)
        a1, b1, a2, b2, h1, h2 = i1[sl], s1[sl], i2[sl], s2[sl], have1[sl], have2[sl]
        for j in range(nt):
            d = S[:, j]
            first = ~h1 | (d < b1)                           # an empty slot takes anything, +inf included
            second = ~first & (~h2 | (d < b2))
            a2[:] = np.where(first, a1, np.where(second, j, a2))
            b2[:] = np.where(first, b1, np.where(second, d, b2))
            h2[:] = np.where(first, h1, h2 | second)
            a1[:] = np.where(first, j, a1)
            b1[:] = np.where(first, d, b1)
            h1[:] = True
    return i1, s1, i2, s2


def knn_keys(dq, dt):
    """Fast form: the two smallest combined keys (bits of s << 32) | j per query row (the same (s, j) order)."""
    nq, nt = len(dq), len(dt)
    i1, s1, i2, s2 = _empty(nq)
    if nt == 0:
        return i1, s1, i2, s2
    j = np.arange(nt, dtype=np.uint64)
    for q0 in range(0, nq, CHUNK):
        S = sq_distances(dq[q0:q0 + CHUNK], dt)
        K = (bits(S).astype(np.uint64) << np.uint64(32)) | j[None, :]
        if nt >= 2:
            two = np.sort(np.partition(K, 1, axis=1)[:, :2], axis=1)
            i2[q0:q0 + CHUNK] = (two[:, 1] & np.uint64(0xffffffff)).astype(np.int64)
            s2[q0:q0 + CHUNK] = (two[:, 1] >> np.uint64(32)).astype(np.uint32).view(np.float32)
            k1 = two[:, 0]
        else:
            k1 = K[:, 0]
        i1[q0:q0 + CHUNK] = (k1 & np.uint64(0xffffffff)).astype(np.int64)
        s1[q0:q0 + CHUNK] = (k1 >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return i1, s1, i2, s2


def ratio_test(i1, s1, i2, s2, nt, ratio=RATIO_F32):
    """prunedMatching: [(q, j_best, bits of float32 dist_best)] in ascending q.  No second neighbour (nt < 2): nothing is kept."""
    if nt < 2:
        return []
    d1, d2 = dist(s1), dist(s2)
    with np.errstate(invalid="ignore"):
        keep = d1.astype(np.float64) < ratio * d2.astype(np.float64)
    q = np.nonzero(keep)[0]
    return list(zip(q.tolist(), i1[q].tolist(), d1[q].view(np.uint32).tolist()))


def match_pair(dq, dt, ratio=RATIO_F32, knn=knn_keys):
    if len(dq) == 0 or len(dt) == 0:
        return []
    return ratio_test(*knn(dq, dt), len(dt), ratio)


def match_features(descs, pairs=None, ratio=RATIO_F32, knn=knn_keys):
    """[((l, r), [(q, j, bits of d), ...]), ...] in the order of the pair list (None = all i < j).  A pair that repeats is computed once."""
    if pairs is None:
        pairs = [(i, j) for i in range(len(descs)) for j in range(i + 1, len(descs))]
    memo = {}
    out = []
    for l, r in pairs:
        key = (int(l), int(r))
        if key not in memo:
            memo[key] = match_pair(descs[l], descs[r], ratio, knn)
        out.append((key, memo[key]))
    return out


def padded_dims(dims, pad=32):
    return -(-dims // pad) * pad


def stage_rows(dims, stage_floats=8192, group=16):
    """Train rows per LDS stage of the unit: min(256, floor(8192 / padded dims / 16) * 16)."""
    return min(256, stage_floats // padded_dims(dims) // group * group)


def plan(rows_per_pair, train_per_pair, tile=512, batch_tiles=256, target_blocks=2048, min_slice_rows=256, max_slices=32):
    """The batch / slice plan stated in include/sfmba.h: [(n_tiles, n_slices)] per batch.  Pairs with < 2 train rows have no tiles."""
    items = []
    for nq, nt in zip(rows_per_pair, train_per_pair):
        if nt >= 2:
            items += [nt] * ((nq + tile - 1) // tile)
    out = []
    for b0 in range(0, len(items), batch_tiles):
        b = items[b0:b0 + batch_tiles]
        by_rows = max(1, -(-max(b) // min_slice_rows))
        by_fill = -(-target_blocks // len(b))
        out.append((len(b), max(1, min(by_fill, by_rows, max_slices))))
    return out


# ---- the six kinds of rows the routes are compared on ---------------------------------------------------------------------------
KINDS = ("uniform", "sift", "unit", "tiny", "huge", "mixed")


def rows_of(kind, rng, n, dims):
    """n float32 rows of `dims` columns: uniform in [-1, 1), SIFT-like integers 0..255, unit-norm, 1e-21 scale (subnormal squares),
    1e19 scale (+inf sums), mixed magnitudes (1e-30 .. 1e18 per element)."""
    if kind == "uniform":
        x = rng.uniform(-1, 1, (n, dims))
    elif kind == "sift":
        x = np.minimum(255, np.floor(rng.exponential(30.0, (n, dims))))
    elif kind == "unit":
        x = rng.normal(size=(n, dims))
        x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)
    elif kind == "tiny":
        x = rng.uniform(-1, 1, (n, dims)) * 1e-21
    elif kind == "huge":
        x = rng.uniform(-1, 1, (n, dims)) * 1e19
    elif kind == "mixed":
        x = rng.uniform(-1, 1, (n, dims)) * 10.0 ** rng.integers(-30, 19, (n, dims))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, np.float32)
