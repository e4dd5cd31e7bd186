"""CPU restatement of the feature matcher's contract (include/sfmba.h, sfmba_match_features) -- TEST INFRASTRUCTURE ONLY.

SfM2DFeatureUtilities::matchFeatures (SfMToyLib/SfM2DFeatureUtilities.cpp:53-71): BFMatcher("BruteForce-Hamming").knnMatch
with K = 2, then the ratio test `best.distance < NN_MATCH_RATIO * second.distance` (float distance, double ratio).  Stated
twice, independently, and held equal by tests/test_feature_match_cpu.py:

  knn_insertion  the K = 2 insertion loop of a brute-force kNN over train rows in ascending index with a strict `<`
                 (the first of equal distances stays ahead), as OpenCV's batchDistance does
  knn_lexsort    the two smallest (d, j) pairs from a lexsort on (d, j)

A third, fast form (knn_keys: the two smallest combined keys d * nt + j) serves the large GPU comparisons and is held equal
to the other two as well.  All work in chunks of query rows, so a 5000 x 5000 pair costs seconds, not memory.  Allowed importers: tests/ and tools/.
"""
import numpy as np

RATIO_F32 = float(np.float32(0.8))       # NN_MATCH_RATIO = 0.8f widened to double: 0.800000011920929
CHUNK = 256


def _words(d):
    """uint8 rows -> uint64 words (zero padding to whole words adds nothing to a distance)."""
    d = np.asarray(d, np.uint8)
    pad = (-d.shape[1]) % 8
    if pad:
        d = np.concatenate([d, np.zeros((d.shape[0], pad), np.uint8)], axis=1)
    return np.ascontiguousarray(d).view(np.uint64)


def distances(dq, dt):
    """[len(dq), len(dt)] Hamming distances of uint8 rows (popcount of the XOR over the row's bytes)."""
    x = np.bitwise_xor(_words(dq)[:, None, :], _words(dt)[None, :, :])
    return np.bitwise_count(x).sum(axis=2, dtype=np.int64)


def knn_insertion(dq, dt):
    """best / second (index, distance) per query: K = 2 insertion with a strict <.  -1 / large where there is none."""
    nq, nt = len(dq), len(dt)
    big = np.iinfo(np.int64).max
    i1 = np.full(nq, -1, np.int64); d1 = np.full(nq, big, np.int64)
    i2 = np.full(nq, -1, np.int64); d2 = np.full(nq, big, np.int64)
    for q0 in range(0, nq, CHUNK):
        D = distances(dq[q0:q0 + CHUNK], dt)
        a1, b1, a2, b2 = i1[q0:q0 + CHUNK], d1[q0:q0 + CHUNK], i2[q0:q0 + CHUNK], d2[q0:q0 + CHUNK]
        for j in range(nt):                       # train rows in ascending index, vectorised over the chunk's queries
            d = D[:, j]
            first = d < b1
            second = ~first & (d < b2)
            a2[:] = np.where(first, a1, np.where(second, j, a2))
            b2[:] = np.where(first, b1, np.where(second, d, b2))
            a1[:] = np.where(first, j, a1)
            b1[:] = np.where(first, d, b1)
    return i1, d1, i2, d2


def knn_lexsort(dq, dt):
    """The same from a lexsort on (d, j) per query row."""
    nq, nt = len(dq), len(dt)
    big = np.iinfo(np.int64).max
    i1 = np.full(nq, -1, np.int64); d1 = np.full(nq, big, np.int64)
    i2 = np.full(nq, -1, np.int64); d2 = np.full(nq, big, np.int64)
    if nt == 0:
        return i1, d1, i2, d2
    j = np.arange(nt)
    for q0 in range(0, nq, CHUNK):
        D = distances(dq[q0:q0 + CHUNK], dt)
        for r in range(len(D)):
            order = np.lexsort((j, D[r]))         # primary key d, then j
            i1[q0 + r] = order[0]; d1[q0 + r] = D[r, order[0]]
            if nt >= 2:
                i2[q0 + r] = order[1]; d2[q0 + r] = D[r, order[1]]
    return i1, d1, i2, d2


def knn_keys(dq, dt):
    """Fast form for large pairs: the two smallest of the combined key d * nt + j (the same (d, j) order) per query row."""
    nq, nt = len(dq), len(dt)
    big = np.iinfo(np.int64).max
    i1 = np.full(nq, -1, np.int64); d1 = np.full(nq, big, np.int64)
    i2 = np.full(nq, -1, np.int64); d2 = np.full(nq, big, np.int64)
    if nt == 0:
        return i1, d1, i2, d2
    j = np.arange(nt, dtype=np.int64)
    for q0 in range(0, nq, CHUNK):
        K = distances(dq[q0:q0 + CHUNK], dt) * nt + j[None, :]
        if nt >= 2:
            two = np.sort(np.partition(K, 1, axis=1)[:, :2], axis=1)
            i2[q0:q0 + CHUNK] = two[:, 1] % nt; d2[q0:q0 + CHUNK] = two[:, 1] // nt
            k1 = two[:, 0]
        else:
            k1 = K[:, 0]
        i1[q0:q0 + CHUNK] = k1 % nt; d1[q0:q0 + CHUNK] = k1 // nt
    return i1, d1, i2, d2


def ratio_test(i1, d1, i2, d2, nt, ratio=RATIO_F32):
    """prunedMatching: [(q, j_best, float32 d_best)] in ascending q.  No second neighbour (nt < 2): nothing is kept."""
    if nt < 2:
        return []
    keep = d1.astype(np.float64) < ratio * d2.astype(np.float64)
    q = np.nonzero(keep)[0]
    return list(zip(q.tolist(), i1[q].tolist(), d1[q].astype(np.float32).tolist()))


def match_pair(dq, dt, ratio=RATIO_F32, knn=knn_lexsort):
    if len(dq) == 0 or len(dt) == 0:
        return []
    return ratio_test(*knn(dq, dt), len(dt), ratio)


def match_features(descs, pairs=None, ratio=RATIO_F32, knn=knn_lexsort):
    """[((l, r), [(q, j, d), ...]), ...] in the order of the pair list (None = all i < j)."""
    if pairs is None:
        pairs = [(i, j) for i in range(len(descs)) for j in range(i + 1, len(descs))]
    return [((int(l), int(r)), match_pair(descs[l], descs[r], ratio, knn)) for l, r in pairs]


def plan(rows_per_pair, train_per_pair, tile=512, batch_tiles=512, target_blocks=4096, min_slice_rows=256, max_slices=32):
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
