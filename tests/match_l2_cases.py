"""The case table of the float matcher's tests (tests/test_match_l2_oracle_cpu.py, tests/test_gpu_match_l2.py) -- TEST INFRASTRUCTURE ONLY.

(query rows, train rows, dims).  Query rows from both sides of the 512-row tile; train rows from both sides of the 256-row slice
bound, of the 16-row accumulator group and of the LDS stage (min(256, floor(8192 / padded dims / 16) * 16) rows: 128 at 33 columns,
64 at 128, 48 at 129, 16 at 512); dims from both sides of the 32-column padding, of the 64-column register window (up to 64 columns
the query rows stay in registers, above they are reloaded: two kernels) and the largest.  Not the full product: every value appears
at least twice and every edge appears with an odd dims (checked by the CPU test)."""
import numpy as np

import match_l2_oracle as lo

QUERY_ROWS = (0, 1, 2, 511, 512, 513)
TRAIN_ROWS = (0, 1, 2, 15, 16, 17, 47, 48, 49, 127, 128, 129, 255, 256, 257, 700)
DIMS = (1, 2, 3, 31, 32, 33, 64, 65, 128, 129, 512)

CASES = [
    (0, 255, 3), (1, 0, 31), (0, 2, 128), (2, 0, 32), (2, 1, 129), (1, 2, 1), (2, 2, 33), (1, 1, 65),
    (511, 255, 1), (512, 256, 31), (513, 257, 33), (511, 256, 2), (512, 257, 129), (513, 255, 3),
    (513, 700, 129),                                         # 2 tiles, 3 slices of 234 rows (asserted through the restated plan)
    (2, 700, 2),
    (37, 15, 33), (37, 16, 512), (37, 17, 129), (5, 15, 512), (5, 17, 65), (3, 16, 3),
    (9, 47, 129), (9, 48, 129), (9, 49, 129), (33, 47, 64), (33, 48, 128), (33, 49, 32),
    (9, 127, 33), (9, 128, 33), (9, 129, 33), (20, 127, 64), (20, 128, 1), (20, 129, 128),
    (70, 130, 64), (70, 130, 65), (40, 33, 512), (511, 2, 31), (512, 17, 2), (1, 257, 32),
]
SLICED = (513, 700, 129)


def case_rows(index):
    """[query rows, train rows] of case `index`, float32: the kind of values cycles through lo.KINDS with the case, and about half
    of the query rows are slightly disturbed copies of train rows, so that matches are kept."""
    nq, nt, dims = CASES[index]
    rng = np.random.default_rng(1000 + index)
    kind = lo.KINDS[index % len(lo.KINDS)]
    t = lo.rows_of(kind, rng, nt, dims)
    q = lo.rows_of(kind, rng, nq, dims)
    if nt and nq:
        src = rng.integers(0, nt, nq)
        take = rng.random(nq) < 0.5
        q[take] = t[src[take]]
        rows, col = np.flatnonzero(take), rng.integers(0, dims, nq)[take]
        if kind == "sift":
            q[rows, col] += np.float32(1.0)                  # stays an integer
        else:
            q[rows, col] *= np.float32(1.0 + 2.0 ** -10)
        if nt > 3:
            t[nt // 2] = t[1]                                # a duplicated train row
    return [np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)]
