"""tests/dist_cg_cases.py is what it claims to be, checked without a GPU: its constants are the source's, every table row sits on the boundary it
names, the restated partition is a partition, tests/test_gpu_dist_cg_ranks.py runs every row, the float64 emulation of the PARTITIONED algorithm
passes every verdict at every row (the bars are attainable) -- and the same emulation with one defect planted does not, at the smallest row where
that defect can act.  The `dcgemu` lines this file prints are the CPU half of profiles/dist_cg_ranks.txt."""
import os
import re

import numpy as np
import pytest

import cg_family_cases as cf
import dist_cg_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfm-toy-library_amd", "csrc")


def test_constants_are_the_sources():
    text = open(os.path.join(CSRC, "dist_cg.hip")).read()
    g = lambda n: int(re.search(r"constexpr int %s = (\d+);" % n, text).group(1))
    assert (dc.CPW, dc.LIN_STRIDE, dc.LIN8_STRIDE, dc.UPD_MAXWG) == (g("CPW"), g("LIN_STRIDE"), g("LIN8_STRIDE"), g("UPD_MAXWG"))
    assert "g->np = (ncam + CPW - 1) / CPW + 1;" in text
    assert "std::max(1, std::min(UPD_MAXWG, (d + 255) / 256))" in text
    assert "for (int i0 = part; i0 < np; i0 += %d)" % dc.START_ROWS_PER_PASS in text
    assert "for (int i0 = tid; i0 < d; i0 += %d)" % dc.START_STRIDE in text and "for (int i0 = tid; i0 < d; i0 += %d)" % dc.UPD_STRIDE in text
    assert "for (int i = lane; i < np; i += 64)" in text and "J < ncam; J += 64" in text and "I < iend; I += 64" in text
    head = open(os.path.join(CSRC, "dist_cg.h")).read()
    assert "constexpr int DCG_PROBE_MAX_WORLD = %d;" % dc.MAX_WORLD in head
    # fp32 where the dense families store fp32: the fast family's bound, which cf holds to pcg_common.h
    assert cf.FAST_MAX_D == 1280


def test_every_row_sits_on_the_boundary_it_names():
    assert len({dc.case_id(c) for c in dc.CASES}) == len(dc.CASES)
    np_of, d_of = dc.n_partial_rows, lambda nc: 6 * nc + 1
    assert np_of(1) == 2 and dc.partition(1, 3)[0] == [0, 1, 1, 1]                       # ranks without rows
    rows2, chunk2 = dc.partition(2, 8)
    assert rows2 == [0] + [1] * 7 + [2] and chunk2 == 1                                    # one block, on rank 0; rank 7 owns the last row, which has none
    assert 5 % dc.CPW == 1
    rows5 = dc.partition(5, 4)[0]
    assert rows5[0] == 0 and rows5[-1] == 5 and len(set(rows5)) >= 4                        # at least three ranks own rows
    assert 66 - 1 == 65 > 64                                                                # row 0 of 66 cameras: 65 blocks; column 65: 65 rows above it
    assert np_of(124) == dc.START_ROWS_PER_PASS and np_of(125) == dc.START_ROWS_PER_PASS + 1
    assert d_of(171) == dc.START_STRIDE + 3 and d_of(170) <= dc.START_STRIDE
    assert d_of(213) <= cf.FAST_MAX_D < d_of(214)
    assert np_of(252) == 64 and np_of(253) == 65
    assert d_of(342) == dc.UPD_STRIDE + 5 and d_of(341) <= dc.UPD_STRIDE
    assert dc.upd_grid(d_of(1366)) == dc.UPD_MAXWG and -(-d_of(1366) // dc.UPD_MAXWG) == 257 and -(-d_of(1365) // dc.UPD_MAXWG) == 256
    assert {w for _, w, _ in dc.CASES} == {1, 2, 3, 4, 5, 8} and max(w for _, w, _ in dc.CASES) == 8
    for nc, w, v in dc.CASES:
        assert v in ("64c", "64n", "32c", "32n") and dc.cf_variant(v) in cf.VARIANTS
        assert not v.startswith("32") or d_of(nc) > cf.FAST_MAX_D                           # fp32 only where the library stores fp32
        assert dc.WHY[nc]


def _check_partition(ncam, world):
    rows, chunk = dc.partition(ncam, world)
    assert len(rows) == world + 1 and rows[0] == 0 and rows[-1] == ncam
    assert all(a <= b for a, b in zip(rows, rows[1:]))
    shares = [sum(ncam - 1 - I for I in range(rows[k], rows[k + 1])) for k in range(world)]
    assert sum(shares) == ncam * (ncam - 1) // 2 and chunk == max(max(shares), 1)
    return shares


def test_partition_restated():
    for nc, w, _ in dc.CASES:
        _check_partition(nc, w)
    for world in range(1, dc.MAX_WORLD + 1):
        for ncam in range(1, 41):
            _check_partition(ncam, world)
    # balanced: no share exceeds the even share by more than one block row
    for ncam, world in ((1366, 8), (342, 5), (253, 8)):
        shares = _check_partition(ncam, world)
        assert max(shares) <= ncam * (ncam - 1) // 2 / world + ncam


def test_gpu_file_runs_every_table_row():
    import test_gpu_dist_cg_ranks as g
    marks = [m for m in g.test_ranks_match_the_reference_cg.pytestmark if m.name == "parametrize" and m.args[0] == "case"]
    assert len(marks) == 1 and list(marks[0].args[1]) == dc.CASES and marks[0].kwargs["ids"] is dc.case_id
    src = open(g.__file__.replace(".pyc", ".py")).read()
    assert "skip" not in src and "xfail" not in src
    assert all(m <= dc.MAX_ITERS <= 200 for m in dc.FORCED) and dc.SURPLUS == 6


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_the_emulation_passes_every_verdict(case):
    nc, w, v = case
    s, runs = dc.emulated_runs(nc, w, v)
    rep, failed = dc.verdicts(s, nc, v, runs)
    print(dc.report_line("dcgemu", case, dc.partition(nc, w)[0], rep), flush=True)
    assert not failed, failed
    # float64 and long double agree on the iterations (so rounding alone cannot reach the bar of 2)
    assert abs(rep["k_ref"] - rep["k_ld"]) <= 1


# (defect, the smallest row where it can act, why there)
DEFECTS = [
    ("identity", (1, 3, "64c"), "the first row with a rank other than 0"),
    ("focal", (1, 3, "64c"), "the first row with a rank other than 0"),
    ("transposed", (2, 8, "64c"), "the first row with a block: column 1 has one row above it"),
    ("stale", (2, 8, "64c"), "the first row of world 8"),
    ("mixed32", (214, 4, "64c"), "the first size that stores fp32; held as the fp64 case it was asked to be"),
]


@pytest.mark.parametrize("defect,case,why", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_the_verdicts_catch_a_planted_defect(defect, case, why):
    nc, w, v = case
    assert case in dc.CASES
    s, runs = dc.emulated_runs(nc, w, v, defect)
    rep, failed = dc.verdicts(s, nc, v, runs)
    print("dcgemu defect %-10s at %-12s (%s): %s" % (defect, dc.case_id(case), why, "; ".join(f.split(" [")[0] for f in failed)[:300]), flush=True)
    assert failed
    if defect == "stale":
        assert any(f.startswith("5 ") for f in failed)


def test_mixed_precision_pair_is_invisible_at_fp32_bars():
    """Written down, not hidden: fp32 blocks with an fp64 focal row differ from the all-fp32 matrix by one fp32 rounding of the focal row, which the
    bars of an fp32 case (unit roundoff 6e-8) allow by construction.  The pairing is held by the probe's interface instead (one flag sets both) and
    by the fp64 case above."""
    s, runs = dc.emulated_runs(214, 4, "32c", "mixed32")
    rep, failed = dc.verdicts(s, 214, "32c", runs)
    assert not failed
