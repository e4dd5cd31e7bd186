"""The distributed CG at every rank count from 1 to 8 against the numpy restatement of the method (-m gpu): tests/dist_cg_cases.py holds the table,
the restated partition, the emulation and the verdicts (systems, long-double reference and bars are tests/cg_family_cases.py's, unchanged);
tests/test_dist_cg_cases_cpu.py proves on the CPU that the bars are attainable and that they catch a planted defect.  The device side is
sfmba_dist_cg_probe: every rank of the world simulated in this one process -- the library's own transform, partition, dcg_begin / dcg_iterate per rank
on that rank's chunk of the reduce-scatter layout, the all-reduce a sum over the ranks' buffers.  No communicator, no second process.

Per case, three probe calls and the second one again without its surplus launches:
    reuse    b, the zero vector, b2                               (max_iters 200 each)
    forced   b2 -- that system solved alone --, then b stopped after 1, 2, 3 iterations, six surplus launches behind every solve
    poison   the forced call with NaN in everything the kernels promise not to read
and eight verdicts: (1) partition, (2) true residual, (3) iterations, (4) forced iterates, (5) surplus launches are inert, (6) replicas identical,
(7) reuse, (8) poison.  One `dcgfam` line per case goes to stdout before anything is asserted (profiles/dist_cg_ranks.txt holds those lines)."""
import numpy as np
import pytest

import dist_cg_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_ranks_match_the_reference_cg(capi, case):
    nc, world, v = case
    s = dc.system(nc)
    Wt, _ = dc.coarse(s, v)
    flags = capi.DCG_PROBE_F32 if v.startswith("32") else 0
    full, forced = dc.MAX_ITERS, list(dc.FORCED)
    zero = np.zeros(s.d)

    reuse = capi.dist_cg_probe(s.S, world, [s.rhs, zero, s.rhs2], Wt, flags, dc.TOL, [full] * 3, 0)
    forc = capi.dist_cg_probe(s.S, world, [s.rhs2, s.rhs, s.rhs, s.rhs], Wt, flags, dc.TOL, [full] + forced, dc.SURPLUS)
    forc0 = capi.dist_cg_probe(s.S, world, [s.rhs2, s.rhs, s.rhs, s.rhs], Wt, flags, dc.TOL, [full] + forced, 0)
    pois = capi.dist_cg_probe(s.S, world, [s.rhs2, s.rhs, s.rhs, s.rhs], Wt, flags | capi.DCG_PROBE_POISON, dc.TOL, [full] + forced, dc.SURPLUS)
    calls = (reuse, forc, forc0, pois)

    rep, failed = dc.verdicts(s, nc, v, {k: (c["Xt"], c["iters"]) for k, c in zip(("reuse", "forced", "forced0", "poison"), calls)})
    print(dc.report_line("dcgfam", case, reuse["rows"], rep, "  poison iters %s  differ %s info %s" % (
        [int(k) for k in pois["iters"]], [c["replicas_differ"] for c in calls], [c["info"] for c in calls])), flush=True)

    # (1) the partition the library chose is the restated one, on every call
    rows, chunk = dc.partition(nc, world)
    assert all(c["rows"] == rows and c["chunk_blocks"] == chunk for c in calls), (reuse["rows"], reuse["chunk_blocks"], rows, chunk)
    assert all(c["info"] == 0 for c in calls)
    # (6) every rank's replicated state equal to rank 0's, bit for bit, at every check of every call
    assert [c["replicas_differ"] for c in calls] == [0] * 4
    # (2) true residual, (3) iterations, (4) forced iterates, (5) surplus launches inert, (7) reuse, (8) poison: dist_cg_cases.verdicts
    assert not failed, failed
