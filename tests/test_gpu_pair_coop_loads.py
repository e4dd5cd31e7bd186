"""The fp32 wave-per-chunk pair pass fetches its point-table entries cooperatively: the four lanes of a quad fetch the four 16-byte pieces
of one 64-byte entry per load, and a private piece of LDS hands every lane its own entry (csrc/sfmba_device.h: ptrec_quad_fetch /
ptrec_quad_take).  That moves data only -- every lane ends up with exactly the bytes the per-lane loads (SFMBA_PAIR_LOADS=lane, read when a
problem is built) give it, and the pass has no atomics -- so, on handles whose other passes are bitwise repeatable too (CREATE_DETERMINISTIC:
a plain handle sums the Jacobi column scales with atomics, and two builds of ONE variant already differ in the last bit of ~20 scales),
  (1) the reduced system (k_schur_pairs<float, 0>) is BITWISE the per-lane one at ~7, ~110 and ~3000 pairs per block and on `small`
      (partly filled rounds, empty blocks, blocks of several chunks through k_schur_combine),
  (2) a whole solve on a deterministic handle (k_schur_pairs<float, 1>, the benchmark's instantiation; such handles are bitwise repeatable)
      has the same summary, trace and parameters in every bit, and
  (3) the default path gives the oracle's reduced system on the mixed first-order-camera problem of test_gpu_pair_packed.py at that file's bar
      (2e-5 of the entry scale), so that a slip common to both variants cannot hide behind (1)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


def _cases():
    spec = importlib.util.spec_from_file_location("pair_forms_cases", os.path.join(ROOT, "tests", "test_gpu_pair_forms.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.CASES


def _summary_fields():
    spec = importlib.util.spec_from_file_location("bench_mod_fields", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.SUMMARY_FIELDS


def _set_loads(monkeypatch, loads):
    if loads is None:
        monkeypatch.delenv("SFMBA_PAIR_LOADS", raising=False)
    else:
        monkeypatch.setenv("SFMBA_PAIR_LOADS", loads)


@pytest.mark.parametrize("name,kw", _cases())
def test_reduced_system_is_bitwise_that_of_the_per_lane_loads(capi, sfm, monkeypatch, name, kw):
    prob = sfm.make_problem(name, **kw)
    monkeypatch.setenv("SFMBA_PAIR_LPB", "64")
    got = {}
    for loads in ("lane", None):
        _set_loads(monkeypatch, loads)
        with capi.Problem(prob, precision=1, flags=sfm.CREATE_DETERMINISTIC) as P:
            got[loads] = P.build_reduced(1e4)
    (S_l, rhs_l, scale_l), (S_q, rhs_q, scale_q) = got["lane"], got[None]
    assert np.abs(S_l).max() > 0 and np.isfinite(S_q).all()
    off = S_l.copy()
    for j in range(prob.n_cam):
        off[6 * j:6 * j + 6, 6 * j:6 * j + 6] = 0
    assert np.abs(off[:6 * prob.n_cam, :6 * prob.n_cam]).max() > 0          # the pair pass wrote something
    print("%s %s: %d differing entries of S" % (name, kw, int((S_l != S_q).sum())))
    assert np.array_equal(S_q, S_l)
    assert np.array_equal(rhs_q, rhs_l)
    assert np.array_equal(scale_q, scale_l)


def test_whole_solve_on_a_deterministic_handle_is_bitwise_that_of_the_per_lane_loads(capi, sfm, monkeypatch):
    monkeypatch.setenv("SFMBA_PAIR_LPB", "64")          # (~1700 pairs per block: the wave-per-chunk pass is the default here anyway)
    prob = sfm.make_problem("cfg3", n_cam=40, n_pt=30000, seed=13)
    opt = capi.default_options(max_seconds=0.0, precision=1, linear_solver=1)
    fields = _summary_fields()
    runs = {}
    for loads in ("lane", None):
        _set_loads(monkeypatch, loads)
        with capi.Problem(prob, precision=1, flags=sfm.CREATE_DETERMINISTIC) as P:
            s, tr = P.solve(opt)
            runs[loads] = (P.get_params(), s, tr)
    (cam_l, pt_l, f_l), s_l, tr_l = runs["lane"]
    (cam_q, pt_q, f_q), s_q, tr_q = runs[None]
    assert s_l["termination_name"] == "CONVERGENCE" and s_l["iterations"] > 1
    for k in fields:
        assert k in s_l and s_q[k] == s_l[k], (k, s_q[k], s_l[k])
    assert len(tr_q) == len(tr_l) and len(tr_l) > 1
    for a, b in zip(tr_q, tr_l):
        assert a == b, (a, b)
    assert np.array_equal(cam_q, cam_l) and np.array_equal(pt_q, pt_l) and f_q == f_l


def test_default_loads_give_the_oracles_reduced_system_with_mixed_first_order_cameras(capi, sfm, oracle, monkeypatch):
    monkeypatch.delenv("SFMBA_PAIR_LOADS", raising=False)
    monkeypatch.setenv("SFMBA_PAIR_LPB", "64")
    prob = sfm.make_problem("cfg3", n_cam=60, n_pt=20000, seed=21)
    prob.cam6[::3, :3] = 0.0            # zero angle-axis: every third camera is on the first-order branch
    S_o, rhs_o, scale_o, _ = oracle.build_reduced(prob, 1e4)
    ent = np.sqrt(np.outer(np.abs(np.diag(S_o)), np.abs(np.diag(S_o))))
    with capi.Problem(prob, precision=1) as P:
        S, rhs, scale = P.build_reduced(1e4)
    err = (np.abs(S - S_o) / ent).max()
    print("default (quad) loads, F32J: max |dS| / entry scale = %.3e (bar 2e-5)" % err)
    assert np.allclose(scale, scale_o, rtol=1e-6)
    assert (np.abs(S - S_o) <= 2e-5 * ent).all(), err
    assert np.abs(rhs - rhs_o).max() <= 2e-5 * np.abs(rhs_o).max()
