"""The wave-per-chunk pair pass in fp32-Jacobian mode evaluates both observations of a pair as the halves of packed fp32 values
(csrc/sfmba_device.h: obs_factored_ab, pair_product_ab; projection in fp32, the 6x6 update in its rank-2 form).  test_gpu_pair_forms.py
holds both pair geometries to the oracle's reduced system at ~7, ~110 and ~3000 pairs per block; here
  (a) the real headline problem (BASELINE config 3: 200 cameras, ~226 pairs per block -- the density bench.py runs at, which no other
      reduced-system test covers): the fp32-Jacobian reduced system against the fp64 one of the same handle type, and
  (b) a problem in which every third camera has zero rotation (the first-order branch, G = -[X]x exactly), so that blocks whose two cameras
      are both, neither, only the row camera's and only the column camera's on that branch all occur: both geometries against the oracle's
      reduced system in both precisions.
Bars: those of test_gpu_pair_forms.py -- 1e-11 (fp64) and 2e-5 (fp32 Jacobian blocks) of the entry scale sqrt(S_ii S_jj)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


def test_headline_density_f32j_reduced_system_against_fp64(capi, sfm, monkeypatch):
    monkeypatch.delenv("SFMBA_PAIR_LPB", raising=False)
    prob = sfm.make_problem("cfg3")
    with capi.Problem(prob, precision=0) as P:
        S64, rhs64, scale64 = P.build_reduced(1e4)
    with capi.Problem(prob, precision=1) as P:
        S32, rhs32, scale32 = P.build_reduced(1e4)
    ent = np.sqrt(np.outer(np.abs(np.diag(S64)), np.abs(np.diag(S64))))
    err = np.abs(S32 - S64) / ent
    print("cfg3 F32J vs fp64 reduced system: max |dS| / entry scale = %.3e (bar 2e-5), max |d rhs| / max |rhs| = %.3e"
          % (err.max(), np.abs(rhs32 - rhs64).max() / np.abs(rhs64).max()))
    assert np.allclose(scale32, scale64, rtol=1e-6)
    assert (err <= 2e-5).all(), err.max()
    assert np.abs(rhs32 - rhs64).max() <= 2e-5 * np.abs(rhs64).max()


@pytest.mark.parametrize("precision,tol", [(0, 1e-11), (1, 2e-5)])
def test_mixed_first_order_cameras_give_the_oracles_reduced_system(capi, sfm, oracle, monkeypatch, precision, tol):
    prob = sfm.make_problem("cfg3", n_cam=60, n_pt=20000, seed=21)
    prob.cam6[::3, :3] = 0.0            # zero angle-axis: these cameras are on the first-order branch, the others are not
    S_o, rhs_o, scale_o, _ = oracle.build_reduced(prob, 1e4)
    ent = np.sqrt(np.outer(np.abs(np.diag(S_o)), np.abs(np.diag(S_o))))
    got = {}
    for lpb in ("64", "16"):
        monkeypatch.setenv("SFMBA_PAIR_LPB", lpb)
        with capi.Problem(prob, precision=precision) as P:
            got[lpb] = P.build_reduced(1e4)
    monkeypatch.delenv("SFMBA_PAIR_LPB")
    # all four kinds of off-diagonal block are present and non-empty
    fo = np.zeros(prob.n_cam, bool)
    fo[::3] = True
    for want_a, want_b in ((True, True), (True, False), (False, True), (False, False)):
        ja, jb = [(a, b) for a in range(prob.n_cam) for b in range(a + 1, prob.n_cam) if fo[a] == want_a and fo[b] == want_b][0]
        assert max(np.abs(S_o[6 * ja:6 * ja + 6, 6 * jb:6 * jb + 6]).max(), np.abs(S_o[6 * jb:6 * jb + 6, 6 * ja:6 * ja + 6]).max()) > 0
    for lpb, (S, rhs, scale) in got.items():
        print("precision %d, %s lanes per block: max |dS| / entry scale = %.3e (bar %g)" % (precision, lpb, (np.abs(S - S_o) / ent).max(), tol))
        assert np.allclose(scale, scale_o, rtol=1e-6 if precision else 1e-12), lpb
        assert (np.abs(S - S_o) <= tol * ent).all(), (lpb, (np.abs(S - S_o) / ent).max())
        assert np.abs(rhs - rhs_o).max() <= tol * np.abs(rhs_o).max(), lpb
    assert (np.abs(got["64"][0] - got["16"][0]) <= tol * ent).all()
