"""Semi-global matching over the sweep's cost volume on the MI355X (-m gpu) against the CPU restatement of its contract
(tests/sgm_oracle.py; include/sfmba.h, sfmba_depth_cost_volume / sfmba_sgm_aggregate / sfmba_depth_sweep_sgm).  Every comparison is
EXACT: the volume, the sums, plane, best, second, and the bit patterns of depth and score.  The shapes are those of tests/sgm_cases.py
and tests/depth_cases.py -- the smallest at which the kernels can still go wrong -- and the restatement's answer for each is computed
once and shared."""
import ctypes as C

import numpy as np
import pytest

import depth_cases as dc
import depth_oracle as do
import sgm_cases as sc
import sgm_oracle as so
import sgm_refusals as sr

pytestmark = pytest.mark.gpu
SFMBA_ERR_INVALID_ARG = 1


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_agg(got, want, what, sums=True):
    for f in ("plane", "best", "second") + (("sums",) if sums else ()):
        bad = np.argwhere(got[f] != want[f])
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape and len(bad) == 0, (what, f, len(bad), bad[:5].tolist())


def assert_maps(got, want, what=""):
    for i, f in enumerate(("depth", "score", "plane")):
        assert same_bits(got[i], want[i]), (what, f, np.argwhere(got[i] != want[i])[:5].tolist())


# ---- sfmba_sgm_aggregate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_aggregate_cases_exact(capi, name):
    c, want = sc.case(name), sc.oracle(name)
    prm = {k: c[k] for k in ("p1", "p2", "n_paths", "invalid_cost")}
    got = capi.sgm_aggregate([c["vol"]], **prm)
    assert len(got) == 1
    assert_agg(got[0], want, name)
    if name in sc.NO_SUMS:                                       # sums = NULL: the three maps are the same
        bare = capi.sgm_aggregate([c["vol"]], want_sums=False, **prm)[0]
        assert bare["sums"] is None
        assert_agg(bare, want, name + " without sums", sums=False)


def test_aggregate_several_volumes_in_one_call(capi):
    names = ["17x33_d65_p8", "2x2_d63_p8", "70x45_d64_p4"]       # one D per call: three volumes cut to 63 planes
    vols = [np.ascontiguousarray(sc.case(n)["vol"][:, :, :63]) for n in names]
    got = capi.sgm_aggregate(vols, p1=3, p2=40, n_paths=8, invalid_cost=9)
    for v, g, n in zip(vols, got, names):
        assert_agg(g, so.sgm_aggregate(v, 3, 40, 8, 9), n)
    some = capi.sgm_aggregate(vols, p1=3, p2=40, n_paths=8, invalid_cost=9, want_sums=[True, False, True])     # sums[1] = NULL
    assert some[1]["sums"] is None
    for j, (g, s) in enumerate(zip(got, some)):
        assert_agg(s, g, "entry %d of sums NULL" % j, sums=j != 1)


# ---- sfmba_depth_cost_volume ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.VOLUME_SCENES)
def test_cost_volume_exact(capi, name):
    c = dc.case(name)
    want, _, _ = sc.volume_oracle(name)
    p = sc.sweep_params(c)
    got = capi.depth_cost_volume(c["images"], c["K"], c["P"], c["jobs"], **p)
    assert len(got) == 1 and same_bits(got[0], want), (name, np.argwhere(got[0] != want)[:5].tolist())
    part = dc.oracle(name)["part"]
    assert (got[0][~part] == so.SENTINEL).all()                  # a pixel that does not take part has no cost at all
    if name in ("blind", "const_ref"):
        assert (got[0] == so.SENTINEL).all()
    else:
        assert (got[0][part] != so.SENTINEL).any()


# ---- sfmba_depth_sweep_sgm --------------------------------------------------------------------------------------------------------
SGM_SETS = [dict(so.DEFAULTS), dict(p1=0, p2=1023, n_paths=4, invalid_cost=0, uniqueness=0), dict(p1=30, p2=30, n_paths=8, invalid_cost=254, uniqueness=100)]


@pytest.mark.parametrize("name", sc.VOLUME_SCENES)
def test_sweep_sgm_equals_the_three_steps_and_the_restatement(capi, name):
    c = dc.case(name)
    p = sc.sweep_params(c)
    vol_o, wf, step = sc.volume_oracle(name)
    vol = capi.depth_cost_volume(c["images"], c["K"], c["P"], c["jobs"], **p)[0]
    for sgm in SGM_SETS:
        agg_prm = {k: v for k, v in sgm.items() if k != "uniqueness"}
        got = capi.depth_sweep_sgm(c["images"], c["K"], c["P"], c["jobs"], **dict(p, **sgm))[0]
        agg = capi.sgm_aggregate([vol], **agg_prm)[0]
        assert_maps(got, so.maps_of(vol, agg, wf, step, sgm["uniqueness"]), (name, "three steps", sgm))
        assert_maps(got, so.maps_of(vol_o, so.sgm_aggregate(vol_o, **agg_prm), wf, step, sgm["uniqueness"]), (name, "restatement", sgm))
        assert (got[2] >= 0).all()                               # a plane for EVERY pixel
    if name in ("blind", "const_ref"):                           # nothing but sentinels: k* = 0, second == best, the score says so
        assert (got[2] == 0).all() and not got[1].any() and not got[0].any()


def test_sweep_sgm_plane_pointer_may_be_null(capi):
    c = dc.case("size_17x33_r2_d3")
    p = sc.sweep_params(c, **so.DEFAULTS)
    a = capi.depth_sweep_sgm(c["images"], c["K"], c["P"], c["jobs"], **p)[0]
    b = capi.depth_sweep_sgm(c["images"], c["K"], c["P"], c["jobs"], want_plane=False, **p)[0]
    assert b[2] is None and same_bits(a[0], b[0]) and same_bits(a[1], b[1])


def test_uniqueness_exactly_on_the_ratio(capi):
    c, sgm, u, agg = sc.uniqueness_case()
    vol, wf, step = sc.volume_oracle("size_48x31_r3_d64")
    b, s = agg["best"].astype(np.int64), agg["second"].astype(np.int64)
    slack = 100 * (s - b) - u * s
    on, above, below = slack == 0, (slack >= -100) & (slack < 0), (slack > 0) & (slack <= 100)
    assert on.any() and above.any() and below.any()
    for uu in (u - 1, u, u + 1):
        got = capi.depth_sweep_sgm(c["images"], c["K"], c["P"], c["jobs"], **sc.sweep_params(c, uniqueness=uu, **sgm))[0]
        assert_maps(got, so.maps_of(vol, agg, wf, step, uu), uu)
        if uu == u:                                              # on the ratio: accepted; one unit of `best` more: not
            assert (got[0][on] > 0).all() and (got[0][below] > 0).all() and not got[0][above].any()


def test_sweep_sgm_batch_equals_single_calls(capi):
    b = dc.batch()
    p = sc.sweep_params(b, **so.DEFAULTS)
    want = so.sweep_sgm(b["images"], b["K"], b["P"], b["jobs"], **p)
    got = capi.depth_sweep_sgm(b["images"], b["K"], b["P"], b["jobs"], **p)
    assert len(got) == 5
    for j, job in enumerate(b["jobs"]):
        assert_maps(got[j], want[j], "batch job %d" % j)
        assert_maps(capi.depth_sweep_sgm(b["images"], b["K"], b["P"], [job], **p)[0], got[j], "single job %d" % j)
    vols = capi.depth_cost_volume(b["images"], b["K"], b["P"], b["jobs"], **sc.sweep_params(b))
    for j, job in enumerate(b["jobs"]):
        assert same_bits(vols[j], capi.depth_cost_volume(b["images"], b["K"], b["P"], [job], **sc.sweep_params(b))[0]), j
    assert sum((g[0] > 0).sum() for g in got) > 500


def test_sweep_sgm_bgr_equals_its_gray_reduction(capi):
    b = dc.batch()
    bgr = dc.bgr_of(b["images"])
    gray = [do.gray(im).astype(np.uint8) for im in bgr]
    p = sc.sweep_params(b, **so.DEFAULTS)
    got = capi.depth_sweep_sgm(bgr, b["K"], b["P"], b["jobs"][:3], **p)
    want = so.sweep_sgm(gray, b["K"], b["P"], b["jobs"][:3], **p)
    for j in range(3):
        assert_maps(got[j], want[j], "bgr job %d" % j)
    vols = capi.depth_cost_volume(bgr, b["K"], b["P"], b["jobs"][:3], **sc.sweep_params(b))
    for j in range(3):
        assert same_bits(vols[j], so.cost_volume(gray, b["K"], b["P"], b["jobs"][j], **sc.sweep_params(b))[0]), j


# ---- argument checks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.REFUSALS))
def test_refusals_write_nothing(capi, name):
    rc, outputs = sr.REFUSALS[name](capi)
    assert rc == SFMBA_ERR_INVALID_ARG, (name, rc)
    for what, arr in outputs.items():
        assert (arr.view(np.uint8) == sr.FILL).all(), (name, what)


def test_the_refusal_harness_accepts_a_good_call(capi):
    for call in (sr.aggregate, sr.cost_volume, sr.sweep_sgm):
        rc, outputs = call(capi)
        assert rc == 0, call.__name__
        assert any((arr.view(np.uint8) != sr.FILL).any() for arr in outputs.values()), call.__name__
