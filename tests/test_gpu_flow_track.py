"""The pyramidal Lucas-Kanade tracker and the snap to key points on the MI355X (-m gpu) against the CPU restatement of their contract
(tests/flow_oracle.py; include/sfmba.h, sfmba_flow_track / sfmba_flow_match).  Every comparison is EXACT: the bit patterns of next
and err, status, the per-level sums, flags, iteration counts and displacements, the pyramid levels, and the matches with their
distances and pair_ptr.  The shapes are those of tests/flow_cases.py -- the smallest at which the kernels can still go wrong -- and the
restatement's answer for each is computed once and shared."""
import numpy as np
import pytest

import flow_cases as fc
import flow_oracle as fo

pytestmark = pytest.mark.gpu
SFMBA_ERR_CAPACITY = 5
FIELDS = ("next", "status", "err", "G", "state")


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_pair(got, want, what=""):
    for f, (a, b) in enumerate(zip(got, want)):
        if not same_bits(a, b):
            rows = np.nonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1))[0] if a.shape == b.shape else []
            raise AssertionError((what, FIELDS[f], a.shape, b.shape, "first differing points", [int(r) for r in rows[:5]]))


def assert_levels(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if w is None:                                                    # an image that no pair names is not written
            assert not any(a.any() for a in g), (what, i)
            continue
        assert len(g) == len(w)
        for l, (a, b) in enumerate(zip(g, w)):
            assert same_bits(a, b), (what, "image", i, "level", l)


@pytest.mark.parametrize("name", list(fc.TRACK_CASES))
def test_track_cases_exact(capi, name):
    c, (want, levels) = fc.case(name), fc.oracle(name)
    got, got_levels = capi.flow_track(c["images"], c["pairs"], c["points"], debug=True, **c["params"])
    assert len(got) == len(want)
    for p in range(len(want)):
        assert_pair(got[p], want[p], "%s pair %d" % (name, p))
    assert_levels(got_levels, levels, name)
    plain = capi.flow_track(c["images"], c["pairs"], c["points"], **c["params"])          # the debug pointers may be NULL
    for p in range(len(want)):
        assert_pair(plain[p], want[p][:3], "%s pair %d without debug arrays" % (name, p))


def test_bgr_equals_its_gray_reduction(capi):
    c = fc.case("bgr")
    grays = [fo.gray(im).astype(np.uint8) for im in c["images"]]
    a, la = capi.flow_track(c["images"], c["pairs"], c["points"], debug=True, **c["params"])
    b, lb = capi.flow_track(grays, c["pairs"], c["points"], debug=True, **c["params"])
    assert_pair(a[0], b[0], "bgr against gray")
    assert_levels(la, lb, "bgr against gray")
    assert same_bits(la[0][0], grays[0])


def test_batch_equals_single_calls(capi):
    c, (want, levels) = fc.case("counts"), fc.oracle("counts")
    got, got_levels = capi.flow_track(c["images"], c["pairs"], c["points"], debug=True, **c["params"])
    assert len(got) == 5
    for p, (pair, pts) in enumerate(zip(c["pairs"], c["points"])):
        (single,), single_levels = capi.flow_track(c["images"], [pair], [pts], debug=True, **c["params"])
        assert_pair(single, got[p], "single pair %d" % p)
        for i in set(pair):
            for a, b in zip(single_levels[i], got_levels[i]):
                assert same_bits(a, b), (p, i)
    assert sum(int(g[1].sum()) for g in got) > 50                      # one image (0) is named by four of the pairs


def test_no_pairs_and_no_points(capi):
    img = fc.texture(12, 9, seed=1)
    assert capi.flow_track([img], [], []) == []
    (nxt, status, err), = capi.flow_track([img], [(0, 0)], [np.zeros((0, 2), np.float32)])
    assert nxt.shape == (0, 2) and status.shape == (0,) and err.shape == (0,)


# ---- matcher -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.MATCH_CASES))
def test_match_cases_exact(capi, name):
    c, want = fc.match_case(name), fc.match_oracle(name)
    got = capi.flow_match(c["keypoints"], c["pairs"], c["tracked"], **c["params"])
    for f, (a, b) in enumerate(zip(got, want)):
        assert same_bits(a, b), (name, ("pair_ptr", "query_idx", "train_idx", "distance")[f], a[:8], b[:8])


def test_match_capacity_protocol(capi):
    c, want = fc.match_case("several_pairs"), fc.match_oracle("several_pairs")
    n = int(want[0][-1])
    assert n >= 4
    kp_ptr = np.concatenate([[0], np.cumsum([len(k) for k in c["keypoints"]])])
    pt_ptr = np.concatenate([[0], np.cumsum([len(t[0]) for t in c["tracked"]])])
    args = dict(kp_ptr=kp_ptr, kp=np.concatenate(c["keypoints"]), pair_dst=[d for _, d in c["pairs"]], pt_ptr=pt_ptr,
                nxt=np.concatenate([t[0] for t in c["tracked"]]), status=np.concatenate([t[1] for t in c["tracked"]]),
                err=np.concatenate([t[2] for t in c["tracked"]]), **c["params"])
    for cap in (0, n - 1):
        rc, ptr, q, t, d, total = fc.raw_match(capi, cap=cap, **args)
        assert rc == SFMBA_ERR_CAPACITY and total == n and same_bits(ptr, want[0])
        assert (q == -7).all() and (t == -7).all() and (d == -7.0).all()                  # nothing else written
    rc, ptr, q, t, d, total = fc.raw_match(capi, cap=n, **args)
    assert rc == 0 and total == n and same_bits(ptr, want[0])
    assert same_bits(q[:n], want[1]) and same_bits(t[:n], want[2]) and same_bits(d[:n], want[3])
    got = capi.flow_match(c["keypoints"], c["pairs"], c["tracked"], cap=1, **c["params"])          # the binding retries once
    assert all(same_bits(a, b) for a, b in zip(got, want))


def test_track_then_match_finds_the_planted_key_points(capi):
    """The two calls end to end at the defaults: the key points of the second view are those of the first moved by the shift."""
    shift = (3.3, -2.6)
    a, b = fc.texture_pair(96, 72, shift, seed=6)
    pts = fc.inner_points(96, 72, 40, 14, seed=9)
    kps = [pts, (pts.astype(np.float64) + np.asarray(shift)).astype(np.float32)]
    tracked = capi.flow_track([a, b], [(0, 1)], [pts], **fo.DEFAULTS)
    want_t = fo.track_vec([a, b], [(0, 1)], [pts], **fo.DEFAULTS)[0]
    assert_pair(tracked[0], want_t[0][:3], "defaults")
    got = capi.flow_match(kps, [(0, 1)], tracked, **fo.MATCH_DEFAULTS)
    want = fo.match_vec(kps, [(0, 1)], tracked, **fo.MATCH_DEFAULTS)
    assert all(same_bits(x, y) for x, y in zip(got, want))
    print("planted 40 key points: %d matched, %d to their own index" % (len(got[1]), int((got[1] == got[2]).sum())))
    assert (got[1] == got[2]).all() and len(got[1]) >= 20            # the ratio test may drop points with a close neighbour
