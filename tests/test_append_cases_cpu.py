"""The growth sequences of tests/append_cases.py on the CPU alone (no GPU): every case really has the property it is there for, the
steps only ever add observations, and the oracle can linearise every step (tests/test_gpu_append_linearisation.py compares the
appended handle with it)."""
import numpy as np
import pytest

import append_cases as ac


@pytest.fixture(scope="module")
def cases():
    return {name: ac.make_case(name) for name in ac.CASES}


def _active(case, k):
    o = ac.step_order(case, k)
    return np.unique(case.prob.obs_cam[o]), np.unique(case.prob.obs_pt[o])


def _keys(case, idx):
    return case.prob.obs_pt[idx].astype(np.int64) * case.prob.n_cam + case.prob.obs_cam[idx]


def test_steps_only_add_observations(cases):
    for name, case in cases.items():
        allidx = np.concatenate(case.steps)
        assert len(np.unique(allidx)) == len(allidx), name                # no observation is handed over twice ...
        assert allidx.min(initial=0) >= 0 and allidx.max(initial=0) < case.prob.n_obs
        assert case.n_steps >= 2 and len(case.params) == case.n_steps
        for k in range(1, case.n_steps):                                   # ... so every step's list is the previous one plus new entries
            a, b = ac.step_order(case, k - 1), ac.step_order(case, k)
            assert np.array_equal(b[:len(a)], a) and ac.step_problem(case, k).n_obs == len(b)
            assert case.params[k][0].shape[0] >= case.params[k - 1][0].shape[0] and case.params[k][1].shape[0] >= case.params[k - 1][1].shape[0]
        if name != "no_new_obs":
            assert all(len(s) > 0 for s in case.steps), name
        assert ac.checked_steps(name) == ([case.n_steps - 1] if name in ac.LAST_STEP_ONLY else list(range(case.n_steps)))


def test_view_order_registers_cameras_and_points_out_of_order(cases):
    case = cases["view_order"]
    p = case.prob
    assert p.n_cam == 10 and p.n_pt == 300 and case.n_steps == len(ac.VIEW_ORDER) - 2 == 7
    for k in range(case.n_steps):
        reg = ac.VIEW_ORDER[:3 + k]
        cams, pts = _active(case, k)
        assert sorted(reg) == cams.tolist()                               # three cameras at create, one more per append
        o = ac.step_order(case, k)
        # a point is in exactly when two registered cameras see it, with all its registered views
        vis = np.isin(p.obs_cam, reg) & ~np.isin(p.obs_pt, (17, p.n_pt - 1))
        cnt = np.bincount(p.obs_pt[vis], minlength=p.n_pt)
        assert np.array_equal(np.sort(o), np.flatnonzero(vis & (cnt[p.obs_pt] >= 2)))
        acam, apt = ac.slot_order(case, k)
        assert sorted(acam.tolist()) == cams.tolist() and sorted(apt.tolist()) == pts.tolist()
        if k == 0:
            assert np.all(np.diff(acam) > 0) and np.all(np.diff(apt) > 0)           # create: slots ascend
        else:
            assert np.any(np.diff(apt) < 0)                                         # after every append the point slots do not ascend,
            assert np.any(np.diff(acam) < 0) == (k >= 2)                            # the camera slots from camera 0's on (1 4 7 8 | 0 ...)
    acam, apt = ac.slot_order(case, case.n_steps - 1)
    assert acam.tolist()[:3] == [1, 4, 7] and acam.tolist()[3:] == list(ac.VIEW_ORDER[3:])
    cams, pts = _active(case, case.n_steps - 1)
    assert 9 not in cams and len(cams) == 9                                # inactive camera at the end of the caller's array
    missing = np.setdiff1d(np.arange(p.n_pt), pts)
    assert 17 in missing and p.n_pt - 1 in missing and len(missing) >= 3  # inactive points inside and at the end
    assert np.any(np.bincount(p.obs_pt, minlength=p.n_pt)[missing] > 0)     # (some of them only because camera 9 never registers)


def test_grow_from_one_hits_every_boundary(cases):
    case = cases["grow_from_one"]
    assert case.n_steps == len(ac.GROW_CAMS) == len(ac.GROW_PTS) == 9
    assert len(case.steps[0]) == 1
    single = []
    for k in range(case.n_steps):
        cams, pts = _active(case, k)
        assert (len(cams), len(pts)) == (ac.GROW_CAMS[k], ac.GROW_PTS[k])
        assert np.array_equal(cams, np.arange(len(cams))) and np.array_equal(pts, np.arange(len(pts)))
        o = ac.step_order(case, k)
        if np.bincount(case.prob.obs_pt[o]).min() == 1:
            single.append(k)
    assert single == sorted(ac.SINGLE_VIEW_INFO)
    # the boundaries: 2^b cameras -> 2^b + 1 (cshift of the sort key), 256 -> 257 points (end_bit; the pointer grid of npt + 1 = 257 -> 258 entries)
    steps = list(zip(ac.GROW_CAMS, ac.GROW_CAMS[1:]))
    assert all(t in steps for t in ((1, 2), (2, 3), (4, 5), (8, 9), (16, 17)))
    psteps = list(zip(ac.GROW_PTS, ac.GROW_PTS[1:]))
    assert all(t in psteps for t in ((1, 2), (255, 256), (256, 257)))


def test_duplicates_repeat_resident_pairs(cases):
    case = cases["duplicates"]
    p = case.prob
    assert p.n_cam == 6 and p.n_pt == 200 and case.n_steps == 3
    k0, k1, k2 = (_keys(case, s) for s in case.steps)
    assert len(np.unique(k0)) == len(k0)                                   # create: every pair once
    assert np.all(np.isin(k1, k0))                                         # first append: resident pairs only ...
    u, c = np.unique(k1, return_counts=True)
    assert c.max() == 2 and np.sum(c == 2) == 1 and np.sum(c == 1) == len(u) - 1          # ... one of them twice in the same append
    assert np.all(np.isin(k2, k0)) and np.any(np.isin(k2, k1)) and np.any(~np.isin(k2, k1))
    # the copies differ in their pixels (+ 0.25, + 0.5, - 0.125): an order mix-up of equal keys shows in the residuals
    first = case.steps[1][0]
    same = np.flatnonzero(_keys(case, np.arange(p.n_obs)) == k1[0])
    assert len(same) >= 4 and len(np.unique(p.obs_xy[same], axis=0)) == len(same)
    assert np.allclose(p.obs_xy[first] - p.obs_xy[same[0]], 0.25)


def test_chunk_edges_cross_the_chunk_lengths(cases):
    case = cases["chunk_edges"]
    p = case.prob
    assert p.n_cam == 3 and case.n_steps == 2
    sizes = []
    for k in range(2):
        o = ac.step_order(case, k)
        seen = np.zeros((3, p.n_pt), int)
        np.add.at(seen, (p.obs_cam[o], p.obs_pt[o]), 1)
        assert seen.max() == 1
        sizes.append((int((seen[0] * seen[1]).sum()), int(seen[2].sum()), int(seen[0].sum())))
        pairs = sum(int((seen[a] * seen[b]).sum()) for a, b in ((0, 1), (0, 2), (1, 2)))
        assert pairs / 3.0 >= 128.0                                        # (mean pairs per block: the wave-per-chunk pair pass, the one with chunk descriptors)
    assert sizes[0][:2] == (ac.PAIR_CHUNK - 1, ac.CAM_CHUNK - 1) == (511, 255)
    assert sizes[1][:2] == (ac.PAIR_CHUNK + 1, ac.CAM_CHUNK + 1) == (513, 257)
    assert sizes[0][2] == 511 and sizes[1][2] == 513                      # camera 0's list: two chunks of 256 -> three

    case = cases["chunk_edges_track"]
    p = case.prob
    assert p.n_cam == 40 and case.n_steps == len(ac.TRACK_LENGTHS)
    for k, m in enumerate(ac.TRACK_LENGTHS):
        o = ac.step_order(case, k)
        cams, _ = _active(case, k)
        assert len(cams) == 40                                             # every camera is resident from create on
        track = p.obs_cam[o][p.obs_pt[o] == 0]
        assert len(track) == len(np.unique(track)) == m
    assert ac.TRACK_LENGTHS[0] == 2 and ac.TRACK_LENGTHS[-1] == p.n_cam
    others = np.bincount(p.obs_pt[p.obs_pt > 0])[1:]
    assert others.min() >= 2 and others.max() <= 6


def test_sizes_straddle_the_sort_switch_and_the_thread_threshold(cases):
    case = cases["sort_switch"]
    assert case.prob.n_cam == 12 and case.prob.n_pt == 8200 and case.n_steps == 2
    assert len(case.steps[0]) == 32700 < ac.SORT_SWITCH < len(case.steps[0]) + len(case.steps[1]) == 32800
    case = cases["host_threads"]
    assert case.prob.n_cam == 6 and case.n_steps == 2
    assert len(case.steps[0]) == 2000 and len(case.steps[1]) == 208000 > ac.PARALLEL_FOR_MIN
    new_pts = np.unique(case.prob.obs_pt[case.steps[1]])
    assert len(new_pts) == 52000 and not np.any(np.isin(new_pts, case.prob.obs_pt[case.steps[0]]))
    # a point's four views are spread over the append: with 8 host threads nearly every point is counted by several of them
    pos = np.argsort(case.prob.obs_pt[case.steps[1]], kind="stable").reshape(-1, 4) * 8 // len(case.steps[1])
    assert np.mean(pos.max(axis=1) > pos.min(axis=1)) > 0.9


def test_no_new_obs_changes_every_parameter(cases, sfm):
    case = cases["no_new_obs"]
    tiny = sfm.make_problem("tiny")
    (c0, p0, f0), (c1, p1, f1) = case.params
    assert np.array_equal(c0, tiny.cam6) and np.array_equal(p0, tiny.pt3) and f0 == tiny.focal
    assert len(case.steps[1]) == 0 and len(case.steps[0]) == tiny.n_obs
    assert c1.shape == (tiny.n_cam + 2, 6) and p1.shape == (tiny.n_pt + 5, 3) and f1 != f0
    assert np.all(np.any(c1[:tiny.n_cam] != c0, axis=1)) and np.all(np.any(p1[:tiny.n_pt] != p0, axis=1))
    a, b = ac.step_problem(case, 0), ac.step_problem(case, 1)
    assert np.array_equal(a.obs_cam, b.obs_cam) and np.array_equal(a.obs_xy, b.obs_xy) and b.n_cam == a.n_cam + 2


@pytest.mark.parametrize("name", ac.CASES)
def test_oracle_linearises_every_step(cases, oracle, name):
    case = cases[name]
    oracle.set_num_threads(min(oracle.num_threads(), 16))
    for k in range(case.n_steps):
        sub = ac.step_problem(case, k)
        S, rhs, scale, info = oracle.build_reduced(sub, 1e4)
        cams, _ = _active(case, k)
        assert S.shape == (6 * len(cams) + 1,) * 2
        assert np.all(np.isfinite(S)) and np.all(np.isfinite(rhs)) and np.all(scale > 0)
        if name == "grow_from_one" and k in ac.SINGLE_VIEW_INFO:
            print("grow_from_one step %d (a point with a single view): oracle info %d" % (k, info))
            assert info == ac.SINGLE_VIEW_INFO[k]
        else:
            assert info == 0, (name, k, info)


def test_single_view_steps_the_oracle_against_long_double(cases, oracle):
    """Where a point has a single view the oracle's explicit fp64 inverse of the point block (cond 2e4) limits the ORACLE: the one
    measured tolerance of the GPU test (ac.MEASURED_TOL) is 4 x the deviation of a fresh handle from the oracle, and that deviation is
    the oracle's own distance from the same formulas in long double."""
    case = cases["grow_from_one"]
    own = {}
    for k in range(4):
        sub = ac.step_problem(case, k)
        res, jc, jp, jf = oracle.eval_jacobian(sub)
        S, rhs, scale, _ = oracle.build_reduced(sub, 1e4)
        Sl, rl, sl = ac.reduced_longdouble(sub, res, jc, jp, jf, 1e4)
        own[k] = (float(np.abs(S - Sl).max() / np.abs(Sl).max()), float(np.abs(rhs - rl).max() / np.abs(rl).max()))
        assert np.allclose(scale, sl.astype(np.float64), rtol=1e-14, atol=0)
        print("grow_from_one step %d: oracle vs long double S %.3g rhs %.3g (max |S| %.3g)" % (k, own[k][0], own[k][1], np.abs(S).max()))
    assert list(ac.MEASURED_TOL) == [("grow_from_one", 0)]
    tol = ac.MEASURED_TOL[("grow_from_one", 0)]
    for what, e in (("S", own[0][0]), ("rhs", own[0][1])):
        assert e > 1e-10                                       # the project's figure is beyond the oracle there ...
        assert 0.5 * tol[what] / 4 <= e <= 1.5 * tol[what] / 4          # ... and the measured base is the oracle's own error
    assert max(own[2]) <= 0.25e-10                             # the other single-view step: the oracle is good for 1e-10
    assert max(own[1] + own[3]) <= 1e-13                       # every point seen twice: rounding level
