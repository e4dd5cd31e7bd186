"""The CPU restatement of the view-label smoothing (tests/label_oracle.py; the contract is in include/sfmba.h), held against itself and
against csrc/label_math.h compiled for the host -- no GPU.

  * the two statements of the candidates, of the adjacency and of the smoothing agree on every case of tests/label_cases.py;
  * the cases exercise what they claim;
  * the movers of a pass are pairwise non-adjacent, the energy falls each pass by exactly the sum of the movers' gains, and every label is
    one of the triangle's own candidates;
  * tools/micro/label_math_host.hip -- the header the kernels run, compiled for the host under ASan + UBSan and run as its own process --
    agrees with the restatement in every intermediate (the lists, adj, the sums of every ring, rank, D, the gains, the movers, the energy);
  * the quality floor on the noisy wall;
  * the new symbols are declared, exported and bound, and the refusals come before the device."""
import os
import subprocess

import numpy as np
import pytest

import label_cases as lc
import label_oracle as lo
import texture_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sfmba_mesh_view_candidates", "sfmba_mesh_adjacency", "sfmba_mesh_view_smooth", "sfmba_mesh_texture_from_views",
               "sfmba_mesh_texture_smooth")
# MEASURED ONCE on the restatement (smooth_np) on the wall of tests/label_cases.py at min_area 0, K = 4, r = 8, p = 256, 100 passes, and
# written to profiles/texture_smooth.txt; the gates are twice these
WALL_DIFF_END_MEASURED = 2501
WALL_AREA_GIVEN_UP_MEASURED = 0.064349


@pytest.fixture(scope="module", autouse=True)
def the_contract_exists():
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    for name in NEW_SYMBOLS:
        assert "SFMBA_API int %s(" % name in header, name
    assert os.path.exists(os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "label_math.h"))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (a.astype(np.int64) == b.astype(np.int64)).all()


# ---- the two statements ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in lc.CASES if lc.case(n)["scene"] is not None])
def test_the_two_statements_of_the_candidates_agree(name):
    c, w = lc.case(name), lc.want(name)
    cv, cs = lo.candidates_loop(*lc.candidate_args(c))
    assert same(cv, w["cand_view"]) and same(cs, w["cand_score"])
    s = c["scene"]
    plain = to.views_np(s["xyz"], s["tri"], s["images"], s["K"], s["P"], s["depth_maps"], s["occl_tol"], s["min_area"])
    if len(c["tri"]):
        assert same(cv[:, 0], plain[0]) and same(cs[:, 0], plain[1])                      # rank 0 is the texture call's choice
        used = cv >= 0
        assert (used[:, :-1] >= used[:, 1:]).all() and (cs[~used] == 0).all() and (cs[used] > 0).all() and (cs[used] < lo.SCORE_LIMIT).all()
        assert (cs[:, :-1] >= cs[:, 1:]).all()
        tie = used[:, 1:] & (cs[:, :-1] == cs[:, 1:])
        assert (cv[:, :-1][tie] < cv[:, 1:][tie]).all()


@pytest.mark.parametrize("name", list(lc.CASES))
def test_the_two_statements_of_the_adjacency_agree(name):
    c, w = lc.case(name), lc.want(name)
    adj, n_pairs, n_open, n_bad = lo.adjacency_dict(c["tri"])
    assert same(adj, w["adj"]) and (n_pairs, n_open, n_bad) == (w["n_pairs"], w["n_open_edges"], w["n_nonmanifold_edges"])
    for t, row in enumerate(adj.tolist()):                                                # symmetric, and as many links as pairs
        for n in row:
            assert n < 0 or (n != t and row.count(n) == adj[n].tolist().count(t))
    assert (adj >= 0).sum() == 2 * n_pairs


@pytest.mark.parametrize("name", list(lc.CASES))
def test_the_two_statements_of_the_smoothing_agree_and_every_pass_keeps_its_promises(name):
    c, w = lc.case(name), lc.want(name)
    cv, cs, adj = w["cand_view"], w["cand_score"], w["adj"]
    a, b = lo.smooth_loop(cv, cs, adj, c["rings"], c["penalty"], c["max_passes"]), w["smooth"]
    for f in ("view", "stats", "start", "s"):
        assert same(a[f], b[f]), f
    assert len(a["trace"]) == len(b["trace"])
    view = a["start"].copy()
    for i, (pa, pb) in enumerate(zip(a["trace"], b["trace"])):
        assert pa == pb, i
        movers = set(pa["movers"])
        for t in movers:                                                                     # pairwise non-adjacent
            assert not movers & set(adj[t].tolist())
        after = a["trace"][i + 1]["energy"] if i + 1 < len(a["trace"]) else a["energy_end"]
        assert pa["energy"] - after == sum(pa["gains"][t] for t in movers)                   # E falls by exactly the movers' gains
        assert all(pa["gains"][t] > 0 for t in movers) and min(pa["gains"], default=0) >= 0
    assert a["stats"][0] == (a["trace"][0]["energy"] if a["trace"] else a["energy_end"]) and a["stats"][1] == a["energy_end"]
    assert a["stats"][6] == sum(len(p["movers"]) for p in a["trace"]) and a["stats"][7] == sum(1 for p in a["trace"] if p["movers"])
    for t, v in enumerate(a["view"].tolist()):                                           # a label is one of the triangle's own candidates
        assert (v == -1 and cv[t, 0] == -1) if v < 0 or cv[t, 0] < 0 else v in cv[t].tolist()
    if c["rings"] == 0 and len(cv):
        assert same(a["start"], cv[:, 0])


# ---- the cases exercise what they claim ----------------------------------------------------------------------------------------------------
def test_the_cases_exercise_what_they_claim():
    w = lc.want
    assert w("three_on_an_edge")["n_nonmanifold_edges"] == 1 and (w("three_on_an_edge")["adj"][:3] == -1).sum() >= 3
    assert w("four_on_an_edge")["n_nonmanifold_edges"] == 1
    assert w("doubled_triangle")["adj"][0].tolist() == [1, 1, 1] and w("doubled_triangle")["n_pairs"] == 4
    assert (w("repeated_index")["adj"][5] == -1).all() and w("repeated_index")["adj"][4].tolist().count(-1) == 2
    assert (w("spoiled_mesh")["cand_view"][3] == -1).all() and (w("nan_coordinate")["cand_view"][3] == -1).all()
    hole = w("hole_in_a_region")
    assert hole["smooth"]["view"][16] == -1 and hole["smooth"]["stats"][5] == (hole["adj"][16] >= 0).sum() > 0
    assert (w("no_images")["cand_view"] == -1).all() and w("three_views_k8")["cand_view"].shape[1] == 8
    assert (w("three_views_k8")["cand_view"][:, 3:] == -1).all() and (w("three_views_k8")["cand_view"][:, 2] >= 0).any()
    for name in ("k1_nothing_moves", "k1_planted"):
        assert w(name)["smooth"]["stats"][6] == 0 and w(name)["smooth"]["stats"][0] == w(name)["smooth"]["stats"][1]
    assert lc.want("equal_scores_scene")["cand_view"].tolist() == [[0, 1]] and len(set(lc.want("equal_scores_scene")["cand_score"][0].tolist())) == 1
    eq = w("equal_scores")
    assert ((eq["cand_score"][:, :-1] == eq["cand_score"][:, 1:]) & (eq["cand_view"][:, 1:] >= 0)).any(axis=1)[eq["cand_view"][:, 1] >= 0].all()
    assert (eq["cand_view"][:, 1] >= 0).sum() > 20
    for passes in (1, 2, 100):                                                           # one triangle per pass, the same gain every time
        ch = w("chain_%d" % passes)["smooth"]
        assert [p["movers"] for p in ch["trace"]] == [[i + 1] for i in range(passes)]
        assert all(p["gains"][i + 1] == 255 for i, p in enumerate(ch["trace"]))
        assert ch["stats"][6] == ch["stats"][7] == passes and same(ch["view"][:passes + 3], [1] * (passes + 1) + [0, 0])
    assert w("penalty_0")["smooth"]["stats"][1] == 0 and same(w("penalty_0")["smooth"]["view"], w("penalty_0")["cand_view"][:, 0])      # all back to rank 0
    assert w("penalty_65535")["smooth"]["stats"][6] > 0
    assert w("top_scores_r8")["smooth"]["s"].max() > 1 << 52 and w("top_scores_r8")["smooth"]["s"].max() < 1 << 53
    assert w("exact_D")["smooth"]["D"].tolist() == [[0, 512, 0], [0, 640, 0], [0, 999, 1000], [0, 1, 1023]]
    assert w("min_area_floor")["smooth"]["stats"][5] > 0                                 # a frontier between textured and untextured
    moved = [n for n in lc.SMALL if w(n)["smooth"]["stats"][6] > 0]
    differ = [n for n in lc.SMALL if not same(w(n)["smooth"]["start"], w(n)["cand_view"][:, 0] if len(w(n)["cand_view"]) else [])]
    print("cases in which a pass moves something: %d, in which the diffusion changes the start: %d of %d" % (len(moved), len(differ), len(lc.SMALL)))
    assert len(moved) >= 12 and len(differ) >= 10
    assert any(w(n)["smooth"]["stats"][6] > 0 for n in lc.SCENES)


def test_the_sphere_at_the_area_floor_is_mostly_frontier():
    """At min_area 256 nearly every pair of the six-view sphere that 'differs' has one side at -1: a frontier, not a seam."""
    s = lc.sphere_scene(256)
    cv, cs = lo.candidates_np(s["xyz"], s["tri"], s["images"], s["K"], s["P"], s["depth_maps"], s["occl_tol"], 256, 4)
    adj = lo.adjacency_sort(s["tri"])[0]
    st = lo.smooth_np(cv, cs, adj, 0, 1024, 100)["stats"]
    pairs, changes = to.view_changes(s["tri"], cv[:, 0])
    print("six-view sphere, min_area 256: %d pairs, view_changes %d = %d seams + %d frontier; relaxation alone moves %d" %
          (pairs, changes, st[2], st[5], st[6]))
    assert changes == st[2] + st[5] and st[5] > 10 * st[2]


# ---- csrc/label_math.h on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path_factory.mktemp("labels") / "label_math_host")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sfm-toy-library_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tools", "micro", "label_math_host.hip")])
    return exe


def host_input(c, w, scores):
    nt, k = len(c["tri"]), c["k"]
    rows = ["%d %d %d %d %d %d" % (nt, k, c["rings"], c["penalty"], c["max_passes"], scores.shape[1] if scores is not None else 0)]
    for a in (c["tri"], w["cand_view"], w["cand_score"]) + (() if scores is None else (scores,)):
        rows += [" ".join(str(v) for v in r) for r in np.asarray(a).reshape(nt, -1).tolist()] if nt else []
    return "\n".join(rows) + "\n"


def host_lines(c, w, scores):
    """what tools/micro/label_math_host.hip prints, from the loop statements of the restatement"""
    nt, k = len(c["tri"]), c["k"]
    lines = []
    if scores is not None and scores.shape[1]:
        lines += ["L %d %s %s" % (t, " ".join(map(str, w["cand_view"][t].tolist())), " ".join(map(str, w["cand_score"][t].tolist()))) for t in range(nt)]
    adj, n_pairs, n_open, n_bad = lo.adjacency_dict(c["tri"])
    lines += ["A %d %d %d %d" % (t, *adj[t].tolist()) for t in range(nt)] + ["N %d %d %d" % (n_pairs, n_open, n_bad)]
    for r in range(c["rings"]):
        s = lo.smooth_loop(w["cand_view"], w["cand_score"], adj, r + 1, c["penalty"], 0)["s"]
        lines += ["S %d %d %s" % (r, t, " ".join(map(str, s[t].tolist()))) for t in range(nt)]
    sm = lo.smooth_loop(w["cand_view"], w["cand_score"], adj, c["rings"], c["penalty"], c["max_passes"])
    lines += ["B %d %d %d %s" % (t, _start_rank(sm, w, t), sm["start"][t], " ".join(map(str, sm["D"][t].tolist()))) for t in range(nt)]
    view = sm["start"].copy()
    for i, p in enumerate(sm["trace"]):
        lines.append("E %d %d" % (i, p["energy"]))
        kstar = _kstar(w["cand_view"], sm["D"], adj, view, c["penalty"], _ranks(w["cand_view"], view))
        lines += ["G %d %d %d %d" % (i, t, p["gains"][t], kstar[t]) for t in range(nt)]
        lines += ["M %d %d" % (i, t) for t in p["movers"]]
        for t in p["movers"]:
            view[t] = w["cand_view"][t][kstar[t]]
    lines += ["F %d %d" % (t, sm["view"][t]) for t in range(nt)] + ["Z " + " ".join(map(str, sm["stats"].tolist()))]
    return lines


def _ranks(cv, view):
    return [cv[t].tolist().index(view[t]) if view[t] >= 0 else -1 for t in range(len(view))]


def _start_rank(sm, w, t):
    return w["cand_view"][t].tolist().index(sm["start"][t]) if sm["start"][t] >= 0 else -1


def _kstar(cv, D, adj, view, p, rank):
    out = list(rank)
    for t in range(len(view)):
        best = None
        for k in range(cv.shape[1]):
            if rank[t] < 0 or cv[t, k] < 0:
                continue
            e = int(D[t, k]) + p * sum(1 for n in adj[t] if n >= 0 and view[n] >= 0 and view[n] != cv[t, k])
            if best is None or e < best:
                best, out[t] = e, k
    return out


HOST_CASES = list(lc.CASES)                       # the chains and the sphere included


@pytest.mark.parametrize("name", HOST_CASES)
def test_label_math_on_the_host_equals_the_restatement_in_every_intermediate(host_exe, tmp_path, name):
    c, w = lc.case(name), lc.want(name)
    scores = None
    if c["scene"] is not None:
        scores = lo.scores_np(*lc.candidate_args(c)[:-1])
    path = tmp_path / "case.txt"
    path.write_text(host_input(c, w, scores))
    got = subprocess.run([host_exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert got.returncode == 0, got.stderr[-2000:]
    want = host_lines(c, w, scores)
    lines = got.stdout.splitlines()
    assert len(lines) == len(want), (len(lines), len(want))
    for a, b in zip(lines, want):
        assert a == b, (a, b)


# ---- the quality floor ----------------------------------------------------------------------------------------------------------------------
def test_quality_on_the_wall():
    """The noisy wall under five similar views (tests/label_cases.py).  CONDITION: the final count of pairs with different views is at
    most half the count under rank 0.  GATE: at most twice the count and twice the mean relative area given up that were measured
    once on this restatement."""
    c, w = lc.wall(), lc.wall_want()
    st = w["smooth"]["stats"]
    assert len(c["tri"]) == 18432 and (w["cand_view"][:, 0] >= 0).mean() > 0.99           # (the noise folds a few triangles over)
    pairs = int((w["adj"] >= 0).sum()) // 2
    given_up = lc.mean_area_given_up(w["cand_score"], w["cand_view"], w["smooth"]["view"])
    print("wall: %d pairs; different views: rank 0 %d (%.4f), start %d (%.4f), end %d (%.4f); %d moves in %d passes; mean area given up %.6f; E %d -> %d" %
          (pairs, st[2], st[2] / pairs, st[3], st[3] / pairs, st[4], st[4] / pairs, st[6], st[7], given_up, st[0], st[1]))
    assert 2 * st[4] <= st[2]
    assert st[4] <= 2 * WALL_DIFF_END_MEASURED and given_up <= 2.0 * WALL_AREA_GIVEN_UP_MEASURED


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build_hip()
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    lib = os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "libsfmba_hip.so")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    from sfm_toy_library_amd import capi
    for name in NEW_SYMBOLS:
        assert "SFMBA_API int %s(" % name in header
        assert " T %s\n" % name in exported
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name) and callable(getattr(capi, name[len("sfmba_"):]))
    assert capi.lib().sfmba_abi_version() == 6
    for text in ("OFF BY DEFAULT", "OUT OF SCOPE", "2^53"):
        assert text in header, text


def test_refusals_come_before_the_device():
    """The argument checks need no device: each returns SFMBA_ERR_INVALID_ARG (1) and writes nothing.  (The full list, with the refusals
    found on the device, runs with the GPU tests, which share refusal_calls.)"""
    import __graft_entry__ as ge
    ge.build_hip()
    from sfm_toy_library_amd import capi
    import label_refusals as lr
    calls = lr.refusal_calls(capi)
    assert len(calls) > 150
    for name, call in calls:
        rc, untouched = call()
        assert rc == 1 and untouched, name
