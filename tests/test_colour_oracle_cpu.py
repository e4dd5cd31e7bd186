"""The CPU restatement of the seam levelling (tests/colour_oracle.py; the contract is in include/sfmba.h, "levelling the colours across
seams"), held against itself and against csrc/colour_math.h compiled for the host -- no GPU.

  * the two statements of the nodes, of the node colours, of a pass and of the levelled raster agree on every named case;
  * the cases exercise what they claim;
  * tools/micro/colour_math_host.hip -- the header the kernels run, compiled for the host under ASan + UBSan and run as its own process --
    agrees with the restatement in every intermediate (keys, sums, F, A, a, B, b, num, den, g of every pass, G and the texel);
  * LOCALITY (exact) and MONOTONE (on the planted grid);
  * the quality floor on the plane under two views of different exposure;
  * the new symbols are declared, exported and bound, and the refusals come before the device."""
import os
import subprocess

import numpy as np
import pytest

import colour_cases as cc
import colour_oracle as co
import texture_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sfmba_mesh_colour_nodes", "sfmba_mesh_colour_level", "sfmba_mesh_texture_levelled", "sfmba_mesh_texture_adjust")
ALL, PLANTED = list(cc.CASES), list(cc.PLANTED)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (a.astype(np.int64) == b.astype(np.int64)).all()


# ---- the two statements ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_the_two_statements_of_the_nodes_and_their_colours_agree(name):
    c, w = cc.case(name), cc.want(name)["nodes"]
    a = co.nodes_dict(c["xyz"], c["tri"], c["view"])
    for f in ("node_vertex", "node_view", "node_of"):
        assert same(a[f], w[f]), f
    assert a["n_nodes"] == w["n_nodes"]
    keys = (w["node_vertex"].astype(np.int64) << 32) | w["node_view"]
    assert (np.diff(keys) > 0).all()                                                       # distinct, in ascending key order
    on = co.contributing(c["xyz"], c["tri"], c["view"])
    assert ((w["node_of"] >= 0).all(axis=1) == on).all() and ((w["node_of"] < 0).all(axis=1) == ~on).all()
    seen, F, sums = co.colours_loop(c["xyz"], c["images"], c["K"], c["P"], w["node_vertex"], w["node_view"], c["radius"])
    assert same(seen, w["seen"]) and same(F, w["F"]) and same(sums, w["sums"])
    assert F.min(initial=0) >= 0 and F.max(initial=0) <= co.F_MAX
    if c["radius"] == 0 and len(F):
        assert same(F, 16 * sums)                                                          # r = 0: F = 16 s12 of the point sample
    if c["images"] and c["images"][0].ndim == 2 and len(F):
        assert (F[:, 0] == F[:, 1]).all() and (F[:, 0] == F[:, 2]).all()                   # a gray image: three equal channels


def _passes_agree(args, passes):
    node_vertex, seen, F, node_of, w = args
    history = []
    g, stats = co.level(node_vertex, seen, F, node_of, w, passes, history=history)
    states = [np.zeros_like(g)] + history
    for i in sorted(set(list(range(min(passes, 6))) + ([passes - 1] if passes else []))):
        assert same(co.pass_loop(node_vertex, seen, F, node_of, w, states[i]), states[i + 1]), i
    return g, stats


@pytest.mark.parametrize("name", ALL)
def test_the_two_statements_of_a_pass_agree_on_the_scenes(name):
    c, w = cc.case(name), cc.want(name)
    nd = w["nodes"]
    g, stats = _passes_agree((nd["node_vertex"], nd["seen"], nd["F"], nd["node_of"], c["weight"]), c["passes"])
    assert same(g, w["g"]) and same(stats, w["stats"])
    assert np.abs(g).max(initial=0) <= co.F_MAX and (g[nd["seen"] == 0] == 0).all()


@pytest.mark.parametrize("name", PLANTED)
def test_the_two_statements_of_a_pass_agree_on_planted_nodes(name):
    c, w = cc.planted_case(name), cc.want_planted(name)
    assert not co.refused_level(c["node_vertex"], c["F"], c["node_of"], len(c["node_vertex"]), c["weight"], c["passes"])
    g, stats = _passes_agree(cc.level_args(c)[:5], c["passes"])
    assert same(g, w["g"]) and same(stats, w["stats"])
    assert (g[c["seen"] == 0] == 0).all()


@pytest.mark.parametrize("name", ALL)
def test_the_two_statements_of_the_levelled_raster_agree(name):
    c, w = cc.case(name), cc.want(name)
    B = to.default_blocks_per_row(len(c["tri"])) if c["blocks_per_row"] is None else c["blocks_per_row"]
    Bl = B if len(c["tri"]) else 1
    atlas, n_clamped = co.raster_loop(c["xyz"], c["bgr"], c["tri"], c["images"], c["K"], c["P"], c["view"], c["patch"], Bl, w["nodes"]["node_of"], w["g"])
    assert same(atlas, w["tex"]["atlas"]) and n_clamped == w["tex"]["n_clamped"]
    zero = co.raster_np(c["xyz"], c["bgr"], c["tri"], c["images"], c["K"], c["P"], c["view"], c["patch"], Bl, w["nodes"]["node_of"], np.zeros_like(w["g"]))
    assert same(zero[0], to.raster_np(c["xyz"], c["bgr"], c["tri"], c["images"], c["K"], c["P"], c["view"], c["patch"], Bl)) and zero[1] == 0


# ---- the cases exercise what they claim ----------------------------------------------------------------------------------------------------
def _trace(c, g_before):
    trace = []
    co.pass_loop(c["node_vertex"], c["seen"], c["F"], c["node_of"], c["weight"], g_before, trace=trace)
    return trace


def test_the_cases_exercise_what_they_claim():
    w = cc.want
    assert w("blind_node")["stats"][1] == 1 and w("blind_node")["nodes"]["seen"].tolist() == [0, 1, 1]
    assert cc.want_planted("blind_among")["stats"][1] == 3
    for n, k in ((2, 2), (3, 2), (4, 4)):                                                   # the most siblings on one vertex
        nd = w("grid_%d_views" % n)["nodes"]
        assert np.bincount(nd["node_vertex"]).max() == k and w("grid_%d_views" % n)["stats"][2] > 0
    assert np.bincount(w("grid_3_views")["nodes"]["node_vertex"]).max() == 2
    assert np.bincount(w("fan_nine_views")["nodes"]["node_vertex"])[0] == 9 and w("fan_nine_views")["stats"][2] == 300
    assert (w("fan_one_view")["nodes"]["node_of"][:, 0] == 0).all() and w("fan_one_view")["stats"][2] == 0      # one node, a run of 300 entries
    assert w("all_unlabelled")["stats"][0] == 0 and w("one_labelled")["stats"][0] == 3
    sp = w("spoiled_mesh")["nodes"]["node_of"]
    assert (sp[3] == -1).all() and ((sp < 0).all(axis=1).sum() >= 3)                         # the repeated index, and the triangles on the NaN vertex
    assert w("disjoint")["stats"][0] == 3 * 20 and w("disjoint")["stats"][2] == 0
    for r in (0, 1, 2):                                                                      # all three vertices clamp to the pixel (7, 0)
        c, nd = cc.case("corner_r%d" % r), w("corner_r%d" % r)["nodes"]
        corner = [256 * int(v) for v in c["images"][0][0, 7]]                               # 1/256 grey level
        assert nd["seen"].tolist() == [1, 1, 1] and nd["F"].tolist() == [nd["F"][0].tolist()] * 3
        assert (nd["F"][0].tolist() == corner) == (r == 0)                                  # r > 0: the window reaches inwards, and is clamped outwards
        img = c["images"][0].astype(np.int64)
        window = img[0:r + 1, 7 - r:8]                                                      # the pixels of the window, the clamped ones counted again
        counts = np.outer([r + 1] + [1] * r, [1] * r + [r + 1])
        assert nd["sums"][0].tolist() == (16 * (window * counts[..., None]).sum(axis=(0, 1))).tolist()
    assert [im.shape[:2] for im in cc.case("tiny_images_bgr")["images"]] == [(1, 1), (2, 2), (7, 9)]
    assert cc.case("tiny_images_gray")["images"][0].ndim == 2 and len({im.shape for im in cc.case("strip_21")["images"]}) > 1
    assert w("passes_0")["stats"][3] == w("passes_0")["stats"][4] and w("passes_0")["stats"][5] == 0
    assert w("passes_1024")["stats"][7] == 1024 and w("passes_1024")["stats"][4] < w("passes_2")["stats"][4] < w("passes_0")["stats"][4]
    assert w("weight_256")["stats"][4] < w("grid_3_views")["stats"][4] < w("weight_1")["stats"][4]
    for n in (21, 22, 43, 85, 86, 171, 10922, 10923):
        assert len(cc.case("strip_%d" % n)["tri"]) == n and w("strip_%d" % n)["stats"][2] > 0
    assert 3 * 10922 < 32768 <= 3 * 10923
    assert sum(w(n)["tex"]["n_clamped"] > 0 for n in cc.CASES) >= 5
    # a permutation of the triangles: the same offset per (vertex, view)
    a, b = w("grid_4_views"), w("grid_permuted")
    assert same(a["nodes"]["node_vertex"], b["nodes"]["node_vertex"]) and same(a["nodes"]["node_view"], b["nodes"]["node_view"]) and same(a["g"], b["g"])
    assert not same(a["nodes"]["node_of"], b["nodes"]["node_of"])
    # the clamp of the offsets binds at both ends
    for name, sign in (("clamp_high", 1), ("clamp_low", -1)):
        c = cc.planted_case(name)
        history = []
        g, stats = co.level(*cc.level_args(c), history=history)
        assert sign * g[0, 0] == co.F_MAX and stats[5] == co.F_MAX
        raw = [(2 * num + den) // (2 * den) for i in range(c["passes"]) for (n, ch, A, a_, B, b_, num, den) in _trace(c, ([np.zeros_like(g)] + history)[i]) if den]
        assert max(sign * v for v in raw) > co.F_MAX
    # numerators on a half on both sides of zero: floor((2 num + den) / (2 den)) rounds both up
    halves = [(num, den) for (n, ch, A, a_, B, b_, num, den) in _trace(cc.planted_case("halves"), np.zeros((5, 3), np.int32)) if den and (2 * num) % den == 0 and (2 * num // den) % 2]
    assert any(num > 0 for num, den in halves) and any(num < 0 for num, den in halves)
    assert cc.want_planted("halves")["g"][:2, 0].tolist() == [1, 0]                          # +1/2 -> 1 and -1/2 -> 0
    assert cc.want_planted("no_nodes")["stats"].tolist() == [0, 0, 0, 0, 0, 0, 0, 3]


# ---- LOCALITY and MONOTONE -------------------------------------------------------------------------------------------------------------------
def _distance_to_a_seam(node_vertex, seen, node_of):
    see, vert, src, dst = co._structure_np(node_vertex, seen, node_of)
    k = np.bincount(vert[see], minlength=int(vert.max()) + 1)
    dist = np.where(see & (k[vert] >= 2), 0, -1)
    links = [[] for _ in vert]
    for s, d in zip(src.tolist(), dst.tolist()):
        if see[s]:
            links[s].append(d)
    front, d = np.flatnonzero(dist == 0).tolist(), 0
    while front:
        d += 1
        nxt = []
        for n in front:
            for u in links[n]:
                if dist[u] < 0:
                    dist[u] = d
                    nxt.append(u)
        front = nxt
    return dist                                                                              # -1: no seam is reachable


@pytest.mark.parametrize("passes", [0, 1, 2, 3, 4])
def test_locality_an_offset_travels_one_link_per_pass(passes):
    """EXACT: after N passes a node at N or more links from every seam vertex (so every node farther than N) has g = 0, and a triangle whose
    three nodes have g = 0 has the texels of the plain raster."""
    c = cc.case("grid_2_views")
    nd = cc.want("grid_2_views")["nodes"]
    g, _ = co.level(nd["node_vertex"], nd["seen"], nd["F"], nd["node_of"], c["weight"], passes)
    dist = _distance_to_a_seam(nd["node_vertex"], nd["seen"], nd["node_of"])
    far = (dist < 0) | (dist >= passes)
    assert (g[far] == 0).all() and far.sum() > 10
    if passes:
        assert (g[dist == passes - 1] != 0).any()                                           # and no slower
    B = to.default_blocks_per_row(len(c["tri"]))
    atlas, _ = co.raster_np(c["xyz"], c["bgr"], c["tri"], c["images"], c["K"], c["P"], c["view"], c["patch"], B, nd["node_of"], g)
    plain = to.raster_np(c["xyz"], c["bgr"], c["tri"], c["images"], c["K"], c["P"], c["view"], c["patch"], B)
    quiet = (g[np.maximum(nd["node_of"], 0)] == 0).all(axis=(1, 2))
    owner = to.ownership(len(c["tri"]), c["patch"], B, atlas.shape[1], atlas.shape[0])[0]
    untouched = (owner >= 0) & quiet[np.maximum(owner, 0)]
    assert (untouched.sum() > 100 or passes == 4) and (atlas[untouched] == plain[untouched]).all()      # (after 4 passes no triangle is left)
    if passes:
        assert (atlas != plain).any()


@pytest.mark.parametrize("weight", [1, 4, 16])
def test_monotone_the_spread_at_the_seam_never_rises(weight):
    c = cc.planted_case("planted_grid")
    history = []
    co.level(c["node_vertex"], c["seen"], c["F"], c["node_of"], weight, 33, history=history)
    spread = [co.spreads(c["node_vertex"], c["seen"], c["F"], g)[2] for g in [np.zeros_like(history[0])] + history]
    print("planted grid, w = %d: the summed spread after 0 / 1 / 4 / 16 / 33 passes: %s" % (weight, [spread[i] for i in (0, 1, 4, 16, 33)]))
    assert len(spread) == 34 and all(b <= a for a, b in zip(spread, spread[1:])) and spread[16] < spread[0]


# ---- csrc/colour_math.h on the host --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path_factory.mktemp("colour") / "colour_math_host")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sfm-toy-library_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tools", "micro", "colour_math_host.hip")])
    return exe


def _bits(a):
    return " ".join(str(v) for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32).tolist())


def _ints(a):
    return " ".join(str(v) for v in np.asarray(a).reshape(-1).tolist())


def scene_input(c, Bl):
    ch = 1 if c["images"] and c["images"][0].ndim == 2 else 3
    rows = ["0", "%d %d %d %d %d %d %d %d %d" % (len(c["xyz"]), len(c["tri"]), len(c["images"]), ch, c["radius"], c["weight"], c["passes"], c["patch"], Bl),
            _bits(c["K"])]
    P = np.asarray(c["P"], np.float32).reshape(-1, 12)
    for i, im in enumerate(c["images"]):
        rows += ["%d %d" % (im.shape[1], im.shape[0]), _bits(P[i]), _ints(im)]
    rows += [_bits(c["xyz"]), _ints(c["tri"]), _ints(c["view"])]
    return "\n".join(rows) + "\n"


def planted_input(c):
    rows = ["1", "%d %d %d %d" % (len(c["node_vertex"]), len(c["node_of"]), c["weight"], c["passes"])]
    rows += ["%d %d %s" % (c["node_vertex"][n], c["seen"][n], _ints(c["F"][n])) for n in range(len(c["node_vertex"]))]
    rows += [_ints(c["node_of"])]
    return "\n".join(rows) + "\n"


def pass_lines(node_vertex, seen, F, node_of, w, passes):
    """the P, G lines and the statistics from the LOOP statement"""
    lines, g = [], np.zeros((len(node_vertex), 3), np.int32)
    for p in range(passes):
        trace = []
        new = co.pass_loop(node_vertex, seen, F, node_of, w, g, trace=trace)
        lines += ["P %d %d %d %d %d %d %d %d %d %d" % (p, n, ch, A, a, B, b, num, den, new[n, ch]) for (n, ch, A, a, B, b, num, den) in trace]
        g = new
    lines += ["G %d %d %d %d" % (n, *g[n].tolist()) for n in range(len(g))]
    _, stats = co.level(node_vertex, seen, F, node_of, w, passes, pass_fn=lambda *a: co.pass_loop(*a))
    return lines, g, stats


def scene_lines(c, Bl):
    """what tools/micro/colour_math_host.hip prints for a scene, from the loop statements of the restatement"""
    on = co.contributing(c["xyz"], c["tri"], c["view"])
    lines = ["K %d %d %d" % (t, q, ((int(c["tri"][t, q]) << 32) | int(c["view"][t])) if on[t] else (1 << 64) - 1) for t in range(len(c["tri"])) for q in range(3)]
    nd = co.nodes_dict(c["xyz"], c["tri"], c["view"])
    lines += ["N %d %d %d" % (n, nd["node_vertex"][n], nd["node_view"][n]) for n in range(nd["n_nodes"])]
    lines += ["O %d %d %d %d" % (t, *nd["node_of"][t].tolist()) for t in range(len(c["tri"]))]
    seen, F, sums = co.colours_loop(c["xyz"], c["images"], c["K"], c["P"], nd["node_vertex"], nd["node_view"], c["radius"])
    lines += ["C %d %d %d %d %d %d %d %d" % (n, seen[n], *sums[n].tolist(), *F[n].tolist()) for n in range(nd["n_nodes"])]
    more, g, stats = pass_lines(nd["node_vertex"], seen, F, nd["node_of"], c["weight"], c["passes"])
    trace = []
    _, n_clamped = co.raster_loop(c["xyz"], c["bgr"], c["tri"], c["images"], c["K"], c["P"], c["view"], c["patch"], Bl, nd["node_of"], g, trace=trace)
    lines += more + ["X %d %d %d %d %d %d %d %d %d %d" % (t, i, j, *G, *px, int(cl)) for (t, i, j, G, px, cl) in trace]
    stats[6] = n_clamped
    return lines + ["Z " + _ints(stats)]


def _run_host(host_exe, tmp_path, text, want):
    path = tmp_path / "case.txt"
    path.write_text(text)
    got = subprocess.run([host_exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert got.returncode == 0, got.stderr[-2000:]
    lines = got.stdout.splitlines()
    assert len(lines) == len(want), (len(lines), len(want))
    for a, b in zip(lines, want):
        assert a == b, (a, b)


@pytest.mark.parametrize("name", ALL)
def test_colour_math_on_the_host_equals_the_restatement_in_every_intermediate(host_exe, tmp_path, name):
    c = cc.case(name)
    B = to.default_blocks_per_row(len(c["tri"])) if c["blocks_per_row"] is None else c["blocks_per_row"]
    Bl = B if len(c["tri"]) else 1
    _run_host(host_exe, tmp_path, scene_input(c, Bl), scene_lines(c, Bl))


@pytest.mark.parametrize("name", PLANTED)
def test_colour_math_on_the_host_equals_the_restatement_on_planted_nodes(host_exe, tmp_path, name):
    c = cc.planted_case(name)
    lines, _, stats = pass_lines(*cc.level_args(c))
    _run_host(host_exe, tmp_path, planted_input(c), lines + ["Z " + _ints(stats)])


# ---- the quality floor ----------------------------------------------------------------------------------------------------------------------
def test_quality_on_the_plane_under_two_exposures():
    """The texture suite's plane at depth 10 under two 160 x 120 views at +-15 degrees, the second photograph brighter by 20 levels, the
    labels of the plain rule, the defaults 16 passes / weight 16 / radius 1.  CONDITION: the summed spread at the seam vertices falls to
    a quarter at most and no texel clamps.  MEASURED on this restatement: 138084 -> 3356, a ratio of 0.024304 < 1/8, so the GATE is twice
    the measured ratio."""
    st = cc.quality_want()["level_stats"]
    print("quality scene: %s; ratio %.6f" % (dict(zip(co.STATS, st.tolist())), st[4] / st[3]))
    assert st[2] == 9 and st[3] > 9 * 3 * 15 * 256                                         # every seam vertex sees a step of 15 levels or more
    assert 4 * st[4] <= st[3] and st[6] == 0
    assert 1000000 * st[4] <= 2 * cc.QUALITY_RATIO_MEASURED_PPM * st[3]


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
    assert os.path.exists(os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "colour_math.h"))
    for text in ("levelling the colours across seams", "unless asked for (off by default)", "Poisson blending", "per-view gain or gamma"):
        assert text in header, text


def test_refusals_come_before_the_device():
    """The argument checks need no device: each returns SFMBA_ERR_INVALID_ARG (1) and writes nothing.  (The full list, with the refusals
    found on the device, runs with the GPU tests, which share refusal_calls.)"""
    import __graft_entry__ as ge
    ge.build_hip()
    from sfm_toy_library_amd import capi
    import colour_refusals as cr
    calls = cr.refusal_calls(capi)
    assert len(calls) > 150
    for name, call in calls:
        rc, untouched = call()
        assert rc == 1 and untouched, name
