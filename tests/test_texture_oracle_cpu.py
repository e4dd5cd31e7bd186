"""The CPU restatement of sfmba_mesh_texture (tests/texture_oracle.py; the contract is in include/sfmba.h), held against itself and
against csrc/texture_math.h compiled for the host -- no GPU.

  * the two statements of the view choice (a loop per triangle and view; numpy over all pairs) and of the raster (a loop per block
    and texel; numpy over the atlas with an ownership map) agree bit for bit on every case of tests/texture_cases.py;
  * the cases exercise what they claim;
  * tools/micro/texture_math_host.hip -- the header the kernels run, compiled for the host under ASan + UBSan and run as its own
    process -- agrees with the restatement in every intermediate (q, u, v, su, sv, a2, the flags, X, s12, the texel, the fallback);
  * every atlas texel is owned by at most one triangle, and inside every uv triangle the four texels of a bilinear fetch belong to
    that triangle (exhaustively over a 1/8-texel lattice, S = 3 .. 8);
  * a permutation of views without ties permutes the labels and nothing else; gray equals BGR of (g, g, g);
  * the planted sphere confirms the sign of the area; the quality floor on the plane;
  * the new symbols are declared, exported and bound, and the refusals come before the device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
import texture_cases as tc
import texture_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sfmba_mesh_texture_size", "sfmba_mesh_texture")
ALL = list(tc.CASES)


@pytest.fixture(scope="module", autouse=True)
def the_contract_exists():
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    for name in NEW_SYMBOLS:
        assert "SFMBA_API int %s(" % name in header, name
    assert os.path.exists(os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "texture_math.h"))


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same(got, want, what):
    assert (got is None) == (want is None), what
    if want is None:
        return
    assert set(got) == set(want), what
    for f in want:
        if isinstance(want[f], np.ndarray) or want[f] is None:
            assert same_bits(got[f], want[f]), (what, f)
        else:
            assert got[f] == want[f], (what, f)


# ---- the two statements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL + list(tc.REFUSED))
def test_two_statements_agree(name):
    c = tc.case(name)
    assert_same(to.texture(*tc.args(c), views_fn=to.views_loop, raster_fn=to.raster_loop), tc.want(name), name)


def test_two_statements_agree_on_the_quality_scene():
    c = tc.quality_scene()
    assert_same(to.texture(*tc.args(c), views_fn=to.views_loop, raster_fn=to.raster_loop), to.texture(*tc.args(c)), "quality")


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def test_cases_exercise_what_they_claim():
    w = tc.want
    for n in (0, 1, 2, 3, 63, 64, 65, 255, 256, 257):
        c, r = tc.case("nt_%d" % n), w("nt_%d" % n)
        assert len(c["tri"]) == n and len(r["view"]) == n and r["uv"].shape == (n, 3, 2)
        assert n == 0 or r["n_textured"] > 0.8 * n, (n, r["n_textured"])
    assert w("nt_0")["atlas"].shape == (4, 5, 3) and not w("nt_0")["atlas"].any() and w("nt_0")["n_textured"] == 0
    assert w("nt_1")["atlas"].shape == (4, 10, 3) and w("nt_3")["atlas"].shape == (4, 10, 3)
    # an odd count leaves the second half of the last block at 0, and the blocks past n_blocks too
    owner, _, _ = to.ownership(17, 4, 3, 15, 12)
    assert (owner == -1).sum() == 10 and not w("blocks_9_odd")["atlas"][owner == -1].any() and w("blocks_9_odd")["atlas"][owner >= 0].any()
    assert [w(n)["atlas"].shape[:2] for n in ("blocks_8_of_9", "blocks_9_of_9", "blocks_10_of_9")] == [(12, 15), (12, 15), (16, 15)]
    owner, _, _ = to.ownership(20, 4, 3, 15, 16)
    assert (owner[12:, 5:] == -1).all() and not w("blocks_10_of_9")["atlas"][12:, 5:].any()
    assert [w("one_column_S%d" % s)["atlas"].shape[:2] for s in (3, 4, 6)] == [(9, 4), (12, 5), (18, 7)] and w("one_column_S64")["atlas"].shape == (128, 65, 3)
    # the exact scenes
    assert w("front")["view"].tolist() == [0] and w("front")["score"].tolist() == [1024]
    for name in ("behind_zero", "behind_minus", "outside_u_0", "outside_u_w1", "back_facing", "below_min_area", "no_area", "above_occl_tol", "zs_zero"):
        assert w(name)["view"].tolist() == [-1] and w(name)["score"].tolist() == [0] and w(name)["n_textured"] == 0, name
    for name in ("on_u_0", "on_u_w1", "on_min_area", "on_occl_tol"):
        assert w(name)["view"].tolist() == [0] and w(name)["score"].tolist() == [1024], name
    k4 = to.k4_of(tc.case("front")["K"])

    def first_vertex(name, corner=0):
        c = tc.case(name)
        X = c["xyz"].astype(np.float64)[c["tri"][0, corner]].tolist()
        p = c["P"].astype(np.float64).reshape(-1, 12)[0].tolist()
        return to.vertex(k4, p, X, 8, 8, c["depth_maps"][0], float(np.float32(c["occl_tol"])))
    assert first_vertex("behind_zero")[1][2] == 0.0 and first_vertex("behind_minus")[1][2] == -1.0
    assert first_vertex("on_u_0")[2] == 0.0 and first_vertex("outside_u_0")[2] == -2.0 ** -51
    assert first_vertex("on_u_w1", 2)[2] == 7.0 and first_vertex("outside_u_w1", 2)[2] == 7.0 + 2.0 ** -50
    assert first_vertex("on_occl_tol")[1][2] - 0.75 == 0.25 and first_vertex("above_occl_tol")[1][2] - 0.75 == 0.25 + 2.0 ** -52
    c = tc.case("back_facing")
    assert to.candidate(k4, c["P"].astype(np.float64).reshape(-1)[:12].tolist(), c["xyz"].astype(np.float64)[c["tri"][0]].tolist(), 8, 8, None, 0.25) == (True, 1024)
    c = tc.case("no_area")
    assert to.candidate(k4, c["P"].astype(np.float64).reshape(-1)[:12].tolist(), c["xyz"].astype(np.float64)[c["tri"][0]].tolist(), 8, 8, None, 0.25) == (True, 0)
    assert w("identical_views")["view"].tolist() == [0] and w("null_map_beside")["view"].tolist() == [1]
    # images
    assert tc.case("gray")["images"][0].ndim == 2 and same_bits(w("gray")["atlas"], w("gray_as_bgr")["atlas"]) and same_bits(w("gray")["view"], w("gray_as_bgr")["view"])
    assert (w("gray")["atlas"][..., 0] == w("gray")["atlas"][..., 2]).all() and w("gray")["n_textured"] > 0
    assert len({im.shape for im in tc.case("four_views")["images"]}) == 4 and len(set(w("four_views")["view"].tolist()) - {-1}) >= 3
    assert w("no_images")["n_textured"] == 0 and w("no_images")["atlas"].any() and (w("no_images")["view"] == -1).all()
    # the mesh
    for name, bad in (("nan_coordinate", np.isnan), ("inf_coordinate", np.isinf)):
        c = tc.case(name)
        v = int(np.argwhere(bad(c["xyz"]).any(axis=1))[0, 0])
        hit = (c["tri"] == v).any(axis=1)
        assert bad(c["xyz"]).sum() == 1 and hit.sum() >= 2 and (w(name)["view"][hit] == -1).all() and (w(name)["view"][~hit] >= 0).any()
    c = tc.case("repeated_index")
    assert c["tri"][3, 0] == c["tri"][3, 2] and w("repeated_index")["view"][3] == -1
    # the fallback: halves go up on both sides of zero, the ends clamp
    a = w("fallback_halves")["atlas"]
    px = lambda t, i, j: a[to.atlas_pixel(t, 4, 1, i, j)[::-1]].tolist()
    assert px(0, 3, 0) == [0, 1, 0] and px(0, 1, 0) == [1, 2, 5] and px(1, 3, 0) == [2, 0, 255] and px(0, 0, 0) == [1, 2, 7]
    assert to.fallback(4, 3, 0, 1, 0, 0) == 0 and to.fallback(4, 3, 0, 3, 0, 0) == 0 and (2 * -1 + 2) // 4 == 0 and (2 * -3 + 2) // 4 == -1
    assert not w("fallback_no_colour")["atlas"].any() and tc.case("no_colour")["bgr"] is None and w("no_colour")["atlas"].any()
    # the gutter
    c = tc.case("texel_clamped")
    A, B, C = c["xyz"].astype(np.float64).tolist()
    p = c["P"].astype(np.float64).reshape(-1).tolist()
    coord, q, u, v = to.texel_coord(k4, p, to.point(4, 0, 3, A, B, C), 8, 8)
    assert u == 8.0 and coord == (16 * 7, 16 * 3) and w("texel_clamped")["view"].tolist() == [0]
    c = tc.case("texel_behind")
    A, B, C = c["xyz"].astype(np.float64).tolist()
    coord, q, u, v = to.texel_coord(k4, p, to.point(4, 3, 0, A, B, C), 8, 8)
    assert coord is None and q[2] == 0.0 and w("texel_behind")["view"].tolist() == [0]
    assert w("texel_behind")["atlas"][0, 3].tolist() == [to.fallback(4, 3, 0, tc.COLOURS[0][k], tc.COLOURS[1][k], tc.COLOURS[2][k]) for k in range(3)]
    assert w("score_null")["score"] is None
    for name in tc.REFUSED:
        assert w(name) is None, name


def test_a_permutation_of_views_permutes_the_labels_only():
    a, b = tc.want("four_views"), tc.want("four_views_permuted")
    c = tc.case("four_views")
    # no ties: every triangle's eligible scores differ
    for t in range(len(c["tri"])):
        scores = [int(to.views_np(c["xyz"], c["tri"][t:t + 1], [c["images"][n]], c["K"], c["P"][n:n + 1], [c["depth_maps"][n]], c["occl_tol"], c["min_area"])[1][0])
                  for n in range(4)]
        top = max(scores)
        assert top == 0 or scores.count(top) == 1, (t, scores)
    assert same_bits(a["atlas"], b["atlas"]) and same_bits(a["score"], b["score"]) and same_bits(a["uv"], b["uv"])
    back = np.asarray(tc.PERMUTATION)                               # new index -> old index
    assert (np.where(b["view"] >= 0, back[np.maximum(b["view"], 0)], -1) == a["view"]).all() and (a["view"] >= 0).sum() > 30


# ---- the layout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 4, 5, 6, 7, 8])
def test_every_texel_has_one_owner_and_a_fetch_stays_in_its_triangle(S):
    nt, B = 7, 2                                                    # an odd count: one half and one block are nobody's
    W, H = to.atlas_size(nt, S, B)
    owner, _, _ = to.ownership(nt, S, B, W, H)
    count = np.zeros((H, W), np.int64)
    for t in range(nt):
        for j in range(S):
            for i in range(S - j):
                X, Y = to.atlas_pixel(t, S, B, i, j)
                count[Y, X] += 1
                assert owner[Y, X] == t
    assert count.max() == 1 and (count == 0).sum() == (owner == -1).sum() == H * W - nt * S * (S + 1) // 2
    uv = to.corner_uv(nt, S, B).astype(np.float64)
    assert (uv % 1.0 == 0.5).all()
    n = 8 * (S - 2)
    for t in range(nt):
        a, b, c = uv[t]
        for p in range(n + 1):
            for q in range(n + 1 - p):                              # the lattice of barycentric steps of 1/8 texel, edges and corners included
                x, y = a + (b - a) * (p / n) + (c - a) * (q / n)
                x0, y0 = int(np.floor(x - 0.5)), int(np.floor(y - 0.5))
                fx, fy = (x - 0.5) - x0, (y - 0.5) - y0
                for dx, dy, wgt in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
                    if wgt > 0.0:
                        assert 0 <= x0 + dx < W and 0 <= y0 + dy < H and owner[y0 + dy, x0 + dx] == t, (S, t, p, q)


# ---- csrc/texture_math.h on the host ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path_factory.mktemp("texture") / "texture_math_host")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sfm-toy-library_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tools", "micro", "texture_math_host.hip")])
    return exe


def hx(v):
    return float(v).hex() if np.isfinite(v) else ("nan" if np.isnan(v) else ("inf" if v > 0 else "-inf"))


def d64(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def f32(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(v)))[0]


def host_input(c, B):
    nv, nt, n = len(c["xyz"]), len(c["tri"]), len(c["images"])
    ch = 1 if n and c["images"][0].ndim == 2 else 3
    K = to.k4_of(c["K"])
    out = ["%d %d %d %d %d %d %d %d" % (nv, nt, n, ch, c["patch"], B, c["min_area"], c["bgr"] is not None),
           " ".join(hx(v) for v in [np.float32(c["occl_tol"])] + K)]
    for v in range(nv):
        col = [0, 0, 0] if c["bgr"] is None else c["bgr"][v].tolist()
        out.append(" ".join(hx(x) for x in c["xyz"][v]) + " %d %d %d" % tuple(col))
    out += ["%d %d %d" % tuple(t) for t in c["tri"].tolist()]
    for i in range(n):
        im, m = c["images"][i], c["depth_maps"][i]
        out.append("%d %d %d" % (im.shape[1], im.shape[0], m is not None))
        out.append(" ".join(hx(v) for v in np.asarray(c["P"], np.float32).reshape(-1, 12)[i]))
        out.append(" ".join(str(v) for v in im.reshape(-1).tolist()))
        if m is not None:
            out.append(" ".join(hx(v) for v in np.asarray(m, np.float32).reshape(-1)))
    return "\n".join(out) + "\n"


def host_lines(c, B):
    """what tools/micro/texture_math_host.hip prints, from the loop statements of the restatement"""
    S, nt = c["patch"], len(c["tri"])
    Bl = B if nt else 1
    W, H = to.atlas_size(nt, S, B)
    k4, tol = to.k4_of(c["K"]), float(np.float32(c["occl_tol"]))
    views = to._views(c["images"], c["P"], c["depth_maps"])
    X = c["xyz"].astype(np.float64)
    uv = to.corner_uv(nt, S, Bl)
    atlas = np.zeros((H, W, 3), np.int64)
    lines = []
    for t, idx in enumerate(c["tri"].tolist()):
        corners = [X[v].tolist() for v in idx]
        view, best = -1, 0
        if len(set(idx)) == 3 and np.isfinite(X[idx]).all():
            for n, (p, w, h, dmap) in enumerate(views):
                for k in range(3):
                    ok, q, u, v, su, sv = to.vertex(k4, p, corners[k], w, h, dmap, tol)
                    lines.append("V %d %d %d %d %s %s %s %s %s %d %d" % (t, n, k, ok, d64(q[0]), d64(q[1]), d64(q[2]), d64(u), d64(v), su, sv))
                cand, a2 = to.candidate(k4, p, corners, w, h, dmap, tol)
                el = to.eligible(cand, a2, c["min_area"])
                lines.append("C %d %d %d %d %d" % (t, n, cand, a2, el))
                if el and -a2 > best:
                    view, best = n, -a2
        lines.append("T %d %d %d " % (t, view, best) + " ".join(f32(v) for v in uv[t].reshape(-1)))
        col = [[0, 0, 0]] * 3 if c["bgr"] is None else [c["bgr"][v].tolist() for v in idx]
        for j in range(S):
            for i in range(S - j):
                fb = [to.fallback(S, i, j, col[0][k], col[1][k], col[2][k]) for k in range(3)]
                out = list(fb)
                if view >= 0:
                    p, w, h, _ = views[view]
                    Xp = to.point(S, i, j, *corners)
                    coord, q, u, v = to.texel_coord(k4, p, Xp, w, h)
                    s12 = [0, 0, 0] if coord is None else [to.sample12(c["images"][view], k, *coord) for k in range(3)]
                    if coord is not None:
                        out = [(s + 8) >> 4 for s in s12]
                    su, sv = coord or (0, 0)
                    lines.append("S %d %d %d %s %s %s %d %s %s %s %s %s %d %d %d %d %d" % (t, i, j, d64(Xp[0]), d64(Xp[1]), d64(Xp[2]), coord is not None,
                                                                                              d64(q[0]), d64(q[1]), d64(q[2]), d64(u), d64(v), su, sv, *s12))
                lines.append("P %d %d %d %d %d %d %d %d %d" % (t, i, j, *out, *fb))
                ax, ay = to.atlas_pixel(t, S, Bl, i, j)
                atlas[ay, ax] = out
    lines.append("A %d %d" % (W, H))
    lines += [" ".join(str(v) for v in row.reshape(-1).tolist()) for row in atlas]
    return lines, atlas


@pytest.mark.parametrize("name", ALL + ["atlas_too_wide", "atlas_too_high"])
def test_host_program_matches_every_intermediate(host_exe, tmp_path, name):
    c = tc.case(name)
    B = to.default_blocks_per_row(len(c["tri"])) if c["blocks_per_row"] is None else c["blocks_per_row"]
    path = tmp_path / "case.txt"
    path.write_text(host_input(c, B))
    r = subprocess.run([host_exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    got = r.stdout.splitlines()
    if tc.want(name) is None:
        assert got == ["refused"]
        return
    lines, atlas = host_lines(c, B)
    assert len(got) == len(lines)
    for g, w in zip(got, lines):
        assert g == w
    assert same_bits(atlas.astype(np.uint8), tc.want(name)["atlas"])
    kinds = {line[0] for line in lines}
    assert kinds >= ({"A"} if not len(c["tri"]) else {"T", "P", "A"})


# ---- the sign, and the quality floor --------------------------------------------------------------------------------------------------
def sphere_mesh_and_views():
    c, m = mc.integration_case("six_view_sphere"), mc.grid_mesh("six_view_sphere")
    return c, m


def sphere_report(c, m, out):
    pairs, changes = to.view_changes(m["tri"], out["view"])
    share = out["n_textured"] / float(len(m["tri"]))
    print("six-view sphere: %d triangles, %.4f textured, %d adjacent pairs, %.4f with different views" % (len(m["tri"]), share, pairs, changes / float(pairs)))
    return share


def test_the_planted_sphere_confirms_the_sign():
    """The mesh of the six-view unit sphere is oriented outwards, towards the cameras, and every direction is within 54.8 degrees of
    one of the six axes while a camera at distance 3 sees the cap up to 70.5 degrees: with a2 < 0 for a triangle that faces the
    camera nearly every triangle finds a view; with the sign the other way round only the limb would (what faces away is hidden
    but for the strip that the tolerance of two voxels lets through)."""
    c, m = sphere_mesh_and_views()
    out = to.texture(m["xyz"], m["bgr"], m["tri"], c["images"], c["K"], c["P"], c["depth_maps"], 2.0 * float(c["voxel"]), 0, 6)
    assert sphere_report(c, m, out) > 0.9                                                    # (min_area 0: at 64 x 64 px most triangles are below half a pixel)
    flipped = to.texture(m["xyz"], m["bgr"], m["tri"][:, [0, 2, 1]], c["images"], c["K"], c["P"], c["depth_maps"], 2.0 * float(c["voxel"]), 0, 6)
    print("flipped: %.4f textured" % (flipped["n_textured"] / float(len(m["tri"]))))       # the limb, which the tolerance of 2 voxels lets through
    assert flipped["n_textured"] < 0.25 * len(m["tri"])


QUALITY_MEASURED = 0.505394      # the mean absolute texel error of the restatement on the plane, in grey levels; the gate is twice this


def test_quality_on_the_plane():
    c = tc.quality_scene()
    out = to.texture(*tc.args(c))
    assert len(c["tri"]) == 128 and out["n_textured"] == 128                                 # the condition: every triangle gets a view
    err = tc.quality_error(c, out)
    print("plane: mean |texel - pattern| %.6f grey levels over the texels with non-negative weights" % err)
    assert err <= 2.0 * QUALITY_MEASURED


# ---- the library ------------------------------------------------------------------------------------------------------------------
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
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    assert callable(capi.mesh_texture) and callable(capi.mesh_texture_size)
    assert capi.lib().sfmba_abi_version() == 6
    for text in ("NO COLOUR ADJUSTMENT ACROSS VIEWS", "NO SMOOTHING OF THE VIEW LABELS", "NO CHART"):
        assert text in header, text


def test_the_size_call_agrees_with_the_restatement():
    import __graft_entry__ as ge
    ge.build_hip()
    from sfm_toy_library_amd import capi
    for nt in (0, 1, 2, 3, 16, 17, 18, 19, 257, 10922, 10923):
        for S in (3, 4, 6, 64):
            for B in (1, 2, 3, 252, 253, 4096, 4097):
                want = to.atlas_size(nt, S, B)
                if want is None:
                    with pytest.raises(capi.SfmbaError):
                        capi.mesh_texture_size(nt, S, B)
                else:
                    assert capi.mesh_texture_size(nt, S, B) == want, (nt, S, B)


def test_refusals_come_before_the_device():
    """The argument checks need no device: each returns SFMBA_ERR_INVALID_ARG (1) and writes nothing.  (The full list, with the refusal
    found on the device, runs with the GPU tests, which share refusal_calls.)"""
    import __graft_entry__ as ge
    ge.build_hip()
    from sfm_toy_library_amd import capi
    import texture_refusals as tr
    calls = tr.refusal_calls(capi)
    assert len(calls) > 45
    for name, call in calls:
        rc, untouched = call()
        assert rc == 1 and untouched, name
