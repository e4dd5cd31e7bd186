"""The scenes of tests/group_cases.py on the CPU alone (no GPU): every scene really has the properties it is there for, shown from
the restatements' answers.  tests/test_gpu_front_end_groups.py runs the scenes through the units at many groupings and holds every
grouping to the same answers; what is asserted here is why a wrong stitching could not compare equal there."""
import numpy as np
import pytest

import group_cases as gc
import jpeg_oracle as jo
import png_oracle as po
import sgm_oracle as so

GRAY_BGR = ("gray", "bgr")
APART = (1, 2, 3, 4)                     # neighbours, and a whole group apart at every SFMBA_GROUP_ITEMS value the GPU tests use


def same(a, b):
    """Two answers (arrays, None, numbers, or tuples / lists / dicts of them) are equal bit for bit."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_items_differ(answers, empty, what):
    """No two items that yield output, neighbours or a whole group apart, have equal answers: a shifted or repeated block shows."""
    n = len(answers)
    assert max(APART) >= max(gc.items_values(n))
    for d in APART:
        for i in range(n - d):
            if not (empty[i] or empty[i + d]):
                assert not same(answers[i], answers[i + d]), (what, i, i + d)


def assert_empties_where_they_belong(empty, what):
    """An item without output first, one inside, and two next to each other that form a group of their own at two items to a group."""
    n = len(empty)
    assert 5 <= n <= 8, what
    assert empty[0] and not empty[1] and not empty[-1], what
    alone = [i for i in range(1, n - 1) if empty[i] and not empty[i - 1] and not empty[i + 1]]
    pairs = [g for g in gc.groups_of(n, 2) if len(g) == 2 and all(empty[i] for i in g)]
    assert alone and pairs, what


# ---- ORB, SURF -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", GRAY_BGR)
@pytest.mark.parametrize("unit", ("orb", "surf"))
def test_extractor_scenes(unit, kind):
    sizes = gc.ORB_SIZES if unit == "orb" else gc.SURF_SIZES
    images = (gc.orb_images if unit == "orb" else gc.surf_images)(kind)
    answers = (gc.orb_answers if unit == "orb" else gc.surf_answers)(kind)
    n_features = (gc.ORB_PARAMS if unit == "orb" else gc.SURF_PARAMS)["n_features"]
    assert [im.shape[:2] for im in images] == [(h, w) for w, h, _, _ in sizes]
    assert all(im.ndim == (3 if kind == "bgr" else 2) for im in images)
    px = [w * h for w, h, _, _ in sizes]
    assert px[-1] == max(px) and px.count(px[-1]) == 1 and len(set(px)) >= 6           # mixed sizes, the largest image last
    empty = [not y for _, _, _, y in sizes]
    assert_empties_where_they_belong(empty, unit)
    for i, (a, e) in enumerate(zip(answers, empty)):
        assert (len(a["kp"]) == 0) == e, (unit, kind, i)
        if e:                                                # too small for any level / octave: not one candidate anywhere
            assert not a["candidates"].any() and len(a["desc"]) == 0
    assert_items_differ(answers, empty, (unit, kind))
    # the quota cut applies: an image has more candidates than it keeps rows
    cut = [i for i, a in enumerate(answers) if int(a["candidates"].sum()) > len(a["kp"]) > 0]
    assert len(cut) >= 2, (unit, kind)
    if unit == "surf":
        assert max(len(a["kp"]) for a in answers) == n_features
    # the images of the calls past the real cap: five distinct ones, one without output
    cap = [images[i] for i in gc.CAP_ITEMS]
    assert len(cap) == 5 and len({im.tobytes() for im in cap}) == 5 and sum(empty[i] for i in gc.CAP_ITEMS) == 1
    ones = (gc.orb_answers if unit == "orb" else gc.surf_answers)(kind, 1)
    assert all(len(a["kp"]) <= 1 for a in ones)
    for a, b in zip(answers, ones):                          # n_features changes the rows that are kept, not the candidates
        assert np.array_equal(a["candidates"], b["candidates"])


# ---- JPEG, PNG, resize -------------------------------------------------------------------------------------------------------------------
def assert_file_scene(answers, resized, what):
    empty = [px is None for _, px in answers]
    n = len(answers)
    assert 5 <= n <= 8
    assert [s == 0 for s, _ in answers] == [not e for e in empty]
    assert not empty[0] and not empty[-1]
    alone = [i for i in range(1, n - 1) if empty[i] and not empty[i - 1] and not empty[i + 1]]
    pairs = [g for g in gc.groups_of(n, 2) if all(empty[i] for i in g)]
    assert alone and pairs, what                             # a refusal inside; two in a row that form a group without a member
    assert_items_differ([px for _, px in answers], empty, what)
    assert_items_differ([px for _, px in resized], empty, (what, "resized"))
    assert [px is None for _, px in resized] == empty
    for (_, a), (_, b) in zip(answers, resized):
        if a is not None:
            assert b.shape[:2] == tuple(jo.resized_size(a.shape[1], a.shape[0], gc.FACTOR))[::-1] and min(b.shape[:2]) >= 1


def test_jpeg_scene():
    answers, resized = gc.jpeg_answers(), gc.jpeg_answers(gc.FACTOR)
    assert_file_scene(answers, resized, "jpeg")
    assert [s for s, _ in answers] == [0, 1, 0, 0, 1, 2, 0, 0]                          # unsupported and corrupt files both occur
    infos = [jo.info(d) for d, (s, _) in zip(gc.jpeg_files(), answers) if s == 0]
    # (status, w, h, channels, h_samp, v_samp, restart interval): gray, 4:4:4, 4:2:2, 4:2:0, and a file with restart markers
    assert {(i[3], i[4], i[5]) for i in infos} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert any(i[6] > 0 for i in infos)


def test_png_scenes():
    kinds = set()
    for scene in gc.PNG_NAMES:
        answers, resized = gc.png_answers(scene), gc.png_answers(scene, gc.FACTOR)
        assert_file_scene(answers, resized, "png " + scene)
        assert {s for s, _ in answers} >= {0, 2}
        for data, (s, _) in zip(gc.png_files(scene), answers):
            if s == 0:
                i = po.info(data)                            # (status, w, h, channels, bit depth, colour type, interlace)
                kinds.add((i[5], i[4]))
    assert 1 in [s for s, _ in gc.png_answers("a")]          # an interlaced file: unsupported
    assert {k[0] for k in kinds} == {0, 2, 3, 4, 6} and {k[1] for k in kinds} == {1, 2, 4, 8, 16}


@pytest.mark.parametrize("channels", (1, 3))
def test_resize_scene(channels):
    images, answers = gc.resize_images(channels), gc.resize_answers(channels)
    assert len(images) == 5 and all(im.ndim == (2 if channels == 1 else 3) for im in images)
    px = [im.shape[0] * im.shape[1] for im in images]
    assert px[-1] == max(px) and len(set(px)) == 5
    assert all(a.size > 0 for a in answers)
    assert_items_differ(answers, [False] * 5, "resize")


# ---- depth -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", GRAY_BGR)
def test_depth_scene(kind):
    b = gc.depth_scene(kind)
    jobs, n = b["jobs"], len(b["jobs"])
    assert n == 7 and len(b["images"]) == 6 and len({im.shape for im in b["images"]}) == 2
    assert gc.items_values(n) == (2, 3)
    if kind == "bgr":
        assert all(im.ndim == 3 for im in b["images"])
        assert any((g != c[:, :, 0]).any() for g, c in zip(b["gray"], b["images"]))
        assert any((g != h).any() for g, h in zip(b["gray"], gc.depth_scene("gray")["images"]))
    named = [set(gc.depth_images_of(j)) for j in jobs]
    groups = gc.groups_of(n, 2)
    in_group = [set().union(*(named[j] for j in g)) for g in groups]
    # an image is the reference of a job in one group and a source of a job in the next
    assert any(jobs[j][0] in jobs[k][1] for g, h in zip(groups, groups[1:]) for j in g for k in h)
    # the second job of a group names only images that no job before it names
    assert any(len(g) == 2 and not (named[g[1]] & set().union(*named[:g[1]])) for g in groups[1:])
    # one image is named by jobs of three groups (or more)
    assert max(sum(i in s for s in in_group) for i in range(len(b["images"]))) >= 3
    sweep, vols = gc.depth_answers(kind), gc.volume_answers(kind)
    for j in range(n):
        assert (sweep[j][0] > 0).sum() > 100 and (vols[j][0] != so.SENTINEL).any(), j
    assert_items_differ(sweep, [False] * n, ("sweep", kind))
    assert_items_differ([v[0] for v in vols], [False] * n, ("volume", kind))
    for sgm in (so.DEFAULTS, dict(p1=0, p2=1023, n_paths=4, invalid_cost=0, uniqueness=0)):
        maps = gc.sgm_answers(kind, tuple(sorted(sgm.items())))
        assert_items_differ(maps, [False] * n, ("sgm", kind))
        assert all((m[2] >= 0).all() for m in maps)
    # the five jobs of depth_cases.batch() are the head of the extended list, over the same images
    plain = gc.dc.batch()
    assert plain["jobs"] == jobs[:5] and all(np.array_equal(a, c) for a, c in zip(plain["images"], gc.depth_scene("gray")["images"]))


# ---- flow --------------------------------------------------------------------------------------------------------------------------------
def test_flow_scene():
    c = gc.flow_scene()
    pairs, points, n = c["pairs"], c["points"], len(c["pairs"])
    assert n == 6 and len(c["images"]) == 4 and len({im.shape for im in c["images"]}) == 2
    assert gc.items_values(n) == (2, 3, 4)                   # 2 and 3 both divide 6: 4 is the value that does not
    assert (0, 1) in pairs and (1, 0) in pairs and pairs.count((0, 1)) == 2
    empty = [len(p) == 0 for p in points]
    starts = [g[0] for g in gc.groups_of(n, 2)]
    assert any(empty[i] and i not in starts and 0 < i < n - 1 for i in range(n))        # a pair without points inside a group ...
    assert any(empty[i] and i in starts and i > 0 for i in range(n))                    # ... and one that starts a group
    groups = gc.groups_of(n, 2)
    seen = [set(v for p in g for v in pairs[p]) for g in groups]
    last = set(pairs[-1])
    assert last <= set().union(*seen[:-1]) and not last <= seen[0]       # both images of the last pair were uploaded by earlier groups
    assert set(v for p in pairs for v in p) == {0, 1, 2, 3}   # every image has its pyramid in dbg_pyramid
    per_pair, levels = gc.flow_answers()
    for p in range(n):
        assert (len(per_pair[p][0]) == 0) == empty[p]
        assert [len(a) for a in per_pair[p]] == [len(points[p])] * 5
    assert sum(int(a[1].sum()) for a in per_pair) >= 10      # points are tracked, not all lost
    assert_items_differ(per_pair, empty, "flow")
    assert all(lv is not None and len(lv) == c["params"]["n_levels"] for lv in levels)
    assert_items_differ(levels, [False] * 4, "flow pyramids")


# ---- the matchers --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("hamming", "l2"))
def test_match_pair_lists_straddle_the_batches(kind):
    tile, bt = gc.match_constants(kind)[:2]
    assert (tile, bt) == ((512, 512) if kind == "hamming" else (512, 256))
    sets = gc.match_sets(kind)
    assert [len(s) for s in sets] == [3, 17, 40, 29, 300, 2 * tile + 1]
    pairs = gc.match_pairs(kind)
    assert len(pairs) == 2 * bt and pairs[bt - 1] == (5, 2)
    plan = gc.match_plan(kind, pairs)
    assert [t for t, _ in plan] == [bt, bt, 2]               # the three tiles of (5, 2) are the last of batch 0 and the first two of batch 1
    assert plan[0][1] == 1 and plan[-1][1] == 2               # the first and the last batch differ in their train slices
    assert [t for t, _ in gc.match_plan(kind, gc.match_pairs(kind, "exact"))] == [bt]
    assert [t for t, _ in gc.match_plan(kind, gc.match_pairs(kind, "plus_one"))] == [bt, 1]
    distinct = sorted(set(pairs))
    assert len(distinct) <= 20
    kept = {p: gc.match_answer(kind, *p) for p in distinct}
    assert all(len(v) > 0 for v in kept.values())            # every pair keeps matches ...
    assert any(len(v) < len(sets[p[0]]) for p, v in kept.items())                       # ... and the ratio test drops some
    for a, b in zip(pairs, pairs[1:]):                        # neighbours differ, so do the pairs on either side of every boundary
        assert a != b and kept[a] != kept[b]
    for edge in (bt, 2 * bt):
        assert kept[pairs[edge - 2]] != kept[pairs[min(edge, len(pairs) - 1)]]
