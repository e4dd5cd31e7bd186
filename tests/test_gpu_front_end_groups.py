"""The multi-group paths of the front-end units on the MI355X (-m gpu), held to the one-group result.

ORB, SURF, the JPEG and PNG readers, the resize, the three sweep entry points and the tracker cut a call into consecutive groups (a
scratch budget and a cap on the items of a group) and stitch the outputs.  SFMBA_GROUP_BYTES and SFMBA_GROUP_ITEMS
(csrc/unit_common.h) lower both limits, so the scenes of tests/group_cases.py -- 5 to 8 small items each -- run as 1, 2, 3 ... n groups.
The number of groups of a call is read from the `groups N` field of the unit's timing line.  Under EVERY setting the outputs are
byte-equal to the call without the variables, and that call equals the CPU restatement: nothing here is a tolerance.

The last section runs the real limits without the hook (and with huge values in it, which must change nothing: the hook never raises
a limit): 1025 images through ORB and SURF (grid.y 1024, ten image bits in the sort), and pair lists of three batches through the two
matchers.  The constants come from the headers."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import group_cases as gc
import sgm_cases as sgc
from test_gpu_depth_sgm import SGM_SETS
from test_gpu_orb_extract import raw_call as orb_raw
from test_gpu_surf_extract import raw_call as surf_raw

pytestmark = pytest.mark.gpu
SFMBA_ERR_CAPACITY = 5
VARS = ("SFMBA_GROUP_ITEMS", "SFMBA_GROUP_BYTES")
LADDER = [1 << e for e in range(10, 29)]
MALFORMED = ("0", "-3", "x", "")


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


# ---- comparing --------------------------------------------------------------------------------------------------------------------------
def blob(x):
    """Everything a call returned, as one hashable value: equal blobs are equal outputs, byte for byte."""
    if isinstance(x, dict):
        return tuple((k, blob(x[k])) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return tuple(blob(v) for v in x)
    if x is None or isinstance(x, (int, str)):
        return x
    a = np.ascontiguousarray(x)
    return (str(a.dtype), a.shape, a.tobytes())


def assert_is(got, want, what):
    """got equals the restatement's want: the same nesting, every array the same shape and the same values -- floats and records by
    their bytes, integers by value (the restatement does not always use the ABI's integer width)."""
    if isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            assert_is(g, w, what + (i,))
    elif want is None or isinstance(want, int):
        assert got == want, what
    else:
        g, w = np.asarray(got), np.asarray(want)
        assert g.shape == w.shape, (what, g.shape, w.shape)
        if w.dtype.kind in "fV":
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), what
        else:
            assert g.dtype.kind in "iu" and np.array_equal(g, w), what


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
class Scene:
    """A call of a unit over a scene of group_cases: call(capi) -> its outputs, want() -> the restatement's, in the same nesting.
    n items; live[i]: item i can put its group on the count of the timing line (the readers do not count a group without a member)."""

    def __init__(self, name, tag, switch, n, call, want, live=None):
        self.name, self.tag, self.switch, self.n, self.call, self.want = name, tag, switch, n, call, want
        self.live = [True] * n if live is None else live

    def groups_at(self, k):
        """The count of the timing line when k items go to a group."""
        return sum(any(self.live[i] for i in g) for g in gc.groups_of(self.n, k))

    def __repr__(self):
        return self.name


def _extractor(unit, kind):
    images = (gc.orb_images if unit == "orb" else gc.surf_images)(kind)
    params = gc.ORB_PARAMS if unit == "orb" else gc.SURF_PARAMS
    fields = ("kp", "desc", "level_xy", "bin", "harris", "candidates") if unit == "orb" else ("kp", "desc", "bin", "moments", "sums", "candidates")
    call = lambda capi: (capi.orb_extract if unit == "orb" else capi.surf_extract)(list(images), debug=True, **params)
    want = lambda: [tuple(a[f] for f in fields) for a in (gc.orb_answers if unit == "orb" else gc.surf_answers)(kind)]
    return Scene("%s_%s" % (unit, kind), unit, "SFMBA_%s_TIMING" % unit.upper(), len(images), call, want)


def _reader(unit, scene, factor):
    files = gc.jpeg_files() if unit == "jpeg" else gc.png_files(scene)
    answers = (lambda: gc.jpeg_answers(factor)) if unit == "jpeg" else (lambda: gc.png_answers(scene, factor))

    def call(capi):
        infos, images = (capi.jpeg_decode if unit == "jpeg" else capi.png_decode)(list(files), factor=factor)
        return [i["status"] for i in infos], images, [tuple(sorted(i.items())) for i in infos]
    want = lambda: ([s for s, _ in answers()], [px for _, px in answers()])
    live = [s == 0 for s, _ in answers()]
    name = "%s%s_factor_%s" % (unit, "_" + scene if scene else "", factor)
    return Scene(name, unit + "_decode", "SFMBA_%s_TIMING" % unit.upper(), len(files), call, want, live)


def _resize(channels):
    images = gc.resize_images(channels)
    return Scene("resize_%dch" % channels, "resize_images", "SFMBA_JPEG_TIMING", len(images),
                 lambda capi: capi.resize_images(list(images), gc.FACTOR), lambda: gc.resize_answers(channels))


def _depth(entry, kind, want_plane=True, sgm=None):
    b = gc.depth_scene(kind)
    args = (b["images"], b["K"], b["P"], b["jobs"])
    strip = lambda maps: [(d, s, p if want_plane else None) for d, s, p in maps]
    if entry == "depth_sweep":
        call = lambda capi: capi.depth_sweep(*args, want_plane=want_plane, **b["params"])
        want = lambda: strip(gc.depth_answers(kind))
    elif entry == "depth_cost_volume":
        call = lambda capi: capi.depth_cost_volume(*args, **sgc.sweep_params(b))
        want = lambda: [v for v, _, _ in gc.volume_answers(kind)]
    else:
        sgm = dict(gc.so.DEFAULTS) if sgm is None else sgm
        call = lambda capi: capi.depth_sweep_sgm(*args, want_plane=want_plane, **sgc.sweep_params(b, **sgm))
        want = lambda: strip(gc.sgm_answers(kind, tuple(sorted(sgm.items()))))
    name = "%s_%s%s" % (entry, kind, "" if want_plane else "_no_plane")
    return Scene(name, entry, "SFMBA_DEPTH_TIMING", len(b["jobs"]), call, want)


def _flow():
    c = gc.flow_scene()
    call = lambda capi: capi.flow_track(c["images"], c["pairs"], c["points"], debug=True, **c["params"])
    return Scene("flow_track", "flow_track", "SFMBA_FLOW_TIMING", len(c["pairs"]), call, lambda: gc.flow_answers())


SCENES = ([_extractor(u, k) for u in ("orb", "surf") for k in ("gray", "bgr")] +
          [_reader("jpeg", None, f) for f in (1.0, gc.FACTOR)] + [_reader("png", s, f) for s in gc.PNG_NAMES for f in (1.0, gc.FACTOR)] +
          [_resize(ch) for ch in (1, 3)] +
          [_depth("depth_sweep", k, wp) for k in ("gray", "bgr") for wp in (True, False)] +
          [_depth("depth_cost_volume", k) for k in ("gray", "bgr")] +
          [_depth("depth_sweep_sgm", k, wp) for k in ("gray", "bgr") for wp in (True, False)] +
          [_flow()])


def run(scene, capi, monkeypatch, capfd, items=None, nbytes=None, timing=True):
    """One call of the scene with the two variables set as given (None: unset): (outputs, the group count of its timing line)."""
    for var, value in zip(VARS, (items, nbytes)):
        if value is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(value))
    if timing:
        monkeypatch.setenv(scene.switch, "1")
    else:
        monkeypatch.delenv(scene.switch, raising=False)
    capfd.readouterr()
    out = scene.call(capi)
    counts = re.findall(r"^\[sfmba %s\] .*\b(?:groups|batches) (\d+)\b" % re.escape(scene.tag), capfd.readouterr().err, re.M)
    assert bool(counts) == timing, (scene, counts)
    return out, (int(counts[-1]) if timing else None)


def report(capfd, scene, steps):
    with capfd.disabled():
        print("\nGROUPS %s n=%d: %s" % (scene.name, scene.n, " ".join("%s=%s" % kv for kv in steps)))


# ---- the ladder ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", SCENES, ids=repr)
def test_every_grouping_gives_the_one_group_result(capi, monkeypatch, capfd, scene):
    steps = []

    def at(label, want_groups=None, **env):
        out, groups = run(scene, capi, monkeypatch, capfd, **env)
        steps.append((label, groups))
        if want_groups is not None:
            assert groups == want_groups, (scene, label, groups, want_groups)
        assert blob(out) == one, (scene, label, "differs from the one-group result")
        return groups

    # 1. both variables unset: one group, and the restatement bit for bit
    first, groups = run(scene, capi, monkeypatch, capfd)
    assert groups == 1, (scene, groups)
    want = scene.want()
    assert_is(first[:len(want)] if isinstance(want, tuple) else first, want, (scene.name,))
    one = blob(first)
    steps.append(("unset", groups))
    assert blob(run(scene, capi, monkeypatch, capfd, timing=False)[0]) == one           # the timing switch changes no output
    # 2., 3. the cap on the items of a group
    n_alone = scene.groups_at(1)
    assert 4 <= n_alone <= scene.n
    at("items_1", n_alone, items=1)
    ks = gc.items_values(scene.n)
    assert any(scene.n % k for k in ks)
    for k in ks:
        assert scene.groups_at(k) <= math.ceil(scene.n / k)
        at("items_%d" % k, scene.groups_at(k), items=k)
    at("items_%d" % scene.n, 1, items=scene.n)
    # 4., 5. the scratch budget: every item alone at one byte, then ever fewer groups; some step lies strictly between
    at("bytes_1", n_alone, nbytes=1)
    ladder = [at("bytes_2^%d" % int(math.log2(b)), nbytes=b) for b in LADDER]
    assert all(a >= b for a, b in zip(ladder, ladder[1:])), (scene, ladder)
    assert ladder[0] <= n_alone and ladder[-1] == 1, (scene, ladder)
    between = [b for b, g in zip(LADDER, ladder) if 1 < g < n_alone]
    assert between, (scene, ladder)
    # 6. both together: the finer partition holds
    at("items_2+bytes_2^28", scene.groups_at(2), items=2, nbytes=LADDER[-1])
    at("items_%d+bytes_1" % scene.n, n_alone, items=scene.n, nbytes=1)
    mid = ladder[LADDER.index(between[0])]
    both = at("items_2+bytes_2^%d" % int(math.log2(between[0])), items=2, nbytes=between[0])
    assert both <= n_alone
    if all(scene.live):                                        # a partition that meets both limits has no fewer groups than the best for either
        assert both >= max(mid, scene.groups_at(2)), (scene, both, mid)
    # 7. a malformed value is no value
    for bad in MALFORMED:
        at("items_%r" % bad, 1, items=bad)
        at("bytes_%r" % bad, 1, nbytes=bad)
    at("items_2_again", scene.groups_at(2), items=2)           # the arenas of the groups before went back to the cache and come out again
    at("items_2_once_more", scene.groups_at(2), items=2)
    at("unset_after", 1)                                       # a one-group call right behind a multi-group call
    report(capfd, scene, steps)


# ---- the capacity protocol at two items to a group ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", ("orb", "surf"))
def test_extractor_capacity_protocol_across_groups(capi, monkeypatch, unit):
    images = (gc.orb_images if unit == "orb" else gc.surf_images)("gray")
    answers = (gc.orb_answers if unit == "orb" else gc.surf_answers)("gray")
    params = gc.ORB_PARAMS if unit == "orb" else gc.SURF_PARAMS
    raw = orb_raw if unit == "orb" else surf_raw
    ptr = np.concatenate([[0], np.cumsum([len(a["kp"]) for a in answers])]).tolist()
    n = ptr[-1]
    monkeypatch.setenv("SFMBA_GROUP_ITEMS", "2")
    rc, kp_ptr, total, kp, desc = raw(capi, list(images), cap=n - 1, **params)
    assert rc == SFMBA_ERR_CAPACITY and total == n and kp_ptr.tolist() == ptr
    assert (desc.view(np.uint8) == 0x55).all() and (kp.view(np.uint8) == 0x55).all()           # nothing else is written
    rc, kp_ptr, total, kp, desc = raw(capi, list(images), cap=n, **params)
    assert rc == 0 and total == n and kp_ptr.tolist() == ptr
    assert kp[:n].tobytes() == np.concatenate([a["kp"] for a in answers]).tobytes()
    want = np.concatenate([a["desc"] for a in answers])
    assert desc.reshape(len(desc), -1).view(want.dtype)[:n].tobytes() == want.tobytes()
    monkeypatch.delenv("SFMBA_GROUP_ITEMS")
    rc, kp_ptr, total, kp1, desc1 = raw(capi, list(images), cap=n, **params)
    assert rc == 0 and kp1.tobytes() == kp.tobytes() and desc1.tobytes() == desc.tobytes()


@pytest.mark.parametrize("unit,scene", [("jpeg", None), ("png", "a"), ("png", "b")])
def test_reader_capacity_protocol_across_groups(capi, monkeypatch, unit, scene):
    files = gc.jpeg_files() if unit == "jpeg" else gc.png_files(scene)
    answers = gc.jpeg_answers() if unit == "jpeg" else gc.png_answers(scene)
    ptr = np.concatenate([[0], np.cumsum([0 if px is None else px.size for _, px in answers])]).tolist()
    need, n = ptr[-1], len(files)
    fptr, flat = capi._flat_files(list(files))
    lp, bp = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)
    fn = capi.lib().sfmba_jpeg_decode if unit == "jpeg" else capi.lib().sfmba_png_decode

    def raw(cap):
        info = ((capi._ImageInfo if unit == "jpeg" else capi._PngInfo) * n)()
        out_ptr, total, out = np.full(n + 1, -7, np.int64), C.c_int64(-7), np.full(need, 0xAB, np.uint8)
        rc = fn(C.c_int(0), C.c_int(n), fptr.ctypes.data_as(lp), flat.ctypes.data_as(bp), C.c_float(1.0), info, out_ptr.ctypes.data_as(lp),
                out.ctypes.data_as(bp), C.c_int64(cap), C.byref(total))
        return rc, [i.status for i in info], out_ptr.tolist(), total.value, out
    monkeypatch.setenv("SFMBA_GROUP_ITEMS", "2")
    rc, status, out_ptr, total, out = raw(need - 1)
    assert rc == SFMBA_ERR_CAPACITY and total == need and out_ptr == ptr and status == [s for s, _ in answers]
    assert (out == 0xAB).all()                                                             # nothing else is written
    rc, status, out_ptr, total, out = raw(need)
    assert rc == 0 and total == need and out_ptr == ptr and status == [s for s, _ in answers]
    assert out.tobytes() == b"".join(px.tobytes() for _, px in answers if px is not None)
    monkeypatch.delenv("SFMBA_GROUP_ITEMS")
    assert raw(need)[4].tobytes() == out.tobytes()


# ---- the volume and the SGM maps across groups ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("gray", "bgr"))
def test_volume_and_sgm_maps_of_a_multi_group_call(capi, monkeypatch, capfd, kind):
    b = gc.depth_scene(kind)
    args = (b["images"], b["K"], b["P"])
    p = sgc.sweep_params(b)
    monkeypatch.setenv("SFMBA_GROUP_ITEMS", "2")
    monkeypatch.setenv("SFMBA_DEPTH_TIMING", "1")
    capfd.readouterr()
    vols = capi.depth_cost_volume(*args, b["jobs"], **p)
    assert re.findall(r"\[sfmba depth_cost_volume\] .* groups (\d+)", capfd.readouterr().err) == ["4"]
    monkeypatch.delenv("SFMBA_DEPTH_TIMING")
    planes = [gc.do.planes(job[2], job[3], p["n_planes"]) for job in b["jobs"]]
    for j, job in enumerate(b["jobs"]):                        # job j of the call of four groups equals the call of job j alone
        alone = capi.depth_cost_volume(*args, [job], **p)[0]
        assert alone.tobytes() == vols[j].tobytes() and alone.shape == vols[j].shape, j
    for sgm in SGM_SETS:
        agg = {k: v for k, v in sgm.items() if k != "uniqueness"}
        got = capi.depth_sweep_sgm(*args, b["jobs"], **dict(p, **sgm))
        for j in range(len(b["jobs"])):
            wf, step = planes[j]
            assert_is(got[j], gc.so.maps_of(vols[j], gc.so.sgm_aggregate(vols[j], **agg), wf, step, sgm["uniqueness"]), (kind, j, "maps of the device's volume"))
        assert_is(got, gc.sgm_answers(kind, tuple(sorted(sgm.items()))), (kind, "restatement"))


# ---- the real caps, without the hook -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hook", ("unset", "huge"))
@pytest.mark.parametrize("n_features", ("scene", 1))
@pytest.mark.parametrize("unit", ("orb", "surf"))
def test_extractors_past_the_image_cap(capi, monkeypatch, capfd, unit, n_features, hook):
    for var, huge in zip(VARS, (100000, 1 << 62)):             # the hook can lower a limit and never raise it: huge values change nothing
        if hook == "unset":
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(huge))
    cap = gc.header_int("%s_extract.h" % unit, "%s_MAX_GROUP_IMAGES" % unit.upper())
    assert cap == 1024 and cap % len(gc.CAP_ITEMS) != 0
    params = dict(gc.ORB_PARAMS if unit == "orb" else gc.SURF_PARAMS)
    if n_features != "scene":
        params["n_features"] = n_features
    images = (gc.orb_images if unit == "orb" else gc.surf_images)("gray")
    answers = (gc.orb_answers if unit == "orb" else gc.surf_answers)("gray", params["n_features"])
    fields = ("kp", "desc", "level_xy", "bin", "harris", "candidates") if unit == "orb" else ("kp", "desc", "bin", "moments", "sums", "candidates")
    order = [gc.CAP_ITEMS[i % len(gc.CAP_ITEMS)] for i in range(cap + 1)]
    monkeypatch.setenv("SFMBA_%s_TIMING" % unit.upper(), "1")
    capfd.readouterr()
    got = (capi.orb_extract if unit == "orb" else capi.surf_extract)([images[i] for i in order], debug=True, **params)
    groups = re.findall(r"\[sfmba %s\] .* groups (\d+)" % unit, capfd.readouterr().err)
    assert groups == ["2"], groups                              # 1024 images, then one
    with capfd.disabled():
        print("\nGROUPS %s_past_the_cap n_features=%s images=%d hook=%s: groups=%s" % (unit, params["n_features"], len(order), hook, groups[0]))
    assert len(got) == cap + 1
    for i, item in enumerate(order):
        assert_is(got[i], tuple(answers[item][f] for f in fields), (unit, "image", i))


@pytest.mark.parametrize("kind", ("hamming", "l2"))
def test_matchers_past_the_batch_size(capi, monkeypatch, capfd, kind):
    tile, bt = gc.match_constants(kind)[:2]
    sets = gc.match_sets(kind)
    call = capi.match_features if kind == "hamming" else capi.match_features_l2
    tag = "match" if kind == "hamming" else "match_l2"
    monkeypatch.setenv("SFMBA_MATCH_TIMING", "1")

    def rows(res, p):
        ptr = res[2]
        a, b = int(ptr[p]), int(ptr[p + 1])
        d = res[5][a:b]
        return list(zip(res[3][a:b].tolist(), res[4][a:b].tolist(), (d if kind == "hamming" else d.view(np.uint32)).tolist()))

    for shape, want_batches in (("three_batches", 3), ("exact", 1), ("plus_one", 2)):
        pairs = gc.match_pairs(kind, shape)
        assert len(gc.match_plan(kind, pairs)) == want_batches
        capfd.readouterr()
        res = call(list(sets), pairs)
        batches = re.findall(r"\[sfmba %s\] .* batches (\d+)" % tag, capfd.readouterr().err)
        assert batches == [str(want_batches)], (shape, batches)
        with capfd.disabled():
            print("\nGROUPS %s_%s pairs=%d: batches=%s plan=%s" % (tag, shape, len(pairs), batches[0], gc.match_plan(kind, pairs)))
        assert res[0].tolist() == [l for l, r in pairs] and res[1].tolist() == [r for l, r in pairs]
        for p, (l, r) in enumerate(pairs):                     # every pair against the restatement (one answer per distinct pair)
            assert rows(res, p) == [(q, j, d) for q, j, d in gc.match_answer(kind, l, r)], (shape, p, (l, r))
        if shape != "three_batches":
            continue
        # single calls of pairs on both sides of each boundary: the tiles of pair bt - 1 are the items bt - 1 .. bt + 1, batch 2 starts at pair 2 bt - 2
        for p in (0, bt - 3, bt - 2, bt - 1, bt, bt + 1, 2 * bt - 4, 2 * bt - 3, 2 * bt - 2, 2 * bt - 1):
            alone = call(list(sets), [pairs[p]])
            a, b = int(res[2][p]), int(res[2][p + 1])
            for f in (3, 4, 5):
                assert alone[f].tobytes() == res[f][a:b].tobytes(), (p, f)
