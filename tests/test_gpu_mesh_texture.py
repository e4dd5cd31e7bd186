"""Texturing a mesh on the MI355X (-m gpu) against the CPU restatement of its contract (tests/texture_oracle.py; include/sfmba.h,
sfmba_mesh_texture).  Every comparison is EXACT: the bytes of the atlas, the bit patterns of uv, the labels, the scores and the count.
The shapes are those of tests/texture_cases.py -- the smallest at which the kernels can still go wrong -- and the restatement's answer
for each is computed once and shared."""
import numpy as np
import pytest

import mesh_cases as mc
import texture_cases as tc
import texture_oracle as to
import texture_refusals as tr

pytestmark = pytest.mark.gpu
SFMBA_OK, SFMBA_ERR_INVALID_ARG = 0, 1
FIELDS = ("atlas", "uv", "view", "score")
QUALITY_MEASURED = 0.505394      # as tests/test_texture_oracle_cpu.py measured it on the restatement; the gate is twice this


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi as c
    assert c.device_count() >= 1
    return c


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same(got, want, what=""):
    for f in FIELDS:
        assert same_bits(got[f], want[f]), (what, f)
    assert got["n_textured"] == want["n_textured"], what


def textured(capi, c):
    return capi.mesh_texture(*tc.args(c))


@pytest.mark.parametrize("name", list(tc.CASES))
def test_cases_exact(capi, name):
    c, want = tc.case(name), tc.want(name)
    got = textured(capi, c)
    assert_same(got, want, name)
    B = to.default_blocks_per_row(len(c["tri"])) if c["blocks_per_row"] is None else c["blocks_per_row"]
    assert capi.mesh_texture_size(len(c["tri"]), c["patch"], B) == got["atlas"].shape[1::-1] == to.atlas_size(len(c["tri"]), c["patch"], B)


@pytest.mark.parametrize("name", list(tc.REFUSED))
def test_refused_cases_refuse(capi, name):
    assert tc.want(name) is None
    with pytest.raises(capi.SfmbaError):
        textured(capi, tc.case(name))


def test_the_device_mesh_of_the_six_view_sphere_textures_as_the_restatement_says(capi):
    c = mc.integration_case("six_view_sphere")
    m = capi.tsdf_mesh(c["images"], c["K"], c["P"], c["depth_maps"], c["origin"], c["voxel"], c["dims"], c["trunc"])
    assert len(m["tri"]) > 10000
    for min_area in (256, 0):                                                           # the host's rule, and every triangle with an area
        args = (m["xyz"], m["bgr"], m["tri"], c["images"], c["K"], c["P"], c["depth_maps"], 2.0 * float(c["voxel"]), min_area, 6)
        want = to.texture(*args)
        got = capi.mesh_texture(*args)
        assert_same(got, want, min_area)
        pairs, changes = to.view_changes(m["tri"], got["view"])
        print("six-view sphere, min_area %d: %d triangles, %.4f textured, %d adjacent pairs, %.4f with different views (reported, not gated)" %
              (min_area, len(m["tri"]), got["n_textured"] / float(len(m["tri"])), pairs, changes / float(pairs)))


def test_quality_on_the_plane(capi):
    """The plane at depth 10 under two views at +-15 degrees (tests/texture_cases.py).  MEASURED ONCE on the restatement (and written
    to profiles/mesh_texture.txt): the mean absolute difference between the texels with non-negative weights and the pattern at their
    own point is 0.505394 grey levels.  Asserted: at most twice that (one level of headroom covers the 1/16 px snap and the two
    roundings), and every triangle has a view."""
    c = tc.quality_scene()
    got = textured(capi, c)
    assert got["n_textured"] == 128
    err = tc.quality_error(c, got)
    print("plane on the device: mean |texel - pattern| %.6f grey levels" % err)
    assert err <= 2.0 * QUALITY_MEASURED
    assert_same(got, to.texture(*tc.args(c)), "quality")


def test_score_may_be_null(capi):
    a = tr.valid("sfmba_mesh_texture")
    a.update(score=None)
    rc, _ = tr.invoke(capi.lib(), "sfmba_mesh_texture", a)
    assert rc == SFMBA_OK and same_bits(a["view"], tc.want("four_views")["view"]) and same_bits(a["atlas"], tc.want("four_views")["atlas"])


def test_every_refusal_writes_nothing(capi):
    calls = tr.refusal_calls(capi, device_cases=True)
    assert len(calls) > 48
    for name, call in calls:
        rc, untouched = call()
        assert rc == SFMBA_ERR_INVALID_ARG and untouched, name
    assert "index" in capi.lib().sfmba_last_error().decode()


@pytest.mark.parametrize("entry", list(tr.NAMES))
def test_the_valid_call_of_the_refusal_table_succeeds(capi, entry):
    rc, untouched = tr.valid_call(capi, entry)
    assert rc == SFMBA_OK and not untouched
    if entry == "sfmba_mesh_texture":
        a = tr.valid(entry)
        tr.invoke(capi.lib(), entry, a)
        want = tc.want("four_views")
        assert same_bits(a["atlas"], want["atlas"]) and same_bits(a["uv"], want["uv"]) and same_bits(a["score"], want["score"])
        assert int(a["n_textured"][0]) == want["n_textured"]


def test_two_calls_on_one_process_give_the_bits_of_each_alone(capi):
    """The arena hands a call the chunks of the call before it: nothing of one atlas may leak into the next."""
    for first, second in (("one_column_S64", "blocks_9_odd"), ("nt_257", "nt_0"), ("four_views", "no_images")):
        textured(capi, tc.case(first))
        assert_same(textured(capi, tc.case(second)), tc.want(second), (first, second))
