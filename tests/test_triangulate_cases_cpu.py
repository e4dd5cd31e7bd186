"""The geometries of tests/triangulate_cases.py on the two CPU references alone (no GPU): the long-double Jacobi reference of that
module against oracle/triangulate_oracle.py (LAPACK SVD in fp64), and every condition the GPU test relies on.

ULP_BOUND = 4 float ulps per coordinate is the bound tests/test_gpu_triangulate.py holds the device to: the float-rounded h_i and w
of two correct computations may each differ by one rounding, and an ulp spans a factor of 2 in relative size.  Two CPU references
further apart than 2 ulps on a conditioned match would mean that the conditioning rule, not the device, decides the GPU test.
Measured: 0 ulps on every case but `far` (2)."""
import json
import os

import numpy as np
import pytest

import triangulate_cases as tc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_kat.json")
ULP_BOUND = 4.0


@pytest.fixture(scope="module")
def refs():
    """name -> (case, reference at 10 px): computed once, never modified."""
    out = {}
    for name in tc.CASES:
        c = tc.make_case(name)
        out[name] = (c, tc.reference(c["K"], c["P_left"], c["P_right"], c["left"], c["right"], 10.0))
    return out


def test_every_case_has_a_partial_last_block(refs):
    for name, (c, ref) in refs.items():
        assert len(c["left"]) == len(c["right"]) == tc.N == 4159 and tc.N % 256 == 63
        assert c["left"].dtype == c["right"].dtype == c["P_left"].dtype == c["K"].dtype == np.float32
        assert np.all(np.isfinite(c["left"])) and np.all(np.isfinite(c["right"]))
    g = refs["general"][0]
    assert np.abs(g["P_left"][:, :3] - np.eye(3)).max() > 0.1 and np.abs(g["P_left"][:, 3]).max() > 10     # neither P is [I|0]
    assert np.abs(refs["general_far_origin"][0]["P_right"][:, 3]).max() > 50 * np.abs(g["P_right"][:, 3]).max()
    b = refs["behind"][0]
    depth_right = b["X"] @ b["P_right"][:, :3].astype(np.float64).T[:, 2] + float(b["P_right"][2, 3])
    assert np.all(depth_right < 0)


@pytest.mark.parametrize("name", tc.CASES)
def test_the_two_references_agree(refs, name):
    from oracle import triangulate_oracle as tri
    c, ref = refs[name]
    X_o, keep_o, el_o, er_o = tri.triangulate_views(c["K"], c["P_left"], c["P_right"], c["left"], c["right"])
    cond = tc.conditioned(ref)
    left_out = 1.0 - cond.mean()
    ulps = tc.ulp_distance(X_o, ref["points3d"])[cond]
    print("%s: left out %.4f, worst distance %.1f ulps, %d sweeps, %d kept" % (name, left_out, ulps.max(), ref["sweeps"], ref["keep"].sum()))
    assert left_out <= tc.MAX_LEFT_OUT
    assert ulps.max() <= 2.0, "the two CPU references differ by more than 2 ulps: find out why before trusting the GPU bound"
    assert ulps.max() <= ULP_BOUND
    # singular values: descending, none negative
    A_sigma = ref["sigma"]
    assert np.all(np.diff(A_sigma, axis=1) <= 0) and np.all(A_sigma[:, 3] >= 0)
    # same decisions wherever the two references have the same point
    same = np.all(X_o == ref["points3d"], axis=1) | np.all(np.isnan(X_o) & np.isnan(ref["points3d"]), axis=1)
    assert np.array_equal(keep_o[same], ref["keep"][same])


@pytest.mark.parametrize("name", tc.CASES)
def test_both_keep_values_occur_and_errors_are_finite(refs, name):
    c, ref = refs[name]
    w = ref["Xh"][:, 3]
    if name == "pure_rotation":
        # Both cameras stand at the origin, so the fourth column of the DLT matrix is exactly zero whatever the pixels are: the null
        # vector is the common centre (0, 0, 0, +-1) itself, the point 0 / 1 has depth 0 in both views, both errors are 0 / 0 = NaN
        # and the reference's comparison keeps every match.  No mismatch can be dropped by construction.
        assert np.array_equal(np.abs(ref["Xh"]), np.tile(np.float32([0, 0, 0, 1]), (tc.N, 1)))
        assert not ref["points3d"].any() and np.all(ref["sigma"][:, 3] == 0)
        assert np.all(np.isnan(ref["err_left"])) and np.all(np.isnan(ref["err_right"])) and ref["keep"].all()
        return
    assert np.all(np.isfinite(ref["err_left"][w != 0])) and np.all(np.isfinite(ref["err_right"][w != 0]))
    assert ref["keep"].any() and not ref["keep"].all()
    assert (~ref["keep"][c["bad"]]).sum() > 0.5 * c["bad"].sum()          # the planted mismatches are what is dropped ...
    assert ref["keep"][~c["bad"]].mean() > 0.9                             # ... and the rest is kept


@pytest.mark.parametrize("name", tc.CASES)
@pytest.mark.parametrize("thr", [10.0, 1.0])
def test_few_matches_sit_on_the_threshold(refs, name, thr):
    """At most 1 % of a case's matches within 4 float ulps (of the largest pixel coordinate) of the threshold, at the reference's own
    points; and outside that band the recomputed decision is the reference's."""
    c, ref = refs[name]
    e, tol, band, keep = tc.error_check(c["K"], c["P_left"], c["P_right"], c["left"], c["right"], ref["points3d"], thr)
    ref_keep = ~((ref["err_left"] > thr) | (ref["err_right"] > thr))
    assert band.mean() <= 0.01
    assert np.array_equal(keep[~band], ref_keep[~band])
    if thr == 10.0:
        assert not band.any()


def test_reference_kat_through_the_long_double_reference():
    """triangulate_from_2_views (SfMUnitTests.cpp:221-251): every point within 0.01 of its canned 3D point."""
    g = json.load(open(GOLD))
    ref = tc.reference(g["K"], g["P_left"], g["P_right"], g["left"], g["right"])
    assert ref["keep"].all() and tc.conditioned(ref).all()
    assert np.linalg.norm(ref["points3d"].astype(np.float64) - np.array(g["points3d"], dtype=np.float64), axis=1).max() < g["tolerance"]
    assert ref["err_left"].max() < 1e-2 and ref["err_right"].max() < 1e-2


def test_jacobi_reference_on_a_matrix_with_known_singular_values():
    rng = np.random.default_rng(7)
    U, _ = np.linalg.qr(rng.normal(size=(4, 4)))
    V, _ = np.linalg.qr(rng.normal(size=(4, 4)))
    s = np.array([3.0, 1.0, 1e-3, 1e-3 - 1e-9])                            # the two smallest 1e-9 apart
    v, sigma, sweeps = tc.jacobi_null_vectors((U * s) @ V.T[None])
    assert np.abs(sigma[0].astype(np.float64) - s).max() < 1e-15
    assert 1.0 - abs(float(v[0].astype(np.float64) @ V[:, 3])) < 1e-12 and sweeps >= 1
