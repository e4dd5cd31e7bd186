"""Named growth sequences for sfmba_problem_append -- TEST INFRASTRUCTURE ONLY (numpy only, importable without a GPU).

A case is a full BAProblem (synthetic.make_problem, fixed seeds) and a list of STEPS: index arrays into its observation list, step 0
for sfmba_problem_create, every later one for an sfmba_problem_append.  step_problem(case, k) is the concatenated problem the handle
must equal after step k: the observations of steps 0 .. k in that order, with the parameter arrays the caller passes at step k.

What each case reaches in csrc/problem_build.hip / structure_build.hip (the smallest shapes at which that code can still go wrong):

  view_order         cameras registered 4, 7, 1 | 8 | 0 | 5 | 2 | 6 | 3 (three at create, one per append), a point enters when two
                     registered cameras see it; camera 9 and a few points (17 and the last one among them) are never observed:
                     camera AND point slots out of caller order, inactive entries inside and at the end of the caller's arrays
  grow_from_one      create with 1 camera, 1 point, 1 observation; active cameras 1 -> 2 -> 3 -> 4 -> 5 -> 8 -> 9 -> 16 -> 17, active
                     points 1 -> 2 and 255 -> 256 -> 257: cshift / end_bit of the packed sort key change (bits_for), the grid edge of
                     k_pm_ptr / k_pm_paircount at npt + 1, points with a single view
  duplicates         an append repeats resident (camera, point) pairs with xy + 0.25, one of them twice (+ 0.5); a second append
                     repeats pairs that are already double: equal sort keys stay old before new, k_dup_blocks
  chunk_edges        3 cameras; block (0, 1) grows from 511 to 513 pairs across SFMBA_PAIR_CHUNK = 512 and camera 2's list from 255 to
                     257 entries across SFMBA_CAM_CHUNK = 256 in one append
  chunk_edges_track  40 cameras; the track of point 0 grows 2 -> 4 -> 5 -> 16 -> 17 -> 40 views (all cameras)
  sort_switch        12 cameras, 8 200 points x 4 views: 32 700 observations at create, the other 100 appended -- both sides of the
                     32 768-item switch of OnesweepAbove32k
  host_threads       6 cameras, 2 000 resident observations, one append of 208 000 (52 000 new points x 4 views, shuffled so that a
                     point's views fall to different host threads): the multi-threaded count loop of build_structure
  no_new_obs         `tiny`; an append without observations that brings two more cameras, five more points and CHANGED parameters
                     for all old ones

Allowed importers: tests/.
"""
from dataclasses import dataclass, field

import numpy as np

from sfm_toy_library_amd import synthetic
from sfm_toy_library_amd.synthetic import BAProblem

PAIR_CHUNK = 512               # SFMBA_PAIR_CHUNK (csrc/ba_kernels.h)
CAM_CHUNK = 256                # SFMBA_CAM_CHUNK
SORT_SWITCH = 32768            # OnesweepAbove32k (csrc/structure_build.hip)
PARALLEL_FOR_MIN = 200000      # csrc/problem_build.hip

VIEW_ORDER = (4, 7, 1, 8, 0, 5, 2, 6, 3)
GROW_CAMS = (1, 2, 3, 4, 5, 8, 9, 16, 17)
GROW_PTS = (1, 1, 2, 2, 255, 256, 257, 257, 257)
TRACK_LENGTHS = (2, 4, 5, 16, 17, 40)

CASES = ("view_order", "grow_from_one", "duplicates", "chunk_edges", "chunk_edges_track", "sort_switch", "host_threads", "no_new_obs")
LAST_STEP_ONLY = ("sort_switch", "host_threads")          # (the GPU test checks their last step alone and skips the Jacobian dump)
LM_STEP_CASES = ("view_order", "duplicates", "chunk_edges", "chunk_edges_track")
F32J_CASES = ("view_order", "duplicates")

# What oracle.build_reduced returns as `info` at the steps of grow_from_one where a point has a single view (recorded; every other
# step of every case gives 0): the damped point block stays invertible and the damped reduced matrix positive definite, so 0 there too.
SINGLE_VIEW_INFO = {0: 0, 2: 0}

# Reduced-system tolerances (max-norm relative) that had to be MEASURED instead of taken from tests/test_gpu_parity.py, as
# (case, step) -> {"S": .., "rhs": ..}: the deviation of a FRESH handle from the oracle on that step, times 4 for reordering.
#   grow_from_one step 0 (one camera, one point, one observation): fresh handle vs oracle S 6.70e-9, rhs 8.85e-9 of the max norm.
#   The deviation is the ORACLE's: a point with a single view leaves its 3 x 3 block V with one direction that only the damping
#   holds (cond V = 2e4), the Schur complement U - W V^-1 W^T cancels to 2e-4 of its terms (max |S| = 1.97e-4), and the oracle's
#   explicit fp64 inverse of V is 6.70e-9 / 8.85e-9 away from the same formulas evaluated in long double (reduced_longdouble below;
#   tests/test_append_cases_cpu.py asserts it).  The GPU test therefore ALSO holds the single-view steps to reduced_longdouble, at
#   the project's 1e-10.  At step 2 (cond V = 2e4 again, but max |S| = 0.53) the oracle is 1e-12 / 9e-12 off: the project's figure holds.
MEASURED_TOL = {("grow_from_one", 0): {"S": 4 * 6.70e-9, "rhs": 4 * 8.85e-9}}

LD = np.longdouble


def reduced_longdouble(prob, res, jc, jp, jf, radius, min_diag=1e-6, max_diag=1e32):
    """oracle.build_reduced's formulas (Jacobi scaling 1 / (1 + column norm), LM diagonal clamp(column norm^2) / radius, Schur
    complement over the points) in np.longdouble, from the residuals and UNSCALED Jacobian blocks per observation that
    oracle.eval_residuals / eval_jacobian give for `prob`: (S, rhs, scale) in the order of include/sfmba.h.  Dense in the reduced
    dimension per observation: for the small steps only."""
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is not the 80-bit extended type here"
    res, jc, jp, jf = (np.asarray(a).astype(LD) for a in (res, jc, jp, jf))
    act, cs = np.unique(prob.obs_cam, return_inverse=True)
    apt, ps = np.unique(prob.obs_pt, return_inverse=True)
    nc, npt, n = len(act), len(apt), len(cs)
    ncol, pcol = np.zeros((nc, 6), LD), np.zeros((npt, 3), LD)
    np.add.at(ncol, cs, (jc ** 2).sum(axis=1))
    np.add.at(pcol, ps, (jp ** 2).sum(axis=1))
    sc, sp, sf = 1 / (1 + np.sqrt(ncol)), 1 / (1 + np.sqrt(pcol)), 1 / (1 + np.sqrt((jf ** 2).sum()))
    d = 6 * nc + 1
    F = np.zeros((n, 2, d), LD)                           # camera and focal columns of every residual row, scaled
    for k in range(n):
        F[k, :, 6 * cs[k]:6 * cs[k] + 6] = jc[k] * sc[cs[k]]
        F[k, :, d - 1] = jf[k] * sf
    B = jp * sp[ps][:, None, :]
    F2 = F.reshape(2 * n, d)
    S = F2.T @ F2
    S += np.diag(np.clip(np.diag(S).copy(), min_diag, max_diag) / radius)
    rhs = F2.T @ res.reshape(-1)
    for i in range(npt):
        sel = np.flatnonzero(ps == i)
        Bi, Fi, ri = B[sel].reshape(-1, 3), F[sel].reshape(-1, d), res[sel].reshape(-1)
        V = Bi.T @ Bi
        V += np.diag(np.clip(np.diag(V).copy(), min_diag, max_diag) / radius)
        M = np.concatenate([V, np.eye(3, dtype=LD)], axis=1)              # V^-1 by Gauss-Jordan (V is positive definite: no pivoting)
        for c in range(3):
            M[c] /= M[c, c]
            for r in range(3):
                if r != c:
                    M[r] -= M[r, c] * M[c]
        T = (Fi.T @ Bi) @ M[:, 3:]
        S -= T @ (Bi.T @ Fi)
        rhs -= T @ (Bi.T @ ri)
    return S, rhs, np.concatenate([sc.ravel(), [sf]])


@dataclass
class AppendCase:
    name: str
    prob: BAProblem                    # the final arrays and EVERY observation the steps index
    steps: list                        # [k] -> int64 indices into prob's observation list
    params: list = field(default_factory=list)          # [k] -> (cam6, pt3, focal) the caller passes at step k

    def __post_init__(self):
        self.steps = [np.asarray(s, np.int64) for s in self.steps]
        if not self.params:
            self.params = [(self.prob.cam6, self.prob.pt3, self.prob.focal)] * len(self.steps)

    @property
    def n_steps(self):
        return len(self.steps)


def step_order(case, k):
    return np.concatenate(case.steps[:k + 1]) if k >= 0 else np.zeros(0, np.int64)


def step_problem(case, k):
    """The problem a handle holds after step k: what sfmba_problem_create would be given for the concatenated list."""
    o = step_order(case, k)
    cam6, pt3, focal = case.params[k]
    p = case.prob
    return BAProblem(np.ascontiguousarray(cam6), np.ascontiguousarray(pt3), float(focal), np.ascontiguousarray(p.obs_cam[o]),
                     np.ascontiguousarray(p.obs_pt[o]), np.ascontiguousarray(p.obs_xy[o]))


def step_new(case, k):
    """What step k hands to create (k = 0) / append: (cam6, pt3, focal, obs_cam, obs_pt, obs_xy)."""
    s = case.steps[k]
    cam6, pt3, focal = case.params[k]
    p = case.prob
    return cam6, pt3, focal, p.obs_cam[s], p.obs_pt[s], p.obs_xy[s]


def slot_order(case, k):
    """(acam_id, apt_id) after step k by the rule of include/sfmba.h: create gives slots in ascending caller index, an append gives a
    newly observed camera / point the next free slot in order of first observation."""
    p = case.prob
    cams = list(np.unique(p.obs_cam[case.steps[0]]))
    pts = list(np.unique(p.obs_pt[case.steps[0]]))
    for s in case.steps[1:k + 1]:
        for arr, have in ((p.obs_cam[s], cams), (p.obs_pt[s], pts)):
            _, first = np.unique(arr, return_index=True)
            seen = set(have)
            have.extend(int(v) for v in arr[np.sort(first)] if v not in seen)
    return np.asarray(cams, np.int64), np.asarray(pts, np.int64)


def _full(n_cam, n_pt, seed):
    """Every camera sees every point: the pool a case picks its (camera, point) pairs from (one consistent set of parameters and
    noisy pixels).  Observation k = point k // n_cam, camera k % n_cam."""
    prob = synthetic.make_problem("small", n_cam=n_cam, n_pt=n_pt, views=n_cam, seed=seed)
    assert prob.n_obs == n_cam * n_pt and np.array_equal(prob.obs_cam[:n_cam], np.arange(n_cam))
    return prob


def _pick(full, cams, pts):
    """Indices into `full` of the pairs (cams[i], pts[i])."""
    return np.asarray(pts, np.int64) * full.n_cam + np.asarray(cams, np.int64)


def _sub(full, idx):
    """`full` restricted to the observations idx (in that order); the steps of the case then index THIS list."""
    return BAProblem(full.cam6, full.pt3, full.focal, np.ascontiguousarray(full.obs_cam[idx]), np.ascontiguousarray(full.obs_pt[idx]),
                     np.ascontiguousarray(full.obs_xy[idx]))


def _split(lengths):
    at = np.concatenate([[0], np.cumsum(lengths)])
    return [np.arange(at[i], at[i + 1]) for i in range(len(lengths))]


def _view_order():
    prob = synthetic.make_problem("small", n_cam=10, n_pt=300, views=(2, 5), seed=4101)
    never = np.isin(prob.obs_pt, (17, prob.n_pt - 1))
    steps, have = [], np.zeros(prob.n_obs, bool)
    for n in range(3, len(VIEW_ORDER) + 1):
        vis = np.isin(prob.obs_cam, VIEW_ORDER[:n]) & ~never
        cnt = np.bincount(prob.obs_pt[vis], minlength=prob.n_pt)
        now = vis & (cnt[prob.obs_pt] >= 2)
        steps.append(np.flatnonzero(now & ~have))
        have = now
    return AppendCase("view_order", prob, steps)


def _grow_from_one():
    n_cam, n_pt = GROW_CAMS[-1], GROW_PTS[-1]
    full = _full(n_cam, n_pt, 4102)
    rng = np.random.default_rng(4102)
    chunks, nc, npt = [], 0, 0
    for k, (c1, p1) in enumerate(zip(GROW_CAMS, GROW_PTS)):
        cams, pts = [], []
        if k == 0:
            cams, pts = [0], [0]
        else:
            for j in range(nc, c1):                     # a new camera sees every second resident point (at least one) ...
                seen = [i for i in range(npt) if (i + j) % 2 == 0] or [0]
                if k == 2:
                    seen = []                           # ... but camera 2 comes in with point 1 alone: a single view
                cams += [j] * len(seen)
                pts += seen
            for i in range(npt, p1):                    # a new point: 2 .. 4 of the cameras registered by now (one, at step 2)
                view = [c1 - 1] if k == 2 else sorted(rng.choice(c1, size=int(rng.integers(2, min(4, c1) + 1)), replace=False).tolist())
                cams += view
                pts += [i] * len(view)
        chunks.append(_pick(full, cams, pts))
        nc, npt = c1, p1
    idx = np.concatenate(chunks)
    assert len(np.unique(idx)) == len(idx)
    return AppendCase("grow_from_one", _sub(full, idx), _split([len(c) for c in chunks]))


def _duplicates():
    base = synthetic.make_problem("small", n_cam=6, n_pt=200, views=(2, 5), seed=4103)
    n = base.n_obs
    d1 = np.arange(0, n, 7)                             # resident pairs, repeated with xy + 0.25 ...
    d1 = np.concatenate([d1, d1[:1]])                   # ... the first of them twice inside the same append
    d2 = np.concatenate([np.arange(0, n, 21), np.arange(3, n, 50)])      # pairs that are already double, and fresh ones
    src = np.concatenate([np.arange(n), d1, d2])
    xy = base.obs_xy[src].copy()
    xy[n:n + len(d1)] += 0.25
    xy[n + len(d1) - 1] += 0.25                         # (its second copy: + 0.5)
    xy[n + len(d1):] -= 0.125
    prob = BAProblem(base.cam6, base.pt3, base.focal, np.ascontiguousarray(base.obs_cam[src]), np.ascontiguousarray(base.obs_pt[src]), xy)
    return AppendCase("duplicates", prob, _split([n, len(d1), len(d2)]))


def _chunk_edges():
    full = _full(3, PAIR_CHUNK + 1, 4104)
    a, b, c, d = PAIR_CHUNK - 1, PAIR_CHUNK + 1, CAM_CHUNK - 1, CAM_CHUNK + 1
    s0 = np.concatenate([_pick(full, np.tile([0, 1], a), np.repeat(np.arange(a), 2)), _pick(full, np.full(c, 2), np.arange(c))])
    s1 = np.concatenate([_pick(full, np.tile([0, 1], b - a), np.repeat(np.arange(a, b), 2)), _pick(full, np.full(d - c, 2), np.arange(c, d))])
    return AppendCase("chunk_edges", _sub(full, np.concatenate([s0, s1])), _split([len(s0), len(s1)]))


def _chunk_edges_track():
    n_cam, n_pt = TRACK_LENGTHS[-1], 400
    full = _full(n_cam, n_pt, 4105)
    rng = np.random.default_rng(4105)
    cams, pts = [], []
    for i in range(1, n_pt):                            # every other point: 2 .. 6 views, all resident from create on
        view = sorted(rng.choice(n_cam, size=int(rng.integers(2, 7)), replace=False).tolist())
        cams += view
        pts += [i] * len(view)
    track = rng.permutation(n_cam)                      # the order in which the cameras come to see point 0
    chunks, at = [], 0
    for m in TRACK_LENGTHS:
        chunks.append(_pick(full, track[at:m], np.zeros(m - at, np.int64)))
        at = m
    chunks[0] = np.concatenate([_pick(full, cams, pts), chunks[0]])
    return AppendCase("chunk_edges_track", _sub(full, np.concatenate(chunks)), _split([len(c) for c in chunks]))


def _sort_switch():
    prob = synthetic.make_problem("small", n_cam=12, n_pt=8200, views=4, seed=4106)
    perm = np.random.default_rng(4106).permutation(prob.n_obs)
    return AppendCase("sort_switch", prob, [perm[:32700], perm[32700:]])


def _host_threads():
    prob = synthetic.make_problem("small", n_cam=6, n_pt=52500, views=4, seed=4107)
    old = np.flatnonzero(prob.obs_pt < 500)
    new = np.flatnonzero(prob.obs_pt >= 500)
    return AppendCase("host_threads", prob, [old, np.random.default_rng(4107).permutation(new)])


def _no_new_obs():
    tiny = synthetic.make_problem("tiny")
    more = synthetic.make_problem("tiny", n_cam=tiny.n_cam + 2, n_pt=tiny.n_pt + 5, seed=4108)
    rng = np.random.default_rng(4108)
    cam = np.vstack([tiny.cam6 + rng.normal(0.0, 2e-3, tiny.cam6.shape), more.cam6[tiny.n_cam:]])
    pt = np.vstack([tiny.pt3 + rng.normal(0.0, 5e-3, tiny.pt3.shape), more.pt3[tiny.n_pt:]])
    prob = BAProblem(cam, pt, tiny.focal * 0.99, tiny.obs_cam, tiny.obs_pt, tiny.obs_xy)
    return AppendCase("no_new_obs", prob, [np.arange(tiny.n_obs), np.zeros(0, np.int64)],
                      [(tiny.cam6, tiny.pt3, tiny.focal), (cam, pt, tiny.focal * 0.99)])


_MAKERS = {"view_order": _view_order, "grow_from_one": _grow_from_one, "duplicates": _duplicates, "chunk_edges": _chunk_edges,
           "chunk_edges_track": _chunk_edges_track, "sort_switch": _sort_switch, "host_threads": _host_threads, "no_new_obs": _no_new_obs}
_cache = {}


def make_case(name):
    """The case `name`, built once per process and never modified."""
    if name not in _cache:
        _cache[name] = _MAKERS[name]()
    return _cache[name]


def checked_steps(name):
    """The steps of a case at which the GPU test looks."""
    n = make_case(name).n_steps
    return [n - 1] if name in LAST_STEP_ONLY else list(range(n))
