"""Named inputs of sfmba_mesh_decimate for the CPU and GPU tests -- TEST INFRASTRUCTURE ONLY.

A case is a dict: xyz float32 [n, 3], bgr uint8 [n, 3] or None, tri int32 [m, 3], origin float32 [3], quantum (float32), cell,
placement, reg.  want(name) gives the restatement's answer once per process (decimate_oracle.decimate_np; None where the call
refuses); it is shared and not to be changed.  Most geometry is built in integer quanta about origin 0 with quantum 2^-10, so that a
case puts a vertex into the cell, and at the remainder, that its name claims.  The shapes are the smallest at which the kernels can
still go wrong: the wave is 64 lanes, a workgroup 256, a run of more than 32 members is reduced by a wave, and the radix sort changes
its algorithm above 32 768 items."""
import functools

import numpy as np

import decimate_oracle as do
import mesh_clean_cases as cc

Q = 2.0 ** -10
CELL = 256


def _case(xyz, tri, bgr="random", origin=(0.0, 0.0, 0.0), quantum=Q, cell=CELL, placement=1, reg=1024, seed=0):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    if isinstance(bgr, str):
        bgr = np.random.default_rng(seed + 700).integers(0, 256, size=(len(xyz), 3)).astype(np.uint8)
    return dict(xyz=xyz, bgr=bgr, tri=tri, origin=np.asarray(origin, np.float32), quantum=np.float32(quantum), cell=int(cell), placement=int(placement),
                reg=int(reg))


def _quanta(P, tri, **kw):
    """a case from integer positions (|P| < 2^24, so P 2^-10 is a float32)"""
    return _case(np.asarray(P, np.float64).reshape(-1, 3) * kw.get("quantum", Q), tri, **kw)


def with_params(name, **params):
    def make():
        c = dict(case(name))
        c.update(params)
        return c
    return make


# ---- clusters by construction -------------------------------------------------------------------------------------------------
def cell_at(i):
    """the cell of the i-th cluster of cells_mesh: a walk through positive and negative cells with no two alike"""
    return np.array([i % 7 - 3, (i // 7) % 5 - 2, i // 35 - 1])


def cells_mesh(members, seed, cell=CELL, per_link=3, **kw):
    """len(members) clusters, cluster i with members[i] vertices at random remainders of cell_at(i); the vertex numbering is shuffled.
    Triangles: per_link on every three consecutive clusters, with random members, order and orientation (so there are duplicates of
    both orientations), and one inside every cluster of three or more members (collapsed, yet it feeds the quadric)."""
    rng = np.random.default_rng(seed)
    P, owner = [], []
    for i, m in enumerate(members):
        P.append(cell_at(i)[None, :] * cell + rng.integers(0, cell, size=(m, 3)))
        owner += [i] * m
    P, owner = np.concatenate(P), np.asarray(owner)
    perm = rng.permutation(len(P))
    P, owner = P[perm], owner[perm]
    of = [np.nonzero(owner == i)[0] for i in range(len(members))]
    tri = []
    for i in range(len(members)):
        if i + 2 < len(members):
            for _ in range(per_link):
                t = [int(rng.choice(of[j])) for j in (i, i + 1, i + 2)]
                tri.append([t[k] for k in rng.permutation(3)])
        if len(of[i]) >= 3:
            tri.append([int(v) for v in rng.choice(of[i], 3, replace=False)])
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    return _quanta(P, tri[rng.permutation(len(tri))] if len(tri) else tri, cell=cell, seed=seed, **kw)


RUNS = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1, 300, 2, 64, 3)          # member counts across wave and workgroup edges of the sorted order


def sheet_quanta(nx, ny, step, seed, at=(0, 0, 0), noise=0):
    """cc.sheet in integer quanta: nx x ny vertices `step` quanta apart, 2 (nx - 1) (ny - 1) triangles"""
    rng = np.random.default_rng(seed)
    Y, X = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    P = np.stack([X * step + at[0], Y * step + at[1], np.full(X.shape, at[2])], axis=-1).reshape(-1, 3)
    if noise:
        P = P + rng.integers(-noise, noise + 1, size=P.shape)
    v = (Y * nx + X)[:-1, :-1].reshape(-1)
    tri = np.concatenate([np.stack([v, v + 1, v + nx + 1], axis=1), np.stack([v, v + nx + 1, v + nx], axis=1)])
    return P, tri


def _n_vertices(n):
    """a wavy sheet of 181 x 181 = 32 761 vertices and loose vertices up to n"""
    P, tri = sheet_quanta(181, 181, 37, n, at=(-3000, -3100, 0))
    P[:, 2] = np.round(300.0 * np.sin(P[:, 0] / 900.0) * np.cos(P[:, 1] / 700.0)).astype(np.int64)
    loose = np.random.default_rng(n).integers(-4000, 4000, size=(n - len(P), 3))
    return _quanta(np.concatenate([P, loose]), tri, seed=n)


def _n_triangles(n):
    """129 x 129 vertices: 32 768 triangles, one dropped or one repeated"""
    P, tri = sheet_quanta(129, 129, 50, n, at=(-3200, -3200, 77), noise=12)
    tri = tri[:-1] if n == 32767 else np.concatenate([tri, tri[:1]]) if n == 32769 else tri
    assert len(tri) == n
    return _quanta(P, tri, seed=n)


def _faces():
    """vertices exactly on cell faces (r = 0) and one quantum below (r = cell - 1), at positive and negative cells"""
    P = [[256, 0, -256], [255, -1, -257], [-512, 511, 0], [-513, 512, 1], [0, 0, 0], [-1, -1, -1], [768, -768, 255], [767, -769, 256]]
    tri = [[0, 2, 4], [1, 3, 5], [4, 6, 7], [0, 1, 6], [2, 3, 7]]
    return _quanta(P, tri)


def _halves():
    """coordinates on a half quantum: the quotient is k + 0.5 and rounds up, so 255.5 belongs to the next cell and -0.5 to cell 0"""
    h = np.asarray([[255.5, -0.5, 0.5], [-256.5, 511.5, -1.5], [600.5, 300.5, -300.5], [10.0, 700.5, 255.5]], np.float64)
    return _case(h * Q, [[0, 1, 2], [0, 2, 3]])


BIG = cc.BIG                                # 2^25 - 2 is a float32; about an origin of -+1 it quantises to +-(2^25 - 1)


def _rim(x0, origin_x, cell):
    xyz = [[x0, 0, 0], [0, 100, 0], [0, 0, 100], [50, 50, 50], [x0, 1, 1]]
    return _case(xyz, [[0, 1, 2], [0, 2, 3], [0, 3, 1], [4, 1, 2]], origin=(origin_x, 0.0, 0.0), quantum=1.0, cell=cell)


def _cell_max():
    """cell 2^20 with quantum 1: the cells -32 .. 31 an axis"""
    rng = np.random.default_rng(5)
    P = rng.integers(-(1 << 25) + 2, 1 << 25, size=(200, 3)) // 2 * 2                   # even: a float32 below 2^25
    tri = rng.integers(0, 200, size=(300, 3))
    return _case(P.astype(np.float64), tri, quantum=1.0, cell=1 << 20, seed=5)


def _unused():
    P, tri = sheet_quanta(9, 8, 100, 41, at=(-350, -333, 40), noise=20)
    spread = np.arange(len(P)) * 2 + 1                                                  # used vertices at the odd places, loose ones between
    out = np.random.default_rng(41).integers(-3000, 3000, size=(2 * len(P) + 1, 3))
    out[spread] = P
    return _quanta(out, spread[tri], seed=41)


def _repeated_index():
    # (2, 2, 3) names vertex 2 twice: collapsed, no quadric; (6, 6, 6) likewise
    P = [[0, 0, 0], [300, 0, 30], [0, 300, 0], [900, 0, 0], [1200, 0, 50], [900, 300, 0], [2000, 2000, 2000]]
    return _quanta(P, [[0, 1, 2], [3, 4, 5], [2, 2, 3], [6, 6, 6]], seed=42)


def _zero_area():
    # (3, 4, 5) is collinear over three cells: it survives and feeds no quadric; clusters 4 and 5 have no other triangle (the mean)
    P = [[10, 10, 10], [300, 20, 10], [20, 300, 60], [300, 300, 10], [600, 600, 10], [900, 900, 10]]
    return _quanta(P, [[0, 1, 2], [1, 3, 2], [3, 4, 5]], seed=43)


def _duplicates():
    """four groups of two triangles on one cluster triple: equal and opposite orientation, the pair in both input orders; the two
    triangles of a group use different members of the clusters"""
    P, tri = [], []
    for g in range(4):
        base = np.array([g * 1024 - 2000, 0, 0])
        cellc = [base, base + [256, 0, 0], base + [0, 256, 0]]
        first = [len(P) + k for k in range(3)]
        second = [len(P) + 3 + k for k in range(3)]
        P += [list(c + [10 + 7 * g, 20, 30]) for c in cellc] + [list(c + [200, 100 + g, 90]) for c in cellc]
        other = second if g < 2 else [second[0], second[2], second[1]]                  # groups 2, 3: opposite orientation
        other = other[1:] + other[:1]                                                   # and another starting index
        tri += [first, other] if g % 2 == 0 else [other, first]
    return _quanta(P, tri, seed=44)


def _wedge(axis, up):
    """Two small sheets inside one cell on planes that meet 64 quanta OUTSIDE it along `axis` (above cell - 1 with up, below 0
    otherwise), and one triangle to two neighbouring cells so that the cluster is emitted: the solve is clamped."""
    P, tri = [], []
    for sx, x0 in ((3, 40), (-3, 168)):
        for j in range(3):
            for i in range(3):
                x = x0 + 24 * i
                z = 3 * x - 64 if sx > 0 else 704 - 3 * x
                P.append([x, 60 + 50 * j, z])
        b = len(P) - 9
        for j in range(2):
            for i in range(2):
                v = b + 3 * j + i
                tri += [[v, v + 1, v + 4], [v, v + 4, v + 3]]
    P = np.asarray(P)
    if not up:
        P[:, 2] = 255 - P[:, 2]
    link = len(P)
    P = np.concatenate([P, [[300, 100, 128], [100, 300, 128]]])
    tri.append([0, link, link + 1])
    roll = {2: [0, 1, 2], 0: [2, 0, 1], 1: [1, 2, 0]}[axis]                             # the wedge's z becomes `axis`
    P = P[:, roll] + np.array([512, -768, 256])                                         # some cell that is not cell 0
    return P, np.asarray(tri)


def _clamps():
    parts = []
    for k, (axis, up) in enumerate(((0, True), (0, False), (1, True), (1, False), (2, True), (2, False))):
        P, tri = _wedge(axis, up)
        parts.append((P + np.array([2048 * k - 6144, 0, 0]), tri))
    P, tri = cc.join(*parts)
    return _quanta(P, tri, reg=1, seed=45)


def _x_on_a_half():
    """two level triangles at r_z = 10 and 11 inside one cell: u = (0, 0, 1024) exactly, and every product of the solve is exact, so
    x_z = 10.5 and rounds UP to 11; a third triangle without area reaches two neighbouring cells, so that the cluster is emitted and
    its quadric stays what the two level triangles made it"""
    P = [[20, 20, 10], [120, 20, 10], [20, 120, 10], [140, 140, 11], [240, 140, 11], [140, 240, 11], [276, 20, 10], [532, 20, 10]]
    return _quanta(P, [[0, 1, 2], [3, 4, 5], [0, 6, 7]], reg=1024, bgr=None)


def fan(n_triangles):
    """n_triangles + 1 rim vertices about 300 quanta apart on a circle of 2^22 quanta around vertex 0, which sits alone in a cell
    above their plane: every triangle has area, and n_inc of the centre's cluster is n_triangles.  Cells of 2^16 quanta."""
    a = np.arange(n_triangles + 1) * (1.5 * np.pi / n_triangles)
    rim = np.round(np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], axis=1) * float(1 << 22))
    P = np.concatenate([[[100.0, 200.0, float((1 << 17) + 5)]], rim])
    r = np.arange(1, n_triangles + 1)
    return _case(P, np.stack([np.zeros_like(r), r, r + 1], axis=1), bgr=None, quantum=1.0, cell=1 << 16)


def _mean_halves():
    """two members a cluster at r = 10 and 11 (and colours 10 and 11): the mean 10.5 rounds up; three such clusters and a triangle"""
    P, bgr = [], []
    for c in ([0, 0, 0], [-256, 256, 0], [256, 0, -256]):
        P += [[c[0] + 10, c[1] + 20, c[2] + 30], [c[0] + 11, c[1] + 21, c[2] + 31]]
        bgr += [[10, 0, 255], [11, 1, 254]]
    return _quanta(P, [[0, 2, 4], [1, 3, 5]], bgr=np.asarray(bgr, np.uint8), placement=0)


def cube(n=40, rz=0.3, rx=0.2, rotate=True):
    """the surface of the unit cube, n x n x 2 triangles a face, vertices shared along the edges, outward orientation; rotated by rz
    about z, then by rx about x.  Returns float64 xyz, tri and the rotation R (xyz = unit @ R.T)."""
    idx, pts, tri = {}, [], []

    def vid(p):
        if p not in idx:
            idx[p] = len(pts)
            pts.append(p)
        return idx[p]
    for axis in range(3):
        for side in (0, 1):
            a, b = [k for k in range(3) if k != axis]
            for j in range(n):
                for i in range(n):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[a], p[b] = side * n, i + di, j + dj
                        q.append(vid(tuple(p)))
                    flip = (side == 0) != (axis == 1)                                   # (a, b, axis) is right-handed but for axis 1
                    for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
                        tri.append(t[::-1] if flip else t)
    unit = np.asarray(pts, np.float64) / n
    cz, sz, cx, sx = np.cos(rz), np.sin(rz), np.cos(rx), np.sin(rx)
    R = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) if rotate else np.eye(3)
    return unit @ R.T, np.asarray(tri, np.int64), R


def cube_distance(xyz, R):
    """the distance of points to the surface of the unit cube rotated by R"""
    p = np.asarray(xyz, np.float64) @ R                                                 # back: R^T p as rows
    d = np.abs(p - 0.5) - 0.5                                                           # per axis: > 0 outside the slab
    outside = np.linalg.norm(np.maximum(d, 0.0), axis=1)
    inside = -np.max(d, axis=1)
    return np.where((d > 0).any(axis=1), outside, inside)


def cube_case(cell, placement, n=40, **kw):
    xyz, tri, _ = cube(n)
    return _case(xyz, tri, quantum=1.0 / 4096.0, cell=cell, placement=placement, seed=cell, **kw)


def _small_cube():
    """an axis-aligned cube of 8 x 8 x 2 triangles a face, 0.9 wide and off the cell faces: clusters with a plane (rank-1 A), with an
    edge and with a corner"""
    xyz, tri, _ = cube(8, rotate=False)
    return _case(xyz * 0.9 + np.array([0.013, -0.441, 0.207]), tri, quantum=Q, cell=256, seed=46)


def icosphere(level=5, radius=0.5, centre=(0.503, 0.497, 0.511)):
    """20 4^level triangles"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2],
         [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = g
    return np.asarray(v) * radius + np.asarray(centre), np.asarray(f, np.int64)


def _from_cleaning(name, **kw):
    c = cc.case(name)
    return _case(c["xyz"], c["tri"], bgr=c["bgr"], origin=c["origin"], quantum=c["quantum"], cell=2048, **kw)


def permuted_vertices(name, seed):
    """the same geometry with the vertex numbering permuted"""
    def make():
        c = dict(case(name))
        perm = np.random.default_rng(seed).permutation(len(c["xyz"]))                   # old index -> new index
        xyz = np.zeros_like(c["xyz"])
        xyz[perm] = c["xyz"]
        c["xyz"] = xyz
        if c["bgr"] is not None:
            bgr = np.zeros_like(c["bgr"])
            bgr[perm] = c["bgr"]
            c["bgr"] = bgr
        c["tri"] = perm[c["tri"]].astype(np.int32)
        c["perm"] = perm
        return c
    return make


def permuted_triangles(name, seed):
    def make():
        c = dict(case(name))
        c["tri"] = c["tri"][np.random.default_rng(seed).permutation(len(c["tri"]))]
        return c
    return make


CASES = {
    "empty_0": lambda: _case(np.zeros((0, 3)), np.zeros((0, 3))),
    "empty_5": lambda: _case(np.random.default_rng(1).normal(size=(5, 3)), np.zeros((0, 3))),
    "one_triangle": lambda: _quanta([[0, 0, 0], [300, 0, 0], [0, 300, 100]], [[0, 1, 2]]),
    "one_cell": lambda: _quanta(*sheet_quanta(5, 5, 50, 3, at=(10, 10, 100), noise=5), seed=3),
    "clusters_2": lambda: cells_mesh((4, 5), 60),
    "clusters_63": lambda: cells_mesh((3,) * 63, 63),
    "clusters_64": lambda: cells_mesh((3,) * 64, 64),
    "clusters_65": lambda: cells_mesh((3,) * 65, 65),
    "member_runs": lambda: cells_mesh(RUNS, 66),
    "member_runs_mean": with_params("member_runs", placement=0),
    "vertices_32767": lambda: _n_vertices(32767),
    "vertices_32768": lambda: _n_vertices(32768),
    "vertices_32769": lambda: _n_vertices(32769),
    "triangles_32767": lambda: _n_triangles(32767),
    "triangles_32768": lambda: _n_triangles(32768),
    "triangles_32769": lambda: _n_triangles(32769),
    "faces": _faces,
    "halves": _halves,
    "rim_plus": lambda: _rim(BIG, -1.0, 32),
    "rim_minus": lambda: _rim(-BIG, 1.0, 32),
    "cell_32": lambda: cells_mesh((5,) * 40, 67, cell=32),
    "cell_max": _cell_max,
    "unused": _unused,
    "repeated_index": _repeated_index,
    "zero_area": _zero_area,
    "duplicates": _duplicates,
    "small_cube": _small_cube,
    "small_cube_reg_1": with_params("small_cube", reg=1),
    "small_cube_reg_max": with_params("small_cube", reg=1 << 20),
    "small_cube_mean": with_params("small_cube", placement=0),
    "clamps": _clamps,
    "x_on_a_half": _x_on_a_half,
    "fan_65536": lambda: fan(65536),
    "fan_65537": lambda: fan(65537),
    "mean_halves": _mean_halves,
    "no_colour": with_params("member_runs", bgr=None),
    "member_runs_renumbered": permuted_vertices("member_runs", 68),
    "small_cube_renumbered": permuted_vertices("small_cube", 69),
    "member_runs_reordered": permuted_triangles("member_runs", 70),
    "small_cube_reordered": permuted_triangles("small_cube", 71),
    "sphere_14": lambda: _from_cleaning("sphere_14"),
    "torus_18": lambda: _from_cleaning("torus_18"),
    "zeros_14": lambda: _from_cleaning("zeros_14"),
    "sphere_14_mean": lambda: _from_cleaning("sphere_14", placement=0),
}

# the calls that refuse on the device
REFUSED = {
    "rim_plus_refused": lambda: _rim(float(1 << 25), 0.0, 32),
    "rim_minus_refused": lambda: _rim(-float(1 << 25), 0.0, 32),
    "nan_coordinate": lambda: _bad_coordinate(np.nan),
    "inf_coordinate": lambda: _bad_coordinate(-np.inf),
}
SLOW_LOOP = ("fan_65536", "fan_65537", "vertices_32767", "vertices_32768", "vertices_32769", "triangles_32767", "triangles_32768", "triangles_32769")
FIELDS = ("xyz", "bgr", "members", "tri", "triangle_of", "vertex_of")


def _bad_coordinate(value):
    c = dict(case("small_cube"))
    c["xyz"] = c["xyz"].copy()
    c["xyz"][40, 1] = value
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    return (CASES.get(name) or REFUSED[name])()


def args(c):
    return (c["xyz"], c["bgr"], c["tri"], c["origin"], c["quantum"], c["cell"], c["placement"], c["reg"])


@functools.lru_cache(maxsize=None)
def want(name):
    return do.decimate_np(*args(case(name)))


@functools.lru_cache(maxsize=None)
def internals(name):
    return do.decimate_np(*args(case(name)), want_internals=True)["internals"]
