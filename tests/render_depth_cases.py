"""Cases for sparse.render_depth / depth="render" (csrc/render_depth_batched.hip) and their reference.  numpy on the CPU, no device code.

The reference states the rendered depth per view with the oracle's own pieces, one scene and one view at a time -- exactly what the
batched call replaces: oracle.project._project(w2c, the entry's xyz, K) and oracle.project.render_depth(p, pi, (W, H), cut), the
restatement of models/utils/fusion_util.py:126-130 that tests/golden/mapping.npz pins.  A view's entry is the rows whose batch column
EQUALS view_entry[v]: rows with a fractional, negative, too large or NaN batch index belong to no entry, and a view whose entry is
outside 0..65535 has no rows at all.

Generic scenes come from tests/lift_batched_cases.py (cameras near the identity looking down +z, points at z in 0.5 .. 3, images of at
most 16 x 12): row 2 of every camera is (0, 0, 1, t_z), so p_z = z + t_z is one rounding whatever the order of the dot product, and
the images can be compared bit for bit.  The edge cases use identity cameras, a power-of-two focal and dyadic coordinates (the rule
of lift_batched_cases' edge cases); where z is 0.2 or its neighbour the quotient is not dyadic, but with an identity camera the oracle
and the kernel run the same IEEE operations on the same operands, (x * fx) / z + cx, so they agree bit for bit all the same.

LIFT_CASES are lift_batched_cases.Case objects WITHOUT depth maps: the lift tests run them with depth="render" and with the
reference's rendered depth as a tensor.  tests/test_render_depth_cases_host.py checks that the rendered depth hides at least 10 % of the
pairs that depth=None keeps in each of them (and leaves at least 25 %), so "render" cannot pass by behaving like None.
"""
import numpy as np

import lift_batched_cases as lb
from oracle import project as oproj

f64 = np.float64
FAR = 999999.0
# the z-buffer kernel's launch shape (rd_zbuffer_kernel, lb_counts_kernel's): at most 64 blocks of 256 threads per view stride the rows
# of the view's entry, so one trip of the loop covers 16 384 rows
VIEW_BLOCKS, THREADS = 64, 256
ONE_TRIP = VIEW_BLOCKS * THREADS


class RCase:
    """points f64 [N,4]; view_entry i64 [V]; w2c f64 [V,4,4]; intr f64 [V,4]; image H x W; cut"""

    def __init__(self, name, points, view_entry, w2c, intr, H, W, cut=0, **notes):
        self.name, self.H, self.W, self.cut, self.notes = name, int(H), int(W), int(cut), notes
        self.points = np.ascontiguousarray(points, f64)
        self.view_entry = np.ascontiguousarray(view_entry, np.int64)
        self.w2c, self.intr = np.ascontiguousarray(w2c, f64), np.ascontiguousarray(intr, f64)
        self.N, self.V = len(self.points), len(self.view_entry)
        assert self.points.shape == (self.N, 4) and self.w2c.shape == (self.V, 4, 4) and self.intr.shape == (self.V, 4)
        assert self.H <= 12 and self.W <= 16

    def rows_of(self, b):
        """the rows of entry b; none for a b outside 0..65535, whatever the batch column holds"""
        return np.nonzero(self.points[:, 0] == b)[0] if 0 <= b < lb.MAX_ENTRIES else np.zeros(0, np.int64)

    def K(self, v):
        fx, fy, cx, cy = self.intr[v]
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f64)


def of_lift_case(c, name=None, cut=None):
    """the geometry of a lift_batched_cases.Case"""
    return RCase(name or c.name, c.points, c.view_entry, c.w2c, c.intr, c.H, c.W, c.cut if cut is None else cut)


def render_view(c, v, xyz):
    """the oracle's z-buffer of view v over the points xyz f64 [n,3] -> f64 [H,W]"""
    if len(xyz) == 0:
        return np.full((c.H, c.W), FAR)
    with np.errstate(all="ignore"):
        p, pi = oproj._project(c.w2c[v], xyz, c.K(v))
        return oproj.render_depth(p, pi, (c.W, c.H), c.cut)


def render(c):
    """the reference: f64 [V,H,W], per view over its entry's points"""
    return np.stack([render_view(c, v, c.points[c.rows_of(c.view_entry[v]), 1:]) for v in range(c.V)])


_REFERENCES = {}


def reference(name):
    """computed once per case and shared: callers must not change it"""
    if name not in _REFERENCES:
        _REFERENCES[name] = render(case(name))
        _REFERENCES[name].setflags(write=False)
    return _REFERENCES[name]


def restatement(c):
    """fusion_util.py:126-130 once more, as the sequential loop it is: for every point in row order,
    `if p2 > 0.2 and inside and depth[v, u] > p2: depth[v, u] = p2` -- none of the oracle's functions"""
    out = np.full((c.V, c.H, c.W), FAR)
    with np.errstate(all="ignore"):
        for v in range(c.V):
            M, (fx, fy, cx, cy) = c.w2c[v], c.intr[v]
            for r in c.rows_of(c.view_entry[v]):
                x, y, z = c.points[r, 1:]
                p0, p1, p2 = (M[a, 0] * x + M[a, 1] * y + M[a, 2] * z + M[a, 3] for a in range(3))
                u, t = np.round(p0 * fx / p2 + cx), np.round(p1 * fy / p2 + cy)
                if not (np.isfinite(u) and np.isfinite(t)):
                    continue
                u, t = int(u), int(t)
                inside = u >= c.cut and t >= c.cut and u < c.W - c.cut and t < c.H - c.cut
                if p2 > 0.2 and inside and out[v, t, u] > p2:
                    out[v, t, u] = p2
    return out


# ------------------------------------------------------------------------------------------ the pairs a lift keeps
def pairs(c, depth, tau=0.25):
    """the (point, view) pairs of the geometry c that the lift's visibility test keeps: depth None (p_z > 0) or f64 [V,H,W]
    -> bool [N,V] (False outside a view's entry)"""
    keep = np.zeros((c.N, c.V), bool)
    for v in range(c.V):
        rows = c.rows_of(c.view_entry[v])
        if len(rows) == 0:
            continue
        with np.errstate(all="ignore"):
            m, _ = oproj.compute_mapping_scannet(c.w2c[v].T, c.points[rows, 1:], None if depth is None else depth[v], c.K(v), (c.W, c.H), c.cut,
                                                 tau)
        keep[rows, v] = m[:, 2] == 1
    return keep


# ------------------------------------------------------------------------------------------ cases
def _generic(name, seed, sizes, views, **kw):
    return lb.generic(name, seed, sizes, views, 1, depth=False, **kw)


def case_twins():
    """Two entries under the SAME camera in views of different entries: entry 1 is entry 0 moved 0.25 towards the camera, so the two
    hit many of the same pixels at different depths, and both images would change if entries mixed"""
    rng = np.random.default_rng(31)
    xyz = lb.cloud(rng, 80)
    near = xyz - [0, 0, 0.25]
    pts = np.vstack([np.column_stack([np.full(80, b, f64), a]) for b, a in ((0, xyz), (1, near))])[np.arange(160).reshape(2, 80).T.reshape(-1)]
    M, K = lb.camera(rng)
    return RCase("twins", pts, [0, 1, 1, 0], np.tile(M, (4, 1, 1)), np.tile(K, (4, 1)), 12, 16)


def case_stride():
    """An entry whose rows exceed one trip of the stride loop (ONE_TRIP + 316) beside a one-row entry, rows shuffled"""
    rng = np.random.default_rng(32)
    n = ONE_TRIP + 316
    pts = np.vstack([np.column_stack([np.full(n, 3.0), lb.cloud(rng, n)]), [[1.0, 0.0, 0.0, 1.0]]])[rng.permutation(n + 1)]
    cams = [lb.camera(rng) for _ in range(3)]
    return RCase("stride", pts, [3, 1, 3], np.stack([m for m, _ in cams]), np.stack([k for _, k in cams]), 12, 16)


EXACT_FX = 8.0
Z_EDGE = 0.2                                                # the reference's near limit: p_z > 0.2


def exact_rows():
    """(name, entry, x, y, z) at W = 16, H = 12, cut = 0, identity cameras of focal 8, centre (8, 6): u = 8 x / z + 8, v = 8 y / z + 6"""
    at = lambda u, v, z: ((u - 8) * z / 8, (v - 6) * z / 8, z)                     # noqa: E731
    up = np.nextafter(Z_EDGE, 1.0)
    return [("z_on_the_limit", 0, 0.0, 0.0, Z_EDGE),                               # pixel (6, 8): excluded, p_z > 0.2 is strict
            ("z_past_the_limit", 0, 3 * up / 8, 0.0, up),                          # pixel (6, 11): included
            ("behind", 0, *at(7.0, 6.0, -1.0)), ("behind_far", 0, *at(2.0, 2.0, -4.0)),
            ("on_the_camera_plane", 0, 0.25, 0.0, 0.0), ("at_the_camera", 0, 0.0, 0.0, 0.0),          # p2 == 0: inf and NaN pixels
            ("half_down", 0, *at(4.5, 9.0, 1.0)), ("half_up", 0, *at(5.5, 10.0, 1.0)),                # 4.5 -> 4, 5.5 -> 6
            ("half_row", 0, *at(1.0, 0.5, 1.0)), ("half_row_z2", 0, *at(14.0, 1.5, 2.0)),             # rows 0.5 -> 0, 1.5 -> 2
            ("half_out", 0, *at(15.5, 6.0, 1.0)), ("half_in", 0, *at(-0.5, 6.0, 1.0)),                # 15.5 -> 16 (outside), -0.5 -> -0 (column 0)
            ("pair_far", 0, *at(3.0, 3.0, 2.0)), ("pair_near", 0, *at(3.25, 3.0, 1.5)),               # two points in pixel (3, 3)
            ("triple_a", 0, *at(4.0, 3.0, 1.5)), ("triple_b", 0, *at(4.25, 3.25, 1.5)), ("triple_c", 0, *at(3.75, 2.75, 2.5)),   # pixel (3, 4), equal z
            ("first_is_nearest", 0, *at(6.0, 3.0, 0.5)), ("then_farther", 0, *at(6.0, 3.0, 4.0)),
            ("other_entry_nearer", 1, *at(3.0, 3.0, 0.5)), ("other_entry_farther", 1, *at(4.0, 3.0, 8.0)),
            ("other_entry_alone", 1, *at(12.0, 8.0, 1.0))]


def case_exact():
    rows = exact_rows()
    order = np.random.default_rng(33).permutation(len(rows))
    pts = np.array([(b, x, y, z) for _, b, x, y, z in rows], f64)[order]
    M, K = lb._identity_views(3, EXACT_FX, 16, 12)
    return RCase("exact", pts, [0, 1, 0], M, K, 12, 16, row_names=[rows[i][0] for i in order],
                 expect={0: {(6, 8): FAR, (6, 11): np.nextafter(Z_EDGE, 1.0), (6, 7): FAR, (9, 4): 1.0, (9, 5): FAR, (10, 6): 1.0, (10, 5): FAR,
                             (0, 1): 1.0, (2, 14): 2.0, (1, 14): FAR, (6, 0): 1.0, (3, 3): 1.5, (3, 4): 1.5, (3, 6): 0.5, (8, 12): FAR},
                         1: {(3, 3): 0.5, (3, 4): 8.0, (8, 12): 1.0, (6, 11): FAR}})


def case_bad():
    """ops level only (sparse refuses them): views whose entry is outside 0..65535 and rows whose batch index is fractional, negative,
    too large or NaN, all placed where they would be rendered if they belonged to an entry"""
    rng = np.random.default_rng(34)
    good = np.vstack([np.column_stack([np.full(n, b, f64), lb.cloud(rng, n)]) for b, n in ((0, 40), (65535, 30))])
    bad = np.column_stack([[0.5, -1.0, 65536.0, np.nan, 1e300], lb.cloud(rng, 5)])
    bad[:, 1:3] = 0.0                                                            # on the optical axis: inside every image
    pts = np.vstack([good, bad])[rng.permutation(75)]
    ve = np.array([0, -1, 65535, 65536, 2 ** 40, 0], np.int64)
    cams = [lb.camera(rng) for _ in ve]
    return RCase("bad", pts, ve, np.stack([m for m, _ in cams]), np.stack([k for _, k in cams]), 12, 16, bad_rows=4, nonfinite_rows=1, bad_views=3,
                 top_batch=65535)


_BUILDERS = {
    # entries 0, 2 and 65535 with gaps between them, entry 0 with one row; rows shuffled, views interleaved
    "entries": lambda: of_lift_case(_generic("entries", 21, {0: 1, 2: 45, 65535: 30}, {0: 2, 2: 3, 65535: 2})),
    # entry 1: points and no views; entry 3: views and no points
    "no_points_no_views": lambda: of_lift_case(_generic("no_points_no_views", 22, {0: 40, 1: 30}, {0: 2, 3: 2})),
    "v1": lambda: of_lift_case(_generic("v1", 23, {0: 50}, {0: 1})),
    "views_130": lambda: of_lift_case(_generic("views_130", 24, {0: 60, 1: 300}, {0: 2, 1: 130})),
    "ordered": lambda: of_lift_case(_generic("ordered", 25, {0: 70, 1: 80}, {0: 2, 1: 3}, shuffle=False, interleave=False)),
    # 3 x 11 x 13 = 429 values: the fill's pairs leave a scalar tail
    "image_11x13": lambda: of_lift_case(_generic("image_11x13", 26, {0: 300, 4: 200}, {0: 2, 4: 1}, hw=(11, 13))),
    # 11 x 11 with cut 5: the interior is the one pixel (5, 5); with cut 6: nothing
    "cut_one_pixel": lambda: of_lift_case(_generic("cut_one_pixel", 27, {0: 300, 1: 300}, {0: 2, 1: 2}, hw=(11, 11), cut=5)),
    "cut_nothing": lambda: of_lift_case(_generic("cut_nothing", 27, {0: 300, 1: 300}, {0: 2, 1: 2}, hw=(11, 11), cut=6)),
    "stride": case_stride,
    "twins": case_twins,
    "exact": case_exact,
}
CASES = tuple(_BUILDERS)
OPS_ONLY = ("bad",)
_BUILDERS["bad"] = case_bad
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


# ------------------------------------------------------------------------------------------ the lift cases
_LIFT_BUILDERS = {
    # "nearest": about 300 points per entry on 16 x 12 (the rendered depth then hides about one pair in seven)
    "lift_nearest": lambda: lb.generic("lift_nearest", 41, {0: 300, 2: 320}, {0: 3, 2: 4}, 5, depth=False),
    "lift_bilinear": lambda: lb.generic("lift_bilinear", 42, {0: 310, 1: 300}, {0: 4, 1: 3}, 3, hw=(5, 7), image_shape=(12, 16), mode="bilinear",
                                        depth=False, cut=1),
    # more views than one lane group of the lift kernel, a drop rule that bites
    "lift_views_70": lambda: lb.generic("lift_views_70", 43, {0: 300, 1: 300}, {0: 70, 1: 2}, 2, depth=False, min_visible=100),
}
LIFT_CASES = tuple(_LIFT_BUILDERS)
_LIFT_CASES = {}
HIDDEN_AT_LEAST, VISIBLE_AT_LEAST = 0.10, 0.25


def lift_case(name):
    """a lift_batched_cases.Case without depth maps"""
    if name not in _LIFT_CASES:
        _LIFT_CASES[name] = _LIFT_BUILDERS[name]()
    return _LIFT_CASES[name]


_LIFT_DEPTHS = {}


def lift_depth(name):
    """the reference's rendered depth of a lift case, f64 [V,H,W]; shared, read-only"""
    if name not in _LIFT_DEPTHS:
        _LIFT_DEPTHS[name] = render(of_lift_case(lift_case(name)))
        _LIFT_DEPTHS[name].setflags(write=False)
    return _LIFT_DEPTHS[name]


def with_depth(c, depth):
    """the lift case c with depth maps: a lift_batched_cases.Case that its reference machinery takes"""
    return lb.Case(c.name + "+rendered", c.points, c.maps, c.view_entry, c.w2c, c.intr, depth, (c.H, c.W), c.mode, cut=c.cut, tau=c.tau,
                   min_visible=c.min_visible, max_visible=c.max_visible)
