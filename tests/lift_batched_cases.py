"""Cases for sparse.lift (csrc/lift_batched.hip) and their reference.  numpy / torch on the CPU, no device code.

The reference states the lift per batch entry with the oracle's own pieces, one scene at a time -- exactly what the batched call
replaces: oracle.project.compute_mapping_scannet(w2c.T, ...) for every view of the entry, the ascending visible lists, the loader's
drop rule (n_v != 0 and min_visible <= n_v <= max_visible), then oracle.lift.lift_dense ("nearest") or lift_lseg ("bilinear") over the
kept views, the scene-level fill redone with nn1_indices_bruteforce (the lowest index among equal distances) on the fp32 xyz.

Generic scenes: a camera near the origin looking down +z (a small rotation about z, a small translation), points at z in 0.5 .. 3,
images of at most 16 x 12, focal 10 at that size; depth maps around 1.75 with vis_thres 0.25 see the points at 1.31 .. 2.19 only, so
entries hold seen and unseen points.  The edge cases (pixels, depth, drop rule, fill) use identity cameras, power-of-two focals and
dyadic coordinates: every product, quotient and sum of the projection is exact in fp64 whatever the order of the operations, so a
projection "at x.5" or a depth test "at equality" is one in the oracle, in the restatement and in the kernel alike.
"""
import numpy as np
import torch

from oracle import lift as olift
from oracle import project as oproj

f32, f64 = np.float32, np.float64
MAX_ENTRIES = 65536


class Case:
    """points f64 [N,4]; maps f32 [V,D,h,w]; view_entry i64 [V]; w2c f64 [V,4,4]; intr f64 [V,4]; depth f64 [V,H,W] or None"""

    def __init__(self, name, points, maps, view_entry, w2c, intr, depth=None, image_shape=None, mode="nearest", cut=0, tau=0.25,
                 min_visible=0, max_visible=None, **notes):
        self.name, self.mode, self.cut, self.tau, self.min_visible, self.max_visible = name, mode, cut, tau, min_visible, max_visible
        self.points = np.ascontiguousarray(points, f64)
        self.maps = np.ascontiguousarray(maps, f32)
        self.view_entry = np.ascontiguousarray(view_entry, np.int64)
        self.w2c, self.intr = np.ascontiguousarray(w2c, f64), np.ascontiguousarray(intr, f64)
        self.V, self.D, self.h, self.w = self.maps.shape
        self.H, self.W = (self.h, self.w) if image_shape is None else image_shape
        self.depth = None if depth is None else np.ascontiguousarray(depth, f64)
        self.N = len(self.points)
        self.notes = notes
        assert self.points.shape == (self.N, 4) and self.view_entry.shape == (self.V,) and self.w2c.shape == (self.V, 4, 4)
        assert self.intr.shape == (self.V, 4) and (self.depth is None or self.depth.shape == (self.V, self.H, self.W))
        assert self.H <= 12 and self.W <= 16

    def entries(self):
        return np.unique(self.points[:, 0]).astype(np.int64)

    def rows_of(self, b):
        return np.nonzero(self.points[:, 0] == b)[0]

    def views_of(self, b):
        return np.nonzero(self.view_entry == b)[0]

    def K(self, v):
        fx, fy, cx, cy = self.intr[v]
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f64)


class Reference:
    def __init__(self, features, seen, count, view_count, view_keep, filled_from, lists):
        self.features, self.seen, self.count, self.view_count, self.view_keep = features, seen, count, view_count, view_keep
        self.filled_from, self.lists = filled_from, lists


def visible_list(c, v, xyz):
    """the oracle's mapping of view v over the points xyz f64 [n,3] -> (ascending point ids, pixel rows, pixel columns)"""
    with np.errstate(all="ignore"):
        mapping, _ = oproj.compute_mapping_scannet(c.w2c[v].T, xyz, None if c.depth is None else c.depth[v], c.K(v), (c.W, c.H), c.cut, c.tau)
    pt = np.nonzero(mapping[:, 2] == 1)[0]
    return pt, mapping[pt, 0], mapping[pt, 1]


def keep_rule(c, n_v):
    return n_v != 0 and n_v >= c.min_visible and (c.max_visible is None or n_v <= c.max_visible)


_REFERENCES = {}


def reference(name):
    """computed once per case and shared: callers must not change it"""
    if name not in _REFERENCES:
        _REFERENCES[name] = _reference(case(name))
    return _REFERENCES[name]


def _reference(c):
    feats = np.zeros((c.N, c.D), f32)
    seen, count = np.zeros(c.N, bool), np.zeros(c.N, np.int32)
    view_count, view_keep = np.zeros(c.V, np.int64), np.zeros(c.V, bool)
    filled_from = np.full(c.N, -1, np.int64)
    lists = {}
    for b in c.entries():
        rows, vs = c.rows_of(b), c.views_of(b)
        xyz = c.points[rows, 1:]
        kept = []
        for v in vs:
            pt, x, y = visible_list(c, v, xyz)
            lists[int(v)] = (rows[pt], x, y)
            view_count[v] = len(pt)
            view_keep[v] = keep_rule(c, len(pt))
            if view_keep[v]:
                kept.append((v, pt, x, y))
                count[rows[pt]] += 1
        if not kept:
            continue
        maps = [torch.from_numpy(c.maps[v]) for v, _, _, _ in kept]
        pts, xs, ys = ([torch.from_numpy(np.asarray(k[i], np.int64)) for k in kept] for i in (1, 2, 3))
        coords32 = torch.from_numpy(xyz.astype(f32))
        if c.mode == "nearest":
            out, s = olift.lift_dense(maps, pts, xs, ys, coords32)
        else:
            out, s = olift.lift_lseg(maps, (c.H, c.W), pts, xs, ys, coords32)
        out, s = out.numpy().copy(), s.numpy().copy()
        if s.any() and (~s).any():
            # the fill again, with the lowest index among equal distances (the oracle's KDTree names no rule for them)
            ref_idx, qry_idx = np.nonzero(s)[0], np.nonzero(~s)[0]
            j = olift.nn1_indices_bruteforce(coords32.numpy()[s], coords32.numpy()[~s])
            out[qry_idx] = out[ref_idx[j]]
            filled_from[rows[qry_idx]] = rows[ref_idx[j]]
        feats[rows], seen[rows] = out, s
    return Reference(feats, seen, count, view_count, view_keep, filled_from, lists)


# ------------------------------------------------------------------------------------------ an independent whole-batch restatement
def restatement(c):
    """The lift written once more, over the whole batch at once with dense (point, view) tables and explicit loops -- no per-entry
    pass, none of the oracle's functions.  -> (features f64 [N,D] for "bilinear", f32 for "nearest", seen, count, view_count,
    view_keep, filled_from)"""
    N, V, H, W = c.N, c.V, c.H, c.W
    x, y, z = c.points[:, 1], c.points[:, 2], c.points[:, 3]
    mine = c.points[:, 0][:, None] == c.view_entry[None, :]                     # [N, V]: the view looks at the point's entry
    vis = np.zeros((N, V), bool)
    prow, pcol = np.zeros((N, V), np.int64), np.zeros((N, V), np.int64)
    with np.errstate(all="ignore"):
        for v in range(V):
            M, (fx, fy, cx, cy) = c.w2c[v], c.intr[v]
            p = [M[a, 0] * x + M[a, 1] * y + M[a, 2] * z + M[a, 3] for a in range(3)]
            u, t = np.round(p[0] * fx / p[2] + cx), np.round(p[1] * fy / p[2] + cy)
            ok = np.isfinite(u) & np.isfinite(t)
            u, t = np.where(ok, u, -1).astype(np.int64), np.where(ok, t, -1).astype(np.int64)
            ok &= (u >= c.cut) & (t >= c.cut) & (u < W - c.cut) & (t < H - c.cut)
            if c.depth is None:
                ok &= p[2] > 0
            else:
                d = c.depth[v][np.where(ok, t, 0), np.where(ok, u, 0)]
                ok &= np.abs(d - p[2]) <= c.tau * d
            vis[:, v], prow[:, v], pcol[:, v] = ok & mine[:, v], t, u
    view_count = vis.sum(0)
    view_keep = np.array([keep_rule(c, int(n)) for n in view_count])
    use = vis & view_keep[None, :]
    count = use.sum(1).astype(np.int32)
    seen = count > 0
    acc_t = f32 if c.mode == "nearest" else f64
    feats = np.zeros((N, c.D), acc_t)
    maps = c.maps.astype(acc_t)
    for p in range(N):
        acc = np.zeros(c.D, acc_t)
        for v in np.nonzero(use[p])[0]:                                         # ascending view index
            if c.mode == "nearest":
                acc = acc + maps[v, :, prow[p, v], pcol[p, v]]
            else:
                acc = acc + bilinear_at(maps[v], prow[p, v], pcol[p, v], H, W)
        feats[p] = acc / (acc_t(count[p]) if count[p] else acc_t(1e-6))
    filled_from = np.full(N, -1, np.int64)
    xyz = c.points[:, 1:].astype(f32).astype(f64)
    for p in np.nonzero(~seen)[0]:
        best, src = np.inf, -1
        for r in np.nonzero(seen & (c.points[:, 0] == c.points[p, 0]))[0]:      # ascending row: the first strict minimum is the lowest row
            dx, dy, dz = xyz[p] - xyz[r]
            d2 = (dx * dx + dy * dy) + dz * dz
            if d2 < best:
                best, src = d2, r
        filled_from[p] = src
    out = feats.copy()
    out[filled_from >= 0] = feats[filled_from[filled_from >= 0]]
    return out, seen, count, view_count, view_keep, filled_from


def bilinear_at(m, row, col, H, W):
    """F.interpolate(bilinear, align_corners=True) of m f64 [D,h,w] to (H, W) at one pixel, in fp64"""
    _, h, w = m.shape
    sy = (h - 1) / (H - 1) * row if H > 1 else 0.0
    sx = (w - 1) / (W - 1) * col if W > 1 else 0.0
    r0, c0 = min(int(np.floor(sy)), h - 1), min(int(np.floor(sx)), w - 1)
    r1, c1 = min(r0 + 1, h - 1), min(c0 + 1, w - 1)
    ly, lx = sy - r0, sx - c0
    top = (1 - lx) * m[:, r0, c0] + lx * m[:, r0, c1]
    bot = (1 - lx) * m[:, r1, c0] + lx * m[:, r1, c1]
    return (1 - ly) * top + ly * bot


# ------------------------------------------------------------------------------------------ generic scenes
def camera(rng, W=16, H=12):
    """world->camera near the identity: a rotation about z of up to 0.2 rad, a translation of up to 0.3 (0.05 along z); focal 10 at
    16 x 12, the principal point at the image centre"""
    a = rng.uniform(-0.2, 0.2)
    M = np.eye(4)
    M[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    M[:3, 3] = rng.uniform(-0.3, 0.3, 3) * [1, 1, 1 / 6]
    return M, np.array([10.0 * W / 16, 10.0 * H / 12, W / 2, H / 2])


def cloud(rng, n):
    return np.column_stack([rng.uniform(-2.4, 2.4, n), rng.uniform(-1.8, 1.8, n), rng.uniform(0.5, 3.0, n)])


def generic(name, seed, sizes, views, D, *, hw=(12, 16), image_shape=None, mode="nearest", depth=True, shuffle=True, interleave=True, **kw):
    """sizes: {batch index: points}, views: {batch index: views}.  Rows in shuffled batch order, views interleaved over the entries."""
    rng = np.random.default_rng(seed)
    H, W = hw if image_shape is None else image_shape
    pts = np.vstack([np.column_stack([np.full(n, b, f64), cloud(rng, n)]) for b, n in sizes.items()])
    if shuffle:
        pts = pts[rng.permutation(len(pts))]
    ve = np.concatenate([np.full(n, b, np.int64) for b, n in views.items()])
    if interleave:
        ve = ve[rng.permutation(len(ve))]
    cams = [camera(rng, W, H) for _ in ve]
    V = len(ve)
    maps = rng.uniform(-1, 1, (V, D) + tuple(hw)).astype(f32)
    dm = (1.75 + rng.uniform(-0.3, 0.3, (V, H, W))) if depth else None
    return Case(name, pts, maps, ve, np.stack([m for m, _ in cams]), np.stack([k for _, k in cams]), dm, image_shape, mode, **kw)


# ------------------------------------------------------------------------------------------ edge cases on exact arithmetic
def _identity_views(V, fx, W, H):
    return np.tile(np.eye(4), (V, 1, 1)), np.tile(np.array([fx, fx, W / 2, H / 2], f64), (V, 1))


PIXEL_FX, PIXEL_CUT = 8.0, 2


def pixel_rows():
    """(name, x, y, z, visible without depths, visible with the depth map of case_pixels) at W = 16, H = 12, cut = 2, focal 8, centre
    (8, 6): u = 8 x / z + 8, v = 8 y / z + 6"""
    at = lambda u, v=6.0, z=1.0: ((u - 8) * z / 8, (v - 6) * z / 8, z)          # noqa: E731
    rows = [("u_on_cut", *at(2.0), True), ("u_below_cut", *at(1.0), False), ("u_last", *at(13.0), True), ("u_first_out", *at(14.0), False),
            ("v_on_cut", *at(8.0, 2.0), True), ("v_below_cut", *at(8.0, 1.0), False), ("v_last", *at(8.0, 9.0), True),
            ("v_first_out", *at(8.0, 10.0), False),
            ("half_to_even_down", *at(4.5), True), ("half_to_even_up", *at(5.5), True), ("half_onto_cut", *at(1.5), True),
            ("half_to_cut_from_above", *at(2.5), True), ("half_out", *at(13.5), False), ("half_in", *at(12.5, 8.5), True),
            ("half_z2", *at(6.5, 6.5, 2.0), True), ("behind", *at(9.0, 6.0, -1.0), False), ("on_the_camera_plane", 0.25, 0.0, 0.0, False)]
    return rows


def case_pixels(depth):
    """One entry, one identity view, one point per row of pixel_rows.  With depth: every pixel holds d = 1 (the rows at z = 1 pass the
    depth test exactly, the one at z = 2 fails it) except pixel (6, 4), where "half_to_even_down" lands only if 4.5 rounds to 4, and
    the pixels of the depth rows below; the host test pins the rows that matter."""
    W, H = 16, 12
    rows = pixel_rows()
    pts = [(0.0, x, y, z) for _, x, y, z, _ in rows]
    names = [r[0] for r in rows]
    dm = None
    if depth:
        dm = np.full((1, H, W), 1.0)
        dm[0, 6, 4] = 2.0                                                        # "half_to_even_down": |2 - 1| > 0.5
        # depth rows: pixel (row 3, columns 3..8), d = 2, tau = 0.25: |d - p_z| == tau d at p_z = 1.5 and 2.5
        extra = [("depth_equal_near", 3, 1.5, 2.0), ("depth_equal_far", 4, 2.5, 2.0), ("depth_just_past", 5, 2.5 + 2.0 ** -40, 2.0),
                 ("depth_inside", 6, 2.25, 2.0), ("depth_negative", 7, 1.0, -1.0), ("depth_negative_behind", 8, -1.0, -1.0)]
        for name, col, z, d in extra:
            dm[0, 3, col] = d
            pts.append((0.0, (col - 8) * z / 8, (3 - 6) * z / 8, z))
            names.append(name)
    rng = np.random.default_rng(11)
    maps = rng.uniform(-1, 1, (1, 3, H, W)).astype(f32)
    M, K = _identity_views(1, PIXEL_FX, W, H)
    return Case("pixels_depth" if depth else "pixels", np.array(pts, f64), maps, [0], M, K, dm, cut=PIXEL_CUT, row_names=names)


DROP_COUNTS = (9, 10, 11, 20, 21, 0)                  # min_visible = 10, max_visible = 20: kept are 10, 11, 20


def case_drop():
    """30 points at z = 1 .. 30 near the optical axis; view i is the identity moved by -(30 - n_i) - 0.5 along z, so it sees exactly the
    n_i farthest points (p_z > 0, no depths).  A second entry rides along with two ordinary views."""
    rng = np.random.default_rng(12)
    W, H = 16, 12
    z = np.arange(1, 31, dtype=f64)
    pts = np.column_stack([np.zeros(30), rng.integers(-4, 5, 30) / 64.0 * z / 8, rng.integers(-4, 5, 30) / 64.0 * z / 8, z])
    other = np.column_stack([np.full(20, 3.0), cloud(rng, 20)])
    M, K = _identity_views(len(DROP_COUNTS) + 2, 8.0, W, H)
    for i, n in enumerate(DROP_COUNTS):
        M[i, 2, 3] = -(30 - n) - 0.5
    ve = np.array([0] * len(DROP_COUNTS) + [3, 3])
    order = rng.permutation(len(ve))
    maps = rng.uniform(-1, 1, (len(ve), 5, H, W)).astype(f32)
    rows = rng.permutation(50)
    return Case("drop", np.vstack([pts, other])[rows], maps[order], ve[order], M[order], K[order], None, min_visible=10, max_visible=20,
                counts={int(np.nonzero(order == i)[0][0]): n for i, n in enumerate(DROP_COUNTS)})


def case_fill():
    """Identity cameras of focal 2 on 16 x 12 with cut 3 (columns 3 .. 12 are inside), no depths: a point is seen when p_z > 0 and it
    projects inside.  Entry 1's camera looks down -z.  Rows are listed so that the tie's two references come in DESCENDING x: the lower
    row is not the first in any geometric order.
      entry 0: refs (1,0,1) [row a], (-1,0,1) [row b > a], query (0,0,-1): d^2 = 5 to both, row a wins;
               query (0.25,0,-1): nearer to (1,0,1); a seen point of ENTRY 1 sits exactly on (0,0,-1);
               ref (2.25,0,1) projects to u = 12.5 -> 12 (inside); a query at x = 2.25 + 2^-40, u -> 13 (outside), equal to it in fp32;
      entry 1: seen (0,0,-1), (0.5,0,-1); unseen (0,0,1);
      entry 2: fully seen; entry 4: never seen (its view looks away); entry 5: points, no views."""
    W, H = 16, 12
    P = [(0, 1.0, 0.0, 1.0), (0, -1.0, 0.0, 1.0), (0, 0.0, 0.0, -1.0), (0, 0.25, 0.0, -1.0), (0, 2.25, 0.0, 1.0), (0, 2.25 + 2.0 ** -40, 0.0, 1.0),
         (1, 0.0, 0.0, -1.0), (1, 0.5, 0.0, -1.0), (1, 0.0, 0.0, 1.0),
         (2, 0.5, 0.5, 1.0), (2, -0.5, 0.25, 2.0), (2, 0.0, 0.0, 4.0),
         (4, 0.5, 0.5, -1.0), (4, -0.5, 0.25, -2.0),
         (5, 0.5, 0.5, 1.0), (5, 0.0, 0.0, 1.0)]
    ve = np.array([0, 1, 2, 4, 0])
    M, K = _identity_views(len(ve), 2.0, W, H)
    M[1, 2, 2] = -1.0
    rng = np.random.default_rng(13)
    maps = rng.uniform(-1, 1, (len(ve), 4, H, W)).astype(f32)
    return Case("fill", np.array(P, f64), maps, ve, M, K, None, cut=3,
                expect_from={2: 0, 3: 0, 5: 4, 8: 6}, tie=(2, 0, 1), coincide=(5, 4), other_entry_nearer=(2, 6))


def case_twins():
    """Two entries occupying identical world coordinates, with different views and maps, rows interleaved"""
    rng = np.random.default_rng(14)
    xyz = cloud(rng, 60)
    pts = np.vstack([np.column_stack([np.full(60, b, f64), xyz]) for b in (0, 1)])[np.arange(120).reshape(2, 60).T.reshape(-1)]
    ve = np.array([1, 0, 1, 0, 0])
    cams = [camera(rng) for _ in ve]
    maps = rng.uniform(-1, 1, (len(ve), 6, 12, 16)).astype(f32)
    dm = 1.75 + rng.uniform(-0.3, 0.3, (len(ve), 12, 16))
    return Case("twins", pts, maps, ve, np.stack([m for m, _ in cams]), np.stack([k for _, k in cams]), dm)


def col_chunk():
    """the channels one pass of the lift kernel holds in registers, asked of the library (a CPU-only host can load it)"""
    from geopurify_amd import ops
    return ops.lift_batched_col_chunk()


_BUILDERS = {
    # views per entry: 0, 1, 63 / 64, 65 / 130 (+2), view_entry interleaved
    "views_0_1_63": lambda: generic("views_0_1_63", 1, {0: 40, 1: 50, 2: 120}, {1: 1, 2: 63}, 3),
    "views_64_65": lambda: generic("views_64_65", 2, {0: 90, 1: 110}, {0: 64, 1: 65}, 1),
    "views_130": lambda: generic("views_130", 3, {0: 60, 1: 300}, {0: 2, 1: 130}, 64),
    "views_130_bilinear": lambda: generic("views_130_bilinear", 4, {0: 150, 7: 30}, {0: 130, 7: 3}, 5, hw=(5, 7), image_shape=(12, 16),
                                          mode="bilinear"),
    # widths
    "D65": lambda: generic("D65", 5, {0: 70, 1: 80}, {0: 3, 1: 4}, 65),
    "D512": lambda: generic("D512", 6, {0: 70, 1: 60}, {0: 3, 1: 2}, 512, hw=(6, 8)),
    "D_chunk_plus_1": lambda: generic("D_chunk_plus_1", 7, {0: 70, 1: 60}, {0: 3, 1: 2}, col_chunk() + 1, hw=(6, 8)),
    "D_chunk_plus_1_bilinear": lambda: generic("D_chunk_plus_1_bilinear", 8, {0: 70, 1: 60}, {0: 3, 1: 2}, col_chunk() + 1, hw=(3, 4),
                                               image_shape=(6, 8), mode="bilinear"),
    # the LSeg form at its shape edges
    "bilinear_h1": lambda: generic("bilinear_h1", 9, {0: 80, 1: 70}, {0: 3, 1: 3}, 65, hw=(1, 5), image_shape=(12, 16), mode="bilinear"),
    "bilinear_w1": lambda: generic("bilinear_w1", 10, {0: 80, 1: 70}, {0: 3, 1: 3}, 3, hw=(5, 1), image_shape=(12, 16), mode="bilinear"),
    "bilinear_ratio": lambda: generic("bilinear_ratio", 15, {0: 80, 1: 70}, {0: 4, 1: 3}, 64, hw=(5, 7), image_shape=(12, 16),
                                      mode="bilinear", depth=False),
    "bilinear_H1": lambda: generic("bilinear_H1", 16, {0: 80, 1: 70}, {0: 3, 1: 3}, 3, hw=(3, 4), image_shape=(1, 16), mode="bilinear"),
    "bilinear_W1": lambda: generic("bilinear_W1", 17, {0: 80, 1: 70}, {0: 3, 1: 3}, 3, hw=(3, 4), image_shape=(12, 1), mode="bilinear"),
    # entries
    "entries": lambda: generic("entries", 18, {0: 1, 2: 45, 65535: 30}, {0: 2, 2: 3, 65535: 2}, 3),
    "no_depth": lambda: generic("no_depth", 19, {0: 50, 1: 60}, {0: 3, 1: 2}, 3, depth=False, cut=2),
    "twins": case_twins,
    "pixels": lambda: case_pixels(False),
    "pixels_depth": lambda: case_pixels(True),
    "drop": case_drop,
    "fill": case_fill,
}
CASES = tuple(_BUILDERS)
BILINEAR = tuple(n for n in CASES if "bilinear" in n)
_CASES = {}


# ------------------------------------------------------------------------------------------ large cases: all rows and no bytes
# The shared kernels of csrc/gp_lift_entries.h, gp_lift_stream_state.h and lift_masks_batched.hip change behaviour at a size: a second
# fill block (256 queries), a second LDS trip of the fill (1024 references), a second trip of the count loops and of the ordered walk
# (16 384 rows of one entry), rows beyond the offset table's 65 538 words.  These cases reach every one of them on images of 16 x 12
# and three channels.  They are reachable through case() and reference() and are NOT in CASES: the parametrisations over CASES run
# "singles" partitions, per-scene sequences and restatement() -- a minute and more at 17 000 rows -- on every member.
FILL_BLOCK, FILL_TILE, COUNT_TRIP, WALK_PARTS, ENTRY_TABLE = 256, 1024, 64 * 256, 64, MAX_ENTRIES + 2
PLANTED_FX = 4.0


def planted(name, seed, plan, views, D=3, **kw):
    """plan = [(entry, n_seen, n_unseen), ...], views = {entry: views}.  No depth maps, identity cameras of focal 4 on 16 x 12 (as
    case_fill: a row is seen when p_z > 0 and it projects inside).  A seen row is (a z, b z, z) with z in 0.5 .. 3, |a| <= 1.5 and
    |b| <= 1: u = 4 a + 8 in 2 .. 14 and v = 4 b + 6 in 2 .. 10, clear of the image's edge (no cut) by two pixels.  An unseen row is the
    same with z in -3 .. -0.5: p_z < 0, never visible.  So every entry has exactly n_seen seen and n_unseen unseen rows whatever the
    number of its views -- or none seen if it has no view.  Rows shuffled across the entries, views interleaved, as generic does."""
    rng = np.random.default_rng(seed)
    W, H = 16, 12
    rows = []
    for b, n_seen, n_unseen in plan:
        n = n_seen + n_unseen
        z = rng.uniform(0.5, 3.0, n) * np.where(np.arange(n) < n_seen, 1.0, -1.0)
        a, t = rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n)
        rows.append(np.column_stack([np.full(n, b, f64), a * z, t * z, z]))
    pts = np.vstack(rows)
    pts = pts[rng.permutation(len(pts))]
    ve = np.concatenate([np.full(n, b, np.int64) for b, n in views.items()])
    ve = ve[rng.permutation(len(ve))]
    M, K = _identity_views(len(ve), PLANTED_FX, W, H)
    maps = rng.uniform(-1, 1, (len(ve), D, H, W)).astype(f32)
    return Case(name, pts, maps, ve, M, K, None, plan={b: (s, u) for b, s, u in plan}, **kw)


# (entry, references, queries).  Entry 2: a view and nothing before it; 3: fully seen; 6: a view and no rows; 11: rows and no view.
FILL_BLOCKS_PLAN = ((0, 61, 239), (1, 8, 32), (2, 0, 40), (3, 50, 0), (4, 9, 21), (5, 2500, 1500), (7, 1, 700), (9, 1100, 1),
                    (65535, 30, 30), (11, 0, 5))
FILL_BLOCKS_VIEWS = {0: 2, 1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 6: 1, 7: 1, 9: 1, 65535: 1}


def case_fill_blocks():
    """The scene-level fill over eleven blocks of 256 queries, the last one partial.  In the entry-sorted order the queries are 239 of
    entry 0, 32 of entry 1, 40 of entry 2 (which has no reference), 21 of entry 4, 1500 of entry 5 ...: the second block holds queries
    of entries 1, 2, 4 and 5 and streams the references of entry 3, which has none of its queries; entry 5's 2500 references take three
    LDS trips.  tests/test_lift_batched_cases_host.py asserts all of it from the reference."""
    return planted("fill_blocks", 31, FILL_BLOCKS_PLAN, FILL_BLOCKS_VIEWS)


TIE_LINE, TIE_STEP, TIE_GONE = 2400, 2.0 ** -9, (301, 1203, 1801, 2049, 2255)


def case_fill_tie_trips():
    """On the exact arithmetic of case_fill (dyadic coordinates, focal 2, identity cameras, no depths).  Entry 3 holds a line of
    references at z = 1, y = 0, x_k = (k - 1200) 2^-9 for k = 0 .. 2399 without the five odd k of TIE_GONE: u = 2 x + 8 in 3.3 .. 12.7,
    all seen.  The rows list the even k first and then the odd ones, so spatial neighbours lie about 1200 references apart: in
    different LDS trips of 1024.  A query sits at z = -1 (unseen) exactly midway between x_k and x_k+1: d^2 = 4 + 2^-20 to both, exactly,
    and the lower row -- the even k, an earlier trip -- must win although the equal distance turns up a trip or two later.  The queries
    at the x of TIE_GONE lie midway between k - 1 and k + 1, consecutive references of one trip.  Entry 0, 37 rows that are all seen, comes
    first in the entry order: the block's range starts at reference 37, not 0.  The queries come first in the row order.
    notes: ties = [(query row, lower row, higher row)], same_trip = the ties at TIE_GONE."""
    W, H = 16, 12
    x_of = lambda k: (k - 1200) * TIE_STEP                                       # noqa: E731
    ks = [k for k in range(0, TIE_LINE, 2)] + [k for k in range(1, TIE_LINE, 2) if k not in TIE_GONE]
    cross = [k for k in range(7, TIE_LINE - 1, 61) if k not in TIE_GONE and k + 1 not in TIE_GONE]     # both parities of k
    queries = [(3.0, x_of(k) + TIE_STEP / 2, 0.0, -1.0) for k in cross] + [(3.0, x_of(k), 0.0, -1.0) for k in TIE_GONE]
    line = [(3.0, x_of(k), 0.0, 1.0) for k in ks]
    other = [(0.0, (j - 18) / 8.0, 0.25, 2.0) for j in range(37)]
    first = len(queries)
    row_of = {k: first + i for i, k in enumerate(ks)}
    ties = [(q, min(row_of[k], row_of[k + 1]), max(row_of[k], row_of[k + 1])) for q, k in enumerate(cross)]
    same = [(len(cross) + q, row_of[k - 1], row_of[k + 1]) for q, k in enumerate(TIE_GONE)]
    ve = np.array([3, 0, 3])
    M, K = _identity_views(len(ve), 2.0, W, H)
    rng = np.random.default_rng(33)
    maps = rng.uniform(-1, 1, (len(ve), 3, H, W)).astype(f32)
    return Case("fill_tie_trips", np.array(queries + line + other, f64), maps, ve, M, K, None, ties=ties + same, same_trip=same)


# the entry-1 views of walk_trips see 2117, 2149 and 2155 rows (tests/test_lift_batched_cases_host.py asserts the split); those among
# the entry's first 16 384 sorted rows alone are about 90 fewer, below the bound for every view
WALK_MAX_VISIBLE = 2130


def case_walk_trips():
    """An entry of 16384 + 700 rows under depth maps: the count kernels' stride loop (64 blocks of 256 rows per view) takes a second
    trip, the ordered walk of the mask lift has per = ceil(17084 / 64) = 267 > 256 rows per part -- a second trip in every part -- and
    the fill takes 60 blocks over the 2117 references that are left, three LDS trips.  max_visible = 2130 keeps the entry-1 view that
    sees 2117 rows and drops the two that see 2149 and 2155; each of them sees 2071 among the first 16 384 sorted rows, so the drop is
    decided by what the second trip counts."""
    return generic("walk_trips", 32, {0: 200, 1: COUNT_TRIP + 700, 2: 1}, {0: 2, 1: 3, 2: 1}, 3, max_visible=WALK_MAX_VISIBLE)


def case_rows_past_table():
    """n = 65538 + 300 rows: more than the 65 538 words of the offset table, so the checked copy of a stream's tables has threads that
    copy keys and rows only.  Entry 1, 65 538 rows, has no view: nothing of it is seen or filled, its reference costs nothing, and its
    rows are 257 fill blocks of queries without a reference.  Entries 0 and 2, 150 rows and two and three views each, lie on both sides
    of it in the sorted order; 240 of their rows are spread over the rows below 65 538 and 60 over those from 65 538 on."""
    n_bulk, n_small = ENTRY_TABLE, 150
    g = generic("rows_past_table", 34, {0: n_small, 1: n_bulk, 2: n_small}, {0: 2, 2: 3}, 3, shuffle=False)
    rng = np.random.default_rng(35)
    N = g.N
    at = np.sort(np.concatenate([rng.choice(ENTRY_TABLE, 240, replace=False), ENTRY_TABLE + rng.choice(N - ENTRY_TABLE, 60, replace=False)]))
    small = np.concatenate([np.arange(n_small), n_small + n_bulk + np.arange(n_small)])[rng.permutation(2 * n_small)]
    pts = np.empty_like(g.points)
    bulk_at = np.ones(N, bool)
    bulk_at[at] = False
    pts[at], pts[bulk_at] = g.points[small], g.points[n_small:n_small + n_bulk]
    return Case("rows_past_table", pts, g.maps, g.view_entry, g.w2c, g.intr, g.depth)


_LARGE_BUILDERS = {"fill_blocks": case_fill_blocks, "fill_tie_trips": case_fill_tie_trips, "walk_trips": case_walk_trips,
                   "rows_past_table": case_rows_past_table}
LARGE = tuple(_LARGE_BUILDERS)
_BUILDERS.update(_LARGE_BUILDERS)                     # (after CASES: case() and reference() find them, no parametrisation does)


def fill_blocking(c, mask):
    """The blocking of the scene-level fill (lb_fill_kernel of csrc/gp_lift_entries.h) restated: rows in the entry-sorted stable order,
    the references (mask) and the queries (not mask; every row of a case lies in a valid entry) compacted in that order, the queries
    cut into blocks of 256; a block streams the references lo .. hi, the union of the non-empty runs of its queries' entries, in trips
    of 1024 from lo.  -> (rank i64 [N]: the compacted position of a reference row, -1 for a query; blocks: a list of dicts with rows
    (the block's query rows), entry, r0, r1 (each query's run), lo, hi (None, None when no query of the block has a reference))"""
    entry = c.points[:, 0].astype(np.int64)
    order = np.argsort(entry, kind="stable")
    keys, is_ref = entry[order], np.asarray(mask, bool)[order]
    rs = np.concatenate([[0], np.cumsum(is_ref)])
    rank = np.full(c.N, -1, np.int64)
    rank[order[is_ref]] = rs[:-1][is_ref]
    qpos = np.nonzero(~is_ref)[0]
    blocks = []
    for i in range(0, len(qpos), FILL_BLOCK):
        s = qpos[i:i + FILL_BLOCK]
        b = keys[s]
        r0, r1 = rs[np.searchsorted(keys, b, "left")], rs[np.searchsorted(keys, b, "right")]
        has = r1 > r0
        blocks.append(dict(rows=order[s], entry=b, r0=r0, r1=r1, lo=int(r0[has].min()) if has.any() else None,
                           hi=int(r1[has].max()) if has.any() else None))
    return rank, blocks


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]
