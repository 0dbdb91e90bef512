"""Cases for sparse.lift_labels (csrc/lift_labels.hip) and their reference.  numpy on the CPU, no device code.

The reference goes through a batch one entry at a time with the oracle's own pieces, as tests/lift_batched_cases.py does:
oracle.project.compute_mapping_scannet(w2c.T, ...) for every view of the entry (depth None, a map, or the string "render": the oracle
then renders the z-buffer from the entry's points itself), the ascending visible lists, the loader's drop rule, then the vote with
np.bincount over (point, class), np.argmax (the lowest index among equal counts) and the fill with oracle.lift.nn1_indices_bruteforce
(the lowest index among equal distances) on the fp32 xyz.  Everything is integer: every comparison with it is array_equal.

Geometry comes from tests/lift_batched_cases.py: its generic scenes (cameras near the identity, images of at most 16 x 12) and its
edge cases on exact arithmetic (identity cameras, power-of-two focals, dyadic coordinates: a projection at x.5 or a depth test at
equality is one in the oracle, in the restatement and in the kernel alike).
"""
import numpy as np

import lift_batched_cases as lb
from oracle import lift as olift
from oracle import project as oproj

f32, f64 = np.float32, np.float64
RENDER = "render"
MAX_CLASSES = 1024


class Case:
    """points f64 [N,4]; labels integer [V,H,W]; view_entry i64 [V]; w2c f64 [V,4,4]; intr f64 [V,4]; depth f64 [V,H,W], None or
    "render"; C classes; ignore: the ignore_labels; unlabeled."""

    def __init__(self, name, points, labels, view_entry, w2c, intr, C, depth=None, ignore=(255,), unlabeled=255, cut=0, tau=0.25,
                 min_visible=0, max_visible=None, **notes):
        self.name, self.C, self.ignore, self.unlabeled = name, int(C), tuple(ignore), unlabeled
        self.cut, self.tau, self.min_visible, self.max_visible = cut, tau, min_visible, max_visible
        self.points = np.ascontiguousarray(points, f64)
        self.labels = np.ascontiguousarray(labels)
        self.view_entry = np.ascontiguousarray(view_entry, np.int64)
        self.w2c, self.intr = np.ascontiguousarray(w2c, f64), np.ascontiguousarray(intr, f64)
        self.V, self.H, self.W = self.labels.shape
        self.depth = depth if depth is None or isinstance(depth, str) else np.ascontiguousarray(depth, f64)
        self.N = len(self.points)
        self.notes = notes
        assert self.labels.dtype in (np.uint8, np.int16, np.int32, np.int64)
        assert self.points.shape == (self.N, 4) and self.view_entry.shape == (self.V,) and self.w2c.shape == (self.V, 4, 4)
        assert self.intr.shape == (self.V, 4) and (self.depth is None or isinstance(self.depth, str) or self.depth.shape == self.labels.shape)
        assert self.H <= 12 and self.W <= 16 and 1 <= self.C <= MAX_CLASSES and not 0 <= unlabeled < self.C

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
    def __init__(self, **kw):
        self.__dict__.update(kw)


def keep_rule(c, n_v):
    return n_v != 0 and n_v >= c.min_visible and (c.max_visible is None or n_v <= c.max_visible)


def visible_list(c, v, xyz):
    """the oracle's mapping of view v over the points xyz f64 [n,3] -> (ascending point ids, pixel rows, pixel columns)"""
    depth = c.depth if c.depth is None or isinstance(c.depth, str) else c.depth[v]
    with np.errstate(all="ignore"):
        mapping, _ = oproj.compute_mapping_scannet(c.w2c[v].T, xyz, depth, c.K(v), (c.W, c.H), c.cut, c.tau)
    pt = np.nonzero(mapping[:, 2] == 1)[0]
    return pt, mapping[pt, 0], mapping[pt, 1]


_REFERENCES = {}


def reference(name):
    """computed once per case and shared: callers must not change it"""
    if name not in _REFERENCES:
        _REFERENCES[name] = _reference(case(name))
    return _REFERENCES[name]


def _reference(c, views=None):
    """views: the view indices that take part, default all (a stream's prefix is lift_labels on the chunks so far)"""
    N, C = c.N, c.C
    part = np.ones(c.V, bool) if views is None else np.isin(np.arange(c.V), views)
    votes = np.zeros((N, C), np.int32)
    count = np.zeros(N, np.int32)
    view_count, view_keep = np.zeros(c.V, np.int64), np.zeros(c.V, bool)
    labels = np.full(N, c.unlabeled, np.int64)
    filled_from = np.full(N, -1, np.int64)
    out_of_range = 0
    for b in c.entries():
        rows = c.rows_of(b)
        xyz = c.points[rows, 1:]
        n = len(rows)
        ev = np.zeros((n, C), np.int64)
        for v in c.views_of(b):
            if not part[v]:
                continue
            pt, r, q = visible_list(c, v, xyz)
            view_count[v], view_keep[v] = len(pt), keep_rule(c, len(pt))
            if not view_keep[v]:
                continue
            count[rows[pt]] += 1
            lab = c.labels[v, r, q].astype(np.int64)
            live = ~np.isin(lab, c.ignore)
            bad = live & ((lab < 0) | (lab >= C))
            out_of_range += int(bad.sum())
            ok = live & ~bad
            ev += np.bincount(pt[ok] * C + lab[ok], minlength=n * C).reshape(n, C)
        votes[rows] = ev
        s = ev.sum(1) > 0
        el = np.where(s, np.argmax(ev, 1), c.unlabeled)
        labels[rows] = el
    plain = labels.copy()
    voted = votes.sum(1).astype(np.int32)
    for b in c.entries():
        rows = c.rows_of(b)
        s = voted[rows] > 0
        if s.any() and (~s).any():
            xyz32 = c.points[rows, 1:].astype(f32)
            ref_idx, qry_idx = np.nonzero(s)[0], np.nonzero(~s)[0]
            j = olift.nn1_indices_bruteforce(xyz32[s], xyz32[~s])
            labels[rows[qry_idx]] = plain[rows[ref_idx[j]]]
            filled_from[rows[qry_idx]] = rows[ref_idx[j]]
    return Reference(labels=labels, labels_unfilled=plain, votes=votes, voted=voted, seen=count > 0, count=count, view_count=view_count[part],
                     view_keep=view_keep[part], filled_from=filled_from, out_of_range=out_of_range)


def prefix_reference(c, views):
    """the reference over the views `views` (ascending view indices) alone"""
    return _reference(c, np.asarray(views))


# ------------------------------------------------------------------------------------------ an independent whole-batch restatement
def rendered(c):
    """fusion_util.py:126-130 as the sequential loop it is, per view over the points of its entry -- none of the oracle's functions"""
    out = np.full((c.V, c.H, c.W), 999999.0)
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
                if p2 > 0.2 and c.cut <= u < c.W - c.cut and c.cut <= t < c.H - c.cut and out[v, t, u] > p2:
                    out[v, t, u] = p2
    return out


def restatement(c):
    """The vote written once more, over the whole batch at once with dense (point, view) tables and explicit loops -- no per-entry
    pass, no bincount, no argmax, none of the oracle's functions.  -> Reference"""
    N, V, H, W, C = c.N, c.V, c.H, c.W, c.C
    x, y, z = c.points[:, 1], c.points[:, 2], c.points[:, 3]
    depth = rendered(c) if isinstance(c.depth, str) else c.depth
    mine = c.points[:, 0][:, None] == c.view_entry[None, :]
    vis = np.zeros((N, V), bool)
    lab = np.zeros((N, V), np.int64)
    with np.errstate(all="ignore"):
        for v in range(V):
            M, (fx, fy, cx, cy) = c.w2c[v], c.intr[v]
            p = [M[a, 0] * x + M[a, 1] * y + M[a, 2] * z + M[a, 3] for a in range(3)]
            u, t = np.round(p[0] * fx / p[2] + cx), np.round(p[1] * fy / p[2] + cy)
            ok = np.isfinite(u) & np.isfinite(t)
            u, t = np.where(ok, u, -1).astype(np.int64), np.where(ok, t, -1).astype(np.int64)
            ok &= (u >= c.cut) & (t >= c.cut) & (u < W - c.cut) & (t < H - c.cut)
            if depth is None:
                ok &= p[2] > 0
            else:
                d = depth[v][np.where(ok, t, 0), np.where(ok, u, 0)]
                ok &= np.abs(d - p[2]) <= c.tau * d
            vis[:, v] = ok & mine[:, v]
            lab[:, v] = c.labels[v][np.where(ok, t, 0), np.where(ok, u, 0)]
    view_count = vis.sum(0)
    view_keep = np.array([keep_rule(c, int(n)) for n in view_count], bool)
    use = vis & view_keep[None, :]
    count = use.sum(1).astype(np.int32)
    votes = np.zeros((N, C), np.int32)
    out_of_range = 0
    for p in range(N):
        for v in np.nonzero(use[p])[0]:
            a = int(lab[p, v])
            if a in c.ignore:
                continue
            if 0 <= a < C:
                votes[p, a] += 1
            else:
                out_of_range += 1
    voted = np.zeros(N, np.int32)
    plain = np.full(N, c.unlabeled, np.int64)
    for p in range(N):
        best, arg = 0, c.unlabeled
        for k in range(C):
            voted[p] += votes[p, k]
            if votes[p, k] > best:                                              # strict: the lowest class among equal counts
                best, arg = votes[p, k], k
        plain[p] = arg
    filled_from = np.full(N, -1, np.int64)
    xyz = c.points[:, 1:].astype(f32).astype(f64)
    has = voted > 0
    for p in np.nonzero(~has)[0]:
        best, src = np.inf, -1
        for r in np.nonzero(has & (c.points[:, 0] == c.points[p, 0]))[0]:        # ascending row: the first strict minimum is the lowest row
            dx, dy, dz = xyz[p] - xyz[r]
            d2 = (dx * dx + dy * dy) + dz * dz
            if d2 < best:
                best, src = d2, r
        filled_from[p] = src
    labels = plain.copy()
    labels[filled_from >= 0] = plain[filled_from[filled_from >= 0]]
    return Reference(labels=labels, labels_unfilled=plain, votes=votes, voted=voted, seen=count > 0, count=count, view_count=view_count,
                     view_keep=view_keep, filled_from=filled_from, out_of_range=out_of_range)


# ------------------------------------------------------------------------------------------ label maps
def random_maps(rng, V, H, W, C, dtype=np.uint8, ignore_value=None, ignore_frac=0.0):
    maps = rng.integers(0, C, (V, H, W))
    maps = np.where(rng.random((V, H, W)) < 0.15, C - 1, maps).astype(dtype)     # the last class often enough to be voted for
    if ignore_value is not None and ignore_frac > 0:
        maps[rng.random((V, H, W)) < ignore_frac] = ignore_value
    return maps


def generic(name, seed, sizes, views, C, *, dtype=np.uint8, depth="tensor", ignore_frac=0.1, ignore=(255,), unlabeled=255, **kw):
    """lift_batched_cases.generic's geometry (rows shuffled, views interleaved over the entries) under random label maps, a tenth of the
    pixels ignored"""
    g = lb.generic(name, seed, sizes, views, 1, depth=depth == "tensor", **kw)
    rng = np.random.default_rng(1000 + seed)
    maps = random_maps(rng, g.V, g.H, g.W, C, dtype, ignore[0] if ignore else None, ignore_frac)
    return Case(name, g.points, maps, g.view_entry, g.w2c, g.intr, C, RENDER if depth == RENDER else g.depth, ignore, unlabeled, g.cut, g.tau,
                g.min_visible, g.max_visible)


def of_lift(name, lift_name, C, seed, *, ignore_frac=0.0, **notes):
    """the geometry of a lift_batched_cases edge case (pixels, depth, drop rule, fill) under random label maps"""
    g = lb.case(lift_name)
    rng = np.random.default_rng(2000 + seed)
    maps = random_maps(rng, g.V, g.H, g.W, C, np.uint8, 255, ignore_frac)
    return Case(name, g.points, maps, g.view_entry, g.w2c, g.intr, C, g.depth, (255,), 255, g.cut, g.tau, g.min_visible, g.max_visible,
                **{**g.notes, **notes})


# ------------------------------------------------------------------------------------------ votes at their edges, on exact arithmetic
TIE_ROWS = ("tie_63_64", "only_64", "tie_0_64", "all_ignored", "half_to_even", "behind", "outside")


def case_ties():
    """One entry, four identity views of focal 8 on 16 x 12 (u = 8 x / z + 8, v = 8 y / z + 6), C = 65, no depths; a second entry of one
    point rides along.  Every view sees a point at the same pixel, the label maps differ per view:
      tie_63_64    pixel (row 4, column 3) holds 63, 64, 64, 63: two votes each -- classes 63 and 64 lie in different lanes of the
                   read-back (63 and 0) and on either side of the 64-class stride; the lowest class, 63, wins
      only_64      (4, 4) holds 64 four times: the class C - 1
      tie_0_64     (4, 5) holds 0, 64, 64, 0: the same lane, consecutive strides; 0 wins
      all_ignored  (4, 6) holds 255 four times: seen by four views, no vote
      half_to_even u = 4.5 exactly -> column 4 (row 5), which holds 7; column 5 holds 9
      behind       z = -1: unseen
      outside      u = 20: unseen
    The unvoted rows (all_ignored, behind, outside) are filled inside the entry; the fill's own tie is case "fill"."""
    W, H, C = 16, 12, 65
    at = lambda u, v, z=1.0: ((u - 8) * z / 8, (v - 6) * z / 8, z)              # noqa: E731
    pts = [(0.0, *at(3, 4)), (0.0, *at(4, 4)), (0.0, *at(5, 4)), (0.0, *at(6, 4)), (0.0, *at(4.5, 5)), (0.0, *at(9, 6, -1.0)),
           (0.0, *at(20, 4)), (3.0, *at(3, 4))]
    maps = np.full((5, H, W), 1, np.uint8)
    for v, (a, b, d) in enumerate(((63, 64, 0), (64, 64, 64), (64, 64, 64), (63, 64, 0))):
        maps[v, 4, 3], maps[v, 4, 4], maps[v, 4, 5], maps[v, 4, 6] = a, b, d, 255
        maps[v, 5, 4], maps[v, 5, 5] = 7, 9
    maps[4, 4, 3] = 33                                                           # entry 3's only view
    M, K = lb._identity_views(5, 8.0, W, H)
    return Case("ties", np.array(pts, f64), maps, [0, 0, 0, 0, 3], M, K, C, row_names=TIE_ROWS + ("other_entry",))


def case_dtype(dtype):
    """One geometry and one set of labels in each of the four dtypes: the ignored pixels hold 255 in the uint8 maps and -1 (a negative
    value) in the signed ones, ignore_labels = (255, -1) for all four, so the results are equal"""
    base = generic("dtype", 31, {0: 70, 1: 90}, {0: 5, 1: 4}, 200, ignore_frac=0.0)
    rng = np.random.default_rng(32)
    hole = rng.random(base.labels.shape) < 0.15
    maps = base.labels.astype(dtype)
    maps[hole] = 255 if dtype == np.uint8 else -1
    return Case(f"dtype_{np.dtype(dtype).name}", base.points, maps, base.view_entry, base.w2c, base.intr, 200, base.depth, (255, -1), 255,
                holes=int(hole.sum()))


def sampled_pixels(c):
    """bool [V,H,W]: the pixels some point of the view's entry is visible at in a kept view (what the vote reads and counts)"""
    hit = np.zeros((c.V, c.H, c.W), bool)
    for b in c.entries():
        xyz = c.points[c.rows_of(b), 1:]
        for v in c.views_of(b):
            pt, r, q = visible_list(c, v, xyz)
            if keep_rule(c, len(pt)):
                hit[v, r, q] = True
    return hit


def case_out_of_range(sampled):
    """Values outside 0..C-1 that are not ignored: at three SAMPLED pixels (C, 254 and -- int16 maps -- a negative value: the call is
    refused and says how many samples hit them) or at every UNSAMPLED pixel (no error: what is never read is never judged)"""
    base = generic("oor", 33, {0: 80, 1: 60}, {0: 3, 1: 3}, 100, dtype=np.int16, cut=2)
    hit = sampled_pixels(base)
    maps = base.labels.copy()
    if sampled:
        where = np.argwhere(hit)[[0, len(np.argwhere(hit)) // 2, -1]]
        for (v, r, q), value in zip(where, (100, 254, -7)):
            maps[v, r, q] = value
    else:
        maps[~hit] = np.where(np.arange((~hit).sum()) % 2 == 0, 100, -7).astype(np.int16)
    return Case("out_of_range_sampled" if sampled else "out_of_range_unsampled", base.points, maps, base.view_entry, base.w2c, base.intr, 100,
                base.depth, (255,), 255, cut=2)


def case_fill():
    """lift_batched_cases' fill case (the (d^2, row) tie, the nearer point of another entry, entries fully voted, never voted and
    without views) under label maps whose pixels all differ, so a wrong source shows as a wrong label"""
    g = lb.case("fill")
    maps = ((np.arange(g.H * g.W).reshape(g.H, g.W)[None] + 7 * np.arange(g.V)[:, None, None]) % 200).astype(np.uint8)
    return Case("fill", g.points, maps, g.view_entry, g.w2c, g.intr, 200, None, (255,), 255, g.cut, **g.notes)


_BUILDERS = {
    # views per entry: 0, 1, 63 / 64, 65 / 130 (+2), view_entry interleaved; classes 1, 2, 63, 64, 65, 200, 1024
    "views_0_1_63": lambda: generic("views_0_1_63", 1, {0: 40, 1: 50, 2: 120}, {1: 1, 2: 63}, 20),
    "views_64_65_C2": lambda: generic("views_64_65_C2", 2, {0: 90, 1: 110}, {0: 64, 1: 65}, 2),
    "views_130_C200": lambda: generic("views_130_C200", 3, {0: 60, 1: 300}, {0: 2, 1: 130}, 200),
    "C1": lambda: generic("C1", 4, {0: 60, 1: 50}, {0: 3, 1: 4}, 1, ignore_frac=0.4),
    "C63": lambda: generic("C63", 5, {0: 60, 1: 50}, {0: 5, 1: 4}, 63),
    "C64": lambda: generic("C64", 6, {0: 60, 1: 50}, {0: 5, 1: 4}, 64),
    "C65": lambda: generic("C65", 7, {0: 60, 1: 50}, {0: 5, 1: 4}, 65),
    "C1024": lambda: generic("C1024", 8, {0: 60, 1: 50}, {0: 5, 1: 70}, 1024, dtype=np.int16, ignore=(-1,), unlabeled=-1),
    "ties": case_ties,
    # label dtypes, a negative value in the signed ones
    "dtype_uint8": lambda: case_dtype(np.uint8),
    "dtype_int16": lambda: case_dtype(np.int16),
    "dtype_int32": lambda: case_dtype(np.int32),
    "dtype_int64": lambda: case_dtype(np.int64),
    # ignore and range
    "out_of_range_sampled": lambda: case_out_of_range(True),
    "out_of_range_unsampled": lambda: case_out_of_range(False),
    # entries and rows
    "entries": lambda: generic("entries", 18, {0: 1, 2: 45, 65535: 30}, {0: 2, 2: 3, 65535: 2}, 20),
    "odd_u8": lambda: generic("odd_u8", 21, {0: 60, 1: 50}, {0: 2, 1: 1}, 20, hw=(11, 15)),        # 3 x 11 x 15 bytes: an odd length
    "clean": lambda: generic("clean", 22, {0: 80, 1: 70}, {0: 65, 1: 3}, 64, ignore_frac=0.0),      # no ignored pixel anywhere
    "twins": lambda: of_lift("twins", "twins", 20, 14, ignore_frac=0.1),
    # visibility edges, depth kinds, the drop rule, the fill
    "pixels": lambda: of_lift("pixels", "pixels", 200, 11),
    "pixels_depth": lambda: of_lift("pixels_depth", "pixels_depth", 200, 12),
    "no_depth": lambda: generic("no_depth", 19, {0: 50, 1: 60}, {0: 3, 1: 2}, 20, depth=None, cut=2),
    "render": lambda: generic("render", 20, {0: 150, 1: 120}, {0: 4, 1: 3}, 20, depth=RENDER),
    "drop": lambda: of_lift("drop", "drop", 20, 13),
    "fill": case_fill,
}
CASES = tuple(_BUILDERS)
DTYPES = ("dtype_uint8", "dtype_int16", "dtype_int32", "dtype_int64")
_CASES = {}
# the large geometries of tests/lift_batched_cases.py (more than one fill block, LDS trip and count trip) under random label maps with a
# tenth of the pixels ignored, so "voted" -- the fill's reference mask here -- is not "seen": reachable through case() and reference(),
# not in CASES -- restatement() is not for them
_LARGE_BUILDERS = {"fill_blocks": lambda: of_lift("fill_blocks", "fill_blocks", 5, 41, ignore_frac=0.1),
                   "walk_trips": lambda: of_lift("walk_trips", "walk_trips", 7, 42, ignore_frac=0.1)}
LARGE = tuple(_LARGE_BUILDERS)
_BUILDERS.update(_LARGE_BUILDERS)


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]
