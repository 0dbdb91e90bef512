"""Cases for sparse.render_rows (csrc/render_rows.hip) and their reference.  numpy on the CPU, no device code.

The rule.  A point p of view v's entry is a candidate of v when the lifts' visibility test accepts it against the chosen depth (None:
p_z > 0; "render": the view's own z-buffer; or given maps) and p_z > 0; it covers the square of side 2 * radius + 1 centred on its
pixel, clipped to [cut, H - cut) x [cut, W - cut); a pixel's owner is the covering candidate with the smallest p_z, the lowest row
among equal p_z.

The reference runs one view and one entry at a time with the oracle's own pieces -- oracle.project._project, oracle.project.render_depth
and oracle.project._finish give the candidates -- and then takes the (p_z, row) minimum over the clipped footprints.  The restatement
uses none of the oracle's functions: scalar loops over views, rows and footprint pixels.

Geometry: every case of tests/render_depth_cases.py (its cameras make p_z a single rounding, so depths compare bit for bit), and two
cases of edge rows on identity cameras of focal 8 with dyadic coordinates, the rule of the existing edge cases.
"""
import numpy as np

import lift_batched_cases as lb
import render_depth_cases as rd
from oracle import project as oproj

f64 = np.float64
FAR = rd.FAR
TAU = 0.25
KINDS = ("none", "render")                                  # the depth forms every case runs under; "sensor" where a case carries maps
RADII = (0, 1, 2, 4)


class Ref:
    """rows i32 [V,H,W] (-1: no owner), depth f64 [V,H,W] (999999 without one), view_count / pixel_count i64 [V], cands: per view the
    candidates' rows of points (ascending), contests: pixels whose smallest p_z is shared by two or more covering candidates"""

    def __init__(self, rows, depth, view_count, pixel_count, cands, contests):
        self.rows, self.depth, self.view_count, self.pixel_count, self.cands, self.contests = rows, depth, view_count, pixel_count, cands, contests


def _depth_of(kind, c):
    return None if kind == "none" else ("render" if kind == "render" else c.notes["sensor"])


def candidates(c, v, depth, tau=TAU):
    """the oracle's candidates of view v: (rows of points ascending, pixel rows, pixel columns, p_z).  depth: None, "render" or f64 [V,H,W]"""
    rows = c.rows_of(c.view_entry[v])
    if len(rows) == 0:
        return rows, rows, rows, np.zeros(0, f64)
    with np.errstate(all="ignore"):
        p, pi = oproj._project(c.w2c[v], c.points[rows, 1:], c.K(v))
        d = None if depth is None else (oproj.render_depth(p, pi, (c.W, c.H), c.cut) if isinstance(depth, str) else depth[v])
        m = oproj._finish(p, pi, (c.W, c.H), c.cut, d, tau)
        ok = (m[:, 2] == 1) & (p[2] > 0)
    return rows[ok], m[ok, 0], m[ok, 1], p[2][ok]


def render(c, depth, radius, tau=TAU):
    """the reference -> Ref.  Every (candidate, footprint pixel) pair of a view sorted by (pixel, p_z, row): the first of a pixel owns it"""
    rows_img = np.full((c.V, c.H, c.W), -1, np.int32)
    z_img = np.full((c.V, c.H, c.W), FAR)
    vc, pc, cands, contests = np.zeros(c.V, np.int64), np.zeros(c.V, np.int64), [], 0
    off = np.arange(-radius, radius + 1)
    for v in range(c.V):
        r, vi, ui, pz = candidates(c, v, depth, tau)
        cands.append(r)
        vc[v] = len(r)
        if len(r) == 0:
            continue
        y = (vi[:, None, None] + off[None, :, None]) + 0 * off[None, None, :]
        x = (ui[:, None, None] + off[None, None, :]) + 0 * off[None, :, None]
        inside = (y >= c.cut) & (y < c.H - c.cut) & (x >= c.cut) & (x < c.W - c.cut)
        pix = (y * c.W + x)[inside]
        rr = np.broadcast_to(r[:, None, None], y.shape)[inside]
        zz = np.broadcast_to(pz[:, None, None], y.shape)[inside]
        order = np.lexsort((rr, zz, pix))
        pix, rr, zz = pix[order], rr[order], zz[order]
        first = np.ones(len(pix), bool)
        first[1:] = pix[1:] != pix[:-1]
        rows_img[v].reshape(-1)[pix[first]] = rr[first]
        z_img[v].reshape(-1)[pix[first]] = zz[first]
        pc[v] = int(first.sum())
        second = np.zeros(len(pix), bool)
        second[1:] = first[:-1] & ~first[1:] & (zz[1:] == zz[:-1])
        contests += int(second.sum())
    return Ref(rows_img, z_img, vc, pc, cands, contests)


_REFERENCES = {}


def reference(name, kind, radius):
    """computed once per (case, depth form, radius) and shared: callers must not change it"""
    key = (name, kind, radius)
    if key not in _REFERENCES:
        c = case(name)
        ref = render(c, _depth_of(kind, c), radius)
        for a in (ref.rows, ref.depth, ref.view_count, ref.pixel_count):
            a.setflags(write=False)
        _REFERENCES[key] = ref
    return _REFERENCES[key]


def restatement(c, depth, radius, tau=TAU):
    """The rule once more as the sequential loops it is, with none of the oracle's functions -> (rows, depth, view_count, pixel_count)"""
    rows_img = np.full((c.V, c.H, c.W), -1, np.int64)
    z_img = np.full((c.V, c.H, c.W), FAR)
    vc, pc = np.zeros(c.V, np.int64), np.zeros(c.V, np.int64)
    with np.errstate(all="ignore"):
        for v in range(c.V):
            M, (fx, fy, cx, cy) = c.w2c[v], c.intr[v]
            proj = []
            for r in c.rows_of(c.view_entry[v]):
                x, y, z = c.points[r, 1:]
                p0, p1, p2 = (M[a, 0] * x + M[a, 1] * y + M[a, 2] * z + M[a, 3] for a in range(3))
                u, t = np.round(p0 * fx / p2 + cx), np.round(p1 * fy / p2 + cy)
                if not (np.isfinite(u) and np.isfinite(t)):
                    continue
                u, t = int(u), int(t)
                if u >= c.cut and t >= c.cut and u < c.W - c.cut and t < c.H - c.cut:
                    proj.append((int(r), t, u, p2))
            if isinstance(depth, str):                                           # the view's own z-buffer (fusion_util.py:126-130)
                dv = np.full((c.H, c.W), FAR)
                for _, t, u, p2 in proj:
                    if p2 > 0.2 and dv[t, u] > p2:
                        dv[t, u] = p2
            else:
                dv = None if depth is None else depth[v]
            for r, t, u, p2 in proj:
                visible = p2 > 0 if dv is None else abs(dv[t, u] - p2) <= tau * dv[t, u]
                if not (visible and p2 > 0):
                    continue
                vc[v] += 1
                for yy in range(max(t - radius, c.cut), min(t + radius, c.H - c.cut - 1) + 1):
                    for xx in range(max(u - radius, c.cut), min(u + radius, c.W - c.cut - 1) + 1):
                        if rows_img[v, yy, xx] < 0 or p2 < z_img[v, yy, xx] or (p2 == z_img[v, yy, xx] and r < rows_img[v, yy, xx]):
                            rows_img[v, yy, xx], z_img[v, yy, xx] = r, p2
            pc[v] = int((rows_img[v] >= 0).sum())
    return rows_img.astype(np.int32), z_img, vc, pc


def merged(c):
    """the geometry of c with every row and every view in entry 0: what rendering would see if entries mixed"""
    pts = c.points.copy()
    pts[:, 0] = 0.0
    return rd.RCase(c.name + "+merged", pts, np.zeros(c.V, np.int64), c.w2c, c.intr, c.H, c.W, c.cut)


# ------------------------------------------------------------------------------------------ edge cases
FX = 8.0


def _at(u, v, z):
    """the point that an identity camera of focal 8, centre (8, 6), puts on pixel (row v, column u) at depth z"""
    return ((u - 8) * z / 8, (v - 6) * z / 8, z)


def case_clip():
    """cut = 2 on 16 x 12: the interior is rows 2..9, columns 2..13.  One entry, one view; candidates on each of the four sides and in
    two corners, every one at its own depth, so a radius-2 footprint is clipped on the left, right, top, bottom and at a corner."""
    rows = [("left", 6.0, 2.0, 1.0), ("right", 5.0, 13.0, 2.0), ("top", 2.0, 8.0, 0.5), ("bottom", 9.0, 7.0, 4.0),
            ("corner_top_left", 2.0, 2.0, 1.5), ("corner_bottom_right", 9.0, 13.0, 2.5), ("middle", 6.0, 8.0, 3.0)]
    pts = np.array([(0.0, *_at(u, v, z)) for _, v, u, z in rows], f64)
    M, K = lb._identity_views(1, FX, 16, 12)
    return rd.RCase("clip", pts, [0], M, K, 12, 16, 2, row_names=[r[0] for r in rows],
                    expect={2: {(2, 2): 4, (3, 4): 4, (4, 4): 0, (4, 2): 0, (5, 2): 0, (8, 4): 0, (9, 4): -1, (3, 13): 1, (7, 11): 1, (7, 13): 1,
                                (2, 6): 2, (4, 10): 2, (5, 8): 6, (9, 5): 3, (7, 5): 3, (7, 9): 6, (9, 11): 5, (8, 12): 5, (9, 13): 5}})


def case_contests():
    """cut = 0 on 16 x 12, one entry and one view per scenario (entries never mix, so the scenarios do not meet):
    entry 0 -- two candidates at the same p_z = 2 on pixels (5, 4) and (5, 6), the one on (5, 6) in the LOWER row: at radius 2 their
      footprints share columns 4..6, which the lower row owns, and each owns the rest of its own;
    entry 1 -- a near candidate (z = 1) on (5, 5) and a far one (z = 2) on (5, 6): at radius 1 the near footprint hides the far
      candidate's centre pixel, and the far one still owns column 7 of its own footprint;
    entry 2 -- sensor depth only: a point on (3, 3) at z = 1 over a NEGATIVE depth value (never a candidate) beside one on (8, 8) over
      depth 1;
    entry 3 -- points at p_z = 0.125 on (6, 8) and p_z = 0.2 on (6, 10): candidates under depth None, ignored by the rendered depth
      (p_z > 0.2), whose pixels stay 999999 and so fail the depth test."""
    rows = [(0, 5.0, 6.0, 2.0), (1, 5.0, 5.0, 1.0), (0, 5.0, 4.0, 2.0), (2, 3.0, 3.0, 1.0), (1, 5.0, 6.0, 2.0), (3, 6.0, 8.0, 0.125),
            (2, 8.0, 8.0, 1.0), (3, 6.0, 10.0, rd.Z_EDGE)]
    pts = np.array([(float(b), *_at(u, v, z)) for b, v, u, z in rows], f64)
    M, K = lb._identity_views(4, FX, 16, 12)
    sensor = np.full((4, 12, 16), 1.0)
    sensor[0], sensor[1], sensor[3] = 2.0, 2.0, 0.125
    sensor[1, 5, 5] = 1.0
    sensor[2, 3, 3] = -1.0
    return rd.RCase("contests", pts, [0, 1, 2, 3], M, K, 12, 16, 0, sensor=sensor)


_BUILDERS = {"clip": case_clip, "contests": case_contests}
EDGE_CASES = tuple(_BUILDERS)
CASES = rd.CASES + EDGE_CASES
_CASES = {}


def case(name):
    if name in _BUILDERS:
        if name not in _CASES:
            _CASES[name] = _BUILDERS[name]()
        return _CASES[name]
    return rd.case(name)
