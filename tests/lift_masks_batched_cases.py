"""Cases for sparse.lift_masks (csrc/lift_masks_batched.hip) and their reference.  numpy / torch on the CPU, no device code.

The reference states the lift per batch entry with the oracle's own pieces, one scene at a time -- what the batched call replaces:
the visible lists and the drop rule of tests/lift_batched_cases.py (oracle.project.compute_mapping_scannet), then
oracle.lift.lift_masks_view(..., return_debug=True) for every kept view and oracle.lift.fuse_views_top3(..., return_debug=True).  Both
nearest-neighbour fills are redone with nn1_indices_bruteforce (the lowest index among equal distances; the oracle's KDTree names no
rule for them): while the reference runs, oracle.lift.nn1_indices is bound to it.  The reference code cannot state one situation: a
kept view in which NO visible point has a segment (all scores 0, or no pixel reaches sigmoid >= 0.5) -- its KDTree is built over
nothing.  The rule here is the one the per-scene kernels follow: such a view fills nothing, its points keep no segment, and a slot
without a segment carries a zero feature and zero logits into the fusion.  The binding above raises on an empty reference set and
oracle.lift.lift_masks_view is wrapped to turn that into zero rows; the no-cover views of the cases keep every resized logit below
-0.5 (checked by the host test), far from the sigmoid >= 0.5 decision, so they hold no near tie of their own.

Near ties: oracle.parity.lift_near_ties on the entry's kept views with its EPS_* unchanged, under the same binding.

Generic scenes are those of tests/lift_batched_cases.py (generic, camera, cloud: images of at most 12 x 16, depth maps that leave seen
and unseen points in an entry) with random VLM outputs: mask logits N(0, 4) on at most 8 x 10, class logits N(0, 2), embeddings and
text N(0, 1).  The in-view fill cases use identity cameras, dyadic coordinates and masks of the image's own size -- the
bicubic-antialias resize to the same size is the identity (taps 0, 1, 0, 0) --, so coverage, segment and every squared distance are
exact and a tie is a tie in the oracle, in the restatement and in the kernel alike.
"""
import contextlib

import numpy as np
import torch

import lift_batched_cases as lb
from lift_batched_cases import camera, cloud, generic, keep_rule, visible_list     # noqa: F401  (camera, cloud: for callers)
from oracle import lift as olift
from oracle import parity as oparity

f32, f64 = np.float32, np.float64


class Case:
    """geo: a lift_batched_cases.Case (points, view_entry, poses, depth, image shape, cut, tau, drop rule; its maps are not used);
    pred_masks f32 [V,Q,h,w]; pred_logits f32 [V,Q,C+1]; mask_embed f32 [V,Q,D]; text f32 [C,D]; scale"""

    def __init__(self, name, geo, pred_masks, pred_logits, mask_embed, text, scale, exact=False, **notes):
        self.name, self.geo, self.exact, self.notes = name, geo, exact, notes
        self.pred_masks, self.pred_logits = np.ascontiguousarray(pred_masks, f32), np.ascontiguousarray(pred_logits, f32)
        self.mask_embed, self.text, self.scale = np.ascontiguousarray(mask_embed, f32), np.ascontiguousarray(text, f32), float(scale)
        self.points, self.view_entry, self.w2c, self.intr, self.depth = geo.points, geo.view_entry, geo.w2c, geo.intr, geo.depth
        self.N, self.V, self.H, self.W = geo.N, geo.V, geo.H, geo.W
        self.cut, self.tau, self.min_visible, self.max_visible = geo.cut, geo.tau, geo.min_visible, geo.max_visible
        _, self.Q, self.h, self.w = self.pred_masks.shape
        self.C, self.D = self.text.shape
        assert self.pred_masks.shape[0] == self.V and self.pred_logits.shape == (self.V, self.Q, self.C + 1)
        assert self.mask_embed.shape == (self.V, self.Q, self.D) and self.h <= self.H and self.w <= self.W
        assert self.H <= 12 and self.W <= 16 and self.h <= 8 and self.w <= 10

    entries = lambda self: self.geo.entries()               # noqa: E731
    rows_of = lambda self, b: self.geo.rows_of(b)           # noqa: E731
    views_of = lambda self, b: self.geo.views_of(b)         # noqa: E731

    def vlm(self):
        return {"pred_masks": self.pred_masks, "pred_logits": self.pred_logits, "mask_embed": self.mask_embed, "text_embed": self.text,
                "logit_scale": self.scale}


class Reference:
    """features f32 [N,D] (after the scene-level fill), pre (before it: zero rows for unseen points), seen, count, view_count,
    view_keep, filled_from i64 [N] (-1: not filled), near bool [N] (the oracle's own near-tie flags), views: {view: (global rows,
    pixel rows, pixel columns, segment after the in-view fill, the global row an uncovered entry took it from or -1)}"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _NoCover(Exception):
    pass


def _nn1_lowest(ref_xyz, query_xyz):
    if len(ref_xyz) == 0:
        raise _NoCover()
    return olift.nn1_indices_bruteforce(ref_xyz, query_xyz)


@contextlib.contextmanager
def oracle_rules():
    """oracle.lift with both fills taking the lowest index among equal distances, and a view without a covered point keeping zero rows"""
    nn1, view = olift.nn1_indices, olift.lift_masks_view

    def lift_masks_view(pred_masks, pred_logits, mask_embed, text_embed, logit_scale, x_label, y_label, coords_view, mask_shape, **kw):
        try:
            return view(pred_masks, pred_logits, mask_embed, text_embed, logit_scale, x_label, y_label, coords_view, mask_shape, **kw)
        except _NoCover:
            n_v = x_label.shape[0]
            out = (torch.zeros((n_v, mask_embed.shape[-1])), torch.zeros((n_v, text_embed.shape[0])))
            return out + ({"zero_before_fill": torch.ones(n_v, dtype=torch.bool)},) if kw.get("return_debug") else out

    olift.nn1_indices, olift.lift_masks_view = _nn1_lowest, lift_masks_view
    try:
        yield
    finally:
        olift.nn1_indices, olift.lift_masks_view = nn1, view


_REFERENCES = {}


def reference(name):
    """computed once per case and shared: callers must not change it"""
    if name not in _REFERENCES:
        _REFERENCES[name] = _reference(case(name))
    return _REFERENCES[name]


def _reference(c):
    N, V, D = c.N, c.V, c.D
    feats, pre = np.zeros((N, D), f32), np.zeros((N, D), f32)
    seen, count, near = np.zeros(N, bool), np.zeros(N, np.int32), np.zeros(N, bool)
    view_count, view_keep = np.zeros(V, np.int64), np.zeros(V, bool)
    filled_from = np.full(N, -1, np.int64)
    views = {}
    text = torch.from_numpy(c.text)
    with oracle_rules():
        for b in c.entries():
            rows, vs = c.rows_of(b), c.views_of(b)
            xyz = c.points[rows, 1:]
            xyz32 = torch.from_numpy(xyz.astype(f32))
            kept = []
            for v in vs:
                pt, x, y = visible_list(c.geo, v, xyz)
                view_count[v], view_keep[v] = len(pt), keep_rule(c.geo, len(pt))
                views[int(v)] = (rows[pt], np.asarray(x, np.int64), np.asarray(y, np.int64), np.full(len(pt), -1, np.int64),
                                 np.full(len(pt), -1, np.int64))
                if view_keep[v]:
                    kept.append({"src_view": int(v), "pt": torch.from_numpy(np.asarray(pt, np.int64)),
                                 "x": torch.from_numpy(np.asarray(x, np.int64)), "y": torch.from_numpy(np.asarray(y, np.int64))})
                    count[rows[pt]] += 1
            if not kept:
                continue
            fs, lgs = [], []
            for k in kept:
                v = k["src_view"]
                f, lg, dbg = olift.lift_masks_view(torch.from_numpy(c.pred_masks[v]), torch.from_numpy(c.pred_logits[v]),
                                                   torch.from_numpy(c.mask_embed[v]), text, c.scale, k["x"], k["y"], xyz32[k["pt"]],
                                                   (c.H, c.W), return_debug=True)
                fs.append(f), lgs.append(lg)
                zero = dbg["zero_before_fill"].numpy()
                seg, src = views[v][3], views[v][4]
                if "seg" in dbg:
                    seg[~zero] = dbg["seg"].numpy()[~zero]
                if "fill_src" in dbg:
                    took = dbg["fill_src"].numpy()
                    seg[zero], src[zero] = seg[took], views[v][0][took]
            n = len(rows)
            out, dbg = olift.fuse_views_top3(n, [k["pt"] for k in kept], fs, lgs, xyz32, return_debug=True)
            s = dbg["seen"].numpy()
            out = out.numpy().copy()
            if "fill_src" in dbg:
                filled_from[rows[~s]] = rows[dbg["fill_src"].numpy()]
            feats[rows], seen[rows] = out, s
            pre[rows] = np.where(s[:, None], out, f32(0))
            near[rows] = oparity.lift_near_ties(kept, c.vlm(), xyz32, (c.H, c.W), n).numpy()
    return Reference(features=feats, pre=pre, seen=seen, count=count, view_count=view_count, view_keep=view_keep, filled_from=filled_from,
                     near=near, views=views)


# ------------------------------------------------------------------------------------------ an independent whole-batch restatement
def _fma32(a, b, t):
    return (a.astype(f64) * f64(b) + t.astype(f64)).astype(f32)


def resized_at(m, taps, row, col):
    """F.interpolate(bicubic, antialias) of m f32 [Q,h,w] to the taps' size at one pixel: fp32, horizontal taps first, t = s0 w0 then
    fused multiply-adds -> f32 [Q]"""
    tx0, twx, ty0, twy = taps
    _, h, w = m.shape
    hr = []
    for j in range(4):
        r = m[:, min(ty0[row] + j, h - 1), :]
        t = (r[:, min(tx0[col], w - 1)] * twx[col, 0]).astype(f32)
        for a in range(1, 4):
            t = _fma32(r[:, min(tx0[col] + a, w - 1)], twx[col, a], t)
        hr.append(t)
    v = (hr[0] * twy[row, 0]).astype(f32)
    for j in range(1, 4):
        v = _fma32(hr[j], twy[row, j], v)
    return v


def restatement(c):
    """The lift written once more, over the whole batch at once with dense (point, view) tables and explicit loops -- no per-entry pass,
    none of the oracle's functions (the resize through geopurify_amd.bicubic's tap tables, the fusion in fp64).  -> dict(features f64
    [N,D], pre, seen, count, view_count, view_keep, filled_from, seg i64 [N,V] (after the in-view fill; -2: no entry), src i64 [N,V])"""
    from geopurify_amd.bicubic import aa_bicubic_taps
    N, V, H, W, Q = c.N, c.V, c.H, c.W, c.Q
    x, y, z = c.points[:, 1], c.points[:, 2], c.points[:, 3]
    mine = c.points[:, 0][:, None] == c.view_entry[None, :]
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
    view_keep = np.array([keep_rule(c.geo, int(n)) for n in view_count], bool)
    use = vis & view_keep[None, :]
    count = use.sum(1).astype(np.int32)
    seen = count > 0
    taps = aa_bicubic_taps(c.w, W) + aa_bicubic_taps(c.h, H)
    scores = torch.softmax(torch.from_numpy(c.pred_logits), dim=-1)[..., :-1].max(-1).values.numpy()
    xyz = c.points[:, 1:].astype(f32).astype(f64)
    seg, src = np.full((N, V), -2, np.int64), np.full((N, V), -1, np.int64)
    for v in np.nonzero(view_keep)[0]:
        pts = np.nonzero(use[:, v])[0]                                           # ascending row
        for p in pts:
            lg = resized_at(c.pred_masks[v], taps, prow[p, v], pcol[p, v])
            with np.errstate(over="ignore"):
                sg = (f32(1) / (f32(1) + np.exp(-lg).astype(f32))).astype(f32)
            best, bq = f32(-1), -1
            for q in range(Q):                                                   # ascending q: the first maximum is kept
                if scores[v, q] > 0 and f32(scores[v, q] * sg[q]) > best:
                    best, bq = f32(scores[v, q] * sg[q]), q
            seg[p, v] = bq if bq >= 0 and sg[bq] >= f32(0.5) else -1
        cov = [p for p in pts if seg[p, v] >= 0]
        for p in pts:
            if seg[p, v] >= 0 or not cov:
                continue
            bd, bs = np.inf, -1
            for r in cov:                                                        # ascending row: the first strict minimum is the lowest row
                dx, dy, dz = xyz[p] - xyz[r]
                d2 = (dx * dx + dy * dy) + dz * dz
                if d2 < bd:
                    bd, bs = d2, r
            src[p, v] = bs
        for p in pts:
            if src[p, v] >= 0:
                seg[p, v] = seg[src[p, v], v]
    emb, text = c.mask_embed.astype(f64), c.text.astype(f64)
    fseg = emb / np.maximum(np.sqrt((emb * emb).sum(-1, keepdims=True)), 1e-12)
    tn = text / np.maximum(np.sqrt((text * text).sum(-1, keepdims=True)), 1e-12)
    pre = np.zeros((N, c.D), f64)
    for p in np.nonzero(seen)[0]:
        slots = np.nonzero(use[p])[0]                                            # ascending view index
        fl = [(fseg[v, seg[p, v]], c.scale * (fseg[v, seg[p, v]] @ tn.T)) if seg[p, v] >= 0 else (np.zeros(c.D), np.zeros(c.C)) for v in slots]
        mean = sum(l for _, l in fl) / len(fl)
        cstar = int(np.argmax(mean))                                             # the first maximum
        agree = np.array([l[cstar] for _, l in fl])
        top = sorted(range(len(fl)), key=lambda j: (-agree[j], j))[:3]           # the earlier slot among equals
        wgt = np.exp(agree[top] - agree[top].max())
        wgt = wgt / wgt.sum()
        pre[p] = sum(wj * fl[j][0] for wj, j in zip(wgt, top))
    filled_from = np.full(N, -1, np.int64)
    for p in np.nonzero(~seen)[0]:
        bd, bs = np.inf, -1
        for r in np.nonzero(seen & (c.points[:, 0] == c.points[p, 0]))[0]:
            dx, dy, dz = xyz[p] - xyz[r]
            d2 = (dx * dx + dy * dy) + dz * dz
            if d2 < bd:
                bd, bs = d2, r
        filled_from[p] = bs
    out = pre.copy()
    out[filled_from >= 0] = pre[filled_from[filled_from >= 0]]
    return dict(features=out, pre=pre, seen=seen, count=count, view_count=view_count, view_keep=view_keep, filled_from=filled_from, seg=seg,
                src=src)


# ------------------------------------------------------------------------------------------ VLM outputs
def vlm_outputs(rng, V, Q, C, D, hw):
    pm = rng.normal(0, 4, (V, Q) + tuple(hw)).astype(f32)
    pl = rng.normal(0, 2, (V, Q, C + 1)).astype(f32)
    me = rng.normal(0, 1, (V, Q, D)).astype(f32)
    return pm, pl, me, rng.normal(0, 1, (C, D)).astype(f32)


def with_vlm(name, geo, seed, Q=5, C=3, D=4, hw=(6, 8), scale=14.25, edit=None, **notes):
    rng = np.random.default_rng(1000 + seed)
    pm, pl, me, text = vlm_outputs(rng, geo.V, Q, C, D, hw)
    if edit is not None:
        edit(geo, pm, pl, me)
    return Case(name, geo, pm, pl, me, text, scale, **notes)


def masks(name, seed, sizes, views, Q=5, C=3, D=4, hw=(6, 8), image_shape=(12, 16), edit=None, **kw):
    return with_vlm(name, generic(name, seed, sizes, views, 1, hw=image_shape, **kw), seed, Q, C, D, hw, edit=edit)


def _scores_edit(geo, pm, pl, me):
    """entry 0: its first view has all scores 0; entry 1: its first view reaches sigmoid >= 0.5 nowhere; entry 2: one view, all scores 0"""
    for b, kind in ((0, "zero"), (1, "low"), (2, "zero")):
        v = geo.views_of(b)[0]
        if kind == "zero":
            pl[v, :, :-1], pl[v, :, -1] = -100.0, 100.0
        else:
            pm[v] = -np.abs(pm[v]) / 4 - 1                                       # logits in about [-5, -1]: the cubic's overshoot stays far below 0


# ------------------------------------------------------------------------------------------ the in-view fill on exact arithmetic
FILL_W, FILL_H, FILL_FX = 10, 8, 2.0                        # the image, and the masks: centre (5, 4)


def _stripes(V, Q, cover):
    """masks of the image's size: cover[v] = {pixel column: query}; that query's logit is +4 in the column (all rows), every other
    logit -4"""
    pm = np.full((V, Q, FILL_H, FILL_W), -4.0, f32)
    for v, cols in cover.items():
        for col, q in cols.items():
            pm[v, q, :, col] = 4.0
    return pm


def _class_logits(V, Q, C):
    """scores 0.9, 0.8, 0.7, ... per query (distinct products whatever the query)"""
    pl = np.zeros((V, Q, C + 1), f32)
    for q in range(Q):
        s = 0.9 - 0.1 * q
        pl[:, q, 0], pl[:, q, 1:] = np.log(s), np.log((1 - s) / C)
    return pl


def _at(col, row=4, z=1.0):
    """the world point that an identity camera of focal 2 and centre (5, 4) projects to pixel (row, col) from depth z"""
    return (col - 5) * z / FILL_FX, (row - 4) * z / FILL_FX, z


def case_fill_inview():
    """Identity cameras of focal 2 on 10 x 8 (u = 2 x / z + 5, v = 2 y / z + 4), no depths, masks of the image's size, three queries.
      entry 0, view A (view 1): covered (2,0,1) [row 0, column 9, query 0] and (-2,0,1) [row 1, column 1, query 1]; uncovered (0,0,1)
        [row 2, column 5]: d^2 = 4 to both, the lower row 0 wins though it comes second in ascending x;
        view B (view 0, looking down -z) sees (0.25,0,-0.5) [row 3, column 6] covered by query 2: d^2 = 2.3125 from row 2, nearer than
        both, but it is no entry of view A; in view B row 4 = (1,0,-1) [column 7] is uncovered and takes query 2 from row 3;
      entry 1, view C (view 2): (0,0,1) [row 5, column 5, query 2 there] coincides with row 2 of entry 0 and must not reach it;
        (0.5,0,1) [row 6, column 6] uncovered takes query 2 from row 5."""
    P = [(0, 2.0, 0.0, 1.0), (0, -2.0, 0.0, 1.0), (0, 0.0, 0.0, 1.0), (0, 0.25, 0.0, -0.5), (0, 1.0, 0.0, -1.0),
         (1, 0.0, 0.0, 1.0), (1, 0.5, 0.0, 1.0)]
    ve = np.array([0, 0, 1])
    M, K = lb._identity_views(3, FILL_FX, FILL_W, FILL_H)
    M[0, 2, 2] = -1.0                                                            # view B: p_z = -z
    pm = _stripes(3, 3, {1: {9: 0, 1: 1}, 0: {6: 2}, 2: {5: 2}})
    rng = np.random.default_rng(31)
    geo = lb.Case("fill_inview", np.array(P, f64), np.zeros((3, 1, FILL_H, FILL_W), f32), ve, M, K, None)
    # expect: (row, view) -> (segment, the row it came from)
    return Case("fill_inview", geo, pm, _class_logits(3, 3, 3), rng.normal(0, 1, (3, 3, 4)), rng.normal(0, 1, (3, 4)), 14.25, exact=True,
                expect={(2, 1): (0, 0), (4, 0): (2, 3), (6, 2): (2, 5)}, tie=(2, 0, 1), other_view_nearer=(2, 3), other_entry_nearer=(2, 5))


FILL_257_DEPTHS = (1.0, 1.25, 1.5, 1.75, 2.0, 2.5, 3.0)


def case_fill_257():
    """One view with 257 uncovered entries (columns 1 .. 5, rows 0 .. 7, seven depths: 280 pixels-at-depths, the first 257) and covered
    ones on both sides, in columns 0 (query 0) and 9 (query 1) at rows 1, 4, 6: the second block of 256 queries holds one.  A second
    entry with a view of its own rides along."""
    unc = [(0,) + _at(col, row, z) for z in FILL_257_DEPTHS for row in range(8) for col in range(1, 6)][:257]
    cov = [(0,) + _at(col, row, z) for col in (0, 9) for row in (1, 4, 6) for z in (1.0, 2.0)]
    other = [(1,) + _at(col, 3, 1.0) for col in (2, 3, 8, 9)]
    rng = np.random.default_rng(32)
    P = np.array(unc + cov + other, f64)[rng.permutation(257 + 12 + 4)]
    M, K = lb._identity_views(2, FILL_FX, FILL_W, FILL_H)
    pm = _stripes(2, 3, {0: {0: 0, 9: 1}, 1: {8: 2, 2: 1}})
    geo = lb.Case("fill_257", P, np.zeros((2, 1, FILL_H, FILL_W), f32), np.array([0, 1]), M, K, None)
    return Case("fill_257", geo, pm, _class_logits(2, 3, 3), rng.normal(0, 1, (2, 3, 4)), rng.normal(0, 1, (3, 4)), 14.25, exact=True)


_BUILDERS = {
    # views per entry: 0, 1, 63 / 64, 65 (129 views in all) / 128, 129 / 2, 130; view_entry interleaved, rows shuffled
    "views_0_1_63": lambda: masks("views_0_1_63", 1, {0: 40, 1: 50, 2: 120}, {1: 1, 2: 63}),
    "views_64_65": lambda: masks("views_64_65", 2, {0: 90, 1: 110}, {0: 64, 1: 65}),
    "views_128_129": lambda: masks("views_128_129", 3, {0: 60, 1: 70}, {0: 128, 1: 129}),
    "views_130": lambda: masks("views_130", 4, {0: 60, 1: 150}, {0: 2, 1: 130}, D=6),
    # queries
    "Q1": lambda: masks("Q1", 5, {0: 60, 1: 50}, {0: 3, 1: 2}, Q=1),
    "Q63": lambda: masks("Q63", 6, {0: 60, 1: 50}, {0: 3, 1: 2}, Q=63),
    "Q64": lambda: masks("Q64", 7, {0: 60, 1: 50}, {0: 3, 1: 2}, Q=64),
    "Q65": lambda: masks("Q65", 8, {0: 60, 1: 50}, {0: 3, 1: 2}, Q=65),
    "Q200": lambda: masks("Q200", 9, {0: 60, 1: 50}, {0: 3, 1: 2}, Q=200, hw=(4, 5)),
    "Q1024": lambda: masks("Q1024", 10, {0: 60, 1: 50}, {0: 3, 1: 2}, Q=1024, hw=(2, 3)),
    # scores
    # (C = 1: a point that only no-cover views see has all-zero logits -- with two classes the oracle flags that exact tie of its class
    # arg-max, though the row is zero whichever class wins; one class has no such decision)
    "scores": lambda: masks("scores", 11, {0: 70, 1: 80, 2: 40}, {0: 3, 1: 2, 2: 1}, C=1, edit=_scores_edit),
    # widths and classes
    # (D = 1 with C = 1: unit rows are +-1, so with two classes every class arg-max would be an exact tie)
    "D1": lambda: masks("D1", 12, {0: 60, 1: 50}, {0: 3, 1: 2}, D=1, C=1),
    "D6": lambda: masks("D6", 13, {0: 60, 1: 50}, {0: 3, 1: 2}, D=6),
    "D65": lambda: masks("D65", 14, {0: 60, 1: 50}, {0: 3, 1: 2}, D=65),
    "D512": lambda: masks("D512", 15, {0: 60, 1: 50}, {0: 3, 1: 2}, D=512),
    "C1": lambda: masks("C1", 16, {0: 60, 1: 50}, {0: 3, 1: 2}, C=1),
    "C19": lambda: masks("C19", 17, {0: 60, 1: 50}, {0: 3, 1: 2}, C=19),
    "C65": lambda: masks("C65", 18, {0: 60, 1: 50}, {0: 3, 1: 2}, C=65),
    # mask sizes
    "mask_full": lambda: masks("mask_full", 19, {0: 60, 1: 50}, {0: 3, 1: 2}, hw=(8, 10), image_shape=(8, 10)),
    "mask_h1": lambda: masks("mask_h1", 20, {0: 60, 1: 50}, {0: 3, 1: 2}, hw=(1, 5)),
    "mask_w1": lambda: masks("mask_w1", 21, {0: 60, 1: 50}, {0: 3, 1: 2}, hw=(5, 1)),
    # entries: 0, 2 and 65535 present; entry 5 has points and no views, entry 9 views and no points
    "entries": lambda: masks("entries", 22, {0: 1, 2: 45, 5: 20, 65535: 30}, {0: 2, 2: 3, 9: 2, 65535: 2}),
    # the situations of the dense cases: the scene-level fill, twins, the drop rule
    "fill": lambda: with_vlm("fill", lb.case("fill"), 23),
    "twins": lambda: with_vlm("twins", lb.case("twins"), 24),
    "drop": lambda: with_vlm("drop", lb.case("drop"), 25),
    # the in-view fill on exact arithmetic
    "fill_inview": case_fill_inview,
    "fill_257": case_fill_257,
}
CASES = tuple(_BUILDERS)
_CASES = {}
# the large geometries of tests/lift_batched_cases.py (more than one fill block, LDS trip, count trip and walk trip) under random VLM
# outputs: reachable through case() and reference(), not in CASES -- restatement() and the per-scene sequences are not for them
_LARGE_BUILDERS = {"fill_blocks": lambda: with_vlm("fill_blocks", lb.case("fill_blocks"), 41),
                   "walk_trips": lambda: with_vlm("walk_trips", lb.case("walk_trips"), 42)}
LARGE = tuple(_LARGE_BUILDERS)
_BUILDERS.update(_LARGE_BUILDERS)


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]
