"""sparse.lift_masks on the GPU: the mask-embedding lift with top-3 fusion over batched point clouds against the per-entry reference of
tests/lift_masks_batched_cases.py (the oracle's lift_masks_view and fuse_views_top3, one scene at a time), against the per-scene kernels
it replaces, and against the reference's own fixtures.

Bounds.  Exact: seen, count, view_count, view_keep, the visible lists, the scene-level fill's choice (nn) and the in-view fill's (the
segment every entry holds after it: in the exact-arithmetic cases every candidate source carries another segment).  Features: within
1e-5 (tol_lift of oracle/parity.py; a wrong pick differs by ~0.1) of the reference on every row the reference's own near-tie flags do
not cover -- and tests/test_lift_masks_batched_cases_host.py caps those flags at max(1 %, 2 rows) per case, 0 in the exact cases.  The
same bits as ops.views_visible_lists -> ops.lift_masks_views -> ops.segment_tables -> ops.fuse_views_top3 -> ops.nn1_masked ->
ops.gather_rows on every entry by itself (entries beyond that path's 128 views: the view-by-view kernels).
"""
import os
import sys

import numpy as np
import pytest
import torch

import extent_fence
import lift_batched_cases as lb
import lift_masks_batched_cases as lm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_LIFT = 1e-5


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import _lib, ops, sparse
    _lib.load()
    return ops, sparse


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _views(sparse, c):
    return sparse.MaskViews(_dev(c.pred_masks), _dev(c.pred_logits), _dev(c.mask_embed), _dev(c.view_entry), _dev(c.w2c), _dev(c.intr),
                            None if c.depth is None else _dev(c.depth), (c.H, c.W))


def _options(c):
    return dict(cut_bound=c.cut, vis_thres=c.tau, min_visible=c.min_visible, max_visible=c.max_visible)


def _lift(env, c, points=None, views=None, **kw):
    ops, sparse = env
    return sparse.lift_masks(_dev(c.points) if points is None else points, _views(sparse, c) if views is None else views, _dev(c.text), c.scale,
                             **{**_options(c), **kw})


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pad4(d):
    return (d + 3) // 4 * 4


def _tables(ops, embed, text, scale):
    """ops.segment_tables on columns padded to a multiple of 4 (the fusion kernel's rows) -> f_seg [V,Q,d4], logit_seg [V,Q,C], the
    normalised text [C,D]"""
    V, Q, D = embed.shape
    d4 = _pad4(D)
    tn = torch.nn.functional.normalize(text.float(), dim=-1)
    e4, t4 = torch.zeros((V * Q, d4), device="cuda"), torch.zeros((text.shape[0], d4), device="cuda")
    e4[:, :D], t4[:, :D] = embed.reshape(V * Q, D), tn
    f_seg, l_seg = torch.empty((V, Q, d4), device="cuda"), torch.empty((V, Q, text.shape[0]), device="cuda")
    ops.segment_tables(e4, t4, float(scale), f_seg.view(V * Q, d4), l_seg.view(V * Q, -1))
    return f_seg, l_seg, tn


def _scores(pred_logits):
    return torch.softmax(pred_logits, dim=-1)[..., :-1].max(-1).values.contiguous()


def _lists(env, c, **kw):
    ops, _ = env
    return ops.lift_masks_batched_lists(_dev(c.points), _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), None if c.depth is None else _dev(c.depth),
                                        (c.H, c.W), c.cut, c.tau, c.min_visible, 2 ** 63 - 1 if c.max_visible is None else c.max_visible, **kw)


def _words(c):
    return max(1, -(-max(len(c.views_of(b)) for b in np.unique(c.view_entry)) // 64))


def _raw(env, c, lists=None, **kw):
    """the two ops wrappers on a case -> (LiftMasksLists, LiftMasksBatched)"""
    ops, sparse = env
    lists = _lists(env, c) if lists is None else lists
    f_seg, l_seg, _ = _tables(ops, _dev(c.mask_embed), _dev(c.text), c.scale)
    r = ops.lift_masks_batched(_dev(c.points), _dev(c.view_entry), _dev(c.pred_masks), _scores(_dev(c.pred_logits)),
                               sparse._tap_tables(c.h, c.w, c.H, c.W, torch.device("cuda", torch.cuda.current_device())), (c.H, c.W),
                               (lists.pt, lists.x, lists.y, lists.view), lists.view_off, lists.view_keep, lists.total, _words(c), f_seg, l_seg, **kw)
    return lists, r


def _taps(env, c):
    return env[1]._tap_tables(c.h, c.w, c.H, c.W, torch.device("cuda", torch.cuda.current_device()))


def _per_scene(env, c):
    """The sequence the batched call replaces, entry by entry on the same inputs: ops.views_visible_lists, ops.lift_masks_views (at
    most 128 views; beyond: ops.lift_masks_view + ops.nn1_masked + ops.pv_count / ops.pv_fill view by view, HotPath.lift_masks' other
    path), ops.segment_tables, ops.fuse_views_top3, ops.nn1_masked, ops.gather_rows -> (features, seen, view_count, view_keep)"""
    ops, _ = env
    feats = torch.zeros((c.N, c.D), dtype=torch.float32, device="cuda")
    seen = torch.zeros(c.N, dtype=torch.bool, device="cuda")
    view_count, view_keep = torch.zeros(c.V, dtype=torch.int64), torch.zeros(c.V, dtype=torch.bool)
    pm, scores, emb, taps = _dev(c.pred_masks), _scores(_dev(c.pred_logits)), _dev(c.mask_embed), _taps(env, c)
    for b in c.entries():
        rows, vs = c.rows_of(b), c.views_of(b)
        if len(vs) == 0:
            continue
        n, nv = len(rows), len(vs)
        params = _dev(np.concatenate([c.w2c[vs].reshape(nv, 16), c.intr[vs]], 1))
        ent = ops.views_visible_lists(_dev(c.points[rows, 1:]), params, None if c.depth is None else _dev(c.depth[vs]), c.W, c.H, c.cut, c.tau,
                                      c.min_visible, 2 ** 62 if c.max_visible is None else c.max_visible)
        off, keep = ent["view_off"].tolist(), ent["keep"].tolist()
        for i, v in enumerate(vs):
            view_count[v], view_keep[v] = off[i + 1] - off[i], bool(keep[i])
        total = off[-1]
        if total == 0:
            continue
        xyz = _dev(c.points[rows, 1:].astype(np.float32))
        vs_d = _dev(vs)
        f_seg, l_seg, _ = _tables(ops, emb[vs_d], _dev(c.text), c.scale)
        if nv <= 128:
            _, start, pvv, pvs = ops.lift_masks_views(pm[vs_d].contiguous(), scores[vs_d].contiguous(), taps, (c.H, c.W), xyz, ent, total, nv)
        else:
            cnt = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            segs = {}
            for i, v in enumerate(vs):
                if not keep[i]:
                    continue
                pt, x, y = (ent[k][off[i]:off[i + 1]] for k in ("pt", "x", "y"))
                seg = ops.lift_masks_view(pm[v], scores[v], taps, (c.H, c.W), x, y)
                covered = (seg >= 0).to(torch.uint8)
                nn = ops.nn1_masked(xyz[pt].contiguous(), covered, 1 - covered)
                segs[i] = torch.where(nn >= 0, seg[nn.clamp(min=0)], seg)
                ops.pv_count(pt, cnt)
            start = ops.exclusive_scan_i64(cnt)
            cursor = torch.zeros(n, dtype=torch.int32, device="cuda")
            pvv, pvs = (torch.empty(total, dtype=torch.int32, device="cuda") for _ in range(2))
            for i, seg in segs.items():                                          # ascending view
                ops.pv_fill(ent["pt"][off[i]:off[i + 1]], seg, i, start, cursor, pvv, pvs)
        F = torch.empty((n, _pad4(c.D)), dtype=torch.float32, device="cuda")
        sn = ops.fuse_views_top3(start, pvv, pvs, n, f_seg, l_seg, F)
        nn = ops.nn1_masked(xyz, sn, 1 - sn)
        out = ops.gather_rows(F, F.shape[1], torch.where(nn >= 0, nn, torch.arange(n, device="cuda")))
        feats[_dev(rows)], seen[_dev(rows)] = out[:, :c.D], sn.bool()
    return feats, seen, view_count, view_keep


# ------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", lm.CASES)
def test_lift_masks_matches_the_reference(env, name):
    c, ref = lm.case(name), lm.reference(name)
    got = _lift(env, c)
    assert got.features.dtype == torch.float32 and got.features.shape == (c.N, c.D) and not got.features.requires_grad
    assert got.seen.dtype == torch.bool and got.count.dtype == torch.int32 and got.view_count.dtype == torch.int64 and got.view_keep.dtype == torch.bool
    assert np.array_equal(got.seen.cpu().numpy(), ref.seen) and np.array_equal(got.count.cpu().numpy(), ref.count)
    assert np.array_equal(got.view_count.cpu().numpy(), ref.view_count) and np.array_equal(got.view_keep.cpu().numpy(), ref.view_keep)
    assert got.logit_scale == c.scale
    # (unit rows in fp32 on two machines: the norm's sum in another order, one square root, one division -- within 4 ulp of values <= 1)
    assert float((got.text_features.cpu() - torch.nn.functional.normalize(torch.from_numpy(c.text), dim=-1)).abs().max()) <= 4 * 2.0 ** -24
    lists, raw = _raw(env, c)
    # the visible lists, view-major, rows ascending inside a view; the segment of every entry after the in-view fill
    off = lists.view_off.tolist()
    assert off[0] == 0 and off[-1] == lists.total == sum(len(v[0]) for v in ref.views.values())
    assert lists.max_views == max(len(c.views_of(b)) for b in np.unique(c.view_entry))
    ent = [t.cpu().numpy() for t in (lists.pt, lists.x, lists.y, lists.view)] + [raw.seg.cpu().numpy()]
    for v in range(c.V):
        rows, x, y, seg, _ = ref.views.get(v, (np.zeros(0, np.int64),) * 5)
        s = slice(off[v], off[v + 1])
        assert np.array_equal(ent[0][s], rows) and np.array_equal(ent[1][s], x) and np.array_equal(ent[2][s], y) and (ent[3][s] == v).all(), v
        if ref.view_keep[v]:
            sure = ~ref.near[rows]
            assert np.array_equal(ent[4][s][sure], seg[sure]), v                # (the in-view fill's choice)
        else:
            assert (ent[4][s] == -1).all(), v
    assert np.array_equal(raw.nn.cpu().numpy(), ref.filled_from)                 # the scene-level fill's choice
    status = raw.status.tolist()
    assert status[:3] == [0, 0, 0] and status[3] == int(c.entries().max()) and status[4] == int(ref.seen.sum())
    assert status[5] == int((ref.filled_from >= 0).sum()) and status[6:] == [0, 0]
    d = np.abs(got.features.cpu().numpy().astype(np.float64) - ref.features.astype(np.float64)).max(1)
    differ = d > TOL_LIFT
    print(f"{name}: {int(ref.near.sum())} rows flagged as near ties, {int(differ.sum())} rows differ by more than {TOL_LIFT} (max off the flags "
          f"{float(d[~ref.near].max()) if (~ref.near).any() else 0.0:.3e})")
    assert not (differ & ~ref.near).any()
    # without the fill an unseen row is zero and a seen row is the filled call's
    plain = _lift(env, c, fill=False)
    seen = got.seen
    assert torch.equal(_bits(plain.features[seen]), _bits(got.features[seen])) and not bool(plain.features[~seen].any())
    assert torch.equal(_bits(plain.features), _bits(raw.out[:, :c.D]))


@pytest.mark.parametrize("name", lm.CASES)
def test_bit_equal_to_the_per_scene_kernels(env, name):
    c = lm.case(name)
    got = _lift(env, c)
    feats, seen, view_count, view_keep = _per_scene(env, c)
    assert torch.equal(got.seen, seen) and torch.equal(got.view_count.cpu(), view_count) and torch.equal(got.view_keep.cpu(), view_keep)
    assert torch.equal(_bits(got.features), _bits(feats))


# ------------------------------------------------------------------------------------------ the reference's fixtures
def _fixture_batch(golden_dir):
    """ref_lift_masks (14 views, Q = 24) and ref_lift_masks_manyviews (94 views, Q = 10, padded to 24 with queries of score 0) as three
    entries of one call: masks, manyviews, manyviews again -- 202 views -- with the fixtures' own visible lists.  The two fixtures have
    text embeddings of their own: the wrapper takes segment tables, so every entry's views get the tables of its fixture's text."""
    ga, gb = (np.load(os.path.join(golden_dir, f"{n}.npz")) for n in ("ref_lift_masks", "ref_lift_masks_manyviews"))
    assert tuple(ga["mask_shape"]) == tuple(gb["mask_shape"]) and ga["text_embed"].shape == gb["text_embed"].shape
    Q = ga["pred_masks"].shape[1]
    src = gb["view_source"]

    def padded(a, fill):
        out = np.broadcast_to(np.asarray(fill, np.float32), (a.shape[0], Q) + a.shape[2:]).copy()
        out[:, :a.shape[1]] = a
        return out
    none = np.full(gb["pred_logits"].shape[2], -100.0, np.float32)
    none[-1] = 100.0
    many = [padded(gb["pred_masks"][src], 0.0), padded(gb["pred_logits"][src], none), padded(gb["mask_embed"][src], 0.0)]
    pm, pl, me = (np.concatenate([a, m, m]) for a, m in zip((ga["pred_masks"], ga["pred_logits"], ga["mask_embed"]), many))
    entries = [(ga, 0), (gb, len(ga["scene_coords"])), (gb, len(ga["scene_coords"]) + len(gb["scene_coords"]))]
    points = np.concatenate([np.column_stack([np.full(len(g["scene_coords"]), b, np.float64), g["scene_coords"].astype(np.float64)])
                             for b, (g, _) in enumerate(entries)])
    view_entry = np.concatenate([np.full(int(g["num_views"]), b, np.int64) for b, (g, _) in enumerate(entries)])
    lists = [(g[f"v{i}_pt"].astype(np.int64) + row0, g[f"v{i}_x"].astype(np.int64), g[f"v{i}_y"].astype(np.int64))
             for g, row0 in entries for i in range(int(g["num_views"]))]
    return dict(points=points, view_entry=view_entry, lists=lists, pm=pm, pl=pl, me=me, text=[g["text_embed"] for g, _ in entries],
                scale=[float(g["logit_scale"]) for g, _ in entries], out_text=[g["out_text_features"] for g, _ in entries],
                mask_shape=tuple(int(v) for v in ga["mask_shape"]), out=[g["out_features"] for g, _ in entries],
                first=[row0 for _, row0 in entries])


def _run_fixture(env, fx, order=None):
    """through ops.lift_masks_batched with the fixtures' lists; order: the new row of every point (None: as they are)"""
    ops, sparse = env
    N = len(fx["points"])
    order = np.arange(N) if order is None else order
    points = np.empty_like(fx["points"])
    points[order] = fx["points"]
    pt = torch.from_numpy(np.concatenate([order[p] for p, _, _ in fx["lists"]])).cuda()
    x, y = (torch.from_numpy(np.concatenate([l[k] for l in fx["lists"]])).cuda() for k in (1, 2))
    counts = [len(p) for p, _, _ in fx["lists"]]
    V = len(counts)
    view = torch.from_numpy(np.repeat(np.arange(V, dtype=np.int32), counts)).cuda()
    view_off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).cuda()
    me = _dev(fx["me"])
    tabs = [_tables(ops, me[_dev(np.nonzero(fx["view_entry"] == b)[0])], _dev(fx["text"][b]), fx["scale"][b]) for b in range(3)]
    f_seg, l_seg, tn = torch.cat([t[0] for t in tabs]), torch.cat([t[1] for t in tabs]), [t[2] for t in tabs]
    h, w = fx["pm"].shape[2:]
    H, W = fx["mask_shape"]
    taps = sparse._tap_tables(h, w, H, W, torch.device("cuda", torch.cuda.current_device()))
    r = ops.lift_masks_batched(_dev(points), _dev(fx["view_entry"]), _dev(fx["pm"]), _scores(_dev(fx["pl"])), taps, (H, W), (pt, x, y, view),
                               view_off, torch.ones(V, dtype=torch.uint8, device="cuda"), int(sum(counts)), 2, f_seg, l_seg)
    assert r.status.tolist()[:3] == [0, 0, 0] and r.status.tolist()[6:] == [0, 0]
    out = ops.gather_rows(r.out, r.out.shape[1], torch.where(r.nn >= 0, r.nn, torch.arange(N, device="cuda")))
    return out[torch.from_numpy(order).cuda()], tn                               # back in the fixtures' row order


def test_reference_fixtures_as_three_entries_of_one_call(env, golden_dir):
    fx = _fixture_batch(golden_dir)
    assert len(fx["view_entry"]) == 202 and fx["pm"].shape[1] == 24
    out, tn = _run_fixture(env, fx)
    for t, ref in zip(tn, fx["out_text"]):
        assert float((t.cpu() - torch.from_numpy(ref)).abs().max()) <= 1e-7
    for b, (ref, row0) in enumerate(zip(fx["out"], fx["first"])):
        d = (out[row0:row0 + len(ref)].cpu() - torch.from_numpy(ref)).abs().max(dim=1).values
        bad = d > 1e-5
        print(f"fixture entry {b}: {int(bad.sum())} rows beyond 1e-5, max of the rest {float(d[~bad].max()):.3e}, median {float(d.median()):.3e}")
        assert int(bad.sum()) <= 2, (b, int(bad.sum()), float(d.max()))
        assert float(d[~bad].max()) <= 1e-5 and float(d.median()) <= 1e-6
    assert torch.equal(_bits(out[fx["first"][1]:fx["first"][2]]), _bits(out[fx["first"][2]:]))     # the two copies of manyviews
    # the same entries with their rows interleaved (a stable merge: every entry keeps its relative order)
    N = len(fx["points"])
    key = np.concatenate([np.arange(n) / n for n in (len(o) for o in fx["out"])])
    order = np.empty(N, np.int64)
    order[np.argsort(key, kind="stable")] = np.arange(N)
    assert (np.diff(fx["points"][np.argsort(order), 0]) != 0).sum() > 1000
    mixed, _ = _run_fixture(env, fx, order)
    assert torch.equal(_bits(mixed), _bits(out))


# ------------------------------------------------------------------------------------------ invariances
@pytest.mark.parametrize("name", ["views_130", "views_64_65", "Q200", "D65", "entries", "twins", "scores"])
def test_runs_row_order_dtype_and_view_order_do_not_change_a_point(env, name):
    ops, sparse = env
    c = lm.case(name)
    base, again = _lift(env, c), _lift(env, c)
    assert torch.equal(_bits(base.features), _bits(again.features)) and torch.equal(base.count, again.count)
    assert torch.equal(base.view_count, again.view_count)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(c.N)).cuda()
    sh = _lift(env, c, points=_dev(c.points)[perm])
    assert torch.equal(_bits(sh.features), _bits(base.features[perm])) and torch.equal(sh.seen, base.seen[perm])
    assert torch.equal(sh.count, base.count[perm]) and torch.equal(sh.view_count, base.view_count) and torch.equal(sh.view_keep, base.view_keep)
    if np.array_equal(c.points.astype(np.float32).astype(np.float64), c.points):
        assert torch.equal(_bits(_lift(env, c, points=_dev(c.points.astype(np.float32))).features), _bits(base.features))
    # another view order that keeps every entry's relative order: the views sorted stably by entry
    order = np.argsort(c.view_entry, kind="stable")
    assert not np.array_equal(order, np.arange(c.V))
    o = torch.from_numpy(order).cuda()
    v = _views(sparse, c)
    moved = sparse.MaskViews(v.pred_masks[o], v.pred_logits[o], v.mask_embed[o], v.view_entry[o], v.world_to_camera[o], v.intrinsics[o],
                             None if v.depth is None else v.depth[o], v.image_shape)
    mv = _lift(env, c, views=moved)
    assert torch.equal(_bits(mv.features), _bits(base.features)) and torch.equal(mv.count, base.count)
    assert torch.equal(mv.view_count, base.view_count[o]) and torch.equal(mv.view_keep, base.view_keep[o])


# ------------------------------------------------------------------------------------------ extents
@pytest.mark.parametrize("name", ["views_130", "Q65", "D65", "entries", "fill_257", "drop"])
def test_the_entry_points_stay_inside_their_extents(env, name):
    """ops.lift_masks_batched_lists and ops.lift_masks_batched on fenced arrays: every fp32 and integer input, every output (the rows
    with a pitch of their own), the workspaces of exactly the reported bytes; the fp64 inputs have no fence type and stay plain.  Nothing
    outside the extents is written, nothing read from there reaches a result."""
    ops, sparse = env
    from geopurify_amd import _lib
    lib = _lib.load()
    c, ref = lm.case(name), lm.reference(name)
    N, V, D, d4 = c.N, c.V, c.D, _pad4(c.D)
    total = sum(len(v[0]) for v in ref.views.values())
    f_seg0, l_seg0, _ = _tables(ops, _dev(c.mask_embed), _dev(c.text), c.scale)
    scores0, taps0 = _scores(_dev(c.pred_logits)), _taps(env, c)

    def case(a):
        ve = a.inp(torch.from_numpy(c.view_entry), name="view_entry")
        bufs = {"pt": a.out(total, torch.int64, name="pt"), "x": a.out(total, torch.int64, name="x"), "y": a.out(total, torch.int64, name="y"),
                "view": a.out(total, torch.int32, name="view"), "view_off": a.out(V + 1, torch.int64, name="view_off"),
                "view_count": a.out(V, torch.int64, name="view_count"), "view_keep": a.out(V, torch.uint8, name="view_keep"),
                "status": a.out(8, torch.int64, name="lists_status")}
        ws = a.out(lib.gp_lift_masks_batched_lists_workspace_bytes(N, V), torch.uint8, name="lists_workspace")
        lists = ops.lift_masks_batched_lists(_dev(c.points), ve, _dev(c.w2c), _dev(c.intr), None if c.depth is None else _dev(c.depth), (c.H, c.W),
                                             c.cut, c.tau, c.min_visible, 2 ** 63 - 1 if c.max_visible is None else c.max_visible, buffers=bufs,
                                             workspace=ws)
        assert lists.total == total
        pitch = d4 + 4 if a.fence else d4
        out = {"out": a.out((N, d4), torch.float32, pitch=pitch, name="out"), "seen": a.out(N, torch.uint8, name="seen"),
               "count": a.out(N, torch.int32, name="count"), "nn": a.out(N, torch.int64, name="nn"), "seg": a.out(total, torch.int32, name="seg"),
               "status": a.out(8, torch.int64, name="status")}
        fill_cap = min(total, 300)
        ws2 = a.out(lib.gp_lift_masks_batched_workspace_bytes(N, V, c.Q, c.h, c.w, c.H, c.W, total, _words(c), fill_cap), torch.uint8,
                    name="workspace")
        taps = tuple(a.inp(t.cpu(), name=f"tap{i}") for i, t in enumerate(taps0))
        r = ops.lift_masks_batched(_dev(c.points), ve, a.inp(torch.from_numpy(c.pred_masks), name="pred_masks"), a.inp(scores0.cpu(), name="scores"),
                                   taps, (c.H, c.W), (lists.pt, lists.x, lists.y, lists.view), lists.view_off, lists.view_keep, total, _words(c),
                                   a.inp(f_seg0.cpu(), name="f_seg"), a.inp(l_seg0.cpu(), name="logit_seg"), fill_cap=fill_cap, buffers=out,
                                   workspace=ws2)
        return {"pt": lists.pt, "x": lists.x, "y": lists.y, "view": lists.view, "view_off": lists.view_off, "view_count": lists.view_count,
                "view_keep": lists.view_keep, "out": r.out, "seen": r.seen, "count": r.count, "nn": r.nn, "seg": r.seg, "status": r.status}

    got = extent_fence.run(case)
    for k, v in got.items():
        assert extent_fence.unwritten(v) == 0, k
    assert np.array_equal(got["nn"].cpu().numpy(), ref.filled_from) and np.array_equal(got["count"].cpu().numpy(), ref.count)
    assert np.array_equal(got["view_count"].cpu().numpy(), ref.view_count)


def test_overlapping_arguments_are_refused(env):
    ops, _ = env
    from geopurify_amd._lib import GeoPurifyHipError
    c = lm.case("C19")
    both = torch.zeros(c.V + c.V + 1, dtype=torch.int64, device="cuda")
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        _lists(env, c, total=5, buffers={"view_off": both[:c.V + 1], "view_count": both[c.V:c.V + c.V]})
    ve = _dev(c.view_entry)
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        ops.lift_masks_batched_lists(_dev(c.points), ve, _dev(c.w2c), _dev(c.intr), None, (c.H, c.W), c.cut, c.tau, 0, 2 ** 63 - 1, total=5,
                                     buffers={"view_count": ve})
    lists = _lists(env, c)
    n8 = torch.zeros(5 * c.N + 8, dtype=torch.uint8, device="cuda")
    first = c.N // 4 * 4 - 4                                                     # (a 4-byte aligned offset inside seen)
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        _raw(env, c, lists=lists, buffers={"seen": n8[:c.N], "count": n8[first:first + 4 * c.N].view(torch.int32)})
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        _raw(env, c, lists=lists, buffers={"seg": lists.view})


# ------------------------------------------------------------------------------------------ the status errors
def test_status_errors(env):
    ops, sparse = env
    c = lm.case("C19")
    P = _dev(c.points)
    for value, message in ((65536.0, "1 rows have a batch index"), (-1.0, "1 rows have a batch index"), (0.5, "1 rows have a batch index"),
                           (float("nan"), "1 rows of points are not finite"), (float("inf"), "1 rows of points are not finite")):
        bad = P.clone()
        bad[7, 0] = value
        with pytest.raises(ValueError, match=message):
            _lift(env, c, points=bad)
    for col, value in ((1, float("nan")), (2, float("-inf")), (3, float("inf"))):
        bad = P.clone()
        bad[3, col], bad[9, col] = value, value
        with pytest.raises(ValueError, match="2 rows of points are not finite"):
            _lift(env, c, points=bad)
    for value in (65536, -1, 2 ** 40):
        v = _views(sparse, c)
        v.view_entry = v.view_entry.clone()
        v.view_entry[1] = value
        with pytest.raises(ValueError, match="1 views have a view_entry outside 0..65535"):
            _lift(env, c, views=v)
    # the rows and views that are counted belong to no entry: the others' results do not change
    _, ref = _raw(env, c)
    bad = c.points.copy()
    bad[7, 0] = 70000.0
    ve = c.view_entry.copy()
    ve[c.views_of(1)[0]] = -5
    moved = lm.Case("moved", lb.Case("moved", bad, c.geo.maps, ve, c.w2c, c.intr, c.depth), c.pred_masks, c.pred_logits, c.mask_embed, c.text, c.scale)
    lists, r = _raw(env, moved)
    assert lists.status.tolist()[:3] == [1, 1, 0] and r.status.tolist()[:3] == [1, 1, 0] and r.status.tolist()[6:] == [0, 0]
    assert int(r.count[7]) == 0 and int(r.nn[7]) == -1 and not bool(r.out[7].any()) and int(lists.view_count[c.views_of(1)[0]]) == 0
    # (a point that left its entry may have been somebody's in-view source: the rows are compared with the per-scene kernels on the same
    # inputs, the counts of the points whose views all stayed with the first run)
    feats, seen, view_count, _ = _per_scene(env, moved)
    out = ops.gather_rows(r.out, r.out.shape[1], torch.where(r.nn >= 0, r.nn, torch.arange(c.N, device="cuda")))[:, :c.D]
    assert torch.equal(_bits(out), _bits(feats)) and torch.equal(r.seen.bool(), seen) and torch.equal(lists.view_count.cpu(), view_count)
    rows0 = _dev(np.setdiff1d(c.rows_of(0), [7]))
    assert torch.equal(r.count[rows0], ref.count[rows0])


def test_entries_that_are_not_lists_are_counted_and_take_no_part(env):
    """ops.lift_masks_batched takes entry arrays from anywhere: an entry whose view, point or pixel is not what the lists promise, and
    a view beyond the bit set's words, are counted in the status and left out; the call stays inside its extents."""
    ops, _ = env
    c = lm.case("views_130")
    lists, ref = _raw(env, c)
    off = lists.view_off.tolist()
    v = next(v for v in range(c.V) if off[v + 1] - off[v] >= 4 and bool(lists.view_keep[v]))
    e = off[v]
    pt, x, y, view = (t.clone() for t in (lists.pt, lists.x, lists.y, lists.view))
    view[e] = (v + 1) % c.V                                                      # another view than view_off says
    pt[e + 1] = c.N                                                              # no row
    x[e + 2] = c.H                                                               # no pixel
    broken = type(lists)(pt, x, y, view, lists.view_off, lists.view_count, lists.view_keep, lists.status, lists.total, lists.max_views)
    _, r = _raw(env, c, lists=broken)
    assert r.status.tolist()[6] >= 3 and r.status.tolist()[:3] == [0, 0, 0]
    hit = set(lists.pt[e:e + 4].tolist())
    same = _dev(np.array([p for p in range(c.N) if c.points[p, 0] != c.view_entry[v]]))
    assert torch.equal(r.count[same], ref.count[same]) and torch.equal(_bits(r.out[same]), _bits(ref.out[same])) and len(hit) == 4
    # one word holds 64 views of an entry: the other 66 of the 130 are counted and dropped
    f_seg, l_seg, _ = _tables(ops, _dev(c.mask_embed), _dev(c.text), c.scale)
    r1 = ops.lift_masks_batched(_dev(c.points), _dev(c.view_entry), _dev(c.pred_masks), _scores(_dev(c.pred_logits)), _taps(env, c), (c.H, c.W),
                                (lists.pt, lists.x, lists.y, lists.view), lists.view_off, lists.view_keep, lists.total, 1, f_seg, l_seg)
    assert r1.status.tolist()[7] == 66 and int(r1.count.max()) <= 64


# ------------------------------------------------------------------------------------------ limits
def test_limits(env):
    ops, sparse = env
    c = lm.case("C19")
    v = _views(sparse, c)
    v.pred_masks = torch.zeros((c.V, 1025, 2, 3), device="cuda")
    v.pred_logits, v.mask_embed = torch.zeros((c.V, 1025, c.C + 1), device="cuda"), torch.zeros((c.V, 1025, c.D), device="cuda")
    with pytest.raises(ValueError, match="1025 queries"):
        _lift(env, c, views=v)
    v = _views(sparse, c)
    v.pred_masks = torch.zeros((c.V, c.Q, c.H + 1, c.w), device="cuda")
    with pytest.raises(ValueError, match="larger than image_shape"):
        _lift(env, c, views=v)
    for field in ("pred_masks", "pred_logits", "mask_embed"):
        v = _views(sparse, c)
        setattr(v, field, getattr(v, field).requires_grad_())
        with pytest.raises(ValueError, match="require grad"):
            _lift(env, c, views=v)
    got = sparse.lift_masks(_dev(c.points).requires_grad_(), _views(sparse, c), _dev(c.text), c.scale, **_options(c))
    assert not got.features.requires_grad


def test_two_host_synchronisations(env):
    ops, sparse = env
    c = lm.case("views_130")
    points, views, text, kw = _dev(c.points), _views(sparse, c), _dev(c.text), _options(c)
    torch.cuda.synchronize()
    before = ops.READBACK["calls"]
    real = ops.readback
    torch.cuda.set_sync_debug_mode("error")
    try:
        # (the read-backs themselves are ops.readback's .tolist(), the only synchronising call allowed: count them, forbid every other)

        def counted(t):
            torch.cuda.set_sync_debug_mode("default")
            try:
                return real(t)
            finally:
                torch.cuda.set_sync_debug_mode("error")
        ops.readback = counted
        sparse._TAPS.clear()                                                     # the tap tables are built and uploaded inside the call too
        sparse.lift_masks(points, views, text, c.scale, **kw)
    finally:
        ops.readback = real
        torch.cuda.set_sync_debug_mode("default")
    assert ops.READBACK["calls"] == before + 2


# ------------------------------------------------------------------------------------------ the chain
def test_chain_lift_masks_quantize_purify_segment(env):
    """lift_masks -> quantize -> purify(student) -> segment on two small entries: it runs, the labels are labels and the counts add up"""
    ops, sparse = env
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import MinkowskiEngine as ME
    finally:
        sys.path.pop(0)
    from geopurify_amd import pipeline as pl
    from geopurify_amd.affinity_module import AffinityPredictor
    D, Cn = 64, 20
    c = lm.masks("chain", 26, {0: 400, 1: 500}, {0: 4, 1: 5}, Q=12, C=Cn, D=D)
    m = AffinityPredictor(D + 6, 128, 128)
    m.load_state_dict(pl.random_student_state_dict(D + 6, hidden=128, embed=128, num_blocks=4, seed=6))
    m = m.cuda()
    points = _dev(c.points)
    lifted = _lift(env, c)
    assert bool(lifted.seen.any()) and not bool(lifted.seen.all()) and bool(torch.isfinite(lifted.features).all())
    feats = torch.cat([lifted.features, points[:, 1:].float(), torch.ones((c.N, 3), device="cuda")], 1)
    q = sparse.quantize(points, feats, quantization_size=0.2)
    x = ME.SparseTensor(features=q.features, coordinates=q.coordinates)
    y = sparse.purify(m, x, feature_dim=D, K=24, num_iters=3)
    labels = torch.randint(0, Cn, (c.N,), generator=torch.Generator().manual_seed(3)).cuda()
    seg = sparse.segment(y, lifted.text_features, lifted.logit_scale, labels=labels, inverse_mapping=q.inverse_mapping)
    assert bool(torch.isfinite(y.F).all())
    assert seg.pred.shape == (c.N,) and int(seg.pred.min()) >= 0 and int(seg.pred.max()) < Cn
    assert seg.counts.shape == (2, 3, Cn) and int(seg.counts[:, 2].sum()) == c.N
    assert seg.counts[:, 2].sum(1).tolist() == [400, 500]
