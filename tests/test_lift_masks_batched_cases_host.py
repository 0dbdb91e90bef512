"""CPU checks of tests/lift_masks_batched_cases.py -- the cases and the reference that tests/test_gpu_lift_masks_batched.py holds
sparse.lift_masks to -- and of sparse.lift_masks' refusals that need no GPU.

The reference goes through the batch one entry at a time with the oracle's functions (fp32, torch's resize); restatement() is written
once more over the whole batch with explicit loops, the resize through the tap tables and the fusion in fp64.  Off the rows the oracle
flags as near ties the two must agree exactly on every mask, count, index and segment, and within 1e-5 (tol_lift of oracle/parity.py;
a wrong pick differs by ~0.1) on the features.  The flags themselves are capped: at most 1 % of a case's rows or 2 rows, whichever is
larger, and none in the exact-arithmetic cases -- the cap is what keeps the GPU test from excusing a real failure.
"""
import numpy as np
import pytest
import torch

import lift_batched_cases as lb
import lift_masks_batched_cases as lm

f32, f64 = np.float32, np.float64
TOL_LIFT = 1e-5


def near_cap(c):
    return 0 if c.exact else max(2, c.N // 100)


@pytest.mark.parametrize("name", lm.CASES)
def test_reference_equals_the_whole_batch_restatement(name):
    c, ref = lm.case(name), lm.reference(name)
    s = lm.restatement(c)
    assert np.array_equal(s["view_count"], ref.view_count) and np.array_equal(s["view_keep"], ref.view_keep)
    assert np.array_equal(s["seen"], ref.seen) and np.array_equal(s["count"], ref.count) and np.array_equal(s["filled_from"], ref.filled_from)
    ok = ~ref.near
    for v, (rows, x, y, seg, src) in ref.views.items():
        assert np.array_equal(np.nonzero(s["seg"][:, v] != -2)[0], np.sort(rows) if ref.view_keep[v] else []), v
        if ref.view_keep[v]:
            assert (np.diff(rows) > 0).all()                                     # rows ascend inside a view
            sel = ok[rows]
            assert np.array_equal(s["seg"][rows, v][sel], seg[sel]) and np.array_equal(s["src"][rows, v][sel], src[sel]), v
    d = np.abs(s["features"] - ref.features.astype(f64)).max(1)
    assert d[ok].max() <= TOL_LIFT, (name, float(d[ok].max()))
    dp = np.abs(s["pre"] - ref.pre.astype(f64)).max(1)
    assert dp[ok].max() <= TOL_LIFT
    # structure
    assert np.array_equal(ref.seen, ref.count > 0) and not ref.pre[~ref.seen].any()
    idle = ~ref.seen & (ref.filled_from < 0)
    assert not ref.features[idle].any()
    took = np.nonzero(ref.filled_from >= 0)[0]
    assert np.array_equal(ref.features[took], ref.features[ref.filled_from[took]])
    assert (c.points[took, 0] == c.points[ref.filled_from[took], 0]).all() and ref.seen[ref.filled_from[took]].all()


@pytest.mark.parametrize("name", lm.CASES)
def test_the_reference_flags_few_near_ties(name):
    c, ref = lm.case(name), lm.reference(name)
    print(f"{name}: {int(ref.near.sum())} of {c.N} rows flagged")
    assert int(ref.near.sum()) <= near_cap(c)


@pytest.mark.parametrize("name", lm.LARGE)
def test_the_large_cases_flag_few_near_ties_and_share_the_dense_geometry(name):
    """the large geometries of tests/lift_batched_cases.py (no restatement: it takes minutes there): the same cap on the flags, and the
    masks, counts and the scene-level fill's choice are the dense reference's -- both fills follow "seen" """
    import lift_batched_cases as lb
    assert name not in lm.CASES
    c, ref, dense = lm.case(name), lm.reference(name), lb.reference(name)
    print(f"{name}: {int(ref.near.sum())} of {c.N} rows flagged")
    assert int(ref.near.sum()) <= near_cap(c)
    assert np.array_equal(ref.seen, dense.seen) and np.array_equal(ref.count, dense.count) and np.array_equal(ref.view_count, dense.view_count)
    assert np.array_equal(ref.view_keep, dense.view_keep) and np.array_equal(ref.filled_from, dense.filled_from)
    for v, (rows, x, y, seg, src) in ref.views.items():
        assert np.array_equal(rows, dense.lists[v][0]) and np.array_equal(x, dense.lists[v][1]) and np.array_equal(y, dense.lists[v][2]), v
    took = ref.filled_from >= 0
    assert np.array_equal(ref.features[took], ref.features[ref.filled_from[took]]) and not ref.features[~ref.seen & ~took].any()


def test_the_cases_cover_what_they_are_named_for():
    per_entry = lambda c: sorted(len(c.views_of(b)) for b in c.entries())       # noqa: E731
    assert per_entry(lm.case("views_0_1_63")) == [0, 1, 63] and per_entry(lm.case("views_64_65")) == [64, 65]
    assert per_entry(lm.case("views_128_129")) == [128, 129] and per_entry(lm.case("views_130")) == [2, 130]
    assert lm.case("views_64_65").V > 128 and max(per_entry(lm.case("views_64_65"))) <= 128      # two entries that sum above 128
    for name in ("views_0_1_63", "views_64_65", "views_128_129", "views_130", "twins"):
        c = lm.case(name)
        assert (np.diff(c.view_entry) < 0).any() and (np.diff(c.view_entry) > 0).any(), name      # interleaved
        assert (np.diff(c.points[:, 0]) < 0).any(), name                                        # rows in shuffled batch order
    assert lm.reference("views_130").count.max() > 64 and lm.reference("views_128_129").count.max() > 64      # the fusion's plain loops
    assert {lm.case(n).Q for n in lm.CASES} >= {1, 63, 64, 65, 200, 1024} and (lm.case("Q1024").h, lm.case("Q1024").w) == (2, 3)
    assert {lm.case(n).D for n in lm.CASES} >= {1, 4, 6, 65, 512} and {lm.case(n).C for n in lm.CASES} >= {1, 19, 65}
    c = lm.case("mask_full")
    assert (c.h, c.w) == (c.H, c.W) and lm.case("mask_h1").h == 1 and lm.case("mask_w1").w == 1
    e = lm.case("entries")
    assert list(e.entries()) == [0, 2, 5, 65535] and len(e.views_of(5)) == 0 and len(e.views_of(9)) == 2 and len(e.rows_of(9)) == 0
    assert not lm.reference("entries").features[e.rows_of(5)].any()
    # generic cases hold seen and unseen points in one entry, covered and uncovered entries in one view
    for name in ("views_130", "views_0_1_63", "Q1", "D65"):
        c, ref = lm.case(name), lm.reference(name)
        assert any(ref.seen[c.rows_of(b)].any() and not ref.seen[c.rows_of(b)].all() for b in c.entries()), name
        assert any((src >= 0).any() for *_, src in ref.views.values()), name


def test_score_cases():
    c, ref = lm.case("scores"), lm.reference("scores")
    scores = torch.softmax(torch.from_numpy(c.pred_logits), dim=-1)[..., :-1].max(-1).values.numpy()
    zero0, low1, zero2 = (c.views_of(b)[0] for b in (0, 1, 2))
    assert not scores[zero0].any() and not scores[zero2].any() and (scores[low1] > 0).all()
    resized = torch.nn.functional.interpolate(torch.from_numpy(c.pred_masks[low1])[None], size=(c.H, c.W), mode="bicubic", align_corners=False,
                                              antialias=True)[0]
    assert float(resized.max()) < -0.5                                           # far from sigmoid >= 0.5: no decision of this view is near
    for v in (zero0, low1, zero2):
        rows, _, _, seg, src = ref.views[int(v)]
        assert ref.view_keep[v] and len(rows) and (seg == -1).all() and (src == -1).all(), v
    # zero rows that are still seen: the points only no-cover views see -- all seen points of entry 2, some of entries 0 and 1
    r2 = c.rows_of(2)
    assert ref.seen[r2].any() and not ref.features[r2].any()
    for b, v in ((0, zero0), (1, low1)):
        only = [p for p in ref.views[int(v)][0] if ref.count[p] == 1]
        assert only and not ref.pre[only].any() and ref.seen[only].all(), b
        assert ref.pre[c.rows_of(b)].any()


def test_in_view_fill_conditions():
    c, ref = lm.case("fill_inview"), lm.reference("fill_inview")
    xyz = c.points[:, 1:].astype(f32).astype(f64)
    d2 = lambda a, b: float((((xyz[a] - xyz[b]) ** 2)[0] + ((xyz[a] - xyz[b]) ** 2)[1]) + ((xyz[a] - xyz[b]) ** 2)[2])   # noqa: E731
    for (row, v), (seg, src) in c.notes["expect"].items():
        rows, _, _, sg, sr = ref.views[v]
        i = int(np.nonzero(rows == row)[0][0])
        assert (sg[i], sr[i]) == (seg, src), (row, v)
    q, a, b = c.notes["tie"]
    assert d2(q, a) == d2(q, b) and a < b and xyz[a, 0] > xyz[b, 0]                # an exact tie in fp64; the lower row is not first in x
    q, r = c.notes["other_view_nearer"]
    assert d2(q, r) < d2(q, 0) and c.points[q, 0] == c.points[r, 0] and r not in ref.views[1][0] and q in ref.views[1][0]
    assert r in ref.views[0][0] and ref.views[0][3][list(ref.views[0][0]).index(r)] == 2
    q, r = c.notes["other_entry_nearer"]
    assert d2(q, r) == 0.0 and c.points[q, 0] != c.points[r, 0]
    assert ref.seen.all() and (ref.count == 1).all()
    # 257 uncovered entries in one view, every one filled from a covered entry of its view
    c, ref = lm.case("fill_257"), lm.reference("fill_257")
    rows, _, _, seg, src = ref.views[0]
    assert len(rows) == 257 + 12 and int((src >= 0).sum()) == 257 and (seg >= 0).all()
    assert set(src[src >= 0]) <= set(rows[src < 0]) and (c.points[rows, 0] == 0).all()
    assert len(set(seg[src >= 0])) == 2 and len(set(src[src >= 0])) >= 6         # both covered columns, many of their entries: somebody's nearest


def test_scene_fill_twins_and_drop_are_the_dense_situations():
    for name in ("fill", "twins", "drop"):
        ref, dense = lm.reference(name), lb.reference(name)
        assert np.array_equal(ref.seen, dense.seen) and np.array_equal(ref.count, dense.count)
        assert np.array_equal(ref.filled_from, dense.filled_from) and np.array_equal(ref.view_keep, dense.view_keep)
    c, ref = lm.case("fill"), lm.reference("fill")
    for row, src in c.geo.notes["expect_from"].items():
        assert ref.filled_from[row] == src
    c, ref = lm.case("twins"), lm.reference("twins")
    a, b = c.rows_of(0), c.rows_of(1)
    assert np.array_equal(c.points[a, 1:], c.points[b, 1:]) and not np.array_equal(ref.features[a], ref.features[b])
    c, ref = lm.case("drop"), lm.reference("drop")
    for v, n in c.geo.notes["counts"].items():
        assert ref.view_count[v] == n and bool(ref.view_keep[v]) == (n in (10, 11, 20))


def test_the_same_size_resize_is_the_identity():
    from geopurify_amd.bicubic import aa_bicubic_taps
    for n in (lm.FILL_W, lm.FILL_H):
        x0, w = aa_bicubic_taps(n, n)
        for i in range(n):
            taps = {min(x0[i] + j, n - 1): w[i, j] for j in range(4) if w[i, j] != 0}
            assert taps == {i: f32(1)}, (n, i, taps)


# ------------------------------------------------------------------------------------------ sparse.lift_masks' refusals without a GPU
def _args(**over):
    from geopurify_amd import sparse
    c = lm.case("C19")
    t = dict(points=torch.from_numpy(c.points), pred_masks=torch.from_numpy(c.pred_masks), pred_logits=torch.from_numpy(c.pred_logits),
             mask_embed=torch.from_numpy(c.mask_embed), view_entry=torch.from_numpy(c.view_entry), world_to_camera=torch.from_numpy(c.w2c),
             intrinsics=torch.from_numpy(c.intr), depth=None, image_shape=(c.H, c.W), text_embed=torch.from_numpy(c.text))
    t.update(over)
    points, text = t.pop("points"), t.pop("text_embed")
    return sparse, points, sparse.MaskViews(**t), text


@pytest.mark.parametrize("over, message", [
    (dict(points=torch.zeros(5, 3, dtype=torch.float64)), "points must be"),
    (dict(points=torch.zeros(5, 4, dtype=torch.int64)), "fp64 or fp32"),
    (dict(points=torch.zeros(0, 4, dtype=torch.float64)), "0 points"),
    (dict(pred_masks=torch.zeros(5, 5, 6)), "pred_masks must be"),
    (dict(pred_masks=torch.zeros(5, 5, 6, 8, dtype=torch.float64)), "pred_masks must be"),
    (dict(pred_masks=torch.zeros(5, 1025, 2, 3)), "1025 queries"),
    (dict(pred_masks=torch.zeros(5, 5, 13, 8)), "larger than image_shape"),
    (dict(pred_masks=torch.zeros(5, 5, 6, 17)), "larger than image_shape"),
    (dict(pred_logits=torch.zeros(5, 5, 19)), "pred_logits must be"),
    (dict(mask_embed=torch.zeros(5, 5, 5)), "mask_embed must be"),
    (dict(text_embed=torch.zeros(19)), "text_embed must be"),
    (dict(view_entry=torch.zeros(4, dtype=torch.int64)), "view_entry must be"),
    (dict(world_to_camera=torch.zeros(5, 4, 4)), "world_to_camera must be"),
    (dict(intrinsics=torch.zeros(5, 3, dtype=torch.float64)), "intrinsics must be"),
    (dict(depth=torch.zeros(5, 12, 15, dtype=torch.float64)), "depth must be"),
    (dict(image_shape=None), "image_shape"),
    (dict(image_shape=(12,)), "image_shape"),
])
def test_lift_masks_refuses_wrong_shapes_and_dtypes(over, message):
    sparse, points, views, text = _args(**over)
    with pytest.raises(ValueError, match=message):
        sparse.lift_masks(points, views, text, 14.25)


def test_lift_masks_refuses_grad_inputs_bad_options_and_cpu_tensors():
    sparse, points, views, text = _args()
    with pytest.raises(ValueError, match="views must be a MaskViews"):
        sparse.lift_masks(points, sparse.Views(views.pred_masks, views.view_entry, views.world_to_camera, views.intrinsics), text, 14.25)
    for kw in (dict(cut_bound=-1), dict(min_visible=-1), dict(max_visible=2.5), dict(vis_thres="a")):
        with pytest.raises(ValueError, match="|".join(kw)):
            sparse.lift_masks(points, views, text, 14.25, **kw)
    with pytest.raises(ValueError, match="logit_scale"):
        sparse.lift_masks(points, views, text, "a")
    with pytest.raises(ValueError, match="there is no CPU path"):
        sparse.lift_masks(points, views, text, 14.25)
    for field in ("pred_masks", "pred_logits", "mask_embed"):
        _, points, grad, text = _args(**{field: getattr(views, field).clone().requires_grad_()})
        with pytest.raises(ValueError, match="require grad"):
            sparse.lift_masks(points, grad, text, 14.25)
    with pytest.raises(ValueError, match="text_embed require grad"):
        sparse.lift_masks(points, views, text.clone().requires_grad_(), 14.25)
