"""CPU checks of tests/lift_batched_cases.py -- the cases and the reference that tests/test_gpu_lift_batched.py holds sparse.lift to --
and of sparse.lift's refusals that need no GPU.

The reference goes through the batch one entry at a time with the oracle's functions; restatement() is written once more over the
whole batch with dense (point, view) tables and none of them.  The two must agree exactly on every mask, count and index and on the
"nearest" features (the same fp32 adds in the same order); the "bilinear" features of the restatement are fp64 and must lie within 1e-6
of the reference's fp32 resize on maps in [-1, 1] (the bound tests/test_gpu_lift_edges.py holds the kernels to).  Then every case's own
conditions: a tie is a tie in fp64, a projection at x.5 is one, the drop rule meets its three counts.
"""
import numpy as np
import pytest
import torch

import lift_batched_cases as lb

f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("name", lb.CASES)
def test_reference_equals_the_whole_batch_restatement(name):
    c, ref = lb.case(name), lb.reference(name)
    feats, seen, count, view_count, view_keep, filled_from = lb.restatement(c)
    assert np.array_equal(seen, ref.seen) and np.array_equal(count, ref.count)
    assert np.array_equal(view_count, ref.view_count) and np.array_equal(view_keep, ref.view_keep)
    assert np.array_equal(filled_from, ref.filled_from)
    if c.mode == "nearest":
        assert feats.dtype == f32 and np.array_equal(feats, ref.features)
    else:
        assert np.abs(c.maps).max() <= 1.0
        assert np.abs(feats - ref.features.astype(f64)).max() <= 1e-6
    # structure: an unseen row that was not filled is zero, count and seen agree, a filled row carries its source's row
    assert np.array_equal(ref.seen, ref.count > 0)
    idle = ~ref.seen & (ref.filled_from < 0)
    assert not ref.features[idle].any()
    took = np.nonzero(ref.filled_from >= 0)[0]
    assert np.array_equal(ref.features[took], ref.features[ref.filled_from[took]])
    assert (c.points[took, 0] == c.points[ref.filled_from[took], 0]).all() and ref.seen[ref.filled_from[took]].all()


def test_the_cases_cover_what_they_are_named_for():
    per_entry = lambda c: sorted(len(c.views_of(b)) for b in c.entries())       # noqa: E731
    assert per_entry(lb.case("views_0_1_63")) == [0, 1, 63]
    assert per_entry(lb.case("views_64_65")) == [64, 65]
    assert per_entry(lb.case("views_130")) == [2, 130] and per_entry(lb.case("views_130_bilinear")) == [3, 130]
    widths = {lb.case(n).D for n in lb.CASES}
    assert {1, 3, 64, 65, 512, lb.col_chunk() + 1} <= widths
    for name in ("views_0_1_63", "views_64_65", "views_130", "twins"):
        c = lb.case(name)
        assert (np.diff(c.view_entry) < 0).any() and (np.diff(c.view_entry) > 0).any(), name      # interleaved
        assert (np.diff(c.points[:, 0]) < 0).any(), name                                        # rows in shuffled batch order
    shapes = {n: (lb.case(n).h, lb.case(n).w, lb.case(n).H, lb.case(n).W) for n in lb.BILINEAR}
    assert shapes["bilinear_h1"][0] == 1 and shapes["bilinear_w1"][1] == 1
    assert shapes["bilinear_H1"][2] == 1 and shapes["bilinear_W1"][3] == 1
    h, w, H, W = shapes["bilinear_ratio"]
    assert (H - 1) % (h - 1) and (W - 1) % (w - 1)                              # no integer ratio on either axis
    e = lb.case("entries")
    assert list(e.entries()) == [0, 2, 65535] and len(e.rows_of(0)) == 1
    # generic cases hold seen and unseen points in one entry, and more than one lift block (4 points) and fill block (256 queries)
    for name in ("views_130", "views_0_1_63", "D65", "no_depth"):
        c, ref = lb.case(name), lb.reference(name)
        mixed = [b for b in c.entries() if ref.seen[c.rows_of(b)].any() and not ref.seen[c.rows_of(b)].all()]
        assert mixed and (ref.filled_from >= 0).any(), name
    assert lb.reference("views_130").count.max() > 64                           # a point seen by more views than one ballot holds
    assert lb.reference("views_64_65").count.max() >= 2


def test_twins_do_not_mix():
    c, ref = lb.case("twins"), lb.reference("twins")
    a, b = c.rows_of(0), c.rows_of(1)
    assert np.array_equal(c.points[a, 1:], c.points[b, 1:])
    assert not np.array_equal(ref.seen[a], ref.seen[b]) and not np.array_equal(ref.features[a], ref.features[b])
    assert (c.points[ref.filled_from[ref.filled_from >= 0], 0] == c.points[ref.filled_from >= 0, 0]).all()


def test_pixel_rows_sit_where_they_are_named():
    c, ref = lb.case("pixels"), lb.reference("pixels")
    rows = lb.pixel_rows()
    x, y, z = c.points[:, 1], c.points[:, 2], c.points[:, 3]
    with np.errstate(all="ignore"):
        u, v = x * lb.PIXEL_FX / z + 8, y * lb.PIXEL_FX / z + 6
    want_u = {"u_on_cut": 2.0, "u_below_cut": 1.0, "u_last": 13.0, "u_first_out": 14.0, "half_to_even_down": 4.5, "half_to_even_up": 5.5,
              "half_onto_cut": 1.5, "half_to_cut_from_above": 2.5, "half_out": 13.5, "half_in": 12.5, "half_z2": 6.5, "behind": 9.0}
    for i, (name, *_rest, visible) in enumerate(rows):
        if name in want_u:
            assert u[i] == want_u[name], name                                    # exactly: the arithmetic is exact
        assert bool(ref.seen[i]) == visible, name
    names = [r[0] for r in rows]
    assert v[names.index("v_on_cut")] == 2.0 and v[names.index("v_last")] == 9.0 and v[names.index("v_first_out")] == 10.0
    assert c.cut == 2 and c.W - c.cut == 14 and c.H - c.cut == 10
    assert z[names.index("behind")] < 0 and z[names.index("on_the_camera_plane")] == 0
    # round half to even: 4.5 -> 4, 5.5 -> 6
    pt, px_row, px_col = ref.lists[0]
    col_of = dict(zip(pt.tolist(), px_col.tolist()))
    assert col_of[names.index("half_to_even_down")] == 4 and col_of[names.index("half_to_even_up")] == 6
    assert col_of[names.index("half_onto_cut")] == 2 and col_of[names.index("half_to_cut_from_above")] == 2 and col_of[names.index("half_in")] == 12


def test_depth_rows_sit_on_the_test():
    c, ref = lb.case("pixels_depth"), lb.reference("pixels_depth")
    names = c.notes["row_names"]
    z = c.points[:, 3]
    d = 2.0
    for name, visible in (("depth_equal_near", True), ("depth_equal_far", True), ("depth_just_past", False), ("depth_inside", True),
                          ("depth_negative", False), ("depth_negative_behind", False), ("half_to_even_down", False), ("half_to_even_up", True),
                          ("u_on_cut", True), ("u_first_out", False)):
        assert bool(ref.seen[names.index(name)]) == visible, name
    assert abs(d - z[names.index("depth_equal_near")]) == c.tau * d and abs(d - z[names.index("depth_equal_far")]) == c.tau * d
    assert abs(d - z[names.index("depth_just_past")]) > c.tau * d and z[names.index("depth_just_past")] - 2.5 == 2.0 ** -40
    assert (c.depth < 0).sum() == 2


def test_drop_rule_meets_its_counts():
    c, ref = lb.case("drop"), lb.reference("drop")
    assert (c.min_visible, c.max_visible) == (10, 20)
    for v, n in c.notes["counts"].items():
        assert ref.view_count[v] == n and bool(ref.view_keep[v]) == (n in (10, 11, 20)), (v, n)
    assert sorted(c.notes["counts"].values()) == [0, 9, 10, 11, 20, 21]          # just below, at, above; at and just above the maximum
    rows = c.rows_of(0)
    assert ref.count[rows].max() == 3 and ref.seen[rows].sum() == 20 and (ref.filled_from[rows] >= 0).sum() == 10
    assert ref.view_keep[c.views_of(3)].all()


def test_fill_conditions():
    c, ref = lb.case("fill"), lb.reference("fill")
    xyz = c.points[:, 1:].astype(f32).astype(f64)
    d2 = lambda a, b: float((((xyz[a] - xyz[b]) ** 2)[0] + ((xyz[a] - xyz[b]) ** 2)[1]) + ((xyz[a] - xyz[b]) ** 2)[2])   # noqa: E731
    for row, src in c.notes["expect_from"].items():
        assert ref.filled_from[row] == src and not ref.seen[row] and ref.seen[src], row
    q, a, b = c.notes["tie"]
    assert d2(q, a) == d2(q, b) and a < b and xyz[a, 0] > xyz[b, 0] and ref.filled_from[q] == a            # an exact tie in fp64: the lowest row
    q, r = c.notes["coincide"]
    assert d2(q, r) == 0.0 and c.points[q, 1] != c.points[r, 1] and ref.seen[r] and not ref.seen[q]         # equal in fp32 only
    q, r = c.notes["other_entry_nearer"]
    assert d2(q, r) == 0.0 and ref.seen[r] and c.points[q, 0] != c.points[r, 0] and d2(q, ref.filled_from[q]) > 0
    assert ref.seen[c.rows_of(2)].all() and not ref.seen[c.rows_of(4)].any() and len(c.views_of(4)) == 1
    assert len(c.views_of(5)) == 0 and not ref.features[c.rows_of(4)].any() and not ref.features[c.rows_of(5)].any()
    assert (ref.filled_from[c.rows_of(4)] == -1).all()


# ------------------------------------------------------------------------------------------ sparse.lift's refusals without a GPU
def _args(**over):
    from geopurify_amd import sparse
    c = lb.case("no_depth")
    t = dict(points=torch.from_numpy(c.points), features=torch.from_numpy(c.maps), view_entry=torch.from_numpy(c.view_entry),
             world_to_camera=torch.from_numpy(c.w2c), intrinsics=torch.from_numpy(c.intr), depth=None, image_shape=None)
    t.update(over)
    points = t.pop("points")
    return sparse, points, sparse.Views(**t)


@pytest.mark.parametrize("over, message", [
    (dict(points=torch.zeros(5, 3, dtype=torch.float64)), "points must be"),
    (dict(points=torch.zeros(5, 4, dtype=torch.int64)), "fp64 or fp32"),
    (dict(points=torch.zeros(5, 4, dtype=torch.float16)), "fp64 or fp32"),
    (dict(points=torch.zeros(0, 4, dtype=torch.float64)), "0 points"),
    (dict(features=torch.zeros(5, 3, 12)), "features must be"),
    (dict(features=torch.zeros(5, 3, 12, 16, dtype=torch.int32)), "floating point"),
    (dict(view_entry=torch.zeros(4, dtype=torch.int64)), "view_entry must be"),
    (dict(view_entry=torch.zeros(5)), "view_entry must be"),
    (dict(world_to_camera=torch.zeros(5, 3, 4, dtype=torch.float64)), "world_to_camera must be"),
    (dict(world_to_camera=torch.zeros(5, 4, 4)), "world_to_camera must be"),
    (dict(intrinsics=torch.zeros(5, 3, dtype=torch.float64)), "intrinsics must be"),
    (dict(intrinsics=torch.zeros(5, 4)), "intrinsics must be"),
    (dict(depth=torch.zeros(5, 12, 15, dtype=torch.float64)), "depth must be"),
    (dict(depth=torch.zeros(5, 12, 16)), "depth must be"),
    (dict(image_shape=(12,)), "image_shape"),
    (dict(image_shape=(24, 32)), "'nearest' samples"),
])
def test_lift_refuses_wrong_shapes_and_dtypes(over, message):
    sparse, points, views = _args(**over)
    with pytest.raises(ValueError, match=message):
        sparse.lift(points, views)


def test_lift_refuses_a_mode_typo_grad_maps_and_cpu_tensors():
    sparse, points, views = _args()
    with pytest.raises(ValueError, match="mode="):
        sparse.lift(points, views, mode="bilinaer")
    with pytest.raises(ValueError, match="views must be a Views"):
        sparse.lift(points, (views.features, views.view_entry))
    for kw in (dict(cut_bound=-1), dict(cut_bound=1.5), dict(min_visible=-1), dict(max_visible=2.5), dict(vis_thres="a")):
        with pytest.raises(ValueError, match="|".join(kw)):
            sparse.lift(points, views, **kw)
    with pytest.raises(ValueError, match="there is no CPU path"):
        sparse.lift(points, views)
    with pytest.raises(ValueError, match="there is no CPU path"):
        sparse.lift(points.float(), views, mode="bilinear")
    _, points, grad = _args(features=views.features.clone().requires_grad_())
    with pytest.raises(ValueError, match="require grad"):
        sparse.lift(points, grad)


def test_col_chunk_is_asked_of_the_library():
    assert lb.col_chunk() % 64 == 0 and lb.col_chunk() >= 64
