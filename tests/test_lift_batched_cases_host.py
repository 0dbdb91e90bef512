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
    # generic cases hold seen and unseen points in one entry and more than one lift block (4 points).  The fill of every case in CASES
    # is ONE block of at most 256 queries and one LDS trip: more blocks and trips are the LARGE cases' (the tests further down)
    for name in ("views_130", "views_0_1_63", "D65", "no_depth"):
        c, ref = lb.case(name), lb.reference(name)
        mixed = [b for b in c.entries() if ref.seen[c.rows_of(b)].any() and not ref.seen[c.rows_of(b)].all()]
        assert mixed and (ref.filled_from >= 0).any(), name
    for name in lb.CASES:
        rank, blocks = lb.fill_blocking(lb.case(name), lb.reference(name).seen)
        assert len(blocks) <= 1 and all(b["lo"] is None or b["hi"] - b["lo"] <= lb.FILL_TILE for b in blocks), name
    assert not set(lb.LARGE) & set(lb.CASES)
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


# ------------------------------------------------------------------------------------------ the large cases hold what they are named for
def _trip(b, r):
    """the LDS trip of block b in which the reference of compacted position r is streamed"""
    return (r - b["lo"]) // lb.FILL_TILE


def _reference_structure(c, ref):
    """what test_reference_equals_the_whole_batch_restatement asserts beside the restatement (which takes minutes at these sizes)"""
    assert np.array_equal(ref.seen, ref.count > 0)
    idle = ~ref.seen & (ref.filled_from < 0)
    assert not ref.features[idle].any()
    took = np.nonzero(ref.filled_from >= 0)[0]
    assert np.array_equal(ref.features[took], ref.features[ref.filled_from[took]])
    assert (c.points[took, 0] == c.points[ref.filled_from[took], 0]).all() and ref.seen[ref.filled_from[took]].all()


def test_fill_blocks_spans_blocks_entries_and_trips():
    c, ref = lb.case("fill_blocks"), lb.reference("fill_blocks")
    _reference_structure(c, ref)
    assert c.depth is None and (c.H, c.W, c.D) == (12, 16, 3)
    assert (np.diff(c.view_entry) < 0).any() and (np.diff(c.view_entry) > 0).any() and (np.diff(c.points[:, 0]) < 0).any()
    # the plan, exactly: seen and unseen rows per entry
    assert sorted(c.entries()) == sorted(b for b, _, _ in lb.FILL_BLOCKS_PLAN) and 6 not in c.entries() and len(c.views_of(6)) == 1
    for b, n_seen, n_unseen in lb.FILL_BLOCKS_PLAN:
        rows = c.rows_of(b)
        want = n_seen if len(c.views_of(b)) else 0
        assert len(rows) == n_seen + n_unseen and int(ref.seen[rows].sum()) == want, b
        assert int((ref.filled_from[rows] >= 0).sum()) == (n_unseen if want else 0), b
    assert len(c.views_of(2)) == 1 and ref.view_count[c.views_of(2)[0]] == 0 and len(c.views_of(11)) == 0
    assert ref.seen[c.rows_of(3)].all() and ref.count[c.rows_of(0)].max() == 2
    rank, blocks = lb.fill_blocking(c, ref.seen)
    # more than one block, a partial last block
    assert len(blocks) == 11 and all(len(b["rows"]) == lb.FILL_BLOCK for b in blocks[:-1]) and 0 < len(blocks[-1]["rows"]) < lb.FILL_BLOCK
    # one block spans at least three entries; its range contains the run of an entry that has none of its queries; it holds queries
    # of an entry without references, and they are not filled
    run_of = {int(b): (int(rank[c.rows_of(b)][ref.seen[c.rows_of(b)]].min()), int(rank[c.rows_of(b)][ref.seen[c.rows_of(b)]].max()) + 1)
              for b in c.entries() if ref.seen[c.rows_of(b)].any()}
    wide = [b for b in blocks if len(np.unique(b["entry"])) >= 3]
    assert wide
    b = wide[0]
    assert sorted(np.unique(b["entry"])) == [1, 2, 4, 5]
    foreign = [e for e, (s, t) in run_of.items() if e not in b["entry"] and b["lo"] <= s and t <= b["hi"]]
    assert foreign == [3]
    bare = b["rows"][b["r1"] == b["r0"]]
    assert len(bare) == 40 and (c.points[bare, 0] == 2).all() and (ref.filled_from[bare] == -1).all()
    # an entry's run starts and ends strictly inside one trip of that block: entries 3 and 4 (the latter with queries in the block)
    for e in (3, 4):
        s, t = run_of[e]
        assert _trip(b, s) == _trip(b, t - 1) and (s - b["lo"]) % lb.FILL_TILE > 0 and (t - b["lo"]) % lb.FILL_TILE > 0 and t < b["hi"]
    # ... and entry 5's starts inside the first trip of the block and ends inside its third
    assert b["hi"] - b["lo"] > 2 * lb.FILL_TILE and _trip(b, run_of[5][0]) == 0 and (run_of[5][0] - b["lo"]) % lb.FILL_TILE > 0
    assert _trip(b, run_of[5][1] - 1) == 2
    # blocks with a range of more than two trips, in which the chosen references lie in every trip
    deep = [b for b in blocks if b["lo"] is not None and b["hi"] - b["lo"] > 2 * lb.FILL_TILE]
    assert len(deep) >= 6
    for b in deep:
        chosen = ref.filled_from[b["rows"]]
        trips = set(_trip(b, rank[chosen[chosen >= 0]]).tolist())
        assert trips == set(range(-(-(b["hi"] - b["lo"]) // lb.FILL_TILE))), trips
    # a later block of two trips in which a run (entry 9) starts inside the first trip and ends inside the second, before hi
    late = [b for b in blocks if 9 in b["entry"]]
    assert len(late) == 1 and lb.FILL_TILE < late[0]["hi"] - late[0]["lo"] <= 2 * lb.FILL_TILE
    s, t = run_of[9]
    assert _trip(late[0], s) == 0 and s > late[0]["lo"] and _trip(late[0], t - 1) == 1 and t < late[0]["hi"]
    assert sorted(np.unique(late[0]["entry"])) == [7, 9, 11, 65535] and c.entries().max() == 65535


def test_fill_tie_trips_ties_across_trips():
    c, ref = lb.case("fill_tie_trips"), lb.reference("fill_tie_trips")
    _reference_structure(c, ref)
    xyz = c.points[:, 1:].astype(f32).astype(f64)
    assert np.array_equal(xyz, c.points[:, 1:])                                  # dyadic: fp32 holds every coordinate
    d2 = lambda a, b: float((((xyz[a] - xyz[b]) ** 2)[0] + ((xyz[a] - xyz[b]) ** 2)[1]) + ((xyz[a] - xyz[b]) ** 2)[2])   # noqa: E731
    rank, blocks = lb.fill_blocking(c, ref.seen)
    assert len(blocks) == 1 and blocks[0]["lo"] == 37 and blocks[0]["hi"] - blocks[0]["lo"] >= 1200
    assert int(ref.seen[c.rows_of(3)].sum()) == lb.TIE_LINE - len(lb.TIE_GONE) and ref.seen[c.rows_of(0)].all()
    b = blocks[0]
    same = set(c.notes["same_trip"])
    pairs = set()
    assert len(c.notes["ties"]) >= 40 and len(same) == len(lb.TIE_GONE)
    for q, low, high in c.notes["ties"]:
        assert not ref.seen[q] and ref.seen[low] and ref.seen[high] and low < high and rank[low] < rank[high]
        assert d2(q, low) == d2(q, high)                                         # an exact tie in fp64 on the fp32-rounded xyz
        others = np.setdiff1d(np.nonzero(ref.seen & (c.points[:, 0] == 3))[0], [low, high])
        assert (((xyz[others] - xyz[q]) ** 2).sum(1) > d2(q, low)).all()          # ... and nobody is nearer or as near
        assert ref.filled_from[q] == low, q
        if (q, low, high) in same:
            assert _trip(b, rank[low]) == _trip(b, rank[high]) and rank[high] == rank[low] + 1
        else:
            assert rank[high] - rank[low] > lb.FILL_TILE and _trip(b, rank[low]) < _trip(b, rank[high])
            pairs.add((int(_trip(b, rank[low])), int(_trip(b, rank[high]))))
            # in space the lower row may lie on either side of the query
    assert pairs == {(0, 1), (0, 2), (1, 2)}
    side = {bool(xyz[low, 0] < xyz[q, 0]) for q, low, high in c.notes["ties"] if (q, low, high) not in same}
    assert side == {True, False}


def test_walk_trips_takes_second_trips():
    c, ref = lb.case("walk_trips"), lb.reference("walk_trips")
    _reference_structure(c, ref)
    rows = c.rows_of(1)
    assert len(rows) > lb.COUNT_TRIP and c.depth is not None
    per = -(-len(rows) // lb.WALK_PARTS)
    assert per > 256 and per * (lb.WALK_PARTS - 1) < len(rows) < per * lb.WALK_PARTS          # 64 parts, a short last one
    vs = c.views_of(1)
    assert len(vs) == 3
    first = {}
    for v in vs:
        pos = np.searchsorted(rows, ref.lists[int(v)][0])                        # the positions among the entry's sorted rows
        assert len(pos) == ref.view_count[v] and (pos >= lb.COUNT_TRIP).any()    # visible rows in the count loops' second trip
        assert (pos % per >= 256).any() and (pos % per < 256).any()              # ... and in the second trip of a part of the walk
        assert len(np.unique(pos // per)) == lb.WALK_PARTS                       # every part has visible rows
        first[int(v)] = int((pos < lb.COUNT_TRIP).sum())
    kept, dropped = [v for v in vs if ref.view_keep[v]], [v for v in vs if not ref.view_keep[v]]
    assert kept and dropped and c.min_visible == 0 and c.max_visible == lb.WALK_MAX_VISIBLE
    assert sorted(ref.view_count[vs].tolist()) == [2117, 2149, 2155]
    for v in dropped:                                                            # dropped by what the second trip counts
        assert first[int(v)] <= c.max_visible < ref.view_count[v]
    for v in kept:
        assert 0 < ref.view_count[v] <= c.max_visible
    rank, blocks = lb.fill_blocking(c, ref.seen)
    assert len(blocks) > 50 and max(b["hi"] - b["lo"] for b in blocks if b["lo"] is not None) > 2 * lb.FILL_TILE


def test_rows_past_table_lies_on_both_sides_of_the_table_length():
    c, ref = lb.case("rows_past_table"), lb.reference("rows_past_table")
    _reference_structure(c, ref)
    assert c.N == lb.ENTRY_TABLE + 300 and lb.ENTRY_TABLE == 65538
    assert len(c.views_of(1)) == 0 and len(c.rows_of(1)) == lb.ENTRY_TABLE
    assert not ref.seen[c.rows_of(1)].any() and (ref.filled_from[c.rows_of(1)] == -1).all() and not ref.features[c.rows_of(1)].any()
    order = np.argsort(c.points[:, 0], kind="stable")
    for b in (0, 2):
        rows = c.rows_of(b)
        assert len(c.views_of(b)) >= 2 and (rows < lb.ENTRY_TABLE).any() and (rows >= lb.ENTRY_TABLE).any(), b
        assert ref.seen[rows].any() and (ref.filled_from[rows] >= 0).any(), b
    # in the sorted order entry 2 lies wholly beyond the table's length: positions the checked copy's table threads do not reach
    assert (np.nonzero(c.points[order, 0] == 2)[0] >= lb.ENTRY_TABLE).all() and (np.nonzero(c.points[order, 0] == 0)[0] < 256).all()
    rank, blocks = lb.fill_blocking(c, ref.seen)
    assert len(blocks) > 256 and sum(b["lo"] is None for b in blocks) > 250


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
