"""The cases of tests/lift_labels_cases.py on the CPU: the per-entry reference (the oracle's mapper, np.bincount, np.argmax,
nn1_indices_bruteforce) against a whole-batch restatement with dense (point, view) tables that uses none of them, each case's own
conditions (a vote tie is a tie, a projection at x.5 is one, a fill tie is a tie in fp64, the all-ignored point is seen and unvoted),
and the refusals of sparse.lift_labels / LiftLabelsStream that precede the device check."""
import numpy as np
import pytest
import torch

import lift_labels_cases as ll

f32, f64 = np.float32, np.float64
FIELDS = ("labels", "labels_unfilled", "votes", "voted", "seen", "count", "view_count", "view_keep", "filled_from", "out_of_range")


@pytest.mark.parametrize("name", ll.CASES)
def test_reference_equals_the_restatement(name):
    c, ref = ll.case(name), ll.reference(name)
    again = ll.restatement(c)
    for k in FIELDS:
        assert np.array_equal(getattr(ref, k), getattr(again, k)), k
    assert ref.votes.dtype == np.int32 and ref.labels.dtype == np.int64 and ref.votes.shape == (c.N, c.C)
    assert np.array_equal(ref.voted, ref.votes.sum(1)) and np.all(ref.voted <= ref.count)
    unvoted = ref.voted == 0
    assert not ref.votes[ref.filled_from >= 0].any() and np.all(unvoted[ref.filled_from >= 0])
    assert np.all(ref.labels[unvoted & (ref.filled_from < 0)] == c.unlabeled)
    assert np.all((ref.labels_unfilled[~unvoted] >= 0) & (ref.labels_unfilled[~unvoted] < c.C))
    assert (ref.out_of_range > 0) == (name == "out_of_range_sampled")


def test_the_cases_cover_what_they_name():
    per_entry = lambda c: sorted(len(c.views_of(b)) for b in c.entries())      # noqa: E731
    assert per_entry(ll.case("views_0_1_63")) == [0, 1, 63] and per_entry(ll.case("views_64_65_C2")) == [64, 65]
    assert per_entry(ll.case("views_130_C200")) == [2, 130]
    assert sorted(ll.case(n).C for n in ("C1", "views_64_65_C2", "C63", "C64", "C65", "views_130_C200", "C1024")) == [1, 2, 63, 64, 65, 200, 1024]
    for n in ("views_0_1_63", "views_130_C200"):                                # view_entry interleaved, rows shuffled
        c = ll.case(n)
        assert np.any(np.diff(c.view_entry) < 0) and np.any(np.diff(c.points[:, 0]) < 0)
    c = ll.case("entries")
    assert c.entries().tolist() == [0, 2, 65535] and len(c.rows_of(0)) == 1
    c = ll.case("twins")
    a, b = c.points[c.rows_of(0), 1:], c.points[c.rows_of(1), 1:]
    assert np.array_equal(a, b)
    assert ll.case("no_depth").depth is None and ll.case("render").depth == "render" and isinstance(ll.case("entries").depth, np.ndarray)
    # some class C - 1 is voted for, and wins somewhere
    for n in ("C63", "C64", "C65", "C1024", "views_130_C200"):
        c, ref = ll.case(n), ll.reference(n)
        assert ref.votes[:, c.C - 1].any(), n
    # every case but the one made for it runs without an error; seen and unseen, voted and filled points exist
    for n in ("views_130_C200", "twins", "render"):
        ref = ll.reference(n)
        assert ref.seen.any() and not ref.seen.all() and (ref.filled_from >= 0).any()
    assert ll.reference("render").seen.sum() < ll.reference("render").seen.size


@pytest.mark.parametrize("name", ll.LARGE)
def test_the_large_cases_fill_from_voted_which_is_not_seen(name):
    """The fill of the label vote takes "voted" as its reference mask, the other lifts "seen": on the large geometries the two differ in
    an entry of more than 256 queries, so the blocks, runs and trips of the fill are not those of tests/lift_batched_cases.py"""
    import lift_batched_cases as lb
    assert name not in ll.CASES
    c, ref, dense = ll.case(name), ll.reference(name), lb.reference(name)
    assert np.array_equal(c.points, lb.case(name).points) and c.C <= 8 and np.isin(c.labels, c.ignore).mean() > 0.05
    assert np.array_equal(ref.seen, dense.seen) and np.array_equal(ref.view_count, dense.view_count) and ref.out_of_range == 0
    voted = ref.voted > 0
    assert not (voted & ~ref.seen).any()
    differ = [int(b) for b in c.entries() if (ref.seen & ~voted)[c.rows_of(b)].any() and int((~voted)[c.rows_of(b)].sum()) > 256
              and voted[c.rows_of(b)].any()]
    assert differ, "no entry of more than 256 queries in which voted differs from seen"
    rank, blocks = lb.fill_blocking(c, voted)
    rank_seen, _ = lb.fill_blocking(c, ref.seen)
    assert len(blocks) > 1 and max(b["hi"] - b["lo"] for b in blocks if b["lo"] is not None) > lb.FILL_TILE
    assert not np.array_equal(rank, rank_seen) and not np.array_equal(ref.filled_from, dense.filled_from)
    assert np.array_equal(ref.voted, ref.votes.sum(1)) and np.all(ref.voted <= ref.count)
    assert not ref.votes[ref.filled_from >= 0].any() and np.all(ref.labels[~voted & (ref.filled_from < 0)] == c.unlabeled)
    took = ref.filled_from >= 0
    assert np.array_equal(ref.labels[took], ref.labels_unfilled[ref.filled_from[took]]) and voted[ref.filled_from[took]].all()


def test_vote_ties_half_pixels_and_the_all_ignored_point():
    c, ref = ll.case("ties"), ll.reference("ties")
    row = {n: i for i, n in enumerate(c.notes["row_names"])}
    assert c.C == 65
    v = ref.votes[row["tie_63_64"]]
    assert v[63] == 2 and v[64] == 2 and v.sum() == 4 and ref.labels[row["tie_63_64"]] == 63          # a tie is a tie; the lowest class
    assert ref.votes[row["only_64"], 64] == 4 and ref.labels[row["only_64"]] == c.C - 1
    v = ref.votes[row["tie_0_64"]]
    assert v[0] == 2 and v[64] == 2 and ref.labels[row["tie_0_64"]] == 0
    i = row["all_ignored"]
    assert ref.seen[i] and ref.count[i] == 4 and ref.voted[i] == 0 and not ref.votes[i].any()            # seen and unvoted
    assert ref.labels_unfilled[i] == c.unlabeled and ref.filled_from[i] >= 0 and ref.labels[i] == ref.labels[ref.filled_from[i]]
    # the projection at x.5 is one: u = 8 x + 8 = 4.5 exactly, rounded half to even onto column 4 (7), not column 5 (9)
    i = row["half_to_even"]
    x, y, z = c.points[i, 1:]
    assert 8.0 * x / z + 8.0 == 4.5 and 8.0 * y / z + 6.0 == 5.0
    assert ref.votes[i, 7] == 4 and ref.votes[i, 9] == 0 and ref.labels[i] == 7
    for n in ("behind", "outside"):
        assert not ref.seen[row[n]] and ref.filled_from[row[n]] >= 0
    # the other entry's only point sits on tie_63_64's coordinates and votes for its own view's label
    assert np.array_equal(c.points[row["other_entry"], 1:], c.points[row["tie_63_64"], 1:]) and ref.labels[row["other_entry"]] == 33


def test_pixel_and_depth_edges():
    import lift_batched_cases as lb
    for name in ("pixels", "pixels_depth"):
        c, ref = ll.case(name), ll.reference(name)
        names = c.notes["row_names"]
        want = {r[0]: (r[5] if name == "pixels_depth" and len(r) > 5 else r[4]) for r in lb.pixel_rows()}
        for i, n in enumerate(names):
            if n in want and name == "pixels":
                assert bool(ref.seen[i]) == want[n], n
        row = {n: i for i, n in enumerate(names)}
        assert ref.seen[row["u_on_cut"]] and ref.seen[row["u_last"]] and not ref.seen[row["u_first_out"]] and not ref.seen[row["behind"]]
        if name == "pixels_depth":
            assert ref.seen[row["depth_equal_near"]] and ref.seen[row["depth_equal_far"]] and not ref.seen[row["depth_just_past"]]
            assert not ref.seen[row["half_to_even_down"]]
        # without ignored pixels a seen point has voted, once per view
        assert np.array_equal(ref.voted, ref.count)


def test_the_drop_rule_and_the_fill():
    c, ref = ll.case("drop"), ll.reference("drop")
    assert c.min_visible == 10 and c.max_visible == 20
    for v, n in c.notes["counts"].items():
        assert ref.view_count[v] == n and bool(ref.view_keep[v]) == (n in (10, 11, 20)), (v, n)
    c, ref = ll.case("fill"), ll.reference("fill")
    for q, src in c.notes["expect_from"].items():
        assert ref.filled_from[q] == src and ref.labels[q] == ref.labels_unfilled[src], q
    q, a, b = c.notes["tie"]
    xyz = c.points[:, 1:].astype(f32).astype(f64)
    d2 = lambda i, j: float(((xyz[i] - xyz[j]) ** 2)[:2].sum() + ((xyz[i] - xyz[j]) ** 2)[2])      # noqa: E731
    assert d2(q, a) == d2(q, b) and a < b and ref.filled_from[q] == a                               # a tie in fp64; the lower row
    assert ref.labels_unfilled[a] != ref.labels_unfilled[b] and ref.labels[q] == ref.labels_unfilled[a]
    q, other = c.notes["other_entry_nearer"]
    assert c.points[q, 0] != c.points[other, 0] and np.array_equal(xyz[q], xyz[other]) and ref.voted[other] > 0
    per = {int(b): ref.voted[c.rows_of(b)] > 0 for b in c.entries()}
    assert per[2].all() and not per[4].any() and len(c.views_of(4)) == 1 and not per[5].any() and len(c.views_of(5)) == 0
    assert np.all(ref.labels[c.rows_of(4)] == c.unlabeled) and np.all(ref.labels[c.rows_of(5)] == c.unlabeled)


def test_label_dtypes_and_the_range_cases():
    refs = [ll.reference(n) for n in ll.DTYPES]
    for n in ll.DTYPES[1:]:
        assert (ll.case(n).labels < 0).any() and ll.case(n).notes["holes"] > 0
    assert (ll.case("dtype_uint8").labels == 255).any()
    for r in refs[1:]:
        for k in FIELDS:
            assert np.array_equal(getattr(r, k), getattr(refs[0], k)), k
    assert (refs[0].voted < refs[0].count).any()                                # ignored pixels were sampled
    bad, ok = ll.case("out_of_range_sampled"), ll.case("out_of_range_unsampled")
    assert ll.reference("out_of_range_sampled").out_of_range >= 3 and (bad.labels < 0).any() and (bad.labels == bad.C).any()
    hit = ll.sampled_pixels(ok)
    outside = (ok.labels < 0) | (ok.labels >= ok.C)
    assert outside.any() and not (outside & hit).any() and ll.reference("out_of_range_unsampled").out_of_range == 0


def test_a_prefix_is_a_call_on_the_views_so_far():
    c = ll.case("twins")
    whole = ll.prefix_reference(c, np.arange(c.V))
    for k in FIELDS:
        assert np.array_equal(getattr(whole, k), getattr(ll.reference("twins"), k)), k
    part = ll.prefix_reference(c, [0, 1, 2])
    assert part.view_count.shape == (3,) and np.all(part.votes <= whole.votes) and (part.votes < whole.votes).any()


# ------------------------------------------------------------------------------------------ the refusals before the device check
def _views(sparse, c, **kw):
    t = torch.from_numpy
    f = dict(labels=t(c.labels), view_entry=t(c.view_entry), world_to_camera=t(c.w2c), intrinsics=t(c.intr),
             depth=c.depth if c.depth is None or isinstance(c.depth, str) else t(c.depth))
    f.update(kw)
    return sparse.LabelViews(f["labels"], f["view_entry"], f["world_to_camera"], f["intrinsics"], f["depth"])


def test_refusals_before_the_device_check():
    from geopurify_amd import sparse
    c = ll.case("no_depth")
    P = torch.from_numpy(c.points)
    lab = torch.from_numpy(c.labels)

    def refused(match, points=P, num_classes=c.C, views=None, **kw):
        with pytest.raises(ValueError, match=match):
            sparse.lift_labels(points, _views(sparse, c) if views is None else views, num_classes, **kw)

    refused("views must be a LabelViews", views=sparse.Views(lab, None, None, None))
    refused(r"points must be \[N, 4\]", points=P[:, :3])
    refused("points must be fp64 or fp32", points=P.to(torch.int64))
    refused(r"views.labels must be \[V, H, W\]", views=_views(sparse, c, labels=lab[0]))
    for bad in (lab.bool(), lab.float(), lab.double(), lab.half(), lab.to(torch.int8)):
        refused("views.labels must be uint8, int16, int32 or int64", views=_views(sparse, c, labels=bad))
    refused(r"views.view_entry must be an integer tensor", views=_views(sparse, c, view_entry=torch.from_numpy(c.view_entry).double()))
    refused(r"views.world_to_camera must be fp64", views=_views(sparse, c, world_to_camera=torch.from_numpy(c.w2c).float()))
    refused(r"views.intrinsics must be fp64", views=_views(sparse, c, intrinsics=torch.from_numpy(c.intr)[:, :3]))
    refused("views.depth", views=_views(sparse, c, depth="zbuffer"))
    refused(r"views.depth must be fp64", views=_views(sparse, c, depth=torch.zeros((c.V, c.H, c.W + 1), dtype=torch.float64)))
    refused("cut_bound=-1", cut_bound=-1)
    refused("vis_thres", vis_thres="a")
    refused("min_visible", min_visible=-1)
    for bad in (0, 1025, 2.0, True, None):
        refused("num_classes=.* must be an integer in 1..1024", num_classes=bad)
    refused("unlabeled=3 must be an integer outside", unlabeled=3)
    refused("unlabeled=255 must be an integer outside", num_classes=256)
    refused("ignore_labels", ignore_labels=(1.5,))
    refused("ignore_labels", ignore_labels=tuple(range(300, 317)))
    refused("ignore_labels", ignore_labels=255)
    refused("there is no CPU path")                                             # everything else is in order: the device check is the last
    with pytest.raises(ValueError, match="LiftLabelsStream: num_classes"):
        sparse.LiftLabelsStream(P, 0)
    with pytest.raises(ValueError, match="LiftLabelsStream: unlabeled"):
        sparse.LiftLabelsStream(P, 20, unlabeled=19)
    with pytest.raises(ValueError, match="LiftLabelsStream: .*no CPU path"):
        sparse.LiftLabelsStream(P, 20)
