"""CPU checks of tests/lift_stream_cases.py: every partition is what its name claims, so that tests/test_gpu_lift_stream.py exercises
the chunk boundaries it means to.  No GPU.
"""
import numpy as np
import pytest

import lift_batched_cases as lb
import lift_stream_cases as ls


def _kinds(name):
    c = lb.case(name)
    kinds = list(ls.EVERY_CASE) + ["by_entry"]
    if name in ls.BOUNDARY_CASES:
        kinds += list(ls.BOUNDARIES)
    return c, kinds


@pytest.mark.parametrize("name", lb.CASES)
def test_every_view_is_in_one_chunk_and_an_entrys_views_keep_their_order(name):
    c, kinds = _kinds(name)
    for kind in kinds:
        chunks = ls.partition(c, kind)
        assert all(len(ch) >= 1 and ch.dtype == np.int64 for ch in chunks), kind
        order = ls.concatenation(chunks)
        assert np.array_equal(np.sort(order), np.arange(c.V)), kind             # every view, once
        for b in np.unique(c.view_entry):
            assert np.array_equal(order[c.view_entry[order] == b], c.views_of(b)), (kind, b)   # ascending inside the entry
        if kind != "by_entry":
            assert np.array_equal(order, np.arange(c.V)), kind                   # slices of the global order
    assert len(ls.partition(c, "whole")) == 1
    assert [len(ch) for ch in ls.partition(c, "singles")] == [1] * c.V
    sizes = [len(ch) for ch in ls.partition(c, "random")]
    assert all(1 <= s <= ls.RANDOM_MAX for s in sizes) and (len(sizes) >= 2 or c.V == 1)
    assert [len(ch) for ch in ls.partition(c, "random")] == sizes                # seeded: the same again
    by_entry = ls.partition(c, "by_entry")
    assert [set(c.view_entry[ch]) for ch in by_entry] == [{b} for b in np.unique(c.view_entry)]


def test_random_partitions_use_all_sizes_and_by_entry_reorders():
    sizes = [len(ch) for ch in ls.partition(lb.case("views_130"), "random")]
    assert set(sizes[:-1]) == set(range(1, ls.RANDOM_MAX + 1))
    for name in ("views_130", "views_64_65", "twins"):                            # interleaved view_entry: by_entry is no slice
        order = ls.concatenation(ls.partition(lb.case(name), "by_entry"))
        assert not np.array_equal(order, np.arange(len(order))), name


@pytest.mark.parametrize("name", ls.BOUNDARY_CASES)
def test_the_boundaries_fall_on_63_64_65(name):
    c = lb.case(name)
    b = ls.widest_entry(c)
    assert len(c.views_of(b)) >= 65 and len(c.views_of(b)) == max(len(c.views_of(e)) for e in np.unique(c.view_entry))
    for kind, k in ls.BOUNDARIES.items():
        chunks = ls.partition(c, kind)
        first = chunks[0]
        assert int((c.view_entry[first] == b).sum()) == k, kind                  # the entry has received exactly k views ...
        assert c.view_entry[first[-1]] == b, kind                                # ... and the chunk ends with the k-th
        rest = len(c.views_of(b)) - k
        assert len(chunks) == (2 if len(first) < c.V else 1)
        if len(chunks) == 2:
            assert int((c.view_entry[chunks[1]] == b).sum()) == rest
    # below, on and above one lane group of 64 views: the first chunk of the widest entry is a partial group, a full group, a full
    # group and one view of the next; the second chunk of views_130 continues with 67 / 66 / 65 views
    if name != "views_64_65":
        assert [len(c.views_of(b)) - k for k in ls.BOUNDARIES.values()] == [67, 66, 65]


def test_the_idle_chunks_hold_only_dropped_or_pointless_views():
    c = ls.idle_case()
    base = lb.case("drop")
    rest, dropped, pointless = ls.idle_partition()
    assert np.array_equal(np.sort(ls.concatenation([rest, dropped, pointless])), np.arange(c.V))
    counts = base.notes["counts"]
    assert sorted(counts.values()) == sorted(lb.DROP_COUNTS)
    assert sorted(counts[int(v)] for v in dropped) == sorted(ls.IDLE_DROPPED) == [0, 9, 21]
    assert base.min_visible == 10 and base.max_visible == 20
    assert not any(lb.keep_rule(base, counts[int(v)]) for v in dropped)
    assert all(lb.keep_rule(base, counts[int(v)]) for v in rest if int(v) in counts)
    assert len(pointless) == 2 and (c.view_entry[pointless] == ls.IDLE_ENTRY).all() and len(c.rows_of(ls.IDLE_ENTRY)) == 0
    # the reference agrees: the dropped views have the counts above and are not kept, the pointless ones count nothing
    ref = ls.reference_of(c, np.arange(c.V))
    assert [int(ref.view_count[v]) for v in dropped] == [counts[int(v)] for v in dropped] and not ref.view_keep[dropped].any()
    assert not ref.view_count[pointless].any() and not ref.view_keep[pointless].any()
    assert ref.view_keep[rest].all()
    # ... and an idle chunk changes nothing: the reference of every prefix that ends before, inside or after the idle chunks is the same
    order = ls.concatenation([rest, dropped, pointless])
    r0 = ls.reference_of(c, rest)
    for upto in (len(rest) + len(dropped), len(order)):
        r = ls.reference_of(c, order[:upto])
        assert np.array_equal(r.features.view(np.int32), r0.features.view(np.int32)) and np.array_equal(r.count, r0.count)
        assert np.array_equal(r.seen, r0.seen) and np.array_equal(r.filled_from, r0.filled_from)
        assert np.array_equal(r.view_count[:len(rest)], r0.view_count) and not r.view_keep[len(rest):].any()


@pytest.mark.parametrize("name", ["twins", "drop", "fill", "no_depth"])
def test_a_prefix_reference_is_the_reference_of_the_truncated_case(name):
    """What a snapshot after k chunks must equal: lift_batched_cases._reference on the case truncated to those chunks' views.  Its
    per-view fields are the full reference's (a view's count and keep depend on that view alone), its point counts are the sums over the
    kept views of the prefix of their visible lists, and the last prefix is the full reference."""
    c, full = lb.case(name), lb.reference(name)
    chunks = ls.partition(c, "random")
    for k in range(1, len(chunks) + 1):
        order = ls.concatenation(chunks[:k])
        r = ls.reference_of(c, order)
        assert np.array_equal(r.view_count, full.view_count[order]) and np.array_equal(r.view_keep, full.view_keep[order])
        count = np.zeros(c.N, np.int32)
        for v in order:
            if full.view_keep[v]:
                count[full.lists[int(v)][0]] += 1
        assert np.array_equal(r.count, count) and np.array_equal(r.seen, count > 0)
    assert np.array_equal(r.features.view(np.int32), full.features.view(np.int32)) and np.array_equal(r.filled_from, full.filled_from)


def test_subcase_keeps_everything_but_the_views():
    c = lb.case("views_130_bilinear")
    order = ls.concatenation(ls.partition(c, "by_entry"))
    s = ls.subcase(c, order)
    assert s.points is not None and np.array_equal(s.points, c.points) and (s.H, s.W, s.h, s.w) == (c.H, c.W, c.h, c.w)
    assert (s.mode, s.cut, s.tau, s.min_visible, s.max_visible) == (c.mode, c.cut, c.tau, c.min_visible, c.max_visible)
    assert np.array_equal(s.maps, c.maps[order]) and np.array_equal(s.view_entry, c.view_entry[order])
    assert np.array_equal(s.depth, c.depth[order]) and np.array_equal(s.w2c, c.w2c[order]) and np.array_equal(s.intr, c.intr[order])
    assert [len(ch) for ch in ls.equal_chunks(lb.case("views_130"), 8)] == [16] * 8
