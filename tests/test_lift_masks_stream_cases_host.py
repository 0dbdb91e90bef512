"""CPU checks of tests/lift_masks_stream_cases.py: every partition is what its name claims, so that tests/test_gpu_lift_masks_stream.py
exercises the chunk boundaries it means to.  No GPU.
"""
import numpy as np
import pytest

import lift_masks_batched_cases as lm
import lift_masks_stream_cases as ms


@pytest.mark.parametrize("name", ms.CASES + ms.BOUNDARY_CASES)
def test_every_view_is_in_one_chunk_and_an_entrys_views_keep_their_order(name):
    c = lm.case(name)
    kinds = list(ms.EVERY_CASE) + ["by_entry"] + (list(ms.BOUNDARIES) if name in ms.BOUNDARY_CASES else [])
    for kind in kinds:
        chunks = ms.partition(c, kind)
        assert all(len(ch) >= 1 and ch.dtype == np.int64 for ch in chunks), kind
        order = ms.concatenation(chunks)
        assert np.array_equal(np.sort(order), np.arange(c.V)), kind             # every view, exactly once
        for b in np.unique(c.view_entry):
            assert np.array_equal(order[c.view_entry[order] == b], c.views_of(b)), (kind, b)   # ascending inside the entry
        if kind != "by_entry":
            assert np.array_equal(order, np.arange(c.V)), kind                   # slices of the global order
    assert [len(ch) for ch in ms.partition(c, "singles")] == [1] * c.V
    sizes = [len(ch) for ch in ms.partition(c, "random")]
    assert all(1 <= s <= 7 for s in sizes) and (len(sizes) >= 2 or c.V == 1)
    assert [len(ch) for ch in ms.partition(c, "random")] == sizes                # seeded: the same again


@pytest.mark.parametrize("name", ms.BOUNDARY_CASES)
def test_the_boundaries_leave_the_widest_entrys_counter_at_63_64_65(name):
    """the position of the entry's next view is its counter: 63 is the last bit of the bit set's first word, 64 the first of the second"""
    c = lm.case(name)
    b = ms.widest_entry(c)
    assert len(c.views_of(b)) >= 65 and len(c.views_of(b)) == max(len(c.views_of(e)) for e in np.unique(c.view_entry))
    for kind, k in ms.BOUNDARIES.items():
        chunks = ms.partition(c, kind)
        first = chunks[0]
        assert int((c.view_entry[first] == b).sum()) == k and c.view_entry[first[-1]] == b, kind
        assert len(chunks) == (2 if len(first) < c.V else 1)
        if len(chunks) == 2:
            positions = k + np.arange(int((c.view_entry[chunks[1]] == b).sum()))  # of the entry's views in the second chunk
            assert positions[0] // 64 == (0 if k == 63 else 1) and positions[-1] == len(c.views_of(b)) - 1
    assert -(-len(c.views_of(b)) // 64) >= 2                                      # more than one word


@pytest.mark.parametrize("name", ms.BOUNDARY_CASES)
def test_by_entry_reorders_and_its_reference_has_seen_and_unseen_points(name):
    c = lm.case(name)
    order = ms.concatenation(ms.partition(c, "by_entry"))
    assert not np.array_equal(order, np.arange(c.V))                             # interleaved view_entry: by_entry is no slice
    s = ms.subcase(c, order)
    assert np.array_equal(s.pred_masks, c.pred_masks[order]) and np.array_equal(s.pred_logits, c.pred_logits[order])
    assert np.array_equal(s.mask_embed, c.mask_embed[order]) and np.array_equal(s.view_entry, c.view_entry[order])
    assert np.array_equal(s.w2c, c.w2c[order]) and np.array_equal(s.intr, c.intr[order]) and np.array_equal(s.depth, c.depth[order])
    assert np.array_equal(s.points, c.points) and (s.H, s.W, s.cut, s.tau) == (c.H, c.W, c.cut, c.tau) and s.text is c.text
    ref = ms.reference_of(c, order)
    assert np.isfinite(ref.features).all()
    assert any(ref.seen[c.rows_of(b)].any() and not ref.seen[c.rows_of(b)].all() for b in c.entries())
    full = lm.reference(name)                                                    # a view's own fields do not depend on the order
    assert np.array_equal(ref.view_count, full.view_count[order]) and np.array_equal(ref.view_keep, full.view_keep[order])
    assert np.array_equal(ref.count, full.count) and np.array_equal(ref.seen, full.seen)


def test_the_idle_chunks_hold_only_dropped_or_pointless_views():
    c, base = ms.idle_case(), lm.case("drop")
    rest, dropped, pointless = ms.idle_partition()
    assert np.array_equal(np.sort(ms.concatenation([rest, dropped, pointless])), np.arange(c.V)) and c.V == base.V + 2
    assert len(pointless) == 2 and (c.view_entry[pointless] == ms.IDLE_ENTRY).all() and len(c.rows_of(ms.IDLE_ENTRY)) == 0
    assert np.array_equal(c.pred_masks[pointless], base.pred_masks[:2]) and np.array_equal(c.mask_embed[:base.V], base.mask_embed)
    ref = ms.reference_of(c, np.arange(c.V))
    assert sorted(int(ref.view_count[v]) for v in dropped) == sorted(ms.IDLE_DROPPED) and not ref.view_keep[dropped].any()
    assert not ref.view_count[pointless].any() and not ref.view_keep[pointless].any() and ref.view_keep[rest].all()
    # an idle chunk changes nothing: the reference of the prefix that ends before the idle chunks is the reference of all
    r0 = ms.reference_of(c, rest)
    assert np.array_equal(ref.features.view(np.int32), r0.features.view(np.int32)) and np.array_equal(ref.count, r0.count)
    assert np.array_equal(ref.seen, r0.seen) and np.array_equal(ref.filled_from, r0.filled_from)
