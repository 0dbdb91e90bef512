"""Partitions of the cases of tests/lift_masks_batched_cases.py into chunks of views, for sparse.LiftMasksStream
(csrc/lift_masks_stream.hip).  numpy on the CPU, no device code.

The partitions are those of tests/lift_stream_cases.py (a mask case answers V, view_entry, views_of and name like the dense case it is
built on): whole, singles, random (seeded, chunks of at most 7), at_63 / at_64 / at_65, by_entry.  The stream's contract is stated on
the CONCATENATION of the chunks: finish() equals sparse.lift_masks -- and the reference of lift_masks_batched_cases -- on subcase(case,
concatenation(chunks)), the case with all its per-view arrays taken in that order.

What the boundary kinds cut here: the stream gives every view its POSITION INSIDE ITS ENTRY (the entry's view counter before the chunk
plus the view's rank inside the chunk), and finish sets bit `position` of the point's bit set of 64-bit words.  A first chunk that ends
with the widest entry's 63rd / 64th / 65th view leaves that entry's counter at 63 / 64 / 65: the next chunk starts on the last bit of
the first word, on the first bit of the second word, and one bit into it.

  idle       on idle_case() ("drop" with two more views of an entry without points, VLM outputs attached): the ordinary views, then a
             chunk of dropped views only, then a chunk of views whose entry has no points
"""
import numpy as np

import lift_masks_batched_cases as lm
import lift_stream_cases as ls
from lift_stream_cases import BOUNDARIES, EVERY_CASE, IDLE_DROPPED, IDLE_ENTRY, KINDS, concatenation, partition, widest_entry   # noqa: F401

# the cases of the bit-equality test: every case x EVERY_CASE, the boundary cases x the boundary kinds and by_entry
CASES = ("views_0_1_63", "scores", "drop", "entries", "fill", "twins", "fill_inview", "fill_257", "D6", "D65", "C19", "Q65", "mask_full")
BOUNDARY_CASES = ("views_64_65", "views_128_129", "views_130")


def subcase(c, order, name=None):
    """the mask case with its views `order` (a selection, a truncation, a reordering): every per-view array, everything else as it is"""
    o = np.asarray(order, np.int64)
    return lm.Case(name or f"{c.name}[{len(o)} views]", ls.subcase(c.geo, o), c.pred_masks[o], c.pred_logits[o], c.mask_embed[o], c.text, c.scale,
                   exact=c.exact)


_REFERENCES = {}


def reference_of(c, order):
    """lift_masks_batched_cases._reference on subcase(c, order): computed once per (case, order) and shared; callers must not change it"""
    key = (c.name, np.asarray(order, np.int64).tobytes())
    if key not in _REFERENCES:
        _REFERENCES[key] = lm._reference(subcase(c, order))
    return _REFERENCES[key]


# ------------------------------------------------------------------------------------------ the idle chunks
_IDLE = {}


def idle_case():
    """lift_stream_cases.idle_case() -- "drop" with two more views, copies of its first two, that look at an entry without points --
    with the VLM outputs of the mask case "drop", the two copies included"""
    if "case" not in _IDLE:
        c, geo = lm.case("drop"), ls.idle_case()
        o = np.asarray(list(range(c.V)) + [0, 1], np.int64)
        assert geo.V == len(o) and np.array_equal(geo.points, c.points)
        _IDLE["case"] = lm.Case("drop_idle", geo, c.pred_masks[o], c.pred_logits[o], c.mask_embed[o], c.text, c.scale)
    return _IDLE["case"]


def idle_partition():
    """-> [ordinary views, the dropped views of entry 0, the views of the entry without points] (lift_stream_cases.idle_partition)"""
    return ls.idle_partition()
