"""Partitions of the cases of tests/lift_batched_cases.py into chunks of views, for sparse.LiftStream (csrc/lift_stream.hip).  numpy on
the CPU, no device code.

A partition is a list of chunks, a chunk an int64 array of view indices of the case, in the order the chunk hands them over.  The
stream's contract is stated on the CONCATENATION of the chunks: finish() equals sparse.lift -- and the reference of
lift_batched_cases -- on subcase(case, concatenation(chunks)), the case with its views taken in that order.  Every partition keeps
an entry's views in their ascending order (built from case.views_of(b) or from slices of the global order), which is all the lift's
sum depends on.

  whole      one chunk
  singles    every view its own chunk
  at_63 / at_64 / at_65   for the entry with the most views: a first chunk that ends exactly with that entry's 63rd / 64th / 65th
             view, then the rest -- the boundary below, on and above the 64-view lane group of the accumulating kernel
  by_entry   one chunk per entry with all its views: no slice of the global order, the concatenation is a reordering
  random     consecutive chunks of 1..7 views from a seeded generator (1..ceil(V / 2) for a case of fewer than 14 views, so that every
             case of two views or more is cut at least once)
  idle       on idle_case() ("drop" plus two views of an entry without points): the ordinary views, then a chunk of dropped views only,
             then a chunk of views whose entry has no points
"""
import zlib

import numpy as np

import lift_batched_cases as lb

EVERY_CASE = ("whole", "singles", "random")
BOUNDARIES = {"at_63": 63, "at_64": 64, "at_65": 65}
BOUNDARY_CASES = ("views_64_65", "views_130", "views_130_bilinear")
KINDS = EVERY_CASE + tuple(BOUNDARIES) + ("by_entry",)
RANDOM_MAX = 7
IDLE_ENTRY = 7                                        # an entry of idle_case() that has views and no points
IDLE_DROPPED = (9, 21, 0)                             # the counts of "drop" that the rule min_visible = 10, max_visible = 20 drops


def _ix(a):
    return np.asarray(a, np.int64)


def widest_entry(c):
    """the entry with the most views (the lowest among equals)"""
    ids, counts = np.unique(c.view_entry, return_counts=True)
    return int(ids[np.argmax(counts)])


def partition(c, kind):
    V = c.V
    if kind == "whole":
        return [np.arange(V, dtype=np.int64)]
    if kind == "singles":
        return [_ix([v]) for v in range(V)]
    if kind in BOUNDARIES:
        vs = c.views_of(widest_entry(c))
        cut = int(vs[BOUNDARIES[kind] - 1]) + 1       # (IndexError: the case has no entry with that many views)
        return [ch for ch in (np.arange(cut, dtype=np.int64), np.arange(cut, V, dtype=np.int64)) if len(ch)]
    if kind == "by_entry":
        return [_ix(c.views_of(b)) for b in np.unique(c.view_entry)]
    if kind == "random":
        rng = np.random.default_rng(zlib.crc32(c.name.encode()))
        most = min(RANDOM_MAX, (V + 1) // 2)
        chunks, v = [], 0
        while v < V:
            k = int(rng.integers(1, most + 1))
            chunks.append(np.arange(v, min(v + k, V), dtype=np.int64))
            v += k
        return chunks
    raise ValueError(f"partition: kind={kind!r}")


def equal_chunks(c, parts):
    """`parts` consecutive chunks of V // parts views each (the views beyond parts * (V // parts) are left out)"""
    k = c.V // parts
    assert k >= 1
    return [np.arange(i * k, (i + 1) * k, dtype=np.int64) for i in range(parts)]


def concatenation(chunks):
    return np.concatenate([_ix(ch) for ch in chunks]) if len(chunks) else np.zeros(0, np.int64)


def subcase(c, order, name=None):
    """the case with its views `order` (a selection, a truncation, a reordering), everything else as it is"""
    o = _ix(order)
    return lb.Case(name or f"{c.name}[{len(o)} views]", c.points, c.maps[o], c.view_entry[o], c.w2c[o], c.intr[o],
                   None if c.depth is None else c.depth[o], (c.H, c.W), c.mode, c.cut, c.tau, c.min_visible, c.max_visible)


_REFERENCES = {}


def reference_of(c, order):
    """lift_batched_cases._reference on subcase(c, order): computed once per (case, order) and shared; callers must not change it"""
    key = (c.name, _ix(order).tobytes())
    if key not in _REFERENCES:
        _REFERENCES[key] = lb._reference(subcase(c, order))
    return _REFERENCES[key]


# ------------------------------------------------------------------------------------------ the idle chunks
_IDLE = {}


def idle_case():
    """"drop" with two more views, copies of its first two, that look at entry IDLE_ENTRY: an entry without points"""
    if "case" not in _IDLE:
        c = lb.case("drop")
        assert IDLE_ENTRY not in c.entries()
        o = _ix(list(range(c.V)) + [0, 1])
        ve = c.view_entry[o].copy()
        ve[c.V:] = IDLE_ENTRY
        _IDLE["case"] = lb.Case("drop_idle", c.points, c.maps[o], ve, c.w2c[o], c.intr[o], None, (c.H, c.W), c.mode, c.cut, c.tau,
                                c.min_visible, c.max_visible, counts=dict(c.notes["counts"]))
    return _IDLE["case"]


def idle_partition():
    """-> [ordinary views, the dropped views of entry 0 (counts 9, 21, 0), the views of the entry without points]"""
    c = idle_case()
    counts = c.notes["counts"]                        # view -> the number of points it sees, for the views of entry 0
    dropped = _ix(sorted(v for v, n in counts.items() if n in IDLE_DROPPED))
    pointless = _ix(c.views_of(IDLE_ENTRY))
    rest = np.setdiff1d(np.arange(c.V), np.concatenate([dropped, pointless]))
    return [_ix(rest), dropped, pointless]
