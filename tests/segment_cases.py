"""Shared inputs and numpy references for the batched scene tail (gp_nn1_batched, gp_iou_hist_batched_i64, geopurify_amd.sparse.segment):
the cases, the brute-force fill, a model of the kernel's ladder, the feature recipe and the per-entry counts.

A case is (C int32 [N,4] = batch, x, y, z, zero bool [N]): the rows flagged `zero` are the queries, every other row a reference.
Rows are shuffled (or placed by hand where the input order is the point), so the sorted order differs from the input order.

REFERENCES
  fill      per entry, brute force in int64: the reference row minimising (d^2 over the chosen axes, input row); -1 where the entry has
            none and for rows that are no queries.
  labels    features are 4 * text_norm[class] + 0.05 * noise with the zero rows set to exact zeros; the label of a non-zero row is the
            fp64 arg-max of its cosine against the text rows, and features() asserts that every such row's top-2 margin is at least 0.1
            (a fp32 kernel's cosine is within 1e-5), so labels are compared for exact equality with no row excused.  A zero row's
            arg-max is class 0 (all logits 0, first maximum), as run/validation.py:413-416 gives it.
  counts    oracle.metric.intersection_and_union per entry (it returns U = O + T - I; converted back to O).
"""
import functools

import numpy as np

import knn_batched_cases as kc
from oracle import metric as o_metric

RING1, RING3, SCAN, NONE = 1, 3, 0, -1
MARGIN = 0.1
AXES = {"xyz": 7, "yz": 6}


def _case(C, zero):
    C = np.ascontiguousarray(np.asarray(C, dtype=np.int32))
    zero = np.asarray(zero, dtype=bool)
    assert C.shape == (len(zero), 4) and len(np.unique(C, axis=0)) == len(C)
    C.setflags(write=False)
    zero.setflags(write=False)
    return C, zero


def _placed(rows):
    """[(batch, x, y, z, zero)] in exactly this input order"""
    a = np.array(rows, dtype=np.int64)
    return _case(a[:, :4], a[:, 4] != 0)


# ------------------------------------------------------------------------------------------ the cases
def _overlap():
    """two entries with identical coordinates, zero rows at different places"""
    rng = np.random.default_rng(301)
    v = kc.surface_exact(rng, 300, ext=24)
    C = kc.batched({0: v, 1: v.copy()}, rng)
    zero = np.where(C[:, 0] == 0, C[:, 1] < 7, C[:, 2] > 15)
    return _case(C, zero)


def _empty_entry():
    """entry 0 all zero, entry 3 without a zero row, entry 65535 a single voxel -- all at overlapping coordinates"""
    rng = np.random.default_rng(302)
    C = kc.batched({0: kc.cube(4), 3: kc.cube(3), 65535: np.array([[1, 1, 1]])}, rng)
    return _case(C, C[:, 0] == 0)


def _rung_cell():
    """single zero rows scattered through a dense cube: the nearest reference is a direct neighbour"""
    rng = np.random.default_rng(303)
    C = kc.batched({0: kc.cube(12), 1: kc.cube(9, (2, 2, 2))}, rng)
    return _case(C, rng.random(len(C)) < 0.04)


def _strip(lo, hi):
    """a strip 96 x 8 x 1 whose columns lo .. hi are zero: a query's nearest reference is min(x - lo + 1, hi + 1 - x) columns away"""
    def make():
        g = np.stack(np.meshgrid(np.arange(96), np.arange(8), indexing="ij"), -1).reshape(-1, 2)
        v = np.c_[g, np.zeros(len(g), int)]
        C = kc.batched({2: v}, np.random.default_rng(304))
        return _case(C, (C[:, 1] >= lo) & (C[:, 1] <= hi))
    return make


def _tie_bound_1():
    """query (16,16,16); (25,16,16) is inside the ring-1 block (cells 1..3 = 8..31), (7,16,16) outside it with the LOWER input row; both
    d^2 = 81 = (8 + 1)^2.  The voxel at the origin keeps the key shift at zero."""
    return _placed([(0, 7, 16, 16, 0), (0, 0, 0, 0, 0), (0, 25, 16, 16, 0), (0, 16, 16, 16, 1)])


def _tie_bound_3():
    """the ring-3 analogue: query (32,32,32), block cells 1..7 = 8..63, references (57,32,32) inside and (7,32,32) outside, d^2 = 625"""
    return _placed([(0, 7, 32, 32, 0), (0, 0, 0, 0, 0), (0, 57, 32, 32, 0), (0, 32, 32, 32, 1)])


def _ties():
    """query (12,12,12) and the 24 lattice points at d^2 = 5 around it, all inside ring 1.  The tie with the lowest key -- the lowest
    SORTED row -- comes last in the input order, so the two tie rules differ."""
    q = np.array([12, 12, 12])
    pts = kc.shell(5) + q
    with_origin = np.vstack([np.zeros((1, 3), int), pts])                          # (the key shift of the case: its minimum is the origin)
    key = kc.keys_of(np.c_[np.zeros(len(with_origin), int), with_origin].astype(np.int64))[1:]
    pts = pts[np.argsort(key)[::-1]]
    rows = [(1, 0, 0, 0, 0), (1, *q, 1)] + [(1, *p, 0) for p in pts]
    return _placed(rows)


def _extent():
    """negative coordinates and an extent of 32767 along x: the queries' only references sit at the far end, d^2 = 32766^2 + ... just
    below 2^30"""
    return _placed([(4, -100, -5, -7, 1), (4, 32666, -5, -7, 0), (4, -100, -4, -7, 1), (4, 32666, -3, -7, 0)])


def _yz():
    """two surface entries with zero patches, plus (entry 0) a zero row at (10,50,50) whose (y, z) column holds three references that
    differ in x only: the masked distance ties at 0 and the lowest input row wins"""
    rng = np.random.default_rng(305)
    a, b = kc.surface_exact(rng, 300, ext=24), kc.surface_exact(rng, 280, ext=24)
    col = np.array([[20, 50, 50], [3, 50, 50], [11, 50, 50], [10, 50, 50]])
    C = kc.batched({0: np.vstack([a, col]), 1: b}, rng)
    zero = np.where(C[:, 0] == 0, (C[:, 1] > 4) & (C[:, 1] < 12) & (C[:, 2] < 20), (C[:, 3] > 10) & (C[:, 2] < 30))
    zero |= (C == np.array([0, 10, 50, 50])).all(1)
    return _case(C, zero)


def _queries(nq, side=7):
    def make():
        rng = np.random.default_rng(306 + nq)
        C = kc.batched({0: kc.cube(side)}, rng)
        zero = np.zeros(len(C), bool)
        zero[rng.permutation(len(C))[:nq]] = True
        return _case(C, zero)
    return make


CASES = {
    "overlap": _overlap,
    "empty_entry": _empty_entry,
    "rung_cell": _rung_cell,
    "rung_ring3": _strip(16, 47),
    "rung_scan": _strip(16, 79),
    "tie_bound_1": _tie_bound_1,
    "tie_bound_3": _tie_bound_3,
    "ties": _ties,
    "extent": _extent,
    "yz": _yz,
    "one_row": lambda: _placed([(0, 5, 6, 7, 0)]),
    "one_zero_row": lambda: _placed([(2, 5, 6, 7, 1)]),
    "queries_63": _queries(63),
    "queries_64": _queries(64),
    "queries_65": _queries(65),
    "queries_257": _queries(257),
    "all_but_one": _queries(124, side=5),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def _entries(C):
    for b in np.unique(C[:, 0]):
        yield int(b), np.flatnonzero(C[:, 0] == b)


# ------------------------------------------------------------------------------------------ the fill: brute force and the ladder model
def fill_of(C, zero, axes=7):
    """filled_from int64 [N]: for every zero row the input row of the non-zero row of its entry with the smallest (d^2, row), d^2 over
    the axes in `axes`; -1 for non-zero rows and where the entry has no non-zero row"""
    out = np.full(len(C), -1, np.int64)
    w = np.array([axes & 1, axes >> 1 & 1, axes >> 2 & 1], np.int64)
    for b, idx in _entries(C):
        q, r = idx[zero[idx]], idx[~zero[idx]]
        if not len(q) or not len(r):
            continue
        p = C[:, 1:].astype(np.int64)
        d2 = (((p[q][:, None, :] - p[r][None, :, :]) ** 2) * w).sum(-1)
        key = d2 * len(C) + r[None, :]                       # (d2 < 2^31, rows < 2^13: exact in int64)
        out[q] = r[np.argmin(key, axis=1)]
    return out


@functools.lru_cache(maxsize=None)
def fill(name, axes=7):
    return fill_of(*case(name), axes)


def ladder_of(C, zero, axes=7):
    """Model of gp_nn1_batched's ladder -> (filled_from int64 [N], path int [N]: RING1, RING3, SCAN for queries, NONE elsewhere and for
    queries whose entry has no reference).  Ring R takes the references of the (2R+1)^3 cells of key >> 9 around the query's cell, same
    batch bits, and is final only when its best d^2 is strictly below (8R+1)^2; with axes != 7 every query is scanned."""
    keys = kc.keys_of(C.astype(np.int64))
    batch, xyz = kc.decode(keys)
    cell = xyz >> 3
    w = np.array([axes & 1, axes >> 1 & 1, axes >> 2 & 1], np.int64)
    out = np.full(len(C), -1, np.int64)
    path = np.full(len(C), NONE, np.int64)
    for q in np.flatnonzero(zero):
        refs = np.flatnonzero(~zero & (batch == batch[q]))
        if not len(refs):
            continue
        cheb = np.abs(cell[refs] - cell[q]).max(1)
        for R, tag in ((1, RING1), (3, RING3), (None, SCAN)):
            if R is not None and axes != 7:
                continue
            cand = refs if R is None else refs[cheb <= R]
            if not len(cand):
                continue
            d2 = (((xyz[cand] - xyz[q]) ** 2) * w).sum(1)
            best = np.lexsort((cand, d2))[0]
            if R is None or d2[best] < (8 * R + 1) ** 2:
                out[q], path[q] = cand[best], tag
                break
    return out, path


# ------------------------------------------------------------------------------------------ features, labels, counts
@functools.lru_cache(maxsize=None)
def text(D, Cn):
    t = np.random.default_rng(400 + D + Cn).standard_normal((Cn, D)) * 3.0             # (not unit: segment normalises)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def features(name, D, Cn):
    """-> (F fp32 [N,D], cls int64 [N]): cls is the fp64 arg-max label of every row (0 for the zero rows)"""
    C, zero = case(name)
    return features_of(zero, D, Cn, 500 + len(C))


def features_of(zero, D, Cn, seed):
    rng = np.random.default_rng(seed)
    t = text(D, Cn)
    tn = t / np.linalg.norm(t, axis=1, keepdims=True)
    want = rng.integers(0, Cn, len(zero))
    F = (4.0 * tn[want] + 0.05 * rng.standard_normal((len(zero), D))).astype(np.float32)
    F[zero] = 0.0
    cls = labels_of(F, t)
    assert np.array_equal(cls[~zero], want[~zero])
    F.setflags(write=False)
    return F, cls


def margins(F, t):
    """fp64 top-2 cosine margin per row (0 for all-zero rows) and the arg-max"""
    F = np.asarray(F, np.float64)
    tn = t / np.linalg.norm(t, axis=1, keepdims=True)
    norm = np.linalg.norm(F, axis=1, keepdims=True)
    cos = np.where(norm > 0, F / np.where(norm > 0, norm, 1.0), 0.0) @ tn.T
    top = np.sort(cos, axis=1)
    return (top[:, -1] - top[:, -2]) if t.shape[0] > 1 else np.ones(len(F)), np.argmax(cos, axis=1).astype(np.int64)


def labels_of(F, t):
    """arg-max labels in fp64; asserts the margin of every non-zero row"""
    m, cls = margins(F, t)
    nz = np.abs(np.asarray(F, np.float64)).sum(1) > 0
    assert not nz.any() or m[nz].min() >= MARGIN, f"top-2 margin {m[nz].min():.3f} below {MARGIN}"
    return cls


def pred_of(cls, filled_from):
    return np.where(filled_from >= 0, cls[np.clip(filled_from, 0, None)], cls)


def target_of(cls, Cn, seed, ignore=(255,)):
    """ground-truth labels for the counts: the classes with a fifth of them redrawn, some ignore ids, some values outside 0..C-1"""
    rng = np.random.default_rng(seed)
    t = cls.copy()
    r = rng.random(len(t))
    t[r < 0.2] = rng.integers(0, Cn, int((r < 0.2).sum()))
    for k, ig in enumerate(ignore):
        t[(r >= 0.2 + 0.05 * k) & (r < 0.25 + 0.05 * k)] = ig
    t[(r >= 0.9) & (r < 0.93)] = Cn + 3
    t[(r >= 0.93) & (r < 0.95)] = -1
    return t


def counts_of(pred, target, batch, B, Cn, ignore):
    """int64 [B,3,C] = (I, O, T) per entry from oracle.metric.intersection_and_union (which returns U = O + T - I)"""
    out = np.zeros((B, 3, Cn), np.int64)
    for b in range(B):
        m = batch == b
        if m.any():
            i, u, t = o_metric.intersection_and_union(pred[m], target[m], Cn, list(ignore))
            out[b] = np.stack([i, u - t + i, t])
    return out
