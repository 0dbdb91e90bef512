"""Shared inputs and numpy fp64 references for the contrastive sampler over batched SparseTensors (gp_sim_segments_f16x3,
gp_sampler_select_segments, gp_sampler_micro_segments, geopurify_amd.sparse.sample_pairs / info_nce).

The REFERENCE (reference()) restates the definition per batch entry in fp64: rows of an entry in the key order of
ops.coords_order_batched (knn_batched_cases.keys_of), s_j = <Fn_a, Fn_j> with Fn = teacher / max(|teacher|, 1e-12); positive = the
arg-max over j != a, the first in key order on ties; macro = the num_macro lowest other than anchor and positive by (value, key row);
micro = the lowest of the anchor's K neighbours (knn_batched_cases.oracle_lists_of: the lists of sparse.knn) by (value, slot), a
neighbour equal to the positive counting as +inf.  test_contrast_cases_host.py shows that, per entry, this is
oracle.train.sample_pairs on that entry alone.

DECISIONS WITHOUT EXCUSES.  A selection is a comparison of similarities, and the device computes them in three f16 products with
fp32 accumulation (2e-6 from fp64, tests/test_gpu_training.py).  An anchor whose decisive gaps -- the positive's top-2 gap, the gap
between the num_macro-th and the next lowest, the gap between the last local negative and the next local value -- are all at least
MARGIN = 1e-4 (50 x that bound) must come out exactly, so the cases keep such anchors only (kept()) and the GPU tests excuse none.
The `ties` case is the other extreme: teacher rows drawn from 12 distinct unit vectors, equal rows give bit-equal similarities on the
device as in fp64, values of different vectors lie far apart, and every anchor is kept -- order included.

A case is (C int32 [N,4] shuffled rows, T fp32 [N,Dt], anchors int64 [A] input rows, K).  Everything comes from fixed seeds.
"""
import functools

import numpy as np

import knn_batched_cases as kc

MARGIN = 1e-4
NUM_NEGATIVES, NUM_MACRO = 63, 48
K0 = 32
DRAW_CAP = 96                                               # anchors drawn per entry: min(DRAW_CAP, N_b // 3), as the sampler's own draw


def _teacher(rng, n, dt):
    return rng.standard_normal((n, dt)).astype(np.float32) * rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)


def _draw(rng, C, entries=None):
    """min(DRAW_CAP, N_b // 3) distinct rows of every entry (of `entries` only, when given), in a shuffled order over all entries"""
    out = []
    for b in np.unique(C[:, 0]):
        if entries is not None and int(b) not in entries:
            continue
        idx = np.flatnonzero(C[:, 0] == b)
        out.append(rng.choice(idx, min(DRAW_CAP, len(idx) // 3), replace=False))
    out = np.concatenate(out)
    return out[rng.permutation(len(out))].astype(np.int64)


def _two_scenes():
    rng = np.random.default_rng(301)
    C = kc.batched({0: kc.surface_exact(rng, 1500, 40), 5: kc.surface_exact(rng, 700, 30)}, rng)
    return C, _teacher(rng, len(C), 64), _draw(rng, C), K0


def _boundaries(dt):
    def make():
        rng = np.random.default_rng(302)                               # (the same voxels and anchors at every width)
        C = kc.batched({0: kc.surface_exact(rng, 257, 20), 1: kc.surface_exact(rng, 130, 14), 2: kc.surface_exact(rng, 511, 26)}, rng)
        anchors = _draw(rng, C)
        return C, _teacher(np.random.default_rng(3020 + dt), len(C), dt), anchors, K0
    return make


def _overlap():
    """entries 0 / 1: the same voxels, different teachers; entries 2 / 3: the same voxels AND the same teacher rows, anchors on the same
    voxels -- their results must agree voxel for voxel (twin_rows)"""
    rng = np.random.default_rng(303)
    v, w = kc.surface_exact(rng, 300, 24), kc.surface_exact(rng, 280, 22)
    C = kc.batched({0: v, 1: v.copy(), 2: w, 3: w.copy()}, rng)
    T = _teacher(rng, len(C), 64)
    twin = twin_rows(C, 2, 3)
    T[twin[:, 1]] = T[twin[:, 0]]
    pick = rng.choice(len(twin), len(twin) // 3, replace=False)
    anchors = np.concatenate([_draw(rng, C, entries=(0, 1)), twin[pick, 0], twin[pick, 1]]).astype(np.int64)
    return C, T, anchors[rng.permutation(len(anchors))], K0


def twin_rows(C, b0, b1):
    """int64 [n, 2]: the input rows of the same voxel in entries b0 and b1 (which hold the same voxels)"""
    r0, r1 = np.flatnonzero(C[:, 0] == b0), np.flatnonzero(C[:, 0] == b1)
    o0, o1 = np.lexsort(C[r0, 1:].T), np.lexsort(C[r1, 1:].T)
    assert np.array_equal(C[r0[o0], 1:], C[r1[o1], 1:])
    return np.stack([r0[o0], r1[o1]], 1)


def _ties():
    rng = np.random.default_rng(304)
    C = kc.batched({0: kc.surface_exact(rng, 900, 34), 1: kc.surface_exact(rng, 600, 28)}, rng)
    basis = rng.standard_normal((12, 64))
    basis = (basis / np.linalg.norm(basis, axis=1, keepdims=True)).astype(np.float32)
    return C, np.ascontiguousarray(basis[rng.integers(0, 12, len(C))]), _draw(rng, C), K0


def _anchors_in_one_entry():
    rng = np.random.default_rng(305)
    C = kc.batched({1: kc.surface_exact(rng, 200, 18), 2: kc.surface_exact(rng, 300, 22), 4: kc.surface_exact(rng, 250, 20)}, rng)
    return C, _teacher(rng, len(C), 64), _draw(rng, C, entries=(2,)), K0


CASES = {
    "two_scenes": _two_scenes,
    "boundaries_32": _boundaries(32),
    "boundaries_48": _boundaries(48),
    "boundaries_160": _boundaries(160),
    "overlap": _overlap,
    "ties": _ties,
    "anchors_in_one_entry": _anchors_in_one_entry,
}
EXACT_ORDER = ("ties",)                                     # cases whose anchors are all kept and compared in order


@functools.lru_cache(maxsize=None)
def case(name):
    C, T, anchors, K = CASES[name]()
    for a in (C, T, anchors):
        a.setflags(write=False)
    return C, T, anchors, K


# ------------------------------------------------------------------------------------------ the reference
def key_order(C):
    """(perm: key row -> input row, rank: input row -> key row, first / size of the entry of every KEY row)"""
    keys = kc.keys_of(C.astype(np.int64))
    perm = np.argsort(keys, kind="stable")
    rank = np.empty(len(C), np.int64)
    rank[perm] = np.arange(len(C))
    b = C[perm, 0]
    first = np.searchsorted(b, b, "left")
    size = np.searchsorted(b, b, "right") - first
    return perm, rank, first, size


def unit_rows(T):
    T = T.astype(np.float64)
    return T / np.maximum(np.linalg.norm(T, axis=1, keepdims=True), 1e-12)


def sim_rows(C, T, anchors):
    """the fp64 similarity rows: for every anchor the s_j of its entry's rows in key order -> list of [N_b] arrays"""
    perm, rank, first, size = key_order(C)
    Fn = unit_rows(T)
    out = []
    for a in anchors:
        ka = rank[a]
        rows = perm[first[ka]:first[ka] + size[ka]]
        out.append(Fn[rows] @ Fn[a] + 0.0)                               # (+ 0.0: -0 counts as +0)
    return out


def select(row, anchor_at, num_macro):
    """positive and macro of one similarity row (positions in the row) and the two gaps that decide them"""
    n = len(row)
    m = row.copy()
    m[anchor_at] = -np.inf
    pos = int(np.argmax(m))
    top = np.partition(m, n - 2)[n - 2:]
    m = row.copy()
    m[[anchor_at, pos]] = np.inf
    order = np.lexsort((np.arange(n), m))
    gap_macro = m[order[num_macro]] - m[order[num_macro - 1]] if n - 2 > num_macro else np.inf
    return pos, order[:num_macro], top[1] - top[0], gap_macro


def select_micro(row, lists_at, pos, num_micro):
    """micro (slots of the list) and its gap: lists_at = positions in the row of the anchor's neighbours"""
    v = row[lists_at].copy()
    v[lists_at == pos] = np.inf
    order = np.lexsort((np.arange(len(v)), v))
    gap = v[order[num_micro]] - v[order[num_micro - 1]] if len(v) > num_micro else np.inf
    return order[:num_micro], gap


def reference_of(C, T, anchors, K, lists=None, num_negatives=NUM_NEGATIVES, num_macro=NUM_MACRO):
    """-> dict(positive int64 [A], negative int64 [A, num_negatives], margins fp64 [A, 3]) in input rows.  lists: int64 [A, K] input
    rows per anchor (default: the rows of knn_batched_cases.oracle_lists_of)."""
    perm, rank, first, size = key_order(C)
    if lists is None:
        lists = kc.oracle_lists_of(C, K)[anchors]
    num_micro = num_negatives - num_macro
    rows = sim_rows(C, T, anchors)
    A = len(anchors)
    positive = np.empty(A, np.int64)
    negative = np.empty((A, num_negatives), np.int64)
    margins = np.empty((A, 3))
    for i, a in enumerate(anchors):
        f = first[rank[a]]
        pos, macro, g_pos, g_macro = select(rows[i], rank[a] - f, num_macro)
        positive[i] = perm[f + pos]
        negative[i, :num_macro] = perm[f + macro]
        at = rank[lists[i]] - f
        assert (at >= 0).all() and (at < len(rows[i])).all()
        micro, g_micro = select_micro(rows[i], at, pos, num_micro)
        negative[i, num_macro:] = lists[i][micro]
        margins[i] = g_pos, g_macro, g_micro
    return {"positive": positive, "negative": negative, "margins": margins}


@functools.lru_cache(maxsize=None)
def reference(name):
    C, T, anchors, K = case(name)
    return reference_of(C, T, anchors, K)


@functools.lru_cache(maxsize=None)
def kept(name):
    """-> (anchors int64 [A'], positive [A'], negative [A', 63]): the anchors of the case whose margins are all at least MARGIN (all of
    them in the EXACT_ORDER cases) with their reference"""
    C, T, anchors, K = case(name)
    ref = reference(name)
    keep = np.ones(len(anchors), bool) if name in EXACT_ORDER else (ref["margins"] >= MARGIN).all(1)
    return anchors[keep], ref["positive"][keep], ref["negative"][keep]


def assert_pairs(name, positive, negative, ref_positive, ref_negative, num_macro=NUM_MACRO):
    """positives exact; macro and micro as sets (in order in the EXACT_ORDER cases); no anchor excused"""
    assert np.array_equal(positive, ref_positive), np.flatnonzero(positive != ref_positive)[:8]
    if name in EXACT_ORDER:
        assert np.array_equal(negative, ref_negative), np.argwhere(negative != ref_negative)[:8]
        return
    for lo, hi in ((0, num_macro), (num_macro, negative.shape[1])):
        got, ref = np.sort(negative[:, lo:hi], 1), np.sort(ref_negative[:, lo:hi], 1)
        assert np.array_equal(got, ref), (lo, np.flatnonzero((got != ref).any(1))[:8])


# ------------------------------------------------------------------------------------------ InfoNCE
def info_nce_weights(entry, reduction):
    """w [A] fp64 with loss = sum_a w_a l_a: "anchor" the mean over anchors, "entry" the mean over present entries of entry means"""
    entry = np.asarray(entry)
    if reduction == "anchor":
        return np.full(len(entry), 1.0 / len(entry))
    present, inverse, counts = np.unique(entry, return_inverse=True, return_counts=True)
    return 1.0 / (len(present) * counts[inverse])
