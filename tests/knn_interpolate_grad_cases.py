"""Cases and numpy references for the backward of sparse.interpolate (csrc/knn_interpolate_grad.hip).  Imports nothing from
geopurify_amd: test_knn_interpolate_grad_cases_host.py checks the cases' own claims on the CPU, test_gpu_knn_interpolate_grad.py runs
them on the GPU.

The rule (rule_reference below, literally).  A reference is a flat slot f = j*k + s whose forward weight is in effect: s is a slot the
mode reads, its list entry is valid, its row r = index[indices[j,s]] (or indices[j,s]) is valid, and query row j is not excused (a
query row with a list entry outside -1..N-1 or an index value outside 0..R-1 among the slots the mode reads names no row).
d_values[r,c] starts at +0.f; over the references of r in ascending f, acc = acc + w32[f] * g[j,c], product and sum each rounded once
in fp32.  The weights are an INPUT of that reference: the tests hand it what the GPU emitted, and bound those against weights64.

Every case is the smallest shape at which its mechanism can go wrong; lists and references are computed once per process and handed
out read-only.
"""
import functools

import numpy as np

import knn_query_cases as kc

GRAD_D = (1, 3, 70, 512)
GRAD_K = (1, 3, 32)
GRAD_EPS = (1e-8, 0.0, 0.5)
N_POINTS = 300                                                   # kc.interp_lists' points
R_INDEX = 130                                                    # rows of values behind the index: 120 .. 129 are never named
HUB_QUERIES = 5000
BIG_R, BIG_M, BIG_K, BIG_D = 262147, 90000, 3, 4                 # more rows than the backward's launch has waves (4 * 65536)
BACKWARD_WAVES = 4 * 65536


class Lists:
    """indices i64 [M,k], d2 f64 [M,k], index i64 [N] or None, N = the range of the list entries, R = rows of values"""

    def __init__(self, name, indices, d2, index, N, R, **marks):
        self.name, self.indices, self.d2, self.index, self.N, self.R, self.marks = name, indices, d2, index, N, R, marks
        for a in (indices, d2) + (() if index is None else (index,)):
            a.setflags(write=False)


# ------------------------------------------------------------------------------------------ references
def references(L, mode="inverse_distance"):
    """-> (ref bool [M,k]: the flat slots that are references, rows i64 [M,k]: their rows of values (0 elsewhere), excused bool [M],
    named bool [M,k]: slots that name a valid row whether or not the query row is excused -- the slots the forward weighs)"""
    M, k = L.indices.shape
    read = np.zeros((M, k), bool)
    read[:, :1 if mode == "nearest" else k] = True
    valid = (L.indices != -1) & read
    wrong = valid & ((L.indices < 0) | (L.indices >= L.N))
    rows = np.where(valid & ~wrong, L.indices, 0)
    if L.index is not None:
        rows = L.index[rows]
    wrong_index = valid & ~wrong & ((rows < 0) | (rows >= L.R))
    excused = wrong.any(1) | wrong_index.any(1)
    named = valid & ~wrong & ~wrong_index
    ref = named & ~excused[:, None]
    return ref, np.where(ref, rows, 0), excused, named


def weights64(L, mode="inverse_distance", eps=1e-8):
    """the forward's weights in fp64 [M,k]: over the slots that name a row, w = 1 / (d^2 + eps) normalised (slots with d^2 + eps == 0
    share the weight alone), 1 for slot 0 of "nearest"; 0 where the slot is no reference"""
    ref, _, _, named = references(L, mode)
    if mode == "nearest":
        return ref.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = L.d2 + eps
        zero = named & (t == 0)
        w = np.where(zero.any(1, keepdims=True), zero.astype(np.float64), np.where(named, 1.0 / np.where(named, t, 1.0), 0.0))
        s = w.sum(1, keepdims=True)
        w = np.where(s > 0, w / np.where(s > 0, s, 1.0), 0.0)
    return np.where(ref, w, 0.0)


def _by_row(ref, rows):
    """the references sorted stably by row: (flat slots f, their rows, rank of each inside its row)"""
    f = np.nonzero(ref.reshape(-1))[0]
    r = rows.reshape(-1)[f]
    order = np.argsort(r, kind="stable")                          # ascending f inside a row
    f, r = f[order], r[order]
    start = np.concatenate([[0], np.nonzero(np.diff(r))[0] + 1]) if f.size else np.zeros(0, np.int64)
    rank = np.arange(f.size) - np.repeat(start, np.diff(np.concatenate([start, [f.size]])))
    return f, r, rank


def rule_reference(g, L, w32, mode="inverse_distance"):
    """g f32 [M,D], w32 f32 [M,k] -> d_values f32 [R,D] by the rule: per row its references in ascending f, acc = acc + w * g in fp32.
    Sequential inside a row, vectorised across rows: step t adds every row's t-th reference."""
    g, w32 = np.asarray(g, np.float32), np.asarray(w32, np.float32).reshape(-1)
    k = L.indices.shape[1]
    ref, rows, _, _ = references(L, mode)
    f, r, rank = _by_row(ref, rows)
    out = np.zeros((L.R, g.shape[1]), np.float32)
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(rank))]) if f.size else [0]
    for t in range(len(bounds) - 1):
        sel = by_rank[bounds[t]:bounds[t + 1]]                    # one reference per row at most
        prod = w32[f[sel], None] * g[f[sel] // k]                 # fp32, rounded once
        out[r[sel]] = out[r[sel]] + prod                          # fp32, rounded once
    return out


def fp64_reference(g, L, mode="inverse_distance", eps=1e-8):
    """-> (d_values f64 [R,D], scale f64 [R,D] = sum over the row's references of |w g|, count i64 [R] = its references)"""
    g = np.asarray(g, np.float64)
    k = L.indices.shape[1]
    ref, rows, _, _ = references(L, mode)
    w = weights64(L, mode, eps).reshape(-1)
    f = np.nonzero(ref.reshape(-1))[0]
    r = rows.reshape(-1)[f]
    out, scale = np.zeros((L.R, g.shape[1])), np.zeros((L.R, g.shape[1]))
    contrib = w[f, None] * g[f // k]
    np.add.at(out, r, contrib)
    np.add.at(scale, r, np.abs(contrib))
    return out, scale, np.bincount(r, minlength=L.R)


def grad_bound(count, scale):
    """the weights rounded once (2^-24 relative), L products and L - 1 additions in fp32 over a row of L references:
    (L + 2) 2^-23 sum |w g| per element"""
    return (count[:, None] + 2) * 2.0 ** -23 * scale


def forward_reference(values, L, w32, mode="inverse_distance"):
    """the forward recomputed from emitted weights in list order, fp32: out f32 [M,D]"""
    values, w32 = np.asarray(values, np.float32), np.asarray(w32, np.float32)
    ref, rows, _, _ = references(L, mode)
    out = np.zeros((L.indices.shape[0], values.shape[1]), np.float32)
    for s in range(L.indices.shape[1]):
        q = np.nonzero(ref[:, s])[0]
        out[q] = out[q] + w32[q, s, None] * values[rows[q, s]]
    return out


# ------------------------------------------------------------------------------------------ cases
def grad_index():
    """point -> row of values: 300 points onto rows 0..119 of R_INDEX = 130, so rows 120..129 have no references"""
    index = np.random.default_rng(31).integers(0, 120, N_POINTS).astype(np.int64)
    return index


@functools.lru_cache(None)
def grid_lists(k, with_index):
    """kc.interp_lists' clouds at k neighbours: entry 1 holds 3 points (a -1 tail for k > 3), entry 2 none (no valid slot), 40 queries
    sit on points, some of them stored twice (zero-distance ties)"""
    points, queries, _, _, _ = kc.interp_lists()
    idx, d2 = kc.knn_reference(points, queries, k)
    return Lists(f"grid k={k}", idx, d2, grad_index() if with_index else None, N_POINTS, R_INDEX if with_index else N_POINTS)


@functools.lru_cache(None)
def hub():
    """300 ordinary points in a unit box and 300 ordinary queries, then HUB_QUERIES queries far outside it: all of those list the
    same point first, so one row of values has thousands of references (k = 3, no index)"""
    rng = np.random.default_rng(32)
    pts = rng.random((N_POINTS, 3)) * [0.99, 1.0, 1.0]
    pts[7] =[0.999, 0.5, 0.5]                                   # the point nearest to everything far out along +x
    far = np.concatenate([1e3 + rng.random((HUB_QUERIES, 1)), 0.5 + 1e-3 * rng.random((HUB_QUERIES, 2))], 1)
    points = np.concatenate([np.zeros((N_POINTS, 1)), pts], 1)
    queries = np.concatenate([np.zeros((300 + HUB_QUERIES, 1)), np.concatenate([rng.random((300, 3)), far], 0)], 1)
    idx, d2 = kc.knn_reference_vectorised(points, queries, 3)
    return Lists("hub", idx, d2, None, N_POINTS, N_POINTS, hub_row=7)


@functools.lru_cache(None)
def folded():
    """an index that folds the 300 points onto 12 rows: every row is named by many points, and lists name one row twice"""
    base = grid_lists(3, False)
    index = np.random.default_rng(33).integers(0, 12, N_POINTS).astype(np.int64)
    return Lists("folded", base.indices.copy(), base.d2.copy(), index, N_POINTS, 12)


@functools.lru_cache(None)
def planted():
    """grid lists (k = 3, index) with entries that must never be dereferenced: list entries below -1 and past N - 1, an index value
    past R - 1 and a negative one; the query rows that hold them are excused"""
    base = grid_lists(3, True)
    idx, index = base.indices.copy(), base.index.copy()
    idx[0, 1], idx[1, 0], idx[2, 2] = -5, N_POINTS, 2 ** 40
    index[base.indices[5, 0]] = R_INDEX
    index[base.indices[9, 1]] = -1
    return Lists("planted", idx, base.d2.copy(), index, N_POINTS, R_INDEX)


@functools.lru_cache(None)
def big():
    """BIG_R rows of values, more than the backward's launch has waves; hand-made lists of BIG_M queries, k = 3, no index"""
    rng = np.random.default_rng(34)
    idx = rng.integers(0, BIG_R, (BIG_M, BIG_K)).astype(np.int64)
    idx[:, 0] = np.where(rng.random(BIG_M) < 0.5, BIG_R - 1 - rng.integers(0, 8, BIG_M), idx[:, 0])   # the last rows, those of the second trip
    d2 = np.sort(rng.random((BIG_M, BIG_K)) + 1e-3, 1)
    return Lists("big", idx, d2, None, BIG_R, BIG_R)


def grads(M, D, seed=35):
    """fp32 upstream gradients, a few large rows"""
    g = np.random.default_rng(seed + D).normal(size=(M, D)).astype(np.float32)
    g[::11] *= 50.0
    return g
