"""Cases and numpy references for sparse.knn_query / sparse.interpolate (csrc/knn_query.hip).  Imports nothing from geopurify_amd:
test_knn_query_cases_host.py checks the cases' own claims on the CPU, test_gpu_knn_query.py runs them on the GPU.

The rule (reference below, literally): xyz rounded to fp32 first; d^2 = (dx*dx + dy*dy) + dz*dz in fp64, numpy's separate multiply and
add ufuncs rounding each operation once; a query lists the points of its own batch entry by np.lexsort((row, d2)); slots past the
entry's count hold -1 / +inf.  Interpolation: w_j = 1 / (d^2_j + eps) over the valid slots, normalised, the sum in fp64.

Every case is the smallest shape at which its mechanism can go wrong; the references are computed once per process (lru_cache) and
handed out read-only.
"""
import functools

import numpy as np

MAX_K = 32                                                       # GP_KNN_QUERY_MAX_K (asserted equal on the host)
BOX = 10.0                                                       # the ladder's box
CLUMP_RADIUS = 1e-3


class Cloud:
    """points f64 [N,4] and queries f64 [M,4] = batch, x, y, z; ks: the k values the case is run at; marks: named row sets of the queries"""

    def __init__(self, name, points, queries, ks, **marks):
        self.name, self.points, self.queries, self.ks, self.marks = name, points, queries, tuple(ks), marks
        for a in (points, queries):
            a.setflags(write=False)


def _rows(batch, xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.concatenate([np.full((xyz.shape[0], 1), float(batch)), xyz], 1)


def _shuffled(rng, *blocks):
    a = np.concatenate(blocks, 0)
    return a[rng.permutation(a.shape[0])]


# ------------------------------------------------------------------------------------------ references
def knn_reference(points, queries, k, round32=True):
    """-> (indices i64 [M,k], d2 f64 [M,k]) by brute force per entry; round32=False: the same on the unrounded coordinates (only to
    show that the rounding matters)"""
    points, queries = np.asarray(points, np.float64), np.asarray(queries, np.float64)
    P, Q = points[:, 1:], queries[:, 1:]
    if round32:
        P, Q = P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
    M = queries.shape[0]
    idx, d2 = np.full((M, k), -1, np.int64), np.full((M, k), np.inf, np.float64)
    for b in np.unique(queries[:, 0]):
        rows, qrows = np.nonzero(points[:, 0] == b)[0], np.nonzero(queries[:, 0] == b)[0]
        if rows.size == 0:
            continue
        Pb = P[rows]
        for q in qrows:
            dx, dy, dz = Q[q, 0] - Pb[:, 0], Q[q, 1] - Pb[:, 1], Q[q, 2] - Pb[:, 2]
            d = (dx * dx + dy * dy) + dz * dz
            order = np.lexsort((rows, d))[:k]
            idx[q, :order.size], d2[q, :order.size] = rows[order], d[order]
    return idx, d2


def knn_reference_vectorised(points, queries, k, chunk=16384):
    """knn_reference for many queries: a stable argsort of d2 over the entry's rows in ascending row is np.lexsort((row, d2))"""
    points, queries = np.asarray(points, np.float64), np.asarray(queries, np.float64)
    P, Q = points[:, 1:].astype(np.float32).astype(np.float64), queries[:, 1:].astype(np.float32).astype(np.float64)
    idx, d2 = np.full((queries.shape[0], k), -1, np.int64), np.full((queries.shape[0], k), np.inf, np.float64)
    for b in np.unique(queries[:, 0]):
        rows, qrows = np.nonzero(points[:, 0] == b)[0], np.nonzero(queries[:, 0] == b)[0]
        for s in range(0, qrows.size if rows.size else 0, chunk):
            qs = qrows[s:s + chunk]
            d = Q[qs, None, :] - P[None, rows, :]
            dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            order = np.argsort(dist, axis=1, kind="stable")[:, :k]
            idx[qs, :order.shape[1]], d2[qs, :order.shape[1]] = rows[order], np.take_along_axis(dist, order, 1)
    return idx, d2


def interpolate_reference(values, indices, d2, num_points, index=None, mode="inverse_distance", eps=1e-8):
    """values f64 [R,D] (the upcast values) -> (out f64 [M,D], vmax f64 [M,D] = the largest |v_j| among the row's used slots per
    element -- the scale of the bound --, bad_list rows, bad_index rows).  A row with a list entry outside -1..num_points-1, or with
    an index value outside 0..R-1 among the slots the mode reads, is zero and counted."""
    values = np.asarray(values, np.float64)
    R, D = values.shape
    M, k = indices.shape
    slots = 1 if mode == "nearest" else k
    out, vmax = np.zeros((M, D)), np.zeros((M, D))
    bad_list = bad_index = 0
    for q in range(M):
        ids, dd = indices[q, :slots], d2[q, :slots]
        valid = ids != -1
        wrong = valid & ((ids < 0) | (ids >= num_points))
        rows = np.where(valid & ~wrong, ids, 0)
        if index is not None:
            rows = index[rows]
        wrong_index = valid & ~wrong & ((rows < 0) | (rows >= R))
        bad_list += int(wrong.any())
        bad_index += int(wrong_index.any())
        if wrong.any() or wrong_index.any() or not valid.any():
            continue
        rows, dd = rows[valid], dd[valid]
        if mode == "nearest":
            w = np.ones(1)
        else:
            t = dd + eps
            w = (t == 0).astype(np.float64) if (t == 0).any() else 1.0 / t
            w = w / w.sum()
        out[q] = (w[:, None] * values[rows]).sum(0)
        vmax[q] = np.abs(values[rows][w > 0]).max(0)
    return out, vmax, bad_list, bad_index


def labels_reference(values, indices, num_points, index=None, unlabeled=255):
    """integer values [R]: slot 0 -> (out i64 [M], bad_list, bad_index)"""
    R, ids = values.shape[0], indices[:, 0]
    valid = ids != -1
    wrong = valid & ((ids < 0) | (ids >= num_points))
    rows = np.where(valid & ~wrong, ids, 0)
    if index is not None:
        rows = index[rows]
    wrong_index = valid & ~wrong & ((rows < 0) | (rows >= R))
    ok = valid & ~wrong & ~wrong_index
    return np.where(ok, values[np.where(ok, rows, 0)], unlabeled).astype(np.int64), int(wrong.sum()), int(wrong_index.sum())


def interpolate_bound(k, vmax):
    """weights rounded once (2^-24 relative), k products and k - 1 additions in fp32: (k + 2) 2^-23 max_j |v_j| per element"""
    return (k + 2) * 2.0 ** -23 * vmax


# ------------------------------------------------------------------------------------------ cases
@functools.lru_cache(None)
def ties():
    """a 6 x 6 x 6 unit lattice, every point stored twice; queries at the cell centres and on the nodes: d^2 is exact, dozens of
    candidates tie at the k-th distance, node queries have d^2 = 0 twice over"""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(6.0), np.arange(6.0), np.arange(6.0), indexing="ij"), -1).reshape(-1, 3)
    c = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 3) + 0.5
    queries = np.concatenate([_rows(0, c), _rows(0, g)], 0)
    return Cloud("ties", _shuffled(rng, _rows(0, g), _rows(0, g)), queries, (1, 3, 8, 32), centres=np.arange(125), nodes=np.arange(125, 341))


ENTRY_IDS = (0, 3, 7, 4000, 65535)


@functools.lru_cache(None)
def entries():
    """five entries, rows interleaved at random: 0 and 3 fill the same unit box (3 eight times as densely), 7 has points and no
    queries, 4000 queries and no points, 65535 two points"""
    rng = np.random.default_rng(12)
    points = _shuffled(rng, _rows(0, rng.random((100, 3))), _rows(3, rng.random((800, 3))), _rows(7, rng.random((150, 3)) + 2.0),
                       _rows(65535, [[0.25, 0.5, 0.5], [0.75, 0.5, 0.5]]))
    queries = _shuffled(rng, _rows(0, rng.random((300, 3))), _rows(3, rng.random((50, 3))), _rows(4000, rng.random((40, 3))),
                        _rows(65535, rng.random((30, 3))))
    return Cloud("entries", points, queries, (3,))


def ladder_directions():
    """the 20 directions of the far queries: 6 axes, 8 space diagonals, 6 face diagonals"""
    d = [(s if a == 0 else 0, s if a == 1 else 0, s if a == 2 else 0) for a in range(3) for s in (1, -1)]
    d += [(x, y, z) for x in (1, -1) for y in (1, -1) for z in (1, -1)]
    d += [(1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1)]
    return np.array(d, np.float64)


def _ball(rng, n, centre, radius):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return centre + v * (radius * 0.999 * rng.random((n, 1)) ** (1.0 / 3.0))


CLUMP_POINTS = 2100                                              # more than 64 * MAX_K = 2048 (the issue's "2 000" is not)


@functools.lru_cache(None)
def ladder():
    """one entry: a clump inside a ball of radius 1e-3 and 1000 points uniform in a 10-unit box.  Whatever ng is chosen the clump sits
    in one cell and overflows a shell's worth of candidates; the far queries exhaust the grid"""
    rng = np.random.default_rng(13)
    centre = np.array([3.3, 6.1, 4.7])
    points = _shuffled(rng, _rows(0, _ball(rng, CLUMP_POINTS, centre, CLUMP_RADIUS)), _rows(0, rng.random((1000, 3)) * BOX))
    far = BOX / 2 + ladder_directions() * (BOX / 2 + 1e3)
    corners = np.array([(x, y, z) for x in (0, BOX) for y in (0, BOX) for z in (0, BOX)] + [(0, 0, BOX / 2), (BOX, BOX / 2, BOX)], np.float64)
    queries = np.concatenate([_rows(0, _ball(rng, 300, centre, CLUMP_RADIUS)), _rows(0, rng.random((300, 3)) * BOX), _rows(0, far), _rows(0, corners)], 0)
    return Cloud("ladder", points, queries, (16, 32), clump=np.arange(300), uniform=np.arange(300, 600), far=np.arange(600, 620),
                 corners=np.arange(620, 630), centre=centre)


@functools.lru_cache(None)
def degenerate():
    """boxes without a volume, one call: entry 0 a plane, 1 a line, 2 one location 500 times over, 3..6 one point each"""
    rng = np.random.default_rng(14)
    plane = np.concatenate([rng.random((400, 2)) * 4, np.full((400, 1), 1.5)], 1)
    line = np.concatenate([rng.random((300, 1)) * 8, np.full((300, 1), -2.0), np.full((300, 1), 0.25)], 1)
    spot = np.tile([[7.0, 7.0, 7.0]], (500, 1))
    singles = [_rows(3 + i, rng.random((1, 3)) * 3) for i in range(4)]
    points = _shuffled(rng, _rows(0, plane), _rows(1, line), _rows(2, spot), *singles)
    queries = _shuffled(rng, _rows(0, rng.random((60, 3)) * 4), _rows(0, plane[:20]), _rows(1, rng.random((60, 3)) * 8 - [0, 2, 0]), _rows(1, line[:20]),
                        _rows(2, spot[:10]), _rows(2, rng.random((20, 3)) * 14), *[_rows(3 + i, rng.random((5, 3)) * 3) for i in range(4)])
    return Cloud("degenerate", points, queries, (1, 3, 32))


@functools.lru_cache(None)
def rounding():
    """fp64 coordinates at 1e4 + t * 1e-5: the fp32 grid there is 2^-10 wide, so about 98 neighbours merge; the reference rounds first"""
    rng = np.random.default_rng(15)
    t = rng.permutation(4000)[:600].astype(np.float64)
    u = rng.integers(0, 300, (600, 2)).astype(np.float64)
    points = _rows(0, np.concatenate([1e4 + t[:, None] * 1e-5, 1e4 + u * 1e-5], 1))
    tq = rng.integers(0, 4000, 200).astype(np.float64) + 0.5
    uq = rng.integers(0, 300, (200, 2)).astype(np.float64) + 0.5
    queries = _rows(0, np.concatenate([1e4 + tq[:, None] * 1e-5, 1e4 + uq * 1e-5], 1))
    return Cloud("rounding", points, queries, (1, 8))


@functools.lru_cache(None)
def blocks():
    """M = 4 * 256 + 1 queries, N = 4097 points, k = 16: the last partial wave, workgroup and (40 far queries) pending list"""
    rng = np.random.default_rng(16)
    points = _shuffled(rng, _rows(0, rng.random((2049, 3)) * 5), _rows(1, rng.normal(size=(2048, 3))))
    near = np.concatenate([_rows(0, rng.random((500, 3)) * 5), _rows(1, rng.normal(size=(485, 3)))], 0)
    far = np.concatenate([_rows(0, rng.random((20, 3)) * 5 + 400), _rows(1, rng.normal(size=(20, 3)) - 300)], 0)
    return Cloud("blocks", points, _shuffled(rng, near, far), (16,))


WALK_WAVES = 4 * 8192                                            # the grid walk's launch: workgroups of 4 waves, at most 8192 of them
INTERP_WAVES = 4 * 65536                                         # the interpolation's


@functools.lru_cache(None)
def many_queries():
    """more queries than the grid walk's launch has waves, so every wave takes a second query: 300 points of two entries"""
    rng = np.random.default_rng(19)
    points = _shuffled(rng, _rows(0, rng.random((200, 3))), _rows(1, rng.random((100, 3)) * 2))
    M = WALK_WAVES + 5
    queries = np.concatenate([rng.integers(0, 2, (M, 1)).astype(np.float64), rng.random((M, 3)) * 2], 1)
    queries.setflags(write=False), points.setflags(write=False)
    return points, queries


CASES = (ties, entries, ladder, degenerate, rounding, blocks)


@functools.lru_cache(None)
def reference(name, k):
    """the (indices, d2) of case `name` at k: computed once, read-only"""
    c = {f.__name__: f for f in CASES}[name]()
    idx, d2 = knn_reference(c.points, c.queries, k)
    idx.setflags(write=False), d2.setflags(write=False)
    return idx, d2


# ------------------------------------------------------------------------------------------ interpolation
INTERP_D = (1, 3, 70, 512)
INTERP_K = 5


@functools.lru_cache(None)
def interp_lists():
    """lists for interpolate, made by the reference: N = 300 points of two entries (entry 1 holds 3, so its queries have a partial
    tail at k = 5; entry 2 has queries and no points: no valid slot), 40 queries placed on points (zero distances, some twice over:
    duplicates).  -> (points, queries, indices, d2, index i64 [N] into R = 120 rows)"""
    rng = np.random.default_rng(17)
    a = rng.random((297, 3))
    a[1::9] = a[0::9]                                            # duplicate locations: two zero distances for a query placed there
    points = _shuffled(rng, _rows(0, a), _rows(1, rng.random((3, 3))))
    on = points[rng.permutation(300)[:40]]
    queries = np.concatenate([on, _rows(0, rng.random((150, 3))), _rows(1, rng.random((30, 3))), _rows(2, rng.random((10, 3)))], 0)
    idx, d2 = knn_reference(points, queries, INTERP_K)
    index = rng.integers(0, 120, 300).astype(np.int64)
    for a in (idx, d2, index):
        a.setflags(write=False)
    return points, queries, idx, d2, index


def interp_values(R, D, seed=18):
    """fp32 values whose fp16 and bf16 roundings differ from them (so a half input is a different matrix), a few large rows"""
    rng = np.random.default_rng(seed + D)
    v = rng.normal(size=(R, D)).astype(np.float32)
    v[::7] *= 100.0
    return v
