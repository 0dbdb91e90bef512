"""Shared inputs and numpy models for the per-entry kNN over batched coordinates (gp_knn_batched, geopurify_amd.sparse.knn /
affinity_pool): the cases, the key of ops.coords_order_batched, a model of the kernel's ladder (which queries resolve at ring 1, at
ring 3, exhaustively) and the reference lists.

The REFERENCE is oracle.affinity.knn_lattice run per batch entry on that entry's rows in input order, its local row numbers taken
back to input rows: the K+1 smallest by (d^2, row) among the entry's rows, self dropped.  Lists are compared for exact equality,
order included, no row excused.

A case is (C int32 [N,4] = batch, x, y, z in a shuffled row order, K).  Every array is generated from a fixed seed.
"""
import functools

import numpy as np

from oracle import affinity as o_aff

KNN_MAXTIE = 256                       # ties at the threshold distance the ring kernels keep in LDS
RING1, RING3, EXHAUSTIVE, SHORT = 1, 3, 0, -1


# ------------------------------------------------------------------------------------------ building blocks
def surface_voxels(rng, n, ext=40):
    """about n unique voxels on three sheets (a floor of two layers, a wall, an oblique sheet): the shape of a scanned room"""
    a = np.c_[rng.integers(0, ext, n), rng.integers(0, ext, n), rng.integers(3, 5, n)]
    b = np.c_[rng.integers(0, ext, n // 2), np.full(n // 2, 17), rng.integers(0, 30, n // 2)]
    c = np.c_[rng.integers(0, ext, n // 2), (rng.integers(0, ext, n // 2) * 0.6).astype(int), np.zeros(n // 2, int)]
    c[:, 2] = (c[:, 0] * 0.5).astype(int) + 6
    v = np.unique(np.vstack([a, b, c]), axis=0)
    return v[rng.permutation(len(v))]


def surface_exact(rng, n, ext=40):
    """exactly n unique surface voxels"""
    v = surface_voxels(rng, 2 * n, ext)
    assert len(v) >= n
    return v[:n]


def cube(side, origin=(0, 0, 0)):
    g = np.arange(side)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.asarray(origin)


def shell(d2):
    """every lattice point at squared distance d2 from the origin"""
    r = int(np.sqrt(d2)) + 1
    g = np.arange(-r, r + 1)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return p[(p ** 2).sum(1) == d2]


def sparse_clusters():
    """the clusters of test_knn_sparse_fallback (tests/test_gpu_kernels.py): 9-voxel clumps 60 apart, far beyond ring 3"""
    rng = np.random.default_rng(2)
    pts = []
    for cx in range(0, 900, 60):
        pts.append(np.c_[rng.integers(0, 3, 9) + cx, rng.integers(0, 3, 9), rng.integers(0, 3, 9) + (cx // 7)])
    return np.unique(np.vstack(pts), axis=0)


def batched(entries, rng):
    """{batch index: [n,3]} -> int32 [N,4], the rows of all entries interleaved and shuffled"""
    C = np.vstack([np.c_[np.full(len(v), b), v] for b, v in entries.items()]).astype(np.int64)
    assert len(np.unique(C, axis=0)) == len(C), "the cases hold unique rows"
    return np.ascontiguousarray(C[rng.permutation(len(C))].astype(np.int32))


# ------------------------------------------------------------------------------------------ the cases
INNER5 = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0]])
INNER10 = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [-1, -1, 0]])
TIES120_CENTRE = np.array([20, 20, 20])
TIES312_CENTRE = np.array([40, 40, 40])


def _overlap():
    rng = np.random.default_rng(101)
    v = surface_exact(rng, 300, ext=24)
    return batched({0: v, 1: v.copy()}, rng), 16


def _sizes_97_3000():
    rng = np.random.default_rng(102)
    return batched({0: surface_exact(rng, 97, ext=12), 1: surface_exact(rng, 3000, ext=60)}, rng), 96


def _cube14(K):
    return lambda: (batched({0: cube(14)}, np.random.default_rng(103)), K)


def _ties120():
    """query at the centre, 5 inner voxels and all 120 lattice points with d^2 = 74 (r3(74) = 120, the most below 81): the 17th
    neighbour is one of 120 ties, inside the LDS budget and inside ring 1's bound"""
    pts = np.vstack([np.zeros((1, 3), int), INNER5, shell(74)]) + TIES120_CENTRE
    return batched({0: pts}, np.random.default_rng(104)), 16


def _ties312():
    """centre, 10 inner voxels and all 312 points with d^2 = 314 (r3(314) = 312 > 256, radius below 24): ring 1 finds 11 candidates,
    ring 3 more ties than it keeps, the exhaustive path answers"""
    pts = np.vstack([np.zeros((1, 3), int), INNER10, shell(314)]) + TIES312_CENTRE
    return batched({0: pts}, np.random.default_rng(105)), 20


def _sparse_between_dense():
    """entry 1 = the far-apart clusters, between two dense entries that cover its coordinates: an exhaustive scan over all rows, or a
    cell search that ignores the batch bits, finds the dense entries' voxels"""
    rng = np.random.default_rng(106)
    return batched({0: cube(7, (0, 0, 0)), 1: sparse_clusters(), 2: cube(7, (58, 0, 6))}, rng), 20


def _borders():
    """negative coordinates; entries 0 and 1 both hold the voxel at the global minimum of every axis (its -1 neighbour cells do not
    exist: skipped, never wrapped to 65535); batch indices 0, 1 and 65535; the last cell of one entry and the first of the next are
    adjacent in key order, with equal Morton bits for entries 0 / 1"""
    rng = np.random.default_rng(107)
    return batched({0: cube(7, (-20, -33, -9)), 1: cube(6, (-20, -33, -9)), 65535: np.vstack([cube(6, (30, 30, 30)), cube(3, (-20, 30, -9))])},
                   rng), 20


CASES = {
    "overlap": _overlap,
    "sizes_97_3000": _sizes_97_3000,
    "cube14_k1": _cube14(1),
    "cube14_k7": _cube14(7),
    "cube14_k127": _cube14(127),
    "ties120": _ties120,
    "ties312": _ties312,
    "sparse_between_dense": _sparse_between_dense,
    "borders": _borders,
}


@functools.lru_cache(maxsize=None)
def case(name):
    C, K = CASES[name]()
    C.setflags(write=False)
    return C, K


def row_of(C, batch, xyz):
    """the input row of voxel (batch, x, y, z)"""
    hit = np.flatnonzero((C == np.r_[batch, xyz]).all(1))
    assert len(hit) == 1
    return int(hit[0])


def short_entry_case():
    """an entry of exactly K voxels (entry 3) between two that are long enough -> (C, K, batch index, its rows' count)"""
    rng = np.random.default_rng(108)
    K = 16
    return batched({1: cube(4), 3: cube(4, (1, 2, 3))[:K], 7: cube(5, (9, 9, 9))}, rng), K, 3, K


# ------------------------------------------------------------------------------------------ the key of ops.coords_order_batched
def _spread3(v):
    """bit i of v (i < 16) -> bit 3 i"""
    v = v.astype(np.uint64)
    out = np.zeros_like(v)
    for i in range(16):
        out |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
    return out


def _compact3(m):
    """bit 3 i of m (i < 16) -> bit i"""
    out = np.zeros_like(m)
    for i in range(16):
        out |= ((m >> np.uint64(3 * i)) & np.uint64(1)) << np.uint64(i)
    return out


def keys_of(C):
    """batch << 48 | morton(xyz - min), 16 bits per axis, x lowest; min per axis over ALL rows"""
    rel = C[:, 1:].astype(np.int64) - C[:, 1:].astype(np.int64).min(0)
    assert rel.max() < 65536 and C[:, 0].min() >= 0 and C[:, 0].max() < 65536
    m = _spread3(rel[:, 0]) | (_spread3(rel[:, 1]) << np.uint64(1)) | (_spread3(rel[:, 2]) << np.uint64(2))
    return (C[:, 0].astype(np.uint64) << np.uint64(48)) | m


def decode(keys):
    """-> (batch [N], xyz [N,3]) of the keys"""
    m = keys & np.uint64((1 << 48) - 1)
    xyz = np.stack([_compact3(m), _compact3(m >> np.uint64(1)), _compact3(m >> np.uint64(2))], 1).astype(np.int64)
    return (keys >> np.uint64(48)).astype(np.int64), xyz


# ------------------------------------------------------------------------------------------ the reference and the ladder model
def _entries(C):
    for b in np.unique(C[:, 0]):
        yield int(b), np.flatnonzero(C[:, 0] == b)           # ascending input rows: the local order IS the tie-break order


@functools.lru_cache(maxsize=None)
def oracle_lists(name):
    return oracle_lists_of(*case(name))


def oracle_lists_of(C, K):
    """int64 [N,K] of input rows; rows of an entry with K or fewer voxels hold -1"""
    out = np.full((len(C), K), -1, np.int64)
    for b, idx in _entries(C):
        if len(idx) > K:
            out[idx] = idx[o_aff.knn_lattice(C[idx, 1:], K).numpy()]
    return out


@functools.lru_cache(maxsize=None)
def ladder(name):
    return ladder_of(*case(name))


def ladder_of(C, K):
    """Model of gp_knn_batched's ladder -> (lists int64 [N,K] of input rows, path int [N]: RING1, RING3, EXHAUSTIVE or SHORT).
    Ring R takes its candidates from the (2R+1)^3 cells of key >> 9 around the query's cell, same batch bits; it resolves the query when
    the histogram of d^2 below B = (8R+1)^2 holds K+1 candidates and the threshold distance T -- the d^2 of the (K+1)-th -- has at most
    KNN_MAXTIE candidates; its list is then the K+1 smallest (d^2, id) among the candidates with d^2 <= T, self dropped.  What neither
    ring resolves is answered from all rows of the entry."""
    keys = keys_of(C)
    batch, xyz = decode(keys)
    _, cell = decode((keys >> np.uint64(9)) & np.uint64((1 << 39) - 1))      # the cell's coordinates: 13 bits per axis of key >> 9, under the batch bits
    assert np.array_equal(cell, xyz >> 3) and np.array_equal(batch, C[:, 0])
    N = len(C)
    lists = np.full((N, K), -1, np.int64)
    path = np.full(N, SHORT, np.int64)
    big = np.int64(1) << 40
    for b, idx in _entries(C):
        n = len(idx)
        if n <= K:
            continue
        p, c = xyz[idx], cell[idx]
        d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        cheb = np.abs(c[:, None, :] - c[None, :, :]).max(-1)
        local = np.arange(n)
        todo = np.ones(n, bool)

        def take(rows, eligible):
            key = np.where(eligible, d2[rows] * n + local[None, :], big * n)
            part = np.argpartition(key, K, axis=1)[:, :K + 1]
            order = np.take_along_axis(part, np.argsort(np.take_along_axis(key, part, 1), axis=1), 1)
            return idx[order[:, 1:]]

        for R, tag in ((1, RING1), (3, RING3)):
            rows = np.flatnonzero(todo)
            if not len(rows):
                break
            B = (8 * R + 1) ** 2
            cand = cheb[rows] <= R
            hist = np.where(cand & (d2[rows] < B), d2[rows], big)
            enough = (hist < big).sum(1) >= K + 1
            T = np.partition(hist, K, axis=1)[:, K]
            ok = enough & ((hist == T[:, None]).sum(1) <= KNN_MAXTIE)
            got = take(rows, cand & (d2[rows] <= T[:, None]))
            lists[idx[rows[ok]]] = got[ok]
            path[idx[rows[ok]]] = tag
            todo[rows[ok]] = False
        rows = np.flatnonzero(todo)
        if len(rows):
            lists[idx[rows]] = take(rows, np.ones((len(rows), n), bool))
            path[idx[rows]] = EXHAUSTIVE
    return lists, path


# ------------------------------------------------------------------------------------------ affinity_pool inputs
@functools.lru_cache(maxsize=None)
def pool_case():
    """3 entries of 400 / 650 / 900 surface voxels, shuffled rows -> (C int32 [N,4], X fp32 [N,512] ~ N(0,1), E fp32 [N,128] unit rows)"""
    rng = np.random.default_rng(201)
    C = batched({0: surface_exact(rng, 400, 30), 1: surface_exact(rng, 650, 36), 5: surface_exact(rng, 900, 40)}, rng)
    X = rng.standard_normal((len(C), 512)).astype(np.float32)
    E = rng.standard_normal((len(C), 128))
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)
    for a in (C, X, E):
        a.setflags(write=False)
    return C, X, E


@functools.lru_cache(maxsize=None)
def pool_reference(K=96, sharpen=20.0, num_iters=19):
    """Per entry: oracle.affinity.affinity_weights and pool_gather in fp64 on the oracle's lists -> (w fp64 [N,K] by input row, Y fp64
    [N,512]).  Computed once (the narrower widths are its leading columns: a column never influences another)."""
    import torch
    C, X, E = pool_case()
    nbr = oracle_lists_of(C, K)
    W = np.zeros((len(C), K))
    Y = np.zeros((len(C), X.shape[1]))
    for b, idx in _entries(C):
        inv = np.full(len(C), -1, np.int64)
        inv[idx] = np.arange(len(idx))
        nb = torch.from_numpy(inv[nbr[idx]])
        assert int(nb.min()) >= 0
        w = o_aff.affinity_weights(torch.from_numpy(E[idx]).double(), nb, sharpen)
        W[idx] = w.numpy()
        Y[idx] = o_aff.pool_gather(torch.from_numpy(X[idx].copy()), nb, w, num_iters, chunk=64).numpy() if num_iters else X[idx]
    return W, Y
