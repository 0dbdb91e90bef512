"""The claims of tests/knn_query_cases.py, checked on the CPU: each case holds the mechanism it was built for, the references agree with
an independent formulation, and sparse.knn_query / sparse.interpolate refuse what they can refuse before any kernel."""
import numpy as np
import pytest
import torch

import knn_query_cases as kc


def test_max_k_is_the_library_constant():
    from geopurify_amd import _lib
    assert kc.MAX_K == _lib.GP_KNN_QUERY_MAX_K == 32
    assert _lib.GP_KNN_MAX_K == 127


@pytest.mark.parametrize("case", kc.CASES, ids=lambda f: f.__name__)
def test_reference_is_the_stable_sort_of_exact_distances(case):
    """np.lexsort((row, d2)) per query == a stable argsort of d2 over the entry's rows in ascending row, in one vectorised pass"""
    c = case()
    k = c.ks[-1]
    idx, d2 = kc.reference(c.name, k)
    P, Q = c.points[:, 1:].astype(np.float32).astype(np.float64), c.queries[:, 1:].astype(np.float32).astype(np.float64)
    for b in np.unique(c.queries[:, 0]):
        rows, qrows = np.nonzero(c.points[:, 0] == b)[0], np.nonzero(c.queries[:, 0] == b)[0]
        if rows.size == 0:
            assert (idx[qrows] == -1).all() and np.isinf(d2[qrows]).all()
            continue
        d = Q[qrows, None, :] - P[None, rows, :]
        dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        order = np.argsort(dist, axis=1, kind="stable")[:, :k]
        m = order.shape[1]
        assert np.array_equal(idx[qrows, :m], rows[order])
        assert np.array_equal(d2[qrows, :m].view(np.int64), np.take_along_axis(dist, order, 1).view(np.int64))
        assert (idx[qrows, m:] == -1).all() and np.isinf(d2[qrows, m:]).all()
    assert not idx.flags.writeable and not d2.flags.writeable


def test_ties_are_exact_and_outnumber_the_slots():
    c = kc.ties()
    assert c.points.shape == (432, 4) and c.queries.shape == (341, 4) and c.ks == (1, 3, 8, 32)
    assert np.unique(c.points, axis=0).shape[0] == 216                        # every point stored twice
    xyz = c.points[:, 1:]
    for k in c.ks:
        idx, d2 = kc.reference("ties", k)
        assert np.array_equal(d2 * 4, np.round(d2 * 4))                       # quarters: no rounding anywhere
        kth = d2[:, -1]
        dq = ((c.queries[:, None, 1:] - xyz[None]) ** 2).sum(-1)
        tied, below = (dq == kth[:, None]).sum(1), (dq < kth[:, None]).sum(1)
        assert ((tied > k - below)[c.marks["centres"]]).all() or k == 1       # more candidates at the k-th distance than slots left
        if k == 32:
            assert tied[c.marks["centres"]].min() >= 24                       # dozens
        if k >= 3:
            assert (d2[c.marks["nodes"], :2] == 0).all() and (d2[c.marks["nodes"], 2] > 0).all()    # d^2 = 0 twice over
            n = idx[c.marks["nodes"]]
            assert (n[:, 0] < n[:, 1]).all() and np.array_equal(xyz[n[:, 0]], xyz[n[:, 1]])           # the duplicate rows, by row


def test_entries_overlap_interleave_and_run_short():
    c = kc.entries()
    pb, qb = c.points[:, 0], c.queries[:, 0]
    assert set(pb) == {0, 3, 7, 65535} and set(qb) == {0, 3, 4000, 65535} and set(kc.ENTRY_IDS) == set(pb) | set(qb)
    assert (np.diff(pb) < 0).any() and (np.diff(qb) < 0).any()               # rows interleaved
    idx, d2 = kc.reference("entries", 3)
    both = np.isin(qb, (0, 3))
    other = np.where(qb[both] == 0, 3, 0)
    nearer = 0
    for q, o, own in zip(c.queries[both], other, d2[both, 0]):
        P = c.points[pb == o, 1:].astype(np.float32).astype(np.float64)
        nearer += int((((q[1:].astype(np.float32) - P) ** 2).sum(1)).min() < own)
    assert nearer * 2 >= int(both.sum()), (nearer, int(both.sum()))           # a point of the other entry is nearer: at least half
    assert (pb[idx[both]] == qb[both][:, None]).all()                         # and still never listed
    assert (idx[qb == 4000] == -1).all() and np.isinf(d2[qb == 4000]).all()
    short = qb == 65535
    assert (idx[short, :2] >= 0).all() and (idx[short, 2] == -1).all() and np.isinf(d2[short, 2]).all() and np.isfinite(d2[short, :2]).all()


def test_ladder_overflows_a_cell_and_exhausts_the_grid():
    c = kc.ladder()
    assert c.points.shape[0] == kc.CLUMP_POINTS + 1000 and c.queries.shape[0] == 630 and kc.ladder_directions().shape == (20, 3)
    assert np.unique(kc.ladder_directions(), axis=0).shape[0] == 20
    in_clump = np.linalg.norm(c.points[:, 1:] - c.marks["centre"], axis=1) <= kc.CLUMP_RADIUS
    assert int(in_clump.sum()) > 64 * kc.MAX_K
    for k in c.ks:
        idx, d2 = kc.reference("ladder", k)
        assert (np.sqrt(d2[c.marks["far"], -1]) > kc.BOX * np.sqrt(3.0)).all()       # farther than the box diagonal
        assert (np.sqrt(d2[c.marks["clump"], -1]) <= 2 * kc.CLUMP_RADIUS).all() and in_clump[idx[c.marks["clump"]]].all()
    outside = np.abs(c.queries[c.marks["far"], 1:] - kc.BOX / 2).max(1) - kc.BOX / 2
    assert np.allclose(outside, 1e3)


def test_degenerate_boxes():
    c = kc.degenerate()
    P = c.points
    assert np.ptp(P[P[:, 0] == 0, 3]) == 0 and np.ptp(P[P[:, 0] == 1, 2]) == 0 and np.ptp(P[P[:, 0] == 1, 3]) == 0
    assert np.ptp(P[P[:, 0] == 2, 1:], axis=0).max() == 0 and int((P[:, 0] == 2).sum()) == 500
    assert all(int((P[:, 0] == b).sum()) == 1 for b in (3, 4, 5, 6))
    idx, d2 = kc.reference("degenerate", 32)
    spot = np.nonzero(c.queries[:, 0] == 2)[0]
    lowest = np.nonzero(P[:, 0] == 2)[0][:32]
    assert (idx[spot] == lowest).all()                                        # the 32 lowest rows ...
    assert (d2[spot] == d2[spot, :1]).all() and (d2[spot] == 0).any()         # ... d^2 equal
    single = c.queries[:, 0] >= 3
    assert (idx[single, 0] >= 0).all() and (idx[single, 1:] == -1).all()


def test_rounding_to_fp32_merges_neighbours_and_changes_the_order():
    c = kc.rounding()
    assert np.unique(c.points[:, 1:], axis=0).shape[0] == 600
    assert np.unique(c.points[:, 1:].astype(np.float32), axis=0).shape[0] < 600          # some pairs merge
    idx, d2 = kc.reference("rounding", 8)
    idx64, _ = kc.knn_reference(c.points, c.queries, 8, round32=False)
    assert (idx != idx64).any(1).mean() > 0.5                                 # the order differs from the unrounded one
    assert (d2[:, 0] == d2[:, 1]).any()                                       # merged locations tie exactly


def test_blocks_case_sizes():
    c = kc.blocks()
    assert c.queries.shape[0] == 4 * 256 + 1 and c.points.shape[0] == 4097 and c.ks == (16,)


def test_vectorised_reference_is_the_reference():
    for name, k in (("entries", 3), ("ties", 8), ("degenerate", 32)):
        c = {f.__name__: f for f in kc.CASES}[name]()
        idx, d2 = kc.reference(name, k)
        vi, vd = kc.knn_reference_vectorised(c.points, c.queries, k, chunk=100)
        assert np.array_equal(vi, idx) and np.array_equal(vd.view(np.int64), d2.view(np.int64))
    points, queries = kc.many_queries()
    assert queries.shape[0] > kc.WALK_WAVES and set(queries[:, 0]) == {0.0, 1.0} == set(points[:, 0])


def test_interpolation_lists_hold_every_kind_of_row():
    points, queries, idx, d2, index = kc.interp_lists()
    valid = (idx >= 0).sum(1)
    assert set(valid) == {0, 3, 5}                                            # no valid slot, a partial tail, full rows
    assert ((d2[:, :2] == 0).all(1)).any() and ((d2[:, 0] == 0) & (d2[:, 1] > 0)).any()   # zero distances, twice over and once
    assert index.shape == (300,) and index.max() < 120


def test_interpolate_reference_properties():
    points, queries, idx, d2, index = kc.interp_lists()
    v = kc.interp_values(120, 3).astype(np.float64)
    out, vmax, bl, bi = kc.interpolate_reference(v, idx, d2, 300, index, "nearest")
    has = idx[:, 0] >= 0
    assert np.array_equal(out[has], v[index[idx[has, 0]]]) and (out[~has] == 0).all() and (bl, bi) == (0, 0)
    out0, _, _, _ = kc.interpolate_reference(v, idx, d2, 300, index, "inverse_distance", eps=0.0)
    two = (d2[:, :2] == 0).all(1) & (d2[:, 2] > 0)
    assert two.any() and np.allclose(out0[two], (v[index[idx[two, 0]]] + v[index[idx[two, 1]]]) / 2, rtol=1e-15, atol=0)
    oute, vmax, _, _ = kc.interpolate_reference(v, idx, d2, 300, index)
    assert (np.abs(oute) <= vmax * (1 + 1e-12)).all()                         # a convex combination
    planted = idx.copy()
    planted[0, 1], planted[1, 0], planted[2, 2] = -5, 300, 300
    bad_index = index.copy()
    bad_index[idx[5, 0]] = 120
    _, _, bl, bi = kc.interpolate_reference(v, planted, d2, 300, bad_index)
    assert bl == 3 and bi == int((idx[3:] == idx[5, 0]).any(1).sum())
    lab, bl, bi = kc.labels_reference(np.arange(120), planted, 300, bad_index, unlabeled=77)
    assert bl == 1 and lab[1] == 77 and (lab[idx[:, 0] == -1] == 77).all()
    assert kc.interpolate_bound(5, np.ones(1))[0] == 7 * 2.0 ** -23


# ------------------------------------------------------------------------------------------ refusals that need no kernel
def _cloud(n=4, dtype=torch.float64):
    return torch.zeros((n, 4), dtype=dtype)


@pytest.mark.parametrize("k", [True, 3.0, "3", None, 0, -1, 33])
def test_knn_query_refuses_k(k):
    from geopurify_amd import sparse
    with pytest.raises(ValueError, match="knn_query: k="):
        sparse.knn_query(_cloud(), _cloud(), k)


@pytest.mark.parametrize("name,pos", [("points", 0), ("queries", 1)])
def test_knn_query_refuses_shapes_dtypes_and_devices(name, pos):
    from geopurify_amd import sparse

    def call(bad):
        args = [_cloud(), _cloud()]
        args[pos] = bad
        return sparse.knn_query(*args, 3)

    for bad in (torch.zeros((4, 3), dtype=torch.float64), torch.zeros(4, dtype=torch.float64), np.zeros((4, 4)), None):
        with pytest.raises(ValueError, match=rf"knn_query: {name} must be \[[NM], 4\]"):
            call(bad)
    for bad in (_cloud(dtype=torch.float16), _cloud(dtype=torch.int64)):
        with pytest.raises(ValueError, match=f"knn_query: {name} must be fp64 or fp32"):
            call(bad)
    with pytest.raises(ValueError, match=rf"knn_query: 0 {name} outside 1\.\.2\^31-1"):
        call(_cloud(0))
    with pytest.raises(ValueError, match=rf"knn_query: {2 ** 31} {name} outside 1\.\.2\^31-1"):
        call(torch.zeros((2 ** 31, 4), dtype=torch.float64, device="meta"))
    with pytest.raises(ValueError, match="knn_query: points and queries must be CUDA tensors on one device"):
        call(_cloud())


def test_interpolate_refuses_before_any_kernel():
    from geopurify_amd import sparse
    nb = sparse.Neighbors(torch.zeros((6, 3), dtype=torch.int64), torch.zeros((6, 3), dtype=torch.float64), 10)
    v = torch.zeros((10, 4))
    refusals = [
        (dict(values=v, nb=(nb.indices, nb.distances2)), "nb must be the Neighbors"),
        (dict(values=v, nb=sparse.Neighbors(nb.indices.int(), nb.distances2)), "nb must hold indices i64"),
        (dict(values=v, nb=sparse.Neighbors(nb.indices, nb.distances2.float())), "nb must hold indices i64"),
        (dict(values=v, nb=sparse.Neighbors(torch.zeros((6, 33), dtype=torch.int64), torch.zeros((6, 33), dtype=torch.float64))), "k in 1..32"),
        (dict(values=v.double(), nb=nb), "values must be fp32, fp16 or bf16"),
        (dict(values=torch.zeros(10), nb=nb), "values must be fp32, fp16 or bf16"),
        (dict(values=torch.zeros((10, 8))[:, ::2], nb=nb), "values must have unit column stride"),
        (dict(values=torch.zeros((10, 2), dtype=torch.int64), nb=nb), r"integer values must be \[R\]"),
        (dict(values=torch.zeros((9, 4)), nb=nb), "values holds 9 rows, the lists name rows of 10 points"),
        (dict(values=v, nb=nb, index=torch.zeros(10)), "index must be an integer tensor"),
        (dict(values=v, nb=nb, index=torch.zeros((10, 1), dtype=torch.int64)), "index must be an integer tensor"),
        (dict(values=v, nb=nb, index=torch.zeros(11, dtype=torch.int64)), "index holds 11 rows"),
        (dict(values=v, nb=nb, mode="linear"), "mode='linear'"),
        (dict(values=v, nb=nb, eps=-1e-8), "eps="),
        (dict(values=v, nb=nb, eps=float("nan")), "eps="),
        (dict(values=v, nb=nb, eps=True), "eps="),
        (dict(values=torch.zeros(10, dtype=torch.int64), nb=nb, unlabeled=2.5), "unlabeled="),
        (dict(values=v, nb=nb, status=torch.zeros(3, dtype=torch.int64)), "status must be"),
        (dict(values=v, nb=nb), "must be CUDA tensors on one device"),
    ]
    for kw, words in refusals:
        values, lists = kw.pop("values"), kw.pop("nb")
        with pytest.raises(ValueError, match="interpolate: .*" + words):
            sparse.interpolate(values, lists, **kw)


def test_docstrings_state_the_contract():
    from geopurify_amd import sparse
    assert "knn_query(points, benchmark_vertices, 3)" in sparse.__doc__ and "interpolate(seg.pred, nb, index=q.inverse_mapping)" in sparse.__doc__
    assert "requires_grad is ignored" in sparse.interpolate.__doc__ and "detached" in sparse.interpolate.__doc__
