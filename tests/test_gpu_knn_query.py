"""sparse.knn_query / sparse.interpolate and ops.knn_query / ops.knn_interpolate on the GPU (csrc/knn_query.hip) against the numpy
references of tests/knn_query_cases.py.

Conditions, not tolerances.  Indices and d^2 are compared as bit patterns and no row is excused: the kernel's d^2 is the reference's
expression with one rounding per operation, and the order is (d^2, row).  The only bound is interpolation's, derived in
knn_query_cases.interpolate_bound: (k + 2) 2^-23 max_j |v_j| per element against the fp64 reference on the upcast values; half inputs
must give the bits of the call on their fp32 upcast; integer results are exact.
"""
import numpy as np
import pytest
import torch

import extent_fence
import knn_query_cases as kc

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import _lib, ops, sparse
    _lib.load()
    return ops, sparse


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _assert_lists(nb, idx, d2, what):
    assert nb.indices.dtype == torch.int64 and nb.distances2.dtype == torch.float64 and nb.indices.shape == idx.shape, what
    got_i, got_d = nb.indices.cpu().numpy(), nb.distances2.cpu().numpy()
    wrong = (got_i != idx).any(1) | (got_d.view(np.int64) != d2.view(np.int64)).any(1)
    assert not wrong.any(), f"{what}: {int(wrong.sum())} rows differ, first {int(np.nonzero(wrong)[0][0])}: {got_i[wrong][0]} {got_d[wrong][0]} " \
                            f"instead of {idx[wrong][0]} {d2[wrong][0]}"


CASE_KS = [(f.__name__, k) for f in kc.CASES for k in f().ks]


@pytest.mark.parametrize("name,k", CASE_KS, ids=[f"{n}-k{k}" for n, k in CASE_KS])
def test_knn_query_is_the_reference(env, name, k):
    ops, sparse = env
    c = {f.__name__: f for f in kc.CASES}[name]()
    idx, d2 = kc.reference(name, k)
    nb = sparse.knn_query(_dev(c.points), _dev(c.queries), k)
    assert nb.num_points == c.points.shape[0]
    _assert_lists(nb, idx, d2, f"{name} k={k}")


def test_ladder_reaches_both_rungs(env):
    """the status words of ops.knn_query on the ladder case: the far queries take the entry scan, the others stop on a shell"""
    ops, sparse = env
    c = kc.ladder()
    _, _, st = ops.knn_query(_dev(c.points), _dev(c.queries), 16)
    st = st.tolist()
    assert st[:3] == [0, 0, 0] and st[3] == 0 and st[8:11] == [0, 0, 0]
    assert st[11] >= len(c.marks["far"]) and sum(st[11:16]) == c.queries.shape[0] and sum(st[12:16]) >= 300


def test_fp32_inputs_are_their_fp64_upcast(env):
    ops, sparse = env
    c = kc.rounding()
    idx, d2 = kc.reference("rounding", 8)
    _assert_lists(sparse.knn_query(_dev(c.points).float(), _dev(c.queries).float(), 8), idx, d2, "fp32 points and queries")
    _assert_lists(sparse.knn_query(_dev(c.points), _dev(c.queries).float(), 8), idx, d2, "fp32 queries")


def test_whole_call_equals_the_per_entry_calls(env):
    ops, sparse = env
    c = kc.entries()
    k = 3
    whole = sparse.knn_query(_dev(c.points), _dev(c.queries), k)
    wi, wd = whole.indices.cpu().numpy(), whole.distances2.cpu().numpy()
    for b in kc.ENTRY_IDS:
        rows, qrows = np.nonzero(c.points[:, 0] == b)[0], np.nonzero(c.queries[:, 0] == b)[0]
        if qrows.size == 0:
            continue
        if rows.size == 0:
            assert (wi[qrows] == -1).all() and np.isinf(wd[qrows]).all()
            continue
        one = sparse.knn_query(_dev(c.points[rows]), _dev(c.queries[qrows]), k)
        oi, od = one.indices.cpu().numpy(), one.distances2.cpu().numpy()
        assert np.array_equal(np.where(oi >= 0, rows[np.maximum(oi, 0)], -1), wi[qrows]), b
        assert np.array_equal(od.view(np.int64), wd[qrows].view(np.int64)), b


def test_row_order_does_not_matter(env):
    """permuting the points renumbers the lists and nothing else -- where d^2 ties, the lower NEW row comes first, as the rule says"""
    ops, sparse = env
    c = kc.blocks()
    rng = np.random.default_rng(5)
    perm = rng.permutation(c.points.shape[0])
    idx, d2 = kc.knn_reference(c.points[perm], c.queries, 16)
    _assert_lists(sparse.knn_query(_dev(c.points[perm]), _dev(c.queries), 16), idx, d2, "permuted points")


def test_more_queries_than_the_walk_has_waves(env):
    """the workgroups stride the queries: every wave of the launch takes a second one"""
    ops, sparse = env
    points, queries = kc.many_queries()
    idx, d2 = kc.knn_reference_vectorised(points, queries, 2)
    _assert_lists(sparse.knn_query(_dev(points), _dev(queries), 2), idx, d2, "many queries")


def test_more_rows_than_the_interpolation_has_waves(env):
    """the same stride in interpolate, on lists made by hand: slot 0 exactly, the weighted sum within the bound"""
    ops, sparse = env
    rng = np.random.default_rng(23)
    M, R, D, k = kc.INTERP_WAVES + 3, 50, 2, 2
    idx, d2 = rng.integers(0, R, (M, k)), rng.random((M, k)) + 0.1
    v = kc.interp_values(R, D)
    nb = sparse.Neighbors(_dev(idx), _dev(d2))
    near = sparse.interpolate(_dev(v), nb, mode="nearest")
    assert torch.equal(near, _dev(v)[_dev(idx[:, 0])])
    w = 1.0 / (d2 + 1e-8)
    w /= w.sum(1, keepdims=True)
    rows = v.astype(np.float64)[idx]                                          # [M, k, D]
    ref, vmax = (w[:, :, None] * rows).sum(1), np.abs(rows).max(1)
    got = sparse.interpolate(_dev(v), nb)
    assert (np.abs(got.cpu().double().numpy() - ref) <= kc.interpolate_bound(k, vmax)).all()
    lab = sparse.interpolate(_dev(np.arange(R)), nb)
    assert torch.equal(lab, _dev(idx[:, 0]))


# ------------------------------------------------------------------------------------------ refusals from the status read-back
@pytest.mark.parametrize("which", ["points", "queries"])
def test_refusals_name_the_offender(env, which):
    ops, sparse = env
    c = kc.entries()

    def call(bad_rows):
        P, Q = c.points.copy(), c.queries.copy()
        target = P if which == "points" else Q
        for r, col, v in bad_rows:
            target[r, col] = v
        return sparse.knn_query(_dev(P), _dev(Q), 3)

    for v in (np.nan, np.inf, -np.inf):
        for col in (1, 2, 3):
            with pytest.raises(ValueError, match=f"knn_query: 1 rows of {which} are not finite"):
                call([(5, col, v)])
    with pytest.raises(ValueError, match=f"knn_query: 2 rows of {which} are not finite"):
        call([(5, 0, np.nan), (9, 2, np.inf)])
    with pytest.raises(ValueError, match=f"knn_query: 1 rows of {which} are not finite"):
        call([(5, 2, 1e39)])                                                  # finite in fp64, not in the fp32 the rule rounds to
    for v in (0.5, -1.0, 65536.0):
        with pytest.raises(ValueError, match=f"knn_query: 1 rows of {which} have a batch index that is no integer in 0..65535"):
            call([(7, 0, v)])
    with pytest.raises(ValueError, match=f"knn_query: 3 rows of {which} have a batch index"):
        call([(1, 0, 0.5), (2, 0, -1.0), (3, 0, 65536.0)])


def test_refusals_on_device_tensors(env):
    ops, sparse = env
    P, Q = _dev(kc.entries().points), _dev(kc.entries().queries)
    with pytest.raises(ValueError, match="knn_query: k=33 outside 1..32"):
        sparse.knn_query(P, Q, 33)
    with pytest.raises(ValueError, match="knn_query: points and queries must be CUDA tensors on one device"):
        sparse.knn_query(P, Q.cpu(), 3)
    with pytest.raises(ValueError, match="queries: expected contiguous CUDA torch.float64"):
        ops.knn_query(P, Q.float(), 3)
    with pytest.raises(ValueError, match="knn_query: k=0 outside"):
        ops.knn_query(P, Q, 0)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.knn_query(P, Q, 3, workspace=torch.empty(256, dtype=torch.uint8, device="cuda"))
    both = torch.empty(Q.shape[0] * 3 * 2, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="two outputs overlap"):
        ops.knn_query(P, Q, 3, buffers={"indices": both[:Q.shape[0] * 3].view(-1, 3), "dist2": both[8:8 + Q.shape[0] * 3].view(torch.float64).view(-1, 3)})


# ------------------------------------------------------------------------------------------ extents
def _f64_out(a, shape, name):
    """extent_fence has no float64 entry: an int64 allocation viewed as float64"""
    return a.out(shape, torch.int64, name=name).view(torch.float64)


def _f64_in(a, array, name):
    return a.inp(torch.from_numpy(array.copy()).view(torch.int64), name=name).view(torch.float64)


@pytest.mark.parametrize("name,k", [("blocks", 16), ("entries", 3), ("ladder", 32)])
def test_knn_query_stays_inside_its_extents(env, name, k):
    ops, sparse = env
    from geopurify_amd import _lib
    lib = _lib.load()
    c = {f.__name__: f for f in kc.CASES}[name]()
    N, M = c.points.shape[0], c.queries.shape[0]
    idx, d2 = kc.reference(name, k)

    def case(a):
        P, Q = _f64_in(a, c.points, "points"), _f64_in(a, c.queries, "queries")
        buffers = {"indices": a.out((M, k), torch.int64, name="indices"), "dist2": _f64_out(a, (M, k), "dist2"),
                   "status": a.out(16, torch.int64, name="status")}
        ws = a.out(lib.gp_knn_query_workspace_bytes(N, M), torch.uint8, name="workspace")
        i, d, st = ops.knn_query(P, Q, k, buffers=buffers, workspace=ws)
        return {"indices": i, "dist2": d.view(torch.int64), "status": st}

    got = extent_fence.run(case)
    assert np.array_equal(got["indices"].cpu().numpy(), idx) and np.array_equal(got["dist2"].cpu().numpy(), d2.view(np.int64))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("D", kc.INTERP_D)
def test_knn_interpolate_stays_inside_its_extents(env, D, dtype):
    ops, sparse = env
    points, queries, idx, d2, index = kc.interp_lists()
    v = torch.from_numpy(kc.interp_values(120, D)).to(dtype)
    M = idx.shape[0]
    item = v.element_size()
    pitch = (D + 16 // item + 16 // item - 1) // (16 // item) * (16 // item)   # pitched values: the next multiple of 16 bytes past D

    def case(a):
        # (extent_fence has no bfloat16 entry either: its bits travel as the int16 it poisons fp16 through)
        V = a.inp(v, pitch=pitch, name="values") if dtype != torch.bfloat16 else a.inp(v.view(torch.float16), pitch=pitch, name="values").view(dtype)
        I, Dd = a.inp(torch.from_numpy(idx.copy()), name="indices"), _f64_in(a, d2, "dist2")
        X = a.inp(torch.from_numpy(index.copy()), name="index")
        outs = {}
        for mode in ("inverse_distance", "nearest"):
            buffers = {"out": a.out((M, D), torch.float32, name=f"out {mode}"), "status": a.out(2, torch.int64, name=f"status {mode}")}
            outs[mode] = ops.knn_interpolate(V, I, Dd, X, mode, buffers=buffers)
            outs[mode + " status"] = buffers["status"]
        lab = {"out": a.out(M, torch.int64, name="labels"), "status": a.out(2, torch.int64, name="status labels")}
        outs["labels"] = ops.knn_interpolate(a.inp(torch.arange(120) * 3, name="label values"), I, Dd, X, buffers=lab)
        return outs

    got = extent_fence.run(case)
    assert extent_fence.unwritten(got["inverse_distance"]) == 0 and got["inverse_distance status"].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------ interpolate
def _nb(sparse, idx, d2, n):
    return sparse.Neighbors(_dev(idx), _dev(d2), n)


@pytest.mark.parametrize("with_index", [True, False], ids=["index", "direct"])
@pytest.mark.parametrize("mode,eps", [("inverse_distance", 1e-8), ("inverse_distance", 0.0), ("inverse_distance", 0.5), ("nearest", 1e-8)])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("D", kc.INTERP_D)
def test_interpolate_is_within_the_derived_bound(env, D, dtype, mode, eps, with_index):
    ops, sparse = env
    points, queries, idx, d2, index = kc.interp_lists()
    R = 120 if with_index else 300
    v = torch.from_numpy(kc.interp_values(R, D)).to(dtype)
    up = v.float()                                                            # exact
    ix = index if with_index else None
    ref, vmax, bl, bi = kc.interpolate_reference(up.double().numpy(), idx, d2, 300, ix, mode, eps)
    status = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    nb = _nb(sparse, idx, d2, 300)
    kw = dict(index=None if ix is None else _dev(ix), mode=mode, eps=eps)
    got = sparse.interpolate(v.cuda(), nb, status=status, **kw)
    assert got.dtype == torch.float32 and got.shape == (idx.shape[0], D) and got.is_contiguous() and not got.requires_grad
    err = np.abs(got.cpu().double().numpy() - ref)
    bound = kc.interpolate_bound(kc.INTERP_K, vmax)
    worst = float((err - bound).max())
    print(f"D={D} {dtype} {mode} eps={eps}: max err {err.max():.3e}, max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert worst <= 0, f"|out - ref| exceeds (k + 2) 2^-23 max|v| by {worst:.3e}"
    assert (got[_dev((idx == -1).all(1))] == 0).all()                         # no valid slot: a zero row
    assert status.tolist() == [0, 0] == [bl, bi]
    if mode == "nearest":
        has = idx[:, 0] >= 0
        rows = idx[has, 0] if ix is None else ix[idx[has, 0]]
        assert torch.equal(got[_dev(has)], up.cuda()[_dev(rows)])             # slot 0, exactly
    if dtype != torch.float32:
        again = sparse.interpolate(up.cuda(), nb, **kw)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))    # the bits of the call on the fp32 upcast


def test_interpolate_reads_strided_values_and_ignores_requires_grad(env):
    ops, sparse = env
    points, queries, idx, d2, index = kc.interp_lists()
    wide = torch.from_numpy(kc.interp_values(120, 75)).cuda()
    view = wide[:, 2:72]                                                      # row stride 75, an odd base: the one-element path
    nb = _nb(sparse, idx, d2, 300)
    got = sparse.interpolate(view.requires_grad_(False), nb, index=_dev(index))
    plain = sparse.interpolate(view.contiguous().requires_grad_(True), nb, index=_dev(index))
    assert torch.equal(got.view(torch.int32), plain.view(torch.int32)) and not plain.requires_grad and plain.grad_fn is None


@pytest.mark.parametrize("with_index", [True, False], ids=["index", "direct"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.uint8], ids=str)
def test_integer_values_take_slot_0(env, dtype, with_index):
    ops, sparse = env
    points, queries, idx, d2, index = kc.interp_lists()
    R = 120 if with_index else 300
    values = (np.arange(R) * 7 % 200).astype(np.int64)
    ix = index if with_index else None
    ref, _, _ = kc.labels_reference(values, idx, 300, ix, unlabeled=254)
    nb = _nb(sparse, idx, d2, 300)
    for mode in ("inverse_distance", "nearest"):
        got = sparse.interpolate(_dev(values, dtype), nb, index=None if ix is None else _dev(ix), mode=mode, unlabeled=254)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), ref)
    assert (ref == 254).sum() == (idx[:, 0] == -1).sum() > 0
    default = sparse.interpolate(_dev(values), nb, index=None if ix is None else _dev(ix))
    assert (default.cpu().numpy()[idx[:, 0] == -1] == 255).all()


def test_planted_entries_are_never_dereferenced(env):
    """-5 and N in the lists, R and -5 in the index: zero rows / unlabeled, the exact counts in the status, every other row unchanged"""
    ops, sparse = env
    points, queries, idx, d2, index = kc.interp_lists()
    N, R, D = 300, 120, 70
    v = kc.interp_values(R, D)
    planted = idx.copy()
    planted[0, 1], planted[1, 0], planted[2, 4], planted[3, 0] = -5, N, N, 2 ** 40
    bad_index = index.copy()
    bad_index[idx[60, 0]], bad_index[idx[61, 1]] = R, -5
    for mode in ("inverse_distance", "nearest"):
        ref, vmax, bl, bi = kc.interpolate_reference(v.astype(np.float64), planted, d2, N, bad_index, mode)
        clean, _, _, _ = kc.interpolate_reference(v.astype(np.float64), idx, d2, N, index, mode)
        assert bl >= 2 and bi >= 1
        status = torch.zeros(2, dtype=torch.int64, device="cuda")
        got = sparse.interpolate(_dev(v), _nb(sparse, planted, d2, N), index=_dev(bad_index), mode=mode, status=status)
        assert status.tolist() == [bl, bi]
        zero = (ref == 0).all(1)
        assert (got.cpu().numpy()[zero] == 0).all() and zero.sum() >= (clean == 0).all(1).sum() + bl
        assert (np.abs(got.cpu().double().numpy() - ref) <= kc.interpolate_bound(kc.INTERP_K, vmax)).all()
    values = np.arange(R, dtype=np.int64)
    ref, bl, bi = kc.labels_reference(values, planted, N, bad_index)
    status = torch.zeros(2, dtype=torch.int64, device="cuda")
    got = sparse.interpolate(_dev(values), _nb(sparse, planted, d2, N), index=_dev(bad_index), status=status)
    assert np.array_equal(got.cpu().numpy(), ref) and status.tolist() == [bl, bi] and bl == 2 and bi >= 1
    hand = sparse.Neighbors(_dev(planted), _dev(d2))                          # lists made by hand: the index's length is the range
    assert torch.equal(sparse.interpolate(_dev(values), hand, index=_dev(bad_index)), got)


def test_composition_with_quantize_is_a_gather(env):
    """interpolate(y_F, knn_query(points, points, 1), index=inv) == y_F[inv], bit for bit, on a cloud without duplicate locations"""
    ops, sparse = env
    rng = np.random.default_rng(21)
    xyz = rng.permutation(40 * 40 * 40)[:3000]
    xyz = np.stack([xyz // 1600, xyz // 40 % 40, xyz % 40], 1) * 0.013 + 0.004          # distinct locations, several per voxel at 0.05
    points = _dev(np.concatenate([rng.integers(0, 3, (3000, 1)).astype(np.float64), xyz], 1))
    q = sparse.quantize(points, quantization_size=0.05)
    inv = q.inverse_mapping
    nv = q.coordinates.shape[0]
    assert nv < 3000
    y_F = torch.from_numpy(rng.normal(size=(nv, 96)).astype(np.float32)).cuda()
    nb = sparse.knn_query(points, points, 1)
    assert torch.equal(nb.indices[:, 0], torch.arange(3000, device="cuda")) and (nb.distances2 == 0).all()
    got = sparse.interpolate(y_F, nb, index=inv)
    assert torch.equal(got.view(torch.int32), y_F[inv].view(torch.int32))
    pred = torch.from_numpy(rng.integers(0, 20, nv)).cuda()
    assert torch.equal(sparse.interpolate(pred, nb, index=inv), pred[inv])
