"""The claims of tests/knn_interpolate_grad_cases.py, checked on the CPU: each case holds the mechanism it was built for, the fp64
reference is torch's fp64 autograd of the dense composite, the rule's reference is within the derived bound of it, and
sparse.interpolate(differentiable=True) / Neighbors.transpose refuse what they can refuse before any kernel."""
import numpy as np
import pytest
import torch

import knn_interpolate_grad_cases as gc


def _cases():
    return [gc.grid_lists(1, True), gc.grid_lists(3, False), gc.grid_lists(32, True), gc.hub(), gc.folded(), gc.planted()]


def _autograd64(g, L, mode, eps):
    """torch fp64 autograd of the dense composite (values64[rows] * w[..., None]).sum(1) against the upstream gradient g"""
    ref, rows, _, _ = gc.references(L, mode)
    w = torch.from_numpy(gc.weights64(L, mode, eps))
    values = torch.zeros((L.R, g.shape[1]), dtype=torch.float64, requires_grad=True)
    out = (values[torch.from_numpy(rows)] * w[..., None]).sum(1)
    out.backward(torch.from_numpy(g.astype(np.float64)))
    return values.grad.numpy()


@pytest.mark.parametrize("mode,eps", [("inverse_distance", 1e-8), ("inverse_distance", 0.0), ("inverse_distance", 0.5), ("nearest", 1e-8)])
def test_fp64_reference_is_torch_autograd(mode, eps):
    for L in _cases():
        g = gc.grads(L.indices.shape[0], 3)
        d, scale, count = gc.fp64_reference(g, L, mode, eps)
        auto = _autograd64(g, L, mode, eps)
        assert np.abs(d - auto).max() <= 1e-12 * max(1.0, scale.max()), L.name     # (summation order differs: fp64 round-off only)
        assert count.sum() == gc.references(L, mode)[0].sum()
        assert (d[count == 0] == 0).all()


def test_weights64_are_a_partition_of_one():
    for L in _cases():
        for eps in gc.GRAD_EPS:
            w = gc.weights64(L, "inverse_distance", eps)
            ref, _, _, _ = gc.references(L)
            has = ref.any(1)
            assert np.allclose(w[has].sum(1), 1.0, rtol=1e-14, atol=0) and (w[~has] == 0).all() and (w[~ref] == 0).all()
        w = gc.weights64(L, "nearest")
        assert (w[:, 1:] == 0).all() and set(np.unique(w[:, 0])) <= {0.0, 1.0}


def test_rule_reference_is_within_the_bound_of_the_fp64_reference():
    """with fp32-rounded fp64 weights the rule's own reference meets (L + 2) 2^-23 sum |w g|: the bound is the rule's, not the GPU's"""
    for L in _cases():
        g = gc.grads(L.indices.shape[0], 3)
        w32 = gc.weights64(L).astype(np.float32)
        d = gc.rule_reference(g, L, w32)
        ref, scale, count = gc.fp64_reference(g, L)
        assert (np.abs(d.astype(np.float64) - ref) <= gc.grad_bound(count, scale)).all(), L.name
        assert d.dtype == np.float32 and not np.signbit(d[count == 0]).any()


def test_rule_reference_is_sequential_in_ascending_flat_slot():
    """against the literal loop, on the case with the longest lists after the hub"""
    L = gc.folded()
    g = gc.grads(L.indices.shape[0], 3)
    w32 = gc.weights64(L).astype(np.float32)
    ref, rows, _, _ = gc.references(L)
    k = L.indices.shape[1]
    out = np.zeros((L.R, 3), np.float32)
    for f in np.nonzero(ref.reshape(-1))[0]:
        r = rows.reshape(-1)[f]
        out[r] = out[r] + w32.reshape(-1)[f] * g[f // k]
    assert np.array_equal(gc.rule_reference(g, L, w32).view(np.int32), out.view(np.int32))


def test_forward_reference_is_the_weighted_gather():
    L = gc.grid_lists(3, True)
    v = gc.grads(L.R, 3, seed=50)
    w = gc.weights64(L)
    ref, rows, _, _ = gc.references(L)
    dense = (v.astype(np.float64)[rows] * w[..., None]).sum(1)
    assert np.allclose(gc.forward_reference(v, L, w.astype(np.float32)), dense, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------ each case holds what it exists for
def test_hub_row_has_more_than_4096_references():
    L = gc.hub()
    ref, rows, _, _ = gc.references(L)
    count = np.bincount(rows[ref], minlength=L.R)
    assert count[L.marks["hub_row"]] > 4096 and count[L.marks["hub_row"]] >= gc.HUB_QUERIES
    assert (L.indices[300:, 0] == L.marks["hub_row"]).all()
    assert np.median(count) < 64                                              # among ordinary rows


def test_some_rows_have_no_references():
    for L in (gc.grid_lists(3, True), gc.grid_lists(3, False), gc.grid_lists(1, False), gc.hub()):
        ref, rows, _, _ = gc.references(L)
        count = np.bincount(rows[ref], minlength=L.R)
        assert (count == 0).any() and (count > 0).any(), L.name
    L = gc.grid_lists(3, True)
    assert (np.bincount(gc.references(L)[1][gc.references(L)[0]], minlength=L.R)[120:] == 0).all() and L.R == gc.R_INDEX == 130


def test_some_list_names_one_row_twice():
    L = gc.folded()
    ref, rows, _, _ = gc.references(L)
    twice = [(ref[q].sum() >= 2) and len(set(rows[q][ref[q]])) < ref[q].sum() for q in range(L.indices.shape[0])]
    assert sum(twice) >= 10
    assert np.bincount(rows[ref], minlength=L.R).min() > 20                  # many points, and references, per row


def test_some_query_rows_are_excused():
    L = gc.planted()
    ref, rows, excused, named = gc.references(L)
    assert excused[:3].all() and excused[5] and excused[9] and 5 <= excused.sum() < 40
    assert not ref[excused].any() and named[excused].any()                   # valid slots of an excused row are no references
    base = gc.grid_lists(3, True)
    assert base.indices[5, 0] >= 0 and base.indices[9, 1] >= 0
    assert not gc.references(gc.planted(), "nearest")[2][0]                   # row 0's planted entry is in slot 1: "nearest" does not read it
    assert gc.references(gc.planted(), "nearest")[2][1]


def test_minus_one_tails_are_present():
    for k in gc.GRAD_K:
        L = gc.grid_lists(k, True)
        valid = (L.indices >= 0).sum(1)
        assert 0 in set(valid) and k in set(valid)
        if k > 3:
            assert 3 in set(valid)                                            # entry 1 holds 3 points: a -1 tail
    tail = gc.grid_lists(32, False).indices
    assert ((tail[:, 3:] == -1).all(1) & (tail[:, :3] >= 0).all(1)).any()


def test_zero_distance_ties_are_present():
    L = gc.grid_lists(3, False)
    assert ((L.d2[:, :2] == 0).all(1) & (L.d2[:, 2] > 0)).any()
    w = gc.weights64(L, eps=0.0)
    two = (L.d2[:, :2] == 0).all(1) & (L.d2[:, 2] > 0)
    assert (w[two, :2] == 0.5).all() and (w[two, 2] == 0).all()
    assert gc.references(L)[0][two].all()                                     # weight 0, still a reference


def test_big_case_takes_the_row_strides():
    L = gc.big()
    assert L.R == 262147 > gc.BACKWARD_WAVES and L.indices.shape == (90000, 3)
    ref, rows, _, _ = gc.references(L)
    assert ref.all() and (rows >= gc.BACKWARD_WAVES).any() and L.indices.shape[0] * 3 < 2 ** 31


# ------------------------------------------------------------------------------------------ refusals that need no kernel
def _nb(sparse, M=6, k=3, n=10, device=None):
    return sparse.Neighbors(torch.zeros((M, k), dtype=torch.int64, device=device), torch.zeros((M, k), dtype=torch.float64, device=device), n)


def test_differentiable_interpolate_refuses_before_any_kernel():
    from geopurify_amd import sparse
    nb, v = _nb(sparse), torch.zeros((10, 4), requires_grad=True)
    t = sparse.NeighborsTranspose(torch.zeros(11, dtype=torch.int64), torch.zeros(18, dtype=torch.int32), torch.zeros(18), 6, 3, 10,
                                  "inverse_distance", 1e-8)
    refusals = [
        (dict(values=torch.zeros(10, dtype=torch.int64), differentiable=True), "differentiable=True takes floating values"),
        (dict(values=v, differentiable=1), "differentiable=1 must be a bool"),
        (dict(values=v, transpose=t), "transpose goes with differentiable=True"),
        (dict(values=v, differentiable=True, transpose=(1, 2)), "transpose must be the NeighborsTranspose"),
        (dict(values=v, differentiable=True, transpose=t, eps=0.5), "transpose was built for"),
        (dict(values=v, differentiable=True, transpose=t, mode="nearest"), "transpose was built for"),
        (dict(values=v, differentiable=True, transpose=sparse.NeighborsTranspose(t.offsets, t.slots, t.weights, 6, 3, 11, t.mode, t.eps)),
         "transpose was built for"),
        (dict(values=v, differentiable=True, transpose=t), "must be CUDA tensors on one device"),
    ]
    for kw, words in refusals:
        values = kw.pop("values")
        with pytest.raises(ValueError, match="interpolate: .*" + words):
            sparse.interpolate(values, nb, **kw)


def test_too_many_flat_slots_are_refused_without_allocating():
    """M * k over 2^31-1: a hand-made Neighbors on the meta device has the shapes and no memory"""
    from geopurify_amd import sparse
    M = 2 ** 31 // 32
    nb = _nb(sparse, M, 32, None, device="meta")
    assert M * 32 == 2 ** 31
    with pytest.raises(ValueError, match=r"interpolate: M \* k = 2147483648 flat slots, more than 2\^31-1"):
        sparse.interpolate(torch.zeros((10, 4), requires_grad=True), nb, differentiable=True)
    with pytest.raises(ValueError, match=r"Neighbors.transpose: M \* k = 2147483648 flat slots"):
        nb.transpose(num_rows=10)
    ok = _nb(sparse, M, 31, None, device="meta")                              # 2^31 - 2^26 slots pass this check (and stop at the device's)
    with pytest.raises(ValueError, match="must be CUDA tensors on one device"):
        sparse.interpolate(torch.zeros((10, 4), requires_grad=True), ok, differentiable=True)


def test_transpose_refuses_before_any_kernel():
    from geopurify_amd import sparse
    nb = _nb(sparse)
    for kw, words in [(dict(index=torch.zeros(10, dtype=torch.int64)), "num_rows=None must be the row count"),
                      (dict(num_rows=True), "num_rows=True"), (dict(num_rows=0), "num_rows=0"),
                      (dict(num_rows=9), "num_rows is 9 rows, the lists name rows of 10 points"),
                      (dict(index=torch.zeros(11, dtype=torch.int64), num_rows=4), "index holds 11 rows"),
                      (dict(index=torch.zeros(10), num_rows=4), "index must be an integer tensor"),
                      (dict(mode="linear"), "mode='linear'"), (dict(eps=-1.0), "eps="),
                      (dict(), "must be CUDA tensors on one device")]:
        with pytest.raises(ValueError, match="Neighbors.transpose: .*" + words):
            nb.transpose(**kw)


def test_the_library_exports_the_three_entry_points():
    from geopurify_amd import _lib, ops
    lib = _lib.load()
    for name in ("gp_knn_interpolate_weights", "gp_knn_interpolate_transpose", "gp_knn_interpolate_backward"):
        assert hasattr(lib, name)
    assert ops.knn_interpolate_transpose_workspace_bytes(90000, 3, 262147) > 3 * 270000 * 4
    assert ops.knn_interpolate_transpose_workspace_bytes(2 ** 31 // 32, 32, 10) == 0 and ops.knn_interpolate_transpose_workspace_bytes(4, 33, 10) == 0
    assert ops.KNN_INTERPOLATE_MAX_SLOTS == 2 ** 31 - 1


def test_docstrings_state_the_rule():
    from geopurify_amd import sparse
    doc = sparse.interpolate.__doc__
    for words in ("differentiable=True", "ascending f", "acc = acc + w32[f] * g[j,c]", "-ffp-contract=off", "explicit zero row", "no float atomics",
                  "no double backward"):
        assert words in doc, words
    assert "ops.knn_interpolate_transpose" in sparse.__doc__ and "differentiable=True" in sparse.__doc__
