"""sparse.interpolate(differentiable=True), Neighbors.transpose and ops.knn_interpolate_weights / _transpose / _backward on the GPU
(csrc/knn_interpolate_grad.hip) against the numpy references of tests/knn_interpolate_grad_cases.py.

Conditions, not tolerances.  d_values is compared as bit patterns with the rule's reference evaluated on the weights the GPU emitted,
no row excused; fp16 / bf16 gradients are that fp32 reference rounded once.  The emitted weights are within 2^-23 relative of the fp64
weights, and the forward recomputed from them in list order reproduces `out` bit for bit.  The only bound is the derived one against
the fp64 reference: (L + 2) 2^-23 sum |w g| per element, L the row's reference count (knn_interpolate_grad_cases.grad_bound).
"""
import os
import sys

import numpy as np
import pytest
import torch

import extent_fence
import knn_interpolate_grad_cases as gc
import knn_query_cases as kc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
MODES = [("inverse_distance", 1e-8), ("inverse_distance", 0.0), ("inverse_distance", 0.5), ("nearest", 1e-8)]


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


def _nb(sparse, L):
    return sparse.Neighbors(_dev(L.indices), _dev(L.d2), L.N)


def _ix(L):
    return None if L.index is None else _dev(L.index)


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _weights(ops, L, mode, eps):
    return ops.knn_interpolate_weights(_dev(L.indices), _dev(L.d2), _ix(L), L.R, mode, eps).cpu().numpy()


def _backward(sparse, L, values, g, mode="inverse_distance", eps=1e-8, **kw):
    """-> (out, d_values) of interpolate(values, differentiable=True) and out.backward(g)"""
    leaf = values.detach().requires_grad_()
    out = sparse.interpolate(leaf, _nb(sparse, L), index=_ix(L), mode=mode, eps=eps, differentiable=True, **kw)
    out.backward(g)
    return out.detach(), leaf.grad


def _assert_rule(ops, sparse, L, D, dtype=torch.float32, mode="inverse_distance", eps=1e-8, what=""):
    """the whole contract of one call: graph, forward bits, emitted weights, bit-exact gradient, derived bound.  -> the worst
    |d - ref| / bound"""
    M = L.indices.shape[0]
    v = torch.from_numpy(kc.interp_values(L.R, D)).to(dtype)
    g = gc.grads(M, D)
    plain = sparse.interpolate(v.cuda(), _nb(sparse, L), index=_ix(L), mode=mode, eps=eps)
    out, d = _backward(sparse, L, v.cuda(), _dev(g), mode, eps)
    assert _same_bits(out, plain), f"{what}: the differentiable forward is not the default call's bits"
    assert d.dtype == dtype and d.shape == (L.R, D) and d.is_contiguous()
    w32 = _weights(ops, L, mode, eps)
    w64 = gc.weights64(L, mode, eps)
    assert (np.abs(w32.astype(np.float64) - w64) <= 2.0 ** -23 * w64).all(), f"{what}: emitted weights off the fp64 weights"
    fwd = gc.forward_reference(v.float().numpy(), L, w32, mode)
    assert np.array_equal(out.cpu().numpy().view(np.int32), fwd.view(np.int32)), f"{what}: out is not the emitted weights applied in list order"
    rule = gc.rule_reference(g, L, w32, mode)
    want = torch.from_numpy(rule).to(dtype)                                   # one rounding at the end
    got = d.cpu()
    wrong = (_bits(got) != _bits(want)).any(1)
    assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} rows of d_values differ from the rule, first {int(wrong.nonzero()[0, 0])}"
    ref, scale, count = gc.fp64_reference(g, L, mode, eps)
    assert (got[torch.from_numpy(count == 0)].view(torch.int16 if dtype != torch.float32 else torch.int32) == 0).all()   # +0 rows
    if dtype != torch.float32:
        return 0.0
    err, bound = np.abs(got.double().numpy() - ref), gc.grad_bound(count, scale)
    frac = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max err {err.max():.3e}, worst err / bound {frac:.3f}")
    assert (err <= bound).all(), f"{what}: |d - ref| exceeds (L + 2) 2^-23 sum |w g| by {float((err - bound).max()):.3e}"
    return frac


# ------------------------------------------------------------------------------------------ fails without the feature
def test_differentiable_result_is_in_the_graph_with_the_default_bits(env):
    ops, sparse = env
    L = gc.grid_lists(3, True)
    v = torch.from_numpy(kc.interp_values(L.R, 70)).cuda()
    nb = _nb(sparse, L)
    plain = sparse.interpolate(v, nb, index=_ix(L))
    out = sparse.interpolate(v.requires_grad_(), nb, index=_ix(L), differentiable=True)
    assert out.grad_fn is not None and out.requires_grad and _same_bits(out.detach(), plain)
    still = sparse.interpolate(v, nb, index=_ix(L))                           # the default: requires_grad ignored, detached
    assert still.grad_fn is None and not still.requires_grad and _same_bits(still, plain)
    with torch.no_grad():
        off = sparse.interpolate(v, nb, index=_ix(L), differentiable=True)
    none = sparse.interpolate(v.detach(), nb, index=_ix(L), differentiable=True)   # nothing needs a gradient: the plain result
    assert off.grad_fn is None and none.grad_fn is None and _same_bits(off, plain) and _same_bits(none, plain)
    out.sum().backward()
    with pytest.raises(RuntimeError):                                         # once_differentiable: no double backward
        leaf = v.detach().requires_grad_()
        o = sparse.interpolate(leaf, nb, index=_ix(L), differentiable=True)
        (gr,) = torch.autograd.grad(o.sum(), leaf, create_graph=True)
        gr.sum().backward()


# ------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize("k", gc.GRAD_K)
@pytest.mark.parametrize("with_index", [True, False], ids=["index", "direct"])
@pytest.mark.parametrize("mode,eps", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("D", gc.GRAD_D)
def test_gradient_is_the_rule_bit_for_bit(env, D, dtype, mode, eps, with_index, k):
    ops, sparse = env
    _assert_rule(ops, sparse, gc.grid_lists(k, with_index), D, dtype, mode, eps, what=f"D={D} {dtype} {mode} eps={eps} k={k} index={with_index}")


def test_pitched_values_and_non_contiguous_g(env):
    ops, sparse = env
    L = gc.grid_lists(3, True)
    M, D = L.indices.shape[0], 70
    wide = torch.from_numpy(kc.interp_values(L.R, 75)).cuda()
    values = wide[:, 2:72]                                                    # row stride 75, an odd base
    g = gc.grads(M, D)
    _, want = _backward(sparse, L, values.contiguous(), _dev(g))
    _, d = _backward(sparse, L, values, _dev(g))
    assert d.is_contiguous() and d.shape == (L.R, D) and _same_bits(d, want)  # a contiguous gradient for pitched values
    odd = torch.zeros((M, 75), device="cuda")
    odd[:, 1:71] = _dev(g)
    _, d1 = _backward(sparse, L, values, odd[:, 1:71])                        # g read in place: pitch 75, an odd base -> single columns
    pitched = torch.zeros((M, 80), device="cuda")
    pitched[:, :70] = _dev(g)
    _, d2 = _backward(sparse, L, values, pitched[:, :70])                     # pitch 80 on a 16-byte base, D = 70: wide loads, a tail, narrow stores
    _, d3 = _backward(sparse, L, values, _dev(np.ascontiguousarray(g.T)).t())  # column stride != 1: copied
    _, d4 = _backward(sparse, L, values, _dev(g[:1]).expand(M, D))            # row stride 0: copied
    _, want4 = _backward(sparse, L, values, _dev(np.repeat(g[:1], M, 0)))
    assert _same_bits(d1, want) and _same_bits(d2, want) and _same_bits(d3, want) and _same_bits(d4, want4)
    t = _nb(sparse, L).transpose(_ix(L), L.R)
    for dtype in DTYPES:                                                      # the ops wrapper, g in place: the wide-store path of each dtype at D = 72
        p72 = torch.zeros((M, 76), device="cuda")
        p72[:, :72] = _dev(gc.grads(M, 72))
        a = ops.knn_interpolate_backward(p72[:, :72], t.offsets, t.slots, t.weights, 3, dtype)
        b = ops.knn_interpolate_backward(p72[:, :72].contiguous(), t.offsets, t.slots, t.weights, 3, dtype)
        c = ops.knn_interpolate_backward(p72[:, :72].contiguous(), t.offsets, t.slots, t.weights, 3, torch.float32)
        assert _same_bits(a, b) and _same_bits(b, c.to(dtype))


# ------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("D", [3, 8])
def test_hub_row_is_walked_in_order(env, D):
    """5 000 queries list one point: a list of more than 4096 references, walked 64 at a time by one wave"""
    ops, sparse = env
    _assert_rule(ops, sparse, gc.hub(), D, what=f"hub D={D}")


def test_rows_without_references_are_written_as_zeros(env):
    ops, sparse = env
    L = gc.grid_lists(3, True)
    t = _nb(sparse, L).transpose(_ix(L), L.R)
    for dtype in DTYPES:
        for D in (3, 8):
            out = torch.full((L.R, D), extent_fence.POISON["out"][torch.float32 if dtype == torch.float32 else torch.float16],
                             dtype=torch.int32 if dtype == torch.float32 else torch.int16, device="cuda").view(dtype)
            got = ops.knn_interpolate_backward(_dev(gc.grads(L.indices.shape[0], D)), t.offsets, t.slots, t.weights, 3, dtype, buffers={"out": out})
            assert got is out and (_bits(out[120:]) == 0).all() and bool(torch.isfinite(out.float()).all())


def test_folded_index_names_rows_many_times(env):
    ops, sparse = env
    _assert_rule(ops, sparse, gc.folded(), 3, what="folded")
    _assert_rule(ops, sparse, gc.folded(), 512, mode="inverse_distance", eps=0.0, what="folded D=512")


@pytest.mark.parametrize("mode", ["inverse_distance", "nearest"])
def test_excused_rows_contribute_nothing_and_are_counted(env, mode):
    ops, sparse = env
    L = gc.planted()
    _assert_rule(ops, sparse, L, 3, mode=mode, what=f"planted {mode}")
    v = torch.from_numpy(kc.interp_values(L.R, 3))
    _, _, bl, bi = kc.interpolate_reference(v.double().numpy(), L.indices, L.d2, L.N, L.index, mode)
    status = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    out, d = _backward(sparse, L, v.cuda(), _dev(gc.grads(L.indices.shape[0], 3)), mode, status=status)
    assert status.tolist() == [bl, bi] and bl >= 1 and bi >= 1
    _, _, excused, _ = gc.references(L, mode)
    assert (out[_dev(excused)] == 0).all()
    clean = gc.Lists("clean", np.where(excused[:, None], -1, L.indices), L.d2.copy(), np.clip(L.index, 0, L.R - 1), L.N, L.R)
    _, d_clean = _backward(sparse, clean, v.cuda(), _dev(gc.grads(L.indices.shape[0], 3)), mode)
    assert _same_bits(d, d_clean)                                             # as if the excused rows had empty lists


def test_more_rows_than_the_backward_has_waves(env):
    ops, sparse = env
    frac = _assert_rule(ops, sparse, gc.big(), gc.BIG_D, what="big")
    assert frac <= 1.0


# ------------------------------------------------------------------------------------------ the transpose
@pytest.mark.parametrize("case,mode", [("grid", "inverse_distance"), ("grid", "nearest"), ("hub", "inverse_distance"), ("planted", "inverse_distance")])
def test_transpose_invariants(env, case, mode):
    ops, sparse = env
    L = {"grid": gc.grid_lists(32, True), "hub": gc.hub(), "planted": gc.planted()}[case]
    M, k = L.indices.shape
    nb = _nb(sparse, L)
    t = nb.transpose(_ix(L), L.R, mode=mode)
    assert (t.M, t.k, t.R, t.mode, t.eps) == (M, k, L.R, mode, 1e-8)
    off, slots, w = t.offsets.cpu().numpy(), t.slots.cpu().numpy(), t.weights.cpu().numpy()
    ref, rows, _, _ = gc.references(L, mode)
    flat = np.nonzero(ref.reshape(-1))[0]
    assert off.shape == (L.R + 1,) and off[0] == 0 and (np.diff(off) >= 0).all() and off[L.R] == flat.size
    assert np.array_equal(np.diff(off), np.bincount(rows[ref], minlength=L.R))
    assert np.array_equal(np.sort(slots[:flat.size]), flat) and np.array_equal(np.sort(slots), np.arange(M * k))   # each exactly once
    inside = np.ones(flat.size, bool)
    inside[off[1:L.R][off[1:L.R] < flat.size]] = False                        # positions that start a row
    assert (np.diff(slots[:flat.size])[inside[1:]] > 0).all()                 # ascending f inside every row
    assert np.array_equal(rows.reshape(-1)[slots[:flat.size]], np.repeat(np.arange(L.R), np.diff(off)))
    w32 = _weights(ops, L, mode, 1e-8).reshape(-1)
    assert np.array_equal(w[:flat.size].view(np.int32), w32[slots[:flat.size]].view(np.int32)) and (w[flat.size:] == 0).all()
    v, g = torch.from_numpy(kc.interp_values(L.R, 8)).cuda(), _dev(gc.grads(M, 8))
    _, without = _backward(sparse, L, v, g, mode)
    _, given = _backward(sparse, L, v, g, mode, transpose=t)
    assert _same_bits(given, without)


def test_a_mismatched_transpose_is_refused(env):
    ops, sparse = env
    L = gc.grid_lists(3, True)
    nb, v = _nb(sparse, L), torch.from_numpy(kc.interp_values(L.R, 4)).cuda().requires_grad_()
    t = nb.transpose(_ix(L), L.R, eps=0.5)
    for kw in (dict(), dict(mode="nearest", eps=0.5)):
        with pytest.raises(ValueError, match="interpolate: transpose was built for"):
            sparse.interpolate(v, nb, index=_ix(L), differentiable=True, transpose=t, **kw)
    other = _nb(sparse, gc.grid_lists(1, True)).transpose(_ix(L), L.R, eps=0.5)
    with pytest.raises(ValueError, match="interpolate: transpose was built for"):
        sparse.interpolate(v, nb, index=_ix(L), differentiable=True, transpose=other, eps=0.5)
    assert sparse.interpolate(v, nb, index=_ix(L), differentiable=True, transpose=t, eps=0.5).grad_fn is not None


# ------------------------------------------------------------------------------------------ reproducibility
def test_two_backward_calls_give_the_same_bits(env):
    ops, sparse = env
    for L, D in ((gc.hub(), 70), (gc.folded(), 512)):
        v, g = torch.from_numpy(kc.interp_values(L.R, D)).cuda(), _dev(gc.grads(L.indices.shape[0], D))
        _, a = _backward(sparse, L, v, g)
        _, b = _backward(sparse, L, v, g)
        assert _same_bits(a, b)


def test_permuting_the_rows_of_values_permutes_the_gradient(env):
    ops, sparse = env
    L = gc.grid_lists(3, True)
    perm = np.random.default_rng(41).permutation(L.R)
    inv = np.argsort(perm)                                                    # values2 = values[perm]: row r moves to inv[r]
    L2 = gc.Lists("permuted", L.indices.copy(), L.d2.copy(), inv[L.index], L.N, L.R)
    v, g = torch.from_numpy(kc.interp_values(L.R, 70)).cuda(), _dev(gc.grads(L.indices.shape[0], 70))
    out, d = _backward(sparse, L, v, g)
    out2, d2 = _backward(sparse, L2, v[_dev(perm)], g)
    assert _same_bits(out2, out) and _same_bits(d2, d[_dev(perm)])


# ------------------------------------------------------------------------------------------ composition
def _cloud(rng, n, batch):
    return np.concatenate([np.full((n, 1), float(batch)), rng.random((n, 3)) * 6.0], 1)


def test_composition_with_quantize_reaches_the_point_features(env):
    """leaf point features -> quantize(average) -> interpolate(index=q.inverse_mapping, differentiable=True) -> a fixed linear functional:
    d leaf[i] = d voxel[inverse[i]] / counts[inverse[i]].  The bound: the interpolation's on the voxel rows, divided by the counts, plus
    one rounding of that division (2^-23 |ref| covers its 2^-24 relative on a value within the bound of ref)."""
    ops, sparse = env
    rng = np.random.default_rng(42)
    pts = np.concatenate([_cloud(rng, 700, 0), _cloud(rng, 500, 1)], 0)
    pts = pts[rng.permutation(len(pts))]
    verts = np.concatenate([_cloud(rng, 400, 0), _cloud(rng, 300, 1)], 0)
    D = 6
    leaf = torch.from_numpy(kc.interp_values(len(pts), D)).cuda().requires_grad_()
    q = sparse.quantize(_dev(pts), leaf, mode="average")
    nv = q.features.shape[0]
    assert nv < len(pts) and int(q.counts.max()) >= 2                         # voxels shared by several points
    nb = sparse.knn_query(_dev(pts), _dev(verts), 3)
    feat = sparse.interpolate(q.features, nb, index=q.inverse_mapping, differentiable=True)
    C = gc.grads(len(verts), D, seed=43)
    (feat * _dev(C)).sum().backward()
    inverse, counts = q.inverse_mapping.cpu().numpy(), q.counts.cpu().numpy()
    L = gc.Lists("composition", nb.indices.cpu().numpy(), nb.distances2.cpu().numpy(), inverse.copy(), len(pts), nv)
    ref, scale, count = gc.fp64_reference(C, L)
    ref_leaf = ref[inverse] / counts[inverse, None]
    bound = gc.grad_bound(count, scale)[inverse] / counts[inverse, None] + 2.0 ** -23 * np.abs(ref_leaf)
    err = np.abs(leaf.grad.cpu().double().numpy() - ref_leaf)
    print(f"composition: max err {err.max():.3e}, worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all() and np.abs(ref_leaf).max() > 0
    values64 = torch.from_numpy(leaf.detach().cpu().double().numpy()).requires_grad_()        # the torch composite, fp64, on the CPU
    vox = torch.zeros((nv, D), dtype=torch.float64).index_add_(0, torch.from_numpy(inverse), values64) / torch.from_numpy(counts)[:, None]
    refs, rows, _, _ = gc.references(L)
    dense = (vox[torch.from_numpy(inverse)[torch.from_numpy(np.where(refs, L.indices, 0))]] * torch.from_numpy(gc.weights64(L))[..., None]).sum(1)
    (dense * torch.from_numpy(C.astype(np.float64))).sum().backward()
    assert np.abs(values64.grad.numpy() - ref_leaf).max() <= 1e-12 * np.abs(ref_leaf).max()
    assert np.abs(feat.detach().cpu().double().numpy() - dense.detach().numpy()).max() <= 5 * 2.0 ** -23 * float(leaf.detach().abs().max())


def test_chain_through_purify_reaches_the_student(env):
    """quantize -> student -> purify(differentiable=True) -> interpolate(differentiable=True) onto other vertices -> a fixed linear
    functional: every parameter of the student gets a finite gradient that is not all zero, the same bits in a second run"""
    ops, sparse = env
    import knn_batched_cases as kb
    from geopurify_amd import pipeline as pl
    from geopurify_amd.affinity_module import AffinityPredictor
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import MinkowskiEngine as ME
    finally:
        sys.path.pop(0)
    D = 64
    m = AffinityPredictor(D + 6, 128, 128)
    m.load_state_dict(pl.random_student_state_dict(D + 6, hidden=128, embed=128, num_blocks=4, seed=6))
    m = m.cuda().train()
    rng = np.random.default_rng(8)
    vox = kb.batched({0: kb.surface_exact(rng, 300, 24), 1: kb.surface_exact(rng, 420, 28)}, rng)
    pts = np.vstack([vox, vox[rng.integers(0, len(vox), 500)]])
    pts = pts[rng.permutation(len(pts))]
    feats = (torch.randn(len(pts), D + 6, generator=torch.Generator().manual_seed(3)) * 0.3).cuda()
    verts = pts[rng.integers(0, len(pts), 600)].astype(np.float64)
    verts[:, 1:] += rng.random((600, 3)) - 0.5
    q = sparse.quantize(_dev(pts), feats)
    x = ME.SparseTensor(features=q.features, coordinates=q.coordinates)
    nb = sparse.knn_query(_dev(pts.astype(np.float64)), _dev(verts), 3)
    t = nb.transpose(q.inverse_mapping, q.features.shape[0])
    C = _dev(gc.grads(600, D, seed=44))
    runs = []
    for transpose in (None, t):
        m.zero_grad(set_to_none=True)
        y = sparse.purify(m, x, feature_dim=D, differentiable=True, K=24, num_iters=3)
        feat = sparse.interpolate(y.F, nb, index=q.inverse_mapping, differentiable=True, transpose=transpose)
        assert feat.shape == (600, D) and feat.grad_fn is not None
        (feat * C).sum().backward()
        runs.append({n: p.grad.clone() for n, p in m.named_parameters()})
    assert len(runs[0]) > 10
    for n, g in runs[0].items():
        assert bool(torch.isfinite(g).all()) and bool((g != 0).any()), n
        assert torch.equal(g.view(torch.int32), runs[1][n].view(torch.int32)), n


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(env):
    ops, sparse = env
    L = gc.grid_lists(3, True)
    nb = _nb(sparse, L)
    with pytest.raises(ValueError, match="interpolate: differentiable=True takes floating values"):
        sparse.interpolate(torch.zeros(L.R, dtype=torch.int64, device="cuda"), nb, index=_ix(L), differentiable=True)
    huge = sparse.Neighbors(torch.zeros((2 ** 26, 32), dtype=torch.int64, device="meta"), torch.zeros((2 ** 26, 32), dtype=torch.float64, device="meta"))
    with pytest.raises(ValueError, match=r"interpolate: M \* k = 2147483648 flat slots"):
        sparse.interpolate(torch.zeros((4, 4), device="cuda", requires_grad=True), huge, differentiable=True)
    with pytest.raises(ValueError, match=r"knn_interpolate_weights: m \* k = 2147483648 flat slots"):
        ops.knn_interpolate_weights(_FakeLists(2 ** 26, 32), None, None, 4)
    t = nb.transpose(_ix(L), L.R)
    g = torch.zeros((L.indices.shape[0], 4), device="cuda")
    for bad, words in ((dict(g=g.double()), "g must be CUDA fp32"), (dict(k=33), "k=33"), (dict(dtype=torch.float64), "dtype must be one of"),
                       (dict(slots=t.slots[:-1]), "expected offsets"), (dict(offsets=t.offsets.int()), "offsets")):
        kw = dict(g=g, offsets=t.offsets, slots=t.slots, sorted_weights=t.weights, k=3, dtype=torch.float32)
        kw.update(bad)
        with pytest.raises(ValueError, match=words):
            ops.knn_interpolate_backward(**kw)
    with pytest.raises(ValueError, match="knn_interpolate_transpose: expected weights"):
        ops.knn_interpolate_transpose(_dev(L.indices), torch.zeros((3, 3), device="cuda"), _ix(L), L.R)
    from geopurify_amd import _lib
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.GeoPurifyHipError, match="workspace too small"):
        ops.knn_interpolate_transpose(_dev(L.indices), torch.zeros(L.indices.shape, device="cuda"), _ix(L), L.R, workspace=ws)


class _FakeLists:
    """the shape, dtype and flags of an i64 CUDA tensor [m, k] without its memory: what the ops wrapper checks before the library call"""
    dtype, is_cuda = torch.int64, True

    def __init__(self, m, k):
        self.shape = (m, k)

    def is_contiguous(self):
        return True

    def dim(self):
        return 2


# ------------------------------------------------------------------------------------------ extents
@pytest.mark.parametrize("mode", ["inverse_distance", "nearest"])
def test_weights_and_transpose_stay_inside_their_extents(env, mode):
    ops, sparse = env
    L = gc.planted()
    M, k = L.indices.shape

    def case(a):
        I = a.inp(torch.from_numpy(L.indices.copy()), name="indices")
        Dd = a.inp(torch.from_numpy(L.d2.copy()).view(torch.int64), name="dist2").view(torch.float64)
        X = a.inp(torch.from_numpy(L.index.copy()), name="index")
        w = ops.knn_interpolate_weights(I, Dd, X, L.R, mode, buffers={"weights": a.out((M, k), torch.float32, name="weights")})
        buffers = {"offsets": a.out(L.R + 1, torch.int64, name="offsets"), "slots": a.out(M * k, torch.int32, name="slots"),
                   "sorted_weights": a.out(M * k, torch.float32, name="sorted_weights")}
        ws = a.out(ops.knn_interpolate_transpose_workspace_bytes(M, k, L.R), torch.uint8, name="workspace")
        off, slots, sw = ops.knn_interpolate_transpose(I, w, X, L.R, mode, buffers=buffers, workspace=ws)
        return {"weights": w, "offsets": off, "slots": slots, "sorted_weights": sw}

    got = extent_fence.run(case)
    assert all(extent_fence.unwritten(got[n]) == 0 for n in got)
    assert int(got["offsets"][L.R]) == int(gc.references(L, mode)[0].sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("D", [1, 3, 70, 72, 512])
def test_backward_stays_inside_its_extents(env, D, dtype):
    ops, sparse = env
    L = gc.grid_lists(3, True)
    M = L.indices.shape[0]
    t = _nb(sparse, L).transpose(_ix(L), L.R)
    off, slots, sw = t.offsets.cpu(), t.slots.cpu(), t.weights.cpu()
    g = torch.from_numpy(gc.grads(M, D))
    pitch = (D + 4 + 3) // 4 * 4                                              # pitched g: the next multiple of 16 bytes past D

    def case(a):
        G = a.inp(g, pitch=pitch, name="g")
        # (extent_fence has no bfloat16 entry: its bits travel as the int16 it poisons fp16 through)
        out = a.out(L.R * D, torch.float16 if dtype == torch.bfloat16 else dtype, name="out").view(dtype).view(L.R, D)
        got = ops.knn_interpolate_backward(G, a.inp(off, name="offsets"), a.inp(slots, name="slots"), a.inp(sw, name="sorted_weights"), 3, dtype,
                                           buffers={"out": out})
        return {"out": got.view(torch.float16) if dtype == torch.bfloat16 else got}

    got = extent_fence.run(case)
    assert extent_fence.unwritten(got["out"]) == 0
