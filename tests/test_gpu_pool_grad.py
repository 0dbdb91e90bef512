"""The backward of the purifying step on the GPU: the five kernels alone (ops.pool_transpose_build, pool_ell_transpose, pool_ell_wgrad,
affinity_softmax_backward, l2norm_rows_backward), sparse.affinity_pool(..., differentiable=True) end to end, and the chain
quantize -> student -> purify(differentiable=True) -> per-point rows.

Cases and references: tests/pool_grad_cases.py (torch autograd in fp64 on the oracle's lists; test_pool_grad_cases_host.py proves the
closed form the kernels implement against it on the host).

Bounds.  Kernels alone, against fp64 on the same fp32 inputs:
  * index arrays: exact;
  * the two sum kernels: |err| <= 2 (n + 2) 2^-24 sum |a_i b_i| per element -- n sequential (or tree) fp32 multiply-adds with unit
    roundoff 2^-24 have the a-priori bound gamma_n sum |a_i b_i|, gamma_n < (n + 2) 2^-24 here; the factor 2 covers the final
    accumulate of pool_ell_wgrad and the wave reduction's different order.  n = the list length (transpose), D (weight gradient);
  * affinity_softmax_backward: da = s w (dw - S), S = sum_k w_k dw_k carries (K + 2) u sum |w dw|, the three further operations 3 u
    each: |err da| <= s w (K + 6) u (|dw| + sum |w dw|) + 3 u |da|; the row is a sum of n = K + in-degree products da e:
    |err| <= sum |err da| |e| + 2 (n + 2) u sum |da e|, u = 2^-24;
  * l2norm_rows_backward: (du - v <v, du>) / |e| with v = e / |e|: |err| <= 2 (d + 8) u (|du_c| + |v_c| sum |v du|) / |e|.
End to end: the forward within the 1e-4 the project holds for pooled features (test_gpu_sparse_pool.py); the gradients as
max |g - ref| / max |ref| per tensor and case, bound GRAD_TOL below: twice the worst ratio measured on an MI355X (DESIGN.md 5.7
lists them per case), which is inside the 5e-3 of a tensor's maximum that test_gpu_training.py holds for the student's gradients.
The fp16 features' gradient comes back rounded to fp16: GRAD_TOL + 2^-11 (round to nearest, relative to the element, hence to the
maximum).
"""
import os
import sys

import numpy as np
import pytest
import torch

import extent_fence
import knn_batched_cases as kc
import pool_grad_cases as gc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
Y_TOL = 1e-4
GRAD_CEILING = 5e-3                       # test_gpu_training.py's bound for the student's gradients: GRAD_TOL must not exceed it
GRAD_TOL = 1.6e-6                         # twice the worst measured ratio, 7.75e-7 (iters_D512_T19, the embeddings' gradient)
HALF_ROUNDING = 2.0 ** -11                # an fp16 gradient is the fp32 one rounded to nearest: half an ulp of 2^-10, relative
assert GRAD_TOL + HALF_ROUNDING <= GRAD_CEILING

KERNEL_CASES = ["star", "widths_D4_d16", "widths_D10_d128", "widths_D256_d16", "widths_D260_d128", "widths_D512_d16",
                "k_edges_K1", "k_edges_K8", "k_edges_K9", "k_edges_K127", "iters_D64_T1"]
END_TO_END = [n for n in gc.CASES if n not in ("flags_plain",)]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import _lib, ops, sparse
    _lib.load()
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import MinkowskiEngine as ME
    finally:
        sys.path.pop(0)
    return ops, sparse, ME


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _pad4(a):
    """columns padded with zeros to a multiple of 4 (what affinity_pool does before the kernels)"""
    d = a.shape[1]
    return np.ascontiguousarray(np.pad(a, ((0, 0), (0, (-d) % 4))))


class _Arrays:
    """a case's arrays as the kernels take them: lists of input rows, fp32 weights / rows / upstream gradients, and fp64 copies of the
    SAME fp32 values for the references"""

    def __init__(self, name):
        c = gc.case(name)
        self.c, self.n, self.K = c, c.N, c.K
        self.nbr = gc.lists(name).astype(np.int32)
        self.w = gc.reference(name)["w"].astype(np.float32)
        self.g = _pad4(np.asarray(c.R, dtype=np.float32))
        self.x = _pad4(c.X)
        self.Dp = self.g.shape[1]
        norm = np.linalg.norm(c.E.astype(np.float64), axis=1, keepdims=True)
        self.e_unit = (c.E / np.maximum(norm, 1e-12)).astype(np.float32)
        self.tr_off, self.tr_slot = gc.inverted_index(self.nbr, self.n)
        self.dest = np.repeat(np.arange(self.n), np.diff(self.tr_off))
        self.src = self.tr_slot // self.K

    def transposed(self, values):
        """fp64 [n,n] with [m, i] = values[i, j] where nbr[i,j] = m"""
        M = np.zeros((self.n, self.n))
        M[self.dest, self.src] = np.asarray(values, dtype=np.float64).reshape(-1)[self.tr_slot]
        return M


_ARRAYS = {}


def _arrays(name):
    if name not in _ARRAYS:
        _ARRAYS[name] = _Arrays(name)
    return _ARRAYS[name]


def _within(what, got, ref, bound):
    got = got.detach().double().cpu().numpy()
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max |err| = {err.max():.3e}, worst |err| / bound = {worst:.3f}")
    assert (err <= bound).all(), f"{what}: |err| / bound up to {worst:.3f}"


# ------------------------------------------------------------------------------------------ kernels alone
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_transpose_build_equals_the_model(env, name):
    ops, sparse, ME = env
    from geopurify_amd import _lib
    a = _arrays(name)
    nbytes = _lib.load().gp_pool_transpose_workspace_bytes(a.n, a.K)
    assert nbytes > 0

    def call(ar):
        off, slot = ops.pool_transpose_build(ar.inp(_dev(a.nbr), name="nbr"), tr_off=ar.out(a.n + 1, torch.int64, name="tr_off"),
                                             tr_slot=ar.out(a.n * a.K, torch.int32, name="tr_slot"),
                                             workspace=ar.out(nbytes, torch.uint8, name="workspace"))
        return {"tr_off": off, "tr_slot": slot}

    out = extent_fence.run(call)
    assert np.array_equal(out["tr_off"].cpu().numpy(), a.tr_off)
    assert np.array_equal(out["tr_slot"].cpu().numpy(), a.tr_slot)
    off, slot = ops.pool_transpose_build(_dev(a.nbr))                                # (buffers of its own)
    assert torch.equal(off, out["tr_off"]) and torch.equal(slot, out["tr_slot"])


def test_transpose_build_puts_foreign_ids_behind_the_lists(env):
    ops, sparse, ME = env
    nbr = np.array([[1, -1], [0, 7], [0, 1]], np.int32)
    off, slot = ops.pool_transpose_build(_dev(nbr))
    assert off.tolist() == [0, 2, 4, 4] and slot.tolist() == [2, 4, 0, 5, 1, 3]


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_pool_ell_transpose(env, name):
    ops, sparse, ME = env
    a = _arrays(name)
    d = a.Dp

    def call(ar):
        out = ops.pool_ell_transpose(ar.inp(_dev(a.g), pitch=d + 4, name="g"), ar.inp(_dev(a.tr_off), name="tr_off"),
                                     ar.inp(_dev(a.tr_slot), name="tr_slot"), ar.inp(_dev(a.w), name="w"), a.K,
                                     ar.out((a.n, d), torch.float32, pitch=d + 8, name="out"))
        return {"out": out}

    out = extent_fence.run(call)["out"]
    assert extent_fence.unwritten(out) == 0
    PT = a.transposed(a.w)
    ref = PT @ a.g.astype(np.float64)
    length = np.diff(a.tr_off)[:, None]
    _within(f"{name} transpose", out, ref, 2 * (length + 2) * U * (np.abs(PT) @ np.abs(a.g.astype(np.float64))))
    empty = np.flatnonzero(np.diff(a.tr_off) == 0)
    if name == "star":
        assert len(empty) == 6
    if len(empty):
        rows = out[torch.from_numpy(empty).cuda()]
        assert bool((rows.view(torch.int32) == 0).all())                             # exactly +0.0


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_pool_ell_wgrad(env, name):
    ops, sparse, ME = env
    a = _arrays(name)
    d = a.Dp

    def call(ar):
        g, x = ar.inp(_dev(a.g), pitch=d + 4, name="g"), ar.inp(_dev(a.x), pitch=d + 8, name="x_prev")
        nbr = ar.inp(_dev(a.nbr), name="nbr")
        dw = ops.pool_ell_wgrad(g, x, nbr, ar.out((a.n, a.K), torch.float32, name="dw"), accumulate=False)   # (overwrites the poison)
        twice = ar.out((a.n, a.K), torch.float32, name="twice")
        ops.pool_ell_wgrad(g, x, nbr, twice, accumulate=False)
        ops.pool_ell_wgrad(g, x, nbr, twice, accumulate=True)
        return {"dw": dw, "twice": twice}

    out = extent_fence.run(call)
    assert extent_fence.unwritten(out["dw"]) == 0
    g64, x64 = a.g.astype(np.float64), a.x.astype(np.float64)
    ref = np.take_along_axis(g64 @ x64.T, a.nbr.astype(np.int64), 1)
    mag = np.take_along_axis(np.abs(g64) @ np.abs(x64).T, a.nbr.astype(np.int64), 1)
    _within(f"{name} wgrad", out["dw"], ref, 2 * (d + 2) * U * mag)
    assert torch.equal(out["twice"], out["dw"] + out["dw"])                          # accumulate adds the same bits once more


@pytest.mark.parametrize("d", [772, 1028])
def test_sum_kernels_on_wide_rows(env, d):
    """772 columns: four slabs, the last with one active lane (g in registers); 1028: five slabs, the form that re-reads g"""
    ops, sparse, ME = env
    a = _arrays("widths_D4_d16")
    rng = np.random.default_rng(d)
    g, x = rng.standard_normal((a.n, d)).astype(np.float32), rng.standard_normal((a.n, d)).astype(np.float32)

    def call(ar):
        gd, xd = ar.inp(_dev(g), pitch=d + 4, name="g"), ar.inp(_dev(x), pitch=d + 8, name="x_prev")
        dw = ops.pool_ell_wgrad(gd, xd, ar.inp(_dev(a.nbr), name="nbr"), ar.out((a.n, a.K), torch.float32, name="dw"), accumulate=False)
        out = ops.pool_ell_transpose(gd, ar.inp(_dev(a.tr_off), name="tr_off"), ar.inp(_dev(a.tr_slot), name="tr_slot"),
                                     ar.inp(_dev(a.w), name="w"), a.K, ar.out((a.n, d), torch.float32, pitch=d + 8, name="out"))
        return {"dw": dw, "out": out}

    out = extent_fence.run(call)
    assert extent_fence.unwritten(out["dw"]) == 0 and extent_fence.unwritten(out["out"]) == 0
    g64, x64, nb = g.astype(np.float64), x.astype(np.float64), a.nbr.astype(np.int64)
    _within(f"D={d} wgrad", out["dw"], np.take_along_axis(g64 @ x64.T, nb, 1),
            2 * (d + 2) * U * np.take_along_axis(np.abs(g64) @ np.abs(x64).T, nb, 1))
    PT = a.transposed(a.w)
    _within(f"D={d} transpose", out["out"], PT @ g64, 2 * (np.diff(a.tr_off)[:, None] + 2) * U * (np.abs(PT) @ np.abs(g64)))


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_affinity_softmax_backward(env, name):
    ops, sparse, ME = env
    from geopurify_amd import _lib
    a = _arrays(name)
    d = a.e_unit.shape[1]
    s = a.c.sharpen
    dw = np.random.default_rng(11).standard_normal((a.n, a.K)).astype(np.float32)
    nbytes = _lib.load().gp_affinity_softmax_backward_workspace_bytes(a.n, a.K)
    assert nbytes >= a.n * a.K * 4

    def call(ar):
        out = ops.affinity_softmax_backward(ar.inp(_dev(a.e_unit), pitch=d + 4, name="e_unit"), ar.inp(_dev(a.nbr), name="nbr"),
                                            ar.inp(_dev(a.w), name="w"), ar.inp(_dev(dw), name="dw"), s,
                                            ar.inp(_dev(a.tr_off), name="tr_off"), ar.inp(_dev(a.tr_slot), name="tr_slot"),
                                            out=ar.out((a.n, d), torch.float32, pitch=d + 8, name="de_unit"),
                                            workspace=ar.out(nbytes, torch.uint8, name="workspace"))
        return {"de": out}

    out = extent_fence.run(call)["de"]
    assert extent_fence.unwritten(out) == 0
    w, g, e = a.w.astype(np.float64), dw.astype(np.float64), a.e_unit.astype(np.float64)
    nb = a.nbr.astype(np.int64)
    da = s * w * (g - (w * g).sum(1, keepdims=True))
    err_da = s * w * (a.K + 6) * U * (np.abs(g) + np.abs(w * g).sum(1, keepdims=True)) + 3 * U * np.abs(da)
    ref = np.einsum("ij,ijc->ic", da, e[nb]) + a.transposed(da) @ e
    terms = (a.K + np.diff(a.tr_off))[:, None]
    ae = np.abs(e)
    bound = (np.einsum("ij,ijc->ic", err_da, ae[nb]) + a.transposed(err_da) @ ae
             + 2 * (terms + 2) * U * (np.einsum("ij,ijc->ic", np.abs(da), ae[nb]) + a.transposed(np.abs(da)) @ ae))
    _within(f"{name} softmax backward", out, ref, bound)


@pytest.mark.parametrize("name", ["star", "widths_D4_d128", "k_edges_K9"])
def test_l2norm_rows_backward(env, name):
    ops, sparse, ME = env
    c = gc.case(name)
    e = np.array(c.E)
    e[3] = 0.0                                                                       # below the clamp: du / 1e-12, no projection
    e[5] *= 1e-20
    d = e.shape[1]
    du = np.random.default_rng(12).standard_normal(e.shape).astype(np.float32)

    def call(ar):
        out = ops.l2norm_rows_backward(ar.inp(_dev(e), pitch=d + 4, name="e_raw"), ar.inp(_dev(du), pitch=d + 8, name="de_unit"),
                                       out=ar.out(e.shape, torch.float32, pitch=d + 4, name="de_raw"))
        return {"de": out}

    out = extent_fence.run(call)["de"]
    assert extent_fence.unwritten(out) == 0
    e64, du64 = e.astype(np.float64), du.astype(np.float64)
    norm = np.linalg.norm(e64, axis=1, keepdims=True)
    small = norm[:, 0] < 1e-12
    assert small.sum() == 2
    v = e64 / np.maximum(norm, 1e-300)
    ref = np.where(small[:, None], du64 / 1e-12, (du64 - v * (v * du64).sum(1, keepdims=True)) / np.maximum(norm, 1e-300))
    bound = 2 * (d + 8) * U * (np.abs(du64) + np.abs(v) * np.abs(v * du64).sum(1, keepdims=True)) / np.maximum(norm, 1e-12)
    bound[small] = 4 * U * np.abs(ref[small])                                        # (the fp32 constant 1e-12f and one division)
    _within(f"{name} l2norm backward", out, ref, bound)
    e_t = torch.from_numpy(e).cuda().requires_grad_()                                # ... and F.normalize's own autograd agrees
    torch.nn.functional.normalize(e_t, dim=1, eps=1e-12).backward(_dev(du))
    _within(f"{name} l2norm backward against F.normalize", e_t.grad, ref, bound + 4 * U * np.abs(ref))


def test_kernels_refuse_bad_arguments(env):
    """a pitch that is no multiple of 4, k = 0, k = 129, an output that aliases an input: refused before any launch"""
    ops, sparse, ME = env
    from geopurify_amd._lib import GeoPurifyHipError
    a = _arrays("star")
    d, n, K = a.Dp, a.n, a.K
    g, x, w, nbr = _dev(a.g), _dev(a.x), _dev(a.w), _dev(a.nbr)
    off, slot = _dev(a.tr_off), _dev(a.tr_slot)
    out = torch.empty_like(g)
    e = _dev(a.e_unit)
    odd = torch.zeros((n, d + 2), device="cuda")[:, :d]                              # row stride d + 2 floats
    with pytest.raises(GeoPurifyHipError, match="pitches must be multiples of 4"):
        ops.pool_ell_transpose(odd, off, slot, w, K, out)
    with pytest.raises(GeoPurifyHipError, match="pitches must be multiples of 4"):
        ops.pool_ell_transpose(g, off, slot, w, K, odd)
    with pytest.raises(GeoPurifyHipError, match="pitches must be multiples of 4"):
        ops.pool_ell_wgrad(g, odd, nbr, torch.empty_like(w), False)
    with pytest.raises(GeoPurifyHipError, match="pitches must be multiples of 4"):
        ops.l2norm_rows_backward(e, torch.zeros((n, e.shape[1] + 2), device="cuda")[:, :e.shape[1]])
    with pytest.raises(GeoPurifyHipError, match="pitches must be multiples of 4"):
        ops.affinity_softmax_backward(e, nbr, w, w.clone(), 20.0, off, slot, out=torch.zeros((n, e.shape[1] + 2), device="cuda")[:, :e.shape[1]])
    for k in (0, 129):
        with pytest.raises(GeoPurifyHipError, match=f"k={k} not in 1..128"):
            ops.pool_ell_transpose(g, off, slot, w, k, out)
        wide = torch.zeros((n, k), dtype=torch.int32, device="cuda")
        with pytest.raises(GeoPurifyHipError, match=f"k={k} not in 1..128"):
            ops.pool_transpose_build(wide)
        with pytest.raises(GeoPurifyHipError, match=f"k={k} not in 1..128"):
            ops.pool_ell_wgrad(g, x, wide, torch.zeros((n, k), device="cuda"), False)
        with pytest.raises(GeoPurifyHipError, match=f"k={k} not in 1..128"):
            ops.affinity_softmax_backward(e, wide, torch.zeros((n, k), device="cuda"), torch.zeros((n, k), device="cuda"), 20.0, off,
                                          torch.zeros(n * k, dtype=torch.int32, device="cuda"))
    with pytest.raises(GeoPurifyHipError, match="must not alias"):
        ops.pool_ell_transpose(g, off, slot, w, K, g)
    with pytest.raises(GeoPurifyHipError, match="must not alias"):
        ops.pool_ell_wgrad(g, x, nbr, g.view(-1)[:n * K].view(n, K), False)
    with pytest.raises(GeoPurifyHipError, match="must not alias"):
        ops.affinity_softmax_backward(e, nbr, w, w.clone(), 20.0, off, slot, out=e)
    with pytest.raises(GeoPurifyHipError, match="must not alias"):
        ops.l2norm_rows_backward(e, e.clone(), out=e)
    from geopurify_amd import _lib
    lib = _lib.load()
    assert lib.gp_pool_transpose_workspace_bytes(n, 0) == 0 and lib.gp_pool_transpose_workspace_bytes(n, 129) == 0
    assert lib.gp_affinity_softmax_backward_workspace_bytes(n, 0) == 0


# ------------------------------------------------------------------------------------------ end to end
def _pool(env, name, x_grad=True, e_grad=True, sparse_embeddings=False, half=False, **kw):
    """-> (c, x.F leaf, embeddings leaf, y) of sparse.affinity_pool(..., differentiable=True) on the case"""
    ops, sparse, ME = env
    c = gc.case(name)
    C = _dev(c.C)
    xf = _dev(c.X, torch.float16 if half else None).requires_grad_(x_grad)
    ef = _dev(c.E).requires_grad_(e_grad)
    x = ME.SparseTensor(features=xf, coordinates=C)
    e = ME.SparseTensor(features=ef, coordinates=C.clone()) if sparse_embeddings else ef
    y = sparse.affinity_pool(x, e, K=c.K, sharpen=c.sharpen, num_iters=c.T, normalize=c.normalize, differentiable=True, **kw)
    return c, xf, ef, y


def _ratio(what, got, ref):
    scale = float(np.abs(ref).max())
    err = float(np.abs(got.detach().double().cpu().numpy() - ref).max())
    r = err / scale if scale else err
    print(f"{what}: max |g - ref| / max |ref| = {r:.3e} (max |ref| = {scale:.3e}, bound {GRAD_TOL:g})")
    return r


@pytest.mark.parametrize("name", END_TO_END)
def test_forward_and_gradients_against_fp64(env, name):
    ops, sparse, ME = env
    c, xf, ef, y = _pool(env, name)
    ref = gc.reference(name)
    assert y.F.dtype == torch.float32 and y.F.shape == (c.N, c.D) and y.F.requires_grad
    err = float(np.abs(y.F.detach().double().cpu().numpy() - ref["Y"]).max())
    print(f"{name} forward: max |difference| = {err:.3e} (bound {Y_TOL:g})")
    assert err <= Y_TOL
    again = _pool(env, name)[3]
    assert torch.equal(y.F.detach(), again.F.detach())
    (y.F * _dev(c.R, torch.float32)).sum().backward()
    assert xf.grad.shape == xf.shape and xf.grad.dtype == torch.float32
    rx = _ratio(f"{name} d x.F", xf.grad, ref["dX"])
    if c.T == 0:
        assert ef.grad is None and torch.equal(xf.grad, _dev(c.R, torch.float32))   # the identity, and no gradient for the embeddings
        return
    assert ef.grad.shape == ef.shape and ef.grad.dtype == torch.float32
    re_ = _ratio(f"{name} d embeddings", ef.grad, ref["dE"])
    assert rx <= GRAD_TOL and re_ <= GRAD_TOL


@pytest.mark.parametrize("what", ["x_only", "e_only", "both", "sparse_embeddings", "plain_unit_rows", "fp16_features"])
def test_flags(env, what):
    name = "flags_plain" if what == "plain_unit_rows" else "flags"
    kw = {"x_only": dict(e_grad=False), "e_only": dict(x_grad=False), "sparse_embeddings": dict(sparse_embeddings=True),
          "fp16_features": dict(half=True)}.get(what, {})
    c, xf, ef, y = _pool(env, name, **kw)
    ref = gc.reference(name)
    assert y.F.requires_grad and y.F.dtype == torch.float32
    assert float(np.abs(y.F.detach().double().cpu().numpy() - ref["Y"]).max()) <= Y_TOL
    (y.F * _dev(c.R, torch.float32)).sum().backward()
    if what == "e_only":
        assert xf.grad is None
    else:
        assert xf.grad.dtype == xf.dtype                                             # fp16 features: an fp16 gradient
        assert _ratio(f"{what} d x.F", xf.grad, ref["dX"]) <= GRAD_TOL + (HALF_ROUNDING if what == "fp16_features" else 0.0)
    if what == "x_only":
        assert ef.grad is None
    else:
        assert _ratio(f"{what} d embeddings", ef.grad, ref["dE"]) <= GRAD_TOL


def test_two_backward_passes_give_the_same_bits(env):
    c, xf, ef, y = _pool(env, "iters_D64_T2")
    loss = (y.F * _dev(c.R, torch.float32)).sum()
    loss.backward(retain_graph=True)
    gx, ge = xf.grad.clone(), ef.grad.clone()
    xf.grad = ef.grad = None
    loss.backward()
    assert torch.equal(gx.view(torch.int32), xf.grad.view(torch.int32)) and torch.equal(ge.view(torch.int32), ef.grad.view(torch.int32))
    with pytest.raises(RuntimeError, match="second time"):                           # autograd's own error: the stack is freed
        loss.backward()


def test_a_loss_on_one_entry_leaves_the_other_entry_zero(env):
    c, xf, ef, y = _pool(env, "star")
    first = _dev(c.C[:, 0] == 0)
    (y.F[first] * _dev(c.R, torch.float32)[first]).sum().backward()
    other = ~first
    assert bool(other.any()) and bool((xf.grad[other] == 0).all()) and bool((ef.grad[other] == 0).all())
    assert bool((xf.grad[first] != 0).any()) and bool((ef.grad[first] != 0).any())


def test_without_gradients_it_is_the_default_call(env):
    ops, sparse, ME = env
    c = gc.case("iters_D64_T2")
    C, X, E = _dev(c.C), _dev(c.X), _dev(c.E)
    default = sparse.affinity_pool(ME.SparseTensor(features=X, coordinates=C), E, K=c.K, num_iters=c.T)
    plain = sparse.affinity_pool(ME.SparseTensor(features=X, coordinates=C), E, K=c.K, num_iters=c.T, differentiable=True)
    assert not plain.F.requires_grad and torch.equal(plain.F, default.F)
    with torch.no_grad():
        x = ME.SparseTensor(features=X.clone().requires_grad_(), coordinates=C)
        quiet = sparse.affinity_pool(x, E.clone().requires_grad_(), K=c.K, num_iters=c.T, differentiable=True)
    assert not quiet.F.requires_grad and torch.equal(quiet.F, default.F)


def test_refusals_before_any_kernel(env):
    ops, sparse, ME = env
    c = gc.case("iters_D512_T19")
    x = ME.SparseTensor(features=_dev(c.X).requires_grad_(), coordinates=_dev(c.C))
    with pytest.raises(ValueError, match=r"pool_mode='mfma_cs' with differentiable=True"):
        sparse.affinity_pool(x, _dev(c.E), differentiable=True, pool_mode="mfma_cs")
    with pytest.raises(ValueError, match=r"differentiable=True takes embeddings of width 16 / 32 / 64 / 128, got 24"):
        sparse.affinity_pool(x, _dev(c.E)[:, :24], differentiable=True)
    y = sparse.affinity_pool(x, _dev(c.E), differentiable=True, pool_mode="ell", num_iters=1)
    assert y.F.requires_grad


# ------------------------------------------------------------------------------------------ the chain
def _chain_inputs(env):
    ops, sparse, ME = env
    from geopurify_amd import pipeline as pl
    from geopurify_amd.affinity_module import AffinityPredictor
    D = 64
    m = AffinityPredictor(D + 6, 128, 128)
    m.load_state_dict(pl.random_student_state_dict(D + 6, hidden=128, embed=128, num_blocks=4, seed=6))
    m = m.cuda()
    rng = np.random.default_rng(8)
    vox = kc.batched({0: kc.surface_exact(rng, 300, 24), 1: kc.surface_exact(rng, 420, 28)}, rng)
    pts = np.vstack([vox, vox[rng.integers(0, len(vox), 500)]])                       # 500 points share a voxel with another
    pts = pts[rng.permutation(len(pts))]
    feats = (torch.randn(len(pts), D + 6, device="cuda") * 0.3).requires_grad_()
    return m, _dev(pts), feats, D


def test_chain_reaches_the_student_and_the_points(env):
    """quantize -> student -> purify(differentiable=True) -> per-point rows -> a sum loss: every parameter and the point features get
    finite gradients that are not all zero, and the parameters' equal those of the two-step route (d embeddings from a pooling call on
    a leaf, then e.F.backward(dE)) within 1e-6 of each tensor's maximum"""
    ops, sparse, ME = env
    m, pts, feats, D = _chain_inputs(env)
    m.train()
    kw = dict(K=24, num_iters=3)

    q = sparse.quantize(pts, feats)
    x = ME.SparseTensor(features=q.features, coordinates=q.coordinates)
    y = sparse.purify(m, x, feature_dim=D, differentiable=True, **kw)
    assert m.training and y.F.requires_grad and y.F.shape == (len(q.coordinates), D)
    per_point = y.F[q.inverse_mapping]
    assert per_point.shape == (len(pts), D)
    weights = torch.randn_like(per_point)
    (per_point * weights).sum().backward()
    grads = {n: p.grad.clone() for n, p in m.named_parameters()}
    assert len(grads) > 10
    for n, g in list(grads.items()) + [("point features", feats.grad)]:
        assert g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any()), n

    m.zero_grad(set_to_none=True)
    x2 = ME.SparseTensor(features=q.features.detach(), coordinates=q.coordinates)
    e = m(x2)
    leaf = e.F.detach().requires_grad_()
    y2 = sparse.affinity_pool(ME.SparseTensor(features=x2.F[:, :D], coordinates=x2.C), leaf, differentiable=True, **kw)
    (y2.F[q.inverse_mapping] * weights).sum().backward()
    e.F.backward(leaf.grad)
    for n, p in m.named_parameters():
        scale = float(grads[n].abs().max())
        err = float((p.grad - grads[n]).abs().max())
        print(f"{n}: max |difference| / max |gradient| = {err / scale:.2e}")
        assert err <= 1e-6 * scale, n


@pytest.mark.parametrize("training", [True, False])
def test_purify_differentiable_leaves_the_students_mode(env, training):
    """no forced eval(): BatchNorm runs in the mode the caller set -- batch statistics (and a running-mean update) in train mode, the
    running statistics (untouched) in eval mode -- and the flag is as it was"""
    ops, sparse, ME = env
    m, pts, feats, D = _chain_inputs(env)
    q = sparse.quantize(pts, feats.detach())
    x = ME.SparseTensor(features=q.features.requires_grad_(), coordinates=q.coordinates)
    m.train(training)
    tracked = {n: b.clone() for n, b in m.named_buffers() if n.endswith("num_batches_tracked")}
    assert tracked
    y = sparse.purify(m, x, feature_dim=D, differentiable=True, K=24, num_iters=2)
    assert m.training is training and y.F.requires_grad
    for n, b in m.named_buffers():
        if n in tracked:
            assert int(b) == int(tracked[n]) + (1 if training else 0), n
    default = sparse.purify(m, x, feature_dim=D, K=24, num_iters=2)                  # (the default: eval mode under no_grad inside)
    assert m.training is training and not default.F.requires_grad
    for n, b in m.named_buffers():
        if n in tracked:
            assert int(b) == int(tracked[n]) + (1 if training else 0), n
