"""sparse.segment_loss on the GPU: the cross-entropy of SparseTensor rows against text embeddings, forward and gradient, against the
fp64 references of tests/segment_loss_cases.py (torch autograd of the dense formulation on the same fp32 inputs), at the kernels'
edges, for determinism, for agreement with sparse.segment, inside extent fences and through the chain
quantize -> student -> purify(differentiable=True) -> segment_loss -> backward.

Bounds.  Exact: loss.valid, the NaN pattern of loss.per_entry, the +0.0 gradient rows of rows without valid items, one class.
  * the loss, against the fp64 value: every valid item contributes lse_i - z_il.  z_il is an fp32 product of s with a dot product over
    D_padded (D to a multiple of 32) unit-row and unit-text elements, |error| <= s (D_padded + 8) 2^-24 with the two normalisations
    and the scale; lse carries the same through its largest logit, and the fp32 max / exp / log / sums add a few units of 2^-24 of
    max(|lse|, |z|).  A-priori, per item and hence for their weighted mean:
        LOSS_CEILING(case) = 4 s (D_padded + 8) 2^-24 + 16 * 2^-24 * max(|lse|, |z|).
    The test's bound is LOSS_FRACTION of it: twice the worst ratio of |loss - ref| and of the per-entry means' error to LOSS_CEILING
    measured over the cases on an MI355X (DESIGN.md 5.10 lists them), which must stay below 1;
  * the gradient: max |g - ref| / max |ref| per case (the natural row size s / min |y_i| in place of max |ref| where the gradient is
    analytically zero, D = 1) <= GRAD_TOL, twice the worst measured ratio, inside the 5e-3 of a tensor's maximum that
    test_gpu_training.py holds.  One case has a bound of its own, GRAD_TOL_ONE_ROW: N1's single row is classified right with
    p = 0.99984, so its only gradient is w (p - 1), a difference of 1.6e-4 that an fp32 softmax carries to 6e-8; every other case has
    misclassified rows that set the maximum.  fp16 / bf16 features get their gradient back rounded to their dtype: + 2^-11 / 2^-8 (round to nearest,
    relative to the element, hence to the maximum);
  * per_entry: the loss's bound (an entry's mean is a loss of its own).
"""
import os
import sys

import numpy as np
import pytest
import torch

import extent_fence
import segment_cases as sc
import segment_loss_cases as lc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
GRAD_CEILING = 5e-3                       # test_gpu_training.py's bound for the student's gradients
GRAD_TOL = 1.9e-6                         # twice the worst measured ratio of every case but N1, 9.16e-7 (C4096)
GRAD_TOL_ONE_ROW = 1.2e-4                 # N1 alone, twice its 5.60e-5: one row classified right, its only gradient is w (p - 1) with p = 0.99984
LOSS_FRACTION = 9.5e-3                    # twice the worst measured error / LOSS_CEILING: 4.71e-3 (s1_collinear's per-entry means; the loss: 2.21e-3, C4096)
ROUNDING = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
assert GRAD_TOL_ONE_ROW + max(ROUNDING.values()) <= GRAD_CEILING and GRAD_TOL <= GRAD_TOL_ONE_ROW and LOSS_FRACTION <= 1.0


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


def _pad(v, m):
    return (v + m - 1) // m * m


def loss_ceiling(c, ref):
    d_pad = _pad(c.D, lc.K_PAD)
    return 4 * c.s * (d_pad + 8) * U + 16 * U * max(float(np.abs(ref.lse).max()), ref.z_max)


def _call(env, c, dtype=None, feats=None, grad=True, **kw):
    """segment_loss on a case -> (loss, the features tensor)"""
    ops, sparse, ME = env
    f = _dev(c.F, dtype) if feats is None else feats
    f = f.requires_grad_() if grad else f
    y = ME.SparseTensor(features=f, coordinates=_dev(c.coordinates()))
    loss = sparse.segment_loss(y, _dev(c.text), c.s, labels=_dev(c.labels), ignore_labels=c.ignore,
                               inverse_mapping=None if c.inv is None else _dev(c.inv), reduction=c.reduction, **kw)
    return loss, f


def _grad_ratio(c, g, ref):
    top = float(np.abs(ref.dY).max())
    scale = top if top > 1e-10 * c.grad_scale() else c.grad_scale()
    return float(np.abs(g.double().cpu().numpy() - ref.dY).max()) / scale


def _check(env, c, dtype=None, **kw):
    ref = lc.reference(c.name)
    loss, f = _call(env, c, dtype, **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    loss.backward()
    g = f.grad
    assert g.dtype == f.dtype and g.shape == f.shape
    err, ceiling = abs(float(loss.detach()) - ref.loss), loss_ceiling(c, ref)
    ratio = _grad_ratio(c, g, ref)
    pe, ok = loss.per_entry.cpu().numpy(), ref.valid > 0
    pe_err = float(np.abs(pe[ok] - ref.per_entry[ok]).max()) if ok.any() else 0.0
    print(f"{c.name}{'' if dtype is None else ' ' + str(dtype)}: loss {float(loss.detach()):.7g} |loss - ref| = {err:.3e}, {err / ceiling:.3e} of the "
          f"ceiling {ceiling:.3e}; per entry {pe_err:.3e}, {pe_err / ceiling:.3e} of it; max |g - ref| / max |ref| = {ratio:.3e}")
    assert np.isfinite(float(loss.detach())) and bool(torch.isfinite(g).all())
    assert err <= LOSS_FRACTION * ceiling
    assert ratio <= (GRAD_TOL_ONE_ROW if c.name == "N1" else GRAD_TOL) + ROUNDING.get(dtype, 0.0)
    # counts and the per-entry means
    assert loss.valid.dtype == torch.int64 and np.array_equal(loss.valid.cpu().numpy(), ref.valid)
    assert loss.per_entry.dtype == torch.float32 and not loss.per_entry.requires_grad and pe.shape == ref.per_entry.shape
    assert np.array_equal(np.isnan(pe), ref.valid == 0)
    assert pe_err <= LOSS_FRACTION * ceiling
    # rows without valid items: an exact +0.0 gradient row
    m = np.bincount(c.rows()[c.valid()], minlength=c.N)
    idle = torch.from_numpy(m == 0).cuda()
    bits = g.contiguous().view(torch.int16 if g.element_size() == 2 else torch.int32)
    assert not bool(bits[idle].any())
    return loss, g


# ------------------------------------------------------------------------------------------ against the fp64 reference
@pytest.mark.parametrize("name", lc.CASES)
def test_loss_and_gradient_match_fp64(env, name):
    """every case of segment_loss_cases: class counts 1 .. 4096 and around the row kernel's column step and the GEMM's column padding,
    widths 1 .. 1024, row counts around the GEMM's row tile, zero rows, a voxel of 1000 points, a voxel without one, labels -100 / C /
    255 / a second ignore id, an entry of invalid items only, no valid item at all, absent entries, batch index 65535, scales 1 / 14.3
    / 100 with rows collinear to a text row"""
    c = lc.case(name)
    loss, g = _check(env, c)
    if name == "C1" or name.startswith("no_valid"):
        assert float(loss.detach()) == 0.0 and not bool(g.view(torch.int32).any())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_features_get_their_gradient_in_their_dtype(env, dtype):
    """the reference takes the rounded features, so the difference is the kernels' and the gradient's rounding to the dtype"""
    _check(env, lc.case(f"points_item_{str(dtype).split('.')[-1]}"), dtype)


def test_features_with_a_row_pitch(env):
    c = lc.case("D33")
    wide = torch.zeros((c.N, c.D + 7), device="cuda")
    wide[:, 3:3 + c.D] = _dev(c.F)
    leaf = wide.requires_grad_()
    ops, sparse, ME = env
    y = ME.SparseTensor(features=leaf[:, 3:3 + c.D], coordinates=_dev(c.coordinates()))
    loss = sparse.segment_loss(y, _dev(c.text), c.s, labels=_dev(c.labels), ignore_labels=c.ignore, reduction=c.reduction)
    loss.backward()
    plain, f = _call(env, c)
    plain.backward()
    assert torch.equal(loss.detach(), plain.detach()) and torch.equal(leaf.grad[:, 3:3 + c.D], f.grad)
    assert not bool(leaf.grad[:, :3].any()) and not bool(leaf.grad[:, 3 + c.D:].any())


def test_row_scale_does_not_change_the_loss(env):
    """|y| x 1e-3 and x 1e3: the same unit rows, so the same loss within the bound"""
    ref = lc.reference("unit_scale_rows")
    ceiling = loss_ceiling(lc.case("unit_scale_rows"), ref)
    for name in ("small_rows", "large_rows"):
        loss, _ = _call(env, lc.case(name), grad=False)
        print(f"{name}: loss {float(loss):.7g}, reference of the unscaled rows {ref.loss:.7g}")
        assert abs(float(loss) - ref.loss) <= LOSS_FRACTION * ceiling


def test_tensor_logit_scale_and_no_grad(env):
    ops, sparse, ME = env
    c = lc.case("C19")
    y = ME.SparseTensor(features=_dev(c.F), coordinates=_dev(c.coordinates()))
    a = sparse.segment_loss(y, _dev(c.text), c.s, labels=_dev(c.labels))
    b = sparse.segment_loss(y, _dev(c.text), torch.tensor(c.s, device="cuda"), labels=_dev(c.labels))
    assert not a.requires_grad and abs(float(a) - float(b)) <= 4 * U * abs(float(a))
    # the forward alone stores no G: the same loss and per-entry means, bit for bit, as the call that takes the gradient
    with_grad, _ = _call(env, c)
    assert torch.equal(with_grad.detach().view(torch.int32), a.view(torch.int32))
    assert torch.equal(with_grad.per_entry.view(torch.int32), a.per_entry.view(torch.int32)) and torch.equal(with_grad.valid, a.valid)
    y64 = ME.SparseTensor(features=_dev(c.F), coordinates=_dev(c.coordinates()).long())
    assert torch.equal(sparse.segment_loss(y64, _dev(c.text), c.s, labels=_dev(c.labels).int()), a)


# ------------------------------------------------------------------------------------------ determinism and order
@pytest.mark.parametrize("name", ["points_item", "voxel_1000_points", "entry_reduction"])
def test_two_runs_are_bit_equal(env, name):
    c = lc.case(name)
    runs = []
    for _ in range(2):
        loss, f = _call(env, c)
        loss.backward()
        runs.append((loss.detach().clone(), f.grad.clone(), loss.per_entry.clone()))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    assert torch.equal(runs[0][2].view(torch.int32), runs[1][2].view(torch.int32))


@pytest.mark.parametrize("name", ["points_item", "entry_reduction"])
def test_permuting_the_rows_permutes_the_gradient(env, name):
    ops, sparse, ME = env
    c = lc.case(name)
    loss, f = _call(env, c)
    loss.backward()
    perm = np.random.default_rng(5).permutation(c.N)                          # new row j is old row perm[j]
    back = np.argsort(perm)
    f2 = _dev(c.F[perm]).requires_grad_()
    y2 = ME.SparseTensor(features=f2, coordinates=_dev(c.coordinates()[perm]))
    if c.inv is None:
        labels2, inv2 = _dev(c.labels[perm]), None
    else:
        labels2, inv2 = _dev(c.labels), _dev(back[c.inv])
    loss2 = sparse.segment_loss(y2, _dev(c.text), c.s, labels=labels2, ignore_labels=c.ignore, inverse_mapping=inv2, reduction=c.reduction)
    loss2.backward()
    assert torch.equal(f2.grad.view(torch.int32), f.grad[torch.from_numpy(perm).cuda()].view(torch.int32))
    assert torch.equal(loss2.valid, loss.valid)


@pytest.mark.parametrize("name", ["points_item", "C129", "entry_reduction"])
def test_chunking_does_not_change_the_bits(env, name):
    c = lc.case(name)
    whole, f = _call(env, c)
    whole.backward()
    c_pad = _pad(c.C, lc.COL_PAD)
    rows = (c.N + 2) // 3
    assert 2 * rows < c.N <= 3 * rows                                         # three chunks, the last one shorter
    parts, f3 = _call(env, c, logits_budget_bytes=8 * c_pad * rows)
    parts.backward()
    assert torch.equal(parts.detach().view(torch.int32), whole.detach().view(torch.int32))
    assert torch.equal(f3.grad.view(torch.int32), f.grad.view(torch.int32))
    assert torch.equal(parts.per_entry.view(torch.int32), whole.per_entry.view(torch.int32))
    one_row, f1 = _call(env, lc.case("N129"), logits_budget_bytes=1)          # a budget below one row: chunks of one row
    one_row.backward()
    ref, fr = _call(env, lc.case("N129"))
    ref.backward()
    assert torch.equal(one_row.detach(), ref.detach()) and torch.equal(f1.grad, fr.grad)


# ------------------------------------------------------------------------------------------ agreement with segment
@pytest.mark.parametrize("D,Cn", [(32, 19), (64, 200), (12, 8)])
def test_argmax_of_the_logits_is_segments_pred(env, D, Cn):
    """rows with a top-2 cosine margin of 0.1 (segment_cases' recipe): the arg-max of the loss's logits is segment's pred on the
    non-zero rows, on both of segment's classify kernels"""
    ops, sparse, ME = env
    C, zero = sc.case("overlap")
    F, cls = sc.features_of(zero, D, Cn, 900 + D)
    text = _dev(sc.text(D, Cn).astype(np.float32))
    y = ME.SparseTensor(features=_dev(F), coordinates=_dev(np.asarray(C, np.int32)))
    pred = sparse.segment(y, text, 14.3, fill=None).pred
    s = torch.full((1,), 14.3, device="cuda")
    tp = sparse._TextProducts(text, s, D)
    U_, z = ops.segment_loss_unit_rows(_dev(F), D)
    logits = tp.logits(U_, torch.empty((len(F), tp.Cp), device="cuda"))[:, :Cn]
    nz = ~z.bool()
    assert bool(nz.any()) and torch.equal(z.bool().cpu(), torch.from_numpy(np.array(zero)))
    assert torch.equal(logits.argmax(1)[nz], pred[nz])
    assert np.array_equal(pred[nz].cpu().numpy(), cls[np.asarray(~zero)])


# ------------------------------------------------------------------------------------------ extents
@pytest.mark.parametrize("name", ["points_item", "C65", "D33", "N129"])
def test_entry_points_stay_inside_their_extents(env, name):
    """the four entry points on fenced arrays: pitches ld + 4, workspaces of exactly the reported bytes; nothing outside the extents is
    written, nothing read from there reaches a result (the fenced and the plain results are the same bits)"""
    ops, sparse, ME = env
    from geopurify_amd import _lib
    lib = _lib.load()
    c = lc.case(name)
    N, D, Cn = c.N, c.D, c.C
    P = len(c.labels)
    d_pad, c_pad = _pad(D, lc.K_PAD), _pad(Cn, lc.COL_PAD)
    text = _dev(c.text)
    tp = sparse._TextProducts(text, torch.full((1,), c.s, device="cuda"), D)
    B = c.B

    def case(a):
        pitch = (lambda w: w + 4) if a.fence else (lambda w: w)
        d_in = (D + 3) // 4 * 4                                               # (a fence's pitch is a multiple of 16 bytes)
        y = a.inp(torch.from_numpy(np.pad(c.F, ((0, 0), (0, d_in - D)))), pitch=pitch(d_in), name="y")[:, :D]
        u = a.out((N, d_pad), torch.float32, pitch=pitch(d_pad), name="u")
        zero = a.out(N, torch.uint8, name="zero")
        ops.segment_loss_unit_rows(y, D, u=u, zero=zero)
        coords = a.inp(torch.from_numpy(c.coordinates()), name="coords")
        labels = a.inp(torch.from_numpy(np.array(c.labels)), name="labels")
        index = a.inp(torch.from_numpy(np.array(c.inv)), name="index") if c.inv is not None else None
        bufs = {"entry_cnt": a.out(65536, torch.int64, name="entry_cnt"), "entry_w": a.out(65536, torch.float32, name="entry_w"),
                "status": a.out(4, torch.int64, name="status")}
        ws = None
        if index is None:
            bufs["row_valid"] = a.out(N, torch.uint8, name="row_valid")
        else:
            bufs["item_off"], bufs["item_id"] = a.out(N + 1, torch.int64, name="item_off"), a.out(P, torch.int32, name="item_id")
            ws = a.out(lib.gp_segment_loss_items_workspace_bytes(N, P), torch.uint8, name="items workspace")
        it = ops.segment_loss_items(coords, zero, labels, Cn, c.ignore, c.reduction, index=index, buffers=bufs, workspace=ws)
        z = a.out((N, c_pad), torch.float32, pitch=pitch(c_pad), name="z")
        tp.logits(u, z)
        g = a.out((N, c_pad), torch.float32, pitch=pitch(c_pad), name="g")
        lse, term = a.out(N, torch.float32, name="lse"), a.out(N, torch.int64, name="term").view(torch.float64)
        ops.segment_loss_rows(z, Cn, coords, it, labels, 0, g, lse, term)
        lse_fwd, term_fwd = a.out(N, torch.float32, name="lse forward"), a.out(N, torch.int64, name="term forward").view(torch.float64)
        ops.segment_loss_rows(z, Cn, coords, it, labels, 0, None, lse_fwd, term_fwd)       # (the forward alone: no g)
        assert torch.equal(lse_fwd.view(torch.int32), lse.view(torch.int32)) and torch.equal(term_fwd.view(torch.int64), term.view(torch.int64))
        loss, per_entry = a.out(1, torch.float32, name="loss"), a.out(B, torch.float32, name="per_entry")
        rws = a.out(lib.gp_segment_loss_reduce_workspace_bytes(N, B), torch.uint8, name="reduce workspace")
        ops.segment_loss_reduce(term, coords, it.entry_cnt, B, c.reduction, loss=loss.view(()), per_entry=per_entry, workspace=rws)
        outs = {"u": u, "zero": zero, "g": g, "lse": lse, "term": term.view(torch.int64), "loss": loss, "per_entry": per_entry,
                "entry_cnt": it.entry_cnt, "entry_w": it.entry_w, "status": it.status}
        if index is None:
            outs["row_valid"] = it.row_valid
        else:
            outs["item_off"] = it.item_off
            outs["item_valid_ids"] = it.item_id[:int(it.status[3])]            # (the tail holds the invalid items in sorted order too)
            outs["item_id"] = it.item_id
        return outs

    got = extent_fence.run(case)
    ref = lc.reference(name)
    assert abs(float(got["loss"][0]) - ref.loss) <= LOSS_FRACTION * loss_ceiling(c, ref)
    assert int(got["status"][3]) == int(ref.valid.sum()) and int(got["status"][2]) == B - 1
    assert extent_fence.unwritten(got["g"]) == 0 and not bool(got["g"][:, Cn:].any())


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(env):
    ops, sparse, ME = env
    c = lc.case("points_item")
    F, C, T, L, I = _dev(c.F), _dev(c.coordinates()), _dev(c.text), _dev(c.labels), _dev(c.inv)
    y = ME.SparseTensor(features=F, coordinates=C)
    ok = dict(labels=L, inverse_mapping=I)
    with pytest.raises(ValueError, match="reduction"):
        sparse.segment_loss(y, T, 1.0, reduction="anchor", **ok)
    with pytest.raises(ValueError, match="ignore labels"):
        sparse.segment_loss(y, T, 1.0, ignore_labels=(1, 2, 3, 4, 5), **ok)
    with pytest.raises(ValueError, match="1..4096"):
        sparse.segment_loss(y, torch.randn(4097, c.D, device="cuda"), 1.0, **ok)
    for s in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite and positive"):
            sparse.segment_loss(y, T, s, **ok)
        with pytest.raises(ValueError, match="finite and positive"):
            sparse.segment_loss(y, T, torch.tensor(s, device="cuda"), **ok)
    with pytest.raises(ValueError, match="text_features must be"):
        sparse.segment_loss(y, T[:, :-1], 1.0, **ok)
    with pytest.raises(ValueError, match="labels must be"):
        sparse.segment_loss(y, T, 1.0, labels=L[:-1], inverse_mapping=I)
    with pytest.raises(ValueError, match="labels must be"):
        sparse.segment_loss(y, T, 1.0, labels=L.float(), inverse_mapping=I)
    with pytest.raises(ValueError, match="no CPU path"):
        sparse.segment_loss(y, T.cpu(), 1.0, **ok)
    bad = I.clone()
    bad[3], bad[9] = c.N, -1
    with pytest.raises(ValueError, match=f"2 inverse_mapping values outside 0..{c.N - 1}"):
        sparse.segment_loss(y, T, 1.0, labels=L, inverse_mapping=bad)
    for value, coords in ((65536, C.clone()), (-1, C.clone()), (2 ** 40, C.long())):
        coords[5, 0] = value
        with pytest.raises(ValueError, match="1 rows have a batch index outside 0..65535"):
            sparse.segment_loss(ME.SparseTensor(features=F, coordinates=coords), T, 1.0, **ok)
    with pytest.raises(ValueError, match="not differentiated"):
        sparse.segment_loss(y, T.clone().requires_grad_(), 1.0, **ok)
    with pytest.raises(ValueError, match="not differentiated"):
        sparse.segment_loss(y, T, torch.tensor(2.0, device="cuda", requires_grad=True), **ok)
    with torch.no_grad():                                                      # (grad mode off: nothing is dropped)
        sparse.segment_loss(y, T.clone().requires_grad_(), 1.0, **ok)


def test_one_host_synchronisation(env):
    ops, sparse, ME = env
    c = lc.case("points_item")
    y = ME.SparseTensor(features=_dev(c.F).requires_grad_(), coordinates=_dev(c.coordinates()))
    args = (_dev(c.text), c.s)
    kw = dict(labels=_dev(c.labels), inverse_mapping=_dev(c.inv))
    torch.cuda.synchronize()
    before = ops.READBACK["calls"]
    real = ops.readback
    torch.cuda.set_sync_debug_mode("error")
    try:
        # (the read-back itself is ops.readback's .tolist(), the only synchronising call allowed: count it, forbid every other)

        def counted(t):
            torch.cuda.set_sync_debug_mode("default")
            try:
                return real(t)
            finally:
                torch.cuda.set_sync_debug_mode("error")
        ops.readback = counted
        loss = sparse.segment_loss(y, *args, **kw)
        loss.backward()
    finally:
        ops.readback = real
        torch.cuda.set_sync_debug_mode("default")
    assert ops.READBACK["calls"] == before + 1


# ------------------------------------------------------------------------------------------ the chain
def _chain_inputs():
    import knn_batched_cases as kc
    from geopurify_amd import pipeline as pl
    from geopurify_amd.affinity_module import AffinityPredictor
    D, Cn = 64, 20
    m = AffinityPredictor(D + 6, 128, 128)
    m.load_state_dict(pl.random_student_state_dict(D + 6, hidden=128, embed=128, num_blocks=4, seed=6))
    m = m.cuda()
    rng = np.random.default_rng(8)
    vox = kc.batched({0: kc.surface_exact(rng, 300, 24), 1: kc.surface_exact(rng, 420, 28)}, rng)
    pts = np.vstack([vox, vox[rng.integers(0, len(vox), 500)]])               # 500 points share a voxel with another
    pts = pts[rng.permutation(len(pts))]
    g = torch.Generator().manual_seed(3)
    feats = (torch.randn(len(pts), D + 6, generator=g) * 0.3).cuda()
    text = torch.randn(Cn, D, generator=g).cuda()
    labels = torch.randint(0, Cn, (len(pts),), generator=g)
    labels[::17] = 255
    return m, _dev(pts), feats, text, labels.cuda(), D


def test_chain_reaches_the_student(env):
    """quantize -> student -> purify(differentiable=True) -> segment_loss -> backward: every parameter gets a finite gradient that is
    not all zero, equal bit for bit to the two-step route (dY from segment_loss on a leaf, then Y.backward(dY)); purified_loss is the
    two calls"""
    ops, sparse, ME = env
    m, pts, feats, text, labels, D = _chain_inputs()
    m.train()
    kw = dict(K=24, num_iters=3)
    q = sparse.quantize(pts, feats)
    x = ME.SparseTensor(features=q.features, coordinates=q.coordinates)
    lkw = dict(labels=labels, inverse_mapping=q.inverse_mapping, reduction="entry")

    y = sparse.purify(m, x, feature_dim=D, differentiable=True, **kw)
    loss = sparse.segment_loss(y, text, 14.3, **lkw)
    assert loss.requires_grad and loss.valid.shape == (2,) and int(loss.valid.sum()) == int((labels != 255).sum())
    loss.backward()
    grads = {n: p.grad.clone() for n, p in m.named_parameters()}
    assert len(grads) > 10
    for n, g in grads.items():
        assert bool(torch.isfinite(g).all()) and bool((g != 0).any()), n

    m.zero_grad(set_to_none=True)
    y2 = sparse.purify(m, x, feature_dim=D, differentiable=True, **kw)
    leaf = y2.F.detach().requires_grad_()
    loss2 = sparse.segment_loss(ME.SparseTensor(features=leaf, coordinates=y2.C), text, 14.3, **lkw)
    loss2.backward()
    y2.F.backward(leaf.grad)
    assert torch.equal(loss2.detach(), loss.detach())
    for n, p in m.named_parameters():
        assert torch.equal(p.grad.view(torch.int32), grads[n].view(torch.int32)), n

    m.zero_grad(set_to_none=True)
    both = sparse.purified_loss(m, x, text, 14.3, feature_dim=D, **lkw, **kw)
    assert torch.equal(both.detach(), loss.detach()) and torch.equal(both.purified.F, y.F) and torch.equal(both.per_entry, loss.per_entry)
    both.backward()
    for n, p in m.named_parameters():
        assert torch.equal(p.grad.view(torch.int32), grads[n].view(torch.int32)), n
