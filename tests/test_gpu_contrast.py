"""The contrastive sampler and InfoNCE over batched SparseTensors on the GPU: gp_sim_segments_f16x3 (ops.sim_segments),
gp_sampler_select_segments, gp_sampler_micro_segments, gp_infonce_weighted_fwd_bwd and geopurify_amd.sparse.sample_pairs / info_nce /
contrastive_loss.

References (tests/contrast_cases.py): the fp64 similarity rows and the per-entry selections on them.  The similarities are held to
2e-6 (the bound tests/test_gpu_training.py holds the same three-product arithmetic to); the kernels that select are compared with numpy
on the values the device produced, order included; the API is compared with the fp64 reference on the anchors whose decisions lie
1e-4 outside the rounding (all anchors in `ties`), positives exactly, negatives as sets, no anchor excused."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import contrast_cases as cc
import extent_fence
import knn_batched_cases as kc

from oracle import train as o_train

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURE_OPS = ("sim_segments", "sampler_select_segments", "sampler_micro_segments", "infonce_weighted_fwd_bwd")
SIM_BOUND = 2e-6


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import _lib, ops, sparse
    _lib.load()
    assert all(hasattr(ops, n) for n in FEATURE_OPS) and all(hasattr(sparse, n) for n in ("sample_pairs", "info_nce", "contrastive_loss"))
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import MinkowskiEngine as ME
    finally:
        sys.path.pop(0)
    return ops, sparse, ME


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda() if isinstance(a, np.ndarray) else a.clone().cuda()      # (a copy: the cases are read-only arrays)


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------ kernel level
class Ragged:
    """the descriptors of a case's anchors, sorted by key row (grouped by entry), and the teacher planes in key order"""

    def __init__(self, ops, name):
        C, T, anchors, K = cc.case(name)
        self.perm, self.rank, first, size = cc.key_order(C)
        self.a_key = np.sort(self.rank[anchors])
        self.first, self.len = first[self.a_key], size[self.a_key]
        padded = (self.len + 3) // 4 * 4
        self.off = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
        self.floats = int(padded.sum())
        dt = T.shape[1]
        Tk = np.zeros((len(C), (dt + 31) // 32 * 32), np.float32)
        Tk[:, :dt] = T[self.perm]
        self.hi, self.lo = ops.normalize_split_f16(_dev(Tk))
        self.rows64 = cc.sim_rows(C, T, self.perm[self.a_key])
        self.lists = self.rank[kc.oracle_lists_of(C, K)[self.perm[self.a_key]]]      # key rows
        self.max_len = int(self.len.max())

    def dev(self):
        return (_dev(self.a_key.astype(np.int32)), _dev(self.first.astype(np.int32)), _dev(self.len.astype(np.int32)), _dev(self.off))

    def sim(self, ops):
        buf = torch.full((self.floats,), float("nan"), device="cuda")
        a_row, first, length, off = self.dev()
        ops.sim_segments(self.hi, self.lo, a_row, first, length, off, self.max_len, buf)
        return buf


@pytest.mark.parametrize("name", ["two_scenes", "boundaries_32", "boundaries_48", "boundaries_160", "ties"])
def test_sim_segments_vs_fp64(env, name):
    """every element of every anchor's row within 2e-6 of fp64; the floats between the rows (the 16-byte padding) are not written"""
    ops = env[0]
    r = Ragged(ops, name)
    got = _np(r.sim(ops)).astype(np.float64)
    owned = np.zeros(r.floats, bool)
    worst = 0.0
    for i, row in enumerate(r.rows64):
        mine = got[r.off[i]:r.off[i] + r.len[i]]
        owned[r.off[i]:r.off[i] + r.len[i]] = True
        assert np.isfinite(mine).all(), (i, np.flatnonzero(~np.isfinite(mine))[:4])
        worst = max(worst, np.abs(mine - row).max())
    print(name, "max |sim - fp64| =", worst)
    assert worst <= SIM_BOUND
    assert np.isnan(got[~owned]).all()


def test_sim_segments_reads_and_writes_inside_its_extents(env):
    """boundaries_48 (every entry begins and ends inside a tile, one is smaller than a tile, 16 zero columns of padding): planes with a
    row pitch, descriptors and the ragged buffer inside fences; the fences stay intact and the values are those of the plain call"""
    ops = env[0]
    r = Ragged(ops, "boundaries_48")

    def case(arena):
        hi = arena.inp(r.hi, pitch=r.hi.shape[1] + 8, name="hi")
        lo = arena.inp(r.lo, pitch=r.lo.shape[1] + 8, name="lo")
        a_row, first, length, off = (arena.inp(t, name=n) for t, n in zip(r.dev(), ("anchor_row", "seg_first", "seg_len", "row_off")))
        out = arena.out(r.floats, torch.float32, name="sim")
        ops.sim_segments(hi, lo, a_row, first, length, off, r.max_len, out)
        return {"sim": out}
    got = _np(extent_fence.run(case)["sim"])
    assert extent_fence.unwritten(torch.from_numpy(got)) == r.floats - int(r.len.sum())


def _select_numpy(row, anchor_at, lists_at, num_macro, num_micro):
    pos, macro, _, _ = cc.select(row.astype(np.float64) + 0.0, anchor_at, num_macro)
    micro = cc.select_micro(row.astype(np.float64) + 0.0, lists_at, pos, num_micro)[0] if lists_at is not None else None
    return pos, macro, micro


@pytest.mark.parametrize("name", ["two_scenes", "boundaries_48", "ties"])
def test_select_and_micro_on_the_device_values(env, name):
    """ops.sampler_select_segments and ops.sampler_micro_segments against numpy on the similarities the device produced: positive, macro
    in (value, key row) order, micro in (value, slot) order, all exact -- `ties` has thousands of equal values per row"""
    ops = env[0]
    r = Ragged(ops, name)
    buf = r.sim(ops)
    a_row, first, length, off = r.dev()
    before = buf.clone()
    pos, macro = ops.sampler_select_segments(buf, off, length, first, a_row.long(), cc.NUM_MACRO, r.max_len)
    micro = ops.sampler_micro_segments(buf, off, first, length, _dev(r.lists.astype(np.int32)), pos, cc.NUM_NEGATIVES - cc.NUM_MACRO)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))
    vals, pos, macro, micro = _np(buf), _np(pos), _np(macro), _np(micro)
    for i in range(len(r.a_key)):
        f = r.first[i]
        rp, rm, rmi = _select_numpy(vals[r.off[i]:r.off[i] + r.len[i]], r.a_key[i] - f, r.lists[i] - f, cc.NUM_MACRO, cc.NUM_NEGATIVES - cc.NUM_MACRO)
        assert pos[i] == f + rp, i
        assert np.array_equal(macro[i], f + rm), i
        assert np.array_equal(micro[i], r.lists[i][rmi]), i


def test_select_long_row_takes_the_radix_path_through_a_descriptor(env):
    """a ragged buffer of three rows: 100 elements, 600 001 elements of the `one_stride` recipe of test_sampler_select_is_argmax_and_k_lowest
    (all low values in 20 threads' strides: 11.7k elements at or below the bound, more than the candidates' LDS holds) and 5000 elements;
    the bases are not zero; NaN between the rows"""
    ops = env[0]
    rng = np.random.default_rng(2)
    n = 600001
    big = rng.random(n, dtype=np.float32) + 1.0
    j = np.arange(0, n // 4, 1024)
    idx = ((4 * (np.arange(20)[:, None] + j[None, :]))[:, :, None] + np.arange(4)[None, None, :]).reshape(-1)
    idx = idx[idx < n]
    big[idx] = -rng.random(len(idx), dtype=np.float32)
    rows = [rng.standard_normal(100).astype(np.float32), big, rng.standard_normal(5000).astype(np.float32)]
    length = np.array([len(v) for v in rows])
    padded = (length + 3) // 4 * 4
    off = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    base = np.array([7, 1000, 700000])
    anchor_at = np.array([99, 123456, 0])
    buf = np.full(int(padded.sum()), np.nan, np.float32)
    for o, v in zip(off, rows):
        buf[o:o + len(v)] = v
    pos, macro = ops.sampler_select_segments(_dev(buf), _dev(off), _dev(length.astype(np.int32)), _dev(base.astype(np.int32)),
                                             _dev((base + anchor_at).astype(np.int64)), cc.NUM_MACRO, int(length.max()))
    for i, v in enumerate(rows):
        rp, rm, _ = _select_numpy(v, anchor_at[i], None, cc.NUM_MACRO, 0)
        assert int(pos[i]) == base[i] + rp
        assert np.array_equal(_np(macro[i]), base[i] + rm)


def _entry_p2b(p2b, A, Nn, sel):
    sel = torch.as_tensor(sel)
    return torch.cat([p2b[:A][sel], p2b[A:2 * A][sel], p2b[2 * A:].view(A, Nn)[sel].flatten()])


def _oracle_loss(E, s2v, p2b, A, Nn, T, entry, reduction):
    """oracle.train.info_nce: over all anchors ("anchor"), or the mean over the entries of its value on each entry's anchors"""
    if reduction == "anchor":
        return o_train.info_nce(E[s2v], p2b, A, Nn, T)
    parts = []
    for b in np.unique(entry):
        sel = np.flatnonzero(entry == b)
        parts.append(o_train.info_nce(E[s2v], _entry_p2b(p2b, A, Nn, sel), len(sel), Nn, T))
    return torch.stack(parts).mean()


@pytest.mark.parametrize("reduction", ["anchor", "entry"])
def test_infonce_weighted_forward_backward(env, reduction):
    """ops.infonce_weighted_fwd_bwd against oracle.train.info_nce under autograd, two entries of 64 and 32 anchors; tolerances of
    test_infonce_forward_backward (loss 1e-5 relative, gradient 1e-6 + 1e-4 max); uniform weights meet ops.infonce_fwd_bwd"""
    ops = env[0]
    torch.manual_seed(1)
    nv, d, S, A, Nn = 500, 128, 700, 96, 63
    E = torch.randn(nv, d)
    s2v = torch.randint(0, nv, (S,))
    p2b = torch.randint(0, S, (A * (2 + Nn),))
    entry = np.r_[np.zeros(64, np.int64), np.full(32, 3)]
    w = cc.info_nce_weights(entry, reduction)
    Er = E.clone().requires_grad_(True)
    loss_ref = _oracle_loss(Er, s2v, p2b, A, Nn, 0.07, entry, reduction)
    loss_ref.backward()
    loss, per_anchor, dE = ops.infonce_weighted_fwd_bwd(_dev(E), _dev(s2v), _dev(p2b), A, Nn, 0.07, _dev(w.astype(np.float32)))
    ref = float(loss_ref.detach())
    print(reduction, "loss", float(loss), ref, "grad err", float((dE.cpu() - Er.grad).abs().max()), float(Er.grad.abs().max()))
    assert abs(float(loss) - ref) < 1e-5 * max(1.0, abs(ref))
    assert (dE.cpu() - Er.grad).abs().max() < 1e-6 + 1e-4 * Er.grad.abs().max()
    each = torch.stack([o_train.info_nce(E[s2v].double(), _entry_p2b(p2b, A, Nn, [a]), 1, Nn, 0.07) for a in range(A)])
    assert (per_anchor.cpu().double() - each).abs().max() < 1e-5 * max(1.0, float(each.abs().max()))
    if reduction == "anchor":
        loss0, dE0 = ops.infonce_fwd_bwd(_dev(E), _dev(s2v), _dev(p2b), A, Nn, 0.07)
        assert abs(float(loss) - float(loss0)) < 1e-5 * max(1.0, abs(float(loss0)))
        assert (dE - dE0).abs().max() < 1e-6 + 1e-4 * dE0.abs().max()


# ------------------------------------------------------------------------------------------ API level
def _sample(env, name, anchors=None, C=None, T=None, **kw):
    ops, sparse, ME = env
    C0, T0, _, K = cc.case(name)
    anchors = cc.kept(name)[0] if anchors is None else anchors
    if "neighbors" not in kw:
        kw["K"] = K
    return sparse.sample_pairs(_dev(C0 if C is None else C), _dev(T0 if T is None else T), anchor_indices=_dev(anchors), **kw)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_sample_pairs_vs_fp64(env, name):
    C, T, _, K = cc.case(name)
    anchors, ref_pos, ref_neg = cc.kept(name)
    pairs = _sample(env, name)
    for t in (pairs.anchor, pairs.positive, pairs.negative, pairs.entry, pairs.rows, pairs.index):
        assert t.dtype == torch.int64 and t.is_cuda
    assert pairs.negative.shape == (len(anchors), cc.NUM_NEGATIVES) and pairs.num_rows == len(C) and pairs.num_entries == int(C[:, 0].max()) + 1
    assert np.array_equal(_np(pairs.anchor), anchors) and np.array_equal(_np(pairs.entry), C[anchors, 0])
    pos, neg = _np(pairs.positive), _np(pairs.negative)
    # rows of other entries never appear; the anchor and the positive are no negatives (a local one may repeat a global one)
    assert (C[pos, 0] == C[anchors, 0]).all() and (C[neg, 0] == C[anchors, 0][:, None]).all()
    assert (pos != anchors).all() and (neg != anchors[:, None]).all() and (neg != pos[:, None]).all()
    cc.assert_pairs(name, pos, neg, ref_pos, ref_neg)
    sampled = np.concatenate([anchors, pos, neg.reshape(-1)])
    assert np.array_equal(_np(pairs.rows), np.unique(sampled)) and np.array_equal(_np(pairs.rows)[_np(pairs.index)], sampled)


def test_twin_entries_agree_voxel_for_voxel(env):
    """overlap: entries 2 and 3 hold the same voxels with the same teacher rows; anchors on the same voxels get the same voxels, order
    included (equal rows give bit-equal similarities, and the key order inside an entry depends on the voxels alone).  The local
    negatives agree once the lists do: sparse.knn breaks distance ties at the K-th place by INPUT row, so the twins' own lists may hold
    different voxels there -- given the same lists (neighbors=), everything agrees."""
    C, T, anchors, K = cc.case("overlap")
    tw = cc.twin_rows(C, 2, 3)
    pick = tw[np.isin(tw[:, 0], anchors)]
    to3 = np.full(len(C), -1, np.int64)
    to3[tw[:, 0]] = tw[:, 1]
    p2, p3 = _sample(env, "overlap", anchors=pick[:, 0]), _sample(env, "overlap", anchors=pick[:, 1])
    assert np.array_equal(to3[_np(p2.positive)], _np(p3.positive))
    assert np.array_equal(to3[_np(p2.negative)[:, :cc.NUM_MACRO]], _np(p3.negative)[:, :cc.NUM_MACRO])
    lists = kc.oracle_lists_of(C, K)[pick[:, 0]]
    q3 = _sample(env, "overlap", anchors=pick[:, 1], neighbors=_dev(to3[lists]))
    assert np.array_equal(to3[_np(p2.positive)], _np(q3.positive)) and np.array_equal(to3[_np(p2.negative)], _np(q3.negative))


@pytest.mark.parametrize("name", ["two_scenes", "ties"])
def test_permuting_the_rows_permutes_the_result(env, name):
    """ties go by key row, which the voxels alone decide: with the rows permuted, anchors, positives and the global negatives are the
    permuted ones, order included.  The local negatives come from lists, and sparse.knn breaks distance ties at the K-th place by INPUT
    row: with the permuted lists given (neighbors=) they are the permuted ones too; with the kNN's own lists they are held to the
    reference of the permuted input."""
    C, T, _, K = cc.case(name)
    anchors = cc.kept(name)[0]
    P = np.random.default_rng(7).permutation(len(C))                     # new row i is old row P[i]
    new_of = np.empty_like(P)
    new_of[P] = np.arange(len(C))
    a = _sample(env, name)
    b = _sample(env, name, anchors=new_of[anchors], C=C[P], T=T[P], neighbors=_dev(new_of[kc.oracle_lists_of(C, K)[anchors]]))
    assert np.array_equal(P[_np(b.anchor)], _np(a.anchor)) and np.array_equal(P[_np(b.positive)], _np(a.positive))
    assert np.array_equal(P[_np(b.negative)], _np(a.negative)) and torch.equal(a.entry, b.entry)
    c = _sample(env, name, anchors=new_of[anchors], C=C[P], T=T[P])
    assert np.array_equal(P[_np(c.positive)], _np(a.positive))
    assert np.array_equal(P[_np(c.negative)[:, :cc.NUM_MACRO]], _np(a.negative)[:, :cc.NUM_MACRO])
    ref = cc.reference_of(C[P], T[P], new_of[anchors], K)
    keep = np.ones(len(anchors), bool) if name in cc.EXACT_ORDER else (ref["margins"] >= cc.MARGIN).all(1)
    assert keep.mean() >= 0.8
    cc.assert_pairs(name, _np(c.positive)[keep], _np(c.negative)[keep], ref["positive"][keep], ref["negative"][keep])


def test_chunks_do_not_change_the_result(env, monkeypatch):
    ops = env[0]
    calls = []
    run = ops.sim_segments
    monkeypatch.setattr(ops, "sim_segments", lambda *a, **k: (calls.append(a[2].shape[0]), run(*a, **k))[1])
    whole = _sample(env, "two_scenes")
    assert len(calls) == 1
    del calls[:]
    parts = _sample(env, "two_scenes", sim_budget_bytes=1500 * 4 * 50)      # 50 anchors of the longer entry per chunk
    assert len(calls) >= 3 and sum(calls) == len(whole.anchor) and max(calls) <= 50
    for k in ("anchor", "positive", "negative", "entry", "rows", "index"):
        assert torch.equal(getattr(whole, k), getattr(parts, k)), k


def test_drawn_anchors(env):
    """none given: min(num_anchors, N_b // 3) per entry (85, 43 and 100 of 257 / 130 / 511 voxels at num_anchors = 100), unique, the
    same seed gives the same draw, another seed another; and the pairs of the drawn anchors are the reference's where it decides"""
    ops, sparse, ME = env
    C, T, _, K = cc.case("boundaries_48")
    Cd, Td = _dev(C), _dev(T)

    def draw(seed):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return sparse.sample_pairs(Cd, Td, K=K, num_anchors=100, generator=g)
    p, q, other = draw(11), draw(11), draw(12)
    anchors = _np(p.anchor)
    assert len(np.unique(anchors)) == len(anchors) == 85 + 43 + 100
    assert {int(b): int((C[anchors, 0] == b).sum()) for b in (0, 1, 2)} == {0: 85, 1: 43, 2: 100}
    assert np.array_equal(_np(p.entry), C[anchors, 0])
    for k in ("anchor", "positive", "negative"):
        assert torch.equal(getattr(p, k), getattr(q, k)), k
    assert not np.array_equal(np.sort(_np(other.anchor)), np.sort(anchors))
    ref = cc.reference_of(C, T, anchors, K)
    keep = (ref["margins"] >= cc.MARGIN).all(1)
    assert keep.mean() >= 0.8
    cc.assert_pairs("boundaries_48", _np(p.positive)[keep], _np(p.negative)[keep], ref["positive"][keep], ref["negative"][keep])


def test_reference_sampler_fixture_as_two_entries(env):
    """sample_contrastive_pairs_hybrid's own output (tests/golden/ref_sampler.npz: N=2500, Dt=48, 192 anchors, K=96) as entries 0 and 1
    of one batch, entry 1 with its rows reversed, on made-up unique coordinates with the fixture's own neighbour lists; each entry is held
    to the rule of test_sampler_vs_reference_fixture: at most 1 % of the positives differ, each by less than 2e-6 in fp64; a set that
    differs does so in at most 4 rows spanning less than 2e-6"""
    ops, sparse, ME = env
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_sampler.npz"))
    Ft, n = g["F_teacher"], len(g["F_teacher"])
    anchor, nbr = g["out_anchor"].astype(np.int64), g["nbr_anchor"].astype(np.int64)
    ref_pos, ref_neg = g["out_positive"].astype(np.int64), g["out_negative"].astype(np.int64)
    r = np.arange(n)
    xyz = np.c_[r % 50, r // 50, np.zeros(n, np.int64)]
    flip = lambda rows: n + (n - 1 - rows)                                # scene row -> input row of entry 1
    C = np.r_[np.c_[np.zeros(n, np.int64), xyz], np.c_[np.ones(n, np.int64), xyz[::-1]]].astype(np.int32)
    pairs = sparse.sample_pairs(_dev(C), _dev(np.r_[Ft, Ft[::-1]]), anchor_indices=_dev(np.r_[anchor, flip(anchor)]),
                                neighbors=_dev(np.r_[nbr, flip(nbr)]), num_negatives=int(g["num_negatives"]))
    Fn = F.normalize(torch.from_numpy(Ft).double(), dim=1)
    sim = (Fn[anchor] @ Fn.t()).numpy()
    A = len(anchor)
    ar = np.arange(A)
    for b, scene_row in ((0, lambda rows: rows), (1, lambda rows: n - 1 - (rows - n))):
        pos, neg = scene_row(_np(pairs.positive)[b * A:(b + 1) * A]), scene_row(_np(pairs.negative)[b * A:(b + 1) * A])
        assert (_np(pairs.entry)[b * A:(b + 1) * A] == b).all() and pos.min() >= 0 and pos.max() < n and neg.min() >= 0 and neg.max() < n
        pm = pos != ref_pos
        assert pm.mean() <= 0.01
        if pm.any():
            assert np.abs(sim[ar[pm], pos[pm]] - sim[ar[pm], ref_pos[pm]]).max() < 2e-6
        for a in range(A):
            for lo, hi in ((0, 48), (48, neg.shape[1])):
                s_got, s_ref = set(neg[a, lo:hi].tolist()), set(ref_neg[a, lo:hi].tolist())
                if s_got != s_ref:
                    diff = list(s_got ^ s_ref)
                    vals = sim[a, diff]
                    assert len(diff) <= 4 and vals.max() - vals.min() < 2e-6, (b, a, diff)


@pytest.mark.parametrize("subset,reduction", [(True, "anchor"), (False, "entry")])
def test_contrastive_loss_reaches_the_student(env, monkeypatch, subset, reduction):
    """contrastive_loss on a small AffinityPredictor (hidden 128, 38 input columns, train mode) over two_scenes: every parameter gets a
    finite gradient; loss and gradients against the CPU oracle run from the device's pairs -- oracle.train.student_train_forward on the
    same rows with the device's ReLU decisions + info_nce under autograd -- within the bounds test_gpu_student_module.py holds this
    module to at these widths (its GRAD_BOUNDS["train-128-38"])"""
    import test_gpu_student_module as sm
    from geopurify_amd import pipeline as pl
    ops, sparse, ME = env
    C, T, _, K = cc.case("two_scenes")
    anchors = cc.kept("two_scenes")[0]
    rng = np.random.default_rng(41)
    X = sm._features(rng, len(C), 38)
    m = sm._student(pl, 38, 128, seed=3).train(True)
    sd0 = {k: v.clone().cpu() for k, v in m.state_dict().items()}
    outs = sm._keep_relu_outputs(ops, monkeypatch)
    x = ME.SparseTensor(features=X.cuda(), coordinates=_dev(C))
    loss = sparse.contrastive_loss(m, x, _dev(T), subset=subset, reduction=reduction, K=K, anchor_indices=_dev(anchors))
    monkeypatch.undo()
    loss.backward()
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    pairs = loss.pairs
    rows = _np(pairs.rows) if subset else np.arange(len(C))
    Cs = C[rows]
    rank = ops.coords_order_batched(_dev(Cs).contiguous())[1].long()
    masks = [(o[rank] > 0).cpu() for o in outs]
    assert len(masks) == 9
    params = {k: v.double().clone().requires_grad_(True) for k, v in sd0.items()
              if k.endswith("kernel") or k.endswith(".bn.weight") or k.endswith(".bn.bias")}
    bn_state = {k[:-len(".bn.running_mean")]: (v.double().clone(), sd0[k.replace("running_mean", "running_var")].double().clone())
                for k, v in sd0.items() if k.endswith("running_mean")}
    E64 = o_train.student_train_forward(X[rows].double(), sm._oracle_map(Cs), params, bn_state, 4, momentum=0.1, relu_masks=masks)
    A, Nn = pairs.negative.shape
    s2v = torch.arange(len(rows)) if subset else pairs.rows.cpu()
    loss64 = _oracle_loss(E64, s2v, pairs.index.cpu(), A, Nn, 0.07, _np(pairs.entry), reduction)
    loss64.backward()
    bounds = sm.GRAD_BOUNDS["train-128-38"]
    err = {"loss": abs(float(loss.detach()) - float(loss64.detach())) / abs(float(loss64.detach()))}
    for name, p in m.named_parameters():
        g64 = params[name].grad
        err["grad:" + name] = float((p.grad.cpu().double() - g64).abs().max() / g64.abs().max())
    print({k: f"{v:.3e} / {bounds[k]:.3e}" for k, v in err.items()})
    per_entry = loss.per_entry.cpu()
    assert per_entry.shape == (6,) and bool(torch.isnan(per_entry[1:5]).all()) and bool(torch.isfinite(per_entry[[0, 5]]).all())
    if reduction == "entry":
        assert abs(float(per_entry[[0, 5]].mean()) - float(loss.detach())) < 1e-6 * abs(float(loss.detach()))
    for k, e in err.items():
        assert e <= bounds[k], (k, e, bounds[k])


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_run_no_kernel_of_the_sampler(env, monkeypatch):
    ops, sparse, ME = env
    for name in FEATURE_OPS:
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a kernel of the sampler ran"))
    C, T, anchors, K = cc.case("anchors_in_one_entry")
    Cd, Td, Ad = _dev(C), _dev(T), _dev(anchors)
    n = len(C)
    nb = _dev(kc.oracle_lists_of(C, K)[anchors])
    other_entry = nb.clone()
    other_entry[3, 5] = int(np.flatnonzero(C[:, 0] == 4)[0])

    def edited(row, values):
        c = C.copy()
        c[row] = values
        return _dev(c)
    small = np.flatnonzero(C[:, 0] == 1)                                 # entry 1 cut to 40 voxels: more than K, fewer than 48 + 2
    cut = np.ones(n, bool)
    cut[small[40:]] = False
    refused = [
        ("duplicate", (edited(1, C[0]), Td), dict(anchor_indices=Ad)),
        ("batch index", (edited(1, [70000, 0, 0, 0]), Td), dict(anchor_indices=Ad)),
        ("32768", (edited(1, [int(C[1, 0]), 40000, 0, 0]), Td), dict(anchor_indices=Ad)),
        ("need more than K", (_dev(C[cut]), _dev(T[cut])), dict(anchor_indices=_dev(np.arange(4)), K=40)),
        ("need more than K", (_dev(C[cut]), _dev(T[cut])), dict(anchor_indices=_dev(np.arange(4)), neighbors=_dev(np.zeros((4, 60), np.int64)))),
        ("anchor_indices outside", (Cd, Td), dict(anchor_indices=_dev(np.array([0, n])))),
        ("anchor_indices outside", (Cd, Td), dict(anchor_indices=_dev(np.array([-1, 3])))),
        ("neighbors outside", (Cd, Td), dict(anchor_indices=Ad, neighbors=torch.where(nb == nb[0, 0], n, nb))),
        ("another batch entry", (Cd, Td), dict(anchor_indices=Ad, neighbors=other_entry)),
        ("teacher", (Cd, Td[:-1]), dict(anchor_indices=Ad)),
        ("teacher", (Cd, Td[:, 0]), dict(anchor_indices=Ad)),
        ("teacher", (Cd, Td.long()), dict(anchor_indices=Ad)),
        ("teacher", (Cd, Td.cpu()), dict(anchor_indices=Ad)),
        ("anchor_indices", (Cd, Td), dict(anchor_indices=Ad.cpu())),
        ("anchor_indices", (Cd, Td), dict(anchor_indices=Ad.float())),
        ("neighbors", (Cd, Td), dict(anchor_indices=Ad, neighbors=nb[:-1])),
        ("at least 50", (_dev(C[cut]), _dev(T[cut])), dict(anchor_indices=_dev(np.flatnonzero(C[cut][:, 0] == 1)[:5]))),
        ("at least 50", (_dev(C[cut]), _dev(T[cut])), dict(num_anchors=10)),                     # the draw would put anchors into the cut entry
        ("sim_budget_bytes", (Cd, Td), dict(anchor_indices=Ad, sim_budget_bytes=4 * 299)),       # one row of entry 2 takes 4 * 300 bytes
    ]
    for what, args, kw in refused:
        kw = dict(K=K) | kw if "neighbors" not in kw else kw
        with pytest.raises(ValueError, match="sample_pairs") as e:
            sparse.sample_pairs(*args, **kw)
        assert what in str(e.value), (what, str(e.value))
    monkeypatch.undo()
    pairs = sparse.sample_pairs(Cd, Td, K=K, anchor_indices=Ad, neighbors=nb)               # (the same lists given: the same pairs)
    same = sparse.sample_pairs(Cd, Td, K=K, anchor_indices=Ad)
    assert torch.equal(pairs.positive, same.positive) and torch.equal(pairs.negative, same.negative)
    for name in FEATURE_OPS:
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a kernel of the sampler ran"))
    S = pairs.rows.shape[0]
    assert S + 1 < n
    for E in (torch.zeros((S + 1, 16), device="cuda"), torch.zeros((S, 257), device="cuda"), torch.zeros((S, 16)),
              torch.zeros((S, 16), device="cuda").long(), ME.SparseTensor(features=torch.zeros((n - 1, 16), device="cuda"), coordinates=Cd[:-1])):
        with pytest.raises(ValueError, match="info_nce"):
            sparse.info_nce(E, pairs)
    with pytest.raises(ValueError, match="subset"):
        pairs.subset(ME.SparseTensor(features=Td[:-1], coordinates=Cd[:-1]))


def test_info_nce_on_all_rows_equals_the_subset(env):
    """embeddings with N rows (all of x) and with S rows (those of pairs.subset) are the same loss, and the gradient lands on the
    sampled rows only"""
    ops, sparse, ME = env
    pairs = _sample(env, "boundaries_32")
    torch.manual_seed(5)
    E = torch.randn(pairs.num_rows, 32, device="cuda", requires_grad=True)
    a = sparse.info_nce(E, pairs)
    a.backward()
    Es = E.detach()[pairs.rows].clone().requires_grad_(True)
    b = sparse.info_nce(Es, pairs, reduction="anchor")
    b.backward()
    # (the same arithmetic; the atomic sums of the two calls may round in another order)
    assert abs(float(a) - float(b)) <= 1e-6 * abs(float(a)) and (E.grad[pairs.rows] - Es.grad).abs().max() <= 1e-6 * Es.grad.abs().max()
    rest = torch.ones(pairs.num_rows, dtype=torch.bool, device="cuda")
    rest[pairs.rows] = False
    assert not bool(E.grad[rest].any()) and a.per_entry.shape == (3,)
    c = sparse.info_nce(Es.detach().half(), pairs, reduction="entry")
    assert not c.requires_grad and abs(float(c) - float(a.per_entry.mean())) < 1e-2
