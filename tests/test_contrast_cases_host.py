"""The cases of tests/contrast_cases.py on the host: the fp64 reference is, per batch entry, oracle.train.sample_pairs on that entry
alone; enough drawn anchors survive the margin filter; the cases have the shapes their names promise; and the refusals of
geopurify_amd.sparse.sample_pairs / info_nce that need no device."""
import numpy as np
import pytest
import torch

import contrast_cases as cc
import knn_batched_cases as kc
from oracle import train as o_train


@pytest.mark.parametrize("name", list(cc.CASES))
def test_reference_is_the_oracle_sampler_per_entry(name):
    """every entry by itself, rows in key order (so that index ties mean key-row ties), through oracle.train.sample_pairs: the same
    positives, and the same negatives in order -- in `ties` the same VALUES in order, since torch.topk does not order equal values"""
    C, T, anchors, K = cc.case(name)
    ref = cc.reference(name)
    perm, rank, first, size = cc.key_order(C)
    lists = kc.oracle_lists_of(C, K)
    Fn = cc.unit_rows(T)
    for b in np.unique(C[anchors, 0]):
        sel = np.flatnonzero(C[anchors, 0] == b)
        f = first[rank[anchors[sel[0]]]]
        rows = perm[f:f + size[f]]                                       # the entry's input rows in key order
        local = torch.from_numpy(rank[anchors[sel]] - f)
        nb = torch.from_numpy(rank[lists[anchors[sel]]] - f)
        pos, neg, _ = o_train.sample_pairs(torch.from_numpy(T[rows]).double(), nb, local, cc.NUM_NEGATIVES)
        pos, neg = rows[pos.numpy()], rows[neg.numpy()]
        if name in cc.EXACT_ORDER:
            s = lambda a, j: np.einsum("ad,and->an", Fn[a], Fn[j])
            assert np.array_equal(s(anchors[sel], pos[:, None]), s(anchors[sel], ref["positive"][sel][:, None]))
            # (the local negatives that are the positive read +inf in both: compare the rest)
            assert np.allclose(s(anchors[sel], neg[:, :cc.NUM_MACRO]), s(anchors[sel], ref["negative"][sel][:, :cc.NUM_MACRO]), rtol=0, atol=1e-14)
        else:
            ok = (ref["margins"][sel] >= 1e-12).all(1)                   # (an fp64 tie would be a coincidence: none is expected)
            assert ok.all()
            assert np.array_equal(pos, ref["positive"][sel])
            assert np.array_equal(neg, ref["negative"][sel])


@pytest.mark.parametrize("name", [n for n in cc.CASES if n not in cc.EXACT_ORDER])
def test_enough_anchors_decide_outside_the_rounding(name):
    anchors = cc.case(name)[2]
    keep = cc.kept(name)[0]
    assert len(keep) >= 0.8 * len(anchors), (len(keep), len(anchors))
    assert len(np.unique(cc.case(name)[0][keep, 0])) == len(np.unique(cc.case(name)[0][anchors, 0]))    # every entry keeps some


def test_case_shapes():
    sizes = lambda C: {int(b): int((C[:, 0] == b).sum()) for b in np.unique(C[:, 0])}
    C, T, anchors, K = cc.case("two_scenes")
    assert sizes(C) == {0: 1500, 5: 700} and T.shape[1] == 64 and K == 32
    for dt in (32, 48, 160):
        C, T, anchors, K = cc.case(f"boundaries_{dt}")
        assert sizes(C) == {0: 257, 1: 130, 2: 511} and T.shape[1] == dt
        assert np.array_equal(C, cc.case("boundaries_32")[0]) and np.array_equal(anchors, cc.case("boundaries_32")[2])
    C, T, anchors, K = cc.case("overlap")
    for b0, b1, same in ((0, 1, False), (2, 3, True)):
        tw = cc.twin_rows(C, b0, b1)
        assert np.array_equal(T[tw[:, 0]], T[tw[:, 1]]) == same
    tw = cc.twin_rows(C, 2, 3)
    in2 = np.isin(tw[:, 0], anchors)
    assert in2.sum() > 50 and np.array_equal(in2, np.isin(tw[:, 1], anchors))
    C, T, anchors, K = cc.case("ties")
    assert len(np.unique(T, axis=0)) == 12
    rows = cc.sim_rows(C, T, anchors[:4])
    assert all(len(np.unique(r)) <= 12 for r in rows) and sum(len(r) - len(np.unique(r)) for r in rows) > 2000     # thousands of exact ties
    C, T, anchors, K = cc.case("anchors_in_one_entry")
    assert sorted(sizes(C)) == [1, 2, 4] and set(C[anchors, 0].tolist()) == {2}


def test_ties_go_by_key_row_not_input_row():
    """the case makes the two rules differ: some positive is not the lowest INPUT row among its equals"""
    C, T, anchors, K = cc.case("ties")
    ref = cc.reference("ties")
    Fn = cc.unit_rows(T)
    differ = 0
    for a, p in zip(anchors, ref["positive"]):
        v = Fn @ Fn[a]
        same = np.flatnonzero((C[:, 0] == C[a, 0]) & (np.arange(len(C)) != a) & (v == v[p]))
        assert p in same
        differ += p != same.min()
    assert differ > len(anchors) // 2


def test_info_nce_weights():
    entry = np.array([0, 0, 0, 5, 5])
    assert np.allclose(cc.info_nce_weights(entry, "anchor"), 0.2)
    assert np.allclose(cc.info_nce_weights(entry, "entry"), [1 / 6, 1 / 6, 1 / 6, 1 / 4, 1 / 4])


# ------------------------------------------------------------------------------------------ refusals that need no device
def test_refusals_without_a_device(monkeypatch):
    from geopurify_amd import ops, sparse
    for name in ("sim_segments", "sampler_select_segments", "sampler_micro_segments", "infonce_weighted_fwd_bwd", "coords_order_batched"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a kernel ran"))
    C = torch.zeros((100, 4), dtype=torch.int32)
    T = torch.zeros((100, 8))
    bad = [
        dict(num_macro=0), dict(num_macro=49, num_negatives=48), dict(num_negatives=64), dict(num_macro=True), dict(num_negatives=63.0),
        dict(K=0), dict(K=128), dict(K=15),                                # (15 local negatives need K - 1 >= 15)
        dict(num_macro=1, num_negatives=33, K=32),
        dict(num_anchors=0), dict(sim_budget_bytes=0), dict(sim_budget_bytes=1.5),
        dict(neighbors=torch.zeros((4, 32), dtype=torch.int64)),           # lists without anchors
        dict(anchor_indices=torch.zeros(4, dtype=torch.int64), neighbors=torch.zeros((4, 32))),      # floating lists
        dict(anchor_indices=torch.zeros(4, dtype=torch.int64), neighbors=torch.zeros((4, 8), dtype=torch.int64)),       # K = 8 < 16
        {},                                                                # CPU coordinates: there is no CPU path
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="sample_pairs"):
            sparse.sample_pairs(C, T, **kw)
    with pytest.raises(ValueError, match="sample_pairs"):
        sparse.sample_pairs(C[:, :3], T)
    with pytest.raises(ValueError, match="sample_pairs"):
        sparse.sample_pairs(C.float(), T)
    pairs = sparse.ContrastivePairs(*(torch.zeros(3, dtype=torch.int64),) * 2, torch.zeros((3, 63), dtype=torch.int64),
                                    torch.zeros(3, dtype=torch.int64), 100, 1)
    E = torch.zeros((100, 16))
    for args, kw in (((E, None), {}), ((E, pairs), dict(reduction="mean")), ((E, pairs), dict(temperature=0.0)), ((E, pairs), dict(temperature=None)),
                     ((E.long(), pairs), {}), ((E[0], pairs), {}), ((torch.zeros((100, 257)), pairs), {}), ((torch.zeros((50, 16)), pairs), {})):
        with pytest.raises(ValueError, match="info_nce"):
            sparse.info_nce(*args, **kw)
    with pytest.raises(ValueError, match="contrastive_loss"):
        sparse.contrastive_loss(lambda x: x, E, T)
