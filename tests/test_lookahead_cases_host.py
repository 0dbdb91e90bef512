"""The cases of tests/lookahead_cases.py hold what they are named for, and their numpy references agree with fp64 (no GPU)."""
import numpy as np
import pytest

import lift_cases as lc
import lookahead_cases as la


@pytest.mark.parametrize("d", la.FUSE_D)
def test_mixed_fuse_case_holds_every_named_point(d):
    c = la.case_fuse_fill("mixed", d)
    start, names = c["start"], c["names"]
    M = np.diff(start)
    seen = la.ref_seen(start)
    assert seen.sum() == (M > 0).sum() and 0 < seen.sum() < c["n"]
    nn = la.ref_nn(c["xyz"], seen)
    assert (nn[seen == 1] == -1).all() and (nn[seen == 0] >= 0).all() and (seen[nn[seen == 0]] == 1).all()
    fused = lc.ref_fuse(start, c["pv_view"], c["pv_seg"], c["fseg"], c["lseg"])
    want_neg = {"m65": None, "neg1": 1, "neg2": 2, "neg3": 3, "plain3": 0}
    for name in la.SPECIAL:
        p, t = names.index(name), names.index(name + ".twin")
        assert M[t] == 0 and nn[t] == p, name                       # the unseen twin is filled from the hand-built point
        top = fused["top"][p]
        if want_neg[name] is not None:
            assert M[p] == 3 and (c["pv_seg"][top] < 0).sum() == want_neg[name], name
    assert M[names.index("m65")] == 65                               # the M > 64 loops
    assert np.abs(fused["out"][names.index("neg3")]).max() == 0      # all slots -1: a zero row that is SEEN
    assert c["pv_view"].max() < c["V"] and c["pv_seg"].max() < c["Q"] and c["pv_seg"].min() == -1
    # the fill is a proper mix: some filled rows come from rows that are themselves zero, some unseen points sit among generic ones
    assert (M == 0).sum() > 50


def test_small_fuse_cases():
    c = la.case_fuse_fill("none_seen", 64)
    assert c["start"].max() == 0 and c["n"] == 40 and (la.ref_nn(c["xyz"], la.ref_seen(c["start"])) == -1).all()
    one = la.case_fuse_fill("single", 512)
    assert one["n"] == 1 and one["start"].tolist() == [0, 2] and la.ref_nn(one["xyz"], la.ref_seen(one["start"])).tolist() == [-1]
    none = la.case_fuse_fill("single_unseen", 768)
    assert none["n"] == 1 and none["start"].tolist() == [0, 0]


def test_ref_nn_takes_the_lowest_index_among_equals():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [5, 5, 5]], np.float32)
    assert la.ref_nn(xyz, np.array([0, 1, 1, 0], np.uint8)).tolist() == [1, -1, -1, 1]


def test_ref_pow2_for():
    for amax, k in ((1.0, 13), (0.75, 14), (16383.0, 0), (16384.0, -1), (1e-30, 100), (1e30, -86)):
        s = la.ref_pow2_for(amax)
        assert s == np.float32(2.0) ** k, (amax, s)
        if abs(k) < 100:
            assert 2.0 ** 13 <= np.float32(amax) * s < 2.0 ** 14
    assert la.ref_pow2_for(0.0) == 1 and la.ref_pow2_for(np.inf) == 1


@pytest.mark.parametrize("nv,d", la.VOXEL_SHAPES)
def test_voxel_case_and_its_reference(nv, d):
    c = la.case_voxel_rows(nv, d)
    sizes = np.diff(c["seg_start"])
    assert c["cin_pad"] == {512: 544, 64: 96}[d] and c["cin_pad"] % 32 == 0
    assert sorted(c["row_map"].tolist()) == list(range(nv)) and sorted(c["order"].tolist()) == list(range(c["N"]))
    for v in range(nv):                                              # ascending point ids inside a voxel
        seg = c["order"][c["seg_start"][v]:c["seg_start"][v + 1]]
        assert (np.diff(seg) > 0).all()
    if nv == 1:
        assert sizes.tolist() == [2]
    else:
        assert set(sizes.tolist()) == {1, 2, 37} and nv % 4 != 0     # the last workgroup of 4 waves is partly filled
    X, row_inv, sc = la.ref_voxel_rows(c)
    # the fp32 sums against fp64 means
    # sequential fp32 sum of n <= 37 terms and one division: |error| <= n 2^-24 max |x| over the voxel's points, per column
    want, bound = np.zeros((nv, d + la.GEO_DIM)), np.zeros((nv, d + la.GEO_DIM))
    both = np.concatenate([c["F"], c["geo"]], 1).astype(np.float64)
    for v in range(nv):
        seg = c["order"][c["seg_start"][v]:c["seg_start"][v + 1]]
        want[c["row_map"][v]] = both[seg].mean(0)
        bound[c["row_map"][v]] = len(seg) * 2.0 ** -24 * np.abs(both[seg]).max(0)
    assert (np.abs(X[:, :d + la.GEO_DIM] - want) <= bound).all()
    assert (X[:, d + la.GEO_DIM:] == 0).all()
    if nv >= 5:
        rm = c["row_map"]
        assert np.abs(X[rm[la.ZERO_V]]).max() == 0 and row_inv[rm[la.ZERO_V]] == 1
        assert 0 < np.abs(X[rm[la.TINY_V]]).max() < 1e-29 and row_inv[rm[la.TINY_V]] == np.float32(2.0) ** -100     # the clamped exponent
        assert sizes[la.HUGE_V] == 37
        r, col = np.unravel_index(np.abs(X[:, :d]).argmax(), (nv, d))
        assert (r, col) == (rm[la.HUGE_V], d - 1)                    # the global maximum sits in the last feature column
        assert np.abs(X[rm[la.GEO_V], d:]).max() > np.abs(X[:, :d]).max()          # geometry above it: the row's scale only
        assert sc[0] == la.ref_pow2_for(np.abs(X[rm[la.HUGE_V], d - 1])) and sc[0] * sc[1] == 1
        assert row_inv[rm[la.GEO_V]] > 1 / sc[0]


@pytest.mark.parametrize("name", list(la.KNN_CASES))
def test_knn_cases_reach_their_paths(name):
    import lattice_cases as ltc
    v = la.case_knn(name)
    cand = la.first_ring_candidates(v)
    if name == "above_max":
        assert cand.min() == 4096 > la.KNN_KEEP_CANDIDATES
    elif name == "at_max":
        assert cand.min() == cand.max() == la.KNN_KEEP_CANDIDATES
    else:
        centre = ltc.row_of(v, la.TIES257_CENTRE)
        K = la.KNN_CASES[name][0]
        kept, ties = ltc.kept_ties(v, K, centre, np.arange(len(v)))
        d2 = ((v.astype(np.int64) - v[centre]) ** 2).sum(1)
        assert ties == 257 == ltc.KNN_MAXTIE + 1 and (d2 < 81).sum() == 11 < K + 1          # ring 1 lacks candidates, ring 3 has one tie too many
        _, path = ltc.ladder(v, K)
        assert path[centre] == ltc.EXHAUSTIVE
