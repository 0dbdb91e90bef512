"""The cases of tests/segment_cases.py on the host: the numpy model of gp_nn1_batched's ladder (same acceptance bound, same cell blocks)
agrees with the brute-force fill on every case, and each case takes the rung it is meant to take -- so a case cannot silently stop
covering its branch.  No GPU."""
import numpy as np
import pytest

import knn_batched_cases as kc
import segment_cases as sc


@pytest.mark.parametrize("name", list(sc.CASES))
def test_ladder_model_equals_brute_force(name):
    C, zero = sc.case(name)
    for axes in (7, 6):
        got, path = sc.ladder_of(C, zero, axes)
        assert np.array_equal(got, sc.fill_of(C, zero, axes)), (name, axes)
        assert (path[~zero] == sc.NONE).all()
        if axes != 7:
            assert set(path[zero].tolist()) <= {sc.SCAN, sc.NONE}


def _paths(name):
    C, zero = sc.case(name)
    return sc.ladder_of(C, zero)[1][zero]


def test_each_case_takes_its_rung():
    assert set(_paths("rung_cell").tolist()) == {sc.RING1}
    assert set(_paths("rung_ring3").tolist()) == {sc.RING1, sc.RING3}
    p = _paths("rung_scan")
    assert {sc.RING1, sc.RING3, sc.SCAN} == set(p.tolist()) and (p == sc.SCAN).sum() >= 64
    assert _paths("tie_bound_1").tolist() == [sc.RING3]                # the tie at 81 = (8 + 1)^2 is not final at ring 1
    assert _paths("tie_bound_3").tolist() == [sc.SCAN]                 # nor the tie at 625 = (24 + 1)^2 at ring 3
    assert _paths("ties").tolist() == [sc.RING1]
    assert set(_paths("extent").tolist()) == {sc.SCAN}
    assert set(_paths("empty_entry").tolist()) == {sc.NONE} and set(_paths("one_zero_row").tolist()) == {sc.NONE}
    for n in (63, 64, 65, 257):
        assert len(_paths(f"queries_{n}")) == n
    C, zero = sc.case("all_but_one")
    assert zero.sum() == len(C) - 1


def test_the_tie_cases_tie_where_they_should():
    for name, R, inside, outside in (("tie_bound_1", 1, (25, 16, 16), (7, 16, 16)), ("tie_bound_3", 3, (57, 32, 32), (7, 32, 32))):
        C, zero = sc.case(name)
        q = int(np.flatnonzero(zero)[0])
        ri, ro = kc.row_of(C, 0, inside), kc.row_of(C, 0, outside)
        d2 = lambda r: int(((C[r, 1:].astype(np.int64) - C[q, 1:]) ** 2).sum())
        assert d2(ri) == d2(ro) == (8 * R + 1) ** 2 and ro < ri
        cell = C[:, 1:] >> 3                                            # (the minimum is the origin: the key shift is zero)
        assert np.abs(cell[ri] - cell[q]).max() <= R < np.abs(cell[ro] - cell[q]).max()
        assert sc.fill_of(C, zero)[q] == ro
    # ties: the lowest input row among the 24 is not the lowest sorted row
    C, zero = sc.case("ties")
    q = int(np.flatnonzero(zero)[0])
    d2 = ((C[:, 1:].astype(np.int64) - C[q, 1:]) ** 2).sum(1)
    tied = np.flatnonzero((d2 == 5) & ~zero)
    assert len(tied) == 24
    keys = kc.keys_of(C.astype(np.int64))
    assert sc.fill_of(C, zero)[q] == tied.min() != tied[np.argmin(keys[tied])]
    # yz: three references share the query's (y, z); the masked distance ties at 0, the full one does not
    C, zero = sc.case("yz")
    q = kc.row_of(C, 0, (10, 50, 50))
    col = [kc.row_of(C, 0, (x, 50, 50)) for x in (20, 3, 11)]
    assert sc.fill_of(C, zero, 6)[q] == min(col) and sc.fill_of(C, zero, 7)[q] == kc.row_of(C, 0, (11, 50, 50))


def test_overlap_and_extent_are_what_they_claim():
    C, zero = sc.case("overlap")
    a, b = C[C[:, 0] == 0], C[C[:, 0] == 1]
    assert np.array_equal(np.unique(a[:, 1:], axis=0), np.unique(b[:, 1:], axis=0))
    ff = sc.fill_of(C, zero)
    assert (ff[zero] >= 0).all() and (C[ff[zero], 0] == C[zero, 0]).all()
    # a fill that ignored the entries would differ: some zero row's nearest non-zero voxel of the OTHER entry is nearer
    merged = sc.fill_of(np.c_[np.zeros(len(C), np.int32), C[:, 1:] * 2 + C[:, :1]].astype(np.int32), zero)
    assert (C[merged[zero], 0] != C[zero, 0]).any()
    C, zero = sc.case("extent")
    ext = C[:, 1:].astype(np.int64).max(0) - C[:, 1:].min(0) + 1
    assert ext[0] == 32767 and C[:, 1:].min() < 0
    d2 = ((C[sc.fill_of(C, zero)[zero], 1:].astype(np.int64) - C[zero, 1:]) ** 2).sum(1)
    assert (d2 > 2 ** 30 - 2 ** 18).all() and (d2 < 2 ** 30).all()


@pytest.mark.parametrize("D,Cn", [(64, 20), (512, 20), (96, 160), (10, 3)])
def test_feature_recipe_keeps_its_margin(D, Cn):
    """the recipe's fp64 top-2 cosine margin at the widths the GPU tests use: far above the 0.1 the exact comparison asks for"""
    F, cls = sc.features("overlap", D, Cn)
    zero = sc.case("overlap")[1]
    m, am = sc.margins(F, sc.text(D, Cn))
    print(f"D={D} C={Cn}: smallest margin {m[~zero].min():.3f}")
    assert m[~zero].min() >= 0.3 and (cls[zero] == 0).all() and (m[zero] == 0).all()


def test_counts_reference_on_a_hand_case():
    pred = np.array([0, 1, 1, 2, 5, 1])
    target = np.array([0, 1, 2, 255, 1, 7])
    batch = np.array([0, 0, 2, 2, 2, 2])
    got = sc.counts_of(pred, target, batch, 3, 3, (255,))
    assert got[0].tolist() == [[1, 1, 0], [1, 1, 0], [1, 1, 0]]
    assert got[1].sum() == 0
    assert got[2].tolist() == [[0, 0, 0], [0, 2, 0], [0, 1, 1]]         # the ignored row's prediction is overwritten; 5 and 7 are dropped
