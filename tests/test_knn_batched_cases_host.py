"""The cases of tests/knn_batched_cases.py on the host: the numpy model of gp_knn_batched's ladder reaches, in every case, the path
the case is named for, and its lists equal the reference's (oracle.affinity.knn_lattice per entry) -- which alone judges the GPU.
Also what geopurify_amd.sparse refuses before it touches a device."""
import numpy as np
import pytest
import torch

import knn_batched_cases as kc
from geopurify_amd import sparse


def test_lattice_shells_have_the_stated_sizes():
    """r3(74) = 120 is the largest shell below 81 = ring 1's bound, r3(314) = 312 exceeds the 256 ties kept, inside ring 3's bound"""
    assert len(kc.shell(74)) == 120 and max(len(kc.shell(d)) for d in range(81)) == 120
    assert len(kc.shell(314)) == 312 > kc.KNN_MAXTIE and 314 < 25 ** 2 and np.abs(kc.shell(314)).max() < 24


@pytest.mark.parametrize("name", list(kc.CASES))
def test_model_equals_oracle(name):
    C, K = kc.case(name)
    lists, path = kc.ladder(name)
    ref = kc.oracle_lists(name)
    assert ref.min() >= 0 and (path != kc.SHORT).all()
    assert np.array_equal(lists, ref)
    # no list crosses entries, none holds its own row
    assert (C[ref, 0] == C[:, :1]).all() and (ref != np.arange(len(C))[:, None]).all()


def _paths(name, batch=None):
    C, K = kc.case(name)
    path = kc.ladder(name)[1]
    return path if batch is None else path[C[:, 0] == batch]


def test_every_case_reaches_its_path():
    # surface entries: ring 1 answers nearly every query; the dense 14^3 cube: every query at every K
    assert (_paths("overlap") == kc.RING1).mean() > 0.9
    for name in ("cube14_k1", "cube14_k7", "cube14_k127"):
        assert (_paths(name) == kc.RING1).all(), name
    # K+1 = 97 of 97: every query needs the whole entry, which ring 1 cannot prove for all of them; the 3000-voxel entry (the shape of
    # test_knn_exact_with_ties) is answered by the two rings, mostly the first
    p97, p3000 = _paths("sizes_97_3000", 0), _paths("sizes_97_3000", 1)
    assert len(p97) == 97 and (p97 != kc.RING1).any() and (p3000 == kc.RING1).mean() > 0.5 and (p3000 == kc.RING3).any()
    # 120 ties at the 17th neighbour: within the LDS budget, ring 1 resolves the centre
    C, K = kc.case("ties120")
    centre = kc.row_of(C, 0, kc.TIES120_CENTRE)
    assert kc.ladder("ties120")[1][centre] == kc.RING1
    ref = kc.oracle_lists("ties120")[centre]
    d2 = ((C[ref, 1:].astype(np.int64) - kc.TIES120_CENTRE) ** 2).sum(1)
    assert (d2[:5] == 1).all() and (d2[5:] == 74).all() and (np.diff(ref[5:]) > 0).all()      # 11 of the 120 ties: the lowest rows
    # 312 ties at the 21st: ring 1 has 11 candidates below 81, ring 3 more ties than it keeps -> exhaustive
    C, K = kc.case("ties312")
    centre = kc.row_of(C, 0, kc.TIES312_CENTRE)
    assert kc.ladder("ties312")[1][centre] == kc.EXHAUSTIVE
    ref = kc.oracle_lists("ties312")[centre]
    d2 = ((C[ref, 1:].astype(np.int64) - kc.TIES312_CENTRE) ** 2).sum(1)
    assert (d2[:10] <= 2).all() and (d2[10:] == 314).all() and (np.diff(ref[10:]) > 0).all()
    # the far-apart clusters (at most 9 voxels within ring 3's reach, K = 20): every query is handed on twice and answered exhaustively;
    # the dense entries beside it stay on ring 1
    assert (_paths("sparse_between_dense", 1) == kc.EXHAUSTIVE).all()
    assert (_paths("sparse_between_dense", 0) == kc.RING1).all() and (_paths("sparse_between_dense", 2) == kc.RING1).all()


def test_sparse_entry_would_fail_without_the_batch_bits():
    """the lists of entry 1 over ALL rows (what a scan that ignores the entries finds) hold rows of the dense entries"""
    C, K = kc.case("sparse_between_dense")
    from oracle import affinity as o_aff
    flat = o_aff.knn_lattice(C[:, 1:].copy(), K).numpy()
    rows = np.flatnonzero(C[:, 0] == 1)
    assert (C[flat[rows], 0] != 1).any()


def test_borders_case_holds_its_edges():
    C, K = kc.case("borders")
    assert sorted(np.unique(C[:, 0]).tolist()) == [0, 1, 65535] and C[:, 1:].min() < 0
    lo = C[:, 1:].min(0)
    for b in (0, 1):
        kc.row_of(C, b, lo)                                              # the voxel at the global minimum of every axis, in two entries
    keys = np.sort(kc.keys_of(C))
    batch, _ = kc.decode(keys)
    cells = keys >> np.uint64(9)
    edge = np.flatnonzero(np.diff(batch) != 0)
    assert len(edge) == 2 and (cells[edge] != cells[edge + 1]).all()       # adjacent cells of different entries differ in the batch bits only ...
    assert (cells[edge[0] + 1] & np.uint64((1 << 39) - 1)) == 0            # ... entry 1 opens with the cell at the origin


def test_short_entry_case():
    C, K, b, n = kc.short_entry_case()
    assert (C[:, 0] == b).sum() == n == K
    lists, path = kc.ladder_of(C, K)
    assert (path[C[:, 0] == b] == kc.SHORT).all() and (lists[C[:, 0] == b] == -1).all() and (path[C[:, 0] != b] != kc.SHORT).all()
    assert np.array_equal(lists, kc.oracle_lists_of(C, K))


def test_pool_family_by_width():
    assert sparse.pool_family(512, 96, 19) == "cs" and sparse.pool_family(256, 96, 19) == "cs"
    assert sparse.pool_family(64, 96, 19) == "ell" and sparse.pool_family(70, 96, 19) == "ell" and sparse.pool_family(512, 96, 1) == "ell"
    assert sparse.pool_family(1024, 96, 19) == "tiles" and sparse.pool_family(512, 96, 19, "mfma_chain") == "chain"
    with pytest.raises(ValueError):
        sparse.pool_family(70, 96, 19, "mfma_cs")
    with pytest.raises(ValueError):
        sparse.pool_family(512, 96, 19, "no_such_mode")


class _ST:
    def __init__(self, features=None, coordinates=None):
        self.F, self.C = features, coordinates


def test_refusals_that_need_no_device():
    C = torch.zeros((5, 4), dtype=torch.int32)
    x = _ST(torch.zeros(5, 8), C)
    for k in (0, 128, -1, 2.0, True):
        with pytest.raises(ValueError, match="outside 1..127"):
            sparse.knn(C, k)
        with pytest.raises(ValueError, match="outside 1..127"):
            sparse.affinity_pool(x, torch.zeros(5, 4), K=k)
    with pytest.raises(ValueError, match="num_iters"):
        sparse.affinity_pool(x, torch.zeros(5, 4), K=2, num_iters=-1)
    with pytest.raises(ValueError, match="CUDA"):
        sparse.knn(C, 2)
    with pytest.raises(ValueError, match="CUDA"):
        sparse.affinity_pool(x, torch.zeros(5, 4), K=2)
    with pytest.raises(ValueError, match=r"\[N, 4\]"):
        sparse.knn(torch.zeros((5, 3), dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="integers"):
        sparse.knn(torch.zeros((5, 4)), 2)
    with pytest.raises(ValueError, match="SparseTensor"):
        sparse.affinity_pool(torch.zeros(5, 8), torch.zeros(5, 4))
