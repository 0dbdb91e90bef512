"""Per-entry exact kNN over batched coordinates (gp_knn_batched, ops.knn_batched, geopurify_amd.sparse.knn) and the purifying step
over batched SparseTensors (sparse.affinity_pool / purify) on the GPU.

kNN reference: oracle.affinity.knn_lattice per entry on the entry's rows in input order (tests/knn_batched_cases.py); lists are
compared for exact equality, order included, every row.  The cases are the smallest shapes at which each branch of the kernel can go
wrong; test_knn_batched_cases_host.py shows on the host which path of the ladder each of them takes.

Pooling reference: per entry oracle.affinity.affinity_weights and pool_gather in fp64 on the oracle's lists.  Bounds, the ones the
project holds for these kernels (test_affinity_on_matrix_cores_vs_reference_fixture, test_pool_cs_matches_ell_and_oracle): weights
within 2e-6, pooled features within 1e-4 absolute.
"""
import os
import sys

import numpy as np
import pytest
import torch

import extent_fence
import knn_batched_cases as kc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_TOL, Y_TOL = 2e-6, 1e-4


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


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # (a copy: the cases are read-only arrays)


def _ordered(ops, C):
    perm, rank, keys, st = ops.coords_order_batched(_dev(C))
    assert st.tolist() == [0, 0, 0]
    return perm, rank, keys


def _to_input_rows(perm, rank, nbr):
    """lists of sorted-row numbers in the sorted order -> int64 numpy lists of input rows in the input's order (-1 stays -1)"""
    p, n = perm.long(), nbr.long()
    return torch.where(n >= 0, p[n.clamp(min=0)], n).index_select(0, rank.long()).cpu().numpy()


# ------------------------------------------------------------------------------------------ kNN: the cases
@pytest.mark.parametrize("name", list(kc.CASES))
def test_lists_equal_the_oracle(env, name):
    """overlapping entries, K+1 voxels beside 3000, K = 1 / 7 / 127, ties inside and beyond the LDS budget, the sparse entry between
    dense ones, the borders: through ops.knn_batched (status clean) and through sparse.knn, every list exact"""
    ops, sparse, ME = env
    C, K = kc.case(name)
    ref = kc.oracle_lists(name)
    perm, rank, keys = _ordered(ops, C)
    nbr, status = ops.knn_batched(keys, perm, K)
    assert status.tolist() == [0, -1, 0, 0]
    got = _to_input_rows(perm, rank, nbr)
    assert got.min() >= 0 and (C[got, 0] == C[:, :1]).all()                       # no index crosses entries
    assert np.array_equal(got, ref)
    pub = sparse.knn(_dev(C), K)
    assert pub.dtype == torch.int64 and np.array_equal(pub.cpu().numpy(), ref)
    if name == "overlap":                                                          # int64 coordinates take the same route
        assert np.array_equal(sparse.knn(_dev(C.astype(np.int64)), K).cpu().numpy(), ref)


def test_one_entry_equals_the_lattice_path(env):
    """sparse.knn on a single entry = ops.knn_lattice on the same voxels, brought to input rows as test_knn_exact_with_ties does"""
    ops, sparse, ME = env
    K = 96
    c = kc.surface_exact(np.random.default_rng(1), 3000, 60).astype(np.int32)
    ct = _dev(c)
    perm, rank = ops.morton_order(ct)
    cs = ct[perm.long()].contiguous()
    grid = ops.grid_build(cs)
    assert grid.status() == 0
    nbr_int = ops.knn_lattice(grid, cs, perm, K)
    nbr_ref = torch.empty_like(nbr_int)
    nbr_ref[perm.long()] = perm[nbr_int.long()]
    got = sparse.knn(_dev(np.c_[np.zeros(len(c), np.int32), c]), K)
    assert torch.equal(got, nbr_ref.long())


def test_short_entry_is_reported_and_the_others_stay_exact(env):
    ops, sparse, ME = env
    C, K, b, n = kc.short_entry_case()
    perm, rank, keys = _ordered(ops, C)
    nbr, status = ops.knn_batched(keys, perm, K)
    assert status.tolist() == [n, b, n, 0]
    got = _to_input_rows(perm, rank, nbr)
    assert (got[C[:, 0] == b] == -1).all()
    assert np.array_equal(got, kc.oracle_lists_of(C, K))                           # (-1 rows for the short entry, exact lists elsewhere)


def test_axis_mask_is_reported_and_the_call_returns(env):
    """a decoded coordinate of 32768 or more on y: status[3] = 2; the lists are undefined, the stored values stay rows of the entry"""
    ops, sparse, ME = env
    C = kc.batched({0: np.vstack([kc.cube(3), kc.cube(3, (0, 40000, 0))])}, np.random.default_rng(3))
    perm, rank, keys = _ordered(ops, C)
    nbr, status = ops.knn_batched(keys, perm, 5)
    assert status.tolist() == [0, -1, 0, 2]
    assert int(nbr.min()) >= 0 and int(nbr.max()) < len(C)


# ------------------------------------------------------------------------------------------ kNN: refusals (one call each)
def _refused():
    C, K, b, n = kc.short_entry_case()
    yield "entry_of_k_voxels", C, K, rf"knn: batch entry {b} holds {n} voxels, K={K}"
    wide = kc.batched({0: np.vstack([kc.cube(3), kc.cube(3, (32765, 0, 0))])}, np.random.default_rng(4))
    assert wide[:, 1].max() - wide[:, 1].min() + 1 == 32768
    yield "extent_32768", wide, 5, r"knn: coordinate extent of 32768 or more along x"
    dup = kc.batched({0: kc.cube(4), 1: kc.cube(4)}, np.random.default_rng(5))
    dup = np.ascontiguousarray(np.vstack([dup, dup[7:9]]))
    yield "duplicate_rows", dup, 5, r"knn: 2 duplicate coordinate rows \(MinkowskiEngine would merge them; quantise first\)"


@pytest.mark.parametrize("what,C,K,message", [pytest.param(*r, id=r[0]) for r in _refused()])
def test_knn_refuses(env, what, C, K, message):
    ops, sparse, ME = env
    with pytest.raises(ValueError, match=message):
        sparse.knn(_dev(C), K)


def test_affinity_pool_refuses_mismatched_coordinates(env):
    ops, sparse, ME = env
    C, K = kc.case("overlap")
    x = ME.SparseTensor(features=torch.randn(len(C), 8, device="cuda"), coordinates=_dev(C))
    other = _dev(C).clone()
    other[5, 2] += 1
    e = ME.SparseTensor(features=torch.randn(len(C), 16, device="cuda"), coordinates=other)
    with pytest.raises(ValueError, match="affinity_pool: the embeddings' coordinates differ from x.C in 1 elements"):
        sparse.affinity_pool(x, e, K=K)


# ------------------------------------------------------------------------------------------ kNN: extents
def _fence_inputs():
    C, K = kc.case("sparse_between_dense")                                         # ring 1 and the exhaustive kernel answer rows here ...
    yield "ring1_exhaustive", C, K
    C, K = kc.case("overlap")                                                      # ... ring 1 and ring 3 here
    yield "ring1_ring3", C, K
    C, K, b, n = kc.short_entry_case()                                             # the -1 fill and the status words
    yield "short_entry", C, K


@pytest.mark.parametrize("what,C,K", [pytest.param(*r, id=r[0]) for r in _fence_inputs()])
def test_no_access_outside_the_extents(env, what, C, K):
    """keys, ids, lists, status and a workspace of exactly the reported bytes inside poisoned guards: guards intact, same bits"""
    ops, sparse, ME = env
    from geopurify_amd import _lib
    perm, rank, keys = _ordered(ops, C)
    nv = len(C)
    nbytes = _lib.load().gp_knn_batched_workspace_bytes(nv)
    assert nbytes > 0

    def call(a):
        nbr, status = ops.knn_batched(a.inp(keys, name="keys"), a.inp(perm, name="ids"), K, nbr=a.out((nv, K), torch.int32, name="nbr"),
                                      status=a.out(4, torch.int32, name="status"), workspace=a.out(nbytes, torch.uint8, name="workspace"))
        return {"nbr": nbr, "status": status}

    out = extent_fence.run(call)
    assert extent_fence.unwritten(out["nbr"]) == 0 and extent_fence.unwritten(out["status"]) == 0
    assert np.array_equal(_to_input_rows(perm, rank, out["nbr"]), kc.oracle_lists_of(C, K))


# ------------------------------------------------------------------------------------------ affinity_pool
@pytest.fixture(scope="module")
def pool(env):
    C, X, E = kc.pool_case()
    return _dev(C), _dev(X), _dev(E)


def _report(what, got, ref, tol):
    err = float((got.double().cpu() - torch.from_numpy(np.ascontiguousarray(ref))).abs().max())
    print(f"{what}: max |difference| = {err:.3e} (bound {tol:g})")
    return err


def test_weights_on_the_batched_lists(env, pool):
    """the chain affinity_pool runs -- sorted order, ops.knn_batched, ops.l2norm_rows_, ops.affinity_softmax -- taken back to input rows:
    the oracle's lists exactly, its weights within 2e-6"""
    ops, sparse, ME = env
    C, X, E = pool
    Cn = kc.pool_case()[0]
    perm, rank, keys = _ordered(ops, Cn)
    nbr, status = ops.knn_batched(keys, perm, 96)
    assert status.tolist() == [0, -1, 0, 0]
    assert np.array_equal(_to_input_rows(perm, rank, nbr), kc.oracle_lists_of(Cn, 96))
    Es = ops.l2norm_rows_(ops.gather_rows(E * 2.5, E.shape[1], perm.long()))
    w = ops.affinity_softmax(Es, nbr, 20.0).index_select(0, rank.long())
    assert _report("weights", w, kc.pool_reference()[0], W_TOL) <= W_TOL


@pytest.mark.parametrize("D,family,sparse_embeddings", [(512, "cs", False), (64, "ell", True), (70, "ell", False)])
def test_pooled_features_per_entry(env, pool, D, family, sparse_embeddings):
    """K = 96, 19 applications; D = 512 on the column-sliced matrix-core kernels, 64 and 70 (padded to 72 inside) on the ELL kernel.
    The rows of the case are shuffled over the entries: the result comes back in the input's row order."""
    ops, sparse, ME = env
    C, X, E = pool
    assert sparse.pool_family(D, 96, 19) == family
    x = ME.SparseTensor(features=X[:, :D], coordinates=C)
    e = ME.SparseTensor(features=E, coordinates=C.clone()) if sparse_embeddings else E
    y = sparse.affinity_pool(x, e)
    assert type(y) is type(x) and y.C is x.C and y.F.shape == (len(C), D) and y.F.dtype == torch.float32 and not y.F.requires_grad
    assert _report(f"pooled D={D}", y.F, kc.pool_reference()[1][:, :D], Y_TOL) <= Y_TOL


def test_iterations_normalisation_and_grad_flags(env, pool):
    ops, sparse, ME = env
    C, X, E = pool
    D = 64
    x = ME.SparseTensor(features=X[:, :D].clone().requires_grad_(), coordinates=C)
    y0 = sparse.affinity_pool(x, E, num_iters=0)
    assert torch.equal(y0.F, X[:, :D]) and not y0.F.requires_grad                  # the features themselves, detached
    y1 = sparse.affinity_pool(x, E, num_iters=1)
    assert _report("one application", y1.F, kc.pool_reference(num_iters=1)[1][:, :D], Y_TOL) <= Y_TOL
    ref = kc.pool_reference()[1][:, :D]
    plain = sparse.affinity_pool(x, E, normalize=False)                            # rows that are unit already
    assert _report("normalize=False", plain.F, ref, Y_TOL) <= Y_TOL
    scaled = sparse.affinity_pool(x, (E * 3.0).requires_grad_())                   # normalised inside
    assert _report("normalize=True", scaled.F, ref, Y_TOL) <= Y_TOL


def test_a_batch_equals_its_entries_run_alone(env, pool):
    """D = 512: the operator's row blocks differ between the batch and an entry alone, so the results agree within the bound, not bit for bit"""
    ops, sparse, ME = env
    C, X, E = pool
    whole = sparse.affinity_pool(ME.SparseTensor(features=X, coordinates=C), E).F
    for b in C[:, 0].unique().tolist():
        rows = (C[:, 0] == b).nonzero().flatten()
        alone = sparse.affinity_pool(ME.SparseTensor(features=X[rows], coordinates=C[rows]), E[rows]).F
        err = float((alone - whole[rows]).abs().max())
        print(f"entry {b} alone against the batch: max |difference| = {err:.3e}")
        assert err <= Y_TOL


def test_chained_launch_by_name(env, pool):
    """pool_mode="mfma_chain": all applications in one launch, checked (pool_chain_check) before the rows are handed out"""
    ops, sparse, ME = env
    C, X, E = pool
    y = sparse.affinity_pool(ME.SparseTensor(features=X, coordinates=C), E, pool_mode="mfma_chain")
    assert _report("chained", y.F, kc.pool_reference()[1], Y_TOL) <= Y_TOL


# ------------------------------------------------------------------------------------------ purify
def test_purify_is_student_then_affinity_pool(env):
    ops, sparse, ME = env
    from geopurify_amd import pipeline as pl
    from geopurify_amd.affinity_module import AffinityPredictor
    D = 64
    m = AffinityPredictor(D + 6, 128, 128)
    m.load_state_dict(pl.random_student_state_dict(D + 6, hidden=128, embed=128, num_blocks=4, seed=6))
    m = m.cuda()
    rng = np.random.default_rng(7)
    C = _dev(kc.batched({0: kc.surface_exact(rng, 300, 24), 1: kc.surface_exact(rng, 420, 28)}, rng))
    x = ME.SparseTensor(features=torch.randn(len(C), D + 6, device="cuda") * 0.3, coordinates=C)
    m.eval()
    with torch.no_grad():
        e = m(x)
    exp = sparse.affinity_pool(ME.SparseTensor(features=x.F[:, :D], coordinates=C), e, K=24, num_iters=3)
    for training in (True, False):
        m.train(training)
        got = sparse.purify(m, x, feature_dim=D, K=24, num_iters=3)
        assert m.training is training
        assert got.F.shape == (len(C), D) and got.C is x.C
        assert torch.equal(got.F.view(torch.int32), exp.F.view(torch.int32))
    assert bool((exp.F - x.F[:, :D]).abs().max() > 1e-3)                           # (the pooling did something)
