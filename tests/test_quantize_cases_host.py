"""CPU side of the quantisation tests: the numpy oracle of tests/quantize_cases.py against a plain fp64 mean, the cases themselves,
the MinkowskiEngine stub's SparseTensor staying a data holder when no quantization mode is given, and the argument checks of
geopurify_amd.sparse.quantize, which fire before any kernel is launched (this file runs without a GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

import quantize_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ME():
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import MinkowskiEngine
    finally:
        sys.path.pop(0)
    return MinkowskiEngine


def test_cases_cover_the_shapes_they_claim():
    cs = qc.cases()
    assert [len(cs[f"n{n}"]) for n in (1, 255, 256, 257, 700)] == [1, 255, 256, 257, 700]
    assert qc.Oracle(cs["distinct700"]).nv == 700 and qc.Oracle(cs["identical700"]).nv == 1
    o = qc.Oracle(cs["segments2000"])
    assert 1800 <= o.n <= 2200 and set(np.unique(o.counts)) == {1, 2, 3, 4, 5}
    # some multi-row segment lies across a 256-row edge of the sorted rows (checked in the oracle's order as a sample of orders: with
    # ~700 voxels of 1..5 rows over 8 blocks no order avoids it)
    ends = np.cumsum(o.counts)
    assert any((e - 1) // 256 != (e - c) // 256 for e, c in zip(ends, o.counts))
    C = cs["batches_0_5_65535"]
    assert sorted(np.unique(C[:, 0])) == [0, 5, 65535]
    xyz0, xyz2 = {tuple(r) for r in C[C[:, 0] == 0, 1:]}, {tuple(r) for r in C[C[:, 0] == 65535, 1:]}
    assert xyz0 == xyz2 and {tuple(r) for r in C[C[:, 0] == 5, 1:]} & xyz0
    assert all((c[:, 1:] < 0).any() for c in cs.values())
    e = cs["extent65535_y"]
    assert int(e[:, 2].max()) - int(e[:, 2].min()) + 1 == 65535
    for c, axis in qc.rejected_cases().values():
        a = 1 + "xyz".index(axis)
        assert int(c[:, a].max()) - int(c[:, a].min()) + 1 == 65536


@pytest.mark.parametrize("name", ["n257", "identical700", "segments2000"])
@pytest.mark.parametrize("d", [3, 38])
def test_oracle_average_within_the_fp32_summation_bound_of_the_fp64_mean(name, d):
    """An n-term fp32 sum in any order is within (n - 1) * 2^-24 * sum|x| of the exact one (to first order), the division adds one
    rounding of 2^-24 relative: together below count * 2^-23 * mean|x|, derived, not measured."""
    C = qc.cases()[name]
    F = qc.features(name, len(C), d)
    o = qc.Oracle(C)
    got = o.average(F)
    assert got.dtype == np.float32
    bound = o.counts[:, None] * 2.0 ** -23 * o.mean_abs_f64(F)
    err = np.abs(got.astype(np.float64) - o.mean_f64(F))
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    single = o.counts == 1
    assert np.array_equal(got[single], F[o.unique_index[single]])                 # one row: the row itself


def test_oracle_label_rules():
    C = np.array([[0, 1, 1, 1], [0, 2, 2, 2], [0, 1, 1, 1], [0, 3, 3, 3], [0, 3, 3, 3], [0, 1, 1, 1]], np.int32)
    lab = np.array([4, 9, 4, 7, 8, 4])
    o = qc.Oracle(C)
    assert o.labels(lab, "first").tolist() == [4, 9, 7]
    assert o.labels(lab, "differ").tolist() == [4, 9, qc.IGNORE]
    assert o.labels(lab, "count").tolist() == [qc.IGNORE, 9, qc.IGNORE]
    perm = np.array([2, 0, 1])
    od = o.to_device_rows(o.coordinates[perm])
    assert np.array_equal(od.coordinates[od.inverse], C) and od.unique_index.tolist() == [3, 0, 1] and od.counts.tolist() == [2, 3, 1]


def test_sparse_tensor_without_a_mode_is_the_data_holder(ME):
    F = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    C = torch.tensor([[0, 1, 1, 1], [0, 1, 1, 1], [0, 2, 2, 2], [1, 1, 1, 1]], dtype=torch.int32)        # a duplicate row stays
    for kw in ({}, {"quantization_mode": ME.SparseTensorQuantizationMode.NO_QUANTIZATION}, {"quantization_mode": None}):
        x = ME.SparseTensor(features=F, coordinates=C, **kw)
        assert x.F is F and x.C is C and x.features is F and x.coordinates is C
        assert not hasattr(x, "inverse_mapping") and not hasattr(x, "unique_index")
    x = ME.SparseTensor(F, C)
    assert x.F is F and x.C is C
    x = ME.SparseTensor(features=F, coordinates=C, device="cpu", tensor_stride=1)
    assert torch.equal(x.F, F) and x.C is C
    assert [m.name for m in ME.SparseTensorQuantizationMode][:3] == ["NO_QUANTIZATION", "RANDOM_SUBSAMPLE", "UNWEIGHTED_AVERAGE"]


def test_unsupported_modes_raise_by_name(ME):
    F, C = torch.zeros(2, 3), torch.zeros(2, 4, dtype=torch.int32)
    for mode in (ME.SparseTensorQuantizationMode.UNWEIGHTED_SUM, ME.SparseTensorQuantizationMode.MAX_POOL,
                 ME.SparseTensorQuantizationMode.SPLAT_LINEAR_INTERPOLATION):
        with pytest.raises(NotImplementedError, match=mode.name):
            ME.SparseTensor(features=F, coordinates=C, quantization_mode=mode)


def test_quantize_rejects_bad_arguments_before_any_launch(ME):
    from geopurify_amd import sparse
    F, C = torch.zeros(5, 3), torch.zeros(5, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"quantize: coordinates, features and labels must be CUDA tensors \(got cpu / cpu / None\)"):
        sparse.quantize(C, F)
    with pytest.raises(ValueError, match=r"must be CUDA tensors \(got cpu / None / None\)"):
        sparse.quantize(C)
    with pytest.raises(ValueError, match=r"quantize: coordinates must be \[N, 4\] \(batch, x, y, z\), got \[5, 3\]"):
        sparse.quantize(C[:, :3], F)
    with pytest.raises(ValueError, match=r"quantize: coordinates must be \[N, 4\] \(batch, x, y, z\), got list"):
        sparse.quantize([[0, 0, 0, 0]], F)
    with pytest.raises(ValueError, match=r"quantize: coordinates must be integers or floating point, got torch.bool"):
        sparse.quantize(C.bool(), F)
    with pytest.raises(ValueError, match=r"quantize: features must be \[N, D\] with N = 5 coordinate rows, got \[4, 3\]"):
        sparse.quantize(C, F[:4])
    with pytest.raises(ValueError, match=r"quantize: features must be \[N, D\] with N = 5 coordinate rows, got \[5\]"):
        sparse.quantize(C, F[:, 0])
    with pytest.raises(ValueError, match=r"quantize: labels must be \[N\] with N = 5 coordinate rows, got \[5, 1\]"):
        sparse.quantize(C, F, torch.zeros(5, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"quantize: mode='sum'"):
        sparse.quantize(C, F, mode="sum")
    with pytest.raises(ValueError, match=r"quantize: collision='any'"):
        sparse.quantize(C, F, collision="any")
    # the stub hands the same checks on
    with pytest.raises(ValueError, match="must be CUDA tensors"):
        ME.SparseTensor(features=F, coordinates=C, quantization_mode=ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE)
    with pytest.raises(ValueError, match=r"sparse_quantize: coordinates must be \[N, 3\], got \[5, 4\]"):
        ME.utils.sparse_quantize(C)


def test_workspace_query_without_gpu():
    from geopurify_amd import _lib
    lib = _lib.load()
    n = 150000
    assert lib.gp_quantize_batched_workspace_bytes(n) >= n * (2 * 8 + 4 * 4)      # two key arrays, four row-sized int32 arrays
    assert lib.gp_quantize_batched_workspace_bytes(0) == 0 and lib.gp_quantize_batched_workspace_bytes(2 ** 31) == 0
    EINVAL = -22
    one = torch.zeros(64, dtype=torch.int64)
    p = one.data_ptr()
    assert lib.gp_quantize_batched(p, 0, p, p, p, p, p, p, p, 1 << 20, None) == EINVAL
    assert lib.gp_quantize_batched(p, 2 ** 31, p, p, p, p, p, p, p, 1 << 20, None) == EINVAL
    assert b"out of range" in lib.gp_last_error()
    assert lib.gp_segment_labels(p, 4, p, p, p, 5, 255, 1, p, None) == EINVAL            # nv > n
    assert lib.gp_segment_labels(p, 4, p, p, p, 2, 255, 3, p, None) == EINVAL            # no such rule
