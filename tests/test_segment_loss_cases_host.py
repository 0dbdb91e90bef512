"""The references of tests/segment_loss_cases.py agree with each other on the host: the closed form the kernels implement
(dz = w (m softmax - cnt), du = s dz t, the backward of the row normalisation) equals torch's fp64 autograd of the dense formulation,
on every case -- and sparse.segment_loss has no CPU path."""
import numpy as np
import pytest
import torch

import segment_loss_cases as lc

TOL = 1e-10


@pytest.mark.parametrize("name", lc.CASES)
def test_closed_form_equals_autograd(name):
    ref, got = lc.reference(name), lc.closed_form(name)
    scale = max(1.0, abs(ref.loss))
    assert abs(got.loss - ref.loss) <= TOL * scale, (got.loss, ref.loss)
    # relative to the gradient's maximum; only where the gradient is analytically zero (D = 1, one class, no valid item), and the
    # reference's maximum is its own rounding noise, to the natural size of a gradient row
    top, natural = float(np.abs(ref.dY).max()), lc.case(name).grad_scale()
    gmax = top if top > 1e-10 * natural else natural
    assert gmax == top or name in ("D1", "C1", "no_valid", "no_valid_points"), name
    assert float(np.abs(got.dY - ref.dY).max()) <= TOL * gmax
    assert np.array_equal(got.valid, ref.valid)
    assert np.array_equal(np.isnan(got.per_entry), np.isnan(ref.per_entry)) and np.array_equal(np.isnan(ref.per_entry), ref.valid == 0)
    ok = ~np.isnan(ref.per_entry)
    assert np.allclose(got.per_entry[ok], ref.per_entry[ok], rtol=TOL, atol=TOL)


def test_cases_cover_their_edges():
    """what the GPU tests rely on: zero rows, a voxel without points, a voxel of 1000 points, an entry without valid items, absent
    entries, labels of every invalid kind"""
    c = lc.case("voxel_1000_points")
    per_row = np.bincount(c.inv, minlength=c.N)
    assert per_row[7] >= 1000 and per_row[11] == 0 and len(set(c.labels[c.inv == 7].tolist())) > 5
    c = lc.case("entry_all_invalid_entry")
    assert lc.reference(c.name).valid[1] == 0 and np.isnan(lc.reference(c.name).per_entry[1])
    c = lc.case("absent_entries")
    assert set(c.batch.tolist()) == {0, 2, 5} and list(lc.reference(c.name).valid[[1, 3, 4]]) == [0, 0, 0]
    assert lc.case("batch_65535").B == 65536
    c = lc.case("ignore_255_2")
    assert {-100, c.C, 255, 2} <= set(c.labels.tolist()) and (np.abs(c.F).sum(1) == 0).sum() == 6
    for name in ("no_valid", "no_valid_points"):
        assert lc.reference(name).loss == 0.0 and not lc.reference(name).dY.any()
    # one class: the loss and the gradient are exactly zero in any arithmetic
    assert lc.closed_form("C1").loss == 0.0 and not lc.closed_form("C1").dY.any()


def test_segment_loss_has_no_cpu_path():
    from geopurify_amd import sparse

    class ST:
        def __init__(self, features, coordinates):
            self.F, self.C = features, coordinates

    c = lc.case("C19")
    y = ST(torch.from_numpy(c.F.copy()), torch.from_numpy(c.coordinates()))
    with pytest.raises(ValueError, match="no CPU path"):
        sparse.segment_loss(y, torch.from_numpy(c.text.copy()), c.s, labels=torch.from_numpy(c.labels.copy()))
