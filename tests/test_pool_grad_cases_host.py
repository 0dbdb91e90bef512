"""The cases of tests/pool_grad_cases.py on the host: the numpy model of the inverted index against a brute-force transpose of every
case's lists, the closed-form backward the kernels implement (numpy fp64) against torch autograd of the dense formulation, and the
in-degrees the `star` case is built for.  No GPU."""
import numpy as np
import pytest

import pool_grad_cases as gc

REL = 1e-10


@pytest.mark.parametrize("name", list(gc.CASES))
def test_inverted_index_model_equals_the_brute_force_transpose(name):
    c = gc.case(name)
    nbr = gc.lists(name)
    tr_off, tr_slot = gc.inverted_index(nbr, c.N)
    assert tr_off[0] == 0 and tr_off[c.N] == c.N * c.K and tr_slot.dtype == np.int32
    assert np.array_equal(np.diff(tr_off), gc.in_degrees(nbr, c.N))                  # counting
    brute = gc.inverted_index_brute(nbr, c.N)
    for m in range(c.N):
        got = tr_slot[tr_off[m]:tr_off[m + 1]]
        assert np.array_equal(got, brute[m]), m                                       # the slots that name m, ascending (stable order)
    assert np.array_equal(np.sort(tr_slot), np.arange(c.N * c.K))                     # every slot once


def test_inverted_index_model_puts_foreign_ids_behind_the_lists():
    nbr = np.array([[1, -1], [0, 7], [0, 1]])
    tr_off, tr_slot = gc.inverted_index(nbr, 3)
    assert tr_off.tolist() == [0, 2, 4, 4]
    assert tr_slot.tolist() == [2, 4, 0, 5, 1, 3]


def _rel(got, ref):
    scale = np.abs(ref).max()
    return np.abs(got - ref).max() / scale if scale else np.abs(got).max()


@pytest.mark.parametrize("name", list(gc.CASES))
def test_closed_form_backward_equals_autograd_of_the_dense_formulation(name):
    c = gc.case(name)
    ref = gc.reference(name)
    got = gc.closed_form(c.X, c.E, gc.lists(name), c.T, c.sharpen, c.normalize, c.R)
    for what in ("Y", "dX", "dE", "w"):
        err = _rel(got[what], ref[what])
        print(f"{name} {what}: max |closed form - autograd| / max |autograd| = {err:.2e}")
        assert err <= REL, (what, err)
    if c.T == 0:
        assert not ref["dE"].any() and not got["dE"].any() and np.array_equal(got["dX"], c.R)


def test_closed_form_clamps_a_zero_row_like_f_normalize():
    """a row below the 1e-12 clamp: the plain 1 / 1e-12 scaling, no projection (F.normalize's autograd)"""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    E = rng.standard_normal((6, 4))
    E[2] = 0.0
    nbr = np.array([[(i + 1) % 6, (i + 2) % 6] for i in range(6)])
    X, R = rng.standard_normal((6, 3)), rng.standard_normal((6, 3))
    got = gc.closed_form(X, E, nbr, 2, 20.0, True, R)
    Et, Xt = torch.tensor(E, requires_grad=True), torch.tensor(X)
    u = F.normalize(Et, dim=1, eps=1e-12)
    w = torch.softmax(20.0 * (u[:, None, :] * u[torch.from_numpy(nbr)]).sum(-1), 1)
    P = torch.zeros((6, 6), dtype=torch.float64).scatter(1, torch.from_numpy(nbr), w)
    ((P @ (P @ Xt)) * torch.tensor(R)).sum().backward()
    assert _rel(got["dE"], Et.grad.numpy()) <= REL


def test_star_in_degrees():
    c = gc.case("star")
    deg = gc.in_degrees(gc.lists("star"), c.N)
    far = np.flatnonzero((c.C[:, 0] == 0) & (np.abs(c.C[:, 1:] - 1).max(1) > 1000))
    assert len(far) == 6 and not deg[far].any()
    assert deg.min() == 0 and deg.max() >= 2 * c.K, (deg.min(), deg.max())
    print(f"star: in-degree min {deg.min()}, max {deg.max()} at K = {c.K}")
