"""Shared inputs, numpy models and fp64 references for the backward of the purifying step (sparse.affinity_pool(differentiable=True),
ops.pool_transpose_build / pool_ell_transpose / pool_ell_wgrad / affinity_softmax_backward / l2norm_rows_backward).

A case is a GradCase: C int32 [N,4] = batch, x, y, z, X fp32 [N,D] features, E fp32 [N,d] embeddings, K neighbours, T applications,
the sharpening factor and the normalisation flag.  Every array comes from a fixed seed.

The REFERENCE is torch autograd in float64 on the CPU, per batch entry, on the oracle's lists (knn_batched_cases.oracle_lists_of): the
weights of oracle.affinity.affinity_weights on F.normalize'd rows, the operator as a dense [n,n] matrix built by `scatter` of the
weights (differentiable, a few MB per entry), applied T times; the loss is (Y * R).sum() with a fixed random R.

The cases are the smallest at which each kernel can go wrong:
  star     in-degree 0 (six voxels far outside a 3x3x3 cube) and in-degree >= 2K (a cube voxel), two entries
  widths   D = 4, 10 (padded to 12 inside), 256 (one full slab), 260 (a second slab with one active lane), 512; d = 16 and 128
  k_edges  K = 1, 8, 9 (across the unroll of 8) and 127 (every row of the entry in every list)
  iters    T = 0, 1, 2, 19 on knn_batched_cases.pool_case() at D = 64, K = 96, and D = 512 at T = 19
  flags    a two-entry base for the requires_grad / SparseTensor / normalize=False / fp16 variants
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import knn_batched_cases as kc
from oracle import affinity as o_aff


class GradCase:
    def __init__(self, name, C, X, E, K, T, sharpen=20.0, normalize=True):
        self.name, self.K, self.T, self.sharpen, self.normalize = name, K, T, sharpen, normalize
        self.C = np.ascontiguousarray(C, dtype=np.int32)
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.E = np.ascontiguousarray(E, dtype=np.float32)
        for a in (self.C, self.X, self.E):
            a.setflags(write=False)

    @property
    def N(self):
        return len(self.C)

    @property
    def D(self):
        return self.X.shape[1]

    @property
    def R(self):
        """the fixed random weights of the loss (Y * R).sum(), fp64 [N,D]"""
        return _loss_weights(self.name, self.N, self.D)


@functools.lru_cache(maxsize=None)
def _loss_weights(name, n, d):
    import zlib
    r = np.random.default_rng(zlib.crc32(name.encode())).standard_normal((n, d))
    r.setflags(write=False)
    return r


def _features(rng, n, D, d):
    """features ~ N(0,1); embeddings with row norms between 0.5 and 3 (the normalisation's backward has something to do)"""
    X = rng.standard_normal((n, D))
    E = rng.standard_normal((n, d)) * rng.uniform(0.5, 3.0, (n, 1)) / np.sqrt(d)
    return X, E


# ------------------------------------------------------------------------------------------ the cases
STAR_K = 8


def _star():
    """entry 0: a 3x3x3 cube and six voxels at (1,1,1) +- 3000 along each axis, rows in construction order; entry 1: 40 surface voxels"""
    rng = np.random.default_rng(301)
    far = np.array([[1, 1, 1]] * 6) + 3000 * np.vstack([np.eye(3, dtype=int), -np.eye(3, dtype=int)])
    e0 = np.vstack([kc.cube(3), far])
    e1 = kc.surface_exact(rng, 40, 12)
    C = np.vstack([np.c_[np.zeros(len(e0), int), e0], np.c_[np.ones(len(e1), int), e1]])
    X, E = _features(rng, len(C), 8, 16)
    return GradCase("star", C, X, E, STAR_K, 2)


WIDTHS_D = (4, 10, 256, 260, 512)
WIDTHS_d = (16, 128)


def _widths(D, d):
    def make():
        rng = np.random.default_rng(302)
        C = kc.batched({0: kc.surface_exact(rng, 130, 16)}, rng)
        X, E = _features(np.random.default_rng(3020 + D + d), len(C), D, d)
        return GradCase(f"widths_D{D}_d{d}", C, X, E, 7, 3)
    return make


K_EDGES = (1, 8, 9, 127)


def _k_edges(K):
    def make():
        rng = np.random.default_rng(303)
        C = kc.batched({0: kc.surface_exact(rng, 128, 16)}, rng)
        X, E = _features(rng, len(C), 12, 32)
        return GradCase(f"k_edges_K{K}", C, X, E, K, 1)
    return make


ITERS_T = (0, 1, 2, 19)


def _iters(D, T):
    def make():
        C, X, E = kc.pool_case()
        return GradCase(f"iters_D{D}_T{T}", C, X[:, :D], E * 2.5, 96, T)
    return make


def _flags(normalize):
    def make():
        rng = np.random.default_rng(304)
        C = kc.batched({0: kc.surface_exact(rng, 60, 12), 2: kc.surface_exact(rng, 70, 12)}, rng)
        X, E = _features(rng, len(C), 12, 32)
        if not normalize:
            E = E / np.linalg.norm(E, axis=1, keepdims=True)
        X = X.astype(np.float16).astype(np.float32)                  # exact in fp16: the fp16 variant shares the reference
        return GradCase("flags" if normalize else "flags_plain", C, X, E, 8, 3, normalize=normalize)
    return make


CASES = {"star": _star}
CASES.update({f"widths_D{D}_d{d}": _widths(D, d) for D in WIDTHS_D for d in WIDTHS_d})
CASES.update({f"k_edges_K{K}": _k_edges(K) for K in K_EDGES})
CASES.update({f"iters_D64_T{T}": _iters(64, T) for T in ITERS_T})
CASES["iters_D512_T19"] = _iters(512, 19)
CASES["flags"] = _flags(True)
CASES["flags_plain"] = _flags(False)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def lists(name):
    """the oracle's lists of the case, int64 [N,K] of input rows"""
    c = case(name)
    nbr = kc.oracle_lists_of(c.C, c.K)
    assert nbr.min() >= 0
    nbr.setflags(write=False)
    return nbr


# ------------------------------------------------------------------------------------------ the inverted index
def inverted_index(nbr, n):
    """numpy model of gp_pool_transpose_build -> (tr_off int64 [n+1], tr_slot int32 [n*K]): in-degree count, exclusive scan, stable
    sort of the flat slots by their neighbour id.  Ids outside 0..n-1 sort behind every list."""
    flat = np.asarray(nbr).reshape(-1).astype(np.int64)
    key = np.where((flat >= 0) & (flat < n), flat, n)
    count = np.bincount(key, minlength=n + 1)[:n]
    tr_off = np.zeros(n + 1, np.int64)
    np.cumsum(count, out=tr_off[1:])
    tr_slot = np.argsort(key, kind="stable").astype(np.int32)
    return tr_off, tr_slot


def inverted_index_brute(nbr, n):
    """for every destination row the slots that name it, by search"""
    flat = np.asarray(nbr).reshape(-1)
    return [np.flatnonzero(flat == m) for m in range(n)]


def in_degrees(nbr, n):
    return np.bincount(np.asarray(nbr).reshape(-1), minlength=n)


# ------------------------------------------------------------------------------------------ the reference: torch autograd, fp64
def _entries(C):
    for b in np.unique(C[:, 0]):
        yield np.flatnonzero(C[:, 0] == b)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict: Y fp64 [N,D], dX fp64 [N,D], dE fp64 [N,d] (zeros when T = 0), w fp64 [N,K], all in the input's row order"""
    c = case(name)
    nbr = lists(name)
    X = torch.from_numpy(c.X.astype(np.float64)).requires_grad_()
    E = torch.from_numpy(c.E.astype(np.float64)).requires_grad_()
    R = torch.from_numpy(np.array(c.R))
    Y = torch.zeros_like(X)
    W = np.zeros((c.N, c.K))
    loss = torch.zeros((), dtype=torch.float64)
    for idx in _entries(c.C):
        n = len(idx)
        inv = np.full(c.N, -1, np.int64)
        inv[idx] = np.arange(n)
        nb = torch.from_numpy(inv[nbr[idx]])
        assert int(nb.min()) >= 0
        rows = torch.from_numpy(idx)
        e = E[rows]
        if c.normalize:
            e = F.normalize(e, p=2, dim=1, eps=1e-12)
        w = o_aff.affinity_weights(e, nb, c.sharpen)
        P = torch.zeros((n, n), dtype=torch.float64).scatter(1, nb, w)
        y = X[rows]
        for _ in range(c.T):
            y = P @ y
        loss = loss + (y * R[rows]).sum()
        Y[idx] = y.detach()
        W[idx] = w.detach().numpy()
    dX, dE = torch.autograd.grad(loss, (X, E), allow_unused=True)
    out = {"Y": Y.numpy(), "dX": dX.numpy(), "dE": np.zeros_like(c.E, dtype=np.float64) if dE is None else dE.numpy(), "w": W}
    for a in out.values():
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------ the closed form the kernels implement
def closed_form(X, E, nbr, T, sharpen, normalize, R):
    """numpy fp64, all rows at once (the lists never cross entries) -> dict Y, dX, dE, w, dw, da:
        u_i = e_i / max(|e_i|, 1e-12);  w_ij = softmax_j(s <u_i, u_n(i,j)>);  X_t[i] = sum_j w_ij X_{t-1}[n(i,j)]
        G_T = R;  dw_ij += <G_t[i], X_{t-1}[n(i,j)]>;  G_{t-1}[m] = sum_{(i,j): n(i,j) = m} w_ij G_t[i]   (through the inverted index)
        da_ij = s w_ij (dw_ij - sum_k w_ik dw_ik);  du_i = sum_j da_ij u_n(i,j) + sum_{(r,j): n(r,j) = i} da_rj u_r
        de_i = (du_i - u_i <u_i, du_i>) / |e_i|   (du_i / 1e-12 where |e_i| < 1e-12; du_i itself without the normalisation)"""
    X, E, R = (np.asarray(a, dtype=np.float64) for a in (X, E, R))
    n, K = nbr.shape
    norm = np.linalg.norm(E, axis=1, keepdims=True)
    u = E / np.maximum(norm, 1e-12) if normalize else E
    sim = np.stack([(u * u[nbr[:, j]]).sum(1) for j in range(K)], 1) * sharpen
    w = np.exp(sim - sim.max(1, keepdims=True))
    w /= w.sum(1, keepdims=True)
    P = np.zeros((n, n))
    P[np.arange(n)[:, None], nbr] = w                                  # (ids are distinct inside a list)
    Xs = [X]
    for _ in range(T):
        Xs.append(P @ Xs[-1])
    tr_off, tr_slot = inverted_index(nbr, n)
    assert tr_off[n] == n * K
    dest, src = np.repeat(np.arange(n), np.diff(tr_off)), tr_slot // K

    def transposed(values):                                            # the matrix with [m, i] = values[i, j] where n(i,j) = m (ids are distinct inside a list)
        M = np.zeros((n, n))
        M[dest, src] = values.reshape(-1)[tr_slot]
        return M

    PT = transposed(w)
    G, dw = R, np.zeros((n, K))
    for t in range(T, 0, -1):
        dw += np.take_along_axis(G @ Xs[t - 1].T, nbr, 1)             # <G[i], X_{t-1}[n(i,j)]>
        G = PT @ G
    da = sharpen * w * (dw - (w * dw).sum(1, keepdims=True))
    du = sum(da[:, j:j + 1] * u[nbr[:, j]] for j in range(K)) + transposed(da) @ u
    if normalize:
        safe = np.maximum(norm, 1e-12)
        de = np.where(norm < 1e-12, du / 1e-12, (du - u * (u * du).sum(1, keepdims=True)) / safe)
    else:
        de = du
    return {"Y": Xs[-1], "dX": G, "dE": de, "w": w, "dw": dw, "da": da}
