"""Cases for sparse.segment_loss -- the classification cross-entropy of SparseTensor rows against text embeddings -- as numpy arrays,
with two references on the fp32 inputs:

  reference(name)    torch autograd in fp64 on the CPU over the dense formulation (F.normalize-style rows, all logits, cross_entropy
                     per item, the weights of the reduction);
  closed_form(name)  a numpy fp64 restatement of the closed form the kernels implement (dz = w (m softmax - cnt), du = s dz t, the
                     backward of the row normalisation); test_segment_loss_cases_host.py proves it against the first.

A case: F fp32 [N,D], batch int32 [N] (the coordinates' batch column), text fp32 [C,D] (not unit: the loss normalises), s, labels
int64 [N] per voxel or [P] per point with inv int64 [P], ignore, reduction.  Both references are computed once per case and shared.
"""
import functools

import numpy as np
import torch

from geopurify_amd import ops


class Case:
    def __init__(self, name, F, batch, text, s, labels, inv, ignore, reduction):
        self.name, self.F, self.batch, self.text, self.s = name, F, batch, text, float(s)
        self.labels, self.inv, self.ignore, self.reduction = labels, inv, tuple(ignore), reduction
        for a in (F, batch, text, labels) + ((inv,) if inv is not None else ()):
            a.setflags(write=False)

    @property
    def N(self):
        return self.F.shape[0]

    @property
    def D(self):
        return self.F.shape[1]

    @property
    def C(self):
        return self.text.shape[0]

    @property
    def B(self):
        return int(self.batch.max()) + 1

    def coordinates(self):
        """int32 [N,4]: the batch column and distinct cells (the loss reads the batch column only)"""
        c = np.zeros((self.N, 4), np.int32)
        c[:, 0] = self.batch
        c[:, 1] = np.arange(self.N) % 97
        c[:, 2] = np.arange(self.N) // 97
        return c

    def rows(self):
        return np.arange(self.N) if self.inv is None else self.inv

    def grad_scale(self):
        """the natural size of a gradient row, s / |y_i| at the shortest non-zero row (w m <= 1, |dz| <= 2 w m): what a gradient that
        is analytically zero -- D = 1, one class -- is small against, where the fp64 reference holds its own rounding noise only"""
        norm = np.linalg.norm(self.F.astype(np.float64), axis=1)
        return self.s / norm[norm > 0].min() if (norm > 0).any() else self.s

    def valid(self):
        """bool per item: the label inside 0..C-1 and not ignored, the row not a zero row"""
        l = self.labels
        zero = np.abs(self.F.astype(np.float64)).sum(1) == 0
        return (l >= 0) & (l < self.C) & ~np.isin(l, self.ignore) & ~zero[self.rows()]

    def weights(self):
        """(w per item -- 0 for invalid ones --, valid items per entry int64 [B])"""
        v = self.valid()
        b = self.batch[self.rows()]
        Vb = np.bincount(b[v], minlength=self.B).astype(np.int64)
        if not v.any():
            return np.zeros(len(v)), Vb
        if self.reduction == "item":
            w = np.full(len(v), 1.0 / v.sum())
        else:
            w = 1.0 / ((Vb > 0).sum() * np.maximum(Vb[b], 1).astype(np.float64))
        return np.where(v, w, 0.0), Vb


def _text(rng, C, D):
    return (rng.standard_normal((C, D)) * 3.0).astype(np.float32)


def make(name, N=300, D=32, C=19, s=14.3, B=3, seed=0, reduction="item", ignore=(255,), points=0, zero_rows=6, odd_labels=True,
         collinear=0, entries=None, scale=1.0):
    """N rows in B entries (or the batch indices `entries`); rows = a random multiple of a text row + noise; zero_rows all-zero rows;
    collinear rows that are exact multiples of a text row; labels random with (odd_labels) a tenth of them -100 / C / 255 / the second
    ignore id; points > 0: that many points spread over the voxels (every voxel but the last gets at least one when points >= N)."""
    rng = np.random.default_rng(1000 + seed)
    text = _text(rng, C, D)
    tn = text / np.linalg.norm(text, axis=1, keepdims=True)
    want = rng.integers(0, C, N)
    F = (rng.uniform(0.2, 2.0, (N, 1)) * tn[want] + 0.3 / np.sqrt(D) * rng.standard_normal((N, D))).astype(np.float32)
    if collinear:
        F[:collinear] = (np.float32(1.7) * tn[want[:collinear]]).astype(np.float32)
    if zero_rows and N > zero_rows:
        F[rng.choice(N, zero_rows, replace=False)] = 0.0
    F = (F * np.float32(scale)).astype(np.float32)
    ids = np.arange(B) if entries is None else np.asarray(entries)
    batch = ids[rng.integers(0, len(ids), N)].astype(np.int32)
    if N >= len(ids):
        batch[:len(ids)] = ids                                               # every listed entry is present
    inv = None
    items = N
    if points:
        items = points
        inv = rng.integers(0, max(N - 1, 1), points).astype(np.int64)        # (the last voxel holds no point)
        if points >= N - 1:
            inv[:N - 1] = np.arange(N - 1)
        inv = inv[rng.permutation(points)]
    rows = np.arange(N) if inv is None else inv
    labels = np.where(rng.random(items) < 0.6, want[rows], rng.integers(0, C, items)).astype(np.int64)
    if odd_labels:
        r = rng.random(items)
        odd = [-100, C, 255] + [i for i in ignore if i != 255]
        for k, v in enumerate(odd):
            labels[(r >= 0.03 * k) & (r < 0.03 * (k + 1))] = v
    return Case(name, F, batch, text, s, labels, inv, ignore, reduction)


def _voxel_of_1000():
    """40 voxels, voxel 7 holds 1000 points with mixed labels, voxel 11 none, the others a few"""
    c = make("voxel_1000_points", N=40, D=32, C=19, B=2, seed=31, points=200, zero_rows=2, reduction="entry")
    rng = np.random.default_rng(77)
    inv = np.concatenate([np.where(c.inv == 11, 12, c.inv), np.full(1000, 7, np.int64)])
    labels = np.concatenate([c.labels, rng.integers(0, 19, 1000)])
    labels[-50:] = 255
    p = rng.permutation(len(inv))
    F = c.F.copy()
    F[7] = F[8] + np.float32(0.01)                                            # (voxel 7 must not be a zero row)
    return Case(c.name, F, c.batch.copy(), c.text.copy(), c.s, labels[p].copy(), inv[p].copy(), c.ignore, c.reduction)


def _entry_all_invalid(reduction):
    c = make(f"entry_all_invalid_{reduction}", N=200, B=3, seed=41, reduction=reduction)
    labels = c.labels.copy()
    labels[c.batch == 1] = 255
    return Case(c.name, c.F.copy(), c.batch.copy(), c.text.copy(), c.s, labels, None, c.ignore, reduction)


def _no_valid(points):
    c = make("no_valid_points" if points else "no_valid", N=70, B=2, seed=43, points=points)
    labels = np.where(np.arange(len(c.labels)) % 2 == 0, 255, -100).astype(np.int64)
    return Case(c.name, c.F.copy(), c.batch.copy(), c.text.copy(), c.s, labels, None if c.inv is None else c.inv.copy(), c.ignore, c.reduction)


def _rounded(dtype):
    """points_item with its features rounded to a 16-bit dtype: what an fp16 / bf16 y.F holds"""
    c = make("points_item", **_SPECS["points_item"])
    F = torch.from_numpy(c.F.copy()).to(dtype).float().numpy()
    return Case(f"points_item_{str(dtype).split('.')[-1]}", F, c.batch.copy(), c.text.copy(), c.s, c.labels.copy(), c.inv.copy(), c.ignore,
                c.reduction)


# the GEMM's row tile, column padding and channel step, the row kernel's per-lane column step: asked of the library, so that the edge
# cases below sit at the kernels' real boundaries
ROW_TILE, COL_PAD, K_PAD = ops.sparse_conv_tiles()
COL_STEP = ops.segment_loss_col_step()

_SPECS = {}
for _C in (1, 2, 19, 160, 200, COL_STEP - 1, COL_STEP, COL_STEP + 1, COL_PAD - 1, COL_PAD, COL_PAD + 1):
    _SPECS[f"C{_C}"] = dict(N=150, D=32, C=_C, seed=_C)
_SPECS["C4096"] = dict(N=130, D=32, C=4096, seed=4096, s=30.0)
for _D in (1, 4, 10, 31, 32, 33, 512, 768, 1024):
    _SPECS[f"D{_D}"] = dict(N=140, D=_D, C=19, seed=100 + _D, points=300 if _D in (10, 512) else 0)
for _N in (1, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1):
    _SPECS[f"N{_N}"] = dict(N=_N, D=32, C=19, seed=200 + _N, zero_rows=0 if _N == 1 else 3, odd_labels=_N != 1, B=1 if _N == 1 else 2)
for _s in (1.0, 14.3, 100.0):
    _SPECS[f"s{_s:g}_collinear"] = dict(N=200, D=64, C=20, s=_s, seed=300 + int(_s), collinear=40, points=500, reduction="entry")
_SPECS["entry_reduction"] = dict(N=400, D=48, C=19, B=4, seed=51, reduction="entry")
_SPECS["points_item"] = dict(N=350, D=32, C=19, B=3, seed=52, points=1200)
_SPECS["ignore_255_2"] = dict(N=300, D=32, C=19, B=2, seed=53, ignore=(255, 2))
_SPECS["absent_entries"] = dict(N=200, D=32, C=19, seed=54, entries=(0, 2, 5), reduction="entry")
_SPECS["batch_65535"] = dict(N=120, D=32, C=19, seed=55, entries=(0, 65535), reduction="entry")
_SPECS["product_classes"] = dict(N=1500, D=512, C=200, B=4, seed=56, points=4000, reduction="entry")
_SPECS["small_rows"] = dict(N=200, D=64, C=20, seed=57, scale=1e-3)
_SPECS["large_rows"] = dict(N=200, D=64, C=20, seed=57, scale=1e3)
_SPECS["unit_scale_rows"] = dict(N=200, D=64, C=20, seed=57)

_BUILDERS = {"voxel_1000_points": _voxel_of_1000, "entry_all_invalid_item": lambda: _entry_all_invalid("item"),
             "entry_all_invalid_entry": lambda: _entry_all_invalid("entry"), "no_valid": lambda: _no_valid(0),
             "no_valid_points": lambda: _no_valid(150), "points_item_float16": lambda: _rounded(torch.float16),
             "points_item_bfloat16": lambda: _rounded(torch.bfloat16)}

CASES = list(_SPECS) + list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]() if name in _BUILDERS else make(name, **_SPECS[name])


class Result:
    """loss float, dY fp64 [N,D], per_entry fp64 [B] (NaN without valid items), valid int64 [B], lse fp64 [N], z_max = max |z|"""

    def __init__(self, loss, dY, per_entry, valid, lse, z_max):
        self.loss, self.dY, self.per_entry, self.valid, self.lse, self.z_max = loss, dY, per_entry, valid, lse, z_max


def _per_entry(c, ce, v, Vb):
    b = c.batch[c.rows()]
    sums = np.bincount(b[v], weights=ce[v], minlength=c.B)
    return np.where(Vb > 0, sums / np.maximum(Vb, 1), np.nan)


@functools.lru_cache(maxsize=None)
def reference(name):
    """torch fp64 autograd on the CPU over the dense formulation"""
    c = case(name)
    y = torch.tensor(c.F.astype(np.float64), requires_grad=True)
    t = torch.nn.functional.normalize(torch.tensor(c.text.astype(np.float64)), dim=-1)
    u = y / y.norm(dim=1, keepdim=True).clamp_min(1e-12)
    z = c.s * u @ t.T
    rows = torch.from_numpy(np.array(c.rows()))
    v = c.valid()
    w, Vb = c.weights()
    target = torch.from_numpy(np.where(v, c.labels, 0))
    ce = torch.nn.functional.cross_entropy(z[rows], target, reduction="none")
    loss = (ce * torch.from_numpy(w))[torch.from_numpy(v)].sum()
    if v.any():
        loss.backward()
        dY = y.grad.numpy()
    else:
        dY = np.zeros_like(c.F, dtype=np.float64)
    zz = z.detach()
    return Result(float(loss.detach()), dY, _per_entry(c, ce.detach().numpy(), v, Vb), Vb, torch.logsumexp(zz, 1).numpy(), float(zz.abs().max()))


@functools.lru_cache(maxsize=None)
def closed_form(name):
    """the closed form of the kernels in numpy fp64"""
    c = case(name)
    y = c.F.astype(np.float64)
    t = c.text.astype(np.float64)
    t = t / np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-12)
    raw = np.linalg.norm(y, axis=1, keepdims=True)
    nrm = np.maximum(raw, 1e-12)
    u = y / nrm
    z = c.s * u @ t.T
    mx = z.max(1, keepdims=True)
    e = np.exp(z - mx)
    lse = mx[:, 0] + np.log(e.sum(1))
    sm = e / e.sum(1, keepdims=True)
    rows, v = c.rows(), c.valid()
    w, Vb = c.weights()
    cnt = np.zeros((c.N, c.C))
    np.add.at(cnt, (rows[v], c.labels[v]), 1.0)
    m = cnt.sum(1)
    ce = lse[rows] - z[rows, np.where(v, c.labels, 0)]
    loss = float((w * ce)[v].sum())
    w_row = np.zeros(c.N)
    w_row[rows[v]] = w[v]                                                     # (one weight per entry: every item of a row has its row's)
    dz = w_row[:, None] * (m[:, None] * sm - cnt)
    du = c.s * dz @ t
    dY = np.where(raw >= 1e-12, (du - u * (u * du).sum(1, keepdims=True)) / nrm, du / 1e-12)
    return Result(loss, dY, _per_entry(c, ce, v, Vb), Vb, lse, float(np.abs(z).max()))
