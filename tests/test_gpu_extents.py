"""Extents of the C ABI (include/geopurify_hip.h): no entry point reads or writes outside the arrays the header gives it.

Every case runs its entry point twice, on plain, contiguous, exactly sized tensors and on fenced views (tests/extent_fence.py: the
same values with poisoned guard rows before and behind, poisoned pitch columns, workspaces at exactly the reported bytes), and asks:
  1. writes: every fence is intact after the call;
  2. reads:  the fenced call's outputs equal the plain call's bit for bit (a kernel that reads a guard gets a NaN or a wild index);
  3. values: the plain call's outputs against the fp64 oracle of that kernel, at the bound the kernel's own test uses (cited beside it);
  4. no element is excused: all guards, all in-extent elements.
The shapes sit at the kernels' row tiles (named beside each parametrisation): one row, one fewer and one more than a tile, a last
block of one row.  Voxel sets are prefixes of one surface_voxels set in Morton order, their kernel maps and kNN lists the oracle's.
Everything stays inside allocations of the test's own: nothing here can fault.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from extent_fence import INT_VIEW, POISON, Arena, assert_intact, bits, fence_in, fenced, run, unwritten
from lattice_cases import rcb_reference
from oracle import affinity as o_aff
from oracle import metric as o_metric
from oracle import student as o_student

pytestmark = pytest.mark.gpu

F16, F32, I32, I64, U8 = torch.float16, torch.float32, torch.int32, torch.int64, torch.uint8


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import ops as _ops
    from geopurify_amd import _lib
    _lib.load()                      # fails loudly if the HIP library is missing
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from geopurify_amd import _lib
    return _lib.load()


def ok(lib, rc):
    assert rc == 0, (rc, lib.gp_last_error().decode())


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def up(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)) if not torch.is_tensor(a) else a
    return (t.to(dtype) if dtype is not None else t).cuda().contiguous()


def whole(t, what):
    """an output that the call must write whole: no element still holds the poison it was allocated with"""
    assert unwritten(t) == 0, f"{what}: {unwritten(t)} elements were not written"


# ------------------------------------------------------------------------------------------ voxel sets
def surface_voxels(rng, n=4000, ext=60):
    a = np.c_[rng.integers(0, ext, n), rng.integers(0, ext, n), rng.integers(3, 5, n)]
    b = np.c_[rng.integers(0, ext, n // 2), np.full(n // 2, 17), rng.integers(0, 40, n // 2)]
    c = np.c_[rng.integers(0, ext, n // 2), (rng.integers(0, ext, n // 2) * 0.6).astype(int), np.zeros(n // 2, int)]
    c[:, 2] = (c[:, 0] * 0.5).astype(int) + 6                     # oblique sheet
    iso = np.array([[ext + 200, 5, 5], [ext + 330, 90, 41], [ext + 331, 90, 41]])   # isolated voxels
    v = np.unique(np.vstack([a, b, c, iso]), axis=0)
    return v[rng.permutation(len(v))].astype(np.int32)


def morton_perm(c):
    """gp_morton_order restated: rows by the bit interleave (x lowest) of coords - min; the codes of distinct voxels are distinct"""
    q = (c.astype(np.int64) - c.astype(np.int64).min(0)).astype(np.uint64)
    key = np.zeros(len(c), np.uint64)
    for b in range(21):
        for ax in range(3):
            key |= ((q[:, ax] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + ax)
    return np.argsort(key, kind="stable")


_GEO = {}


_SETS = {}


def voxel_prefix(nv):
    """The first nv voxels of the smallest (densest) surface_voxels set that holds nv: most cells of its sheets are taken, so a prefix
    keeps most of its face neighbours"""
    for ext in range(2, 64):
        if ext not in _SETS:
            _SETS[ext] = surface_voxels(np.random.default_rng(2024), 4000, ext)
        v = _SETS[ext]
        if len(v) >= nv:
            return v[:nv]
    raise ValueError(nv)


def geo(nv, K=0):
    """nv voxels (c, any order), in Morton order (cs), with the oracle's kernel map (nm, K == 0), its kNN lists (nbr: rows of cs,
    K > 0) or neither (K is None)."""
    if (nv, K) not in _GEO:
        c = voxel_prefix(nv)
        perm = morton_perm(c)
        cs = np.ascontiguousarray(c[perm])
        g = dict(c=c, perm=perm.astype(np.int32), cs=cs)
        if K:
            g["nbr"] = o_aff.knn_lattice(cs, K).to(I32)
        elif K == 0:
            g["nm"] = o_student.build_kernel_map(cs).astype(np.int32)
        _GEO[(nv, K)] = g
    return _GEO[(nv, K)]


def grid_of(ops, cs):
    g = ops.grid_build(up(cs))
    assert g.status() == 0
    return g


def unit_rows(n, d, seed):
    return F.normalize(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), dim=1)


# ------------------------------------------------------------------------------------------ gp_split_f16 / _scaled / gp_pow2_scale
def pow2_for(amax):
    """s = 2^k with amax * s in [2^13, 2^14) (exact: frexp's exponent)"""
    _, e = torch.frexp(amax)
    return torch.ldexp(torch.ones_like(amax), 14 - e)


def split_rows(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g) * torch.exp(torch.randn(n, 1, generator=g) * 2.0)


def split_error_ok(hi, lo, xs, what):
    """hi + lo against x * s in fp64.  From the formats: hi = RN16(v) leaves |v - hi| <= 2^-12 |v|, lo = RN16(v - hi) leaves
    2^-12 of that, 2^-24 |v| -- or half a subnormal step, 2^-25, where lo is subnormal.  The header states 2^-22 relative (normal
    lo) and 2^-25 absolute (subnormal lo); their sum bounds every element.  A bound from the number formats, not from an existing
    test: the one there is (test_sparse_conv_f16x3_matches_fp32_accuracy: hi + lo within 1e-6 of x, absolute) is looser at every
    magnitude these inputs have below 4."""
    err = (hi.double() + lo.double() - xs).abs()
    bound = 2.0 ** -22 * xs.abs() + 2.0 ** -25
    assert bool((err <= bound).all()), (what, float((err / bound).max()))


# elementwise kernels: 256 threads per workgroup (gp_split_f16: 4 columns per thread; the scaled kernel: a row per wave, 4 waves)
@pytest.mark.parametrize("n", [1, 3, 257])
@pytest.mark.parametrize("form", ["unscaled", "global_scale", "row_scale", "interleaved", "dst_row"])
def test_split_f16(ops, lib, form, n):
    d = 96                                                   # fp32 pitch 104, plane pitch 128, interleaved pitch 200
    X = split_rows(n, d, 100 + n)
    s_glob = pow2_for(X.abs().max())
    s_row = pow2_for(X.abs().max(dim=1).values)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).to(I32)

    def case(a):
        x = a.inp(X, 104, "x")
        o = {}
        if form == "interleaved":
            hi, lo = a.out((n, 2 * d), F16, 200, "rows"), None
        else:
            hi, lo = a.out((n, d), F16, 128, "hi"), a.out((n, d), F16, 128, "lo")
            o["lo"] = lo
        o["hi"] = hi
        if form == "unscaled":
            ok(lib, lib.gp_split_f16(P(x), x.stride(0), d, n, P(hi), P(lo), hi.stride(0), S()))
            return o
        scale = a.inp(s_glob.reshape(1), name="scale") if form == "global_scale" else None
        rinv = a.out(n, F32, name="row_inv_scale") if form != "global_scale" else None
        dst = a.inp(perm, name="dst_row") if form == "dst_row" else None
        ok(lib, lib.gp_split_f16_scaled(P(x), x.stride(0), d, n, P(hi), P(lo), hi.stride(0), P(scale), P(rinv), P(dst), S()))
        if rinv is not None:
            o["row_inv_scale"] = rinv
        return o

    r = run(case)
    for k, v in r.items():
        whole(v, k)
    hi, lo = (r["hi"], r["lo"]) if form != "interleaved" else ops.deinterleave_planes(r["hi"])
    hi, lo = hi.cpu(), lo.cpu()
    if form == "unscaled":
        s = torch.ones(n)
    elif form == "global_scale":
        s = s_glob.expand(n)
    else:
        s = s_row
        rinv = r["row_inv_scale"].cpu()
        if form == "dst_row":                                # row r of x lands in row dst_row[r] of every output
            hi, lo, rinv = hi[perm.long()], lo[perm.long()], rinv[perm.long()]
        assert torch.equal(rinv, 1.0 / s_row)                # powers of two: exact
    split_error_ok(hi, lo, X.double() * s.double()[:, None], form)


@pytest.mark.parametrize("n", [1, 3, 257])                  # 256 threads per workgroup, one atomic word of workspace
def test_pow2_scale(ops, lib, n):
    d = 96
    X = split_rows(n, d, 200 + n)

    def case(a):
        x = a.inp(X, 104, "x")
        s2, ws = a.out(2, F32, name="scale2"), a.out(4, U8, name="workspace")            # the header's 4 bytes
        ok(lib, lib.gp_pow2_scale(P(x), x.stride(0), d, n, P(s2), P(ws), 4, S()))
        return {"scale2": s2}

    s = pow2_for(X.abs().max())
    assert torch.equal(run(case)["scale2"].cpu(), torch.stack([s, 1.0 / s]))


# ------------------------------------------------------------------------------------------ gather / classify / scatter / l2norm
def label_rule(pred, rows, text, scale, what):
    """test_classify_and_iou's rule: labels exact where the fp64 oracle's top-2 margin exceeds 1e-4, at least 99 % of the rows inside it
    (checked here, on the CPU, in the oracle alone).  An all-zero row has 19 equal logits in any arithmetic: the header's "first max
    on ties" makes its label 0, exactly."""
    ref, logits = o_metric.classify(rows.double(), text.double(), scale)
    top2 = logits.topk(2, dim=1).values
    zero = rows.abs().sum(1) == 0
    safe = ((top2[:, 0] - top2[:, 1]) > 1e-4) | zero
    assert safe.double().mean() >= 0.99, what
    ref = torch.where(zero, torch.zeros_like(ref), ref)
    assert torch.equal(pred[safe], ref[safe]), what
    return zero


def gather_inputs(n, d, seed, m=40):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(m, d, generator=g)
    src[3] = 0.0
    index = torch.randint(0, m, (n,), generator=g)
    if n >= 15:
        index[7] = 5                                         # row_map[5] = 3 below: the all-zero row
    rmap = torch.randperm(m, generator=g).to(I32)
    at3, at5 = int((rmap == 3).nonzero()), int(rmap[5])
    rmap[5], rmap[at3] = 3, at5
    text = F.normalize(torch.randn(19, d, generator=g), dim=1)
    return src, index, rmap, text


# gather_rows_kernel: a row per wave, 4 rows per workgroup; the classifying forms: 16 points (d <= 512, 16 lanes per point) or
# 4 points (wider rows, a wave per point) per workgroup
@pytest.mark.parametrize("n", [1, 15, 17, 65])
@pytest.mark.parametrize("d", [64, 576])
@pytest.mark.parametrize("entry", ["gather_rows", "gather_rows_classify"])
def test_gather_rows(ops, lib, entry, d, n):
    src, index, rmap, text = gather_inputs(n, d, 300 + n + d)

    def case(a):
        s, ix, rm = a.inp(src, d + 8, "src"), a.inp(index, name="index"), a.inp(rmap, name="row_map")
        out = a.out((n, d), F32, d + 8, "out")
        if entry == "gather_rows":
            ok(lib, lib.gp_gather_rows(P(s), s.stride(0), d, P(ix), n, P(rm), P(out), out.stride(0), S()))
            return {"out": out}
        tx = a.inp(text, name="text_norm")
        pred, zero = a.out(n, I64, name="pred"), a.out(n, U8, name="zero_row")
        ok(lib, lib.gp_gather_rows_classify(P(s), s.stride(0), d, P(ix), n, P(rm), P(out), out.stride(0), P(tx), 19, 14.285, P(pred),
                                            P(zero), S()))
        return {"out": out, "pred": pred, "zero_row": zero}

    r = run(case)
    want = src[rmap.long()[index]]
    assert torch.equal(r["out"].cpu(), want)                 # a copy: exact
    if entry == "gather_rows_classify":
        zero = label_rule(r["pred"].cpu(), want, text, 14.285, (d, n))
        assert torch.equal(r["zero_row"].cpu().bool(), zero)


# classify16_lds_kernel / classify16_kernel: 16 points per workgroup (x 2 per group of the LDS form); classify_kernel: a wave per
# point, 4 points per workgroup; rows_argmax_kernel: the same
@pytest.mark.parametrize("n", [1, 15, 17, 65])
@pytest.mark.parametrize("form", ["lanes16_text_in_lds", "lanes16_plain", "one_wave", "rows_argmax"])
def test_classify_argmax(ops, lib, form, n):
    d = 96 if form == "one_wave" else 64                     # d % 64 != 0: the one-wave kernel
    g = torch.Generator().manual_seed(400 + n)
    feat = torch.randn(n, d, generator=g)
    if n >= 15:
        feat[4] = 0.0
    text = F.normalize(torch.randn(19, d, generator=g), dim=1)
    logits64 = 14.285 * F.normalize(feat.double(), dim=1) @ text.double().T
    logits = logits64.float()

    def case(a):
        f = a.inp(feat, d + 8, "feat")
        pred, zero = a.out(n, I64, name="pred"), a.out(n, U8, name="zero_row")
        if form == "rows_argmax":
            lg = a.inp(logits, 24, "logits")
            ok(lib, lib.gp_rows_argmax(P(lg), lg.stride(0), 19, n, P(f), f.stride(0), d, P(pred), P(zero), S()))
        else:
            tx = a.inp(text, name="text_norm")
            ok(lib, lib.gp_classify_argmax(P(f), f.stride(0), d, n, P(tx), 19, 14.285, P(pred), P(zero), S()))
        return {"pred": pred, "zero_row": zero}

    try:
        if form == "lanes16_plain":
            ok(lib, lib.gp_debug_set(14, 1))
        r = run(case)
    finally:
        ok(lib, lib.gp_debug_set(14, 0))
    if form == "rows_argmax":
        zero = feat.abs().sum(1) == 0
        assert torch.equal(r["pred"].cpu(), logits.argmax(1))           # the arg-max of given fp32 numbers (no ties among them): exact
    else:
        zero = label_rule(r["pred"].cpu(), feat, text, 14.285, (form, n))
    assert torch.equal(r["zero_row"].cpu().bool(), zero)


# scatter_mean_csr kernels: a voxel per wave, 4 voxels per workgroup; 41 voxels leave a last workgroup of one
@pytest.mark.parametrize("form", ["scalar_d6", "float4_d8", "row_map"])
def test_scatter_mean_csr(ops, lib, form):
    n, nv = 300, 41
    d, col0, width = (6, 4, 16) if form == "scalar_d6" else (8, 4, 16)
    g = torch.Generator().manual_seed(17)
    inv = torch.cat([torch.arange(nv), torch.randint(0, nv, (n - nv,), generator=g)])[torch.randperm(n, generator=g)]
    order = torch.sort(inv, stable=True).indices
    seg = torch.zeros(nv + 1, dtype=I64)
    seg[1:] = torch.bincount(inv, minlength=nv).cumsum(0)
    src = torch.randn(n, d, generator=g)
    rmap = torch.randperm(nv, generator=g).to(I32) if form == "row_map" else None

    def case(a):
        s, od, sg = a.inp(src, 8, "src"), a.inp(order, name="order"), a.inp(seg, name="seg_start")
        rm = a.inp(rmap, name="row_map") if rmap is not None else None
        out = a.out((nv, width), F32, 24, "out")
        ok(lib, lib.gp_scatter_mean_csr(P(s), s.stride(0), d, P(od), P(sg), nv, P(rm), P(out), out.stride(0), col0, S()))
        return {"out": out}

    out = run(case)["out"].cpu()
    ref = o_aff.scatter_mean(src, inv, nv)                   # test_scatter_mean_gather_bit_exact: the same summation order, bit exact
    rows = rmap.long() if rmap is not None else torch.arange(nv)
    assert torch.equal(out[rows][:, col0:col0 + d], ref)
    keep = torch.ones(width, dtype=torch.bool)
    keep[col0:col0 + d] = False                              # the columns outside [col0, col0 + d) of the written rows stay as they were
    assert bool((bits(out[:, keep]) == POISON["out"][F32]).all())


@pytest.mark.parametrize("n", [1, 257])                     # l2norm_rows_kernel: a row per wave, 4 rows per workgroup
def test_l2norm_rows_in_place(ops, lib, n):
    d = 96
    X = split_rows(n, d, 500 + n)

    def case(a):
        x = a.inp(X, 104, "x")
        ok(lib, lib.gp_l2norm_rows(P(x), x.stride(0), d, n, S()))
        return {"x": x}

    y = run(case)["x"].cpu().double()
    # test_student_forward_vs_oracle: unit-norm rows against fp64 within 1e-5
    assert (y - F.normalize(X.double(), dim=1)).abs().max() < 1e-5


# ------------------------------------------------------------------------------------------ gp_affinity_softmax / _scatter
# affinity_block_kernel: 16 rows per workgroup (knob 15 = 2: 8 rows); the wave form (knob 15 = 1): a row per wave, 4 per workgroup
@pytest.mark.parametrize("nv", [31, 33])
@pytest.mark.parametrize("knob", [0, 1, 2], ids=["block16", "wave", "block8"])
@pytest.mark.parametrize("entry", ["softmax", "softmax_scatter"])
def test_affinity_softmax(ops, lib, entry, knob, nv):
    K, d = 20, 128
    nbr = geo(nv, K)["nbr"]
    E = unit_rows(nv, d, 600 + nv)
    op = ops.pool_cs_plan(up(nbr), 128, structure=True) if entry == "softmax_scatter" else None

    def case(a):
        e, nb = a.inp(E, 136, "e"), a.inp(nbr, name="nbr")
        w = a.out((nv, K), F32, name="w")
        if op is None:
            ok(lib, lib.gp_affinity_softmax(P(e), e.stride(0), d, P(nb), K, nv, 20.0, P(w), S()))
            return {"w": w}
        dst = a.inp(op.dst, name="dst")
        hi, lo = a.out(op.wa_hi.numel(), F16, name="wa_hi"), a.out(op.wa_lo.numel(), F16, name="wa_lo")
        hi.copy_(op.wa_hi), lo.copy_(op.wa_lo)               # the structure pass's zeroed fragments
        ok(lib, lib.gp_affinity_softmax_scatter(P(e), e.stride(0), d, P(nb), K, nv, 20.0, P(w), P(dst), P(hi), P(lo), S()))
        return {"w": w, "wa_hi": hi, "wa_lo": lo}

    try:
        ok(lib, lib.gp_debug_set(15, knob))
        r = run(case)
    finally:
        ok(lib, lib.gp_debug_set(15, 0))
    whole(r["w"], "w")
    # test_affinity_and_pooling: fp32 softmax within 2e-6 of the oracle
    assert (r["w"].cpu().double() - o_aff.affinity_weights(E.double(), nbr.long(), 20.0)).abs().max() < 2e-6
    if op is not None:
        # test_pool_cs_matches_ell_and_oracle: the fragments are the ones gp_pool_cs_fill makes of these weights
        ref = ops.pool_cs_build(up(nbr), r["w"], 128)
        at = op.dst.long().flatten()
        for got, want, was in ((r["wa_hi"], ref.wa_hi, op.wa_hi), (r["wa_lo"], ref.wa_lo, op.wa_lo)):
            assert torch.equal(got[at], want[at])
            rest = torch.ones_like(got, dtype=torch.bool)
            rest[at] = False                                 # only the elements the dst table names are written
            assert torch.equal(bits(got[rest]), bits(was[rest]))


# ------------------------------------------------------------------------------------------ the column-sliced pooling operator
def pool_inputs(nv, K, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(nv, K, generator=g), dim=1), torch.randn(nv, d, generator=g)


def block_unions(nbc, nv, rows):
    return np.array([len(np.unique(nbc[b:b + rows])) for b in range(0, nv, rows)])


def cs_operator_inputs(a, op):
    """the operator's arrays as fenced inputs at exactly the header's sizes"""
    return (a.inp(op.bu_off, name="bu_off"), a.inp(op.bu_row, name="bu_row"), a.inp(op.bu_mask, name="bu_mask"),
            a.inp(op.wa_hi, name="wa_hi"), a.inp(op.wa_lo, name="wa_lo"))


# cs builders: a row block (rows_per_block rows) per workgroup; union rows padded to steps of 32; 129 and 255 rows leave a last block
# of 1 and of rows_per_block - 1 rows at 128, of 29 and 55 at 100
@pytest.mark.parametrize("rpb", [128, 100])
@pytest.mark.parametrize("nv", [129, 255])
@pytest.mark.parametrize("entry", ["count", "fill", "structure", "structure_valid", "affinity_cs_fragments"])
def test_pool_cs_builders(ops, lib, entry, nv, rpb):
    K = 20
    nbr = geo(nv, K)["nbr"]
    nb = -(-nv // rpb)
    W, X = pool_inputs(nv, K, 256, 700 + nv + rpb)
    E = unit_rows(nv, 128, 710 + nv)
    full = ops.pool_cs_plan(up(nbr), rpb, structure=True)    # sizes (two host read-backs) and the reference dst table
    total, mu = full.total, full.max_union
    steps = total // 32
    valid_op = ops.pool_cs_plan(up(nbr), rpb, structure="valid") if entry == "affinity_cs_fragments" else None
    eh, el = ops.split_f16(up(E), 128, scale=up(torch.tensor([1024.0])))

    def arrays(a, dst=False, valid=False):
        o = {"bu_row": a.out(total, I32, name="bu_row"), "bu_mask": a.out(steps, I32, name="bu_mask")}
        if not valid:
            o["wa_hi"], o["wa_lo"] = a.out(steps * 8 * 512, F16, name="wa_hi"), a.out(steps * 8 * 512, F16, name="wa_lo")
        if dst:
            o["dst"] = a.out((nv, K), I32, name="dst")
        if valid:
            o["valid"] = a.out(steps * 128 + 64, I32, name="valid")
        return o

    def case(a):
        nbd = a.inp(nbr, name="nbr")
        if entry == "count":
            nbytes = lib.gp_pool_cs_workspace_bytes(nv, rpb)
            ws = a.out(nbytes, U8, name="workspace")
            o = {"bu_off": a.out(nb + 1, I64, name="bu_off"), "bu_n": a.out(nb, I32, name="bu_n"), "max_union": a.out(1, I64, name="max_union")}
            ok(lib, lib.gp_pool_cs_count(P(nbd), nv, K, rpb, P(o["bu_off"]), P(o["bu_n"]), P(o["max_union"]), P(ws), nbytes, S()))
            return o
        off = a.inp(full.bu_off, name="bu_off")
        if entry == "fill":
            o, w = arrays(a), a.inp(W, name="w")
            ok(lib, lib.gp_pool_cs_fill(P(nbd), P(w), nv, K, rpb, P(off), total, mu, P(o["bu_row"]), P(o["bu_mask"]), P(o["wa_hi"]),
                                        P(o["wa_lo"]), S()))
        elif entry == "structure":
            o = arrays(a, dst=True)
            ok(lib, lib.gp_pool_cs_structure(P(nbd), nv, K, rpb, P(off), total, mu, P(o["bu_row"]), P(o["bu_mask"]), P(o["wa_hi"]),
                                             P(o["wa_lo"]), P(o["dst"]), S()))
        elif entry == "structure_valid":
            o = arrays(a, valid=True)
            ok(lib, lib.gp_pool_cs_structure_valid(P(nbd), nv, K, rpb, P(off), total, mu, P(o["bu_row"]), P(o["bu_mask"]), P(o["valid"]), S()))
        else:
            row, mask, valid = a.inp(valid_op.bu_row, name="bu_row"), a.inp(valid_op.bu_mask, name="bu_mask"), a.inp(valid_op.valid, name="valid")
            h, l = a.inp(eh, name="e_hi"), a.inp(el, name="e_lo")
            o = {"wa_hi": a.out(steps * 8 * 512, F16, name="wa_hi"), "wa_lo": a.out(steps * 8 * 512, F16, name="wa_lo")}
            ok(lib, lib.gp_affinity_cs_fragments(P(h), P(l), nv, 128, K, 20.0, P(off), P(row), P(mask), P(valid), rpb, P(o["wa_hi"]),
                                                 P(o["wa_lo"]), S()))
        return o

    r = run(case)
    dst = full.dst.long()
    if entry == "count":
        off, bn = r["bu_off"].cpu().numpy(), r["bu_n"].cpu().numpy()
        assert np.array_equal(bn, block_unions(nbr.numpy(), nv, rpb))                   # index outputs: exact
        assert off[0] == 0 and np.array_equal(np.diff(off), -(-bn // 32) * 32)           # padded to whole steps of 32 union rows
        assert np.array_equal(off, full.bu_off.cpu().numpy()) and int(r["max_union"]) == bn.max()      # the largest (unpadded) block union
        return
    if entry == "affinity_cs_fragments":
        r["bu_row"], r["bu_mask"] = valid_op.bu_row, valid_op.bu_mask
    whole(r["bu_row"], "bu_row"), whole(r["bu_mask"], "bu_mask")
    assert torch.equal(r["bu_row"], full.bu_row) and torch.equal(r["bu_mask"], full.bu_mask)      # index outputs: exact, and the same from every builder
    assert int(r["bu_row"].min()) >= 0 and int(r["bu_row"].max()) < nv
    if entry == "structure":
        whole(r["dst"], "dst")
        assert torch.equal(r["dst"], full.dst)
        d_ = r["dst"].long()
        assert int(d_.min()) >= 0 and int(d_.max()) < steps * 8 * 512 and d_.unique().numel() == d_.numel()
        assert bool((r["wa_hi"][d_] == 0).all()) and bool((r["wa_lo"][d_] == 0).all())   # the fragments the weights go to are zeroed
        return
    if entry == "structure_valid":
        # test_affinity_cs_fragments_vs_fp64_and_the_block_kernel: the validity words are the dst table's (step, row, bit) set ...
        st, grp, ln, e8 = dst // 4096, (dst // 512) % 8, (dst // 8) % 64, dst % 8
        krow, rl = (ln // 16) * 8 + e8, grp * 16 + ln % 16
        want = torch.zeros(steps * 128, dtype=I64, device="cuda")
        want.index_put_(((st * 128 + rl).flatten(),), torch.bitwise_left_shift(torch.ones_like(krow), krow).flatten(), accumulate=True)
        assert torch.equal(r["valid"][:steps * 128].long() & 0xFFFFFFFF, want)
        assert bool((r["valid"][steps * 128:] == 0).all())    # ... and the 64 padding words behind them are zero
        return
    # fill / fragments: the weights read back from the fragments, and one application of the operator
    w = (r["wa_hi"][dst].float() + r["wa_lo"][dst].float()) / 1024.0
    if entry == "fill":
        # the fragments hold w x 2^10 as hi + lo: 2^-22 relative by the formats (split_error_ok), w <= 1.  No existing test states a bound
        # of its own here; test_pool_mfma_matches_ell_and_oracle's 1e-7 on the rebuilt dense block is the nearest, and 2^-22 < 1e-6 is no looser
        # than what test_sparse_conv_f16x3_matches_fp32_accuracy allows a split
        assert (w.cpu().double() - W.double()).abs().max() <= 2.0 ** -22
        w_ref = W
    else:
        w_ref = torch.softmax(20.0 * (E.double()[:, None, :] * E.double()[nbr.long()]).sum(-1), dim=1)
        # test_affinity_cs_fragments_vs_fp64_and_the_block_kernel: 2e-6 against the fp64 softmax
        assert (w.cpu().double() - w_ref).abs().max() < 2e-6
    op = ops.PoolCs(full.bu_off, full.bu_n, r["bu_row"], r["bu_mask"], r["wa_hi"], r["wa_lo"], nv, total, block_rows=rpb)
    y = torch.empty((nv, 256), device="cuda")
    ops.pool_cs_apply(ops.split_f16(up(X)), op, 256, out_f32=y)
    # test_pool_cs_tiny_voxel_sets: one application within 1e-5 of the fp64 gather
    assert (y.cpu().double() - o_aff.pool_gather(X, nbr.long(), w_ref, 1)).abs().max() < 1e-5


# cs_pool_ns_kernel (d = 256: one 256-column slice): a row block of rows_per_block rows per workgroup, every wave all rows x 32 columns
@pytest.mark.parametrize("rpb", [128, 100])
@pytest.mark.parametrize("nv", [129, 255])
@pytest.mark.parametrize("form", ["planes", "fp32", "both"])
def test_pool_cs_apply(ops, lib, form, nv, rpb):
    K, d = 20, 256
    nbr = geo(nv, K)["nbr"]
    W, X = pool_inputs(nv, K, d, 800 + nv + rpb)
    op = ops.pool_cs_build(up(nbr), up(W), rpb)
    xh, xl = ops.split_f16(up(X))

    def case(a):
        h, l = a.inp(xh, d + 8, "x_hi"), a.inp(xl, d + 8, "x_lo")
        off, row, mask, wh, wl = cs_operator_inputs(a, op)
        o = {}
        if form != "fp32":
            o["y_hi"], o["y_lo"] = a.out((nv, d), F16, d + 8, "y_hi"), a.out((nv, d), F16, d + 8, "y_lo")
        if form != "planes":
            o["y_f32"] = a.out((nv, d), F32, d + 8, "y_f32")
        yh, yl, yf = o.get("y_hi"), o.get("y_lo"), o.get("y_f32")
        ok(lib, lib.gp_pool_cs_apply(P(h), P(l), h.stride(0), P(off), P(row), P(mask), P(wh), P(wl), nv, d, rpb, P(yh), P(yl),
                                     yh.stride(0) if yh is not None else 0, P(yf), yf.stride(0) if yf is not None else 0, None, S()))
        return o

    r = run(case)
    ref = o_aff.pool_gather(X, nbr.long(), W, 1)
    for k, v in r.items():
        whole(v, k)
    if "y_f32" in r:
        assert (r["y_f32"].cpu().double() - ref).abs().max() < 1e-5                # test_pool_cs_tiny_voxel_sets
    if "y_hi" in r:
        # test_pool_cs_matches_ell_and_oracle: the planes' sum is within 1e-6 of the fp32 rows, which are within 1e-5 of fp64
        assert ((r["y_hi"].cpu().double() + r["y_lo"].cpu().double()) - ref).abs().max() < 1e-5 + 1e-6


# cs_chain_ns_kernel: the same tiles, T x the grid; flags at exactly gp_pool_cs_chain_flag_words_d words, dep [nblocks * 64]
@pytest.mark.parametrize("rpb", [128, 100])
@pytest.mark.parametrize("nv", [129, 255])
def test_pool_cs_deps_and_chain(ops, lib, nv, rpb):
    K, d, T = 20, 256, 3
    nbr = geo(nv, K)["nbr"]
    nb = -(-nv // rpb)
    W, X = pool_inputs(nv, K, d, 900 + nv + rpb)
    op = ops.pool_cs_build(up(nbr), up(W), rpb)
    xh, xl = ops.split_f16(up(X))
    words = lib.gp_pool_cs_chain_flag_words_d(nv, rpb, d)
    assert words == 32 + (d // 256) * nb                      # the header's formula

    def case(a):
        off, row, mask, wh, wl = cs_operator_inputs(a, op)
        dep, scratch = a.out(nb * 64, I32, name="dep"), a.out(nb, I32, name="scratch")
        ok(lib, lib.gp_pool_cs_deps(P(off), P(row), nv, rpb, P(dep), P(scratch), S()))
        h, l = a.inp(xh, d + 8, "x_hi"), a.inp(xl, d + 8, "x_lo")                    # rewritten from application 1 on
        ph, pl = a.out((nv, d), F16, d + 8, "p_hi"), a.out((nv, d), F16, d + 8, "p_lo")
        y = a.out((nv, d), F32, d + 8, "y_f32")
        flags = a.out(words, I32, name="flags")
        flags.zero_()
        ok(lib, lib.gp_pool_cs_apply_chain(P(h), P(l), P(ph), P(pl), h.stride(0), P(off), P(row), P(mask), P(wh), P(wl), nv, d, rpb, T,
                                           P(y), y.stride(0), None, P(dep), P(flags), 0, S()))
        torch.cuda.synchronize()
        chk = ops.PoolCs(off, None, row, mask, wh, wl, nv, op.total, block_rows=rpb)
        chk.flags = flags
        ops.pool_cs_chain_check(chk)                          # the abort word is clear
        return {"dep_counts": dep.view(-1, 64)[:, 0].clone(), "x_hi": h, "x_lo": l, "p_hi": ph, "p_lo": pl, "y_f32": y}

    r = run(case)
    for k in ("p_hi", "p_lo", "y_f32"):
        whole(r[k], k)
    # dependency lists against numpy (test_pool_cs_chained_launch_small_and_overflowing_lists)
    off_, row_ = op.bu_off.cpu().numpy(), op.bu_row.cpu().numpy()
    src, dst = np.repeat(np.arange(nb), np.diff(off_)), row_ // rpb
    e = np.unique(np.concatenate([src * nb + dst, dst * nb + src, np.arange(nb) * (nb + 1)]))
    assert np.array_equal(r["dep_counts"].cpu().numpy(), np.bincount(e // nb, minlength=nb))
    # test_pool_cs_matches_ell_and_oracle: repeated applications within 2e-5 of the fp64 gather
    assert (r["y_f32"].cpu().double() - o_aff.pool_gather(X, nbr.long(), W, T)).abs().max() < 2e-5
    # the planes left behind are those of the applications one by one (T = 3: p after the first, x after the second)
    one = o_aff.pool_gather(X, nbr.long(), W, 1)
    two = o_aff.pool_gather(X, nbr.long(), W, 2)
    assert ((r["p_hi"].cpu().double() + r["p_lo"].cpu().double()) - one).abs().max() < 1e-5 + 1e-6
    assert ((r["x_hi"].cpu().double() + r["x_lo"].cpu().double()) - two).abs().max() < 2e-5 + 1e-6


# ------------------------------------------------------------------------------------------ ELL, tiles, matrix-core blocks
@pytest.mark.parametrize("nv", [129, 255])                  # pool_ell_kernel: a (row, 256-column slab) per wave, 4 per workgroup
def test_pool_ell(ops, lib, nv):
    K, d = 20, 64
    nbr = geo(nv, K)["nbr"]
    W, X = pool_inputs(nv, K, d, 1000 + nv)

    def case(a):
        x, nb, w = a.inp(X, 72, "x"), a.inp(nbr, name="nbr"), a.inp(W, name="w")
        y = a.out((nv, d), F32, 72, "y")
        ok(lib, lib.gp_pool_ell(P(x), x.stride(0), P(nb), P(w), K, nv, d, P(y), y.stride(0), S()))
        return {"y": y}

    y = run(case)["y"]
    whole(y, "y")
    # test_pool_tiles_matches_ell_and_oracle holds the ELL kernel and the fp64 gather 1e-5 apart over five applications
    assert (y.cpu().double() - o_aff.pool_gather(X, nbr.long(), W, 1)).abs().max() < 1e-5


# tiles of r rows: a tile per wave in the builders, a (tile, slab) per wave in the apply; 129 = 32 r + 1 and 255 = 64 r - 1 at r = 4
@pytest.mark.parametrize("nv", [129, 255])
@pytest.mark.parametrize("r", [4, 16])
@pytest.mark.parametrize("entry", ["count", "fill", "apply"])
def test_pool_tiles(ops, lib, entry, r, nv):
    K = 20
    d = 512 if r == 4 else 256                               # r = 4 keeps 512 columns per wave: d a multiple of 512
    nbr = geo(nv, K)["nbr"]
    nbc = nbr.numpy()
    nt = -(-nv // r)
    W, X = pool_inputs(nv, K, d, 1100 + nv + r)
    tiles = ops.pool_tiles_build(up(nbr), up(W), r)
    total = tiles.total

    def case(a):
        nbd = a.inp(nbr, name="nbr")
        if entry == "count":
            nbytes = lib.gp_pool_tiles_workspace_bytes(nv, r)
            ws, off = a.out(nbytes, U8, name="workspace"), a.out(nt + 1, I64, name="tile_off")
            ok(lib, lib.gp_pool_tiles_count(P(nbd), nv, K, r, P(off), P(ws), nbytes, S()))
            return {"tile_off": off}
        off = a.inp(tiles.tile_off, name="tile_off")
        if entry == "fill":
            w = a.inp(W, name="w")
            urow, uw = a.out(total, I32, name="u_row"), a.out((total, r), F32, name="u_w")
            ok(lib, lib.gp_pool_tiles_fill(P(nbd), P(w), nv, K, r, P(off), P(urow), P(uw), S()))
            return {"u_row": urow, "u_w": uw}
        urow, uw = a.inp(tiles.u_row, name="u_row"), a.inp(tiles.u_w, name="u_w")
        x = a.inp(X, d + 8, "x")
        y = a.out((nv, d), F32, d + 8, "y")
        ok(lib, lib.gp_pool_tiles_apply(P(x), x.stride(0), P(off), P(urow), P(uw), r, nv, d, P(y), y.stride(0), S()))
        return {"y": y}

    res = run(case)
    for k, v in res.items():
        whole(v, k)
    if entry == "count":
        assert np.array_equal(res["tile_off"].cpu().numpy(), np.concatenate([[0], np.cumsum(block_unions(nbc, nv, r))]))
    elif entry == "fill":
        # test_pool_tiles_matches_ell_and_oracle: every (row, neighbour, weight) exactly once in its tile's dense block, exact
        off, urow, uw = tiles.tile_off.cpu().numpy(), res["u_row"].cpu().numpy(), res["u_w"].cpu().numpy()
        for t in range(nt):
            rows = range(t * r, min((t + 1) * r, nv))
            u = urow[off[t]:off[t + 1]]
            assert len(np.unique(u)) == len(u) and set(u) == set(nbc[list(rows)].reshape(-1))
            dense = np.zeros((len(u), r), np.float32)
            pos = {v: i for i, v in enumerate(u)}
            for r_i, row in enumerate(rows):
                for j in range(K):
                    dense[pos[nbc[row, j]], r_i] = W[row, j]
            assert np.array_equal(uw[off[t]:off[t + 1]], dense)
    else:
        # test_pool_tiles_matches_ell_and_oracle: 1e-5 against the fp64 gather
        assert (res["y"].cpu().double() - o_aff.pool_gather(X, nbr.long(), W, 1)).abs().max() < 1e-5


# pm kernels: blocks of 64 rows (129 = 2 blocks + 1 row, 255 = 4 blocks - 1 row); union rows padded to steps of 32; the persistent
# kernel stores whole blocks, so its output holds ceil(nv / 64) * 64 rows and the rows from nv on receive zeros
@pytest.mark.parametrize("nv", [129, 255])
@pytest.mark.parametrize("entry", ["count", "fill", "apply_planes", "apply_fp32", "persistent_planes", "persistent_fp32"])
def test_pool_mfma(ops, lib, entry, nv):
    K, d, BR = 20, 512, 64
    persistent = entry.startswith("persistent")
    min_steps = 9 if persistent else 0
    nbr = geo(nv, K)["nbr"]
    nbc = nbr.numpy()
    nb = -(-nv // BR)
    W, X = pool_inputs(nv, K, d, 1200 + nv)
    op = ops.pool_mfma_build(up(nbr), up(W), BR, min_steps=min_steps)
    total = op.total
    xh, xl = ops.split_f16(up(X))
    y_rows = nb * BR if persistent else nv

    def case(a):
        if entry in ("count", "fill"):
            nbd = a.inp(nbr, name="nbr")
        if entry == "count":
            nbytes = lib.gp_pool_mfma_workspace_bytes(nv, BR)
            ws = a.out(nbytes, U8, name="workspace")
            off, bn = a.out(nb + 1, I64, name="bu_off"), a.out(nb, I32, name="bu_n")
            ok(lib, lib.gp_pool_mfma_count(P(nbd), nv, K, BR, min_steps, P(off), P(bn), P(ws), nbytes, S()))
            return {"bu_off": off, "bu_n": bn}
        off = a.inp(op.bu_off, name="bu_off")
        if entry == "fill":
            w, bn = a.inp(W, name="w"), a.inp(op.bu_n, name="bu_n")
            row = a.out(total, I32, name="bu_row")
            wh, wl = a.out(total // 32 * 4 * 64 * 8, F16, name="wa_hi"), a.out(total // 32 * 4 * 64 * 8, F16, name="wa_lo")
            ok(lib, lib.gp_pool_mfma_fill(P(nbd), P(w), nv, K, BR, P(off), P(bn), total, P(row), P(wh), P(wl), S()))
            return {"bu_row": row, "wa_hi": wh, "wa_lo": wl}
        row, wh, wl = a.inp(op.bu_row, name="bu_row"), a.inp(op.wa_hi, name="wa_hi"), a.inp(op.wa_lo, name="wa_lo")
        h, l = a.inp(xh, d + 8, "x_hi"), a.inp(xl, d + 8, "x_lo")
        o = {}
        if entry.endswith("planes"):
            o["y_hi"], o["y_lo"] = a.out((y_rows, d), F16, d + 8, "y_hi"), a.out((y_rows, d), F16, d + 8, "y_lo")
        else:
            o["y_f32"] = a.out((y_rows, d), F32, d + 8, "y_f32")
        yh, yl, yf = o.get("y_hi"), o.get("y_lo"), o.get("y_f32")
        ldy, ldf = (yh.stride(0) if yh is not None else 0), (yf.stride(0) if yf is not None else 0)
        if persistent:
            queue = a.out(9, I32, name="queue")
            queue.zero_()
            ok(lib, lib.gp_pool_mfma_apply_persistent(P(h), P(l), h.stride(0), P(off), P(row), P(wh), P(wl), nv, d, BR, op.min_steps, P(yh),
                                                      P(yl), ldy, P(yf), ldf, y_rows, None, P(queue), S()))
            o["queue"] = queue
        else:
            ok(lib, lib.gp_pool_mfma_apply(P(h), P(l), h.stride(0), P(off), P(row), P(wh), P(wl), nv, d, BR, P(yh), P(yl), ldy, P(yf), ldf,
                                           None, S()))
        return o

    r = run(case)
    for k, v in r.items():
        whole(v, k)
    if entry == "count":
        off, bn = r["bu_off"].cpu().numpy(), r["bu_n"].cpu().numpy()
        assert np.array_equal(bn, block_unions(nbc, nv, BR))
        assert off[0] == 0 and np.array_equal(np.diff(off), np.maximum(-(-bn // 32), min_steps) * 32)      # padded to steps of 32, min_steps of them
        return
    if entry == "fill":
        # test_pool_mfma_matches_ell_and_oracle: sorted unions, padded with the first union row; the weights through an application
        off, bn, br = op.bu_off.cpu().numpy(), op.bu_n.cpu().numpy(), r["bu_row"].cpu().numpy()
        for b in range(nb):
            u = br[off[b]:off[b] + bn[b]]
            assert (np.diff(u) > 0).all() and set(u) == set(nbc[b * BR:b * BR + BR].reshape(-1)) and (br[off[b] + bn[b]:off[b + 1]] == u[0]).all()
        op2 = ops.PoolMfma(op.bu_off, op.bu_n, r["bu_row"], r["wa_hi"], r["wa_lo"], nv, total, BR)
        y = torch.empty((nv, d), device="cuda")
        ops.pool_mfma_apply((xh, xl), op2, d, out_f32=y)
    else:
        if persistent:
            assert bool((r["queue"] == 0).all())              # left zero by every launch
        for k, v in r.items():
            assert k == "queue" or bool((bits(v[nv:]) == 0).all()), k      # the padded rows nv .. ceil(nv / 64) * 64 - 1 receive zeros (+0)
        y = (r["y_f32"] if "y_f32" in r else r["y_hi"].float() + r["y_lo"].float())[:nv]
    # test_pool_mfma_tiny_voxel_sets: one application within 1e-5 of the fp64 gather (+ 1e-6 for planes, test_pool_mfma_matches_ell_and_oracle)
    assert (y.cpu().double() - o_aff.pool_gather(X, nbr.long(), W, 1)).abs().max() < 1e-5 + (1e-6 if "y_hi" in r else 0.0)


# ------------------------------------------------------------------------------------------ orders, kernel map, kNN
@pytest.mark.parametrize("nv", [1, 257])                    # elementwise kernels of 256 threads around a radix sort
def test_morton_order(ops, lib, nv):
    c = geo(nv, None)["c"]

    def case(a):
        cd = a.inp(torch.from_numpy(c), name="coords")
        nbytes = lib.gp_morton_order_workspace_bytes(nv)
        ws = a.out(nbytes, U8, name="workspace")
        perm, rank = a.out(nv, I32, name="perm"), a.out(nv, I32, name="rank")
        ok(lib, lib.gp_morton_order(P(cd), nv, P(perm), P(rank), P(ws), nbytes, S()))
        return {"perm": perm, "rank": rank}

    r = run(case)
    want = geo(nv, None)["perm"]
    assert np.array_equal(r["perm"].cpu().numpy(), want)
    assert np.array_equal(r["rank"].cpu().numpy()[want], np.arange(nv))


@pytest.mark.parametrize("nv", [1, 257])                    # kernel_map_kernel: 256 threads, a voxel each
def test_kernel_map_build(ops, lib, nv):
    g = geo(nv)
    grid = grid_of(ops, g["cs"])
    nbytes = lib.gp_grid_bytes(nv, (ctypes.c_int32 * 3)(*grid.extent))

    def case(a):
        gb, cd = a.inp(grid.buf[:nbytes], name="grid"), a.inp(torch.from_numpy(g["cs"]), name="coords")
        nm = a.out((27, nv), I32, name="nbr_map")
        ok(lib, lib.gp_kernel_map_build(P(gb), P(cd), nv, P(nm), S()))
        return {"nbr_map": nm}

    assert np.array_equal(run(case)["nbr_map"].cpu().numpy(), g["nm"])        # test_morton_grid_kernel_map: the oracle's map, exact


# rcb_chunk_kernel: a chunk of 1024 rows per workgroup, leaves of 128; 1025 and 1151 leave a last chunk of 1 and of 127 rows
@pytest.mark.parametrize("nv", [1025, 1151])
def test_rcb_order(ops, lib, nv):
    cs = geo(nv, None)["cs"]

    def case(a):
        cd = a.inp(torch.from_numpy(cs), name="coords")
        sigma, rho = a.out(nv, I32, name="sigma"), a.out(nv, I32, name="rho")
        ok(lib, lib.gp_rcb_order(P(cd), nv, 1024, 128, P(sigma), P(rho), S()))
        return {"sigma": sigma, "rho": rho}

    r = run(case)
    sg, rh = r["sigma"].cpu().numpy().astype(np.int64), r["rho"].cpu().numpy().astype(np.int64)
    assert np.array_equal(sg, rcb_reference(cs, 1024, 128))
    assert np.array_equal(rh[sg], np.arange(nv)) and np.array_equal(sg // 1024, np.arange(nv) // 1024)


@pytest.mark.parametrize("nv", [1, 257])                    # rows_renumber_kernel: 256 threads, grid-stride over nv * k elements
def test_rows_renumber(ops, lib, nv):
    K = 20
    g = torch.Generator().manual_seed(1300 + nv)
    nbr = torch.randint(0, nv, (nv, K), generator=g).to(I32)
    sigma = torch.randperm(nv, generator=g)
    rho = torch.empty_like(sigma)
    rho[sigma] = torch.arange(nv)

    def case(a):
        nb, sg, rh = a.inp(nbr, name="nbr"), a.inp(sigma.to(I32), name="sigma"), a.inp(rho.to(I32), name="rho")
        out = a.out((nv, K), I32, name="out")
        ok(lib, lib.gp_rows_renumber_i32(P(nb), nv, K, P(sg), P(rh), P(out), S()))
        return {"out": out}

    assert torch.equal(run(case)["out"].cpu().long(), rho[nbr.long()[sigma]])


# knn_ring_kernel: 4 queries per workgroup in ring 1, 2 in ring 3; 21 voxels with K = 20: every query ends in the exhaustive kernel
@pytest.mark.parametrize("nv", [21, 1025])
def test_knn_lattice(ops, lib, nv):
    K = 20
    g = geo(nv, None)
    grid = grid_of(ops, g["cs"])
    nbytes = lib.gp_grid_bytes(nv, (ctypes.c_int32 * 3)(*grid.extent))
    perm = torch.from_numpy(g["perm"])

    def case(a):
        gb, cd, ids = a.inp(grid.buf[:nbytes], name="grid"), a.inp(torch.from_numpy(g["cs"]), name="coords"), a.inp(perm, name="ids")
        wbytes = lib.gp_knn_workspace_bytes(nv)
        ws = a.out(wbytes, U8, name="workspace")
        nbr = a.out((nv, K), I32, name="nbr")
        ok(lib, lib.gp_knn_lattice(P(gb), P(cd), P(ids), nv, K, P(nbr), P(ws), wbytes, S()))
        return {"nbr": nbr}

    nbr = run(case)["nbr"].cpu().long()
    back = torch.empty_like(nbr)
    back[perm.long()] = perm.long()[nbr]                     # rows and ids of the reference order
    assert torch.equal(back, o_aff.knn_lattice(g["c"], K))    # test_knn_exact_with_ties: exact, the (d2, id) order included


# ------------------------------------------------------------------------------------------ the convolutions
def conv_inputs(nv, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(nv, cin, generator=g) * 3.0
    X[:, :8] *= 1e-3                                         # small-magnitude channels too
    W = torch.randn(27, cin, cout, generator=g) * 0.05
    return X, W, torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g), torch.randn(nv, cout, generator=g)


# sparse_conv_kernel: tiles of 128 rows x 128 columns (cout a multiple of 128: the narrowest layer it takes)
@pytest.mark.parametrize("nv", [1, 255, 257])
def test_sparse_conv_fp32(ops, lib, nv):
    cin, cout = 32, 128
    nm = geo(nv)["nm"]
    X, W, sc, sh, res = conv_inputs(nv, cin, cout, 1400 + nv)

    def case(a):
        x, m, w = a.inp(X, cin + 8, "x"), a.inp(torch.from_numpy(nm), name="nbr_map"), a.inp(W.reshape(27 * cin, cout), name="w")
        s_, b_, r_ = a.inp(sc, name="scale"), a.inp(sh, name="shift"), a.inp(res, cout + 8, "residual")
        y = a.out((nv, cout), F32, cout + 8, "y")
        ok(lib, lib.gp_sparse_conv(P(x), x.stride(0), P(m), nv, P(w), 27, cin, cout, P(s_), P(b_), P(r_), r_.stride(0), 1, P(y), y.stride(0), S()))
        return {"y": y}

    y = run(case)["y"]
    whole(y, "y")
    ref = torch.relu(o_student.sparse_conv3(X.double(), nm.astype(np.int64), W.double()) * sc.double() + sh.double() + res.double())
    assert (y.cpu().double() - ref).abs().max() < 2e-5       # test_sparse_conv_single_layer


def tiles_of(nmc, r0, r1):
    return int((((nmc[:, r0:r1] >= 0).sum(1) + 255) // 256).sum())


# chunk_count_kernel: a granule of 256 rows per workgroup; 255 / 257 / 513 rows: one granule short of a row, and a last granule of one row
@pytest.mark.parametrize("nv", [255, 257, 513])
@pytest.mark.parametrize("target", [752, 30], ids=["one_chunk", "tight"])
def test_conv_chunk_plan(ops, lib, target, nv):
    nm = geo(nv)["nm"]
    max_chunks = -(-nv // 256)

    def case(a):
        m = a.inp(torch.from_numpy(nm), name="nbr_map")
        nbytes = lib.gp_conv_chunk_plan_workspace_bytes(nv, 256)
        ws = a.out(nbytes, U8, name="workspace")
        rows, n = a.out(max_chunks + 1, I32, name="chunk_row_off"), a.out(1, I32, name="n_chunks")
        ok(lib, lib.gp_conv_chunk_plan(P(m), nv, 27, 256, 1, target, max_chunks, P(rows), P(n), P(ws), nbytes, S()))
        return {"chunk_row_off": rows, "n_chunks": n}

    r = run(case)
    n = int(r["n_chunks"])
    rows = r["chunk_row_off"].cpu().tolist()[:n + 1]
    # test_sparse_conv_f16x3_matches_fp32_accuracy: chunks of whole granules within the tile target, greedy
    assert 1 <= n <= max_chunks and rows[0] == 0 and rows[-1] == nv and all(b > a and (b % 256 == 0 or b == nv) for a, b in zip(rows[:-1], rows[1:]))
    for ci in range(n):
        assert tiles_of(nm, rows[ci], rows[ci + 1]) <= target or rows[ci + 1] - rows[ci] <= 256
        if ci + 1 < n:
            assert tiles_of(nm, rows[ci], rows[ci + 1] + 256) > target


# pair kernels: 256 threads over the kv * nv map entries; pairs in 256-pair tiles per (chunk, offset) segment
@pytest.mark.parametrize("nv", [255, 257, 513])
@pytest.mark.parametrize("chunking", ["rows256", "balanced"])
def test_conv_pairs_build(ops, lib, chunking, nv):
    nm, kv = geo(nv)["nm"], 27
    if chunking == "rows256":
        rows = list(range(0, nv, 256)) + [nv]
    else:
        old, ops.CONV_TARGET_TILES = ops.CONV_TARGET_TILES, 30
        try:
            rows = list(ops.conv_pairs_build(up(nm), "balanced", col_tiles=1).chunk_row_off)
        finally:
            ops.CONV_TARGET_TILES = old
    nch = len(rows) - 1
    nseg = nch * kv

    def case(a):
        m, ro = a.inp(torch.from_numpy(nm), name="nbr_map"), a.inp(torch.tensor(rows, dtype=I32), name="chunk_row_off")
        nbytes = lib.gp_conv_pairs_workspace_bytes(nv, kv)
        ws = a.out(nbytes, U8, name="workspace")
        o = {"pair_in": a.out(kv * nv, I32, name="pair_in"), "pair_pos": a.out((kv, nv), I32, name="pair_pos"),
             "seg_off": a.out(nseg + 1, I32, name="seg_off"), "tile_start": a.out(nseg + 1, I32, name="tile_start"),
             "tile_desc": a.out(((kv * nv) // 256 + nseg + 1, 4), I32, name="tile_desc")}             # the sizes ops.conv_pairs_build computes
        ok(lib, lib.gp_conv_pairs_build(P(m), nv, kv, nch, P(ro), P(o["pair_in"]), P(o["pair_pos"]), P(o["seg_off"]), P(o["tile_start"]),
                                        P(o["tile_desc"]), P(ws), nbytes, S()))
        return o

    r = {k: v.cpu().numpy() for k, v in run(case).items()}
    # test_sparse_conv_f16x3_matches_fp32_accuracy: the pair arrays against the map, exact
    num_pairs = int((nm >= 0).sum())
    pos, off, ts = r["pair_pos"], r["seg_off"], r["tile_start"]
    assert off[-1] == num_pairs and np.array_equal(pos >= 0, nm >= 0)
    assert np.array_equal(r["pair_in"][pos[pos >= 0]], nm[nm >= 0])
    assert np.array_equal(np.sort(pos[pos >= 0]), np.arange(num_pairs))
    seg_counts = np.concatenate([(nm[:, a:b] >= 0).sum(1) for a, b in zip(rows[:-1], rows[1:])])
    assert off[0] == 0 and np.array_equal(np.diff(off), seg_counts)
    assert ts[0] == 0 and np.array_equal(np.diff(ts), (seg_counts + 255) // 256)
    desc = r["tile_desc"][:ts[-1]]                           # {k, first pair, count, 0} per tile
    want = [(s % kv, off[s] + 256 * t, min(256, seg_counts[s] - 256 * t), 0) for s in range(nseg) for t in range((seg_counts[s] + 255) // 256)]
    assert np.array_equal(desc, np.array(want, dtype=np.int32).reshape(-1, 4))


# conv_phase1 kernels: tiles of 256 pairs x 256 columns; phase 2: output rows of a chunk; chunks of 256 rows: 255 / 257 / 513 rows are
# one chunk short of a row, and a last chunk of ONE row behind one and two full ones
@pytest.mark.parametrize("nv", [255, 257, 513])
@pytest.mark.parametrize("form", ["fp32_rows", "planes", "row_scaled_planes", "interleaved"])
def test_sparse_conv_f16x3(ops, lib, form, nv):
    cin, cout, kv = 32, 256, 27
    nm = geo(nv)["nm"]
    X, W, sc, sh, res = conv_inputs(nv, cin, cout, 1500 + nv)
    pairs = ops.conv_pairs_build(up(nm), 256)
    assert pairs.num_chunks == -(-nv // 256)
    n_tiles = int(pairs.chunk_tile_off[pairs.num_chunks])     # tile_start[nseg]: the tiles there are
    assert 0 < n_tiles <= pairs.num_pairs // 256 + pairs.nseg                                       # (the header's upper bound)
    p2 = 2.0 ** int(np.floor(np.log2(2.0 / float(W.abs().max()))))
    blocked = form != "planes"                               # w_blocked = 1 (the step-blocked halves) and 0 (row-major)
    w_hi, w_lo = ops.conv_weights_split(up(W), p2, blocked=blocked)
    scaled = form in ("row_scaled_planes", "interleaved")
    il = form == "interleaved"
    if form == "fp32_rows":
        x_eff, res_eff = X.double(), res.double()
    else:
        xs = ops.split_f16(up(X), per_row=True) if scaled else ops.split_f16(up(X)) + (None,)
        x_eff = (xs[0].double() + xs[1].double()).cpu() * (xs[2].double().cpu()[:, None] if scaled else 1.0)
        rs = ops.split_f16(up(res), per_row=True) if scaled else None
        res_eff = ((rs[0].double() + rs[1].double()) * rs[2].double()[:, None]).cpu() if scaled else None
    xp, yp = cin + 8, cout + 8                               # plane pitches; interleaved rows need whole 128-byte lines: 128 and 576 halves

    def case(a):
        # the pair tables at the header's extents: pair_in [num_pairs], tile_desc [tiles, 4] (what ops.conv_pairs_build allocates beyond
        # them is uninitialised slack that no kernel may read: a 256-pair tile's tail behind num_pairs lands in the poison)
        tabs = [a.inp(t, name=n) for t, n in ((pairs.pair_in[:pairs.num_pairs], "pair_in"), (pairs.pair_pos, "pair_pos"),
                                                (pairs.pair_off, "seg_off"), (pairs.tile_start, "tile_start"),
                                                (pairs.tile_desc[:n_tiles], "tile_desc"))]
        wh, wl = a.inp(w_hi.reshape(-1), name="w_hi"), a.inp(w_lo.reshape(-1), name="w_lo")
        partial = a.out(max(pairs.max_chunk_pairs, 1) * cout, F32, name="partial")                  # 4 * pairs of the largest chunk * cout bytes
        s_, b_ = a.inp(sc / p2, name="scale"), a.inp(sh, name="shift")
        x = xh = xl = xinv = r_ = rh = rl = rinv = y = yh = yl = yinv = None
        o = {}
        if form == "fp32_rows":
            x, r_ = a.inp(X, xp, "x"), a.inp(res, yp, "residual")
            y = o["y"] = a.out((nv, cout), F32, yp, "y")
        elif il:
            xh = a.inp(ops.interleave_planes(xs[0], xs[1]), 128, "x_rows")
            rh = a.inp(ops.interleave_planes(rs[0], rs[1]), 576, "res_rows")
            yh = o["y_rows"] = a.out((nv, 2 * cout), F16, 576, "y_rows")
        else:
            xh, xl = a.inp(xs[0], xp, "x_hi"), a.inp(xs[1], xp, "x_lo")
            yh, yl = a.out((nv, cout), F16, yp, "y_hi"), a.out((nv, cout), F16, yp, "y_lo")
            o["y_hi"], o["y_lo"] = yh, yl
            if scaled:
                rh, rl = a.inp(rs[0], yp, "res_hi"), a.inp(rs[1], yp, "res_lo")
                y = o["y"] = a.out((nv, cout), F32, yp, "y")                                       # the fp32 rows beside the planes
        if scaled:
            xinv, rinv = a.inp(xs[2], name="x_row_inv_scale"), a.inp(rs[2], name="res_row_inv_scale")
            yinv = o["y_row_inv_scale"] = a.out(nv, F32, name="y_row_inv_scale")
        flags = 7 if il else 0
        ok(lib, lib.gp_sparse_conv_f16x3(P(x), x.stride(0) if x is not None else 0, P(xh), P(xl), xh.stride(0) if xh is not None else 0,
                                         P(tabs[0]), P(tabs[1]), P(tabs[2]), P(tabs[3]), P(tabs[4]), pairs.nseg, pairs.num_pairs, nv, kv,
                                         P(wh), P(wl), cin, cout, P(partial), P(s_), P(b_), P(r_), r_.stride(0) if r_ is not None else 0, 1,
                                         P(y), y.stride(0) if y is not None else 0, P(yh), P(yl), yh.stride(0) if yh is not None else 0,
                                         pairs.num_chunks, pairs.chunk_row_off, pairs.chunk_tile_off, pairs.chunk_pair_off, P(xinv), P(yinv),
                                         P(rh), P(rl), rh.stride(0) if rh is not None else 0, P(rinv), int(blocked), flags, S()))
        return o

    r = run(case)
    for k, v in r.items():
        whole(v, k)
    ref = o_student.sparse_conv3(x_eff, nm.astype(np.int64), W.double()) * sc.double() + sh.double()
    ref = torch.relu(ref + res_eff if res_eff is not None else ref)
    if "y" in r:
        # test_sparse_conv_f16x3_matches_fp32_accuracy: 5e-5 against fp64 (err, err2)
        assert (r["y"].cpu().double() - ref).abs().max() < 5e-5
    if form != "fp32_rows":
        yh, yl = ops.deinterleave_planes(r["y_rows"]) if il else (r["y_hi"], r["y_lo"])
        back = (yh.cpu().double() + yl.cpu().double()) * (r["y_row_inv_scale"].cpu().double()[:, None] if scaled else 1.0)
        # ... and its bound between the planes and the fp32 rows: 2e-6 max(1, max |y|)
        assert (back - ref).abs().max() < 5e-5 + 2e-6 * max(1.0, float(ref.abs().max()))


# embed_head_kernel: 128 rows per workgroup, 32 per wave; A rows clamped to nv - 1, stores guarded by row < nv
@pytest.mark.parametrize("nv", [1, 33, 127, 129])
@pytest.mark.parametrize("form", ["rows", "planes", "planes_permuted", "planes_only"])
def test_embed_head_f16x3(ops, lib, form, nv):
    cin, cout = 64, 128
    g = torch.Generator().manual_seed(1600 + nv)
    X = torch.relu(torch.randn(nv, cin, generator=g)) * torch.exp(torch.randn(nv, 1, generator=g) * 3.0)
    if nv > 17:
        X[17] = 0.0                                          # F.normalize: 0 / max(0, 1e-12) = 0
    W = torch.randn(cin, cout, generator=g) * 0.04
    p2 = 2.0 ** int(np.floor(np.log2(16384.0 / float(W.abs().max()))))
    w_hi, w_lo = ops.conv_weights_split(up(W.reshape(1, cin, cout)), p2, blocked=False)
    xs = ops.split_f16(up(X), cin, per_row=True)
    perm = torch.randperm(nv, generator=g).to(I32)

    def case(a):
        xh, xl, xinv = a.inp(xs[0], cin + 8, "x_hi"), a.inp(xs[1], cin + 8, "x_lo"), a.inp(xs[2], name="x_row_inv_scale")
        wh, wl = a.inp(w_hi.reshape(cout, cin), name="w_hi"), a.inp(w_lo.reshape(cout, cin), name="w_lo")
        o = {}
        y = eh = el = dst = None
        if form != "planes_only":
            y = o["y"] = a.out((nv, cout), F32, cout + 8, "y")
        if form != "rows":
            eh, el = a.out((nv, cout), F16, name="e_hi"), a.out((nv, cout), F16, name="e_lo")
            o["e_hi"], o["e_lo"] = eh, el
        if form == "planes_permuted":
            dst = a.inp(perm, name="e_dst_row")
        ok(lib, lib.gp_embed_head_f16x3(P(xh), P(xl), xh.stride(0), P(xinv), P(wh), P(wl), nv, cin, cout, 1.0 / p2, 1, P(y),
                                        y.stride(0) if y is not None else 0, P(eh), P(el), 1024.0, P(dst), S()))
        return o

    r = run(case)
    for k, v in r.items():
        whole(v, k)
    ref = X.double() @ W.double()
    refn = ref / ref.norm(dim=1, keepdim=True).clamp_min(1e-12)
    if "y" in r:
        # test_embed_head_f16x3_matches_fp64_and_the_fp32_kernel: unit rows within 2e-6 of fp64 ...
        assert (r["y"].cpu().double() - refn).abs().max() < 2e-6
    if "e_hi" in r:
        eh, el = r["e_hi"], r["e_lo"]
        if form == "planes_permuted":                        # plane row e_dst_row[r] holds input row r
            eh, el = eh[perm.long().cuda()], el[perm.long().cuda()]
        if "y" in r:                                         # ... and the planes are the split of exactly those rows x 2^10
            sv = r["y"] * 1024.0
            assert torch.equal(eh, sv.half()) and torch.equal(el, (sv - sv.half().float()).half())
        else:                                                # without the fp32 rows: the same bound + the split's 2^-22
            assert ((eh.cpu().double() + el.cpu().double()) / 1024.0 - refn).abs().max() < 2e-6 + 2.0 ** -22


# ------------------------------------------------------------------------------------------ the fences bite
@pytest.mark.parametrize("entry", ["gp_gather_rows", "gp_split_f16"])
def test_a_call_over_one_more_row_trips_the_fence_at_row_n(ops, lib, entry):
    """Negative controls: an ordinary, valid call over n + 1 rows -- the index array and the input really hold n + 1 rows -- while the
    output fences enclose n.  Everything lands inside the test's allocation; the fence reports row n, and row n alone."""
    n, d = 16, 64
    g = torch.Generator().manual_seed(5)
    if entry == "gp_gather_rows":
        src = fence_in(torch.randn(40, d, generator=g).cuda(), d + 8)
        index = fence_in(torch.randint(0, 40, (n + 1,), generator=g).cuda())
        outs = [fenced(n, d, F32, pitch=d + 8, device="cuda")]
        ok(lib, lib.gp_gather_rows(P(src), src.stride(0), d, P(index), n + 1, None, P(outs[0]), outs[0].stride(0), S()))
        ins = [src, index]
    else:
        x = fence_in(torch.randn(n + 1, d, generator=g).cuda(), d + 8)
        outs = [fenced(n, d, F16, pitch=d + 8, device="cuda"), fenced(n, d, F16, pitch=d + 8, device="cuda")]
        ok(lib, lib.gp_split_f16(P(x), x.stride(0), d, n + 1, P(outs[0]), P(outs[1]), outs[0].stride(0), S()))
        ins = [x]
    torch.cuda.synchronize()
    assert_intact(*ins)
    for o in outs:
        assert unwritten(o) == 0                             # the n rows inside are written ...
        assert o.fence.changed_rows() == [n]                 # ... and so is row n, and nowhere else
        assert o.fence.changed() == (n, 0)
        with pytest.raises(AssertionError, match=rf"\(row {n}, column 0\)"):
            assert_intact(o)
        row = o.fence.ints()[o.fence.guard + n]
        assert bool((row[:d] != o.fence.poison).all()) and bool((row[d:] == o.fence.poison).all())      # its d columns, not its pitch columns
