"""The two-phase convolution (gp_sparse_conv_f16x3) against fp64 at its tile, width and exponent edges: the cases of tests/conv_cases.py
(proved to reach their branches by tests/test_conv_cases_host.py) on the device.

Exact cases: integers and powers of two, the fp64 reference is the answer, every output form must equal it bit for bit -- no element
is excused.  Random cases: a per-element bound against fp64,
    |err(u, c)| <= gamma 2^-22 [S(u, c) + sum_k Q_k(u, c)]        (+ 2^-22 max_c |y(u, c)| for outputs read back from f16 planes)
with S = sum |x| |w| |scale| and Q_k = the largest magnitude of partial row k inside c's 128-column quarter, times |scale| (what the 24-bit
partial rows are rounded against).  gamma is MEASURED: the worst ratio seen on an MI355X per width is in GAMMA_MEASURED below, the test
asserts twice that, and never more than the a-priori ceiling 3 cin / 4 + 27 + 4 (fp32 accumulation of 3 cin products, 27 additions, the
split, quantise and output roundings).  A dropped hi * lo term is 2^-12 relative PER PRODUCT -- 2^10 times the unit of this bound, hundreds
of times the asserted gamma -- and cannot hide in it.  The exact-fp32 kernel (ops.sparse_conv) passes the same bound with its own gamma.
"""
import numpy as np
import pytest
import torch

import conv_cases as cc
from extent_fence import INT_VIEW, POISON, assert_intact, bits, fence_in, fenced, unwritten
from oracle import conv_partial as o_cp

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
TABLE_MAPS = ["A", "B", "C"]
BLOCK_COUNT_CASES = [("A7", [(32, 256)]), ("A8", [(32, 256)])]          # one-row chunks of 7 and 8 tiles: grids of 7 and 8 workgroups

# worst err / (2^-22 [S + sum Q]) seen on an MI355X over maps A, B, C, D and every random form, per (cin, cout): (f16x3, exact-fp32 kernel)
# (the two 1280-column widths: the worst element is in the UNSCALED f16 planes -- no row scale beyond 1024 columns -- of map C's small rows;
# their fp32 rows stay at 0.8 - 1.0 like every other width)
GAMMA_MEASURED = {(32, 256): (0.920, 0.755), (64, 256): (0.750, 0.510), (96, 256): (0.767, 0.533), (160, 256): (0.652, 0.663),
                  (32, 512): (1.029, 0.731), (64, 512): (0.784, 0.727), (96, 512): (0.775, 0.705), (160, 512): (0.702, 0.661),
                  (32, 768): (1.021, 0.671), (96, 768): (0.796, 0.725), (32, 1024): (1.126, 0.724), (64, 1024): (0.904, 0.619),
                  (32, 1280): (2.772, 0.796), (160, 1280): (3.722, 0.736)}


def exact_params():
    return [(n, ci, co) for n in TABLE_MAPS for ci, co in cc.WIDTHS] + [(n, ci, co) for n, ws in BLOCK_COUNT_CASES for ci, co in ws]


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


def poisoned(shape, dtype):
    return torch.full(shape, POISON["out"][dtype], dtype=INT_VIEW[dtype], device="cuda").view(dtype)


_PAIRS = {}


def pairs_of(ops, name, chunk_rows="own"):
    m = cc.get_map(name)
    rows = m.chunk_rows if chunk_rows == "own" else chunk_rows
    if (name, rows) not in _PAIRS:
        p = ops.conv_pairs_build(torch.from_numpy(m.nm).cuda(), rows)
        assert list(p.chunk_row_off) == m.chunks(rows) and p.num_pairs == int((m.nm >= 0).sum())
        tiles = cc.tile_pairs_of(m.nm, m.chunks(rows))
        assert np.diff(np.array(list(p.chunk_tile_off))).tolist() == [len(t) for t in tiles]
        assert p.tile_desc[:list(p.chunk_tile_off)[-1], 2].cpu().tolist() == sum(tiles, [])          # the tile pair counts phase 1 is given
        _PAIRS[(name, rows)] = p
    return _PAIRS[(name, rows)]


def device_inputs(ops, d, exact):
    """every operand form of a case on the device.  exact: the crafted planes of ExactData; else what the split kernels make of X"""
    dev = "cuda"
    W = d.W.float().to(dev)
    i = dict(w1=ops.conv_weights_split(W, d.p2, blocked=True), w0=ops.conv_weights_split(W, d.p2, blocked=False),
             scale=d.kernel_scale().float().to(dev), shift=d.shift.float().to(dev), res=d.residual.float().to(dev), x=d.X.float().to(dev))
    if exact:
        c = lambda t3: tuple(t.to(dev) for t in t3)
        i["planes0"] = c(d.x_planes0[:2]) + (None,)
        i["planes"], i["res_planes"] = c(d.x_planes), c(d.res_planes)
    else:
        i["planes0"] = ops.split_f16(i["x"]) + (None,)
        i["planes"] = ops.split_f16(i["x"], per_row=True)
        i["res_planes"] = ops.split_f16(i["res"], per_row=True)
        rows, none, inv = ops.split_f16(i["x"], per_row=True, interleaved=True)
        assert torch.equal(rows, ops.interleave_planes(*i["planes"][:2])) and torch.equal(inv, i["planes"][2])
    i["il"] = (ops.interleave_planes(*i["planes"][:2]), None, i["planes"][2])
    i["res_il"] = (ops.interleave_planes(*i["res_planes"][:2]), None, i["res_planes"][2])
    return i


def conv(ops, pairs, i, cout, x, out, res="none", relu=False, blocked=True, rowscale=True, fp32_partials=False, reference_walk=False, outs=None):
    """one call; -> its outputs by name, in buffers that start poisoned (outs: the caller's).  out: f32 | planes | planes_f32 | il | il_f32"""
    nv = pairs.nv
    rowscale = rowscale and cout <= 1024 and out != "f32"
    if outs is None:
        outs = {}
        if out in ("f32", "planes_f32", "il_f32"):
            outs["y"] = poisoned((nv, cout), F32)
        if out.startswith("planes"):
            outs["y_hi"], outs["y_lo"] = poisoned((nv, cout), F16), poisoned((nv, cout), F16)
        if out.startswith("il"):
            outs["y_rows"] = poisoned((nv, 2 * cout), F16)
        if rowscale:
            outs["y_inv"] = poisoned((nv,), F32)
    w = i["w1"] if blocked else i["w0"]
    xs = None if x == "f32" else i[x]
    residual = {"none": None, "f32": i["res"], "planes": i["res_planes"], "il": i["res_il"]}[res]
    split = (outs["y_rows"], None) if "y_rows" in outs else ((outs["y_hi"], outs["y_lo"]) if "y_hi" in outs else None)
    ops.sparse_conv_f16x3(i["x"] if x == "f32" else None, pairs, w[0], w[1], scale=i["scale"], shift=i["shift"], residual=residual, relu=relu,
                          out=outs.get("y"), x_split=None if xs is None else xs[:2], out_split=split, x_row_inv=None if xs is None else xs[2],
                          out_row_inv=outs.get("y_inv"), want_f32="y" in outs, fp32_partials=fp32_partials, reference_walk=reference_walk)
    torch.cuda.synchronize()
    return outs


def values(ops, outs):
    """what the outputs say, as f64 on the host: {"y": fp32 rows, "split": (hi + lo) * row_inv}"""
    v = {}
    if "y" in outs:
        v["y"] = outs["y"].cpu().double()
    if "y_rows" in outs or "y_hi" in outs:
        hi, lo = ops.deinterleave_planes(outs["y_rows"].contiguous()) if "y_rows" in outs else (outs["y_hi"], outs["y_lo"])
        s = hi.cpu().double() + lo.cpu().double()
        v["split"] = s * outs["y_inv"].cpu().double()[:, None] if "y_inv" in outs else s
    return v


def same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = bits(a[k]), bits(b[k])
        if not torch.equal(x, y):
            at = (x != y).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {k} differs, first at {at} ({int((x != y).sum())} elements)")


def written(outs):
    for k, t in outs.items():
        assert unwritten(t) == 0, (k, unwritten(t))
    if "y_inv" in outs:
        inv = outs["y_inv"]
        assert bool(torch.isfinite(inv).all()) and float(inv.min()) > 0.0


# (x, out, residual, relu, blocked weights, fp32 partial rows, reference walk)
EXACT_FORMS = [("f32", "f32", "f32", True, True, False, False),
               ("planes0", "planes_f32", "none", False, False, False, False),
               ("planes", "planes_f32", "planes", True, True, False, False),
               ("il", "il", "il", False, True, False, False),
               ("planes", "planes_f32", "planes", True, True, True, False),
               ("il", "il_f32", "f32", True, False, True, False),
               ("il", "il", "il", False, False, False, True)]


@pytest.mark.parametrize("name,cin,cout", exact_params(), ids=[f"{n}-{ci}-{co}" for n, ci, co in exact_params()])
def test_exact_cases_equal_fp64(ops, name, cin, cout):
    """every operand and output form, chunked as the map asks and as one chunk: bit for bit the fp64 reference (cast to fp32)"""
    d = cc.exact_data(name, cin, cout)
    i = device_inputs(ops, d, exact=True)
    m = d.m
    no_pair = torch.from_numpy((m.nm >= 0).sum(0) == 0)
    got = {}
    for chunk_rows in ("own", None):
        pairs = pairs_of(ops, name, chunk_rows)
        for f in EXACT_FORMS:
            x, out, res, relu, blocked, f32p, refwalk = f
            if refwalk and cout > 512 and chunk_rows is None:
                continue                                               # (the wide form has one walk: this is the row-major run, once)
            outs = conv(ops, pairs, i, cout, x, out, res, relu, blocked, fp32_partials=f32p, reference_walk=refwalk)
            written(outs)
            ref = d.reference(res != "none", relu)
            for k, v in values(ops, outs).items():
                bad = v != ref
                assert not bool(bad.any()), (name, cin, cout, chunk_rows, f, k, int(bad.sum()), bad.nonzero()[0].tolist())
                if bool(no_pair.any()):                                  # rows that no offset hits: relu(shift + residual), exactly
                    e0 = d.shift + (d.residual[no_pair] if res != "none" else 0.0)
                    assert torch.equal(v[no_pair], torch.relu(e0) if relu else e0.expand(int(no_pair.sum()), -1))
            got[(chunk_rows, f)] = outs
    for f in EXACT_FORMS:
        if ("own", f) in got and (None, f) in got:
            same_bits(got[("own", f)], got[(None, f)], f"chunks against one chunk {f}")
    same_bits({"y": got[("own", EXACT_FORMS[2])]["y"]}, {"y": got[("own", EXACT_FORMS[4])]["y"]}, "24-bit against fp32 partial rows")
    if cout <= 512:
        same_bits(got[("own", EXACT_FORMS[3])], got[("own", EXACT_FORMS[6])], "pipelined against reference walk, blocked against row-major")


def test_out_row_inv_beyond_1024_columns_is_refused(ops):
    from geopurify_amd._lib import GeoPurifyHipError
    d = cc.exact_data("C", 32, 1280)
    i = device_inputs(ops, d, exact=True)
    pairs = pairs_of(ops, "C")
    outs = {"y_rows": poisoned((d.m.nv, 2 * 1280), F16), "y_inv": poisoned((d.m.nv,), F32)}
    with pytest.raises(GeoPurifyHipError, match="cout <= 1024"):
        ops.sparse_conv_f16x3(None, pairs, i["w1"][0], i["w1"][1], scale=i["scale"], x_split=i["il"][:2], x_row_inv=i["il"][2],
                              out_split=(outs["y_rows"], None), out_row_inv=outs["y_inv"], want_f32=False)
    torch.cuda.synchronize()
    assert all(unwritten(t) == t.numel() for t in outs.values())         # refused before any launch


# ------------------------------------------------------------------------------------------ random cases
def random_data(name, cin, cout, decades=True):
    return cc.RandomData(cc.get_map(name), cin, cout, 2000 + 7 * cin + cout, decades)


def worst_ratio(v, ref, unit, extra=None):
    """max |v - ref| / unit over the elements; where the unit is 0 (a row no pair reaches) the value must BE the reference"""
    err = (v - ref).abs()
    u = unit if extra is None else unit + extra
    zero = u == 0
    assert bool((err[zero] == 0).all())
    return float((err[~zero] / u[~zero]).max()) if bool((~zero).any()) else 0.0


# (decades, x, out, residual, relu, blocked weights, fp32 partial rows)
RANDOM_FORMS = [(False, "f32", "f32", "f32", True, True, False), (False, "il", "il_f32", "il", True, True, False),
                (True, "planes", "planes_f32", "planes", False, True, False), (True, "il", "il", "il", True, False, False),
                (True, "il", "il_f32", "f32", True, True, True)]
RANDOM_PARAMS = [(n, ci, co) for n in ("A", "B", "C", "D") for ci, co in cc.WIDTHS]


@pytest.mark.parametrize("name,cin,cout", RANDOM_PARAMS, ids=[f"{n}-{ci}-{co}" for n, ci, co in RANDOM_PARAMS])
def test_random_cases_within_the_bound(ops, name, cin, cout):
    """(see the module docstring)  Measured on an MI355X, worst ratio per width over the four maps and five forms (GAMMA_MEASURED):
    (cin, cout): 32,256 0.92  64,256 0.75  96,256 0.77  160,256 0.65  32,512 1.03  64,512 0.78  96,512 0.78  160,512 0.70  32,768 1.02
    96,768 0.80  32,1024 1.13  64,1024 0.90  32,1280 2.77  160,1280 3.72 (unscaled f16 planes; their fp32 rows 1.0), against 0.51 - 0.80 for
    the exact-fp32 kernel;
    the test asserts twice the width's figure, the ceiling 3 cin / 4 + 27 + 4 is 55 at cin 32.  One dropped hi * lo term of one product
    is 2^-12 of that product: 1024 units of the bound where the product carries its row."""
    m = cc.get_map(name)
    pairs = pairs_of(ops, name)
    no_pair = torch.from_numpy((m.nm >= 0).sum(0) == 0)
    worst = 0.0
    for decades in (False, True):
        d = random_data(name, cin, cout, decades)
        i = device_inputs(ops, d, exact=False)
        sc = d.scale.double()
        eff = lambda t3: (t3[0].cpu().double() + t3[1].cpu().double()) * t3[2].cpu().double()[:, None]
        assert torch.equal(eff(i["res_planes"]), d.residual.double())      # (13-bit mantissas: the planes hold them exactly)
        terms = {}
        for decades_f, x, out, res, relu, blocked, f32p in RANDOM_FORMS:
            if decades_f != decades:
                continue
            outs = conv(ops, pairs, i, cout, x, out, res, relu, blocked, fp32_partials=f32p)
            written(outs)
            key = "f32" if x == "f32" else "split"                           # the effective input: X, or (hi + lo) * row_inv of the planes
            if key not in terms:
                terms[key] = cc.conv_terms(m.nm, d.X.double() if x == "f32" else eff(i["planes"]), d.W.double(), want_bound=True)
            Y, S, Q = terms[key]
            unit = 2.0 ** -22 * (S + Q) * sc
            ref = cc.epilogue(Y, sc, d.shift.double(), d.residual.double() if res != "none" else None, relu)
            for k, v in values(ops, outs).items():
                extra = 2.0 ** -22 * ref.abs().amax(1, keepdim=True).expand_as(ref) if k == "split" else None
                r = worst_ratio(v, ref, unit, extra)
                print(f"GAMMA f16x3 {name} {cin} {cout} {decades}/{x}/{out}/{res}/{relu}/{blocked}/{f32p} {k} {r:.3f}")
                worst = max(worst, r)
            if bool(no_pair.any()) and "y" in outs:                          # rows without a pair, on random data: relu(shift + residual), exactly
                e0 = d.shift + (d.residual[no_pair] if res != "none" else 0.0)
                assert torch.equal(outs["y"].cpu()[no_pair], torch.relu(e0) if relu else e0)
        if not decades and m.kv == 27:                                       # margin: the exact-fp32 kernel on the same inputs, its own gamma
            Y, S, Q = terms["f32"]
            y32 = ops.sparse_conv(i["x"], torch.from_numpy(m.nm).cuda(), d.W.float().cuda(), d.scale.float().cuda(), i["shift"], residual=i["res"], relu=True)
            r32 = worst_ratio(y32.cpu().double(), cc.epilogue(Y, sc, d.shift.double(), d.residual.double(), True), 2.0 ** -22 * (S + Q) * sc)
            print(f"GAMMA fp32 {name} {cin} {cout} {r32:.3f}")
            g32 = GAMMA_MEASURED.get((cin, cout), (None, None))[1]
            assert r32 <= (cc.gamma_ceiling(cin) if g32 is None else min(2.0 * g32, cc.gamma_ceiling(cin))), r32
    g = GAMMA_MEASURED.get((cin, cout), (None, None))[0]
    limit = cc.gamma_ceiling(cin) if g is None else min(2.0 * g, cc.gamma_ceiling(cin))
    assert worst <= limit, (worst, limit)


def test_gamma_table_is_complete_and_under_the_ceiling():
    assert set(GAMMA_MEASURED) == set(cc.WIDTHS)
    for (cin, cout), (g, g32) in GAMMA_MEASURED.items():
        assert 0 < 2 * g <= cc.gamma_ceiling(cin) and 0 < 2 * g32 <= cc.gamma_ceiling(cin), (cin, cout)


# ------------------------------------------------------------------------------------------ equalities that need no reference
@pytest.mark.parametrize("cin,cout", [(64, 256), (32, 512), (96, 768), (32, 1280)])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_forms_agree_bit_for_bit(ops, name, cin, cout):
    """random data: blocked against row-major weights, chunks of 256 rows against one chunk, the pipelined against the reference walk"""
    d = random_data(name, cin, cout)
    i = device_inputs(ops, d, exact=False)
    base = conv(ops, pairs_of(ops, name, None), i, cout, "il", "il_f32", "il", True, True)
    written(base)
    same_bits(base, conv(ops, pairs_of(ops, name, None), i, cout, "il", "il_f32", "il", True, False), "row-major weights")
    same_bits(base, conv(ops, pairs_of(ops, name, 256), i, cout, "il", "il_f32", "il", True, True), "chunks of 256 rows")
    same_bits(base, conv(ops, pairs_of(ops, name, 256), i, cout, "il", "il_f32", "il", True, True, reference_walk=True), "reference walk")
    planes = conv(ops, pairs_of(ops, name, 256), i, cout, "planes", "planes_f32", "planes", True, True)
    assert torch.equal(bits(planes["y"]), bits(base["y"]))
    assert torch.equal(ops.interleave_planes(planes["y_hi"], planes["y_lo"]), base["y_rows"])


# ------------------------------------------------------------------------------------------ the exponent edges of the 24-bit rows
@pytest.mark.parametrize("cout", [256, 512])
def test_exponent_edges_byte_for_byte(ops, cout):
    e = cc.exponent_case(cout)
    pairs = ops.conv_pairs_build(torch.from_numpy(e.m.nm).cuda(), None)
    assert pairs.num_chunks == 1
    hi, lo = (t.cuda() for t in e.planes())
    w = ops.conv_weights_split(e.W.float().cuda(), 1.0)
    acc, ks, us, ins = e.accumulators()
    P = len(ks)
    assert P == pairs.num_pairs and np.array_equal(pairs.pair_in.cpu().numpy()[:P], ins)
    others = torch.arange(e.nv) != 7
    runs = {}
    for overflow in (True, False):
        inv, ex = e.x_row_inv(overflow)
        want_rows, want_E, want_y, dec = e.expected(overflow)
        for f32p in (False, True):
            for refwalk in ((False, True) if not f32p else (False,)):
                y = poisoned((e.nv, cout), F32)
                ops.sparse_conv_f16x3(None, pairs, w[0], w[1], x_split=(hi, lo), x_row_inv=inv.cuda(), out=y, fp32_partials=f32p, reference_walk=refwalk)
                torch.cuda.synchronize()
                runs[(overflow, f32p, refwalk)] = y.cpu()
                if not f32p:                                             # the bytes phase 1 left: rows and exponent bytes
                    raw = pairs.partial.view(torch.uint8).flatten().cpu().numpy()
                    e_off = o_cp.exponent_offset(P, cout)
                    assert np.array_equal(raw[e_off:e_off + want_E.size], want_E)
                    assert np.array_equal(raw[:want_rows.size], want_rows)
                    assert {0, 1 << 23} <= set(np.unique(o_cp.units(acc.float().numpy())).tolist()) and {22, 255 if overflow else 22} <= set(want_E.tolist())
        exact = torch.from_numpy(acc.numpy() * np.exp2(ex[ins].astype(np.float64))[:, None])
        y_exact = torch.zeros((e.nv, cout), dtype=F64).index_add_(0, torch.from_numpy(us), exact)
        for refwalk in (False, True):
            y = runs[(overflow, False, refwalk)]
            keep = others if overflow else torch.ones(e.nv, dtype=torch.bool)
            assert torch.equal(y[keep], want_y[keep].float())            # the decoded rows, summed: exact
            same = want_y[keep] == y_exact[keep]
            assert int((~same).sum()) == 5                               # all but the three edge maxima (half a unit) and the two elements below the clamp
            assert float(y[4, :cc.QUARTER].abs().max()) <= 2.0 ** -104 and float((y[4].double() - y_exact[4]).abs().max()) <= 2.0 ** -104
        assert torch.equal(runs[(overflow, True, False)][others], y_exact[others].float())      # fp32 partial rows: the products themselves
    for f32p, refwalk in ((False, False), (False, True), (True, False)):
        y, plain = runs[(True, f32p, refwalk)], runs[(False, f32p, refwalk)]
        finite = torch.isfinite(y).all(1)
        assert torch.equal(~finite, ~others)                             # non-finite in exactly the output row that gathers the pair row
        assert torch.equal(bits(y[others]), bits(plain[others])) and bool(torch.isfinite(plain).all())
    assert bool(torch.isnan(runs[(True, False, False)][7, :cc.QUARTER]).all()) and bool(torch.isinf(runs[(True, True, False)][7, 9]))


# ------------------------------------------------------------------------------------------ fences
@pytest.mark.parametrize("cout", [256, 512, 768, 1280])
def test_fenced_partial_rows_and_pitched_outputs(ops, cout):
    """map A inside guard bands: `partial` sized to exactly max_chunk_pairs x cout floats, pitched outputs, the pair positions fenced"""
    d = random_data("A", 32, cout)
    i = device_inputs(ops, d, exact=False)
    base = pairs_of(ops, "A")
    nv = base.nv
    plain = conv(ops, base, i, cout, "il", "il_f32", "il", True, True)
    pos = fence_in(base.pair_pos.reshape(-1))
    pairs = ops.ConvPairs(base.pair_in, pos.view(27, nv), base.pair_off, base.tile_start, base.nseg, base.num_pairs, nv)
    pairs.tile_desc = base.tile_desc
    pairs._set_chunks(list(base.chunk_row_off), list(base.chunk_tile_off), list(base.chunk_pair_off))
    pairs.partial = fenced(base.max_chunk_pairs, cout, F32, device="cuda")
    outs = {"y_rows": fenced(nv, 2 * cout, F16, pitch=2 * cout + 64, device="cuda"), "y": fenced(nv, cout, F32, pitch=cout + 8, device="cuda")}
    if cout <= 1024:
        outs["y_inv"] = fenced(nv, None, F32, device="cuda")
    x = (fence_in(i["il"][0]), None, fence_in(i["il"][2]))
    got = conv(ops, pairs, dict(i, il=x), cout, "il", "il_f32", "il", True, True, outs=outs)
    assert_intact(pos, pairs.partial, x[0], x[2], *outs.values())
    written(got)
    same_bits({k: v.clone() for k, v in got.items()}, plain, "fenced against plain")
