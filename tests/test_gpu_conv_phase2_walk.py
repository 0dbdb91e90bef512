"""Phase 2 of the two-phase convolution: the pipelined row walk against the reference walk, bit for bit.

conv_phase2_q24_kernel sums an output row's 24-bit partial rows in ascending offset order.  Its pipelined walk keeps the next row's first
batch of partial rows in flight while a row is decoded; the reference walk (plane_flags bit 5, ops.sparse_conv_f16x3(reference_walk=True))
holds one row at a time.  Both must write the same bits: the interleaved rows or the separate planes, y_row_inv_scale, and the fp32 rows
where they are written.  The lattice below is built so that the edges of the walk occur, and every case ASSERTS that they do:
  * partial rows per output row: every count from 1 (an isolated voxel) to 27 (the interior of a filled block) -- so NL - 1, NL, NL + 1,
    2 NL and 2 NL + 1 for every batch size NL the kernel was swept over (4, 6, 8);
  * chunks of 1, 3 and 257 rows, and of W - 1, W, W + 1 and 2 W + 1 rows for W = the waves of one resident grid at 3 and at 4 waves per
    SIMD (the grids the kernel was swept over; both walks run at 4): waves with no row, one row, two and three rows, and every "no next
    row" end;
  * a row count that is no multiple of 4, 64 or 256.
"""
import numpy as np
import pytest
import torch

from extent_fence import assert_intact, bits, fence_in, fenced
from oracle import student as o_student

pytestmark = pytest.mark.gpu

F16, F32, I32 = torch.float16, torch.float32, torch.int32
CIN = 32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import ops as _ops
    from geopurify_amd import _lib
    _lib.load()                      # fails loudly if the HIP library is missing
    return _ops


def resident_waves(per_simd):
    """waves of one resident phase-2 grid: 4 SIMDs per CU"""
    return 4 * per_simd * torch.cuda.get_device_properties(0).multi_processor_count


def morton_perm(c):
    q = (c.astype(np.int64) - c.astype(np.int64).min(0)).astype(np.uint64)
    key = np.zeros(len(c), np.uint64)
    for b in range(21):
        for ax in range(3):
            key |= ((q[:, ax] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + ax)
    return np.argsort(key, kind="stable")


_LATTICE = {}


def lattice(nv):
    """nv voxels in Morton order + their kernel map: a filled 5 x 5 x 5 block (27 partial rows inside), three random blobs of density
    0.25 / 0.5 / 0.8 (every count in between), isolated voxels (1), and a holed sheet that fills up to nv rows"""
    if nv not in _LATTICE:
        rng = np.random.default_rng(77)
        block = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3)
        blobs = []
        for i, dens in enumerate((0.25, 0.5, 0.8)):
            g = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), -1).reshape(-1, 3)
            blobs.append(g[rng.random(len(g)) < dens] + [20 + 15 * i, 0, 0])
        iso = np.array([[300, 5, 5], [330, 90, 41], [400, 1, 77], [-40, 3, 3]])
        fixed = np.unique(np.vstack([block] + blobs + [iso]), axis=0)
        sheet = np.stack(np.meshgrid(np.arange(140), np.arange(140), indexing="ij"), -1).reshape(-1, 2)
        sheet = sheet[rng.random(len(sheet)) < 0.7]
        sheet = np.c_[sheet[:, 0], sheet[:, 1] + 30, np.full(len(sheet), 50)]
        assert len(fixed) + len(sheet) >= nv, (len(fixed), len(sheet), nv)
        c = np.vstack([fixed, sheet[:nv - len(fixed)]]).astype(np.int32)
        cs = np.ascontiguousarray(c[morton_perm(c)])
        nm = o_student.build_kernel_map(cs).astype(np.int32)
        _LATTICE[nv] = (cs, nm)
    return _LATTICE[nv]


def the_nv():
    """rows for chunks of up to 2 W + 1 rows at 4 waves per SIMD, and no multiple of 4, 64 or 256"""
    nv = 2 * resident_waves(4) + 7
    assert nv % 4 and nv % 64 and nv % 256
    return nv


_INPUTS = {}


def inputs(ops, nv, cout, special=False):
    """x as row-scaled interleaved rows, the split weights, scale / shift and a residual in its three forms -- made once per width"""
    key = (nv, cout, special)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(900 + cout)
        X = torch.randn(nv, CIN, generator=g) * 3.0
        X[:, :8] *= 1e-3
        if special:
            X[11, 5] = float("inf")
            X[nv - 9, 17] = float("nan")
        W = torch.randn(27, CIN, cout, generator=g) * 0.05
        p2 = 2.0 ** int(np.floor(np.log2(2.0 / float(W.abs().max()))))
        res = torch.randn(nv, cout, generator=g)
        d = dict(x=ops.split_f16(X.cuda(), per_row=True, interleaved=True), w=ops.conv_weights_split(W.cuda(), p2),
                 scale=((torch.rand(cout, generator=g) + 0.5) / p2).cuda(), shift=torch.randn(cout, generator=g).cuda(), res=res.cuda())
        d["res_planes"] = ops.split_f16(d["res"], per_row=True)
        d["res_rows"] = ops.split_f16(d["res"], per_row=True, interleaved=True)
        _INPUTS[key] = d
    return _INPUTS[key]


_PAIRS = {}


def pairs_of(ops, nv, chunk_rows):
    if (nv, chunk_rows) not in _PAIRS:
        _PAIRS[(nv, chunk_rows)] = ops.conv_pairs_build(torch.from_numpy(lattice(nv)[1]).cuda(), chunk_rows)
    return _PAIRS[(nv, chunk_rows)]


def conv(ops, pairs, d, cout, residual, relu, out_form, reference, outs=None):
    """one layer; returns the outputs it wrote, by name.  outs: caller's buffers (the fenced case)"""
    nv = pairs.nv
    dev = "cuda"
    if outs is None:
        outs = {"y_row_inv_scale": torch.zeros(nv, dtype=F32, device=dev)}
        if out_form == "interleaved":
            outs["y_rows"] = torch.zeros((nv, 2 * cout), dtype=F16, device=dev)
        else:
            outs["y_hi"], outs["y_lo"] = torch.zeros((nv, cout), dtype=F16, device=dev), torch.zeros((nv, cout), dtype=F16, device=dev)
            outs["y"] = torch.zeros((nv, cout), dtype=F32, device=dev)
    res = {"none": None, "fp32": d["res"], "planes": d["res_planes"], "interleaved": d["res_rows"]}[residual]
    split = (outs["y_rows"], None) if "y_rows" in outs else (outs["y_hi"], outs["y_lo"])
    ops.sparse_conv_f16x3(None, pairs, d["w"][0], d["w"][1], scale=d["scale"], shift=d["shift"], residual=res, relu=relu, out=outs.get("y"),
                          x_split=(d["x"][0], None), out_split=split, x_row_inv=d["x"][2], out_row_inv=outs["y_row_inv_scale"],
                          want_f32="y" in outs, reference_walk=reference)
    torch.cuda.synchronize()
    return outs


def same_bits(a, b, what):
    for k in a:
        x, y = bits(a[k]), bits(b[k])
        if not torch.equal(x, y):
            at = (x != y).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {k} differs between the walks, first at {at} ({int((x != y).sum())} elements)")


def both_walks(ops, pairs, d, cout, residual, relu, out_form, what):
    ref = conv(ops, pairs, d, cout, residual, relu, out_form, True)
    got = conv(ops, pairs, d, cout, residual, relu, out_form, False)
    same_bits(ref, got, what)
    return ref


def test_lattice_has_every_partial_row_count(ops):
    nv = the_nv()
    counts = (lattice(nv)[1] >= 0).sum(0)
    assert set(range(1, 28)) <= set(counts.tolist()), sorted(set(range(1, 28)) - set(counts.tolist()))
    for nl in (4, 6, 8):
        assert {1, nl - 1, nl, nl + 1, 2 * nl, 2 * nl + 1, 27} <= set(counts.tolist())


@pytest.mark.parametrize("out_form", ["interleaved", "planes_f32"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("residual", ["none", "fp32", "planes", "interleaved"])
@pytest.mark.parametrize("cout", [256, 512])
def test_walks_agree_over_forms(ops, cout, residual, relu, out_form):
    nv = the_nv()
    pairs = pairs_of(ops, nv, 257)
    assert nv % 257 and pairs.num_chunks == -(-nv // 257)
    r = both_walks(ops, pairs, inputs(ops, nv, cout), cout, residual, relu, out_form, f"{cout} {residual} {relu} {out_form}")
    assert all(bool(torch.isfinite(v.float()).all()) for v in r.values())
    assert float(r["y_row_inv_scale"].min()) > 0.0          # (written: the buffers start as zeros)


# None: one chunk; "lastN": one large chunk and a last one of N rows; (w, k): chunks of k rows, W = w waves per CU (3 and 4 per SIMD)
CHUNKINGS = [None, "last1", "last3", 257] + [(w, k) for w in (12, 16) for k in ("W-1", "W", "W+1", "2W+1")]


@pytest.mark.parametrize("cout", [256, 512])
@pytest.mark.parametrize("chunking", CHUNKINGS, ids=["one_chunk", "last1", "last3", "257"] + [f"{w}perCU_{k}" for w in (12, 16) for k in ("W-1", "W", "W+1", "2W+1")])
def test_walks_agree_at_chunk_edges(ops, chunking, cout):
    nv = the_nv()
    if chunking is None or isinstance(chunking, int):
        rows, want = chunking, None
    elif isinstance(chunking, str):
        want = int(chunking[4:])
        rows = nv - want                                     # one large chunk, then a last chunk of 1 or 3 rows
    else:
        W = chunking[0] * torch.cuda.get_device_properties(0).multi_processor_count
        want = {"W-1": W - 1, "W": W, "W+1": W + 1, "2W+1": 2 * W + 1}[chunking[1]]
        rows = want
    pairs = pairs_of(ops, nv, rows)
    heights = np.diff(np.array(list(pairs.chunk_row_off)))
    if want is not None:
        assert want in heights.tolist(), (want, heights.tolist())
    else:
        assert (pairs.num_chunks == 1) if rows is None else (257 in heights.tolist() and nv % 257 in heights.tolist())
    both_walks(ops, pairs, inputs(ops, nv, cout), cout, "planes", True, "interleaved", f"chunks of {rows}")


@pytest.mark.parametrize("cout", [256, 512])
def test_walks_agree_on_inf_and_nan_rows(ops, cout):
    nv = the_nv()
    nm = lattice(nv)[1]
    pairs = pairs_of(ops, nv, 257)
    r = both_walks(ops, pairs, inputs(ops, nv, cout, special=True), cout, "none", False, "planes_f32", "inf / nan")
    # the output rows that read input row 11 (Inf) or nv - 9 (NaN) are the rows that are not finite, under both walks (same_bits above)
    touched = torch.from_numpy(((nm == 11) | (nm == nv - 9)).any(0))
    bad = ~torch.isfinite(r["y"]).all(1).cpu()
    assert bool(touched.any()) and torch.equal(bad, touched)
    nan_rows = torch.from_numpy((nm == nv - 9).any(0))
    assert bool(torch.isnan(r["y"].cpu()[nan_rows]).all())


def test_walks_keep_the_fences(ops):
    """The partial rows, pair_pos and the outputs inside poisoned guard bands: both walks leave every band untouched and write the same
    bits (a walk that loaded past the chunk's partial rows or past pair_pos would sum the poison NaN into its rows)."""
    nv, cout = the_nv(), 512
    base = pairs_of(ops, nv, resident_waves(3) + 1)
    d = inputs(ops, nv, cout)
    got = []
    for reference in (True, False):
        pos = fence_in(base.pair_pos.reshape(-1))
        pairs = ops.ConvPairs(base.pair_in, pos.view(27, nv), base.pair_off, base.tile_start, base.nseg, base.num_pairs, nv)
        pairs.tile_desc = base.tile_desc
        pairs._set_chunks(list(base.chunk_row_off), list(base.chunk_tile_off), list(base.chunk_pair_off))
        pairs.partial = fenced(base.max_chunk_pairs, cout, F32, device="cuda")
        outs = {"y_rows": fenced(nv, 2 * cout, F16, pitch=2 * cout + 64, device="cuda"), "y_row_inv_scale": fenced(nv, None, F32, device="cuda"),
                "y": fenced(nv, cout, F32, pitch=cout + 8, device="cuda")}
        conv(ops, pairs, d, cout, "interleaved", True, "interleaved", reference, outs=outs)
        assert_intact(pos, pairs.partial, *outs.values())
        got.append({k: v.clone() for k, v in outs.items()})
    same_bits(got[0], got[1], "fenced")
    plain = conv(ops, base, d, cout, "interleaved", True, "interleaved", False)
    same_bits({k: got[0][k] for k in plain}, plain, "fenced against plain")
