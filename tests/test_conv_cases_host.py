"""The cases of tests/conv_cases.py reach the branches they are meant for -- proved here without a device, on the maps and the fp64
references alone; tests/test_gpu_conv_edges.py then runs them."""
import numpy as np
import pytest
import torch

import conv_cases as cc
from oracle import conv_partial as o_cp

SYNTHETIC = ["A3", "A7", "A8", "B"]


@pytest.mark.parametrize("name", SYNTHETIC)
def test_synthetic_maps_are_what_was_asked_for(name):
    m = cc.get_map(name)
    nm = m.nm
    assert nm.dtype == np.int32 and nm.min() == -1 and nm.max() == m.nv - 1 and (nm == 0).any()          # rows 0 and nv - 1 are inputs
    assert cc.tile_pairs_of(nm, m.chunks()) == m.tile_pairs                                             # the tile pair counts
    assert np.array_equal((nm >= 0).sum(0), m.partial_rows)                                              # partial rows per output row
    ins = nm[nm >= 0]
    assert len(np.unique(ins)) < len(ins) // 4                                                           # input rows repeat
    ks, us, ins = cc.pair_order(nm, m.chunks())
    first = 0
    full_same = 0
    for tiles in m.tile_pairs:
        for cnt in tiles:
            full_same += cnt == cc.TM and len(set(ins[first:first + cnt].tolist())) == 1
            first += cnt
    assert first == len(ins) and full_same >= 1                                                          # a tile whose 256 pairs gather one row


def test_map_a_tiles_chunks_and_rows():
    m = cc.get_map("A")
    assert m.nv == 3 * 256 + 1 and m.chunks() == [0, 256, 512, 768, 769]
    per_offset = (m.nm[:, :256] >= 0).sum(1).tolist()
    assert set(cc.EDGE_COUNTS) <= set(per_offset)
    tiles = cc.tile_pairs_of(m.nm, m.chunks())
    assert set(cc.EDGE_COUNTS) - {0} <= set(tiles[0])
    assert tiles[1] == [] and not (m.nm[:, 256:512] >= 0).any()                                          # a chunk with no pair
    assert tiles[2] == [256] and sorted((m.nm[:, 512:768] >= 0).sum(1).tolist())[:26] == [0] * 26         # one offset at 256, the rest 0
    assert tiles[3] == [1, 1, 1]                                                                         # the one-row chunk
    nrt = {v for t in sum(tiles, []) for v in cc.nrt_of(t)}
    assert nrt == {0, 1, 2, 3, 4}                                                                        # every copy of the K loop
    for cnt, want in ((1, [1, 0, 0, 0]), (16, [1, 0, 0, 0]), (17, [2, 0, 0, 0]), (63, [4, 0, 0, 0]), (65, [4, 1, 0, 0]), (129, [4, 4, 1, 0]),
                      (191, [4, 4, 4, 0]), (193, [4, 4, 4, 1]), (255, [4, 4, 4, 4]), (256, [4, 4, 4, 4])):
        assert cc.nrt_of(cnt) == want
    assert {0, 1, 3, 4, 5, 8, 9} <= set(m.partial_rows.tolist())
    assert (m.partial_rows[256:512] == 0).all() and (m.partial_rows[:256] >= 1).all()


def test_map_b_long_segments():
    m = cc.get_map("B")
    assert m.nv == 600 and m.chunks() == [0, 600]
    assert {257, 511, 512, 513, 600} <= set((m.nm >= 0).sum(1).tolist())
    t = m.tile_pairs[0]
    assert any(t[i:i + 2] == [256, 1] for i in range(len(t))) and any(t[i:i + 3] == [256, 256, 1] for i in range(len(t)))
    assert any(t[i:i + 3] == [256, 256, 88] for i in range(len(t)))
    nb = cc.P2_BATCH
    assert {1, nb - 1, nb, nb + 1, 2 * nb, 2 * nb + 1, 27} <= set(m.partial_rows.tolist())


def test_block_counts_1_to_9_and_column_tiles():
    """phase 1 launches tile_count x n_tiles workgroups per chunk, rounded up to 8 and remapped over the XCDs: every count 1 .. 9 occurs
    for some (map, chunk, cout) that the device module runs"""
    from test_gpu_conv_edges import BLOCK_COUNT_CASES, TABLE_MAPS
    seen = {}
    for name, widths in [(n, cc.WIDTHS) for n in TABLE_MAPS] + BLOCK_COUNT_CASES:
        m = cc.get_map(name)
        for tiles in cc.tile_pairs_of(m.nm, m.chunks()):
            for cin, cout in widths:
                seen.setdefault(len(tiles) * (cout // cc.TN), (name, cout))
    assert set(range(1, 10)) <= set(seen), sorted(seen)
    assert 0 in seen                                                    # the chunk that launches no phase 1
    assert {cout // cc.TN for _, cout in cc.WIDTHS} == {1, 2, 3, 4, 5}  # n_tiles 3 and 5 among them
    assert {cin // cc.TK for cin, _ in cc.WIDTHS} == {1, 2, 3, 5}       # K-loop steps
    for cout in (256, 512, 768, 1024, 1280):
        cins = {ci for ci, co in cc.WIDTHS if co == cout}
        assert 32 in cins and any(ci > 32 for ci in cins)
    for cin in (32, 64, 96, 160):
        assert {256, 512} <= {co for ci, co in cc.WIDTHS if ci == cin}


def test_map_c_and_d():
    c = cc.get_map("C")
    assert c.kv == 1 and c.nv == 300 and 80 <= int((c.nm < 0).sum()) <= 120 and (c.nm == 0).any() and (c.nm == 299).any()
    d = cc.get_map("D")
    assert d.kv == 27 and 650 <= d.nv <= 750 and (d.nm[13] == np.arange(d.nv)).all()
    assert int((d.nm >= 0).sum(0).max()) >= 2 * cc.P2_BATCH + 1


EXACT_CASES = [(n, ci, co) for n in ("A", "B", "C") for ci, co in cc.WIDTHS] + [("A7", 32, 256), ("A8", 32, 256)]


@pytest.mark.parametrize("name,cin,cout", EXACT_CASES, ids=[f"{n}-{ci}-{co}" for n, ci, co in EXACT_CASES])
def test_exact_cases_are_exact(name, cin, cout):
    d = cc.exact_data(name, cin, cout)
    for chunk_rows in ("own", None):
        r = cc.exactness(d, d.m.chunks(chunk_rows))
        assert r["partial"] and r["sums"] and r["outputs"], r
        assert r["partial_span"] < 2.0 ** 22 and r["output_span"] < 2.0 ** 21, r
    for residual in (False, True):
        for relu in (False, True):
            y = d.reference(residual, relu)
            assert torch.equal(y.float().double(), y)                   # the reference equals its fp32 rounding
    # the crafted planes carry the same values, with a lo plane that is not all zero
    for (hi, lo, inv), v in ((d.x_planes, d.X), (d.res_planes, d.residual)):
        assert torch.equal((hi.double() + lo.double()) * inv.double()[:, None], v) and bool((lo != 0).any())
        assert set(np.log2(inv.numpy()).tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}


def test_no_exact_case_is_skipped():
    from test_gpu_conv_edges import exact_params
    assert sorted(set(exact_params())) == sorted(set(EXACT_CASES))


@pytest.mark.parametrize("cout", [256, 512])
def test_exponent_cases_reach_the_format_edges(cout):
    e = cc.exponent_case(cout)
    acc, ks, us, ins = e.accumulators()
    assert cc.is_fp32(acc)                                              # one exact product per element
    a32 = acc.float().numpy()
    nq = cout // cc.QUARTER
    row = {i: int(np.nonzero((ks == cc.K_STAR) & (us == i))[0][0]) for i in range(8)}
    assert all(ins[row[i]] == cc.SPECIAL_IN + i for i in range(8)) and all((e.m.nm[:, i] >= 0).sum() == 1 for i in range(8))
    seg = np.nonzero(ks == cc.K_STAR)[0]
    assert len(seg) == 208 and len(seg) <= cc.TM                        # the special pair rows share ONE tile with ordinary ones
    mant = lambda v: int(np.abs(np.float32(v)).view(np.uint32)) & 0x7fffff
    q0 = lambda i: a32[row[i], :cc.QUARTER]
    assert mant(np.abs(q0(0)).max()) == 0x7fffff and mant(np.abs(q0(1)).max()) == 0x7ffffe and q0(1).max() == -q0(1).min()
    assert not q0(2).any() and a32[row[2], cc.QUARTER:].any() and not a32[row[3]].any()
    rows, E, y, dec = e.expected()
    E = E.reshape(-1, nq).astype(int)
    u = o_cp.units(a32)
    Em = o_cp.exponents(a32)
    assert Em[row[0], 0] == 127 + 12 and E[row[0], 0] == 139            # the all-ones mantissa takes the next exponent
    assert u[row[1], 0].max() == 1 << 23 and u[row[1], 0].min() == 0    # u = 2^23 and u = 0
    assert E[row[1], 0] == 138 and dec[row[1], 5] == 2.0 ** 12 and dec[row[1], 6] == -2.0 ** 12
    assert E[row[2], 0] == 22 and (u[row[2], 0] == 1 << 22).all() and (E[row[3]] == 22).all()          # E = 22 for zero quarters
    assert Em[row[4], 0] - 90 < 22 and E[row[4], 0] == 22 and E[row[4], 1] > 22                         # ... and below the clamp
    assert float(np.abs(a32[row[4], :cc.QUARTER]).max()) * 2.0 ** -90 == 2.0 ** -110
    assert float(dec[row[4], :cc.QUARTER].abs().max()) < 2.0 ** -104
    assert (E[row[5]] == Em[row[5]] - 60).all() and (E[row[6]] == Em[row[6]] + 60).all()
    assert E[row[7], 0] == 255 and np.isfinite(a32[row[7]]).all() and Em[row[7], 0] + 120 > 254         # E = 255 through the row scale
    assert bool(torch.isnan(y[7]).any()) and bool(torch.isfinite(y[torch.arange(e.nv) != 7]).all())
    # every special quarter sits next to an ordinary one, and every other pair row is ordinary
    ordinary = np.ones(len(ks), bool)
    ordinary[list(row.values())] = False
    assert ((E[ordinary] >= 127) & (E[ordinary] <= 131)).all() and all(127 <= E[row[i], nq - 1] <= 131 for i in (0, 1, 2))
    # where nothing is clamped or marked, the decoded rows are the products themselves, except the three edge maxima (within half a unit)
    exact = torch.from_numpy(a32.astype(np.float64) * np.exp2(e.x_row_inv()[1][ins].astype(np.float64))[:, None])
    diff = (dec - exact).abs()
    diff[row[7]] = 0.0
    diff[row[4], :cc.QUARTER] = 0.0
    assert float(diff[row[0], 17]) == 2.0 ** -12 and float(diff[row[1], 5]) == float(diff[row[1], 6]) == 2.0 ** -11 and int((diff != 0).sum()) == 3
    # the whole-format restatement keeps what the earlier one stated: random finite rows decode within half a unit
    v = (np.random.default_rng(0).standard_normal((50, cout)) * np.exp(np.random.default_rng(1).standard_normal((50, 1)) * 8)).astype(np.float32)
    r2, E2 = o_cp.encode(v)
    d2 = o_cp.decode(r2, E2, 50, cout)
    assert (np.abs(d2 - v).reshape(50, nq, -1) <= np.exp2(E2.reshape(50, nq).astype(np.float64) - 149.0)[:, :, None]).all()


def test_gamma_ceiling():
    assert [cc.gamma_ceiling(c) for c in (32, 64, 96, 160)] == [55, 79, 103, 151]
