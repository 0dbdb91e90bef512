"""The cases of tests/lattice_cases.py on the host: the numpy model of gp_knn_lattice's ladder reaches, in every case, the path the
case is named for, and its lists equal the reference's (oracle.affinity.knn_lattice), which alone judges the GPU; the span and tie
cases discriminate (a key of the low 10-bit group alone, a tie-break by Morton row, would give other results); rcb_reference keeps
the promises of gp_rcb_order's header on the new inputs; the visibility model equals oracle.project's mapper, view by view."""
import functools

import numpy as np
import pytest

import lattice_cases as lc
from oracle import project as o_proj


def test_lattice_shells_have_the_stated_sizes():
    assert len(lc.shell(74)) == 120 and 74 < 81 and len(lc.shell(314)) == 312 > lc.KNN_MAXTIE and 314 < 25 ** 2
    assert len(lc.case("ties120")[0]) == 126 and len(lc.case("ties312")[0]) == 323


# ------------------------------------------------------------------------------------------ the ladder
@functools.lru_cache(maxsize=None)
def ladder(name):
    g = lc.geometry(name)
    return lc.ladder(g["v"], g["K"])


def counts(name):
    path = ladder(name)[1]
    return tuple(int((path == t).sum()) for t in (lc.RING1, lc.RING3, lc.EXHAUSTIVE))


@pytest.mark.parametrize("name", list(lc.CASES))
def test_model_equals_oracle(name):
    g = lc.geometry(name)
    lists, path = ladder(name)
    assert np.array_equal(lists, g["ref"]) and (path >= 0).all()
    assert (g["ref"] != np.arange(len(g["v"]))[:, None]).all()                 # no list holds its own row
    assert len(g["v"]) > g["K"] and np.array_equal(np.sort(g["perm"]), np.arange(len(g["v"])))


SIZES = {"negative_cube": (729, 20), "dense_cells_k127": (2048, 127), "dense_cells_k1": (2048, 1), "ties120": (126, 16),
         "ties312": (323, 20), "clusters": (112, 20), "nv_k_plus_1": (21, 20), "surface_257_k96": (257, 96), "span1031": (1715, 20),
         "span32768_x": (375, 20), "span32768_z": (375, 20)}


def test_every_case_has_its_shape_and_reaches_its_path():
    for name, (nv, K) in SIZES.items():
        v, k = lc.case(name)
        assert (len(v), k) == (nv, K), name
    # all on ring 1: the cubes, the full cells (27 x 512 candidates, K + 1 = 128 winners)
    assert counts("negative_cube") == (729, 0, 0)
    assert counts("dense_cells_k127") == (2048, 0, 0) and counts("dense_cells_k1") == (2048, 0, 0)
    for name in lc.SPAN_CASES:
        assert counts(name)[0] == SIZES[name][0], name
    v, _ = lc.case("negative_cube")
    assert v.max() <= 0 and (v[:, [0, 2]] < 0).all() and (v.min(0) % 8 != 0).any()     # nothing positive, the origin not cell-aligned
    # four FULL cells from the grid's origin = min: every bitmap word all ones
    v, _ = lc.case("dense_cells_k127")
    cells, n = np.unique((v.astype(np.int64) - v.min(0)) >> 3, axis=0, return_counts=True)
    assert len(cells) == 4 and (n == 512).all() and v[:, :2].min() < 0
    # 120 ties at the 17th neighbour: ring 1 answers the centre; 11 are kept
    v, K = lc.case("ties120")
    centre = lc.row_of(v, lc.TIES120_CENTRE)
    assert ladder("ties120")[1][centre] == lc.RING1
    ref = lc.geometry("ties120")["ref"][centre]
    d2 = ((v[ref].astype(np.int64) - lc.TIES120_CENTRE) ** 2).sum(1)
    assert (d2[:5] == 1).all() and (d2[5:] == 74).all() and len(d2[5:]) == 11 and (np.diff(ref[5:]) > 0).all()
    # 312 ties at the 21st: ring 1 144 queries, ring 3 178, exhaustive exactly the centre
    assert counts("ties312") == (144, 178, 1)
    v, K = lc.case("ties312")
    centre = lc.row_of(v, lc.TIES312_CENTRE)
    assert ladder("ties312")[1][centre] == lc.EXHAUSTIVE
    ref = lc.geometry("ties312")["ref"][centre]
    d2 = ((v[ref].astype(np.int64) - lc.TIES312_CENTRE) ** 2).sum(1)
    assert (d2[:10] <= 2).all() and (d2[10:] == 314).all() and (np.diff(ref[10:]) > 0).all()
    # the far-apart clusters: every query handed on twice
    assert counts("clusters") == (0, 0, 112)
    # K + 1 = nv: every list is the whole set; ring 3 and the exhaustive kernel both answer
    r1, r3, ex = counts("nv_k_plus_1")
    assert r3 > 0 and ex > 0
    ref = lc.geometry("nv_k_plus_1")["ref"]
    assert all(sorted(ref[i].tolist() + [i]) == list(range(21)) for i in range(21))
    # one row more than a 256-thread block, both rings populated, negative coordinates
    r1, r3, ex = counts("surface_257_k96")
    assert r1 > 0 and r3 > 0 and lc.case("surface_257_k96")[0].min() < 0


@pytest.mark.parametrize("name", ["ties120", "ties312"])
def test_tie_cases_tell_input_rows_from_morton_rows(name):
    """gp_knn_lattice works on Morton rows and breaks ties by ids = the input row: a kernel that broke them by its own row would keep
    another set of the centre's ties"""
    g = lc.geometry(name)
    v, K = g["v"], g["K"]
    centre = lc.row_of(v, lc.TIES120_CENTRE if name == "ties120" else lc.TIES312_CENTRE)
    rank = np.empty(len(v), np.int64)
    rank[g["perm"]] = np.arange(len(v))
    by_input, n_ties = lc.kept_ties(v, K, centre, np.arange(len(v)))
    by_morton, _ = lc.kept_ties(v, K, centre, rank)
    assert n_ties == (120 if name == "ties120" else 312) and len(by_input) == len(by_morton) == K - (5 if name == "ties120" else 10)
    assert by_input != by_morton
    assert by_input <= set(g["ref"][centre].tolist())
    # ids = NULL: the reference on the Morton rows keeps the other set
    cs_centre = int(rank[centre])
    assert {int(g["perm"][r]) for r in g["ref_sorted"][cs_centre]} >= by_morton


@pytest.mark.parametrize("name", list(lc.SPAN_CASES))
def test_span_cases_discriminate(name):
    g = lc.geometry(name)
    v, cs, edge = g["v"], g["cs"].astype(np.int64), lc.SPAN_CASES[name]
    lo, ext = lc.tight_box(v)
    assert ext.max() == (32768 if name != "span1031" else 1027) and (name != "span1031" or (ext >= 1027).all())
    cells = np.prod(((ext - 1) >> 3) + 1)
    assert cells * 4 <= 9 * 2 ** 20                                           # the grid's cell index stays at or below 9 MB
    # a key of the low 10 bits per axis alone orders the rows differently
    assert not np.array_equal(lc.morton_perm(v), lc.morton_perm(v, bits=10))
    # a kernel-map pair and a kNN list join voxels on opposite sides of the boundary
    side = (cs - lo) >= edge
    nm = g["nm"]
    hit = nm >= 0
    assert (side[np.where(hit, nm, 0)] != side[None, :, :]).any(-1)[hit].any()
    side_v = (v.astype(np.int64) - lo) >= edge
    assert (side_v[g["ref"]] != side_v[:, None, :]).any(-1).any()


@pytest.mark.parametrize("name", lc.EXPLICIT_BOX_CASES)
def test_loose_box_changes_cells_not_lists(name):
    g = lc.geometry(name)
    origin, extent = lc.loose_box(g["v"])
    tight = lc.tight_box(g["v"])[1]
    assert (extent <= 32768).all() and (extent >= tight).all() and (extent > tight).any() and (extent % 8 != 0).any()
    assert (((extent - 1) >> 3) > ((tight - 1) >> 3)).any()                   # an extra layer of empty cells
    lists, _ = lc.ladder(g["v"], g["K"], origin, extent)
    assert np.array_equal(lists, g["ref"])


# ------------------------------------------------------------------------------------------ gp_rcb_order
@pytest.mark.parametrize("chunk,leaf", lc.RCB_SHAPES)
@pytest.mark.parametrize("name", list(lc.RCB_INPUTS))
def test_rcb_reference_keeps_the_header_promises(name, chunk, leaf):
    cs, nbr = lc.rcb_input(name)
    nv = len(cs)
    assert nv == {"plane": 2304, "column": 2400, "wide_chunk": 1300}[name] and nbr.shape == (nv, lc.RCB_K)
    assert np.array_equal(cs, cs[lc.morton_perm(cs)])                         # Morton-sorted
    sigma = lc.rcb_sigma(name, chunk, leaf)
    assert np.array_equal(np.sort(sigma), np.arange(nv)) and np.array_equal(sigma // chunk, np.arange(nv) // chunk)
    for base in range(0, nv, chunk):
        leaves = lc.rcb_leaves(min(chunk, nv - base), leaf)
        assert all(n == leaf for n in leaves[:-1]) and 0 < leaves[-1] <= leaf


def test_rcb_inputs_reach_their_edges():
    # tails: longer than a leaf after a full chunk, and no multiple of the leaf
    tails = {(n, chunk, leaf): len(lc.rcb_input(n)[0]) % chunk for n in lc.RCB_INPUTS for chunk, leaf in lc.RCB_SHAPES}
    assert tails[("plane", 2048, 128)] == 256 and tails[("column", 2048, 128)] == 352 and tails[("column", 1024, 128)] == 352
    for chunk in (1024, 2048):
        assert any(t > leaf and t % leaf and len(lc.rcb_input(n)[0]) > chunk for (n, c, leaf), t in tails.items() if c == chunk)
    # plane: the extents of x and y tie in chunk 0, the lower axis wins -- the first cut separates x, not y
    cs, _ = lc.rcb_input("plane")
    for chunk, leaf in lc.RCB_SHAPES:
        first = cs[:chunk].astype(np.int64)
        ext = first.max(0) - first.min(0)
        assert ext[0] == ext[1] > ext[2] == 0
        sigma = lc.rcb_sigma("plane", chunk, leaf)
        a, b = cs[sigma[:chunk // 2]], cs[sigma[chunk // 2:chunk]]
        assert a[:, 0].max() <= b[:, 0].min() and a[:, 1].max() > b[:, 1].min()
        assert len(np.unique(first[:, 0])) < chunk // 16                      # thousands of equal coordinates along the cut axis
    # column: the largest extent on z, in the 2048-row chunk and in the set's last 352 rows
    cs, _ = lc.rcb_input("column")
    for rows in (cs[:2048].astype(np.int64), cs[2048:].astype(np.int64)):
        ext = rows.max(0) - rows.min(0)
        assert ext[2] > ext[0] > ext[1] == 0
    # wide_chunk: in a 2048-row chunk (all 1300 rows) the coordinate along the first cut axis reaches 32767 = the end of the key's
    # 15-bit field; the last 276 rows, a 1024-row chunk's tail, still use its top bit
    cs, _ = lc.rcb_input("wide_chunk")
    assert cs[:, 0].max() - cs[:, 0].min() == 32767 and cs[1024:, 0].max() - cs[1024:, 0].min() >= 2 ** 14


# ------------------------------------------------------------------------------------------ Part B: the visibility model
def mapper_entries(with_depth):
    """oracle.project._project + _finish per view, compacted by hand"""
    c = lc.vis_case()
    pt, x, y, view, off = [], [], [], [], [0]
    for v in range(lc.VIS_V):
        M, (fx, fy, cx, cy) = c["params"][v, :16].reshape(4, 4), c["params"][v, 16:]
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
        with np.errstate(all="ignore"):
            p, pi = o_proj._project(M, c["coords"], K)
            m = o_proj._finish(p, pi, (lc.VIS_W, lc.VIS_H), lc.VIS_CUT, c["depth"][v] if with_depth else None, lc.VIS_TAU)
        idx = np.flatnonzero(m[:, 2])
        pt.append(idx), x.append(m[idx, 0]), y.append(m[idx, 1]), view.append(np.full(len(idx), v))
        off.append(off[-1] + len(idx))
    return dict(pt=np.concatenate(pt), x=np.concatenate(x), y=np.concatenate(y), view=np.concatenate(view), view_off=np.array(off))


@pytest.mark.parametrize("with_depth", [True, False])
def test_visibility_model_equals_the_mapper(with_depth):
    got, want = lc.vis_entries(with_depth), mapper_entries(with_depth)
    for k, a in want.items():
        assert np.array_equal(got[k], a), k


def test_visibility_case_sits_on_the_keep_boundaries():
    c = lc.vis_case()
    assert c["coords"].shape == (700, 3) and 700 % 256 and (700 * 5) % 256
    e = lc.vis_entries()
    n = np.diff(e["view_off"])
    assert tuple(n) == lc.VIS_COUNTS == (0, lc.VIS_MIN_VISIBLE, lc.VIS_VAL_KEEP, lc.VIS_VAL_KEEP + 1, 0)
    assert tuple(e["keep"]) == lc.VIS_KEEP == (0, 1, 1, 0, 0)
    assert e["view_off"][0] == e["view_off"][1] == 0                           # an empty FIRST view
    assert (c["depth"][0] == 0).all() and (c["coords"][:, 2] != 0).sum() == 698
    last = lc.VIS_N - 1                                                        # the last point of the last view is invisible
    assert not ((e["view"] == lc.VIS_V - 1) & (e["pt"] == last)).any()
    # without depth maps z > 0 decides: other counts, the keep flags recomputed (val_keep = 303 keeps what 300 drops)
    f = lc.vis_entries(False, 40, 303)
    assert tuple(np.diff(f["view_off"])) != tuple(n) and tuple(f["keep"]) == (1, 1, 1, 0, 1) and not lc.vis_entries(False)["keep"].any()


def test_visibility_edge_points_decide_as_stated():
    c, e = lc.vis_case(), lc.vis_entries()
    in2 = e["view"] == 2

    def seen(xyz):
        """-> (row, column) of the point in view 2 or None"""
        i = np.flatnonzero((c["coords"] == np.array(xyz)).all(1))
        assert len(i) == 1
        at = np.flatnonzero(in2 & (e["pt"] == i[0]))
        return (int(e["x"][at[0]]), int(e["y"][at[0]])) if len(at) else None

    at = lc._at
    assert seen(at("swap", 9.5, 70, 2.0)) == (70, 10) and seen(at("swap", 10.5, 71, 2.0)) == (71, 10)      # half-to-even at the cut
    assert seen(at("swap", 117.5, 72, 2.0)) is None and seen(at("swap", 116.5, 73, 2.0)) == (73, 116)
    assert seen(at("swap", 30, 9.5, 2.0)) == (10, 30) and seen(at("swap", 31, 85.5, 2.0)) is None
    assert seen(at("swap", 32, 84.5, 2.0)) == (84, 32)
    assert seen((0.25, 0.25, 0.0)) is None and seen((0.0, 0.0, 0.0)) is None                                # z = 0
    assert seen(at("swap", 64, 48, -8.0)) is None                                                           # z < 0, pixel inside
    assert c["depth"][2, 74, 40] == 0 and seen(at("swap", 40, 74, 2.0)) is None                             # depth pixel 0
    assert seen(at("swap", 41, 75, 1.0)) == (75, 41) and seen((0.0, 0.0, 3.0)) == (48, 64)                  # |d - z| == tau d
    assert seen(at("swap", 42, 75, 4.0)) is None and seen(at("swap", 43, 75, 0.5)) is None
