"""The single-scene lattice kernels (csrc/order_grid.hip, gp_grid.h, knn.hip, rcb.hip) at their sign, span, cell and tie edges, and the
visibility lists (csrc/voxelize.hip, misc.hip) at the boundaries of the keep rule, against the references of tests/lattice_cases.py.

Part A runs every case of lattice_cases.CASES through gp_minmax_i32, gp_morton_order, gp_grid_build + gp_kernel_map_build and
gp_knn_lattice (ids = the input rows; ids = NULL; a tight and an explicit, looser box) and the rcb inputs through both templates of
gp_rcb_order and gp_rows_renumber_i32.  Part B runs one scene of 700 points and 5 exact-arithmetic views through
gp_views_visible_lists and through gp_project_points_f64 + gp_visible_lists view by view.  Every comparison is np.array_equal /
torch.equal on all rows: the outputs are integers.  test_lattice_cases_host.py proves on the host that each case reaches the branch
it is named for.  A grid that gp_grid_build flags is never handed on; refusals are read from the exception alone.
"""
import numpy as np
import pytest
import torch

import lattice_cases as lc

pytestmark = pytest.mark.gpu

I32, I64 = torch.int32, torch.int64


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import ops as _ops
    from geopurify_amd import _lib
    _lib.load()                      # fails loudly if the HIP library is missing
    return _ops


def up(a, dtype=None):
    t = torch.from_numpy(np.array(a)) if not torch.is_tensor(a) else a            # a copy: the cases' arrays are read-only
    return (t.to(dtype) if dtype is not None else t).cuda().contiguous()


def host(t):
    return t.cpu().numpy().astype(np.int64)


_DEV = {}


def device_case(ops, name):
    """the case on the device, once: cs, perm (the references' -- the kernels under test get no output of another kernel under test),
    and the grid over the tight box that grid_build computes itself"""
    if name not in _DEV:
        g = lc.geometry(name)
        cs = up(g["cs"])
        grid = ops.grid_build(cs)
        assert grid.status() == 0
        lo, ext = lc.tight_box(g["v"])
        assert grid.origin == lo.tolist() and grid.extent == ext.tolist()
        _DEV[name] = dict(cs=cs, perm=up(g["perm"], I32), grid=grid)
    return _DEV[name]


def to_input_rows(nbr_sorted, perm):
    """lists of Morton rows, by Morton row -> lists of input rows, by input row (as test_knn_exact_with_ties)"""
    out = np.empty_like(nbr_sorted)
    out[perm] = perm[nbr_sorted]
    return out


# ------------------------------------------------------------------------------------------ gp_minmax_i32
def minmax_sets():
    rng = np.random.default_rng(401)
    sets = {name: (lambda n=name: lc.case(n)[0]) for name in lc.CASES}
    sets["one_row"] = lambda: np.array([[-7, 0, 19]], np.int32)
    # minmax_kernel: at most 64 blocks of 256 threads, 16384 rows per stride; the extremes sit in the last row and in the first
    far = rng.integers(-1000, 1000, (16385, 3)).astype(np.int32)
    far[-1] = (-5000, 6000, -7000)
    far[0] = (5000, -6000, 7000)
    sets["one_past_the_grid_stride"] = lambda: far
    wide = rng.integers(-9, 9, (300, 3)).astype(np.int32)
    wide[17] = (lc.INT32_MIN + 1, lc.INT32_MAX, 0)
    wide[299] = (lc.INT32_MAX, lc.INT32_MIN + 1, lc.INT32_MAX)
    sets["int32_ends"] = lambda: wide
    return sets


MINMAX = minmax_sets()


@pytest.mark.parametrize("name", list(MINMAX))
def test_minmax_i32(ops, name):
    v = np.ascontiguousarray(MINMAX[name]())
    mm = ops.minmax_i32(up(v)).cpu().numpy()
    assert mm.dtype == np.int32 and np.array_equal(mm, np.r_[v.min(0), v.max(0)])


# ------------------------------------------------------------------------------------------ gp_morton_order
@pytest.mark.parametrize("name", list(lc.CASES))
def test_morton_order(ops, name):
    g = lc.geometry(name)
    perm, rank = ops.morton_order(up(g["v"]))
    assert np.array_equal(host(perm), g["perm"])
    assert np.array_equal(host(rank)[g["perm"]], np.arange(len(g["v"])))


# ------------------------------------------------------------------------------------------ gp_grid_build + gp_kernel_map_build
def kernel_map_ok(nm, want):
    assert nm.dtype == np.int32 and nm.shape == want.shape
    assert np.array_equal(nm[13], np.arange(nm.shape[1]))
    assert np.array_equal(nm == -1, want == -1)              # a wrap at rel = -1 or rel = extent would find a row where there is none
    assert np.array_equal(nm, want)


@pytest.mark.parametrize("name", list(lc.CASES))
def test_grid_and_kernel_map(ops, name):
    d = device_case(ops, name)
    kernel_map_ok(ops.kernel_map_build(d["grid"], d["cs"]).cpu().numpy(), lc.geometry(name)["nm"])


# ------------------------------------------------------------------------------------------ gp_knn_lattice
@pytest.mark.parametrize("name", list(lc.CASES))
def test_knn_lattice_breaks_ties_by_input_row(ops, name):
    g, d = lc.geometry(name), device_case(ops, name)
    nbr = ops.knn_lattice(d["grid"], d["cs"], d["perm"], g["K"])
    assert nbr.dtype == I32 and tuple(nbr.shape) == (len(g["v"]), g["K"])
    assert np.array_equal(to_input_rows(host(nbr), g["perm"]), g["ref"])          # every row, order included


@pytest.mark.parametrize("name", lc.IDS_NONE_CASES)
def test_knn_lattice_without_ids_breaks_ties_by_its_own_row(ops, name):
    g, d = lc.geometry(name), device_case(ops, name)
    nbr = ops.knn_lattice(d["grid"], d["cs"], None, g["K"])
    assert np.array_equal(host(nbr), g["ref_sorted"])


@pytest.mark.parametrize("name", lc.EXPLICIT_BOX_CASES)
def test_explicit_looser_box_changes_nothing(ops, name):
    """pipeline.py hands grid_build an origin and an extent of its own: a box with an extra layer of empty cells, no multiple of 8,
    gives the same kernel map and the same lists, bit for bit, as the tight one -- and as the references"""
    g, d = lc.geometry(name), device_case(ops, name)
    origin, extent = lc.loose_box(g["v"])
    grid = ops.grid_build(d["cs"], origin=origin.tolist(), extent=extent.tolist())
    assert grid.status() == 0 and grid.extent == extent.tolist() and grid.extent != d["grid"].extent
    nm = ops.kernel_map_build(grid, d["cs"])
    assert torch.equal(nm, ops.kernel_map_build(d["grid"], d["cs"]))
    kernel_map_ok(nm.cpu().numpy(), g["nm"])
    nbr = ops.knn_lattice(grid, d["cs"], d["perm"], g["K"])
    assert torch.equal(nbr, ops.knn_lattice(d["grid"], d["cs"], d["perm"], g["K"]))
    assert np.array_equal(to_input_rows(host(nbr), g["perm"]), g["ref"])


# ------------------------------------------------------------------------------------------ status and refusals
def test_grid_status_flags_duplicates_and_voxels_outside_the_box(ops):
    """only the status is read: a flagged grid is never searched"""
    cs = lc.geometry("negative_cube")["cs"]
    dup = np.ascontiguousarray(np.insert(cs, 400, cs[400], axis=0))               # rows 400 and 401 equal: sorted, not strictly
    assert ops.grid_build(up(dup)).status() & 1
    box = lc.cube(4)
    box = box[lc.morton_perm(box)].astype(np.int32)
    assert ops.grid_build(up(box), origin=[0, 0, 0], extent=[4, 4, 4]).status() == 0
    for ax in range(3):
        out = np.zeros((1, 3), np.int32)
        out[0, ax] = 4                                                           # = origin + extent on one axis; its code 64 << ax follows all 64 others
        rows = np.ascontiguousarray(np.vstack([box, out]))
        assert np.array_equal(rows, rows[lc.morton_perm(rows)])                  # sorted: only the extent can be objected to
        assert ops.grid_build(up(rows), origin=[0, 0, 0], extent=[4, 4, 4]).status() & 1, ax


def test_refusals(ops):
    from geopurify_amd._lib import GeoPurifyHipError
    d = device_case(ops, "dense_cells_k127")
    with pytest.raises(GeoPurifyHipError, match="k=128"):
        ops.knn_lattice(d["grid"], d["cs"], d["perm"], 128)
    d = device_case(ops, "nv_k_plus_1")
    with pytest.raises(GeoPurifyHipError, match="more than k"):
        ops.knn_lattice(d["grid"], d["cs"][:20].contiguous(), d["perm"][:20].contiguous(), 20)      # nv = K
    for ax in range(3):
        two = np.zeros((2, 3), np.int32)
        two[1, ax] = 32768                                                       # extent 32769
        with pytest.raises(GeoPurifyHipError, match="32768"):
            ops.grid_build(up(two))


# ------------------------------------------------------------------------------------------ gp_rcb_order / gp_rows_renumber_i32
@pytest.mark.parametrize("chunk,leaf", lc.RCB_SHAPES)
@pytest.mark.parametrize("name", list(lc.RCB_INPUTS))
def test_rcb_order_and_rows_renumber(ops, name, chunk, leaf):
    cs, nbr = lc.rcb_input(name)
    nv = len(cs)
    sigma, rho = ops.rcb_order(up(cs), chunk, leaf)
    sg, rh = host(sigma), host(rho)
    assert np.array_equal(sg, lc.rcb_sigma(name, chunk, leaf))
    assert np.array_equal(rh[sg], np.arange(nv))
    out = ops.rows_renumber(up(nbr, I32), sigma, rho)
    assert np.array_equal(host(out), rh[nbr[sg]])


# ------------------------------------------------------------------------------------------ Part B: visibility lists
def entries_ok(ent, want):
    off = host(ent["view_off"])
    assert np.array_equal(off, want["view_off"])
    total = int(off[-1])
    for k in ("pt", "x", "y", "view"):
        assert np.array_equal(host(ent[k][:total]), want[k]), k
    assert np.array_equal(ent["keep"].cpu().numpy(), want["keep"])


def per_view_lists(ops, with_depth):
    """gp_project_points_f64 + gp_visible_lists, view by view -> the same dict as lattice_cases.vis_entries (no keep flags)"""
    c = lc.vis_case()
    coords = up(c["coords"])
    n = lc.VIS_N
    pt, x, y, view, off = [], [], [], [], [0]
    for v in range(lc.VIS_V):
        fx, fy, cx, cy = c["params"][v, 16:]
        m = ops.project_points(coords, c["params"][v, :16].reshape(4, 4), fx, fy, cx, cy, up(c["depth"][v]) if with_depth else None,
                               lc.VIS_W, lc.VIS_H, lc.VIS_CUT, lc.VIS_TAU)
        p_, x_, y_ = (torch.full((n,), -7, dtype=I64, device="cuda") for _ in range(3))
        cnt = torch.zeros(1, dtype=I64, device="cuda")
        ops.visible_lists(m, p_, x_, y_, cnt)
        k = int(cnt.item())
        assert bool((p_[k:] == -7).all())                    # nothing written behind the count
        pt.append(host(p_[:k])), x.append(host(x_[:k])), y.append(host(y_[:k])), view.append(np.full(k, v))
        off.append(off[-1] + k)
    return dict(pt=np.concatenate(pt), x=np.concatenate(x), y=np.concatenate(y), view=np.concatenate(view), view_off=np.array(off))


def test_views_visible_lists_against_the_mapper(ops):
    c, want = lc.vis_case(), lc.vis_entries()
    ent = ops.views_visible_lists(up(c["coords"]), up(c["params"]), up(c["depth"]), lc.VIS_W, lc.VIS_H, lc.VIS_CUT, lc.VIS_TAU,
                                  lc.VIS_MIN_VISIBLE, lc.VIS_VAL_KEEP)
    entries_ok(ent, want)
    n = np.diff(host(ent["view_off"]))
    assert tuple(n) == lc.VIS_COUNTS and tuple(ent["keep"].cpu().tolist()) == lc.VIS_KEEP
    assert ent["keep"].cpu().tolist() == [int(k != 0 and lc.VIS_MIN_VISIBLE <= k <= lc.VIS_VAL_KEEP) for k in n]
    one = per_view_lists(ops, True)
    for k, a in one.items():
        assert np.array_equal(a, want[k]), k


def test_views_visible_lists_without_depth_maps(ops):
    """z > 0 decides; other counts, the keep flags recomputed from them"""
    c = lc.vis_case()
    for min_visible, val_keep in ((lc.VIS_MIN_VISIBLE, lc.VIS_VAL_KEEP), (40, 303)):
        want = lc.vis_entries(False, min_visible, val_keep)
        ent = ops.views_visible_lists(up(c["coords"]), up(c["params"]), None, lc.VIS_W, lc.VIS_H, lc.VIS_CUT, lc.VIS_TAU, min_visible,
                                      val_keep)
        entries_ok(ent, want)
    one = per_view_lists(ops, False)
    for k, a in one.items():
        assert np.array_equal(a, want[k]), k
