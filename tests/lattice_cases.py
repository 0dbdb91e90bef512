"""Shared inputs and numpy models for the single-scene lattice kernels (gp_minmax_i32, gp_morton_order, gp_grid_build,
gp_kernel_map_build, gp_knn_lattice, gp_rcb_order / gp_rows_renumber_i32: csrc/order_grid.hip, gp_grid.h, knn.hip, rcb.hip) and for
the visibility lists (gp_views_visible_lists, gp_project_points_f64 + gp_visible_lists: csrc/voxelize.hip, misc.hip).

Part A.  A case is (v int32 [nv,3] in a shuffled row order, K), every array from a fixed seed.  The REFERENCES are
    morton_perm(v)    rows by the 21-bit-per-axis interleave (x lowest) of v - min
    kernel_map(cs)    oracle.student.build_kernel_map
    lists(v, K)       oracle.affinity.knn_lattice on the input rows: the K+1 smallest by (d^2, row), self dropped
    rcb_reference     gp_rcb_order restated
and are compared for exact equality, no row excused.  ladder(v, K, origin) models WHICH of gp_knn_lattice's three kernels answers a
query; it only proves on the host that a case reaches its path.

Part B.  One scene of 700 points under 5 exact-arithmetic views; vis_entries restates the mapper's rule, the host test holds it against
oracle.project._project / _finish.
"""
import functools

import numpy as np

from knn_batched_cases import (EXHAUSTIVE, INNER5, INNER10, KNN_MAXTIE, RING1, RING3, cube, shell, sparse_clusters,  # noqa: F401
                               surface_exact)
from oracle import affinity as o_aff
from oracle import student as o_student

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


# ------------------------------------------------------------------------------------------ the cases
def _shuffled(v, seed):
    v = np.asarray(v, np.int64)
    assert len(np.unique(v, axis=0)) == len(v), "the cases hold unique voxels"
    assert v.min() >= INT32_MIN and v.max() <= INT32_MAX
    return np.ascontiguousarray(v[np.random.default_rng(seed).permutation(len(v))].astype(np.int32))


TIES120_CENTRE = np.array([-3, 11, 200])
TIES312_CENTRE = np.array([-40, 5, 17])
SPAN1031_CORNERS = ((0, 0, 0), (1020, 0, 0), (0, 1020, 3), (5, 2, 1020), (1020, 1020, 1020))


def _negative_cube():
    """no coordinate positive (y reaches 0), the minimum (-37, -8, -64) no multiple of 8 on x: the face voxels' rel - 1 = -1 neighbours do not exist"""
    return _shuffled(cube(9, (-37, -8, -64)), 301), 20


def _dense_cells(K):
    """x -8..7, y -16..-1, z 0..7: four full 8^3 cells (bitmaps of all ones), 27 x 512-candidate blocks on ring 1"""
    def make():
        gx, gy, gz = np.arange(-8, 8), np.arange(-16, 0), np.arange(0, 8)
        return _shuffled(np.stack(np.meshgrid(gx, gy, gz, indexing="ij"), -1).reshape(-1, 3), 302), K
    return make


def _ties120():
    """centre, 5 inner voxels and the 120 lattice points at d^2 = 74: the centre's 17th neighbour is one of 120 ties, inside ring 1's
    bound of 81 and the KNN_MAXTIE ties kept.  Seed 303: the 11 ties with the lowest INPUT rows are not the 11 with the lowest Morton
    rows (test_lattice_cases_host.py checks it)."""
    return _shuffled(np.vstack([np.zeros((1, 3), int), INNER5, shell(74)]) + TIES120_CENTRE, 303), 16


def _ties312():
    """centre, 10 inner voxels and the 312 points at d^2 = 314 (> KNN_MAXTIE, radius below 24): ring 1 finds 11 candidates, ring 3 more
    ties than it keeps, the exhaustive kernel answers the centre.  Seed 304: input-row and Morton-row tie-breaks keep different sets."""
    return _shuffled(np.vstack([np.zeros((1, 3), int), INNER10, shell(314)]) + TIES312_CENTRE, 304), 20


def _clusters():
    return _shuffled(sparse_clusters(), 305), 20


def _nv_k_plus_1():
    """21 voxels, K = 20: every list is the whole set but the query"""
    return _shuffled(surface_exact(np.random.default_rng(306), 21, ext=12), 306), 20


def _surface_257_k96():
    """one voxel more than a 256-thread block; shifted so that x and z go negative"""
    return _shuffled(surface_exact(np.random.default_rng(307), 257, ext=12) - np.array([5, 0, 9]), 307), 96


def _span1031():
    """7^3 cubes that straddle coordinate 1024 on every axis: face neighbours and kNN lists cross the boundary between the low and the
    mid 10-bit groups of gp_morton3; extents 1027 -> 129^3 cells, a cell index of 8.6 MB"""
    return _shuffled(np.vstack([cube(7, o) for o in SPAN1031_CORNERS]), 308), 20


def _span32768(reverse):
    """5^3 cubes at 0, 16381 and 32763 along one axis: extent exactly 32768, the largest gp_grid_build takes; the middle cube
    straddles 16384 (Morton bit 14 of that axis)"""
    def make():
        v = np.vstack([cube(5, (o, 0, 0)) for o in (0, 16381, 32763)])
        return _shuffled(v[:, ::-1] if reverse else v, 309), 20
    return make


CASES = {
    "negative_cube": _negative_cube,
    "dense_cells_k127": _dense_cells(127),
    "dense_cells_k1": _dense_cells(1),
    "ties120": _ties120,
    "ties312": _ties312,
    "clusters": _clusters,
    "nv_k_plus_1": _nv_k_plus_1,
    "surface_257_k96": _surface_257_k96,
    "span1031": _span1031,
    "span32768_x": _span32768(False),
    "span32768_z": _span32768(True),
}
SPAN_CASES = {"span1031": 1024, "span32768_x": 16384, "span32768_z": 16384}      # case -> the coordinate (above the minimum) its cubes straddle
IDS_NONE_CASES = ("ties120", "ties312", "dense_cells_k1")
EXPLICIT_BOX_CASES = ("negative_cube", "ties312", "span32768_x")


@functools.lru_cache(maxsize=None)
def case(name):
    v, K = CASES[name]()
    v.setflags(write=False)
    return v, K


def row_of(v, xyz):
    hit = np.flatnonzero((v == np.asarray(xyz)).all(1))
    assert len(hit) == 1
    return int(hit[0])


# ------------------------------------------------------------------------------------------ references
def morton_key(v, bits=21):
    q = (v.astype(np.int64) - v.astype(np.int64).min(0)).astype(np.uint64)
    key = np.zeros(len(v), np.uint64)
    for b in range(bits):
        for ax in range(3):
            key |= ((q[:, ax] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + ax)
    return key


def morton_perm(v, bits=21):
    """gp_morton_order restated: rows by the bit interleave (x lowest) of v - min, 21 bits per axis; the codes of distinct voxels are
    distinct.  (bits=10: what a key built from the low 10-bit group alone would give -- the span cases must tell the two apart.)"""
    return np.argsort(morton_key(v, bits), kind="stable")


def kernel_map(cs):
    return o_student.build_kernel_map(cs)


def lists(v, K):
    """int64 [nv,K] of rows of v"""
    return o_aff.knn_lattice(np.array(v), K).numpy()


@functools.lru_cache(maxsize=None)
def geometry(name):
    """the case in Morton order with every reference: v, K, perm, cs = v[perm], nm = kernel_map(cs), ref = lists(v, K) (input rows),
    ref_sorted = lists(cs, K) (Morton rows, what ids = NULL must give; only for IDS_NONE_CASES)"""
    v, K = case(name)
    perm = morton_perm(v)
    cs = np.ascontiguousarray(v[perm])
    g = dict(v=v, K=K, perm=perm, cs=cs, nm=kernel_map(cs), ref=lists(v, K))
    if name in IDS_NONE_CASES:
        g["ref_sorted"] = lists(cs, K)
    for a in g.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return g


def tight_box(v):
    lo = v.astype(np.int64).min(0)
    return lo, v.astype(np.int64).max(0) - lo + 1


def loose_box(v):
    """origin = min, extent = tight + (9, 17, 1) clipped to 32768: an extra layer of empty cells, no multiple of 8"""
    lo, ext = tight_box(v)
    return lo, np.minimum(ext + np.array([9, 17, 1]), 32768)


def ladder(v, K, origin=None, extent=None, ids=None):
    """Model of gp_knn_lattice's ladder -> (lists int64 [nv,K] of rows of v, path int [nv]: RING1, RING3 or EXHAUSTIVE).  It is
    knn_batched_cases.ladder_of for one entry with the grid's cells: cell = (xyz - origin) >> 3, a ring's candidate cells clipped to
    the grid's cell dimensions ((extent - 1) >> 3) + 1.  Ring R takes its candidates from the (2R+1)^3 cells around the query's; it
    resolves the query when the histogram of d^2 below B = (8R+1)^2 holds K+1 candidates and the threshold distance T -- the d^2 of
    the (K+1)-th -- has at most KNN_MAXTIE candidates; its list is then the K+1 smallest (d^2, id) among the candidates with
    d^2 <= T, self dropped.  What neither ring resolves is answered from all rows.  ids: the tie-break number of every row (default:
    the row itself)."""
    p = v.astype(np.int64)
    n = len(p)
    lo, ext = tight_box(v)
    origin = lo if origin is None else np.asarray(origin, np.int64)
    extent = ext if extent is None else np.asarray(extent, np.int64)
    cell = (p - origin) >> 3
    cdim = ((extent - 1) >> 3) + 1
    assert (cell >= 0).all() and (cell < cdim).all(), "every voxel lies inside the box: clipping the candidate cells drops no voxel"
    ids = np.arange(n) if ids is None else np.asarray(ids, np.int64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    cheb = np.abs(cell[:, None, :] - cell[None, :, :]).max(-1)
    out = np.full((n, K), -1, np.int64)
    path = np.full(n, -1, np.int64)
    big = np.int64(1) << 40
    todo = np.ones(n, bool)

    def take(rows, eligible):
        key = np.where(eligible, d2[rows] * n + ids[None, :], big * n)
        part = np.argpartition(key, K, axis=1)[:, :K + 1]
        order = np.take_along_axis(part, np.argsort(np.take_along_axis(key, part, 1), axis=1), 1)
        return order[:, 1:]

    for R, tag in ((1, RING1), (3, RING3)):
        rows = np.flatnonzero(todo)
        if not len(rows):
            break
        B = (8 * R + 1) ** 2
        cand = cheb[rows] <= R
        hist = np.where(cand & (d2[rows] < B), d2[rows], big)
        enough = (hist < big).sum(1) >= K + 1
        T = np.partition(hist, K, axis=1)[:, K]
        ok = enough & ((hist == T[:, None]).sum(1) <= KNN_MAXTIE)
        got = take(rows, cand & (d2[rows] <= T[:, None]))
        out[rows[ok]] = got[ok]
        path[rows[ok]] = tag
        todo[rows[ok]] = False
    rows = np.flatnonzero(todo)
    if len(rows):
        out[rows] = take(rows, np.ones((len(rows), n), bool))
        path[rows] = EXHAUSTIVE
    return out, path


def kept_ties(v, K, centre_row, ids):
    """the rows of v that a (d^2, ids) selection keeps among the candidates at the centre's threshold distance"""
    p = v.astype(np.int64)
    d2 = ((p - p[centre_row]) ** 2).sum(1)
    order = np.lexsort((ids, d2))[:K + 1]
    T = d2[order[-1]]
    return set(order[d2[order] == T].tolist()), int((d2 == T).sum())


# ------------------------------------------------------------------------------------------ gp_rcb_order
def rcb_reference(cs, chunk, leaf):
    """gp_rcb_order restated (csrc/rcb.hip): inside every chunk, a segment longer than a leaf is sorted along the axis of its largest
    extent (ties: the lower axis; equal coordinates keep their order) and cut at ceil(len / 2 / leaf) * leaf rows."""
    nv = len(cs)
    sigma = np.empty(nv, np.int64)
    for base in range(0, nv, chunk):
        n = min(chunk, nv - base)
        order, segs, more = np.arange(n), [(0, n)], n > leaf
        while more:
            new, more = [], False
            for start, ln in segs:
                if ln <= leaf:
                    new.append((start, ln))
                    continue
                idx = order[start:start + ln]
                p = cs[base + idx].astype(np.int64)
                ax = int(np.argmax(p.max(0) - p.min(0)))
                order[start:start + ln] = idx[np.argsort(p[:, ax], kind="stable")]
                half = (ln // 2 + leaf - 1) // leaf * leaf
                half = ln // 2 if half >= ln else half
                new += [(start, half), (start + half, ln - half)]
                more |= half > leaf or ln - half > leaf
            segs = new
        sigma[base:base + n] = base + order
    return sigma


def _plane():
    """48 x 48 x 1: x and y extents tie in the first segments (the lower axis wins), thousands of equal coordinates along the cut axis"""
    g = np.arange(48)
    return np.stack(np.meshgrid(g, g, [7], indexing="ij"), -1).reshape(-1, 3)


def _column():
    """40 x 1 x 60: the largest extent on z"""
    return np.stack(np.meshgrid(np.arange(40), [3], np.arange(60), indexing="ij"), -1).reshape(-1, 3)


def _wide_chunk():
    """the span32768_x voxels and 925 surface voxels beside the first cube: 1300 rows, x - min up to 32767 inside one chunk -- the
    key's 15-bit coordinate field used to its end"""
    v = np.vstack([case("span32768_x")[0], surface_exact(np.random.default_rng(310), 925, ext=30) + np.array([64, 0, 0])])
    assert len(np.unique(v, axis=0)) == 1300
    return v


RCB_INPUTS = {"plane": _plane, "column": _column, "wide_chunk": _wide_chunk}
RCB_SHAPES = ((1024, 128), (1024, 64), (2048, 128), (2048, 256), (2048, 64))
RCB_K = 20


@functools.lru_cache(maxsize=None)
def rcb_input(name):
    """-> (cs int32 [nv,3] in Morton order, nbr int64 [nv, RCB_K] = lists(cs, RCB_K))"""
    v = np.asarray(RCB_INPUTS[name]())
    cs = np.ascontiguousarray(v[morton_perm(v)].astype(np.int32))
    nbr = lists(cs, RCB_K)
    cs.setflags(write=False), nbr.setflags(write=False)
    return cs, nbr


@functools.lru_cache(maxsize=None)
def rcb_sigma(name, chunk, leaf):
    s = rcb_reference(rcb_input(name)[0], chunk, leaf)
    s.setflags(write=False)
    return s


def rcb_leaves(n, leaf):
    """the leaf lengths of a chunk of n rows, in order (the cutting rule alone)"""
    segs = [n]
    while any(s > leaf for s in segs):
        new = []
        for ln in segs:
            if ln <= leaf:
                new.append(ln)
                continue
            half = (ln // 2 + leaf - 1) // leaf * leaf
            half = ln // 2 if half >= ln else half
            new += [half, ln - half]
        segs = new
    return segs


# ------------------------------------------------------------------------------------------ Part B: visibility lists
VIS_W, VIS_H, VIS_CUT, VIS_TAU = 128, 96, 10, 0.5
VIS_F, VIS_CX, VIS_CY = 256.0, 64.0, 48.0
VIS_MIN_VISIBLE, VIS_VAL_KEEP = 40, 300
VIS_N, VIS_V = 700, 5
VIS_COUNTS = (0, 40, 300, 301, 0)                              # visible points per view, with the depth maps
VIS_KEEP = (0, 1, 1, 0, 0)                                     # empty | == min_visible | == val_keep | val_keep + 1 | empty

_IDENT = np.eye(4)
_SWAP = np.array([[0., 1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])          # camera x = world y, camera y = world x
_BACK = np.diag([-1., 1, -1, 1])                                                   # half a turn about y: sees what lies at world z < 0


def _at(view, u, v, z):
    """the world point that the view's camera sees at pixel position (u = column, v = row) and camera depth z; z a power of two (or
    u - cx = v - cy = 0) makes every product and quotient of the mapper exact"""
    xc, yc = (u - VIS_CX) * z / VIS_F, (v - VIS_CY) * z / VIS_F
    return {"ident": (xc, yc, z), "swap": (yc, xc, z), "back": (-xc, yc, -z)}[view]


@functools.lru_cache(maxsize=None)
def vis_case():
    """-> dict(coords f64 [700,3] shuffled, params f64 [5,20], depth f64 [5,H,W]).

    view 0  identity, depth all zero            -> sees nothing (|0 - z| <= 0 fails for every z != 0; z = 0 has no finite pixel)
    view 1  identity, depth 2 on one pixel row  -> exactly the 40 points of group A (min_visible)
    view 2  x / y swapped, depth 2 but a pixel  -> groups A, B and 7 of the edge points: 300 (val_keep)
    view 3  half a turn about y, depth 2        -> the 301 points of group C, which lie behind the other cameras (val_keep + 1)
    view 4  x / y swapped, depth 64             -> sees nothing (no point within tau * 64 of 64), the last point invisible"""
    A = [_at("ident", 30 + i, 20, 2.0) for i in range(40)]                                   # view 2: column 36, rows 14..53
    B = [_at("ident", 26 + i % 76, 30 + i // 76, 2.0) for i in range(253)]                   # view 2: columns 46..49, rows 10..85
    C = [_at("back", 26 + i % 76, 40 + i // 76, 2.0) for i in range(301)]
    E = [_at("swap", VIS_CUT - 0.5, 70, 2.0),                # u = 9.5: half-to-even -> 10 = cut, visible
         _at("swap", VIS_CUT + 0.5, 71, 2.0),                # u = 10.5 -> 10, visible (half-up would say column 11)
         _at("swap", VIS_W - VIS_CUT - 0.5, 72, 2.0),        # u = 117.5 -> 118 = W - cut, outside
         _at("swap", VIS_W - VIS_CUT - 1.5, 73, 2.0),        # u = 116.5 -> 116, visible
         _at("swap", 30, VIS_CUT - 0.5, 2.0),                # v = 9.5 -> 10, visible
         _at("swap", 31, VIS_H - VIS_CUT - 0.5, 2.0),        # v = 85.5 -> 86 = H - cut, outside
         _at("swap", 32, VIS_H - VIS_CUT - 1.5, 2.0),        # v = 84.5 -> 84, visible
         (0.25, 0.25, 0.0), (0.0, 0.0, 0.0),                 # z = 0: u = inf, u = nan
         _at("swap", 64, 48, -8.0),                          # behind the camera, its pixel inside the image, a depth map given
         _at("swap", 40, 74, 2.0),                           # the depth pixel that holds 0
         _at("swap", 41, 75, 1.0),                           # |d - z| == tau d exactly (d = 2, z = 1): visible
         (0.0, 0.0, 3.0),                                    # |2 - 3| == tau d from the other side: visible, at (cx, cy)
         _at("swap", 42, 75, 4.0), _at("swap", 43, 75, 0.5)]  # |d - z| = 2 and 1.5 > 1: invisible
    rng = np.random.default_rng(311)
    fill = [_at("swap", float(rng.integers(10, 118)), float(rng.integers(10, 86)), -16.0) for _ in range(VIS_N - 609)]
    coords = np.array(A + B + C + E + fill, np.float64)
    assert coords.shape == (VIS_N, 3)
    coords = np.ascontiguousarray(coords[rng.permutation(VIS_N)])
    intr = [VIS_F, VIS_F, VIS_CX, VIS_CY]
    params = np.stack([np.r_[m.reshape(16), intr] for m in (_IDENT, _IDENT, _SWAP, _BACK, _SWAP)])
    depth = np.zeros((VIS_V, VIS_H, VIS_W))
    depth[1, 20, 30:70] = 2.0
    depth[2] = 2.0
    depth[2, 74, 40] = 0.0
    depth[3] = 2.0
    depth[4] = 64.0
    for a in (coords, params, depth):
        a.setflags(write=False)
    return dict(coords=coords, params=params, depth=depth)


def vis_entries(with_depth=True, min_visible=VIS_MIN_VISIBLE, val_keep=VIS_VAL_KEEP):
    """The mapper's rule restated for every view -> dict(pt, x, y int64 [total], view int32 [total], view_off int64 [V+1], keep uint8
    [V]): a point is an entry of a view when its rounded (half-to-even) pixel is finite and inside the cut bound and either
    |depth[pixel] - z| <= tau depth[pixel] (depth maps given) or z > 0 (none); x = pixel ROW, y = pixel COLUMN; entries view-major,
    ascending point inside a view; keep = the view has entries, at least min_visible and at most val_keep of them."""
    c = vis_case()
    X = np.c_[c["coords"], np.ones(VIS_N)]
    ent = dict(pt=[], x=[], y=[], view=[])
    off = [0]
    for v in range(VIS_V):
        M, (fx, fy, cx, cy) = c["params"][v, :16].reshape(4, 4), c["params"][v, 16:]
        p = X @ M.T
        with np.errstate(all="ignore"):
            u, w = np.rint(p[:, 0] * fx / p[:, 2] + cx), np.rint(p[:, 1] * fy / p[:, 2] + cy)
        ok = np.isfinite(u) & np.isfinite(w)
        ui, wi = np.where(ok, u, -1).astype(np.int64), np.where(ok, w, -1).astype(np.int64)
        ok &= (ui >= VIS_CUT) & (wi >= VIS_CUT) & (ui < VIS_W - VIS_CUT) & (wi < VIS_H - VIS_CUT)
        if with_depth:
            d = c["depth"][v][np.where(ok, wi, 0), np.where(ok, ui, 0)]
            ok &= np.abs(d - p[:, 2]) <= VIS_TAU * d
        else:
            ok &= p[:, 2] > 0
        idx = np.flatnonzero(ok)
        ent["pt"].append(idx), ent["x"].append(wi[idx]), ent["y"].append(ui[idx]), ent["view"].append(np.full(len(idx), v))
        off.append(off[-1] + len(idx))
    out = {k: np.concatenate(a).astype(np.int32 if k == "view" else np.int64) for k, a in ent.items()}
    out["view_off"] = np.array(off, np.int64)
    nv = np.diff(out["view_off"])
    out["keep"] = ((nv != 0) & (nv >= min_visible) & (nv <= val_keep)).astype(np.uint8)
    return out
