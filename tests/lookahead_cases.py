"""Cases for the one-pass look-ahead entries: the fusion with the scene-level fill inside (gp_seen_masks, gp_fuse_views_top3_fill) and the
voxel rows with their operands (gp_voxel_rows_operands); lattices for the kNN's read-once first ring.  Plain numpy, no device code.

The kernel tests (test_gpu_lookahead.py) compare the new entries with the chains of calls they replace, bit for bit; the references
here state what those chains compute, and test_lookahead_cases_host.py checks that every case holds the situations it is named for.

  masks    seen[p] = the point has a list (pv_start[p + 1] > pv_start[p]), unseen = 1 - seen
  fill     a point without a list takes the row of the seen point at the lexicographic minimum of (d^2 in fp64 from the fp32 xyz,
           point index); -1 when no point is seen
  rows     X[row_map[v]] = [mean of F over the voxel | mean of geo | zeros up to cin_pad]: fp32 sums in ascending CSR order, one
           division; the row's power of two from max |X[row]| over all cin_pad columns, the global one from max |X[:, :d]|
"""
import numpy as np

import lift_cases as lc

f32, f64 = np.float32, np.float64

FUSE_D = (64, 512, 768)
FUSE_KINDS = ("mixed", "none_seen", "single", "single_unseen")
VOXEL_SHAPES = ((1, 512), (5, 512), (1027, 512), (5, 64), (1027, 64))          # (nv, d)
VOXEL_STRIDE_SHAPE = (16391, 64)              # more voxels than the kernel's 16384 waves: some waves walk two voxels (kernel test only)
GEO_DIM, CONV_PAD = 6, 32
SPECIAL = ("m65", "neg1", "neg2", "neg3", "plain3")                               # hand-built points of the "mixed" case, in this order


def cin_pad_of(d):
    return (d + GEO_DIM + CONV_PAD - 1) // CONV_PAD * CONV_PAD


# ------------------------------------------------------------------------------------------ references
def ref_seen(start):
    return (np.diff(start) > 0).astype(np.uint8)


def ref_nn(xyz, seen):
    """nn i64 [n]: for a point without a list the nearest seen point ((d^2 fp64, index) minimum), -1 for seen points and when none is seen"""
    n = len(xyz)
    nn = np.full(n, -1, np.int64)
    ref = np.nonzero(seen)[0]
    if len(ref) == 0:
        return nn
    p = xyz.astype(f64)
    for q in np.nonzero(seen == 0)[0]:
        dx, dy, dz = (p[q, k] - p[ref, k] for k in range(3))
        nn[q] = ref[((dx * dx + dy * dy) + dz * dz).argmin()]                   # first minimum = lowest index
    return nn


def ref_pow2_for(amax):
    """gp_pow2_for: the power of two s with amax * s in [2^13, 2^14); 1 for 0"""
    amax = f32(amax)
    if not (amax > 0 and amax < f32(3.0e38)):
        return f32(1)
    _, e = np.frexp(amax)
    return f32(np.ldexp(1.0, int(np.clip(14 - e, -100, 100))))


def ref_voxel_rows(case):
    """-> X f32 [nv, cin_pad] (rows through row_map), row_inv f32 [nv], scale2 f32 [2]"""
    d, nv, cp = case["d"], case["nv"], case["cin_pad"]
    X = np.zeros((nv, cp), f32)
    for v in range(nv):
        b, e = int(case["seg_start"][v]), int(case["seg_start"][v + 1])
        acc = np.zeros(d + GEO_DIM, f32)
        for j in range(b, e):                                                    # ascending CSR order, fp32 adds
            r = int(case["order"][j])
            acc = acc + np.concatenate([case["F"][r], case["geo"][r]])
        X[case["row_map"][v], :d + GEO_DIM] = acc / f32(max(e - b, 1))
    row_inv = np.array([f32(1) / ref_pow2_for(np.abs(X[r]).max()) for r in range(nv)], f32)
    s = ref_pow2_for(np.abs(X[:, :d]).max())
    return X, row_inv, np.array([s, f32(1) / s], f32)


# ------------------------------------------------------------------------------------------ the fusion with the fill inside
def case_fuse_fill(kind, d, seed=11, V=70, Q=6, C=19):
    """-> dict(start, pv_view, pv_seg, fseg, lseg, xyz, n, names).  "mixed": the SPECIAL points (a point seen by 65 views; three-entry
    points with segment -1 in one, two and all three of their slots -- with M = 3 every slot is a top slot; a plain one), each with an
    unseen twin a quarter unit away that the fill must give its row, among generic points of 0..5 entries; "none_seen": no point has a
    list; "single" / "single_unseen": n = 1 with and without a list."""
    rng = np.random.default_rng(seed + 1000 * FUSE_KINDS.index(kind) + d)
    lseg = (rng.integers(-128, 129, (V, Q, C)) / 8.0).astype(f32)
    f = rng.normal(size=(V, Q, d))
    fseg = (f / np.linalg.norm(f, axis=2, keepdims=True)).astype(f32)
    pts, names, xyz = [], [], []

    def add(name, vs, sg, pos):
        names.append(name), pts.append((np.asarray(vs, np.int64), np.asarray(sg, np.int64))), xyz.append(pos)

    if kind == "mixed":
        hand = {"m65": (np.arange(65), rng.integers(0, 4, 65)), "neg1": ([3, 20, 41], [-1, 2, 1]), "neg2": ([5, 6, 69], [-1, -1, 3]),
                "neg3": ([0, 33, 68], [-1, -1, -1]), "plain3": ([1, 2, 3], [0, 5, 4])}
        for k, name in enumerate(SPECIAL):
            add(name, *hand[name], (100.0 + 4 * k, 0.0, 0.0))
            add(name + ".twin", [], [], (100.0 + 4 * k, 0.25, 0.0))
        cloud = lc.lattice_points(rng, 290)
        for i in range(len(cloud)):
            M = 0 if rng.random() < 0.35 else int(rng.integers(1, 6))
            vs = np.sort(rng.choice(V, M, replace=False))
            sg = rng.integers(0, Q, M)
            if M >= 2 and rng.random() < 0.2:
                sg[int(rng.integers(M))] = -1
            add(f"g{i}", vs, sg, tuple(cloud[i]))
        order = rng.permutation(len(pts))                                        # point ids shuffled against the construction order
        pts, names, xyz = [pts[i] for i in order], [names[i] for i in order], [xyz[i] for i in order]
    elif kind == "none_seen":
        cloud = lc.lattice_points(rng, 40)
        for i in range(40):
            add(f"g{i}", [], [], tuple(cloud[i]))
    elif kind == "single":
        add("only", [4, 9], [1, 0], (1.0, 2.0, 3.0))
    elif kind == "single_unseen":
        add("only", [], [], (1.0, 2.0, 3.0))
    else:
        raise ValueError(kind)
    start = np.concatenate([[0], np.cumsum([len(p[0]) for p in pts])]).astype(np.int64)
    cat = lambda k: np.concatenate([p[k] for p in pts]).astype(np.int32) if start[-1] else np.zeros(0, np.int32)   # noqa: E731
    return dict(kind=kind, d=d, C=C, Q=Q, V=V, n=len(pts), names=names, start=start, pv_view=cat(0), pv_seg=cat(1), fseg=fseg, lseg=lseg,
                xyz=np.asarray(xyz, f32))


# ------------------------------------------------------------------------------------------ the voxel rows
VOXEL_SIZES = (1, 2, 37)
ZERO_V, TINY_V, HUGE_V, GEO_V = 0, 1, 2, 3          # voxels of an nv >= 5 case: all-zero row, 1e-30 row, 1e30 row with the global maximum, geometry above it


def case_voxel_rows(nv, d, seed=21):
    """-> dict(F f32 [N, d], geo f32 [N, 6], order i64 [N], seg_start i64 [nv + 1], row_map i32 [nv] (a permutation), nv, d, cin_pad).
    Voxel v holds VOXEL_SIZES[v % 3] points (nv = 1: two), whose ids are spread over the cloud and ascend inside the voxel.  With
    nv >= 5: voxel 0 is an all-zero row, voxel 1 has magnitude 1e-30, voxel 2 (37 points) magnitude 1e30 and the largest |mean| of all
    feature columns in column d - 1, voxel 3 geometry values above that maximum (they move its row's scale, not the global one)."""
    rng = np.random.default_rng(seed + 7 * nv + d)
    sizes = np.array([2] if nv == 1 else [VOXEL_SIZES[v % 3] for v in range(nv)])
    N = int(sizes.sum())
    vox_of = np.repeat(np.arange(nv), sizes)[rng.permutation(N)]                 # point -> voxel
    order = np.argsort(vox_of, kind="stable").astype(np.int64)
    seg_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    F = rng.normal(size=(N, d)).astype(f32)
    geo = rng.uniform(-1, 1, (N, GEO_DIM)).astype(f32)
    if nv >= 5:
        pts = lambda v: order[seg_start[v]:seg_start[v + 1]]                      # noqa: E731
        F[pts(ZERO_V)], geo[pts(ZERO_V)] = 0, 0
        F[pts(TINY_V)] *= f32(1e-30)
        geo[pts(TINY_V)] *= f32(1e-30)
        F[pts(HUGE_V)] *= f32(1e29)
        geo[pts(HUGE_V)] *= f32(1e29)
        F[pts(HUGE_V), d - 1] = f32(3e30)
        geo[pts(GEO_V)] = f32(8e30)
    return dict(F=F, geo=geo, order=order, seg_start=seg_start, row_map=rng.permutation(nv).astype(np.int32), nv=nv, d=d, N=N,
                cin_pad=cin_pad_of(d))


# ------------------------------------------------------------------------------------------ the kNN's read-once first ring
KNN_KEEP_CANDIDATES = 64 * 32                    # what a wave keeps in registers (csrc/knn.hip: KNN_KEEP per lane)
KNN_CASES = {"above_max": (96, 5), "at_max": (96, 5), "ties257": (20,)}          # case -> the K it runs with
TIES257_CENTRE = np.array([7, -30, 12])


def case_knn(name):
    """-> v int32 [nv, 3] in a shuffled row order.  "above_max": a full 16^3 lattice -- eight full 8^3 cells, 4096 candidates in every
    query's first ring, twice what a wave keeps: the two-pass code inside gp_knn_lattice; "at_max": four full cells (16 x 16 x 8), every
    first ring holds exactly KNN_KEEP_CANDIDATES; "ties257": a centre, ten inner voxels and 257 of the 312 lattice points at d^2 = 314:
    the first ring finds eleven candidates, the third 257 ties -- one more than it keeps -- and the exhaustive kernel answers."""
    from knn_batched_cases import INNER10, cube, shell
    if name == "above_max":
        v = cube(16, (-8, -16, 0))
    elif name == "at_max":
        v = cube(16, (-8, -16, 0))
        v = v[v[:, 2] < 8]
    elif name == "ties257":
        sh = shell(314)
        sh = sh[np.random.default_rng(31).permutation(len(sh))[:257]]
        v = np.vstack([np.zeros((1, 3), int), INNER10, sh]) + TIES257_CENTRE
    else:
        raise ValueError(name)
    assert len(np.unique(v, axis=0)) == len(v)
    return np.ascontiguousarray(v[np.random.default_rng(32).permutation(len(v))].astype(np.int32))


def first_ring_candidates(v):
    """per voxel: the voxels in the 27 cells (8^3, counted from the minimum) around its own"""
    cell = (v.astype(np.int64) - v.astype(np.int64).min(0)) >> 3
    return (np.abs(cell[:, None, :] - cell[None, :, :]).max(-1) <= 1).sum(1)
