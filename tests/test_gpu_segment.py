"""The batched scene tail on the GPU: gp_nn1_batched (ops.nn1_batched), gp_iou_hist_batched_i64 (ops.iou_hist_batched) and
geopurify_amd.sparse.segment.

References (tests/segment_cases.py): the brute-force fill in int64 with the (d^2, input row) rule per entry, fp64 arg-max labels on
features whose top-2 cosine margin is at least 0.1 (asserted there), oracle.metric.intersection_and_union per entry.  Everything is
compared for exact equality, no row excused.  test_segment_cases_host.py shows on the host which rung of the ladder each case takes.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import extent_fence
import knn_batched_cases as kc
import segment_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D0, C0 = 64, 20


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import _lib, ops, sparse
    _lib.load()
    assert hasattr(ops, "nn1_batched") and hasattr(ops, "iou_hist_batched") and hasattr(sparse, "segment")
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import MinkowskiEngine as ME
    finally:
        sys.path.pop(0)
    return ops, sparse, ME


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                # (a copy: the cases are read-only arrays)


def _fill(ops, C, zero, axes=7, ids=True):
    """ops.nn1_batched on the case -> (filled_from int64 numpy [N] of input rows in input order, status list, nn, perm)"""
    perm, rank, keys, st = ops.coords_order_batched(_dev(C))
    assert st.tolist() == [0, 0, 0]
    zs = _dev(zero.astype(np.uint8)).index_select(0, perm.long())
    nn, status = ops.nn1_batched(keys, perm if ids else None, 1 - zs, zs, axes)
    n = nn.long()
    ff = torch.where(n >= 0, perm.long()[n.clamp(min=0)], n).index_select(0, rank.long())
    return ff.cpu().numpy(), status.tolist(), nn, perm


def _segment(env, name, D=D0, Cn=C0, **kw):
    ops, sparse, ME = env
    C, zero = sc.case(name)
    F, cls = sc.features(name, D, Cn)
    y = ME.SparseTensor(features=_dev(F), coordinates=_dev(C))
    return sparse.segment(y, _dev(sc.text(D, Cn)).float(), 3.0, **kw), cls


# ------------------------------------------------------------------------------------------ the fill: every case, both entries into it
@pytest.mark.parametrize("name", list(sc.CASES))
def test_fill_equals_brute_force(env, name):
    """overlapping entries, the empty / full / one-voxel entries, every rung and both ties at an acceptance bound, equidistant
    references, the widest extent, 1 / 63 / 64 / 65 / 257 / all-but-one queries: ops.nn1_batched and sparse.segment, every row exact"""
    ops, sparse, ME = env
    C, zero = sc.case(name)
    ref = sc.fill(name)
    got, status, nn, perm = _fill(ops, C, zero)
    assert status == [int(zero.sum()), int((~zero).sum()), int((zero & (ref < 0)).sum()), 0]
    assert np.array_equal(got, ref)
    seg, cls = _segment(env, name)
    assert seg.pred.dtype == torch.int64 and seg.filled_from.dtype == torch.int64 and seg.zero.dtype == torch.bool
    assert np.array_equal(seg.zero.cpu().numpy(), zero)
    assert np.array_equal(seg.filled_from.cpu().numpy(), ref)
    assert np.array_equal(seg.pred.cpu().numpy(), sc.pred_of(cls, ref))
    assert seg.unfilled == int((zero & (ref < 0)).sum()) and seg.counts is None


def test_overlapping_entries_never_mix(env):
    ops, sparse, ME = env
    C, zero = sc.case("overlap")
    got = _fill(ops, C, zero)[0]
    assert (got[zero] >= 0).all() and (C[got[zero], 0] == C[zero, 0]).all()


def test_empty_entry_keeps_its_argmax(env):
    """entry 0 all zero: every query -1, unfilled = its size, labels the arg-max (class 0 of an all-zero row); entries 3 and 65535 beside
    it are untouched; counts have 65536 blocks, zero except for the three entries"""
    C, zero = sc.case("empty_entry")
    cls = sc.features("empty_entry", D0, C0)[1]
    target = sc.target_of(cls, C0, 11)
    seg, _ = _segment(env, "empty_entry", labels=_dev(target))
    assert seg.unfilled == 64 == int(zero.sum())
    assert (seg.filled_from.cpu().numpy() == -1).all()
    pred = seg.pred.cpu().numpy()
    assert (pred[zero] == 0).all() and np.array_equal(pred, cls)
    counts = seg.counts.cpu().numpy()
    assert counts.shape == (65536, 3, C0)
    present = np.zeros(65536, bool)
    present[[0, 3, 65535]] = True
    assert counts[~present].sum() == 0
    assert np.array_equal(counts[present], sc.counts_of(pred, target, C[:, 0], 65536, C0, (255,))[present])


def test_ties_resolve_by_input_row_not_sorted_row(env):
    """the (d^2, id) rule with ids = perm; with ids = None the same call resolves by sorted row, and the case makes the two differ"""
    ops, sparse, ME = env
    C, zero = sc.case("ties")
    q = int(np.flatnonzero(zero)[0])
    by_input = _fill(ops, C, zero)[0][q]
    by_sorted = _fill(ops, C, zero, ids=False)[0][q]
    assert by_input == sc.fill("ties")[q] and by_sorted != by_input
    keys = kc.keys_of(C.astype(np.int64))
    d2 = ((C[:, 1:].astype(np.int64) - C[q, 1:]) ** 2).sum(1)
    tied = np.flatnonzero((d2 == 5) & ~zero)
    assert by_sorted == tied[np.argmin(keys[tied])]


def test_axis_mask_is_reported_and_the_call_returns(env):
    """a decoded coordinate of 32768 or more on y: status[3] = 2; nn is undefined, the stored values stay rows of the query's entry"""
    ops, sparse, ME = env
    C = kc.batched({0: np.vstack([kc.cube(3), kc.cube(3, (0, 40000, 0))]), 1: kc.cube(3)}, np.random.default_rng(3))
    zero = (C[:, 1] == 1)
    for axes in (7, 6):
        perm, rank, keys, st = ops.coords_order_batched(_dev(C))
        zs = _dev(zero.astype(np.uint8)).index_select(0, perm.long())
        nn, status = ops.nn1_batched(keys, perm, 1 - zs, zs, axes)
        assert status.tolist() == [int(zero.sum()), int((~zero).sum()), 0, 2]
        nn, zs, p = nn.cpu().numpy(), zs.cpu().numpy().astype(bool), perm.cpu().numpy()
        assert (nn[~zs] == -1).all() and (nn[zs] >= 0).all() and (nn[zs] < len(C)).all()
        assert (C[p[nn[zs]], 0] == C[p[zs], 0]).all() and not zs[nn[zs]].any()


# ------------------------------------------------------------------------------------------ fill="yz" and the parent's scene tail
def test_yz_fill_and_the_scene_tail_per_entry(env):
    """fill="yz": the masked distance (ties at 0 along x resolved by input row) equals the brute force, and per entry pred and counts
    equal validation.scene_tail run on that entry's rows alone"""
    ops, sparse, ME = env
    from geopurify_amd import validation
    C, zero = sc.case("yz")
    F, cls = sc.features("yz", D0, C0)
    ref = sc.fill("yz", 6)
    q = kc.row_of(C, 0, (10, 50, 50))
    assert ref[q] == min(kc.row_of(C, 0, (x, 50, 50)) for x in (20, 3, 11)) != sc.fill("yz")[q]
    target = sc.target_of(cls, C0, 12)
    seg, _ = _segment(env, "yz", fill="yz", labels=_dev(target))
    assert np.array_equal(seg.filled_from.cpu().numpy(), ref)
    assert np.array_equal(seg.pred.cpu().numpy(), sc.pred_of(cls, ref))
    text = _dev(sc.text(D0, C0)).float()
    for b in (0, 1):
        rows = np.flatnonzero(C[:, 0] == b)
        counts = torch.zeros((3, C0), dtype=torch.int64, device="cuda")
        res = {"scene_features": _dev(F[rows]), "text_features": text, "logit_scale": 3.0}
        pred = validation.scene_tail(None, res, _dev(C[rows, 1:].astype(np.float32)), _dev(target[rows]), C0, [255], counts)
        assert torch.equal(seg.pred[_dev(rows)], pred)
        assert torch.equal(seg.counts[b], counts)


def test_fill_none_leaves_the_argmax(env):
    C, zero = sc.case("overlap")
    seg, cls = _segment(env, "overlap", fill=None)
    assert np.array_equal(seg.pred.cpu().numpy(), cls) and (seg.filled_from.cpu().numpy() == -1).all()
    assert np.array_equal(seg.zero.cpu().numpy(), zero) and seg.unfilled == 0


# ------------------------------------------------------------------------------------------ the classification routes
@pytest.mark.parametrize("D,Cn", [(10, 3), (512, 20), (96, 160)])
def test_classes_and_widths(env, D, Cn):
    """C = 3 at D = 10 (the generic classify kernel), C = 20 at D = 512, C = 160 at D = 96 (the GEMM route): labels exact"""
    seg, cls = _segment(env, "overlap", D, Cn)
    assert np.array_equal(seg.pred.cpu().numpy(), sc.pred_of(cls, sc.fill("overlap")))


# ------------------------------------------------------------------------------------------ the counts
def _absent_middle():
    C, zero = sc.case("overlap")
    C = C.copy()
    C[C[:, 0] == 1, 0] = 2
    return C, zero


def test_counts_per_entry(env):
    """two ignore labels, labels outside 0..C-1, B = 3 with the middle entry absent; counts.sum(0) equals ops.iou_hist over all rows"""
    ops, sparse, ME = env
    C, zero = _absent_middle()
    F, cls = sc.features("overlap", D0, C0)
    target = sc.target_of(cls, C0, 13, ignore=(255, 254))
    assert ((target == 255).sum() > 0 and (target == 254).sum() > 0 and (target >= C0).sum() > (target >= 254).sum() and (target < 0).sum() > 0)
    y = ME.SparseTensor(features=_dev(F), coordinates=_dev(C))
    seg = sparse.segment(y, _dev(sc.text(D0, C0)).float(), 3.0, labels=_dev(target), ignore_labels=(255, 254))
    pred = seg.pred.cpu().numpy()
    assert np.array_equal(pred, sc.pred_of(cls, sc.fill("overlap")))
    counts = seg.counts.cpu().numpy()
    assert counts.shape == (3, 3, C0) and counts[1].sum() == 0 and counts[0].sum() > 0 and counts[2].sum() > 0
    assert np.array_equal(counts, sc.counts_of(pred, target, C[:, 0], 3, C0, (255, 254)))
    whole = torch.zeros((3, C0), dtype=torch.int64, device="cuda")
    ops.iou_hist(seg.pred, _dev(target), C0, [255, 254], whole)
    assert torch.equal(seg.counts.sum(0), whole)


def test_counts_per_point_through_an_inverse_mapping(env):
    ops, sparse, ME = env
    C, zero = _absent_middle()
    F, cls = sc.features("overlap", D0, C0)
    rng = np.random.default_rng(14)
    inv = rng.integers(0, len(C), 1500)
    per_voxel = sc.pred_of(cls, sc.fill("overlap"))
    target = sc.target_of(per_voxel[inv], C0, 15)
    y = ME.SparseTensor(features=_dev(F), coordinates=_dev(C))
    seg = sparse.segment(y, _dev(sc.text(D0, C0)).float(), 3.0, labels=_dev(target), inverse_mapping=_dev(inv))
    assert np.array_equal(seg.pred.cpu().numpy(), per_voxel[inv])
    assert seg.filled_from.shape == (len(C),) and seg.zero.shape == (len(C),)
    assert np.array_equal(seg.counts.cpu().numpy(), sc.counts_of(per_voxel[inv], target, C[inv, 0], 3, C0, (255,)))


@pytest.mark.parametrize("Cn", [20, 4096])
def test_iou_hist_batched_both_stagings(env, Cn):
    """B * 3 * C = 180 words (LDS counters) and 36864 (past the LDS budget: 64-bit atomics on the counts); rows whose batch index is
    outside 0..B-1 are counted nowhere; the call adds to what counts holds"""
    ops, sparse, ME = env
    rng = np.random.default_rng(16 + Cn)
    n, B = 3000, 3
    batch = rng.integers(-1, B + 1, n)
    pred = rng.integers(0, Cn, n)
    target = np.where(rng.random(n) < 0.5, pred, rng.integers(-2, Cn + 2, n))
    target[rng.random(n) < 0.05] = 255
    coords = np.c_[batch, rng.integers(0, 50, (n, 3))].astype(np.int32)
    counts = torch.full((B, 3, Cn), 7, dtype=torch.int64, device="cuda")
    ops.iou_hist_batched(_dev(pred), _dev(coords), _dev(target), B, Cn, [255], counts)
    assert np.array_equal(counts.cpu().numpy() - 7, sc.counts_of(pred, target, batch, B, Cn, (255,)))


# ------------------------------------------------------------------------------------------ the whole chain
def test_chain_quantize_pool_segment(env):
    """quantize (duplicate points, 2 entries of about 300 voxels) -> affinity_pool (K = 8, D = 16, 2 applications, random embeddings) ->
    segment per point.  Labels equal the fp64 arg-max on the features affinity_pool returned wherever the top-2 margin is at least 0.1
    (pooling mixes classes, so some rows sit between two); at least 95 % of the rows do.  The counts are exact on the labels returned."""
    ops, sparse, ME = env
    rng = np.random.default_rng(17)
    D, Cn = 16, 5
    vox = kc.batched({0: kc.surface_exact(rng, 300, ext=24), 1: kc.surface_exact(rng, 310, ext=24)}, rng)
    pts = np.vstack([vox, vox[rng.integers(0, len(vox), 400)]])
    pts = pts[rng.permutation(len(pts))]
    t = sc.text(D, Cn)
    tn = t / np.linalg.norm(t, axis=1, keepdims=True)
    want = (pts[:, 1] // 8) % Cn                                                     # classes in slabs: neighbours mostly agree
    Fp = (4.0 * tn[want] + 0.05 * rng.standard_normal((len(pts), D))).astype(np.float32)
    q = sparse.quantize(_dev(pts), _dev(Fp), mode="average")
    x = ME.SparseTensor(features=q.features, coordinates=q.coordinates)
    E = torch.from_numpy(rng.standard_normal((q.coordinates.shape[0], 16)).astype(np.float32)).cuda()
    y = sparse.affinity_pool(x, E, K=8, num_iters=2)
    target = sc.target_of(want, Cn, 18)
    seg = sparse.segment(y, _dev(t).float(), 1.0, labels=_dev(target), inverse_mapping=q.inverse_mapping)
    inv = q.inverse_mapping.cpu().numpy()
    margin, cls = sc.margins(y.F.cpu().numpy(), t)
    ok = (margin >= sc.MARGIN)[inv]
    print(f"chain: {ok.mean():.4f} of {len(inv)} points have a top-2 margin of at least {sc.MARGIN}")
    assert ok.mean() >= 0.95
    pred = seg.pred.cpu().numpy()
    assert pred.shape == (len(pts),) and np.array_equal(pred[ok], cls[inv][ok])
    assert not bool(seg.zero.any()) and seg.unfilled == 0
    batch = q.coordinates.cpu().numpy()[inv, 0]
    assert np.array_equal(batch, pts[:, 0])
    assert np.array_equal(seg.counts.cpu().numpy(), sc.counts_of(pred, target, batch, 2, Cn, (255,)))


# ------------------------------------------------------------------------------------------ extents
@pytest.mark.parametrize("name,axes", [("rung_scan", 7), ("overlap", 7), ("yz", 6), ("empty_entry", 7)])
def test_nn1_batched_no_access_outside_the_extents(env, name, axes):
    """keys, ids, masks, nn, status and a workspace of exactly the reported bytes inside poisoned guards: guards intact, same bits"""
    ops, sparse, ME = env
    from geopurify_amd import _lib
    C, zero = sc.case(name)
    perm, rank, keys, st = ops.coords_order_batched(_dev(C))
    zs = _dev(zero.astype(np.uint8)).index_select(0, perm.long())
    nv = len(C)
    nbytes = _lib.load().gp_nn1_batched_workspace_bytes(nv)
    assert nbytes > 0

    def call(a):
        nn, status = ops.nn1_batched(a.inp(keys, name="keys"), a.inp(perm, name="ids"), a.inp(1 - zs, name="ref_mask"), a.inp(zs, name="query_mask"),
                                     axes, nn=a.out(nv, torch.int32, name="nn"), status=a.out(4, torch.int32, name="status"),
                                     workspace=a.out(nbytes, torch.uint8, name="workspace"))
        return {"nn": nn, "status": status}

    out = extent_fence.run(call)
    assert extent_fence.unwritten(out["nn"]) == 0 and extent_fence.unwritten(out["status"]) == 0
    n = out["nn"].long()
    ff = torch.where(n >= 0, perm.long()[n.clamp(min=0)], n).index_select(0, rank.long())
    assert np.array_equal(ff.cpu().numpy(), sc.fill(name, axes))


@pytest.mark.parametrize("Cn,indexed", [(20, False), (20, True), (4096, True)])
def test_iou_hist_batched_no_access_outside_the_extents(env, Cn, indexed):
    ops, sparse, ME = env
    rng = np.random.default_rng(19)
    rows, B = 700, 3
    n = 1000 if indexed else rows
    coords = np.c_[rng.integers(-1, B + 1, rows), rng.integers(0, 50, (rows, 3))].astype(np.int32)
    pred = rng.integers(-1, Cn + 1, rows)
    index = rng.integers(-2, rows + 2, n) if indexed else None                       # (values outside the rows: counted nowhere, read nowhere)
    target = rng.integers(-1, Cn + 1, n)

    def call(a):
        counts = a.inp(torch.zeros((B, 3, Cn), dtype=torch.int64), name="counts")
        ops.iou_hist_batched(a.inp(_dev(pred), name="pred"), a.inp(_dev(coords), name="coords"), a.inp(_dev(target), name="target"), B, Cn, [255],
                             counts, index=a.inp(_dev(index), name="index") if indexed else None)
        return {"counts": counts}

    out = extent_fence.run(call)
    row = index if indexed else np.arange(rows)
    ok = (row >= 0) & (row < rows)
    ref = sc.counts_of(pred[row[ok]], target[ok], coords[row[ok], 0], B, Cn, (255,))
    assert np.array_equal(out["counts"].cpu().numpy(), ref)


def test_entries_refuse_before_any_launch(env):
    """axes = 0, a workspace one byte short, C = 4097, 5 ignore ids: the error code, the message, and outputs that still hold their poison"""
    ops, sparse, ME = env
    from geopurify_amd import _lib
    lib = _lib.load()
    C, zero = sc.case("overlap")
    perm, rank, keys, st = ops.coords_order_batched(_dev(C))
    zs = _dev(zero.astype(np.uint8)).index_select(0, perm.long())
    ref = 1 - zs
    nv = len(C)
    a = extent_fence.Arena(False)
    nn, status = a.out(nv, torch.int32), a.out(4, torch.int32)
    nbytes = lib.gp_nn1_batched_workspace_bytes(nv)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.gp_nn1_batched(p(keys), p(perm), p(ref), p(zs), nv, 0, p(nn), p(status), p(ws), nbytes, stream) == -22
    assert b"gp_nn1_batched: axes=0 not in 1..7" in lib.gp_last_error()
    assert lib.gp_nn1_batched(p(keys), p(perm), p(ref), p(zs), nv, 8, p(nn), p(status), p(ws), nbytes, stream) == -22
    assert lib.gp_nn1_batched(p(keys), p(perm), p(ref), p(zs), nv, 7, p(nn), p(status), p(ws), nbytes - 1, stream) == -12
    assert f"gp_nn1_batched: workspace too small ({nbytes - 1} < {nbytes})".encode() in lib.gp_last_error()
    assert lib.gp_nn1_batched(p(keys), p(perm), None, p(zs), nv, 7, p(nn), p(status), p(ws), nbytes, stream) == -22
    assert lib.gp_nn1_batched(p(keys), p(perm), p(ref), p(zs), 0, 7, p(nn), p(status), p(ws), nbytes, stream) == -22
    assert lib.gp_nn1_batched_workspace_bytes(0) == 0 and lib.gp_nn1_batched_workspace_bytes(2 ** 31) == 0
    counts = a.out((3, 3, 20), torch.int64)
    pred, coords, target = torch.zeros(nv, dtype=torch.int64, device="cuda"), _dev(C), torch.zeros(nv, dtype=torch.int64, device="cuda")
    ig = (ctypes.c_int64 * 5)(1, 2, 3, 4, 5)
    hist = lambda B, Cn, nig, n=nv: lib.gp_iou_hist_batched_i64(p(pred), p(coords), nv, p(target), None, n, B, Cn, ig, nig, p(counts), stream)
    assert hist(3, 4097, 1) == -22 and b"num_classes=4097 not in 1..4096" in lib.gp_last_error()
    assert hist(3, 20, 5) == -22 and b"at most 4 ignore ids" in lib.gp_last_error()
    assert hist(0, 20, 1) == -22 and hist(3, 0, 1) == -22 and hist(3, 20, 1, nv - 1) == -22
    torch.cuda.synchronize()
    assert extent_fence.unwritten(nn) == nv and extent_fence.unwritten(status) == 4 and extent_fence.unwritten(counts) == counts.numel()


# ------------------------------------------------------------------------------------------ refusals of the public call
def _refusals():
    C, zero = sc.case("overlap")
    n = len(C)
    F = sc.features("overlap", D0, C0)[0]
    base = dict(C=C, F=F, text=sc.text(D0, C0), kw={})
    def r(name, message, **ch):
        d = dict(base)
        d.update(ch)
        return pytest.param(d, message, id=name)
    wide = kc.batched({0: np.vstack([kc.cube(3), kc.cube(3, (32765, 0, 0))])}, np.random.default_rng(4))
    dup = np.ascontiguousarray(np.vstack([C, C[7:9]]))
    neg = C.copy()
    neg[3, 0] = -1
    top = C.copy()
    top[C[:, 0] == 1, 0] = 65535
    labels = np.zeros(n, np.int64)
    yield r("extent_32768", r"segment: coordinate extent of 32768 or more along x", C=wide, F=np.ones((len(wide), D0), np.float32))
    yield r("duplicate_rows", r"segment: 2 duplicate coordinate rows", C=dup, F=np.ones((len(dup), D0), np.float32))
    yield r("batch_index", r"segment: 1 rows have a batch index outside 0\.\.65535", C=neg)
    yield r("float_coordinates", r"segment: coordinates must be integers, got torch.float32", C=C.astype(np.float32))
    yield r("feature_rows", rf"segment: features must be \[N, D\] with N = {n} coordinate rows", F=F[:-1])
    yield r("text_width", rf"segment: text_features must be \[C, D\] with D = {D0} feature columns", text=sc.text(D0 + 1, C0))
    yield r("num_classes", r"segment: num_classes=4097 outside 1\.\.4096", kw=dict(num_classes=4097))
    yield r("num_classes_0", r"segment: num_classes=0 outside 1\.\.4096", kw=dict(num_classes=0))
    yield r("ignore_labels", r"segment: 5 ignore labels, at most 4", kw=dict(ignore_labels=(1, 2, 3, 4, 5)))
    yield r("labels_length", rf"segment: labels must be an integer tensor \[{n}\] \(one per voxel\)", kw=dict(labels=labels[:-1]))
    yield r("labels_dtype", rf"segment: labels must be an integer tensor \[{n}\]", kw=dict(labels=labels.astype(np.float32)))
    yield r("labels_per_point", r"segment: labels must be an integer tensor \[7\] \(one per point of inverse_mapping\)",
            kw=dict(labels=labels, inverse_mapping=np.arange(7)))
    yield r("inverse_dtype", r"segment: inverse_mapping must be an integer tensor \[P\]", kw=dict(inverse_mapping=np.zeros(7, np.float32)))
    yield r("inverse_range", rf"segment: 2 inverse_mapping values outside 0\.\.{n - 1}", kw=dict(inverse_mapping=np.array([0, n, 5, -1])))
    yield r("fill", r"segment: fill='zyx', expected one of", kw=dict(fill="zyx"))
    yield r("counts_size", r"segment: counts \[65536, 3, 4096\] would hold more than 2\^27 elements \(the highest batch index is 65535\)",
            C=top, kw=dict(labels=labels, num_classes=4096))


@pytest.mark.parametrize("case,message", list(_refusals()))
def test_segment_refuses(env, case, message):
    ops, sparse, ME = env
    kw = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in case["kw"].items()}
    y = ME.SparseTensor(features=_dev(case["F"]), coordinates=_dev(case["C"]))
    with pytest.raises(ValueError, match=message):
        sparse.segment(y, _dev(case["text"]).float(), **kw)


def test_segment_refuses_what_is_no_sparse_tensor(env):
    ops, sparse, ME = env
    with pytest.raises(ValueError, match="segment: y must be a SparseTensor"):
        sparse.segment(torch.zeros(3, 4, device="cuda"), torch.zeros(2, 4, device="cuda"))


# ------------------------------------------------------------------------------------------ determinism, no gradients, read-backs
def test_twice_the_same_bits_no_grad_one_readback(env):
    ops, sparse, ME = env
    C, zero = sc.case("rung_scan")
    F, cls = sc.features("rung_scan", D0, C0)
    target = _dev(sc.target_of(cls, C0, 20))
    feats = _dev(F).requires_grad_(True)
    text = _dev(sc.text(D0, C0)).float().requires_grad_(True)
    y = ME.SparseTensor(features=feats, coordinates=_dev(C))
    before = ops.READBACK["calls"]
    a = sparse.segment(y, text, 3.0, labels=target)
    assert ops.READBACK["calls"] - before == 1                                       # int32 coordinates: the status read-back alone
    b = sparse.segment(y, text, 3.0, labels=target)
    for name in ("pred", "zero", "filled_from", "counts"):
        ta, tb = getattr(a, name), getattr(b, name)
        assert torch.equal(ta, tb) and not ta.requires_grad
    assert a.unfilled == b.unfilled == 0
    before = ops.READBACK["calls"]
    c = sparse.segment(ME.SparseTensor(features=feats, coordinates=_dev(C).long()), text, 3.0, labels=target)
    assert ops.READBACK["calls"] - before == 2                                       # int64 coordinates: the range read-back first
    assert torch.equal(c.pred, a.pred) and torch.equal(c.counts, a.counts)
