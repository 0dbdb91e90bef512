"""sparse.lift on the GPU: the 2D -> 3D lift over batched point clouds against the per-entry reference of tests/lift_batched_cases.py
(the oracle's mapping, drop rule and lift, one scene at a time) and against the per-scene kernels it replaces.

Bounds.  Exact: seen, count, view_count, view_keep and the fill's choice (nn).  "nearest" features: the same bits as the reference --
the fp32 adds are the same, in the same order, and the one division is the same (tests/test_gpu_kernels.py::test_lift_dense holds the
per-view kernels to that).  "bilinear" features: the same bits as the existing ops.lift_dense_bilinear_accum sequence run per entry on
the same lists, and within 1e-6 of the oracle's F.interpolate on maps in [-1, 1], the bound of tests/test_gpu_lift_edges.py and
tests/test_gpu_configs.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

import extent_fence
import lift_batched_cases as lb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BILINEAR_TOL = 1e-6


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import _lib, ops, sparse
    _lib.load()
    return ops, sparse


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _views(sparse, c, layout="nchw", maps=None):
    maps = _dev(c.maps) if maps is None else maps
    if layout == "channels_last":
        maps = maps.contiguous(memory_format=torch.channels_last)
    return sparse.Views(maps, _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), None if c.depth is None else _dev(c.depth),
                        None if (c.H, c.W) == (c.h, c.w) else (c.H, c.W))


def _options(c):
    return dict(mode=c.mode, cut_bound=c.cut, vis_thres=c.tau, min_visible=c.min_visible, max_visible=c.max_visible)


def _lift(env, c, layout="nchw", points=None, **kw):
    ops, sparse = env
    return sparse.lift(_dev(c.points) if points is None else points, _views(sparse, c, layout), **{**_options(c), **kw})


def _raw(env, c, buffers=None, workspace=None, maps_pm=None, view_entry=None, fill=True):
    """ops.lift_batched on a case (the pixel-major maps through ops.lift_batched_transpose)"""
    ops, _ = env
    maps_pm = ops.lift_batched_transpose(_dev(c.maps)) if maps_pm is None else maps_pm
    return ops.lift_batched(_dev(c.points), maps_pm, (c.h, c.w), _dev(c.view_entry) if view_entry is None else view_entry, _dev(c.w2c),
                            _dev(c.intr), None if c.depth is None else _dev(c.depth), (c.H, c.W), c.mode == "bilinear", c.cut, c.tau,
                            c.min_visible, 2 ** 63 - 1 if c.max_visible is None else c.max_visible, fill=fill, buffers=buffers,
                            workspace=workspace)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _per_scene(env, c):
    """The sequence the batched call replaces, entry by entry on the same inputs: ops.views_visible_lists, one accumulating launch per
    kept view, ops.lift_dense_finish, ops.nn1_masked, ops.gather_rows -> (features, seen, view_count, view_keep)"""
    ops, _ = env
    feats = torch.zeros((c.N, c.D), dtype=torch.float32, device="cuda")
    seen = torch.zeros(c.N, dtype=torch.bool, device="cuda")
    view_count, view_keep = torch.zeros(c.V, dtype=torch.int64), torch.zeros(c.V, dtype=torch.bool)
    maps = _dev(c.maps)
    for b in c.entries():
        rows, vs = c.rows_of(b), c.views_of(b)
        if len(vs) == 0:
            continue
        n = len(rows)
        params = _dev(np.concatenate([c.w2c[vs].reshape(len(vs), 16), c.intr[vs]], 1))
        ent = ops.views_visible_lists(_dev(c.points[rows, 1:]), params, None if c.depth is None else _dev(c.depth[vs]), c.W, c.H, c.cut, c.tau,
                                      c.min_visible, 2 ** 62 if c.max_visible is None else c.max_visible)
        off, keep = ent["view_off"].tolist(), ent["keep"].tolist()
        s = torch.zeros((n, c.D), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(n, dtype=torch.float32, device="cuda")
        for i, v in enumerate(vs):
            view_count[v], view_keep[v] = off[i + 1] - off[i], bool(keep[i])
            if not keep[i]:
                continue
            pt, x, y = (ent[k][off[i]:off[i + 1]] for k in ("pt", "x", "y"))
            if c.mode == "bilinear":
                ops.lift_dense_bilinear_accum(maps[v], c.H, c.W, pt, x, y, s, cnt)
            else:
                ops.lift_dense_accum(maps[v], pt, x, y, s, cnt)
        sn = ops.lift_dense_finish(s, c.D, cnt)
        nn = ops.nn1_masked(_dev(c.points[rows, 1:].astype(np.float32)), sn, 1 - sn)
        out = ops.gather_rows(s, c.D, torch.where(nn >= 0, nn, torch.arange(n, device="cuda")))
        feats[_dev(rows)], seen[_dev(rows)] = out, sn.bool()
    return feats, seen, view_count, view_keep


# ------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", lb.CASES)
def test_lift_matches_the_reference(env, name):
    c, ref = lb.case(name), lb.reference(name)
    got = _lift(env, c)
    assert got.features.dtype == torch.float32 and got.features.shape == (c.N, c.D) and not got.features.requires_grad
    assert got.seen.dtype == torch.bool and got.count.dtype == torch.int32 and got.view_count.dtype == torch.int64 and got.view_keep.dtype == torch.bool
    assert np.array_equal(got.seen.cpu().numpy(), ref.seen) and np.array_equal(got.count.cpu().numpy(), ref.count)
    assert np.array_equal(got.view_count.cpu().numpy(), ref.view_count) and np.array_equal(got.view_keep.cpu().numpy(), ref.view_keep)
    raw = _raw(env, c)
    assert np.array_equal(raw.nn.cpu().numpy(), ref.filled_from)                 # the fill's choice
    status = raw.status.tolist()
    assert status[:3] == [0, 0, 0] and status[3] == int(c.entries().max()) and status[4] == int(ref.seen.sum())
    assert status[5] == int((ref.filled_from >= 0).sum())
    f = got.features.cpu().numpy()
    if c.mode == "nearest":
        assert np.array_equal(f.view(np.int32), ref.features.view(np.int32))
    else:
        err = float(np.abs(f.astype(np.float64) - ref.features.astype(np.float64)).max())
        print(f"{name}: max |features - oracle| = {err:.3e}")
        assert np.abs(c.maps).max() <= 1.0 and err <= BILINEAR_TOL
    # without the fill an unseen row is zero and a seen row is the filled call's
    plain = _lift(env, c, fill=False)
    seen = got.seen
    assert torch.equal(_bits(plain.features[seen]), _bits(got.features[seen])) and not bool(plain.features[~seen].any())


@pytest.mark.parametrize("name", lb.CASES)
def test_bit_equal_to_the_per_scene_kernels(env, name):
    c = lb.case(name)
    got = _lift(env, c)
    feats, seen, view_count, view_keep = _per_scene(env, c)
    assert torch.equal(got.seen, seen) and torch.equal(got.view_count.cpu(), view_count) and torch.equal(got.view_keep.cpu(), view_keep)
    assert torch.equal(_bits(got.features), _bits(feats))


# ------------------------------------------------------------------------------------------ invariances
@pytest.mark.parametrize("name", ["views_130", "views_130_bilinear", "D_chunk_plus_1", "bilinear_h1", "entries", "twins"])
def test_row_order_and_map_layout_do_not_change_a_point(env, name):
    c = lb.case(name)
    base = _lift(env, c)
    again = _lift(env, c)
    for a, b in ((base.features, again.features), (base.count, again.count), (base.view_count, again.view_count)):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    cl = _lift(env, c, layout="channels_last")
    assert torch.equal(_bits(cl.features), _bits(base.features)) and torch.equal(cl.seen, base.seen) and torch.equal(cl.count, base.count)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(c.N)).cuda()
    sh = _lift(env, c, points=_dev(c.points)[perm])
    assert torch.equal(_bits(sh.features), _bits(base.features[perm])) and torch.equal(sh.seen, base.seen[perm])
    assert torch.equal(sh.count, base.count[perm]) and torch.equal(sh.view_count, base.view_count) and torch.equal(sh.view_keep, base.view_keep)
    # fp32 points that hold the same values, and maps of another floating dtype that holds them too
    p32 = _dev(c.points.astype(np.float32))
    if np.array_equal(c.points.astype(np.float32).astype(np.float64), c.points):
        assert torch.equal(_bits(_lift(env, c, points=p32).features), _bits(base.features))
    ops, sparse = env
    wide = sparse.lift(_dev(c.points), _views(sparse, c, maps=_dev(c.maps).double()), **_options(c))
    assert torch.equal(_bits(wide.features), _bits(base.features))


# ------------------------------------------------------------------------------------------ extents
@pytest.mark.parametrize("name", ["views_130", "D65", "D_chunk_plus_1_bilinear", "entries", "fill", "drop"])
def test_the_entry_points_stay_inside_their_extents(env, name):
    """ops.lift_batched_transpose and ops.lift_batched on fenced arrays: the fp32 maps, the integer table and every output (the rows
    with a pitch of their own, the workspace of exactly the reported bytes); the fp64 inputs have no fence type and stay plain.  Nothing
    outside the extents is written, nothing read from there reaches a result."""
    ops, _ = env
    from geopurify_amd import _lib
    lib = _lib.load()
    c, ref = lb.case(name), lb.reference(name)
    N, V, D = c.N, c.V, c.D

    def case(a):
        maps = a.inp(torch.from_numpy(c.maps), name="maps")
        maps_pm = a.out((V, c.h * c.w, D), torch.float32, name="maps_pm")
        ops.lift_batched_transpose(maps, out=maps_pm)
        ve = a.inp(torch.from_numpy(c.view_entry), name="view_entry")
        pitch = (D + 3) // 4 * 4 + 4 if a.fence else D
        bufs = {"out": a.out((N, D), torch.float32, pitch=pitch, name="out"), "seen": a.out(N, torch.uint8, name="seen"),
                "count": a.out(N, torch.int32, name="count"), "view_count": a.out(V, torch.int64, name="view_count"),
                "view_keep": a.out(V, torch.uint8, name="view_keep"), "nn": a.out(N, torch.int64, name="nn"),
                "status": a.out(8, torch.int64, name="status")}
        ws = a.out(lib.gp_lift_batched_workspace_bytes(N, V), torch.uint8, name="workspace")
        r = _raw(env, c, buffers=bufs, workspace=ws, maps_pm=maps_pm, view_entry=ve)
        return {"maps_pm": maps_pm, "out": r.out, "seen": r.seen, "count": r.count, "view_count": r.view_count, "view_keep": r.view_keep,
                "nn": r.nn, "status": r.status}

    got = extent_fence.run(case)
    for k in ("maps_pm", "out", "seen", "count", "view_count", "view_keep", "nn", "status"):
        assert extent_fence.unwritten(got[k]) == 0, k
    assert np.array_equal(got["nn"].cpu().numpy(), ref.filled_from) and np.array_equal(got["count"].cpu().numpy(), ref.count)
    assert np.array_equal(got["maps_pm"].cpu().numpy(), c.maps.reshape(V, D, -1).transpose(0, 2, 1))


def test_overlapping_arguments_are_refused(env):
    ops, _ = env
    from geopurify_amd._lib import GeoPurifyHipError
    c = lb.case("no_depth")
    both = torch.zeros(c.N + c.V, dtype=torch.uint8, device="cuda")
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        _raw(env, c, buffers={"seen": both[:c.N], "view_keep": both[c.N - 1:c.N - 1 + c.V]})
    maps_pm = ops.lift_batched_transpose(_dev(c.maps))
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        _raw(env, c, maps_pm=maps_pm, buffers={"out": maps_pm.view(-1)[:c.N * c.D].view(c.N, c.D)})
    with pytest.raises(GeoPurifyHipError, match="dst overlaps src"):
        ops.lift_batched_transpose(maps_pm.view(c.V, c.D, c.h, c.w), out=maps_pm)


# ------------------------------------------------------------------------------------------ the status errors
def test_status_errors(env):
    ops, sparse = env
    c = lb.case("no_depth")
    P = _dev(c.points)
    for value, message in ((65536.0, "1 rows have a batch index"), (-1.0, "1 rows have a batch index"), (0.5, "1 rows have a batch index"),
                           (float("nan"), "1 rows of points are not finite"), (float("inf"), "1 rows of points are not finite")):
        bad = P.clone()
        bad[7, 0] = value
        with pytest.raises(ValueError, match=message):
            sparse.lift(bad, _views(sparse, c), **_options(c))
    for col, value in ((1, float("nan")), (2, float("-inf")), (3, float("inf"))):
        bad = P.clone()
        bad[3, col], bad[9, col] = value, value
        with pytest.raises(ValueError, match="2 rows of points are not finite"):
            sparse.lift(bad, _views(sparse, c), **_options(c))
    for value in (65536, -1, 2 ** 40):
        v = _views(sparse, c)
        v.view_entry = v.view_entry.clone()
        v.view_entry[1] = value
        with pytest.raises(ValueError, match="1 views have a view_entry outside 0..65535"):
            sparse.lift(P, v, **_options(c))
    # the rows and views that are counted belong to no entry: the others' results do not change
    ref = _raw(env, c)
    bad = c.points.copy()
    bad[7, 0] = 70000.0
    ve = c.view_entry.copy()
    ve[c.views_of(1)[0]] = -5
    r = ops.lift_batched(_dev(bad), ops.lift_batched_transpose(_dev(c.maps)), (c.h, c.w), _dev(ve), _dev(c.w2c), _dev(c.intr), None, (c.H, c.W),
                         False, c.cut, c.tau, 0, 2 ** 63 - 1)
    assert r.status.tolist()[:3] == [1, 1, 0] and int(r.count[7]) == 0 and int(r.nn[7]) == -1 and not bool(r.out[7].any())
    assert int(r.view_count[c.views_of(1)[0]]) == 0
    rows0 = _dev(np.setdiff1d(c.rows_of(0), [7]))
    assert torch.equal(r.count[rows0], ref.count[rows0]) and torch.equal(_bits(r.out[rows0]), _bits(ref.out[rows0]))


def test_one_host_synchronisation(env):
    ops, sparse = env
    c = lb.case("views_130_bilinear")
    points, views, kw = _dev(c.points), _views(sparse, c), _options(c)
    torch.cuda.synchronize()
    before = ops.READBACK["calls"]
    real = ops.readback
    torch.cuda.set_sync_debug_mode("error")
    try:
        # (the read-back itself is ops.readback's .tolist(), the only synchronising call allowed: count it, forbid every other)

        def counted(t):
            torch.cuda.set_sync_debug_mode("default")
            try:
                return real(t)
            finally:
                torch.cuda.set_sync_debug_mode("error")
        ops.readback = counted
        sparse.lift(points, views, **kw)
    finally:
        ops.readback = real
        torch.cuda.set_sync_debug_mode("default")
    assert ops.READBACK["calls"] == before + 1


# ------------------------------------------------------------------------------------------ the chain
def test_chain_lift_quantize_purify_segment(env):
    """lift -> quantize -> purify(student) -> segment on two small entries: it runs, the labels are labels and the counts add up"""
    ops, sparse = env
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import MinkowskiEngine as ME
    finally:
        sys.path.pop(0)
    from geopurify_amd import pipeline as pl
    from geopurify_amd.affinity_module import AffinityPredictor
    D, Cn = 64, 20
    c = lb.generic("chain", 21, {0: 400, 1: 500}, {0: 4, 1: 5}, D)
    m = AffinityPredictor(D + 6, 128, 128)
    m.load_state_dict(pl.random_student_state_dict(D + 6, hidden=128, embed=128, num_blocks=4, seed=6))
    m = m.cuda()
    points = _dev(c.points)
    lifted = sparse.lift(points, _views(sparse, c), **_options(c))
    assert bool(lifted.seen.any()) and not bool(lifted.seen.all()) and bool(torch.isfinite(lifted.features).all())
    feats = torch.cat([lifted.features, points[:, 1:].float(), torch.ones((c.N, 3), device="cuda")], 1)
    q = sparse.quantize(points, feats, quantization_size=0.2)
    x = ME.SparseTensor(features=q.features, coordinates=q.coordinates)
    y = sparse.purify(m, x, feature_dim=D, K=24, num_iters=3)
    g = torch.Generator().manual_seed(3)
    text = torch.randn(Cn, D, generator=g).cuda()
    labels = torch.randint(0, Cn, (c.N,), generator=g).cuda()
    seg = sparse.segment(y, text, 14.3, labels=labels, inverse_mapping=q.inverse_mapping)
    assert bool(torch.isfinite(y.F).all())
    assert seg.pred.shape == (c.N,) and int(seg.pred.min()) >= 0 and int(seg.pred.max()) < Cn
    assert seg.counts.shape == (2, 3, Cn) and int(seg.counts[:, 2].sum()) == c.N
    assert seg.counts[:, 2].sum(1).tolist() == [400, 500]
