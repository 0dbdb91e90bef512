"""sparse.LiftMasksStream on the GPU: the mask-embedding lift with the views arriving in chunks (csrc/lift_masks_stream.hip) against
sparse.lift_masks on the concatenation of the chunks -- bit for bit in all six fields -- and against the per-entry reference of
tests/lift_masks_batched_cases.py.  The partitions come from tests/lift_masks_stream_cases.py, whose own claims
tests/test_lift_masks_stream_cases_host.py checks on the CPU.

Bounds.  Against sparse.lift_masks: the same bits (floats compared as int32), whatever the partition: everything before the fusion is
per view and runs through the same kernels, the fusion reads the same slot lists and table rows.  Against the reference: the rule of
tests/test_gpu_lift_masks_batched.py::test_lift_masks_matches_the_reference -- masks and counts exact, features within its TOL_LIFT
(imported) on every row the reference's own near-tie flags do not cover.  State size: a condition derived from the stream's contract
(what it may keep), not a measurement.
"""
import os
import sys

import numpy as np
import pytest
import torch

import extent_fence
import lift_masks_batched_cases as lm
import lift_masks_stream_cases as ms
from test_gpu_lift_masks_batched import TOL_LIFT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("features", "seen", "count", "view_count", "view_keep", "text_features")


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


def _views(sparse, c, idx=None):
    """the views idx of the case (all of them: None) as a MaskViews"""
    idx = np.arange(c.V) if idx is None else np.asarray(idx, np.int64)
    return sparse.MaskViews(_dev(c.pred_masks[idx]), _dev(c.pred_logits[idx]), _dev(c.mask_embed[idx]), _dev(c.view_entry[idx]), _dev(c.w2c[idx]),
                            _dev(c.intr[idx]), None if c.depth is None else _dev(c.depth[idx]), (c.H, c.W))


def _options(c):
    return dict(cut_bound=c.cut, vis_thres=c.tau, min_visible=c.min_visible, max_visible=c.max_visible)


def _stream(sparse, c, points=None):
    return sparse.LiftMasksStream(_dev(c.points) if points is None else points, _dev(c.text), c.scale, **_options(c))


def _streamed(sparse, c, chunks, fill=True):
    s = _stream(sparse, c)
    for ch in chunks:
        s.add(_views(sparse, c, ch))
    return s.finish(fill=fill)


_ONE_CALL = {}


def _one_call(sparse, c, order, fill):
    """sparse.lift_masks on the case's views in `order`: computed once per (case, order, fill) and shared"""
    key = (c.name, np.asarray(order, np.int64).tobytes(), fill)
    if key not in _ONE_CALL:
        _ONE_CALL[key] = sparse.lift_masks(_dev(c.points), _views(sparse, c, order), _dev(c.text), c.scale, fill=fill, **_options(c))
    return _ONE_CALL[key]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(got, want, what=""):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        if not torch.equal(_bits(a), _bits(b)):
            at = (_bits(a) != _bits(b)).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {f} differs from the one-call lift_masks, first at {at} ({int((_bits(a) != _bits(b)).sum())} elements)")
    assert got.logit_scale == want.logit_scale


def _assert_reference(c, ref, got):
    """the rule of tests/test_gpu_lift_masks_batched.py::test_lift_masks_matches_the_reference, its tolerance imported"""
    assert got.features.dtype == torch.float32 and got.features.shape == (c.N, c.D) and not got.features.requires_grad
    assert got.seen.dtype == torch.bool and got.count.dtype == torch.int32 and got.view_count.dtype == torch.int64 and got.view_keep.dtype == torch.bool
    assert np.array_equal(got.seen.cpu().numpy(), ref.seen) and np.array_equal(got.count.cpu().numpy(), ref.count)
    assert np.array_equal(got.view_count.cpu().numpy(), ref.view_count) and np.array_equal(got.view_keep.cpu().numpy(), ref.view_keep)
    assert got.logit_scale == c.scale
    assert float((got.text_features.cpu() - torch.nn.functional.normalize(torch.from_numpy(c.text), dim=-1)).abs().max()) <= 4 * 2.0 ** -24
    d = np.abs(got.features.cpu().numpy().astype(np.float64) - ref.features.astype(np.float64)).max(1)
    differ = d > TOL_LIFT
    print(f"{c.name}: {int(ref.near.sum())} rows flagged as near ties, {int(differ.sum())} rows differ by more than {TOL_LIFT} (max off the flags "
          f"{float(d[~ref.near].max()) if (~ref.near).any() else 0.0:.3e})")
    assert not (differ & ~ref.near).any()


# ------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize("kind", ms.EVERY_CASE)
@pytest.mark.parametrize("name", ms.CASES)
def test_bit_equal_to_the_one_call_lift_masks(env, name, kind):
    _, sparse = env
    c = lm.case(name)
    chunks = ms.partition(c, kind)
    order = ms.concatenation(chunks)
    for fill in (True, False):
        _assert_same(_streamed(sparse, c, chunks, fill), _one_call(sparse, c, order, fill), f"{name} / {kind} / fill={fill}")


@pytest.mark.parametrize("kind", tuple(ms.BOUNDARIES) + ("by_entry",))
@pytest.mark.parametrize("name", ms.BOUNDARY_CASES)
def test_bit_equal_at_the_word_boundaries_and_by_entry(env, name, kind):
    _, sparse = env
    c = lm.case(name)
    chunks = ms.partition(c, kind)
    order = ms.concatenation(chunks)                                             # (by_entry: the reordered concatenation)
    for fill in (True, False):
        _assert_same(_streamed(sparse, c, chunks, fill), _one_call(sparse, c, order, fill), f"{name} / {kind} / fill={fill}")


@pytest.mark.parametrize("name,kind", [("views_0_1_63", "singles"), ("scores", "singles"), ("fill_inview", "singles"), ("fill_257", "singles"),
                                       ("views_64_65", "by_entry")])
def test_stream_matches_the_reference(env, name, kind):
    _, sparse = env
    c = lm.case(name)
    chunks = ms.partition(c, kind)
    order = ms.concatenation(chunks)
    ref = lm.reference(name) if np.array_equal(order, np.arange(c.V)) else ms.reference_of(c, order)
    got = _streamed(sparse, c, chunks)
    _assert_reference(ms.subcase(c, order, name=c.name), ref, got)
    plain = _streamed(sparse, c, chunks, fill=False)                             # without the fill an unseen row is zero
    seen = got.seen
    assert torch.equal(_bits(plain.features[seen]), _bits(got.features[seen])) and not bool(plain.features[~seen].any())


# ------------------------------------------------------------------------------------------ snapshots
@pytest.mark.parametrize("name", ["views_130", "twins", "drop", "scores"])
def test_finish_is_a_snapshot(env, name):
    _, sparse = env
    c = lm.case(name)
    chunks = ms.partition(c, "random")
    s = _stream(sparse, c)
    for k, ch in enumerate(chunks):
        s.add(_views(sparse, c, ch))
        got = s.finish()
        _assert_same(got, _one_call(sparse, c, ms.concatenation(chunks[:k + 1]), True), f"{name} after {k + 1} chunks")
    _assert_same(got, _streamed(sparse, c, chunks), "against a stream that never finished in between")
    again = s.finish()
    _assert_same(again, got, "the last finish, twice")
    assert again.features.data_ptr() != got.features.data_ptr() and again.count.data_ptr() != got.count.data_ptr()   # new tensors
    assert again.view_count.data_ptr() != got.view_count.data_ptr()
    _assert_same(s.finish(fill=False), _one_call(sparse, c, np.arange(c.V), False), "fill=False after fill=True")


def test_idle_chunks_change_nothing(env):
    """a chunk of dropped views only, then a chunk of views whose entry has no points: finish before and after gives the same bits, and
    only the per-view fields grow"""
    _, sparse = env
    c = ms.idle_case()
    rest, dropped, pointless = ms.idle_partition()
    s = _stream(sparse, c)
    s.add(_views(sparse, c, rest))
    before = s.finish()
    ref_all = ms.reference_of(c, np.arange(c.V))
    seen_views, records = len(rest), s.num_records
    kept = (s._f_seg.data_ptr(), s._rec_row.data_ptr(), s._rec_row.numel())
    for idle in (dropped, pointless):
        s.add(_views(sparse, c, idle))
        after = s.finish()
        for f in ("features", "seen", "count"):
            assert torch.equal(_bits(getattr(after, f)), _bits(getattr(before, f))), f
        assert torch.equal(after.view_count[:seen_views], before.view_count[:seen_views])
        assert np.array_equal(after.view_count[seen_views:].cpu().numpy(), ref_all.view_count[idle])      # the reference's counts ...
        assert not bool(after.view_keep[seen_views:].any())                                               # ... and none is kept
        assert s.num_records == records and (s._rec_row.data_ptr(), s._rec_row.numel()) == kept[1:]       # no record was stored
        before, seen_views = after, seen_views + len(idle)
    order = ms.concatenation([rest, dropped, pointless])
    for fill in (True, False):
        _assert_same(_streamed(sparse, c, [rest, dropped, pointless], fill), _one_call(sparse, c, order, fill), f"idle / fill={fill}")
    _assert_reference(ms.subcase(c, order, name=c.name), ms.reference_of(c, order), before)
    # idle chunks first: the stream starts with views that leave nothing
    _assert_same(_streamed(sparse, c, [pointless, dropped, rest]), _one_call(sparse, c, ms.concatenation([pointless, dropped, rest]), True),
                 "idle chunks first")
    s = _stream(sparse, c)
    s.add(_views(sparse, c, pointless))
    _assert_same(s.finish(), _one_call(sparse, c, pointless, True), "nothing but views of an entry without points")


# ------------------------------------------------------------------------------------------ what the stream keeps
def _granules(nbytes):
    return -(-max(int(nbytes), 256) // 512) * 512


def test_state_size(env):
    """Contract 4, derived: after all views of views_130 were added one by one, the stream has grown since its construction by at most
    twice (the segment tables V x Q x (d4 + C) x 4 + 8 bytes x the visible entries lift_masks_batched_lists reports + 64 bytes per view)
    -- twice: the growing buffers double -- plus the scratch one single-view add retains, read from the workspace queries.  No term in
    Q x h x w times the views."""
    ops, sparse = env
    c = lm.case("views_130")
    chunks = ms.partition(c, "singles")
    want = _one_call(sparse, c, np.arange(c.V), True)                            # (also leaves the tap tables in their cache)
    views = [_views(sparse, c, ch) for ch in chunks]
    ref = lm.reference("views_130")
    entries, most = int(ref.view_count.sum()), int(ref.view_count.max())
    d4 = (c.D + 3) // 4 * 4
    s = _stream(sparse, c)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    grown, held = [], []
    for v in views:
        s.add(v)
        torch.cuda.synchronize()
        grown.append(torch.cuda.memory_allocated() - base)
        held.append(sum(_granules(w.numel()) for w in s._ws.values()))          # add's retained workspaces
    scratch = (_granules(ops.lift_masks_batched_lists_workspace_bytes(c.N, 1)) + _granules(ops.lift_masks_stream_sizes_workspace_bytes(1))
               + _granules(28 * ((most + 31) // 32 * 32)) + _granules(ops.lift_masks_stream_add_workspace_bytes(c.N, 1, c.Q, (c.h, c.w), (c.H, c.W), most)))
    kept = c.V * c.Q * (d4 + c.C) * 4 + 8 * entries + 64 * c.V
    masks = c.V * c.Q * c.h * c.w * 4
    print(f"grown by {grown[-1]} B after {c.V} views ({grown[1]} B after 2); kept terms {kept} B, retained scratch <= {scratch} B; the masks are "
          f"{masks} B")
    assert grown[-1] <= 2 * kept + scratch and held[-1] <= scratch
    assert (grown[-1] - held[-1]) - (grown[1] - held[1]) <= 2 * kept            # from the 2nd to the last chunk: the kept terms alone
    assert s.num_records == int(ref.view_count[ref.view_keep].sum()) <= entries
    _assert_same(s.finish(), want, "views_130 one by one")


def test_one_read_back_per_add_and_one_per_finish(env):
    ops, sparse = env
    c = lm.case("views_130")
    chunks = ms.partition(c, "random")
    views = [_views(sparse, c, ch) for ch in chunks]
    points, text = _dev(c.points), _dev(c.text)
    torch.cuda.synchronize()
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
        sparse._TAPS.clear()                                                     # the tap tables are built and uploaded inside an add too
        before = ops.READBACK["calls"]
        s = sparse.LiftMasksStream(points, text, c.scale, **_options(c))
        assert ops.READBACK["calls"] == before                                   # construction: none
        for i, v in enumerate(views):
            s.add(v)
            assert ops.READBACK["calls"] == before + i + 1                       # every add: exactly one
        got = s.finish()
        assert ops.READBACK["calls"] == before + len(views) + 1                  # finish: exactly one
        s.finish(fill=False)
        assert ops.READBACK["calls"] == before + len(views) + 2
    finally:
        ops.readback = real
        torch.cuda.set_sync_debug_mode("default")
    _assert_same(got, _one_call(sparse, c, np.arange(c.V), True), "under the sync debug mode")


# ------------------------------------------------------------------------------------------ refusals before any kernel
def test_refusals_before_any_kernel(env):
    ops, sparse = env
    c = lm.case("twins")
    chunks = ms.partition(c, "by_entry")
    P, T = _dev(c.points), _dev(c.text)
    with pytest.raises(ValueError, match="CUDA tensors"):
        sparse.LiftMasksStream(P.cpu(), T, c.scale)
    with pytest.raises(ValueError, match="CUDA tensors"):
        sparse.LiftMasksStream(P, T.cpu(), c.scale)
    with pytest.raises(ValueError, match=r"points must be \[N, 4\]"):
        sparse.LiftMasksStream(P[:, :3], T, c.scale)
    with pytest.raises(ValueError, match="text_embed must be floating point"):
        sparse.LiftMasksStream(P, T[0], c.scale)
    with pytest.raises(ValueError, match="text_embed require grad"):
        sparse.LiftMasksStream(P, T.clone().requires_grad_(), c.scale)
    with pytest.raises(ValueError, match="logit_scale"):
        sparse.LiftMasksStream(P, T, "14")
    with pytest.raises(ValueError, match="cut_bound"):
        sparse.LiftMasksStream(P, T, c.scale, cut_bound=-1)
    with pytest.raises(ValueError, match="vis_thres"):
        sparse.LiftMasksStream(P, T, c.scale, vis_thres=None)
    with pytest.raises(ValueError, match="min_visible"):
        sparse.LiftMasksStream(P, T, c.scale, min_visible=-2)
    s = _stream(sparse, c)
    with pytest.raises(ValueError, match="no views were added"):
        s.finish()
    s.add(_views(sparse, c, chunks[0]))
    want = s.finish()
    launches = {"n": 0}
    names = ("lift_masks_batched_lists", "lift_masks_stream_sizes", "lift_masks_stream_add", "segment_tables")
    real = [getattr(ops, n) for n in names]

    def counted(f):
        def g(*a, **k):
            launches["n"] += 1
            return f(*a, **k)
        return g

    def refused(views, match):
        for n, f in zip(names, real):
            setattr(ops, n, counted(f))
        try:
            with pytest.raises(ValueError, match=match):
                s.add(views)
        finally:
            for n, f in zip(names, real):
                setattr(ops, n, f)
        assert launches["n"] == 0                                                # no op of the call ran
        _assert_same(s.finish(), want, f"after the refusal '{match}'")           # ... and the stream is as it was

    ch = chunks[1]
    good = lambda: _views(sparse, c, ch)                                         # noqa: E731
    V = len(ch)
    refused("views", "must be a MaskViews")
    refused(None, "must be a MaskViews")
    v = good()                                                                   # another Q
    v.pred_masks, v.pred_logits, v.mask_embed = (torch.cat([t, t[:, :1]], 1) for t in (v.pred_masks, v.pred_logits, v.mask_embed))
    refused(v, "Q of a chunk")
    v = good()                                                                   # another C
    v.pred_logits = torch.cat([v.pred_logits, v.pred_logits[..., :1]], -1)
    refused(v, "views.pred_logits must be floating point")
    v = good()                                                                   # another D
    v.mask_embed = torch.cat([v.mask_embed, v.mask_embed[..., :1]], -1)
    refused(v, "views.mask_embed must be floating point")
    v = good()                                                                   # another (h, w)
    v.pred_masks = v.pred_masks[:, :, :-1].contiguous()
    refused(v, r"\(h, w\) of a chunk")
    v = good()                                                                   # another image_shape
    v.image_shape, v.depth = (c.H + 1, c.W), None if v.depth is None else torch.cat([v.depth, v.depth[:, :1]], 1)
    refused(v, "image_shape of a chunk")
    v = good()                                                                   # depth present, then absent (or the other way round)
    v.depth = None if v.depth is not None else torch.ones((V, c.H, c.W), dtype=torch.float64, device="cuda")
    refused(v, "the presence of depth")
    v = good()                                                                   # another device
    v.pred_masks = v.pred_masks.cpu()
    refused(v, "CUDA tensors")
    v = good()
    v.view_entry = v.view_entry.cpu()
    refused(v, "CUDA tensors")
    for field in ("pred_masks", "pred_logits", "mask_embed"):
        v = good()
        setattr(v, field, getattr(v, field).clone().requires_grad_())
        refused(v, "require grad")
    v = good()
    v.world_to_camera = v.world_to_camera.float()
    refused(v, "world_to_camera must be fp64")
    v = good()
    v.pred_masks = torch.zeros((V, c.Q, c.H + 1, c.w), device="cuda")
    refused(v, "larger than image_shape")
    v = good()
    v.pred_masks = v.pred_masks.double()
    refused(v, "views.pred_masks must be fp32")
    v = good()
    v.image_shape = None
    refused(v, "views.image_shape must be")
    # records past 2^31 - 2: known from the chunk's read-back, before anything of the stream has changed
    records = s.num_records
    s.num_records = 2 ** 31 - 2 - 3
    try:
        with pytest.raises(ValueError, match=r"at most 2\^31 - 2 in all"):
            s.add(good())
    finally:
        s.num_records = records
    _assert_same(s.finish(), want, "after the refused records")
    s.add(good())
    _assert_same(s.finish(), _one_call(sparse, c, ms.concatenation(chunks), True), "after the refusals")
    # Q > 1024 is lift_masks' own refusal
    v = good()
    v.pred_masks = torch.zeros((V, 1025, 2, 3), device="cuda")
    v.pred_logits, v.mask_embed = torch.zeros((V, 1025, c.C + 1), device="cuda"), torch.zeros((V, 1025, c.D), device="cuda")
    with pytest.raises(ValueError, match="1025 queries"):
        _stream(sparse, c).add(v)
    assert not s.finish().features.requires_grad
    assert not sparse.LiftMasksStream(P.clone().requires_grad_(), T, c.scale, **_options(c))._st.points.requires_grad


def test_the_65536th_view_is_refused(env):
    _, sparse = env
    V = 65535
    P = _dev(np.array([[0, 0.0, 0.0, 1.0], [0, 0.0, 0.0, 2.0], [1, 0.0, 0.0, 1.0], [1, 0.0, 0.0, -1.0]]))
    g = torch.Generator().manual_seed(7)
    pm = torch.randn((V, 2, 1, 1), generator=g).cuda() * 4
    pl, me, text = torch.randn((V, 2, 3), generator=g).cuda(), torch.randn((V, 2, 4), generator=g).cuda(), torch.randn((2, 4), generator=g).cuda()
    ve = (torch.arange(V) % 2).cuda()
    M = torch.eye(4, dtype=torch.float64).repeat(V, 1, 1).cuda()
    K = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float64).repeat(V, 1).cuda()
    views = sparse.MaskViews(pm, pl, me, ve, M, K, None, (1, 1))
    s = sparse.LiftMasksStream(P, text, 10.0)
    s.add(views)
    want = s.finish()
    assert want.count.tolist() == [32768, 32768, 32767, 0] and s.num_views == V and s.most_views == 32768
    _assert_same(want, sparse.lift_masks(P, views, text, 10.0), "65535 views")
    with pytest.raises(ValueError, match="at most 65535 in all"):
        s.add(sparse.MaskViews(pm[:1], pl[:1], me[:1], ve[:1], M[:1], K[:1], None, (1, 1)))
    _assert_same(s.finish(), want, "after the refused 65536th view")


# ------------------------------------------------------------------------------------------ the status errors
def test_status_errors(env):
    ops, sparse = env
    c = lm.case("C19")
    chunks = ms.partition(c, "by_entry")
    assert len(chunks) == 2
    P = _dev(c.points)

    def run(points=None, second=None):
        s = _stream(sparse, c, points=points)
        s.add(_views(sparse, c, chunks[0]))
        s.add(_views(sparse, c, chunks[1]) if second is None else second)
        return s

    for value, message in ((65536.0, "1 rows have a batch index"), (-1.0, "1 rows have a batch index"), (0.5, "1 rows have a batch index"),
                           (float("nan"), "1 rows of points are not finite"), (float("inf"), "1 rows of points are not finite")):
        bad = P.clone()
        bad[7, 0] = value
        s = run(points=bad)                                                      # (the construction and the adds raise nothing)
        with pytest.raises(ValueError, match=message):
            s.finish()
    for col, value in ((1, float("nan")), (2, float("-inf")), (3, float("inf"))):
        bad = P.clone()
        bad[3, col], bad[9, col] = value, value
        with pytest.raises(ValueError, match="2 rows of points are not finite"):
            run(points=bad).finish()
    for value in (65536, -1, 2 ** 40):
        v = _views(sparse, c, chunks[1])
        v.view_entry = v.view_entry.clone()
        v.view_entry[1] = value
        s = run(second=v)
        for _ in range(2):                                                       # counted once, whatever the number of finish calls
            with pytest.raises(ValueError, match="1 views have a view_entry outside 0..65535"):
                s.finish()
    # precedence: non-finite rows, then bad batch rows, then bad views -- lift_masks' own, on the same inputs
    bad = P.clone()
    bad[7, 0], bad[8, 1] = 70000.0, float("nan")
    v = _views(sparse, c, chunks[1])
    v.view_entry = v.view_entry.clone()
    v.view_entry[0] = -1
    with pytest.raises(ValueError, match="1 rows of points are not finite"):
        run(points=bad, second=v).finish()
    bad[8, 1] = 0.0
    with pytest.raises(ValueError, match="1 rows have a batch index"):
        run(points=bad, second=v).finish()
    # the rows and views that are counted belong to no entry: the stream and the one call agree on everybody else
    bad = c.points.copy()
    bad[7, 0] = 70000.0
    ve = c.view_entry.copy()
    ve[int(chunks[1][0])] = -5
    moved = lm.Case("moved", lm.lb.Case("moved", bad, c.geo.maps, ve, c.w2c, c.intr, c.depth), c.pred_masks, c.pred_logits, c.mask_embed, c.text,
                    c.scale)
    raw = _raw(env, moved, chunks, extent_fence.Arena(False))
    order = ms.concatenation(chunks)
    lists = ops.lift_masks_batched_lists(_dev(bad), _dev(ve[order]), _dev(c.w2c[order]), _dev(c.intr[order]),
                                         None if c.depth is None else _dev(c.depth[order]), (c.H, c.W), moved.cut, moved.tau, moved.min_visible,
                                         2 ** 63 - 1 if moved.max_visible is None else moved.max_visible)
    f_seg, l_seg = _tables(ops, moved, order)
    one = ops.lift_masks_batched(_dev(bad), _dev(ve[order]), _dev(c.pred_masks[order]), _scores(_dev(c.pred_logits[order])), _taps(env, c), (c.H, c.W),
                                 (lists.pt, lists.x, lists.y, lists.view), lists.view_off, lists.view_keep, lists.total,
                                 max(1, -(-lists.max_views // 64)), f_seg, l_seg)
    assert raw["status"].tolist()[:3] == [1, 1, 0] == one.status.tolist()[:3] and raw["status"].tolist()[6:] == [0, 0]
    for k in ("out", "seen", "count", "nn"):
        assert torch.equal(_bits(raw[k]), _bits(getattr(one, k))), k
    assert int(raw["count"][7]) == 0 and int(raw["view_pos"][len(chunks[0])]) == -1


# ------------------------------------------------------------------------------------------ the entry points, raw
def _scores(pred_logits):
    return torch.softmax(pred_logits, dim=-1)[..., :-1].max(-1).values.contiguous()


def _taps(env, c):
    return env[1]._tap_tables(c.h, c.w, c.H, c.W, torch.device("cuda", torch.cuda.current_device()))


def _tables(ops, c, order):
    """ops.segment_tables on the case's views in `order`, columns padded to a multiple of 4 -> f_seg [V,Q,d4], logit_seg [V,Q,C]"""
    V, Q, D, d4 = len(order), c.Q, c.D, (c.D + 3) // 4 * 4
    tn = torch.nn.functional.normalize(_dev(c.text).float(), dim=-1)
    e4, t4 = torch.zeros((V * Q, d4), device="cuda"), torch.zeros((c.C, d4), device="cuda")
    e4[:, :D], t4[:, :D] = _dev(c.mask_embed[order]).reshape(V * Q, D), tn
    f_seg, l_seg = torch.empty((V, Q, d4), device="cuda"), torch.empty((V, Q, c.C), device="cuda")
    ops.segment_tables(e4, t4, float(c.scale), f_seg.view(V * Q, d4), l_seg.view(V * Q, -1))
    return f_seg, l_seg


def _raw(env, c, chunks, a, fill=True, spoil=None, words=None):
    """begin / (lists, sizes, add) per chunk / finish through the ops wrappers, every integer and fp32 array from the arena `a` (fenced or
    plain) and every workspace of exactly the reported bytes; spoil(k, kept): called after chunk k and after the last (k = None) with
    the dict of everything kept -> dict of the kept arrays and finish's outputs"""
    ops, sparse = env
    from geopurify_amd import _lib
    lib = _lib.load()
    N, Q, C, d4 = c.N, c.Q, c.C, (c.D + 3) // 4 * 4
    order = ms.concatenation(chunks)
    V = len(order)
    points = _dev(c.points)
    mx = 2 ** 63 - 1 if c.max_visible is None else c.max_visible
    st = ops.lift_masks_stream_begin(points, buffers={"state": a.out(lib.gp_lift_masks_stream_state_bytes(N), torch.uint8, name="state"),
                                                      "status": a.out(8, torch.int64, name="running status")},
                                     workspace=a.out(lib.gp_lift_masks_stream_begin_workspace_bytes(N), torch.uint8, name="begin workspace"))
    # the sizes of everything kept, from plain calls of the lists on every chunk
    per_chunk = []
    for ch in chunks:
        l0 = ops.lift_masks_batched_lists(points, _dev(c.view_entry[ch]), _dev(c.w2c[ch]), _dev(c.intr[ch]),
                                          None if c.depth is None else _dev(c.depth[ch]), (c.H, c.W), c.cut, c.tau, c.min_visible, mx)
        per_chunk.append((l0.total, int(l0.view_count[l0.view_keep.bool()].sum())))
    R = sum(k for _, k in per_chunk)
    f0, l0 = _tables(ops, c, order)
    kept = {"view_entry": a.inp(torch.from_numpy(c.view_entry[order]), name="view_entry"), "view_pos": a.out(V, torch.int32, name="view_pos"),
            "view_keep": a.out(V, torch.uint8, name="view_keep"), "view_count": a.out(V, torch.int64, name="view_count"),
            "rec_off": a.out(V + 1, torch.int64, name="rec_off"), "rec_row": a.out(max(R, 1), torch.int32, name="rec_row"),
            "rec_seg": a.out(max(R, 1), torch.int32, name="rec_seg"), "f_seg": a.inp(f0.cpu(), name="f_seg"), "logit_seg": a.inp(l0.cpu(), name="logit_seg"),
            "state": st.state, "running status": st.status}
    taps = tuple(a.inp(t.cpu(), name=f"tap{i}") for i, t in enumerate(_taps(env, c)))
    V0 = R0 = most = 0
    for k, (ch, (total, kept_k)) in enumerate(zip(chunks, per_chunk)):
        nv = len(ch)
        ve = kept["view_entry"][V0:V0 + nv]
        bufs = {"view_off": a.out(nv + 1, torch.int64, name=f"view_off {k}"), "view_count": kept["view_count"][V0:V0 + nv],
                "view_keep": kept["view_keep"][V0:V0 + nv], "status": a.out(8, torch.int64, name=f"lists status {k}")}
        if total:
            bufs.update(pt=a.out(total, torch.int64, name=f"pt {k}"), x=a.out(total, torch.int64, name=f"x {k}"),
                        y=a.out(total, torch.int64, name=f"y {k}"), view=a.out(total, torch.int32, name=f"view {k}"))
        found = {}

        def sizes(got):
            s = ops.lift_masks_stream_sizes(st, ve, got["view_count"], got["view_keep"], buffers={"sizes": a.out(4, torch.int64, name=f"sizes {k}")},
                                            workspace=a.out(lib.gp_lift_masks_stream_sizes_workspace_bytes(nv), torch.uint8, name=f"sizes workspace {k}"))
            found["sizes"] = s.tolist()
            return found["sizes"][0], found["sizes"][2]

        lists = ops.lift_masks_batched_lists(points, ve, _dev(c.w2c[ch]), _dev(c.intr[ch]), None if c.depth is None else _dev(c.depth[ch]),
                                             (c.H, c.W), c.cut, c.tau, c.min_visible, mx, buffers=bufs, sizes=sizes,
                                             workspace=a.out(lib.gp_lift_masks_batched_lists_workspace_bytes(N, nv), torch.uint8, name=f"lists workspace {k}"))
        assert found["sizes"][:2] == [total, kept_k] and found["sizes"][3] == 0 and lists.total == total
        most = found["sizes"][2]
        fill_cap = min(total, 300)
        ws = a.out(lib.gp_lift_masks_stream_add_workspace_bytes(N, nv, Q if total else 1, c.h if total else 1, c.w if total else 1, c.H, c.W, total,
                                                                fill_cap), torch.uint8, name=f"add workspace {k}")
        pm = a.inp(torch.from_numpy(c.pred_masks[ch]), name=f"pred_masks {k}") if total else None
        sc = a.inp(_scores(_dev(c.pred_logits[ch])).cpu(), name=f"scores {k}") if total else None
        ops.lift_masks_stream_add(st, ve, pm, sc, taps if total else None, (c.H, c.W), (lists.pt, lists.x, lists.y, lists.view), lists.view_off,
                                  lists.view_keep, total, kept["rec_row"] if total else None, kept["rec_seg"] if total else None, R0,
                                  kept["rec_off"][V0:V0 + nv + 1], kept["view_pos"][V0:V0 + nv], fill_cap=fill_cap, workspace=ws)
        V0, R0 = V0 + nv, R0 + kept_k
        if spoil is not None:
            spoil(k, kept)
    if spoil is not None:
        spoil(None, kept)
    words = max(1, -(-most // 64)) if words is None else words
    pitch = d4 + 4 if a.fence else d4
    out = {"out": a.out((N, d4), torch.float32, pitch=pitch, name="out"), "seen": a.out(N, torch.uint8, name="seen"),
           "count": a.out(N, torch.int32, name="count"), "status": a.out(8, torch.int64, name="status")}
    if fill:
        out["nn"] = a.out(N, torch.int64, name="nn")
    got = dict(kept)
    if R:
        r = ops.lift_masks_stream_finish(st, kept["view_entry"], kept["view_pos"], kept["view_keep"], kept["rec_off"], kept["rec_row"], kept["rec_seg"], R,
                                         words, kept["f_seg"], kept["logit_seg"], fill=fill, buffers=out,
                                         workspace=a.out(lib.gp_lift_masks_stream_finish_workspace_bytes(N, V, R, words), torch.uint8,
                                                         name="finish workspace"))
        got.update(out=r.out, seen=r.seen, count=r.count, status=r.status)
        if fill:
            got["nn"] = r.nn
    got["most"], got["records"] = most, R
    return got


@pytest.mark.parametrize("name,kind", [("views_130", "random"), ("views_64_65", "at_64"), ("Q65", "singles"), ("D65", "whole"), ("entries", "by_entry"),
                                       ("fill_257", "singles"), ("drop", "random")])
def test_the_entry_points_stay_inside_their_extents(env, name, kind):
    """The four entry points (and the lists between them) on fenced arrays: every fp32 and integer input, the state, the per-view arrays
    and the records, every output (the rows with a pitch of their own), the workspaces of exactly the reported bytes; the fp64 inputs
    have no fence type and stay plain.  Nothing outside the extents is written, nothing read from there reaches a result."""
    ops, sparse = env
    c = lm.case(name)
    chunks = ms.partition(c, kind)
    order = ms.concatenation(chunks)
    keys = ("view_pos", "view_keep", "view_count", "rec_off", "rec_row", "rec_seg", "out", "seen", "count", "nn", "status", "running status")

    def case(a):
        got = _raw(env, c, chunks, a)
        return {k: got[k] for k in keys}

    got = extent_fence.run(case)
    for k, v in got.items():
        assert extent_fence.unwritten(v) == 0, k
    ref = lm.reference(name) if np.array_equal(order, np.arange(c.V)) else ms.reference_of(c, order)
    assert np.array_equal(got["nn"].cpu().numpy(), ref.filled_from) and np.array_equal(got["count"].cpu().numpy(), ref.count)
    assert np.array_equal(got["view_count"].cpu().numpy(), ref.view_count) and got["status"].tolist()[6:] == [0, 0]
    assert got["status"].tolist()[4] == int(ref.seen.sum()) and got["status"].tolist()[5] == int((ref.filled_from >= 0).sum())
    # a view's position is its rank among the views of its entry in arrival order, its records are its visible points when it is kept
    ve = c.view_entry[order]
    pos = np.array([int((ve[:i] == ve[i]).sum()) for i in range(len(ve))])
    assert np.array_equal(got["view_pos"].cpu().numpy(), pos)
    off = np.concatenate([[0], np.cumsum(np.where(ref.view_keep, ref.view_count, 0))])
    assert np.array_equal(got["rec_off"].cpu().numpy(), off)
    rows = got["rec_row"].cpu().numpy()
    for i, v in enumerate(order):
        assert np.array_equal(rows[off[i]:off[i + 1]], ref.views[i][0] if ref.view_keep[i] else []), int(v)
    one = sparse.lift_masks(_dev(c.points), _views(sparse, c, order), _dev(c.text), c.scale, fill=False, **_options(c))
    assert torch.equal(_bits(got["out"][:, :c.D]), _bits(one.features))


def test_overlapping_arguments_are_refused(env):
    ops, _ = env
    from geopurify_amd._lib import GeoPurifyHipError
    c = lm.case("C19")
    chunks = ms.partition(c, "whole")
    got = _raw(env, c, chunks, extent_fence.Arena(False))
    st = ops.LiftMasksStreamState(_dev(c.points), got["state"], got["running status"])
    args = (got["view_entry"], got["view_pos"], got["view_keep"], got["rec_off"], got["rec_row"], got["rec_seg"], got["records"], 1, got["f_seg"],
            got["logit_seg"])
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        ops.lift_masks_stream_finish(st, *args, buffers={"seen": got["f_seg"].view(-1).view(torch.uint8)[:c.N]})
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        ops.lift_masks_stream_finish(st, *args, buffers={"status": got["running status"]})
    both = torch.zeros(16 * c.N, dtype=torch.uint8, device="cuda")
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        ops.lift_masks_stream_finish(st, *args, buffers={"seen": both[:c.N], "count": both[c.N // 4 * 4 - 4:c.N // 4 * 4 - 4 + 4 * c.N].view(torch.int32)})
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        ops.lift_masks_stream_begin(_dev(c.points), buffers={"state": both.new_zeros(1 << 20), "status": both[:64].view(torch.int64)},
                                    workspace=both)
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        ops.lift_masks_stream_sizes(st, got["view_entry"], got["view_count"], got["view_keep"], buffers={"sizes": got["view_count"][:4]})
    # add: the records inside the chunk's own entry arrays, and the positions inside the record offsets
    lists = ops.lift_masks_batched_lists(_dev(c.points), got["view_entry"], _dev(c.w2c), _dev(c.intr), None if c.depth is None else _dev(c.depth),
                                         (c.H, c.W), c.cut, c.tau, c.min_visible, 2 ** 63 - 1)
    fresh = ops.lift_masks_stream_begin(_dev(c.points))
    common = (got["view_entry"], _dev(c.pred_masks), _scores(_dev(c.pred_logits)), _taps(env, c), (c.H, c.W),
              (lists.pt, lists.x, lists.y, lists.view), lists.view_off, lists.view_keep, lists.total)
    rec = torch.zeros(got["records"], dtype=torch.int32, device="cuda")
    off, pos = torch.zeros(c.V + 1, dtype=torch.int64, device="cuda"), torch.zeros(c.V, dtype=torch.int32, device="cuda")
    assert lists.view.numel() >= got["records"]
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        ops.lift_masks_stream_add(fresh, *common, lists.view[:got["records"]], rec, 0, off, pos)
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        ops.lift_masks_stream_add(fresh, *common, rec, rec.clone(), 0, off, off.view(torch.int32)[:c.V])
    assert fresh.status.tolist()[4] == 0                                         # the refused calls advanced nothing
    ops.lift_masks_stream_add(fresh, *common, rec, rec.clone(), 0, off, pos)
    assert fresh.status.tolist()[4] == got["most"] and torch.equal(pos, got["view_pos"])


def test_a_foreign_state_and_foreign_records_take_no_kernel_outside_an_extent(env):
    """Everything the stream keeps is the caller's memory between the calls.  Under fences: after the first chunk the state is
    overwritten with 0xFF (counters -1, row numbers -1, offsets -1, keys 2^32 - 1), after the last the records, the record offsets and
    the positions get values outside their ranges.  add and finish stay inside the extents, and finish counts what it had to force
    into range or leave out."""
    ops, _ = env
    c = lm.case("entries")
    chunks = ms.partition(c, "by_entry")
    assert len(chunks) >= 3
    N, Q = c.N, c.Q

    def spoil(k, kept):
        if k == 0:
            kept["state"].fill_(0xFF)
        if k is None:
            R, V = kept["rec_row"].numel(), kept["view_pos"].numel()
            assert R >= 12 and V >= 6
            kept["rec_row"][0::7] = N                                            # no row
            kept["rec_row"][3::7] = -7
            kept["rec_row"][5::11] = 2 ** 31 - 1
            kept["rec_seg"][1::5] = Q                                            # no segment
            kept["rec_seg"][2::9] = -2 ** 31
            kept["view_pos"][1] = 70000                                          # beyond any word
            kept["view_pos"][2] = -3
            kept["rec_off"][1] = -5                                              # descending, beyond the records
            kept["rec_off"][3] = 2 ** 40
            kept["view_keep"][4] = 0xA5

    a = extent_fence.Arena(True)
    got = _raw(env, c, chunks, a, spoil=spoil)
    torch.cuda.synchronize()
    extent_fence.assert_intact(*a.fences)
    status = got["status"].tolist()
    print(f"status after the foreign state and records: {status}")
    assert status[6] >= 2 * N + 65538 and status[7] >= 1                         # (the entry tables alone: 2 N + 65538 values)
    assert got["running status"].tolist()[6] >= 1                                # add: the counters of the later chunks' entries were -1
    assert extent_fence.unwritten(got["out"]) == 0 and extent_fence.unwritten(got["count"]) == 0
    assert int(got["count"].max()) <= c.V and bool((got["nn"] == -1).all())      # (no entry table survived: nobody is filled)
    assert bool(torch.isfinite(got["out"]).all())


# ------------------------------------------------------------------------------------------ the chain
def test_chain_stream_quantize_purify_segment(env):
    """LiftMasksStream -> quantize -> purify(student) -> segment on two small entries gives the bits of the chain started from lift_masks"""
    ops, sparse = env
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import MinkowskiEngine as ME
    finally:
        sys.path.pop(0)
    from geopurify_amd import pipeline as pl
    from geopurify_amd.affinity_module import AffinityPredictor
    D, Cn = 64, 20
    c = lm.masks("chain", 26, {0: 400, 1: 500}, {0: 4, 1: 5}, Q=12, C=Cn, D=D)
    m = AffinityPredictor(D + 6, 128, 128)
    m.load_state_dict(pl.random_student_state_dict(D + 6, hidden=128, embed=128, num_blocks=4, seed=6))
    m = m.cuda()
    points = _dev(c.points)
    labels = torch.randint(0, Cn, (c.N,), generator=torch.Generator().manual_seed(3)).cuda()

    def chain(lifted):
        feats = torch.cat([lifted.features, points[:, 1:].float(), torch.ones((c.N, 3), device="cuda")], 1)
        q = sparse.quantize(points, feats, quantization_size=0.2)
        x = ME.SparseTensor(features=q.features, coordinates=q.coordinates)
        y = sparse.purify(m, x, feature_dim=D, K=24, num_iters=3)
        seg = sparse.segment(y, lifted.text_features, lifted.logit_scale, labels=labels, inverse_mapping=q.inverse_mapping)
        return y.F, seg.pred, seg.counts

    chunks = ms.partition(c, "random")
    assert len(chunks) >= 2
    streamed = _streamed(sparse, c, chunks)
    assert bool(streamed.seen.any()) and not bool(streamed.seen.all()) and bool(torch.isfinite(streamed.features).all())
    a, b = chain(streamed), chain(_one_call(sparse, c, np.arange(c.V), True))
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[1].shape == (c.N,) and int(a[2][:, 2].sum()) == c.N
