"""sparse.LiftStream on the GPU: the lift with the views arriving in chunks (csrc/lift_stream.hip) against sparse.lift on the
concatenation of the chunks -- bit for bit in all five fields -- and against the per-entry reference of tests/lift_batched_cases.py.
The partitions come from tests/lift_stream_cases.py, whose own claims tests/test_lift_stream_cases_host.py checks on the CPU.

Bounds.  Against sparse.lift: the same bits (features compared as int32), whatever the partition: the fp32 adds are the same in the
same order, a partial sum stored and reloaded between two chunks changes no bit, counts are integers, the division is one.  Against
the reference: the rule of tests/test_gpu_lift_batched.py -- masks, counts and the fill's choice exact, "nearest" features the same
bits, "bilinear" features within its BILINEAR_TOL (1e-6, imported) on maps in [-1, 1].
"""
import numpy as np
import pytest
import torch

import extent_fence
import lift_batched_cases as lb
import lift_stream_cases as ls
from test_gpu_lift_batched import BILINEAR_TOL

pytestmark = pytest.mark.gpu

FIELDS = ("features", "seen", "count", "view_count", "view_keep")


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


def _views(sparse, c, idx=None, layout="nchw", dtype=None):
    """the views idx of the case (all of them: None) as a Views"""
    idx = np.arange(c.V) if idx is None else np.asarray(idx, np.int64)
    maps = _dev(c.maps[idx], dtype)
    if layout == "channels_last":
        maps = maps.contiguous(memory_format=torch.channels_last)
    return sparse.Views(maps, _dev(c.view_entry[idx]), _dev(c.w2c[idx]), _dev(c.intr[idx]), None if c.depth is None else _dev(c.depth[idx]),
                        None if (c.H, c.W) == (c.h, c.w) else (c.H, c.W))


def _options(c):
    return dict(mode=c.mode, cut_bound=c.cut, vis_thres=c.tau, min_visible=c.min_visible, max_visible=c.max_visible)


def _stream(sparse, c, points=None, D=None):
    return sparse.LiftStream(_dev(c.points) if points is None else points, feature_dim=c.D if D is None else D, **_options(c))


def _streamed(sparse, c, chunks, fill=True, **kw):
    s = _stream(sparse, c)
    for ch in chunks:
        s.add(_views(sparse, c, ch, **kw))
    return s.finish(fill=fill)


_ONE_CALL = {}


def _one_call(sparse, c, order, fill):
    """sparse.lift on the case's views in `order`: computed once per (case, order, fill) and shared"""
    key = (c.name, np.asarray(order, np.int64).tobytes(), fill)
    if key not in _ONE_CALL:
        _ONE_CALL[key] = sparse.lift(_dev(c.points), _views(sparse, c, order), fill=fill, **_options(c))
    return _ONE_CALL[key]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(got, want, what=""):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        if not torch.equal(_bits(a), _bits(b)):
            at = (_bits(a) != _bits(b)).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {f} differs from the one-call lift, first at {at} ({int((_bits(a) != _bits(b)).sum())} elements)")


def _assert_reference(c, ref, got):
    """the rule of tests/test_gpu_lift_batched.py::test_lift_matches_the_reference"""
    assert np.array_equal(got.seen.cpu().numpy(), ref.seen) and np.array_equal(got.count.cpu().numpy(), ref.count)
    assert np.array_equal(got.view_count.cpu().numpy(), ref.view_count) and np.array_equal(got.view_keep.cpu().numpy(), ref.view_keep)
    f = got.features.cpu().numpy()
    if c.mode == "nearest":
        assert np.array_equal(f.view(np.int32), ref.features.view(np.int32))
    else:
        err = float(np.abs(f.astype(np.float64) - ref.features.astype(np.float64)).max())
        print(f"{c.name}: max |features - oracle| = {err:.3e}")
        assert np.abs(c.maps).max() <= 1.0 and err <= BILINEAR_TOL


# ------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize("kind", ls.EVERY_CASE)
@pytest.mark.parametrize("name", lb.CASES)
def test_bit_equal_to_the_one_call_lift(env, name, kind):
    _, sparse = env
    c = lb.case(name)
    chunks = ls.partition(c, kind)
    order = ls.concatenation(chunks)
    for fill in (True, False):
        _assert_same(_streamed(sparse, c, chunks, fill), _one_call(sparse, c, order, fill), f"{name} / {kind} / fill={fill}")


@pytest.mark.parametrize("kind", tuple(ls.BOUNDARIES) + ("by_entry",))
@pytest.mark.parametrize("name", ls.BOUNDARY_CASES)
def test_bit_equal_at_the_lane_group_boundaries_and_by_entry(env, name, kind):
    _, sparse = env
    c = lb.case(name)
    chunks = ls.partition(c, kind)
    order = ls.concatenation(chunks)                                             # (by_entry: the reordered concatenation)
    for fill in (True, False):
        _assert_same(_streamed(sparse, c, chunks, fill), _one_call(sparse, c, order, fill), f"{name} / {kind} / fill={fill}")
    if kind == "by_entry":
        _assert_reference(c, ls.reference_of(c, order), _streamed(sparse, c, chunks))


def test_idle_chunks_change_nothing(env):
    """a chunk of dropped views only, then a chunk of views whose entry has no points: finish before and after gives the same bits"""
    _, sparse = env
    c = ls.idle_case()
    rest, dropped, pointless = ls.idle_partition()
    s = _stream(sparse, c)
    s.add(_views(sparse, c, rest))
    before = s.finish()
    ref_all = ls.reference_of(c, np.arange(c.V))
    seen_views = len(rest)
    for idle in (dropped, pointless):
        s.add(_views(sparse, c, idle))
        after = s.finish()
        for f in ("features", "seen", "count"):
            assert torch.equal(_bits(getattr(after, f)), _bits(getattr(before, f))), f
        assert torch.equal(after.view_count[:seen_views], before.view_count[:seen_views])
        assert np.array_equal(after.view_count[seen_views:].cpu().numpy(), ref_all.view_count[idle])      # the reference's counts ...
        assert not bool(after.view_keep[seen_views:].any())                                               # ... and none is kept
        before, seen_views = after, seen_views + len(idle)
    order = ls.concatenation([rest, dropped, pointless])
    for fill in (True, False):
        _assert_same(_streamed(sparse, c, [rest, dropped, pointless], fill), _one_call(sparse, c, order, fill), f"idle / fill={fill}")
    _assert_reference(c, ls.reference_of(c, order), before)


# ------------------------------------------------------------------------------------------ against the reference
def _raw(env, c, chunks, fill=True, begin_buffers=None, add_buffers=None, finish_buffers=None, workspaces=None, maps_pm=None, view_entry=None,
         points=None):
    """the three ops on a case: -> (LiftStreamState, [(view_count, view_keep) per chunk], LiftStreamFinish)"""
    ops, _ = env
    workspaces = workspaces or {}
    st = ops.lift_stream_begin(_dev(c.points) if points is None else points, c.D, buffers=begin_buffers, workspace=workspaces.get("begin"))
    per_chunk = []
    for i, ch in enumerate(chunks):
        pm = ops.lift_batched_transpose(_dev(c.maps[ch])) if maps_pm is None else maps_pm[i]
        ve = _dev(c.view_entry[ch]) if view_entry is None else view_entry[i]
        ws = workspaces.get("add")
        per_chunk.append(ops.lift_stream_add(st, pm, (c.h, c.w), ve, _dev(c.w2c[ch]), _dev(c.intr[ch]),
                                             None if c.depth is None else _dev(c.depth[ch]), (c.H, c.W), c.mode == "bilinear", c.cut, c.tau,
                                             c.min_visible, 2 ** 63 - 1 if c.max_visible is None else c.max_visible,
                                             buffers=None if add_buffers is None else add_buffers[i], workspace=None if ws is None else ws[i]))
    return st, per_chunk, ops.lift_stream_finish(st, fill=fill, buffers=finish_buffers, workspace=workspaces.get("finish"))


@pytest.mark.parametrize("name", lb.CASES)
def test_stream_matches_the_reference(env, name):
    _, sparse = env
    c, ref = lb.case(name), lb.reference(name)
    chunks = ls.partition(c, "random")
    got = _streamed(sparse, c, chunks)
    assert got.features.dtype == torch.float32 and got.features.shape == (c.N, c.D) and not got.features.requires_grad
    assert got.seen.dtype == torch.bool and got.count.dtype == torch.int32 and got.view_count.dtype == torch.int64 and got.view_keep.dtype == torch.bool
    _assert_reference(c, ref, got)
    st, per_chunk, fin = _raw(env, c, chunks)
    assert np.array_equal(fin.nn.cpu().numpy(), ref.filled_from)                 # the fill's choice
    status = fin.status.tolist()
    assert status[:3] == [0, 0, 0] and status[3] == int(c.entries().max()) and status[4] == int(ref.seen.sum())
    assert status[5] == int((ref.filled_from >= 0).sum()) and status[6:] == [0, 0]
    assert np.array_equal(st.count.cpu().numpy(), ref.count)
    assert np.array_equal(torch.cat([vc for vc, _ in per_chunk]).cpu().numpy(), ref.view_count)
    # without the fill an unseen row is zero and a seen row is the filled call's
    plain = _streamed(sparse, c, chunks, fill=False)
    seen = got.seen
    assert torch.equal(_bits(plain.features[seen]), _bits(got.features[seen])) and not bool(plain.features[~seen].any())


# ------------------------------------------------------------------------------------------ snapshots
@pytest.mark.parametrize("name", ["views_130", "views_130_bilinear", "twins", "drop", "fill"])
def test_finish_is_a_snapshot(env, name):
    _, sparse = env
    c = lb.case(name)
    chunks = ls.partition(c, "random")
    s = _stream(sparse, c)
    for k, ch in enumerate(chunks):
        s.add(_views(sparse, c, ch))
        prefix = ls.concatenation(chunks[:k + 1])
        got = s.finish()
        _assert_same(got, _one_call(sparse, c, prefix, True), f"{name} after {k + 1} chunks")
        if c.V <= 8:
            _assert_reference(c, ls.reference_of(c, prefix), got)                # (the small cases: the CPU reference of every prefix)
    again = s.finish()
    _assert_same(again, got, "the last finish, twice")
    assert again.features.data_ptr() != got.features.data_ptr() and again.count.data_ptr() != got.count.data_ptr()   # new tensors
    _assert_same(s.finish(fill=False), _one_call(sparse, c, np.arange(c.V), False), "fill=False after fill=True")


# ------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("name", ["views_130_bilinear", "D_chunk_plus_1", "bilinear_ratio", "twins"])
def test_layouts_and_dtypes_may_alternate_inside_one_stream(env, name):
    _, sparse = env
    c = lb.case(name)
    chunks = ls.partition(c, "random")
    base = _streamed(sparse, c, chunks)
    s = _stream(sparse, c)
    for i, ch in enumerate(chunks):
        s.add(_views(sparse, c, ch, layout="channels_last" if i % 2 else "nchw", dtype=torch.float64 if i % 3 == 1 else None))
    _assert_same(s.finish(), base, "alternating layouts")
    assert len(chunks) >= 2
    s = _stream(sparse, c)
    for i, ch in enumerate(chunks):
        s.add(_views(sparse, c, ch, dtype=torch.float64 if i % 2 == 0 else None))   # (NCHW fp64: upcast, then the scratch)
    _assert_same(s.finish(), base, "fp64 chunks")
    _assert_same(_streamed(sparse, c, chunks, layout="channels_last"), base, "channels_last")
    # the NCHW scratch grows only when a chunk is larger than every one before it
    s = _stream(sparse, c)
    sizes, ptrs = [], []
    for ch in chunks:
        s.add(_views(sparse, c, ch))
        sizes.append(s._scratch.numel())
        ptrs.append(s._scratch.data_ptr())
    per_view = c.D * c.h * c.w
    assert sizes == [per_view * max(len(ch) for ch in chunks[:i + 1]) for i in range(len(chunks))]
    assert all(ptrs[i] == ptrs[i - 1] for i in range(1, len(chunks)) if sizes[i] == sizes[i - 1])


# ------------------------------------------------------------------------------------------ memory
def test_memory_does_not_grow_with_the_views_added(env):
    """Eight equal chunks of views_130: the peak of the second add and the peak of the last differ by the per-view count and keep vectors
    alone (9 bytes per view in 512-byte granules) -- at most 64 KiB, a cap against any per-view [N, .] or map-sized growth."""
    _, sparse = env
    c = lb.case("views_130")
    chunks = ls.equal_chunks(c, 8)
    views = [_views(sparse, c, ch) for ch in chunks]
    s = _stream(sparse, c)
    peaks = {}
    for i, v in enumerate(views):
        if i in (1, len(views) - 1):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
        s.add(v)
        if i in (1, len(views) - 1):
            torch.cuda.synchronize()
            peaks[i] = torch.cuda.max_memory_allocated()
    print(f"peak of add 2: {peaks[1]} B, of add {len(views)}: {peaks[len(views) - 1]} B")
    assert abs(peaks[len(views) - 1] - peaks[1]) <= 64 * 1024
    _assert_same(s.finish(), _one_call(sparse, c, ls.concatenation(chunks), True), "eight equal chunks")


# ------------------------------------------------------------------------------------------ extents
@pytest.mark.parametrize("name", ["views_130", "D65", "D_chunk_plus_1_bilinear", "entries", "fill", "drop"])
def test_the_entry_points_stay_inside_their_extents(env, name):
    """ops.lift_stream_begin / _add / _finish on fenced arrays: the fp32 maps and the integer view table of every chunk, the state, the
    sums and the rows with pitches of their own, every other output, and workspaces of exactly the reported bytes; the fp64 inputs have
    no fence type and stay plain.  Nothing outside the extents is written, nothing read from there reaches a result."""
    ops, _ = env
    from geopurify_amd import _lib
    lib = _lib.load()
    c, ref = lb.case(name), lb.reference(name)
    N, D = c.N, c.D
    chunks = ls.partition(c, "random")

    def case(a):
        pitch = (D + 3) // 4 * 4 + 4 if a.fence else D
        begin = {"state": a.out(lib.gp_lift_stream_state_bytes(N), torch.uint8, name="state"),
                 "sums": a.out((N, D), torch.float32, pitch=pitch, name="sums"), "count": a.out(N, torch.int32, name="count"),
                 "status": a.out(8, torch.int64, name="running status")}
        maps_pm = [a.inp(torch.from_numpy(np.ascontiguousarray(c.maps[ch].reshape(len(ch), D, -1).transpose(0, 2, 1))), name=f"maps {i}")
                   for i, ch in enumerate(chunks)]
        ve = [a.inp(torch.from_numpy(c.view_entry[ch]), name=f"view_entry {i}") for i, ch in enumerate(chunks)]
        add = [{"view_count": a.out(len(ch), torch.int64, name=f"view_count {i}"), "view_keep": a.out(len(ch), torch.uint8, name=f"view_keep {i}")}
               for i, ch in enumerate(chunks)]
        finish = {"out": a.out((N, D), torch.float32, pitch=pitch + (4 if a.fence else 0), name="out"), "seen": a.out(N, torch.uint8, name="seen"),
                  "nn": a.out(N, torch.int64, name="nn"), "status": a.out(8, torch.int64, name="status")}
        ws = {"begin": a.out(lib.gp_lift_stream_begin_workspace_bytes(N), torch.uint8, name="begin workspace"),
              "add": [a.out(lib.gp_lift_stream_add_workspace_bytes(len(ch)), torch.uint8, name=f"add workspace {i}") for i, ch in enumerate(chunks)],
              "finish": a.out(lib.gp_lift_stream_finish_workspace_bytes(N), torch.uint8, name="finish workspace")}
        st, per_chunk, fin = _raw(env, c, chunks, begin_buffers=begin, add_buffers=add, finish_buffers=finish, workspaces=ws, maps_pm=maps_pm,
                                  view_entry=ve)
        return {"sums": st.sums, "count": st.count, "running status": st.status, "out": fin.out, "seen": fin.seen, "nn": fin.nn,
                "status": fin.status, "view_count": torch.cat([vc for vc, _ in per_chunk]), "view_keep": torch.cat([vk for _, vk in per_chunk])}

    got = extent_fence.run(case)
    for k in got:
        assert extent_fence.unwritten(got[k]) == 0, k
    assert np.array_equal(got["nn"].cpu().numpy(), ref.filled_from) and np.array_equal(got["count"].cpu().numpy(), ref.count)
    assert np.array_equal(got["view_count"].cpu().numpy(), ref.view_count) and got["status"].tolist()[6] == 0
    one = env[1].lift(_dev(c.points), _views(env[1], c), fill=False, **_options(c))
    assert torch.equal(_bits(got["out"]), _bits(one.features))


def test_overlapping_arguments_are_refused(env):
    ops, _ = env
    from geopurify_amd._lib import GeoPurifyHipError
    c = lb.case("no_depth")
    chunks = ls.partition(c, "whole")
    both = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    assert both.numel() >= ops.lift_stream_add_workspace_bytes(c.V) and c.N % 8
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        _raw(env, c, chunks, add_buffers=[{"view_keep": both[:c.V]}], workspaces={"add": [both]})
    st, _, _ = _raw(env, c, chunks)
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        ops.lift_stream_finish(st, buffers={"out": st.sums})
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        ops.lift_stream_finish(st, buffers={"seen": both[:c.N], "status": both[c.N // 8 * 8:c.N // 8 * 8 + 64].view(torch.int64)})
    # the sums lie inside the chunk's maps
    maps_pm = ops.lift_batched_transpose(_dev(c.maps))
    assert maps_pm.numel() >= c.N * c.D
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        _raw(env, c, chunks, begin_buffers={"sums": maps_pm.view(-1)[:c.N * c.D].view(c.N, c.D)}, maps_pm=[maps_pm])
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        ops.lift_stream_begin(_dev(c.points), c.D, buffers={"count": both[:4 * c.N].view(torch.int32), "state": both})


# ------------------------------------------------------------------------------------------ the status errors
def test_status_errors(env):
    ops, sparse = env
    c = lb.case("no_depth")
    chunks = ls.partition(c, "by_entry")
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
    # precedence: non-finite rows, then bad batch rows, then bad views
    bad = P.clone()
    bad[7, 0], bad[8, 1] = 70000.0, float("nan")
    v = _views(sparse, c, chunks[1])
    v.view_entry = v.view_entry.clone()
    v.view_entry[0] = -1
    with pytest.raises(ValueError, match="1 rows of points are not finite"):
        run(points=bad, second=v).finish()
    # the rows and views that are counted belong to no entry: the others' results do not change
    order = ls.concatenation(chunks)
    _, _, ref = _raw(env, c, chunks)
    bad = c.points.copy()
    bad[7, 0] = 70000.0
    ve = [c.view_entry[ch].copy() for ch in chunks]
    gone = int(chunks[1][0])
    assert c.view_entry[gone] == 1
    ve[1][0] = -5
    st, per_chunk, r = _raw(env, c, chunks, points=_dev(bad), view_entry=[_dev(x) for x in ve])
    assert r.status.tolist()[:3] == [1, 1, 0] and int(st.count[7]) == 0 and int(r.nn[7]) == -1 and not bool(r.out[7].any())
    assert int(per_chunk[1][0][0]) == 0 and not bool(per_chunk[1][1][0])
    rows0 = _dev(np.setdiff1d(c.rows_of(0), [7]))
    one = ops.lift_batched(_dev(c.points), ops.lift_batched_transpose(_dev(c.maps[order])), (c.h, c.w), _dev(c.view_entry[order]), _dev(c.w2c[order]),
                           _dev(c.intr[order]), None, (c.H, c.W), False, c.cut, c.tau, 0, 2 ** 63 - 1)
    assert torch.equal(_bits(ref.out), _bits(one.out))
    assert torch.equal(st.count[rows0], one.count[rows0]) and torch.equal(_bits(r.out[rows0]), _bits(one.out[rows0]))


def test_a_foreign_state_takes_no_kernel_outside_an_extent(env):
    """A state that begin did not write (every byte 0xFF: row numbers -1, offsets -1, keys 2^32 - 1) under fences: add and finish stay
    inside the extents, nobody is counted, and finish reports what it had to force into range."""
    ops, _ = env
    from geopurify_amd import _lib
    lib = _lib.load()
    c = lb.case("entries")
    chunks = ls.partition(c, "whole")
    N, D = c.N, c.D
    a = extent_fence.Arena(True)
    good = ops.lift_stream_begin(_dev(c.points), D)
    state = a.out(lib.gp_lift_stream_state_bytes(N), torch.uint8, name="state")
    state.fill_(0xFF)
    st = ops.LiftStreamState(good.points, state, a.out((N, D), torch.float32, pitch=(D + 3) // 4 * 4 + 4, name="sums"),
                             a.out(N, torch.int32, name="count"), a.out(8, torch.int64, name="running status"))
    st.sums.zero_(), st.count.zero_(), st.status.zero_()
    vc, vk = ops.lift_stream_add(st, ops.lift_batched_transpose(_dev(c.maps)), (c.h, c.w), _dev(c.view_entry), _dev(c.w2c), _dev(c.intr),
                                 _dev(c.depth), (c.H, c.W), False, c.cut, c.tau, 0, 2 ** 63 - 1,
                                 workspace=a.out(lib.gp_lift_stream_add_workspace_bytes(c.V), torch.uint8, name="add workspace"))
    fin = ops.lift_stream_finish(st, buffers={"out": a.out((N, D), torch.float32, pitch=(D + 3) // 4 * 4 + 8, name="out"),
                                              "seen": a.out(N, torch.uint8, name="seen"), "nn": a.out(N, torch.int64, name="nn"),
                                              "status": a.out(8, torch.int64, name="status")},
                                 workspace=a.out(lib.gp_lift_stream_finish_workspace_bytes(N), torch.uint8, name="finish workspace"))
    torch.cuda.synchronize()
    extent_fence.assert_intact(*a.fences)
    assert not bool(vc.any()) and not bool(vk.any()) and not bool(st.count.any()) and not bool(fin.seen.any())
    assert fin.status.tolist()[6] == 2 * N + 65538 and bool((fin.nn == -1).all())


# ------------------------------------------------------------------------------------------ refusals before any kernel
def test_refusals_before_any_kernel(env):
    ops, sparse = env
    c = lb.case("twins")
    chunks = ls.partition(c, "by_entry")
    P = _dev(c.points)
    with pytest.raises(ValueError, match="mode='cubic'"):
        sparse.LiftStream(P, feature_dim=c.D, mode="cubic")
    with pytest.raises(ValueError, match="CUDA tensors"):
        sparse.LiftStream(P.cpu(), feature_dim=c.D)
    with pytest.raises(ValueError, match=r"points must be \[N, 4\]"):
        sparse.LiftStream(P[:, :3], feature_dim=c.D)
    with pytest.raises(ValueError, match="feature_dim"):
        sparse.LiftStream(P, feature_dim=0)
    s = _stream(sparse, c)
    with pytest.raises(ValueError, match="no views were added"):
        s.finish()
    s.add(_views(sparse, c, chunks[0]))
    want = s.finish()
    launches = {"n": 0}
    real = (ops.lift_stream_add, ops.lift_batched_transpose)

    def counted(f):
        def g(*a, **k):
            launches["n"] += 1
            return f(*a, **k)
        return g

    def refused(views, match):
        ops.lift_stream_add, ops.lift_batched_transpose = counted(real[0]), counted(real[1])
        try:
            with pytest.raises(ValueError, match=match):
                s.add(views)
        finally:
            ops.lift_stream_add, ops.lift_batched_transpose = real
        assert launches["n"] == 0                                                # no op of the call ran
        _assert_same(s.finish(), want, f"after the refusal '{match}'")           # ... and the stream is as it was

    ch = chunks[1]
    good = lambda: _views(sparse, c, ch)                                         # noqa: E731
    v = good()
    v.features = torch.cat([v.features, v.features[:, :1]], 1)
    refused(v, f"{c.D + 1} channels")
    v = good()
    v.features, v.image_shape = v.features[:, :, :-1].contiguous(), (c.H, c.W)
    refused(v, "mode 'nearest' samples")                                         # (lift's own refusal comes first in this mode)
    v = good()
    v.depth = None
    refused(v, "the presence of depth")
    v = good()
    v.features = v.features.clone().requires_grad_(True)
    refused(v, "require grad")
    v = good()
    v.features = v.features.cpu()
    refused(v, "CUDA tensors")
    v = good()
    v.world_to_camera = v.world_to_camera.float()
    refused(v, "world_to_camera must be fp64")
    refused("views", "must be a Views")
    s.add(good())
    _assert_same(s.finish(), _one_call(sparse, c, ls.concatenation(chunks), True), "after the refusals")

    # another (h, w) and another image_shape: the bilinear form, where lift itself takes both
    cb = lb.case("views_130_bilinear")
    first = np.arange(3)
    sb = _stream(sparse, cb)
    sb.add(_views(sparse, cb, first))
    want = sb.finish()
    s = sb
    v = _views(sparse, cb, first)
    v.features = v.features[:, :, :-1].contiguous()
    refused(v, r"\(h, w\) of a chunk")
    v = _views(sparse, cb, first)
    v.image_shape, v.depth = (cb.H - 1, cb.W), v.depth[:, :-1].contiguous()
    refused(v, "image_shape of a chunk")
    # depth absent, then present
    cn = lb.case("no_depth")
    s = _stream(sparse, cn)
    s.add(_views(sparse, cn, [0, 1]))
    want = s.finish()
    v = _views(sparse, cn, [2])
    v.depth = torch.ones((1, cn.H, cn.W), dtype=torch.float64, device="cuda")
    refused(v, "the presence of depth")


def test_the_65536th_view_is_refused(env):
    _, sparse = env
    V = 65535
    P = _dev(np.array([[0, 0.0, 0.0, 1.0], [0, 0.0, 0.0, 2.0], [1, 0.0, 0.0, 1.0], [1, 0.0, 0.0, -1.0]]))
    g = torch.Generator().manual_seed(7)
    maps = torch.rand((V, 1, 1, 1), generator=g).cuda()
    ve = (torch.arange(V) % 2).cuda()
    M = torch.eye(4, dtype=torch.float64).repeat(V, 1, 1).cuda()
    K = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float64).repeat(V, 1).cuda()
    s = sparse.LiftStream(P, feature_dim=1)
    s.add(sparse.Views(maps, ve, M, K))
    want = s.finish()
    assert want.count.tolist() == [32768, 32768, 32767, 0] and s.num_views == V
    _assert_same(want, sparse.lift(P, sparse.Views(maps, ve, M, K)), "65535 views")
    with pytest.raises(ValueError, match="at most 65535 in all"):
        s.add(sparse.Views(maps[:1], ve[:1], M[:1], K[:1]))
    _assert_same(s.finish(), want, "after the refused 65536th view")


# ------------------------------------------------------------------------------------------ host synchronisations
def test_add_never_synchronises_and_finish_does_once(env):
    ops, sparse = env
    c = lb.case("views_130_bilinear")
    chunks = ls.partition(c, "random")
    views = [_views(sparse, c, ch, layout="channels_last" if i % 2 else "nchw") for i, ch in enumerate(chunks)]
    points = _dev(c.points)
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
        s = sparse.LiftStream(points, feature_dim=c.D, **_options(c))
        for v in views:
            s.add(v)
        assert ops.READBACK["calls"] == before                                   # construction and every add: none
        got = s.finish()
        assert ops.READBACK["calls"] == before + 1                               # finish: exactly one
        s.add(views[0])
        assert ops.READBACK["calls"] == before + 1
    finally:
        ops.readback = real
        torch.cuda.set_sync_debug_mode("default")
    _assert_same(got, _one_call(sparse, c, np.arange(c.V), True), "under the sync debug mode")
