"""sparse.lift_labels and sparse.LiftLabelsStream on the GPU against the per-entry reference of tests/lift_labels_cases.py (the oracle's
mapping and drop rule, np.bincount, np.argmax, nn1_indices_bruteforce), against sparse.lift on the same geometry, and against the
one-hot workaround (lift of one-hot maps, times count).

Bounds: none.  Every output is an integer or a flag and every comparison is array_equal / torch.equal.
"""
import os
import sys

import numpy as np
import pytest
import torch

import extent_fence
import lift_labels_cases as ll

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("labels", "votes", "voted", "seen", "count", "view_count", "view_keep")
TORCH_OF = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}


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


def _depth(c, views=None):
    if c.depth is None or isinstance(c.depth, str):
        return c.depth
    return _dev(c.depth if views is None else c.depth[views])


def _views(sparse, c, views=None, labels=None, depth="case"):
    """the LabelViews of a case, or of its views `views` (a chunk)"""
    pick = (lambda a: a) if views is None else (lambda a: a[views])
    return sparse.LabelViews(_dev(pick(c.labels)) if labels is None else labels, _dev(pick(c.view_entry)), _dev(pick(c.w2c)), _dev(pick(c.intr)),
                             _depth(c, views) if isinstance(depth, str) and depth == "case" else depth)


def _options(c):
    return dict(ignore_labels=c.ignore, unlabeled=c.unlabeled, cut_bound=c.cut, vis_thres=c.tau, min_visible=c.min_visible,
                max_visible=c.max_visible)


def _call(env, c, points=None, views=None, **kw):
    ops, sparse = env
    return sparse.lift_labels(_dev(c.points) if points is None else points, _views(sparse, c) if views is None else views, c.C,
                              **{**_options(c), **kw})


def _stream(env, c, points=None):
    ops, sparse = env
    return sparse.LiftLabelsStream(_dev(c.points) if points is None else points, c.C, **_options(c))


def _assert_equal(got, ref, fill=True, what=""):
    """every output of a LiftedLabels against a Reference (or another LiftedLabels), exactly"""
    for k in OUTPUTS:
        a = getattr(got, k)
        b = getattr(ref, "labels_unfilled" if k == "labels" and not fill and hasattr(ref, "labels_unfilled") else k)
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        b = b.cpu().numpy() if torch.is_tensor(b) else b
        assert a.shape == b.shape and np.array_equal(a, b), f"{what} {k}"


# ------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", ll.CASES)
def test_lift_labels_matches_the_reference(env, name):
    c, ref = ll.case(name), ll.reference(name)
    if ref.out_of_range:
        with pytest.raises(ValueError, match=f"lift_labels: {ref.out_of_range} sampled labels are neither in 0..{c.C - 1} nor in ignore_labels"):
            _call(env, c)
        return
    got = _call(env, c)
    assert got.labels.dtype == torch.int64 and got.votes.dtype == torch.int32 and got.voted.dtype == torch.int32 and got.seen.dtype == torch.bool
    assert got.count.dtype == torch.int32 and got.view_count.dtype == torch.int64 and got.view_keep.dtype == torch.bool
    assert got.votes.shape == (c.N, c.C) and got.labels.shape == (c.N,)
    _assert_equal(got, ref, what=name)
    _assert_equal(_call(env, c, fill=False), ref, fill=False, what=f"{name} unfilled")


@pytest.mark.parametrize("name", ll.CASES)
def test_geometry_outputs_equal_lifts(env, name):
    """seen, count, view_count and view_keep are sparse.lift's on the same geometry (a one-channel dummy map)"""
    ops, sparse = env
    c = ll.case(name)
    lifted = sparse.lift(_dev(c.points), sparse.Views(torch.ones((c.V, 1, c.H, c.W), device="cuda"), _dev(c.view_entry), _dev(c.w2c), _dev(c.intr),
                                                      _depth(c)), cut_bound=c.cut, vis_thres=c.tau, min_visible=c.min_visible,
                         max_visible=c.max_visible, fill=False)
    ref = ll.reference(name)
    for k in ("seen", "count", "view_count", "view_keep"):
        assert np.array_equal(getattr(lifted, k).cpu().numpy(), getattr(ref, k)), k
    if not ref.out_of_range:
        got = _call(env, c, fill=False)
        for k in ("seen", "count", "view_count", "view_keep"):
            assert torch.equal(getattr(got, k), getattr(lifted, k)), k


CLEAN = ("clean", "pixels", "pixels_depth", "drop", "fill")       # the cases without ignored pixels


@pytest.mark.parametrize("name", CLEAN)
def test_votes_equal_the_one_hot_lift(env, name):
    """Without ignored pixels and without the fill, votes == round(lift(one-hot fp32 maps, "nearest").features * count): the
    workaround the vote replaces, through an independently tested kernel"""
    ops, sparse = env
    c = ll.case(name)
    assert not np.isin(c.labels, c.ignore).any() and int(c.labels.min()) >= 0 and int(c.labels.max()) < c.C
    one_hot = torch.nn.functional.one_hot(_dev(c.labels).long(), c.C).permute(0, 3, 1, 2).float().contiguous()
    lifted = sparse.lift(_dev(c.points), sparse.Views(one_hot, _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), _depth(c)), mode="nearest",
                         cut_bound=c.cut, vis_thres=c.tau, min_visible=c.min_visible, max_visible=c.max_visible, fill=False)
    got = _call(env, c, fill=False)
    want = torch.round(lifted.features * lifted.count.unsqueeze(1).float()).to(torch.int32)
    assert torch.equal(got.votes, want) and torch.equal(got.count, lifted.count)


# ------------------------------------------------------------------------------------------ invariances
@pytest.mark.parametrize("name", ["views_130_C200", "C1024", "entries", "twins", "fill"])
def test_row_order_and_a_second_call_do_not_change_a_point(env, name):
    c = ll.case(name)
    base, again = _call(env, c), _call(env, c)
    _assert_equal(again, base, what="second call")
    perm = torch.from_numpy(np.random.default_rng(5).permutation(c.N)).cuda()
    sh = _call(env, c, points=_dev(c.points)[perm])
    for k in ("votes", "voted", "seen", "count"):
        assert torch.equal(getattr(sh, k), getattr(base, k)[perm]), k
    assert torch.equal(sh.view_count, base.view_count) and torch.equal(sh.view_keep, base.view_keep)
    # the labels too, except where the fill's (d^2, row) tie now falls on another row
    unfilled = _call(env, c, points=_dev(c.points)[perm], fill=False)
    assert torch.equal(unfilled.labels, _call(env, c, fill=False).labels[perm])


def test_every_label_dtype_gives_the_same_result(env):
    base = _call(env, ll.case(ll.DTYPES[0]))
    for n in ll.DTYPES[1:]:
        c = ll.case(n)
        assert TORCH_OF[c.labels.dtype] == _dev(c.labels).dtype
        _assert_equal(_call(env, c), base, what=n)


# ------------------------------------------------------------------------------------------ extents
def _fenced_labels(a, c):
    """the label maps inside a fence: int16 has no poison of its own and travels as its bytes"""
    t = torch.from_numpy(c.labels)
    if t.dtype == torch.int16:
        return a.inp(t.view(torch.uint8).reshape(-1), name="labels").view(torch.int16).view(t.shape)
    return a.inp(t, name="labels")


@pytest.mark.parametrize("name", ["odd_u8", "dtype_int16", "dtype_int32", "dtype_int64", "views_130_C200", "C65", "fill"])
def test_the_one_call_entry_stays_inside_its_extents(env, name):
    """ops.lift_labels_batched on fenced arrays: the label maps (a uint8 map of odd byte length among them), the integer view table,
    every output (the votes rows with a pitch of their own) and a workspace of exactly the reported bytes; the fp64 inputs have no
    fence type and stay plain"""
    ops, _ = env
    c, ref = ll.case(name), ll.reference(name)
    N, V, C = c.N, c.V, c.C
    if name == "odd_u8":
        assert c.labels.dtype == np.uint8 and c.labels.size % 2 == 1

    def case(a):
        labels2d = _fenced_labels(a, c)
        ve = a.inp(torch.from_numpy(c.view_entry), name="view_entry")
        pitch = (C + 3) // 4 * 4 + 4 if a.fence else C
        bufs = {"labels": a.out(N, torch.int64, name="labels_out"), "votes": a.out((N, C), torch.int32, pitch=pitch, name="votes"),
                "voted": a.out(N, torch.int32, name="voted"), "seen": a.out(N, torch.uint8, name="seen"), "count": a.out(N, torch.int32, name="count"),
                "view_count": a.out(V, torch.int64, name="view_count"), "view_keep": a.out(V, torch.uint8, name="view_keep"),
                "status": a.out(8, torch.int64, name="status")}
        ws = a.out(ops.lift_labels_batched_workspace_bytes(N, V), torch.uint8, name="workspace")
        r = ops.lift_labels_batched(_dev(c.points), labels2d, C, ve, _dev(c.w2c), _dev(c.intr), _depth(c), c.cut, c.tau, c.min_visible,
                                    2 ** 63 - 1 if c.max_visible is None else c.max_visible, ignore_ids=c.ignore, unlabeled=c.unlabeled,
                                    buffers=bufs, workspace=ws)
        return {k: getattr(r, k) for k in OUTPUTS + ("status",)}

    got = extent_fence.run(case)
    for k in OUTPUTS + ("status",):
        assert extent_fence.unwritten(got[k]) == 0, k
    assert np.array_equal(got["labels"].cpu().numpy(), ref.labels) and np.array_equal(got["votes"].cpu().numpy(), ref.votes)
    status = got["status"].tolist()
    assert status[:3] == [0, 0, 0] and status[4] == int((ref.voted > 0).sum()) and status[5] == int((ref.filled_from >= 0).sum()) and status[7] == 0


@pytest.mark.parametrize("name", ["odd_u8", "dtype_int16", "views_130_C200"])
def test_the_stream_entries_stay_inside_their_extents(env, name):
    """ops.lift_labels_stream_begin / _add (two chunks) / _finish on fenced arrays, each workspace of exactly the reported bytes"""
    ops, _ = env
    c, ref = ll.case(name), ll.reference(name)
    N, C = c.N, c.C
    halves = [np.arange(0, c.V // 2 + 1), np.arange(c.V // 2 + 1, c.V)]

    def case(a):
        pitch = (C + 3) // 4 * 4 + 4 if a.fence else C
        st = ops.lift_labels_stream_begin(_dev(c.points), C, buffers={
            "state": a.out(ops.lift_labels_stream_state_bytes(N), torch.uint8, name="state"),
            "votes": a.out((N, C), torch.int32, pitch=pitch, name="votes"), "count": a.out(N, torch.int32, name="count"),
            "status": a.out(8, torch.int64, name="running")}, workspace=a.out(ops.lift_labels_stream_begin_workspace_bytes(N), torch.uint8, name="ws_begin"))
        outs = {}
        whole = _fenced_labels(a, c)
        for i, vs in enumerate(halves):
            lo, hi = int(vs[0]), int(vs[-1]) + 1
            vc, vk = ops.lift_labels_stream_add(st, whole[lo:hi], a.inp(torch.from_numpy(c.view_entry[vs]), name=f"view_entry{i}"), _dev(c.w2c[vs]),
                                                _dev(c.intr[vs]), _depth(c, vs), c.cut, c.tau, c.min_visible,
                                                2 ** 63 - 1 if c.max_visible is None else c.max_visible, ignore_ids=c.ignore,
                                                buffers={"view_count": a.out(len(vs), torch.int64, name=f"view_count{i}"),
                                                         "view_keep": a.out(len(vs), torch.uint8, name=f"view_keep{i}")},
                                                workspace=a.out(ops.lift_labels_stream_add_workspace_bytes(len(vs)), torch.uint8, name=f"ws_add{i}"))
            outs[f"view_count{i}"], outs[f"view_keep{i}"] = vc, vk
        r = ops.lift_labels_stream_finish(st, unlabeled=c.unlabeled, buffers={
            "labels": a.out(N, torch.int64, name="labels_out"), "voted": a.out(N, torch.int32, name="voted"), "seen": a.out(N, torch.uint8, name="seen"),
            "status": a.out(8, torch.int64, name="status")}, workspace=a.out(ops.lift_labels_stream_finish_workspace_bytes(N), torch.uint8, name="ws_finish"))
        outs.update(labels=r.labels, voted=r.voted, seen=r.seen, status=r.status, votes=st.votes, count=st.count)
        return outs

    got = extent_fence.run(case)
    for k, v in got.items():
        assert extent_fence.unwritten(v) == 0, k
    assert np.array_equal(got["labels"].cpu().numpy(), ref.labels) and np.array_equal(got["votes"].cpu().numpy(), ref.votes)
    assert np.array_equal(torch.cat([got["view_count0"], got["view_count1"]]).cpu().numpy(), ref.view_count)
    assert got["status"].tolist()[6:] == [0, 0]


def test_overlapping_arguments_are_refused(env):
    ops, _ = env
    from geopurify_amd._lib import GeoPurifyHipError
    c = ll.case("no_depth")
    args = lambda labels2d: (_dev(c.points), labels2d, c.C, _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), None, c.cut, c.tau, 0, 2 ** 63 - 1)  # noqa: E731
    both = torch.zeros(c.N + c.V, dtype=torch.uint8, device="cuda")
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        ops.lift_labels_batched(*args(_dev(c.labels)), buffers={"seen": both[:c.N], "view_keep": both[c.N - 1:c.N - 1 + c.V]})
    big = torch.zeros(max(c.N * 8, c.labels.size), dtype=torch.uint8, device="cuda")
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        ops.lift_labels_batched(*args(big[:c.labels.size].view(c.labels.shape)), buffers={"labels": big[:c.N * 8].view(torch.int64)})
    both32 = torch.zeros(2 * c.N, dtype=torch.int32, device="cuda")
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        ops.lift_labels_batched(*args(_dev(c.labels)), buffers={"voted": both32[:c.N], "count": both32[c.N - 1:2 * c.N - 1]})


# ------------------------------------------------------------------------------------------ the status errors
def test_status_errors_and_their_precedence(env):
    ops, sparse = env
    c, ref = ll.case("out_of_range_sampled"), ll.reference("out_of_range_sampled")
    P = _dev(c.points)
    label_message = f"{ref.out_of_range} sampled labels are neither in 0..{c.C - 1} nor in ignore_labels"
    with pytest.raises(ValueError, match=label_message):
        _call(env, c)
    # the three of lift come first, in lift's order
    v = _views(sparse, c)
    v.view_entry = v.view_entry.clone()
    v.view_entry[1] = 65536
    with pytest.raises(ValueError, match="1 views have a view_entry outside 0..65535"):
        _call(env, c, views=v)
    bad = P.clone()
    bad[7, 0] = -1.0
    with pytest.raises(ValueError, match="1 rows have a batch index"):
        _call(env, c, points=bad, views=v)
    bad[9, 2] = float("nan")
    with pytest.raises(ValueError, match="1 rows of points are not finite"):
        _call(env, c, points=bad, views=v)
    # the out-of-range samples cast no vote and change nothing else
    r = ops.lift_labels_batched(P, _dev(c.labels), c.C, _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), _depth(c), c.cut, c.tau, 0, 2 ** 63 - 1)
    assert r.status.tolist()[7] == ref.out_of_range and r.status.tolist()[:3] == [0, 0, 0]
    assert np.array_equal(r.votes.cpu().numpy(), ref.votes) and np.array_equal(r.labels.cpu().numpy(), ref.labels)
    # a stream keeps the count in its state: every finish reports it
    s = _stream(env, c)
    s.add(_views(sparse, c))
    for _ in range(2):
        with pytest.raises(ValueError, match=f"LiftLabelsStream.finish: {label_message}"):
            s.finish()


def _no_sync_but_readback(ops, run):
    """run() with every synchronising call forbidden but ops.readback -> the read-backs it made"""
    torch.cuda.synchronize()
    before = ops.READBACK["calls"]
    real = ops.readback
    torch.cuda.set_sync_debug_mode("error")
    try:
        def counted(t):
            torch.cuda.set_sync_debug_mode("default")
            try:
                return real(t)
            finally:
                torch.cuda.set_sync_debug_mode("error")
        ops.readback = counted
        run()
    finally:
        ops.readback = real
        torch.cuda.set_sync_debug_mode("default")
    return ops.READBACK["calls"] - before


def test_one_host_synchronisation(env):
    ops, sparse = env
    c = ll.case("views_130_C200")
    points, views, kw = _dev(c.points), _views(sparse, c), _options(c)
    assert _no_sync_but_readback(ops, lambda: sparse.lift_labels(points, views, c.C, **kw)) == 1
    r = ll.case("render")
    rp, rv = _dev(r.points), _views(sparse, r)
    assert _no_sync_but_readback(ops, lambda: sparse.lift_labels(rp, rv, r.C, **_options(r))) == 1
    chunks = [_views(sparse, c, np.arange(i, min(i + 50, c.V))) for i in range(0, c.V, 50)]
    stream = sparse.LiftLabelsStream(points, c.C, **kw)

    def adds():
        for ch in chunks:
            stream.add(ch)
    assert _no_sync_but_readback(ops, adds) == 0
    assert _no_sync_but_readback(ops, stream.finish) == 1


# ------------------------------------------------------------------------------------------ streams
def _chunks(c, bounds):
    return [np.arange(a, b) for a, b in zip(bounds[:-1], bounds[1:])]


def _run_stream(env, c, chunks, check_prefixes=False, dtypes=None):
    """the chunks (arrays of view indices) through a stream -> the final LiftedLabels"""
    ops, sparse = env
    s = _stream(env, c)
    done = []
    for i, vs in enumerate(chunks):
        labels = None if dtypes is None else _dev(c.labels[vs].astype(dtypes[i % len(dtypes)]))
        s.add(_views(sparse, c, vs, labels=labels))
        done.append(vs)
        if check_prefixes:
            so_far = np.concatenate(done)
            _assert_equal(s.finish(), _call(env, c, views=_views(sparse, c, so_far)), what=f"prefix of {i + 1} chunks")
    assert s.num_views == sum(len(vs) for vs in chunks)
    return s.finish()


@pytest.mark.parametrize("name", ["views_0_1_63", "twins", "render", "fill", "drop"])
def test_stream_of_single_views_and_every_prefix(env, name):
    """chunks of one view; finish after every chunk equals the one-call result on the views so far; the end equals the reference"""
    c, ref = ll.case(name), ll.reference(name)
    got = _run_stream(env, c, _chunks(c, list(range(c.V + 1))), check_prefixes=c.V <= 8)
    _assert_equal(got, ref, what=name)


@pytest.mark.parametrize("name", ["views_64_65_C2", "views_130_C200", "C1024", "entries", "no_depth"])
def test_stream_split_inside_an_entry_and_permuted(env, name):
    ops, sparse = env
    c, ref = ll.case(name), ll.reference(name)
    bounds = sorted({0, 1, c.V // 3, c.V // 2 + 1, c.V})
    chunks = _chunks(c, bounds)                             # view_entry is interleaved: every cut falls inside entries
    got = _run_stream(env, c, chunks, check_prefixes=True)
    _assert_equal(got, ref, what=name)
    order = np.random.default_rng(9).permutation(len(chunks))
    assert not np.array_equal(order, np.arange(len(chunks)))
    moved = _run_stream(env, c, [chunks[i] for i in order])
    arrival = np.concatenate([chunks[i] for i in order])
    for k in ("labels", "votes", "voted", "seen", "count"):
        assert torch.equal(getattr(moved, k), getattr(got, k)), k
    assert np.array_equal(moved.view_count.cpu().numpy(), ref.view_count[arrival]) and np.array_equal(moved.view_keep.cpu().numpy(), ref.view_keep[arrival])


def test_stream_of_mixed_dtypes_and_finish_twice(env):
    ops, sparse = env
    c, ref = ll.case("dtype_int16"), ll.reference("dtype_int16")
    chunks = _chunks(c, [0, 2, 3, 7, c.V])
    got = _run_stream(env, c, chunks, dtypes=(np.int16, np.int64, np.int32))
    _assert_equal(got, ref, what="mixed signed dtypes")
    u = ll.case("views_0_1_63")                              # labels < 20 and 255: every dtype holds them
    s = _stream(env, u)
    for i, vs in enumerate(_chunks(u, [0, 5, 6, 40, u.V])):
        s.add(_views(sparse, u, vs, labels=_dev(u.labels[vs].astype((np.uint8, np.int64, np.int16, np.int32)[i]))))
    first, second = s.finish(), s.finish()
    _assert_equal(first, ll.reference("views_0_1_63"), what="mixed dtypes")
    _assert_equal(second, first, what="finish twice")
    _assert_equal(s.finish(fill=False), ll.reference("views_0_1_63"), fill=False, what="unfilled after filled")
    assert first.votes.data_ptr() != second.votes.data_ptr()                    # snapshots: new tensors


def test_stream_refusals_leave_the_stream_as_it_was(env):
    ops, sparse = env
    c, ref = ll.case("twins"), ll.reference("twins")
    s = _stream(env, c)
    with pytest.raises(ValueError, match="no views were added"):
        s.finish()
    first, rest = np.arange(0, 2), np.arange(2, c.V)
    s.add(_views(sparse, c, first))
    before = (s._st.votes.clone(), s._st.count.clone(), s._st.status.clone(), s.num_views)
    refusals = [
        ("views must be a LabelViews", "a string"),
        (r"\(H, W\) of a chunk must be the first chunk's", _views(sparse, c, rest, labels=_dev(c.labels[rest][:, :-1]), depth=_dev(c.depth[rest][:, :-1]))),
        ("the presence of depth", _views(sparse, c, rest, depth=None)),
        ("the presence of depth", _views(sparse, c, rest, depth="render")),
        ("views.labels must be uint8, int16, int32 or int64", _views(sparse, c, rest, labels=_dev(c.labels[rest]).float())),
        ("views.depth must be fp64", _views(sparse, c, rest, depth=_dev(c.depth[rest]).float())),
        ("no CPU path", _views(sparse, c, rest, labels=torch.from_numpy(c.labels[rest]))),
    ]
    for match, chunk in refusals:
        with pytest.raises(ValueError, match=match):
            s.add(chunk)
    s.num_views = 65535 - len(rest) + 1
    with pytest.raises(ValueError, match="at most 65535 in all"):
        s.add(_views(sparse, c, rest))
    s.num_views = before[3]
    assert torch.equal(s._st.votes, before[0]) and torch.equal(s._st.count, before[1]) and torch.equal(s._st.status, before[2])
    assert len(s._view_count) == 1
    s.add(_views(sparse, c, rest))
    _assert_equal(s.finish(), ref, what="after the refusals")


def test_render_equals_the_call_given_the_rendered_tensor(env):
    ops, sparse = env
    c, ref = ll.case("render"), ll.reference("render")
    points = _dev(c.points)
    depth = sparse.render_depth(points, _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), (c.H, c.W), cut_bound=c.cut)
    given = _call(env, c, views=_views(sparse, c, depth=depth))
    _assert_equal(_call(env, c), given, what="one call")
    _assert_equal(given, ref, what="reference")
    s = _stream(env, c)
    for vs in _chunks(c, [0, 3, 4, c.V]):
        s.add(_views(sparse, c, vs))                          # depth="render" per chunk, from the stream's own tables
    _assert_equal(s.finish(), given, what="stream")


# ------------------------------------------------------------------------------------------ the chain
def test_chain_labels_feed_the_loss_and_votes_feed_the_pooling(env):
    """lift_labels -> segment_loss(labels=lifted.labels, ignore_labels=(255,)); quantize(points, votes.float()) -> affinity_pool"""
    ops, sparse = env
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import MinkowskiEngine as ME
    finally:
        sys.path.pop(0)
    D, Cn = 64, 20
    c = ll.generic("chain", 41, {0: 400, 1: 500}, {0: 4, 1: 5}, Cn)
    points = _dev(c.points)
    lifted = _call(env, c)
    assert bool((lifted.voted > 0).any()) and bool((lifted.labels == 255).any() | (lifted.voted == 0).any())
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(c.N, D, generator=g).cuda()
    q = sparse.quantize(points, feats, quantization_size=0.2)
    y = ME.SparseTensor(features=q.features.clone().requires_grad_(), coordinates=q.coordinates)
    text = torch.randn(Cn, D, generator=g).cuda()
    loss = sparse.segment_loss(y, text, 14.3, labels=lifted.labels, ignore_labels=(255,), inverse_mapping=q.inverse_mapping)
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0
    qv = sparse.quantize(points, lifted.votes.float(), quantization_size=0.2)
    x = ME.SparseTensor(features=qv.features, coordinates=qv.coordinates)
    pooled = sparse.affinity_pool(x, torch.randn(len(qv.coordinates), 16, generator=g).cuda(), K=24, num_iters=3)
    assert pooled.F.shape == (len(qv.coordinates), Cn) and bool(torch.isfinite(pooled.F).all())
