"""Rendered depth over batched point clouds on the GPU (csrc/render_depth_batched.hip): sparse.render_depth, ops.render_depth_batched and
ops.render_depth_stream against the per-view reference of tests/render_depth_cases.py and against the per-scene kernel, and
depth="render" in sparse.lift, LiftStream, lift_masks and LiftMasksStream against the same calls given the rendered depth as a tensor.

Bounds.  The images: the same bits as the reference (np.array_equal on fp64) -- the minimum of a set of doubles has one value, the
kernel's decision is the per-scene kernel's arithmetic, and the cases keep p_z free of rounding choices (see render_depth_cases).
"render" against the tensor: the same bits in every returned field, since the lift kernels then read the same depth values.  Against
the reference of tests/lift_batched_cases.py on a Case whose depth is the reference's rendered depth: that file's bounds, exact for
"nearest" and 1e-6 for "bilinear" (tests/test_gpu_lift_batched.py).
"""
import contextlib
import inspect

import numpy as np
import pytest
import torch

import extent_fence
import lift_batched_cases as lb
import lift_masks_batched_cases as lm
import render_depth_cases as rd
from test_gpu_lift_batched import BILINEAR_TOL

pytestmark = pytest.mark.gpu

LIFT_FIELDS = ("features", "seen", "count", "view_count", "view_keep")
MASK_FIELDS = LIFT_FIELDS + ("text_features",)


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


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else (t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t)


def _assert_same(got, want, fields, what=""):
    for f in fields:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        if not torch.equal(_bits(a), _bits(b)):
            at = (_bits(a) != _bits(b)).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {f} differs, first at {at} ({int((_bits(a) != _bits(b)).sum())} elements)")


def _geometry(c, idx=None):
    idx = np.arange(c.V) if idx is None else np.asarray(idx, np.int64)
    return _dev(c.view_entry[idx]), _dev(c.w2c[idx]), _dev(c.intr[idx])


def _per_scene(ops, c):
    """what a caller does without the batched call: ops.render_depth per view on the entry's slice of the points"""
    out = torch.full((c.V, c.H, c.W), rd.FAR, dtype=torch.float64, device="cuda")
    for v in range(c.V):
        rows = c.rows_of(c.view_entry[v])
        if len(rows):
            fx, fy, cx, cy = c.intr[v]
            out[v] = ops.render_depth(_dev(c.points[rows, 1:]), c.w2c[v], fx, fy, cx, cy, c.W, c.H, c.cut)
    return out


# ------------------------------------------------------------------------------------------ the images
@pytest.mark.parametrize("name", rd.CASES)
def test_images_are_the_reference_bit_for_bit(env, name):
    ops, sparse = env
    c, ref = rd.case(name), rd.reference(name)
    P = _dev(c.points)
    ve, M, K = _geometry(c)
    with _readbacks(ops) as rb:
        got = sparse.render_depth(P, ve, M, K, (c.H, c.W), cut_bound=c.cut)
    assert rb["n"] == 1                                                          # the status
    assert got.dtype == torch.float64 and got.shape == (c.V, c.H, c.W) and got.is_contiguous() and not got.requires_grad
    assert np.array_equal(got.cpu().numpy(), ref)
    raw, status = ops.render_depth_batched(P, ve, M, K, (c.H, c.W), c.cut)
    assert np.array_equal(raw.cpu().numpy(), ref)
    assert status.tolist() == [0, 0, 0, int(c.points[:, 0].max()), 0, 0, 0, 0]
    assert torch.equal(_bits(raw), _bits(got))                                   # two calls, the same bits
    assert np.array_equal(_per_scene(ops, c).cpu().numpy(), ref)                 # the per-scene kernel, view by view
    # fp32 points are upcast first
    got32 = sparse.render_depth(P.float(), ve.int(), M, K, [c.H, c.W], cut_bound=c.cut)
    c32 = rd.RCase(c.name, c.points.astype(np.float32), c.view_entry, c.w2c, c.intr, c.H, c.W, c.cut)
    assert np.array_equal(got32.cpu().numpy(), rd.render(c32))


@pytest.mark.parametrize("name", rd.CASES)
def test_the_state_form_gives_the_same_bits(env, name):
    """ops.render_depth_stream on the state of either stream, whole and in chunks of views"""
    ops, _ = env
    c, ref = rd.case(name), rd.reference(name)
    P = _dev(c.points)
    ve, M, K = _geometry(c)
    for st in (ops.lift_stream_begin(P, 3), ops.lift_masks_stream_begin(P)):
        state = st.state.clone()
        got, status = ops.render_depth_stream(st, ve, M, K, (c.H, c.W), c.cut)
        assert np.array_equal(got.cpu().numpy(), ref) and status.tolist() == [0] * 8
        assert torch.equal(st.state, state)                                      # the state is only read
    half = c.V // 2
    for idx in ([np.arange(half), np.arange(half, c.V)] if half else []):
        got, _ = ops.render_depth_stream(st, *_geometry(c, idx), (c.H, c.W), c.cut)
        assert np.array_equal(got.cpu().numpy(), ref[idx])


def test_bad_views_and_bad_rows_at_the_ops_level(env):
    """a view whose entry is outside 0..65535 keeps a 999999 image, rows with a bad or NaN batch index are never rendered, and the
    status words count them"""
    ops, sparse = env
    c, ref = rd.case("bad"), rd.reference("bad")
    n = c.notes
    P = _dev(c.points)
    ve, M, K = _geometry(c)
    got, status = ops.render_depth_batched(P, ve, M, K, (c.H, c.W), c.cut)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert status.tolist() == [n["bad_rows"], n["bad_views"], n["nonfinite_rows"], n["top_batch"], 0, 0, 0, 0]
    bad = (c.view_entry < 0) | (c.view_entry > 65535)
    assert bool((got[_dev(bad)] == rd.FAR).all())
    got, status = ops.render_depth_stream(ops.lift_stream_begin(P, 1), ve, M, K, (c.H, c.W), c.cut)
    assert np.array_equal(got.cpu().numpy(), ref) and status.tolist() == [0, n["bad_views"], 0, 0, 0, 0, 0, 0]
    # sparse refuses them, non-finite rows first, as lift does
    with pytest.raises(ValueError, match="rows of points are not finite"):
        sparse.render_depth(P, ve, M, K, (c.H, c.W))
    finite = np.isfinite(c.points).all(1)
    with pytest.raises(ValueError, match="batch index that is no integer"):
        sparse.render_depth(_dev(c.points[finite]), ve, M, K, (c.H, c.W))
    b = c.points[:, 0]
    good = finite & (b >= 0) & (b <= 65535) & (b == np.floor(b))
    with pytest.raises(ValueError, match="view_entry outside 0..65535"):
        sparse.render_depth(_dev(c.points[good]), ve, M, K, (c.H, c.W))
    assert np.array_equal(sparse.render_depth(_dev(c.points[good]), ve[~_dev(bad)], M[~_dev(bad)], K[~_dev(bad)], (c.H, c.W)).cpu().numpy(), ref[~bad])


def test_a_depth_buffer_off_the_16_byte_boundary(env):
    """the fill's scalar head: a caller's depth buffer that starts 8 bytes past a 16-byte boundary, nothing written around it"""
    ops, _ = env
    c, ref = rd.case("image_11x13"), rd.reference("image_11x13")
    size = c.V * c.H * c.W
    for lead, tail in ((1, 1), (1, 2), (2, 1)):
        big = torch.full((lead + size + tail,), -7.0, dtype=torch.float64, device="cuda")
        depth = big[lead:lead + size].view(c.V, c.H, c.W)
        assert depth.data_ptr() % 16 == (8 if lead % 2 else 0)
        got, _ = ops.render_depth_batched(_dev(c.points), *_geometry(c), (c.H, c.W), c.cut, depth=depth)
        assert got.data_ptr() == depth.data_ptr() and np.array_equal(got.cpu().numpy(), ref)
        assert bool((big[:lead] == -7.0).all()) and bool((big[lead + size:] == -7.0).all())


# ------------------------------------------------------------------------------------------ depth="render" in the one-call lifts
def _lift_views(sparse, c, depth, idx=None):
    idx = np.arange(c.V) if idx is None else np.asarray(idx, np.int64)
    d = depth[idx] if torch.is_tensor(depth) else depth
    return sparse.Views(_dev(c.maps[idx]), *_geometry(c, idx), d, None if (c.H, c.W) == (c.h, c.w) else (c.H, c.W))


def _lift_options(c):
    return dict(mode=c.mode, cut_bound=c.cut, vis_thres=c.tau, min_visible=c.min_visible, max_visible=c.max_visible)


def _rendered(sparse, c):
    return sparse.render_depth(_dev(c.points), *_geometry(c), (c.H, c.W), cut_bound=c.cut)


@contextlib.contextmanager
def _readbacks(ops):
    """counts the calls of ops.readback inside the block"""
    real, n = ops.readback, {"n": 0}

    def counted(t):
        n["n"] += 1
        return real(t)
    ops.readback = counted
    try:
        yield n
    finally:
        ops.readback = real


@pytest.mark.parametrize("name", rd.LIFT_CASES)
def test_lift_render_is_lift_on_the_rendered_tensor(env, name):
    ops, sparse = env
    c = rd.lift_case(name)
    P, depth = _dev(c.points), _rendered(sparse, c)
    assert np.array_equal(depth.cpu().numpy(), rd.lift_depth(name))
    for fill in (True, False):
        with _readbacks(ops) as rb:
            got = sparse.lift(P, _lift_views(sparse, c, "render"), fill=fill, **_lift_options(c))
        assert rb["n"] == 1                                                      # lift's own status read-back and no other
        _assert_same(got, sparse.lift(P, _lift_views(sparse, c, depth), fill=fill, **_lift_options(c)), LIFT_FIELDS, f"{name} / fill={fill}")
    # ... and it is not the lift without depths
    none = sparse.lift(P, _lift_views(sparse, c, None), **_lift_options(c))
    assert not torch.equal(none.count, got.count)


@pytest.mark.parametrize("name", rd.LIFT_CASES)
def test_lift_render_matches_the_lift_reference(env, name):
    """lift_batched_cases' reference on a Case whose depth is the reference's rendered depth, with that file's bounds"""
    _, sparse = env
    c = rd.lift_case(name)
    ref = lb._reference(rd.with_depth(c, rd.lift_depth(name)))
    got = sparse.lift(_dev(c.points), _lift_views(sparse, c, "render"), **_lift_options(c))
    assert np.array_equal(got.seen.cpu().numpy(), ref.seen) and np.array_equal(got.count.cpu().numpy(), ref.count)
    assert np.array_equal(got.view_count.cpu().numpy(), ref.view_count) and np.array_equal(got.view_keep.cpu().numpy(), ref.view_keep)
    f = got.features.cpu().numpy()
    if c.mode == "nearest":
        assert np.array_equal(f.view(np.int32), ref.features.view(np.int32))
    else:
        err = float(np.abs(f.astype(np.float64) - ref.features.astype(np.float64)).max())
        print(f"{name}: max |features - oracle| = {err:.3e}")
        assert np.abs(c.maps).max() <= 1.0 and err <= BILINEAR_TOL


_MASK_CASES = {}


def _mask_case(name):
    """the geometry of a lift case with X-Decoder outputs of tests/lift_masks_batched_cases.py"""
    if name not in _MASK_CASES:
        _MASK_CASES[name] = lm.with_vlm(name, rd.lift_case(name), 7 + rd.LIFT_CASES.index(name))
    return _MASK_CASES[name]


def _mask_views(sparse, c, depth, idx=None):
    idx = np.arange(c.V) if idx is None else np.asarray(idx, np.int64)
    d = depth[idx] if torch.is_tensor(depth) else depth
    return sparse.MaskViews(_dev(c.pred_masks[idx]), _dev(c.pred_logits[idx]), _dev(c.mask_embed[idx]), *_geometry(c, idx), d, (c.H, c.W))


def _mask_options(c):
    return dict(cut_bound=c.cut, vis_thres=c.tau, min_visible=c.min_visible, max_visible=c.max_visible)


@pytest.mark.parametrize("name", ["lift_nearest", "lift_views_70"])
def test_lift_masks_render_is_lift_masks_on_the_rendered_tensor(env, name):
    ops, sparse = env
    c = _mask_case(name)
    P, text, depth = _dev(c.points), _dev(c.text), _rendered(sparse, c)
    for fill in (True, False):
        with _readbacks(ops) as rb:
            got = sparse.lift_masks(P, _mask_views(sparse, c, "render"), text, c.scale, fill=fill, **_mask_options(c))
        assert rb["n"] == 2                                                      # the sizes and the status, as without "render"
        want = sparse.lift_masks(P, _mask_views(sparse, c, depth), text, c.scale, fill=fill, **_mask_options(c))
        _assert_same(got, want, MASK_FIELDS, f"{name} / fill={fill}")
    none = sparse.lift_masks(P, _mask_views(sparse, c, None), text, c.scale, **_mask_options(c))
    assert not torch.equal(none.count, got.count)


# ------------------------------------------------------------------------------------------ depth="render" in the streams
def _chunkings(V):
    """chunks of one view each, and uneven chunks (1, 2, 4, ... views, then the rest)"""
    uneven, at, size = [], 0, 1
    while at < V:
        uneven.append(np.arange(at, min(at + size, V)))
        at, size = at + size, size * 2
    return {"singles": [np.array([v]) for v in range(V)], "uneven": uneven}


@pytest.mark.parametrize("kind", ["singles", "uneven"])
@pytest.mark.parametrize("name", rd.LIFT_CASES)
def test_lift_stream_render(env, name, kind):
    """LiftStream with depth="render": after every prefix of the chunks finish gives the bits of lift(depth="render") on the views so
    far (checked midway and at the end); add makes no read-back, finish one"""
    ops, sparse = env
    c = rd.lift_case(name)
    P = _dev(c.points)
    chunks = _chunkings(c.V)[kind]
    mid = len(chunks) // 2
    s = sparse.LiftStream(P, feature_dim=c.D, **_lift_options(c))
    for i, ch in enumerate(chunks):
        with _readbacks(ops) as rb:
            s.add(_lift_views(sparse, c, "render", ch))
        assert rb["n"] == 0
        if i in (mid, len(chunks) - 1):
            sofar = np.concatenate(chunks[:i + 1])
            for fill in (True, False):
                with _readbacks(ops) as rb:
                    got = s.finish(fill=fill)
                assert rb["n"] == 1
                want = sparse.lift(P, _lift_views(sparse, c, "render", sofar), fill=fill, **_lift_options(c))
                _assert_same(got, want, LIFT_FIELDS, f"{name} / {kind} / after chunk {i} / fill={fill}")


@pytest.mark.parametrize("kind", ["singles", "uneven"])
@pytest.mark.parametrize("name", ["lift_nearest", "lift_bilinear"])
def test_lift_masks_stream_render(env, name, kind):
    """LiftMasksStream with depth="render": the bits of lift_masks(depth="render") midway and at the end; add makes its one read-back,
    finish one"""
    ops, sparse = env
    c = _mask_case(name)
    P, text = _dev(c.points), _dev(c.text)
    chunks = _chunkings(c.V)[kind]
    mid = len(chunks) // 2
    s = sparse.LiftMasksStream(P, text, c.scale, **_mask_options(c))
    for i, ch in enumerate(chunks):
        with _readbacks(ops) as rb:
            s.add(_mask_views(sparse, c, "render", ch))
        assert rb["n"] == 1
        if i in (mid, len(chunks) - 1):
            sofar = np.concatenate(chunks[:i + 1])
            with _readbacks(ops) as rb:
                got = s.finish()
            assert rb["n"] == 1
            want = sparse.lift_masks(P, _mask_views(sparse, c, "render", sofar), text, c.scale, **_mask_options(c))
            _assert_same(got, want, MASK_FIELDS, f"{name} / {kind} / after chunk {i}")


# ------------------------------------------------------------------------------------------ refusals
@contextlib.contextmanager
def _no_op_runs(ops):
    """every public function of ops but readback counts its calls inside the block; none may be called"""
    real = {k: f for k, f in vars(ops).items() if inspect.isfunction(f) and not k.startswith("_") and k != "readback"}
    calls = []

    def counted(k, f):
        def g(*a, **kw):
            calls.append(k)
            return f(*a, **kw)
        return g
    for k, f in real.items():
        setattr(ops, k, counted(k, f))
    try:
        yield
    finally:
        for k, f in real.items():
            setattr(ops, k, f)
    assert calls == []


def test_refusals_before_any_kernel(env):
    ops, sparse = env
    c = rd.lift_case("lift_nearest")
    m = _mask_case("lift_nearest")
    P, text = _dev(c.points), _dev(m.text)
    ve, M, K = _geometry(c)
    depth = _rendered(sparse, c)
    half = [np.arange(c.V // 2), np.arange(c.V // 2, c.V)]
    ls = sparse.LiftStream(P, feature_dim=c.D, **_lift_options(c))
    ls.add(_lift_views(sparse, c, "render", half[0]))
    lt = sparse.LiftStream(P, feature_dim=c.D, **_lift_options(c))
    lt.add(_lift_views(sparse, c, depth, half[0]))
    ms = sparse.LiftMasksStream(P, text, m.scale, **_mask_options(m))
    ms.add(_mask_views(sparse, m, "render", half[0]))
    mn = sparse.LiftMasksStream(P, text, m.scale, **_mask_options(m))
    mn.add(_mask_views(sparse, m, None, half[0]))
    before = (ls.finish(), ms.finish())
    with _no_op_runs(ops):
        # exactly the string "render"
        for word in ("rendered", "Render", "", "render "):
            with pytest.raises(ValueError, match="the string 'render'"):
                sparse.lift(P, _lift_views(sparse, c, word), **_lift_options(c))
            with pytest.raises(ValueError, match="the string 'render'"):
                sparse.lift_masks(P, _mask_views(sparse, m, word), text, m.scale, **_mask_options(m))
            with pytest.raises(ValueError, match="the string 'render'"):
                ls.add(_lift_views(sparse, c, word, half[1]))
            with pytest.raises(ValueError, match="the string 'render'"):
                ms.add(_mask_views(sparse, m, word, half[1]))
        # the three kinds do not mix in a stream
        with pytest.raises(ValueError, match="the presence of depth"):
            ls.add(_lift_views(sparse, c, depth, half[1]))
        with pytest.raises(ValueError, match="the presence of depth"):
            ls.add(_lift_views(sparse, c, None, half[1]))
        with pytest.raises(ValueError, match="the presence of depth"):
            lt.add(_lift_views(sparse, c, "render", half[1]))
        with pytest.raises(ValueError, match="the presence of depth"):
            ms.add(_mask_views(sparse, m, depth, half[1]))
        with pytest.raises(ValueError, match="the presence of depth"):
            mn.add(_mask_views(sparse, m, "render", half[1]))
        # CPU tensors
        with pytest.raises(ValueError, match="CUDA tensors"):
            sparse.render_depth(P.cpu(), ve, M, K, (c.H, c.W))
        with pytest.raises(ValueError, match="CUDA tensors"):
            sparse.render_depth(P, ve, M.cpu(), K, (c.H, c.W))
        v = _lift_views(sparse, c, "render")
        v.intrinsics = v.intrinsics.cpu()
        with pytest.raises(ValueError, match="CUDA tensors"):
            sparse.lift(P, v, **_lift_options(c))
        # image shapes with a non-positive side
        for shape in ((0, c.W), (c.H, -1), (c.H,), None, (c.H, 2.5)):
            with pytest.raises(ValueError, match="image_shape must be"):
                sparse.render_depth(P, ve, M, K, shape)
        v = _lift_views(sparse, c, "render")
        v.image_shape = (c.H, 0)
        with pytest.raises(ValueError, match="image_shape must be"):
            sparse.lift(P, v, **_lift_options(c))
        # the other fields, with lift's words
        with pytest.raises(ValueError, match=r"points must be \[N, 4\]"):
            sparse.render_depth(P[:, :3], ve, M, K, (c.H, c.W))
        with pytest.raises(ValueError, match="view_entry must be an integer tensor"):
            sparse.render_depth(P, ve.double(), M, K, (c.H, c.W))
        with pytest.raises(ValueError, match="world_to_camera must be fp64"):
            sparse.render_depth(P, ve, M.float(), K, (c.H, c.W))
        with pytest.raises(ValueError, match="intrinsics must be fp64"):
            sparse.render_depth(P, ve, M, K[:, :3], (c.H, c.W))
        with pytest.raises(ValueError, match="cut_bound"):
            sparse.render_depth(P, ve, M, K, (c.H, c.W), cut_bound=-1)
    # the refused adds left the streams as they were
    _assert_same(ls.finish(), before[0], LIFT_FIELDS, "LiftStream after the refusals")
    _assert_same(ms.finish(), before[1], MASK_FIELDS, "LiftMasksStream after the refusals")
    # the ops wrappers check dtype, shape and contiguity
    for bad in (lambda: ops.render_depth_batched(P.float(), ve, M, K, (c.H, c.W), 0), lambda: ops.render_depth_batched(P, ve.int(), M, K, (c.H, c.W), 0),
                lambda: ops.render_depth_batched(P, ve, M[:, :3], K, (c.H, c.W), 0), lambda: ops.render_depth_batched(P, ve, M, K, (0, c.W), 0),
                lambda: ops.render_depth_batched(P.t().contiguous().t(), ve, M, K, (c.H, c.W), 0),
                lambda: ops.render_depth_batched(P, ve, M, K, (c.H, c.W), 0, depth=depth[:, :-1]),
                lambda: ops.render_depth_stream(ls._st, ve, M, K[:-1], (c.H, c.W), 0)):
        with pytest.raises(ValueError):
            bad()


def test_the_library_refuses_what_the_wrappers_cannot_see(env):
    """overlapping arguments and a workspace or state that is too small: GP_EINVAL / GP_ENOMEM before any launch"""
    ops, _ = env
    from geopurify_amd._lib import GeoPurifyHipError
    c = rd.case("image_11x13")
    P = _dev(c.points)
    ve, M, K = _geometry(c)
    size = c.V * c.H * c.W
    both = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        ops.render_depth_batched(P, ve, M, K, (c.H, c.W), 0, depth=both[:size * 8].view(torch.float64).view(c.V, c.H, c.W), workspace=both)
    buf = torch.zeros(c.N * 4 + size, dtype=torch.float64, device="cuda")
    buf[:c.N * 4].view(c.N, 4).copy_(P)
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):                     # the depth begins on the last point row
        ops.render_depth_batched(buf[:c.N * 4].view(c.N, 4), ve, M, K, (c.H, c.W), 0, depth=buf[c.N * 4 - 2:c.N * 4 - 2 + size].view(c.V, c.H, c.W))
    with pytest.raises(GeoPurifyHipError, match="workspace too small"):
        ops.render_depth_batched(P, ve, M, K, (c.H, c.W), 0, workspace=both[:256])
    st = ops.lift_stream_begin(P, 1)
    with pytest.raises(GeoPurifyHipError, match="workspace too small"):
        ops.render_depth_stream(st, ve, M, K, (c.H, c.W), 0, workspace=both[:256])
    with pytest.raises(GeoPurifyHipError, match="state too small"):
        ops.render_depth_stream(ops.LiftStreamState(P, st.state[:256], None, None, None), ve, M, K, (c.H, c.W), 0)
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        ops.render_depth_stream(st, ve, M, K, (c.H, c.W), 0, workspace=st.state)


# ------------------------------------------------------------------------------------------ extents
def _f64(t):
    """fp64 arrays travel through the fences as their int64 bit patterns (extent_fence has no fp64 poison of its own)"""
    return t.view(torch.int64)


@pytest.mark.parametrize("entry", ["one_call", "state"])
def test_the_entry_points_stay_inside_their_extents(env, entry):
    """gp_render_depth_batched / gp_render_depth_batched_state on fenced arrays at their exact extents: every input (the fp64 ones as
    their bit patterns), the depth output, the status and a workspace of exactly the reported bytes.  Nothing outside the extents is
    written, nothing read from there reaches the image."""
    ops, _ = env
    from geopurify_amd import _lib
    lib = _lib.load()
    c, ref = rd.case("image_11x13"), rd.reference("image_11x13")
    V, H, W, N = c.V, c.H, c.W, c.N
    state = ops.lift_stream_begin(_dev(c.points), 1).state
    assert state.numel() == lib.gp_lift_stream_state_bytes(N)

    def case(a):
        P = a.inp(_f64(torch.from_numpy(c.points)), name="points").view(torch.float64)
        ve = a.inp(torch.from_numpy(c.view_entry), name="view_entry")
        M = a.inp(_f64(torch.from_numpy(c.w2c)).reshape(-1), name="w2c").view(torch.float64).view(V, 4, 4)
        K = a.inp(_f64(torch.from_numpy(c.intr)), name="intrinsics").view(torch.float64)
        depth = a.out(V * H * W, torch.int64, name="depth").view(torch.float64).view(V, H, W)
        status = a.out(8, torch.int64, name="status")
        if entry == "one_call":
            ws = a.out(lib.gp_render_depth_batched_workspace_bytes(N, V), torch.uint8, name="workspace")
            d, s = ops.render_depth_batched(P, ve, M, K, (H, W), c.cut, depth=depth, status=status, workspace=ws)
        else:
            ws = a.out(lib.gp_render_depth_batched_state_workspace_bytes(N, V), torch.uint8, name="workspace")
            st = ops.LiftStreamState(P, a.inp(state, name="state"), None, None, None)
            d, s = ops.render_depth_stream(st, ve, M, K, (H, W), c.cut, depth=depth, status=status, workspace=ws)
        return {"depth": _f64(d), "status": s}

    got = extent_fence.run(case)
    assert extent_fence.unwritten(got["depth"]) == 0 and extent_fence.unwritten(got["status"]) == 0
    assert np.array_equal(got["depth"].view(torch.float64).cpu().numpy(), ref)
    assert got["status"].tolist() == ([0, 0, 0, 4, 0, 0, 0, 0] if entry == "one_call" else [0] * 8)


def test_a_foreign_state_takes_the_kernel_outside_no_extent(env):
    """a state that no begin wrote (every byte 0xFF: keys 2^32 - 1, row numbers and offsets -1) under fences: the tables are forced into
    range, the forced values are counted, nothing outside an extent is written, and no row of another entry is rendered"""
    ops, _ = env
    from geopurify_amd import _lib
    lib = _lib.load()
    c = rd.case("entries")
    a = extent_fence.Arena(True)
    P = _dev(c.points)
    state = a.out(lib.gp_lift_stream_state_bytes(c.N), torch.uint8, name="state")
    state.fill_(0xFF)
    depth = a.out(c.V * c.H * c.W, torch.int64, name="depth").view(torch.float64).view(c.V, c.H, c.W)
    d, status = ops.render_depth_stream(ops.LiftStreamState(P, state, None, None, None), *_geometry(c), (c.H, c.W), c.cut, depth=depth,
                                        status=a.out(8, torch.int64, name="status"),
                                        workspace=a.out(lib.gp_render_depth_batched_state_workspace_bytes(c.N, c.V), torch.uint8, name="workspace"))
    torch.cuda.synchronize()
    extent_fence.assert_intact(*a.fences)
    assert status.tolist()[6] > 0 and bool((d == rd.FAR).all())                  # (offsets forced to 0: every entry is empty)
