"""The four batched lifts on fp16 / bf16 VLM outputs read in place (sparse.lift, LiftStream, lift_masks, LiftMasksStream; cases of
tests/lift_half_cases.py).

The yardstick is exact.  fp16 -> fp32 and bf16 -> fp32 lose nothing and the kernels sum in fp32, so a call on a half tensor gives the
BITS of the same call on the caller's own fp32 copy: every comparison with the upcast call is torch.equal on the int32 view.  Against
the oracle on the rounded maps: "nearest" the same bits, "bilinear" within 1e-6 (the bound of tests/test_gpu_lift_batched.py on maps in
[-1, 1]).  The memory tests state conditions, not measurements: a half call never allocates an fp32 copy of its maps (M elements):
channels_last maps are read where they lie, NCHW maps get one transposed buffer of 2 M bytes where fp32 maps get one of 4 M.
"""
import numpy as np
import pytest
import torch

import extent_fence
import lift_batched_cases as lb
import lift_half_cases as lh

pytestmark = pytest.mark.gpu

KEYS = tuple(lh.DTYPES)
BILINEAR_TOL = 1e-6                                         # tests/test_gpu_lift_batched.py; measured there 1.2e-7
ALLOC_SLACK = 4096                                          # allocator rounding: a few blocks of 512 bytes
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
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(got, want, fields, what=""):
    for f in fields:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        if not torch.equal(_bits(a), _bits(b)):
            at = (_bits(a) != _bits(b)).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {f} differs from the upcast call, first at {at} ({int((_bits(a) != _bits(b)).sum())} elements)")


def _options(c):
    return dict(mode=c.mode, cut_bound=c.cut, vis_thres=c.tau, min_visible=c.min_visible, max_visible=c.max_visible)


def _laid(maps, layout):
    return maps.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else maps.contiguous()


def _views(sparse, c, maps, depth="case", idx=None):
    """the case's views (idx: a subset) with `maps` as given -- dtype and layout are the caller's"""
    idx = np.arange(c.V) if idx is None else np.asarray(idx, np.int64)
    if depth == "case":
        depth = None if c.depth is None else _dev(c.depth[idx])
    return sparse.Views(maps, _dev(c.view_entry[idx]), _dev(c.w2c[idx]), _dev(c.intr[idx]), depth, None if (c.H, c.W) == (c.h, c.w) else (c.H, c.W))


def _half(c, key, layout="nchw"):
    return _laid(_dev(c.maps).to(lh.DTYPES[key]), layout)


# ------------------------------------------------------------------------------------------ 1. bit equality with the upcast call
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", lh.LIFT_CASES + lh.WIDTH_CASES)
def test_lift_on_half_maps_is_the_upcast_call(env, name, key):
    _, sparse = env
    c = lh.case(name, key)
    points = _dev(c.points)
    for layout in ("nchw", "channels_last"):
        half = _half(c, key, layout)
        assert half.dtype == lh.DTYPES[key] and torch.equal(half.float(), _dev(c.maps))
        for fill in (True, False):
            got = sparse.lift(points, _views(sparse, c, half), fill=fill, **_options(c))
            want = sparse.lift(points, _views(sparse, c, _laid(half.float(), layout)), fill=fill, **_options(c))
            assert got.features.dtype == torch.float32 and got.features.shape == (c.N, c.D)
            _assert_same(got, want, LIFT_FIELDS, f"{name} / {key} / {layout} / fill={fill}")


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("depth", [None, "render"])
@pytest.mark.parametrize("name", ["views_130_bilinear", "D65", "twins", "width_520", "width_12_bilinear"])
def test_lift_on_half_maps_without_depth_and_with_rendered_depth(env, name, depth, key):
    _, sparse = env
    c = lh.case(name, key)
    points = _dev(c.points)
    for layout in ("nchw", "channels_last"):
        half = _half(c, key, layout)
        got = sparse.lift(points, _views(sparse, c, half, depth=depth), **_options(c))
        want = sparse.lift(points, _views(sparse, c, _laid(half.float(), layout), depth=depth), **_options(c))
        _assert_same(got, want, LIFT_FIELDS, f"{name} / {key} / {layout} / depth={depth}")
        assert bool(got.seen.any())


# ------------------------------------------------------------------------------------------ 2. against the oracle on the rounded maps
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", lh.LIFT_CASES + ("width_8", "width_12", "width_520", "width_521", "width_8_bilinear", "width_516_bilinear",
                                                  "width_1024_bilinear"))
def test_lift_on_half_maps_matches_the_oracle(env, name, key):
    ops, sparse = env
    c, ref = lh.case(name, key), lh.reference(name, key)
    for layout in ("nchw", "channels_last"):
        got = sparse.lift(_dev(c.points), _views(sparse, c, _half(c, key, layout)), **_options(c))
        assert np.array_equal(got.seen.cpu().numpy(), ref.seen) and np.array_equal(got.count.cpu().numpy(), ref.count)
        assert np.array_equal(got.view_count.cpu().numpy(), ref.view_count) and np.array_equal(got.view_keep.cpu().numpy(), ref.view_keep)
        f = got.features.cpu().numpy()
        if c.mode == "nearest":
            assert np.array_equal(f.view(np.int32), ref.features.view(np.int32)), layout
        else:
            err = float(np.abs(f.astype(np.float64) - ref.features.astype(np.float64)).max())
            print(f"{name} / {key} / {layout}: max |features - oracle| = {err:.3e}")
            assert np.abs(c.maps).max() <= 1.0 and err <= BILINEAR_TOL
    # the fill's choice
    half_pm = ops.lift_batched_transpose(_half(c, key))
    r = ops.lift_batched(_dev(c.points), half_pm, (c.h, c.w), _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), None if c.depth is None else _dev(c.depth),
                         (c.H, c.W), c.mode == "bilinear", c.cut, c.tau, c.min_visible, 2 ** 63 - 1 if c.max_visible is None else c.max_visible)
    assert half_pm.dtype == lh.DTYPES[key] and np.array_equal(r.nn.cpu().numpy(), ref.filled_from)
    assert r.status.tolist()[:3] == [0, 0, 0]


# ------------------------------------------------------------------------------------------ 3. exact conversion
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("D", lh.CONVERSION_WIDTHS)
def test_every_element_is_converted_exactly(env, D, key):
    """independent of the fp32 path: the expectation is torch's conversion on the CPU (lift_half_cases.conversion_expected)"""
    _, sparse = env
    c, half = lh.conversion_case(key, D)
    expected, _ = lh.conversion_expected(key, D)
    for layout in ("nchw", "channels_last"):
        got = sparse.lift(_dev(c.points), _views(sparse, c, _laid(half.cuda(), layout)), fill=False, **_options(c))
        assert bool(got.seen.all()) and bool((got.count == 1).all())
        f = got.features.cpu().numpy()
        bad = f.view(np.int32) != expected.view(np.int32)
        assert not bad.any(), (layout, int(bad.sum()), f[bad][:4], expected[bad][:4])


# ------------------------------------------------------------------------------------------ 4. alignment
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", lh.ALIGNMENT_CASES)
def test_a_base_that_is_only_2_byte_aligned(env, name, key):
    _, sparse = env
    c = lh.case(name, key)
    points = _dev(c.points)
    for layout in ("nchw", "channels_last"):
        aligned = _half(c, key, layout)
        off = lh.misaligned(aligned)
        assert off.data_ptr() % 4 == 2 and aligned.data_ptr() % 16 == 0 and torch.equal(off.view(torch.int16), aligned.view(torch.int16))
        got = sparse.lift(points, _views(sparse, c, off), **_options(c))
        want = sparse.lift(points, _views(sparse, c, aligned), **_options(c))
        _assert_same(got, want, LIFT_FIELDS, f"{name} / {key} / {layout}")


# ------------------------------------------------------------------------------------------ 5. streams
def _chunk_views(sparse, c, idx, kind, layout):
    maps = _dev(c.maps[idx])
    if kind != "fp32":
        maps = maps.to(lh.DTYPES[kind])
    return _views(sparse, c, _laid(maps, layout), idx=idx)


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("name", lh.STREAM_CASES)
def test_a_stream_of_mixed_dtypes_is_lift_on_the_upcast_concatenation(env, name, layout):
    _, sparse = env
    c, chunks = lh.stream_case(name)
    points = _dev(c.points)
    stream = sparse.LiftStream(points, c.D, **_options(c))
    seen_kinds, so_far = set(), []
    for idx, kind in chunks:
        stream.add(_chunk_views(sparse, c, idx, kind, layout))
        seen_kinds.add(kind)
        so_far = np.concatenate([so_far, idx]).astype(np.int64)
        for fill in (True, False):                                               # finish after every chunk
            got = stream.finish(fill=fill)
            want = sparse.lift(points, _views(sparse, c, _dev(c.maps[so_far]), idx=so_far), fill=fill, **_options(c))
            _assert_same(got, want, LIFT_FIELDS, f"{name} / {layout} / after {len(so_far)} views / fill={fill}")
    assert seen_kinds == set(lh.STREAM_KINDS)


@pytest.mark.parametrize("key", KEYS)
def test_the_stream_scratch_is_bytes_and_a_refused_add_changes_nothing(env, key):
    _, sparse = env
    c = lh.case("views_130", key)
    points = _dev(c.points)
    stream = sparse.LiftStream(points, c.D, **_options(c))
    a, b = np.arange(0, 3), np.arange(3, 9)                                      # 3 fp32 views, then 6 half views: the same bytes
    stream.add(_views(sparse, c, _dev(c.maps[a]), idx=a))
    scratch = stream._scratch
    assert scratch is not None and scratch.numel() * scratch.element_size() == 3 * c.D * c.h * c.w * 4
    stream.add(_views(sparse, c, _dev(c.maps[b]).to(lh.DTYPES[key]), idx=b))
    assert stream._scratch is scratch and stream._scratch.data_ptr() == scratch.data_ptr()      # no growth: no more bytes than before
    before = stream.finish()
    views_before = stream.num_views
    # refused: another width, integer maps, maps on the CPU -- each before any kernel
    wide = torch.zeros((2, c.D + 1, c.h, c.w), dtype=lh.DTYPES[key], device="cuda")
    for bad, message in ((wide, "channels"), (_dev(c.maps[:2]).to(torch.int32), "floating point"), (torch.from_numpy(c.maps[:2]).to(lh.DTYPES[key]), "CUDA")):
        with pytest.raises(ValueError, match=message):
            stream.add(_views(sparse, c, bad, idx=np.arange(2)))
    assert stream.num_views == views_before and stream._scratch is scratch
    _assert_same(stream.finish(), before, LIFT_FIELDS, "after the refused adds")
    rest = np.arange(9, c.V)
    stream.add(_views(sparse, c, _dev(c.maps[rest]).to(lh.DTYPES[key]), idx=rest))
    want = sparse.lift(points, _views(sparse, c, _dev(c.maps)), **_options(c))
    _assert_same(stream.finish(), want, LIFT_FIELDS, "the whole stream")


# ------------------------------------------------------------------------------------------ 6. masks
def _mask_views(sparse, c, pred_masks, idx=None):
    idx = np.arange(c.V) if idx is None else np.asarray(idx, np.int64)
    return sparse.MaskViews(pred_masks, _dev(c.pred_logits[idx]), _dev(c.mask_embed[idx]), _dev(c.view_entry[idx]), _dev(c.w2c[idx]),
                            _dev(c.intr[idx]), None if c.depth is None else _dev(c.depth[idx]), (c.H, c.W))


def _mask_options(c):
    return dict(cut_bound=c.cut, vis_thres=c.tau, min_visible=c.min_visible, max_visible=c.max_visible)


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", lh.MASK_CASES)
def test_lift_masks_on_half_masks_is_the_upcast_call(env, name, key):
    """fails where half masks are refused"""
    _, sparse = env
    c = lh.mask_case(name, key)
    points, text = _dev(c.points), _dev(c.text)
    half = _dev(c.pred_masks).to(lh.DTYPES[key])
    assert torch.equal(half.float(), _dev(c.pred_masks))
    for fill in (True, False):
        got = sparse.lift_masks(points, _mask_views(sparse, c, half), text, c.scale, fill=fill, **_mask_options(c))
        want = sparse.lift_masks(points, _mask_views(sparse, c, half.float()), text, c.scale, fill=fill, **_mask_options(c))
        _assert_same(got, want, MASK_FIELDS, f"{name} / {key} / fill={fill}")
        assert got.logit_scale == want.logit_scale
    assert bool(got.seen.any()) or name == "Q1"


@pytest.mark.parametrize("name", lh.MASK_CASES)
def test_a_mask_stream_of_mixed_dtypes_is_lift_masks_on_the_upcast_concatenation(env, name):
    _, sparse = env
    c, chunks = lh.mask_stream_case(name)
    points, text = _dev(c.points), _dev(c.text)
    stream = sparse.LiftMasksStream(points, text, c.scale, **_mask_options(c))
    so_far = []
    for idx, kind in chunks:
        pm = _dev(c.pred_masks[idx])
        stream.add(_mask_views(sparse, c, pm if kind == "fp32" else pm.to(lh.DTYPES[kind]), idx=idx))
        so_far = np.concatenate([so_far, idx]).astype(np.int64)
    for fill in (True, False):
        got = stream.finish(fill=fill)
        want = sparse.lift_masks(points, _mask_views(sparse, c, _dev(c.pred_masks)), text, c.scale, fill=fill, **_mask_options(c))
        _assert_same(got, want, MASK_FIELDS, f"{name} / fill={fill}")
    assert len(so_far) == c.V


def _counting(ops):
    """the counting spy of tests/test_gpu_lift_batched.py: ops.readback is the only synchronising call allowed"""
    real = ops.readback

    def counted(t):
        torch.cuda.set_sync_debug_mode("default")
        try:
            return real(t)
        finally:
            torch.cuda.set_sync_debug_mode("error")
    return real, counted


@pytest.mark.parametrize("key", KEYS)
def test_the_read_backs_stay_what_they_were(env, key):
    ops, sparse = env
    c = lh.mask_case("Q65", key)
    points, text = _dev(c.points), _dev(c.text)
    half = _dev(c.pred_masks).to(lh.DTYPES[key])
    whole = _mask_views(sparse, c, half)
    parts = [_mask_views(sparse, c, half[idx].contiguous(), idx=idx) for idx in (np.arange(0, 1), np.arange(1, c.V))]
    d = lh.case("views_130_bilinear", key)
    dpoints, dviews = _dev(d.points), _views(sparse, d, _half(d, key))
    sparse.lift_masks(points, whole, text, c.scale, **_mask_options(c))          # (the tap tables are uploaded once, outside the count)
    torch.cuda.synchronize()
    real, counted = _counting(ops)
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.readback = counted
        n0 = ops.READBACK["calls"]
        sparse.lift_masks(points, whole, text, c.scale, **_mask_options(c))
        assert ops.READBACK["calls"] == n0 + 2                                   # lift_masks: two
        stream = sparse.LiftMasksStream(points, text, c.scale, **_mask_options(c))
        assert ops.READBACK["calls"] == n0 + 2
        for i, p in enumerate(parts):
            stream.add(p)
            assert ops.READBACK["calls"] == n0 + 3 + i                           # every add: one
        stream.finish()
        assert ops.READBACK["calls"] == n0 + 3 + len(parts)                      # finish: one
        sparse.lift(dpoints, dviews, **_options(d))
        assert ops.READBACK["calls"] == n0 + 4 + len(parts)                      # lift: one
    finally:
        ops.readback = real
        torch.cuda.set_sync_debug_mode("default")


# ------------------------------------------------------------------------------------------ 7. no fp32 copy is made
MEM_V, MEM_D, MEM_HW = 16, 1024, (12, 16)                   # M = 3 * 2^20 elements: 2 M = 6 MiB, 4 M = 12 MiB


def _mem_case():
    return lb.generic("half_memory", 77, {0: 60, 1: 50}, {0: MEM_V // 2, 1: MEM_V // 2}, MEM_D, hw=MEM_HW)


def _peak(fn):
    """bytes the call holds at its peak on top of what was allocated before it.  The call allocates from a memory pool of its own: the
    caching allocator hands out a cached block whole when less than 1 MiB of it would be left over, so inside the suite's shared pool
    the same call is charged differently from one run to the next; in a fresh pool every block is cut to the request (rounded to 512
    bytes), and a transposed copy of 2 M or 4 M bytes -- whole multiples of the allocator's 2 MiB granule here -- is charged as such."""
    torch.cuda.synchronize()
    pool = torch.cuda.MemPool()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.cuda.use_mem_pool(pool):
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out                                                                  # (everything the call allocated dies before its pool)
    return peak


@pytest.mark.parametrize("key", KEYS)
def test_lift_makes_no_fp32_copy_of_half_maps(env, key):
    ops, sparse = env
    c = _mem_case()
    M = c.maps.size
    assert M == MEM_V * MEM_D * MEM_HW[0] * MEM_HW[1] and 2 * M % 2 ** 21 == 0 and 2 * M > 1000 * ALLOC_SLACK
    points = _dev(c.points)
    peaks = {}
    for layout in ("channels_last", "nchw"):
        for kind in ("fp32", key):
            maps = _laid(_dev(c.maps) if kind == "fp32" else _dev(c.maps).to(lh.DTYPES[key]), layout)
            views = _views(sparse, c, maps)
            sparse.lift(points, views, **_options(c))                            # (warm: lazily initialised library state stays out of the count)
            peaks[layout, kind] = _peak(lambda: sparse.lift(points, views, **_options(c)))
    print(f"{key}: M = {M}, peaks {peaks}")
    # (a) channels_last: read in place, whatever the dtype -- neither call allocates a map-sized buffer
    assert peaks["channels_last", key] <= peaks["channels_last", "fp32"] + ALLOC_SLACK
    assert peaks["channels_last", "fp32"] < 2 * M                                # (the entry tables and the rows: 1.5 MB)
    # (b) NCHW: one transposed buffer of the maps' own dtype, 2 M bytes below the fp32 call's
    assert peaks["nchw", key] <= peaks["nchw", "fp32"] - 2 * M + ALLOC_SLACK
    assert peaks["nchw", key] < peaks["channels_last", key] + 2 * M + ALLOC_SLACK


@pytest.mark.parametrize("key", KEYS)
def test_stream_add_makes_no_fp32_copy_of_half_maps(env, key):
    ops, sparse = env
    c = _mem_case()
    M = c.maps.size
    points = _dev(c.points)
    peaks = {}
    for layout in ("channels_last", "nchw"):
        for kind in ("fp32", key):
            maps = _laid(_dev(c.maps) if kind == "fp32" else _dev(c.maps).to(lh.DTYPES[key]), layout)
            views = _views(sparse, c, maps)
            warm = sparse.LiftStream(points, c.D, **_options(c))
            warm.add(views)
            del warm
            # (a fresh stream: its scratch is taken inside the add; the construction, the same for every dtype, is inside the count)
            peaks[layout, kind] = _peak(lambda: sparse.LiftStream(points, c.D, **_options(c)).add(views))
    print(f"{key}: M = {M}, peaks {peaks}")
    assert peaks["channels_last", key] <= peaks["channels_last", "fp32"] + ALLOC_SLACK
    assert peaks["channels_last", "fp32"] < 2 * M
    assert peaks["nchw", key] <= peaks["nchw", "fp32"] - 2 * M + ALLOC_SLACK
    assert peaks["nchw", key] < peaks["channels_last", key] + 2 * M + ALLOC_SLACK


@pytest.mark.parametrize("key", KEYS)
def test_the_kernels_receive_the_half_tensors(env, key):
    ops, sparse = env
    dtype = lh.DTYPES[key]
    got = {}
    real = {n: getattr(ops, n) for n in ("lift_batched", "lift_stream_add", "lift_masks_batched", "lift_masks_stream_add")}

    def spy(name, pos):
        def call(*a, **kw):
            got.setdefault(name, []).append((a[pos].dtype, a[pos].data_ptr()))
            return real[name](*a, **kw)
        return call
    c, m = lh.case("twins", key), lh.mask_case("twins", key)
    cl = _half(c, key, "channels_last")
    pm = _dev(m.pred_masks).to(dtype)
    try:
        ops.lift_batched, ops.lift_stream_add = spy("lift_batched", 1), spy("lift_stream_add", 1)
        ops.lift_masks_batched, ops.lift_masks_stream_add = spy("lift_masks_batched", 2), spy("lift_masks_stream_add", 2)
        sparse.lift(_dev(c.points), _views(sparse, c, cl), **_options(c))
        sparse.lift(_dev(c.points), _views(sparse, c, _half(c, key)), **_options(c))
        s = sparse.LiftStream(_dev(c.points), c.D, **_options(c))
        s.add(_views(sparse, c, cl))
        sparse.lift_masks(_dev(m.points), _mask_views(sparse, m, pm), _dev(m.text), m.scale, **_mask_options(m))
        ms = sparse.LiftMasksStream(_dev(m.points), _dev(m.text), m.scale, **_mask_options(m))
        ms.add(_mask_views(sparse, m, pm))
    finally:
        for n, f in real.items():
            setattr(ops, n, f)
    assert [d for d, _ in got["lift_batched"]] == [dtype, dtype] and got["lift_batched"][0][1] == cl.data_ptr()   # channels_last: in place
    assert got["lift_stream_add"] == [(dtype, cl.data_ptr())]
    assert got["lift_masks_batched"] == [(dtype, pm.data_ptr())] and got["lift_masks_stream_add"] == [(dtype, pm.data_ptr())]


@pytest.mark.parametrize("key", KEYS)
def test_the_mask_workspace_halves_its_transposed_copy(env, key):
    ops, _ = env
    n, V, Q, hw, HW, total, words = 5000, 7, 65, (8, 10), (12, 16), 9000, 2
    saved = 2 * V * hw[0] * hw[1] * Q
    full = ops.lift_masks_batched_workspace_bytes(n, V, Q, hw, HW, total, words)
    half = ops.lift_masks_batched_workspace_bytes(n, V, Q, hw, HW, total, words, dtype=lh.DTYPES[key])
    assert full == ops.lift_masks_batched_workspace_bytes(n, V, Q, hw, HW, total, words, dtype=torch.float32) > half > 0
    assert abs((full - half) - saved) < 256                                      # (the carver aligns every array to 256 bytes)
    full = ops.lift_masks_stream_add_workspace_bytes(n, V, Q, hw, HW, total)
    half = ops.lift_masks_stream_add_workspace_bytes(n, V, Q, hw, HW, total, dtype=lh.DTYPES[key])
    assert abs((full - half) - saved) < 256
    with pytest.raises(ValueError, match="torch.float64"):
        ops.lift_masks_batched_workspace_bytes(n, V, Q, hw, HW, total, words, dtype=torch.float64)


# ------------------------------------------------------------------------------------------ 8. extents
# extent_fence has poison for torch.float16 and none for torch.bfloat16: a bf16 array is fenced as the float16 array of the same
# bits (the copy into the fence is a copy of bits) and handed to the call as its bfloat16 view
def _fenced_in(a, t, name):
    return a.inp(t.view(torch.float16), name=name).view(t.dtype)


def _fenced_out(a, shape, dtype, name):
    return a.out(shape, torch.float16, name=name).view(dtype)


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", ["D65", "D_chunk_plus_1_bilinear", "width_520", "width_12_bilinear"])
def test_the_half_entry_points_stay_inside_their_extents(env, name, key):
    """ops.lift_batched_transpose, ops.lift_batched and ops.lift_stream_add in their half forms on fenced arrays: the half maps, the half
    transposed copy, every output and workspaces of exactly the reported bytes"""
    ops, sparse = env
    from geopurify_amd import _lib
    lib = _lib.load()
    dtype = lh.DTYPES[key]
    c, ref = lh.case(name, key), lh.reference(name, key)
    N, V, D = c.N, c.V, c.D
    half = torch.from_numpy(c.maps).to(dtype)
    args = lambda ve: (ve, _dev(c.w2c), _dev(c.intr), None if c.depth is None else _dev(c.depth), (c.H, c.W), c.mode == "bilinear", c.cut,   # noqa: E731
                       c.tau, c.min_visible, 2 ** 63 - 1 if c.max_visible is None else c.max_visible)

    def case(a):
        maps = _fenced_in(a, half, "maps")
        maps_pm = _fenced_out(a, (V, c.h * c.w, D), dtype, "maps_pm")
        ops.lift_batched_transpose(maps, out=maps_pm)
        ve = a.inp(torch.from_numpy(c.view_entry), name="view_entry")
        pitch = (D + 3) // 4 * 4 + 4 if a.fence else D
        bufs = {"out": a.out((N, D), torch.float32, pitch=pitch, name="out"), "seen": a.out(N, torch.uint8, name="seen"),
                "count": a.out(N, torch.int32, name="count"), "view_count": a.out(V, torch.int64, name="view_count"),
                "view_keep": a.out(V, torch.uint8, name="view_keep"), "nn": a.out(N, torch.int64, name="nn"),
                "status": a.out(8, torch.int64, name="status")}
        ws = a.out(lib.gp_lift_batched_workspace_bytes(N, V), torch.uint8, name="workspace")
        r = ops.lift_batched(_dev(c.points), maps_pm, (c.h, c.w), *args(ve), buffers=bufs, workspace=ws)
        # the stream's add on the same fenced copy
        begin = {"state": a.out(lib.gp_lift_stream_state_bytes(N), torch.uint8, name="state"),
                 "sums": a.out((N, D), torch.float32, pitch=pitch, name="sums"), "count": a.out(N, torch.int32, name="stream count"),
                 "status": a.out(8, torch.int64, name="running status")}
        st = ops.lift_stream_begin(_dev(c.points), D, buffers=begin,
                                   workspace=a.out(lib.gp_lift_stream_begin_workspace_bytes(N), torch.uint8, name="begin workspace"))
        add = {"view_count": a.out(V, torch.int64, name="stream view_count"), "view_keep": a.out(V, torch.uint8, name="stream view_keep")}
        vc, vk = ops.lift_stream_add(st, maps_pm, (c.h, c.w), *args(ve), buffers=add,
                                     workspace=a.out(lib.gp_lift_stream_add_workspace_bytes(V), torch.uint8, name="add workspace"))
        return {"maps_pm": maps_pm.view(torch.float16), "out": r.out, "seen": r.seen, "count": r.count, "view_count": r.view_count,
                "view_keep": r.view_keep, "nn": r.nn, "status": r.status, "sums": st.sums, "stream count": st.count, "stream view_count": vc,
                "stream view_keep": vk}

    got = extent_fence.run(case)
    for k, v in got.items():
        assert extent_fence.unwritten(v) == 0 or k == "maps_pm", k               # (a map may hold the poison's bits as a value)
    assert np.array_equal(got["nn"].cpu().numpy(), ref.filled_from) and np.array_equal(got["count"].cpu().numpy(), ref.count)
    assert np.array_equal(got["stream count"].cpu().numpy(), ref.count) and torch.equal(got["stream view_count"], got["view_count"])
    want_pm = half.view(torch.int16).reshape(V, D, -1).transpose(1, 2).contiguous()
    assert torch.equal(got["maps_pm"].cpu().view(torch.int16), want_pm)
    # the sums are the rows before the division: the same bits as the fp32 call's
    one = sparse.lift(_dev(c.points), _views(sparse, c, _dev(c.maps)), fill=False, **_options(c))
    assert torch.equal(_bits(got["out"]), _bits(one.features))


@pytest.mark.parametrize("key", KEYS)
def test_the_half_mask_entry_point_stays_inside_its_extents(env, key):
    ops, sparse = env
    from geopurify_amd import _lib
    lib = _lib.load()
    dtype = lh.DTYPES[key]
    c = lh.mask_case("Q65", key)
    N, V, D = c.N, c.V, c.D
    d4 = (D + 3) // 4 * 4
    half = torch.from_numpy(c.pred_masks).to(dtype)
    lists = ops.lift_masks_batched_lists(_dev(c.points), _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), None if c.depth is None else _dev(c.depth),
                                         (c.H, c.W), c.cut, c.tau, c.min_visible, 2 ** 63 - 1 if c.max_visible is None else c.max_visible)
    total = lists.total
    words = max(1, -(-lists.max_views // 64))
    tn = torch.nn.functional.normalize(_dev(c.text), dim=-1)
    e4, t4 = torch.zeros((V * c.Q, d4), device="cuda"), torch.zeros((c.C, d4), device="cuda")
    e4[:, :D], t4[:, :D] = _dev(c.mask_embed).reshape(V * c.Q, D), tn
    f_seg, l_seg = torch.empty((V, c.Q, d4), device="cuda"), torch.empty((V, c.Q, c.C), device="cuda")
    ops.segment_tables(e4, t4, c.scale, f_seg.view(V * c.Q, d4), l_seg.view(V * c.Q, -1))
    scores = torch.softmax(_dev(c.pred_logits), dim=-1)[..., :-1].max(-1).values.contiguous()
    taps = sparse._tap_tables(c.h, c.w, c.H, c.W, torch.device("cuda", torch.cuda.current_device()))
    fill_cap = min(total, 300)

    def case(a):
        pitch = d4 + 4 if a.fence else d4
        out = {"out": a.out((N, d4), torch.float32, pitch=pitch, name="out"), "seen": a.out(N, torch.uint8, name="seen"),
               "count": a.out(N, torch.int32, name="count"), "nn": a.out(N, torch.int64, name="nn"), "seg": a.out(total, torch.int32, name="seg"),
               "status": a.out(8, torch.int64, name="status")}
        ws = a.out(ops.lift_masks_batched_workspace_bytes(N, V, c.Q, (c.h, c.w), (c.H, c.W), total, words, fill_cap, dtype=dtype), torch.uint8,
                   name="workspace")
        assert ws.numel() == lib.gp_lift_masks_batched_workspace_bytes_t(ops.ELEM_TAG[dtype], N, V, c.Q, c.h, c.w, c.H, c.W, total, words, fill_cap)
        r = ops.lift_masks_batched(_dev(c.points), _dev(c.view_entry), _fenced_in(a, half, "pred_masks"), scores, taps, (c.H, c.W),
                                   (lists.pt, lists.x, lists.y, lists.view), lists.view_off, lists.view_keep, total, words, f_seg, l_seg,
                                   fill_cap=fill_cap, buffers=out, workspace=ws)
        return {"out": r.out, "seen": r.seen, "count": r.count, "nn": r.nn, "seg": r.seg, "status": r.status}

    got = extent_fence.run(case)
    for k, v in got.items():
        assert extent_fence.unwritten(v) == 0, k
    full = ops.lift_masks_batched(_dev(c.points), _dev(c.view_entry), _dev(c.pred_masks), scores, taps, (c.H, c.W),
                                  (lists.pt, lists.x, lists.y, lists.view), lists.view_off, lists.view_keep, total, words, f_seg, l_seg,
                                  fill_cap=fill_cap)
    assert torch.equal(got["seg"], full.seg) and torch.equal(_bits(got["out"]), _bits(full.out)) and torch.equal(got["nn"], full.nn)


def test_unknown_tags_and_overlaps_are_refused_by_the_entry_points(env):
    """GP_EINVAL from the C entry points, before any launch: a tag that names no element type; a transposed output that overlaps its
    input when the extents are counted at 2 bytes per element (and one that does not overlap at 2 bytes, though it would at 4)"""
    ops, _ = env
    import ctypes
    from geopurify_amd import _lib
    lib = _lib.load()
    EINVAL = -22
    V, D, hw = 2, 8, 12
    n = V * D * hw
    buf = torch.zeros(4 * n, dtype=torch.float16, device="cuda")
    p = lambda off: ctypes.c_void_p(buf.data_ptr() + 2 * off)                    # noqa: E731
    for tag in (3, -1, 7):
        assert lib.gp_lift_batched_transpose_t(p(0), tag, V, D, hw, p(2 * n), None) == EINVAL
        assert b"element type" in lib.gp_last_error()
        assert lib.gp_lift_masks_batched_workspace_bytes_t(tag, 100, 2, 5, 6, 8, 12, 16, 50, 1, 0) == 0
        assert lib.gp_lift_masks_stream_add_workspace_bytes_t(tag, 100, 2, 5, 6, 8, 12, 16, 50, 0) == 0
    for tag in (1, 2):
        assert lib.gp_lift_batched_transpose_t(p(0), tag, V, D, hw, p(n - 1), None) == EINVAL       # the last element of src
        assert b"dst overlaps src" in lib.gp_last_error()
        assert lib.gp_lift_batched_transpose_t(p(0), tag, V, D, hw, p(n), None) == 0                # adjacent at 2 bytes per element
    assert lib.gp_lift_batched_transpose_t(p(0), 0, V, D, hw, p(n), None) == EINVAL                   # the same elements as fp32: overlap
    torch.cuda.synchronize()
    # the tagged lift and stream entries: an unknown tag before anything else is looked at
    c = lh.case("D65", "fp16")
    pm = ops.lift_batched_transpose(_half(c, "fp16"))
    r = ops.lift_batched(_dev(c.points), pm, (c.h, c.w), _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), _dev(c.depth), (c.H, c.W), False, c.cut, c.tau,
                         0, 2 ** 63 - 1)
    real = dict(ops.ELEM_TAG)
    try:
        ops.ELEM_TAG[torch.float16] = 5
        with pytest.raises(_lib.GeoPurifyHipError, match="element type 5"):
            ops.lift_batched(_dev(c.points), pm, (c.h, c.w), _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), _dev(c.depth), (c.H, c.W), False, c.cut,
                             c.tau, 0, 2 ** 63 - 1)
        st = ops.lift_stream_begin(_dev(c.points), c.D)
        with pytest.raises(_lib.GeoPurifyHipError, match="element type 5"):
            ops.lift_stream_add(st, pm, (c.h, c.w), _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), _dev(c.depth), (c.H, c.W), False, c.cut, c.tau, 0,
                                2 ** 63 - 1)
    finally:
        ops.ELEM_TAG.clear()
        ops.ELEM_TAG.update(real)
    # an output that overlaps the half maps, extents at 2 bytes per element: the rows start inside the maps' last bytes
    flat = torch.zeros(pm.numel() + 2 * c.N * c.D, dtype=torch.float16, device="cuda")
    maps_in = flat[:pm.numel()].view(pm.shape)
    maps_in.copy_(pm)
    rows = flat[pm.numel() - 2:pm.numel() - 2 + 2 * c.N * c.D].view(torch.float32).view(c.N, c.D)
    with pytest.raises(_lib.GeoPurifyHipError, match="an output overlaps an input"):
        ops.lift_batched(_dev(c.points), maps_in, (c.h, c.w), _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), _dev(c.depth), (c.H, c.W), False, c.cut,
                         c.tau, 0, 2 ** 63 - 1, buffers={"out": rows})
    rows = flat[pm.numel():].view(torch.float32).view(c.N, c.D)                  # right behind them: no overlap at 2 bytes per element
    ok = ops.lift_batched(_dev(c.points), maps_in, (c.h, c.w), _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), _dev(c.depth), (c.H, c.W), False, c.cut,
                          c.tau, 0, 2 ** 63 - 1, buffers={"out": rows})
    assert torch.equal(_bits(ok.out), _bits(r.out))


# ------------------------------------------------------------------------------------------ 9. refusals
def test_other_dtypes_are_refused_as_before(env):
    ops, sparse = env
    c = lh.mask_case("Q65", "fp16")
    points, text = _dev(c.points), _dev(c.text)
    pm = _dev(c.pred_masks)
    bad = [pm.to(torch.int32), pm.double(), pm.to(torch.int16)]
    if hasattr(torch, "float8_e4m3fn"):
        bad.append(torch.zeros(pm.shape, dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn))
    for t in bad:
        with pytest.raises(ValueError, match="views.pred_masks must be fp32"):
            sparse.lift_masks(points, _mask_views(sparse, c, t), text, c.scale, **_mask_options(c))
        stream = sparse.LiftMasksStream(points, text, c.scale, **_mask_options(c))
        with pytest.raises(ValueError, match="views.pred_masks must be fp32"):
            stream.add(_mask_views(sparse, c, t))
    for half_points in (points.half(), points.bfloat16()):
        with pytest.raises(ValueError, match="points must be fp64 or fp32"):
            sparse.lift_masks(half_points, _mask_views(sparse, c, pm.half()), text, c.scale, **_mask_options(c))
        d = lh.case("twins", "fp16")
        with pytest.raises(ValueError, match="points must be fp64 or fp32"):
            sparse.lift(_dev(d.points).to(half_points.dtype), _views(sparse, d, _half(d, "fp16")), **_options(d))
    with pytest.raises(ValueError, match="expected contiguous CUDA"):
        ops.lift_batched_transpose(_dev(lh.case("twins", "fp16").maps).double())


@pytest.mark.parametrize("name", ["twins", "views_130_bilinear"])
def test_fp64_maps_still_give_the_bits_of_fp32(env, name):
    _, sparse = env
    c = lb.case(name)
    base = sparse.lift(_dev(c.points), _views(sparse, c, _dev(c.maps)), **_options(c))
    wide = sparse.lift(_dev(c.points), _views(sparse, c, _dev(c.maps).double()), **_options(c))
    _assert_same(wide, base, LIFT_FIELDS, name)
