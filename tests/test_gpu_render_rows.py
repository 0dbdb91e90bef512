"""Lifted clouds rendered back into their views on the GPU (csrc/render_rows.hip): sparse.render_rows, Rendered.labels / .features,
sparse.segment_views, ops.render_rows and ops.render_gather against the reference of tests/render_rows_cases.py.

Bounds.  Everything is an integer or a selection of fp64 / fp32 values, so every comparison is exact (np.array_equal / torch.equal on
bit patterns): the owner is a minimum over integers (the bit pattern of p_z, then the row), the cases keep p_z free of rounding
choices (see render_depth_cases), and the gather converts each element once with torch's own rounding.
"""
import numpy as np
import pytest
import torch

import extent_fence
import render_depth_cases as rd
import render_rows_cases as rr

pytestmark = pytest.mark.gpu

GATHER_D = (1, 3, 4, 6, 64, 100, 260, 512, 1028)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


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


def _geometry(c, idx=None):
    idx = np.arange(c.V) if idx is None else np.asarray(idx, np.int64)
    return _dev(c.view_entry[idx]), _dev(c.w2c[idx]), _dev(c.intr[idx])


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()]) if t.dtype.is_floating_point else t


def _render(sparse, c, depth, radius, idx=None, points=None):
    d = depth[np.arange(c.V) if idx is None else idx] if torch.is_tensor(depth) else depth
    return sparse.render_rows(_dev(c.points if points is None else points), *_geometry(c, idx), (c.H, c.W), depth=d, cut_bound=c.cut, radius=radius)


def _assert_is(got, ref, what):
    assert got.rows.dtype == torch.int32 and got.depth.dtype == torch.float64 and got.rows.is_contiguous(), what
    assert np.array_equal(got.rows.cpu().numpy(), ref.rows), what
    assert np.array_equal(got.depth.cpu().numpy().view(np.int64), ref.depth.view(np.int64)), what
    assert np.array_equal(got.view_count.cpu().numpy(), ref.view_count) and np.array_equal(got.pixel_count.cpu().numpy(), ref.pixel_count), what


def _same(a, b):
    return all(torch.equal(_bits(getattr(a, f)), _bits(getattr(b, f))) for f in ("rows", "depth", "view_count", "pixel_count"))


# ------------------------------------------------------------------------------------------ the owners
@pytest.mark.parametrize("name", rr.CASES)
def test_owners_are_the_reference(env, name):
    """rows, depth, view_count and pixel_count for depth None, "render" and the reference's rendered depth as a tensor, radius 0, 1, 2
    and 4; "render" equals the tensor form; two calls give the same bits"""
    _, sparse = env
    c = rr.case(name)
    maps = _dev(rd.reference(name)) if name in rd.CASES else None
    for radius in rr.RADII:
        none = _render(sparse, c, None, radius)
        _assert_is(none, rr.reference(name, "none", radius), (name, "none", radius))
        rend = _render(sparse, c, "render", radius)
        _assert_is(rend, rr.reference(name, "render", radius), (name, "render", radius))
        assert rend.image_shape == (c.H, c.W) and rend.num_entries == int(c.points[:, 0].max()) + 1
        assert _same(rend, _render(sparse, c, "render", radius))
        if maps is not None:
            assert _same(rend, _render(sparse, c, maps, radius)), (name, "tensor", radius)
        if "sensor" in c.notes:
            _assert_is(_render(sparse, c, _dev(c.notes["sensor"]), radius), rr.render(c, c.notes["sensor"], radius), (name, "sensor", radius))
    # fp32 points are upcast first
    c32 = rd.RCase(c.name, c.points.astype(np.float32), c.view_entry, c.w2c, c.intr, c.H, c.W, c.cut)
    got = sparse.render_rows(_dev(c.points).float(), *_geometry(c), [c.H, c.W], cut_bound=c.cut, radius=1)
    _assert_is(got, rr.render(c32, "render", 1), (name, "fp32"))


@pytest.mark.parametrize("name", ["views_130", "image_11x13", "stride", "twins", "cut_one_pixel"])
def test_view_count_is_the_lifts_and_depth_is_render_depths(env, name):
    _, sparse = env
    c = rr.case(name)
    P = _dev(c.points)
    ve, M, K = _geometry(c)
    maps = torch.zeros((c.V, 1, c.H, c.W), device="cuda")
    for depth in (None, "render"):
        lifted = sparse.lift(P, sparse.Views(maps, ve, M, K, depth), cut_bound=c.cut, min_visible=0, fill=False)
        for radius in (0, 2):
            assert torch.equal(_render(sparse, c, depth, radius).view_count, lifted.view_count)
    got, z = _render(sparse, c, "render", 0), sparse.render_depth(P, ve, M, K, (c.H, c.W), cut_bound=c.cut)
    near = got.depth > 0.2
    assert bool(near.any()) or name == "cut_one_pixel"
    assert torch.equal(_bits(got.depth[near]), _bits(z[near])) and bool((z[got.rows < 0] == rd.FAR).all())


@pytest.mark.parametrize("name", ["views_130", "image_11x13", "stride", "exact"])
def test_rows_permuted(env, name):
    """any row order: on the tie-free generic cases the owners are the same points after mapping through the permutation; on "exact"
    (equal depths: the lowest row wins, which the permutation changes) the result is the reference of the permuted input"""
    _, sparse = env
    c = rr.case(name)
    perm = np.random.default_rng(5).permutation(c.N)                         # new row i holds old row perm[i]
    cp = rd.RCase(c.name, c.points[perm], c.view_entry, c.w2c, c.intr, c.H, c.W, c.cut)
    for depth, radius in ((None, 1), ("render", 0), ("render", 2)):
        got = _render(sparse, cp, depth, radius)
        if name == "exact":
            _assert_is(got, rr.render(cp, depth, radius), (name, depth, radius))
            continue
        ref = rr.reference(name, "none" if depth is None else "render", radius)
        assert ref.contests == 0
        rows = got.rows.cpu().numpy()
        assert np.array_equal(np.where(rows >= 0, perm[np.maximum(rows, 0)], -1), ref.rows)
        assert np.array_equal(got.depth.cpu().numpy(), ref.depth) and np.array_equal(got.view_count.cpu().numpy(), ref.view_count)


def test_chunks_of_views_equal_the_whole(env):
    _, sparse = env
    c = rr.case("views_130")
    whole = _render(sparse, c, "render", 1)
    for size in (1, 7, c.V):
        parts = [_render(sparse, c, "render", 1, idx=np.arange(at, min(at + size, c.V))) for at in range(0, c.V, size)]
        for f in ("rows", "depth", "view_count", "pixel_count"):
            assert torch.equal(_bits(torch.cat([getattr(p, f) for p in parts])), _bits(getattr(whole, f))), (size, f)


def test_entries_do_not_mix(env):
    _, sparse = env
    c = rr.case("twins")
    own, mixed = _render(sparse, c, "render", 0), _render(sparse, rr.merged(c), "render", 0)
    _assert_is(mixed, rr.render(rr.merged(c), "render", 0), "merged")
    entry = torch.from_numpy(c.points[:, 0]).cuda()
    for v in range(c.V):
        assert not torch.equal(own.rows[v], mixed.rows[v])
        owners = own.rows[v][own.rows[v] >= 0].long()
        assert bool((entry[owners] == float(c.view_entry[v])).all())


def test_bad_views_and_bad_rows_at_the_ops_level(env):
    """bad rows and bad views touch nothing, the status words are the case's counts, the images of bad views stay -1 / 999999"""
    ops, sparse = env
    c = rd.case("bad")
    n = c.notes
    P = _dev(c.points)
    ve, M, K = _geometry(c)
    bad = (c.view_entry < 0) | (c.view_entry > 65535)
    for depth in (None, "render"):
        for radius in (0, 2):
            r = ops.render_rows(P, ve, M, K, (c.H, c.W), c.cut, depth=depth, radius=radius)
            ref = rr.render(c, depth, radius)
            assert r.status.tolist() == [n["bad_rows"], n["bad_views"], n["nonfinite_rows"], n["top_batch"], 0, 0, 0, 0]
            assert np.array_equal(r.rows.cpu().numpy(), ref.rows) and np.array_equal(r.depth.cpu().numpy(), ref.depth)
            assert np.array_equal(r.view_count.cpu().numpy(), ref.view_count) and np.array_equal(r.pixel_count.cpu().numpy(), ref.pixel_count)
            assert bool((r.rows[_dev(bad)] == -1).all()) and bool((r.depth[_dev(bad)] == rd.FAR).all()) and bool((r.view_count[_dev(bad)] == 0).all())
            b = c.points[:, 0]
            good = np.isfinite(c.points).all(1) & (b >= 0) & (b <= 65535) & (b == np.floor(b))
            owners = r.rows[r.rows >= 0].unique().cpu().numpy()
            assert good[owners].all()
    with pytest.raises(ValueError, match="rows of points are not finite"):
        sparse.render_rows(P, ve, M, K, (c.H, c.W))
    finite = np.isfinite(c.points).all(1)
    with pytest.raises(ValueError, match="batch index that is no integer"):
        sparse.render_rows(_dev(c.points[finite]), ve, M, K, (c.H, c.W))
    with pytest.raises(ValueError, match="view_entry outside 0..65535"):
        sparse.render_rows(_dev(c.points[good]), ve, M, K, (c.H, c.W))


def test_the_library_refuses_what_the_wrappers_cannot_see(env):
    ops, _ = env
    from geopurify_amd._lib import GeoPurifyHipError
    c = rr.case("image_11x13")
    P = _dev(c.points)
    ve, M, K = _geometry(c)
    size = c.V * c.H * c.W
    both = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    with pytest.raises(GeoPurifyHipError, match="two outputs overlap"):
        ops.render_rows(P, ve, M, K, (c.H, c.W), 0, buffers={"rows": both[:size * 4].view(torch.int32).view(c.V, c.H, c.W)}, workspace=both)
    with pytest.raises(GeoPurifyHipError, match="workspace too small"):
        ops.render_rows(P, ve, M, K, (c.H, c.W), 0, depth="render", workspace=both[:256])
    with pytest.raises(ValueError, match="radius"):
        ops.render_rows(P, ve, M, K, (c.H, c.W), 0, radius=5)
    src = torch.zeros((4, 8), device="cuda")
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        ops.render_gather(torch.zeros(4, dtype=torch.int32, device="cuda"), src, out=src)


# ------------------------------------------------------------------------------------------ the gather
def _special_rows(R, D, seed):
    """fp32 rows with values that overflow fp16 to inf, fp16 / bf16 subnormals, -0.0, rounding ties and a NaN row"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randn((R, D), generator=g)
    special = torch.tensor([70000.0, -1e6, 65520.0, 65519.0, 6e-8, -3e-8, 2.98e-8, 1e-40, -0.0, 0.0, 1.0009765625, 1.00048828125, 3.3895e38, float("inf")])
    src.view(-1)[torch.randperm(R * D, generator=g)[:min(len(special), R * D)]] = special[:min(len(special), R * D)]
    src[R - 1] = float("nan")
    return src


def _expected(rows, index, src, dtype):
    at = rows.reshape(-1).long().clamp(min=0)
    at = at if index is None else index[at]
    return torch.where((rows.reshape(-1) >= 0).unsqueeze(1), src[at], torch.zeros((), device=src.device)).to(dtype)


@pytest.mark.parametrize("D", GATHER_D)
def test_gather_is_a_selection_converted_once(env, D):
    """every width path (scalar, 16-byte with a tail, a second trip of the 256-column loop, odd widths under 2-byte outputs), source
    pitches D, D + 1 and D + 4, fp32 / fp16 / bf16, with and without an index, a pixel count that is no multiple of the pixels per block,
    a map that is all -1"""
    ops, _ = env
    N, R, npix = 37, 23, 4 * 13 + 3
    g = torch.Generator().manual_seed(D)
    index = torch.randint(0, R, (N,), generator=g).cuda()
    index[3] = R - 1                                                             # the NaN row is reachable
    for pitch in (D, D + 1, D + 4):
        for use_index in (False, True):
            rows_n = N if use_index else R
            rows = torch.randint(-1, rows_n, (npix,), generator=g, dtype=torch.int32)
            rows[:3] = torch.tensor([rows_n - 1, -1, 3 if use_index else R - 1])
            rows = rows.cuda().view(5, 11)
            base = torch.full((R, pitch), float("nan"), device="cuda")
            base[:, :D] = _special_rows(R, D, D + pitch).cuda()
            src = base[:, :D]
            idx = index if use_index else None
            for dtype in DTYPES:
                got = ops.render_gather(rows, src, idx, dtype)
                assert got.shape == (5, 11, D) and got.dtype == dtype
                want = _expected(rows, idx, src, dtype)
                assert torch.equal(_bits(got.reshape(-1, D)), _bits(want)), (D, pitch, use_index, dtype)
                empty = ops.render_gather(torch.full_like(rows, -1), src, idx, dtype)
                assert bool((_bits(empty) == 0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("D", [3, 6, 100, 260])
def test_gather_stays_inside_its_extents(env, D, dtype):
    """the pitched input and the pitched output inside poisoned guards, the rows and the index at their exact extents"""
    ops, _ = env
    N, R, npix = 19, 11, 45
    g = torch.Generator().manual_seed(7 * D)
    vals, index = torch.randn((R, D), generator=g), torch.randint(0, R, (N,), generator=g)
    rows = torch.randint(-1, N, (npix,), generator=g, dtype=torch.int32)
    pad = 8 if dtype == torch.float16 else 4
    pitch_in, pitch_out = (D + 3) // 4 * 4 + 4, (D + pad - 1) // pad * pad + pad

    def case(a):
        src = a.inp(vals, pitch=pitch_in, name="src")
        out = a.out((npix, D), dtype, pitch=pitch_out, name="out")
        ops.render_gather(a.inp(rows, name="rows"), src, a.inp(index, name="index"), dtype, out=out)
        return {"out": out}

    got = extent_fence.run(case)
    assert extent_fence.unwritten(got["out"]) == 0
    assert torch.equal(_bits(got["out"]), _bits(_expected(rows.cuda(), index.cuda(), vals.cuda(), dtype)))


def test_render_rows_stays_inside_its_extents(env):
    """rows, depth, the counts, the status and a workspace of exactly the reported bytes inside poisoned guards"""
    ops, _ = env
    from geopurify_amd import _lib
    lib = _lib.load()
    c = rr.case("image_11x13")
    V, H, W, N = c.V, c.H, c.W, c.N
    f64 = lambda t: t.view(torch.int64)                                          # noqa: E731
    for depth, mode in ((None, 0), ("render", 2)):
        def case(a):
            P = a.inp(f64(torch.from_numpy(c.points)), name="points").view(torch.float64)
            ve = a.inp(torch.from_numpy(c.view_entry), name="view_entry")
            M = a.inp(f64(torch.from_numpy(c.w2c)).reshape(-1), name="w2c").view(torch.float64).view(V, 4, 4)
            K = a.inp(f64(torch.from_numpy(c.intr)), name="intrinsics").view(torch.float64)
            buffers = {"rows": a.out(V * H * W, torch.int32, name="rows").view(V, H, W),
                       "depth": a.out(V * H * W, torch.int64, name="depth").view(torch.float64).view(V, H, W),
                       "view_count": a.out(V, torch.int64, name="view_count"), "pixel_count": a.out(V, torch.int64, name="pixel_count"),
                       "status": a.out(8, torch.int64, name="status")}
            ws = a.out(lib.gp_render_rows_workspace_bytes(N, V, H, W, mode), torch.uint8, name="workspace")
            r = ops.render_rows(P, ve, M, K, (H, W), c.cut, depth=depth, radius=2, buffers=buffers, workspace=ws)
            return {"rows": r.rows, "depth": f64(r.depth), "view_count": r.view_count, "pixel_count": r.pixel_count, "status": r.status}

        got = extent_fence.run(case)
        ref = rr.reference("image_11x13", "none" if depth is None else "render", 2)
        assert np.array_equal(got["rows"].cpu().numpy(), ref.rows) and np.array_equal(got["depth"].view(torch.float64).cpu().numpy(), ref.depth)
        assert np.array_equal(got["view_count"].cpu().numpy(), ref.view_count) and np.array_equal(got["pixel_count"].cpu().numpy(), ref.pixel_count)
        assert got["status"].tolist() == [0, 0, 0, 4, 0, 0, 0, 0]


def test_rows_off_the_16_byte_boundary(env):
    """the fills' scalar heads and tails: caller's buffers that start 4, 8 and 12 bytes past a 16-byte boundary"""
    ops, _ = env
    c, ref = rr.case("image_11x13"), rr.reference("image_11x13", "render", 0)
    size = c.V * c.H * c.W
    for lead in (1, 2, 3):
        big = torch.full((lead + size + 5,), -7, dtype=torch.int32, device="cuda")
        bigd = torch.full((lead + size + 5,), -7.0, dtype=torch.float64, device="cuda")
        r = ops.render_rows(_dev(c.points), *_geometry(c), (c.H, c.W), c.cut, depth="render",
                            buffers={"rows": big[lead:lead + size].view(c.V, c.H, c.W), "depth": bigd[lead:lead + size].view(c.V, c.H, c.W)})
        assert np.array_equal(r.rows.cpu().numpy(), ref.rows) and np.array_equal(r.depth.cpu().numpy(), ref.depth)
        assert bool((big[:lead] == -7).all()) and bool((big[lead + size:] == -7).all())
        assert bool((bigd[:lead] == -7).all()) and bool((bigd[lead + size:] == -7).all())


# ------------------------------------------------------------------------------------------ labels, features, counts
def test_features_through_sparse(env):
    """Rendered.features on a pitched y.F-like source, through an index, a slice and an index tensor of views"""
    ops, sparse = env
    c = rr.case("image_11x13")
    r = _render(sparse, c, "render", 1)
    g = torch.Generator().manual_seed(3)
    R, D = 40, 20
    index = torch.randint(0, R, (c.N,), generator=g).cuda()
    wide = torch.randn((R, D + 12), generator=g).cuda()
    src = wide[:, 4:4 + D]                                                       # pitched, base off the 16-byte boundary of a row
    for dtype in DTYPES:
        want = _expected(r.rows, index, src, dtype).view(c.V, c.H, c.W, D)
        got = r.features(src, index=index, dtype=dtype)
        assert got.shape == (c.V, c.H, c.W, D) and got.is_contiguous() and torch.equal(_bits(got), _bits(want))
        assert torch.equal(_bits(r.features(src, index=index, dtype=dtype, views=slice(1, 3))), _bits(want[1:3]))
        pick = torch.tensor([2, 0], device="cuda")
        assert torch.equal(_bits(r.features(src, index=index, dtype=dtype, views=pick)), _bits(want[pick]))
    per_point = torch.randn((c.N, 5), generator=g).cuda()
    assert torch.equal(r.features(per_point).reshape(-1, 5), _expected(r.rows, None, per_point, torch.float32))
    assert r.features(per_point, views=slice(0, 0)).shape == (0, c.H, c.W, 5)


@pytest.mark.parametrize("ldtype", [torch.int64, torch.uint8])
def test_labels_and_segment_views_against_numpy(env, ldtype):
    """views_130: per-voxel predictions through a quantiser's inverse_mapping, 2D labels with an ignored value present; the counts
    against np.bincount per entry"""
    ops, sparse = env
    c, C = rr.case("views_130"), 5
    r = _render(sparse, c, "render", 1)
    P = _dev(c.points)
    q = sparse.quantize(P, None, quantization_size=0.5)
    inv = q.inverse_mapping
    rng = np.random.default_rng(11)
    pred = rng.integers(0, C, q.coordinates.shape[0])
    maps = rng.integers(0, C + 1, (c.V, c.H, c.W))
    maps[maps == C] = 255                                                        # the ignored 2D label
    rows, invn = r.rows.cpu().numpy(), inv.cpu().numpy()
    for index, per in ((inv, pred), (None, pred[invn])):
        got = r.labels(_dev(per, ldtype), index=index)
        assert got.dtype == ldtype and np.array_equal(got.cpu().numpy(), np.where(rows >= 0, pred[invn[np.maximum(rows, 0)]], 255).astype(got.cpu().numpy().dtype))
        assert bool((r.labels(_dev(per, ldtype), index=index, fill=7)[r.rows < 0] == 7).all())
        counts = sparse.segment_views(r, _dev(per, ldtype), _dev(maps, ldtype), _dev(c.view_entry), C, index=index)
        want = np.zeros((r.num_entries, 3, C), np.int64)
        for v in range(c.V):
            ok = (rows[v] >= 0) & (maps[v] != 255)
            p, t = pred[invn[rows[v][ok]]], maps[v][ok]
            e = c.view_entry[v]
            want[e, 0] += np.bincount(p[p == t], minlength=C)
            want[e, 1] += np.bincount(p, minlength=C)
            want[e, 2] += np.bincount(t, minlength=C)
        assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), want) and want[:, 0].sum() > 0
    empty = sparse.render_rows(P, *_geometry(c), (c.H, c.W), cut_bound=6, depth=None)
    assert int(sparse.segment_views(empty, _dev(pred[invn]), _dev(maps), _dev(c.view_entry), C).sum()) == 0


def test_labels_voted_then_rendered_come_back(env):
    """lift_labels -> render_rows -> Rendered.labels on label maps that are constant per view: every owned pixel carries its view's
    own label wherever the owner voted from that view only"""
    _, sparse = env
    c, C = rr.case("image_11x13"), 7
    P = _dev(c.points)
    ve, M, K = _geometry(c)
    maps = torch.stack([torch.full((c.H, c.W), v % C, dtype=torch.int64) for v in range(c.V)]).cuda()
    voted = sparse.lift_labels(P, sparse.LabelViews(maps, ve, M, K, "render"), num_classes=C, cut_bound=c.cut, fill=False)
    r = _render(sparse, c, "render", 0)
    painted = r.labels(voted.labels)
    checked = 0
    for v in range(c.V):
        own = r.rows[v] >= 0
        single = own & (voted.votes[r.rows[v].clamp(min=0).long()].sum(-1) == 1)         # the owner is a candidate of v: its one vote is v's
        assert bool((painted[v][single] == v % C).all()) and bool((painted[v][~own] == 255).all())
        checked += int(single.sum())
    assert checked > 0
