"""The claims of tests/render_rows_cases.py, checked on the CPU: the reference is the sequential rule, the cases are hard enough that a
kernel which paints every candidate, the last one, or the first to arrive cannot pass, and the argument checks of sparse.render_rows,
Rendered.features, Rendered.labels and segment_views refuse what they must before any kernel runs."""
import numpy as np
import pytest
import torch

import render_depth_cases as rd
import render_rows_cases as rr

BUSY = ("views_130", "image_11x13", "stride")
OWNED_AT_LEAST, HIDDEN_AT_LEAST = 0.45, 0.14


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("kind", rr.KINDS)
@pytest.mark.parametrize("name", rr.CASES)
def test_reference_is_the_sequential_rule(name, kind, radius):
    c = rr.case(name)
    want = rr.reference(name, kind, radius)
    rows, depth, vc, pc = rr.restatement(c, rr._depth_of(kind, c), radius)
    assert want.rows.dtype == rows.dtype == np.int32 and want.depth.dtype == np.float64
    assert np.array_equal(rows, want.rows) and np.array_equal(depth.view(np.int64), want.depth.view(np.int64))
    assert np.array_equal(vc, want.view_count) and np.array_equal(pc, want.pixel_count)
    assert np.array_equal(want.pixel_count, (want.rows >= 0).sum((1, 2))) and ((want.rows == -1) == (want.depth == rr.FAR)).all()


def test_the_sensor_form_and_the_largest_radius():
    c = rr.case("contests")
    for radius in rr.RADII:
        want = rr.render(c, c.notes["sensor"], radius)
        rows, depth, vc, pc = rr.restatement(c, c.notes["sensor"], radius)
        assert np.array_equal(rows, want.rows) and np.array_equal(depth, want.depth) and np.array_equal(vc, want.view_count)
    for name in ("cut_one_pixel", "clip"):                                       # a radius larger than the interior / clipped on all sides
        for kind in rr.KINDS:
            want = rr.reference(name, kind, 4)
            rows, depth, vc, pc = rr.restatement(rr.case(name), rr._depth_of(kind, rr.case(name)), 4)
            assert np.array_equal(rows, want.rows) and np.array_equal(depth, want.depth) and np.array_equal(pc, want.pixel_count)
    one = rr.reference("cut_one_pixel", "render", 4)
    assert (one.rows[:, 5, 5] >= 0).any() and (np.delete(one.rows.reshape(len(one.rows), -1), 5 * 11 + 5, axis=1) == -1).all()
    assert (rr.reference("cut_nothing", "none", 4).rows == -1).all() and (rr.reference("cut_nothing", "none", 4).view_count == 0).all()


def _hidden(ref):
    """the fraction of the candidates that own no pixel"""
    n = sum(len(r) for r in ref.cands)
    owners = sum(len(np.setdiff1d(np.unique(ref.rows[v]), [-1])) for v in range(len(ref.cands)))
    return 1.0 - owners / n


@pytest.mark.parametrize("kind", rr.KINDS)
@pytest.mark.parametrize("name", BUSY)
def test_busy_cases_are_owned_and_contended(name, kind):
    """at radius 0 owners on at least 45 % of the pixels, and at least 14 % of the candidates own nothing: neither painting every
    candidate nor painting the last one can pass"""
    ref = rr.reference(name, kind, 0)
    owned, hidden = float((ref.rows >= 0).mean()), _hidden(ref)
    print(f"{name} / {kind}: {owned:.1%} of the pixels owned, {hidden:.1%} of the candidates hidden")
    assert owned >= OWNED_AT_LEAST and hidden >= HIDDEN_AT_LEAST


def test_stride_contends_in_both_passes():
    c, ref = rr.case("stride"), rr.reference("stride", "none", 0)
    big = [v for v in range(c.V) if c.view_entry[v] == 3]
    # about 13 500 candidates in two views of 192 pixels each, every pixel owned: some 35 atomics per pixel in either pass
    assert c.N > rd.ONE_TRIP + 1 and sum(ref.view_count[v] for v in big) > 13000 and c.H * c.W == 192
    assert all(ref.view_count[v] > 6000 and ref.pixel_count[v] == 192 for v in big)
    # "render" and None differ in their CANDIDATES (view_count), and so in which kernel paths 13 000 hidden points take, but not in
    # their owners while every p_z is > 0.2: a pixel's owner is the nearest point over the pixels within the radius, that is the nearest
    # of those pixels' own nearest points, and a pixel's nearest point is its rendered depth, which passes the depth test.  The owners
    # part where a point lies at 0 < p_z <= 0.2, which the z-buffer ignores: entry 3 of "contests".
    for radius in (0, 1, 2):
        none, rend = rr.reference("stride", "none", radius), rr.reference("stride", "render", radius)
        assert np.array_equal(none.rows, rend.rows) and (none.view_count[big] > 10 * rend.view_count[big]).all()
        assert not np.array_equal(rr.reference("contests", "none", radius).rows, rr.reference("contests", "render", radius).rows)


def test_exact_has_equal_depth_contests():
    """a tie-break by arrival order fails: two or more pixels whose smallest p_z is shared, and the lower row owns them"""
    c = rr.case("exact")
    names = c.notes["row_names"]
    for kind in rr.KINDS:
        ref = rr.reference("exact", kind, 0)
        assert ref.contests >= 2
        a, b = names.index("triple_a"), names.index("triple_b")
        assert ref.rows[0, 3, 4] == ref.rows[2, 3, 4] == min(a, b) and ref.depth[0, 3, 4] == 1.5


def test_twins_change_when_entries_merge():
    c = rr.case("twins")
    for kind in rr.KINDS:
        own, mixed = rr.reference("twins", kind, 0), rr.render(rr.merged(c), rr._depth_of(kind, c), 0)
        for v in range(c.V):
            assert not np.array_equal(own.rows[v], mixed.rows[v]) and not np.array_equal(own.depth[v], mixed.depth[v])


def test_edge_rows_land_where_their_names_say():
    c = rr.case("clip")
    for kind in rr.KINDS:
        ref = rr.reference("clip", kind, 2)
        for (y, x), row in c.notes["expect"][2].items():
            assert ref.rows[0, y, x] == row, (kind, y, x)
        assert (ref.rows[0, :2] == -1).all() and (ref.rows[0, 10:] == -1).all() and (ref.rows[0, :, :2] == -1).all() and (ref.rows[0, :, 14:] == -1).all()
        assert ref.view_count[0] == 7
    c = rr.case("contests")
    r2 = rr.reference("contests", "render", 2).rows
    assert (r2[0, 3:8, 4:7] == 0).all() and (r2[0, 3:8, 2:4] == 2).all() and (r2[0, 3:8, 7:9] == 0).all()     # equal p_z: the lower row where both cover
    r1 = rr.reference("contests", "render", 1)
    assert (r1.rows[1, 4:7, 4:7] == 1).all() and (r1.rows[1, 4:7, 7] == 4).all() and r1.rows[1, 5, 6] == 1      # the far one keeps column 7 only
    assert rr.reference("contests", "render", 0).rows[1, 5, 6] == 4
    for radius in rr.RADII:
        s = rr.render(c, c.notes["sensor"], radius)
        area = (min(8 + radius, 11) - (8 - radius) + 1) * (2 * radius + 1)                 # pixel (8, 8) on 12 x 16: clipped at the bottom only
        assert not (s.rows == 3).any() and s.view_count[2] == 1 and (s.rows[2] == 6).sum() == area           # negative depth: never
        assert s.view_count[3] == 1
    near = rr.reference("contests", "none", 0)
    assert near.rows[3, 6, 8] == 5 and near.depth[3, 6, 8] == 0.125 and near.rows[3, 6, 10] == 7 and near.view_count[3] == 2
    assert (rr.reference("contests", "render", 0).rows[3] == -1).all() and rr.reference("contests", "render", 0).view_count[3] == 0


# ------------------------------------------------------------------------------------------ refusals without a GPU
def _cpu_rendered(sparse, V=2, H=3, W=4, N=5):
    rows = torch.full((V, H, W), -1, dtype=torch.int32)
    return sparse.Rendered(rows, torch.full((V, H, W), rr.FAR, dtype=torch.float64), torch.zeros(V, dtype=torch.int64),
                           torch.zeros(V, dtype=torch.int64), 1, (H, W), N)


def test_refusals_before_any_kernel():
    from geopurify_amd import sparse
    c = rr.case("v1")
    P, E, M, K = (torch.from_numpy(a) for a in (c.points, c.view_entry, c.w2c, c.intr))
    shape = (c.H, c.W)
    with pytest.raises(ValueError, match="there is no CPU path"):
        sparse.render_rows(P, E, M, K, shape)
    with pytest.raises(ValueError, match="there is no CPU path"):
        sparse.render_rows(P, E, M, K, shape, depth=None, radius=2)
    for radius in (5, -1, 1.0, True):
        with pytest.raises(ValueError, match="radius="):
            sparse.render_rows(P, E, M, K, shape, radius=radius)
    with pytest.raises(ValueError, match="the string 'render'"):
        sparse.render_rows(P, E, M, K, shape, depth="rendered")
    for bad in (torch.zeros(c.V, c.H, c.W + 1, dtype=torch.float64), torch.zeros(c.V, c.H, c.W), torch.zeros(c.H, c.W, dtype=torch.float64)):
        with pytest.raises(ValueError, match="depth must be fp64"):
            sparse.render_rows(P, E, M, K, shape, depth=bad)
    with pytest.raises(ValueError, match=r"points must be \[N, 4\]"):
        sparse.render_rows(P[:, :3], E, M, K, shape)
    with pytest.raises(ValueError, match="image_shape must be"):
        sparse.render_rows(P, E, M, K, (c.H, 0))
    with pytest.raises(ValueError, match="cut_bound"):
        sparse.render_rows(P, E, M, K, shape, cut_bound=-1)
    r = _cpu_rendered(sparse)
    feats = torch.zeros(5, 8)
    with pytest.raises(ValueError, match="dtype=torch.float64"):
        r.features(feats, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"index must be an int64 tensor \[5\]"):
        r.features(torch.zeros(3, 8), index=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"index must be an int64 tensor \[5\]"):
        r.features(torch.zeros(3, 8), index=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="rows_features must be fp32"):
        r.features(feats.double())
    with pytest.raises(ValueError, match="4 feature rows for 5 points"):
        r.features(feats[:4])
    with pytest.raises(ValueError, match="views must be"):
        r.features(feats, views=1.5)
    with pytest.raises(ValueError, match="there is no CPU path"):
        r.features(feats)
    with pytest.raises(ValueError, match=r"index must be an int64 tensor \[5\]"):
        r.labels(torch.zeros(3, dtype=torch.int64), index=torch.zeros(6, dtype=torch.int64))
    with pytest.raises(ValueError, match="point_labels must be an integer tensor"):
        r.labels(torch.zeros(5))
    assert r.labels(torch.arange(5, dtype=torch.uint8)).tolist() == torch.full((2, 3, 4), 255, dtype=torch.uint8).tolist()   # torch indexing only
    maps, ve, pred = torch.zeros(2, 3, 4, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="there is no CPU path"):
        sparse.segment_views(r, pred, maps, ve, 4)
    with pytest.raises(ValueError, match=r"index must be an int64 tensor \[5\]"):
        sparse.segment_views(r, pred[:3], maps, ve, 4, index=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="label_maps must be"):
        sparse.segment_views(r, pred, maps.float(), ve, 4)
    with pytest.raises(ValueError, match="label_maps must be"):
        sparse.segment_views(r, pred, maps[:, :2], ve, 4)
    with pytest.raises(ValueError, match="num_classes"):
        sparse.segment_views(r, pred, maps, ve, 0)
    with pytest.raises(ValueError, match="at most 4 ignore labels"):
        sparse.segment_views(r, pred, maps, ve, 4, ignore_labels=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="rendered must be a Rendered"):
        sparse.segment_views(None, pred, maps, ve, 4)


def test_the_workspace_query_needs_no_gpu():
    from geopurify_amd import _lib, ops
    lib = _lib.load()
    sizes = [lib.gp_render_rows_workspace_bytes(1000, 7, 12, 16, mode) for mode in (0, 1, 2)]
    assert sizes[0] > 0 and sizes[0] == sizes[1] and sizes[2] >= sizes[0] + 7 * 12 * 16 * 8
    assert ops.render_rows_workspace_bytes(1000, 7, (12, 16), "render") == sizes[2]
    for n, v, h, w, mode in ((0, 7, 12, 16, 0), (1000, 0, 12, 16, 0), (1000, 7, 0, 16, 2), (1000, 7, 12, 16, 3), (2 ** 31, 7, 12, 16, 0)):
        assert lib.gp_render_rows_workspace_bytes(n, v, h, w, mode) == 0
