"""The claims of tests/render_depth_cases.py, checked on the CPU: the reference is the reference's sequential loop, the edge rows land
where their names say, and the rendered depth hides enough of what depth=None keeps for the lift tests to tell the two apart."""
import numpy as np
import pytest

import render_depth_cases as rd


@pytest.mark.parametrize("name", rd.CASES + rd.OPS_ONLY)
def test_reference_is_the_sequential_loop(name):
    """oracle.project.render_depth (np.minimum.at) against `if p2 > 0.2 and inside and depth[v, u] > p2` point by point, bit for bit"""
    c = rd.case(name)
    if c.N > 2000:                                                               # "stride": the loop over its first and last rows per entry
        keep = np.zeros(c.N, bool)
        keep[:600] = keep[-600:] = True
        c = rd.RCase(c.name, c.points[keep], c.view_entry, c.w2c, c.intr, c.H, c.W, c.cut)
        want = rd.render(c)
    else:
        want = rd.reference(name)
    got = rd.restatement(c)
    assert got.dtype == want.dtype == np.float64 and got.shape == (c.V, c.H, c.W)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


def test_shapes_the_cases_promise():
    assert rd.reference("image_11x13").size % 2 == 1                             # the fill's scalar tail
    assert rd.case("stride").N > rd.ONE_TRIP + 1 and len(rd.case("stride").rows_of(1)) == 1
    assert len(rd.case("entries").rows_of(0)) == 1 and set(np.unique(rd.case("entries").points[:, 0])) == {0, 2, 65535}
    c = rd.case("no_points_no_views")
    assert len(c.rows_of(3)) == 0 and (c.view_entry == 3).sum() == 2 and len(c.rows_of(1)) == 30 and not (c.view_entry == 1).any()
    assert (rd.reference("no_points_no_views")[c.view_entry == 3] == rd.FAR).all()
    assert rd.case("v1").V == 1 and rd.case("views_130").V == 132
    one = rd.reference("cut_one_pixel")
    inner = one[:, 5, 5].copy()
    assert (inner < rd.FAR).any() and (np.delete(one.reshape(len(one), -1), 5 * 11 + 5, axis=1) == rd.FAR).all()
    assert (rd.reference("cut_nothing") == rd.FAR).all()
    c = rd.case("ordered")
    assert (np.diff(c.points[:, 0]) >= 0).all() and (np.diff(rd.case("entries").points[:, 0]) < 0).any()


def test_twins_would_differ_if_entries_mixed():
    c, ref = rd.case("twins"), rd.reference("twins")
    assert np.array_equal(ref[0], ref[3]) and np.array_equal(ref[1], ref[2])
    both = (ref[0] < rd.FAR) & (ref[1] < rd.FAR)
    assert both.sum() >= 10 and (ref[1][both] != ref[0][both]).all()             # pixels that both entries hit, at different depths
    mixed = rd.render(rd.RCase("mixed", np.column_stack([np.zeros(c.N), c.points[:, 1:]]), [0], c.w2c[:1], c.intr[:1], c.H, c.W))
    assert (mixed[0] != ref[0]).sum() >= 10 and (mixed[0] != ref[1]).sum() >= 10


def test_exact_rows_land_where_their_names_say():
    c, ref = rd.case("exact"), rd.reference("exact")
    for v, pixels in c.notes["expect"].items():
        for (row, col), z in pixels.items():
            assert ref[v, row, col] == z, (v, row, col, ref[v, row, col], z)
    assert np.array_equal(ref[0], ref[2])
    assert np.nextafter(rd.Z_EDGE, 1.0) > rd.Z_EDGE and ref[0, 6, 11] - rd.Z_EDGE < 1e-16


def test_bad_rows_and_views_render_nothing():
    c, ref = rd.case("bad"), rd.reference("bad")
    bad_views = (c.view_entry < 0) | (c.view_entry > 65535)
    assert bad_views.sum() == c.notes["bad_views"] and (ref[bad_views] == rd.FAR).all() and (ref[~bad_views] < rd.FAR).any()
    b = c.points[:, 0]
    finite = np.isfinite(c.points).all(1)
    bad = finite & ~((b >= 0) & (b <= 65535) & (b == np.floor(b)))
    assert bad.sum() == c.notes["bad_rows"] and (~finite).sum() == c.notes["nonfinite_rows"]
    # every bad row would be rendered (nearest in its pixel, in a view of a valid entry) if it were given to entry 0
    moved = c.points.copy()
    moved[bad | ~finite, 0] = 0.0
    assert not np.array_equal(rd.render(rd.RCase("moved", moved, c.view_entry, c.w2c, c.intr, c.H, c.W))[0], ref[0])


@pytest.mark.parametrize("name", rd.LIFT_CASES)
def test_rendered_depth_hides_what_none_keeps(name):
    """the occlusion condition: of the (point, view) pairs that depth=None keeps, the rendered depth hides at least 10 % and leaves at
    least 25 % -- so a lift that treated "render" as None, or as "nothing visible", fails the lift tests"""
    c = rd.lift_case(name)
    assert c.depth is None
    g = rd.of_lift_case(c)
    none, rendered = rd.pairs(g, None, c.tau), rd.pairs(g, rd.lift_depth(name), c.tau)
    assert not (rendered & ~none).any()
    hidden, kept = int((none & ~rendered).sum()), int(none.sum())
    print(f"{name}: depth=None keeps {kept} pairs, the rendered depth hides {hidden} ({hidden / kept:.1%})")
    assert hidden >= rd.HIDDEN_AT_LEAST * kept and int(rendered.sum()) >= rd.VISIBLE_AT_LEAST * kept
    # ... and the lift itself differs: counts, and for the drop rule of lift_views_70 the kept views
    import lift_batched_cases as lb
    with_d = lb._reference(rd.with_depth(c, rd.lift_depth(name)))
    without = lb._reference(c)
    assert not np.array_equal(with_d.count, without.count)
    if c.min_visible:
        assert with_d.view_keep.any() and not with_d.view_keep.all() and not np.array_equal(with_d.view_keep, without.view_keep)


# ------------------------------------------------------------------------------------------ the package, as far as a CPU goes
def test_the_library_sizes_the_workspaces_without_a_gpu():
    from geopurify_amd import _lib
    lib = _lib.load()
    n, V = 150_000, 100
    one, state = lib.gp_render_depth_batched_workspace_bytes(n, V), lib.gp_render_depth_batched_state_workspace_bytes(n, V)
    assert one > 16 * n and 8 * n <= state < one                                 # the one-call form sorts, the state form copies the tables
    for bad in ((0, V), (2 ** 31, V), (n, 0), (n, 65536)):
        assert lib.gp_render_depth_batched_workspace_bytes(*bad) == 0 and lib.gp_render_depth_batched_state_workspace_bytes(*bad) == 0


def test_refusals_need_no_gpu():
    """the checks of sparse.render_depth and of depth=<str> run before any tensor is touched on a device"""
    import torch

    from geopurify_amd import sparse
    c = rd.lift_case("lift_nearest")
    P, ve, M, K = (torch.from_numpy(a) for a in (c.points, c.view_entry, c.w2c, c.intr))
    with pytest.raises(ValueError, match="no CPU path"):
        sparse.render_depth(P, ve, M, K, (c.H, c.W))
    with pytest.raises(ValueError, match="image_shape must be"):
        sparse.render_depth(P, ve, M, K, (c.H, 0))
    maps = torch.from_numpy(c.maps)
    for word in ("rendered", "RENDER", ""):
        with pytest.raises(ValueError, match="the string 'render'"):
            sparse.lift(P, sparse.Views(maps, ve, M, K, word))
    with pytest.raises(ValueError, match="no CPU path"):                          # "render" itself passes the check of the field
        sparse.lift(P, sparse.Views(maps, ve, M, K, "render"))
    with pytest.raises(ValueError, match="no CPU path"):
        sparse.LiftStream(P, feature_dim=c.D)
