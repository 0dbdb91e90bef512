"""The cases and references of tests/normals_cases.py, checked on the CPU: the restated vertex-normal loop against the golden of the
reference's own function (bit for bit), the batched reference against the loop, every condition the GPU tests rely on (valences,
degenerate faces, the two kinds of face permutation, the share of rows the eigenvector and sign margins exclude), and the recorded
worst angle of the scene test."""
import os

import numpy as np
import pytest

import normals_cases as nc


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ref_vertex_normal.npz"))


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("name", ["grid", "fan65", "odd"])
def test_loop_is_the_reference_bit_for_bit(golden, name, dtype):
    tag = np.dtype(dtype).name
    mesh = nc.mesh_case(name)
    vertex = np.ascontiguousarray(mesh.cast(dtype)[:, 1:])
    assert np.array_equal(golden[f"{name}_face"], mesh.faces)
    assert np.array_equal(nc.bits(golden[f"{name}_{tag}_vertex"]), nc.bits(vertex))
    want = golden[f"{name}_{tag}_normal"]
    assert want.dtype == dtype and 250 <= len(nc.mesh_case("grid").points) <= 400
    got = nc.vertex_normal_loop(vertex, mesh.faces)
    assert got.dtype == dtype
    assert np.array_equal(nc.bits(got), nc.bits(want))
    # and the batched reference on a single entry is the loop
    assert np.array_equal(nc.bits(nc.mesh_reference(mesh.cast(dtype), mesh.faces)), nc.bits(want))


def test_mesh_cases_hold_what_they_promise():
    grid = nc.mesh_case("grid")
    assert 250 <= len(grid.points) <= 400 and len(grid.points) > 256 and len(grid.faces) > 256     # more than one block of each kernel
    v65, v300 = (nc.valence(nc.mesh_case(n).faces, len(nc.mesh_case(n).points)) for n in ("fan65", "fan300"))
    assert 64 < v65.max() <= 256 and v300.max() > 256
    odd = nc.mesh_case("odd")
    val = nc.valence(odd.faces, len(odd.points))
    assert (val == 0).sum() >= 2 and (val == 1).sum() >= 3
    c = nc.face_contributions(np.ascontiguousarray(odd.points[:, 1:]), odd.faces)
    twice = np.array([len(set(f.tolist())) < 3 for f in odd.faces])
    zero_area = ~c.any(1)
    assert twice.sum() >= 2 and (zero_area & ~twice).sum() >= 2                                     # coincident and collinear corners
    rows, counts = np.unique(odd.faces, axis=0, return_counts=True)
    assert counts.max() >= 2                                                                        # a face listed more than once
    ref = nc.mesh_reference(odd.points, odd.faces)
    assert not ref[val == 0].any() and np.isfinite(ref).all()
    three = nc.mesh_case("three")
    assert sorted(np.unique(three.points[:, 0]).tolist()) == [0.0, 1.0, 2.0]
    assert (np.diff(three.points[:, 0]) != 0).sum() > 20                                            # rows interleaved
    fe = three.points[three.faces[:, 0], 0]
    assert (np.diff(fe) != 0).sum() > 20                                                            # faces interleaved


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_three_entries_are_three_meshes(dtype):
    parts, rows = nc.three_parts()
    whole = nc.mesh_case("three")
    ref = nc.mesh_reference(whole.cast(dtype), whole.faces)
    for part, r in zip(parts, rows):
        alone = nc.vertex_normal_loop(np.ascontiguousarray(part.cast(dtype)[:, 1:]), part.faces)
        assert np.array_equal(nc.bits(ref[r]), nc.bits(alone))


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_the_two_kinds_of_face_permutation(dtype):
    mesh = nc.mesh_case("grid")
    P = mesh.cast(dtype)
    base = nc.mesh_reference(P, mesh.faces)
    n = len(P)
    keep = nc.order_preserving_permutation(mesh.faces, np.random.default_rng(5))
    assert (keep != np.arange(len(keep))).sum() >= 20
    assert nc.vertex_orders(mesh.faces[keep], n) == nc.vertex_orders(mesh.faces, n)
    assert np.array_equal(nc.bits(nc.mesh_reference(P, mesh.faces[keep])), nc.bits(base))
    shuffled = np.random.default_rng(6).permutation(len(mesh.faces))
    assert nc.vertex_orders(mesh.faces[shuffled], n) != nc.vertex_orders(mesh.faces, n)
    moved = nc.mesh_reference(P, mesh.faces[shuffled])
    assert (nc.bits(moved) != nc.bits(base)).any(), "the order of a vertex's faces does not show in this case's bits"
    assert np.abs(moved.astype(np.float64) - base).max() < (1e-5 if dtype == np.float32 else 1e-13)


# ------------------------------------------------------------------------------------------ neighbour-list normals
@pytest.mark.parametrize("toward", [None, "entry", "row"])
def test_margins_exclude_at_most_one_percent_of_the_corner_rows(toward):
    excluded = total = 0
    for name in nc.CORNER_CASES:
        c = nc.knn_case(name)
        n, k = c.neighbors.shape
        assert n % 64 != 0 and n > nc.CORNER_CASES[name][1]
        for dtype in nc.DTYPES:
            P = c.positions.astype(dtype)
            t, tr = (None, None) if toward is None else nc.viewpoints(c, np.random.default_rng(3), toward == "row")
            ref = nc.knn_normals_reference(P, c.neighbors, t, tr)
            excluded += int(((ref.gap < nc.EIG_GAP) | ref.sign_free).sum())
            total += n
            assert np.abs(np.linalg.norm(ref.normals.astype(np.float64), axis=1) - 1).max() <= nc.UNIT_TOL
            nc.compare_knn_normals(ref.normals, ref.variation, ref, name)          # the comparison accepts the reference itself
    assert excluded <= 0.01 * total, (excluded, total)
    sizes = [len(nc.knn_case(name).positions) for name in nc.CORNER_CASES]
    assert max(sizes) > 256 and min(sizes) > 127                                   # more than one block of 256 rows; k = 127 fits


def test_the_corner_normals_are_the_planes():
    """away from the two edges the direction of least spread is the plane's axis: the reference means what it says"""
    c = nc.knn_case("corner40_k16")
    ref = nc.knn_normals_reference(c.positions, c.neighbors)
    P = c.positions
    for axis in range(3):
        others = [(axis + 1) % 3, (axis + 2) % 3]
        inner = (np.abs(P[:, axis]) < 0.01) & (P[:, others] > 0.25).all(1)
        assert inner.sum() > 50
        assert (np.abs(ref.normals[inner, axis]) > 0.99).all()
        assert (ref.normals[inner, axis] > 0).all()                               # the largest component is positive


def test_degenerate_cases_are_degenerate():
    line = nc.knn_normals_reference(nc.knn_case("line").positions, nc.knn_case("line").neighbors)
    assert (line.gap < nc.EIG_GAP).all() and (line.evals[:, 2] > 0).all()
    lat = nc.knn_case("lattice")
    ref = nc.knn_normals_reference(lat.positions, lat.neighbors)
    assert np.abs(ref.evals[:, 0]).max() == 0 and (np.abs(ref.normals[:, 2]) == 1).all()
    interior = (np.abs(lat.positions[:, :2] - 0.25) < 0.2).all(1)
    assert (np.abs(ref.evals[interior, 1] - ref.evals[interior, 2]) < 1e-15).all()
    pt = nc.knn_normals_reference(nc.knn_case("point").positions, nc.knn_case("point").neighbors)
    assert not pt.evals.any() and not pt.variation.any()
    bad = nc.knn_case("bad_index")
    ref = nc.knn_normals_reference(bad.positions, bad.neighbors)
    assert ref.bad.sum() == 1 and ref.bad[37] and not ref.normals[37].any()


# ------------------------------------------------------------------------------------------ the scene
@pytest.fixture(scope="module")
def scene_reference():
    from geopurify_amd import synthetic as syn
    scene = syn.make_scene(syn.CONFIGS["T"], nc.SCENE_SEED)
    points = np.column_stack([np.zeros(len(scene.coords)), scene.coords])
    ref, cent, lists, inverse, coords = nc.estimate_reference(points, nc.SCENE_VOXEL, nc.SCENE_K)
    ok, analytic = nc.scene_interior(scene.coords, scene.normals, lists, inverse)
    return ref, ok, analytic


def test_scene_angle_is_the_recorded_one(scene_reference):
    ref, ok, analytic = scene_reference
    assert ok.sum() > 0.2 * len(ok) and ok.sum() > 300, (int(ok.sum()), len(ok))
    worst = nc.angle_up_to_sign(ref.normals[ok], analytic[ok]).max()
    print(f"worst angle of the reference over {int(ok.sum())} interior voxels of {len(ok)}: {worst:.6f} rad")
    assert abs(worst - nc.SCENE_WORST_ANGLE) < 1e-6, worst
    assert worst < 0.2                                                             # a loose angle, but an angle: ~11 degrees
