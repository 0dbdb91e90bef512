"""The geometry channels on the GPU (csrc/normals.hip): sparse.mesh_normals, ops.knn_normals and sparse.estimate_normals against the
references of tests/normals_cases.py.

Bounds.  mesh_normals is the reference's arithmetic, one rounding per operation in the points' dtype: every comparison is on bit
patterns (np.array_equal on the integer views).  ops.knn_normals computes in fp64 and rounds to fp32 last; on rows whose relative
eigenvalue gap (l1 - l0) / l2 is at least 1e-3 an fp64 eigenvector is good to about 1e-11 and rounding a component of magnitude at
most 1 to fp32 moves it by at most 2^-25, so max |n_gpu - n_ref| <= 2^-23 leaves a factor of four; |variation_gpu - variation_ref| <=
2^-23 wherever l2 > 0; every row, degenerate ones included, is finite and unit within 2^-22 (normals_cases.compare_knn_normals; the
rows outside the margins are at most 1 % of the corner cases, asserted on the CPU).  estimate_normals is a composition: bit patterns
against the same calls made by hand.
"""
import numpy as np
import pytest
import torch

import extent_fence
import normals_cases as nc

pytestmark = pytest.mark.gpu

TORCH_OF = {np.float32: torch.float32, np.float64: torch.float64}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import _lib, ops, sparse
    _lib.load()
    return ops, sparse


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mesh(sparse, points, faces):
    return sparse.mesh_normals(_dev(points), _dev(faces)).cpu().numpy()


# ------------------------------------------------------------------------------------------ mesh normals
@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("name", nc.MESH_CASES)
def test_mesh_normals_are_the_loop_bit_for_bit(env, name, dtype):
    _, sparse = env
    mesh = nc.mesh_case(name)
    P = mesh.cast(dtype)
    want = nc.mesh_reference(P, mesh.faces)
    got = sparse.mesh_normals(_dev(P), _dev(mesh.faces))
    assert got.dtype == TORCH_OF[dtype] and got.shape == (len(P), 3) and got.is_contiguous() and not got.requires_grad
    assert np.array_equal(nc.bits(got.cpu().numpy()), nc.bits(want)), name
    again = sparse.mesh_normals(_dev(P), _dev(mesh.faces.astype(np.int32)))          # a second run, the faces as int32: the same bits
    assert np.array_equal(nc.bits(again.cpu().numpy()), nc.bits(want)), name


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_three_entries_in_one_call_are_three_calls(env, dtype):
    _, sparse = env
    parts, rows = nc.three_parts()
    whole = nc.mesh_case("three")
    got = _mesh(sparse, whole.cast(dtype), whole.faces)
    for part, r in zip(parts, rows):
        alone = _mesh(sparse, part.cast(dtype), part.faces)
        assert np.array_equal(nc.bits(got[r]), nc.bits(alone))


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_face_order_is_honoured_not_hidden(env, dtype):
    _, sparse = env
    mesh = nc.mesh_case("grid")
    P = mesh.cast(dtype)
    base = _mesh(sparse, P, mesh.faces)
    keep = nc.order_preserving_permutation(mesh.faces, np.random.default_rng(5))
    assert np.array_equal(nc.bits(_mesh(sparse, P, mesh.faces[keep])), nc.bits(base))
    shuffled = np.random.default_rng(6).permutation(len(mesh.faces))
    want = nc.mesh_reference(P, mesh.faces[shuffled])
    assert (nc.bits(want) != nc.bits(base)).any()
    assert np.array_equal(nc.bits(_mesh(sparse, P, mesh.faces[shuffled])), nc.bits(want))


def test_mesh_normals_refusals(env):
    _, sparse = env
    mesh = nc.mesh_case("three")
    P, Fc = _dev(mesh.cast(np.float32)), _dev(mesh.faces)
    n = P.shape[0]
    for bad_p, bad_f in ((P[:, :3], Fc), (P.half(), Fc), (P.long(), Fc), (P[:0], Fc), (P, Fc[:, :2]), (P, Fc.float()), (P, Fc.reshape(-1)),
                         (P, Fc[:0]), (P.cpu(), Fc), (P, Fc.cpu()), (P.cpu(), Fc.cpu())):
        with pytest.raises(ValueError, match="mesh_normals"):
            sparse.mesh_normals(bad_p, bad_f)
    with pytest.raises(ValueError, match="no faces"):
        sparse.mesh_normals(P, Fc[:0])

    def refused(points, faces, match):
        with pytest.raises(ValueError, match=match):
            sparse.mesh_normals(points, faces)

    f = Fc.clone()
    f[5, 1] = n
    refused(P, f, "1 faces have an index outside")
    f = Fc.clone()
    f[7, 2] = -1
    refused(P, f, "1 faces have an index outside")
    other = int((P[:, 0] != P[Fc[3, 0], 0]).nonzero()[0, 0])                         # a row of another entry
    f = Fc.clone()
    f[3, 2] = other
    refused(P, f, "1 faces name rows of different batch entries")
    for value, match in ((-1.0, "batch index"), (0.5, "batch index"), (65536.0, "batch index")):
        p = P.clone()
        p[11, 0] = value
        refused(p, Fc, match)
    for value in (float("nan"), float("inf")):
        p = P.clone()
        p[13, 2] = value
        refused(p, Fc, "not finite")


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_mesh_normals_stay_inside_their_extents(env, dtype):
    """points, faces, normals, the status and a workspace of exactly the reported bytes inside poisoned guards"""
    ops, _ = env
    mesh = nc.mesh_case("three")
    P = mesh.cast(dtype)
    n, nf, tdt = len(P), len(mesh.faces), TORCH_OF[dtype]
    idt = torch.int32 if dtype == np.float32 else torch.int64                        # (the fences hold the floats as integers)

    def case(a):
        pts = a.inp(torch.from_numpy(P).view(idt), name="points").view(tdt)
        faces = a.inp(torch.from_numpy(mesh.faces), name="faces")
        buffers = {"normals": a.out(n * 3, idt, name="normals").view(tdt).view(n, 3), "status": a.out(8, torch.int64, name="status")}
        ws = a.out(ops.mesh_normals_workspace_bytes(n, nf, tdt), torch.uint8, name="workspace")
        normals, status = ops.mesh_normals_batched(pts, faces, buffers=buffers, workspace=ws)
        return {"normals": normals.view(idt), "status": status}

    got = extent_fence.run(case)
    assert np.array_equal(got["normals"].cpu().numpy(), nc.bits(nc.mesh_reference(P, mesh.faces)))
    assert got["status"].tolist() == [0, 0, 0, 2, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------ normals from neighbour lists
def _knn_normals(ops, P, nbr, toward=None, rows=None, pitched=False, index=torch.int64):
    """-> (normals, variation, status) as numpy; pitched: the positions as columns 2..4 of a wider tensor, read in place"""
    pos = torch.from_numpy(P)
    if pitched:
        wide = torch.full((len(P), 9), float("nan"), dtype=pos.dtype)
        wide[:, 2:5] = pos
        pos = wide.cuda()[:, 2:5]
        assert not pos.is_contiguous()
    else:
        pos = pos.cuda()
    status = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    n, v = ops.knn_normals(pos, torch.from_numpy(nbr).to(index).cuda(), None if toward is None else _dev(toward),
                           None if rows is None else _dev(rows), buffers={"status": status})
    assert n.dtype == torch.float32 and v.dtype == torch.float32 and n.shape == (len(P), 3) and v.shape == (len(P),)
    return n.cpu().numpy(), v.cpu().numpy(), status.tolist()


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("name", list(nc.CORNER_CASES))
def test_knn_normals_on_the_corner(env, name, dtype):
    ops, _ = env
    c = nc.knn_case(name)
    P = np.ascontiguousarray(c.positions.astype(dtype))              # rounded first: the reference sees what the kernel sees
    ref = nc.knn_normals_reference(P, c.neighbors)
    first = None
    for pitched in (False, True):
        for index in (torch.int64, torch.int32):
            n, v, status = _knn_normals(ops, P, c.neighbors, pitched=pitched, index=index)
            assert status == [0, 0]
            exact, loose, skipped = nc.compare_knn_normals(n, v, ref, (name, pitched, index))
            assert exact > 0.98 * len(P)
            if first is None:
                first = (n, v)
            assert np.array_equal(n.view(np.int32), first[0].view(np.int32)) and np.array_equal(v.view(np.int32), first[1].view(np.int32))
    for per_row in (False, True):
        t, tr = nc.viewpoints(c, np.random.default_rng(3), per_row)
        ref_t = nc.knn_normals_reference(P, c.neighbors, t, tr)
        n, v, status = _knn_normals(ops, P, c.neighbors, t, tr)
        assert status == [0, 0]
        nc.compare_knn_normals(n, v, ref_t, (name, "toward", per_row))
        assert np.array_equal(v.view(np.int32), first[1].view(np.int32))             # the sign rule does not touch the variation
        assert np.array_equal(np.abs(n).view(np.int32), np.abs(first[0]).view(np.int32))
        n32, _, _ = _knn_normals(ops, P, c.neighbors, t.astype(np.float32), tr.astype(np.int32))
        ref32 = nc.knn_normals_reference(P, c.neighbors, t.astype(np.float32), tr)
        nc.compare_knn_normals(n32, v, ref32, (name, "toward fp32 / i32", per_row))


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("name", ["line", "lattice", "point"])
def test_knn_normals_degenerate_rows_are_unit_vectors(env, name, dtype):
    ops, _ = env
    c = nc.knn_case(name)
    P = np.ascontiguousarray(c.positions.astype(dtype))
    ref = nc.knn_normals_reference(P, c.neighbors)
    n, v, status = _knn_normals(ops, P, c.neighbors)
    assert status == [0, 0]
    nc.compare_knn_normals(n, v, ref, name)                          # finite, unit, the variation; the vector where it is defined
    if name == "lattice":
        assert np.abs(n - np.array([0, 0, 1], np.float32)).max() <= nc.EIG_TOL and not v.any()
    if name == "point":
        assert not v.any()
    t, tr = nc.viewpoints(c, np.random.default_rng(4), True)
    n, v, _ = _knn_normals(ops, P, c.neighbors, t, tr)
    nc.compare_knn_normals(n, v, nc.knn_normals_reference(P, c.neighbors, t, tr), (name, "toward"))


def test_knn_normals_bad_index_is_counted_and_zero(env):
    ops, _ = env
    c = nc.knn_case("bad_index")
    P = np.ascontiguousarray(c.positions.astype(np.float32))
    ref = nc.knn_normals_reference(P, c.neighbors)
    for index in (torch.int64, torch.int32):
        n, v, status = _knn_normals(ops, P, c.neighbors, index=index)
        assert status == [1, 0]
        assert not n[37].any() and v[37] == 0
        nc.compare_knn_normals(n, v, ref, "bad_index")
    nbr = c.neighbors.copy()
    nbr[37, 5] = -1
    nbr[200, 0] = 2 ** 40
    n, v, status = _knn_normals(ops, P, nbr)
    assert status == [2, 0] and not n[[37, 200]].any()
    t, tr = nc.viewpoints(nc.knn_case("corner24_k16"), np.random.default_rng(3), False)
    tr = tr.copy()
    tr[[3, 99]] = [2, -1]                                            # a viewpoint row outside toward
    n, v, status = _knn_normals(ops, P, nc.knn_case("corner24_k16").neighbors, t, tr)
    assert status == [0, 2] and not n[[3, 99]].any() and not v[[3, 99]].any() and n[4].any()


def test_knn_normals_refusals(env):
    ops, _ = env
    c = nc.knn_case("corner24_k16")
    P, nbr = _dev(c.positions), _dev(c.neighbors)
    n = len(c.positions)
    t, tr = torch.zeros((2, 3), device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    for args in ((P[:, :2], nbr), (P.half(), nbr), (P.cpu(), nbr), (P, nbr[:, :2]), (P, nbr.float()), (P, nbr[:-1]), (P.t().contiguous().t(), nbr),
                 (P, nbr, t), (P, nbr, None, tr), (P, nbr, t[:, :2], tr), (P, nbr, t, tr[:-1]), (P, nbr, t, tr.float()),
                 (P, torch.cat([nbr] * 8, 1))):
        with pytest.raises(ValueError, match="knn_normals"):
            ops.knn_normals(*args)


def test_knn_normals_stay_inside_their_extents(env):
    """pitched positions, the lists, toward and its rows, and the three outputs inside poisoned guards"""
    ops, _ = env
    c = nc.knn_case("corner40_k16")
    P = np.ascontiguousarray(c.positions.astype(np.float32))
    n = len(P)
    t, tr = nc.viewpoints(c, np.random.default_rng(3), False)

    def case(a):
        pos = a.inp(torch.from_numpy(P), pitch=8, name="positions")
        nbr = a.inp(torch.from_numpy(c.neighbors), name="neighbors")
        buffers = {"normals": a.out(n * 3, torch.float32, name="normals").view(n, 3), "variation": a.out(n, torch.float32, name="variation"),
                   "status": a.out(2, torch.int64, name="status")}
        # (toward is converted to fp64 by the wrapper: a copy of its own; the rows are handed over as they are)
        normals, variation = ops.knn_normals(pos, nbr, _dev(t), a.inp(torch.from_numpy(tr), name="toward_rows"), buffers=buffers)
        return {"normals": normals, "variation": variation, "status": buffers["status"]}

    got = extent_fence.run(case)
    assert extent_fence.unwritten(got["normals"]) == 0 and extent_fence.unwritten(got["variation"]) == 0
    assert got["status"].tolist() == [0, 0]
    nc.compare_knn_normals(got["normals"].cpu().numpy(), got["variation"].cpu().numpy(), nc.knn_normals_reference(P, c.neighbors, t, tr), "fenced")


# ------------------------------------------------------------------------------------------ estimate_normals
VOXEL, K = 0.05, 16


@pytest.fixture(scope="module")
def two_entries():
    """two corners, the second turned and moved, their rows interleaved -> points f64 [N,4]"""
    a = nc.corner_points(np.random.default_rng(31), 24)
    b = nc.corner_points(np.random.default_rng(32), 24)[:, [2, 0, 1]] * [1.0, -1.0, 1.0] + [0.3, 0.1, -0.2]
    pts = np.concatenate([np.column_stack([np.zeros(len(a)), a]), np.column_stack([np.ones(len(b)), b])])
    return pts[np.random.default_rng(33).permutation(len(pts))]


def _by_hand(ops, sparse, P, toward):
    q = sparse.quantize(P, P[:, 1:].float(), mode="average", quantization_size=VOXEL)
    nbr = sparse.knn(q.coordinates, K)
    rows = None if toward is None else (q.unique_index if toward.shape[0] == P.shape[0] else q.coordinates[:, 0].long())
    vn, vv = ops.knn_normals(q.features, nbr, toward, rows)
    return q, vn, vv


def _b(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("toward", [None, "entry", "point"])
def test_estimate_normals_is_its_composition(env, two_entries, toward, dtype):
    ops, sparse = env
    P = _dev(two_entries).to(dtype)
    N = P.shape[0]
    if toward == "entry":
        t = torch.tensor([[0.5, 0.6, 0.4], [0.9, -0.3, 0.2]], dtype=torch.float64, device="cuda")
    elif toward == "point":
        t = (P[:, 1:] + torch.randn((N, 3), device="cuda", dtype=dtype)).float()
    else:
        t = None
    q, vn, vv = _by_hand(ops, sparse, P, t)
    before = ops.READBACK["calls"]
    got = sparse.estimate_normals(P, quantization_size=VOXEL, k=K, toward=t)
    calls = ops.READBACK["calls"] - before
    assert isinstance(got, sparse.Normals)
    assert got.normals.shape == (N, 3) and got.variation.shape == (N,) and got.normals.dtype == torch.float32 and not got.normals.requires_grad
    assert torch.equal(_b(got.voxel_normals), _b(vn)) and torch.equal(_b(got.voxel_variation), _b(vv))
    assert torch.equal(_b(got.positions), _b(q.features)) and torch.equal(got.quantized.coordinates, q.coordinates)
    assert torch.equal(got.quantized.inverse_mapping, q.inverse_mapping)
    assert torch.equal(_b(got.normals), _b(vn[q.inverse_mapping])) and torch.equal(_b(got.variation), _b(vv[q.inverse_mapping]))
    norm = got.normals.double().norm(dim=1)
    assert float((norm - 1).abs().max()) <= nc.UNIT_TOL
    if t is not None:                                                # oriented: towards the target, up to the margin of a tie
        target = t.double()[q.coordinates[:, 0].long()] if toward == "entry" else t.double()[q.unique_index]
        d = target - q.features.double()
        assert bool(((vn.double() * d).sum(1) >= -nc.SIGN_MARGIN * d.norm(dim=1)).all())
    # quantized=q: the same bits, and quantize's read-backs saved (at least the one of its status)
    before = ops.READBACK["calls"]
    sparse.quantize(P, None, quantization_size=VOXEL)
    quantize_calls = ops.READBACK["calls"] - before
    q_other = sparse.quantize(P, torch.randn((N, 5), device="cuda"), mode="subsample", quantization_size=VOXEL)
    before = ops.READBACK["calls"]
    again = sparse.estimate_normals(P, quantization_size=VOXEL, k=K, toward=t, quantized=q_other)
    calls_q = ops.READBACK["calls"] - before
    assert quantize_calls >= 1 and calls - calls_q == quantize_calls
    assert again.quantized is q_other
    for f in ("normals", "variation", "voxel_normals", "voxel_variation", "positions"):
        assert torch.equal(_b(getattr(again, f)), _b(getattr(got, f))), f


def test_overlapping_entries_do_not_see_each_other(env):
    _, sparse = env
    a = nc.corner_points(np.random.default_rng(31), 24)
    one = _dev(np.column_stack([np.zeros(len(a)), a]))
    # rows 2 i and 2 i + 1 are point i in entry 0 and in entry 1: interleaved, and every voxel's points in the order of the single call
    both = torch.stack([one, one + torch.tensor([1.0, 0, 0, 0], dtype=torch.float64, device="cuda")], 1).reshape(-1, 4)
    alone = sparse.estimate_normals(one, quantization_size=VOXEL, k=K)
    got = sparse.estimate_normals(both, quantization_size=VOXEL, k=K)
    nv = alone.voxel_normals.shape[0]
    assert got.voxel_normals.shape[0] == 2 * nv
    for b in (0, 1):
        sel = got.quantized.coordinates[:, 0] == b
        assert torch.equal(got.quantized.coordinates[sel][:, 1:], alone.quantized.coordinates[:, 1:])
        assert torch.equal(_b(got.voxel_normals[sel]), _b(alone.voxel_normals)) and torch.equal(_b(got.voxel_variation[sel]), _b(alone.voxel_variation))
        assert torch.equal(_b(got.normals[b::2]), _b(alone.normals)) and torch.equal(_b(got.variation[b::2]), _b(alone.variation))


def test_scene_normals_agree_with_the_analytic_ones(env):
    """config T of geopurify_amd.synthetic, away from patch borders: the estimated voxel normal against scene.normals up to sign.
    Bound: the worst angle of the numpy reference on this scene, 0.0180402 rad (1.03 degrees, over 716 interior voxels of 1813;
    recomputed by test_normals_cases_host.test_scene_angle_is_the_recorded_one), plus 1e-3 rad."""
    _, sparse = env
    from geopurify_amd import synthetic as syn
    scene = syn.make_scene(syn.CONFIGS["T"], nc.SCENE_SEED)
    P = _dev(np.column_stack([np.zeros(len(scene.coords)), scene.coords]))
    got = sparse.estimate_normals(P, quantization_size=nc.SCENE_VOXEL, k=nc.SCENE_K)
    lists = sparse.knn(got.quantized.coordinates, nc.SCENE_K).cpu().numpy()
    ok, analytic = nc.scene_interior(scene.coords, scene.normals, lists, got.quantized.inverse_mapping.cpu().numpy())
    assert ok.sum() > 300
    worst = nc.angle_up_to_sign(got.voxel_normals.cpu().numpy()[ok], analytic[ok]).max()
    print(f"worst angle over {int(ok.sum())} interior voxels of {len(ok)}: {worst:.7f} rad (the reference: {nc.SCENE_WORST_ANGLE})")
    assert worst <= nc.SCENE_WORST_ANGLE + 1e-3
    # the geometry columns of the chain: per point, unit, the voxel's
    assert torch.equal(_b(got.normals), _b(got.voxel_normals[got.quantized.inverse_mapping]))


def test_estimate_normals_refusals(env, two_entries):
    _, sparse = env
    P = _dev(two_entries)
    N = P.shape[0]
    q = sparse.quantize(P, None, quantization_size=VOXEL)
    for kw in (dict(k=2), dict(k=128), dict(k=True), dict(k=16.0), dict(toward=torch.zeros((2, 4), device="cuda")),
               dict(toward=torch.zeros(3, device="cuda")), dict(toward=torch.zeros((2, 3), dtype=torch.int64, device="cuda")),
               dict(toward=torch.zeros((2, 3))), dict(quantized=sparse.quantize(P[:-1], None, quantization_size=VOXEL)), dict(quantized=q.coordinates)):
        with pytest.raises(ValueError, match="estimate_normals"):
            sparse.estimate_normals(P, **{"quantization_size": VOXEL, **kw})
    with pytest.raises(ValueError, match="estimate_normals"):
        sparse.estimate_normals(P[:, :3], quantization_size=VOXEL)
    with pytest.raises(ValueError, match="beyond"):                  # one viewpoint for two entries
        sparse.estimate_normals(P, quantization_size=VOXEL, toward=torch.zeros((1, 3), device="cuda"))
    with pytest.raises(ValueError, match="voxels"):                  # knn's refusal, unchanged: an entry of k or fewer voxels
        sparse.estimate_normals(P[:40], quantization_size=VOXEL, k=127)
