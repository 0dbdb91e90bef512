"""The one-pass look-ahead entries against the chains of calls they replace, bit for bit, inside extent fences.

  fusion with the fill   gp_seen_masks + gp_nn1_masked_f64 + gp_fuse_views_top3_fill  ==  gp_fuse_views_top3 + gp_nn1_masked_f64 +
                         gp_gather_rows(nn >= 0 ? nn : p)
  voxel rows             gp_voxel_rows_operands  ==  gp_scatter_mean_csr x 2 into a zeroed X, gp_split_f16_scaled(per row,
                         interleaved), gp_pow2_scale
  pipeline               HotPath.lift_masks + prepare  ==  the same tensors composed from the old calls in this process
  kNN                    gp_knn_lattice (a first ring of up to 2048 candidates read once)  ==  gp_knn_lattice_two_pass  ==  the exact lists
The cases and what they hold: tests/lookahead_cases.py (checked on the host by test_lookahead_cases_host.py).
"""
import dataclasses

import numpy as np
import pytest
import torch

import lookahead_cases as la
from extent_fence import bits, run, unwritten

pytestmark = pytest.mark.gpu

F32, F16, I32, I64, U8 = torch.float32, torch.float16, torch.int32, torch.int64, torch.uint8


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import ops as _ops
    from geopurify_amd import _lib
    _lib.load()                      # fails loudly if the HIP library is missing
    return _ops


def up(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda().contiguous()


def same(got, want, name):
    x, y = bits(got), bits(want)
    assert x.shape == y.shape, (name, x.shape, y.shape)
    if not torch.equal(x, y):
        at = (x != y).nonzero()[0].tolist()
        raise AssertionError(f"{name}: {int((x != y).sum())} elements differ, first at {at}: {got[tuple(at)].item()} instead of {want[tuple(at)].item()}")


# ------------------------------------------------------------------------------------------ fusion with the fill inside
_OLD_FUSE = {}


def lists(c):
    """(pv_view, pv_seg) on the device; an empty list array still needs an address: one slot that no offset reaches"""
    return tuple(up(c[k]) if len(c[k]) else torch.zeros(1, dtype=I32, device="cuda") for k in ("pv_view", "pv_seg"))


def old_fuse_chain(ops, key, c):
    """(seen, nn, F) of today's chain, computed once per case and left unchanged"""
    if key not in _OLD_FUSE:
        n, d = c["n"], c["d"]
        F = torch.empty((n, d), dtype=F32, device="cuda")
        seen = ops.fuse_views_top3(up(c["start"]), *lists(c), n, up(c["fseg"]), up(c["lseg"]), F)
        nn = ops.nn1_masked(up(c["xyz"]), seen, 1 - seen)
        src = torch.where(nn >= 0, nn, torch.arange(n, device="cuda"))
        _OLD_FUSE[key] = (seen, nn, ops.gather_rows(F, d, src))
    return _OLD_FUSE[key]


@pytest.mark.parametrize("d", la.FUSE_D)
@pytest.mark.parametrize("kind", la.FUSE_KINDS)
def test_fuse_with_fill_equals_fuse_fill_gather(ops, kind, d):
    from geopurify_amd import _lib
    lib = _lib.load()
    c = la.case_fuse_fill(kind, d)
    n = c["n"]
    seen_old, nn_old, F_old = old_fuse_chain(ops, (kind, d), c)
    ref_seen = la.ref_seen(c["start"])
    assert seen_old.cpu().numpy().tolist() == ref_seen.tolist()
    assert nn_old.cpu().numpy().tolist() == la.ref_nn(c["xyz"], ref_seen).tolist()

    def case(a):
        start = a.inp(up(c["start"]), name="pv_start")
        pvv, pvs = (a.inp(t, name=k) for t, k in zip(lists(c), ("pv_view", "pv_seg")))
        fseg, lseg = a.inp(up(c["fseg"]).view(-1, d), name="f_seg"), a.inp(up(c["lseg"]).view(-1, c["C"]), name="logit_seg")
        xyz = a.inp(up(c["xyz"]), name="xyz")
        seen, unseen = a.out(n, U8, name="seen"), a.out(n, U8, name="unseen")
        s = ops._stream()
        ops.check(lib.gp_seen_masks(ops._ptr(start), n, ops._ptr(seen), ops._ptr(unseen), s), "gp_seen_masks")
        nn = ops.nn1_masked(xyz, seen, unseen)
        nn_in = a.inp(nn, name="nn")
        F = a.out((n, d), F32, pitch=d + 4, name="out")
        ops.check(lib.gp_fuse_views_top3_fill(ops._ptr(start), ops._ptr(pvv), ops._ptr(pvs), n, ops._ptr(fseg), ops._ptr(lseg), c["Q"], d, c["C"],
                                              ops._ptr(nn_in), ops._ptr(F), F.stride(0), s), "gp_fuse_views_top3_fill")
        return {"seen": seen, "unseen": unseen, "nn": nn, "F": F}

    got = run(case)
    same(got["seen"], seen_old, "seen")
    same(got["unseen"], 1 - seen_old, "unseen")
    same(got["nn"], nn_old, "nn")
    same(got["F"], F_old, "F")
    assert unwritten(got["F"]) == 0
    if kind in ("none_seen", "single_unseen"):
        assert int(bits(got["F"]).abs().max()) == 0                  # no seen point anywhere: all-zero rows
    if kind == "mixed":
        for name in la.SPECIAL:                                      # a filled row has the bits of the row it copies
            p, t = c["names"].index(name), c["names"].index(name + ".twin")
            same(got["F"][t], got["F"][p], name)


def test_fuse_with_fill_rejects_bad_arguments(ops):
    from geopurify_amd import _lib
    lib = _lib.load()
    z = torch.zeros(64, dtype=I64, device="cuda")
    f = torch.zeros(64, dtype=F32, device="cuda")
    p = ops._ptr
    assert lib.gp_fuse_views_top3_fill(p(z), p(z), p(z), 1, p(f), p(f), 1, 6, 1, p(z), p(f), 8, None) == -22          # d % 4
    assert lib.gp_fuse_views_top3_fill(p(z), p(z), p(z), 1, p(f), p(f), 1, 8, 1, None, p(f), 8, None) == -22          # no nn
    assert lib.gp_seen_masks(p(z), 0, p(z), p(z), None) == -22


# ------------------------------------------------------------------------------------------ voxel rows
_OLD_ROWS = {}


def old_rows_chain(ops, key, c):
    """(X, rows, row_inv, scale2) of today's chain, computed once per case and left unchanged"""
    if key not in _OLD_ROWS:
        nv, d, cp = c["nv"], c["d"], c["cin_pad"]
        order, seg, rm = up(c["order"]), up(c["seg_start"]), up(c["row_map"])
        X = torch.zeros((nv, cp), dtype=F32, device="cuda")
        ops.scatter_mean_csr(up(c["F"]), d, order, seg, nv, X, col0=0, row_map=rm)
        ops.scatter_mean_csr(up(c["geo"]), la.GEO_DIM, order, seg, nv, X, col0=d, row_map=rm)
        rows, _, rinv = ops.split_f16(X, cp, per_row=True, interleaved=True)
        _OLD_ROWS[key] = (X, rows, rinv, ops.pow2_scale(X, d))
    return _OLD_ROWS[key]


@pytest.mark.parametrize("nv,d", la.VOXEL_SHAPES + (la.VOXEL_STRIDE_SHAPE,))
def test_voxel_rows_equal_scatter_split_scale(ops, nv, d):
    from geopurify_amd import _lib
    lib = _lib.load()
    c = la.case_voxel_rows(nv, d)
    cp = c["cin_pad"]
    X_old, rows_old, rinv_old, sc_old = old_rows_chain(ops, (nv, d), c)
    if nv <= 1027:                                                  # (the numpy reference walks the points one by one)
        _, rinv_ref, sc_ref = la.ref_voxel_rows(c)
        assert rinv_old.cpu().numpy().tolist() == rinv_ref.tolist() and sc_old.cpu().numpy().tolist() == sc_ref.tolist()

    def case(a):
        F, geo = a.inp(up(c["F"]), pitch=d + 4, name="f"), a.inp(up(c["geo"]), pitch=la.GEO_DIM + 2, name="geo")
        order, seg, rm = a.inp(up(c["order"]), name="order"), a.inp(up(c["seg_start"]), name="seg_start"), a.inp(up(c["row_map"]), name="row_map")
        X = a.out((nv, cp), F32, pitch=cp + 8, name="x")
        rows = a.out((nv, 2 * cp), F16, pitch=2 * cp + 8, name="rows")
        rinv, sc, ws = a.out(nv, F32, name="row_inv"), a.out(4, F32, name="scale2"), a.out(16, U8, name="workspace")
        ops.check(lib.gp_voxel_rows_operands(ops._ptr(F), F.stride(0), d, ops._ptr(geo), geo.stride(0), la.GEO_DIM, ops._ptr(order), ops._ptr(seg),
                                             nv, ops._ptr(rm), ops._ptr(X), X.stride(0), cp, ops._ptr(rows), rows.stride(0), ops._ptr(rinv),
                                             ops._ptr(sc), ops._ptr(ws), 16, ops._stream()), "gp_voxel_rows_operands")
        return {"X": X, "rows": rows, "row_inv": rinv, "scale2": sc}

    got = run(case)
    same(got["X"], X_old, "X")
    same(got["rows"], rows_old, "rows")
    same(got["row_inv"], rinv_old, "row_inv")
    same(got["scale2"][:2], sc_old, "scale2")
    assert unwritten(got["X"]) == 0 and unwritten(got["rows"]) == 0 and unwritten(got["row_inv"]) == 0
    assert unwritten(got["scale2"]) == 2                             # two floats, no more
    # the wrapper the pipeline calls: no row map, no scale
    X2, xs2, sc2 = ops.voxel_rows_operands(up(c["F"]), d, up(c["geo"]), la.GEO_DIM, up(c["order"]), up(c["seg_start"]), nv, cp, want_scale=False)
    assert sc2 is None and xs2[1] is None
    same(X2, X_old[up(c["row_map"]).long()], "X without a row map")
    same(xs2[0], rows_old[up(c["row_map"]).long()], "rows without a row map")


def test_voxel_rows_reject_bad_arguments(ops):
    from geopurify_amd import _lib
    lib = _lib.load()
    f = torch.zeros(4096, dtype=F32, device="cuda")
    z = torch.zeros(64, dtype=I64, device="cuda")
    p = ops._ptr

    def call(d=64, cp=96, ld_x=96, ld_rows=192, sc=None, ws=None, wsb=0):
        return lib.gp_voxel_rows_operands(p(f), d, d, p(f), 6, 6, p(z), p(z), 1, None, p(f), ld_x, cp, p(f), ld_rows, p(f), sc, ws, wsb, None)

    assert call(d=62) == -22 and call(cp=64) == -22 and call(cp=80) == -22 and call(ld_x=64) == -22 and call(ld_rows=96) == -22
    assert call(d=1024, cp=1056, ld_x=1056, ld_rows=2112) == -22                  # wider than a wave holds
    assert call(sc=p(f)) == -22                                                   # a scale needs its workspace


# ------------------------------------------------------------------------------------------ pipeline
def test_pipeline_lift_and_prepare_equal_the_old_calls(ops):
    from geopurify_amd import pipeline as pl
    from geopurify_amd import synthetic as syn
    cfg = dataclasses.replace(syn.CONFIGS["T"], feat_dim=512)
    scene = syn.make_scene(cfg, 123)
    vlm = pl.SyntheticVLM(syn.make_vlm_outputs(cfg, cfg.num_views, 123), "cuda")
    sd = pl.random_student_state_dict(cfg.feat_dim + pl.GEO_DIM, hidden=256, embed=128, num_blocks=1, seed=2)
    batch = pl.build_scene_batch(pl.upload_scene(scene, "cuda"), pl.scene_rigid_transform(cfg.voxel_size, 123), "cuda")
    st = pl.StudentWeights(sd, "cuda")
    hp = pl.HotPath(st, cfg.mask_shape, K=24, num_iters=3, device="cuda")
    seenargs = {}
    inner = hp._fuse_and_fill

    def spy(batch_, start, pvv, pvs, f_seg, l_seg, D, text, logit_scale):
        seenargs.update(start=start, pvv=pvv, pvs=pvs, f_seg=f_seg, l_seg=l_seg, D=D)
        return inner(batch_, start, pvv, pvs, f_seg, l_seg, D, text, logit_scale)

    hp._fuse_and_fill = spy
    F, text, scale = hp.lift_masks(batch, vlm)
    N, D = F.shape
    # the lift from the old calls
    F0 = torch.empty((N, D), dtype=F32, device="cuda")
    seen = ops.fuse_views_top3(seenargs["start"], seenargs["pvv"], seenargs["pvs"], N, seenargs["f_seg"], seenargs["l_seg"], F0)
    nn = ops.nn1_masked(batch.scene_coords, seen, 1 - seen)
    F_old = ops.gather_rows(F0, D, torch.where(nn >= 0, nn, torch.arange(N, device="cuda")))
    same(F, F_old, "F")
    # prepare from the old calls
    assert st.one_pass_input(F, batch.scene_gauss_features)
    state = hp.prepare(batch, F)
    Nv, rank = state["Nv"], state["rank"]
    X_old = torch.zeros((Nv, st.cin_pad), dtype=F32, device="cuda")
    ops.scatter_mean_csr(F_old, D, batch.order, batch.seg_start, Nv, X_old, col0=0, row_map=rank)
    ops.scatter_mean_csr(batch.scene_gauss_features, pl.GEO_DIM, batch.order, batch.seg_start, Nv, X_old, col0=D, row_map=rank)
    xs_old = st.split_input(X_old)
    same(state["X"], X_old, "X")
    assert state["xs"][1] is None and xs_old[1] is None
    same(state["xs"][0], xs_old[0], "xs rows")
    same(state["xs"][2], xs_old[2], "row_inv")
    assert state["pool"] is not None
    sc_old = ops.pow2_scale(X_old, D)
    same(state["pool"]["sc"], sc_old, "sc")
    hi, lo = ops.split_f16(X_old, D, scale=sc_old[0:1], dst_row=state["pool"]["rho"])
    same(state["pool"]["x_split"][0], hi, "pooling plane hi")
    same(state["pool"]["x_split"][1], lo, "pooling plane lo")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ kNN: every candidate read once
_KNN = {}


def knn_case(ops, name):
    """the case in Morton order on the device with its grid, and the reference lists per K, computed once"""
    if name not in _KNN:
        import lattice_cases as ltc
        v = la.case_knn(name)
        perm = ltc.morton_perm(v)
        cs = up(v[perm])
        grid = ops.grid_build(cs)
        assert grid.status() == 0
        _KNN[name] = dict(v=v, perm=perm, cs=cs, perm_dev=up(perm.astype(np.int32)), grid=grid, ref={K: ltc.lists(v, K) for K in la.KNN_CASES[name]})
    return _KNN[name]


@pytest.mark.parametrize("name,K", [(n, K) for n, ks in la.KNN_CASES.items() for K in ks])
def test_knn_read_once_equals_two_pass(ops, name, K):
    c = knn_case(ops, name)
    once = ops.knn_lattice(c["grid"], c["cs"], c["perm_dev"], K)
    twice = ops.knn_lattice(c["grid"], c["cs"], c["perm_dev"], K, two_pass=True)
    same(once, twice, "lists")
    got = once.cpu().numpy().astype(np.int64)
    back = np.empty_like(got)
    back[c["perm"]] = c["perm"][got]                              # Morton rows -> input rows
    assert np.array_equal(back, c["ref"][K])                      # and both are the exact (d^2, row) lists
    same(ops.knn_lattice(c["grid"], c["cs"], None, K), ops.knn_lattice(c["grid"], c["cs"], None, K, two_pass=True), "lists without ids")
