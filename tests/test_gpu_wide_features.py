"""Row 12 and the fused final pass at feature widths other than 512: the column-sliced matrix-core pooling at D = 256, 768 and 1024
(d / 256 column slices per row block), its chained launch, the fused gather + classify at 768 and 1024, and the hot path at D = 768."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import affinity as o_aff  # noqa: E402
from oracle import pipeline as o_pipe  # noqa: E402

WIDE = [256, 768, 1024]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import ops as _ops
    from geopurify_amd import _lib
    _lib.load()
    return _ops


def _voxels(rng, n, ext):
    """A sheet, a wall and scattered voxels: lattice neighbourhoods of uneven size."""
    a = np.c_[rng.integers(0, ext, n), rng.integers(0, ext, n), rng.integers(3, 5, n)]
    b = np.c_[rng.integers(0, ext, n // 2), np.full(n // 2, 17), rng.integers(0, 40, n // 2)]
    v = np.unique(np.vstack([a, b]), axis=0)
    return v[rng.permutation(len(v))].astype(np.int32)


def _operator(ops, n, ext, K, seed):
    """Morton-sorted voxels, their K-NN lists and softmax weights: (cs, nbr, w)."""
    rng = np.random.default_rng(seed)
    c = torch.from_numpy(_voxels(rng, n, ext)).cuda()
    perm, _ = ops.morton_order(c)
    cs = c[perm.long()].contiguous()
    grid = ops.grid_build(cs)
    nbr = ops.knn_lattice(grid, cs, perm, K)
    g = torch.Generator().manual_seed(seed)
    E = F.normalize(torch.randn(cs.shape[0], 128, generator=g), dim=1).cuda()
    w = ops.affinity_softmax(E, nbr, 20.0)
    return cs, nbr, w


# (voxel draw, extent, K): a ragged last row block, and fewer rows than one block
SHAPES = [(1800, 60, 96), (60, 8, 32)]


@pytest.mark.parametrize("D", WIDE)
@pytest.mark.parametrize("shape", SHAPES)
def test_pool_cs_single_application_vs_fp64_and_ell(ops, D, shape):
    """One application of gp_pool_cs_apply at D = 256 / 768 / 1024 against the fp64 gather of the operator and against the ELL
    kernel on the same weights, in the Morton row order and in the operator's own (rcb) order; both outputs at once."""
    n, ext, K = shape
    cs, nbr, w = _operator(ops, n, ext, K, seed=D + n)
    Nv = cs.shape[0]
    assert Nv % 128 != 0
    g = torch.Generator().manual_seed(D)
    X = torch.randn(Nv, D + 32, generator=g)
    Xd = X.cuda()
    ref = o_aff.pool_gather(X[:, :D], nbr.cpu().long(), w.cpu(), 1)
    y_ell = torch.empty(Nv, D, device="cuda")
    ops.pool_ell(Xd, nbr, w, D, y_ell)
    sc = ops.pow2_scale(Xd, D)
    op = ops.pool_cs_build(nbr, w)
    xs = ops.split_f16(Xd, D, scale=sc[0:1])
    y = torch.full((Nv, D + 64), float("nan"), device="cuda")            # a row pitch wider than d: the columns past d stay untouched
    ys = tuple(torch.full((Nv, D), float("nan"), dtype=torch.float16, device="cuda") for _ in range(2))
    ops.pool_cs_apply(xs, op, D, out_split=ys, out_f32=y, out_scale=sc[1:2])
    torch.cuda.synchronize()
    assert torch.isnan(y[:, D:]).all()
    yd = y[:, :D]
    assert (yd.cpu().double() - ref).abs().max() < 1e-4
    assert (yd - y_ell).abs().max() < 2e-5
    assert ((ys[0].float() + ys[1].float()) * sc[1] - yd).abs().max() < 1e-6 * float(X.abs().max())
    if Nv > 1024:                                                        # the operator's own row order (HotPath's default there)
        sigma, rho = ops.rcb_order(cs, 1024, 128)
        op_r = ops.pool_cs_build(ops.rows_renumber(nbr, sigma, rho), w[sigma.long()].contiguous())
        yr = torch.empty(Nv, D, device="cuda")
        ops.pool_cs_apply(ops.split_f16(Xd, D, scale=sc[0:1], dst_row=rho), op_r, D, out_f32=yr, out_scale=sc[1:2])
        yr = yr[rho.long()]
        assert (yr.cpu().double() - ref).abs().max() < 1e-4
        assert (yr - y_ell).abs().max() < 2e-5


@pytest.mark.parametrize("D", WIDE)
@pytest.mark.parametrize("shape", SHAPES)
def test_pool_cs_chain_equals_the_launches(ops, D, shape):
    """gp_pool_cs_apply_chain over T = 19 applications at D = 256 / 768 / 1024: the same planes and output, bit for bit, as 19
    calls of gp_pool_cs_apply ping-ponging between two plane sets; flags sized for d; the abort word reads 0."""
    from geopurify_amd import _lib
    n, ext, K = shape
    T = 19
    cs, nbr, w = _operator(ops, n, ext, K, seed=3 * D + n)
    Nv = cs.shape[0]
    op = ops.pool_cs_build(nbr, w)
    ops.pool_cs_deps(op, D)
    nb = op.bu_off.numel() - 1
    assert op.flags.numel() == 32 + (D // 256) * nb == _lib.load().gp_pool_cs_chain_flag_words_d(Nv, 128, D)
    X = torch.randn(Nv, D, device="cuda")
    sc = ops.pow2_scale(X, D)
    x0 = ops.split_f16(X, D, scale=sc[0:1])
    sp = [tuple(t.clone() for t in x0), tuple(torch.full((Nv, D), float("nan"), dtype=torch.float16, device="cuda") for _ in range(2))]
    ref = torch.full((Nv, D), float("nan"), device="cuda")
    src = sp[0]
    for t in range(T):
        last = t == T - 1
        dst = None if last else sp[(t + 1) % 2]
        ops.pool_cs_apply(src, op, D, out_split=dst, out_f32=ref if last else None, out_scale=sc[1:2] if last else None)
        src = dst
    xs = tuple(t.clone() for t in x0)
    pong = tuple(torch.full((Nv, D), float("nan"), dtype=torch.float16, device="cuda") for _ in range(2))
    out = torch.full((Nv, D), float("nan"), device="cuda")
    ops.pool_cs_apply_chain(xs, pong, op, D, T, out, out_scale=sc[1:2])
    ops.pool_cs_chain_check(op)
    assert int(op.flags[0].item()) == 0
    for a, b in zip([out, *xs, *pong], [ref, *sp[0], *sp[1]]):
        assert torch.equal(a, b)
    assert not torch.isnan(out).any()


def test_pool_cs_rejects_other_widths(ops):
    """Widths that are not whole 256-column slices, or more than four of them, are an error that names the widths taken."""
    cs, nbr, w = _operator(ops, 300, 12, 16, seed=9)
    Nv = cs.shape[0]
    op = ops.pool_cs_build(nbr, w)
    X = torch.randn(Nv, 1536, device="cuda")
    for d in (128, 640, 1280):
        xs = ops.split_f16(X, d)
        with pytest.raises(Exception, match="256, 512, 768 or 1024"):
            ops.pool_cs_apply(xs, op, d, out_f32=torch.empty(Nv, d, device="cuda"))
        with pytest.raises(Exception, match="256, 512, 768 or 1024"):
            ops.pool_cs_apply_chain(xs, tuple(torch.empty_like(t) for t in xs), op, d, 3, torch.empty(Nv, d, device="cuda"))


@pytest.mark.parametrize("D,C", [(768, 19), (1024, 16), (576, 20)])
def test_gather_rows_classify_wide_equals_the_two_calls(ops, D, C):
    """gp_gather_rows_classify above 512 columns: the rows of gp_gather_rows and the labels / zero flags of gp_classify_argmax on
    them, bit for bit, with and without a row map, with a row of zeros and a point count that leaves the last group partly empty."""
    g = torch.Generator().manual_seed(D)
    Nv, N = 2000, 5003
    X = torch.randn(Nv, D + 32, generator=g)
    X[17, :D] = 0.0
    idx = torch.randint(0, Nv, (N,), generator=g)
    idx[5] = 17
    rmap = torch.randperm(Nv, generator=g).to(torch.int32)
    text = F.normalize(torch.randn(C, D, generator=g), dim=1)
    Xd, idd, rd, td = X.cuda(), idx.cuda(), rmap.cuda(), text.cuda()
    assert ops.can_gather_rows_classify(D, C)
    for row_map in (None, rd):
        ref = ops.gather_rows(Xd, D, idd, row_map=row_map)
        pred_ref, zero_ref = ops.classify_argmax(ref, td, 14.2)
        out, pred, zero = ops.gather_rows_classify(Xd, D, idd, td, 14.2, row_map=row_map)
        assert torch.equal(out, ref) and torch.equal(pred, pred_ref) and torch.equal(zero, zero_ref)
        assert int(zero.sum()) >= 1 or row_map is not None
        assert len(torch.unique(pred)) > 1
    assert not ops.can_gather_rows_classify(D, 32)
    with pytest.raises(Exception, match="gp_gather_rows_classify"):
        ops.gather_rows_classify(Xd, D, idd, F.normalize(torch.randn(32, D), dim=1).cuda(), 1.0)


@pytest.fixture(scope="module")
def scene768():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import pipeline as pl
    from geopurify_amd import synthetic as syn
    cfg = dataclasses.replace(syn.CONFIGS["S"], num_points=9000, num_views=3, feat_dim=768)
    scene = syn.make_scene(cfg, 4242)
    vlm_np = syn.make_vlm_outputs(cfg, cfg.num_views, 4242)
    sd = pl.random_student_state_dict(cfg.feat_dim + pl.GEO_DIM, hidden=256, embed=128, num_blocks=1, seed=6)
    rigid = pl.scene_rigid_transform(cfg.voxel_size, 4242)
    K, T = 32, 4
    ref = o_pipe.evaluate_scene_oracle(scene, vlm_np, sd, rigid, K=K, num_iters=T)
    batch = pl.build_scene_batch(pl.upload_scene(scene, "cuda"), rigid, "cuda")
    return dict(pl=pl, cfg=cfg, sd=sd, ref=ref, batch=batch, K=K, T=T)


def test_hot_path_refine_at_768(scene768):
    """rows 8-12 and the final gather at D = 768 (the student at 774 input channels on the f16x3 kernels) against the oracle,
    through the column-sliced pooling ("auto") and its chained launch; the fused classification gives classify_argmax's labels."""
    from geopurify_amd import ops
    pl, ref, b, cfg = scene768["pl"], scene768["ref"], scene768["batch"], scene768["cfg"]
    st = pl.StudentWeights(scene768["sd"], "cuda")
    assert st.cin == 774 and all(l[0] == "f16x3" for l in st.layers), [l[0] for l in st.layers]
    lifted = ref["lifted"].cuda().contiguous()
    outs = {}
    for mode, kernel in (("auto", "cs_pool_ns_kernel"), ("mfma_chain", "cs_chain_ns_kernel")):
        hp = pl.HotPath(st, cfg.mask_shape, K=scene768["K"], num_iters=scene768["T"], device="cuda", pool_mode=mode)
        out = hp.refine(b, lifted)
        hp.pool_chain_check()
        assert hp.stats["pool_kernel"] == kernel, hp.stats["pool_kernel"]
        assert hp.stats["pool_bytes_per_iter"] == hp.stats["Nv"] * (2 * 768 * 4 + scene768["K"] * 8)
        d = (out.cpu() - ref["scene_features"]).abs().max()
        assert d < 1e-4, (mode, float(d))
        outs[mode] = out
    assert torch.equal(outs["auto"], outs["mfma_chain"])
    text = torch.randn(19, 768, device="cuda")
    hp = pl.HotPath(st, cfg.mask_shape, K=scene768["K"], num_iters=scene768["T"], device="cuda")
    out = hp.refine(b, lifted, classify_text=(text, 14.2))
    assert hp._fused_pred is not None
    assert torch.equal(out, outs["auto"])
    pred_ref, zero_ref = ops.classify_argmax(out, F.normalize(text, dim=-1).contiguous(), 14.2)
    assert torch.equal(hp._fused_pred[2], pred_ref) and torch.equal(hp._fused_pred[3], zero_ref)


def test_d512_resolution_and_kernel_unchanged(scene768):
    """D = 512 still resolves to the product kernels (the suite checks their outputs)."""
    pl = scene768["pl"]
    assert pl.resolve_pool_mode("auto", 512, 32, 4, 8, 64) == "cs"
    sd = pl.random_student_state_dict(512 + pl.GEO_DIM, hidden=256, embed=128, num_blocks=1, seed=7)
    st = pl.StudentWeights(sd, "cuda")
    b = scene768["batch"]
    Fl = torch.randn(b.scene_inds_reconstruct.shape[0], 512, device="cuda")
    for mode, kernel in (("auto", "cs_pool_kernel"), ("mfma_chain", "cs_chain_kernel")):
        hp = pl.HotPath(st, scene768["cfg"].mask_shape, K=32, num_iters=4, device="cuda", pool_mode=mode)
        hp.refine(b, Fl)
        hp.pool_chain_check()
        assert hp.stats["pool_kernel"] == kernel
