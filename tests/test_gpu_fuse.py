"""sparse.fuse, FusedChunks (.file, .save, .dense) and sparse.load_fused on the GPU against the restatement of tests/fuse_cases.py
(the keys with numpy, np.argpartition per (entry, file), the rows with torch on the CPU as features[rows].to(dtype)).

Bounds: none.  Masks, offsets and rows are compared with array_equal / torch.equal; feat by its bit patterns, the NaN positions (which
must coincide) masked out, since a NaN's payload is not specified.
"""
import os

import numpy as np
import pytest
import torch

import extent_fence
import fuse_cases as fc

pytestmark = pytest.mark.gpu

INT_OF = {torch.float16: torch.int16, torch.float32: torch.int32}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import _lib, ops, sparse
    _lib.load()
    return ops, sparse


def _dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.array(a))).cuda()


def _features(c, rows=None):
    """the case's features on the device; a misaligned case: a view one element into a larger buffer"""
    f = c.features if rows is None else c.features[torch.from_numpy(rows)]
    if not c.misaligned:
        return f.cuda()
    buf = torch.empty(f.numel() + 1, dtype=f.dtype, device="cuda")
    v = buf[1:].view(f.shape)
    v.copy_(f)
    assert v.is_contiguous() and v.data_ptr() % 16 == f.element_size()
    return v


def _call(env, c, form, rows=None, **kw):
    ops, sparse = env
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    opts = dict(n_split_points=c.n_split, num_files=c.num_files, seed=c.seed, form=form, dtype=c.dtype)
    return sparse.fuse(_dev(pick(c.points)), (_features(c, rows), _dev(pick(c.seen))), **{**opts, **kw})


def _same_rows(got, want, what=""):
    """two tensors of rows: dtype, shape, NaN positions and every other bit"""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions"
    iv = INT_OF[got.dtype]
    assert torch.equal(got.contiguous().view(iv).masked_fill(nan, 0), want.contiguous().view(iv).masked_fill(nan, 0)), f"{what}: bits"


def _assert_chunks(got, ref, what=""):
    assert got.mask_full.dtype == torch.bool and got.offsets.dtype == torch.int64
    assert np.array_equal(got.mask_full.cpu().numpy(), ref.mask_full), f"{what} mask_full"
    assert np.array_equal(got.offsets.cpu().numpy(), ref.offsets), f"{what} offsets"
    _same_rows(got.feat, ref.feat, f"{what} feat")
    if ref.mask is None:
        assert got.mask is None
    else:
        assert got.mask.dtype == torch.bool and np.array_equal(got.mask.cpu().numpy(), ref.mask), f"{what} mask"


def _same_file(got, want, what=""):
    assert set(got) == set(want), what
    for key in want:
        assert not got[key].is_cuda and got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        if key == "feat":
            _same_rows(got[key], want[key], what)
        else:
            assert got[key].dtype == torch.bool and torch.equal(got[key], want[key]), (what, key)


# ------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("form", fc.FORMS)
@pytest.mark.parametrize("name", fc.CASES)
def test_fuse_matches_the_restatement(env, name, form):
    c, ref = fc.case(name), fc.reference(name, form)
    got = _call(env, c, form)
    assert got.feat.dtype == c.dtype and got.feat.shape == (ref.feat.shape[0], c.D) and got.num_files == c.num_files and got.num_entries == c.B
    _assert_chunks(got, ref, f"{name} {form}")


@pytest.mark.parametrize("form", fc.FORMS)
def test_an_entry_by_itself_gives_its_slice(env, form):
    name = "sel_64_f3_s1"
    c, ref = fc.case(name), fc.reference(name, form)
    for b in (0, 2, 3, 5, fc.LARGEST, fc.UNSEEN_ENTRY):
        rows = c.rows_of(b)
        got = _call(env, c, form, rows=rows)
        assert got.num_entries == b + 1
        assert np.array_equal(got.mask_full.cpu().numpy(), ref.mask_full[:, rows]), b
        for k in range(c.num_files):
            lo, hi = got.offsets[k, b].item(), got.offsets[k, b + 1].item()
            assert got.offsets[k, 0].item() == got.offsets[k, b].item() and hi - lo == ref.offsets[k, b + 1] - ref.offsets[k, b]
            _same_rows(got.feat[lo:hi], ref.feat[ref.offsets[k, b]:ref.offsets[k, b + 1]], f"entry {b} file {k}")
            if form == "chunk":
                assert np.array_equal(got.mask[lo:hi].cpu().numpy(), ref.mask[ref.offsets[k, b]:ref.offsets[k, b + 1]])


@pytest.mark.parametrize("form", fc.FORMS)
def test_the_interleaving_of_the_entries_changes_no_file(env, form):
    ops, sparse = env
    name = "sel_nb1_f3_sbig"
    c, ref = fc.case(name), fc.reference(name, form)
    # another interleaving of the same entries, the order inside every entry kept
    batch = c.batch[np.random.default_rng(3).permutation(c.N)]
    src = np.empty(c.N, np.int64)
    for b in range(c.B):
        src[np.nonzero(batch == b)[0]] = c.rows_of(b)
    assert np.array_equal(c.batch[src], batch) and not np.array_equal(batch, c.batch)
    got = _call(env, c, form, rows=src)
    assert np.array_equal(got.offsets.cpu().numpy(), ref.offsets)
    _same_rows(got.feat, ref.feat)
    for b in (1, 4, fc.LARGEST):
        for k in range(c.num_files):
            _same_file(got.file(b, k), ref.files[(b, k)], f"({b}, {k})")
    # and the entries one after the other (no interleaving at all)
    order = np.argsort(c.batch, kind="stable")
    _same_rows(_call(env, c, form, rows=order).feat, ref.feat)


# ------------------------------------------------------------------------------------------ files
@pytest.mark.parametrize("form", fc.FORMS)
def test_file_and_save_give_the_dict_the_reader_loads(env, tmp_path, form):
    name = "sel_64_f3_s0"
    c, ref = fc.case(name), fc.reference(name, form)
    got = _call(env, c, form)
    for (b, k), want in ref.files.items():
        _same_file(got.file(b, k), want, f"file({b}, {k})")
        assert got.file(b, k)["feat"].dtype == torch.float16
    names = [f"scene{b:04d}_00" for b in range(c.B)]
    empty = sorted((b, k) for (b, k), d in ref.files.items() if d["feat"].shape[0] == 0)
    assert (fc.GAP_ENTRY, 0) in empty and ((fc.UNSEEN_ENTRY, 0) in empty) == (form == "merged")
    b0, k0 = min(empty)
    with pytest.raises(ValueError, match=f"file {k0} of entry {b0} \\(scene{b0:04d}_00_{k0}.pt\\) has no rows"):
        got.save(tmp_path / "refused", names)
    assert not os.path.exists(tmp_path / "refused")
    for bad in (names[:-1], names + ["x"], "scene", None, [1] * c.B):
        with pytest.raises(ValueError, match="scene_names must be"):
            got.save(tmp_path / "refused", bad)
    paths = got.save(tmp_path / "out", names, skip_empty=True)
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f"{names[b]}_{k}.pt" for (b, k) in ref.files if (b, k) not in empty)
    assert sorted(os.path.basename(p) for p in paths) == sorted(os.listdir(tmp_path / "out"))
    for (b, k), want in ref.files.items():
        if (b, k) not in empty:
            _same_file(torch.load(tmp_path / "out" / f"{names[b]}_{k}.pt"), want, f"saved ({b}, {k})")
    # nothing empty: save writes every file without skip_empty
    w = fc.case("d8")
    full = _call(env, w, "chunk").save(tmp_path / "full", ["a", "b", "c"])
    assert len(full) == 3 * w.num_files == len(os.listdir(tmp_path / "full"))


@pytest.mark.parametrize("which", ["val_2key", "val_3key", "train_2key", "train_3key"])
def test_the_projects_loader_reads_the_saved_files(env, tmp_path, which):
    """FusedFeatureLoader, host and device="cuda", on save's files gives the items it gives on the files the test builds itself"""
    from geopurify_amd.feature_loader import FusedFeatureLoader
    split, key = which.split("_")
    name, form = f"loader_{key}", "merged" if key == "2key" else "chunk"
    c, ref = fc.case(name), fc.reference(name, form)
    d3 = tmp_path / "scannet_3d"
    os.makedirs(d3 / split)
    for b, scene in enumerate(c.scene_names):
        rows = c.rows_of(b)
        torch.save((c.points[rows, 1:].astype(np.float32), c.colors[rows].copy(), c.labels[rows].copy()), d3 / split / f"{scene}_vh_clean_2.pth")
    _call(env, c, form).save(tmp_path / "saved", c.scene_names)
    os.makedirs(tmp_path / "built")
    for (b, k), d in ref.files.items():
        torch.save(d, tmp_path / "built" / f"{c.scene_names[b]}_{k}.pt")
    assert sorted(os.listdir(tmp_path / "saved")) == sorted(os.listdir(tmp_path / "built")) and len(ref.files) == 2 * c.num_files
    for device in (None, "cuda"):
        items = []
        for feat_dir in ("saved", "built"):
            ds = FusedFeatureLoader(str(d3), str(tmp_path / feat_dir), voxel_size=0.05, split=split, eval_all=True, input_color=True, device=device)
            assert len(ds) == 2
            per = []
            for i in range(2):
                np.random.seed(40 + i)
                per.append(ds[i])
            items.append(per)
        for a, b in zip(*items):
            assert len(a) == len(b) == 6
            for j, (x, y) in enumerate(zip(a, b)):
                assert x.dtype == y.dtype and x.shape == y.shape and x.is_cuda == (device == "cuda") and torch.equal(x, y), (which, device, j)
            assert a[3].shape[0] > 0 and bool(a[4].any())


# ------------------------------------------------------------------------------------------ the way back
def _dense_formula(c, ref, k):
    out = torch.zeros((c.N, c.D), dtype=torch.float32)
    lo, hi = ref.offsets[k, 0], ref.offsets[k, -1]
    out[torch.from_numpy(ref.rows[lo:hi])] = ref.feat[lo:hi].float()
    return out


@pytest.mark.parametrize("form", fc.FORMS)
@pytest.mark.parametrize("name", ["sel_64_f3_s0", "values", "d1", "d3", "d6", "d520", "f32_out_d8", "f32_out_d6", "half_in_d12"])
def test_dense_is_its_formula(env, name, form):
    c, ref = fc.case(name), fc.reference(name, form)
    got = _call(env, c, form)
    for k in range(c.num_files):
        out, mask = got.dense(k)
        assert out.is_cuda and out.dtype == torch.float32 and mask.dtype == torch.bool
        assert np.array_equal(mask.cpu().numpy(), ref.mask_full[k])
        _same_rows(out, _dense_formula(c, ref, k), f"{name} {form} dense({k})")


@pytest.mark.parametrize("form", fc.FORMS)
def test_load_fused_reads_what_save_wrote(env, tmp_path, form):
    ops, sparse = env
    name = "sel_64_f3_s0"
    c, ref = fc.case(name), fc.reference(name, form)
    got = _call(env, c, form)
    names = [f"s{b}" for b in range(c.B)]
    got.save(tmp_path, names, skip_empty=True)
    for k in range(c.num_files):
        files = [tmp_path / f"{names[b]}_{k}.pt" for b in range(c.B)]
        back = sparse.load_fused(_dev(c.points), [str(p) if os.path.exists(p) else None for p in files])
        lo, hi = ref.offsets[k, 0], ref.offsets[k, -1]
        assert back.num_files == 1 and back.form == form
        assert np.array_equal(back.mask_full.cpu().numpy(), ref.mask_full[k:k + 1])
        assert np.array_equal(back.offsets.cpu().numpy(), ref.offsets[k:k + 1] - lo)
        _same_rows(back.feat, ref.feat[lo:hi])
        assert (back.mask is None) if form == "merged" else np.array_equal(back.mask.cpu().numpy(), ref.mask[lo:hi])
        _same_rows(back.dense(0)[0], _dense_formula(c, ref, k))
    if form == "chunk":
        # three-key dicts whose "mask" is a list of row indices (dataset/feature_loader.py:129-139)
        dicts = []
        for b in range(c.B):
            d = dict(ref.files[(b, 1)])
            d["mask"] = d["mask"].nonzero().reshape(-1)
            dicts.append(d if d["feat"].shape[0] else None)
        back = sparse.load_fused(_dev(c.points), dicts)
        lo, hi = ref.offsets[1, 0], ref.offsets[1, -1]
        assert np.array_equal(back.mask.cpu().numpy(), ref.mask[lo:hi]) and np.array_equal(back.mask_full.cpu().numpy(), ref.mask_full[1:2])
        _same_rows(back.feat, ref.feat[lo:hi])
    with pytest.raises(ValueError, match="file of entry 1"):
        sparse.load_fused(_dev(c.points), [ref.files[(0, 0)], ref.files[(2, 0)]] + [None] * (c.B - 2))
    with pytest.raises(ValueError, match="rows have a batch index"):
        sparse.load_fused(_dev(c.points), [ref.files[(0, 0)]])


def test_lift_fuse_dense_quantize_is_quantize_on_the_half_rounded_seen_rows(env):
    ops, sparse = env
    import lift_labels_cases as ll
    c = ll.case("entries")
    D = 8
    g = torch.Generator().manual_seed(4)
    maps = (torch.randn((c.V, D, c.H, c.W), generator=g) * 4).cuda()
    depth = None if c.depth is None or isinstance(c.depth, str) else _dev(c.depth)
    P = _dev(c.points)
    lifted = sparse.lift(P, sparse.Views(maps, _dev(c.view_entry), _dev(c.w2c), _dev(c.intr), depth), cut_bound=c.cut, vis_thres=c.tau,
                         min_visible=c.min_visible, max_visible=c.max_visible, fill=False)
    assert int(lifted.seen.sum()) > 0
    feats, mask = sparse.fuse(P, lifted).dense()
    assert torch.equal(mask, lifted.seen)
    want = torch.where(lifted.seen.unsqueeze(1), lifted.features.half().float(), torch.zeros((), device="cuda"))
    a, b = sparse.quantize(P, feats, quantization_size=0.05), sparse.quantize(P, want, quantization_size=0.05)
    for k in ("coordinates", "features", "inverse_mapping", "unique_index", "counts"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ------------------------------------------------------------------------------------------ refusals and read-backs
def test_refusals_before_any_kernel(env):
    ops, sparse = env
    c = fc.case("d8")
    P, Fe, S = _dev(c.points), c.features.cuda(), _dev(c.seen)
    before = ops.READBACK["calls"]
    bad = [
        (dict(points=P[:, :3]), "points must be"), (dict(points=c.points), "points must be"), (dict(points=torch.from_numpy(c.points)), "CUDA"),
        (dict(points=P.int()), "fp64 or fp32"),
        (dict(features=Fe[:-1]), "features must be"), (dict(features=Fe.double()), "features must be"), (dict(features=Fe.cpu()), "one CUDA device"),
        (dict(features=Fe.reshape(-1)), "features must be"),
        (dict(seen=S[:-1]), "seen must be"), (dict(seen=S.to(torch.uint8)), "seen must be"), (dict(seen=S.cpu()), "one CUDA device"),
        (dict(num_files=0), "num_files"), (dict(num_files=17), "num_files"), (dict(num_files=1.0), "num_files"),
        (dict(n_split_points=0), "n_split_points"), (dict(n_split_points=-3), "n_split_points"), (dict(n_split_points=2.5), "n_split_points"),
        (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(seed=0.5), "seed"),
        (dict(form="both"), "form"), (dict(dtype=torch.bfloat16), "dtype"), (dict(dtype=torch.float64), "dtype"),
    ]
    for kw, message in bad:
        kw = dict(kw)
        points, features, seen = kw.pop("points", P), kw.pop("features", Fe), kw.pop("seen", S)
        with pytest.raises(ValueError, match=message):
            sparse.fuse(points, (features, seen), **kw)
    with pytest.raises(ValueError, match="lifted must be"):
        sparse.fuse(P, Fe)
    assert ops.READBACK["calls"] == before                 # nothing ran far enough to read anything back
    assert sparse.fuse(P, (Fe, S), seed=2 ** 64 - 1, num_files=16, n_split_points=1, form="chunk").feat.shape[0] == 16 * 3


def test_bad_batch_indices_come_from_the_read_back(env):
    ops, sparse = env
    c = fc.case("d8")
    for value, count in ((-1.0, 1), (65536.0, 1), (2.5, 1), (float("nan"), 1)):
        P = _dev(c.points).clone()
        P[5, 0] = value
        with pytest.raises(ValueError, match=f"fuse: {count} rows have a batch index that is no integer in 0..65535"):
            sparse.fuse(P, (c.features.cuda(), _dev(c.seen)))
    # only the batch column is read: non-finite coordinates change nothing
    P = _dev(c.points).clone()
    P[:, 1:] = float("nan")
    _assert_chunks(sparse.fuse(P, (c.features.cuda(), _dev(c.seen)), n_split_points=c.n_split, num_files=c.num_files, seed=c.seed),
                   fc.reference("d8", "merged"))
    # fp32 points, and the highest valid batch index
    top = c.points.astype(np.float32)
    top[:, 0] = 65535
    got = sparse.fuse(_dev(top), (c.features.cuda(), _dev(c.seen)))
    assert got.offsets.shape == (1, 65537) and got.offsets[0, 65535].item() == 0 and got.offsets[0, 65536].item() == int(c.seen.sum())


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


def test_at_most_two_read_backs_and_no_other_synchronisation(env):
    ops, sparse = env
    c = fc.case("sel_64_f3_s0")
    P, Fe, S = _dev(c.points), c.features.cuda(), _dev(c.seen)
    for form in fc.FORMS:
        assert 1 <= _no_sync_but_readback(ops, lambda: sparse.fuse(P, (Fe, S), n_split_points=64, num_files=3, form=form)) <= 2
    assert not sparse.fuse(P, (Fe, S)).feat.requires_grad


# ------------------------------------------------------------------------------------------ extents
@pytest.mark.parametrize("form", fc.FORMS)
@pytest.mark.parametrize("name", ["d1", "d3", "d4", "d6", "d8", "d520", "half_in_d8", "half_in_d3", "f32_out_d8", "half_in_f32_out_d3", "sel_1_f3_s0"])
def test_the_ops_calls_stay_inside_their_extents(env, name, form):
    """ops.fuse_plan / fuse_write / fuse_dense on fenced arrays: seen, the features, every output, the state and the workspaces of
    exactly the reported bytes; the fp64 points have no fence type and stay plain.  d1 ends in a file of one row."""
    ops, _ = env
    c, ref = fc.case(name), fc.reference(name, form)
    N, D, F = c.N, c.D, c.num_files
    k_last = F - 1
    lo, hi = int(ref.offsets[k_last, 0]), int(ref.offsets[k_last, -1])

    def case(a):
        seen = a.inp(torch.from_numpy(c.seen).to(torch.uint8), name="seen")
        feats = a.inp(c.features, name="features")
        plan = ops.fuse_plan(_dev(c.points), seen, c.n_split, F, c.seed, form, buffers={
            "mask_full": a.out((F, N), torch.uint8, name="mask_full"), "state": a.out(ops.fuse_state_bytes(N, F), torch.uint8, name="state"),
            "status": a.out(8, torch.int64, name="status")}, workspace=a.out(ops.fuse_workspace_bytes(N, F, c.n_split), torch.uint8, name="ws_plan"))
        status = plan.status.tolist()
        B, R = status[3] + 1, status[4]
        assert (B, R) == (c.B, ref.feat.shape[0])
        bufs = {"feat": a.out((R, D), c.dtype, name="feat"), "offsets": a.out((F, B + 1), torch.int64, name="offsets")}
        if form == "chunk":
            bufs["mask"] = a.out(R, torch.uint8, name="mask")
        feat, mask, offsets = ops.fuse_write(plan, feats, B, R, c.dtype, buffers=bufs)
        outs = {"mask_full": plan.mask_full, "status": plan.status, "feat": feat, "offsets": offsets}
        if mask is not None:
            outs["mask"] = mask
        # the way back, from the last file set (fenced copies of what was just written)
        rows = a.inp(feat[lo:hi].clone(), name="feat_in")
        dense, dstatus = ops.fuse_dense(_dev(c.points), a.inp(plan.mask_full[k_last].clone(), name="mask_full_in"), rows, buffers={
            "out": a.out((N, D), torch.float32, name="dense"), "status": a.out(8, torch.int64, name="dense_status")},
            workspace=a.out(ops.fuse_dense_workspace_bytes(N), torch.uint8, name="ws_dense"))
        outs.update(dense=dense, dense_status=dstatus)
        return outs

    got = extent_fence.run(case)
    for k, v in got.items():
        assert extent_fence.unwritten(v) == 0, k
    assert np.array_equal(got["mask_full"].cpu().numpy().astype(bool), ref.mask_full) and np.array_equal(got["offsets"].cpu().numpy(), ref.offsets)
    _same_rows(got["feat"], ref.feat)
    _same_rows(got["dense"], _dense_formula(c, ref, k_last))
    assert got["status"].tolist() == [0, 0, 0, c.B - 1, ref.feat.shape[0], 0, 0, 0] and got["dense_status"].tolist() == [0, 0, 0, c.B - 1, hi - lo, 0, 0, 0]
    if name == "d1":
        assert ref.offsets[-1, -1] - ref.offsets[-1, -2] == 1


def test_overlapping_arguments_are_refused(env):
    ops, _ = env
    from geopurify_amd._lib import GeoPurifyHipError
    c = fc.case("d8")
    both = torch.zeros(2 * c.N * c.num_files, dtype=torch.uint8, device="cuda")
    with pytest.raises(GeoPurifyHipError, match="an output overlaps an input"):
        ops.fuse_plan(_dev(c.points), both[c.N - 1:2 * c.N - 1], 64, 1, buffers={"mask_full": both[:c.N].view(1, c.N)})
