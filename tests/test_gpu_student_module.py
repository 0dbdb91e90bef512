"""AffinityPredictor.forward on batched SparseTensors (models/affinity_module.py:68-72): the batch-aware voxel order and kernel map
(gp_coords_order_batched / gp_kernel_map_sorted), the eval forward on the folded inference path, and the autograd path through the
training kernels (train mode: batch statistics; eval mode: running statistics) against fp64 oracles composed from oracle.student /
oracle.train."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import student as o_student  # noqa: E402
from oracle import train as o_train  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import _lib, ops, pipeline
    _lib.load()
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import MinkowskiEngine as ME
    finally:
        sys.path.pop(0)
    return ops, pipeline, ME


def _entry(rng, n, lo=-40, ext=14):
    """n distinct voxels of a dense-ish random blob with negative coordinates (27-neighbour occupancy ~10)"""
    v = np.unique(rng.integers(lo, lo + ext, size=(3 * n, 3)), axis=0)
    return v[rng.permutation(len(v))[:n]].astype(np.int32)


def _batched(rng, entries):
    """-> C int32 [N, 4] (batch, x, y, z) with the rows of all entries shuffled together"""
    C = np.concatenate([np.c_[np.full(len(e), b, np.int32), e] for b, e in enumerate(entries)])
    return C[rng.permutation(len(C))]


def _oracle_map(C):
    """oracle.student.build_kernel_map per batch entry, in global (input) rows: int64 [27, N]"""
    out = np.full((27, len(C)), -1, dtype=np.int64)
    for b in np.unique(C[:, 0]):
        idx = np.where(C[:, 0] == b)[0]
        m = o_student.build_kernel_map(C[idx, 1:])
        out[:, idx] = np.where(m >= 0, idx[np.maximum(m, 0)], -1)
    return out


def _device_map_in_input_rows(ops, Cd):
    perm, rank, keys, status = ops.coords_order_batched(Cd)
    assert status.tolist() == [0, 0, 0]
    nm = ops.kernel_map_sorted(keys).long().cpu()
    perm, rank = perm.long().cpu(), rank.long().cpu()
    g = nm[:, rank]                                        # [27, input row] -> sorted row of the neighbour
    return torch.where(g >= 0, perm[g.clamp(min=0)], g).numpy()


def _student(pl, cin, hidden, seed):
    from geopurify_amd.affinity_module import AffinityPredictor
    m = AffinityPredictor(input_dim=cin, embed_dim=128, hidden_dim=hidden)
    m.load_state_dict(pl.random_student_state_dict(cin, hidden=hidden, embed=128, num_blocks=4, seed=seed))
    return m.cuda()


def _features(rng, n, cin):
    """rows shaped like evaluate_scene's voxel inputs: unit-norm-ish semantic part + geometry columns"""
    d = cin - 6
    sem = rng.normal(0, 1, size=(n, d))
    sem = sem / np.linalg.norm(sem, axis=1, keepdims=True) * rng.uniform(0.3, 1.0, size=(n, 1))
    geo = np.c_[rng.uniform(0, 1, size=(n, 3)), rng.normal(0, 0.6, size=(n, 3))]
    return torch.from_numpy(np.c_[sem, geo].astype(np.float32))


# ------------------------------------------------------------------------------------------ 1. order and kernel map
def test_batched_kernel_map_vs_oracle_per_entry(env):
    ops, pl, ME = env
    rng = np.random.default_rng(11)
    a = _entry(rng, 700)
    entries = [a, _entry(rng, 500, lo=-3, ext=11), a + np.array([1, 0, -1], np.int32)]     # entry 2: a translated copy of entry 0
    C = _batched(rng, entries)
    assert (C[:, 1:] < 0).any()
    got = _device_map_in_input_rows(ops, torch.from_numpy(C).cuda().contiguous())
    exp = _oracle_map(C)
    assert np.array_equal(got, exp)
    # the translated copy shares xyz with entry 0 without ever connecting to it
    b = C[:, 0]
    assert all((b[got[k][got[k] >= 0]] == b[got[k] >= 0]).all() for k in range(27))


def test_single_entry_matches_existing_builder_bit_for_bit(env):
    ops, pl, ME = env
    rng = np.random.default_rng(12)
    xyz = _entry(rng, 3000, lo=-500, ext=18)
    xyz[0] = (3000, -9, 77)                                              # a far outlier: extents 3500 x 70 x 600
    for bidx in (0, 5):
        c = torch.from_numpy(xyz).cuda().contiguous()
        Cd = torch.cat([torch.full((len(xyz), 1), bidx, dtype=torch.int32, device="cuda"), c], 1).contiguous()
        perm0, rank0 = ops.morton_order(c)
        cs = c[perm0.long()].contiguous()
        nm0 = ops.kernel_map_build(ops.grid_build(cs), cs)
        perm1, rank1, keys, status = ops.coords_order_batched(Cd)
        nm1 = ops.kernel_map_sorted(keys)
        assert status.tolist() == [0, 0, 0]
        assert torch.equal(perm0, perm1) and torch.equal(rank0, rank1)
        assert torch.equal(nm0, nm1)
        assert bool((keys[1:] > keys[:-1]).all())


def test_bad_coordinates_raise(env):
    ops, pl, ME = env
    rng = np.random.default_rng(13)
    m = _student(pl, 38, 128, 1).eval()
    xyz = _entry(rng, 50)
    X = torch.zeros(52, 38, device="cuda")

    def run(C):
        with torch.no_grad():
            return m(ME.SparseTensor(features=X[:len(C)], coordinates=torch.from_numpy(C).cuda()))
    C = np.c_[np.zeros(50, np.int32), xyz]
    dup = np.concatenate([C, C[[3, 17]]])
    with pytest.raises(ValueError, match="2 duplicate"):
        run(dup)
    st = ops.coords_order_batched(torch.from_numpy(dup).cuda().contiguous())[3]
    assert st.tolist() == [2, 0, 0]
    bad_b = C.copy()
    bad_b[7, 0] = 65536
    with pytest.raises(ValueError, match="batch index"):
        run(bad_b)
    neg_b = C.copy()
    neg_b[8, 0] = -1
    with pytest.raises(ValueError, match="batch index"):
        run(neg_b)
    wide = C.copy()
    wide[0, 1:] = (-30000, 0, 0)
    wide[1, 1:] = (35535, 0, 0)                                         # extent 65536 along x
    with pytest.raises(ValueError, match="65536 or more along x"):
        run(wide)
    wide[1, 1:] = (35534, 0, 0)                                         # extent 65535: still in range
    st = ops.coords_order_batched(torch.from_numpy(wide).cuda().contiguous())[3]
    assert st.tolist() == [0, 0, 0]
    run(wide)


# ------------------------------------------------------------------------------------------ 2. eval forward without gradients
def _oracle_raw(X64, nm, sd):
    """AffinityPredictor.forward in fp64 with eval BatchNorm, before F.normalize (oracle.student pieces)"""
    p = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    out = F.relu(o_student.bn_eval(o_student.sparse_conv3(X64, nm, p["input_layer.0.kernel"]), p, "input_layer.1"))
    for i in range(4):
        idt = out
        o = F.relu(o_student.bn_eval(o_student.sparse_conv3(out, nm, p[f"res_blocks.{i}.conv1.kernel"]), p, f"res_blocks.{i}.norm1"))
        o = o_student.bn_eval(o_student.sparse_conv3(o, nm, p[f"res_blocks.{i}.conv2.kernel"]), p, f"res_blocks.{i}.norm2")
        out = F.relu(o + idt)
    return out @ p["output_layer.kernel"]


@pytest.mark.parametrize("hidden,cin", [(256, 518), (512, 518), (128, 38)])
def test_eval_forward_vs_fp64_and_student_weights(env, hidden, cin):
    ops, pl, ME = env
    rng = np.random.default_rng(20 + hidden)
    C = _batched(rng, [_entry(rng, 900), _entry(rng, 400, lo=5)])
    X = _features(rng, len(C), cin)
    m = _student(pl, cin, hidden, seed=hidden).eval()
    Cd = torch.from_numpy(C).cuda()
    with torch.no_grad():
        out = m(ME.SparseTensor(features=X.cuda(), coordinates=Cd))
    assert out.C is Cd
    E = out.F
    assert E.dtype == torch.float32 and E.shape == (len(C), 128) and E.is_cuda
    E64 = _oracle_raw(X.double(), _oracle_map(C), {k: v.cpu() for k, v in m.state_dict().items()})
    Ec = E.cpu().double()
    # the bound of test_f16x3_student_chain_vs_fp64_oracle on the normalised rows, and on the row norms relative to each row
    assert (F.normalize(Ec, dim=1) - F.normalize(E64, dim=1)).abs().max().item() <= 1e-5
    n, n64 = Ec.norm(dim=1), E64.norm(dim=1)
    assert ((n - n64).abs() / n64).max().item() <= 1e-5
    # the rows of StudentWeights(raw=True) on the existing order and map of each entry, bit for bit
    st = m.device_weights(torch.device("cuda"))
    assert st.fast == (hidden % 256 == 0)
    for b in range(2):
        idx = np.where(C[:, 0] == b)[0]
        c = torch.from_numpy(C[idx, 1:]).cuda().contiguous()
        perm, rank = ops.morton_order(c)
        cs = c[perm.long()].contiguous()
        nm = ops.kernel_map_build(ops.grid_build(cs), cs)
        Xd = torch.zeros((len(idx), st.cin_pad), device="cuda")
        Xd[:, :cin] = X[idx].cuda()[perm.long()]
        raw = st.forward(Xd, nm, raw=True)[rank.long()]
        assert torch.equal(raw, E[torch.from_numpy(idx).cuda()])


# ------------------------------------------------------------------------------------------ 3. batching
def test_batch_entries_independent_and_row_order(env):
    ops, pl, ME = env
    rng = np.random.default_rng(30)
    a = _entry(rng, 800)
    entries = [a, np.array([[7, -3, 2]], np.int32), a + np.array([0, 2, 0], np.int32), _entry(rng, 300, lo=-2)]
    C = _batched(rng, entries)
    X = _features(rng, len(C), 518).cuda()
    m = _student(pl, 518, 256, seed=3).eval()
    assert m.device_weights(torch.device("cuda")).fast
    Cd = torch.from_numpy(C).cuda()
    with torch.no_grad():
        E = m(ME.SparseTensor(features=X, coordinates=Cd)).F
        for b in range(len(entries)):
            idx = torch.from_numpy(np.where(C[:, 0] == b)[0]).cuda()
            alone = m(ME.SparseTensor(features=X[idx], coordinates=Cd[idx])).F
            assert torch.equal(alone, E[idx]), b
        sh = torch.randperm(len(C), device="cuda")
        E_sh = m(ME.SparseTensor(features=X[sh], coordinates=Cd[sh])).F
    assert torch.equal(E_sh, E[sh])


# ------------------------------------------------------------------------------------------ 4. train mode
def _morton_scene(ops, rng, n):
    """one entry whose rows are already in Morton order"""
    xyz = torch.from_numpy(_entry(rng, n)).cuda().contiguous()
    perm, _ = ops.morton_order(xyz)
    return xyz[perm.long()].contiguous()


def test_train_mode_matches_student_trainer_bit_for_bit(env):
    ops, pl, ME = env
    from geopurify_amd.training import StudentTrainer
    rng = np.random.default_rng(40)
    cs = _morton_scene(ops, rng, 900)
    N = cs.shape[0]
    X = _features(rng, N, 518).cuda()
    m = _student(pl, 518, 256, seed=4).train()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    A, Nn = 32, 7
    s2v = torch.randperm(N, device="cuda")
    p2b = torch.randint(0, N, (A * (2 + Nn),), device="cuda")
    out = m(ME.SparseTensor(features=X, coordinates=ME.utils.batched_coordinates([cs], device="cuda")))
    loss, dE = ops.infonce_fwd_bwd(out.F.detach().contiguous(), s2v, p2b, A, Nn, 0.07)
    out.F.backward(dE)

    tr = StudentTrainer(sd0, "cuda", bn_momentum=0.1, bn_eps=1e-5)
    Xd = torch.zeros((N, tr.cin_pad), device="cuda")
    Xd[:, :518] = X
    nm = ops.kernel_map_build(ops.grid_build(cs), cs)
    # (the InfoNCE kernel's sums are not bitwise repeatable: the trainer's step is handed the same loss and dE)
    infonce = ops.infonce_fwd_bwd
    try:
        ops.infonce_fwd_bwd = lambda e, *a: (loss, dE) if torch.equal(e, out.F) else infonce(e, *a)
        loss2, g2, E2 = tr.forward_backward(Xd, nm, s2v, p2b, A, Nn)
    finally:
        ops.infonce_fwd_bwd = infonce
    assert torch.equal(out.F, E2) and loss2 is loss
    for name, p in m.named_parameters():
        g = g2[name][:, :518] if name == "input_layer.0.kernel" else g2[name]
        assert torch.equal(p.grad, g.view_as(p)), name
    for name, b in m.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(sd0[name]) + 1, name
        else:
            assert torch.equal(b, tr.buffers[name]), name


def _keep_relu_outputs(ops, monkeypatch):
    """every BatchNorm + ReLU output of the device's forward (fp32 rows, sorted order), in the oracle's ReLU order"""
    outs = []
    apply = ops.bn_train_apply

    def keeping_apply(*a, **k):
        k["want_f32"] = True
        o, sp = apply(*a, **k)
        outs.append(o)
        return o, sp
    monkeypatch.setattr(ops, "bn_train_apply", keeping_apply)
    return outs


def _objective(E, R):
    return (E * R).sum() / E.shape[0] + 0.5 * (E * E).mean()


def _grad_case(ops, pl, ME, monkeypatch, seed, hidden, cin, train):
    """one forward + backward of the module (B = 2, shuffled rows, x.F requiring grad) and of the fp64 oracle with the device's ReLU
    decisions; returns (relative / absolute errors, differing ReLU decisions)"""
    rng = np.random.default_rng(1000 + seed)
    C = _batched(rng, [_entry(rng, 500), _entry(rng, 300, lo=2)])
    N = len(C)
    X = _features(rng, N, cin)
    R = torch.from_numpy(rng.normal(0, 1, size=(N, 128)))
    m = _student(pl, cin, hidden, seed=seed).train(train)
    sd0 = {k: v.clone().cpu() for k, v in m.state_dict().items()}
    Cd = torch.from_numpy(C).cuda()
    Xd = X.cuda().requires_grad_(True)
    outs = _keep_relu_outputs(ops, monkeypatch)
    out = m(ME.SparseTensor(features=Xd, coordinates=Cd))
    monkeypatch.undo()
    loss = _objective(out.F, R.float().cuda())
    loss.backward()
    rank = ops.coords_order_batched(Cd.contiguous())[1].long()
    masks = [(o[rank] > 0).cpu() for o in outs]
    assert len(masks) == 9

    nm = _oracle_map(C)
    params = {k: v.double().clone().requires_grad_(True) for k, v in sd0.items()
              if k.endswith("kernel") or k.endswith(".bn.weight") or k.endswith(".bn.bias")}
    X64 = X.double().requires_grad_(True)
    pre = []
    if train:
        bn_state = {k[:-len(".bn.running_mean")]: (v.double().clone(), sd0[k.replace("running_mean", "running_var")].double().clone())
                    for k, v in sd0.items() if k.endswith("running_mean")}
        E64 = o_train.student_train_forward(X64, nm, params, bn_state, 4, momentum=0.1, relu_masks=masks, relu_inputs=pre)
    else:
        p = dict(params)
        p.update({k: v.double() for k, v in sd0.items() if "running" in k})
        E64 = _eval_forward64(X64, nm, p, masks, pre)
    loss64 = _objective(E64, R)
    loss64.backward()
    flips = 0
    for mk, pr, o in zip(masks, pre, outs):
        o = o[rank].cpu().double()
        pre_err = float((o - pr)[mk].abs().max())
        differ = mk != (pr > 0)
        assert (pr[differ].abs() <= 4 * pre_err).all()
        flips += int(differ.sum())
    err = {"loss": abs(float(loss) - float(loss64)) / abs(float(loss64)),
           "dF": float((Xd.grad.cpu().double() - X64.grad).abs().max() / X64.grad.abs().max())}
    for name, p in m.named_parameters():
        g64 = params[name].grad
        err["grad:" + name] = float((p.grad.cpu().double() - g64).abs().max() / g64.abs().max())
    for name, b in m.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(sd0[name]) + (1 if train else 0), name
            continue
        if not train:
            assert torch.equal(b.cpu(), sd0[name]), name            # eval mode updates nothing
            continue
        prefix, which = name.rsplit(".bn.", 1)
        ref = bn_state[prefix][0 if which == "running_mean" else 1]
        err["running:" + name] = float((b.cpu().double() - ref).abs().max())
    return err, flips


def _eval_forward64(X, nm, p, masks, pre):
    """AffinityPredictor.forward in fp64 with eval BatchNorm under autograd; ReLU(x) = x * mask (the device's decisions)"""
    it = iter(masks)

    def relu(x):
        pre.append(x.detach())
        return x * next(it).to(x.dtype)

    def bn(x, prefix):
        return F.batch_norm(x, p[prefix + ".bn.running_mean"], p[prefix + ".bn.running_var"], p[prefix + ".bn.weight"],
                            p[prefix + ".bn.bias"], training=False, eps=o_student.BN_EPS)

    def conv(x, name):
        W = p[name]
        out = torch.zeros((x.shape[0], W.shape[2]), dtype=x.dtype)
        for k in range(27):
            mk = torch.from_numpy(nm[k])
            rows = torch.where(mk >= 0)[0]
            if len(rows):
                out = out.index_add(0, rows, x[mk[rows]] @ W[k])
        return out
    out = relu(bn(conv(X, "input_layer.0.kernel"), "input_layer.1"))
    for i in range(4):
        idt = out
        o = relu(bn(conv(out, f"res_blocks.{i}.conv1.kernel"), f"res_blocks.{i}.norm1"))
        o = bn(conv(o, f"res_blocks.{i}.conv2.kernel"), f"res_blocks.{i}.norm2")
        out = relu(o + idt)
    return out @ p["output_layer.kernel"]


# the largest error of eight seeds (1000 + 0..7) per quantity and case, measured on the MI355X; every bound is 3x that.  Relative to the
# fp64 reference's maximum for the loss, dF and the gradients, absolute for the running statistics.
GRAD_MEASURED = {
    "train-256-518": {
        "loss": 3.941e-7, "dF": 1.070e-6, "grad:input_layer.0.kernel": 9.685e-7,
        "grad:input_layer.1.bn.weight": 1.407e-6, "grad:input_layer.1.bn.bias": 1.201e-6, "grad:res_blocks.0.conv1.kernel": 1.321e-6,
        "grad:res_blocks.0.norm1.bn.weight": 1.226e-6, "grad:res_blocks.0.norm1.bn.bias": 1.025e-6, "grad:res_blocks.0.conv2.kernel": 1.494e-6,
        "grad:res_blocks.0.norm2.bn.weight": 1.193e-6, "grad:res_blocks.0.norm2.bn.bias": 7.887e-7, "grad:res_blocks.1.conv1.kernel": 1.176e-6,
        "grad:res_blocks.1.norm1.bn.weight": 1.272e-6, "grad:res_blocks.1.norm1.bn.bias": 7.762e-7, "grad:res_blocks.1.conv2.kernel": 1.317e-6,
        "grad:res_blocks.1.norm2.bn.weight": 1.129e-6, "grad:res_blocks.1.norm2.bn.bias": 5.966e-7, "grad:res_blocks.2.conv1.kernel": 1.592e-6,
        "grad:res_blocks.2.norm1.bn.weight": 1.994e-6, "grad:res_blocks.2.norm1.bn.bias": 6.582e-7, "grad:res_blocks.2.conv2.kernel": 1.361e-6,
        "grad:res_blocks.2.norm2.bn.weight": 1.410e-6, "grad:res_blocks.2.norm2.bn.bias": 4.525e-7, "grad:res_blocks.3.conv1.kernel": 1.321e-6,
        "grad:res_blocks.3.norm1.bn.weight": 1.375e-6, "grad:res_blocks.3.norm1.bn.bias": 7.265e-7, "grad:res_blocks.3.conv2.kernel": 1.381e-6,
        "grad:res_blocks.3.norm2.bn.weight": 1.477e-6, "grad:res_blocks.3.norm2.bn.bias": 3.290e-7, "grad:output_layer.kernel": 1.061e-6,
        "running:input_layer.1.bn.running_mean": 2.681e-8, "running:input_layer.1.bn.running_var": 1.426e-7, "running:res_blocks.0.norm1.bn.running_mean": 2.750e-8,
        "running:res_blocks.0.norm1.bn.running_var": 1.459e-7, "running:res_blocks.0.norm2.bn.running_mean": 2.541e-8, "running:res_blocks.0.norm2.bn.running_var": 1.426e-7,
        "running:res_blocks.1.norm1.bn.running_mean": 3.834e-8, "running:res_blocks.1.norm1.bn.running_var": 1.419e-7, "running:res_blocks.1.norm2.bn.running_mean": 2.104e-8,
        "running:res_blocks.1.norm2.bn.running_var": 1.426e-7, "running:res_blocks.2.norm1.bn.running_mean": 3.211e-8, "running:res_blocks.2.norm1.bn.running_var": 1.440e-7,
        "running:res_blocks.2.norm2.bn.running_mean": 2.216e-8, "running:res_blocks.2.norm2.bn.running_var": 1.450e-7, "running:res_blocks.3.norm1.bn.running_mean": 2.337e-8,
        "running:res_blocks.3.norm1.bn.running_var": 1.520e-7, "running:res_blocks.3.norm2.bn.running_mean": 2.647e-8, "running:res_blocks.3.norm2.bn.running_var": 1.464e-7,
    },
    "train-128-38": {
        "loss": 4.205e-7, "dF": 7.188e-7, "grad:input_layer.0.kernel": 1.693e-6,
        "grad:input_layer.1.bn.weight": 6.671e-7, "grad:input_layer.1.bn.bias": 7.108e-7, "grad:res_blocks.0.conv1.kernel": 1.237e-6,
        "grad:res_blocks.0.norm1.bn.weight": 5.885e-7, "grad:res_blocks.0.norm1.bn.bias": 6.109e-7, "grad:res_blocks.0.conv2.kernel": 1.193e-6,
        "grad:res_blocks.0.norm2.bn.weight": 6.072e-7, "grad:res_blocks.0.norm2.bn.bias": 4.527e-7, "grad:res_blocks.1.conv1.kernel": 1.166e-6,
        "grad:res_blocks.1.norm1.bn.weight": 8.879e-7, "grad:res_blocks.1.norm1.bn.bias": 5.381e-7, "grad:res_blocks.1.conv2.kernel": 9.577e-7,
        "grad:res_blocks.1.norm2.bn.weight": 6.651e-7, "grad:res_blocks.1.norm2.bn.bias": 3.344e-7, "grad:res_blocks.2.conv1.kernel": 1.425e-6,
        "grad:res_blocks.2.norm1.bn.weight": 6.323e-7, "grad:res_blocks.2.norm1.bn.bias": 5.111e-7, "grad:res_blocks.2.conv2.kernel": 1.411e-6,
        "grad:res_blocks.2.norm2.bn.weight": 8.083e-7, "grad:res_blocks.2.norm2.bn.bias": 3.005e-7, "grad:res_blocks.3.conv1.kernel": 1.189e-6,
        "grad:res_blocks.3.norm1.bn.weight": 5.810e-7, "grad:res_blocks.3.norm1.bn.bias": 4.087e-7, "grad:res_blocks.3.conv2.kernel": 9.509e-7,
        "grad:res_blocks.3.norm2.bn.weight": 7.052e-7, "grad:res_blocks.3.norm2.bn.bias": 2.562e-7, "grad:output_layer.kernel": 1.275e-6,
        "running:input_layer.1.bn.running_mean": 3.092e-8, "running:input_layer.1.bn.running_var": 1.427e-7, "running:res_blocks.0.norm1.bn.running_mean": 2.490e-8,
        "running:res_blocks.0.norm1.bn.running_var": 1.399e-7, "running:res_blocks.0.norm2.bn.running_mean": 1.632e-8, "running:res_blocks.0.norm2.bn.running_var": 1.370e-7,
        "running:res_blocks.1.norm1.bn.running_mean": 2.332e-8, "running:res_blocks.1.norm1.bn.running_var": 1.441e-7, "running:res_blocks.1.norm2.bn.running_mean": 1.827e-8,
        "running:res_blocks.1.norm2.bn.running_var": 1.450e-7, "running:res_blocks.2.norm1.bn.running_mean": 2.100e-8, "running:res_blocks.2.norm1.bn.running_var": 1.467e-7,
        "running:res_blocks.2.norm2.bn.running_mean": 2.478e-8, "running:res_blocks.2.norm2.bn.running_var": 1.416e-7, "running:res_blocks.3.norm1.bn.running_mean": 2.062e-8,
        "running:res_blocks.3.norm1.bn.running_var": 1.381e-7, "running:res_blocks.3.norm2.bn.running_mean": 2.362e-8, "running:res_blocks.3.norm2.bn.running_var": 1.400e-7,
    },
    "eval-256-518": {
        "loss": 2.990e-6, "dF": 5.807e-7, "grad:input_layer.0.kernel": 9.928e-7,
        "grad:input_layer.1.bn.weight": 1.070e-6, "grad:input_layer.1.bn.bias": 6.163e-7, "grad:res_blocks.0.conv1.kernel": 1.123e-6,
        "grad:res_blocks.0.norm1.bn.weight": 1.144e-6, "grad:res_blocks.0.norm1.bn.bias": 8.187e-7, "grad:res_blocks.0.conv2.kernel": 1.108e-6,
        "grad:res_blocks.0.norm2.bn.weight": 6.046e-7, "grad:res_blocks.0.norm2.bn.bias": 5.493e-7, "grad:res_blocks.1.conv1.kernel": 1.320e-6,
        "grad:res_blocks.1.norm1.bn.weight": 1.114e-6, "grad:res_blocks.1.norm1.bn.bias": 9.031e-7, "grad:res_blocks.1.conv2.kernel": 9.773e-7,
        "grad:res_blocks.1.norm2.bn.weight": 5.603e-7, "grad:res_blocks.1.norm2.bn.bias": 4.444e-7, "grad:res_blocks.2.conv1.kernel": 1.163e-6,
        "grad:res_blocks.2.norm1.bn.weight": 1.179e-6, "grad:res_blocks.2.norm1.bn.bias": 6.768e-7, "grad:res_blocks.2.conv2.kernel": 8.300e-7,
        "grad:res_blocks.2.norm2.bn.weight": 4.777e-7, "grad:res_blocks.2.norm2.bn.bias": 3.912e-7, "grad:res_blocks.3.conv1.kernel": 1.080e-6,
        "grad:res_blocks.3.norm1.bn.weight": 6.968e-7, "grad:res_blocks.3.norm1.bn.bias": 8.646e-7, "grad:res_blocks.3.conv2.kernel": 8.802e-7,
        "grad:res_blocks.3.norm2.bn.weight": 4.027e-7, "grad:res_blocks.3.norm2.bn.bias": 2.962e-7, "grad:output_layer.kernel": 7.532e-7,
    },
    "eval-128-38": {
        "loss": 4.098e-5, "dF": 3.745e-7, "grad:input_layer.0.kernel": 1.258e-6,
        "grad:input_layer.1.bn.weight": 4.699e-7, "grad:input_layer.1.bn.bias": 2.754e-7, "grad:res_blocks.0.conv1.kernel": 1.090e-6,
        "grad:res_blocks.0.norm1.bn.weight": 5.760e-7, "grad:res_blocks.0.norm1.bn.bias": 4.083e-7, "grad:res_blocks.0.conv2.kernel": 1.119e-6,
        "grad:res_blocks.0.norm2.bn.weight": 3.119e-7, "grad:res_blocks.0.norm2.bn.bias": 3.306e-7, "grad:res_blocks.1.conv1.kernel": 1.528e-6,
        "grad:res_blocks.1.norm1.bn.weight": 4.149e-7, "grad:res_blocks.1.norm1.bn.bias": 3.601e-7, "grad:res_blocks.1.conv2.kernel": 1.244e-6,
        "grad:res_blocks.1.norm2.bn.weight": 3.045e-7, "grad:res_blocks.1.norm2.bn.bias": 2.941e-7, "grad:res_blocks.2.conv1.kernel": 1.021e-6,
        "grad:res_blocks.2.norm1.bn.weight": 8.130e-7, "grad:res_blocks.2.norm1.bn.bias": 3.059e-7, "grad:res_blocks.2.conv2.kernel": 1.186e-6,
        "grad:res_blocks.2.norm2.bn.weight": 7.222e-7, "grad:res_blocks.2.norm2.bn.bias": 2.725e-7, "grad:res_blocks.3.conv1.kernel": 1.157e-6,
        "grad:res_blocks.3.norm1.bn.weight": 7.604e-7, "grad:res_blocks.3.norm1.bn.bias": 3.221e-7, "grad:res_blocks.3.conv2.kernel": 1.182e-6,
        "grad:res_blocks.3.norm2.bn.weight": 2.559e-7, "grad:res_blocks.3.norm2.bn.bias": 2.621e-7, "grad:output_layer.kernel": 1.053e-6,
    },
    "train-256-512": {
        "loss": 5.234e-7, "dF": 9.663e-7, "grad:input_layer.0.kernel": 9.939e-7,
        "grad:input_layer.1.bn.weight": 1.113e-6, "grad:input_layer.1.bn.bias": 1.101e-6, "grad:res_blocks.0.conv1.kernel": 1.175e-6,
        "grad:res_blocks.0.norm1.bn.weight": 1.270e-6, "grad:res_blocks.0.norm1.bn.bias": 9.864e-7, "grad:res_blocks.0.conv2.kernel": 1.242e-6,
        "grad:res_blocks.0.norm2.bn.weight": 1.390e-6, "grad:res_blocks.0.norm2.bn.bias": 7.832e-7, "grad:res_blocks.1.conv1.kernel": 1.341e-6,
        "grad:res_blocks.1.norm1.bn.weight": 1.451e-6, "grad:res_blocks.1.norm1.bn.bias": 9.281e-7, "grad:res_blocks.1.conv2.kernel": 1.337e-6,
        "grad:res_blocks.1.norm2.bn.weight": 1.252e-6, "grad:res_blocks.1.norm2.bn.bias": 7.047e-7, "grad:res_blocks.2.conv1.kernel": 1.469e-6,
        "grad:res_blocks.2.norm1.bn.weight": 1.531e-6, "grad:res_blocks.2.norm1.bn.bias": 8.941e-7, "grad:res_blocks.2.conv2.kernel": 1.303e-6,
        "grad:res_blocks.2.norm2.bn.weight": 1.240e-6, "grad:res_blocks.2.norm2.bn.bias": 4.837e-7, "grad:res_blocks.3.conv1.kernel": 1.551e-6,
        "grad:res_blocks.3.norm1.bn.weight": 1.616e-6, "grad:res_blocks.3.norm1.bn.bias": 8.869e-7, "grad:res_blocks.3.conv2.kernel": 1.326e-6,
        "grad:res_blocks.3.norm2.bn.weight": 1.505e-6, "grad:res_blocks.3.norm2.bn.bias": 2.426e-7, "grad:output_layer.kernel": 1.189e-6,
        "running:input_layer.1.bn.running_mean": 1.769e-8, "running:input_layer.1.bn.running_var": 1.425e-7, "running:res_blocks.0.norm1.bn.running_mean": 2.264e-8,
        "running:res_blocks.0.norm1.bn.running_var": 1.409e-7, "running:res_blocks.0.norm2.bn.running_mean": 2.644e-8, "running:res_blocks.0.norm2.bn.running_var": 1.444e-7,
        "running:res_blocks.1.norm1.bn.running_mean": 2.143e-8, "running:res_blocks.1.norm1.bn.running_var": 1.487e-7, "running:res_blocks.1.norm2.bn.running_mean": 2.361e-8,
        "running:res_blocks.1.norm2.bn.running_var": 1.399e-7, "running:res_blocks.2.norm1.bn.running_mean": 2.391e-8, "running:res_blocks.2.norm1.bn.running_var": 1.497e-7,
        "running:res_blocks.2.norm2.bn.running_mean": 1.951e-8, "running:res_blocks.2.norm2.bn.running_var": 1.464e-7, "running:res_blocks.3.norm1.bn.running_mean": 3.581e-8,
        "running:res_blocks.3.norm1.bn.running_var": 1.713e-7, "running:res_blocks.3.norm2.bn.running_mean": 2.739e-8, "running:res_blocks.3.norm2.bn.running_var": 1.434e-7,
    },
    "eval-256-512": {
        "loss": 2.716e-6, "dF": 5.995e-7, "grad:input_layer.0.kernel": 7.441e-7,
        "grad:input_layer.1.bn.weight": 8.534e-7, "grad:input_layer.1.bn.bias": 5.961e-7, "grad:res_blocks.0.conv1.kernel": 1.313e-6,
        "grad:res_blocks.0.norm1.bn.weight": 1.466e-6, "grad:res_blocks.0.norm1.bn.bias": 1.131e-6, "grad:res_blocks.0.conv2.kernel": 1.068e-6,
        "grad:res_blocks.0.norm2.bn.weight": 7.830e-7, "grad:res_blocks.0.norm2.bn.bias": 5.874e-7, "grad:res_blocks.1.conv1.kernel": 1.148e-6,
        "grad:res_blocks.1.norm1.bn.weight": 9.052e-7, "grad:res_blocks.1.norm1.bn.bias": 1.022e-6, "grad:res_blocks.1.conv2.kernel": 8.052e-7,
        "grad:res_blocks.1.norm2.bn.weight": 7.605e-7, "grad:res_blocks.1.norm2.bn.bias": 4.474e-7, "grad:res_blocks.2.conv1.kernel": 9.980e-7,
        "grad:res_blocks.2.norm1.bn.weight": 9.426e-7, "grad:res_blocks.2.norm1.bn.bias": 7.884e-7, "grad:res_blocks.2.conv2.kernel": 1.302e-6,
        "grad:res_blocks.2.norm2.bn.weight": 4.602e-7, "grad:res_blocks.2.norm2.bn.bias": 3.659e-7, "grad:res_blocks.3.conv1.kernel": 1.104e-6,
        "grad:res_blocks.3.norm1.bn.weight": 8.503e-7, "grad:res_blocks.3.norm1.bn.bias": 6.143e-7, "grad:res_blocks.3.conv2.kernel": 7.089e-7,
        "grad:res_blocks.3.norm2.bn.weight": 5.288e-7, "grad:res_blocks.3.norm2.bn.bias": 2.606e-7, "grad:output_layer.kernel": 6.601e-7,
    },
}
GRAD_BOUNDS = {case: {k: 3 * v for k, v in errs.items()} for case, errs in GRAD_MEASURED.items()}


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
# (cin 512: a padded input width that is a multiple of 256 and differs from the hidden width -- dF on the exact-fp32 kernel there too)
@pytest.mark.parametrize("hidden,cin", [(256, 518), (128, 38), (256, 512)])
def test_autograd_vs_fp64(env, monkeypatch, hidden, cin, train):
    ops, pl, ME = env
    case = f"{'train' if train else 'eval'}-{hidden}-{cin}"
    bounds = GRAD_BOUNDS[case]
    err, flips = _grad_case(ops, pl, ME, monkeypatch, 0, hidden, cin, train)
    assert flips <= 10, flips
    assert set(err) == set(bounds)
    for k, e in err.items():
        assert e <= bounds[k], (case, k, e, bounds[k])


def test_backward_twice_needs_retain_graph(env):
    """the activations are saved tensors of the autograd node: a second backward works with retain_graph=True (the gradients add up)
    and raises autograd's own error without it"""
    ops, pl, ME = env
    rng = np.random.default_rng(45)
    C = torch.from_numpy(_batched(rng, [_entry(rng, 300), _entry(rng, 200, lo=3)])).cuda()
    X = _features(rng, len(C), 518).cuda().requires_grad_(True)
    m = _student(pl, 518, 256, seed=5).train()
    R = torch.randn(len(C), 128, device="cuda")
    loss = _objective(m(ME.SparseTensor(features=X, coordinates=C)).F, R)
    loss.backward(retain_graph=True)
    once = [p.grad.clone() for p in m.parameters()] + [X.grad.clone()]
    loss.backward()
    for g1, g2 in zip(once, [p.grad for p in m.parameters()] + [X.grad]):
        assert torch.allclose(g2, 2 * g1, rtol=1e-5, atol=1e-6 * float(g1.abs().max()))
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        loss.backward()


def test_input_checks_on_device(env):
    ops, pl, ME = env
    rng = np.random.default_rng(46)
    xyz = _entry(rng, 60)
    C = np.c_[np.zeros(60, np.int32), xyz]
    X = torch.zeros(60, 38, device="cuda")
    m = _student(pl, 38, 128, 2).eval()
    # an int64 coordinate beyond int32 must not wrap into a valid one
    C64 = torch.from_numpy(C.astype(np.int64)).cuda()
    C64[5, 1] += 2 ** 32
    with pytest.raises(ValueError, match="int32 range"), torch.no_grad():
        m(ME.SparseTensor(features=X, coordinates=C64))
    with torch.no_grad():                                                   # in range: the same result as int32
        assert torch.equal(m(ME.SparseTensor(features=X, coordinates=torch.from_numpy(C.astype(np.int64)).cuda())).F,
                           m(ME.SparseTensor(features=X, coordinates=torch.from_numpy(C).cuda())).F)
    # batch 65536 has the key of batch 0: the range is reported, not a duplicate
    Cb = np.concatenate([C, C[[4]]])
    Cb[-1, 0] = 65536
    with pytest.raises(ValueError, match="batch index"), torch.no_grad():
        m(ME.SparseTensor(features=torch.zeros(61, 38, device="cuda"), coordinates=torch.from_numpy(Cb).cuda()))
    # one momentum and one eps for all nine BatchNorm layers; no cumulative average in train mode
    Cd = torch.from_numpy(C).cuda()
    m.res_blocks[1].norm2.bn.eps = 1e-3
    with pytest.raises(ValueError, match="different eps"), torch.no_grad():
        m(ME.SparseTensor(features=X, coordinates=Cd))
    m.res_blocks[1].norm2.bn.eps = 1e-5
    m.train()
    m.res_blocks[0].norm1.bn.momentum = 0.2
    with pytest.raises(ValueError, match="different momenta"):
        m(ME.SparseTensor(features=X, coordinates=Cd))
    for b in m.modules():
        if isinstance(b, torch.nn.BatchNorm1d):
            b.momentum = None
    with pytest.raises(ValueError, match="momentum=None"):
        m(ME.SparseTensor(features=X, coordinates=Cd))


def test_train_mode_multi_rank_raises(env, monkeypatch):
    ops, pl, ME = env
    from geopurify_amd import sharding
    monkeypatch.setattr(sharding, "_world", lambda group=None: 2)
    rng = np.random.default_rng(50)
    C = _batched(rng, [_entry(rng, 40)])
    m = _student(pl, 38, 128, 1).train()
    with pytest.raises(NotImplementedError, match="SonataXAffinityTrainer.forward"):
        m(ME.SparseTensor(features=torch.zeros(len(C), 38, device="cuda"), coordinates=torch.from_numpy(C).cuda()))


# ------------------------------------------------------------------------------------------ 6. drop-in through compat/
def test_compat_drop_in_matches_hot_path_student(env):
    ops, pl, ME = env
    rng = np.random.default_rng(60)
    xyz = _entry(rng, 1500).astype(np.float32) + rng.uniform(0, 0.99, size=(1500, 3)).astype(np.float32)   # floored by batched_coordinates
    X = _features(rng, 1500, 518).cuda()
    m = _student(pl, 518, 512, seed=6).eval()
    with torch.no_grad():
        E = F.normalize(m(ME.SparseTensor(features=X, coordinates=ME.utils.batched_coordinates([torch.from_numpy(xyz)], device="cuda"))).F)
    # HotPath's student: its Morton order, grid map and pairs, the fused normalising head
    st = m.device_weights(torch.device("cuda"))
    c = torch.from_numpy(np.floor(xyz).astype(np.int32)).cuda().contiguous()
    perm, rank = ops.morton_order(c)
    cs = c[perm.long()].contiguous()
    nm = ops.kernel_map_build(ops.grid_build(cs), cs)
    Xd = torch.zeros((len(xyz), st.cin_pad), device="cuda")
    Xd[:, :518] = X[perm.long()]
    hp = st.forward(Xd, nm)[rank.long()]
    assert (E - hp).abs().max().item() <= 1e-6
