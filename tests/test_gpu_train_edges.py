"""The training-step kernels (csrc/train.hip) at their path, tie and extent edges.

The cases and their references come from tests/train_cases.py; tests/test_train_cases_host.py proves without a device which branch
each case takes.  Integer outputs (the sampler's and the kNN's) are compared exactly, no case and no element excused; the float
kernels against fp64 at the bound of each kernel's older test, or at a bound derived beside it.  Wherever the pitches allow, a case
runs twice -- on plain tensors and inside extent fences (tests/extent_fence.py) with workspaces of exactly the reported bytes -- and
the two runs must agree bit for bit (the InfoNCE outputs, summed by atomics: within their bound).  Every case is inside the ranges
include/geopurify_hip.h allows or is refused by the argument checks before anything is launched.
"""
import ctypes

import numpy as np
import pytest
import torch

import train_cases as tc
from extent_fence import INT_VIEW, POISON, Arena, assert_intact, run, unwritten

pytestmark = pytest.mark.gpu

F16, F32, F64, I32, I64, U8 = torch.float16, torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
GP_EINVAL = -22
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from geopurify_amd import _lib
    from geopurify_amd import ops as _ops
    _lib.load()                      # fails loudly if the HIP library is missing
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from geopurify_amd import _lib
    return _lib.load()


def ok(lib, rc):
    assert rc == 0, (rc, lib.gp_last_error().decode())


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def T(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)) if not torch.is_tensor(a) else a
    return t.to(dtype) if dtype is not None else t


def poisoned(shape, dtype):
    return torch.full(shape, POISON["out"][dtype], dtype=INT_VIEW[dtype], device="cuda").view(dtype)


def refused(lib, rc, *outs):
    """the call returned GP_EINVAL and launched nothing: every output still holds its poison"""
    torch.cuda.synchronize()
    assert rc == GP_EINVAL, (rc, lib.gp_last_error().decode())
    for o in outs:
        assert unwritten(o) == o.numel()


class Pitched:
    """Rows of ANY pitch (extent_fence.fenced wants a multiple of 16 bytes): rows x pitch elements inside one flat fence, the pitch
    columns poisoned; check() asserts that they still are.  Plain run: contiguous rows."""

    def __init__(self, a, rows, cols, pitch, dtype, src=None, name=None):
        self.pads = None
        if not a.fence:
            self.v = src.cuda().contiguous().clone() if src is not None else a.out((rows, cols), dtype)
            return
        self.poison = POISON["in" if src is not None else "out"][dtype]
        full = torch.full((rows, pitch), self.poison, dtype=INT_VIEW[dtype]).view(dtype)
        if src is not None:
            full[:, :cols] = src
        flat = a.inp(full.reshape(-1), name=name).view(rows, pitch)
        self.v, self.pads, self.name = flat[:, :cols], flat[:, cols:], name

    def check(self):
        if self.pads is not None:
            assert bool((self.pads.contiguous().view(INT_VIEW[self.pads.dtype]) == self.poison).all()), f"{self.name}: a pitch column changed"


# ------------------------------------------------------------------------------------------ A. gp_sampler_select
@pytest.mark.parametrize("name", tc.SAMPLER_CASES)
def test_sampler_select_edges(lib, name):
    """every LG instance at its first and last n, the hand-over of the vector loop to the tail loop, the smallest and largest k, the
    anchor's placements, ties, -0, infinities and NaNs, and the two sides of the candidate cap: exact against the header's rule.  sim
    (NaN in its pitch columns) is not written."""
    c = tc.sampler_case(name)
    sim, anchors, k, ld = c["sim"], c["anchors"], c["k"], c["ld"]
    A, n = sim.shape
    rp, rm = tc.select_reference(sim, anchors, k)
    full = torch.full((A, ld), float("nan"))
    full[:, :n] = T(sim)

    def case(a):
        buf = a.inp(full.reshape(-1), name="sim")                      # one flat fence: any pitch, the pitch columns NaN
        before = buf.view(I32).clone()
        anc = a.inp(T(anchors), name="anchors")
        pos, macro = a.out(A, I64, name="positive"), a.out((A, k), I64, name="macro")
        ok(lib, lib.gp_sampler_select(P(buf), ld, A, n, P(anc), k, P(pos), P(macro), S()))
        torch.cuda.synchronize()
        assert torch.equal(buf.view(I32), before)
        return {"positive": pos, "macro": macro}

    got = run(case)
    assert np.array_equal(got["positive"].cpu().numpy(), rp)
    bad = np.argwhere(got["macro"].cpu().numpy() != rm)
    assert len(bad) == 0, (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("k,n,what", tc.SAMPLER_REFUSED)
def test_sampler_select_refuses(lib, k, n, what):
    ld = (n + 4) & ~3
    buf, anc = torch.zeros((1, ld), device="cuda"), torch.zeros(1, dtype=I64, device="cuda")
    pos, macro = poisoned((1,), I64), poisoned((1, k), I64)
    refused(lib, lib.gp_sampler_select(P(buf), ld, 1, n, P(anc), k, P(pos), P(macro), S()), pos, macro)


# ------------------------------------------------------------------------------------------ B. gp_knn_points_f32
def knn_call(lib, a, c, flag=None):
    xyz, q = a.inp(T(c["xyz"]), name="xyz"), a.inp(T(c["queries"]), name="queries")
    out = a.out((len(c["queries"]), c["k"]), I64, name="out")
    flag = a.out(1, I32, name="flag") if flag is None else flag
    ok(lib, lib.gp_knn_points_f32(P(xyz), len(c["xyz"]), P(q), len(c["queries"]), c["k"], P(out), P(flag), S()))
    return {"out": out, "flag": flag}


@pytest.mark.parametrize("name", [n for n, w in tc.KNN_CASES.items() if w != "flagged"])
def test_knn_points_edges(lib, name):
    """the smallest legal sizes, 1 / 3 / 4 / 5 queries (a last workgroup of 1 to 3), a repeated query, rows 0 and n - 1, a lattice
    whose distances tie, coincident points and an underflowing cluster (handed back to the single-query kernel), offset coordinates:
    flag 0 and the oracle's rows exactly"""
    c = tc.knn_case(name)
    got = run(lambda a: knn_call(lib, a, c))
    assert int(got["flag"].item()) == 0
    bad = np.argwhere(got["out"].cpu().numpy() != tc.knn_reference(c))
    assert len(bad) == 0, (len(bad), bad[:4].tolist())


def test_knn_points_flags_more_coincident_points_than_the_cap_and_clears_the_flag_on_the_next_call(lib):
    """2100 points at the query's location: the (k+1)-th histogram bin exceeds the cap, the flag is set and the kernel returns early by
    design (out is unspecified then).  A clean call on the same flag tensor leaves 0."""
    flag = torch.zeros(1, dtype=I32, device="cuda")
    knn_call(lib, Arena(False), tc.knn_case("coincident_2100"), flag)
    torch.cuda.synchronize()
    assert int(flag.item()) != 0
    c = tc.knn_case("coincident_2")
    got = knn_call(lib, Arena(False), c, flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and np.array_equal(got["out"].cpu().numpy(), tc.knn_reference(c))


@pytest.mark.parametrize("n,k,what", tc.KNN_REFUSED)
def test_knn_points_refuses(lib, n, k, what):
    xyz, q = torch.rand((n, 3), device="cuda"), torch.zeros(1, dtype=I64, device="cuda")
    out, flag = poisoned((1, k), I64), poisoned((1,), I32)
    refused(lib, lib.gp_knn_points_f32(P(xyz), n, P(q), 1, k, P(out), P(flag), S()), out, flag)


# ------------------------------------------------------------------------------------------ C. gp_infonce_fwd_bwd
def nce_call(lib, a, c, calls=1):
    e, s2v, p2b, A, Nn = c["e"], c["s2v"], c["p2b"], c["A"], c["Nn"]
    nv, d = e.shape
    pe = Pitched(a, nv, d, d + 4, F32, src=e, name="e")
    pde = Pitched(a, nv, d, d + 8, F32, name="de")
    s, p = a.inp(s2v, name="sample_to_voxel"), a.inp(p2b, name="point_to_batch")
    loss = a.out(1, F32, name="loss")
    ws = a.out(lib.gp_infonce_workspace_bytes(len(s2v), d), U8, name="workspace")
    for _ in range(calls):
        ok(lib, lib.gp_infonce_fwd_bwd(P(pe.v), pe.v.stride(0), nv, d, P(s), len(s2v), P(p), A, Nn, tc.NCE_T, P(loss), P(pde.v), pde.v.stride(0),
                                       P(ws), ws.numel(), S()))
    torch.cuda.synchronize()
    assert_intact(*a.fences)
    pe.check(), pde.check()
    return float(loss.item()), pde.v.detach().cpu().double()


@pytest.mark.parametrize("name", tc.NCE_CASES)
def test_infonce_edges_vs_fp64(lib, name):
    """d = 1 .. 256 (every fill of the four strided slots), 0 .. 63 negatives, 1 .. 5 anchors (a last workgroup of 1 to 3 waves),
    repeated samples, one voxel row under 64 samples, rows no sample points at, a zero row: loss and dE against fp64 autograd at the
    bound of test_infonce_forward_backward, with ld_e = d + 4 and ld_de = d + 8 in the fenced run; two calls give one loss.
    (all_equal_map measured 1.075 of the dE bound while the gradient rows were summed by fp32 atomics -- the gradient is 0 there and
    the rounding of the largest partial sum stayed; summed in fp64 it measures 0.000.  DESIGN 10.1 lists every case's ratio.)"""
    c = tc.nce_case(name)
    loss_ref, de_ref = tc.nce_reference(c)
    b_loss, b_de = tc.nce_bounds(loss_ref, de_ref)
    worst = [0.0, 0.0]
    for fence, calls in ((False, 1), (True, 1), (False, 2)):
        loss, de = nce_call(lib, Arena(fence), c, calls)
        worst = [max(worst[0], abs(loss - loss_ref) / b_loss), max(worst[1], float((de - de_ref).abs().max()) / b_de)]
        touched = torch.zeros(de.shape[0], dtype=torch.bool)
        touched[c["s2v"]] = True
        assert not de[~touched].any()                                  # rows no sample points at: exactly 0.0
    print(f"infonce {name}: loss error / bound {worst[0]:.3f}, dE error / bound {worst[1]:.3f}")
    assert worst[0] < 1.0 and worst[1] < 1.0, worst
    if name in ("all_equal_map", "one_voxel_row"):
        assert abs(loss - np.log(1 + c["Nn"])) < b_loss


@pytest.mark.parametrize("d,negatives,what", tc.NCE_REFUSED)
def test_infonce_refuses(lib, d, negatives, what):
    e, s2v = torch.zeros((4, d), device="cuda"), torch.zeros(4, dtype=I64, device="cuda")
    p2b = torch.zeros(2 + negatives, dtype=I64, device="cuda")
    loss, de, ws = poisoned((1,), F32), poisoned((4, d), F32), torch.empty(1 << 16, dtype=U8, device="cuda")
    refused(lib, lib.gp_infonce_fwd_bwd(P(e), d, 4, d, P(s2v), 4, P(p2b), 1, negatives, tc.NCE_T, P(loss), P(de), d, P(ws), ws.numel(), S()), loss, de)


# ------------------------------------------------------------------------------------------ D. gp_adamw_step
@pytest.mark.parametrize("step", tc.ADAMW_STEPS)
@pytest.mark.parametrize("n", tc.ADAMW_N)
def test_adamw_one_step_vs_fp64(lib, n, step):
    """one step from given (p, m, v, g) against the formula in fp64 on the same fp32 inputs: one element, one fewer and one more than
    the 256-thread workgroup; the first steps and one at which both bias corrections round to 1; with and without weight decay; an
    element whose denominator is eps alone and one with p = 0.  |p - ref| <= 2^-22 (|p_ref| + |update_ref|) (the kernel's roughly
    eight rounded fp32 operations), m and v within 2^-22 relative (train_cases.ADAMW_REL)."""
    p0, m0, v0, g0 = tc.adamw_case(n, step)
    lr, (b1, b2), eps = tc.ADAMW_LR, tc.ADAMW_BETAS, tc.ADAMW_EPS
    for wd in tc.ADAMW_WD:
        def case(a):
            p, m, v, g = (a.inp(T(x), name=nm) for x, nm in ((p0, "p"), (m0, "m"), (v0, "v"), (g0, "g")))
            ok(lib, lib.gp_adamw_step(P(p), P(g), P(m), P(v), n, lr, b1, b2, eps, wd, step, S()))
            return {"p": p, "m": m, "v": v, "g": g}

        got = {k: x.cpu().numpy().astype(np.float64) for k, x in run(case).items()}
        pr, mr, vr, ur = tc.adamw_reference(p0, m0, v0, g0, step, wd)
        rp = float(np.max(np.abs(got["p"] - pr) / (tc.ADAMW_REL * (np.abs(pr) + np.abs(ur)))))
        rm = float(np.max(np.abs(got["m"] - mr) / (tc.ADAMW_REL * np.abs(mr))))
        rv = float(np.max(np.abs(got["v"] - vr) / (tc.ADAMW_REL * np.abs(vr) + 1e-300)))
        print(f"adamw n={n} step={step} wd={wd}: error / bound p {rp:.3f}, m {rm:.3f}, v {rv:.3f}")
        assert np.array_equal(got["g"], g0.astype(np.float64))
        assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0, (rp, rm, rv)
        # the kernel's own operations in IEEE fp32, as train_cases restates them: the same bits
        pk, mk, vk = tc.adamw_kernel_model(p0, m0, v0, g0, step, wd)
        assert np.array_equal(got["m"], mk.astype(np.float64)) and np.array_equal(got["v"], vk.astype(np.float64))


# ------------------------------------------------------------------------------------------ E. gp_normalize_split_f16
def norm_check(lib, x, n_pad):
    n, d = x.shape
    ld_h = (d + 8 + 7) // 8 * 8

    def case(a):
        xs = a.inp(x, d + 4, "x")
        hi, lo = a.out((n_pad, d), F16, ld_h, "hi"), a.out((n_pad, d), F16, ld_h, "lo")
        ok(lib, lib.gp_normalize_split_f16(P(xs), xs.stride(0), d, n, n_pad, 1e-12, P(hi), P(lo), hi.stride(0), S()))
        return {"hi": hi, "lo": lo}

    got = run(case)
    y = got["hi"].cpu().double() + got["lo"].cpu().double()
    assert unwritten(got["hi"]) == 0 and unwritten(got["lo"]) == 0
    assert not got["hi"][n:].any() and not got["lo"][n:].any()          # pad rows: exactly zero
    zero = (x == 0).all(1)
    assert not y[:n][zero].any()
    err = float((y[:n] - tc.norm_reference(x)).abs().max())
    assert err < tc.NORM_BOUND, err


@pytest.mark.parametrize("n", tc.NORM_N)
@pytest.mark.parametrize("d", tc.NORM_D)
def test_normalize_split_edges_vs_fp64(lib, d, n):
    """d = 4 (one lane), one float4 fewer than / exactly / one more than a 256-column sweep, the product's 1088; 1 to 5 rows (a last
    workgroup of 1 to 3 waves); with and without pad rows; ld_x > d and ld_h > d in the fenced run; a zero row"""
    x = tc.norm_case(n, d)
    for n_pad in (n, n + 3):
        norm_check(lib, x, n_pad)


def test_normalize_split_more_rows_than_waves(lib):
    """n_pad = 16389 at d = 4: the grid is capped at 16384 waves, so the stride loop takes real rows and pad rows a second time"""
    n, n_pad, d = tc.NORM_STRIDE_CASE
    norm_check(lib, tc.norm_case(n, d), n_pad)


@pytest.mark.parametrize("what", ["d = 6", "misaligned x"])
def test_normalize_split_refuses(lib, what):
    d = 6 if what == "d = 6" else 8
    buf = torch.ones(4 * 16 + 1, device="cuda")
    x = buf[1:] if what == "misaligned x" else buf
    hi, lo = poisoned((4, 16), F16), poisoned((4, 16), F16)
    refused(lib, lib.gp_normalize_split_f16(P(x), 16, d, 4, 4, 1e-12, P(hi), P(lo), 16, S()), hi, lo)


# ------------------------------------------------------------------------------------------ F. the BatchNorm entry points, fenced
BN_EPS, BN_MOM = 1e-5, 0.1


def bn_case(nv, c):
    """the inputs of test_batchnorm_training_kernels_vs_fp64: column 1 has mean ~ 1e3 sigma (cancellation in E[x^2] - mean^2)"""
    g = torch.Generator().manual_seed(31 * nv + c)
    y = torch.randn(nv, c, generator=g) * 2 + 0.5
    y[:, 1] = 1e3 + torch.randn(nv, generator=g)
    res, dout = torch.randn(nv, c, generator=g), torch.randn(nv, c, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1
    rm, rv = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    return y, res, dout, gamma, beta, rm, rv


def f64_of(t):
    """an fp64 output handed out as its int64 image (the fences poison integer patterns)"""
    return t.view(F64).cpu()


@pytest.mark.parametrize("c", [6, 128, 512])               # the scalar path (c % 4 != 0), half a 256-column block of the vector path, two
@pytest.mark.parametrize("nv", [1, 255, 257])              # CS_ROWS = 256 rows per workgroup of the column reductions: one fewer, one more
def test_batchnorm_entry_points_fenced_vs_fp64(lib, nv, c):
    """gp_col_stats, gp_col_sums_f64 (both forms), gp_bn_train_apply (fp32 + split + running statistics; split planes only),
    gp_bn_train_backward (dy; dy + scale; the split planes with their zero row nv) with both mask sources (act, beta_mask),
    gp_bn_bwd_sums_f64 and gp_bn_bwd_apply: plain and fenced (pitch c + 4; c = 6: 8; f16 planes c + 8), workspaces at exactly the
    reported bytes, the two runs bit for bit, values against fp64 at the bounds of test_batchnorm_training_kernels_vs_fp64."""
    y, res, dout, gamma, beta, rm, rv = bn_case(nv, c)
    ld, ld_h = (c + 4 if c % 4 == 0 else 8), c + 8
    ws_stats = lib.gp_col_stats_workspace_bytes(nv, c)

    def stats(a):
        ys, mean, var = a.inp(y, ld, "y"), a.out(c, F32, name="mean"), a.out(c, F32, name="var")
        ws = a.out(ws_stats, U8, name="workspace")
        ok(lib, lib.gp_col_stats(P(ys), ys.stride(0), nv, c, P(mean), P(var), P(ws), ws.numel(), S()))
        return {"mean": mean, "var": var}

    st = run(stats)
    mean, var = st["mean"], st["var"]
    y64 = y.double()
    m64 = y64.mean(0)
    v64 = ((y64 - m64) ** 2).mean(0)
    f64_sum = (256 + nv / 256 + 4) * 2.0 ** -53                          # an fp64 sum of 256-row blocks, relative to the sum of |terms|
    assert ((mean.cpu().double() - m64).abs() <= U32 * m64.abs() + 1e-12).all()
    assert ((var.cpu().double() - v64).abs() <= 2 * U32 * v64 + f64_sum * (m64 ** 2 + v64)).all()
    if nv == 1:
        assert torch.equal(mean.cpu(), y[0]) and not var.any()

    # ---- the SyncBatchNorm reduction vectors: exact fp32 terms (or squares of exact differences, rounded once) summed in fp64
    def sums(a, with_mean):
        ys, out = a.inp(y, ld, "y"), a.out(c, I64, name="out")
        mn = a.inp(mean, name="mean") if with_mean else None
        ws = a.out(ws_stats, U8, name="workspace")
        ok(lib, lib.gp_col_sums_f64(P(ys), ys.stride(0), nv, c, P(mn), P(out), P(ws), ws.numel(), S()))
        return {"out": out}

    s0 = f64_of(run(lambda a: sums(a, False))["out"])
    assert ((s0 - y64.sum(0)).abs() <= f64_sum * y64.abs().sum(0)).all()
    s1 = f64_of(run(lambda a: sums(a, True))["out"])
    sq = (y64 - mean.cpu().double()) ** 2
    assert ((s1 - sq.sum(0)).abs() <= (f64_sum + 2.0 ** -52) * sq.sum(0)).all()

    sigma = (v64 + BN_EPS).sqrt()
    kappa = (y64.abs().max(0).values + m64.abs()) / sigma                # magnitude at which xhat is rounded
    g64, b64 = gamma.double(), beta.double()
    xhat = (y64 - m64) / sigma
    pre1, pre2 = g64 * xhat + b64 + res.double(), g64 * xhat + b64
    tol_out = 8 * U32 * (g64.abs() * kappa + b64.abs() + res.double().abs().max(0).values)

    # ---- forward: residual + fp32 + split + running statistics; no residual, fp32 + split; the split planes alone (a layer whose mask
    # comes from y), which must be the planes of the call before
    def apply(a, full, want_out=True):
        ys, mn, vr, ga, be = a.inp(y, ld, "y"), a.inp(mean, name="mean"), a.inp(var, name="var"), a.inp(gamma, name="gamma"), a.inp(beta, name="beta")
        rs = a.inp(res, ld, "residual") if full else None
        out = a.out((nv, c), F32, ld, "out") if want_out else None
        hi = a.out((nv, c), F16, ld_h, "hi") if c % 4 == 0 else None
        lo = a.out((nv, c), F16, ld_h, "lo") if c % 4 == 0 else None
        r_m, r_v = (a.inp(rm, name="running_mean"), a.inp(rv, name="running_var")) if full else (None, None)
        ok(lib, lib.gp_bn_train_apply(P(ys), ys.stride(0), nv, c, P(mn), P(vr), P(ga), P(be), BN_EPS, P(rs), rs.stride(0) if full else 0, 1,
                                      P(out), out.stride(0) if out is not None else 0, P(hi), P(lo), hi.stride(0) if hi is not None else 0,
                                      BN_MOM, P(r_m), P(r_v), S()))
        outs = {"out": out, "hi": hi, "lo": lo, "running_mean": r_m, "running_var": r_v}
        return {k: v for k, v in outs.items() if v is not None}

    f1, f2 = run(lambda a: apply(a, True)), run(lambda a: apply(a, False))
    acts = []
    for f, pre in ((f1, pre1), (f2, pre2)):
        o = f["out"]
        assert unwritten(o) == 0 and torch.isfinite(o).all()
        assert ((o.cpu().double() - pre.clamp(min=0)).abs() <= tol_out).all()
        if "hi" in f:
            assert unwritten(f["hi"]) == 0 and unwritten(f["lo"]) == 0
            assert ((f["hi"].float() + f["lo"].float()) - o).abs().max() <= 2.0 ** -21 * max(float(o.abs().max()), 1e-30)
        acts.append(o)
    if c % 4 == 0:
        f3 = run(lambda a: apply(a, False, want_out=False))
        assert torch.equal(f3["hi"], f2["hi"]) and torch.equal(f3["lo"], f2["lo"])
    unb = v64 * nv / (nv - 1) if nv > 1 else v64
    assert ((f1["running_mean"].cpu().double() - ((1 - BN_MOM) * rm.double() + BN_MOM * m64)).abs() <= 8 * U32 * (rm.double().abs() + m64.abs())).all()
    assert ((f1["running_var"].cpu().double() - ((1 - BN_MOM) * rv.double() + BN_MOM * unb)).abs() <= 8 * U32 * (rv.double().abs() + unb)).all()

    # ---- backward.  The ReLU masks are the kernel's own (see test_batchnorm_training_kernels_vs_fp64); elsewhere they equal fp64's
    def reference(M):
        dz = dout.double() * M
        if nv == 1:                                                      # xhat = 0: dbeta = dz, dgamma = 0, dy = 0
            return torch.zeros_like(dz), torch.zeros(c, dtype=F64), dz[0].clone(), dz
        yr, gr, br = y64.clone().requires_grad_(True), g64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
        bn = torch.nn.functional.batch_norm(yr, None, None, gr, br, training=True, eps=BN_EPS)
        dy, dg, db = torch.autograd.grad(bn, [yr, gr, br], dz)
        return dy, dg, db, dz

    ws_bwd = lib.gp_bn_train_backward_workspace_bytes(nv, c)
    for source, act_t, pre in (("act", acts[0], pre1), ("beta_mask", None, pre2)):
        M = acts[0 if source == "act" else 1].cpu() > 0
        assert ((M == (pre > 0)) | (pre.abs() <= tol_out)).all()
        dy_r, dg_r, db_r, dz_r = reference(M)
        az, xa = dz_r.abs(), xhat.abs()
        tol_db64, tol_dg64 = f64_sum * az.sum(0), 2 * U32 * (az * (kappa + xa)).sum(0)
        tol_db, tol_dg = U32 * db_r.abs() + tol_db64, U32 * dg_r.abs() + tol_dg64
        tol_dy = 8 * U32 * g64.abs() / sigma * (az.max(0).values + az.sum(0) / nv + (kappa + xa.max(0).values) * (az * (kappa + xa)).sum(0) / nv)

        def common(a):
            d = {"dout": a.inp(dout, ld, "dout"), "y": a.inp(y, ld, "y"), "mean": a.inp(mean, name="mean"), "var": a.inp(var, name="var"),
                 "gamma": a.inp(gamma, name="gamma")}
            d["act"] = a.inp(act_t, ld, "act") if source == "act" else None
            d["beta"] = a.inp(beta, name="beta") if source == "beta_mask" else None
            return d

        def backward(a, form):
            d = common(a)
            dy = a.out((nv, c), F32, ld, "dy") if form != "split" else None
            hi = a.out((nv + 1, c), F16, ld_h, "dy_hi") if form == "split" else None
            lo = a.out((nv + 1, c), F16, ld_h, "dy_lo") if form == "split" else None
            dz = a.out((nv, c), F32, ld, "dz")
            dg, db = a.out(c, F32, name="dgamma"), a.out(c, F32, name="dbeta")
            sc = a.out(2, F32, name="dy_scale2") if form != "dy" else None
            ws = a.out(ws_bwd, U8, name="workspace")
            ok(lib, lib.gp_bn_train_backward(P(d["dout"]), d["dout"].stride(0), P(d["act"]), d["act"].stride(0) if d["act"] is not None else 0,
                                             P(d["y"]), d["y"].stride(0), P(d["mean"]), P(d["var"]), BN_EPS, P(d["gamma"]), P(d["beta"]), nv, c,
                                             P(dy), dy.stride(0) if dy is not None else 0, P(dz), dz.stride(0), P(dg), P(db), P(sc), P(hi), P(lo),
                                             hi.stride(0) if hi is not None else 0, P(ws), ws.numel(), S()))
            outs = {"dy": dy, "dy_hi": hi, "dy_lo": lo, "dz": dz, "dgamma": dg, "dbeta": db, "scale": sc}
            return {k: v for k, v in outs.items() if v is not None}

        first = None
        for form in ("dy", "dy_scale", "split") if c % 4 == 0 else ("dy", "dy_scale"):
            b = run(lambda a: backward(a, form))
            assert torch.equal(b["dz"].cpu(), dout * M.float()), (source, form)
            assert ((b["dgamma"].cpu().double() - dg_r).abs() <= tol_dg).all() and ((b["dbeta"].cpu().double() - db_r).abs() <= tol_db).all(), (source, form)
            if form == "split":
                sc, sh, sl = b["scale"], b["dy_hi"], b["dy_lo"]
                assert float(sc[0] * sc[1]) == 1.0 and not sh[nv].any() and not sl[nv].any()
                dys = ((sh[:nv].double() + sl[:nv].double()) * float(sc[1])).cpu()
                assert ((dys - dy_r).abs() <= tol_dy + 2.0 ** -18 * dy_r.abs().max()).all(), (source, form)
            else:
                assert unwritten(b["dy"]) == 0 and ((b["dy"].cpu().double() - dy_r).abs() <= tol_dy).all(), (source, form)
                if form == "dy_scale":
                    s = float(b["scale"][0])
                    amax = float(b["dy"].abs().max())
                    assert float(b["scale"][0] * b["scale"][1]) == 1.0 and np.log2(s) == round(np.log2(s))
                    assert torch.equal(b["dy"], first["dy"]) and (amax == 0 or np.isfinite(s * amax))
            if first is None:
                first = b
            else:
                assert torch.equal(b["dgamma"], first["dgamma"]) and torch.equal(b["dbeta"], first["dbeta"])
            if nv == 1 and form != "split":
                assert not b["dy"].any() and not b["dgamma"].any() and torch.equal(b["dbeta"].cpu(), dz_r[0].float())

        def bwd_sums(a):
            d = common(a)
            out, ws = a.out(2 * c, I64, name="sums"), a.out(ws_stats, U8, name="workspace")
            ok(lib, lib.gp_bn_bwd_sums_f64(P(d["dout"]), d["dout"].stride(0), P(d["act"]), d["act"].stride(0) if d["act"] is not None else 0,
                                           P(d["y"]), d["y"].stride(0), P(d["mean"]), P(d["var"]), BN_EPS, P(d["gamma"]) if d["beta"] is not None else None,
                                           P(d["beta"]), nv, c, P(out), P(ws), ws.numel(), S()))
            return {"sums": out}

        s = f64_of(run(bwd_sums)["sums"])
        assert ((s[:c] - db_r).abs() <= tol_db64).all() and ((s[c:] - dg_r).abs() <= tol_dg64 + 1e-300).all(), source
        s32 = s.float()

        def bwd_apply(a):
            d = common(a)
            sm = a.inp(s32, name="sums")
            dy, dz = a.out((nv, c), F32, ld, "dy"), a.out((nv, c), F32, ld, "dz")
            ok(lib, lib.gp_bn_bwd_apply(P(d["dout"]), d["dout"].stride(0), P(d["act"]), d["act"].stride(0) if d["act"] is not None else 0,
                                        P(d["y"]), d["y"].stride(0), P(d["mean"]), P(d["var"]), BN_EPS, P(d["gamma"]), P(d["beta"]), P(sm), nv, nv, c,
                                        P(dy), dy.stride(0), P(dz), dz.stride(0), None, S()))
            return {"dy": dy, "dz": dz}

        ap = run(bwd_apply)
        assert torch.equal(ap["dz"].cpu(), dout * M.float()) and ((ap["dy"].cpu().double() - dy_r).abs() <= tol_dy).all(), source


# ------------------------------------------------------------------------------------------ F. gp_conv_wgrad_f16x3, fenced
@pytest.mark.parametrize("cin_pad", [256, 544])
def test_conv_weight_gradient_pair_counts_fenced_vs_fp64(ops, lib, cin_pad):
    """offsets of 0, 1, 32 and 33 pairs (no segment; one pair and 31 padded ones; a full step; a full step and a second segment of one
    pair), steps_per_segment = 1, the cin_pad / cout of test_conv_weight_gradient_kernel: plain and fenced (rows of cin_pad + 8 and
    cout + 8 halves, the workspace at exactly the reported bytes), bit for bit, and against an fp64 gather-GEMM at that test's bound"""
    rng = np.random.default_rng(77 + cin_pad)
    nv, cout, counts = 40, 256, (0, 1, 32, 33)
    pairs = [(torch.from_numpy(rng.integers(0, nv, m)).cuda(), torch.from_numpy(rng.integers(0, nv, m)).cuda()) for m in counts]   # (out, in)
    plan = ops.wgrad_plan_build(pairs, nv, steps_per_segment=1)
    assert plan.num_segments == 4 and plan.seg_off.tolist() == [0, 0, 1, 2, 4]
    X = torch.randn(nv, cin_pad, device="cuda")
    dY = torch.randn(nv, cout, device="cuda") * 3e-5                     # gradient-sized values (need the power-of-two scaling)
    s = 2.0 ** 14
    dys = torch.zeros((nv + 1, cout), device="cuda")
    dys[:nv] = dY * s
    (xh, xl), (yh, yl) = ops.split_f16(X), ops.split_f16(dys)
    inv = torch.tensor([1.0 / s])
    kv = len(counts)
    ws_bytes = lib.gp_conv_wgrad_workspace_bytes(plan.num_segments, cin_pad, cout)

    def case(a):
        xs = [a.inp(t, cin_pad + 8, nm) for t, nm in ((xh, "x_hi"), (xl, "x_lo"))]
        ys = [a.inp(t, cout + 8, nm) for t, nm in ((yh, "y_hi"), (yl, "y_lo"))]
        pin, pout = a.inp(plan.pair_in, name="pair_in"), a.inp(plan.pair_out, name="pair_out")
        segs, seg_off = a.inp(plan.segs.reshape(-1), name="segs"), a.inp(plan.seg_off, name="seg_off")
        isc = a.inp(inv, name="inv_scale")
        dw, ws = a.out(kv * cin_pad * cout, F32, name="dw"), a.out(ws_bytes, U8, name="workspace")
        ok(lib, lib.gp_conv_wgrad_f16x3(P(xs[0]), P(xs[1]), xs[0].stride(0), P(ys[0]), P(ys[1]), ys[0].stride(0), P(pin), P(pout), P(segs),
                                        plan.num_segments, P(seg_off), kv, cin_pad, cin_pad, cout, P(isc), P(dw), P(ws), ws.numel(), S()))
        return {"dw": dw}

    dw = run(case)["dw"]
    assert unwritten(dw) == 0
    dw = dw.view(kv, cin_pad, cout).double()
    assert not dw[0].any()                                               # an offset without pairs: exactly zero
    Xd, Yd = X.double(), dY.double()
    for k, (o, i) in enumerate(pairs[1:], start=1):
        ref = Xd[i].t() @ Yd[o]
        err = float((dw[k] - ref).abs().max() / ref.abs().max())
        assert err < 2e-6, (k, err)                                      # fp32-class: 2^-22 split error, fp32 accumulation
