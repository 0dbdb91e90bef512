"""Cases for the training-step kernels (csrc/train.hip) and their references.  Plain numpy and fp64 torch on the CPU, no device code.

Shared by the CPU checks (test_train_cases_host.py: every case reaches the branch it is named for, and its reference is unambiguous)
and the kernel tests (test_gpu_train_edges.py).  A case is built when it is asked for (the largest sampler rows are 12.5 MB each) and
is a function of its name alone.

The references state the rules as include/geopurify_hip.h does:
  sampler  positive = arg-max over the points other than the anchor, the lowest index among equals; macro = the k points of lowest
           similarity other than the anchor and the positive, ascending by (value, index); -0 counts as +0; a NaN (sign bit clear)
           orders above +inf -- so the first NaN is the positive and NaNs come last among the low values
  kNN      oracle.train.knn_points_bruteforce: (d^2 in fp64 of the fp32 coordinates, row id), the lowest entry dropped
  InfoNCE  oracle.train.info_nce in float64 with autograd
  AdamW    torch.optim.AdamW written out in fp64 on the fp32 images of its inputs, the hyper-parameters included (the ABI takes them
           as floats: 1 - 0.999f is 1.3e-5 off 0.001, which is the caller's rounding, not the kernel's)
  normalise  fp64 F.normalize

The models below restate the branch conditions of train.hip (the constants are the kernel's) so that a case can prove which path it
takes without a device.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import train as o_train

f32, f64 = np.float32, np.float64

# ------------------------------------------------------------------------------------------ sampler: constants and model
SR_NT, SR_CAP, SR_GROUPS = 1024, 2048, 12288
SR_N_MAX = SR_GROUPS * 256


def sampler_lg(n):
    """the LG instance gp_sampler_select launches for a row of n elements: 4 << lg elements per group, the fewest that fit LDS"""
    lg = 0
    while (((n + 3) >> 2) + (1 << lg) - 1) >> lg > SR_GROUPS:
        lg += 1
    return lg


def sampler_key(v):
    """the order-preserving uint image of a float (sr_key): -0 counts as +0, a NaN with a clear sign bit orders above +inf"""
    u = np.ascontiguousarray(v, dtype=f32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def sampler_vector_slots(n, vec):
    """number of float4 slots the 4-slot vector loop of wave w reads (w = 0..15), the rest being the tail loop's"""
    out = []
    for w in range(SR_NT // 64):
        f0, nfull = 64 * w, n >> 2
        while vec and f0 + 3 * SR_NT + 64 <= nfull:
            f0 += 4 * SR_NT
        out.append((f0 - 64 * w) // SR_NT)
    return out


def sampler_model(row, anchor, k, positive):
    """(bound key, number of candidates): the (k+1)-th lowest of the 1024 thread minima (thread = the element's float4 slot mod 1024,
    the anchor left out) and the count of elements at or below it other than the anchor and the positive"""
    key = sampler_key(row)
    idx = np.arange(len(row))
    sel = idx != anchor
    tmin = np.full(SR_NT, 0xFFFFFFFF, dtype=np.uint32)
    np.minimum.at(tmin, ((idx >> 2) & (SR_NT - 1))[sel], key[sel])
    bound = np.sort(tmin)[k]
    return int(bound), int(((key <= bound) & sel & (idx != positive)).sum())


def select_reference(sim, anchors, k):
    """positive i64 [A], macro i64 [A, k] by the header's rule (a stable sort: equal values stay in index order, NaNs last)"""
    A, n = sim.shape
    pos = np.empty(A, dtype=np.int64)
    macro = np.empty((A, k), dtype=np.int64)
    idx = np.arange(n)
    for a in range(A):
        row = sim[a] + f32(0.0)                                      # -0 -> +0
        m = row.astype(f64)
        m[anchors[a]] = -np.inf
        pos[a] = int(np.argmax(m))                                    # numpy: the first NaN if there is one, else the first maximum
        rest = idx[(idx != anchors[a]) & (idx != pos[a])]
        macro[a] = rest[np.argsort(row[rest], kind="stable")[:k]]
    return pos, macro


def _pitch(n, kind):
    if kind == "vector":                                              # rows a lane can read 16 bytes at a time, with pitch columns
        return (n + 4) & ~3
    if kind == "odd":                                                 # rows that start at any 4-byte address: the scalar path
        return (n + 1) | 1
    return n                                                          # "tight"


SAMPLER_LG_N = (49152, 49153, 98305, 150000, 196609, 393217, 786433, 1572865)
SAMPLER_HANDOVER_N = (4 * 4095 + 1, 4 * 4096, 4 * 4096 + 2, 4 * 4097 + 3)
SAMPLER_CASES = tuple(
    [f"lg_n{n}" for n in SAMPLER_LG_N] + ["lg_n3145728", "odd_n150000", "odd_n49153"] + [f"handover_n{n}" for n in SAMPLER_HANDOVER_N] +
    ["k1_n3", "k1023_n1025", "anchor_places", "all_equal", "signed_zeros", "inf_nan", "cap_2048", "cap_2049", "far_block"])
# (k, n, what) the entry point refuses before any launch
SAMPLER_REFUSED = ((48, SR_N_MAX + 1, "n above the maximum"), (1024, 5000, "k = 1024"), (48, 49, "n = k + 1"))


def sampler_case(name):
    """dict(sim f32 [A, n], anchors i64 [A], k, ld)"""
    rng = np.random.default_rng(hash_name(name))
    k, pitch = 48, "vector"
    if name.startswith(("lg_n", "odd_n", "handover_n")):
        n = int(name.split("_n")[1])
        A = 2 if name.startswith("lg_n") else 3
        sim = (rng.standard_normal((A, n)) * 0.03).astype(f32)
        anchors = rng.integers(0, n, A)
        pitch = "odd" if name.startswith("odd_n") else ("tight" if n == SR_N_MAX else "vector")
    elif name == "k1_n3":
        k, sim, anchors = 1, np.array([[0.5, -0.25, 0.125], [1.0, 2.0, 3.0], [-1.0, -1.0, -1.0]], dtype=f32), np.array([0, 2, 1])
    elif name == "k1023_n1025":
        k, sim, anchors = 1023, rng.standard_normal((3, 1025)).astype(f32), np.array([0, 1024, 513])
    elif name == "anchor_places":
        n = 5000
        sim = rng.standard_normal((4, n)).astype(f32)
        order = np.argsort(sim, axis=1, kind="stable")
        anchors = np.array([0, n - 1, order[2, -1], order[3, 4]])    # first, last, the row's maximum, one of the k lowest values
    elif name == "all_equal":
        sim, anchors = np.full((3, 5000), 0.25, dtype=f32), np.array([0, 4999, 77])
    elif name == "signed_zeros":
        n = 5000
        sim = (rng.random((3, n), dtype=f32) + f32(0.5))
        for a in range(3):
            z = rng.choice(n, 60, replace=False)
            sim[a, z[:30]], sim[a, z[30:]] = f32(-0.0), f32(0.0)
        anchors = np.array([int(np.flatnonzero(sim[0] == 0)[0]), 17, 4000])
    elif name == "inf_nan":
        n, k = 60, 58                                                # k = n - 2: every selectable element is ranked
        sim = rng.standard_normal((4, n)).astype(f32)
        sim[:, [3, 20, 41]], sim[:, [5, 19, 50]] = -np.inf, np.inf
        sim[0, 30] = np.nan
        sim[1, [7, 8, 33, 44, 59]] = np.nan
        sim[2, [10, 11, 12]] = np.nan
        sim[3, [0, 58]] = np.nan
        anchors = np.array([2, 19, 10, 3])                           # an ordinary value, a +inf, the first NaN, a -inf
    elif name in ("cap_2048", "cap_2049"):
        n, m = 50001, int(name[4:])
        sim = rng.random((3, n), dtype=f32)
        sim[:, 1000:1000 + m] = -1.0                                 # equal lowest values in 512 threads' slots: the bound is their key
        anchors = np.array([5, 40000, 50000])                        # outside the block, and the positive is a value in [0, 1)
    elif name == "far_block":
        n = 1572865
        sim = rng.random((2, n), dtype=f32)
        sim[:, n - 9000:] = -1.0                                     # 9000 equal lowest values whose indices differ in high bits only
        anchors = np.array([n - 4500, 12])
    else:
        raise KeyError(name)
    return dict(sim=sim, anchors=anchors.astype(np.int64), k=k, ld=_pitch(sim.shape[1], pitch))


def hash_name(name):
    return zlib.crc32(name.encode())


# ------------------------------------------------------------------------------------------ kNN: constants and model
KQ_CAP, KP_CAP, KP_BINS = 512, 2048, 2048


def kp_bin(d2):
    """the histogram bin of a squared distance: the bits of its float image shifted right by 20"""
    return (np.asarray(d2, dtype=f64).astype(f32).view(np.uint32) >> 20).astype(np.int64)


def knn_model(xyz, q, k):
    """What gp_knn_points_f32 does with query row q: dict(handed_back, over_cap, flagged).
    handed_back: the 4-query kernel returns the query to the single-query kernel (more than KQ_CAP candidates under the fp32 bound of
    the 256 thread minima, or that bound below 1e-30); only for k + 1 <= 256.  over_cap: the single-query kernel finds more than KP_CAP
    points under its fp64 bound and takes the histogram.  flagged: the (k+1)-th histogram bin holds more than KP_CAP points."""
    n = len(xyz)
    x32 = np.asarray(xyz, dtype=f32)
    d = x32 - x32[q]
    s32 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]                 # fp32, left to right, no contraction
    x64 = x32.astype(f64)
    e = x64 - x64[q]
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    out = dict(handed_back=False, over_cap=False, flagged=False)
    multi = k + 1 <= 256
    if multi:
        tm = np.full(256, np.inf, dtype=f32)
        np.minimum.at(tm, np.arange(n) % 256, s32)
        b32 = np.sort(tm)[k]
        cnt = int(((s32 <= b32 * (f32(1) + f32(2.0 ** -18))) & (d2 <= f64(b32) * (1.0 + 2.0 ** -19))).sum())
        out["handed_back"] = bool(cnt > KQ_CAP or not b32 >= f32(1e-30))
        if not out["handed_back"]:
            return out
    nt = 256 if multi else 1024
    tm = np.full(nt, np.inf)
    np.minimum.at(tm, np.arange(n) % nt, d2)
    bound = np.sort(tm)[k]
    if int((d2 <= bound).sum()) > KP_CAP:
        out["over_cap"] = True
        run = np.cumsum(np.bincount(kp_bin(d2), minlength=KP_BINS))
        t = int(np.argmax(run >= k + 1))
        out["flagged"] = bool(run[t] > KP_CAP)
    return out


def _cloud(rng, n):
    return (rng.random((n, 3)) * np.array([7, 5, 2.6])).astype(f32)


def _coincident_ids(m, n):
    """m ids below n that fall into distinct threads (id mod 256) as far as m allows, so that k + 1 thread minima are 0"""
    i = np.arange(m)
    ids = (i % 256) + 256 * ((i // 256) + 9 * (i % 8) + 1)              # (same thread: same i % 8, another i // 256)
    assert ids.max() < n and len(np.unique(ids)) == m
    return ids


# name -> expectation: "plain" (answered by the first kernel), "handed_back", "flagged"
KNN_CASES = {
    "n97_k96": "plain", "n256_k255": "plain", "n257_k256": "plain", "n1024_k1023": "plain",
    "n255_k16_q1": "plain", "n256_k16_q3": "plain", "n257_k16_q4": "plain", "n1023_k16_q5": "plain", "n1025_k16_q1": "plain",
    "lattice_k96": "plain", "coincident_2": "plain", "coincident_97": "handed_back", "coincident_600": "handed_back",
    "coincident_2048": "handed_back", "coincident_2100": "flagged", "underflow_k16": "handed_back", "offset_1000": "plain",
}
KNN_REFUSED = ((1025, 1024, "k = 1024"), (97, 97, "k = n"))              # (n, k, what)


def knn_case(name):
    """dict(xyz f32 [n, 3], queries i64, k, named: the queries the case's name speaks of (indices into queries))"""
    rng = np.random.default_rng(hash_name(name))
    named = None
    if name.startswith("n"):
        parts = name.split("_")
        n, k = int(parts[0][1:]), int(parts[1][1:])
        xyz = _cloud(rng, n)
        nq = int(parts[2][1:]) if len(parts) > 2 else 3
        q = {1: [n - 1] if n == 1025 else [0], 3: [0, n - 1, 7], 4: [0, n - 1, 5, 5], 5: [0, n - 1, 3, 3, n // 2]}[nq]   # rows 0 and n - 1, a repeated id
    elif name == "lattice_k96":
        g = np.arange(12)
        xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)
        k, q = 96, [0, 1727, 800, 801, 13]
    elif name.startswith("coincident_"):
        m, n, k = int(name.split("_")[1]), 20000, 96
        xyz = _cloud(rng, n)
        ids = _coincident_ids(m, n)
        xyz[ids] = np.array([3.5, 2.5, 1.25], dtype=f32)
        others = np.setdiff1d(np.arange(n), ids)
        q, named = [int(ids[m // 2]), int(others[11]), int(ids[0]), int(others[4000]), int(ids[-1])], [0, 2, 4]
    elif name == "underflow_k16":
        n, k = 20000, 16
        xyz = _cloud(rng, n) + f32(1.0)
        ids = _coincident_ids(17, n)
        xyz[ids] = 0
        xyz[ids, 0] = (np.arange(17) * 1e-20).astype(f32)            # k + 1 points 1e-20 apart: their fp32 squares underflow
        q, named = [int(ids[0]), int(ids[8]), 123], [0, 1]
    elif name == "offset_1000":
        n, k = 5000, 96
        xyz = (rng.random((n, 3)) * 3).astype(f32) + f32(1000.0)
        q = [0, n - 1, 17, 2500, 2501]
    else:
        raise KeyError(name)
    q = np.asarray(q, dtype=np.int64)
    return dict(xyz=xyz, queries=q, k=k, named=list(range(len(q))) if named is None else named)


def knn_reference(case):
    return o_train.knn_points_bruteforce(case["xyz"], case["queries"], case["k"])


# ------------------------------------------------------------------------------------------ InfoNCE
NCE_T = 0.07
NCE_CASES = tuple([f"d{d}" for d in (1, 63, 64, 65, 128, 255, 256)] + [f"neg{m}" for m in (0, 1, 62, 63)] +
                  [f"anchors{a}" for a in (1, 3, 4, 5)] + ["repeats", "all_equal_map", "one_voxel_row", "untouched_rows", "zero_row"])
NCE_REFUSED = ((257, 5, "d = 257"), (64, 64, "64 negatives"))           # (d, negatives, what)


def nce_case(name):
    """dict(e f32 [nv, d], s2v i64 [S], p2b i64 [A (2 + Nn)], A, Nn)"""
    g = torch.Generator().manual_seed(hash_name(name))
    nv, S, A, Nn, d = 40, 50, 5, 7, 128
    if name.startswith("d"):
        d = int(name[1:])
    elif name.startswith("neg"):
        Nn, A, d = int(name[3:]), 3, 65
    elif name.startswith("anchors"):
        A, Nn = int(name[7:]), 5
    elif name == "all_equal_map":
        A, Nn, d = 4, 63, 64
    elif name == "one_voxel_row":
        nv, S, A, Nn = 1, 64, 4, 15
    e = torch.randn(nv, d, generator=g) * (torch.rand(nv, 1, generator=g) * 4 + 0.25)
    if d == 1:
        e = e + torch.sign(e) * 0.01                                 # (keeps |e| inside the magnitudes the header leaves unambiguous)
    s2v = torch.randint(0, nv, (S,), generator=g)
    p2b = torch.randint(0, S, (A * (2 + Nn),), generator=g)
    if name == "repeats":
        for a in range(A):                                           # anchor = positive = the first two negatives
            p2b[A + a] = p2b[a]
            p2b[2 * A + a * Nn] = p2b[2 * A + a * Nn + 1] = p2b[a]
    elif name == "all_equal_map":
        p2b[:] = 9
    elif name == "one_voxel_row":
        s2v[:] = 0
        p2b = torch.randint(0, S, (A * (2 + Nn),), generator=g)
    elif name == "untouched_rows":
        s2v = s2v - s2v % 2                                          # no sample points at an odd voxel row
    elif name == "zero_row":
        e[3] = 0
        s2v[:4] = 3
        p2b[0], p2b[A + 1], p2b[2 * A + 2] = 0, 1, 2                 # the zero row serves as an anchor, a positive and a negative
    return dict(e=e.contiguous(), s2v=s2v, p2b=p2b, A=A, Nn=Nn)


def nce_reference(case):
    """(loss, dE) in float64: oracle.train.info_nce with autograd.  Without negatives the oracle's reshape(A, 0, -1) cannot infer the
    width; the same expression with the one logit it leaves is written out here."""
    e = case["e"].double().requires_grad_(True)
    A, Nn = case["A"], case["Nn"]
    if Nn:
        loss = o_train.info_nce(e[case["s2v"]], case["p2b"], A, Nn, NCE_T)
    else:
        En = F.normalize(e[case["s2v"]], p=2, dim=1)
        l_pos = torch.einsum("bd,bd->b", En[case["p2b"][:A]], En[case["p2b"][A:2 * A]]).unsqueeze(-1)
        loss = F.cross_entropy(l_pos / NCE_T, torch.zeros(A, dtype=torch.long))
    loss.backward()
    return float(loss.detach()), e.grad.detach()


def nce_bounds(loss_ref, de_ref):
    """the bound of test_infonce_forward_backward: (loss, dE)"""
    return 1e-5 * max(1.0, abs(loss_ref)), 1e-6 + 1e-4 * float(de_ref.abs().max())


# ------------------------------------------------------------------------------------------ AdamW
ADAMW_N = (1, 255, 256, 257)
ADAMW_STEPS = (1, 2, 1000, 10 ** 6)
ADAMW_WD = (0.0, 1e-2)
ADAMW_LR, ADAMW_BETAS, ADAMW_EPS = 3e-4, (0.9, 0.999), 1e-8


def adamw_case(n, step):
    """p, m, v, g f32 [n]: element 0 has g = 0 and v = 0 (the denominator is eps alone), element n - 1 has p = 0"""
    rng = np.random.default_rng(1000 * n + step % 997)
    p, g = rng.standard_normal(n).astype(f32), (rng.standard_normal(n) * 0.1).astype(f32)
    m = (rng.standard_normal(n) * 0.05).astype(f32) if step > 1 else np.zeros(n, f32)
    v = (rng.random(n) * 0.01).astype(f32) if step > 1 else np.zeros(n, f32)
    m = np.copysign(m, g)                                            # no cancellation in b1 m + (1 - b1) g: see ADAMW_REL
    g[0] = v[0] = 0
    m[0] = f32(1e-6)                                                 # (a first moment that the eps-only denominator does not blow up)
    p[n - 1] = 0
    return p, m, v, g


def adamw_reference(p, m, v, g, step, wd, lr=ADAMW_LR, betas=ADAMW_BETAS, eps=ADAMW_EPS):
    """(p, m, v, update) in fp64 of the fp32 images of every input"""
    lr, b1, b2, eps, wd = (f64(f32(x)) for x in (lr, betas[0], betas[1], eps, wd))
    p, m, v, g = (x.astype(f64) for x in (p, m, v, g))
    m2 = b1 * m + (1 - b1) * g
    v2 = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    upd = (lr / bc1) * (m2 / (np.sqrt(v2) / np.sqrt(bc2) + eps))
    return p * (1 - lr * wd) - upd, m2, v2, upd


def adamw_kernel_model(p, m, v, g, step, wd, lr=ADAMW_LR, betas=ADAMW_BETAS, eps=ADAMW_EPS):
    """adamw_kernel's own fp32 operations in numpy (IEEE, no contraction): what a correct device gives, bit for bit"""
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, betas[0], betas[1], eps, wd))
    bc1, bc2s = f32(1.0 - f64(b1) ** step), f32(np.sqrt(1.0 - f64(b2) ** step))
    one = f32(1)
    pi = p * (one - lr * wd)
    mi = b1 * m + (one - b1) * g
    vi = b2 * v + (one - b2) * g * g
    return pi - (lr / bc1) * (mi / (np.sqrt(vi) / bc2s + eps)), mi, vi


# m = b1 m + (1 - b1) g is three rounded operations (1 - b1 is exact) and v = b2 v + (1 - b2) g g four, each within u = 2^-24 of its
# result; where the two terms of a sum have one sign -- v always, m by the cases' construction -- the sum is no smaller than either,
# so m is within 3u and v within 4u = 2^-22 of the fp64 value.  (With opposite signs the same three roundings are relative to the
# TERMS, not to their difference: a bound relative to m would then test the inputs' cancellation, not the kernel.)
ADAMW_REL = 2.0 ** -22


# ------------------------------------------------------------------------------------------ normalise + split
NORM_D = (4, 252, 256, 260, 1088)
NORM_N = (1, 3, 4, 5)
NORM_STRIDE_CASE = (16386, 16389, 4)                                  # (n, n_pad, d): more rows than the grid's 16384 waves
NORM_BOUND = 3e-7


def norm_case(n, d):
    """x f32 [n, d], a zero row at 1 when there is one"""
    g = torch.Generator().manual_seed(7919 * n + d)
    x = torch.randn(n, d, generator=g) * (torch.rand(n, 1, generator=g) * 5 + 0.01)
    if n > 1:
        x[1] = 0
    return x


def norm_reference(x):
    return F.normalize(x.double(), dim=1)


# ------------------------------------------------------------------------------------------ ambiguity
def magnitudes_ok(x, lo=1e-6, hi=1e6):
    """every element is zero or has lo <= |x| <= hi, and every row's sum of squares is 0 or well inside fp32's range"""
    a = np.abs(np.asarray(x, dtype=f64))
    return bool(np.isfinite(a).all() and ((a == 0) | ((a >= lo) & (a <= hi))).all())


def has_negative_nan(x):
    x = np.ascontiguousarray(x, dtype=f32)
    return bool((np.isnan(x) & (x.view(np.uint32) >> 31 != 0)).any())
