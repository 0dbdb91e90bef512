"""The cases of tests/train_cases.py reach the branches they are named for, and their references are unambiguous (CPU only).

The branch conditions of csrc/train.hip are restated in numpy by the case module's models; what is asserted here is what
test_gpu_train_edges.py relies on: which sampler instance (LG) a row length runs, where the vector loop hands over to the tail loop,
how many candidates lie under the bound of the thread minima (2048 and 2049 exactly, for the two sides of the cap), which kNN
queries the 4-query kernel hands back and which exceed the histogram's cap, and that no case depends on something the header
leaves open.
"""
import numpy as np
import pytest
import torch

import train_cases as tc


# ------------------------------------------------------------------------------------------ sampler
def test_the_sampler_cases_run_every_lg_instance_and_both_refusals_of_n():
    lgs = {name: tc.sampler_lg(tc.sampler_case(name)["sim"].shape[1]) for name in tc.SAMPLER_CASES if name.startswith("lg_n")}
    assert sorted(set(lgs.values())) == [0, 1, 2, 3, 4, 5, 6]
    assert [lgs[f"lg_n{n}"] for n in tc.SAMPLER_LG_N] == [0, 1, 2, 2, 3, 4, 5, 6] and lgs["lg_n3145728"] == 6
    # each n is the first or the last of its instance
    for n in (49152, 98304, 196608, 393216, 786432, 1572864, tc.SR_N_MAX):
        assert tc.sampler_lg(n) + 1 == tc.sampler_lg(n + 1) or n == tc.SR_N_MAX
    assert tc.SR_N_MAX == 3145728 and tc.sampler_lg(tc.SR_N_MAX) == 6
    assert tc.sampler_lg(150000) == 2                                 # the product's own point count
    for k, n, _ in tc.SAMPLER_REFUSED:                                 # the entry point's argument check, restated
        assert not (1 <= k < tc.SR_NT and k + 2 <= n <= tc.SR_N_MAX)


def test_the_handover_cases_straddle_the_last_waves_switch_to_the_tail_loop():
    """wave 15 enters the 4-slot vector loop when f0 + 3 * 1024 + 64 <= n >> 2 with f0 = 960: from n >> 2 = 4096 on"""
    slots = {n: tc.sampler_vector_slots(n, True) for n in tc.SAMPLER_HANDOVER_N}
    assert [n >> 2 for n in tc.SAMPLER_HANDOVER_N] == [4095, 4096, 4096, 4097]
    assert sorted({n & 3 for n in tc.SAMPLER_HANDOVER_N}) == [0, 1, 2, 3]
    assert slots[4 * 4095 + 1][14] == 4 and slots[4 * 4095 + 1][15] == 0          # wave 14 in the vector loop, wave 15 in the tail
    for n in tc.SAMPLER_HANDOVER_N[1:]:
        assert slots[n] == [4] * 16
    for name in ("odd_n150000", "odd_n49153"):                                     # the scalar path: no vector loop at all
        c = tc.sampler_case(name)
        assert c["ld"] % 4 != 0 and c["ld"] >= c["sim"].shape[1]
    for n in tc.SAMPLER_HANDOVER_N:
        assert tc.sampler_case(f"handover_n{n}")["ld"] % 4 == 0


@pytest.mark.parametrize("name", tc.SAMPLER_CASES)
def test_sampler_case_candidate_counts_and_reference(name):
    c = tc.sampler_case(name)
    sim, anchors, k = c["sim"], c["anchors"], c["k"]
    A, n = sim.shape
    assert 2 <= A <= 4 and 1 <= k < tc.SR_NT and k + 2 <= n <= tc.SR_N_MAX and c["ld"] >= n
    assert not tc.has_negative_nan(sim)                                # the header leaves a NaN with a set sign bit open
    pos, macro = tc.select_reference(sim, anchors, k)
    counts = [tc.sampler_model(sim[a], anchors[a], k, pos[a])[1] for a in range(A)]
    assert all(cnt >= k for cnt in counts)                             # the bound admits the k lowest
    expect = {"cap_2048": [2048] * 3, "cap_2049": [2049] * 3, "all_equal": [4998] * 3, "far_block": [8999, 9000]}
    if name in expect:
        assert counts == expect[name]
    elif name not in ("k1023_n1025",):
        assert max(counts) <= 64                                       # the common path: a few candidates beyond k
    radix = [cnt > tc.SR_CAP for cnt in counts]
    assert all(radix) == (name in ("cap_2049", "all_equal", "far_block")) and any(radix) == all(radix)
    # the reference: the positive is not the anchor, the macro rows hold k distinct selectable indices in (value, index) order
    keys = tc.sampler_key(sim)
    for a in range(A):
        assert pos[a] != anchors[a] and len(set(macro[a])) == k and anchors[a] not in macro[a] and pos[a] not in macro[a]
        mk = keys[a][macro[a]].astype(np.int64)
        assert ((np.diff(mk) > 0) | ((np.diff(mk) == 0) & (np.diff(macro[a]) > 0))).all()
        others = np.delete(keys[a], [anchors[a]])
        assert keys[a][pos[a]] == others.max()
    if name == "anchor_places":
        assert anchors[0] == 0 and anchors[1] == n - 1 and sim[2, anchors[2]] == sim[2].max() and pos[2] != np.argmax(sim[2])
        assert (sim[3] < sim[3, anchors[3]]).sum() < k
    if name == "signed_zeros":
        z = np.flatnonzero(sim[1] == 0)
        assert np.signbit(sim[1][z]).any() and not np.signbit(sim[1][z]).all() and np.array_equal(macro[1], z[:k])
    if name == "inf_nan":
        assert np.isnan(sim[0, pos[0]]) and pos[1] == 7 and pos[2] == 11 and pos[3] == 0
        assert list(macro[1][-4:]) == [8, 33, 44, 59] and list(macro[1][:3]) == [3, 20, 41]


# ------------------------------------------------------------------------------------------ kNN
@pytest.mark.parametrize("name", list(tc.KNN_CASES))
def test_knn_case_takes_the_path_it_is_named_for(name):
    c = tc.knn_case(name)
    xyz, q, k = c["xyz"], c["queries"], c["k"]
    n = len(xyz)
    assert 1 <= k <= 1023 and k + 1 <= n and q.min() >= 0 and q.max() < n
    models = [tc.knn_model(xyz, int(i), k) for i in q]
    want = tc.KNN_CASES[name]
    for j, m in enumerate(models):
        named = j in c["named"]
        assert m["handed_back"] == (named and want in ("handed_back", "flagged")), (j, m)
        assert m["flagged"] == (named and want == "flagged") and m["over_cap"] == m["flagged"], (j, m)
    ref = tc.knn_reference(c)
    assert ref.shape == (len(q), k) and all(len(set(r)) == k for r in ref)
    if name == "coincident_2":                                          # what is dropped is the lowest (d^2, id) entry, not the query's own row:
        lo, hi = sorted((int(q[0]), int(q[2])))                          # the later of two coincident points keeps ITSELF and loses the earlier
        assert q[0] == hi and ref[0][0] == hi and lo not in ref[0] and ref[2][0] == hi and lo not in ref[2]
    elif not name.startswith("coincident"):
        assert all(int(i) not in r for r, i in zip(ref, q))
    if name == "lattice_k96":                                           # integer distances: most entries tie and the row id decides
        d2 = ((xyz[ref[2]].astype(np.float64) - xyz[q[2]]) ** 2).sum(1)
        assert len(np.unique(d2)) < 12
    if name == "underflow_k16":
        d = xyz[ref[0]] - xyz[q[0]]
        assert ((d * d).sum(1)[:k] < np.float32(1e-30)).all()
    if name == "n257_k16_q4":
        assert q[2] == q[3]
    for nn, kk, _ in tc.KNN_REFUSED:                                    # the entry point's argument check, restated
        assert not (kk >= 1 and kk + 1 <= nn and kk + 1 <= tc.KP_CAP // 2)


def test_the_zero_distance_bin_separates_the_exact_coincident_case_from_the_flagged_one():
    """the cap of the histogram bin is what separates coincident_2048 (exact result) from coincident_2100 (flag)"""
    for name, over in (("coincident_2048", False), ("coincident_2100", True)):
        c = tc.knn_case(name)
        d = c["xyz"].astype(np.float64) - c["xyz"][c["queries"][0]].astype(np.float64)
        zero_bin = int((tc.kp_bin((d * d).sum(1)) == 0).sum())
        assert zero_bin == int(name.split("_")[1]) and (zero_bin > tc.KP_CAP) == over


# ------------------------------------------------------------------------------------------ InfoNCE, AdamW, normalise
@pytest.mark.parametrize("name", tc.NCE_CASES)
def test_infonce_case_is_inside_the_header_and_unambiguous(name):
    c = tc.nce_case(name)
    e, s2v, p2b, A, Nn = c["e"], c["s2v"], c["p2b"], c["A"], c["Nn"]
    nv, d = e.shape
    assert 1 <= d <= 256 and 0 <= Nn < 64 and A >= 1 and p2b.shape[0] == A * (2 + Nn)
    assert 0 <= int(s2v.min()) and int(s2v.max()) < nv and 0 <= int(p2b.min()) and int(p2b.max()) < s2v.shape[0]
    assert tc.magnitudes_ok(e.numpy())
    ss = (e.double() ** 2).sum(1)
    assert (((ss > 1e-12) & (ss < 1e12)) | (ss == 0)).all()            # no square or sum of squares near fp32's ends
    assert bool((ss == 0).any()) == (name == "zero_row")
    loss, de = tc.nce_reference(c)
    assert np.isfinite(loss) and torch.isfinite(de).all()
    if name == "all_equal_map":
        assert abs(loss - np.log(1 + Nn)) < 1e-12
    if name == "one_voxel_row":
        assert nv == 1 and s2v.shape[0] == 64 and abs(loss - np.log(1 + Nn)) < 1e-12
    if name == "neg0":
        assert loss == 0.0 and not de.any()
    if name == "untouched_rows":
        assert not de[1::2].any() and de[0::2].any()
    if name == "repeats":
        assert all(p2b[a] == p2b[A + a] == p2b[2 * A + a * Nn] for a in range(A))
    if name == "zero_row":
        used = set(s2v[p2b].tolist())
        assert 3 in used and float(de[3].abs().max()) > 0


def test_adamw_cases_and_the_kernels_own_operations_meet_the_bound():
    """the bound of the GPU test holds for the kernel's operations carried out in IEEE fp32 -- so a device result outside it is the
    device's doing -- and the cases hold the elements they promise"""
    worst = [0.0, 0.0, 0.0]
    for n in tc.ADAMW_N:
        for step in tc.ADAMW_STEPS:
            p, m, v, g = tc.adamw_case(n, step)
            assert g[0] == 0 and v[0] == 0 and p[n - 1] == 0 and m[0] != 0 and (np.sign(m) * np.sign(g) >= 0).all()
            assert all(np.isfinite(x).all() for x in (p, m, v, g)) and (v >= 0).all()
            for wd in tc.ADAMW_WD:
                pr, mr, vr, ur = tc.adamw_reference(p, m, v, g, step, wd)
                pk, mk, vk = tc.adamw_kernel_model(p, m, v, g, step, wd)
                worst[0] = max(worst[0], float(np.max(np.abs(pk - pr) / (tc.ADAMW_REL * (np.abs(pr) + np.abs(ur))))))
                worst[1] = max(worst[1], float(np.max(np.abs(mk - mr) / (tc.ADAMW_REL * np.abs(mr)))))
                worst[2] = max(worst[2], float(np.max(np.abs(vk - vr) / (tc.ADAMW_REL * np.abs(vr) + 1e-300))))
    assert max(worst) <= 1.0, worst
    b1, b2 = (np.float64(np.float32(b)) for b in tc.ADAMW_BETAS)
    assert np.float32(1 - b1 ** 10 ** 6) == 1 and np.float32(np.sqrt(1 - b2 ** 10 ** 6)) == 1     # both corrections round to 1


def test_normalise_cases_are_unambiguous():
    for n in tc.NORM_N:
        for d in tc.NORM_D:
            x = tc.norm_case(n, d)
            assert d % 4 == 0 and tc.magnitudes_ok(x.numpy()) and bool((x[1] == 0).all() if n > 1 else True)
            ss = (x.double() ** 2).sum(1)
            assert (((ss > 1e-12) & (ss < 1e12)) | (ss == 0)).all()
    n, n_pad, d = tc.NORM_STRIDE_CASE
    assert n_pad > 16384 and n > 16384 and d == 4                       # rows beyond the grid's 16384 waves, real ones and pad ones
