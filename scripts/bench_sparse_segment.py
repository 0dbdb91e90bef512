"""Time the batched scene tail on one MI355X; median of 20 runs after 5 warm-up runs, HIP events.

sparse.segment on 8 entries of 20 000 voxels at D = 512, C = 20, about 5 % of the rows all zero in a few contiguous patches per entry
(unseen regions are patches, not salt and pepper, and patches are what sends queries past ring 1), per-voxel labels -- in both fills --
beside the way the library offered before for the same result: a loop over the entries of classify_argmax + nn1_masked + iou_hist on
masked copies.  The loop's labels and counts must equal segment's exactly.  Also: how many queries each rung of gp_nn1_batched's ladder
resolved (a host model of the acceptance rule on the fill's own answers: a query whose nearest reference lies at d^2 < 81 is final at
ring 1, below 625 at ring 3, else scanned).

One JSON line."""
import dataclasses
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geopurify_amd import ops, sparse, synthetic as syn  # noqa: E402

D, CLASSES, RUNS, WARMUP, ENTRIES, ENTRY_ROWS, PATCHES, ZERO_SHARE = 512, 20, 20, 5, 8, 20000, 4, 0.05


class Holder:
    def __init__(self, features=None, coordinates=None):
        self.F, self.C = features, coordinates


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def voxels(seed):
    cfg = dataclasses.replace(syn.CONFIGS["S"], num_views=0)
    pts = syn.make_scene(cfg, seed).coords
    return np.unique(np.floor(pts / cfg.voxel_size).astype(np.int32), axis=0)


def patches(v, rng):
    """zero flags of one entry: the ENTRY_ROWS * ZERO_SHARE / PATCHES voxels nearest to each of PATCHES random voxels"""
    zero = np.zeros(len(v), bool)
    per = int(len(v) * ZERO_SHARE / PATCHES)
    for c in rng.integers(0, len(v), PATCHES):
        d2 = ((v.astype(np.int64) - v[c]) ** 2).sum(1)
        zero[np.argpartition(d2, per)[:per]] = True
    return zero


def main():
    rng = np.random.default_rng(7)
    slabs = []
    for seed in (5557, 5558):
        u = voxels(seed)
        u = u[np.argsort(u[:, 0], kind="stable")]
        slabs += [u[i:i + ENTRY_ROWS] for i in range(0, len(u) - ENTRY_ROWS + 1, ENTRY_ROWS)]
    slabs = slabs[:ENTRIES]
    assert len(slabs) == ENTRIES
    Cn = np.vstack([np.c_[np.full(len(s), b, np.int32), s] for b, s in enumerate(slabs)]).astype(np.int32)
    zero_n = np.concatenate([patches(s, rng) for s in slabs])
    order = rng.permutation(len(Cn))
    Cn, zero_n = Cn[order], zero_n[order]
    n = len(Cn)
    C = torch.from_numpy(Cn).cuda()
    text = torch.randn(CLASSES, D, device="cuda")
    tn = torch.nn.functional.normalize(text, dim=-1)
    cls = torch.randint(0, CLASSES, (n,), device="cuda")
    X = 4.0 * tn[cls] + 0.05 * torch.randn(n, D, device="cuda")
    X[torch.from_numpy(zero_n).cuda()] = 0.0
    labels = torch.where(torch.rand(n, device="cuda") < 0.8, cls, torch.randint(0, CLASSES, (n,), device="cuda"))
    labels[torch.rand(n, device="cuda") < 0.05] = 255
    rows = [(C[:, 0] == b).nonzero().flatten() for b in range(ENTRIES)]
    y = Holder(X, C)

    def seg(fill):
        return sparse.segment(y, text, 1.0, labels=labels, fill=fill)

    def loop(yz):
        """the per-entry way: masked copies of every array, then the single-scene kernels"""
        pred_all = torch.empty(n, dtype=torch.int64, device="cuda")
        counts = torch.zeros((ENTRIES, 3, CLASSES), dtype=torch.int64, device="cuda")
        for b in range(ENTRIES):
            m = C[:, 0] == b
            f, xyz, lab = X[m], C[m][:, 1:].float(), labels[m]
            pred, zero = ops.classify_argmax(f, tn, 1.0)
            if yz:
                q = torch.zeros_like(xyz)
                q[:, 0], q[:, 1] = xyz[:, 1], xyz[:, 2]
                xyz = q
            nn = ops.nn1_masked(xyz.contiguous(), 1 - zero, zero)
            pred = torch.where(nn >= 0, pred[nn.clamp(min=0)], pred)
            ops.iou_hist(pred, lab, CLASSES, [255], counts[b])
            pred_all[m] = pred
        return pred_all, counts

    out = {"bench": "sparse_segment", "runs": RUNS, "entries": ENTRIES, "rows": n, "d": D, "classes": CLASSES, "zero_rows": int(zero_n.sum())}
    for fill, yz in (("xyz", False), ("yz", True)):
        s = seg(fill)
        pred, counts = loop(yz)
        assert torch.equal(s.pred, pred) and torch.equal(s.counts, counts), fill
        assert s.unfilled == 0 and int(s.zero.sum()) == int(zero_n.sum())
        out[f"segment_{fill}_ms"] = round(median_ms(lambda: seg(fill)), 3)
        out[f"loop_{fill}_ms"] = round(median_ms(lambda: loop(yz)), 3)
    # the rungs: d^2 of every query's answer (fill="xyz") against the acceptance bounds
    s = seg("xyz")
    q = s.zero.nonzero().flatten()
    d2 = ((C[q, 1:].long() - C[s.filled_from[q], 1:].long()) ** 2).sum(1)
    out.update({"queries": int(q.numel()), "ring1": int((d2 < 81).sum()), "ring3": int(((d2 >= 81) & (d2 < 625)).sum()),
                "scan": int((d2 >= 625).sum()), "max_d2": int(d2.max())})
    # the fill alone, both axis masks (sorted keys and flags prepared outside the timing)
    perm, rank, keys, st = ops.coords_order_batched(C)
    zs = s.zero.to(torch.uint8).index_select(0, perm.long())
    ref = 1 - zs
    out["nn1_batched_xyz_ms"] = round(median_ms(lambda: ops.nn1_batched(keys, perm, ref, zs, 7)), 3)
    out["nn1_batched_yz_ms"] = round(median_ms(lambda: ops.nn1_batched(keys, perm, ref, zs, 6)), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
