"""Time the batched contrastive sampler on one MI355X: sparse.sample_pairs beside the loop the library offered before it -- per batch
entry ops.coords_order_batched + ops.knn_batched on the entry's voxels and training.sample_contrastive_pairs_hybrid on its teacher rows --
with the same anchors, in the same process.  Median of RUNS runs after WARMUP, HIP events around the whole call (its host work and its
read-back included: that is what a training step waits for).

Shapes, each at Dt = 1088 (Sonata's width), K = 96, 63 negatives, min(4096, N_b // 3) anchors per entry:
    B = 1 x the S scene (150k points voxelised at 2 cm),  B = 4 x such scenes,  B = 32 x 4000-voxel slabs of one.
One more, untimed-as-a-whole run of sample_pairs has HIP events around each of its three kernels: the similarity GEMM's rate (three
f16 products per element counted as 6 flop), the bytes per second of the select sweep over the ragged buffer, the micro kernel.

One JSON line per shape."""
import dataclasses
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geopurify_amd import ops, sparse, training, synthetic as syn  # noqa: E402

K, DT, RUNS, WARMUP, NUM_ANCHORS, NUM_NEGATIVES = 96, 1088, 7, 2, 4096, 63


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


def kernel_times(fn):
    """one run of fn with HIP events around every call of the sampler's three kernels -> {name: (ms, calls)}, and the descriptors seen"""
    marks, seen = [], {"floats": 0, "flop": 0}
    originals = {n: getattr(ops, n) for n in ("sim_segments", "sampler_select_segments", "sampler_micro_segments")}

    def timed(name):
        def call(*a, **k):
            if name == "sim_segments":
                seen["floats"] += int(a[4].sum())
                seen["flop"] += int(a[4].sum()) * a[0].shape[1] * 6
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = originals[name](*a, **k)
            e1.record()
            marks.append((name, e0, e1))
            return r
        return call
    try:
        for n in originals:
            setattr(ops, n, timed(n))
        fn()
        torch.cuda.synchronize()
    finally:
        for n, f in originals.items():
            setattr(ops, n, f)
    out = {}
    for n in originals:
        out[n] = (sum(e0.elapsed_time(e1) for m, e0, e1 in marks if m == n), sum(1 for m, _, _ in marks if m == n))
    return out, seen


def shape(name, entries):
    """entries: list of int32 [n_b, 3] voxel sets -> one result dict"""
    C = np.vstack([np.c_[np.full(len(v), b, np.int32), v] for b, v in enumerate(entries)]).astype(np.int32)
    C = torch.from_numpy(C).cuda()
    C = C[torch.randperm(len(C), device="cuda")].contiguous()
    n = len(C)
    T = torch.randn(n, DT, device="cuda")
    rows = [(C[:, 0] == b).nonzero().flatten() for b in range(len(entries))]
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    local = [torch.randperm(len(r), device="cuda", generator=g)[:min(NUM_ANCHORS, len(r) // 3)] for r in rows]      # the reference's :1112 per entry
    anchors = torch.cat([r[a] for r, a in zip(rows, local)])
    parts = [(C[r].contiguous(), T[r].contiguous(), a.contiguous()) for r, a in zip(rows, local)]

    def batch():
        return sparse.sample_pairs(C, T, K=K, num_negatives=NUM_NEGATIVES, anchor_indices=anchors)

    def loop():
        out = []
        for Cb, Tb, ab in parts:
            perm, rank, keys, st = ops.coords_order_batched(Cb)
            nbr, _ = ops.knn_batched(keys, perm, K)
            lists = perm.long()[nbr.long()[rank.long()[ab]]]
            out.append(training.sample_contrastive_pairs_hybrid(Tb, lists, ab, NUM_NEGATIVES))
        return out

    got, alone = batch(), loop()
    same = torch.cat([r[p] for r, (p, _) in zip(rows, alone)]) == got.positive
    agree = float(same.float().mean())
    assert agree >= 0.99, agree                              # (near ties and the tie rule -- key row here, row index there -- may differ)
    res = {"bench": "sparse_contrast", "shape": name, "entries": len(entries), "rows": n, "anchors": int(anchors.shape[0]), "dt": DT, "k": K,
           "runs": RUNS, "positives_equal": round(agree, 5),
           "sample_pairs_ms": round(median_ms(batch), 3), "entry_loop_ms": round(median_ms(loop), 3)}
    res["loop_over_batched"] = round(res["entry_loop_ms"] / res["sample_pairs_ms"], 3)
    kt, seen = kernel_times(batch)
    sim_ms, sel_ms, mic_ms = (kt[k][0] for k in ("sim_segments", "sampler_select_segments", "sampler_micro_segments"))
    res.update({"chunks": kt["sim_segments"][1], "sim_floats": seen["floats"], "sim_segments_ms": round(sim_ms, 3),
                "sim_segments_tflops": round(seen["flop"] / (sim_ms * 1e-3) / 1e12, 2),
                "select_segments_ms": round(sel_ms, 3), "select_sweep_gb_per_s": round(seen["floats"] * 4 / (sel_ms * 1e-3) / 1e9, 1),
                "micro_segments_ms": round(mic_ms, 3)})
    print(json.dumps(res), flush=True)


def main():
    scenes = [voxels(5557 + i) for i in range(4)]
    shape("B1_scene", scenes[:1])
    shape("B4_scene", scenes)
    u = scenes[0][np.argsort(scenes[0][:, 0], kind="stable")]
    shape("B32_4k", [u[i:i + 4000] for i in range(0, 32 * 4000, 4000)])


if __name__ == "__main__":
    main()
