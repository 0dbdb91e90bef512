"""Time the batched neighbour search and the batched purifying step on one MI355X; median of 20 runs after warm-up, HIP events.

1. ops.knn_batched (keys in, cell table built inside the call) on ONE S-sized entry -- 150k points voxelised at 2 cm, K = 96 --
   beside ops.knn_lattice on the same voxels (its grid is built outside the call; grid_build + knn_lattice is reported too).  The two
   must return the same lists.
2. sparse.affinity_pool on 8 entries of 20 000 voxels at D = 512 (K = 96, 19 applications) beside 8 serial single-entry calls.

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

K, D, RUNS, WARMUP, ENTRIES, ENTRY_ROWS = 96, 512, 20, 5, 8, 20000


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


def main():
    out = {"bench": "sparse_pool", "k": K, "runs": RUNS}
    # ---- 1: the neighbour search on one entry
    v = voxels(5557)
    v = v[np.random.default_rng(0).permutation(len(v))]
    nv = len(v)
    ct = torch.from_numpy(v).cuda().contiguous()
    perm, rank = ops.morton_order(ct)
    cs = ct[perm.long()].contiguous()
    grid = ops.grid_build(cs)
    Cb = torch.cat([torch.zeros((nv, 1), dtype=torch.int32, device="cuda"), ct], 1).contiguous()
    perm_b, rank_b, keys, st = ops.coords_order_batched(Cb)
    assert st.tolist() == [0, 0, 0]
    nbr_b, status = ops.knn_batched(keys, perm_b, K)
    assert status.tolist() == [0, -1, 0, 0]
    # the same lists, each brought from its own sorted order to input rows
    nbr_l = ops.knn_lattice(grid, cs, perm, K)
    assert torch.equal(perm_b.long()[nbr_b.long()].index_select(0, rank_b.long()), perm.long()[nbr_l.long()].index_select(0, rank.long()))
    out.update({"knn_nv": nv,
                "knn_lattice_ms": round(median_ms(lambda: ops.knn_lattice(grid, cs, perm, K)), 3),
                "grid_build_knn_lattice_ms": round(median_ms(lambda: ops.knn_lattice(ops.grid_build(cs, grid.origin, grid.extent), cs, perm, K)), 3),
                "knn_batched_ms": round(median_ms(lambda: ops.knn_batched(keys, perm_b, K)), 3)})
    out["knn_batched_over_lattice"] = round(out["knn_batched_ms"] / out["knn_lattice_ms"], 3)
    # ---- 2: the purifying step on 8 entries: slabs of 20 000 voxels along x of two scenes
    slabs = []
    for seed in (5557, 5558):
        u = voxels(seed)
        u = u[np.argsort(u[:, 0], kind="stable")]
        slabs += [u[i:i + ENTRY_ROWS] for i in range(0, len(u) - ENTRY_ROWS + 1, ENTRY_ROWS)]
    slabs = slabs[:ENTRIES]
    assert len(slabs) == ENTRIES
    C = torch.from_numpy(np.vstack([np.c_[np.full(len(s), b, np.int32), s] for b, s in enumerate(slabs)]).astype(np.int32)).cuda()
    C = C[torch.randperm(len(C), device="cuda")].contiguous()
    n = len(C)
    X = torch.randn(n, D, device="cuda")
    E = torch.nn.functional.normalize(torch.randn(n, 128, device="cuda"), dim=1)
    rows = [(C[:, 0] == b).nonzero().flatten() for b in range(ENTRIES)]
    parts = [(Holder(X[r].contiguous(), C[r].contiguous()), E[r].contiguous()) for r in rows]

    def batch():
        return sparse.affinity_pool(Holder(X, C), E, K=K).F

    def serial():
        return [sparse.affinity_pool(x, e, K=K).F for x, e in parts]

    whole, alone = batch(), serial()
    diff = max(float((whole[r] - a).abs().max()) for r, a in zip(rows, alone))
    assert diff <= 1e-4, diff
    out.update({"pool_entries": ENTRIES, "pool_rows": n, "pool_d": D, "pool_num_iters": 19, "pool_family": sparse.pool_family(D, K, 19),
                "affinity_pool_batch_ms": round(median_ms(batch), 3), "affinity_pool_8_serial_ms": round(median_ms(serial), 3),
                "batch_vs_serial_max_abs_diff": diff})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
