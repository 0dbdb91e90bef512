"""Time sparse.quantize(mode="average") on one S-shaped cloud (150k points, ~134k voxels of 2 cm, D = 518) beside the composition
StudentTrainer.scene_step uses today for the same job: torch.unique + ops.morton_order + stable torch.sort + bincount().cumsum() +
ops.scatter_mean_csr.  Same box, same process; median of 20 runs after warm-up, wall clock around a device synchronisation (both
routes read a count back to the host, so device events alone would miss part of the cost).

The two start from what each is given in practice: quantize from the points' coordinates [N,4], the composition from the
point -> voxel ids and the voxel coordinate table an earlier voxelisation made.  One JSON line."""
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geopurify_amd import ops, sparse, synthetic as syn  # noqa: E402

D, RUNS, WARMUP = 518, 20, 5


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    cfg = dataclasses.replace(syn.CONFIGS["S"], num_views=0)
    pts = syn.make_scene(cfg, 5557).coords
    cells = np.floor(pts / cfg.voxel_size).astype(np.int32)
    uniq, inv = np.unique(cells, axis=0, return_inverse=True)
    n, nv = len(cells), len(uniq)
    C = torch.from_numpy(np.c_[np.zeros(n, np.int32), cells]).cuda().contiguous()
    F = torch.randn(n, D, device="cuda")
    vox = torch.from_numpy(inv.reshape(-1).astype(np.int64)).cuda()                 # inds_reconstruct
    coords_3d = torch.from_numpy(uniq.astype(np.float32)).cuda()

    def new():
        return sparse.quantize(C, F, mode="average")

    def composition():
        uniq_vox, sample_to_voxel = torch.unique(vox, return_inverse=True)
        cs_ref = coords_3d[uniq_vox].floor().to(torch.int32).contiguous()
        perm, rank = ops.morton_order(cs_ref)
        cs = cs_ref[perm.long()].contiguous()
        s2v = rank.long()[sample_to_voxel].contiguous()
        order = torch.sort(s2v, stable=True).indices
        nvs = cs.shape[0]
        seg = torch.zeros(nvs + 1, dtype=torch.int64, device="cuda")
        seg[1:] = torch.bincount(s2v, minlength=nvs).cumsum(0)
        X = torch.empty((nvs, D), dtype=torch.float32, device="cuda")
        ops.scatter_mean_csr(F, D, order, seg, nvs, X)
        return cs, X, s2v

    q = new()
    cs, X, s2v = composition()
    assert q.coordinates.shape[0] == nv == cs.shape[0]
    assert torch.equal(q.coordinates[:, 1:], cs) and torch.equal(q.inverse_mapping, s2v) and torch.equal(q.features, X)
    print(json.dumps({"bench": "quantize", "n": n, "nv": nv, "d": D, "runs": RUNS,
                      "quantize_average_ms": round(median_ms(new), 3), "torch_composition_ms": round(median_ms(composition), 3),
                      "quantize_indices_only_ms": round(median_ms(lambda: ops.quantize_batched(C)), 3)}))


if __name__ == "__main__":
    main()
