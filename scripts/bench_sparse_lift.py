"""Time sparse.lift on one MI355X beside the per-scene sequence it replaces, looped over the entries on the same inputs:
ops.views_visible_lists and the read-back of its counts, one ops.lift_dense_bilinear_accum launch per kept view, ops.lift_dense_finish,
ops.nn1_masked, ops.gather_rows.  One process, the forms alternated (batched on channels_last maps, batched on NCHW maps, the loop),
a host clock around each call that ends in a device synchronise.

Workload: LM_ENTRIES (4) entries of the synthetic config LM_CONFIG (S: 150 000 points, 25 views of 648 x 484 with ray-cast depths),
the LSeg form: maps [512, H/4, W/4] in [-1, 1], mode "bilinear".  The results of the forms are compared bit for bit at that size.
No threshold: the numbers go to profiles/lift_batched.log and DESIGN.md 5.11.

    python scripts/bench_sparse_lift.py [OUT_FILE]"""
import os
import statistics
import sys
import time
from multiprocessing import get_context

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENTRIES = int(os.environ.get("LM_ENTRIES", 4))
CONFIG = os.environ.get("LM_CONFIG", "S")
ROUNDS = int(os.environ.get("LM_ROUNDS", 10))


def scene_arrays(seed):
    from geopurify_amd import synthetic as sy
    cfg = sy.CONFIGS[CONFIG]
    s = sy.make_scene(cfg, seed=seed)
    w2c = np.stack([v.pose.T.astype(np.float64) for v in s.views])
    K = [sy.mapper_intrinsics(cfg, v.K) for v in s.views]
    intr = np.array([[k[0, 0], k[1, 1], k[0, 2], k[1, 2]] for k in K])
    return s.coords, w2c, intr, np.stack([v.depth for v in s.views])


def main():
    from geopurify_amd import synthetic as sy
    cfg = sy.CONFIGS[CONFIG]
    t0 = time.perf_counter()
    with get_context("spawn").Pool(min(ENTRIES, 4)) as pool:
        scenes = pool.map(scene_arrays, [101 + i for i in range(ENTRIES)])
    gen = time.perf_counter() - t0
    import torch
    from geopurify_amd import ops, sparse
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = "cuda"
    W, H = cfg.image_dim
    h, w = (H + 3) // 4, (W + 3) // 4
    D = cfg.feat_dim
    V = cfg.num_views
    g = torch.Generator(device=dev).manual_seed(1)
    maps = torch.rand((ENTRIES * V, D, h, w), generator=g, device=dev) * 2 - 1
    maps_cl = maps.contiguous(memory_format=torch.channels_last)
    pts = torch.from_numpy(np.vstack([np.column_stack([np.full(len(s[0]), b, np.float64), s[0]]) for b, s in enumerate(scenes)])).to(dev)
    ve = torch.arange(ENTRIES, device=dev).repeat_interleave(V)
    w2c = torch.from_numpy(np.concatenate([s[1] for s in scenes])).to(dev)
    intr = torch.from_numpy(np.concatenate([s[2] for s in scenes])).to(dev)
    depth = torch.from_numpy(np.concatenate([s[3] for s in scenes])).to(dev)
    kw = dict(mode="bilinear", cut_bound=cfg.cut_bound, vis_thres=cfg.vis_thres, min_visible=cfg.min_visible)
    per = []
    for b, s in enumerate(scenes):
        sl = slice(b * V, (b + 1) * V)
        per.append(dict(coords=torch.from_numpy(s[0]).to(dev), xyz=torch.from_numpy(s[0].astype(np.float32)).to(dev),
                        params=torch.cat([w2c[sl].reshape(V, 16), intr[sl]], 1).contiguous(), depth=depth[sl].contiguous(), maps=maps[sl]))

    def batched(m):
        return sparse.lift(pts, sparse.Views(m, ve, w2c, intr, depth, (H, W)), **kw)

    def loop():
        outs, seens = [], []
        for e in per:
            n = e["coords"].shape[0]
            ent = ops.views_visible_lists(e["coords"], e["params"], e["depth"], W, H, cfg.cut_bound, cfg.vis_thres, cfg.min_visible, 2 ** 62)
            off, keep = ops.readback(ent["view_off"]), ops.readback(ent["keep"])
            s = torch.zeros((n, D), dtype=torch.float32, device=dev)
            cnt = torch.zeros(n, dtype=torch.float32, device=dev)
            for i in range(V):
                if keep[i]:
                    ops.lift_dense_bilinear_accum(e["maps"][i], H, W, ent["pt"][off[i]:off[i + 1]], ent["x"][off[i]:off[i + 1]],
                                                  ent["y"][off[i]:off[i + 1]], s, cnt)
            sn = ops.lift_dense_finish(s, D, cnt)
            nn = ops.nn1_masked(e["xyz"], sn, 1 - sn)
            outs.append(ops.gather_rows(s, D, torch.where(nn >= 0, nn, torch.arange(n, device=dev))))
            seens.append(sn)
        return outs, seens

    forms = {"batched, channels_last maps": lambda: batched(maps_cl), "batched, NCHW maps": lambda: batched(maps), "per-scene loop": loop}
    res = {}
    for name, f in forms.items():                                # warm-up, and the results for the comparison
        for _ in range(2):
            res[name] = f()
        torch.cuda.synchronize()
    a, b_, (outs, seens) = res["batched, channels_last maps"], res["batched, NCHW maps"], res["per-scene loop"]
    same = torch.equal(a.features.view(torch.int32), torch.cat(outs).view(torch.int32)) and torch.equal(a.seen, torch.cat(seens).bool())
    same_layout = torch.equal(a.features.view(torch.int32), b_.features.view(torch.int32))
    seen, kept = int(a.seen.sum()), int(a.view_keep.sum())
    pairs = int(a.count.sum())
    del res, a, b_, outs, seens
    times = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for name, f in forms.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) * 1e3)
            del r
    n = pts.shape[0]
    lines = [f"sparse.lift against the per-scene sequence, one process, the forms alternated over {ROUNDS} rounds after 2 warm-up calls each",
             f"device: {torch.cuda.get_device_name(0)}",
             f"workload: {ENTRIES} entries of the synthetic config {CONFIG} ({n} points, {ENTRIES * V} views of {W} x {H}, maps [{D}, {h}, {w}] fp32, "
             f"bilinear, cut {cfg.cut_bound}, vis_thres {cfg.vis_thres}, min_visible {cfg.min_visible}); scenes generated in {gen:.1f} s",
             f"kept views {kept} of {ENTRIES * V}, seen points {seen} of {n}, (view, point) samples {pairs}",
             f"batched == loop, bit for bit (features and seen): {same}; channels_last == NCHW: {same_layout}",
             "wall clock around one call that ends in a device synchronise, ms: median  min  max  (max - min) / median"]
    for name, t in times.items():
        med = statistics.median(t)
        lines.append(f"  {name:30s} {med:8.2f} {min(t):8.2f} {max(t):8.2f}   {(max(t) - min(t)) / med:6.1%}   all: " + " ".join(f"{v:.2f}" for v in t))
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
