"""Time sparse.lift_masks on one MI355X beside the per-scene sequence it replaces, looped over the entries on the same inputs:
ops.views_visible_lists and the read-back of its entry count, ops.lift_masks_views, ops.segment_tables, ops.fuse_views_top3,
ops.nn1_masked, ops.gather_rows.  One process, the two forms alternated; HIP events around each call (the batched call's two read-backs
and the loop's one per scene lie inside the interval), 3 warm-up calls, the median of LM_RUNS (20) runs.

Workload: LM_ENTRIES (4) entries of the synthetic config LM_CONFIG (S: 150 000 points, 25 views of 648 x 484 with ray-cast depths) with
synthetic.make_vlm_outputs (200 queries, masks at stride 4, 512-wide embeddings, 19 classes).  The rows of the two forms are compared
bit for bit at that size.  No threshold: the numbers go to DESIGN.md 5.12.

    python scripts/time_lift_masks_batched.py [OUT_FILE]"""
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
RUNS = int(os.environ.get("LM_RUNS", 20))


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
    V = cfg.num_views
    vlm = sy.make_vlm_outputs(cfg, ENTRIES * V, 101)
    gen = time.perf_counter() - t0
    import torch
    from geopurify_amd import ops, sparse
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    H, W = cfg.mask_shape
    pm, pl, me = (torch.from_numpy(vlm[k]).to(dev) for k in ("pred_masks", "pred_logits", "mask_embed"))
    text, scale = torch.from_numpy(vlm["text_embed"]).to(dev), float(vlm["logit_scale"])
    _, Q, h, w = pm.shape
    D, C = me.shape[2], text.shape[0]
    pts = torch.from_numpy(np.vstack([np.column_stack([np.full(len(s[0]), b, np.float64), s[0]]) for b, s in enumerate(scenes)])).to(dev)
    ve = torch.arange(ENTRIES, device=dev).repeat_interleave(V)
    w2c = torch.from_numpy(np.concatenate([s[1] for s in scenes])).to(dev)
    intr = torch.from_numpy(np.concatenate([s[2] for s in scenes])).to(dev)
    depth = torch.from_numpy(np.concatenate([s[3] for s in scenes])).to(dev)
    kw = dict(cut_bound=cfg.cut_bound, vis_thres=cfg.vis_thres, min_visible=cfg.min_visible)
    views = sparse.MaskViews(pm, pl, me, ve, w2c, intr, depth, (H, W))
    taps = sparse._tap_tables(h, w, H, W, dev)
    text_norm = torch.nn.functional.normalize(text, dim=-1).contiguous()
    per = []
    for b, s in enumerate(scenes):
        sl = slice(b * V, (b + 1) * V)
        per.append(dict(coords=torch.from_numpy(s[0]).to(dev), xyz=torch.from_numpy(s[0].astype(np.float32)).to(dev),
                        params=torch.cat([w2c[sl].reshape(V, 16), intr[sl]], 1).contiguous(), depth=depth[sl].contiguous(), pm=pm[sl],
                        pl=pl[sl], me=me[sl].reshape(V * Q, D)))

    def batched():
        return sparse.lift_masks(pts, views, text, scale, **kw)

    def loop():
        outs = []
        for e in per:
            n = e["coords"].shape[0]
            ent = ops.views_visible_lists(e["coords"], e["params"], e["depth"], W, H, cfg.cut_bound, cfg.vis_thres, cfg.min_visible, 2 ** 62)
            total = ops.readback(ent["view_off"][-1:])[0]
            scores = torch.softmax(e["pl"], dim=-1)[..., :-1].max(-1).values.contiguous()
            f_seg = torch.empty((V, Q, D), dtype=torch.float32, device=dev)
            l_seg = torch.empty((V, Q, C), dtype=torch.float32, device=dev)
            ops.segment_tables(e["me"], text_norm, scale, f_seg.view(V * Q, D), l_seg.view(V * Q, C))
            _, start, pvv, pvs = ops.lift_masks_views(e["pm"], scores, taps, (H, W), e["xyz"], ent, total, V)
            F = torch.empty((n, D), dtype=torch.float32, device=dev)
            sn = ops.fuse_views_top3(start, pvv, pvs, n, f_seg, l_seg, F)
            nn = ops.nn1_masked(e["xyz"], sn, 1 - sn)
            outs.append(ops.gather_rows(F, D, torch.where(nn >= 0, nn, torch.arange(n, device=dev))))
        return outs

    forms = {"batched (sparse.lift_masks)": batched, "per-scene loop": loop}
    res = {}
    for name, f in forms.items():                                # warm-up, and the results for the comparison
        for _ in range(3):
            res[name] = f()
        torch.cuda.synchronize()
    a, outs = res["batched (sparse.lift_masks)"], res["per-scene loop"]
    same = torch.equal(a.features.view(torch.int32), torch.cat(outs).view(torch.int32))
    seen, kept, slots = int(a.seen.sum()), int(a.view_keep.sum()), int(a.count.sum())
    del res, a, outs
    times = {k: [] for k in forms}
    for _ in range(RUNS):
        for name, f in forms.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
            del r
    n = pts.shape[0]
    lines = [f"sparse.lift_masks against the per-scene sequence, one process, the forms alternated over {RUNS} runs after 3 warm-up calls each",
             f"device: {torch.cuda.get_device_name(0)}",
             f"workload: {ENTRIES} entries of the synthetic config {CONFIG} ({n} points, {ENTRIES * V} views of {W} x {H}, masks [{Q}, {h}, {w}] fp32, "
             f"D {D}, C {C}, cut {cfg.cut_bound}, vis_thres {cfg.vis_thres}, min_visible {cfg.min_visible}); inputs generated in {gen:.1f} s",
             f"kept views {kept} of {ENTRIES * V}, seen points {seen} of {n}, (view, point) slots {slots}",
             f"batched == loop, bit for bit (features): {same}",
             "HIP events around one call, ms: median  min  max  (max - min) / median"]
    for name, t in times.items():
        med = statistics.median(t)
        lines.append(f"  {name:30s} {med:8.2f} {min(t):8.2f} {max(t):8.2f}   {(max(t) - min(t)) / med:6.1%}   all: " + " ".join(f"{v:.2f}" for v in t))
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
