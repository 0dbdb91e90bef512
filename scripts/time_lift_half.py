"""Time sparse.lift and sparse.lift_masks on fp16 / bf16 inputs read in place, on one MI355X, beside the same calls on fp32 inputs and
beside "upcast by the caller, then the fp32 call" (what a caller had to do before the lifts took half inputs).  One process, the forms
alternated over LH_ROUNDS (10) rounds after 2 warm-up calls each, a host clock around each call that ends in a device synchronise; per
form the peak of torch's allocator on top of what was allocated before the call.

Workloads: LH_ENTRIES (4) entries of the synthetic config LH_CONFIG (S: 150 000 points, 25 views of 648 x 484 with ray-cast depths).
  lift    the LSeg form of scripts/bench_sparse_lift.py: maps [512, H/4, W/4] in [-1, 1], "bilinear", channels_last and NCHW
  masks   the X-Decoder form of scripts/time_lift_masks_batched.py: synthetic.make_vlm_outputs (200 queries, masks at stride 4)
  nearest maps at the image's size [LH_NEAREST_D (512), H, W] of ONE entry in fp16 (8 GB at S), "nearest", channels_last
The half results are compared bit for bit with the fp32 call on the upcast inputs at that size.  No threshold: the numbers go to
DESIGN.md 5.16.  Kernel times: run the script under `rocprofv3 --kernel-trace --stats -- python scripts/time_lift_half.py`, a run of
its own (LH_ROUNDS=3 keeps it short).

    LH_PARTS=lift,masks,nearest python scripts/time_lift_half.py [OUT_FILE]"""
import os
import statistics
import sys
import time
from multiprocessing import get_context

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENTRIES = int(os.environ.get("LH_ENTRIES", 4))
CONFIG = os.environ.get("LH_CONFIG", "S")
ROUNDS = int(os.environ.get("LH_ROUNDS", 10))
PARTS = os.environ.get("LH_PARTS", "lift,masks").split(",")
NEAREST_D = int(os.environ.get("LH_NEAREST_D", 512))


def scene_arrays(seed):
    from geopurify_amd import synthetic as sy
    cfg = sy.CONFIGS[CONFIG]
    s = sy.make_scene(cfg, seed=seed)
    w2c = np.stack([v.pose.T.astype(np.float64) for v in s.views])
    K = [sy.mapper_intrinsics(cfg, v.K) for v in s.views]
    intr = np.array([[k[0, 0], k[1, 1], k[0, 2], k[1, 2]] for k in K])
    return s.coords, w2c, intr, np.stack([v.depth for v in s.views])


def measure(torch, forms, lines, rounds=None):
    """forms: {name: callable}; 2 warm-up calls each, then the forms alternated; -> the warm-up results"""
    rounds = ROUNDS if rounds is None else rounds
    res = {}
    for name, f in forms.items():
        for _ in range(2):
            res[name] = f()
        torch.cuda.synchronize()
    times, peaks = {k: [] for k in forms}, {}
    for _ in range(rounds):
        for name, f in forms.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) * 1e3)
            peaks[name] = torch.cuda.max_memory_allocated() - base
            del r
    lines.append("wall clock around one call that ends in a device synchronise, ms: median  min  max  (max - min) / median | peak MB on top of the inputs")
    for name, t in times.items():
        med = statistics.median(t)
        lines.append(f"  {name:44s} {med:8.2f} {min(t):8.2f} {max(t):8.2f}   {(max(t) - min(t)) / med:6.1%} | {peaks[name] / 1e6:9.1f}   all: "
                     + " ".join(f"{v:.2f}" for v in t))
    return res


def main():
    from geopurify_amd import synthetic as sy
    cfg = sy.CONFIGS[CONFIG]
    t0 = time.perf_counter()
    with get_context("spawn").Pool(min(ENTRIES, 4)) as pool:
        scenes = pool.map(scene_arrays, [101 + i for i in range(ENTRIES)])
    V = cfg.num_views
    vlm = sy.make_vlm_outputs(cfg, ENTRIES * V, 101) if "masks" in PARTS else None
    gen = time.perf_counter() - t0
    import torch
    from geopurify_amd import sparse
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    W, H = cfg.image_dim
    pts = torch.from_numpy(np.vstack([np.column_stack([np.full(len(s[0]), b, np.float64), s[0]]) for b, s in enumerate(scenes)])).to(dev)
    ve = torch.arange(ENTRIES, device=dev).repeat_interleave(V)
    w2c = torch.from_numpy(np.concatenate([s[1] for s in scenes])).to(dev)
    intr = torch.from_numpy(np.concatenate([s[2] for s in scenes])).to(dev)
    depth = torch.from_numpy(np.concatenate([s[3] for s in scenes])).to(dev)
    n = pts.shape[0]
    half = {"fp16": torch.float16, "bf16": torch.bfloat16}
    lines = [f"the batched lifts on half inputs, one process, the forms alternated over {ROUNDS} rounds after 2 warm-up calls each",
             f"device: {torch.cuda.get_device_name(0)}; {ENTRIES} entries of the synthetic config {CONFIG}: {n} points, {ENTRIES * V} views of {W} x {H}; "
             f"inputs generated in {gen:.1f} s"]

    def bits(t):
        return t.view(torch.int32)

    if "lift" in PARTS:
        h, w, D = (H + 3) // 4, (W + 3) // 4, cfg.feat_dim
        kw = dict(mode="bilinear", cut_bound=cfg.cut_bound, vis_thres=cfg.vis_thres, min_visible=cfg.min_visible)
        g = torch.Generator(device=dev).manual_seed(1)
        maps = torch.rand((ENTRIES * V, D, h, w), generator=g, device=dev) * 2 - 1

        def lift(m):
            return sparse.lift(pts, sparse.Views(m, ve, w2c, intr, depth, (H, W)), **kw)

        forms, same = {}, {}
        for layout in ("channels_last", "NCHW"):
            fmt = torch.channels_last if layout == "channels_last" else torch.contiguous_format
            forms[f"fp32, {layout}"] = lambda m=maps.contiguous(memory_format=fmt): lift(m)
            for key, dt in half.items():
                m = maps.to(dt).contiguous(memory_format=fmt)
                forms[f"{key}, {layout}"] = lambda m=m: lift(m)
                forms[f"{key} upcast by the caller, {layout}"] = lambda m=m: lift(m.float())
        lines += ["", f"sparse.lift, bilinear, maps [{D}, {h}, {w}] ({maps.numel() * 4 / 1e9:.2f} GB in fp32)"]
        res = measure(torch, forms, lines)
        for layout in ("channels_last", "NCHW"):
            for key in half:
                a, b = res[f"{key}, {layout}"], res[f"{key} upcast by the caller, {layout}"]
                same[f"{key}, {layout}"] = torch.equal(bits(a.features), bits(b.features)) and torch.equal(a.count, b.count)
        lines.append(f"half == upcast, bit for bit (features and count): {same}")
        del res, forms, maps

    if "masks" in PARTS:
        Hm, Wm = cfg.mask_shape
        pm, pl, me = (torch.from_numpy(vlm[k]).to(dev) for k in ("pred_masks", "pred_logits", "mask_embed"))
        text, scale = torch.from_numpy(vlm["text_embed"]).to(dev), float(vlm["logit_scale"])
        kw = dict(cut_bound=cfg.cut_bound, vis_thres=cfg.vis_thres, min_visible=cfg.min_visible)

        def lift_masks(m):
            return sparse.lift_masks(pts, sparse.MaskViews(m, pl, me, ve, w2c, intr, depth, (Hm, Wm)), text, scale, **kw)

        forms = {"fp32": lambda: lift_masks(pm)}
        for key, dt in half.items():
            m = pm.to(dt)
            forms[key] = lambda m=m: lift_masks(m)
            forms[f"{key} upcast by the caller"] = lambda m=m: lift_masks(m.float())
        lines += ["", f"sparse.lift_masks, pred_masks {list(pm.shape)} ({pm.numel() * 4 / 1e9:.2f} GB in fp32)"]
        res = measure(torch, forms, lines)
        same = {key: torch.equal(bits(res[key].features), bits(res[f"{key} upcast by the caller"].features)) for key in half}
        lines.append(f"half == upcast, bit for bit (features): {same}")
        del res, forms, pm

    if "nearest" in PARTS:
        # the first "nearest" measurement at the image's size: one entry's fp16 maps, channels_last, made in slices of views
        D = NEAREST_D
        maps = torch.empty((V, D, H, W), dtype=torch.float16, device=dev).contiguous(memory_format=torch.channels_last)
        g = torch.Generator(device=dev).manual_seed(2)
        for v in range(V):
            maps[v] = (torch.rand((D, H, W), generator=g, device=dev) * 2 - 1).half()
        one = ve == 0
        p1 = pts[pts[:, 0] == 0].contiguous()
        kw = dict(mode="nearest", cut_bound=cfg.cut_bound, vis_thres=cfg.vis_thres, min_visible=cfg.min_visible)
        views = sparse.Views(maps, ve[one], w2c[one], intr[one], depth[one], (H, W))
        lines += ["", f"sparse.lift, nearest, ONE entry ({p1.shape[0]} points, {V} views), fp16 channels_last maps [{D}, {H}, {W}] "
                      f"({maps.numel() * 2 / 1e9:.2f} GB)"]
        measure(torch, {"fp16, channels_last, nearest": lambda: sparse.lift(p1, views, **kw)}, lines)

    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
