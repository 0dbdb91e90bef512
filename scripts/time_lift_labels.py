"""Time sparse.lift_labels on uint8 label maps, on one MI355X, beside the workaround it replaces: sparse.lift on channels_last fp16
one-hot maps [V, C, H, W] followed by an argmax.  One process, the forms alternated over LL_ROUNDS (10) rounds after 2 warm-up calls
each, a host clock around each call that ends in a device synchronise; per form the peak of torch's allocator on top of what was
allocated before the call, and the bytes of the form's own input maps.

Workload (DESIGN.md 5.11's): LL_ENTRIES (4) entries of the synthetic config LL_CONFIG (S: 150 000 points, 25 views of 648 x 484 with
ray-cast depths), LL_CLASSES (200) classes; the label maps are random classes in blocks of 16 x 16 pixels, no ignored pixel.
The two results are compared: the votes with round(features * count) of the unfilled one-hot lift, the labels with its argmax where the
maximum is unique.  No threshold: the numbers go to DESIGN.md 5.17.  Kernel times: run the script under
`rocprofv3 --kernel-trace --stats -- python scripts/time_lift_labels.py`, a run of its own (LL_ROUNDS=3 keeps it short).

    python scripts/time_lift_labels.py [OUT_FILE]"""
import os
import sys
import time
from multiprocessing import get_context

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ENTRIES = int(os.environ.get("LL_ENTRIES", 4))
CONFIG = os.environ.get("LL_CONFIG", "S")
ROUNDS = int(os.environ.get("LL_ROUNDS", 10))
CLASSES = int(os.environ.get("LL_CLASSES", 200))
BLOCK = 16


def main():
    os.environ["LH_CONFIG"] = CONFIG                         # scene_arrays reads it, in the pool's processes too
    import time_lift_half as lh
    from geopurify_amd import synthetic as sy
    cfg = sy.CONFIGS[CONFIG]
    t0 = time.perf_counter()
    with get_context("spawn").Pool(min(ENTRIES, 4)) as pool:
        scenes = pool.map(lh.scene_arrays, [101 + i for i in range(ENTRIES)])
    gen = time.perf_counter() - t0
    import torch
    from geopurify_amd import sparse
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    V, C = cfg.num_views, CLASSES
    W, H = cfg.image_dim
    pts = torch.from_numpy(np.vstack([np.column_stack([np.full(len(s[0]), b, np.float64), s[0]]) for b, s in enumerate(scenes)])).to(dev)
    ve = torch.arange(ENTRIES, device=dev).repeat_interleave(V)
    w2c = torch.from_numpy(np.concatenate([s[1] for s in scenes])).to(dev)
    intr = torch.from_numpy(np.concatenate([s[2] for s in scenes])).to(dev)
    depth = torch.from_numpy(np.concatenate([s[3] for s in scenes])).to(dev)
    n, nv = pts.shape[0], ENTRIES * V
    g = torch.Generator(device=dev).manual_seed(1)
    blocks = torch.randint(0, C, (nv, -(-H // BLOCK), -(-W // BLOCK)), generator=g, device=dev, dtype=torch.int64)
    labels = blocks.repeat_interleave(BLOCK, 1).repeat_interleave(BLOCK, 2)[:, :H, :W].to(torch.uint8).contiguous()
    one_hot = torch.zeros((nv, H, W, C), dtype=torch.float16, device=dev)        # channels_last storage of [V, C, H, W]
    for v in range(nv):
        one_hot[v].scatter_(2, labels[v].long().unsqueeze(2), 1.0)
    one_hot = one_hot.permute(0, 3, 1, 2)
    assert one_hot.is_contiguous(memory_format=torch.channels_last)
    kw = dict(cut_bound=cfg.cut_bound, vis_thres=cfg.vis_thres, min_visible=cfg.min_visible)
    label_views = sparse.LabelViews(labels, ve, w2c, intr, depth)
    hot_views = sparse.Views(one_hot, ve, w2c, intr, depth)

    def vote(fill=True):
        return sparse.lift_labels(pts, label_views, C, fill=fill, **kw)

    def workaround(fill=True):
        lifted = sparse.lift(pts, hot_views, mode="nearest", fill=fill, **kw)
        return lifted, lifted.features.argmax(1)

    lines = [f"sparse.lift_labels beside the one-hot workaround, one process, the forms alternated over {ROUNDS} rounds after 2 warm-up calls each",
             f"device: {torch.cuda.get_device_name(0)}; {ENTRIES} entries of the synthetic config {CONFIG}: {n} points, {nv} views of {W} x {H}, "
             f"{C} classes; inputs generated in {gen:.1f} s",
             f"input maps: uint8 labels {labels.numel() / 1e6:.1f} MB; fp16 one-hot maps {one_hot.numel() * 2 / 1e9:.2f} GB", ""]
    forms = {"lift_labels, uint8 maps": vote, "lift on fp16 one-hot maps (channels_last) + argmax": workaround}
    res = lh.measure(torch, forms, lines, ROUNDS)
    got, (lifted, arg) = res["lift_labels, uint8 maps"], res["lift on fp16 one-hot maps (channels_last) + argmax"]
    plain, (hot, _) = vote(fill=False), workaround(fill=False)
    want = torch.round(hot.features * hot.count.unsqueeze(1).float()).to(torch.int32)
    top = plain.votes.max(1).values
    unique = (plain.votes == top.unsqueeze(1)).sum(1) == 1
    decided = (got.voted > 0) & unique
    filled = got.voted == 0
    lines += ["", f"votes == round(one-hot features * count), unfilled: {torch.equal(plain.votes, want)}; count equal: {torch.equal(plain.count, hot.count)}",
              f"points: {n}, voted {int((got.voted > 0).sum())}, with a unique maximum {int(decided.sum())}, filled or unlabeled {int(filled.sum())}",
              f"labels == argmax of the workaround where the maximum is unique: {int((got.labels[decided] == arg[decided]).sum())} of {int(decided.sum())}",
              f"labels == argmax of the workaround on the filled points: {int((got.labels[filled] == arg[filled]).sum())} of {int(filled.sum())}"]
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
