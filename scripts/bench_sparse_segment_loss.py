"""Time sparse.segment_loss (forward + backward) on one MI355X beside the same math under torch autograd -- F.normalize on both
sides, all logits at once, F.cross_entropy with ignore_index -- in the same process.  Median of RUNS runs after WARMUP, HIP events
around the whole call (its host work and its read-back included: that is what a training step waits for).

Shape: 8 entries x 20 000 rows, D = 512, C = 20 and 200, labels per voxel and per point (3 points per voxel on average through an
inverse map), reduction "item" (torch's mean), a twentieth of the labels ignored.  The torch column of the per-point form gathers the
logits by the inverse map.  No threshold: the numbers go to profiles/sparse_segment_loss_bench.log and DESIGN.md 5.10.

One JSON line per shape."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geopurify_amd import sparse  # noqa: E402

ENTRIES, ROWS, D, RUNS, WARMUP, SCALE, IGNORE = 8, 20000, 512, 20, 5, 14.3, 255


class Rows:
    def __init__(self, features, coordinates):
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


def shape(classes, per_point):
    g = torch.Generator(device="cuda")
    g.manual_seed(classes + per_point)
    n = ENTRIES * ROWS
    C = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    C[:, 0] = torch.arange(n, device="cuda") // ROWS
    C[:, 1] = torch.arange(n, device="cuda") % ROWS
    C = C[torch.randperm(n, device="cuda", generator=g)].contiguous()
    text = torch.randn(classes, D, device="cuda", generator=g)
    want = torch.randint(0, classes, (n,), device="cuda", generator=g)
    F = torch.nn.functional.normalize(text, dim=-1)[want] * 2.0 + torch.randn(n, D, device="cuda", generator=g) * 0.05
    inv = torch.randint(0, n, (3 * n,), device="cuda", generator=g) if per_point else None
    items = n if inv is None else inv.shape[0]
    labels = torch.where(torch.rand(items, device="cuda", generator=g) < 0.7, want if inv is None else want[inv],
                         torch.randint(0, classes, (items,), device="cuda", generator=g))
    labels[torch.rand(items, device="cuda", generator=g) < 0.05] = IGNORE
    leaf = F.clone().requires_grad_()

    def hip():
        leaf.grad = None
        loss = sparse.segment_loss(Rows(leaf, C), text, SCALE, labels=labels, ignore_labels=(IGNORE,), inverse_mapping=inv)
        loss.backward()
        return loss

    def torch_autograd():
        leaf.grad = None
        z = SCALE * torch.nn.functional.normalize(leaf, dim=-1) @ torch.nn.functional.normalize(text, dim=-1).t()
        loss = torch.nn.functional.cross_entropy(z if inv is None else z[inv], labels, ignore_index=IGNORE)
        loss.backward()
        return loss

    a = hip()
    ga = leaf.grad.clone()
    b = torch_autograd()
    gb = leaf.grad.clone()
    res = {"bench": "sparse_segment_loss", "entries": ENTRIES, "rows": n, "d": D, "classes": classes, "labels": "point" if per_point else "voxel",
           "items": items, "runs": RUNS, "loss_hip": round(float(a.detach()), 6), "loss_torch": round(float(b.detach()), 6),
           "grad_max_difference_over_max": float((ga - gb).abs().max() / gb.abs().max()),
           "segment_loss_ms": round(median_ms(hip), 3), "torch_autograd_ms": round(median_ms(torch_autograd), 3)}
    res["torch_over_hip"] = round(res["torch_autograd_ms"] / res["segment_loss_ms"], 3)
    print(json.dumps(res), flush=True)


def main():
    for classes in (20, 200):
        for per_point in (False, True):
            shape(classes, per_point)


if __name__ == "__main__":
    main()
