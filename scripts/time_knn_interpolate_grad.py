"""Time the backward of sparse.interpolate on one MI355X beside the only thing a user can do without it: torch's autograd over the
gather and weighted sum, in chunks of KG_TORCH_CHUNK (200 000) queries.  The torch form is the yardstick, never an earlier state of the
kernels; the one requirement is that the backward with a prebuilt transpose is faster than the yardstick's fastest backward run.
One process; HIP events around each call; KG_WARMUP (3) warm-up calls and the median of KG_RUNS (10) runs for the library's forms, one
warm-up and KG_TORCH_RUNS (3) runs for the torch form; the hub timing: one warm-up and KG_HUB_RUNS (3) runs.

Workload, DESIGN.md 5.21's: KG_ENTRIES (4) rooms (those of scripts/time_render_depth_batched.py) of KG_POINTS (150 000) points, queried
by KG_QUERIES (600 000) points per entry, k = 3; values of KG_ROWS (100 000) rows, D = KG_D (512), fp32 and fp16, through a point -> row
index; g = d_out fp32 [M,D].  Reported apart: the transpose build (weights + sort), the backward with a given transpose, forward +
backward.  The hub: the index sends every point of entry 0 to row 0, so one row has a quarter of all references -- the price of the
serial walk.  Peak memory is torch's max_memory_allocated over each form, the inputs included.  The numbers go to DESIGN.md 5.22.

    python scripts/time_knn_interpolate_grad.py [OUT_FILE]"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_knn_query import timed  # noqa: E402
from time_render_depth_batched import room  # noqa: E402

ENTRIES = int(os.environ.get("KG_ENTRIES", 4))
POINTS = int(os.environ.get("KG_POINTS", 150_000))
QUERIES = int(os.environ.get("KG_QUERIES", 600_000))
D = int(os.environ.get("KG_D", 512))
ROWS = int(os.environ.get("KG_ROWS", 100_000))
RUNS = int(os.environ.get("KG_RUNS", 10))
WARMUP = int(os.environ.get("KG_WARMUP", 3))
TORCH_RUNS = int(os.environ.get("KG_TORCH_RUNS", 3))
HUB_RUNS = int(os.environ.get("KG_HUB_RUNS", 3))
CHUNK = int(os.environ.get("KG_TORCH_CHUNK", 200_000))
K = 3
HBM_PEAK = 8.0e12                                               # bytes / s, MI355X


def torch_forward_backward(torch, values, idx, d2, index, g, eps=1e-8):
    """what a user writes today -> (d_values, ms of the backward calls alone): per chunk of queries the gather and weighted sum under
    autograd, the chunk's backward adding into values.grad through index_put_(accumulate=True)"""
    leaf = values.detach().requires_grad_()
    ms = 0.0
    for s in range(0, idx.shape[0], CHUNK):
        w = 1.0 / (d2[s:s + CHUNK].double() + eps)
        w = (w / w.sum(1, keepdim=True)).float()
        out = (leaf[index[idx[s:s + CHUNK]]] * w.unsqueeze(2)).sum(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out.backward(g[s:s + CHUNK])
        e1.record()
        e1.synchronize()
        ms += e0.elapsed_time(e1)
    return leaf.grad, ms


def peak_of(torch, f):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    r = f()
    torch.cuda.synchronize()
    del r
    return torch.cuda.max_memory_allocated()


def row(name, t, tail=""):
    return f"  {name:58s} {statistics.median(t):10.3f} {min(t):10.3f} {max(t):10.3f}{tail}"


def main():
    import torch
    from geopurify_amd import _lib, ops, sparse
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    samples = [room(rng, POINTS + QUERIES) for _ in range(ENTRIES)]
    pts_host = np.vstack([np.column_stack([np.full(POINTS, b, np.float64), s[:POINTS]]) for b, s in enumerate(samples)])
    qry_host = np.vstack([np.column_stack([np.full(QUERIES, b, np.float64), s[POINTS:]]) for b, s in enumerate(samples)])
    pts = torch.from_numpy(pts_host[rng.permutation(pts_host.shape[0])]).to(dev)
    qry = torch.from_numpy(qry_host[rng.permutation(qry_host.shape[0])]).to(dev)
    n, m = pts.shape[0], qry.shape[0]
    nb = sparse.knn_query(pts, qry, K)
    index = torch.randint(0, ROWS, (n,), device=dev)
    g = torch.randn((m, D), device=dev)
    base = torch.randn((ROWS, D), device=dev)
    I, D2 = nb.indices, nb.distances2
    lines = [f"the backward of sparse.interpolate, one process; HIP events around one call; library forms: median of {RUNS} runs after {WARMUP} "
             f"warm-up calls, torch form: {TORCH_RUNS} runs after 1, hub: {HUB_RUNS} runs after 1",
             f"device: {torch.cuda.get_device_name(0)}; library: {os.path.relpath(_lib.LIB_PATH, ROOT)}",
             f"workload: {ENTRIES} x {QUERIES} queries, k = {K}, D = {D}, {ROWS} rows of values through an index over {n} points; transpose "
             f"workspace {ops.knn_interpolate_transpose_workspace_bytes(m, K, ROWS) / 1e6:.1f} MB",
             "ms: median  min  max"]
    t_build = timed(torch, lambda: nb.transpose(index, ROWS).offsets, RUNS, WARMUP)
    t_weights = timed(torch, lambda: ops.knn_interpolate_weights(I, D2, index, ROWS), RUNS, WARMUP)
    tr = nb.transpose(index, ROWS)
    counts = (tr.offsets[1:] - tr.offsets[:-1]).cpu().numpy()
    lines += [row("Neighbors.transpose (weights, keys, sort, offsets, weights sorted)", t_build),
              row("  of which ops.knn_interpolate_weights", t_weights),
              f"  references per row of values: median {int(np.median(counts))}, max {int(counts.max())}, rows without any {int((counts == 0).sum())}"]
    ok = True
    for name, values in (("fp32", base), ("fp16", base.half())):
        es = values.element_size()
        t_bwd = timed(torch, lambda: ops.knn_interpolate_backward(g, tr.offsets, tr.slots, tr.weights, K, values.dtype), RUNS, WARMUP)

        def both(transpose):
            leaf = values.detach().requires_grad_()
            sparse.interpolate(leaf, nb, index=index, differentiable=True, transpose=transpose).backward(g)
            return leaf.grad

        t_given = timed(torch, lambda: both(tr), RUNS, WARMUP)
        t_built = timed(torch, lambda: both(None), RUNS, WARMUP)
        peak = peak_of(torch, lambda: both(tr))
        # what the call cannot avoid moving: g once, d_values once, a slot and a weight per flat slot, the offsets
        must = m * D * 4 + ROWS * D * es + m * K * 8 + (ROWS + 1) * 8
        med = statistics.median(t_bwd)
        lines += [f"values {name}:",
                  row("ops.knn_interpolate_backward, transpose given", t_bwd,
                      f"   compulsory {must / 1e9:.2f} GB, {must / med / 1e9:.2f} TB/s = {must / (med * 1e-3) / HBM_PEAK:.0%} of the "
                      f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak"),
                  row("interpolate forward + backward, transpose given", t_given, f"   peak memory {peak / 1e9:.2f} GB"),
                  row("interpolate forward + backward, transpose built inside", t_built)]
        runs = [torch_forward_backward(torch, values, I, D2, index, g) for _ in range(1 + TORCH_RUNS)][1:]
        t_torch_bwd = [ms for _, ms in runs]
        del runs
        t_torch = timed(torch, lambda: torch_forward_backward(torch, values, I, D2, index, g)[0], TORCH_RUNS, 0)
        peak_t = peak_of(torch, lambda: torch_forward_backward(torch, values, I, D2, index, g)[0])
        want = torch_forward_backward(torch, values, I, D2, index, g)[0]
        got, again = both(tr), both(tr)
        lines += [row(f"torch autograd backward alone, chunks of {CHUNK}", t_torch_bwd, f"   speed-up on its fastest run {min(t_torch_bwd) / med:.1f}x"),
                  row(f"torch autograd forward + backward, chunks of {CHUNK}", t_torch, f"   peak memory {peak_t / 1e9:.2f} GB"),
                  f"  max |ours - torch| {float((got.float() - want.float()).abs().max()):.3g} (max |torch| {float(want.float().abs().max()):.3g}); two "
                  f"of our calls the same bits: {bool(torch.equal(got.view(torch.int16), again.view(torch.int16)))}; two torch calls: "
                  f"{bool(torch.equal(want, torch_forward_backward(torch, values, I, D2, index, g)[0]))}"]
        ok = ok and med < min(t_torch_bwd)
        del want, got, again
    hub_index = torch.where(pts[:, 0] == 0, torch.zeros_like(index), index)
    th = nb.transpose(hub_index, ROWS)
    longest = int((th.offsets[1:] - th.offsets[:-1]).max())
    t_hub = timed(torch, lambda: ops.knn_interpolate_backward(g, th.offsets, th.slots, th.weights, K, torch.float32), HUB_RUNS, 1)
    lines += [row(f"hub: one row with {longest} references, fp32, transpose given", t_hub,
                  f"   {statistics.median(t_hub) * 1e6 / longest / ((D + 255) // 256):.1f} ns per reference and 256-column trip")]
    lines.append(f"backward with a prebuilt transpose faster than the torch form's fastest backward: {ok}")
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the backward is not faster than torch's autograd at this shape")


if __name__ == "__main__":
    main()
