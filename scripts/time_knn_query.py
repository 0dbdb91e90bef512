"""Time sparse.knn_query and sparse.interpolate on one MI355X beside the only thing a user can do without them: per entry, chunked
torch.cdist(...).topk(k, largest=False), then gather and weighted sum in torch.  The torch form is the yardstick, never an earlier state
of the kernels; the one requirement is that knn_query is faster than it at this shape.
One process; HIP events around each call; KQ_WARMUP (3) warm-up calls and the median of KQ_RUNS (10) runs for the library's forms, one
warm-up and KQ_TORCH_RUNS (2) runs for the torch forms (seconds each).

Workload: KQ_ENTRIES (4) rooms (those of scripts/time_render_depth_batched.py) of KQ_POINTS (150 000) points, queried by KQ_QUERIES
(600 000) points per entry sampled from the same rooms a second time, rows interleaved, at k = 1, 3 and 16; then interpolate at D =
KQ_D (512) from KQ_ROWS (100 000) fp32 rows through a point -> row index with the k = 3 lists.  The lists are checked on KQ_CHECK (500)
queries per entry against an fp64 brute force in torch under the rule.  The share of queries per rung of the ladder comes from the
status words of ops.knn_query.  No threshold besides the requirement: the numbers go to DESIGN.md 5.21.

    python scripts/time_knn_query.py [OUT_FILE]"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_render_depth_batched import room  # noqa: E402

ENTRIES = int(os.environ.get("KQ_ENTRIES", 4))
POINTS = int(os.environ.get("KQ_POINTS", 150_000))
QUERIES = int(os.environ.get("KQ_QUERIES", 600_000))
D = int(os.environ.get("KQ_D", 512))
ROWS = int(os.environ.get("KQ_ROWS", 100_000))
RUNS = int(os.environ.get("KQ_RUNS", 10))
WARMUP = int(os.environ.get("KQ_WARMUP", 3))
TORCH_RUNS = int(os.environ.get("KQ_TORCH_RUNS", 2))
CHECK = int(os.environ.get("KQ_CHECK", 500))
CHUNK = int(os.environ.get("KQ_TORCH_CHUNK", 4096))             # queries per cdist: CHUNK x POINTS fp32 distances at a time
KS = (1, 3, 16)
HBM_PEAK = 8.0e12                                               # bytes / s, MI355X


def torch_knn(torch, points, queries, k):
    """what a user writes today: per entry, chunks of queries against the entry's points"""
    idx = torch.full((queries.shape[0], k), -1, dtype=torch.int64, device=points.device)
    d2 = torch.full((queries.shape[0], k), float("inf"), dtype=torch.float32, device=points.device)
    for b in torch.unique(queries[:, 0]).tolist():
        rows, qrows = (points[:, 0] == b).nonzero()[:, 0], (queries[:, 0] == b).nonzero()[:, 0]
        P = points[rows, 1:].float()
        for s in range(0, qrows.shape[0], CHUNK):
            qs = qrows[s:s + CHUNK]
            d, i = torch.cdist(queries[qs, 1:].float(), P).topk(k, dim=1, largest=False)
            idx[qs], d2[qs] = rows[i], d * d
    return idx, d2


def torch_interpolate(torch, values, idx, d2, index, eps=1e-8, chunk=200_000):
    out = torch.empty((idx.shape[0], values.shape[1]), dtype=torch.float32, device=values.device)
    for s in range(0, idx.shape[0], chunk):
        w = 1.0 / (d2[s:s + chunk].double() + eps)
        w = (w / w.sum(1, keepdim=True)).float()
        out[s:s + chunk] = (values[index[idx[s:s + chunk]]] * w.unsqueeze(2)).sum(1)
    return out


def brute_force(torch, points, queries, qrows, k):
    """the rule in torch, fp64, for a few queries: separate multiply and add kernels round each operation once"""
    P32, Q32 = points[:, 1:].float().double(), queries[qrows, 1:].float().double()
    idx = torch.full((qrows.shape[0], k), -1, dtype=torch.int64, device=points.device)
    d2 = torch.full((qrows.shape[0], k), float("inf"), dtype=torch.float64, device=points.device)
    for b in torch.unique(queries[qrows, 0]).tolist():
        rows, sel = (points[:, 0] == b).nonzero()[:, 0], (queries[qrows, 0] == b).nonzero()[:, 0]
        dx, dy, dz = (Q32[sel, None, a] - P32[None, rows, a] for a in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        v, i = torch.sort(d, dim=1, stable=True)                  # rows ascend, so stable in d^2 is ascending in (d^2, row)
        idx[sel], d2[sel] = rows[i[:, :k]], v[:, :k]
    return idx, d2


def timed(torch, f, runs, warmup):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    t = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
        del r
    return t


def main():
    import torch
    from geopurify_amd import _lib, ops, sparse
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    # one sample of POINTS + QUERIES per room (room() shuffles its rows): the first POINTS are the working cloud, the others the
    # cloud that is scored -- the same surfaces sampled a second time
    samples = [room(rng, POINTS + QUERIES) for _ in range(ENTRIES)]
    pts_host = np.vstack([np.column_stack([np.full(POINTS, b, np.float64), s[:POINTS]]) for b, s in enumerate(samples)])
    qry_host = np.vstack([np.column_stack([np.full(QUERIES, b, np.float64), s[POINTS:]]) for b, s in enumerate(samples)])
    pts = torch.from_numpy(pts_host[rng.permutation(pts_host.shape[0])]).to(dev)
    qry = torch.from_numpy(qry_host[rng.permutation(qry_host.shape[0])]).to(dev)
    n, m = pts.shape[0], qry.shape[0]
    lines = [f"results carried to another cloud, one process; HIP events around one call; library forms: median of {RUNS} runs after {WARMUP} "
             f"warm-up calls, torch forms: {TORCH_RUNS} runs after 1",
             f"device: {torch.cuda.get_device_name(0)}; library: {_lib.LIB_PATH}",
             f"workload: {ENTRIES} entries x {POINTS} points queried by {ENTRIES} x {QUERIES} points, rows interleaved; workspace "
             f"{ops.knn_query_workspace_bytes(n, m) / 1e6:.1f} MB",
             "ms: median  min  max"]
    results = {}
    faster = True
    for k in KS:
        p64, q64 = pts.contiguous(), qry.contiguous()
        t_ops = timed(torch, lambda: ops.knn_query(p64, q64, k)[0], RUNS, WARMUP)
        t_sparse = timed(torch, lambda: sparse.knn_query(pts, qry, k).indices, RUNS, WARMUP)
        t_torch = timed(torch, lambda: torch_knn(torch, pts, qry, k)[0], TORCH_RUNS, 1)
        st = ops.knn_query(p64, q64, k)[2].tolist()
        nb = sparse.knn_query(pts, qry, k)
        check = torch.from_numpy(rng.permutation(m)[:CHECK * ENTRIES]).to(dev)
        bi, bd = brute_force(torch, pts, qry, check, k)
        exact = bool(torch.equal(nb.indices[check], bi) and torch.equal(nb.distances2[check].view(torch.int64), bd.view(torch.int64)))
        ti, _ = torch_knn(torch, pts, qry[check], k)
        agree = float((ti == bi).all(1).float().mean())
        results[k] = nb
        med, medt = statistics.median(t_ops), statistics.median(t_torch)
        faster = faster and statistics.median(t_sparse) < medt
        lines += [f"k = {k}:",
                  f"  {'ops.knn_query':44s} {med:10.3f} {min(t_ops):10.3f} {max(t_ops):10.3f}",
                  f"  {'sparse.knn_query (+ the status read-back)':44s} {statistics.median(t_sparse):10.3f} {min(t_sparse):10.3f} {max(t_sparse):10.3f}",
                  f"  {'torch cdist + topk, chunks of ' + str(CHUNK):44s} {medt:10.3f} {min(t_torch):10.3f} {max(t_torch):10.3f}   "
                  f"speed-up {medt / statistics.median(t_sparse):.1f}x",
                  f"  ladder, share of the {m} queries: stopped after shell 0 / 1 / 2 / 3: "
                  + " / ".join(f"{st[12 + r] / m:.2%}" for r in range(4)) + f"; entry scan {st[11] / m:.4%}; no points {st[9] / m:.2%}",
                  f"  {CHECK * ENTRIES} queries against the fp64 brute force: same bits {exact}; torch's fp32 cdist lists agree on {agree:.1%} of them"]
    values = torch.randn((ROWS, D), device=dev)
    index = torch.randint(0, ROWS, (n,), device=dev)
    nb = results[3]
    for name, v in (("fp32", values), ("fp16", values.half())):
        t = timed(torch, lambda: sparse.interpolate(v, nb, index=index), RUNS, WARMUP)
        med = statistics.median(t)
        # what the call cannot avoid moving to and from memory: the lists, an index value per slot, every source row once, the output;
        # and what the lanes load and store: every gathered row instead of every source row once (the repeats come from the caches)
        must = m * 3 * (16 + 8) + ROWS * D * v.element_size() + m * D * 4
        moved = m * 3 * (16 + 8) + m * 3 * D * v.element_size() + m * D * 4
        lines.append(f"  {'sparse.interpolate ' + name + f', k = 3, D = {D}':44s} {med:10.3f} {min(t):10.3f} {max(t):10.3f}   compulsory "
                     f"{must / 1e9:.2f} GB, {must / med / 1e9:.2f} TB/s = {must / (med * 1e-3) / HBM_PEAK:.0%} of the {HBM_PEAK / 1e12:.0f} TB/s HBM "
                     f"peak; loaded and stored by the lanes {moved / 1e9:.2f} GB, {moved / med / 1e9:.2f} TB/s")
    t = timed(torch, lambda: torch_interpolate(torch, values, nb.indices, nb.distances2, index), TORCH_RUNS, 1)
    got, want = sparse.interpolate(values, nb, index=index), torch_interpolate(torch, values, nb.indices, nb.distances2, index)
    lines.append(f"  {'torch gather + weighted sum, fp32':44s} {statistics.median(t):10.3f} {min(t):10.3f} {max(t):10.3f}   max |difference| "
                 f"{float((got - want).abs().max()):.3g}")
    lines.append(f"knn_query faster than the torch form at every k: {faster}")
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if not faster:
        raise SystemExit("knn_query is not faster than torch.cdist + topk at this shape")


if __name__ == "__main__":
    main()
