"""Time sparse.LiftStream on one MI355X beside sparse.lift in one call, on the workload of scripts/bench_sparse_lift.py.  One process,
the forms alternated over LM_ROUNDS (10) rounds after two warm-up calls each, a host clock around each form that ends in a device
synchronise.

Workload: LM_ENTRIES (4) entries of the synthetic config LM_CONFIG (S: 150 000 points, 25 views of 648 x 484 with ray-cast depths), the
LSeg form: channels_last maps [512, H/4, W/4] in [-1, 1], mode "bilinear".  The resident source holds the views VIEW-MAJOR (view v of
entry e at v * entries + e), so that "k views of every entry" is one slice of it: a chunk's maps are made inside the timed loop by
slicing, which allocates nothing, and max_memory_allocated beyond the resident inputs shows what a form needs besides the maps.

Forms: sparse.lift in one call; the stream with 24 views of every entry per chunk (the reference's max_batch_size: 24 + 1 views here),
with 4, and with 1; every stream is built, fed and finished inside the clock.  Reported per form: median, min, max and spread of the
time, bit equality with the one-call result in all five fields, the peak of max_memory_allocated beyond the resident inputs.
No threshold: the numbers go to profiles/lift_stream.log and DESIGN.md 5.13.

    python scripts/bench_sparse_lift_stream.py [OUT_FILE]
    LM_ONE_CALL_ONLY=1 GP_LIB=<another build> python scripts/bench_sparse_lift_stream.py    # the one-call form alone, for same-box A/B
    LM_CHUNKS=24 LM_ROUNDS=3 rocprofv3 --kernel-trace --stats -- python3 scripts/bench_sparse_lift_stream.py   # where a form's time goes"""
import os
import statistics
import sys
import time
from multiprocessing import get_context

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
ENTRIES = int(os.environ.get("LM_ENTRIES", 4))
CONFIG = os.environ.get("LM_CONFIG", "S")
ROUNDS = int(os.environ.get("LM_ROUNDS", 10))
ONE_CALL_ONLY = os.environ.get("LM_ONE_CALL_ONLY", "0") == "1"
CHUNKS = tuple(int(k) for k in os.environ.get("LM_CHUNKS", "24,4,1").split(","))      # views of every entry per chunk, one form each
FIELDS = ("features", "seen", "count", "view_count", "view_keep")


def main():
    from bench_sparse_lift import scene_arrays
    from geopurify_amd import synthetic as sy
    cfg = sy.CONFIGS[CONFIG]
    t0 = time.perf_counter()
    with get_context("spawn").Pool(min(ENTRIES, 4)) as pool:
        scenes = pool.map(scene_arrays, [101 + i for i in range(ENTRIES)])
    gen = time.perf_counter() - t0
    import torch
    from geopurify_amd import _lib, sparse
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = "cuda"
    W, H = cfg.image_dim
    h, w = (H + 3) // 4, (W + 3) // 4
    D, V, E = cfg.feat_dim, cfg.num_views, ENTRIES
    g = torch.Generator(device=dev).manual_seed(1)
    maps = (torch.rand((V * E, h, w, D), generator=g, device=dev) * 2 - 1).permute(0, 3, 1, 2)     # channels_last [V*E, D, h, w]
    assert maps.is_contiguous(memory_format=torch.channels_last)
    pts = torch.from_numpy(np.vstack([np.column_stack([np.full(len(s[0]), b, np.float64), s[0]]) for b, s in enumerate(scenes)])).to(dev)

    def view_major(i):                                           # [E, V, ...] -> [V * E, ...]
        a = np.stack([s[i] for s in scenes])
        return torch.from_numpy(np.ascontiguousarray(a.swapaxes(0, 1).reshape((V * E,) + a.shape[2:]))).to(dev)

    ve = torch.arange(E, device=dev).repeat(V)
    w2c, intr, depth = view_major(1), view_major(2), view_major(3)
    kw = dict(mode="bilinear", cut_bound=cfg.cut_bound, vis_thres=cfg.vis_thres, min_visible=cfg.min_visible)

    def one_call():
        return sparse.lift(pts, sparse.Views(maps, ve, w2c, intr, depth, (H, W)), **kw)

    def streamed(k):
        def f():
            s = sparse.LiftStream(pts, feature_dim=D, **kw)
            for a in range(0, V, k):
                sl = slice(a * E, min(a + k, V) * E)             # views a .. a + k - 1 of every entry: slices, nothing is copied
                s.add(sparse.Views(maps[sl], ve[sl], w2c[sl], intr[sl], depth[sl], (H, W)))
            return s.finish()
        return f

    forms = {"sparse.lift, one call": one_call}
    if not ONE_CALL_ONLY:
        forms.update({f"stream, {k} views of every entry per chunk": streamed(k) for k in CHUNKS})
    res = {}
    for name, f in forms.items():                                # warm-up, and the results for the comparison
        for _ in range(2):
            res[name] = f()
        torch.cuda.synchronize()
    base = res["sparse.lift, one call"]
    same = {name: all(torch.equal(getattr(r, f).view(torch.int32) if f == "features" else getattr(r, f), getattr(base, f).view(torch.int32)
                                  if f == "features" else getattr(base, f)) for f in FIELDS) for name, r in res.items()}
    seen, kept, pairs = int(base.seen.sum()), int(base.view_keep.sum()), int(base.count.sum())
    del res, base
    times, peaks = {k: [] for k in forms}, {}
    for _ in range(ROUNDS):
        for name, f in forms.items():
            torch.cuda.synchronize()
            resident = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) * 1e3)
            peaks[name] = max(peaks.get(name, 0), torch.cuda.max_memory_allocated() - resident)
            del r
    n = pts.shape[0]
    lines = [f"sparse.LiftStream against sparse.lift in one call, one process, the forms alternated over {ROUNDS} rounds after 2 warm-up calls each",
             f"device: {torch.cuda.get_device_name(0)}; library: {os.path.relpath(_lib.LIB_PATH, ROOT)}",
             f"workload: {E} entries of the synthetic config {CONFIG} ({n} points, {E * V} views of {W} x {H}, channels_last maps [{D}, {h}, {w}] "
             f"fp32 = {maps.numel() * 4 / 1e9:.2f} GB resident, bilinear, cut {cfg.cut_bound}, vis_thres {cfg.vis_thres}, min_visible "
             f"{cfg.min_visible}); scenes generated in {gen:.1f} s",
             f"kept views {kept} of {E * V}, seen points {seen} of {n}, (view, point) samples {pairs}; resident inputs {resident / 1e9:.3f} GB",
             "a stream is built, fed (a chunk's maps: a slice of the resident source) and finished inside the clock",
             "wall clock around one form that ends in a device synchronise, ms: median  min  max  (max - min) / median | == one call, bit for bit "
             "(5 fields) | peak of max_memory_allocated beyond the resident inputs, MB"]
    for name, t in times.items():
        med = statistics.median(t)
        lines.append(f"  {name:42s} {med:8.2f} {min(t):8.2f} {max(t):8.2f}   {(max(t) - min(t)) / med:6.1%} | {str(same[name]):5s} | "
                     f"{peaks[name] / 1e6:9.1f} |  all: " + " ".join(f"{v:.2f}" for v in t))
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
