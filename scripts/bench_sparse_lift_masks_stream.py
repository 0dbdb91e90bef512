"""Time sparse.LiftMasksStream on one MI355X beside sparse.lift_masks in one call.  One process, the forms alternated over LM_ROUNDS (10)
rounds after two warm-up calls each, a host clock around each form that ends in a device synchronise.

Workload: LM_ENTRIES (1) entries of the synthetic config LM_CONFIG (S: 150 000 points, 25 views of 648 x 484 with ray-cast depths) with
X-Decoder-shaped outputs: LM_QUERIES (101) queries, masks of a quarter of the image (121 x 162) N(0, 4), class logits N(0, 2) over the
config's classes + 1, embeddings and text N(0, 1) of the config's width (512).  The resident source holds the views VIEW-MAJOR (view v of
entry e at v * entries + e), so that "k views of every entry" is one slice of it: a chunk's arrays are made inside the timed loop by
slicing, which allocates nothing.

Forms: sparse.lift_masks in one call; the stream with 8, 4 and 1 views of every entry per chunk; every stream is built, fed and finished
inside the clock.  Reported per form: median, min, max and spread of the time, bit equality with the one-call result in all six fields,
the peak of max_memory_allocated beyond the resident inputs, and the masks the form needs resident while it runs (all views for the one
call, one chunk for a stream: from the shapes) -- their sum is what the form costs, the ratio of the sums what the stream is for.
No threshold: the numbers go to profiles/lift_masks_stream.log and DESIGN.md.

    python scripts/bench_sparse_lift_masks_stream.py [OUT_FILE]"""
import os
import statistics
import sys
import time
from multiprocessing import get_context

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
ENTRIES = int(os.environ.get("LM_ENTRIES", 1))
CONFIG = os.environ.get("LM_CONFIG", "S")
ROUNDS = int(os.environ.get("LM_ROUNDS", 10))
QUERIES = int(os.environ.get("LM_QUERIES", 101))
CHUNKS = tuple(int(k) for k in os.environ.get("LM_CHUNKS", "8,4,1").split(","))       # views of every entry per chunk, one form each
FIELDS = ("features", "seen", "count", "view_count", "view_keep", "text_features")


def main():
    from bench_sparse_lift import scene_arrays
    from geopurify_amd import synthetic as sy
    cfg = sy.CONFIGS[CONFIG]
    t0 = time.perf_counter()
    with get_context("spawn").Pool(min(ENTRIES, 4)) as pool:
        scenes = pool.map(scene_arrays, [101 + i for i in range(ENTRIES)])
    gen = time.perf_counter() - t0
    import torch
    from geopurify_amd import _lib, ops, sparse
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = "cuda"
    W, H = cfg.image_dim
    h, w = (H + 3) // 4, (W + 3) // 4
    D, C, V, E, Q = cfg.feat_dim, cfg.num_classes + 1, cfg.num_views, ENTRIES, QUERIES
    g = torch.Generator(device=dev).manual_seed(1)
    pm = torch.randn((V * E, Q, h, w), generator=g, device=dev) * 4
    pl = torch.randn((V * E, Q, C + 1), generator=g, device=dev) * 2
    me = torch.randn((V * E, Q, D), generator=g, device=dev)
    text = torch.randn((C, D), generator=g, device=dev)
    scale = 14.25
    pts = torch.from_numpy(np.vstack([np.column_stack([np.full(len(s[0]), b, np.float64), s[0]]) for b, s in enumerate(scenes)])).to(dev)

    def view_major(i):                                           # [E, V, ...] -> [V * E, ...]
        a = np.stack([s[i] for s in scenes])
        return torch.from_numpy(np.ascontiguousarray(a.swapaxes(0, 1).reshape((V * E,) + a.shape[2:]))).to(dev)

    ve = torch.arange(E, device=dev).repeat(V)
    w2c, intr, depth = view_major(1), view_major(2), view_major(3)
    kw = dict(cut_bound=cfg.cut_bound, vis_thres=cfg.vis_thres, min_visible=cfg.min_visible)

    def views(sl):
        return sparse.MaskViews(pm[sl], pl[sl], me[sl], ve[sl], w2c[sl], intr[sl], depth[sl], (H, W))

    feeding = {}

    def one_call():
        return sparse.lift_masks(pts, views(slice(0, V * E)), text, scale, **kw)

    def streamed(k):
        def f():
            s = sparse.LiftMasksStream(pts, text, scale, **kw)
            for a in range(0, V, k):
                s.add(views(slice(a * E, min(a + k, V) * E)))   # views a .. a + k - 1 of every entry: slices, nothing is copied
            feeding["peak"] = torch.cuda.max_memory_allocated()  # (the allocator's own figure: no synchronisation)
            return s.finish()
        return f

    forms = {"sparse.lift_masks, one call": (one_call, V * E)}
    forms.update({f"stream, {k} views of every entry per chunk": (streamed(k), min(k, V) * E) for k in CHUNKS})
    res = {}
    for name, (f, _) in forms.items():                           # warm-up, and the results for the comparison
        for _ in range(2):
            res[name] = f()
        torch.cuda.synchronize()
    base = res["sparse.lift_masks, one call"]

    def bits(t):
        return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t

    same = {name: all(torch.equal(bits(getattr(r, f)), bits(getattr(base, f))) for f in FIELDS) for name, r in res.items()}
    seen, kept, pairs = int(base.seen.sum()), int(base.view_keep.sum()), int(base.count.sum())
    visible = int(base.view_count.sum())
    del res, base
    times, peaks, backs, fed = {k: [] for k in forms}, {}, {}, {}
    for _ in range(ROUNDS):
        for name, (f, _) in forms.items():
            torch.cuda.synchronize()
            resident = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            calls = ops.READBACK["calls"]
            feeding.clear()
            t = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) * 1e3)
            peaks[name] = max(peaks.get(name, 0), torch.cuda.max_memory_allocated() - resident)
            fed[name] = max(fed.get(name, 0), feeding.get("peak", torch.cuda.max_memory_allocated()) - resident)
            backs[name] = ops.READBACK["calls"] - calls
            del r
    n = pts.shape[0]
    per_view = Q * h * w * 4
    lines = [f"sparse.LiftMasksStream against sparse.lift_masks in one call, one process, the forms alternated over {ROUNDS} rounds after 2 warm-up calls "
             "each",
             f"device: {torch.cuda.get_device_name(0)}; library: {os.path.relpath(_lib.LIB_PATH, ROOT)}",
             f"workload: {E} entries of the synthetic config {CONFIG} ({n} points, {E * V} views of {W} x {H}; per view pred_masks [{Q}, {h}, {w}] fp32 = "
             f"{per_view / 1e6:.1f} MB, pred_logits [{Q}, {C + 1}], mask_embed [{Q}, {D}]; text [{C}, {D}]; cut {cfg.cut_bound}, vis_thres "
             f"{cfg.vis_thres}, min_visible {cfg.min_visible}); scenes generated in {gen:.1f} s",
             f"kept views {kept} of {E * V}, visible entries {visible}, seen points {seen} of {n}, (kept view, point) records {pairs}; what a stream "
             f"keeps per view: {Q * (-(-D // 4) * 4 + C) * 4 / 1e3:.0f} kB of tables + 8 B per record",
             "a stream is built, fed (a chunk's arrays: slices of the resident source) and finished inside the clock",
             "wall clock around one form that ends in a device synchronise, ms: median  min  max  (max - min) / median | == one call, bit for bit "
             "(6 fields) | read-backs | peak of max_memory_allocated beyond the resident inputs, MB | masks the form needs resident, MB | sum, MB | "
             "one call's sum / this sum | the same three while views are still being fed (before finish: what has to fit beside the VLM), MB | "
             "one call's sum / this sum",
             f"(the result rows [{n}, {D}] fp32 and their filled copy, {2 * n * D * 4 / 1e6:.0f} MB, are in every form's peak; a stream takes them in "
             "finish only)"]
    sums = {name: peaks[name] + nv * per_view for name, (_, nv) in forms.items()}
    first = sums["sparse.lift_masks, one call"]
    fsums = {name: fed[name] + nv * per_view for name, (_, nv) in forms.items()}
    for name, t in times.items():
        med = statistics.median(t)
        lines.append(f"  {name:42s} {med:8.2f} {min(t):8.2f} {max(t):8.2f}   {(max(t) - min(t)) / med:6.1%} | {str(same[name]):5s} | {backs[name]:3d} | "
                     f"{peaks[name] / 1e6:9.1f} | {forms[name][1] * per_view / 1e6:9.1f} | {sums[name] / 1e6:9.1f} | {first / sums[name]:5.2f} | "
                     f"{fed[name] / 1e6:9.1f} {forms[name][1] * per_view / 1e6:9.1f} {fsums[name] / 1e6:9.1f} | {first / fsums[name]:5.2f} |  all: "
                     + " ".join(f"{v:.2f}" for v in t))
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
