"""Time sparse.render_rows and Rendered.features on one MI355X beside the yardstick they are built from: ops.render_depth_batched (the
entry tables, one fill, one z-buffer pass) on the same inputs in the same process -- render_rows' pass A does that pass's work plus the
footprint, pass B does it again, and depth="render" runs the z-buffer itself first.
One process, the forms alternated; HIP events around each call, 3 warm-up calls, the median of RD_RUNS (20) runs.

Workload: that of scripts/time_render_depth_batched.py -- RD_ENTRIES (4) rooms of RD_POINTS (150 000) points, RD_VIEWS (25) views per
entry, RD_H x RD_W (240 x 320) pixels.  The gather paints RR_D (512) channels from RR_ROWS (100 000) fp32 voxel rows through a point ->
row index, for the first RR_FEATURE_VIEWS (25) views, in fp32 and fp16; its achieved rate counts the index map, one source row per
owned pixel and every output row.  No threshold: the numbers go to DESIGN.md 5.19.

    python scripts/time_render_rows.py [OUT_FILE]"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_render_depth_batched import ENTRIES, H, POINTS, RUNS, VIEWS, W, cameras, room  # noqa: E402

D = int(os.environ.get("RR_D", 512))
ROWS = int(os.environ.get("RR_ROWS", 100_000))
FEATURE_VIEWS = int(os.environ.get("RR_FEATURE_VIEWS", 25))


def main():
    import torch
    from geopurify_amd import _lib, ops, sparse
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    clouds = [room(rng, POINTS) for _ in range(ENTRIES)]
    w2c_host = np.concatenate([cameras(rng, VIEWS) for _ in range(ENTRIES)])
    V = ENTRIES * VIEWS
    intr_host = np.tile(np.array([0.8 * W, 0.8 * W, W / 2, H / 2]), (V, 1))
    pts = torch.from_numpy(np.vstack([np.column_stack([np.full(POINTS, b, np.float64), c]) for b, c in enumerate(clouds)])).to(dev)
    ve = torch.arange(ENTRIES, device=dev).repeat_interleave(VIEWS)
    w2c, intr = torch.from_numpy(w2c_host).to(dev), torch.from_numpy(intr_host).to(dev)
    n = pts.shape[0]
    feats = torch.randn((ROWS, D), device=dev)
    index = torch.randint(0, ROWS, (n,), device=dev)
    depth = ops.render_depth_batched(pts, ve, w2c, intr, (H, W), 0)[0]
    rendered = sparse.render_rows(pts, ve, w2c, intr, (H, W), depth="render")
    fv = slice(0, min(FEATURE_VIEWS, V))

    forms = {"ops.render_depth_batched (yardstick)": lambda: ops.render_depth_batched(pts, ve, w2c, intr, (H, W), 0)[0]}
    for radius in (0, 1, 2):
        forms[f"ops.render_rows(depth='render', radius={radius})"] = lambda r=radius: ops.render_rows(pts, ve, w2c, intr, (H, W), 0, "render", radius=r).rows
        forms[f"ops.render_rows(depth=tensor, radius={radius})"] = lambda r=radius: ops.render_rows(pts, ve, w2c, intr, (H, W), 0, depth, radius=r).rows
        forms[f"ops.render_rows(depth=None, radius={radius})"] = lambda r=radius: ops.render_rows(pts, ve, w2c, intr, (H, W), 0, None, radius=r).rows
    forms["sparse.render_rows (+ read-back), radius 0"] = lambda: sparse.render_rows(pts, ve, w2c, intr, (H, W)).rows
    forms["Rendered.features fp32"] = lambda: rendered.features(feats, index=index, dtype=torch.float32, views=fv)
    forms["Rendered.features fp16"] = lambda: rendered.features(feats, index=index, dtype=torch.float16, views=fv)
    for f in forms.values():
        for _ in range(3):
            f()
        torch.cuda.synchronize()
    again = sparse.render_rows(pts, ve, w2c, intr, (H, W), depth=depth)
    same = all(torch.equal(getattr(again, k), getattr(rendered, k)) for k in ("rows", "view_count", "pixel_count")) \
        and torch.equal(again.depth.view(torch.int64), rendered.depth.view(torch.int64))
    near = rendered.depth > 0.2
    same_depth = torch.equal(rendered.depth[near].view(torch.int64), depth[near].view(torch.int64))
    got = rendered.features(feats, index=index, dtype=torch.float16, views=slice(0, 2))
    r2 = rendered.rows[:2].reshape(-1).long()
    want = torch.where((r2 >= 0).unsqueeze(1), feats[index[r2.clamp(min=0)]], torch.zeros((), device=dev)).half().view(got.shape)
    same_gather = torch.equal(got.view(torch.int16), want.view(torch.int16))
    del got, want, again
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
    cand = {r: int(ops.render_rows(pts, ve, w2c, intr, (H, W), 0, "render", radius=r).pixel_count.sum()) for r in (0, 1, 2)}
    npix = (fv.stop - fv.start) * H * W
    owned = int((rendered.rows[fv] >= 0).sum())
    lines = [f"lifted clouds rendered back into their views, one process, the forms alternated over {RUNS} runs after 3 warm-up calls each",
             f"device: {torch.cuda.get_device_name(0)}; library: {_lib.LIB_PATH}",
             f"workload: {ENTRIES} entries x {POINTS} points, {VIEWS} views each ({V} views of {H} x {W}), cut 0",
             f"candidates under 'render' {int(rendered.view_count.sum())}, under None "
             f"{int(ops.render_rows(pts, ve, w2c, intr, (H, W), 0, None).view_count.sum())}; pixels owned of {V * H * W} at radius 0 / 1 / 2: "
             f"{cand[0]} / {cand[1]} / {cand[2]}",
             f"two calls and the tensor form give the same bits: {same}; depth == render_depth where p_z > 0.2: {same_depth}; "
             f"features == torch.where(...).half() on two views: {same_gather}",
             f"the gather: {fv.stop - fv.start} views, {npix} pixels of which {owned} owned, D {D}, {ROWS} source rows through an index",
             "HIP events around one call, ms: median  min  max  (max - min) / median"]
    for name, t in times.items():
        med = statistics.median(t)
        extra = ""
        if name.startswith("Rendered.features"):
            out_size = 4 if name.endswith("fp32") else 2
            moved = npix * 4 + owned * (8 + D * 4) + npix * D * out_size
            extra = f"   {moved / 1e9:.3f} GB moved, {moved / med / 1e9:.2f} TB/s"
        lines.append(f"  {name:48s} {med:8.3f} {min(t):8.3f} {max(t):8.3f}   {(max(t) - min(t)) / med:6.1%}{extra}")
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
