"""Time the rendered depth over batched point clouds on one MI355X beside what a caller without it does: the per-view loop of
ops.render_depth (gp_render_depth_f64: one launch pair and one host-side matrix upload per view) on each entry's slice of the points.
Also sparse.lift(depth="render") beside sparse.lift(depth=<the rendered tensor>), so the cost of rendering inside the lift is known.
One process, the forms alternated; HIP events around each call, 3 warm-up calls, the median of RD_RUNS (20) runs.

Workload: RD_ENTRIES (4) entries of RD_POINTS (150 000) points each -- the walls, floor and ceiling of a room of 8 x 6 x 3 m and boxes of
furniture inside it --, RD_VIEWS (25) views per entry from near the middle of the room, turned about the vertical axis, RD_H x RD_W
(240 x 320) pixels, focal 0.8 W; the lift samples RD_D (32) channels, channels_last maps generated on the device.  The images of the
batched call, of the state form and of the loop are compared bit for bit at that size.  No threshold: the numbers go to DESIGN.md 5.15.
GP_LIB selects another build of the library (a same-box A/B run, as for the plain-load filter in front of the atomic that DESIGN.md
5.15 records).

    python scripts/time_render_depth_batched.py [OUT_FILE]"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENTRIES = int(os.environ.get("RD_ENTRIES", 4))
POINTS = int(os.environ.get("RD_POINTS", 150_000))
VIEWS = int(os.environ.get("RD_VIEWS", 25))
H, W = int(os.environ.get("RD_H", 240)), int(os.environ.get("RD_W", 320))
D = int(os.environ.get("RD_D", 32))
RUNS = int(os.environ.get("RD_RUNS", 20))
ROOM = np.array([8.0, 6.0, 3.0])


def room(rng, n):
    """n points on the six faces of the room and on the faces of a few boxes inside it (x, y horizontal, z up)"""
    def faces(lo, hi, m):
        p = rng.uniform(lo, hi, (m, 3))
        axis, side = rng.integers(0, 3, m), rng.integers(0, 2, m)
        p[np.arange(m), axis] = np.where(side == 0, lo[axis], hi[axis])
        return p
    parts = [faces(np.zeros(3), ROOM, n - 5 * (n // 10))]
    for _ in range(5):
        size = rng.uniform(0.4, 1.5, 3) * [1, 1, 0.8]
        lo = np.array([*rng.uniform(0.2, ROOM[:2] - size[:2] - 0.2), 0.0])
        parts.append(faces(lo, lo + size, n // 10))
    return np.vstack(parts)[rng.permutation(n)]


def cameras(rng, v):
    """world->camera [v,4,4]: the camera near the middle of the room at eye height, looking along a horizontal direction"""
    out = np.zeros((v, 4, 4))
    for i in range(v):
        a = rng.uniform(0, 2 * np.pi)
        fwd, right, down = np.array([np.cos(a), np.sin(a), 0.0]), np.array([np.sin(a), -np.cos(a), 0.0]), np.array([0.0, 0.0, -1.0])
        R = np.stack([right, down, fwd])
        eye = np.array([*(ROOM[:2] / 2 + rng.uniform(-1.0, 1.0, 2)), rng.uniform(1.2, 1.8)])
        out[i, :3, :3], out[i, :3, 3], out[i, 3, 3] = R, -R @ eye, 1.0
    return out


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
    cut = 0

    def batched():
        return ops.render_depth_batched(pts, ve, w2c, intr, (H, W), cut)[0]

    def checked():
        return sparse.render_depth(pts, ve, w2c, intr, (H, W), cut_bound=cut)

    state = ops.lift_stream_begin(pts, 1)

    def from_state():
        return ops.render_depth_stream(state, ve, w2c, intr, (H, W), cut)[0]

    def loop():
        out = []
        for b in range(ENTRIES):
            xyz = pts[b * POINTS:(b + 1) * POINTS, 1:].contiguous()          # the entry's slice of the points
            for v in range(b * VIEWS, (b + 1) * VIEWS):
                fx, fy, cx, cy = intr_host[v]
                out.append(ops.render_depth(xyz, w2c_host[v], fx, fy, cx, cy, W, H, cut))
        return torch.stack(out)

    maps = torch.rand((V, D, H, W), device=dev).contiguous(memory_format=torch.channels_last)
    depth = batched()

    def lift_render():
        return sparse.lift(pts, sparse.Views(maps, ve, w2c, intr, "render"))

    def lift_tensor():
        return sparse.lift(pts, sparse.Views(maps, ve, w2c, intr, depth))

    def lift_none():
        return sparse.lift(pts, sparse.Views(maps, ve, w2c, intr, None))

    forms = {"ops.render_depth_batched": batched, "sparse.render_depth (+ read-back)": checked, "ops.render_depth_stream (state)": from_state,
             "per-view loop of ops.render_depth": loop, "lift(depth='render')": lift_render, "lift(depth=tensor)": lift_tensor,
             "lift(depth=None)": lift_none}
    res = {}
    for name, f in forms.items():                                # warm-up, and the results for the comparison
        for _ in range(3):
            res[name] = f()
        torch.cuda.synchronize()
    ref = res["per-view loop of ops.render_depth"].view(torch.int64)
    same = {k: torch.equal(res[k].view(torch.int64), ref) for k in list(forms)[:3]}
    a, b, c = res["lift(depth='render')"], res["lift(depth=tensor)"], res["lift(depth=None)"]
    same["lift(depth='render') == lift(depth=tensor)"] = all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("seen", "count", "view_count")) \
        and torch.equal(a.features.view(torch.int32), b.features.view(torch.int32))
    hit = int((depth < 999999.0).sum())
    pairs_none, pairs_render = int(c.count.sum()), int(a.count.sum())
    del res, a, b, c, ref
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
    lines = [f"rendered depth over batched point clouds, one process, the forms alternated over {RUNS} runs after 3 warm-up calls each",
             f"device: {torch.cuda.get_device_name(0)}; library: {_lib.LIB_PATH}",
             f"workload: {ENTRIES} entries x {POINTS} points, {VIEWS} views each ({V} views of {H} x {W}), cut {cut}; the lift: D {D}, nearest, "
             f"channels_last maps",
             f"pixels hit {hit} of {V * H * W}; (point, view) pairs kept by depth=None {pairs_none}, by the rendered depth {pairs_render} "
             f"({1 - pairs_render / max(pairs_none, 1):.1%} hidden)",
             "the same bits as the per-view loop: " + ", ".join(f"{k}: {v}" for k, v in same.items()),
             "HIP events around one call, ms: median  min  max  (max - min) / median"]
    for name, t in times.items():
        med = statistics.median(t)
        lines.append(f"  {name:36s} {med:8.3f} {min(t):8.3f} {max(t):8.3f}   {(max(t) - min(t)) / med:6.1%}   all: " + " ".join(f"{v:.3f}" for v in t))
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
