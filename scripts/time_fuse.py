"""Time sparse.fuse on one MI355X beside the same result formed with torch on the device (per entry and file: the same keys, a top-k
of them, boolean indexing, .half()).  One process, the forms alternated over TF_ROUNDS (10) rounds after 2 warm-up calls each, a host
clock around each call that ends in a device synchronise; per form the peak of torch's allocator on top of what was allocated before.

Shape: TF_ENTRIES (4) entries of TF_POINTS (150 000) points, D = TF_DIM (512) fp32 features, 75 % of the points seen, the rows entry
after entry.  Configurations:
  training    n_split_points = 80 000, num_files = 5, form "merged"
  evaluation  n_split_points = None,   num_files = 1, form "merged"
Reported per form: the time, and the algorithmic bytes -- N * D * 4 read once plus R * D * 2 written -- over that time as a share of
8 TB/s.  ops.fuse_plan and ops.fuse_write are also timed by themselves (the write step is the one that moves the rows).  The results
are compared bit for bit with the torch formulation.  The file write (FusedChunks.save: device -> host copies and torch.save into a
temporary directory) is outside the timed region and stated separately, once.  No threshold: the numbers go to DESIGN.md 5.18.
Kernel times: `rocprofv3 --kernel-trace --stats -- python scripts/time_fuse.py`, a run of its own (TF_ROUNDS=3 keeps it short).

    python scripts/time_fuse.py [OUT_FILE]"""
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENTRIES = int(os.environ.get("TF_ENTRIES", 4))
POINTS = int(os.environ.get("TF_POINTS", 150_000))
DIM = int(os.environ.get("TF_DIM", 512))
ROUNDS = int(os.environ.get("TF_ROUNDS", 10))
SEED = 12345
PEAK = 8e12                                                 # HBM bytes / s
M32 = 0xFFFFFFFF


def fmix32(x):
    x &= M32
    x ^= x >> 16
    x = x * 0x85EBCA6B & M32
    x ^= x >> 13
    x = x * 0xC2B2AE35 & M32
    return x ^ x >> 16


def measure(torch, forms, lines, bytes_of):
    res = {}
    for name, f in forms.items():
        for _ in range(2):
            res[name] = f()
        torch.cuda.synchronize()
    times, peaks = {k: [] for k in forms}, {}
    for _ in range(ROUNDS):
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
    lines.append("wall clock around one call that ends in a device synchronise, ms: median  min  max  (max - min) / median | share of 8 TB/s "
                 "(algorithmic bytes / median) | peak MB on top of the inputs")
    for name, t in times.items():
        med = statistics.median(t)
        share = f"{bytes_of[name] / (med * 1e-3) / PEAK:6.1%}" if name in bytes_of else "     -"
        lines.append(f"  {name:34s} {med:8.3f} {min(t):8.3f} {max(t):8.3f}   {(max(t) - min(t)) / med:6.1%} | {share} | {peaks[name] / 1e6:9.1f}   all: "
                     + " ".join(f"{v:.3f}" for v in t))
    return res


def main():
    import torch
    from geopurify_amd import ops, sparse
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    n = ENTRIES * POINTS
    g = torch.Generator(device=dev).manual_seed(1)
    pts = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    pts[:, 0] = torch.arange(ENTRIES, device=dev).repeat_interleave(POINTS).double()
    feats = torch.randn((n, DIM), generator=g, device=dev)
    seen = torch.rand(n, generator=g, device=dev) < 0.75
    seen8 = seen.to(torch.uint8)
    lines = [f"sparse.fuse beside its torch formulation, one process, the forms alternated over {ROUNDS} rounds after 2 warm-up calls each",
             f"device: {torch.cuda.get_device_name(0)}; {ENTRIES} entries of {POINTS} points, D = {DIM} fp32 ({feats.numel() * 4 / 1e9:.2f} GB), "
             f"{int(seen.sum())} of {n} points seen"]

    def fmix32_t(x):                                        # int64 tensors holding 32-bit values (the products wrap, their low words hold)
        x = x ^ (x >> 16)
        x = (x * 0x85EBCA6B) & M32
        x = x ^ (x >> 13)
        x = (x * 0xC2B2AE35) & M32
        return x ^ (x >> 16)

    def with_torch(n_split, num_files):
        cs = fmix32((SEED & M32) ^ fmix32(SEED >> 32))
        batch = pts[:, 0]
        parts = []
        for k in range(num_files):
            for b in range(ENTRIES):
                rows = torch.nonzero(batch == b).reshape(-1)
                nb = rows.shape[0]
                m = seen[rows]
                if n_split is not None and nb > n_split:
                    h = fmix32_t(torch.arange(nb, device=dev) ^ fmix32(k ^ fmix32(b ^ cs)))
                    chunk = torch.zeros(nb, dtype=torch.bool, device=dev)
                    chunk[torch.topk(h, n_split, largest=False, sorted=False).indices] = True
                    m = m & chunk
                parts.append(feats[rows[m]].half())
        return torch.cat(parts)

    for label, n_split, num_files in (("training", 80_000, 5), ("evaluation", None, 1)):
        kw = dict(n_split_points=n_split, num_files=num_files, seed=SEED)
        chunks = sparse.fuse(pts, (feats, seen), **kw)
        R = chunks.feat.shape[0]
        moved = n * DIM * 4 + R * DIM * 2
        plan = ops.fuse_plan(pts, seen8, n_split, num_files, SEED)
        B = chunks.num_entries
        forms = {"sparse.fuse": lambda: sparse.fuse(pts, (feats, seen), **kw).feat,
                 "torch on the device": lambda: with_torch(n_split, num_files),
                 "ops.fuse_plan alone": lambda: ops.fuse_plan(pts, seen8, n_split, num_files, SEED).status,
                 "ops.fuse_write alone": lambda: ops.fuse_write(plan, feats, B, R)[0]}
        lines += ["", f"{label}: n_split_points = {n_split}, num_files = {num_files}: R = {R} rows of feat; algorithmic bytes {moved / 1e9:.3f} GB "
                      f"(N * D * 4 read + R * D * 2 written)"]
        res = measure(torch, forms, lines, {"sparse.fuse": moved, "torch on the device": moved, "ops.fuse_write alone": moved})
        same = torch.equal(res["sparse.fuse"].view(torch.int16), res["torch on the device"].view(torch.int16))
        lines.append(f"sparse.fuse == the torch formulation, bit for bit: {same}")
        del res, forms
        out = tempfile.mkdtemp(prefix="time_fuse_")
        try:
            torch.cuda.synchronize()
            t = time.perf_counter()
            paths = chunks.save(out, [f"scene{b:04d}_00" for b in range(ENTRIES)])
            wrote = time.perf_counter() - t
            size = sum(os.path.getsize(p) for p in paths)
        finally:
            shutil.rmtree(out, ignore_errors=True)
        lines.append(f"FusedChunks.save (outside the timed region; device -> host copies and torch.save, once): {len(paths)} files, {size / 1e9:.2f} GB "
                     f"in {wrote:.2f} s")
        del chunks, plan

    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
