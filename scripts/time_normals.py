"""Time the geometry channels on one MI355X: sparse.mesh_normals beside the obvious torch form and the CPU loop it restates, and
sparse.estimate_normals / ops.knn_normals beside the gather + torch.linalg.eigh formulation.
One process, the forms alternated; HIP events around each call, 3 warm-up calls, the median of NM_RUNS (20) runs.

Mesh: a ScanNet-sized height field, NM_SIDE x (NM_SIDE + 1) vertices (387: 150 156 vertices, 298 764 faces), one entry, fp32 and fp64.
The torch form is three index_add_ calls of the face contributions: atomic float adds, so it is NOT order-exact (its bits change from
run to run and differ from the reference's); the CPU loop is tests/normals_cases.vertex_normal_loop, timed once on this box.
Estimated normals: the points of synthetic config S (150 000 points, no views) at its voxel size, k = 16.  The torch form takes the
same centroids and lists: positions[sets] in fp64, mean, covariance, torch.linalg.eigh, the first eigenvector.
No threshold: the numbers go to DESIGN.md 5.20.

    python scripts/time_normals.py [OUT_FILE]"""
import dataclasses
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIDE = int(os.environ.get("NM_SIDE", 387))
RUNS = int(os.environ.get("NM_RUNS", 20))
K = int(os.environ.get("NM_K", 16))


def torch_mesh_normals(torch, P, faces):
    """the obvious form: vectorised face contributions, index_add_ per corner (float atomics: not order-exact)"""
    v = P[:, 1:]
    p0, p1, p2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    vec = torch.linalg.cross(p1 - p0, p2 - p0)
    length = vec.square().sum(1, keepdim=True).sqrt() + 1.0e-8
    c = vec / length * (length * 0.5)
    nv = torch.zeros_like(v)
    for corner in range(3):
        nv.index_add_(0, faces[:, corner], c)
    return nv / (nv.square().sum(1, keepdim=True).sqrt() + 1.0e-8)


def torch_knn_normals(torch, positions, nbr):
    n = positions.shape[0]
    sets = torch.cat([torch.arange(n, device=nbr.device).unsqueeze(1), nbr], 1)
    Q = positions.double()[sets]
    D = Q - Q.mean(1, keepdim=True)
    w, V = torch.linalg.eigh(D.transpose(1, 2) @ D)
    return V[:, :, 0].float(), (w[:, 0] / w.sum(1)).float()


def main():
    import torch
    import normals_cases as nc
    from geopurify_amd import _lib, ops, sparse
    from geopurify_amd import synthetic as syn
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    xyz, faces_host = nc.grid_mesh(np.random.default_rng(7), SIDE, SIDE + 1, pitch=0.02, relief=0.005)
    n, nf = len(xyz), len(faces_host)
    pts64 = torch.from_numpy(np.column_stack([np.zeros(n), xyz])).to(dev)
    pts32 = pts64.float()
    faces = torch.from_numpy(faces_host).to(dev)

    cfg = dataclasses.replace(syn.CONFIGS["S"], num_views=0)
    scene = syn.make_scene(cfg, 7)
    cloud = torch.from_numpy(np.column_stack([np.zeros(len(scene.coords)), scene.coords])).to(dev)
    q = sparse.quantize(cloud, cloud[:, 1:].float(), mode="average", quantization_size=cfg.voxel_size)
    nbr = sparse.knn(q.coordinates, K)
    nv = q.coordinates.shape[0]
    centres = torch.tensor([[4.0, 3.0, 1.5]], dtype=torch.float64, device=dev)

    forms = {
        "ops.mesh_normals_batched fp32": lambda: ops.mesh_normals_batched(pts32, faces)[0],
        "ops.mesh_normals_batched fp64": lambda: ops.mesh_normals_batched(pts64, faces)[0],
        "sparse.mesh_normals fp32 (+ read-back)": lambda: sparse.mesh_normals(pts32, faces),
        "torch index_add_ fp32 (not order-exact)": lambda: torch_mesh_normals(torch, pts32, faces),
        "torch index_add_ fp64 (not order-exact)": lambda: torch_mesh_normals(torch, pts64, faces),
        f"ops.knn_normals k={K} (fp32 centroids, i64 lists)": lambda: ops.knn_normals(q.features, nbr)[0],
        f"torch gather + linalg.eigh k={K}": lambda: torch_knn_normals(torch, q.features, nbr)[0],
        f"sparse.estimate_normals k={K} (quantize + knn + kernel, 4 read-backs)":
            lambda: sparse.estimate_normals(cloud, quantization_size=cfg.voxel_size, k=K, toward=centres).normals,
        f"sparse.estimate_normals k={K}, quantized=q": lambda: sparse.estimate_normals(cloud, quantization_size=cfg.voxel_size, k=K, toward=centres,
                                                                                        quantized=q).normals,
    }
    for f in forms.values():
        for _ in range(3):
            f()
        torch.cuda.synchronize()
    # what the forms compute, checked once
    t0 = time.perf_counter()
    loop32 = nc.vertex_normal_loop(np.ascontiguousarray(pts32[:, 1:].cpu().numpy()), faces_host)
    loop_seconds = time.perf_counter() - t0
    ours32 = sparse.mesh_normals(pts32, faces).cpu().numpy()
    same_mesh = np.array_equal(nc.bits(ours32), nc.bits(loop32))
    torch32 = torch_mesh_normals(torch, pts32, faces).cpu().numpy()
    torch_same = np.array_equal(nc.bits(torch32), nc.bits(loop32))
    torch_again = np.array_equal(nc.bits(torch_mesh_normals(torch, pts32, faces).cpu().numpy()), nc.bits(torch32))
    kn, kv = ops.knn_normals(q.features, nbr)
    tn, tv = torch_knn_normals(torch, q.features, nbr)
    ref = nc.knn_normals_reference(q.features.cpu().numpy(), nbr.cpu().numpy())
    sure = torch.from_numpy(ref.gap >= nc.EIG_GAP).to(dev)
    d_eigh = float(torch.minimum((kn - tn).abs().amax(1), (kn + tn).abs().amax(1))[sure].max())
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
    lines = [f"geometry channels, one process, the forms alternated over {RUNS} runs after 3 warm-up calls each",
             f"device: {torch.cuda.get_device_name(0)}; library: {_lib.LIB_PATH}",
             f"mesh: {n} vertices, {nf} faces, one entry; cloud: {cloud.shape[0]} points, voxel {cfg.voxel_size}, {nv} voxels, k {K}",
             f"mesh_normals fp32 == the CPU loop bit for bit: {same_mesh}; torch index_add_ == the loop: {torch_same}, two torch runs the same "
             f"bits: {torch_again}; max |torch - loop| {np.abs(torch32.astype(np.float64) - loop32).max():.3g}",
             f"CPU loop (tests/normals_cases.vertex_normal_loop, fp32, once): {loop_seconds * 1e3:.0f} ms",
             f"knn_normals vs torch eigh on the {int(sure.sum())} rows with gap >= {nc.EIG_GAP}, up to sign: max |d| {d_eigh:.3g}; "
             f"max |variation - eigh's| {float((kv - tv).abs().max()):.3g}",
             "HIP events around one call, ms: median  min  max  (max - min) / median"]
    for name, t in times.items():
        med = statistics.median(t)
        extra = ""
        if name.startswith("ops.mesh_normals_batched"):
            e = 4 if name.endswith("fp32") else 8
            # read points (gathered per corner, once from HBM) and faces; write and read the contributions; write the pairs, the sort
            # reads and writes them once per radix pass (bits / 8 passes at least); the sum reads pairs and writes the normals
            passes = -(-max(n.bit_length(), 1) // 8)
            moved = n * 4 * e + nf * 24 + 2 * nf * 3 * e + 3 * nf * 8 * (2 + 2 * passes) + n * 3 * e
            extra = f"   >= {moved / 1e6:.1f} MB moved, {moved / med / 1e6:.1f} GB/s"
        if name.startswith("ops.knn_normals"):
            moved = nv * K * 8 + nv * 12 + nv * 16
            extra = f"   {moved / 1e6:.1f} MB compulsory (lists, positions once, outputs), {moved / med / 1e6:.1f} GB/s"
        lines.append(f"  {name:72s} {med:8.3f} {min(t):8.3f} {max(t):8.3f}   {(max(t) - min(t)) / med:6.1%}{extra}")
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
