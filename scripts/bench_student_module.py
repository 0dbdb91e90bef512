#!/usr/bin/env python3
"""AffinityPredictor on a SparseTensor at the product's shape: one synthetic S-shaped scene (Nv ~ 125k voxels), student
518 -> 512 x 9 -> 128.  Times (median of HIP-event intervals):
  * the batched voxel order + kernel map (ops.coords_order_batched + kernel_map_sorted) against what HotPath builds
    (ops.morton_order + grid_build + kernel_map_build);
  * the module's eval forward under torch.no_grad() (order, map, pairs, f16x3 convolutions, raw output layer, row gathers) against
    HotPath's student alone (StudentWeights.forward on a prepared map and pairs);
  * the trainer's working copy of the weights that every autograd call builds (StudentTrainer from the module's state_dict).
Usage: bench_student_module.py [reps] [all|module|student]  (module / student: time that forward only -- for a kernel trace of one)"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat"))
import MinkowskiEngine as ME  # noqa: E402

from geopurify_amd import ops, pipeline as pl, synthetic as syn  # noqa: E402
from geopurify_amd.affinity_module import AffinityPredictor  # noqa: E402
from geopurify_amd.training import StudentTrainer  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
which = sys.argv[2] if len(sys.argv) > 2 else "all"
cfg = syn.CONFIGS["S"]
scene = syn.make_scene(cfg, 5557)
rigid = pl.scene_rigid_transform(cfg.voxel_size, 5557)
batch = pl.build_scene_batch(pl.upload_scene(scene, "cuda"), rigid, "cuda")
coords = batch.scene_coords_3d.floor().to(torch.int32).contiguous()
Nv = coords.shape[0]
g = torch.Generator(device="cuda").manual_seed(1)
feats = torch.cat([torch.nn.functional.normalize(torch.randn(Nv, 512, device="cuda", generator=g), dim=1),
                   torch.rand(Nv, pl.GEO_DIM, device="cuda", generator=g)], 1).contiguous()
C = ME.utils.batched_coordinates([coords], device="cuda").contiguous()

sd = pl.random_student_state_dict(512 + pl.GEO_DIM, hidden=512, embed=128, num_blocks=4, seed=0)
student = AffinityPredictor(input_dim=512 + pl.GEO_DIM, embed_dim=128, hidden_dim=512)
student.load_state_dict(sd)
student = student.cuda().eval()
st = student.device_weights(torch.device("cuda"))


def timed(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def grid_map():
    perm, _ = ops.morton_order(coords)
    cs = coords[perm.long()].contiguous()
    return ops.kernel_map_build(ops.grid_build(cs), cs)


def sorted_map():
    _, _, keys, _ = ops.coords_order_batched(C)
    return ops.kernel_map_sorted(keys)


perm, rank = ops.morton_order(coords)
cs = coords[perm.long()].contiguous()
nbr_map = ops.kernel_map_build(ops.grid_build(cs), cs)
pairs = ops.conv_pairs_build(nbr_map, col_tiles=max(1, st.hidden // 256))
X = torch.zeros((Nv, st.cin_pad), dtype=torch.float32, device="cuda")
X[:, :feats.shape[1]] = feats[perm.long()]
xs = st.split_input(X)
x = ME.SparseTensor(features=feats, coordinates=C)


def module_eval():
    with torch.no_grad():
        return student(x)


if which == "module":
    print(f"Nv={Nv}  AffinityPredictor(SparseTensor) eval forward {timed(module_eval):.3f} ms")
    sys.exit(0)
if which == "student":
    print(f"Nv={Nv}  StudentWeights.forward {timed(lambda: st.forward(X, nbr_map, pairs, x_split=xs)):.3f} ms")
    sys.exit(0)
t_grid = timed(grid_map)
t_sorted = timed(sorted_map)
t_student = timed(lambda: st.forward(X, nbr_map, pairs, x_split=xs))
t_module = timed(module_eval)
t_copy = timed(lambda: StudentTrainer(student.state_dict(), torch.device("cuda")))
print(f"Nv={Nv}  reps={reps}")
print(f"order + kernel map: morton_order + grid_build + kernel_map_build {t_grid:.3f} ms | "
      f"coords_order_batched + kernel_map_sorted {t_sorted:.3f} ms")
print(f"student: HotPath's StudentWeights.forward (map, pairs, split input ready) {t_student:.3f} ms | "
      f"AffinityPredictor(SparseTensor) eval forward {t_module:.3f} ms")
print(f"trainer copy of the weights per autograd call (StudentTrainer(state_dict)): {t_copy:.3f} ms")
