"""Time the differentiable purifying step on one MI355X; median of 20 runs after warm-up, HIP events.

Shape: 8 entries of 20 000 voxels, D = 512, d = 128, K = 96, 19 applications (the shape of scripts/bench_sparse_pool.py).
  * sparse.affinity_pool, the default (no gradients);
  * sparse.affinity_pool(differentiable=True), forward only;
  * forward + backward of a sum loss, gradients to the features and the embeddings;
  * the same mathematics with torch.sparse.mm under torch autograd on the same GPU, on lists found once outside the timing (the
    reference's formulation, what a user can write without this library's backward); sparse.knn is timed by itself beside it;
  * one transposed application and one weight gradient alone, with their algorithmic bytes and the share of the 8 TB/s HBM peak
    those bytes would take at the measured time (gathered rows mostly come from the caches, so this is no HBM measurement);
  * the in-degrees of the inverted index.
One JSON line."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_sparse_pool import ENTRIES, ENTRY_ROWS, Holder, K, D, median_ms, voxels  # noqa: E402
from geopurify_amd import ops, sparse  # noqa: E402

T, EMBED, SHARPEN, HBM_PEAK = 19, 128, 20.0, 8e12


def main():
    slabs = []
    for seed in (5557, 5558):
        u = voxels(seed)
        u = u[np.argsort(u[:, 0], kind="stable")]
        slabs += [u[i:i + ENTRY_ROWS] for i in range(0, len(u) - ENTRY_ROWS + 1, ENTRY_ROWS)]
    slabs = slabs[:ENTRIES]
    assert len(slabs) == ENTRIES
    C = torch.from_numpy(np.vstack([np.c_[np.full(len(s), b, np.int32), s] for b, s in enumerate(slabs)]).astype(np.int32)).cuda()
    C = C[torch.randperm(len(C), device="cuda")].contiguous()
    n = len(C)
    X = torch.randn(n, D, device="cuda")
    E = torch.randn(n, EMBED, device="cuda")
    R = torch.randn(n, D, device="cuda")
    out = {"bench": "sparse_pool_grad", "rows": n, "entries": ENTRIES, "d": D, "embed": EMBED, "k": K, "num_iters": T, "runs": 20,
           "stack_bytes": T * n * D * 4}

    def default():
        return sparse.affinity_pool(Holder(X, C), E, K=K, num_iters=T).F

    def forward():
        x, e = X.detach().requires_grad_(), E.detach().requires_grad_()
        return sparse.affinity_pool(Holder(x, C), e, K=K, num_iters=T, differentiable=True).F, x, e

    def forward_backward():
        y, x, e = forward()
        (y * R).sum().backward()
        return x.grad, e.grad

    out["default_forward_ms"] = round(median_ms(default), 3)
    out["default_family"] = sparse.pool_family(D, K, T)
    out["differentiable_forward_ms"] = round(median_ms(lambda: forward()[0]), 3)
    out["forward_backward_ms"] = round(median_ms(forward_backward), 3)
    gx, ge = forward_backward()

    # ---- the torch formulation: lists once, then normalize / softmax / sparse_coo_tensor / 19 x torch.sparse.mm under autograd
    out["knn_ms"] = round(median_ms(lambda: sparse.knn(C, K)), 3)
    nbr = sparse.knn(C, K)
    rows = torch.arange(n, device="cuda").repeat_interleave(K)
    index = torch.stack([rows, nbr.reshape(-1)])

    def torch_forward_backward():
        x, e = X.detach().requires_grad_(), E.detach().requires_grad_()
        u = torch.nn.functional.normalize(e, dim=1)
        sim = (u.unsqueeze(1) * u[nbr]).sum(-1)
        w = torch.softmax(SHARPEN * sim, dim=1)
        A = torch.sparse_coo_tensor(index, w.reshape(-1), (n, n))
        y = x
        for _ in range(T):
            y = torch.sparse.mm(A, y)
        (y * R).sum().backward()
        return x.grad, e.grad

    try:
        tx, te = torch_forward_backward()
        out["grad_x_vs_torch_rel"] = float((gx - tx).abs().max() / tx.abs().max())
        out["grad_e_vs_torch_rel"] = float((ge - te).abs().max() / te.abs().max())
        del tx, te
        out["torch_sparse_mm_forward_backward_ms"] = round(median_ms(torch_forward_backward), 3)
        out["hip_over_torch"] = round(out["forward_backward_ms"] / out["torch_sparse_mm_forward_backward_ms"], 3)
    except RuntimeError as err:                                          # (out of memory in torch's sparse backward: say so, keep the rest)
        out["torch_sparse_mm_forward_backward_ms"] = None
        out["torch_error"] = str(err).splitlines()[0][:200]
    torch.cuda.empty_cache()

    # ---- one backward application alone, in the sorted order the call runs in
    perm, rank, keys, st = ops.coords_order_batched(C)
    nbr_s, status = ops.knn_batched(keys, perm, K)
    Es = ops.l2norm_rows_(ops.gather_rows(E, EMBED, perm.long()))
    w = ops.affinity_softmax(Es, nbr_s, SHARPEN)
    tr_off, tr_slot = ops.pool_transpose_build(nbr_s)
    deg = (tr_off[1:] - tr_off[:-1]).cpu().numpy()
    out.update({"in_degree_median": float(np.median(deg)), "in_degree_max": int(deg.max()), "in_degree_min": int(deg.min())})
    g, spare, dw = R.clone(), torch.empty_like(R), torch.empty((n, K), device="cuda")
    out["transpose_build_ms"] = round(median_ms(lambda: ops.pool_transpose_build(nbr_s)), 3)
    out["transpose_apply_ms"] = round(median_ms(lambda: ops.pool_ell_transpose(g, tr_off, tr_slot, w, K, spare)), 3)
    out["wgrad_apply_ms"] = round(median_ms(lambda: ops.pool_ell_wgrad(g, X, nbr_s, dw, True)), 3)
    out["forward_apply_ms"] = round(median_ms(lambda: ops.pool_ell(X, nbr_s, w, D, spare)), 3)
    tr_bytes = n * K * (D * 4 + 8) + n * D * 4 + (n + 1) * 8             # gathered g rows + slot + weight per element, the row written, the offsets
    wg_bytes = n * K * (D * 4 + 4 + 8) + n * D * 4                       # gathered X rows + id + dw read and written, the g row
    out.update({"transpose_apply_bytes": tr_bytes, "wgrad_apply_bytes": wg_bytes,
                "transpose_share_of_hbm_peak": round(tr_bytes / (out["transpose_apply_ms"] * 1e-3) / HBM_PEAK, 3),
                "wgrad_share_of_hbm_peak": round(wg_bytes / (out["wgrad_apply_ms"] * 1e-3) / HBM_PEAK, 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
