"""Quantisation of batched point clouds on the device: points in, unique voxels and an inverse map out, with autograd back to the
points.  The step the reference writes by hand in front of the student (models/affinity_module.py:1192-1212: torch.unique(...,
return_inverse=True) + torch_scatter.scatter_mean + ME.SparseTensor(features, batched_coordinates), then
s_output.F[sample_to_voxel_map]) and every MinkowskiEngine user gets from SparseTensor(quantization_mode=...).

    q = quantize(coordinates, features, mode="average")         # coordinates [N,4] = batch, x, y, z; duplicates allowed
    y = student(SparseTensor(features=q.features, coordinates=q.coordinates))
    per_point = y.F[q.inverse_mapping]

The indices come from ops.quantize_batched (the key and order of ops.coords_order_batched: batch << 48 | morton(xyz - min)); the
features are reduced by the kernels the pipeline already has, ops.scatter_mean_csr ("average") and ops.gather_rows ("subsample").
"""
import torch

from . import ops

MODES = ("average", "subsample")
COLLISIONS = ("differ", "count", "first")


class Quantized:
    """coordinates i32 [nv,4] in ascending key order, features fp32 [nv,D] or None, labels i64 [nv] or None, inverse_mapping i64 [N]
    (point -> voxel row: coordinates[inverse_mapping] are the points' quantised coordinates), unique_index i64 [nv] (the lowest
    point of each voxel) and counts i64 [nv] (points per voxel)."""

    def __init__(self, coordinates, features, labels, inverse_mapping, unique_index, counts):
        self.coordinates, self.features, self.labels = coordinates, features, labels
        self.inverse_mapping, self.unique_index, self.counts = inverse_mapping, unique_index, counts


def _rows_f32(t):
    """t as contiguous fp32 rows on a 16-byte aligned base.  The alignment is for gather_rows_kernel, which picks its float4 path
    from d and the row strides alone, not from the base pointer (gp_scatter_mean_csr checks the pointer itself)."""
    t = t.float().contiguous()
    return t.clone() if t.data_ptr() % 16 else t


class _Average(torch.autograd.Function):
    """out[v] = mean of the rows of voxel v (ops.scatter_mean_csr: fp32 sums in ascending point row, one division);
    d feats[i] = d out[inverse[i]] / counts[inverse[i]]"""

    @staticmethod
    def forward(ctx, feats, q):
        src = _rows_f32(feats.detach())
        d = src.shape[1]
        out = torch.empty((q.nv, d), dtype=torch.float32, device=src.device)
        ops.scatter_mean_csr(src, d, q.order, q.seg_start, q.nv, out)
        ctx.q, ctx.dtype = q, feats.dtype
        return out

    @staticmethod
    def backward(ctx, d_out):
        q = ctx.q
        g = ops.gather_rows(_rows_f32(d_out), d_out.shape[1], q.inverse)
        g = g / q.counts.index_select(0, q.inverse).to(torch.float32).unsqueeze(1)
        return g.to(ctx.dtype), None


class _Subsample(torch.autograd.Function):
    """out[v] = feats[unique_index[v]] (ops.gather_rows); d feats[i] = d out[v] where i = unique_index[v], zero on every other row
    (a gather by inverse, masked: every row is written once, nothing accumulates)"""

    @staticmethod
    def forward(ctx, feats, q):
        src = _rows_f32(feats.detach())
        ctx.q, ctx.dtype = q, feats.dtype
        return ops.gather_rows(src, src.shape[1], q.unique_index)

    @staticmethod
    def backward(ctx, d_out):
        q = ctx.q
        g = ops.gather_rows(_rows_f32(d_out), d_out.shape[1], q.inverse)
        chosen = q.unique_index.index_select(0, q.inverse) == torch.arange(q.n, device=g.device)
        return torch.where(chosen.unsqueeze(1), g, torch.zeros((), dtype=g.dtype, device=g.device)).to(ctx.dtype), None


def _voxel_size(quantization_size, like):
    """quantization_size (a scalar or 3 values) as a [3] tensor of `like`'s dtype and device"""
    qs = torch.as_tensor(quantization_size, dtype=torch.float64).reshape(-1)
    if qs.numel() == 1:
        qs = qs.expand(3)
    if qs.numel() != 3 or not bool(torch.isfinite(qs).all()) or not bool((qs > 0).all()):
        raise ValueError(f"quantize: quantization_size must be a positive scalar or 3 positive values, got {quantization_size!r}")
    if not like.dtype.is_floating_point and not bool((qs == qs.round()).all()):
        raise ValueError(f"quantize: {like.dtype} coordinates take an integer quantization_size, got {quantization_size!r}")
    return qs.to(device=like.device, dtype=like.dtype)


def quantize(coordinates, features=None, labels=None, *, mode="average", quantization_size=None, ignore_label=255, collision="differ"):
    """coordinates [N,4] (batch, x, y, z), integer or floating, on the GPU, in any row order; with quantization_size (a scalar or one
    value per axis) columns 1..3 become floor(x / quantization_size) first; floating coordinates given without a quantization_size
    are floored to their cells as they are (as ME.utils.batched_coordinates does), the batch column must be integral.
    features [N,D] of any floating dtype and row stride (copied to contiguous fp32 rows when they are not),
    reduced per voxel in fp32 under autograd: mode "average" is the mean (ME's UNWEIGHTED_AVERAGE), "subsample" the row of the
    voxel's lowest point (ME's RANDOM_SUBSAMPLE with the choice made deterministic).  labels [N] integer, merged by `collision`:
    "differ" gives ignore_label where two labels of a voxel differ (ME's sparse_quantize), "count" where a voxel holds more than one
    point (dataset/voxelization_utils.py:86-89), "first" takes the lowest point's label.  -> Quantized.  Host syncs: the status
    read-back of ops.quantize_batched, and one range read-back before it unless the coordinates are int32 already."""
    C, Fe, L = coordinates, features, labels
    if mode not in MODES:
        raise ValueError(f"quantize: mode={mode!r}, expected one of {MODES}")
    if collision not in COLLISIONS:
        raise ValueError(f"quantize: collision={collision!r}, expected one of {COLLISIONS}")
    if not torch.is_tensor(C) or C.dim() != 2 or C.shape[1] != 4:
        raise ValueError(f"quantize: coordinates must be [N, 4] (batch, x, y, z), got "
                         f"{list(C.shape) if torch.is_tensor(C) else type(C).__name__}")
    if C.dtype == torch.bool or C.dtype.is_complex:
        raise ValueError(f"quantize: coordinates must be integers or floating point, got {C.dtype}")
    n = C.shape[0]
    if Fe is not None and (not torch.is_tensor(Fe) or Fe.dim() != 2 or Fe.shape[0] != n or Fe.shape[1] < 1):
        raise ValueError(f"quantize: features must be [N, D] with N = {n} coordinate rows, got "
                         f"{list(Fe.shape) if torch.is_tensor(Fe) else type(Fe).__name__}")
    if L is not None and (not torch.is_tensor(L) or L.dim() != 1 or L.shape[0] != n):
        raise ValueError(f"quantize: labels must be [N] with N = {n} coordinate rows, got "
                         f"{list(L.shape) if torch.is_tensor(L) else type(L).__name__}")
    if not (C.is_cuda and (Fe is None or Fe.is_cuda) and (L is None or L.is_cuda)):
        raise ValueError(f"quantize: coordinates, features and labels must be CUDA tensors (got {C.device} / "
                         f"{Fe.device if Fe is not None else None} / {L.device if L is not None else None}); there is no CPU path")
    if any(t is not None and t.device != C.device for t in (Fe, L)):
        raise ValueError(f"quantize: coordinates, features and labels must be on one device (got {C.device} / "
                         f"{Fe.device if Fe is not None else None} / {L.device if L is not None else None})")
    if Fe is not None and not Fe.dtype.is_floating_point:
        raise ValueError(f"quantize: features must be floating point, got {Fe.dtype}")
    if L is not None and (L.dtype.is_floating_point or L.dtype.is_complex or L.dtype == torch.bool):
        raise ValueError(f"quantize: labels must be integers, got {L.dtype}")
    if n == 0:
        raise ValueError("quantize: empty point cloud")
    dev = C.device
    with torch.cuda.device(dev):
        C = C.detach()
        if quantization_size is not None:
            cells = torch.div(C[:, 1:], _voxel_size(quantization_size, C), rounding_mode="floor")
            C = torch.cat([C[:, :1], cells], 1)
        if C.dtype != torch.int32:
            # (checked before the cast: a coordinate beyond int32 must not wrap into a valid one, NaN / inf must not become one)
            if C.dtype.is_floating_point:
                lo, hi = torch.aminmax(torch.nan_to_num(C.double(), nan=0.0, posinf=0.0, neginf=0.0))
                bad = torch.stack([(~torch.isfinite(C)).sum(), (C[:, 0] != torch.floor(C[:, 0])).sum()]).double()
                lo, hi, n_inf, n_frac = ops.readback(torch.cat([torch.stack([lo, hi]), bad]))
                if n_inf:
                    raise ValueError(f"quantize: {int(n_inf)} coordinates are not finite")
                if n_frac:
                    raise ValueError(f"quantize: {int(n_frac)} rows have a batch index that is not an integer")
                C = torch.floor(C)
                lo, hi = int(lo // 1), int(hi // 1)
            else:
                lo, hi = ops.readback(torch.stack(torch.aminmax(C)).to(torch.int64))
            if lo < -2 ** 31 or hi >= 2 ** 31:
                raise ValueError(f"quantize: coordinates outside the int32 range ({lo} .. {hi})")
        q = ops.quantize_batched(C.to(torch.int32).contiguous())
        # (range first: a row whose batch index is out of range has a meaningless key, which may equal another row's)
        if q.bad_batch:
            raise ValueError(f"quantize: {q.bad_batch} rows have a batch index outside 0..65535")
        if q.bad_axes:
            axes = [a for i, a in enumerate("xyz") if q.bad_axes >> i & 1]
            raise ValueError(f"quantize: coordinate extent of 65536 or more along {', '.join(axes)} (16 bits per axis)")
        feats = None
        if Fe is not None:
            feats = (_Average if mode == "average" else _Subsample).apply(Fe, q)
        labs = None
        if L is not None:
            labs = ops.segment_labels(L.to(torch.int64).contiguous(), q, ignore_label, collision)
    return Quantized(q.coordinates, feats, labs, q.inverse, q.unique_index, q.counts)
