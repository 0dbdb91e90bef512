"""Tensor-level wrappers over the C-ABI (include/geopurify_hip.h).

Every function takes/returns torch CUDA tensors but hands the library raw device pointers, sizes
and the current HIP stream.  PyTorch is plumbing here: allocation and stream ownership only.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _chk(t, dtype, name):
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous CUDA {dtype}, got {t.dtype} cuda={t.is_cuda} contig={t.is_contiguous()}")
    return t


# host time spent BLOCKED in the hot path's device -> host read-backs (voxel count, per-view counts, chunk plan, pair bounds, union
# rows): a scheduler that runs them ahead (bench.py's look-ahead) reports its own enqueue time net of these waits
READBACK = {"seconds": 0.0, "calls": 0}


def readback(t):
    """t.tolist() of a small device tensor, the wait accounted in READBACK (one host synchronisation of the calling stream)"""
    import time
    t0 = time.perf_counter()
    v = t.tolist()
    READBACK["seconds"] += time.perf_counter() - t0
    READBACK["calls"] += 1
    return v


def _dbl16(m):
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(16))
    return (ctypes.c_double * 16)(*a.tolist())


# ------------------------------------------------------------------------------------------ rows 1-3
def voxelize(coords, rigid):
    """coords f64 [N,3] cuda; rigid 4x4 (host).  Returns dict with coords_aug f64 [Nv,3], inds,
    inds_reconstruct, order, seg_start (CSR of each voxel's points), nv.  One host sync (nv)."""
    lib = _lib.load()
    _chk(coords, torch.float64, "coords")
    n = coords.shape[0]
    dev = coords.device
    ws = _ws(lib.gp_voxelize_workspace_bytes(n), dev)
    ca = torch.empty((n, 3), dtype=torch.float64, device=dev)
    inds = torch.empty(n, dtype=torch.int64, device=dev)
    inv = torch.empty(n, dtype=torch.int64, device=dev)
    order = torch.empty(n, dtype=torch.int64, device=dev)
    seg = torch.empty(n + 1, dtype=torch.int64, device=dev)
    nvd = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib.gp_voxelize_f64(_ptr(coords), n, _dbl16(rigid), _ptr(ca), _ptr(inds), _ptr(inv), _ptr(nvd),
                              _ptr(order), _ptr(seg), _ptr(ws), ws.numel(), _stream()), "gp_voxelize_f64")
    nv = int(readback(nvd)[0])
    return {"coords_aug": ca[:nv], "inds": inds[:nv], "inds_reconstruct": inv, "order": order,
            "seg_start": seg[:nv + 1], "nv": nv}


def fnv_hash(coords):
    lib = _lib.load()
    _chk(coords, torch.float64, "coords")
    out = torch.empty(coords.shape[0], dtype=torch.int64, device=coords.device)   # bit pattern of uint64
    check(lib.gp_fnv_hash_f64(_ptr(coords), coords.shape[0], _ptr(out), _stream()), "gp_fnv_hash_f64")
    return out


def project_points(coords, w2c, fx, fy, cx, cy, depth, width, height, cut_bound, vis_thres, want_weight=False):
    lib = _lib.load()
    _chk(coords, torch.float64, "coords")
    n = coords.shape[0]
    if depth is not None:
        _chk(depth, torch.float64, "depth")
        assert depth.shape == (height, width)
    mapping = torch.empty((n, 3), dtype=torch.int64, device=coords.device)
    weight = torch.empty(n, dtype=torch.float64, device=coords.device) if want_weight else None
    check(lib.gp_project_points_f64(_ptr(coords), n, _dbl16(w2c), float(fx), float(fy), float(cx), float(cy),
                                    _ptr(depth), int(width), int(height), int(cut_bound), float(vis_thres),
                                    _ptr(mapping), _ptr(weight), _stream()), "gp_project_points_f64")
    return (mapping, weight) if want_weight else mapping


def render_depth(coords, w2c, fx, fy, cx, cy, width, height, cut_bound):
    """z-buffer of the cloud (ScanNet mapper, depth given as a str: fusion_util.py:126-130) -> f64 [H,W]."""
    lib = _lib.load()
    _chk(coords, torch.float64, "coords")
    depth = torch.empty((height, width), dtype=torch.float64, device=coords.device)
    check(lib.gp_render_depth_f64(_ptr(coords), coords.shape[0], _dbl16(w2c), float(fx), float(fy), float(cx), float(cy),
                                  int(width), int(height), int(cut_bound), _ptr(depth), _stream()), "gp_render_depth_f64")
    return depth


# ------------------------------------------------------------------------------------------ order / grid
def minmax_i32(coords):
    """Per-axis (min xyz, max xyz) of int32 coordinates [n,3] -> int32 [6] on the device, no sync."""
    lib = _lib.load()
    _chk(coords, torch.int32, "coords")
    mm = torch.empty(6, dtype=torch.int32, device=coords.device)
    check(lib.gp_minmax_i32(_ptr(coords), coords.shape[0], _ptr(mm), _stream()), "gp_minmax_i32")
    return mm


def morton_order(coords_i32):
    lib = _lib.load()
    _chk(coords_i32, torch.int32, "coords")
    nv = coords_i32.shape[0]
    dev = coords_i32.device
    ws = _ws(lib.gp_morton_order_workspace_bytes(nv), dev)
    perm = torch.empty(nv, dtype=torch.int32, device=dev)
    rank = torch.empty(nv, dtype=torch.int32, device=dev)
    check(lib.gp_morton_order(_ptr(coords_i32), nv, _ptr(perm), _ptr(rank), _ptr(ws), ws.numel(), _stream()),
          "gp_morton_order")
    return perm, rank


class Grid:
    """Opaque lattice grid buffer (device) + the host-side origin/extent it was built with."""

    def __init__(self, buf, origin, extent, nv):
        self.buf, self.origin, self.extent, self.nv = buf, origin, extent, nv

    def status(self):
        return int(self.buf[36:40].view(torch.int32).item())      # GpGridHeader.status


def grid_build(coords_sorted, origin=None, extent=None):
    """coords_sorted i32 [nv,3] in Morton order.  origin/extent (host ints) are computed with one
    sync if not given."""
    lib = _lib.load()
    _chk(coords_sorted, torch.int32, "coords")
    nv = coords_sorted.shape[0]
    if origin is None or extent is None:
        lo = coords_sorted.amin(0)
        hi = coords_sorted.amax(0)
        lohi = torch.stack([lo, hi]).cpu().tolist()
        origin = lohi[0]
        extent = [lohi[1][a] - lohi[0][a] + 1 for a in range(3)]
    o = (ctypes.c_int32 * 3)(*[int(v) for v in origin])
    e = (ctypes.c_int32 * 3)(*[int(v) for v in extent])
    nbytes = lib.gp_grid_bytes(nv, e)
    if nbytes == 0:
        raise _lib.GeoPurifyHipError("gp_grid_bytes: invalid extent")
    buf = _ws(nbytes, coords_sorted.device)
    check(lib.gp_grid_build(_ptr(coords_sorted), nv, o, e, _ptr(buf), buf.numel(), _stream()), "gp_grid_build")
    return Grid(buf, list(origin), list(extent), nv)


def kernel_map_build(grid, coords_sorted):
    lib = _lib.load()
    nv = coords_sorted.shape[0]
    nm = torch.empty((27, nv), dtype=torch.int32, device=coords_sorted.device)
    check(lib.gp_kernel_map_build(_ptr(grid.buf), _ptr(coords_sorted), nv, _ptr(nm), _stream()), "gp_kernel_map_build")
    return nm


def coords_order_batched(coords_b):
    """Batched coordinates i32 [nv,4] (batch, x, y, z; any row order) -> perm, rank (i32 [nv], as morton_order), the sorted keys
    (u64 held in an i64 [nv]) and status i32 [3] = (duplicate rows, rows with a batch index outside 0..65535, mask of the axes
    whose extent is 65536 or more), all on the device, no sync (gp_coords_order_batched)."""
    lib = _lib.load()
    _chk(coords_b, torch.int32, "coords")
    if coords_b.dim() != 2 or coords_b.shape[1] != 4:
        raise ValueError(f"coords_order_batched: expected [nv, 4], got {list(coords_b.shape)}")
    nv = coords_b.shape[0]
    dev = coords_b.device
    ws = _ws(lib.gp_coords_order_batched_workspace_bytes(nv), dev)
    perm = torch.empty(nv, dtype=torch.int32, device=dev)
    rank = torch.empty(nv, dtype=torch.int32, device=dev)
    keys = torch.empty(nv, dtype=torch.int64, device=dev)
    status = torch.empty(3, dtype=torch.int32, device=dev)
    check(lib.gp_coords_order_batched(_ptr(coords_b), nv, _ptr(perm), _ptr(rank), _ptr(keys), _ptr(status), _ptr(ws), ws.numel(),
                                      _stream()), "gp_coords_order_batched")
    return perm, rank, keys, status


def kernel_map_sorted(keys_sorted):
    """27-offset kernel map i32 [27, nv] over the sorted keys of coords_order_batched (rows in that order; gp_kernel_map_sorted)."""
    lib = _lib.load()
    _chk(keys_sorted, torch.int64, "keys")
    nv = keys_sorted.shape[0]
    nm = torch.empty((27, nv), dtype=torch.int32, device=keys_sorted.device)
    check(lib.gp_kernel_map_sorted(_ptr(keys_sorted), nv, _ptr(nm), _stream()), "gp_kernel_map_sorted")
    return nm


class QuantizedIndex:
    """Result of quantize_batched, every tensor sliced to the nv voxels found: coordinates i32 [nv,4] in ascending key order,
    unique_index i64 [nv] (lowest input row of each voxel), inverse i64 [n], the CSR order i64 [n] + seg_start i64 [nv+1] and
    counts i64 [nv]; bad_batch / bad_axes are the status fields of coords_order_batched (nonzero: the rest is meaningless)."""

    def __init__(self, n, nv, coordinates, unique_index, inverse, order, seg_start, bad_batch, bad_axes):
        self.n, self.nv, self.coordinates, self.unique_index, self.inverse = n, nv, coordinates, unique_index, inverse
        self.order, self.seg_start, self.bad_batch, self.bad_axes = order, seg_start, bad_batch, bad_axes
        self.counts = seg_start[1:] - seg_start[:-1]


QUANTIZE_OUTPUTS = {"vox_coords": (torch.int32, lambda n: (n, 4)), "unique_index": (torch.int64, lambda n: (n,)),
                    "inverse": (torch.int64, lambda n: (n,)), "order": (torch.int64, lambda n: (n,)),
                    "seg_start": (torch.int64, lambda n: (n + 1,)), "status": (torch.int32, lambda n: (3,))}


def quantize_batched(coords_b, buffers=None):
    """Batched coordinates i32 [n,4] (batch, x, y, z; any row order, duplicate rows allowed) -> QuantizedIndex (gp_quantize_batched).
    One read-back, of status (the voxel count sizes the slices).  buffers: optional dict of caller-owned contiguous outputs at
    capacity, by the names and shapes of QUANTIZE_OUTPUTS."""
    lib = _lib.load()
    _chk(coords_b, torch.int32, "coords")
    if coords_b.dim() != 2 or coords_b.shape[1] != 4:
        raise ValueError(f"quantize_batched: expected [n, 4], got {list(coords_b.shape)}")
    n = coords_b.shape[0]
    if not 0 < n < 2 ** 31:
        raise ValueError(f"quantize_batched: n={n} out of range (1 .. 2^31 - 1)")
    dev = coords_b.device
    b = {}
    for name, (dtype, shape) in QUANTIZE_OUTPUTS.items():
        t = (buffers or {}).get(name)
        if t is None:
            t = torch.empty(shape(n), dtype=dtype, device=dev)
        elif _chk(t, dtype, name).shape != shape(n) or t.device != dev:
            raise ValueError(f"quantize_batched: buffer {name} must be {list(shape(n))} on {dev}, got {list(t.shape)} on {t.device}")
        b[name] = t
    ws = _ws(lib.gp_quantize_batched_workspace_bytes(n), dev)
    check(lib.gp_quantize_batched(_ptr(coords_b), n, _ptr(b["vox_coords"]), _ptr(b["unique_index"]), _ptr(b["inverse"]),
                                  _ptr(b["order"]), _ptr(b["seg_start"]), _ptr(b["status"]), _ptr(ws), ws.numel(), _stream()),
          "gp_quantize_batched")
    nv, bad_batch, bad_axes = readback(b["status"])
    return QuantizedIndex(n, nv, b["vox_coords"][:nv], b["unique_index"][:nv], b["inverse"], b["order"], b["seg_start"][:nv + 1],
                     bad_batch, bad_axes)


SEGMENT_LABEL_RULES = {"first": 0, "differ": 1, "count": 2}


def segment_labels(labels, q, ignore_label, rule, out=None):
    """Per-voxel label i64 [nv] of the points' labels i64 [n] over the CSR of q = quantize_batched(...) (gp_segment_labels).
    rule "first": the label of the voxel's lowest row; "differ": ignore_label where two labels of the voxel differ; "count":
    ignore_label where the voxel holds more than one point."""
    lib = _lib.load()
    if rule not in SEGMENT_LABEL_RULES:
        raise ValueError(f"segment_labels: rule={rule!r}, expected one of {sorted(SEGMENT_LABEL_RULES)}")
    _chk(labels, torch.int64, "labels")
    if labels.dim() != 1 or labels.shape[0] != q.n:
        raise ValueError(f"segment_labels: expected labels [{q.n}], got {list(labels.shape)}")
    if labels.device != q.order.device:
        raise ValueError(f"segment_labels: labels on {labels.device}, the quantisation on {q.order.device}")
    if out is None:
        out = torch.empty(q.nv, dtype=torch.int64, device=labels.device)
    elif _chk(out, torch.int64, "out").shape != (q.nv,) or out.device != labels.device:
        raise ValueError(f"segment_labels: expected out [{q.nv}], got {list(out.shape)}")
    check(lib.gp_segment_labels(_ptr(labels), q.n, _ptr(q.order), _ptr(q.seg_start), _ptr(q.unique_index), q.nv, int(ignore_label),
                                SEGMENT_LABEL_RULES[rule], _ptr(out), _stream()), "gp_segment_labels")
    return out


# ------------------------------------------------------------------------------------------ rows 8-12
def scatter_mean_csr(src, d, order, seg_start, nv, out, col0=0, row_map=None):
    lib = _lib.load()
    _chk(src, torch.float32, "src")
    check(lib.gp_scatter_mean_csr(_ptr(src), src.stride(0), int(d), _ptr(order), _ptr(seg_start), int(nv),
                                  _ptr(row_map), _ptr(out), out.stride(0), int(col0), _stream()),
          "gp_scatter_mean_csr")
    return out


def voxel_rows_operands(f, d, geo, dg, order, seg_start, nv, cin_pad, row_map=None, want_scale=True):
    """Row 8 and its operands in one pass (gp_voxel_rows_operands): X f32 [nv, cin_pad] = voxel means of f[:, :d] | geo[:, :dg] | zeros,
    written through row_map; (rows, None, row_inv) = split_f16(X, cin_pad, per_row=True, interleaved=True); sc = pow2_scale(X, d)
    (None unless want_scale).  Returns (X, (rows, None, row_inv), sc), the bits of those calls."""
    lib = _lib.load()
    _chk(f, torch.float32, "f")
    _chk(geo, torch.float32, "geo")
    dev = f.device
    X = torch.empty((nv, cin_pad), dtype=torch.float32, device=dev)
    rows = torch.empty((nv, 2 * cin_pad), dtype=torch.float16, device=dev)
    rinv = torch.empty(nv, dtype=torch.float32, device=dev)
    sc = torch.empty(2, dtype=torch.float32, device=dev) if want_scale else None
    ws = _ws(256, dev) if want_scale else None
    check(lib.gp_voxel_rows_operands(_ptr(f), f.stride(0), int(d), _ptr(geo), geo.stride(0), int(dg), _ptr(order), _ptr(seg_start), int(nv),
                                     _ptr(row_map), _ptr(X), X.stride(0), int(cin_pad), _ptr(rows), rows.stride(0), _ptr(rinv), _ptr(sc),
                                     _ptr(ws), ws.numel() if ws is not None else 0, _stream()), "gp_voxel_rows_operands")
    return X, (rows, None, rinv), sc


def gather_rows(src, d, index, out=None, row_map=None):
    lib = _lib.load()
    n = index.shape[0]
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=src.device)
    check(lib.gp_gather_rows(_ptr(src), src.stride(0), int(d), _ptr(index), n, _ptr(row_map), _ptr(out),
                             out.stride(0), _stream()), "gp_gather_rows")
    return out


def gather_rows_classify(src, d, index, text_norm, logit_scale, row_map=None):
    """gather_rows + classify_argmax in one pass (gp_gather_rows_classify): returns (out [n, d], pred i64 [n], zero u8 [n]).
    d a multiple of 64 up to 1024 and C * d * 4 <= 64 KiB (can_gather_rows_classify)."""
    lib = _lib.load()
    n = index.shape[0]
    out = torch.empty((n, d), dtype=torch.float32, device=src.device)
    pred = torch.empty(n, dtype=torch.int64, device=src.device)
    zero = torch.empty(n, dtype=torch.uint8, device=src.device)
    check(lib.gp_gather_rows_classify(_ptr(src), src.stride(0), int(d), _ptr(index), n, _ptr(row_map), _ptr(out), out.stride(0),
                                      _ptr(text_norm), int(text_norm.shape[0]), float(logit_scale), _ptr(pred), _ptr(zero), _stream()),
          "gp_gather_rows_classify")
    return out, pred, zero


def can_gather_rows_classify(d, num_classes):
    # up to 512 columns the 16-lane form of classify_argmax, wider rows (<= 1024) its one-wave-per-point form; the text matrix in LDS
    return d % 64 == 0 and d <= 1024 and num_classes * d * 4 <= 64 * 1024


def pool_cs_width_ok(d):
    """Widths the column-sliced pooling kernels take (gp_pool_cs_apply / _apply_chain): whole 256-column slices, 1 to 4 of them."""
    return d % 256 == 0 and 256 <= d <= 1024


def sparse_conv(x, nbr_map, w, scale=None, shift=None, residual=None, relu=False, out=None):
    """x fp32 [nv, >=cin] (row stride = x.stride(0)); w fp32 [27,cin,cout] or [cin,cout]."""
    lib = _lib.load()
    nv = x.shape[0]
    if w.dim() == 3:
        kv, cin, cout = w.shape
    else:
        kv, (cin, cout) = 1, w.shape
    _chk(w, torch.float32, "w")
    if out is None:
        out = torch.empty((nv, cout), dtype=torch.float32, device=x.device)
    check(lib.gp_sparse_conv(_ptr(x), x.stride(0), _ptr(nbr_map) if kv > 1 else None, nv, _ptr(w), int(kv),
                             int(cin), int(cout), _ptr(scale), _ptr(shift), _ptr(residual),
                             residual.stride(0) if residual is not None else 0, int(bool(relu)), _ptr(out),
                             out.stride(0), _stream()), "gp_sparse_conv")
    return out


class ConvPairs:
    """Compacted kernel map of one scene (shared by every 3x3x3 layer)."""

    def __init__(self, pair_in, pair_pos, seg_off, tile_start, nseg, num_pairs, nv):
        self.pair_in, self.pair_pos, self.pair_off, self.tile_start = pair_in, pair_pos, seg_off, tile_start
        self.nseg, self.num_pairs, self.nv = nseg, num_pairs, nv
        self.partial = None
        self.num_chunks, self.chunk_row_off, self.chunk_tile_off, self.chunk_pair_off = 0, None, None, None   # 0 = not chunked

    def _set_chunks(self, rows, tiles, pairs):
        n = len(rows) - 1
        self.num_chunks = n
        self.chunk_row_off = (ctypes.c_int32 * (n + 1))(*rows)
        self.chunk_tile_off = (ctypes.c_int32 * (n + 1))(*tiles)
        self.chunk_pair_off = (ctypes.c_int32 * (n + 1))(*pairs)
        self.max_chunk_pairs = max(pairs[i + 1] - pairs[i] for i in range(n))

    def regroup(self, g):
        """The same pair ORDER (chunk-major: a chunk's 27 offset segments gather from the same few thousand input rows, which
        keeps the gathered operand in the XCDs' L2) executed `g` chunks per LAUNCH: phase 1 of g consecutive chunks is one grid
        (fewer partly filled last rounds and kernel boundaries per layer), phase 2 follows for their rows; the partial buffer
        then holds g chunks.  Returns a ConvPairs sharing the device arrays."""
        g = max(1, min(int(g), max(self.num_chunks, 1)))
        cp = ConvPairs(self.pair_in, self.pair_pos, self.pair_off, self.tile_start, self.nseg, self.num_pairs, self.nv)
        cp.tile_desc = self.tile_desc
        n = self.num_chunks
        idx = list(range(0, n, g)) + [n]
        ro, po, to = list(self.chunk_row_off), list(self.chunk_pair_off), list(self.chunk_tile_off)
        cp._set_chunks([ro[i] for i in idx], [to[i] for i in idx], [po[i] for i in idx])
        return cp


# phase-1 tiles per chunk launch of the balanced chunking: None = three rounds of one-tile workgroups less 16 = 3 x the CU count - 16
# (752 on MI355X).  Rounds 3-4, fp32 partial rows: two rounds (512; 768 was slower -- 200 MB of partial rows per chunk).  Round 5, 24-bit
# partial rows (150 MB per 768 tiles): 752 / 768 beat 512 by 1.1 % of the scene, 640 (2.5 rounds) loses 4 %, 1024 is 0.5 % behind 768
CONV_TARGET_TILES = None       # (a tuning script may set it: scripts/conv_layer_time.py)


def conv_pairs_build(nbr_map, chunk_rows="balanced", col_tiles=2):
    """nbr_map i32 [27,nv] -> ConvPairs.  Pairs are ordered chunk-major and phase 1 / phase 2 run chunk by chunk, so the partial
    buffer only holds one chunk.  chunk_rows:
      "balanced" (default): chunk heights chosen on the device from the kernel map (gp_conv_chunk_plan) so that every chunk's
          phase-1 launch is at most 3 x CUs - 16 tiles = three rounds of workgroups (col_tiles = cout / 256 column tiles
          per row tile); two host syncs (the plan, the pair bounds);
      an int: equal heights.  Round 4 on the S scene (profiles/r04_conv_launch_groups.log), per 512->512 layer: 8192 rows (17
          launches, 128 MB of partial rows -- inside the Infinity Cache) 1.87 ms, 16384 rows (250 MB) 1.96 ms, 4096 rows 2.65 ms;
          a layer's time follows the rounds of 256 tiles its launches need (profiles/r04_conv_rounds.log); several chunks per
          launch (ConvPairs.regroup) never wins;  None = one chunk.  One host sync."""
    lib = _lib.load()
    kv, nv = nbr_map.shape
    dev = nbr_map.device
    if isinstance(chunk_rows, str):
        if chunk_rows != "balanced":
            raise ValueError(f"conv_pairs_build: chunk_rows={chunk_rows!r}")
    if isinstance(chunk_rows, str):
        granule = 256
        max_chunks = (nv + granule - 1) // granule
        plan = torch.empty(max_chunks + 2, dtype=torch.int32, device=dev)          # [0 .. max_chunks]: row offsets, [-1]: count
        ws = _ws(lib.gp_conv_chunk_plan_workspace_bytes(nv, granule), dev)
        target = CONV_TARGET_TILES or 3 * torch.cuda.get_device_properties(dev).multi_processor_count - 16
        check(lib.gp_conv_chunk_plan(_ptr(nbr_map), nv, kv, granule, int(col_tiles), int(target), max_chunks, _ptr(plan),
                                     _ptr(plan[max_chunks + 1:]), _ptr(ws), ws.numel(), _stream()), "gp_conv_chunk_plan")
        host = readback(plan)                                                        # host sync 1 of 2
        nchunks = host[max_chunks + 1]
        rows = host[:nchunks + 1]
        row_off = plan[:nchunks + 1]
    else:
        ch = nv if chunk_rows is None else max(int(chunk_rows), 256)
        rows = list(range(0, nv, ch)) + [nv]
        nchunks = len(rows) - 1
        row_off = torch.tensor(rows, dtype=torch.int32, device=dev)
    nseg = nchunks * kv
    ws = _ws(lib.gp_conv_pairs_workspace_bytes(nv, kv), dev)
    pair_in = torch.empty(kv * nv, dtype=torch.int32, device=dev)
    pair_pos = torch.empty((kv, nv), dtype=torch.int32, device=dev)
    seg_off = torch.empty(nseg + 1, dtype=torch.int32, device=dev)
    tile_start = torch.empty(nseg + 1, dtype=torch.int32, device=dev)
    tile_desc = torch.empty(((kv * nv) // 256 + nseg + 1, 4), dtype=torch.int32, device=dev)
    check(lib.gp_conv_pairs_build(_ptr(nbr_map), nv, kv, nchunks, _ptr(row_off), _ptr(pair_in), _ptr(pair_pos), _ptr(seg_off),
                                  _ptr(tile_start), _ptr(tile_desc), _ptr(ws), ws.numel(), _stream()), "gp_conv_pairs_build")
    bounds = readback(torch.stack([seg_off[::kv], tile_start[::kv]]))          # the host sync of this call (number of pairs)
    num_pairs = bounds[0][-1]
    cp = ConvPairs(pair_in, pair_pos, seg_off, tile_start, nseg, num_pairs, nv)
    cp.tile_desc = tile_desc
    # host copies of the chunk boundaries (exact row / tile / pair counts per chunk; a single chunk included)
    cp._set_chunks(rows, bounds[1], bounds[0])
    return cp


def conv_weights_split(w, scale_pow2, blocked=None, transpose_flip=False):
    """w fp32 [kv,cin,cout] -> (w_hi, w_lo) f16 of scale_pow2*w.
    blocked (default: whenever the shape allows, cin % 32 == 0 and cout % 256 == 0): the step-blocked layout of the two-phase
    convolution, tensors of shape [kv, cout/256, cin/32, 256, 32] -- sparse_conv_f16x3 recognises it by its five dimensions;
    else [kv,cout,cin] (the dense output layer's operand, gp_embed_head_f16x3; also accepted by sparse_conv_f16x3).
    transpose_flip: the halves of V[k] = w[kv-1-k]^T (the data-gradient operand; V's cin = w's cout and vice versa) straight from w."""
    lib = _lib.load()
    kv, cin, cout = w.shape
    if transpose_flip:
        if cout % 32 == 0 and cin % 256 == 0 and blocked is not False:
            hi = torch.empty((kv, cin // 256, cout // 32, 256, 32), dtype=torch.float16, device=w.device)
            lo = torch.empty_like(hi)
            check(lib.gp_conv_weights_split_blocked(_ptr(w), kv, cout, cin, float(scale_pow2), _ptr(hi), _ptr(lo), 1, _stream()),
                  "gp_conv_weights_split_blocked")
            return hi, lo
        return conv_weights_split(w.flip(0).transpose(1, 2).contiguous(), scale_pow2, blocked)
    if blocked is None:
        blocked = cin % 32 == 0 and cout % 256 == 0
    if blocked:
        hi = torch.empty((kv, cout // 256, cin // 32, 256, 32), dtype=torch.float16, device=w.device)
        lo = torch.empty_like(hi)
        check(lib.gp_conv_weights_split_blocked(_ptr(w), kv, cin, cout, float(scale_pow2), _ptr(hi), _ptr(lo), 0, _stream()),
              "gp_conv_weights_split_blocked")
        return hi, lo
    hi = torch.empty((kv, cout, cin), dtype=torch.float16, device=w.device)
    lo = torch.empty((kv, cout, cin), dtype=torch.float16, device=w.device)
    check(lib.gp_conv_weights_split(_ptr(w), kv, cin, cout, float(scale_pow2), _ptr(hi), _ptr(lo), _stream()),
          "gp_conv_weights_split")
    return hi, lo


def conv_weights_shape(w_hi):
    """(kv, cout, cin) of a split weight tensor in either layout"""
    if w_hi.dim() == 5:
        return int(w_hi.shape[0]), int(w_hi.shape[1]) * 256, int(w_hi.shape[2]) * 32
    return tuple(int(v) for v in w_hi.shape)


def split_f16(x, d=None, scale=None, per_row=False, interleaved=False, dst_row=None, extra_zero_rows=0):
    """fp32 rows -> (hi, lo) f16 rows with x * s = hi + lo.  Unscaled (s = 1): exact to 2^-22 relative only for |x| >= 2^-3
    (below that the lo half is a subnormal f16: absolute error 2^-25).  scale = device scalar from pow2_scale(): one power of
    two for the whole block; per_row=True: a power of two per row, returns (hi, lo, row_inv_scale).
    dst_row (i32 [n], a permutation; scaled forms only): row r is written to row dst_row[r] of the outputs (rcb_order's map).
    extra_zero_rows (plane forms): that many all-zero rows behind the n rows of hi and lo (the weight gradient's padded pairs point there)."""
    lib = _lib.load()
    d = x.shape[1] if d is None else d
    if interleaved:
        # (rows, None, row_inv_scale): per 32-column step [hi 32 | lo 32] in one tensor -- the operand form sparse_conv_f16x3 stages in full lines
        assert per_row and d % 32 == 0, "interleaved rows are the row-scaled operand of the convolution"
        rows = torch.empty((x.shape[0], 2 * d), dtype=torch.float16, device=x.device)
        rinv = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        check(lib.gp_split_f16_scaled(_ptr(x), x.stride(0), int(d), x.shape[0], _ptr(rows), None, rows.stride(0), None, _ptr(rinv),
                                      _ptr(dst_row), _stream()), "gp_split_f16_scaled")
        return rows, None, rinv
    hi = torch.empty((x.shape[0] + extra_zero_rows, d), dtype=torch.float16, device=x.device)
    lo = torch.empty((x.shape[0] + extra_zero_rows, d), dtype=torch.float16, device=x.device)
    if extra_zero_rows:
        hi[x.shape[0]:].zero_()
        lo[x.shape[0]:].zero_()
    if scale is None and not per_row:
        if dst_row is not None:
            raise ValueError("split_f16: dst_row needs a scaled form (scale= or per_row=True)")
        check(lib.gp_split_f16(_ptr(x), x.stride(0), int(d), x.shape[0], _ptr(hi), _ptr(lo), hi.stride(0), _stream()),
              "gp_split_f16")
        return hi, lo
    rinv = torch.empty(x.shape[0], dtype=torch.float32, device=x.device) if per_row else None
    check(lib.gp_split_f16_scaled(_ptr(x), x.stride(0), int(d), x.shape[0], _ptr(hi), _ptr(lo), hi.stride(0), _ptr(scale),
                                  _ptr(rinv), _ptr(dst_row), _stream()), "gp_split_f16_scaled")
    return (hi, lo, rinv) if per_row else (hi, lo)


def rcb_order(coords_sorted, chunk_rows=1024, leaf_rows=128):
    """Row order for the pooling operator (gp_rcb_order): recursive coordinate bisection of the Morton-ordered integer coords
    [nv, 3] inside chunks of chunk_rows rows into leaves of leaf_rows rows.  Returns (sigma, rho) i32 [nv]: new position -> row,
    row -> new position."""
    lib = _lib.load()
    _chk(coords_sorted, torch.int32, "coords")
    nv = coords_sorted.shape[0]
    sigma = torch.empty(nv, dtype=torch.int32, device=coords_sorted.device)
    rho = torch.empty(nv, dtype=torch.int32, device=coords_sorted.device)
    check(lib.gp_rcb_order(_ptr(coords_sorted), nv, int(chunk_rows), int(leaf_rows), _ptr(sigma), _ptr(rho), _stream()), "gp_rcb_order")
    return sigma, rho


def rows_renumber(nbr, sigma, rho):
    """out[p, j] = rho[nbr[sigma[p], j]]: neighbour lists i32 [nv, k] in the order / numbering of rcb_order"""
    lib = _lib.load()
    nv, k = nbr.shape
    out = torch.empty_like(nbr)
    check(lib.gp_rows_renumber_i32(_ptr(nbr), nv, int(k), _ptr(sigma), _ptr(rho), _ptr(out), _stream()), "gp_rows_renumber_i32")
    return out


def pow2_scale(x, d=None):
    """Device tensor [s, 1/s]: s = the power of two that puts max |x[:, :d]| into [2^13, 2^14).  No host sync."""
    lib = _lib.load()
    d = x.shape[1] if d is None else d
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    ws = _ws(256, x.device)
    check(lib.gp_pow2_scale(_ptr(x), x.stride(0), int(d), x.shape[0], _ptr(out), _ptr(ws), ws.numel(), _stream()), "gp_pow2_scale")
    return out


def sparse_conv_f16x3(x, pairs, w_hi, w_lo, scale=None, shift=None, residual=None, relu=False, out=None,
                      x_split=None, out_split=None, x_row_inv=None, out_row_inv=None, want_f32=True, fp32_partials=False, dense_single_offset=False,
                      reference_walk=False):
    """x fp32 [nv, >=cin] and/or x_split=(hi, lo) f16 (pre-split operand -> LDS-DMA path);
    out_split=(hi, lo) f16 buffers to also receive the split output.  x_row_inv fp32 [nv]: the per-row inverse scales of
    a row-scaled x_split; out_row_inv fp32 [nv]: receive the output's (out_split is then row-scaled).
    residual: fp32 rows [nv, >=cout], or a tuple (hi, lo, row_inv | None) of the split planes an earlier layer wrote -- the producer then
    needs no fp32 copy.
    INTERLEAVED rows: any of x_split / out_split / residual may be (t, None[, row_inv]) with t f16 [nv, 2 * channels] holding per 32-channel
    step [hi 32 | lo 32]: the LDS-DMA kernel stages a row and step as one full 128-byte line (interleave_planes / deinterleave_planes
    convert).
    fp32_partials=True: the partial rows between the two phases as fp32 (the format of rounds 1-4, which the 24-bit block-floating rows
    are checked against; also what a call takes by itself when a chunk's 24-bit rows would pass 4 GiB) -- an explicit argument of the
    call (plane_flags bit 3), not a process-wide switch.
    dense_single_offset=True (plane_flags bit 4): kv = 1 and every output row has its pair -- a gather-GEMM; phase 1 writes the fp32 output
    itself, no partial rows, no phase 2.
    reference_walk=True (plane_flags bit 5): phase 2 over the 24-bit partial rows walks its output rows one at a time -- the form that
    the pipelined walk (the default up to 512 columns) is compared with bit for bit; an argument of the call, not a process-wide switch."""
    lib = _lib.load()
    res_planes = residual if isinstance(residual, (tuple, list)) else None
    if res_planes is not None:
        residual = None
    rh, rl, ri = (tuple(res_planes) + (None,))[:3] if res_planes is not None else (None, None, None)
    kv, cout, cin = conv_weights_shape(w_hi)
    w_blocked = int(w_hi.dim() == 5)
    nv = pairs.nv
    dev = w_hi.device
    if dense_single_offset:
        partial = torch.empty(64, dtype=torch.float32, device=dev)                    # (not written: phase 1 stores into `out`)
    else:
        if pairs.partial is None or pairs.partial.shape[1] < cout or pairs.partial.shape[0] < max(pairs.max_chunk_pairs, 1):
            pairs.partial = torch.empty((max(pairs.max_chunk_pairs, 1), cout), dtype=torch.float32, device=dev)
        partial = pairs.partial
    if out is None and (want_f32 or out_split is None):
        out = torch.empty((nv, cout), dtype=torch.float32, device=dev)        # want_f32=False: only the split planes are written
    xh, xl = x_split if x_split is not None else (None, None)
    yh, yl = out_split if out_split is not None else (None, None)
    # interleaved rows ([K step][hi 32 | lo 32], ONE tensor of 2 x channels halfs per row): given as (tensor, None)
    plane_flags = (1 if (xh is not None and xl is None) else 0) | (2 if (yh is not None and yl is None) else 0) | \
                  (4 if (rh is not None and rl is None) else 0) | (8 if fp32_partials else 0) | (16 if dense_single_offset else 0) | (32 if reference_walk else 0)
    check(lib.gp_sparse_conv_f16x3(_ptr(x), x.stride(0) if x is not None else 0, _ptr(xh), _ptr(xl),
                                   xh.stride(0) if xh is not None else 0, _ptr(pairs.pair_in), _ptr(pairs.pair_pos),
                                   _ptr(pairs.pair_off), _ptr(pairs.tile_start), _ptr(pairs.tile_desc), pairs.nseg, pairs.num_pairs, nv, kv, _ptr(w_hi), _ptr(w_lo), cin, cout,
                                   _ptr(partial), _ptr(scale), _ptr(shift), _ptr(residual),
                                   residual.stride(0) if residual is not None else 0, int(bool(relu)), _ptr(out),
                                   out.stride(0) if out is not None else 0, _ptr(yh), _ptr(yl), yh.stride(0) if yh is not None else 0,
                                   int(pairs.num_chunks), pairs.chunk_row_off, pairs.chunk_tile_off, pairs.chunk_pair_off,
                                   _ptr(x_row_inv), _ptr(out_row_inv), _ptr(rh), _ptr(rl), rh.stride(0) if rh is not None else 0, _ptr(ri),
                                   w_blocked, plane_flags, _stream()),
          "gp_sparse_conv_f16x3")
    return out


def interleave_planes(hi, lo):
    """(hi, lo) f16 [n, c] -> one f16 [n, 2 c] of interleaved rows, per 32-channel step [hi 32 | lo 32] (torch ops: tests, tools)"""
    n, c = hi.shape
    return torch.stack([hi.reshape(n, c // 32, 32), lo.reshape(n, c // 32, 32)], dim=2).reshape(n, 2 * c).contiguous()


def deinterleave_planes(t):
    """the inverse of interleave_planes"""
    n, c2 = t.shape
    v = t.reshape(n, c2 // 64, 2, 32)
    return v[:, :, 0].reshape(n, c2 // 2).contiguous(), v[:, :, 1].reshape(n, c2 // 2).contiguous()


def l2norm_rows_(x, d=None):
    lib = _lib.load()
    d = x.shape[1] if d is None else d
    check(lib.gp_l2norm_rows(_ptr(x), x.stride(0), int(d), x.shape[0], _stream()), "gp_l2norm_rows")
    return x


def embed_head_f16x3(x_split, w_hi, w_lo, out_scale, x_row_inv=None, normalize=True, out=None, planes=False, want_f32=True, plane_rows=None):
    """The student's 1x1x1 output layer on pre-split rows, fused with F.normalize (affinity_module.py:66,71,1547).
    x_split = (hi, lo) f16 [nv, >=cin]; w_hi / w_lo f16 [1, cout, cin] or [cout, cin] (conv_weights_split of the [1, cin, cout]
    kernel with a power-of-two pre-scale whose inverse is out_scale).
    planes=True: also returns the rows x 2^10 as f16 (hi, lo) planes -- the operand of affinity_cs_fragments -- written by the same
    epilogue; want_f32=False then skips the fp32 rows.  plane_rows (i32 [nv]): the plane row of input row r (rcb_order's rho).
    Returns out, or (out_or_None, (e_hi, e_lo))."""
    lib = _lib.load()
    hi, lo = x_split
    cout, cin = w_hi.shape[-2:]
    nv = hi.shape[0]
    _chk(hi, torch.float16, "x_hi"), _chk(lo, torch.float16, "x_lo")
    if hi.stride(0) != lo.stride(0) or hi.shape[1] < cin:
        raise ValueError("embed_head_f16x3: the hi / lo planes must share a row stride and hold cin channels")
    if out is None and (want_f32 or not planes):
        out = torch.empty((nv, cout), dtype=torch.float32, device=hi.device)
    eh = el = None
    if planes:
        eh = torch.empty((nv, cout), dtype=torch.float16, device=hi.device)
        el = torch.empty((nv, cout), dtype=torch.float16, device=hi.device)
    check(lib.gp_embed_head_f16x3(_ptr(hi), _ptr(lo), hi.stride(0), _ptr(x_row_inv), _ptr(w_hi), _ptr(w_lo), nv, int(cin), int(cout),
                                  float(out_scale), int(bool(normalize)), _ptr(out), out.stride(0) if out is not None else 0, _ptr(eh), _ptr(el),
                                  AFFINITY_PLANE_SCALE, _ptr(plane_rows) if planes else None, _stream()), "gp_embed_head_f16x3")
    return (out, (eh, el)) if planes else out


def knn_lattice(grid, coords_sorted, ids, k, two_pass=False):
    """two_pass: gp_knn_lattice_two_pass, the form that reads every candidate twice (tests, timing); the same lists"""
    lib = _lib.load()
    nv = coords_sorted.shape[0]
    dev = coords_sorted.device
    ws = _ws(lib.gp_knn_workspace_bytes(nv), dev)
    nbr = torch.empty((nv, k), dtype=torch.int32, device=dev)
    fn, name = (lib.gp_knn_lattice_two_pass, "gp_knn_lattice_two_pass") if two_pass else (lib.gp_knn_lattice, "gp_knn_lattice")
    check(fn(_ptr(grid.buf), _ptr(coords_sorted), _ptr(ids), nv, int(k), _ptr(nbr), _ptr(ws), ws.numel(), _stream()), name)
    return nbr


def knn_batched(keys_sorted, ids, k, nbr=None, status=None, workspace=None):
    """Exact kNN inside every batch entry (gp_knn_batched): keys_sorted (u64 held in an i64 [nv]) and ids = perm (i32 [nv]) as
    coords_order_batched returns them -> (nbr i32 [nv,k] of SORTED-row numbers in (d^2, id) order, status i32 [4] = (queries whose
    entry holds k or fewer voxels -- their rows are -1 --, the lowest such batch index or -1, its voxel count, mask of the axes with a
    decoded coordinate of 32768 or more: lists undefined)), both on the device, no sync.  nbr / status / workspace: optional
    caller-owned contiguous buffers (the workspace uint8 of at least gp_knn_batched_workspace_bytes(nv))."""
    lib = _lib.load()
    _chk(keys_sorted, torch.int64, "keys")
    _chk(ids, torch.int32, "ids")
    nv, k = keys_sorted.shape[0], int(k)
    if keys_sorted.dim() != 1 or ids.shape != (nv,):
        raise ValueError(f"knn_batched: expected keys [nv] and ids [nv], got {list(keys_sorted.shape)} and {list(ids.shape)}")
    dev = keys_sorted.device
    if nbr is None:
        nbr = torch.empty((nv, max(k, 0)), dtype=torch.int32, device=dev)
    elif _chk(nbr, torch.int32, "nbr").shape != (nv, k):
        raise ValueError(f"knn_batched: expected nbr [{nv}, {k}], got {list(nbr.shape)}")
    if status is None:
        status = torch.empty(4, dtype=torch.int32, device=dev)
    elif _chk(status, torch.int32, "status").shape != (4,):
        raise ValueError(f"knn_batched: expected status [4], got {list(status.shape)}")
    ws = _ws(lib.gp_knn_batched_workspace_bytes(nv), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_knn_batched(_ptr(keys_sorted), _ptr(ids), nv, k, _ptr(nbr), _ptr(status), _ptr(ws), ws.numel(), _stream()),
          "gp_knn_batched")
    return nbr, status


def affinity_softmax(e, nbr, sharpen=20.0, d=None, into=None):
    """into: a PoolCs whose structure is built (pool_cs_plan(structure=True)): the weights also go straight into its fragment
    arrays -- the operator is complete when this returns (no pool_cs_fill)."""
    lib = _lib.load()
    nv, k = nbr.shape
    d = e.shape[1] if d is None else d
    w = torch.empty((nv, k), dtype=torch.float32, device=e.device)
    if into is not None:
        if into.dst is None or into.nv != nv or tuple(into.dst.shape) != (nv, k):
            raise ValueError("affinity_softmax: `into` needs a PoolCs structure built from these neighbour lists")
        check(lib.gp_affinity_softmax_scatter(_ptr(e), e.stride(0), int(d), _ptr(nbr), int(k), nv, float(sharpen), _ptr(w),
                                              _ptr(into.dst), _ptr(into.wa_hi), _ptr(into.wa_lo), _stream()),
              "gp_affinity_softmax_scatter")
        into.filled = True
        return w
    check(lib.gp_affinity_softmax(_ptr(e), e.stride(0), int(d), _ptr(nbr), int(k), nv, float(sharpen), _ptr(w),
                                  _stream()), "gp_affinity_softmax")
    return w


_E_SCALE = {}
AFFINITY_PLANE_SCALE = 1024.0      # the embedding planes of affinity_cs_fragments carry e x 2^10 (lo halves stay normal numbers)


def affinity_cs_fragments(e, sharpen, op, planes=None):
    """Row 11 + the operator fill in one matrix-core kernel (gp_affinity_cs_fragments): e fp32 [nv, 128] unit rows -- or planes = their
    (hi, lo) f16 planes x 2^10 as embed_head_f16x3(planes=True) writes them -- and op a PoolCs whose structure was built with
    pool_cs_plan(structure="valid").  Completes op (no [nv, k] weight matrix is produced)."""
    lib = _lib.load()
    if op.valid is None:
        raise ValueError("affinity_cs_fragments: the operator needs pool_cs_plan(structure='valid')")
    if planes is not None:
        eh, el = planes
    else:
        key = str(e.device)
        if key not in _E_SCALE:
            _E_SCALE[key] = torch.tensor([AFFINITY_PLANE_SCALE], dtype=torch.float32, device=e.device)
        eh, el = split_f16(e, 128, scale=_E_SCALE[key])
    check(lib.gp_affinity_cs_fragments(_ptr(eh), _ptr(el), op.nv, 128, int(op.k), float(sharpen), _ptr(op.bu_off), _ptr(op.bu_row),
                                       _ptr(op.bu_mask), _ptr(op.valid), int(op.block_rows), _ptr(op.wa_hi), _ptr(op.wa_lo), _stream()),
          "gp_affinity_cs_fragments")
    op.filled = True
    return op


def pool_ell(x, nbr, w, d, out):
    lib = _lib.load()
    nv, k = nbr.shape
    check(lib.gp_pool_ell(_ptr(x), x.stride(0), _ptr(nbr), _ptr(w), int(k), nv, int(d), _ptr(out), out.stride(0),
                          _stream()), "gp_pool_ell")
    return out


# ------------------------------------------------------------------------------------------ the backward of affinity + pooling
def _flat_nk(t, dtype, nv, k, name):
    """an [nv, k] array the ABI takes without a leading dimension"""
    if _chk(t, dtype, name).shape != (nv, k):
        raise ValueError(f"{name}: expected [{nv}, {k}], got {list(t.shape)}")
    return t


def _rows(t, name, n=None, d=None):
    """fp32 rows [n, d] with unit column stride (the row stride travels as the leading dimension)"""
    if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: expected CUDA fp32 rows with unit column stride, got {t.dtype} {list(t.shape)} strides {t.stride()}")
    if (n is not None and t.shape[0] != n) or (d is not None and t.shape[1] != d):
        raise ValueError(f"{name}: expected [{n}, {d}], got {list(t.shape)}")
    return t


def pool_transpose_build(nbr, tr_off=None, tr_slot=None, workspace=None):
    """The inverted index of the neighbour lists nbr i32 [nv,k] (gp_pool_transpose_build) -> (tr_off i64 [nv+1], tr_slot i32 [nv*k]):
    tr_slot[tr_off[m]:tr_off[m+1]] = the flat slots i*k+j with nbr[i,j] == m, ascending.  No sync.  tr_off / tr_slot / workspace:
    optional caller-owned contiguous buffers (the workspace uint8 of at least gp_pool_transpose_workspace_bytes(nv, k))."""
    lib = _lib.load()
    _chk(nbr, torch.int32, "nbr")
    if nbr.dim() != 2:
        raise ValueError(f"pool_transpose_build: expected nbr [nv, k], got {list(nbr.shape)}")
    nv, k = nbr.shape
    dev = nbr.device
    if tr_off is None:
        tr_off = torch.empty(nv + 1, dtype=torch.int64, device=dev)
    elif _chk(tr_off, torch.int64, "tr_off").shape != (nv + 1,):
        raise ValueError(f"pool_transpose_build: expected tr_off [{nv + 1}], got {list(tr_off.shape)}")
    if tr_slot is None:
        tr_slot = torch.empty(nv * k, dtype=torch.int32, device=dev)
    elif _chk(tr_slot, torch.int32, "tr_slot").shape != (nv * k,):
        raise ValueError(f"pool_transpose_build: expected tr_slot [{nv * k}], got {list(tr_slot.shape)}")
    ws = _ws(lib.gp_pool_transpose_workspace_bytes(nv, int(k)), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_pool_transpose_build(_ptr(nbr), nv, int(k), _ptr(tr_off), _ptr(tr_slot), _ptr(ws), ws.numel(), _stream()),
          "gp_pool_transpose_build")
    return tr_off, tr_slot


def pool_ell_transpose(g, tr_off, tr_slot, w, k, out):
    """out[m] = sum_p w[slot_p] * g[slot_p // k] over the inverted list of m, in list order (gp_pool_ell_transpose): the transposed
    application of pool_ell's operator.  g / out fp32 [nv, d] with any row stride that is a multiple of 4; w fp32 [nv, k]."""
    lib = _lib.load()
    nv, d = _rows(g, "g").shape
    _rows(out, "out", nv, d)
    _chk(tr_off, torch.int64, "tr_off"), _chk(tr_slot, torch.int32, "tr_slot"), _chk(w, torch.float32, "w")
    if tr_off.shape != (nv + 1,) or tr_slot.numel() != w.numel():
        raise ValueError(f"pool_ell_transpose: expected tr_off [{nv + 1}] and one slot per weight, got {list(tr_off.shape)} / "
                         f"{tr_slot.numel()} / {w.numel()}")
    check(lib.gp_pool_ell_transpose(_ptr(g), g.stride(0), _ptr(tr_off), _ptr(tr_slot), _ptr(w), int(k), nv, int(d), _ptr(out),
                                    out.stride(0), _stream()), "gp_pool_ell_transpose")
    return out


def pool_ell_wgrad(g, x_prev, nbr, dw, accumulate):
    """dw[i,j] (+)= <g[i], x_prev[nbr[i,j]]> (gp_pool_ell_wgrad); accumulate=False overwrites.  g / x_prev fp32 [nv, d] with any row
    stride that is a multiple of 4; dw fp32 [nv, k]."""
    lib = _lib.load()
    nv, d = _rows(g, "g").shape
    _rows(x_prev, "x_prev", nv, d)
    _chk(nbr, torch.int32, "nbr")
    k = nbr.shape[1] if nbr.dim() == 2 else -1
    _flat_nk(nbr, torch.int32, nv, k, "nbr"), _flat_nk(dw, torch.float32, nv, k, "dw")
    check(lib.gp_pool_ell_wgrad(_ptr(g), g.stride(0), _ptr(x_prev), x_prev.stride(0), _ptr(nbr), int(k), nv, int(d), _ptr(dw),
                                int(bool(accumulate)), _stream()), "gp_pool_ell_wgrad")
    return dw


def affinity_softmax_backward(e_unit, nbr, w, dw, sharpen, tr_off, tr_slot, out=None, workspace=None):
    """The backward of affinity_softmax on unit rows (gp_affinity_softmax_backward) -> de_unit fp32 [nv, d]: the gather term over the
    row's own list, then the transposed term over its inverted list, both in fixed order.  out / workspace: optional caller-owned
    buffers (out with any row stride that is a multiple of 4; workspace of gp_affinity_softmax_backward_workspace_bytes(nv, k))."""
    lib = _lib.load()
    nv, d = _rows(e_unit, "e_unit").shape
    _chk(nbr, torch.int32, "nbr")
    k = nbr.shape[1] if nbr.dim() == 2 else -1
    _flat_nk(nbr, torch.int32, nv, k, "nbr"), _flat_nk(w, torch.float32, nv, k, "w"), _flat_nk(dw, torch.float32, nv, k, "dw")
    _chk(tr_off, torch.int64, "tr_off"), _chk(tr_slot, torch.int32, "tr_slot")
    if tr_off.shape != (nv + 1,) or tr_slot.numel() != nv * k:
        raise ValueError(f"affinity_softmax_backward: expected tr_off [{nv + 1}] and tr_slot [{nv * k}], got {list(tr_off.shape)} / "
                         f"{list(tr_slot.shape)}")
    out = torch.empty((nv, d), dtype=torch.float32, device=e_unit.device) if out is None else _rows(out, "out", nv, d)
    ws = (_ws(lib.gp_affinity_softmax_backward_workspace_bytes(nv, int(k)), e_unit.device) if workspace is None
          else _chk(workspace, torch.uint8, "workspace"))
    check(lib.gp_affinity_softmax_backward(_ptr(e_unit), e_unit.stride(0), int(d), _ptr(nbr), _ptr(w), _ptr(dw), int(k), nv, float(sharpen),
                                           _ptr(tr_off), _ptr(tr_slot), _ptr(out), out.stride(0), _ptr(ws), ws.numel(), _stream()),
          "gp_affinity_softmax_backward")
    return out


def l2norm_rows_backward(e_raw, de_unit, out=None):
    """The backward of l2norm_rows_ (gp_l2norm_rows_backward): e_raw the rows before the normalisation, de_unit the gradient of the
    unit rows -> de_raw fp32 [n, d] (F.normalize's autograd, its 1e-12 clamp included)."""
    lib = _lib.load()
    n, d = _rows(e_raw, "e_raw").shape
    _rows(de_unit, "de_unit", n, d)
    out = torch.empty((n, d), dtype=torch.float32, device=e_raw.device) if out is None else _rows(out, "out", n, d)
    check(lib.gp_l2norm_rows_backward(_ptr(e_raw), e_raw.stride(0), _ptr(de_unit), de_unit.stride(0), int(d), n, _ptr(out), out.stride(0),
                                      _stream()), "gp_l2norm_rows_backward")
    return out


class PoolTiles:
    """Affinity operator re-blocked into tiles of r rows (built once per scene, applied many times)."""

    def __init__(self, tile_off, u_row, u_w, r, nv, total):
        self.tile_off, self.u_row, self.u_w, self.r, self.nv, self.total = tile_off, u_row, u_w, r, nv, total


def pool_tiles_build(nbr, w, r=16):
    """One host sync (total union entries, to size the tile arrays)."""
    lib = _lib.load()
    nv, k = nbr.shape
    dev = nbr.device
    nt = (nv + r - 1) // r
    ws = _ws(lib.gp_pool_tiles_workspace_bytes(nv, r), dev)
    off = torch.empty(nt + 1, dtype=torch.int64, device=dev)
    check(lib.gp_pool_tiles_count(_ptr(nbr), nv, int(k), int(r), _ptr(off), _ptr(ws), ws.numel(), _stream()),
          "gp_pool_tiles_count")
    total = int(off[nt].item())
    u_row = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    u_w = torch.empty((max(total, 1), r), dtype=torch.float32, device=dev)
    check(lib.gp_pool_tiles_fill(_ptr(nbr), _ptr(w), nv, int(k), int(r), _ptr(off), _ptr(u_row), _ptr(u_w), _stream()),
          "gp_pool_tiles_fill")
    return PoolTiles(off, u_row, u_w, r, nv, total)


def pool_tiles_apply(x, tiles, d, out):
    lib = _lib.load()
    check(lib.gp_pool_tiles_apply(_ptr(x), x.stride(0), _ptr(tiles.tile_off), _ptr(tiles.u_row), _ptr(tiles.u_w),
                                  int(tiles.r), tiles.nv, int(d), _ptr(out), out.stride(0), _stream()),
          "gp_pool_tiles_apply")
    return out


class PoolMfma:
    """Affinity operator in matrix-core form: per block of block_rows rows the padded neighbour union and the
    dense [block_rows x union] weight block, pre-split to f16 hi/lo in MFMA A-fragment order."""

    def __init__(self, bu_off, bu_n, bu_row, wa_hi, wa_lo, nv, total, block_rows, min_steps=0):
        self.bu_off, self.bu_n, self.bu_row, self.wa_hi, self.wa_lo = bu_off, bu_n, bu_row, wa_hi, wa_lo
        self.nv, self.total, self.block_rows, self.min_steps = nv, total, block_rows, min_steps
        self._queue = None

    @property
    def queue(self):
        """Tile counters of the persistent kernel (9 x uint32, zero between launches)."""
        if self._queue is None:
            self._queue = torch.zeros(16, dtype=torch.int32, device=self.bu_off.device)
        return self._queue

    @property
    def rows_padded(self):
        """Rows the persistent kernel's output buffers must hold (whole row blocks)."""
        return (self.nv + self.block_rows - 1) // self.block_rows * self.block_rows


def pool_mfma_build(nbr, w, block_rows=64, min_steps=0):
    """One host sync (total padded union rows, to size the arrays).  min_steps: pad every row block to at least this many
    32-row steps (9 for pool_mfma_apply_persistent, else 0)."""
    lib = _lib.load()
    nv, k = nbr.shape
    dev = nbr.device
    nb = (nv + block_rows - 1) // block_rows
    ws = _ws(lib.gp_pool_mfma_workspace_bytes(nv, block_rows), dev)
    bu_off = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    bu_n = torch.empty(nb, dtype=torch.int32, device=dev)
    check(lib.gp_pool_mfma_count(_ptr(nbr), nv, int(k), int(block_rows), int(min_steps), _ptr(bu_off), _ptr(bu_n), _ptr(ws),
                                 ws.numel(), _stream()), "gp_pool_mfma_count")
    total, min_rows = torch.stack([bu_off[nb], torch.diff(bu_off).min()]).cpu().tolist()     # the one host sync
    bu_row = torch.empty(total, dtype=torch.int32, device=dev)
    wa_hi = torch.empty(total // 32 * (block_rows // 16) * 64 * 8, dtype=torch.float16, device=dev)
    wa_lo = torch.empty_like(wa_hi)
    check(lib.gp_pool_mfma_fill(_ptr(nbr), _ptr(w), nv, int(k), int(block_rows), _ptr(bu_off), _ptr(bu_n), total,
                                _ptr(bu_row), _ptr(wa_hi), _ptr(wa_lo), _stream()), "gp_pool_mfma_fill")
    return PoolMfma(bu_off, bu_n, bu_row, wa_hi, wa_lo, nv, total, block_rows, min_steps=min_rows // 32)


def pool_mfma_apply(x_split, op, d, out_split=None, out_f32=None, out_scale=None):
    """x_split / out_split: (hi, lo) f16 [Nv, >=d] pairs; out_f32 fp32 [Nv, >=d]; at least one output.
    out_scale: device scalar multiplied into out_f32 (1/s of a pow2_scale()-scaled x_split)."""
    lib = _lib.load()
    xh, xl = x_split
    assert xh.stride(0) == xl.stride(0)
    yh, yl = out_split if out_split is not None else (None, None)
    check(lib.gp_pool_mfma_apply(_ptr(xh), _ptr(xl), xh.stride(0), _ptr(op.bu_off), _ptr(op.bu_row), _ptr(op.wa_hi),
                                 _ptr(op.wa_lo), op.nv, int(d), int(op.block_rows), _ptr(yh), _ptr(yl),
                                 yh.stride(0) if yh is not None else 0, _ptr(out_f32),
                                 out_f32.stride(0) if out_f32 is not None else 0, _ptr(out_scale), _stream()), "gp_pool_mfma_apply")
    return out_f32 if out_f32 is not None else out_split


class PoolCs:
    """Column-sliced matrix-core pooling operator (gp_pool_cs_*): blocks of up to 128 rows, fragment masks."""

    def __init__(self, bu_off, bu_n, bu_row, bu_mask, wa_hi, wa_lo, nv, total, block_rows=128):
        self.bu_off, self.bu_n, self.bu_row, self.bu_mask = bu_off, bu_n, bu_row, bu_mask
        self.wa_hi, self.wa_lo, self.nv, self.total = wa_hi, wa_lo, nv, total
        self.block_rows = block_rows
        self.dst = None            # i32 [nv, k]: fragment element of (row, neighbour) once the structure is built ahead
        self.max_union = 0         # largest block union (pass 1): sizes the LDS tables of the fill passes (0 = not known)
        self.valid = None          # u32 validity words once the structure is built for affinity_cs_fragments; k: its list length
        self.k = 0
        self.dep = self.flags = None   # the chained launch's dependency lists and flags (pool_cs_deps)
        self.epoch = 0
        self.filled = False        # the weights are in the fragments


def pool_cs_plan(nbr, rows_per_block=128, structure=False):
    """First half of the operator build: needs the neighbour lists only (not the weights), so a scheduler can run it -- and its
    one host sync (total padded union rows, to size the arrays) -- before the affinity weights exist.  Returns a PoolCs without
    weights; pool_cs_fill completes it.  rows_per_block: 16..128 (every height from 96 up measures within 4 % on the S scene,
    profiles/r04_pool_block_height.log; 128 is the default)."""
    lib = _lib.load()
    nv, k = nbr.shape
    dev = nbr.device
    rpb = int(rows_per_block)
    nb = (nv + rpb - 1) // rpb
    ws = _ws(lib.gp_pool_cs_workspace_bytes(nv, rpb), dev)
    bu_off = torch.empty(nb + 2, dtype=torch.int64, device=dev)[:nb + 1]                       # (+ one slot behind it: the largest union)
    bu_n = torch.empty(nb, dtype=torch.int32, device=dev)
    tail = bu_off.as_strided((2,), (1,), bu_off.storage_offset() + nb)                        # [total, largest union]: ONE read-back
    check(lib.gp_pool_cs_count(_ptr(nbr), nv, int(k), rpb, _ptr(bu_off), _ptr(bu_n), tail[1:].data_ptr(), _ptr(ws), ws.numel(), _stream()),
          "gp_pool_cs_count")
    total, max_union = (int(v) for v in readback(tail))                                       # the one host sync
    bu_row = torch.empty(total, dtype=torch.int32, device=dev)
    bu_mask = torch.empty(total // 32, dtype=torch.int32, device=dev)
    wa_hi = torch.empty(total // 32 * 8 * 512, dtype=torch.float16, device=dev)
    wa_lo = torch.empty_like(wa_hi)
    op = PoolCs(bu_off, bu_n, bu_row, bu_mask, wa_hi, wa_lo, nv, total, block_rows=rpb)
    op.max_union = max_union                                   # sizes the LDS tables of the fill passes
    if structure == "valid":
        # the structure for affinity_cs_fragments: validity bits instead of the dst table, no fragment zeroed (that kernel writes
        # every non-empty fragment whole)
        op.valid = torch.empty(total // 32 * 128 + 64, dtype=torch.int32, device=dev)
        check(lib.gp_pool_cs_structure_valid(_ptr(nbr), nv, int(k), rpb, _ptr(bu_off), total, max_union, _ptr(bu_row), _ptr(bu_mask),
                                             _ptr(op.valid), _stream()), "gp_pool_cs_structure_valid")
        op.k = int(k)
        return op
    if structure and total * 128 < 2 ** 31:
        # everything of the fill pass that needs the lists only, + where each (row, neighbour) weight goes: affinity_softmax(into=op)
        # then completes the operator
        op.dst = torch.empty((nv, k), dtype=torch.int32, device=dev)
        check(lib.gp_pool_cs_structure(_ptr(nbr), nv, int(k), rpb, _ptr(bu_off), total, max_union, _ptr(bu_row), _ptr(bu_mask), _ptr(wa_hi),
                                       _ptr(wa_lo), _ptr(op.dst), _stream()), "gp_pool_cs_structure")
    return op


def pool_cs_fill(op, nbr, w):
    """Second half: union rows, fragment masks and the weights in fragment order (no host sync)."""
    lib = _lib.load()
    nv, k = nbr.shape
    check(lib.gp_pool_cs_fill(_ptr(nbr), _ptr(w), nv, int(k), int(op.block_rows), _ptr(op.bu_off), op.total, int(op.max_union), _ptr(op.bu_row),
                              _ptr(op.bu_mask), _ptr(op.wa_hi), _ptr(op.wa_lo), _stream()), "gp_pool_cs_fill")
    op.filled = True
    return op


def pool_cs_build(nbr, w, rows_per_block=128):
    """pool_cs_plan + pool_cs_fill."""
    return pool_cs_fill(pool_cs_plan(nbr, rows_per_block), nbr, w)


def pool_cs_apply(x_split, op, d, out_split=None, out_f32=None, out_scale=None):
    """x_split / out_split: (hi, lo) f16 [Nv, >=d] pairs; out_f32 fp32 [Nv, >=d]; at least one output.  d: pool_cs_width_ok
    (256, 512, 768 or 1024).  out_scale: device scalar multiplied into out_f32 (1/s of a pow2_scale()-scaled x_split)."""
    lib = _lib.load()
    xh, xl = x_split
    assert xh.stride(0) == xl.stride(0)
    yh, yl = out_split if out_split is not None else (None, None)
    check(lib.gp_pool_cs_apply(_ptr(xh), _ptr(xl), xh.stride(0), _ptr(op.bu_off), _ptr(op.bu_row), _ptr(op.bu_mask), _ptr(op.wa_hi),
                               _ptr(op.wa_lo), op.nv, int(d), int(op.block_rows), _ptr(yh), _ptr(yl), yh.stride(0) if yh is not None else 0,
                               _ptr(out_f32), out_f32.stride(0) if out_f32 is not None else 0, _ptr(out_scale), _stream()),
          "gp_pool_cs_apply")
    return out_f32 if out_f32 is not None else out_split


def pool_cs_deps(op, d=512):
    """Dependency lists + flags of the chained launch (pool_cs_apply_chain) at width d; needs the operator's structure (bu_row) only."""
    lib = _lib.load()
    words = _pool_cs_flag_words(op, d)                     # (an unsupported width raises before anything is built)
    dev = op.bu_row.device
    nb = op.bu_off.numel() - 1
    op.dep = torch.empty(nb * 64, dtype=torch.int32, device=dev)
    scratch = torch.empty(nb, dtype=torch.int32, device=dev)
    check(lib.gp_pool_cs_deps(_ptr(op.bu_off), _ptr(op.bu_row), op.nv, int(op.block_rows), _ptr(op.dep), _ptr(scratch), _stream()),
          "gp_pool_cs_deps")
    op.flags = torch.zeros(words, dtype=torch.int32, device=dev)          # (a fresh array: the abort word cleared)
    op.epoch = 0
    return op


def _pool_cs_flag_words(op, d):
    """Words of the chained launch's flags array at width d: [32 header][d / 256 slices][nblocks]."""
    words = _lib.load().gp_pool_cs_chain_flag_words_d(op.nv, int(op.block_rows), int(d))
    if words == 0:
        raise ValueError(f"pool_cs: d={d} (the column-sliced kernels take d = 256, 512, 768 or 1024)")
    return words


def pool_cs_apply_chain(x_split, pong, op, d, applications, out_f32, out_scale=None):
    """All `applications` (>= 2) of the operator in ONE launch (gp_pool_cs_apply_chain): the same planes and bits as that many
    pool_cs_apply calls ping-ponging between x_split and pong; x_split is rewritten.  op.flags[0] != 0 afterwards (read at the
    caller's next synchronisation point: pool_cs_chain_check) means the launch gave up and the outputs are invalid."""
    lib = _lib.load()
    if getattr(op, "dep", None) is None:
        pool_cs_deps(op, d)
    elif op.flags is None or op.flags.numel() < _pool_cs_flag_words(op, d):      # flags sized for a narrower width: a fresh array
        op.flags = torch.zeros(_pool_cs_flag_words(op, d), dtype=torch.int32, device=op.bu_row.device)
        op.epoch = 0
    xh, xl = x_split
    ph, pl_ = pong
    assert xh.stride(0) == xl.stride(0) == ph.stride(0) == pl_.stride(0)
    check(lib.gp_pool_cs_apply_chain(_ptr(xh), _ptr(xl), _ptr(ph), _ptr(pl_), xh.stride(0), _ptr(op.bu_off), _ptr(op.bu_row),
                                     _ptr(op.bu_mask), _ptr(op.wa_hi), _ptr(op.wa_lo), op.nv, int(d), int(op.block_rows),
                                     int(applications), _ptr(out_f32), out_f32.stride(0), _ptr(out_scale), _ptr(op.dep), _ptr(op.flags),
                                     op.epoch & 0xFFFFFFFF, _stream()), "gp_pool_cs_apply_chain")
    op.epoch += int(applications)
    op.chain_done = torch.cuda.Event()                    # recorded on the LAUNCHING stream: pool_cs_chain_check waits for it
    op.chain_done.record(torch.cuda.current_stream(xh.device))
    return out_f32


def pool_cs_chain_check(op):
    """Host side of the chained launch's contract: wait for the op's last chained launch (the event recorded on the stream that
    launched it -- the caller may be on another stream) and raise if the abort word is set."""
    if getattr(op, "flags", None) is None:
        return
    ev = getattr(op, "chain_done", None)
    if ev is not None:
        ev.synchronize()
    if int(op.flags[0].item()) != 0:
        raise _lib.GeoPurifyHipError("gp_pool_cs_apply_chain: a workgroup waited 2 s for a dependency; the pooled features are invalid")


def pool_mfma_apply_persistent(x_split, op, d, out_split=None, out_f32=None, out_scale=None, dynamic=True):
    """Persistent matrix-core pooling (one workgroup per CU).  Outputs need op.rows_padded rows; exactly one output form.
    dynamic: workgroups claim tiles from op.queue (False: static tile lists, the slower tuning reference)."""
    lib = _lib.load()
    xh, xl = x_split
    assert xh.stride(0) == xl.stride(0)
    yh, yl = out_split if out_split is not None else (None, None)
    rows = (yh if yh is not None else out_f32).shape[0]
    check(lib.gp_pool_mfma_apply_persistent(_ptr(xh), _ptr(xl), xh.stride(0), _ptr(op.bu_off), _ptr(op.bu_row), _ptr(op.wa_hi),
                                            _ptr(op.wa_lo), op.nv, int(d), int(op.block_rows), int(op.min_steps), _ptr(yh), _ptr(yl),
                                            yh.stride(0) if yh is not None else 0, _ptr(out_f32),
                                            out_f32.stride(0) if out_f32 is not None else 0, int(rows), _ptr(out_scale),
                                            _ptr(op.queue) if dynamic else None, _stream()),
          "gp_pool_mfma_apply_persistent")
    return out_f32 if out_f32 is not None else out_split


# ------------------------------------------------------------------------------------------ rows 5-7
def lift_dense_accum(feat2d, pt, x, y, sum_, cnt):
    lib = _lib.load()
    d, H, W = feat2d.shape
    check(lib.gp_lift_dense_accum(_ptr(feat2d), d, H, W, _ptr(pt), _ptr(x), _ptr(y), pt.shape[0], _ptr(sum_),
                                  sum_.stride(0), _ptr(cnt), _stream()), "gp_lift_dense_accum")


def lift_dense_bilinear_accum(feat_lo, out_h, out_w, pt, x, y, sum_, cnt):
    """LSeg path: feat_lo fp32 [D,h,w]; (x, y) index the [out_h, out_w] image the reference resizes the map to."""
    lib = _lib.load()
    d, h, w = feat_lo.shape
    check(lib.gp_lift_dense_bilinear_accum(_ptr(feat_lo), d, h, w, int(out_h), int(out_w), _ptr(pt), _ptr(x), _ptr(y),
                                           pt.shape[0], _ptr(sum_), sum_.stride(0), _ptr(cnt), _stream()),
          "gp_lift_dense_bilinear_accum")


def lift_dense_finish(sum_, d, cnt):
    lib = _lib.load()
    n = sum_.shape[0]
    seen = torch.empty(n, dtype=torch.uint8, device=sum_.device)
    check(lib.gp_lift_dense_finish(_ptr(sum_), sum_.stride(0), int(d), _ptr(cnt), n, _ptr(seen), _stream()),
          "gp_lift_dense_finish")
    return seen


def lift_masks_view(pred_masks, scores, taps, out_hw, x, y, want_logit=False, workspace=None):
    """pred_masks fp32 [Q,h,w]; scores fp32 [Q]; taps = (x0 i32 [W], wx f32 [W,4], y0 i32 [H], wy f32 [H,4])."""
    lib = _lib.load()
    Q, h, w = pred_masks.shape
    n_v = x.shape[0]
    dev = pred_masks.device
    need = lib.gp_lift_masks_workspace_bytes(Q, h, w)
    if workspace is None or workspace.numel() < need:
        workspace = _ws(need, dev)
    seg = torch.empty(n_v, dtype=torch.int32, device=dev)
    lg = torch.empty(n_v, dtype=torch.float32, device=dev) if want_logit else None
    tx0, twx, ty0, twy = taps
    check(lib.gp_lift_masks_view(_ptr(pred_masks), Q, h, w, _ptr(scores), _ptr(tx0), _ptr(twx), _ptr(ty0), _ptr(twy),
                                 int(out_hw[0]), int(out_hw[1]), _ptr(x), _ptr(y), n_v, _ptr(seg), _ptr(lg),
                                 _ptr(workspace), workspace.numel(), _stream()), "gp_lift_masks_view")
    return (seg, lg) if want_logit else seg


def segment_tables(mask_embed, text_norm, logit_scale, f_seg, logit_seg):
    lib = _lib.load()
    Q, d = mask_embed.shape
    C = text_norm.shape[0]
    check(lib.gp_segment_tables(_ptr(mask_embed), Q, d, _ptr(text_norm), C, float(logit_scale), _ptr(f_seg),
                                _ptr(logit_seg), _stream()), "gp_segment_tables")


def pv_count(pt, cnt):
    lib = _lib.load()
    check(lib.gp_pv_count(_ptr(pt), pt.shape[0], _ptr(cnt), _stream()), "gp_pv_count")


def exclusive_scan_i64(x):
    lib = _lib.load()
    n = x.shape[0]
    out = torch.empty_like(x)
    ws = _ws(lib.gp_scan_workspace_bytes(n), x.device)
    check(lib.gp_exclusive_scan_i64(_ptr(x), n, _ptr(out), _ptr(ws), ws.numel(), _stream()), "gp_exclusive_scan_i64")
    return out


def pv_fill(pt, seg, view, pv_start, cursor, pv_view, pv_seg):
    lib = _lib.load()
    check(lib.gp_pv_fill(_ptr(pt), _ptr(seg), pt.shape[0], int(view), _ptr(pv_start), _ptr(cursor), _ptr(pv_view),
                         _ptr(pv_seg), _stream()), "gp_pv_fill")


def fuse_views_top3(pv_start, pv_view, pv_seg, n, f_seg, logit_seg, out):
    lib = _lib.load()
    V, Q, d = f_seg.shape
    C = logit_seg.shape[2]
    seen = torch.empty(n, dtype=torch.uint8, device=out.device)
    check(lib.gp_fuse_views_top3(_ptr(pv_start), _ptr(pv_view), _ptr(pv_seg), int(n), _ptr(f_seg), _ptr(logit_seg),
                                 Q, d, C, _ptr(out), out.stride(0), _ptr(seen), _stream()), "gp_fuse_views_top3")
    return seen


def seen_masks(pv_start, n):
    """(seen, unseen) u8 [n] from the list offsets: seen[p] = the point has a list (gp_seen_masks)"""
    lib = _lib.load()
    _chk(pv_start, torch.int64, "pv_start")
    seen = torch.empty(n, dtype=torch.uint8, device=pv_start.device)
    unseen = torch.empty(n, dtype=torch.uint8, device=pv_start.device)
    check(lib.gp_seen_masks(_ptr(pv_start), int(n), _ptr(seen), _ptr(unseen), _stream()), "gp_seen_masks")
    return seen, unseen


def fuse_views_top3_fill(pv_start, pv_view, pv_seg, n, f_seg, logit_seg, nn, out):
    """fuse_views_top3 with the scene-level fill inside: row p from the list of nn[p] where nn[p] >= 0 (gp_fuse_views_top3_fill)"""
    lib = _lib.load()
    V, Q, d = f_seg.shape
    C = logit_seg.shape[2]
    _chk(nn, torch.int64, "nn")
    check(lib.gp_fuse_views_top3_fill(_ptr(pv_start), _ptr(pv_view), _ptr(pv_seg), int(n), _ptr(f_seg), _ptr(logit_seg),
                                      Q, d, C, _ptr(nn), _ptr(out), out.stride(0), _stream()), "gp_fuse_views_top3_fill")
    return out


def nn1(ref_xyz, query_xyz):
    """Exact nearest reference index per query (fp32 coords, fp64 distances)."""
    lib = _lib.load()
    _chk(ref_xyz, torch.float32, "ref_xyz")
    _chk(query_xyz, torch.float32, "query_xyz")
    nr, nq = ref_xyz.shape[0], query_xyz.shape[0]
    nn = torch.empty(nq, dtype=torch.int64, device=ref_xyz.device)
    if nq == 0:
        return nn
    ws = _ws(lib.gp_nn1_workspace_bytes(nr, nq), ref_xyz.device)
    check(lib.gp_nn1_f64(_ptr(ref_xyz), nr, _ptr(query_xyz), nq, _ptr(nn), _ptr(ws), ws.numel(), _stream()), "gp_nn1_f64")
    return nn


def nn1_masked(xyz, ref_mask, query_mask, workspace=None):
    """nn[i] = nearest point with ref_mask among xyz for every i with query_mask, else -1.  No sync."""
    lib = _lib.load()
    _chk(xyz, torch.float32, "xyz")
    n = xyz.shape[0]
    nn = torch.empty(n, dtype=torch.int64, device=xyz.device)
    need = lib.gp_nn1_masked_workspace_bytes(n)
    if workspace is None or workspace.numel() < need:
        workspace = _ws(need, xyz.device)
    check(lib.gp_nn1_masked_f64(_ptr(xyz), n, _ptr(ref_mask), _ptr(query_mask), _ptr(nn), _ptr(workspace),
                                workspace.numel(), _stream()), "gp_nn1_masked_f64")
    return nn


def visible_lists(mapping, pt, x, y, count_dev, workspace=None):
    lib = _lib.load()
    n = mapping.shape[0]
    need = lib.gp_visible_lists_workspace_bytes(n)
    if workspace is None or workspace.numel() < need:
        workspace = _ws(need, mapping.device)
    check(lib.gp_visible_lists(_ptr(mapping), n, _ptr(pt), _ptr(x), _ptr(y), _ptr(count_dev), _ptr(workspace),
                               workspace.numel(), _stream()), "gp_visible_lists")


def views_visible_lists(coords, params, depth_all, width, height, cut_bound, vis_thres, min_visible, val_keep):
    """All views of a scene at once: coords f64 [N,3]; params f64 [V,20] (device) = world->camera (16) | fx fy cx cy;
    depth_all f64 [V,H,W] or None.  Returns the view-major entry arrays (sized V*N; view_off[V] = entries used)."""
    lib = _lib.load()
    _chk(coords, torch.float64, "coords")
    _chk(params, torch.float64, "params")
    n, nv = coords.shape[0], params.shape[0]
    dev = coords.device
    if depth_all is not None:
        _chk(depth_all, torch.float64, "depth_all")
        assert depth_all.shape == (nv, height, width)
    ent = {"pt": torch.empty(nv * n, dtype=torch.int64, device=dev), "x": torch.empty(nv * n, dtype=torch.int64, device=dev),
           "y": torch.empty(nv * n, dtype=torch.int64, device=dev), "view": torch.empty(nv * n, dtype=torch.int32, device=dev),
           "view_off": torch.empty(nv + 1, dtype=torch.int64, device=dev), "keep": torch.empty(nv, dtype=torch.uint8, device=dev)}
    ws = _ws(lib.gp_views_visible_lists_workspace_bytes(n, nv), dev)
    check(lib.gp_views_visible_lists(_ptr(coords), n, _ptr(params), _ptr(depth_all), nv, int(width), int(height), int(cut_bound),
                                     float(vis_thres), int(min_visible), int(val_keep), _ptr(ent["pt"]), _ptr(ent["x"]), _ptr(ent["y"]),
                                     _ptr(ent["view"]), _ptr(ent["view_off"]), _ptr(ent["keep"]), _ptr(ws), ws.numel(), _stream()),
          "gp_views_visible_lists")
    return ent


def lift_masks_views(pred_masks, scores, taps, out_hw, xyz, ent, total, nviews, fill_cap=None):
    """Rows 6-7 up to the point -> (view, segment) lists for all views at once.  pred_masks f32 [Vsrc,Q,h,w], scores f32
    [Vsrc,Q], xyz f32 [N,3], ent = views_visible_lists(...), total = entries used.  Returns (seg, pv_start, pv_view, pv_seg).
    fill_cap: capacity of the in-view fill's partial arrays in fill queries (None: a quarter of the entries, at least 65 536 --
    the uncovered share of the visible pixels is a few per cent on every scene measured; more queries than that are still
    answered, by the kernel's overflow path)."""
    lib = _lib.load()
    _chk(pred_masks, torch.float32, "pred_masks")
    _chk(scores, torch.float32, "scores")
    _chk(xyz, torch.float32, "xyz")
    nsrc, Q, h, w = pred_masks.shape
    n = xyz.shape[0]
    dev = xyz.device
    seg = torch.empty(total, dtype=torch.int32, device=dev)
    start = torch.empty(n + 1, dtype=torch.int64, device=dev)
    pvv = torch.empty(total, dtype=torch.int32, device=dev)
    pvs = torch.empty(total, dtype=torch.int32, device=dev)
    if fill_cap is None:
        fill_cap = min(int(total), max(int(total) // 4, 65536))
    ws = _ws(lib.gp_lift_masks_views_workspace_bytes(nsrc, Q, h, w, total, n, int(fill_cap)), dev)
    tx0, twx, ty0, twy = taps
    check(lib.gp_lift_masks_views(_ptr(pred_masks), nsrc, Q, h, w, _ptr(scores), _ptr(tx0), _ptr(twx), _ptr(ty0), _ptr(twy),
                                  int(out_hw[0]), int(out_hw[1]), _ptr(xyz), n, _ptr(ent["pt"]), _ptr(ent["x"]), _ptr(ent["y"]),
                                  _ptr(ent["view"]), _ptr(ent["view_off"]), _ptr(ent["keep"]), int(nviews), int(total), int(fill_cap), _ptr(seg),
                                  _ptr(start), _ptr(pvv), _ptr(pvs), _ptr(ws), ws.numel(), _stream()), "gp_lift_masks_views")
    return seg, start, pvv, pvs


# ------------------------------------------------------------------------------------------ row 13
def classify_argmax(feat, text_norm, logit_scale, d=None):
    lib = _lib.load()
    n = feat.shape[0]
    d = feat.shape[1] if d is None else d
    C = text_norm.shape[0]
    pred = torch.empty(n, dtype=torch.int64, device=feat.device)
    zero = torch.empty(n, dtype=torch.uint8, device=feat.device)
    check(lib.gp_classify_argmax(_ptr(feat), feat.stride(0), int(d), n, _ptr(text_norm), C, float(logit_scale),
                                 _ptr(pred), _ptr(zero), _stream()), "gp_classify_argmax")
    return pred, zero


def classify_argmax_gemm(feat, text_norm, d=None):
    """Same decision as classify_argmax (arg-max_c <f/|f|, t_c> = arg-max_c <f, t_c>) with the logits from
    the exact-fp32 MFMA GEMM kernel -- for large class counts (Matterport-160 / ScanNet200)."""
    lib = _lib.load()
    n = feat.shape[0]
    d = feat.shape[1] if d is None else d
    C = text_norm.shape[0]
    cpad = (C + 127) // 128 * 128
    w = torch.zeros((d, cpad), dtype=torch.float32, device=feat.device)
    w[:, :C] = text_norm.t()
    logits = sparse_conv(feat, None, w)
    pred = torch.empty(n, dtype=torch.int64, device=feat.device)
    zero = torch.empty(n, dtype=torch.uint8, device=feat.device)
    check(lib.gp_rows_argmax(_ptr(logits), logits.stride(0), C, n, _ptr(feat), feat.stride(0), int(d), _ptr(pred),
                             _ptr(zero), _stream()), "gp_rows_argmax")
    return pred, zero


def iou_hist(pred, target, num_classes, ignore_ids, counts):
    lib = _lib.load()
    ig = (ctypes.c_int64 * max(len(ignore_ids), 1))(*[int(v) for v in ignore_ids])
    check(lib.gp_iou_hist_i64(_ptr(pred), _ptr(target), pred.shape[0], int(num_classes), ig, len(ignore_ids),
                              _ptr(counts), _stream()), "gp_iou_hist_i64")
    return counts


def nn1_batched(keys_sorted, ids, ref_mask, query_mask, axes=7, nn=None, status=None, workspace=None):
    """Masked exact 1-NN inside every batch entry (gp_nn1_batched): keys_sorted (u64 held in an i64 [nv]) and ids = perm (i32 [nv], or
    None: the row number) as coords_order_batched returns them, ref_mask / query_mask u8 [nv] in SORTED-row order, axes the mask of
    the axes that count (bit 0 = x, 1 = y, 2 = z) -> (nn i32 [nv]: for a query the SORTED row of the reference of its own entry with the
    smallest (d^2, id), -1 for other rows and for queries whose entry has no reference; status i32 [4] = (queries, references, queries
    left at -1, mask of the axes with a decoded coordinate of 32768 or more: nn undefined)), both on the device, no sync.
    nn / status / workspace: optional caller-owned contiguous buffers (the workspace uint8 of at least
    gp_nn1_batched_workspace_bytes(nv))."""
    lib = _lib.load()
    _chk(keys_sorted, torch.int64, "keys")
    nv = keys_sorted.shape[0]
    if keys_sorted.dim() != 1:
        raise ValueError(f"nn1_batched: expected keys [nv], got {list(keys_sorted.shape)}")
    for t, dtype, name in ((ids, torch.int32, "ids"), (ref_mask, torch.uint8, "ref_mask"), (query_mask, torch.uint8, "query_mask")):
        if t is not None and _chk(t, dtype, name).shape != (nv,):
            raise ValueError(f"nn1_batched: expected {name} [{nv}], got {list(t.shape)}")
    dev = keys_sorted.device
    if nn is None:
        nn = torch.empty(nv, dtype=torch.int32, device=dev)
    elif _chk(nn, torch.int32, "nn").shape != (nv,):
        raise ValueError(f"nn1_batched: expected nn [{nv}], got {list(nn.shape)}")
    if status is None:
        status = torch.empty(4, dtype=torch.int32, device=dev)
    elif _chk(status, torch.int32, "status").shape != (4,):
        raise ValueError(f"nn1_batched: expected status [4], got {list(status.shape)}")
    ws = _ws(lib.gp_nn1_batched_workspace_bytes(nv), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_nn1_batched(_ptr(keys_sorted), _ptr(ids), _ptr(ref_mask), _ptr(query_mask), nv, int(axes), _ptr(nn), _ptr(status),
                             _ptr(ws), ws.numel(), _stream()), "gp_nn1_batched")
    return nn, status


def iou_hist_batched(pred, coords, target, num_batches, num_classes, ignore_ids, counts, index=None):
    """counts i64 [B,3,C] += the (intersection, output, target) histograms of iou_hist, separated by batch entry
    (gp_iou_hist_batched_i64): pred i64 [rows] per voxel row, coords i32 [rows,4] for the batch index, target i64 [n]; index i64 [n]
    (a quantiser's inverse_mapping) makes item p use row index[p]; None is the identity with n = rows.  No sync."""
    lib = _lib.load()
    _chk(pred, torch.int64, "pred")
    _chk(coords, torch.int32, "coords")
    _chk(target, torch.int64, "target")
    _chk(counts, torch.int64, "counts")
    rows, n = pred.shape[0], target.shape[0]
    if pred.dim() != 1 or coords.shape != (rows, 4) or target.dim() != 1:
        raise ValueError(f"iou_hist_batched: expected pred [rows], coords [rows, 4], target [n], got {list(pred.shape)}, "
                         f"{list(coords.shape)}, {list(target.shape)}")
    if index is not None and _chk(index, torch.int64, "index").shape != (n,):
        raise ValueError(f"iou_hist_batched: expected index [{n}], got {list(index.shape)}")
    if counts.numel() != int(num_batches) * 3 * int(num_classes):
        raise ValueError(f"iou_hist_batched: expected counts [{num_batches}, 3, {num_classes}], got {list(counts.shape)}")
    ig = (ctypes.c_int64 * max(len(ignore_ids), 1))(*[int(v) for v in ignore_ids])
    check(lib.gp_iou_hist_batched_i64(_ptr(pred), _ptr(coords), rows, _ptr(target), _ptr(index), n, int(num_batches), int(num_classes),
                                      ig, len(ignore_ids), _ptr(counts), _stream()), "gp_iou_hist_batched_i64")
    return counts


# ------------------------------------------------------------------------------------------ cross-entropy of rows against text embeddings
SEGMENT_LOSS_MAX_ENTRIES = 65536                            # entry_cnt / entry_w of gp_segment_loss_items
SEGMENT_LOSS_REDUCTIONS = {"item": 0, "entry": 1}


def sparse_conv_tiles():
    """(row tile, column tile -- cout is a multiple of it --, channel step -- cin is a multiple of it --) of gp_sparse_conv, asked of
    the library (gp_sparse_conv_tiles): what a caller pads its operands to, and where the tests put their edge cases"""
    t = (ctypes.c_int32 * 3)()
    check(_lib.load().gp_sparse_conv_tiles(t), "gp_sparse_conv_tiles")
    return tuple(int(v) for v in t)


def segment_loss_col_step():
    """columns per lane step of the row kernels of gp_segment_loss_* (asked of the library)"""
    return int(_lib.load().gp_segment_loss_col_step())


def segment_loss_unit_rows(y, d=None, u=None, zero=None):
    """(u fp32 [n, d_pad] = the unit rows of y fp32 [n, >= d] (y / max(|y|, 1e-12), zero columns d .. d_pad-1), zero u8 [n] =
    (sum |y_i| == 0)) (gp_segment_loss_unit_rows).  u: optional caller-owned rows, their width is d_pad; default d padded to the GEMM's
    channel step."""
    lib = _lib.load()
    n = _rows(y, "y").shape[0]
    d = y.shape[1] if d is None else int(d)
    if u is None:
        kp = sparse_conv_tiles()[2]
        u = torch.empty((n, (d + kp - 1) // kp * kp), dtype=torch.float32, device=y.device)
    _rows(u, "u", n)
    zero = torch.empty(n, dtype=torch.uint8, device=y.device) if zero is None else _chk(zero, torch.uint8, "zero")
    if zero.shape != (n,):
        raise ValueError(f"segment_loss_unit_rows: expected zero [{n}], got {list(zero.shape)}")
    check(lib.gp_segment_loss_unit_rows(_ptr(y), y.stride(0), d, n, _ptr(u), u.stride(0), u.shape[1], _ptr(zero), _stream()),
          "gp_segment_loss_unit_rows")
    return u, zero


class SegmentLossItems:
    """The valid items of gp_segment_loss_items: row_valid u8 [n] (per-voxel labels) or item_off i64 [n+1] + item_id i32 [p] (per-point
    labels), entry_cnt i64 [65536], entry_w fp32 [65536], status i64 [4] = (bad batch rows, bad index items, top batch, V)."""

    def __init__(self, row_valid, item_off, item_id, entry_cnt, entry_w, status):
        self.row_valid, self.item_off, self.item_id = row_valid, item_off, item_id
        self.entry_cnt, self.entry_w, self.status = entry_cnt, entry_w, status


def segment_loss_items(coords, zero, labels, num_classes, ignore_ids, reduction, index=None, buffers=None, workspace=None):
    """gp_segment_loss_items: coords i32 [n,4], zero u8 [n], labels i64 [p], index i64 [p] or None (p == n) -> SegmentLossItems, no
    sync.  buffers: optional dict of caller-owned outputs by attribute name; workspace: uint8 of at least
    gp_segment_loss_items_workspace_bytes(n, p) (only read with an index)."""
    lib = _lib.load()
    _chk(coords, torch.int32, "coords"), _chk(zero, torch.uint8, "zero"), _chk(labels, torch.int64, "labels")
    n, p = zero.shape[0], labels.shape[0]
    if coords.shape != (n, 4) or zero.dim() != 1 or labels.dim() != 1:
        raise ValueError(f"segment_loss_items: expected coords [n, 4], zero [n], labels [p], got {list(coords.shape)}, {list(zero.shape)}, "
                         f"{list(labels.shape)}")
    if index is not None and _chk(index, torch.int64, "index").shape != (p,):
        raise ValueError(f"segment_loss_items: expected index [{p}], got {list(index.shape)}")
    if index is None and p != n:
        raise ValueError(f"segment_loss_items: {p} labels for {n} rows and no index")
    dev, B = coords.device, SEGMENT_LOSS_MAX_ENTRIES
    want = {"entry_cnt": (torch.int64, (B,)), "entry_w": (torch.float32, (B,)), "status": (torch.int64, (4,))}
    want.update({"row_valid": (torch.uint8, (n,))} if index is None else {"item_off": (torch.int64, (n + 1,)), "item_id": (torch.int32, (p,))})
    got = {}
    for name, (dtype, shape) in want.items():
        t = (buffers or {}).get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        elif _chk(t, dtype, name).shape != shape:
            raise ValueError(f"segment_loss_items: expected {name} {list(shape)}, got {list(t.shape)}")
        got[name] = t
    ws = None
    if index is not None:
        ws = _ws(lib.gp_segment_loss_items_workspace_bytes(n, p), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    ig = (ctypes.c_int64 * max(len(ignore_ids), 1))(*[int(v) for v in ignore_ids])
    check(lib.gp_segment_loss_items(_ptr(coords), _ptr(zero), n, _ptr(labels), _ptr(index), p, int(num_classes), ig, len(ignore_ids),
                                    SEGMENT_LOSS_REDUCTIONS[reduction], _ptr(got.get("row_valid")), _ptr(got.get("item_off")),
                                    _ptr(got.get("item_id")), _ptr(got["entry_cnt"]), _ptr(got["entry_w"]), _ptr(got["status"]),
                                    _ptr(ws), ws.numel() if ws is not None else 0, _stream()), "gp_segment_loss_items")
    return SegmentLossItems(got.get("row_valid"), got.get("item_off"), got.get("item_id"), got["entry_cnt"], got["entry_w"], got["status"])


def segment_loss_rows(z, num_classes, coords, items, labels, row0, g, lse, term):
    """The row kernel (gp_segment_loss_rows) over the chunk of rows row0 .. row0 + r - 1: z fp32 [r, >= c] the chunk's logits, g fp32
    [r, c_pad] (its width is c_pad) the chunk's own, or None: lse and term alone (the forward); coords i32 [n,4], lse fp32 [n], term
    f64 [n] and the items the whole arrays."""
    lib = _lib.load()
    r = _rows(z, "z").shape[0]
    if g is not None:
        _rows(g, "g", r)
    _chk(coords, torch.int32, "coords"), _chk(labels, torch.int64, "labels"), _chk(lse, torch.float32, "lse"), _chk(term, torch.float64, "term")
    n = coords.shape[0]
    if not 0 <= row0 <= n - r or lse.shape != (n,) or term.shape != (n,):
        raise ValueError(f"segment_loss_rows: rows {row0} .. {row0 + r - 1} of {n}, lse {list(lse.shape)}, term {list(term.shape)}")
    per_row = items.item_off is None
    c_pad, ld_g = (g.shape[1], g.stride(0)) if g is not None else (int(num_classes), 0)
    check(lib.gp_segment_loss_rows(_ptr(z), z.stride(0), r, int(num_classes), c_pad, _ptr(coords[row0:]),
                                   _ptr(items.row_valid[row0:]) if per_row else None, None if per_row else _ptr(items.item_off[row0:]),
                                   None if per_row else _ptr(items.item_id), _ptr(labels[row0:]) if per_row else _ptr(labels),
                                   _ptr(items.entry_w), _ptr(g), ld_g, _ptr(lse[row0:]), _ptr(term[row0:]), _stream()),
          "gp_segment_loss_rows")
    return g


def segment_loss_reduce(term, coords, entry_cnt, num_entries, reduction, loss=None, per_entry=None, workspace=None):
    """(loss fp32 0-d, per_entry fp32 [num_entries]) from the rows' terms f64 [n] in a fixed order (gp_segment_loss_reduce)."""
    lib = _lib.load()
    _chk(term, torch.float64, "term"), _chk(coords, torch.int32, "coords"), _chk(entry_cnt, torch.int64, "entry_cnt")
    n, dev = term.shape[0], term.device
    if coords.shape != (n, 4) or entry_cnt.shape[0] < num_entries:
        raise ValueError(f"segment_loss_reduce: expected coords [{n}, 4] and at least {num_entries} entry counts, got {list(coords.shape)}, "
                         f"{list(entry_cnt.shape)}")
    loss = torch.empty((), dtype=torch.float32, device=dev) if loss is None else _chk(loss, torch.float32, "loss")
    per_entry = torch.empty(num_entries, dtype=torch.float32, device=dev) if per_entry is None else _chk(per_entry, torch.float32, "per_entry")
    if per_entry.shape != (num_entries,):
        raise ValueError(f"segment_loss_reduce: expected per_entry [{num_entries}], got {list(per_entry.shape)}")
    ws = _ws(lib.gp_segment_loss_reduce_workspace_bytes(n, int(num_entries)), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_segment_loss_reduce(_ptr(term), _ptr(coords), n, _ptr(entry_cnt), int(num_entries), SEGMENT_LOSS_REDUCTIONS[reduction],
                                     _ptr(loss), _ptr(per_entry), _ptr(ws), ws.numel(), _stream()), "gp_segment_loss_reduce")
    return loss, per_entry


# ------------------------------------------------------------------------------------------ the lift over batched point clouds
# the element types the batched lifts read maps and mask logits in, by the tag of the *_t entry points
ELEM_TAG = {torch.float32: _lib.GP_ELEM_F32, torch.float16: _lib.GP_ELEM_F16, torch.bfloat16: _lib.GP_ELEM_BF16}


def _chk_elem(t, name):
    """a contiguous CUDA tensor of fp32, fp16 or bf16 -> its element-type tag"""
    if t.dtype not in ELEM_TAG or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous CUDA torch.float32, torch.float16 or torch.bfloat16, got {t.dtype} cuda={t.is_cuda} "
                         f"contig={t.is_contiguous()}")
    return ELEM_TAG[t.dtype]


def _chk_points(who, points):
    """points f64 [n >= 1, 4], contiguous on the GPU -> (n, their device)"""
    _chk(points, torch.float64, "points")
    if points.dim() != 2 or points.shape[1] != 4 or points.shape[0] < 1:
        raise ValueError(f"{who}: expected points [n >= 1, 4], got {list(points.shape)}")
    return points.shape[0], points.device


def _chk_views(who, nv, view_entry, w2c, intrinsics, depth=None, image_hw=None):
    """the arrays of nv views as every batched lift, vote and render takes them: view_entry i64 [nv], w2c f64 [nv,4,4], intrinsics f64
    [nv,4] and, where the caller has one, depth f64 [nv,H,W] with image_hw = (H, W); all contiguous on the GPU"""
    _chk(view_entry, torch.int64, "view_entry"), _chk(w2c, torch.float64, "w2c"), _chk(intrinsics, torch.float64, "intrinsics")
    if view_entry.shape != (nv,) or w2c.shape != (nv, 4, 4) or intrinsics.shape != (nv, 4):
        raise ValueError(f"{who}: expected view_entry [{nv}], w2c [{nv}, 4, 4], intrinsics [{nv}, 4], got {list(view_entry.shape)}, "
                         f"{list(w2c.shape)}, {list(intrinsics.shape)}")
    if depth is not None and _chk(depth, torch.float64, "depth").shape != (nv, int(image_hw[0]), int(image_hw[1])):
        raise ValueError(f"{who}: expected depth [{nv}, {image_hw[0]}, {image_hw[1]}], got {list(depth.shape)}")


def lift_batched_col_chunk():
    """channels one pass of gp_lift_batched's lift kernel holds in registers (asked of the library)"""
    return int(_lib.load().gp_lift_batched_col_chunk())


def lift_batched_transpose(maps, out=None):
    """maps fp32, fp16 or bf16 [V, D, h, w] contiguous (NCHW) -> the pixel-major copy [V, h*w, D] of the same dtype that gp_lift_batched
    reads (gp_lift_batched_transpose_t: the elements are moved, not converted)"""
    lib = _lib.load()
    elem = _chk_elem(maps, "maps")
    if maps.dim() != 4:
        raise ValueError(f"lift_batched_transpose: expected maps [V, D, h, w], got {list(maps.shape)}")
    v, d, h, w = maps.shape
    if out is None:
        out = torch.empty((v, h * w, d), dtype=maps.dtype, device=maps.device)
    elif _chk(out, maps.dtype, "out").shape != (v, h * w, d):
        raise ValueError(f"lift_batched_transpose: expected out [{v}, {h * w}, {d}], got {list(out.shape)}")
    check(lib.gp_lift_batched_transpose_t(_ptr(maps), elem, v, d, h * w, _ptr(out), _stream()), "gp_lift_batched_transpose")
    return out


class LiftBatched:
    """What gp_lift_batched writes: out fp32 [n, D] (before the fill), seen u8 [n], count i32 [n], view_count i64 [V], view_keep u8 [V],
    nn i64 [n] or None (the seen row an unseen row takes, -1 elsewhere), status i64 [8] = (bad batch rows, bad view entries, non-finite
    rows, top batch, seen rows, filled rows, 0, 0)."""

    def __init__(self, out, seen, count, view_count, view_keep, nn, status):
        self.out, self.seen, self.count, self.view_count, self.view_keep, self.nn, self.status = out, seen, count, view_count, view_keep, nn, status


def lift_batched(points, maps_pm, map_hw, view_entry, w2c, intrinsics, depth, image_hw, bilinear, cut_bound, vis_thres, min_visible,
                 max_visible, fill=True, buffers=None, workspace=None):
    """gp_lift_batched_t, no sync: points f64 [n,4]; maps_pm fp32, fp16 or bf16 [V, h*w, D] pixel-major (read in place, the sums and the
    rows are fp32 whatever the maps' dtype) with map_hw = (h, w); view_entry i64 [V]; w2c f64
    [V,4,4]; intrinsics f64 [V,4]; depth f64 [V,H,W] or None; image_hw = (H, W).  -> LiftBatched.  buffers: optional dict of
    caller-owned outputs by attribute name (out: fp32 rows of any pitch); workspace: uint8 of at least
    gp_lift_batched_workspace_bytes(n, V)."""
    lib = _lib.load()
    who = "lift_batched"
    _chk(points, torch.float64, "points")
    elem = _chk_elem(maps_pm, "maps_pm")
    (h, w), (H, W) = map_hw, image_hw
    n, dev = points.shape[0], points.device
    if points.dim() != 2 or points.shape[1] != 4 or maps_pm.dim() != 3 or maps_pm.shape[1] != h * w:
        raise ValueError(f"{who}: expected points [n, 4] and maps_pm [V, {h * w}, D], got {list(points.shape)}, {list(maps_pm.shape)}")
    nv, _, d = maps_pm.shape
    _chk_views(who, nv, view_entry, w2c, intrinsics, depth, image_hw)
    want = {"seen": (torch.uint8, (n,)), "count": (torch.int32, (n,)), "view_count": (torch.int64, (nv,)), "view_keep": (torch.uint8, (nv,)),
            "status": (torch.int64, (8,))}
    if fill:
        want["nn"] = (torch.int64, (n,))
    got = _outputs(who, want, buffers, dev)
    out = (buffers or {}).get("out")
    out = torch.empty((n, d), dtype=torch.float32, device=dev) if out is None else _rows(out, "out", n, d)
    need = lib.gp_lift_batched_workspace_bytes(n, nv)
    ws = _ws(need, dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_batched_t(_ptr(points), n, _ptr(maps_pm), elem, d, int(h), int(w), _ptr(view_entry), _ptr(w2c), _ptr(intrinsics),
                                _ptr(depth), nv, int(H), int(W), 1 if bilinear else 0, int(cut_bound), float(vis_thres), int(min_visible),
                                int(max_visible), 1 if fill else 0, _ptr(out), out.stride(0), _ptr(got["seen"]), _ptr(got["count"]),
                                _ptr(got["view_count"]), _ptr(got["view_keep"]), _ptr(got.get("nn")), _ptr(got["status"]), _ptr(ws), ws.numel(),
                                _stream()), "gp_lift_batched")
    return LiftBatched(out, got["seen"], got["count"], got["view_count"], got["view_keep"], got.get("nn"), got["status"])


# ------------------------------------------------------------------------------------------ the same lift, the views in chunks
class LiftStreamState:
    """What a resumable lift keeps between its calls, all of it the caller's: points f64 [n,4], state u8 (the entry tables, written by
    gp_lift_stream_begin alone), sums fp32 [n, D] rows of any pitch, count i32 [n], status i64 [8] (the running words: bad batch rows,
    bad view entries so far, non-finite rows, top batch)."""

    def __init__(self, points, state, sums, count, status):
        self.points, self.state, self.sums, self.count, self.status = points, state, sums, count, status


def lift_stream_begin(points, d, buffers=None, workspace=None):
    """gp_lift_stream_begin, no sync: points f64 [n,4] -> LiftStreamState for rows of d channels (sums +0, counts 0).  buffers: optional
    dict of caller-owned state / sums / count / status (state: uint8 of at least gp_lift_stream_state_bytes(n); sums: fp32 rows of any
    pitch); workspace: uint8 of at least gp_lift_stream_begin_workspace_bytes(n)."""
    lib = _lib.load()
    (n, dev), d = _chk_points("lift_stream_begin", points), int(d)
    if d < 1:
        raise ValueError(f"lift_stream_begin: expected d >= 1, got d={d}")
    got = _outputs("lift_stream_begin", {"count": (torch.int32, (n,)), "status": (torch.int64, (8,))}, buffers, dev)
    state = (buffers or {}).get("state")
    state = _ws(lib.gp_lift_stream_state_bytes(n), dev) if state is None else _chk(state, torch.uint8, "state")
    sums = (buffers or {}).get("sums")
    sums = torch.empty((n, d), dtype=torch.float32, device=dev) if sums is None else _rows(sums, "sums", n, d)
    ws = _ws(lib.gp_lift_stream_begin_workspace_bytes(n), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_stream_begin(_ptr(points), n, d, _ptr(state), state.numel(), _ptr(sums), sums.stride(0), _ptr(got["count"]),
                                   _ptr(got["status"]), _ptr(ws), ws.numel(), _stream()), "gp_lift_stream_begin")
    return LiftStreamState(points, state, sums, got["count"], got["status"])


def lift_stream_add_workspace_bytes(num_views):
    return int(_lib.load().gp_lift_stream_add_workspace_bytes(int(num_views)))


def lift_stream_finish_workspace_bytes(n):
    return int(_lib.load().gp_lift_stream_finish_workspace_bytes(int(n)))


def lift_stream_add(st, maps_pm, map_hw, view_entry, w2c, intrinsics, depth, image_hw, bilinear, cut_bound, vis_thres, min_visible, max_visible,
                    buffers=None, workspace=None):
    """gp_lift_stream_add_t, no sync: one chunk of views onto the LiftStreamState st; the chunk's arrays as ops.lift_batched takes them
    (maps_pm fp32, fp16 or bf16 [V, h*w, D] pixel-major; the chunks of one stream may differ in dtype).  -> (view_count i64 [V], view_keep u8 [V]) of the chunk.  buffers: optional dict of
    caller-owned view_count / view_keep; workspace: uint8 of at least gp_lift_stream_add_workspace_bytes(V)."""
    lib = _lib.load()
    who = "lift_stream_add"
    elem = _chk_elem(maps_pm, "maps_pm")
    (h, w), (H, W) = map_hw, image_hw
    n, d, dev = st.points.shape[0], st.sums.shape[1], st.points.device
    if maps_pm.dim() != 3 or maps_pm.shape[1] != h * w or maps_pm.shape[2] != d:
        raise ValueError(f"{who}: expected maps_pm [V, {h * w}, {d}], got {list(maps_pm.shape)}")
    nv = maps_pm.shape[0]
    _chk_views(who, nv, view_entry, w2c, intrinsics, depth, image_hw)
    got = _outputs(who, {"view_count": (torch.int64, (nv,)), "view_keep": (torch.uint8, (nv,))}, buffers, dev)
    ws = _ws(lib.gp_lift_stream_add_workspace_bytes(nv), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_stream_add_t(_ptr(st.points), n, _ptr(st.state), st.state.numel(), _ptr(maps_pm), elem, d, int(h), int(w), _ptr(view_entry),
                                   _ptr(w2c), _ptr(intrinsics), _ptr(depth), nv, int(H), int(W), 1 if bilinear else 0, int(cut_bound),
                                   float(vis_thres), int(min_visible), int(max_visible), _ptr(st.sums), st.sums.stride(0), _ptr(st.count),
                                   _ptr(got["view_count"]), _ptr(got["view_keep"]), _ptr(st.status), _ptr(ws), ws.numel(), _stream()),
          "gp_lift_stream_add")
    return got["view_count"], got["view_keep"]


class LiftStreamFinish:
    """What gp_lift_stream_finish writes: out fp32 [n, D] (before the fill), seen u8 [n], nn i64 [n] or None, status i64 [8] = (bad batch
    rows, bad view entries, non-finite rows, top batch, seen rows, filled rows, values of the state outside their range, 0)."""

    def __init__(self, out, seen, nn, status):
        self.out, self.seen, self.nn, self.status = out, seen, nn, status


def lift_stream_finish(st, fill=True, buffers=None, workspace=None):
    """gp_lift_stream_finish, no sync: the LiftStreamState st as it stands -> LiftStreamFinish; st is not changed.  buffers: optional
    dict of caller-owned out (fp32 rows of any pitch) / seen / nn / status; workspace: uint8 of at least
    gp_lift_stream_finish_workspace_bytes(n)."""
    lib = _lib.load()
    n, d, dev = st.points.shape[0], st.sums.shape[1], st.points.device
    want = {"seen": (torch.uint8, (n,)), "status": (torch.int64, (8,))}
    if fill:
        want["nn"] = (torch.int64, (n,))
    got = _outputs("lift_stream_finish", want, buffers, dev)
    out = (buffers or {}).get("out")
    out = torch.empty((n, d), dtype=torch.float32, device=dev) if out is None else _rows(out, "out", n, d)
    ws = _ws(lib.gp_lift_stream_finish_workspace_bytes(n), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_stream_finish(_ptr(st.points), n, _ptr(st.state), st.state.numel(), _ptr(st.sums), d, st.sums.stride(0), _ptr(st.count),
                                    _ptr(st.status), 1 if fill else 0, _ptr(out), out.stride(0), _ptr(got["seen"]), _ptr(got.get("nn")),
                                    _ptr(got["status"]), _ptr(ws), ws.numel(), _stream()), "gp_lift_stream_finish")
    return LiftStreamFinish(out, got["seen"], got.get("nn"), got["status"])


# ------------------------------------------------------------------------------------------ the label vote over batched point clouds
# the element types the label votes read label maps in, by the tag of gp_lift_labels_batched
LABEL_TAG = {torch.uint8: _lib.GP_LABEL_U8, torch.int16: _lib.GP_LABEL_I16, torch.int32: _lib.GP_LABEL_I32, torch.int64: _lib.GP_LABEL_I64}
LIFT_LABELS_MAX_CLASSES = 1024                              # gp_lift_labels_batched: the histogram is a wave's LDS slice
LIFT_LABELS_MAX_IGNORE = 16


def _chk_labels(t, name):
    """a contiguous CUDA tensor of uint8, int16, int32 or int64 -> its element-type tag"""
    if t.dtype not in LABEL_TAG or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous CUDA torch.uint8, torch.int16, torch.int32 or torch.int64, got {t.dtype} cuda={t.is_cuda} "
                         f"contig={t.is_contiguous()}")
    return LABEL_TAG[t.dtype]


def _ignore_ids(who, ignore_ids):
    ids = [int(v) for v in ignore_ids]
    if len(ids) > LIFT_LABELS_MAX_IGNORE or any(not -2 ** 63 <= v < 2 ** 63 for v in ids):
        raise ValueError(f"{who}: at most {LIFT_LABELS_MAX_IGNORE} ignore labels, each a 64-bit integer, got {ids}")
    return (ctypes.c_int64 * max(len(ids), 1))(*ids), len(ids)


def _label_views(who, labels2d, view_entry, w2c, intrinsics, depth):
    """the views' arrays of a label vote, checked -> (elem, V, H, W)"""
    elem = _chk_labels(labels2d, "labels2d")
    if labels2d.dim() != 3 or min(labels2d.shape) < 1:
        raise ValueError(f"{who}: expected labels2d [V, H, W], got {list(labels2d.shape)}")
    nv, H, W = labels2d.shape
    _chk_views(who, nv, view_entry, w2c, intrinsics, depth, (H, W))
    return elem, nv, H, W


def lift_labels_batched_workspace_bytes(n, num_views):
    return int(_lib.load().gp_lift_labels_batched_workspace_bytes(int(n), int(num_views)))


class LiftLabelsBatched:
    """What gp_lift_labels_batched writes: labels i64 [n] (after the fill), votes i32 [n, C], voted i32 [n], seen u8 [n], count i32 [n],
    view_count i64 [V], view_keep u8 [V], status i64 [8] = (bad batch rows, bad view entries, non-finite rows, top batch, voted rows,
    filled rows, 0, sampled labels out of range)."""

    def __init__(self, labels, votes, voted, seen, count, view_count, view_keep, status):
        self.labels, self.votes, self.voted, self.seen, self.count = labels, votes, voted, seen, count
        self.view_count, self.view_keep, self.status = view_count, view_keep, status


def lift_labels_batched(points, labels2d, num_classes, view_entry, w2c, intrinsics, depth, cut_bound, vis_thres, min_visible, max_visible,
                        ignore_ids=(255,), unlabeled=255, fill=True, buffers=None, workspace=None):
    """gp_lift_labels_batched, no sync: points f64 [n,4]; labels2d uint8, int16, int32 or int64 [V,H,W] (read in place); view_entry i64 [V];
    w2c f64 [V,4,4]; intrinsics f64 [V,4]; depth f64 [V,H,W] or None.  -> LiftLabelsBatched.  buffers: optional dict of caller-owned
    outputs by attribute name (votes: int32 rows of any pitch); workspace: uint8 of at least gp_lift_labels_batched_workspace_bytes(n, V)."""
    lib = _lib.load()
    who = "lift_labels_batched"
    (n, dev), C = _chk_points(who, points), int(num_classes)
    elem, nv, H, W = _label_views(who, labels2d, view_entry, w2c, intrinsics, depth)
    if not 1 <= C <= LIFT_LABELS_MAX_CLASSES:
        raise ValueError(f"{who}: num_classes={num_classes} outside 1..{LIFT_LABELS_MAX_CLASSES}")
    ids, n_ids = _ignore_ids(who, ignore_ids)
    got = _outputs(who, {"labels": (torch.int64, (n,)), "voted": (torch.int32, (n,)), "seen": (torch.uint8, (n,)), "count": (torch.int32, (n,)),
                         "view_count": (torch.int64, (nv,)), "view_keep": (torch.uint8, (nv,)), "status": (torch.int64, (8,))}, buffers, dev)
    votes = (buffers or {}).get("votes")
    votes = torch.empty((n, C), dtype=torch.int32, device=dev) if votes is None else _rows_i32(votes, "votes", n, C)
    ws = _ws(lib.gp_lift_labels_batched_workspace_bytes(n, nv), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_labels_batched(_ptr(points), n, _ptr(labels2d), elem, C, _ptr(view_entry), _ptr(w2c), _ptr(intrinsics), _ptr(depth), nv, H, W,
                                     int(cut_bound), float(vis_thres), int(min_visible), int(max_visible), ids, n_ids, int(unlabeled),
                                     1 if fill else 0, _ptr(got["labels"]), _ptr(votes), votes.stride(0), _ptr(got["voted"]), _ptr(got["seen"]),
                                     _ptr(got["count"]), _ptr(got["view_count"]), _ptr(got["view_keep"]), _ptr(got["status"]), _ptr(ws), ws.numel(),
                                     _stream()), "gp_lift_labels_batched")
    return LiftLabelsBatched(got["labels"], votes, got["voted"], got["seen"], got["count"], got["view_count"], got["view_keep"], got["status"])


def _rows_i32(t, name, n, d):
    """caller-owned int32 rows [n, d] of any pitch (unit column stride)"""
    if t.dtype != torch.int32 or not t.is_cuda or t.dim() != 2 or t.shape != (n, d) or t.stride(1) != 1 or (n > 1 and t.stride(0) < d):
        raise ValueError(f"{name}: expected CUDA int32 rows [{n}, {d}] with unit column stride, got {t.dtype} {list(t.shape)} strides {t.stride()}")
    return t


class LiftLabelsStreamState:
    """What a resumable label vote keeps between its calls, all of it the caller's: points f64 [n,4], state u8 (the entry tables, written
    by gp_lift_labels_stream_begin alone; ops.render_depth_stream reads them too), votes i32 [n, C] rows of any pitch, count i32 [n],
    status i64 [8] (the running words: bad batch rows, bad view entries so far, non-finite rows, top batch, ..., labels out of range so
    far)."""

    def __init__(self, points, state, votes, count, status):
        self.points, self.state, self.votes, self.count, self.status = points, state, votes, count, status


def lift_labels_stream_state_bytes(n):
    return int(_lib.load().gp_lift_labels_stream_state_bytes(int(n)))


def lift_labels_stream_begin_workspace_bytes(n):
    return int(_lib.load().gp_lift_labels_stream_begin_workspace_bytes(int(n)))


def lift_labels_stream_add_workspace_bytes(num_views):
    return int(_lib.load().gp_lift_labels_stream_add_workspace_bytes(int(num_views)))


def lift_labels_stream_finish_workspace_bytes(n):
    return int(_lib.load().gp_lift_labels_stream_finish_workspace_bytes(int(n)))


def lift_labels_stream_begin(points, num_classes, buffers=None, workspace=None):
    """gp_lift_labels_stream_begin, no sync: points f64 [n,4] -> LiftLabelsStreamState for num_classes classes (votes 0, counts 0).
    buffers: optional dict of caller-owned state / votes / count / status (state: uint8 of at least
    gp_lift_labels_stream_state_bytes(n); votes: int32 rows of any pitch); workspace: uint8 of at least
    gp_lift_labels_stream_begin_workspace_bytes(n)."""
    lib = _lib.load()
    who = "lift_labels_stream_begin"
    (n, dev), C = _chk_points(who, points), int(num_classes)
    if not 1 <= C <= LIFT_LABELS_MAX_CLASSES:
        raise ValueError(f"{who}: num_classes={num_classes} outside 1..{LIFT_LABELS_MAX_CLASSES}")
    got = _outputs(who, {"count": (torch.int32, (n,)), "status": (torch.int64, (8,))}, buffers, dev)
    state = (buffers or {}).get("state")
    state = _ws(lib.gp_lift_labels_stream_state_bytes(n), dev) if state is None else _chk(state, torch.uint8, "state")
    votes = (buffers or {}).get("votes")
    votes = torch.empty((n, C), dtype=torch.int32, device=dev) if votes is None else _rows_i32(votes, "votes", n, C)
    ws = _ws(lib.gp_lift_labels_stream_begin_workspace_bytes(n), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_labels_stream_begin(_ptr(points), n, C, _ptr(state), state.numel(), _ptr(votes), votes.stride(0), _ptr(got["count"]),
                                          _ptr(got["status"]), _ptr(ws), ws.numel(), _stream()), "gp_lift_labels_stream_begin")
    return LiftLabelsStreamState(points, state, votes, got["count"], got["status"])


def lift_labels_stream_add(st, labels2d, view_entry, w2c, intrinsics, depth, cut_bound, vis_thres, min_visible, max_visible, ignore_ids=(255,),
                           buffers=None, workspace=None):
    """gp_lift_labels_stream_add, no sync: one chunk of views onto the LiftLabelsStreamState st; the chunk's arrays as
    ops.lift_labels_batched takes them (the chunks of one stream may differ in dtype).  -> (view_count i64 [V], view_keep u8 [V]) of the
    chunk.  buffers: optional dict of caller-owned view_count / view_keep; workspace: uint8 of at least
    gp_lift_labels_stream_add_workspace_bytes(V)."""
    lib = _lib.load()
    who = "lift_labels_stream_add"
    n, C, dev = st.points.shape[0], st.votes.shape[1], st.points.device
    elem, nv, H, W = _label_views(who, labels2d, view_entry, w2c, intrinsics, depth)
    ids, n_ids = _ignore_ids(who, ignore_ids)
    got = _outputs(who, {"view_count": (torch.int64, (nv,)), "view_keep": (torch.uint8, (nv,))}, buffers, dev)
    ws = _ws(lib.gp_lift_labels_stream_add_workspace_bytes(nv), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_labels_stream_add(_ptr(st.points), n, _ptr(st.state), st.state.numel(), _ptr(labels2d), elem, C, _ptr(view_entry), _ptr(w2c),
                                        _ptr(intrinsics), _ptr(depth), nv, H, W, int(cut_bound), float(vis_thres), int(min_visible),
                                        int(max_visible), ids, n_ids, _ptr(st.votes), st.votes.stride(0), _ptr(st.count), _ptr(got["view_count"]),
                                        _ptr(got["view_keep"]), _ptr(st.status), _ptr(ws), ws.numel(), _stream()), "gp_lift_labels_stream_add")
    return got["view_count"], got["view_keep"]


class LiftLabelsStreamFinish:
    """What gp_lift_labels_stream_finish writes: labels i64 [n] (after the fill), voted i32 [n], seen u8 [n], status i64 [8] = (bad batch
    rows, bad view entries, non-finite rows, top batch, voted rows, filled rows, values of the state outside their range, sampled labels
    out of range)."""

    def __init__(self, labels, voted, seen, status):
        self.labels, self.voted, self.seen, self.status = labels, voted, seen, status


def lift_labels_stream_finish(st, unlabeled=255, fill=True, buffers=None, workspace=None):
    """gp_lift_labels_stream_finish, no sync: the LiftLabelsStreamState st as it stands -> LiftLabelsStreamFinish; st is not changed.
    buffers: optional dict of caller-owned labels / voted / seen / status; workspace: uint8 of at least
    gp_lift_labels_stream_finish_workspace_bytes(n)."""
    lib = _lib.load()
    who = "lift_labels_stream_finish"
    n, C, dev = st.points.shape[0], st.votes.shape[1], st.points.device
    got = _outputs(who, {"labels": (torch.int64, (n,)), "voted": (torch.int32, (n,)), "seen": (torch.uint8, (n,)), "status": (torch.int64, (8,))},
                   buffers, dev)
    ws = _ws(lib.gp_lift_labels_stream_finish_workspace_bytes(n), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_labels_stream_finish(_ptr(st.points), n, _ptr(st.state), st.state.numel(), _ptr(st.votes), C, st.votes.stride(0),
                                           _ptr(st.count), _ptr(st.status), int(unlabeled), 1 if fill else 0, _ptr(got["labels"]),
                                           _ptr(got["voted"]), _ptr(got["seen"]), _ptr(got["status"]), _ptr(ws), ws.numel(), _stream()),
          "gp_lift_labels_stream_finish")
    return LiftLabelsStreamFinish(got["labels"], got["voted"], got["seen"], got["status"])


# ------------------------------------------------------------------------------------------ rendered depth over batched point clouds
def _render_views(who, view_entry, w2c, intrinsics, image_hw, cut_bound, depth, dev):
    """the views' arrays of a rendered-depth call, checked -> (V, H, W, depth f64 [V,H,W])"""
    H, W = (int(v) for v in image_hw)
    if view_entry.dim() != 1 or view_entry.shape[0] < 1:
        raise ValueError(f"{who}: expected view_entry [V >= 1], got {list(view_entry.shape)}")
    nv = view_entry.shape[0]
    if H < 1 or W < 1 or int(cut_bound) < 0:
        raise ValueError(f"{who}: expected image_hw = (H, W) >= 1 and cut_bound >= 0, got {tuple(image_hw)}, {cut_bound}")
    _chk_views(who, nv, view_entry, w2c, intrinsics, depth, (H, W))
    if depth is None:
        depth = torch.empty((nv, H, W), dtype=torch.float64, device=dev)
    return nv, H, W, depth


def render_depth_batched_workspace_bytes(n, num_views):
    return int(_lib.load().gp_render_depth_batched_workspace_bytes(int(n), int(num_views)))


def render_depth_batched(points, view_entry, w2c, intrinsics, image_hw, cut_bound, depth=None, workspace=None, status=None):
    """gp_render_depth_batched, no sync: the z-buffer of every view over the points of its entry (the ScanNet mapper with depth given as
    a str, fusion_util.py:126-130).  points f64 [n,4]; view_entry i64 [V]; w2c f64 [V,4,4]; intrinsics f64 [V,4]; image_hw = (H, W).
    -> (depth f64 [V,H,W], status i64 [8] = (bad batch rows, bad view entries, non-finite rows, top batch, 0, 0, 0, 0)).  depth / status:
    optional caller-owned outputs; workspace: uint8 of at least gp_render_depth_batched_workspace_bytes(n, V)."""
    lib = _lib.load()
    who = "render_depth_batched"
    n, dev = _chk_points(who, points)
    nv, H, W, depth = _render_views(who, view_entry, w2c, intrinsics, image_hw, cut_bound, depth, dev)
    status = _outputs(who, {"status": (torch.int64, (8,))}, {"status": status}, dev)["status"]
    ws = _ws(lib.gp_render_depth_batched_workspace_bytes(n, nv), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_render_depth_batched(_ptr(points), n, _ptr(view_entry), _ptr(w2c), _ptr(intrinsics), nv, H, W, int(cut_bound), _ptr(depth),
                                      _ptr(status), _ptr(ws), ws.numel(), _stream()), "gp_render_depth_batched")
    return depth, status


def render_depth_stream_workspace_bytes(n, num_views):
    return int(_lib.load().gp_render_depth_batched_state_workspace_bytes(int(n), int(num_views)))


def render_depth_stream(st, view_entry, w2c, intrinsics, image_hw, cut_bound, depth=None, workspace=None, status=None):
    """gp_render_depth_batched_state, no sync: render_depth_batched with the entry tables taken from a stream's state -- st a
    LiftStreamState or a LiftMasksStreamState (its points and state; nothing of st is changed) -- so nothing is sorted.  -> (depth f64
    [V,H,W], status i64 [8] = (0, bad view entries, 0, 0, 0, 0, values of the state outside their range, 0)).  workspace: uint8 of at
    least gp_render_depth_batched_state_workspace_bytes(n, V)."""
    lib = _lib.load()
    who = "render_depth_stream"
    points, state = st.points, _chk(st.state, torch.uint8, "state")
    n, dev = _chk_points(who, points)
    nv, H, W, depth = _render_views(who, view_entry, w2c, intrinsics, image_hw, cut_bound, depth, dev)
    status = _outputs(who, {"status": (torch.int64, (8,))}, {"status": status}, dev)["status"]
    ws = _ws(lib.gp_render_depth_batched_state_workspace_bytes(n, nv), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_render_depth_batched_state(_ptr(points), n, _ptr(state), state.numel(), _ptr(view_entry), _ptr(w2c), _ptr(intrinsics), nv, H, W,
                                            int(cut_bound), _ptr(depth), _ptr(status), _ptr(ws), ws.numel(), _stream()),
          "gp_render_depth_batched_state")
    return depth, status


# ------------------------------------------------------------------------------------------ lifted clouds rendered back into their views
RENDER_ROWS_DEPTH = {"none": 0, "maps": 1, "render": 2}      # gp_render_rows' depth_mode
RENDER_ROWS_MAX_RADIUS = 4


def render_rows_workspace_bytes(n, num_views, image_hw, depth_mode):
    """gp_render_rows_workspace_bytes (no GPU needed): depth_mode "none", "maps" or "render" (the rendered maps live in the workspace)"""
    H, W = (int(v) for v in image_hw)
    return int(_lib.load().gp_render_rows_workspace_bytes(int(n), int(num_views), H, W, RENDER_ROWS_DEPTH[depth_mode]))


class RenderRows:
    """What gp_render_rows writes: rows i32 [V,H,W] (-1: no owner), depth f64 [V,H,W] (the owner's p_z, 999999 without one), view_count
    i64 [V], pixel_count i64 [V], status i64 [8] = (bad batch rows, bad view entries, non-finite rows, top batch, 0, 0, 0, 0)."""

    def __init__(self, rows, depth, view_count, pixel_count, status):
        self.rows, self.depth, self.view_count, self.pixel_count, self.status = rows, depth, view_count, pixel_count, status


def render_rows(points, view_entry, w2c, intrinsics, image_hw, cut_bound, depth=None, vis_thres=0.25, radius=0, buffers=None, workspace=None):
    """gp_render_rows, no sync: per view and pixel the row of the front-most candidate of the view's entry (visualization.py:34-48 with
    the nearest point instead of the last; the mapping of fusion_util.py:99-147).  points f64 [n,4]; view_entry i64 [V]; w2c f64
    [V,4,4]; intrinsics f64 [V,4]; image_hw = (H, W); depth: None (p_z > 0), f64 [V,H,W], or "render" (gp_render_depth_batched's maps,
    made in the workspace); 0 <= radius <= 4.  -> RenderRows(rows i32 [V,H,W] (-1: no owner), depth f64 [V,H,W] (the owner's p_z,
    999999 without one), view_count i64 [V], pixel_count i64 [V], status i64 [8] = (bad batch rows, bad view entries, non-finite rows,
    top batch, 0, 0, 0, 0)).  buffers: optional dict of caller-owned rows / depth / view_count / pixel_count / status; workspace: uint8
    of at least gp_render_rows_workspace_bytes(n, V, H, W, mode)."""
    lib = _lib.load()
    who = "render_rows"
    n, dev = _chk_points(who, points)
    nv, H, W, zmin = _render_views(who, view_entry, w2c, intrinsics, image_hw, cut_bound, (buffers or {}).get("depth"), dev)
    buffers = dict(buffers or {}, depth=zmin)
    if isinstance(depth, str):
        if depth != "render":
            raise ValueError(f"{who}: depth={depth!r}: expected None, f64 [{nv}, {H}, {W}] or 'render'")
        mode, maps = "render", None
    elif depth is None:
        mode, maps = "none", None
    else:
        mode, maps = "maps", _chk(depth, torch.float64, "depth")
        if maps.shape != (nv, H, W):
            raise ValueError(f"{who}: expected depth [{nv}, {H}, {W}], got {list(maps.shape)}")
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= RENDER_ROWS_MAX_RADIUS:
        raise ValueError(f"{who}: radius={radius!r} must be an integer in 0..{RENDER_ROWS_MAX_RADIUS}")
    got = _outputs(who, {"rows": (torch.int32, (nv, H, W)), "depth": (torch.float64, (nv, H, W)), "view_count": (torch.int64, (nv,)),
                         "pixel_count": (torch.int64, (nv,)), "status": (torch.int64, (8,))}, buffers, dev)
    need = lib.gp_render_rows_workspace_bytes(n, nv, H, W, RENDER_ROWS_DEPTH[mode])
    ws = _ws(need, dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_render_rows(_ptr(points), n, _ptr(view_entry), _ptr(w2c), _ptr(intrinsics), nv, H, W, int(cut_bound), RENDER_ROWS_DEPTH[mode],
                             _ptr(maps), float(vis_thres), radius, _ptr(got["rows"]), _ptr(got["depth"]), _ptr(got["view_count"]),
                             _ptr(got["pixel_count"]), _ptr(got["status"]), _ptr(ws), ws.numel(), _stream()), "gp_render_rows")
    return RenderRows(got["rows"], got["depth"], got["view_count"], got["pixel_count"], got["status"])


def render_gather(rows, src, index=None, dtype=torch.float32, out=None):
    """gp_render_gather, no sync: out[p] = src[index[rows[p]]] (src[rows[p]] without index) converted once to dtype, a zero row where
    rows[p] < 0 (and where an index leaves its array).  rows i32 of any shape, contiguous (npix elements); src fp32 [R, D] with unit
    column stride and any row stride >= D (read in place, no copy); index i64 [n] or None; dtype fp32, fp16 or bf16.  -> out
    [*rows.shape, D], or the caller's out [npix, D] of that dtype with unit column stride and any row stride >= D."""
    lib = _lib.load()
    who = "render_gather"
    _chk(rows, torch.int32, "rows")
    if dtype not in ELEM_TAG:
        raise ValueError(f"{who}: dtype={dtype} must be torch.float32, torch.float16 or torch.bfloat16")
    if src.dtype != torch.float32 or not src.is_cuda or src.dim() != 2 or min(src.shape) < 1 or src.stride(1) != 1 or src.stride(0) < src.shape[1]:
        raise ValueError(f"{who}: src must be CUDA fp32 [R >= 1, D >= 1] with unit column stride and a row stride >= D, got "
                         f"{src.dtype} {list(src.shape)} strides {src.stride() if src.dim() == 2 else None}")
    npix, (R, D) = rows.numel(), src.shape
    if npix < 1:
        raise ValueError(f"{who}: rows is empty")
    if index is not None and _chk(index, torch.int64, "index").dim() != 1:
        raise ValueError(f"{who}: expected index [n], got {list(index.shape)}")
    if out is None:
        out = torch.empty((npix, D), dtype=dtype, device=src.device)
        shaped = out.view(*rows.shape, D)
    else:
        if out.dtype != dtype or not out.is_cuda or out.shape != (npix, D) or out.stride(1) != 1 or out.stride(0) < D:
            raise ValueError(f"{who}: out must be CUDA {dtype} [{npix}, {D}] with unit column stride and a row stride >= {D}, got "
                             f"{out.dtype} {list(out.shape)}")
        shaped = out
    check(lib.gp_render_gather(_ptr(rows), npix, _ptr(index), 0 if index is None else index.shape[0], _ptr(src), R, D, src.stride(0),
                               _ptr(out), ELEM_TAG[dtype], out.stride(0), _stream()), "gp_render_gather")
    return shaped


# ------------------------------------------------------------------------------------------ geometry channels: normals
KNN_NORMALS_MIN_K = 3


def mesh_normals_workspace_bytes(n, num_faces, dtype=torch.float64):
    """gp_mesh_normals_batched_workspace_bytes (no GPU needed)"""
    return int(_lib.load().gp_mesh_normals_batched_workspace_bytes(int(n), int(num_faces), 1 if dtype == torch.float64 else 0))


def mesh_normals_batched(points, faces, buffers=None, workspace=None):
    """gp_mesh_normals_batched, no sync: the reference's vertex_normal (models/utils/mapping_util.py:9-29) for the meshes of several
    entries at once, bit for bit, in the dtype of the points.  points f32 or f64 [n,4] = batch, x, y, z; faces i64 [F,3] of rows of
    points, any order.  -> (normals [n,3] of the points' dtype, status i64 [8] = (bad batch rows, 0, non-finite rows, top batch, 0, 0,
    faces with an index outside 0..n-1, faces whose rows are not of one entry)).  buffers: optional dict of caller-owned normals /
    status; workspace: uint8 of at least mesh_normals_workspace_bytes(n, F, dtype)."""
    lib = _lib.load()
    who = "mesh_normals_batched"
    if points.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{who}: points must be torch.float32 or torch.float64, got {points.dtype}")
    _chk(points, points.dtype, "points"), _chk(faces, torch.int64, "faces")
    if points.dim() != 2 or points.shape[1] != 4 or points.shape[0] < 1:
        raise ValueError(f"{who}: expected points [n >= 1, 4], got {list(points.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError(f"{who}: expected faces [F >= 1, 3], got {list(faces.shape)}")
    n, nf, dev, fp64 = points.shape[0], faces.shape[0], points.device, 1 if points.dtype == torch.float64 else 0
    got = _outputs(who, {"normals": (points.dtype, (n, 3)), "status": (torch.int64, (8,))}, buffers, dev)
    need = lib.gp_mesh_normals_batched_workspace_bytes(n, nf, fp64)
    if need == 0:
        raise ValueError(f"{who}: {n} points / {nf} faces outside what the library takes")
    ws = _ws(need, dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_mesh_normals_batched(_ptr(points), fp64, n, _ptr(faces), nf, _ptr(got["normals"]), _ptr(got["status"]), _ptr(ws), ws.numel(),
                                      _stream()), "gp_mesh_normals_batched")
    return got["normals"], got["status"]


def knn_normals(positions, neighbors, toward=None, toward_rows=None, buffers=None):
    """gp_knn_normals, no sync: for every row the direction of least spread of the row and its k listed rows -- the unit eigenvector of
    the smallest eigenvalue l0 of C = sum (p - m)(p - m)^T, all in fp64 in list order -- and variation = l0 / (l0 + l1 + l2); what
    stands in for the mesh normals of models/utils/mapping_util.py:19-29 where a cloud has no faces.  positions f32 or f64 [n, >= 3]
    with unit column stride and any row stride (columns 0..2 are read in place: a column slice of a wider tensor is no copy);
    neighbors i32 or i64 [n,k], 3 <= k <= 127.  Sign: with toward (floating [m,3]) and toward_rows (integer [n]) the vector of row i is
    flipped where <n, toward[toward_rows[i]] - p_i> < 0 (left at exactly 0); without them its component of largest magnitude is made
    positive, the lowest axis among equal magnitudes.  -> (normals f32 [n,3], variation f32 [n]).  A row with a list index outside
    0..n-1 or a toward_rows outside 0..m-1 is returned as zeros (nothing is dereferenced) and counted in status i64 [2] = (rows with
    a bad list index, rows with a bad toward row), which a caller reads from buffers["status"].  buffers: optional dict of
    caller-owned normals / variation / status."""
    lib = _lib.load()
    who = "knn_normals"
    P, Nb = positions, neighbors
    if not torch.is_tensor(P) or P.dtype not in (torch.float32, torch.float64) or not P.is_cuda or P.dim() != 2 or P.shape[0] < 1 or P.shape[1] < 3 \
            or P.stride(1) != 1 or P.stride(0) < 3:
        raise ValueError(f"{who}: positions must be CUDA fp32 or fp64 [n >= 1, >= 3] with unit column stride and a row stride >= 3, got "
                         f"{(P.dtype, list(P.shape), P.stride()) if torch.is_tensor(P) else type(P).__name__}")
    n, dev = P.shape[0], P.device
    if n >= 2 ** 31:
        raise ValueError(f"{who}: {n} rows outside 1..2^31-1")
    if not torch.is_tensor(Nb) or Nb.dtype not in (torch.int32, torch.int64) or Nb.dim() != 2 or Nb.shape[0] != n:
        raise ValueError(f"{who}: neighbors must be i32 or i64 [{n}, k], got {(Nb.dtype, list(Nb.shape)) if torch.is_tensor(Nb) else type(Nb).__name__}")
    _chk(Nb, Nb.dtype, f"{who}: neighbors")
    k = Nb.shape[1]
    if not KNN_NORMALS_MIN_K <= k <= _lib.GP_KNN_MAX_K:
        raise ValueError(f"{who}: k={k} outside {KNN_NORMALS_MIN_K}..{_lib.GP_KNN_MAX_K}")
    if (toward is None) != (toward_rows is None):
        raise ValueError(f"{who}: toward and toward_rows go together")
    m = 0
    if toward is not None:
        if not torch.is_tensor(toward) or not toward.dtype.is_floating_point or toward.dim() != 2 or toward.shape[1] != 3 or toward.shape[0] < 1:
            raise ValueError(f"{who}: toward must be floating point [m >= 1, 3], got "
                             f"{(toward.dtype, list(toward.shape)) if torch.is_tensor(toward) else type(toward).__name__}")
        if not torch.is_tensor(toward_rows) or toward_rows.dtype.is_floating_point or toward_rows.dtype == torch.bool or toward_rows.shape != (n,):
            raise ValueError(f"{who}: toward_rows must be an integer tensor [{n}], got "
                             f"{(toward_rows.dtype, list(toward_rows.shape)) if torch.is_tensor(toward_rows) else type(toward_rows).__name__}")
        toward = toward.detach().to(torch.float64).contiguous()
        toward_rows = toward_rows.detach().to(torch.int64).contiguous()
        m = toward.shape[0]
    if any(t.device != dev for t in (Nb, toward, toward_rows) if t is not None):
        raise ValueError(f"{who}: positions, neighbors, toward and toward_rows must be on one device")
    got = _outputs(who, {"normals": (torch.float32, (n, 3)), "variation": (torch.float32, (n,)), "status": (torch.int64, (2,))}, buffers, dev)
    check(lib.gp_knn_normals(_ptr(P), 1 if P.dtype == torch.float64 else 0, P.stride(0), n, _ptr(Nb), 1 if Nb.dtype == torch.int64 else 0, k,
                             _ptr(toward), m, _ptr(toward_rows), _ptr(got["normals"]), _ptr(got["variation"]), _ptr(got["status"]), _stream()),
          "gp_knn_normals")
    return got["normals"], got["variation"]


# ------------------------------------------------------------------------------------------ results carried to another cloud
KNN_QUERY_STATUS_WORDS = 16
KNN_INTERPOLATE_MODES = {"inverse_distance": 0, "nearest": 1}     # gp_knn_interpolate's mode


def knn_query_workspace_bytes(n, m):
    """gp_knn_query_workspace_bytes (no GPU needed): a function of the two row counts alone"""
    return int(_lib.load().gp_knn_query_workspace_bytes(int(n), int(m)))


def knn_query(points, queries, k, buffers=None, workspace=None):
    """gp_knn_query, no sync: for every row of queries the k nearest rows of points inside the query's own batch entry, exactly (the
    role of the KDTree queries of models/affinity_module.py:445-447, 693-697, for k neighbours, a second cloud and all entries at
    once).  points f64 [n,4] and queries f64 [m,4] = batch, x, y, z; 1 <= k <= 32.  xyz rounded to fp32 first, d^2 = (dx*dx + dy*dy) +
    dz*dz in fp64, a list ascending in (d^2, row).  -> (indices i64 [m,k] of rows of points, dist2 f64 [m,k], status i64 [16]); slots
    past the entry's count hold -1 / +inf.  status: [0] / [2] rows of points with a batch index that is no integer in 0..65535 / with
    a value that is not finite, [3] the points' top batch index, [8] / [10] the same two counts for the queries, [9] queries whose
    entry has no points, [11] queries that took the entry scan, [12..15] queries that stopped after shell 0..3 of the grid walk.
    buffers: optional dict of caller-owned indices / dist2 / status; workspace: uint8 of at least knn_query_workspace_bytes(n, m)."""
    lib = _lib.load()
    who = "knn_query"
    n, dev = _chk_points(who, points)
    _chk(queries, torch.float64, "queries")
    if queries.dim() != 2 or queries.shape[1] != 4 or queries.shape[0] < 1:
        raise ValueError(f"{who}: expected queries [m >= 1, 4], got {list(queries.shape)}")
    m = queries.shape[0]
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.GP_KNN_QUERY_MAX_K:
        raise ValueError(f"{who}: k={k!r} outside 1..{_lib.GP_KNN_QUERY_MAX_K}")
    if queries.device != dev:
        raise ValueError(f"{who}: points and queries must be on one device")
    got = _outputs(who, {"indices": (torch.int64, (m, k)), "dist2": (torch.float64, (m, k)), "status": (torch.int64, (KNN_QUERY_STATUS_WORDS,))},
                   buffers, dev)
    need = lib.gp_knn_query_workspace_bytes(n, m)
    if need == 0:
        raise ValueError(f"{who}: {n} points / {m} queries outside what the library takes (1..2^31-1 each)")
    ws = _ws(need, dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_knn_query(_ptr(points), n, _ptr(queries), m, k, _ptr(got["indices"]), _ptr(got["dist2"]), _ptr(got["status"]), _ptr(ws),
                           ws.numel(), _stream()), "gp_knn_query")
    return got["indices"], got["dist2"], got["status"]


def knn_interpolate(values, indices, dist2, index=None, mode="inverse_distance", eps=1e-8, unlabeled=255, buffers=None):
    """gp_knn_interpolate / gp_knn_interpolate_labels, no sync: rows of values carried through the lists of knn_query.  indices i64
    [m,k], dist2 f64 [m,k]; index i64 [n] (point -> row of values) or None (the lists name rows of values).
    Floating values [R,D] (fp32, fp16 or bf16, unit column stride, any row stride >= D, read in place) -> out f32 [m,D]: mode
    "inverse_distance": w_j = 1 / (d^2_j + eps) in fp64 over the slots that are not -1, normalised in fp64 and rounded to fp32 (slots
    with d^2_j + eps == 0 share the weight alone), out = sum_j w_j v_j in fp32 in list order; mode "nearest": slot 0.  A row without
    a valid slot is zero.  values i64 [R] -> out i64 [m]: values at slot 0 whatever the mode, `unlabeled` where there is none.
    A list entry outside -1..n-1 or an index value outside 0..R-1 is never dereferenced: the row is zero / unlabeled and counted in
    status i64 [2] = (rows with such a list entry, rows with such an index value), which a caller reads from buffers["status"].
    -> out.  buffers: optional dict of caller-owned out / status."""
    lib = _lib.load()
    who = "knn_interpolate"
    _chk(indices, torch.int64, "indices"), _chk(dist2, torch.float64, "dist2")
    if indices.dim() != 2 or indices.shape[0] < 1 or not 1 <= indices.shape[1] <= _lib.GP_KNN_QUERY_MAX_K or dist2.shape != indices.shape:
        raise ValueError(f"{who}: expected indices and dist2 [m >= 1, 1 <= k <= {_lib.GP_KNN_QUERY_MAX_K}], got {list(indices.shape)} and "
                         f"{list(dist2.shape)}")
    m, k = indices.shape
    dev = indices.device
    if mode not in KNN_INTERPOLATE_MODES:
        raise ValueError(f"{who}: mode={mode!r} must be one of {tuple(KNN_INTERPOLATE_MODES)}")
    labels = values.dtype == torch.int64
    if labels:
        if _chk(values, torch.int64, "values").dim() != 1 or values.shape[0] < 1:
            raise ValueError(f"{who}: expected integer values [R >= 1], got {list(values.shape)}")
    elif values.dtype not in ELEM_TAG or not values.is_cuda or values.dim() != 2 or min(values.shape) < 1 or values.stride(1) != 1 \
            or values.stride(0) < values.shape[1]:
        raise ValueError(f"{who}: values must be CUDA fp32, fp16 or bf16 [R >= 1, D >= 1] with unit column stride and a row stride >= D (or "
                         f"int64 [R]), got {values.dtype} {list(values.shape)} strides {values.stride()}")
    R = values.shape[0]
    if index is not None and (_chk(index, torch.int64, "index").dim() != 1 or index.shape[0] < 1):
        raise ValueError(f"{who}: expected index [n >= 1], got {list(index.shape)}")
    if any(t.device != dev for t in (values, dist2, index) if t is not None):
        raise ValueError(f"{who}: values, indices, dist2 and index must be on one device")
    n_index, npoints = (0, R) if index is None else (index.shape[0], index.shape[0])
    if labels:
        got = _outputs(who, {"out": (torch.int64, (m,)), "status": (torch.int64, (2,))}, buffers, dev)
        check(lib.gp_knn_interpolate_labels(_ptr(values), R, _ptr(index), n_index, _ptr(indices), m, k, npoints, int(unlabeled), _ptr(got["out"]),
                                            _ptr(got["status"]), _stream()), "gp_knn_interpolate_labels")
        return got["out"]
    D = values.shape[1]
    got = _outputs(who, {"out": (torch.float32, (m, D)), "status": (torch.int64, (2,))}, buffers, dev)
    check(lib.gp_knn_interpolate(_ptr(values), ELEM_TAG[values.dtype], R, D, values.stride(0), _ptr(index), n_index, _ptr(indices), _ptr(dist2),
                                 m, k, npoints, KNN_INTERPOLATE_MODES[mode], float(eps), _ptr(got["out"]), _ptr(got["status"]), _stream()),
          "gp_knn_interpolate")
    return got["out"]


KNN_INTERPOLATE_MAX_SLOTS = 2 ** 31 - 1                           # flat slots j * k + s of the backward are i32


def _chk_knn_lists(who, indices, index, nrows, mode, dist2=None):
    """the lists of the interpolation's backward: indices i64 [m,k] (dist2 f64 alike, where given), index i64 [n] or None, nrows the
    rows of values -> (m, k, n_index, npoints, their device)"""
    _chk(indices, torch.int64, "indices")
    if indices.dim() != 2 or indices.shape[0] < 1 or not 1 <= indices.shape[1] <= _lib.GP_KNN_QUERY_MAX_K:
        raise ValueError(f"{who}: expected indices [m >= 1, 1 <= k <= {_lib.GP_KNN_QUERY_MAX_K}], got {list(indices.shape)}")
    m, k = indices.shape
    if dist2 is not None and _chk(dist2, torch.float64, "dist2").shape != indices.shape:
        raise ValueError(f"{who}: expected dist2 {list(indices.shape)}, got {list(dist2.shape)}")
    if m * k > KNN_INTERPOLATE_MAX_SLOTS:
        raise ValueError(f"{who}: m * k = {m * k} flat slots, more than 2^31-1")
    if isinstance(nrows, bool) or not isinstance(nrows, int) or not 1 <= nrows < 2 ** 31:
        raise ValueError(f"{who}: nrows={nrows!r} outside 1..2^31-1")
    if mode not in KNN_INTERPOLATE_MODES:
        raise ValueError(f"{who}: mode={mode!r} must be one of {tuple(KNN_INTERPOLATE_MODES)}")
    if index is not None and (_chk(index, torch.int64, "index").dim() != 1 or index.shape[0] < 1):
        raise ValueError(f"{who}: expected index [n >= 1], got {list(index.shape)}")
    if any(t.device != indices.device for t in (dist2, index) if t is not None):
        raise ValueError(f"{who}: indices, dist2 and index must be on one device")
    n_index, npoints = (0, nrows) if index is None else (index.shape[0], index.shape[0])
    return m, k, n_index, npoints, indices.device


def knn_interpolate_weights(indices, dist2, index=None, nrows=None, mode="inverse_distance", eps=1e-8, buffers=None):
    """gp_knn_interpolate_weights, no sync: the fp32 weights knn_interpolate applies, by the same device code, as weights f32 [m,k]; 0
    where the slot is no reference (a -1 entry, a slot the mode does not read, a query row with a list entry outside -1..n-1 or an
    index value outside 0..nrows-1).  nrows: the rows of values (R).  buffers: optional dict with a caller-owned weights."""
    lib = _lib.load()
    who = "knn_interpolate_weights"
    m, k, n_index, npoints, dev = _chk_knn_lists(who, indices, index, nrows, mode, dist2)
    got = _outputs(who, {"weights": (torch.float32, (m, k))}, buffers, dev)
    check(lib.gp_knn_interpolate_weights(_ptr(indices), _ptr(dist2), _ptr(index), n_index, m, k, npoints, nrows, KNN_INTERPOLATE_MODES[mode],
                                         float(eps), _ptr(got["weights"]), _stream()), "gp_knn_interpolate_weights")
    return got["weights"]


def knn_interpolate_transpose_workspace_bytes(m, k, nrows):
    """gp_knn_interpolate_transpose_workspace_bytes (no GPU needed); 0: sizes the library does not take"""
    return int(_lib.load().gp_knn_interpolate_transpose_workspace_bytes(int(m), int(k), int(nrows)))


def knn_interpolate_transpose(indices, weights, index=None, nrows=None, mode="inverse_distance", buffers=None, workspace=None):
    """gp_knn_interpolate_transpose, no sync: the lists of knn_interpolate inverted, for its backward.  weights: what
    knn_interpolate_weights returned for the same lists, index, mode and eps.  -> (offsets i64 [nrows+1], slots i32 [m*k], sorted_weights
    f32 [m*k]): the references of row r of values are the flat slots f = j * k + s at slots[offsets[r] : offsets[r+1]], ascending, their
    weights beside them; offsets[nrows] counts the references, the slots past it are the flat slots that are none.  buffers: optional
    dict of caller-owned offsets / slots / sorted_weights; workspace: uint8 of at least knn_interpolate_transpose_workspace_bytes(m,
    k, nrows)."""
    lib = _lib.load()
    who = "knn_interpolate_transpose"
    m, k, n_index, npoints, dev = _chk_knn_lists(who, indices, index, nrows, mode)
    if _chk(weights, torch.float32, "weights").shape != (m, k) or weights.device != dev:
        raise ValueError(f"{who}: expected weights [{m}, {k}] on the lists' device, got {list(weights.shape)}")
    got = _outputs(who, {"offsets": (torch.int64, (nrows + 1,)), "slots": (torch.int32, (m * k,)), "sorted_weights": (torch.float32, (m * k,))},
                   buffers, dev)
    need = lib.gp_knn_interpolate_transpose_workspace_bytes(m, k, nrows)
    ws = _ws(need, dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_knn_interpolate_transpose(_ptr(indices), _ptr(index), n_index, m, k, npoints, nrows, KNN_INTERPOLATE_MODES[mode], _ptr(weights),
                                           _ptr(got["offsets"]), _ptr(got["slots"]), _ptr(got["sorted_weights"]), _ptr(ws), ws.numel(),
                                           _stream()), "gp_knn_interpolate_transpose")
    return got["offsets"], got["slots"], got["sorted_weights"]


def knn_interpolate_backward(g, offsets, slots, sorted_weights, k, dtype=torch.float32, buffers=None):
    """gp_knn_interpolate_backward, no sync: d_values [R,D] of `dtype` (fp32, fp16 or bf16; contiguous) from g = d_out f32 [m,D] (unit
    column stride, any row stride >= D, read in place) through the lists of knn_interpolate_transpose: per element acc = acc + w * g[j]
    in fp32 over the row's references in ascending flat slot, from +0, rounded to dtype once; zeros for a row without references.
    No atomics: two calls give the same bits.  buffers: optional dict with a caller-owned out."""
    lib = _lib.load()
    who = "knn_interpolate_backward"
    if not torch.is_tensor(g) or g.dtype != torch.float32 or not g.is_cuda or g.dim() != 2 or min(g.shape) < 1 or g.stride(1) != 1 \
            or g.stride(0) < g.shape[1]:
        raise ValueError(f"{who}: g must be CUDA fp32 [m >= 1, D >= 1] with unit column stride and a row stride >= D, got "
                         f"{(g.dtype, list(g.shape), g.stride()) if torch.is_tensor(g) else type(g).__name__}")
    m, D = g.shape
    if dtype not in ELEM_TAG:
        raise ValueError(f"{who}: dtype must be one of {tuple(ELEM_TAG)}, got {dtype}")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.GP_KNN_QUERY_MAX_K:
        raise ValueError(f"{who}: k={k!r} outside 1..{_lib.GP_KNN_QUERY_MAX_K}")
    if m * k > KNN_INTERPOLATE_MAX_SLOTS:
        raise ValueError(f"{who}: m * k = {m * k} flat slots, more than 2^31-1")
    _chk(offsets, torch.int64, "offsets"), _chk(slots, torch.int32, "slots"), _chk(sorted_weights, torch.float32, "sorted_weights")
    if offsets.dim() != 1 or offsets.shape[0] < 2 or slots.shape != (m * k,) or sorted_weights.shape != (m * k,):
        raise ValueError(f"{who}: expected offsets [R + 1], slots and sorted_weights [{m * k}], got {list(offsets.shape)}, {list(slots.shape)} "
                         f"and {list(sorted_weights.shape)}")
    R, dev = offsets.shape[0] - 1, g.device
    if any(t.device != dev for t in (offsets, slots, sorted_weights)):
        raise ValueError(f"{who}: g, offsets, slots and sorted_weights must be on one device")
    got = _outputs(who, {"out": (dtype, (R, D))}, buffers, dev)
    check(lib.gp_knn_interpolate_backward(_ptr(g), g.stride(0), m, D, _ptr(offsets), _ptr(slots), _ptr(sorted_weights), k, R, _ptr(got["out"]),
                                          ELEM_TAG[dtype], _stream()), "gp_knn_interpolate_backward")
    return got["out"]


# ------------------------------------------------------------------------------------------ the mask lift over batched point clouds
def _outputs(who, want, buffers, dev):
    """the named outputs: the caller's (checked) or fresh ones"""
    got = {}
    for name, (dtype, shape) in want.items():
        t = (buffers or {}).get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        elif _chk(t, dtype, name).shape != shape:
            raise ValueError(f"{who}: expected {name} {list(shape)}, got {list(t.shape)}")
        got[name] = t
    return got


class LiftMasksLists:
    """What gp_lift_masks_batched_lists writes: the view-major entries pt / x / y i64 [total] (global point row, pixel row, pixel
    column), view i32 [total], view_off i64 [V+1], view_count i64 [V], view_keep u8 [V], status i64 [8] = (bad batch rows, bad view
    entries, non-finite rows, top batch, 0, entries that did not fit, entries in all, the most views of one entry); total and max_views
    are the two sizes, read back."""

    def __init__(self, pt, x, y, view, view_off, view_count, view_keep, status, total, max_views):
        self.pt, self.x, self.y, self.view, self.view_off, self.view_count, self.view_keep = pt, x, y, view, view_off, view_count, view_keep
        self.status, self.total, self.max_views = status, total, max_views


def lift_masks_batched_lists(points, view_entry, w2c, intrinsics, depth, image_hw, cut_bound, vis_thres, min_visible, max_visible, buffers=None,
                             workspace=None, total=None, sizes=None):
    """The visible lists of all views of all entries: points f64 [n,4]; view_entry i64 [V]; w2c f64 [V,4,4]; intrinsics f64 [V,4]; depth
    f64 [V,H,W] or None; image_hw = (H, W).  -> LiftMasksLists.  Two calls of gp_lift_masks_batched_lists around ONE read-back (ops.readback
    of the counting call's status: the entries in all size the arrays); total: the count when the caller knows it already (no read-back,
    max_views is None then).  sizes: a callable that takes the place of the read-back: called after the counting call with the dict of
    view_off / view_count / view_keep / status, it returns (total, max_views) -- LiftMasksStream's, which reads its own sizes back and
    may still name the entry arrays in buffers.  buffers: optional dict of caller-owned outputs by attribute name (pt, x, y, view need
    total); workspace: uint8 of at least gp_lift_masks_batched_lists_workspace_bytes(n, V)."""
    lib = _lib.load()
    who = "lift_masks_batched_lists"
    _chk(points, torch.float64, "points")
    H, W = image_hw
    n, nv, dev = points.shape[0], view_entry.shape[0], points.device
    if points.dim() != 2 or points.shape[1] != 4:
        raise ValueError(f"{who}: expected points [n, 4], got {list(points.shape)}")
    _chk_views(who, nv, view_entry, w2c, intrinsics, depth, image_hw)
    got = _outputs(who, {"view_off": (torch.int64, (nv + 1,)), "view_count": (torch.int64, (nv,)), "view_keep": (torch.uint8, (nv,)),
                         "status": (torch.int64, (8,))}, buffers, dev)
    need = lib.gp_lift_masks_batched_lists_workspace_bytes(n, nv)
    ws = _ws(need, dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")

    def call(cap, ent):
        check(lib.gp_lift_masks_batched_lists(_ptr(points), n, _ptr(view_entry), _ptr(w2c), _ptr(intrinsics), _ptr(depth), nv, int(H), int(W),
                                              int(cut_bound), float(vis_thres), int(min_visible), int(max_visible), int(cap), _ptr(ent.get("pt")),
                                              _ptr(ent.get("x")), _ptr(ent.get("y")), _ptr(ent.get("view")), _ptr(got["view_off"]),
                                              _ptr(got["view_count"]), _ptr(got["view_keep"]), _ptr(got["status"]), _ptr(ws), ws.numel(),
                                              _stream()), "gp_lift_masks_batched_lists")

    max_views = None
    if total is None:
        call(0, {})
        if sizes is None:
            words = readback(got["status"])
            total, max_views = int(words[6]), int(words[7])
        else:
            total, max_views = sizes(got)
    ent = {}
    if total > 0:
        ent = _outputs(who, {"pt": (torch.int64, (total,)), "x": (torch.int64, (total,)), "y": (torch.int64, (total,)),
                             "view": (torch.int32, (total,))}, buffers, dev)
        call(total, ent)
    return LiftMasksLists(ent.get("pt"), ent.get("x"), ent.get("y"), ent.get("view"), got["view_off"], got["view_count"], got["view_keep"],
                          got["status"], total, max_views)


class LiftMasksBatched:
    """What gp_lift_masks_batched writes: out fp32 [n, d] (before the scene-level fill), seen u8 [n], count i32 [n], nn i64 [n] or None,
    seg i32 [total] (every entry's segment after the in-view fill, -1 = none), status i64 [8] = (bad batch rows, bad view entries,
    non-finite rows, top batch, seen rows, filled rows, entries that are not what the lists promise, views beyond words x 64)."""

    def __init__(self, out, seen, count, nn, seg, status):
        self.out, self.seen, self.count, self.nn, self.seg, self.status = out, seen, count, nn, seg, status


def lift_masks_batched(points, view_entry, pred_masks, scores, taps, out_hw, ent, view_off, view_keep, total, words, f_seg, logit_seg, fill=True,
                       fill_cap=None, buffers=None, workspace=None):
    """gp_lift_masks_batched_t, no sync: from view-major entries to the fused rows.  points f64 [n,4]; view_entry i64 [V]; pred_masks f32,
    f16 or bf16 [V,Q,h,w] (read in place; the workspace's transposed copy keeps their dtype); scores f32 [V,Q]; taps = (x0 i32 [W], wx f32 [W,4], y0 i32 [H], wy f32 [H,4]); out_hw = (H, W); ent = (pt, x, y i64
    [>= total], view i32 [>= total]) -- lift_masks_batched_lists' or the caller's own: entries of a view contiguous, rows ascending inside
    it --; view_off i64 [V+1]; view_keep u8 [V]; words >= ceil(most views of one entry / 64); f_seg f32 [V,Q,d], logit_seg f32 [V,Q,C]
    (segment_tables; d a multiple of 4).  -> LiftMasksBatched.  buffers: optional dict of caller-owned outputs by attribute name (out:
    fp32 rows of a pitch that is a multiple of 4); workspace: uint8 of at least gp_lift_masks_batched_workspace_bytes(...)."""
    lib = _lib.load()
    who = "lift_masks_batched"
    _chk(points, torch.float64, "points"), _chk(view_entry, torch.int64, "view_entry")
    elem = _chk_elem(pred_masks, "pred_masks")
    _chk(scores, torch.float32, "scores"), _chk(view_off, torch.int64, "view_off"), _chk(view_keep, torch.uint8, "view_keep")
    _chk(f_seg, torch.float32, "f_seg"), _chk(logit_seg, torch.float32, "logit_seg")
    tx0, twx, ty0, twy = taps
    _chk(tx0, torch.int32, "tap_x0"), _chk(twx, torch.float32, "tap_wx"), _chk(ty0, torch.int32, "tap_y0"), _chk(twy, torch.float32, "tap_wy")
    pt, x, y, view = ent
    _chk(pt, torch.int64, "ent_pt"), _chk(x, torch.int64, "ent_x"), _chk(y, torch.int64, "ent_y"), _chk(view, torch.int32, "ent_view")
    H, W = out_hw
    n, dev, total = points.shape[0], points.device, int(total)
    if points.dim() != 2 or points.shape[1] != 4 or pred_masks.dim() != 4 or view_entry.shape != (pred_masks.shape[0],):
        raise ValueError(f"{who}: expected points [n, 4], pred_masks [V, Q, h, w], view_entry [V], got {list(points.shape)}, "
                         f"{list(pred_masks.shape)}, {list(view_entry.shape)}")
    nv, Q, h, w = pred_masks.shape
    if scores.shape != (nv, Q) or view_off.shape != (nv + 1,) or view_keep.shape != (nv,):
        raise ValueError(f"{who}: expected scores [{nv}, {Q}], view_off [{nv + 1}], view_keep [{nv}], got {list(scores.shape)}, "
                         f"{list(view_off.shape)}, {list(view_keep.shape)}")
    if tx0.shape != (W,) or twx.shape != (W, 4) or ty0.shape != (H,) or twy.shape != (H, 4):
        raise ValueError(f"{who}: expected taps ([{W}], [{W}, 4], [{H}], [{H}, 4]), got {[list(t.shape) for t in taps]}")
    if total < 1 or any(t.dim() != 1 or t.shape[0] < total for t in ent):
        raise ValueError(f"{who}: expected four entry arrays of at least total = {total} >= 1 elements, got {[list(t.shape) for t in ent]}")
    if f_seg.dim() != 3 or f_seg.shape[:2] != (nv, Q) or logit_seg.dim() != 3 or logit_seg.shape[:2] != (nv, Q):
        raise ValueError(f"{who}: expected f_seg [{nv}, {Q}, d] and logit_seg [{nv}, {Q}, C], got {list(f_seg.shape)}, {list(logit_seg.shape)}")
    d, C = f_seg.shape[2], logit_seg.shape[2]
    want = {"seen": (torch.uint8, (n,)), "count": (torch.int32, (n,)), "seg": (torch.int32, (total,)), "status": (torch.int64, (8,))}
    if fill:
        want["nn"] = (torch.int64, (n,))
    got = _outputs(who, want, buffers, dev)
    out = (buffers or {}).get("out")
    out = torch.empty((n, d), dtype=torch.float32, device=dev) if out is None else _rows(out, "out", n, d)
    if fill_cap is None:
        fill_cap = min(total, max(total // 4, 65536))
    need = lib.gp_lift_masks_batched_workspace_bytes_t(elem, n, nv, Q, h, w, int(H), int(W), total, int(words), int(fill_cap))
    ws = _ws(need, dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_masks_batched_t(_ptr(points), n, _ptr(view_entry), nv, _ptr(pred_masks), elem, Q, h, w, _ptr(scores), _ptr(tx0), _ptr(twx),
                                      _ptr(ty0), _ptr(twy), int(H), int(W), _ptr(pt), _ptr(x), _ptr(y), _ptr(view), _ptr(view_off), _ptr(view_keep),
                                      total, int(words), int(fill_cap), _ptr(f_seg), _ptr(logit_seg), d, C, 1 if fill else 0, _ptr(out),
                                      out.stride(0), _ptr(got["seen"]), _ptr(got["count"]), _ptr(got.get("nn")), _ptr(got["seg"]),
                                      _ptr(got["status"]), _ptr(ws), ws.numel(), _stream()), "gp_lift_masks_batched")
    return LiftMasksBatched(out, got["seen"], got["count"], got.get("nn"), got["seg"], got["status"])


# ------------------------------------------------------------------------------------------ the same mask lift, the views in chunks
class LiftMasksStreamState:
    """What a resumable mask lift keeps between its calls besides the arrays that grow with the views (those are the caller's, see
    lift_masks_stream_add): points f64 [n,4], state u8 (the entry tables and one view counter per entry: written by
    gp_lift_masks_stream_begin, the counters advanced by gp_lift_masks_stream_add), status i64 [8] (the running words: bad batch rows, bad
    view entries so far, non-finite rows, top batch, the most views of one entry, records, entries and counters that did not hold
    together, positions beyond 65535)."""

    def __init__(self, points, state, status):
        self.points, self.state, self.status = points, state, status


def lift_masks_stream_begin(points, buffers=None, workspace=None):
    """gp_lift_masks_stream_begin, no sync: points f64 [n,4] -> LiftMasksStreamState.  buffers: optional dict of caller-owned state (uint8
    of at least gp_lift_masks_stream_state_bytes(n)) / status; workspace: uint8 of at least gp_lift_masks_stream_begin_workspace_bytes(n)."""
    lib = _lib.load()
    n, dev = _chk_points("lift_masks_stream_begin", points)
    got = _outputs("lift_masks_stream_begin", {"status": (torch.int64, (8,))}, buffers, dev)
    state = (buffers or {}).get("state")
    state = _ws(lib.gp_lift_masks_stream_state_bytes(n), dev) if state is None else _chk(state, torch.uint8, "state")
    ws = _ws(lib.gp_lift_masks_stream_begin_workspace_bytes(n), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_masks_stream_begin(_ptr(points), n, _ptr(state), state.numel(), _ptr(got["status"]), _ptr(ws), ws.numel(), _stream()),
          "gp_lift_masks_stream_begin")
    return LiftMasksStreamState(points, state, got["status"])


def lift_masks_stream_state_bytes(n):
    return int(_lib.load().gp_lift_masks_stream_state_bytes(int(n)))


def lift_masks_batched_lists_workspace_bytes(n, num_views):
    return int(_lib.load().gp_lift_masks_batched_lists_workspace_bytes(int(n), int(num_views)))


def lift_masks_stream_sizes_workspace_bytes(num_views):
    return int(_lib.load().gp_lift_masks_stream_sizes_workspace_bytes(int(num_views)))


def _elem_of(dtype, who):
    if dtype not in ELEM_TAG:
        raise ValueError(f"{who}: the masks are torch.float32, torch.float16 or torch.bfloat16, got {dtype}")
    return ELEM_TAG[dtype]


def lift_masks_batched_workspace_bytes(n, num_views, Q, mask_hw, image_hw, total, words, fill_cap=None, dtype=torch.float32):
    """bytes of gp_lift_masks_batched_t's workspace for pred_masks of `dtype`: the transposed copy in it keeps the masks' element size"""
    if fill_cap is None:
        fill_cap = min(total, max(total // 4, 65536))
    return int(_lib.load().gp_lift_masks_batched_workspace_bytes_t(_elem_of(dtype, "lift_masks_batched_workspace_bytes"), int(n), int(num_views),
                                                                   int(Q), int(mask_hw[0]), int(mask_hw[1]), int(image_hw[0]), int(image_hw[1]),
                                                                   int(total), int(words), int(fill_cap)))


def lift_masks_stream_add_workspace_bytes(n, num_views, Q, mask_hw, image_hw, total, fill_cap=None, dtype=torch.float32):
    if fill_cap is None:
        fill_cap = min(total, max(total // 4, 65536))
    return int(_lib.load().gp_lift_masks_stream_add_workspace_bytes_t(_elem_of(dtype, "lift_masks_stream_add_workspace_bytes"), int(n),
                                                                      int(num_views), int(Q), int(mask_hw[0]), int(mask_hw[1]), int(image_hw[0]),
                                                                      int(image_hw[1]), int(total), int(fill_cap)))


def lift_masks_stream_finish_workspace_bytes(n, num_views, total, words):
    return int(_lib.load().gp_lift_masks_stream_finish_workspace_bytes(int(n), int(num_views), int(total), int(words)))


def lift_masks_stream_sizes(st, view_entry, view_count, view_keep, buffers=None, workspace=None):
    """gp_lift_masks_stream_sizes, no sync: a chunk's view_entry i64 [V] with the view_count i64 [V] / view_keep u8 [V] of
    lift_masks_batched_lists' counting call -> sizes i64 [4] = (the chunk's visible entries, those of its kept views, the most views one
    entry has once the chunk is added, 0).  st is not changed.  buffers: optional dict with a caller-owned sizes; workspace: uint8 of at
    least gp_lift_masks_stream_sizes_workspace_bytes(V)."""
    lib = _lib.load()
    who = "lift_masks_stream_sizes"
    _chk(view_entry, torch.int64, "view_entry"), _chk(view_count, torch.int64, "view_count"), _chk(view_keep, torch.uint8, "view_keep")
    nv, n, dev = view_entry.shape[0], st.points.shape[0], st.points.device
    if view_entry.dim() != 1 or view_count.shape != (nv,) or view_keep.shape != (nv,):
        raise ValueError(f"{who}: expected view_entry, view_count, view_keep [V], got {list(view_entry.shape)}, {list(view_count.shape)}, "
                         f"{list(view_keep.shape)}")
    got = _outputs(who, {"sizes": (torch.int64, (4,))}, buffers, dev)
    ws = _ws(lib.gp_lift_masks_stream_sizes_workspace_bytes(nv), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_masks_stream_sizes(n, _ptr(st.state), st.state.numel(), _ptr(st.status), _ptr(view_entry), _ptr(view_count), _ptr(view_keep),
                                         nv, _ptr(got["sizes"]), _ptr(ws), ws.numel(), _stream()), "gp_lift_masks_stream_sizes")
    return got["sizes"]


def lift_masks_stream_add(st, view_entry, pred_masks, scores, taps, out_hw, ent, view_off, view_keep, total, rec_row, rec_seg, rec_base, rec_off,
                          view_pos, fill_cap=None, workspace=None):
    """gp_lift_masks_stream_add, no sync: one chunk of views onto the LiftMasksStreamState st.  The chunk's arrays as
    ops.lift_masks_batched takes them (view_entry i64 [V]; pred_masks f32, f16 or bf16 [V,Q,h,w]; scores f32 [V,Q]; taps; out_hw; ent = (pt, x, y,
    view) and view_off i64 [V+1], view_keep u8 [V], total from lift_masks_batched_lists ON THE CHUNK).  What the caller keeps: rec_row /
    rec_seg i32 [capacity] (the chunk's records go to rec_base ..), rec_off i64 [V+1] and view_pos i32 [V] (the chunk's slices of the
    per-view arrays; rec_off[V] is the next chunk's rec_off[0]).  total = 0: nothing is visible in a kept view of the chunk -- pred_masks,
    scores, ent, rec_row and rec_seg may be None, only view_pos, rec_off and the counters are written.  workspace: uint8 of at least
    lift_masks_stream_add_workspace_bytes(...)."""
    lib = _lib.load()
    who = "lift_masks_stream_add"
    _chk(view_entry, torch.int64, "view_entry"), _chk(view_off, torch.int64, "view_off"), _chk(view_keep, torch.uint8, "view_keep")
    _chk(rec_off, torch.int64, "rec_off"), _chk(view_pos, torch.int32, "view_pos")
    nv, n, dev, total = view_entry.shape[0], st.points.shape[0], st.points.device, int(total)
    H, W = out_hw
    if view_entry.dim() != 1 or view_off.shape != (nv + 1,) or view_keep.shape != (nv,) or rec_off.shape != (nv + 1,) or view_pos.shape != (nv,):
        raise ValueError(f"{who}: expected view_entry [V], view_off [V + 1], view_keep [V], rec_off [V + 1], view_pos [V], got "
                         f"{[list(t.shape) for t in (view_entry, view_off, view_keep, rec_off, view_pos)]}")
    Q = h = w = 1
    tx0 = twx = ty0 = twy = None
    pt = x = y = view = None
    cap, elem = 0, _lib.GP_ELEM_F32
    if total:
        elem = _chk_elem(pred_masks, "pred_masks")
        _chk(scores, torch.float32, "scores")
        _chk(rec_row, torch.int32, "rec_row"), _chk(rec_seg, torch.int32, "rec_seg")
        tx0, twx, ty0, twy = taps
        _chk(tx0, torch.int32, "tap_x0"), _chk(twx, torch.float32, "tap_wx"), _chk(ty0, torch.int32, "tap_y0"), _chk(twy, torch.float32, "tap_wy")
        pt, x, y, view = ent
        _chk(pt, torch.int64, "ent_pt"), _chk(x, torch.int64, "ent_x"), _chk(y, torch.int64, "ent_y"), _chk(view, torch.int32, "ent_view")
        if pred_masks.dim() != 4 or pred_masks.shape[0] != nv or scores.shape != tuple(pred_masks.shape[:2]):
            raise ValueError(f"{who}: expected pred_masks [{nv}, Q, h, w] and scores [{nv}, Q], got {list(pred_masks.shape)}, {list(scores.shape)}")
        _, Q, h, w = pred_masks.shape
        if tx0.shape != (W,) or twx.shape != (W, 4) or ty0.shape != (H,) or twy.shape != (H, 4):
            raise ValueError(f"{who}: expected taps ([{W}], [{W}, 4], [{H}], [{H}, 4]), got {[list(t.shape) for t in taps]}")
        if any(t.dim() != 1 or t.shape[0] < total for t in ent):
            raise ValueError(f"{who}: expected four entry arrays of at least total = {total} elements, got {[list(t.shape) for t in ent]}")
        if rec_row.dim() != 1 or rec_row.shape != rec_seg.shape:
            raise ValueError(f"{who}: expected rec_row and rec_seg [capacity], got {list(rec_row.shape)}, {list(rec_seg.shape)}")
        cap = rec_row.shape[0]
    if fill_cap is None:
        fill_cap = min(total, max(total // 4, 65536))
    need = lib.gp_lift_masks_stream_add_workspace_bytes_t(elem, n, nv, Q, h, w, int(H), int(W), total, int(fill_cap))
    ws = _ws(need, dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_masks_stream_add_t(_ptr(st.points), n, _ptr(st.state), st.state.numel(), _ptr(view_entry), nv, _ptr(pred_masks), elem, Q, h, w,
                                         _ptr(scores), _ptr(tx0), _ptr(twx), _ptr(ty0), _ptr(twy), int(H), int(W), _ptr(pt), _ptr(x), _ptr(y),
                                         _ptr(view), _ptr(view_off), _ptr(view_keep), total, int(fill_cap), _ptr(rec_row), _ptr(rec_seg),
                                         int(rec_base), max(cap, int(rec_base)), _ptr(rec_off), _ptr(view_pos), _ptr(st.status), _ptr(ws),
                                         ws.numel(), _stream()), "gp_lift_masks_stream_add")


class LiftMasksStreamFinish:
    """What gp_lift_masks_stream_finish writes: out fp32 [n, d] (before the scene-level fill), seen u8 [n], count i32 [n], nn i64 [n] or
    None, status i64 [8] = (bad batch rows, bad view entries, non-finite rows, top batch, seen rows, filled rows, values of the state, the
    record offsets and the records that did not hold together, views whose position is beyond words x 64)."""

    def __init__(self, out, seen, count, nn, status):
        self.out, self.seen, self.count, self.nn, self.status = out, seen, count, nn, status


def lift_masks_stream_finish(st, view_entry, view_pos, view_keep, rec_off, rec_row, rec_seg, total, words, f_seg, logit_seg, fill=True,
                             buffers=None, workspace=None):
    """gp_lift_masks_stream_finish, no sync: everything kept since lift_masks_stream_begin -> LiftMasksStreamFinish; nothing kept is
    changed.  view_entry i64 [V], view_pos i32 [V], view_keep u8 [V], rec_off i64 [V+1] over ALL views added; rec_row / rec_seg i32 [>=
    total]; total >= 1 records; words >= ceil(most views of one entry / 64); f_seg f32 [>= V, Q, d], logit_seg f32 [>= V, Q, C] in arrival
    order (segment_tables; d a multiple of 4).  buffers: optional dict of caller-owned out (fp32 rows of a pitch that is a multiple of
    4) / seen / count / nn / status; workspace: uint8 of at least lift_masks_stream_finish_workspace_bytes(n, V, total, words)."""
    lib = _lib.load()
    who = "lift_masks_stream_finish"
    _chk(view_entry, torch.int64, "view_entry"), _chk(view_pos, torch.int32, "view_pos"), _chk(view_keep, torch.uint8, "view_keep")
    _chk(rec_off, torch.int64, "rec_off"), _chk(rec_row, torch.int32, "rec_row"), _chk(rec_seg, torch.int32, "rec_seg")
    _chk(f_seg, torch.float32, "f_seg"), _chk(logit_seg, torch.float32, "logit_seg")
    nv, n, dev, total = view_entry.shape[0], st.points.shape[0], st.points.device, int(total)
    if view_entry.dim() != 1 or view_pos.shape != (nv,) or view_keep.shape != (nv,) or rec_off.shape != (nv + 1,):
        raise ValueError(f"{who}: expected view_entry, view_pos, view_keep [V] and rec_off [V + 1], got "
                         f"{[list(t.shape) for t in (view_entry, view_pos, view_keep, rec_off)]}")
    if total < 1 or rec_row.dim() != 1 or rec_seg.dim() != 1 or rec_row.shape[0] < total or rec_seg.shape[0] < total:
        raise ValueError(f"{who}: expected rec_row and rec_seg of at least total = {total} >= 1 elements, got {list(rec_row.shape)}, "
                         f"{list(rec_seg.shape)}")
    if f_seg.dim() != 3 or logit_seg.dim() != 3 or f_seg.shape[0] < nv or logit_seg.shape[0] < nv or f_seg.shape[1] != logit_seg.shape[1]:
        raise ValueError(f"{who}: expected f_seg [>= {nv}, Q, d] and logit_seg [>= {nv}, Q, C], got {list(f_seg.shape)}, {list(logit_seg.shape)}")
    Q, d, C = f_seg.shape[1], f_seg.shape[2], logit_seg.shape[2]
    want = {"seen": (torch.uint8, (n,)), "count": (torch.int32, (n,)), "status": (torch.int64, (8,))}
    if fill:
        want["nn"] = (torch.int64, (n,))
    got = _outputs(who, want, buffers, dev)
    out = (buffers or {}).get("out")
    out = torch.empty((n, d), dtype=torch.float32, device=dev) if out is None else _rows(out, "out", n, d)
    need = lib.gp_lift_masks_stream_finish_workspace_bytes(n, nv, total, int(words))
    ws = _ws(need, dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_lift_masks_stream_finish(_ptr(st.points), n, _ptr(st.state), st.state.numel(), _ptr(view_entry), _ptr(view_pos), _ptr(view_keep),
                                          _ptr(rec_off), nv, _ptr(rec_row), _ptr(rec_seg), total, int(words), _ptr(f_seg), _ptr(logit_seg), Q, d, C,
                                          _ptr(st.status), 1 if fill else 0, _ptr(out), out.stride(0), _ptr(got["seen"]), _ptr(got["count"]),
                                          _ptr(got.get("nn")), _ptr(got["status"]), _ptr(ws), ws.numel(), _stream()),
          "gp_lift_masks_stream_finish")
    return LiftMasksStreamFinish(out, got["seen"], got["count"], got.get("nn"), got["status"])


# ------------------------------------------------------------------------------------------ training step
def col_stats(y, c=None):
    """mean, biased variance of the rows of y fp32 [nv, >=c] (BatchNorm1d training statistics)."""
    lib = _lib.load()
    nv = y.shape[0]
    c = y.shape[1] if c is None else c
    ws = _ws(lib.gp_col_stats_workspace_bytes(nv, c), y.device)
    mean = torch.empty(c, dtype=torch.float32, device=y.device)
    var = torch.empty(c, dtype=torch.float32, device=y.device)
    check(lib.gp_col_stats(_ptr(y), y.stride(0), nv, int(c), _ptr(mean), _ptr(var), _ptr(ws), ws.numel(), _stream()), "gp_col_stats")
    return mean, var


def col_sums_f64(y, c=None, mean=None):
    """fp64 column sums of y fp32 [nv, >=c] (mean None) or of (y - mean)^2: the SyncBatchNorm reduction vectors."""
    lib = _lib.load()
    nv = y.shape[0]
    c = y.shape[1] if c is None else c
    ws = _ws(lib.gp_col_stats_workspace_bytes(nv, c), y.device)
    out = torch.empty(c, dtype=torch.float64, device=y.device)
    check(lib.gp_col_sums_f64(_ptr(y), y.stride(0), nv, int(c), _ptr(mean), _ptr(out), _ptr(ws), ws.numel(), _stream()), "gp_col_sums_f64")
    return out


def bn_bwd_sums_f64(dout, act, y, mean, var, eps, mask_affine=None):
    """fp64 [2c]: sum dz | sum dz * xhat over this rank's rows (dz = dout masked by act > 0, or -- act None, mask_affine = (gamma, beta) --
    by the sign of the normalised, affine y: see bn_train_backward)."""
    lib = _lib.load()
    nv, c = y.shape[0], mean.shape[0]
    ws = _ws(lib.gp_col_stats_workspace_bytes(nv, c), y.device)
    sums = torch.empty(2 * c, dtype=torch.float64, device=y.device)
    check(lib.gp_bn_bwd_sums_f64(_ptr(dout), dout.stride(0), _ptr(act), act.stride(0) if act is not None else 0, _ptr(y), y.stride(0),
                                 _ptr(mean), _ptr(var), float(eps), _ptr(mask_affine[0]) if mask_affine else None,
                                 _ptr(mask_affine[1]) if mask_affine else None, nv, int(c), _ptr(sums), _ptr(ws), ws.numel(), _stream()),
          "gp_bn_bwd_sums_f64")
    return sums


def bn_bwd_apply(dout, act, y, mean, var, eps, gamma, sums_f32, n_total, want_dz=False, dy_scale2=None, beta_mask=None):
    """dy (and dz) of the BatchNorm backward pass from reduction vectors taken over n_total rows (all ranks).
    dy_scale2 (fp32 [2] device tensor): receives pow2_scale(dy) from the same sweep."""
    lib = _lib.load()
    nv, c = y.shape[0], mean.shape[0]
    dy = torch.empty((nv, c), dtype=torch.float32, device=y.device)
    dz = torch.empty((nv, c), dtype=torch.float32, device=y.device) if want_dz else None
    check(lib.gp_bn_bwd_apply(_ptr(dout), dout.stride(0), _ptr(act), act.stride(0) if act is not None else 0, _ptr(y), y.stride(0),
                              _ptr(mean), _ptr(var), float(eps), _ptr(gamma), _ptr(beta_mask), _ptr(sums_f32), int(n_total), nv, int(c), _ptr(dy), dy.stride(0),
                              _ptr(dz), dz.stride(0) if dz is not None else 0, _ptr(dy_scale2), _stream()), "gp_bn_bwd_apply")
    return (dy, dz) if want_dz else dy


def bn_train_apply(y, mean, var, gamma, beta, eps, residual=None, relu=True, want_split=False, momentum=0.1,
                   running_mean=None, running_var=None, want_f32=True):
    """(out fp32 | None, (hi, lo) | None).  want_f32=False (with want_split): only the split planes are written -- for a layer whose
    backward pass takes its ReLU mask from y (bn_train_backward(beta_mask=))."""
    lib = _lib.load()
    nv, c = y.shape[0], mean.shape[0]
    assert want_f32 or want_split
    out = torch.empty((nv, c), dtype=torch.float32, device=y.device) if want_f32 else None
    hi = lo = None
    if want_split:
        hi = torch.empty((nv, c), dtype=torch.float16, device=y.device)
        lo = torch.empty((nv, c), dtype=torch.float16, device=y.device)
    check(lib.gp_bn_train_apply(_ptr(y), y.stride(0), nv, int(c), _ptr(mean), _ptr(var), _ptr(gamma), _ptr(beta), float(eps),
                                _ptr(residual), residual.stride(0) if residual is not None else 0, int(bool(relu)), _ptr(out),
                                out.stride(0) if out is not None else 0, _ptr(hi), _ptr(lo), hi.stride(0) if hi is not None else 0, float(momentum),
                                _ptr(running_mean), _ptr(running_var), _stream()), "gp_bn_train_apply")
    return out, ((hi, lo) if want_split else None)


def bn_train_backward(dout, act, y, mean, var, eps, gamma, want_dz=False, dy_scale2=None, beta_mask=None, split=False):
    """Returns dy, dgamma, dbeta (, dz).  act: post-ReLU activation (mask) or None; act None and beta_mask = the layer's beta: the mask of a
    layer WITHOUT a residual recomputed from y ((y - mean) * invstd * gamma + beta > 0: the float the forward pass evaluated).
    dy_scale2 (fp32 [2] device tensor): receives pow2_scale(dy) from the sweep that writes dy.
    split=True (needs dy_scale2): dy comes back as ((hi, lo) f16 [nv + 1, c] with a zero last row) holding dy * dy_scale2[0] -- written by
    the sweep itself, the scale from a bound of max |dy| taken in the reduction pass (no fp32 dy, no split pass)."""
    lib = _lib.load()
    nv, c = y.shape[0], mean.shape[0]
    dev = y.device
    hi = lo = dy = None
    if split:
        assert dy_scale2 is not None
        hi = torch.empty((nv + 1, c), dtype=torch.float16, device=dev)
        lo = torch.empty((nv + 1, c), dtype=torch.float16, device=dev)
    else:
        dy = torch.empty((nv, c), dtype=torch.float32, device=dev)
    dz = torch.empty((nv, c), dtype=torch.float32, device=dev) if want_dz else None
    dgamma = torch.empty(c, dtype=torch.float32, device=dev)
    dbeta = torch.empty(c, dtype=torch.float32, device=dev)
    ws = _ws(lib.gp_bn_train_backward_workspace_bytes(nv, int(c)), dev)
    check(lib.gp_bn_train_backward(_ptr(dout), dout.stride(0), _ptr(act), act.stride(0) if act is not None else 0, _ptr(y),
                                   y.stride(0), _ptr(mean), _ptr(var), float(eps), _ptr(gamma), _ptr(beta_mask), nv, int(c), _ptr(dy),
                                   dy.stride(0) if dy is not None else 0, _ptr(dz), dz.stride(0) if dz is not None else 0, _ptr(dgamma),
                                   _ptr(dbeta), _ptr(dy_scale2), _ptr(hi), _ptr(lo), hi.stride(0) if hi is not None else 0, _ptr(ws),
                                   ws.numel(), _stream()), "gp_bn_train_backward")
    dy = (hi, lo) if split else dy
    return (dy, dgamma, dbeta, dz) if want_dz else (dy, dgamma, dbeta)


def infonce_fwd_bwd(e, sample_to_voxel, point_to_batch, num_anchors, num_negatives, temperature):
    """loss (0-d device tensor) and d loss / d e of the InfoNCE over (anchor | positive | negatives) samples."""
    lib = _lib.load()
    nv, d = e.shape
    ns = sample_to_voxel.shape[0]
    _chk(sample_to_voxel, torch.int64, "sample_to_voxel")
    _chk(point_to_batch, torch.int64, "point_to_batch")
    assert point_to_batch.shape[0] == num_anchors * (2 + num_negatives)
    loss = torch.empty((), dtype=torch.float32, device=e.device)
    de = torch.empty((nv, d), dtype=torch.float32, device=e.device)
    ws = _ws(lib.gp_infonce_workspace_bytes(ns, d), e.device)
    check(lib.gp_infonce_fwd_bwd(_ptr(e), e.stride(0), nv, int(d), _ptr(sample_to_voxel), ns, _ptr(point_to_batch),
                                 int(num_anchors), int(num_negatives), float(temperature), _ptr(loss), _ptr(de), de.stride(0),
                                 _ptr(ws), ws.numel(), _stream()), "gp_infonce_fwd_bwd")
    return loss, de


def infonce_weighted_fwd_bwd(e, sample_to_voxel, point_to_batch, num_anchors, num_negatives, temperature, weights):
    """(loss 0-d, per-anchor losses f32 [A], d loss / d e) of loss = sum_a weights[a] l_a (gp_infonce_weighted_fwd_bwd)"""
    lib = _lib.load()
    nv, d = e.shape
    ns = sample_to_voxel.shape[0]
    _chk(e, torch.float32, "e")
    _chk(sample_to_voxel, torch.int64, "sample_to_voxel")
    _chk(point_to_batch, torch.int64, "point_to_batch")
    _chk(weights, torch.float32, "weights")
    if point_to_batch.shape != (num_anchors * (2 + num_negatives),) or weights.shape != (num_anchors,):
        raise ValueError(f"infonce_weighted_fwd_bwd: expected point_to_batch [{num_anchors * (2 + num_negatives)}] and weights [{num_anchors}], got "
                         f"{list(point_to_batch.shape)} and {list(weights.shape)}")
    loss = torch.empty((), dtype=torch.float32, device=e.device)
    anchor_loss = torch.empty(num_anchors, dtype=torch.float32, device=e.device)
    de = torch.empty((nv, d), dtype=torch.float32, device=e.device)
    ws = _ws(lib.gp_infonce_workspace_bytes(ns, d), e.device)
    check(lib.gp_infonce_weighted_fwd_bwd(_ptr(e), e.stride(0), nv, int(d), _ptr(sample_to_voxel), ns, _ptr(point_to_batch), int(num_anchors),
                                          int(num_negatives), float(temperature), _ptr(weights), _ptr(loss), _ptr(anchor_loss), _ptr(de),
                                          de.stride(0), _ptr(ws), ws.numel(), _stream()), "gp_infonce_weighted_fwd_bwd")
    return loss, anchor_loss, de


def adamw_step_(param, grad, exp_avg, exp_avg_sq, lr, step, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8):
    lib = _lib.load()
    for t in (param, grad, exp_avg, exp_avg_sq):
        _chk(t, torch.float32, "adamw tensor")
        assert t.is_contiguous() and t.numel() == param.numel()
    check(lib.gp_adamw_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), float(lr), float(betas[0]),
                            float(betas[1]), float(eps), float(weight_decay), int(step), _stream()), "gp_adamw_step")
    return param


def knn_points(xyz, queries, k):
    """xyz fp32 [N,3]; queries i64 [A] row ids -> i64 [A,k] nearest other rows, (d^2, id) order."""
    lib = _lib.load()
    _chk(xyz, torch.float32, "xyz")
    _chk(queries, torch.int64, "queries")
    out = torch.empty((queries.shape[0], k), dtype=torch.int64, device=xyz.device)
    flag = torch.zeros(1, dtype=torch.int32, device=xyz.device)
    check(lib.gp_knn_points_f32(_ptr(xyz), xyz.shape[0], _ptr(queries), queries.shape[0], int(k), _ptr(out), _ptr(flag),
                                _stream()), "gp_knn_points_f32")
    return out, flag


def sampler_select(sim, anchor_indices, k, n=None):
    """positive i64 [A], macro i64 [A, k] of sim fp32 [A, >= n] (gp_sampler_select): the arg-max over the points other than the anchor
    and the k lowest other than anchor and positive, ascending by (value, index).  sim is not written."""
    lib = _lib.load()
    A = sim.shape[0]
    n = sim.shape[1] if n is None else n
    assert sim.stride(1) == 1 and anchor_indices.dtype == torch.int64 and anchor_indices.is_contiguous()
    positive = torch.empty(A, dtype=torch.int64, device=sim.device)
    macro = torch.empty((A, k), dtype=torch.int64, device=sim.device)
    check(lib.gp_sampler_select(_ptr(sim), sim.stride(0), A, int(n), _ptr(anchor_indices), int(k), _ptr(positive), _ptr(macro), _stream()),
          "gp_sampler_select")
    return positive, macro


def _segment_rows(who, a, *ts):
    for name, t, dt in ts:
        _chk(t, dt, name)
        if t.shape != (a,):
            raise ValueError(f"{who}: expected {name} [{a}], got {list(t.shape)}")


def sim_segments(hi, lo, anchor_row, seg_first, seg_len, row_off, max_len, out):
    """The anchors' similarity rows, each against its own batch entry, into the ragged fp32 buffer `out` (gp_sim_segments_f16x3):
    out[row_off[a] + j] = <x[anchor_row[a]], x[seg_first[a] + j]>, j < seg_len[a], x = hi + lo (normalize_split_f16 planes, width a
    multiple of 32).  anchor_row / seg_first / seg_len i32 [A] with the anchors grouped by entry, row_off i64 [A] multiples of 4;
    max_len: the largest seg_len (host int).  Floats of `out` outside the extents are not written."""
    lib = _lib.load()
    _chk(out, torch.float32, "out")
    for name, t in (("hi", hi), ("lo", lo)):
        if t.dtype != torch.float16 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"sim_segments: expected {name} as CUDA float16 rows [n, d] with unit column stride, got {t.dtype} {list(t.shape)}")
    a = anchor_row.shape[0]
    _segment_rows("sim_segments", a, ("anchor_row", anchor_row, torch.int32), ("seg_first", seg_first, torch.int32), ("seg_len", seg_len, torch.int32),
                  ("row_off", row_off, torch.int64))
    if hi.shape != lo.shape or hi.stride(0) != lo.stride(0) or out.dim() != 1:
        raise ValueError(f"sim_segments: expected hi and lo [n, d] of one row stride and a flat out, got {list(hi.shape)}, {list(lo.shape)}, {list(out.shape)}")
    check(lib.gp_sim_segments_f16x3(_ptr(hi), _ptr(lo), hi.stride(0), hi.shape[1], _ptr(anchor_row), _ptr(seg_first), _ptr(seg_len), _ptr(row_off),
                                    a, int(max_len), _ptr(out), _stream()), "gp_sim_segments_f16x3")
    return out


def sampler_select_segments(sim, row_off, row_len, row_base, anchor_idx, k, max_len):
    """positive i64 [A], macro i64 [A, k] of the ragged rows of sim (gp_sampler_select_segments: sampler_select's kernel with a row
    descriptor): row a = sim[row_off[a] : row_off[a] + row_len[a]], element j standing for index row_base[a] + j; anchor_idx and the
    results are such indices.  sim is not written."""
    lib = _lib.load()
    _chk(sim, torch.float32, "sim")
    a = anchor_idx.shape[0]
    _segment_rows("sampler_select_segments", a, ("row_off", row_off, torch.int64), ("row_len", row_len, torch.int32), ("row_base", row_base, torch.int32),
                  ("anchor_idx", anchor_idx, torch.int64))
    positive = torch.empty(a, dtype=torch.int64, device=sim.device)
    macro = torch.empty((a, k), dtype=torch.int64, device=sim.device)
    check(lib.gp_sampler_select_segments(_ptr(sim), _ptr(row_off), _ptr(row_len), _ptr(row_base), a, int(max_len), _ptr(anchor_idx), int(k),
                                         _ptr(positive), _ptr(macro), _stream()), "gp_sampler_select_segments")
    return positive, macro


def sampler_micro_segments(sim, row_off, seg_first, seg_len, nbr, positive, num_micro):
    """micro i64 [A, num_micro]: of nbr i32 [A, K] (key rows) the num_micro of lowest similarity in the anchor's ragged row, ascending
    by (value, slot); a neighbour equal to positive[a] counts as +inf (gp_sampler_micro_segments)."""
    lib = _lib.load()
    _chk(sim, torch.float32, "sim"), _chk(nbr, torch.int32, "nbr")
    a = positive.shape[0]
    _segment_rows("sampler_micro_segments", a, ("row_off", row_off, torch.int64), ("seg_first", seg_first, torch.int32), ("seg_len", seg_len, torch.int32),
                  ("positive", positive, torch.int64))
    if nbr.dim() != 2 or nbr.shape[0] != a:
        raise ValueError(f"sampler_micro_segments: expected nbr [{a}, K], got {list(nbr.shape)}")
    micro = torch.empty((a, num_micro), dtype=torch.int64, device=sim.device)
    check(lib.gp_sampler_micro_segments(_ptr(sim), _ptr(row_off), _ptr(seg_first), _ptr(seg_len), _ptr(nbr), nbr.stride(0), nbr.shape[1],
                                        _ptr(positive), a, int(num_micro), _ptr(micro), _stream()), "gp_sampler_micro_segments")
    return micro


def normalize_split_f16(x, n_pad=None, eps=1e-12):
    """(hi, lo) f16 [n_pad, d] of F.normalize(x, dim=1); rows beyond x's are zero (gp_normalize_split_f16)."""
    lib = _lib.load()
    n, d = x.shape
    n_pad = n if n_pad is None else n_pad
    hi = torch.empty((n_pad, d), dtype=torch.float16, device=x.device)
    lo = torch.empty((n_pad, d), dtype=torch.float16, device=x.device)
    check(lib.gp_normalize_split_f16(_ptr(x), x.stride(0), int(d), n, int(n_pad), float(eps), _ptr(hi), _ptr(lo), hi.stride(0), _stream()),
          "gp_normalize_split_f16")
    return hi, lo


class WgradPlan:
    """Pair lists of one voxel set in the layout of gp_conv_wgrad_f16x3 (shared by every 3x3x3 layer of a step)."""

    def __init__(self, pair_in, pair_out, segs, seg_off, num_segments, nv):
        self.pair_in, self.pair_out, self.segs, self.seg_off, self.num_segments, self.nv = pair_in, pair_out, segs, seg_off, num_segments, nv
        self.workspace = None


def wgrad_plan_build(offset_pairs, nv, steps_per_segment=128):
    """offset_pairs: list over the kernel offsets of (out_rows i64, in_rows i64) device tensors (host knows the sizes)."""
    dev = offset_pairs[0][0].device
    pin, pout, segs, seg_off = [], [], [], [0]
    step0 = 0
    for k, (out_rows, in_rows) in enumerate(offset_pairs):
        n = int(out_rows.numel())
        pad = (-n) % 32
        pin.append(in_rows.to(torch.int32))
        pout.append(out_rows.to(torch.int32))
        if pad:
            pin.append(torch.zeros(pad, dtype=torch.int32, device=dev))
            pout.append(torch.full((pad,), nv, dtype=torch.int32, device=dev))
        steps = (n + pad) // 32
        for s in range(0, steps, steps_per_segment):
            segs.append((k, step0 + s, min(steps_per_segment, steps - s), 0))
        seg_off.append(len(segs))
        step0 += steps
    return WgradPlan(torch.cat(pin).contiguous(), torch.cat(pout).contiguous(),
                     torch.tensor(segs, dtype=torch.int32, device=dev).contiguous(),
                     torch.tensor(seg_off, dtype=torch.int32, device=dev), len(segs), nv)


def kernel_map_pairs(nbr_map):
    """The (output row, input row) pairs of every kernel offset of nbr_map i32 [kv, nv] in offset-major, row-ascending order:
    (offset i64 [P], out_rows i64 [P], in_rows i64 [P], counts: host list of kv ints).  Two host syncs for the whole map (a per-offset
    torch.nonzero costs one each: 27 syncs with the GPU idle at the head of every training step)."""
    kv, nv = nbr_map.shape
    kk, rr = torch.nonzero(nbr_map >= 0, as_tuple=True)
    counts = readback(torch.bincount(kk, minlength=kv))
    in_rows = nbr_map.reshape(-1)[kk * nv + rr].long()
    return kk, rr, in_rows, [int(c) for c in counts]


def wgrad_plan_from_pairs(kk, out_rows, in_rows, counts, nv, steps_per_segment=128):
    """wgrad_plan_build for the pair arrays of kernel_map_pairs: same layout (every offset padded to a multiple of 32 pairs with
    (in 0, out nv)), built with a handful of device operations instead of four per offset."""
    dev = out_rows.device
    shift, segs, seg_off = [], [], [0]
    base = cum = step0 = 0
    for k, n in enumerate(counts):
        pad = (-n) % 32
        shift.append(base - cum)
        steps = (n + pad) // 32
        for s in range(0, steps, steps_per_segment):
            segs.append((k, step0 + s, min(steps_per_segment, steps - s), 0))
        seg_off.append(len(segs))
        step0 += steps
        base += n + pad
        cum += n
    pin = torch.zeros(max(base, 1), dtype=torch.int32, device=dev)
    pout = torch.full((max(base, 1),), nv, dtype=torch.int32, device=dev)
    if cum:
        dest = torch.arange(cum, device=dev) + torch.tensor(shift, dtype=torch.int64, device=dev)[kk]
        pin[dest] = in_rows.to(torch.int32)
        pout[dest] = out_rows.to(torch.int32)
    return WgradPlan(pin, pout, torch.tensor(segs, dtype=torch.int32, device=dev).reshape(-1, 4).contiguous(),
                     torch.tensor(seg_off, dtype=torch.int32, device=dev), len(segs), nv)


def conv_wgrad_f16x3(x_split, y_split, plan, cin_pad, cin_out, cout, inv_scale=None, out=None):
    """x_split (hi, lo) f16 [nv, >=cin_pad]; y_split (hi, lo) f16 [nv+1, >=cout] whose last row is zero.
    out: contiguous fp32 [kv, cin_out, cout] to receive dW (e.g. a slice of a gradient bucket: sharding.GradientBuckets.view)."""
    lib = _lib.load()
    xh, xl = x_split
    yh, yl = y_split
    assert yh.shape[0] == plan.nv + 1 and xh.shape[0] >= plan.nv
    need = lib.gp_conv_wgrad_workspace_bytes(plan.num_segments, int(cin_pad), int(cout))
    if plan.workspace is None or plan.workspace.numel() < need:
        plan.workspace = _ws(need, xh.device)
    kv = plan.seg_off.shape[0] - 1
    dw = out if out is not None else torch.empty((kv, cin_out, cout), dtype=torch.float32, device=xh.device)
    assert dw.shape == (kv, cin_out, cout) and dw.is_contiguous() and dw.dtype == torch.float32
    check(lib.gp_conv_wgrad_f16x3(_ptr(xh), _ptr(xl), xh.stride(0), _ptr(yh), _ptr(yl), yh.stride(0), _ptr(plan.pair_in),
                                  _ptr(plan.pair_out), _ptr(plan.segs), plan.num_segments, _ptr(plan.seg_off), kv, int(cin_pad),
                                  int(cin_out), int(cout), _ptr(inv_scale), _ptr(dw), _ptr(plan.workspace), plan.workspace.numel(),
                                  _stream()), "gp_conv_wgrad_f16x3")
    return dw


# ------------------------------------------------------------------------------------------ SURVEY 8(f)-3
def fused_decode(mask_chunk, feat, vox_ind, mode, row_keep=None):
    """Rows of a fused-feature file for the voxel representatives (gp_fused_decode; dataset/feature_loader.py:113-192).
    mask_chunk bool/u8 [N], feat [rows, D] (fp16 or fp32), vox_ind i64 [Nv], row_keep bool/u8 [rows] or None.
    mode 0: (feat rows of the kept voxels, compact [n_sel, D]; mask bool [Nv]) -- one host sync for n_sel;
    mode 1: (one row per voxel [Nv, D], zeros outside the chunk; mask bool [Nv])."""
    lib = _lib.load()
    dev = feat.device
    mc = mask_chunk.to(torch.uint8).contiguous()
    rk = row_keep.to(torch.uint8).contiguous() if row_keep is not None else None
    feat = feat.contiguous()
    vox_ind = vox_ind.to(torch.int64).contiguous()
    n, nv = mc.shape[0], vox_ind.shape[0]
    out = torch.empty((nv,) + tuple(feat.shape[1:]), dtype=feat.dtype, device=dev)
    mask_out = torch.empty(nv, dtype=torch.uint8, device=dev)
    n_sel = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = _ws(lib.gp_fused_decode_workspace_bytes(n, nv), dev)
    row_bytes = feat[0].numel() * feat.element_size()
    check(lib.gp_fused_decode(_ptr(mc), n, _ptr(rk), _ptr(feat), feat.shape[0], row_bytes, _ptr(vox_ind), nv, int(mode), _ptr(out),
                              _ptr(mask_out), _ptr(n_sel), _ptr(ws), ws.numel(), _stream()), "gp_fused_decode")
    kept, in_chunk = (int(v) for v in n_sel.tolist())                # the one host sync (a loader item, off the scene's hot path)
    if in_chunk != feat.shape[0]:
        # the host formulation (reference: dataset/feature_loader.py:141-190) fails on such a file; so does the device path
        raise ValueError(f"fused-feature file: mask_full selects {in_chunk} points but feat holds {feat.shape[0]} rows")
    if mode == 0:
        out = out[:kept]
    return out, mask_out.bool()


# ------------------------------------------------------------------------------------------ fused-feature files from batched clouds
FUSE_FORMS = {"merged": 0, "chunk": 1}                      # the two-key and the three-key file of dataset/feature_loader.py:113-192
FUSE_ELEM = {torch.float32: _lib.GP_ELEM_F32, torch.float16: _lib.GP_ELEM_F16}
FUSE_MAX_FILES = 16


def fuse_state_bytes(n, num_files):
    return int(_lib.load().gp_fuse_state_bytes(int(n), int(num_files)))


def fuse_workspace_bytes(n, num_files, n_split_points=None):
    return int(_lib.load().gp_fuse_workspace_bytes(int(n), int(num_files), int(n_split_points or 0)))


def fuse_dense_workspace_bytes(n):
    return int(_lib.load().gp_fuse_dense_workspace_bytes(int(n)))


def _fuse_points(who, points):
    _chk(points, torch.float64, "points")
    if points.dim() != 2 or points.shape[1] != 4 or not 1 <= points.shape[0] < 2 ** 31 - 1:
        raise ValueError(f"{who}: expected points [1 <= n < 2^31 - 1, 4], got {list(points.shape)}")
    return points.shape[0]


class FusePlan:
    """What gp_fuse_plan writes: mask_full u8 [num_files, n], state (opaque, for fuse_write), status i64 [8] = (rows whose batch index
    is no integer in 0..65535, 0, 0, top batch index, rows of feat over all files, 0, 0, 0); and what it was called with."""

    def __init__(self, n, seen, num_files, form, mask_full, state, status):
        self.n, self.seen, self.num_files, self.form = n, seen, num_files, form
        self.mask_full, self.state, self.status = mask_full, state, status


def fuse_plan(points, seen, n_split_points=None, num_files=1, seed=0, form="merged", buffers=None, workspace=None):
    """gp_fuse_plan, no sync: points f64 [n,4] (the batch column is read), seen u8 [n].  n_split_points None: every file holds the whole
    entry.  buffers: optional caller-owned mask_full / state (uint8 of gp_fuse_state_bytes) / status; workspace: uint8 of at least
    fuse_workspace_bytes(n, num_files, n_split_points).  -> FusePlan."""
    lib = _lib.load()
    who = "fuse_plan"
    n = _fuse_points(who, points)
    _chk(seen, torch.uint8, "seen")
    nf, split, seed = int(num_files), int(n_split_points or 0), int(seed)
    if seen.shape != (n,):
        raise ValueError(f"{who}: expected seen [{n}], got {list(seen.shape)}")
    if not 1 <= nf <= FUSE_MAX_FILES or form not in FUSE_FORMS or (n_split_points is not None and split < 1) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: num_files={num_files} outside 1..{FUSE_MAX_FILES}, form={form!r} not in {sorted(FUSE_FORMS)}, "
                         f"n_split_points={n_split_points} < 1 or seed={seed} outside 0..2^64-1")
    dev = points.device
    sb = int(lib.gp_fuse_state_bytes(n, nf))
    got = _outputs(who, {"mask_full": (torch.uint8, (nf, n)), "status": (torch.int64, (8,))}, buffers, dev)
    state = (buffers or {}).get("state")
    state = _ws(sb, dev) if state is None else _chk(state, torch.uint8, "state")
    ws = _ws(lib.gp_fuse_workspace_bytes(n, nf, split), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_fuse_plan(_ptr(points), n, _ptr(seen), nf, split, seed, FUSE_FORMS[form], _ptr(got["mask_full"]), _ptr(state), state.numel(),
                           _ptr(got["status"]), _ptr(ws), ws.numel(), _stream()), "gp_fuse_plan")
    return FusePlan(n, seen, nf, form, got["mask_full"], state, got["status"])


def fuse_write(plan, features, num_entries, total_rows, dtype=torch.float16, buffers=None):
    """gp_fuse_write, no sync: features fp32 or fp16 [n, D] (contiguous; any element-aligned base) -> (feat dtype [total_rows, D], mask
    u8 [total_rows] or None (merged form), offsets i64 [num_files, num_entries + 1]).  num_entries / total_rows: status[3] + 1 /
    status[4] of the plan.  buffers: optional caller-owned feat / mask / offsets."""
    lib = _lib.load()
    who = "fuse_write"
    if features.dtype not in FUSE_ELEM or not features.is_cuda or not features.is_contiguous() or features.dim() != 2 or \
            features.shape[0] != plan.n or features.shape[1] < 1:
        raise ValueError(f"{who}: expected contiguous CUDA fp32 or fp16 features [{plan.n}, D >= 1], got {features.dtype} "
                         f"{list(features.shape)} cuda={features.is_cuda} contig={features.is_contiguous()}")
    if dtype not in FUSE_ELEM:
        raise ValueError(f"{who}: dtype={dtype} (torch.float16 or torch.float32)")
    B, R, D, nf, dev = int(num_entries), int(total_rows), features.shape[1], plan.num_files, features.device
    want = {"feat": (dtype, (R, D)), "offsets": (torch.int64, (nf, B + 1))}
    if plan.form == "chunk":
        want["mask"] = (torch.uint8, (R,))
    got = _outputs(who, want, buffers, dev)
    check(lib.gp_fuse_write(_ptr(features), FUSE_ELEM[features.dtype], D, _ptr(plan.seen), plan.n, nf, _ptr(plan.state), plan.state.numel(), B,
                            _ptr(got["feat"]) if R else None, FUSE_ELEM[dtype], R, _ptr(got["mask"]) if R and "mask" in got else None,
                            _ptr(got["offsets"]), _stream()), "gp_fuse_write")
    return got["feat"], got.get("mask"), got["offsets"]


class FuseBatched:
    """mask_full u8 [num_files, n], feat [R, D], offsets i64 [num_files, B + 1], mask u8 [R] or None, status: the plan's words as a list"""

    def __init__(self, mask_full, feat, offsets, mask, status):
        self.mask_full, self.feat, self.offsets, self.mask, self.status = mask_full, feat, offsets, mask, status


def fuse_batched(points, features, seen, n_split_points=None, num_files=1, seed=0, form="merged", dtype=torch.float16):
    """fuse_plan, ONE read-back (the plan's status: it carries the sizes that allocate feat and offsets), fuse_write.  -> FuseBatched;
    rows whose batch index is no integer in 0..65535 (status[0] of them) are in no file."""
    plan = fuse_plan(points, seen, n_split_points, num_files, seed, form)
    status = readback(plan.status)
    feat, mask, offsets = fuse_write(plan, features, status[3] + 1, status[4], dtype)
    return FuseBatched(plan.mask_full, feat, offsets, mask, status)


def fuse_dense(points, mask_full, feat, buffers=None, workspace=None):
    """gp_fuse_dense, no sync: points f64 [n,4], mask_full u8 [n] (one file set), feat fp16 or fp32 [rows, D] -> (out fp32 [n, D]:
    feat's rows at the points with mask_full, zero rows elsewhere; status i64 [8]: [0] bad batch rows, [3] top batch, [4] the rows
    mask_full selects, to be compared with feat's)."""
    lib = _lib.load()
    who = "fuse_dense"
    n = _fuse_points(who, points)
    _chk(mask_full, torch.uint8, "mask_full")
    if mask_full.shape != (n,):
        raise ValueError(f"{who}: expected mask_full [{n}], got {list(mask_full.shape)}")
    if feat.dtype not in FUSE_ELEM or not feat.is_cuda or not feat.is_contiguous() or feat.dim() != 2 or feat.shape[1] < 1:
        raise ValueError(f"{who}: expected contiguous CUDA fp32 or fp16 feat [rows, D >= 1], got {feat.dtype} {list(feat.shape)} "
                         f"cuda={feat.is_cuda} contig={feat.is_contiguous()}")
    R, D, dev = feat.shape[0], feat.shape[1], points.device
    got = _outputs(who, {"out": (torch.float32, (n, D)), "status": (torch.int64, (8,))}, buffers, dev)
    ws = _ws(lib.gp_fuse_dense_workspace_bytes(n), dev) if workspace is None else _chk(workspace, torch.uint8, "workspace")
    check(lib.gp_fuse_dense(_ptr(points), n, _ptr(mask_full), _ptr(feat) if R else None, FUSE_ELEM[feat.dtype], R, D, _ptr(got["out"]),
                            _ptr(got["status"]), _ptr(ws), ws.numel(), _stream()), "gp_fuse_dense")
    return got["out"], got["status"]
