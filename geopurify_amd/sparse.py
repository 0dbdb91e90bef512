"""Batched point clouds on the device, the second way into the library beside the reference's 20-tuple: quantisation (points in,
unique voxels and an inverse map out, with autograd back to the points), per-entry exact kNN, and the purifying step itself over
ME-style SparseTensors.

Quantisation is the step the reference writes by hand in front of the student (models/affinity_module.py:1192-1212: torch.unique(...,
return_inverse=True) + torch_scatter.scatter_mean + ME.SparseTensor(features, batched_coordinates), then
s_output.F[sample_to_voxel_map]) and every MinkowskiEngine user gets from SparseTensor(quantization_mode=...).  The purifying step is
evaluate_scene's (:1547-1587): exact kNN, sharpened cosine affinity, 19 applications of the operator -- here for every batch entry at
once, entries never mixing.  The full chain, the points, poses, depths and VLM feature maps of several scenes in, purified per-point
features out:

    lifted = lift(points, Views(maps, view_entry, world_to_camera, intrinsics, depth))   # points [N,4] = batch, world x, y, z
    q = quantize(points, lifted.features, mode="average", quantization_size=voxel)       # duplicates allowed
    x = SparseTensor(features=q.features, coordinates=q.coordinates)
    y = affinity_pool(x, student(x))                            # or purify(student, x, feature_dim=D): the two calls in one
    per_point = y.F[q.inverse_mapping]
    seg = segment(y, text, scale, labels=point_labels, inverse_mapping=q.inverse_mapping)   # labels per point, (I, O, T) counts per scene

and, where the cloud that is scored (a benchmark's vertices) is not the cloud that was lifted (a subsample, another reconstruction),
the results carried over: the k nearest working points of every vertex inside its entry, exactly, and rows interpolated through them

    nb = knn_query(points, benchmark_vertices, 3)
    feat = interpolate(y.F, nb, index=q.inverse_mapping)            # purified features on the benchmark's vertices
    pred = interpolate(seg.pred, nb, index=q.inverse_mapping)       # nearest working point's voxel prediction

and, to train on the cloud that is scored, the same call with gradients to the rows it reads (exact and reproducible: no atomics):

    t = nb.transpose(q.inverse_mapping, y.F.shape[0])               # the lists inverted, once for a training run
    feat = interpolate(purify(student, x, differentiable=True).F, nb, index=q.inverse_mapping, differentiable=True, transpose=t)

or, with the VLM producing its maps a batch of views at a time (the reference's own loop, :365-449), the same start without ever
holding more than one batch of maps:

    stream = LiftStream(points, feature_dim=D, mode="bilinear")
    for maps, view_entry, world_to_camera, intrinsics, depth in vlm_batches:
        stream.add(Views(maps, view_entry, world_to_camera, intrinsics, depth, image_shape=(H, W)))
    lifted = stream.finish()                                    # the bits of lift on all the views; add / finish may go on

or, from the X-Decoder form of the VLM's outputs (masks, class logits, mask embeddings: the reference's default lift), the same chain with

    lifted = lift_masks(points, MaskViews(pred_masks, pred_logits, mask_embed, view_entry, world_to_camera, intrinsics, depth,
                                          image_shape=(H, W)), text_embed, logit_scale)   # -> .features, .text_features (normalised)

or, with the X-Decoder producing its outputs a batch of views at a time (the reference's own loop, :495-640), without ever holding
more than one batch of masks:

    stream = LiftMasksStream(points, text_embed, logit_scale)
    for pred_masks, pred_logits, mask_embed, view_entry, world_to_camera, intrinsics, depth in vlm_batches:
        stream.add(MaskViews(pred_masks, pred_logits, mask_embed, view_entry, world_to_camera, intrinsics, depth, image_shape=(H, W)))
    lifted = stream.finish()                                    # the bits of lift_masks on all the views; add / finish may go on

or, the third start of the chain, from integer label maps (a 2D segmenter's per-pixel predictions or 2D ground truth, the loader's
label_2ds): the majority vote per point, its histogram, and the labels that segment_loss / purified_loss and segment take

    voted = lift_labels(points, LabelViews(label_maps, view_entry, world_to_camera, intrinsics, depth), num_classes=C)
    # -> .labels i64 [N] (255 where nothing voted), .votes i32 [N,C]; LiftLabelsStream(points, C).add(...) / .finish() in chunks

The student reads feature_dim + 6 input columns: the lifted features, then the geometry columns -- vertex colours in [0,1] and vertex
normals (dataset/data_loader_ablation.py:162-163).  Colours come with every dataset (or from lift on the RGB images as 3-channel
maps); the normals come from the scans' meshes the reference's way (models/utils/mapping_util.py:9-29, bit for bit), or, for a cloud
without faces, from the neighbourhoods of its voxels:

    normals = mesh_normals(points, faces)                       # faces: rows of points; all entries in one call
    normals = estimate_normals(points, quantization_size=voxel, k=16, toward=camera_centres).normals   # no faces: poses and a cloud
    q = quantize(points, torch.cat([lifted.features, colors, normals.float()], 1), mode="average", quantization_size=voxel)
    x = SparseTensor(features=q.features, coordinates=q.coordinates)      # x.F = cat([lifted.features, colors, normals], 1), averaged
    y = purify(student, x, feature_dim=D)

The chain also has an end and a fourth start on disk: the fused-feature files that dataset/feature_loader.py:113-192 reads (lift once,
then train and evaluate from files many times without the VLM)

    chunks = fuse(points, lifted, n_split_points=80000, num_files=5)   # per scene and file a random chunk of the points, fp16 rows
    chunks.save(out_dir, scene_names)                           # {scene}_{k}.pt, what FusedFeatureLoader loads; chunks.file(b, k): one dict
    feats, mask = load_fused(points, files).dense()             # files back in: fp32 [N,D] (zero rows outside the file), ready for quantize

The chain's end in image space runs the other way, from points back to their views (the reference's visualize_2d_semantic,
models/utils/visualization.py:15-59, paints 3D predictions into a view; scoring against the loader's label_2ds and pseudo-label or
purified feature maps for a 2D model need the same): per view and pixel the front-most visible point of the view's entry

    r = render_rows(points, view_entry, world_to_camera, intrinsics, (H, W), depth="render")   # .rows i32 [V,H,W], -1: no owner
    pred_maps = r.labels(seg.pred, index=q.inverse_mapping)     # per-voxel predictions painted per view, 255 where nothing lands
    feat_maps = r.features(y.F, index=q.inverse_mapping, dtype=torch.float16, views=slice(0, 8))   # [8,H,W,D], channels last
    counts = segment_views(r, seg.pred, label_2ds, view_entry, C, index=q.inverse_mapping)        # (I, O, T) per entry, in image space

and the objective the student is trained with (models/affinity_module.py:1099-1136, :1192-1233 for several scenes at once):

    pairs = sample_pairs(x.C, teacher)                          # per entry: anchors, their positive, 48 global + 15 local negatives
    loss = info_nce(student(pairs.subset(x)), pairs)            # or contrastive_loss(student, x, teacher): the three calls in one
    loss.backward()

and the loss on the purified features, labels per voxel or per point, ground truth or the VLM's own segment(x, ...).pred:

    loss = segment_loss(purify(student, x, differentiable=True), text, scale, labels=point_labels, inverse_mapping=q.inverse_mapping)
    loss.backward()                                             # or purified_loss(student, x, text, scale, labels=...): the two calls in one

Every link carries gradients when asked to: affinity_pool(x, student(x), differentiable=True) -- or purify(student, x,
differentiable=True) -- puts y.F into the autograd graph, so a loss on the purified features reaches the student's parameters, x.F and
through the quantiser the points' features (ops.pool_transpose_build, pool_ell_transpose, pool_ell_wgrad, affinity_softmax_backward,
l2norm_rows_backward).  The default takes no gradients, like the reference's evaluate_scene; segment (labels and counts) never does.

All four lifts read the VLM's large outputs -- the feature maps [V,D,h,w], the mask logits [V,Q,h,w] -- in fp32, fp16 or bf16 as they are:
a VLM run under autocast hands over half tensors, and no fp32 copy of them is made.  The kernels convert every loaded element to fp32
(exact for both half types) and sum in fp32, so the result is, bit for bit, that of the same call on the caller's own upcast copy.
All four lifts decide visibility against the caller's depth maps, by p_z > 0 alone (depth=None), or -- depth="render" -- against depth
maps rendered from the points themselves, the reference's way when it has poses and a reconstructed cloud but no sensor depth
(models/utils/fusion_util.py:126-130):

    depth = render_depth(points, view_entry, world_to_camera, intrinsics, (H, W))         # fp64 [V,H,W]; or Views(..., depth="render")

render_depth is ops.render_depth_batched: the z-buffer of every view over the points of its entry, one call for all entries; the
streams render a chunk's views from their own entry tables (ops.render_depth_stream) into a chunk-sized scratch buffer.
lift is the reference's lift_lseg_features (models/affinity_module.py:404-452) with the point -> pixel mapping of
models/utils/fusion_util.py:45-147 and the loader's view-drop rule (dataset/data_loader_ablation.py:254-288), for all entries and all
views in one call of ops.lift_batched (the maps pixel-major in their own dtype), then ops.gather_rows for the fill.
LiftStream is the same lift resumable over chunks of views: ops.lift_stream_begin (the entry tables, once), ops.lift_stream_add per chunk
(fp32 sums continued in view order), ops.lift_stream_finish (divide and fill; a snapshot), ops.gather_rows.
lift_masks is the reference's lift_xdecoder_features (models/affinity_module.py:455-714: per-view mask-embedding lift, in-view nearest
fill, consensus top-3 fusion, scene-level fill) with the same mapping and drop rule, for all entries and any number of views per entry:
ops.lift_masks_batched_lists (ordered visible lists), ops.segment_tables, ops.lift_masks_batched, ops.gather_rows; two read-backs.
LiftMasksStream is the same lift resumable over chunks of views: ops.lift_masks_stream_begin (the entry tables and the per-entry view
counters, once), per chunk ops.lift_masks_batched_lists around ops.lift_masks_stream_sizes (the one read-back), ops.segment_tables and
ops.lift_masks_stream_add (segments and in-view fill over a chunk-sized workspace, one (row, segment) record per visible pair kept),
ops.lift_masks_stream_finish (slot lists from the records, fusion, fill; a snapshot), ops.gather_rows.
lift_labels has no counterpart in the reference; it votes integer label maps onto the points with lift's geometry (the mapper, the
drop rule) in one call of ops.lift_labels_batched, one read-back; LiftLabelsStream is the same vote over chunks of views
(ops.lift_labels_stream_begin / _add / _finish), order-free because the sums are integers.
fuse has no counterpart in the reference either (it ships the reader and the writer's settings, config/fusion_scannet.yaml:34-35): ops.fuse_plan
(entry tables, an exact radix select of each (file, entry)'s threshold key, flags and scans per file), one read-back, ops.fuse_write
(every row loaded once, converted once, stored to each file that holds it); FusedChunks.dense is ops.fuse_dense.
render_rows is ops.render_rows (the entry tables, with "render" the z-buffer of render_depth, then two order-free passes of integer
atomic minima: the bit pattern of p_z, then the row), one read-back; Rendered.features is ops.render_gather, Rendered.labels torch
indexing on the small maps, segment_views a compaction in torch around ops.iou_hist_batched.
mesh_normals is ops.mesh_normals_batched (one lane per face, a stable radix sort of (vertex, face) pairs, one lane per vertex), one
read-back; estimate_normals is quantize, knn and ops.knn_normals (fp64 covariance and a Jacobi eigen-solve in registers, the lists
staged through LDS), then torch indexing by the inverse mapping.
knn_query is ops.knn_query (the points' entry table, per entry a bounding box and a uniform grid, a wave per query walking the grid's
shells in the (d^2, row) order of lift's fill, an entry scan for the queries the walk leaves), one read-back; interpolate is
ops.knn_interpolate (a wave per query row, weights in fp64, sums in fp32 in list order), no read-back; with differentiable=True its
backward is ops.knn_interpolate_weights (the forward's weights again, by the forward's device code), ops.knn_interpolate_transpose (a
stable radix sort of (row of values, flat slot) pairs; Neighbors.transpose builds it once for a run) and ops.knn_interpolate_backward (a
wave per row of values adding its references in ascending flat slot: no float atomics, the same bits every time).
The indices come from ops.quantize_batched (the key and order of ops.coords_order_batched: batch << 48 | morton(xyz - min)); the
features are reduced by the kernels the pipeline already has, ops.scatter_mean_csr ("average") and ops.gather_rows ("subsample").
The neighbour lists come from ops.knn_batched over the same sorted keys; affinity and pooling are ops.affinity_softmax and the
pooling families of HotPath, applied in the key order.  segment is the per-scene tail of run/validation.py:413-439 for all entries at
once: ops.classify_argmax(_gemm), the zero-row fill by ops.nn1_batched inside each entry, ops.iou_hist_batched.  sample_pairs is
ops.normalize_split_f16 on the teacher rows in the key order, then per chunk of anchors ops.sim_segments (the similarity inside each
anchor's entry, a ragged buffer), ops.sampler_select_segments and ops.sampler_micro_segments; info_nce is ops.infonce_weighted_fwd_bwd.  segment_loss is
ops.segment_loss_unit_rows and ops.segment_loss_items, then per chunk of rows the exact-fp32 GEMM of ops.sparse_conv around
ops.segment_loss_rows, ops.segment_loss_reduce and ops.l2norm_rows_backward.
"""
import torch

from . import ops
from ._lib import GP_KNN_MAX_K, GP_KNN_QUERY_MAX_K

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


# ------------------------------------------------------------------------------------------ the 2D -> 3D lift
LIFT_MODES = ("nearest", "bilinear")


class Views:
    """The views of a batch of scenes: features fp32, fp16 or bf16 [V,D,h,w] (the frozen VLM's maps, NCHW contiguous or
    torch.channels_last; half maps are read as they are, with no fp32 copy, and give the bits of their fp32 copy; fp64 and other
    floating dtypes are upcast to fp32), view_entry integer [V] (the batch entry a view looks at), world_to_camera fp64 [V,4,4], intrinsics fp64
    [V,4] = fx, fy, cx, cy at the image size, depth fp64 [V,H,W], None (a point is visible where it projects inside the image with
    p_z > 0: no occlusion) or the string "render" (the depth maps are rendered from the points themselves, see render_depth: occlusion
    without sensor depth), image_shape = (H, W) shared by all views (default: the maps' (h, w)).
    world_to_camera is the row-major world->camera matrix: the transpose of the reference's world_view_transform, or the inverse of a
    camera-to-world matrix.  lift checks the fields."""

    def __init__(self, features, view_entry, world_to_camera, intrinsics, depth=None, image_shape=None):
        self.features, self.view_entry, self.world_to_camera, self.intrinsics = features, view_entry, world_to_camera, intrinsics
        self.depth, self.image_shape = depth, image_shape


class Lifted:
    """features fp32 [N,D] in the points' row order, seen bool [N] (some kept view sees the point), count i32 [N] (the kept views that
    see it), view_count i64 [V] (the points of its entry a view sees), view_keep bool [V] (the view passed the drop rule)."""

    def __init__(self, features, seen, count, view_count, view_keep):
        self.features, self.seen, self.count, self.view_count, self.view_keep = features, seen, count, view_count, view_keep


def _shape_of(t):
    return list(t.shape) if torch.is_tensor(t) else type(t).__name__


RENDER = "render"                                           # Views.depth / MaskViews.depth: render the depth maps from the points


def _depth_kind(depth):
    """none / tensor / render: the three ways a lift decides visibility"""
    return "none" if depth is None else (RENDER if isinstance(depth, str) else "tensor")


def _check_depth(who, Dp, V, H, W):
    """views.depth: fp64 [V,H,W], None, or the string "render" and no other"""
    if isinstance(Dp, str):
        if Dp != RENDER:
            raise ValueError(f"{who}: views.depth={Dp!r}: expected fp64 [{V}, {H}, {W}] (image_shape), None or the string {RENDER!r}")
    elif Dp is not None and (not torch.is_tensor(Dp) or Dp.shape != (V, H, W) or Dp.dtype != torch.float64):
        raise ValueError(f"{who}: views.depth must be fp64 [{V}, {H}, {W}] (image_shape) or None, got "
                         f"{(list(Dp.shape), Dp.dtype) if torch.is_tensor(Dp) else type(Dp).__name__}")


def _check_points(who, P):
    if not torch.is_tensor(P) or P.dim() != 2 or P.shape[1] != 4:
        raise ValueError(f"{who}: points must be [N, 4] (batch, x, y, z), got {_shape_of(P)}")
    if P.dtype not in (torch.float64, torch.float32):
        raise ValueError(f"{who}: points must be fp64 or fp32, got {P.dtype}")
    n = P.shape[0]
    if n == 0 or n >= 2 ** 31:
        raise ValueError(f"{who}: {n} points outside 1..2^31-1")


def _check_poses(who, name, V, E, M, K):
    """view_entry, world_to_camera and intrinsics of V views; name: how the message calls their owner ("views." or "")"""
    if not _is_int_tensor(E) or E.shape != (V,):
        raise ValueError(f"{who}: {name}view_entry must be an integer tensor [{V}], got "
                         f"{(list(E.shape), E.dtype) if torch.is_tensor(E) else type(E).__name__}")
    if not torch.is_tensor(M) or M.shape != (V, 4, 4) or M.dtype != torch.float64:
        raise ValueError(f"{who}: {name}world_to_camera must be fp64 [{V}, 4, 4], got {(list(M.shape), M.dtype) if torch.is_tensor(M) else type(M).__name__}")
    if not torch.is_tensor(K) or K.shape != (V, 4) or K.dtype != torch.float64:
        raise ValueError(f"{who}: {name}intrinsics must be fp64 [{V}, 4] (fx, fy, cx, cy), got "
                         f"{(list(K.shape), K.dtype) if torch.is_tensor(K) else type(K).__name__}")


def _check_visibility_options(who, cut_bound, vis_thres, min_visible, max_visible):
    """the options every lift decides visibility and the view-drop rule with"""
    if not _is_count(cut_bound, 0) or cut_bound >= 2 ** 31:
        raise ValueError(f"{who}: cut_bound={cut_bound!r} must be an integer >= 0")
    if isinstance(vis_thres, bool) or not isinstance(vis_thres, (int, float)) or vis_thres != vis_thres:
        raise ValueError(f"{who}: vis_thres={vis_thres!r} must be a number")
    if not _is_count(min_visible, 0) or not (max_visible is None or _is_count(max_visible, 0)):
        raise ValueError(f"{who}: min_visible={min_visible!r} / max_visible={max_visible!r} must be integers >= 0 (max_visible may be None)")


def _check_view_count(who, V):
    if V > 65535:
        raise ValueError(f"{who}: {V} views, at most 65535")


def _image_shape(who, name, given, shape, tail=""):
    """shape, the caller's reading of the image_shape it was `given`, as (H, W); tail: what the caller's message says about the pair"""
    if len(shape) != 2 or not all(_is_count(v, 1) and v < 2 ** 31 for v in shape):
        raise ValueError(f"{who}: {name}image_shape must be (H, W), two positive integers{tail}, got {given!r}")
    return shape


def _check_one_device(who, subject, tensors):
    """the last check of every member: all on the GPU of the first (the points)"""
    if not all(t.is_cuda for t in tensors) or any(t.device != tensors[0].device for t in tensors):
        raise ValueError(f"{who}: {subject} must be CUDA tensors on one device (got "
                         f"{' / '.join(str(t.device) for t in tensors)}); there is no CPU path")


def _check_render_views(who, P, E, M, K, image_shape):
    """what render_depth and render_rows check first: the points, the bare view_entry / world_to_camera / intrinsics and image_shape
    -> (V, (H, W))"""
    _check_points(who, P)
    if not _is_int_tensor(E) or E.dim() != 1 or E.shape[0] < 1:
        raise ValueError(f"{who}: view_entry must be an integer tensor [V] with V >= 1, got "
                         f"{(list(E.shape), E.dtype) if torch.is_tensor(E) else type(E).__name__}")
    V = E.shape[0]
    _check_view_count(who, V)
    _check_poses(who, "", V, E, M, K)
    return V, _image_shape(who, "", image_shape, tuple(image_shape) if isinstance(image_shape, (tuple, list)) else ())


# what every member hands to its ops call: written once
def _points64(P):
    return P.detach().to(torch.float64).contiguous()


def _view_args(E, M, K, Dp=None, render=None):
    """-> (view_entry i64, world_to_camera, intrinsics, depth), contiguous and detached.  depth: the tensor, None, or for the string
    "render" what render(view_entry, world_to_camera, intrinsics) makes (without render the string stays: ops.render_rows takes it)"""
    ve, w2c, intr = E.detach().to(torch.int64).contiguous(), M.detach().contiguous(), K.detach().contiguous()
    if isinstance(Dp, str) and render is not None:
        Dp = render(ve, w2c, intr)
    return ve, w2c, intr, Dp.detach().contiguous() if torch.is_tensor(Dp) else Dp


def _render_all(pts, image_hw, cut_bound):
    """depth="render" in a one-call lift, as _view_args takes it: the z-buffer of every view, V * H * W * 8 bytes"""
    return lambda view_entry, w2c, intrinsics: ops.render_depth_batched(pts, view_entry, w2c, intrinsics, image_hw, cut_bound)[0]


def _clamped(max_visible):
    return 2 ** 63 - 1 if max_visible is None else min(max_visible, 2 ** 63 - 1)


def _fill_rows(out, width, nn, D=None):
    """the scene-level fill: the row of its nearest seen point for every row nn names, its own elsewhere (nn None: no fill), cut back
    to D columns where the rows were padded to `width`"""
    feats = out if nn is None else ops.gather_rows(out, width, torch.where(nn >= 0, nn, torch.arange(out.shape[0], device=out.device)))
    return feats if D is None or D == width else feats[:, :D].contiguous()


_LISTS_TORN = "the visible lists do not hold together ({} entries, {} views): the inputs changed during the call"
_STREAM_TORN = ("what the stream keeps does not hold together ({} values of the state, the offsets or the records, {} view positions): it was "
                "overwritten, or the inputs changed during an add")


def _raise_status(who, status, *, num_classes=None, state=False, torn=None):
    """The errors in the words of a member's status read-back (what ops.readback returned), lift's three first, then what the member
    adds: num_classes -- a label vote's samples out of range (word 7); state -- a stream's entry tables out of range (word 6); torn --
    the sentence of a mask lift whose lists (_LISTS_TORN) or kept arrays (_STREAM_TORN) do not hold together (words 6 and 7)."""
    bad_batch, bad_view, nonfinite = status[:3]
    if nonfinite:
        raise ValueError(f"{who}: {nonfinite} rows of points are not finite")
    if bad_batch:
        raise ValueError(f"{who}: {bad_batch} rows have a batch index that is no integer in 0..65535")
    if bad_view:
        raise ValueError(f"{who}: {bad_view} views have a view_entry outside 0..65535")
    if num_classes is not None and status[7]:
        raise ValueError(f"{who}: {status[7]} sampled labels are neither in 0..{num_classes - 1} nor in ignore_labels")
    if state and status[6]:
        raise RuntimeError(f"{who}: {status[6]} values of the stream's entry tables are out of range: the state was overwritten")
    if torn is not None and (status[6] or status[7]):
        raise RuntimeError(f"{who}: {torn.format(status[6], status[7])}")


def _check_lift(who, points, views, mode, cut_bound, vis_thres, min_visible, max_visible):
    """lift's argument checks, in lift's order; views None: those of the points and the options alone (LiftStream's construction).
    -> (V, D, h, w, H, W), or None without views"""
    if mode not in LIFT_MODES:
        raise ValueError(f"{who}: mode={mode!r}, expected one of {LIFT_MODES}")
    if views is not None and not isinstance(views, Views):
        raise ValueError(f"{who}: views must be a Views, got {type(views).__name__}")
    P = points
    _check_points(who, P)
    if views is not None:
        Fm, E, M, K, Dp = views.features, views.view_entry, views.world_to_camera, views.intrinsics, views.depth
        if not torch.is_tensor(Fm) or Fm.dim() != 4 or min(Fm.shape) < 1:
            raise ValueError(f"{who}: views.features must be [V, D, h, w] with V, D, h, w >= 1, got {_shape_of(Fm)}")
        if not Fm.dtype.is_floating_point:
            raise ValueError(f"{who}: views.features must be floating point, got {Fm.dtype}")
        V, D, h, w = Fm.shape
        _check_view_count(who, V)
        _check_poses(who, "views.", V, E, M, K)
        H, W = _image_shape(who, "views.", views.image_shape, (h, w) if views.image_shape is None else tuple(views.image_shape))
        _check_depth(who, Dp, V, H, W)
        if mode == "nearest" and (h, w) != (H, W):
            raise ValueError(f"{who}: mode 'nearest' samples the maps' own pixels: maps of {h} x {w} with image_shape {H} x {W} (use 'bilinear')")
    _check_visibility_options(who, cut_bound, vis_thres, min_visible, max_visible)
    if views is not None and Fm.requires_grad:
        raise ValueError(f"{who}: views.features require grad, but the lift takes no gradients (the VLM is frozen, the reference lifts under "
                         "no_grad); detach them")
    _check_one_device(who, "points and the views' tensors",
                      [P] + ([Fm, E, M, K] + ([Dp] if torch.is_tensor(Dp) else []) if views is not None else []))
    return (V, D, h, w, H, W) if views is not None else None


def _lift_maps(Fm):
    """the maps as the lift kernels read them: fp32, fp16 and bf16 stay what they are (the kernels convert every loaded element to
    fp32, which is exact, so a half map gives the bits of its fp32 copy without that copy existing); fp64 and any other floating
    dtype are upcast to fp32"""
    maps = Fm.detach()
    return maps if maps.dtype in ops.ELEM_TAG else maps.to(torch.float32)


def render_depth(points, view_entry, world_to_camera, intrinsics, image_shape, *, cut_bound=0):
    """The depth maps the reference renders from the cloud itself when it is given no sensor depth (models/utils/fusion_util.py:126-130,
    the ScanNet mapper with depth passed as a str), for all views of all entries in one call, entries never mixing.  points,
    view_entry, world_to_camera and intrinsics as lift takes them (points fp64 or fp32 [N,4], upcast to fp64 first; V views);
    image_shape = (H, W).  -> fp64 [V,H,W]: a pixel holds the smallest p_z > 0.2 among the points of the view's entry that project
    into it (rounded half to even) inside [cut_bound, W - cut_bound) x [cut_bound, H - cut_bound), and 999999 where none does.  A view
    whose entry has no points is 999999 everywhere.  The same bits as ops.render_depth per view on the entry's points, in any row
    order: the minimum is an integer atomic on the fp64 bit pattern, which no arrival order changes.
    This is what depth="render" hands to lift, LiftStream, lift_masks and LiftMasksStream; it holds V * H * W * 8 bytes.
    Inside: ops.render_depth_batched (the entry tables, the fill, the z-buffer kernel).  ValueError before any kernel: lift's refusals
    for these fields; from the ONE status read-back, with lift's messages and precedence: non-finite rows, rows whose batch index is no
    integer in 0..65535, views whose entry is outside 0..65535."""
    who = "render_depth"
    P, E, M, K = points, view_entry, world_to_camera, intrinsics
    V, shape = _check_render_views(who, P, E, M, K, image_shape)
    if not _is_count(cut_bound, 0) or cut_bound >= 2 ** 31:
        raise ValueError(f"{who}: cut_bound={cut_bound!r} must be an integer >= 0")
    _check_one_device(who, "points and the views' tensors", [P, E, M, K])
    with torch.cuda.device(P.device), torch.no_grad():
        depth, status = ops.render_depth_batched(_points64(P), *_view_args(E, M, K)[:3], shape, cut_bound)
        status = ops.readback(status)
    _raise_status(who, status)
    return depth


# ------------------------------------------------------------------------------------------ the chain's end in image space
RENDER_FAR = 999999.0                                       # Rendered.depth where a pixel has no owner (render_depth's value)


class Rendered:
    """What render_rows returns: rows i32 [V,H,W] (the owner's row of points, -1 where nothing covers the pixel), depth fp64 [V,H,W]
    (the owner's p_z, 999999 where rows == -1), view_count i64 [V] (candidates per view: lift's view_count on the same geometry and
    options), pixel_count i64 [V] (pixels with an owner), num_entries (1 + the highest valid batch index), image_shape = (H, W),
    num_points (N: what an index must be long)."""

    def __init__(self, rows, depth, view_count, pixel_count, num_entries, image_shape, num_points):
        self.rows, self.depth, self.view_count, self.pixel_count = rows, depth, view_count, pixel_count
        self.num_entries, self.image_shape, self.num_points = num_entries, image_shape, num_points

    def _index(self, who, index, device):
        if index is None:
            return None
        if not torch.is_tensor(index) or index.dtype != torch.int64 or index.shape != (self.num_points,):
            raise ValueError(f"{who}: index must be an int64 tensor [{self.num_points}] (point -> row, e.g. a quantiser's inverse_mapping), got "
                             f"{(list(index.shape), index.dtype) if torch.is_tensor(index) else type(index).__name__}")
        if index.device != device:
            raise ValueError(f"{who}: index is on {index.device}, the rendered rows on {device}")
        return index.detach().contiguous()

    def labels(self, point_labels, *, fill=255, index=None):
        """Per-point (or, through index, per-row) integer labels painted into the views: -> [V,H,W] of point_labels' dtype, the value
        point_labels[index[rows]] (point_labels[rows] without index) at owned pixels and fill where rows == -1.  index: i64 [N], point
        -> row of point_labels (a quantiser's inverse_mapping, so per-voxel predictions render directly).  Torch indexing: the maps are
        small."""
        who = "Rendered.labels"
        if not _is_int_tensor(point_labels) or point_labels.dim() != 1 or point_labels.shape[0] < 1:
            raise ValueError(f"{who}: point_labels must be an integer tensor [R >= 1], got "
                             f"{(list(point_labels.shape), point_labels.dtype) if torch.is_tensor(point_labels) else type(point_labels).__name__}")
        if isinstance(fill, bool) or not isinstance(fill, int):
            raise ValueError(f"{who}: fill={fill!r} must be an integer")
        index = self._index(who, index, self.rows.device)
        if index is None and point_labels.shape[0] != self.num_points:
            raise ValueError(f"{who}: {point_labels.shape[0]} labels for {self.num_points} points (pass index for labels per row)")
        if point_labels.device != self.rows.device:
            raise ValueError(f"{who}: point_labels is on {point_labels.device}, the rendered rows on {self.rows.device}")
        owned = self.rows >= 0
        at = self.rows.clamp(min=0).to(torch.int64)
        if index is not None:
            at = index[at]
        return torch.where(owned, point_labels.detach()[at], torch.full((), fill, dtype=point_labels.dtype, device=owned.device))

    def features(self, rows_features, *, index=None, dtype=torch.float32, views=None):
        """Per-point (or, through index, per-row) features painted into the views: -> [V',H,W,D], channels last, in fp32, fp16 or bf16.
        A pixel holds the row rows_features[index[rows]] (rows_features[rows] without index) of its owner, every element converted once
        with the rounding of torch's .to(dtype) (fp32 -> fp16 / bf16: to nearest even, overflow to inf, half subnormals kept; the
        conversion fuse states); pixels without an owner are zero rows.  rows_features: fp32 [R,D] on the GPU with unit column stride
        and any row stride >= D -- y.F straight from purify -- read in place: no per-point [N,D] copy is made.  views: a slice or an
        integer index tensor selecting the views to materialise (the full map is V * H * W * D elements).  Inside: ops.render_gather
        (one wave per pixel, or several pixels per wave for narrow rows; 16-byte loads where D's pitch and the base allow)."""
        who = "Rendered.features"
        if dtype not in ops.ELEM_TAG:
            raise ValueError(f"{who}: dtype={dtype} must be torch.float32, torch.float16 or torch.bfloat16")
        Fr = rows_features
        if not torch.is_tensor(Fr) or Fr.dim() != 2 or min(Fr.shape) < 1 or Fr.dtype != torch.float32:
            raise ValueError(f"{who}: rows_features must be fp32 [R, D] with R, D >= 1, got "
                             f"{(list(Fr.shape), Fr.dtype) if torch.is_tensor(Fr) else type(Fr).__name__}")
        index = self._index(who, index, self.rows.device)
        if index is None and Fr.shape[0] != self.num_points:
            raise ValueError(f"{who}: {Fr.shape[0]} feature rows for {self.num_points} points (pass index for features per row)")
        if not (views is None or isinstance(views, slice) or (_is_int_tensor(views) and views.dim() == 1)):
            raise ValueError(f"{who}: views must be None, a slice or a 1-D integer index tensor, got {type(views).__name__}")
        if not Fr.is_cuda or not self.rows.is_cuda or Fr.device != self.rows.device:
            raise ValueError(f"{who}: rows_features and the rendered rows must be CUDA tensors on one device (got {Fr.device} / "
                             f"{self.rows.device}); there is no CPU path")
        rows = self.rows if views is None else self.rows[views]
        H, W = self.image_shape
        D = Fr.shape[1]
        with torch.cuda.device(Fr.device), torch.no_grad():
            if rows.shape[0] == 0:
                return torch.zeros((0, H, W, D), dtype=dtype, device=Fr.device)
            src = Fr.detach()
            if src.stride(1) != 1 or src.stride(0) < D:
                src = src.contiguous()
            return ops.render_gather(rows.contiguous(), src, index, dtype)


def render_rows(points, view_entry, world_to_camera, intrinsics, image_shape, *, depth=RENDER, cut_bound=0, vis_thres=0.25, radius=0):
    """The chain's end in image space: per view and pixel, the row of the front-most visible point of the view's entry -- what the
    reference's visualize_2d_semantic (models/utils/visualization.py:15-59) paints a view with, except that there the last point in
    row order that maps to a pixel wins and here the nearest does.  For all views of all entries in one call, entries never mixing.
    points, view_entry, world_to_camera and intrinsics exactly as render_depth and lift take them (points fp64 or fp32 [N,4], upcast
    to fp64 first; V views); image_shape = (H, W).  depth: None (p_z > 0 alone, no occlusion), fp64 [V,H,W] (sensor depth), or
    "render" (the maps render_depth makes from the entry's own points with the same cut_bound).  radius: an integer in 0..4.
      Candidates.  A point p of view v's entry is a candidate of v when (a) it projects inside [cut_bound, W - cut_bound) x
        [cut_bound, H - cut_bound) (pixels rounded half to even) and |depth - p_z| <= vis_thres * depth there (without depths: p_z > 0)
        -- lift's rule 1, so the candidates of a view are exactly the pairs lift counts in view_count -- and (b) p_z > 0.  For depth
        maps > 0 and 0 <= vis_thres < 1 (b) is implied; it is tested regardless, because the minimum below orders doubles by their bit
        pattern and that ordering holds only for positive values.
      Footprint.  A candidate covers the pixels of the square of side 2 * radius + 1 centred on its own pixel (vi, ui), clipped to
        [cut, H - cut) x [cut, W - cut).  radius = 0 is the reference's one-pixel projection.
      Owner.  A pixel's owner is the covering candidate with the smallest p_z (fp64, the value the lifts compute); among equal p_z
        the lowest row of points wins.  Entries never mix.  (A candidate farther than 999999 owns nothing.)
    -> Rendered: rows i32 [V,H,W] (the owner's row, -1 where nothing covers the pixel), depth fp64 [V,H,W] (the owner's p_z, 999999
    where rows == -1), view_count i64 [V] (candidates per view; equals lift's view_count on the same geometry and options),
    pixel_count i64 [V] (pixels with an owner), num_entries (1 + the highest valid batch index, from the status words), image_shape.
    A view whose entry has no points is all -1 / 999999.  Exact and reproducible: the owner is found by two order-free passes of
    integer atomic minima (the bit pattern of p_z, then the row where the pixel holds the candidate's own p_z), so two calls give the
    same bits, in any row order.  No stream class: views are independent, so a caller renders chunk by chunk and concatenates.  No
    gradients, no blending: everything is a selection.
    Inside: ops.render_rows (the entry tables, with "render" the z-buffer of render_depth in its workspace, two fills, two passes, a
    finalise kernel).  ValueError before any kernel: render_depth's refusals for the shared fields, a depth string other than
    "render", a depth of the wrong shape or dtype, a radius outside 0..4, CPU tensors (there is no CPU path); from the ONE status
    read-back, with render_depth's messages and precedence: non-finite rows, rows whose batch index is no integer in 0..65535, views
    whose entry is outside 0..65535."""
    who = "render_rows"
    P, E, M, K = points, view_entry, world_to_camera, intrinsics
    V, shape = _check_render_views(who, P, E, M, K, image_shape)
    H, W = shape
    _check_depth(who, depth, V, H, W)
    _check_visibility_options(who, cut_bound, vis_thres, 0, None)
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= ops.RENDER_ROWS_MAX_RADIUS:
        raise ValueError(f"{who}: radius={radius!r} must be an integer in 0..{ops.RENDER_ROWS_MAX_RADIUS}")
    _check_one_device(who, "points and the views' tensors", [P, E, M, K] + ([depth] if torch.is_tensor(depth) else []))
    with torch.cuda.device(P.device), torch.no_grad():
        pts = _points64(P)
        ve, w2c, intr, depth = _view_args(E, M, K, depth)
        r = ops.render_rows(pts, ve, w2c, intr, shape, cut_bound, depth=depth, vis_thres=float(vis_thres), radius=radius)
        status = ops.readback(r.status)
    _raise_status(who, status)
    return Rendered(r.rows, r.depth, r.view_count, r.pixel_count, status[3] + 1, shape, P.shape[0])


def segment_views(rendered, pred, label_maps, view_entry, num_classes, *, ignore_labels=(255,), index=None):
    """3D predictions scored against 2D ground truth in image space: the (intersection, output, target) counts of segment, taken over
    the owned pixels of rendered (a Rendered) whose 2D label is not ignored, separated by the view's entry.  pred: integer [N] per
    point, or [R] per row with index i64 [N] (point -> row, a quantiser's inverse_mapping); label_maps: uint8, int16, int32 or int64
    [V,H,W], as lift_labels takes them; view_entry: integer [V], the one render_rows was given; num_classes in 1..4096; at most 4
    ignore labels.  A pixel with prediction p and label t counts in [entry, 1, p] when 0 <= p < C, in [entry, 2, t] when 0 <= t < C,
    and in [entry, 0, p] when both hold and p == t.  -> counts i64 [num_entries, 3, C].  Inside: the owned pixels compacted in torch,
    then ops.iou_hist_batched (integer atomics: exact in any order)."""
    who = "segment_views"
    if not isinstance(rendered, Rendered):
        raise ValueError(f"{who}: rendered must be a Rendered, got {type(rendered).__name__}")
    V, (H, W), dev = rendered.rows.shape[0], rendered.image_shape, rendered.rows.device
    if not _is_int_tensor(pred) or pred.dim() != 1 or pred.shape[0] < 1:
        raise ValueError(f"{who}: pred must be an integer tensor [R >= 1], got {(list(pred.shape), pred.dtype) if torch.is_tensor(pred) else type(pred).__name__}")
    if not torch.is_tensor(label_maps) or label_maps.dtype not in ops.LABEL_TAG or label_maps.shape != (V, H, W):
        raise ValueError(f"{who}: label_maps must be uint8, int16, int32 or int64 [{V}, {H}, {W}], got "
                         f"{(list(label_maps.shape), label_maps.dtype) if torch.is_tensor(label_maps) else type(label_maps).__name__}")
    if not _is_int_tensor(view_entry) or view_entry.shape != (V,):
        raise ValueError(f"{who}: view_entry must be an integer tensor [{V}], got "
                         f"{(list(view_entry.shape), view_entry.dtype) if torch.is_tensor(view_entry) else type(view_entry).__name__}")
    if not _is_count(num_classes, 1) or num_classes > 4096:
        raise ValueError(f"{who}: num_classes={num_classes!r} must be an integer in 1..4096")
    ignore = [int(v) for v in ignore_labels]
    if len(ignore) > 4:
        raise ValueError(f"{who}: at most 4 ignore labels, got {ignore}")
    index = rendered._index(who, index, dev)
    if index is None and pred.shape[0] != rendered.num_points:
        raise ValueError(f"{who}: {pred.shape[0]} predictions for {rendered.num_points} points (pass index for predictions per row)")
    B = rendered.num_entries
    if B * 3 * num_classes > 2 ** 27:
        raise ValueError(f"{who}: {B} entries x 3 x {num_classes} classes exceed 2^27 counters")
    tensors = [rendered.rows, pred, label_maps, view_entry]
    if not all(t.is_cuda for t in tensors) or any(t.device != dev for t in tensors):
        raise ValueError(f"{who}: the rendered rows, pred, label_maps and view_entry must be CUDA tensors on one device (got "
                         f"{' / '.join(str(t.device) for t in tensors)}); there is no CPU path")
    with torch.cuda.device(dev), torch.no_grad():
        counts = torch.zeros((B, 3, num_classes), dtype=torch.int64, device=dev)
        owned = (rendered.rows >= 0).reshape(-1)
        at = rendered.rows.reshape(-1)[owned].to(torch.int64)                # pixel -> point
        if at.shape[0] == 0:
            return counts
        if index is not None:
            at = index[at]                                                   # point -> row
        coords = torch.zeros((at.shape[0], 4), dtype=torch.int32, device=dev)
        coords[:, 0] = view_entry.detach().to(torch.int32).view(V, 1).expand(V, H * W).reshape(-1)[owned]
        ops.iou_hist_batched(pred.detach().to(torch.int64)[at].contiguous(), coords, label_maps.detach().reshape(-1)[owned].to(torch.int64).contiguous(),
                             B, num_classes, ignore, counts)
    return counts


def lift(points, views, *, mode="nearest", cut_bound=0, vis_thres=0.25, min_visible=0, max_visible=None, fill=True):
    """The 2D -> 3D lift of the reference (models/affinity_module.py:404-452, models/utils/fusion_util.py:45-147,
    dataset/data_loader_ablation.py:254-288) for several scenes at once, entries never mixing.  points: floating (fp64 or fp32) [N,4] =
    batch index (integral, 0..65535), world x, y, z, on the GPU, in any row order; views: a Views.  Per entry b -- its points the rows
    with batch b in ascending row order, its views those with view_entry == b in ascending view index:
      1. a point is visible in a view when it projects inside [cut_bound, W - cut_bound) x [cut_bound, H - cut_bound) (pixels rounded
         half to even) and |depth - p_z| <= vis_thres * depth there (without depths: p_z > 0; with views.depth == "render" the depth
         maps are render_depth(points, view_entry, world_to_camera, intrinsics, image_shape, cut_bound=cut_bound), and the result is
         what the call returns when given that tensor; the rendered maps take V * H * W * 8 bytes for the duration of the call);
      2. view_keep[v] = n_v != 0 and n_v >= min_visible and n_v <= max_visible (None: no upper bound), n_v = view_count[v];
      3. the sampled feature columns of the kept views that see a point are summed in fp32 in ascending v;
      4. features = sum / (count == 0 ? 1e-6 : count), seen = count > 0;
      5. with fill, in an entry that has both seen and unseen points every unseen point takes the row of the seen point OF ITS ENTRY
         that minimises (d^2, row number), d^2 = (dx*dx + dy*dy) + dz*dz in fp64 over the fp32-rounded xyz.
    mode "nearest" samples the map's own pixel and needs (h, w) == image_shape; "bilinear" is the LSeg form: F.interpolate(bilinear,
    align_corners=True) of the [h,w] map to image_shape, evaluated at the sampled pixels only.  An entry without views, or with nothing
    seen, keeps zero rows; a view whose entry has no points has view_count 0.  The result is the same bits as HotPath.lift_dense /
    lift_lseg on each scene by itself.  -> Lifted.  No gradients: the VLM is frozen and the reference lifts under no_grad, so maps that
    require grad are refused and the points are detached.
    fp16 / bf16 maps: every sampled element is converted to fp32 as it is loaded (exact) and takes the fp32 arithmetic, so the result
    is bit for bit lift(points, Views(features.float(), ...)) -- without that copy: beside the maps the call holds nothing of their
    size (channels_last) or one transposed buffer of their own dtype (NCHW).  Half rows whose length and base address allow it
    (D % 8 == 0 and 16-byte aligned, or D % 4 == 0 and 8-byte aligned) are read 16 or 8 bytes per lane; any other half tensor 2 bytes.
    Inside: ops.lift_batched (the entry tables, the per-view counts, the fused lift kernel over pixel-major maps -- a channels_last
    tensor is read in place, an NCHW one goes through ops.lift_batched_transpose once, into a buffer of the maps' dtype --, the
    per-entry masked 1-NN) and
    ops.gather_rows; with "render", ops.render_depth_batched first (no read-back of its own: the lift's status says the same).
    ValueError before any kernel: shape / dtype / device mismatches, CPU tensors, an unknown mode, a depth string other than "render",
    maps that require grad, more than 65535 views, N >= 2^31; from the ONE status read-back, taken after the last launch (no buffer is sized by what it
    carries): rows whose batch index is no integer in 0..65535, views whose entry is outside 0..65535, non-finite coordinates."""
    who = "lift"
    V, D, h, w, H, W = _check_lift(who, points, views, mode, cut_bound, vis_thres, min_visible, max_visible)
    P, Fm, E, M, K, Dp = points, views.features, views.view_entry, views.world_to_camera, views.intrinsics, views.depth
    with torch.cuda.device(P.device), torch.no_grad():
        pts = _points64(P)
        maps = _lift_maps(Fm)                                                # (fp32, fp16 and bf16 as they are: no fp32 copy of half maps)
        if maps.is_contiguous(memory_format=torch.channels_last):
            maps_pm = maps.permute(0, 2, 3, 1).reshape(V, h * w, D)          # (a view: channels_last is pixel-major already)
        else:
            maps_pm = ops.lift_batched_transpose(maps.contiguous())          # (of the maps' own dtype)
        ve, w2c, intr, Dp = _view_args(E, M, K, Dp, _render_all(pts, (H, W), cut_bound))
        r = ops.lift_batched(pts, maps_pm, (h, w), ve, w2c, intr, Dp, (H, W), mode == "bilinear", cut_bound, float(vis_thres),
                             min_visible, _clamped(max_visible), fill=bool(fill))
        feats = _fill_rows(r.out, D, r.nn)
        status = ops.readback(r.status)
    _raise_status(who, status)
    return Lifted(feats, r.seen.bool(), r.count, r.view_count, r.view_keep.bool())


class _LiftStream:
    """What LiftStream, LiftLabelsStream and LiftMasksStream share: the points, the device and the visibility options; what a chunk
    must have in common with the first (a subclass names the fields in _CHUNK and hands the tuple to _check_chunk); the running view
    total and its limit; the refusal of a finish before any add; grow-only scratch by name; the depth="render" maps of a chunk; and
    the per-chunk view_count / view_keep in arrival order, for the streams that keep them as lists.  A subclass keeps its own checks,
    its ops.*_stream_* calls and its state, and assigns nothing of the stream before the last refusal of an add: _added is the commit."""
    _CHUNK = ()                                                 # how the messages call the fields of the first-chunk tuple

    def __init__(self, points, cut_bound, vis_thres, min_visible, max_visible):
        self.cut_bound, self.vis_thres, self.min_visible, self.max_visible = cut_bound, vis_thres, min_visible, max_visible
        self.num_views = 0
        self._points, self._device = points, points.device
        self._first = None                                      # the first chunk's tuple
        self._view_count, self._view_keep = [], []
        self._ws = {}                                           # scratch by name

    def _check_chunk(self, who, this, V):
        if self._first is not None:
            for name, a, b in zip(self._CHUNK, this, self._first):
                if a != b:
                    raise ValueError(f"{who}: {name} of a chunk must be the first chunk's: {a} after {b}")
        if self.num_views + V > 65535:
            raise ValueError(f"{who}: {V} more views after {self.num_views}, at most 65535 in all")

    def _check_started(self, who):
        if self._first is None:
            raise ValueError(f"{who}: no views were added")

    def _workspace(self, name, need, dtype=torch.uint8, floor=256):
        """scratch of at least `need` elements, reallocated only when a call needs more than every call before it"""
        ws = self._ws.get(name)
        if ws is None or ws.numel() < need:
            self._ws[name] = None                               # (freed before the larger one is taken)
            ws = self._ws[name] = torch.empty(max(int(need), floor), dtype=dtype, device=self._device)
        return ws

    def _render_chunk(self, image_hw):
        """depth="render" in a stream, as _view_args takes it: the z-buffers of a chunk's views from the stream's entry tables (nothing
        is sorted, nothing read back), into scratch that grows to the largest chunk seen -> fp64 [V,H,W]"""
        def render(view_entry, w2c, intrinsics):
            V, (H, W) = view_entry.shape[0], image_hw
            depth = self._workspace("depth", V * H * W, torch.float64, floor=0)[:V * H * W].view(V, H, W)
            workspace = self._workspace("render", ops.render_depth_stream_workspace_bytes(self._points.shape[0], V))
            return ops.render_depth_stream(self._st, view_entry, w2c, intrinsics, image_hw, self.cut_bound, depth=depth, workspace=workspace)[0]
        return render

    def _added(self, this, V, view_count=None, view_keep=None):
        self._first = this
        self.num_views += V
        if view_count is not None:
            self._view_count.append(view_count)
            self._view_keep.append(view_keep)

    def _views_so_far(self):
        return torch.cat(self._view_count), torch.cat(self._view_keep).bool()


class LiftStream(_LiftStream):
    """lift with the views arriving in chunks -- the reference's own loop (models/affinity_module.py:365-449: the VLM runs on
    max_batch_size views at a time, every chunk is added into sum_features / counter and freed, one division and one fill at the end),
    for several scenes at once.  Only one chunk's maps need to exist at a time:

        stream = LiftStream(points, feature_dim=D, mode="bilinear")
        for chunk in vlm_chunks:                                # a Views: views of any entries, any number of them
            stream.add(chunk)                                   # no host synchronisation
        lifted = stream.finish()                                # -> Lifted; the one status read-back

    points and the options are lift's; every chunk is a Views as lift takes it.
      1. After any sequence of add calls, finish(fill=f) returns what lift(points, Views(the chunks concatenated in the order added),
         fill=f, ...) returns, bit for bit in features, seen, count, view_count and view_keep (the last two in arrival order).
      2. A chunk need not be a slice of one global view list: an entry's views are taken in their order of arrival, which is all that
         lift's rule 3 (the fp32 sum in ascending v) depends on.  view_keep follows from a view's own count (rule 2), so it is final
         when the chunk is added.
      3. finish is a snapshot: it writes new tensors from the sums and counts and changes neither, so add and finish may go on
         alternating (the online use: a result after every chunk for one divide pass over [N, D] and the fill).
      4. fp32, fp16 and bf16 chunks are read as they are and may alternate inside one stream (the sums are fp32 whatever the chunk's
         dtype; a half chunk gives the bits of its fp32 copy); maps of other floating dtypes are upcast to fp32 per chunk.  A
         channels_last chunk is read in place, an NCHW chunk is transposed, in its own dtype, into one scratch buffer of the stream's
         that is sized in bytes, shared by all dtypes, and grows only when a chunk needs more bytes than every chunk before it.  Apart from the
         per-view count and keep vectors the stream holds nothing that grows with the views added: the state is the entry tables
         (8 bytes per point), the fp32 sums [N, D] and the counts [N].
      5. With depth="render" a chunk's depth maps are rendered from the stream's entry tables (ops.render_depth_stream: no sort, no
         read-back) into a scratch buffer of the largest chunk's V * H * W * 8 bytes; the maps of all views never exist at once.
    Why the bits are lift's: a point's sum starts from +0 and takes the kept views that see it in ascending order, one fp32 add each;
    between two chunks the partial sum is stored and reloaded as fp32, which changes no bit.  A point that no kept view of a chunk
    sees is neither read nor written by that chunk.
    Inside: ops.lift_stream_begin at construction (the entry tables, once), per chunk ops.lift_batched_transpose (NCHW only) and
    ops.lift_stream_add (the chunk's view table, the per-view counts and drop rule, the accumulating lift kernel), in finish
    ops.lift_stream_finish (divide, seen, the per-entry masked 1-NN) and ops.gather_rows.
    ValueError before any kernel of the call: lift's refusals, for points and options at construction and for the chunk at add; a
    chunk whose D is not feature_dim, or whose (h, w), image_shape, presence of depth (none, a tensor or "render": three kinds that do
    not mix) or device differ from the first chunk's; a chunk
    that takes the views past 65535 in all (lift's limit); finish before any add.  A refused add leaves the stream as it was.  From
    finish's ONE status read-back, with lift's messages and precedence: non-finite rows, rows whose batch index is no integer in
    0..65535 (both counted once, at construction), views whose entry is outside 0..65535 (counted over all chunks).  Such rows and
    views belong to no entry and change nobody else's result.  (RuntimeError from the same read-back: the entry tables hold values
    outside their range, i.e. somebody wrote into the stream's state; the kernels force them into range before use.)"""

    _CHUNK = ("(h, w)", "image_shape", "the presence of depth (none, tensor or 'render')")

    def __init__(self, points, feature_dim, *, mode="nearest", cut_bound=0, vis_thres=0.25, min_visible=0, max_visible=None):
        who = "LiftStream"
        _check_lift(who, points, None, mode, cut_bound, vis_thres, min_visible, max_visible)
        if not _is_count(feature_dim, 1) or feature_dim >= 2 ** 31:
            raise ValueError(f"{who}: feature_dim={feature_dim!r} must be a positive integer")
        super().__init__(points, cut_bound, vis_thres, min_visible, max_visible)
        self.mode, self.feature_dim = mode, int(feature_dim)
        with torch.cuda.device(self._device), torch.no_grad():
            self._st = ops.lift_stream_begin(_points64(points), self.feature_dim)

    @property
    def _scratch(self):
        """the NCHW transpose scratch, as fp32 words"""
        return self._ws.get("transpose")

    def add(self, views):
        """One chunk of views (a Views) onto the sums.  No host synchronisation."""
        who = "LiftStream.add"
        V, D, h, w, H, W = _check_lift(who, self._points, views, self.mode, self.cut_bound, self.vis_thres, self.min_visible, self.max_visible)
        if D != self.feature_dim:
            raise ValueError(f"{who}: the chunk's maps have {D} channels, the stream was built with feature_dim={self.feature_dim}")
        this = ((h, w), (H, W), _depth_kind(views.depth))
        self._check_chunk(who, this, V)
        Fm, E, M, K, Dp = views.features, views.view_entry, views.world_to_camera, views.intrinsics, views.depth
        with torch.cuda.device(self._device), torch.no_grad():
            maps = _lift_maps(Fm)                                            # (fp32, fp16 and bf16 as they are; the sums are fp32)
            if maps.is_contiguous(memory_format=torch.channels_last):
                maps_pm = maps.permute(0, 2, 3, 1).reshape(V, h * w, D)      # (a view: channels_last is pixel-major already)
            else:
                nbytes = maps.numel() * maps.element_size()                 # (the scratch is sized in bytes: chunks of any dtype share it)
                words = -(-nbytes // 4)                                      # (kept as fp32 words: an fp32 chunk's element count)
                scratch = self._workspace("transpose", words, torch.float32, floor=0)
                maps_pm = ops.lift_batched_transpose(maps.contiguous(), out=scratch.view(torch.uint8)[:nbytes].view(maps.dtype).view(V, h * w, D))
            workspace = self._workspace("add", ops.lift_stream_add_workspace_bytes(V))
            ve, w2c, intr, Dp = _view_args(E, M, K, Dp, self._render_chunk((H, W)))
            vc, vk = ops.lift_stream_add(self._st, maps_pm, (h, w), ve, w2c, intr, Dp, (H, W), self.mode == "bilinear", self.cut_bound,
                                         float(self.vis_thres), self.min_visible, _clamped(self.max_visible), workspace=workspace)
        self._added(this, V, vc, vk)

    def finish(self, fill=True):
        """-> Lifted over the views added so far; the stream goes on.  One host synchronisation (the status read-back)."""
        who = "LiftStream.finish"
        self._check_started(who)
        with torch.cuda.device(self._device), torch.no_grad():
            r = ops.lift_stream_finish(self._st, fill=bool(fill),
                                       workspace=self._workspace("finish", ops.lift_stream_finish_workspace_bytes(self._points.shape[0])))
            feats = _fill_rows(r.out, self.feature_dim, r.nn)
            count = self._st.count.clone()
            view_count, view_keep = self._views_so_far()
            status = ops.readback(r.status)
        _raise_status(who, status, state=True)
        return Lifted(feats, r.seen.bool(), count, view_count, view_keep)


# ------------------------------------------------------------------------------------------ the label vote
LABEL_DTYPES = tuple(ops.LABEL_TAG)                         # uint8, int16, int32, int64
MAX_CLASSES = ops.LIFT_LABELS_MAX_CLASSES


class LabelViews:
    """The views of a batch of scenes with an integer label map each: labels uint8, int16, int32 or int64 [V,H,W] (a 2D segmenter's
    per-pixel predictions, or 2D ground truth: the loader's label_2ds; read in place, no widened copy; bool and floating maps are
    refused), view_entry, world_to_camera, intrinsics and depth (fp64 [V,H,W], None or "render") exactly as Views takes them.  The image
    shape is the maps' (H, W): labels are never resampled.  lift_labels checks the fields."""

    def __init__(self, labels, view_entry, world_to_camera, intrinsics, depth=None):
        self.labels, self.view_entry, self.world_to_camera, self.intrinsics, self.depth = labels, view_entry, world_to_camera, intrinsics, depth


class LiftedLabels:
    """labels i64 [N] in the points' row order (the voted class, a filled one, or `unlabeled`), votes i32 [N, num_classes] (zero rows for
    filled and unlabeled points), voted i32 [N] (the votes of a point), seen bool [N] and count i32 [N] (the kept views that see it:
    lift's), view_count i64 [V] and view_keep bool [V] (lift's)."""

    def __init__(self, labels, votes, voted, seen, count, view_count, view_keep):
        self.labels, self.votes, self.voted, self.seen, self.count = labels, votes, voted, seen, count
        self.view_count, self.view_keep = view_count, view_keep


def _check_lift_labels(who, points, views, num_classes, ignore_labels, unlabeled, cut_bound, vis_thres, min_visible, max_visible):
    """lift_labels' argument checks, in lift's order; views None: those of the points and the options alone (LiftLabelsStream's
    construction).  -> (V, H, W), or None without views"""
    if views is not None and not isinstance(views, LabelViews):
        raise ValueError(f"{who}: views must be a LabelViews, got {type(views).__name__}")
    P = points
    _check_points(who, P)
    if views is not None:
        L, E, M, K, Dp = views.labels, views.view_entry, views.world_to_camera, views.intrinsics, views.depth
        if not torch.is_tensor(L) or L.dim() != 3 or min(L.shape) < 1:
            raise ValueError(f"{who}: views.labels must be [V, H, W] with V, H, W >= 1, got {_shape_of(L)}")
        if L.dtype not in LABEL_DTYPES:
            raise ValueError(f"{who}: views.labels must be uint8, int16, int32 or int64 (bool and floating label maps are refused), got {L.dtype}")
        V, H, W = L.shape
        _check_view_count(who, V)
        _check_poses(who, "views.", V, E, M, K)
        _check_depth(who, Dp, V, H, W)
    _check_visibility_options(who, cut_bound, vis_thres, min_visible, max_visible)
    if not _is_count(num_classes, 1) or num_classes > MAX_CLASSES:
        raise ValueError(f"{who}: num_classes={num_classes!r} must be an integer in 1..{MAX_CLASSES}")
    if not isinstance(ignore_labels, (tuple, list)) or len(ignore_labels) > ops.LIFT_LABELS_MAX_IGNORE or \
            not all(isinstance(v, int) and not isinstance(v, bool) and -2 ** 63 <= v < 2 ** 63 for v in ignore_labels):
        raise ValueError(f"{who}: ignore_labels={ignore_labels!r} must be a tuple of at most {ops.LIFT_LABELS_MAX_IGNORE} integers")
    if not isinstance(unlabeled, int) or isinstance(unlabeled, bool) or not -2 ** 63 <= unlabeled < 2 ** 63 or 0 <= unlabeled < num_classes:
        raise ValueError(f"{who}: unlabeled={unlabeled!r} must be an integer outside 0..{num_classes - 1}, the classes")
    _check_one_device(who, "points and the views' tensors",
                      [P] + ([L, E, M, K] + ([Dp] if torch.is_tensor(Dp) else []) if views is not None else []))
    return (V, H, W) if views is not None else None


def lift_labels(points, views, num_classes, *, ignore_labels=(255,), unlabeled=255, cut_bound=0, vis_thres=0.25, min_visible=0,
                max_visible=None, fill=True):
    """Integer 2D label maps voted onto the points of several scenes at once, entries never mixing: the majority vote of a 2D
    segmenter's per-pixel predictions (the 2D-fusion baseline a purified result is compared with), or of 2D ground truth (pseudo-labels
    for segment_loss / purified_loss).  The reference has no such function; the geometry is its own (models/utils/fusion_util.py:99-147,
    dataset/data_loader_ablation.py:254-288).  points as lift takes them; views: a LabelViews.  Per entry b -- its points the rows with
    batch b, its views those with view_entry == b:
      1. visible(p, v), view_count, view_keep, count and seen are lift's rules 1 and 2: on the same geometry they equal lift's;
      2. votes[p, c] = the kept views v that see p with labels[v, py, px] == c, c in 0..num_classes-1; a sampled pixel whose value is in
         ignore_labels casts no vote;
      3. any other sampled value outside 0..num_classes-1 casts no vote and is an error (ValueError from the status read-back);
      4. voted[p] = sum_c votes[p, c]; a seen point may have voted == 0 (every view that sees it shows an ignored pixel);
      5. labels[p] = the lowest class with the most votes, where voted[p] > 0;
      6. with fill, in an entry that has both voted and unvoted points every unvoted point takes the label of the voted point OF ITS ENTRY
         that minimises (d^2, row number), d^2 = (dx*dx + dy*dy) + dz*dz in fp64 over the fp32-rounded xyz (lift's rule 5 with "seen" read
         as "voted"); its votes row stays zero, so a filled label stays recognisable;
      7. everywhere else labels[p] = unlabeled (which must lie outside 0..num_classes-1).
    Everything is integer arithmetic: the result is exact and independent of any order.  -> LiftedLabels.  No gradients; the points are
    detached.  The vote histogram is a feature matrix too: quantize(points, votes.float()) followed by affinity_pool purifies label
    distributions with the operator that purifies features.
    Inside: ops.lift_labels_batched (the entry tables, the per-view counts, the vote kernel -- one wave per point, one label load per
    (point, view) sample, the histogram in LDS --, the per-entry masked 1-NN over "voted"); with "render", ops.render_depth_batched first.
    ValueError before any kernel: lift's refusals for the shared fields; label maps that are not uint8 / int16 / int32 / int64;
    num_classes outside 1..1024; unlabeled inside 0..num_classes-1; more than 16 ignore labels.  From the ONE status read-back, taken after
    the last launch (no buffer is sized by what it carries), lift's three first: non-finite coordinates, rows whose batch index is no
    integer in 0..65535, views whose entry is outside 0..65535, then sampled labels out of range."""
    who = "lift_labels"
    V, H, W = _check_lift_labels(who, points, views, num_classes, ignore_labels, unlabeled, cut_bound, vis_thres, min_visible, max_visible)
    P, L, E, M, K, Dp = points, views.labels, views.view_entry, views.world_to_camera, views.intrinsics, views.depth
    with torch.cuda.device(P.device), torch.no_grad():
        pts = _points64(P)
        ve, w2c, intr, Dp = _view_args(E, M, K, Dp, _render_all(pts, (H, W), cut_bound))
        r = ops.lift_labels_batched(pts, L.detach().contiguous(), num_classes, ve, w2c, intr, Dp, cut_bound, float(vis_thres), min_visible,
                                    _clamped(max_visible), ignore_ids=tuple(ignore_labels), unlabeled=unlabeled, fill=bool(fill))
        status = ops.readback(r.status)
    _raise_status(who, status, num_classes=num_classes, state=True)
    return LiftedLabels(r.labels, r.votes, r.voted, r.seen.bool(), r.count, r.view_count, r.view_keep.bool())


class LiftLabelsStream(_LiftStream):
    """lift_labels with the views arriving in chunks, for several scenes at once.  Only one chunk's label maps need to exist at a time:

        stream = LiftLabelsStream(points, num_classes=C)
        for chunk in segmenter_chunks:                          # a LabelViews: views of any entries, any number of them
            stream.add(chunk)                                   # no host synchronisation
        lifted = stream.finish()                                # -> LiftedLabels; the one status read-back

    points and the options are lift_labels'; every chunk is a LabelViews as lift_labels takes it.
      1. After any sequence of add calls, finish(fill=f) returns what lift_labels(points, LabelViews(the chunks concatenated in the order
         added), num_classes, fill=f, ...) returns; view_count and view_keep come in arrival order.
      2. votes, voted, count, seen and labels do not depend on the order of the chunks: the sums are integers.
      3. finish is a snapshot: it writes new tensors and changes no state, so add and finish may go on alternating.
      4. Chunks of different label dtypes may alternate.  Apart from the per-view count and keep vectors the stream holds nothing that
         grows with the views added: the state is the entry tables (8 bytes per point), votes i32 [N, num_classes] and count [N].
      5. With depth="render" a chunk's depth maps are rendered from the stream's entry tables (ops.render_depth_stream), as LiftStream
         does it.
    Inside: ops.lift_labels_stream_begin at construction (the entry tables, once), per chunk ops.lift_labels_stream_add (the chunk's view
    table, the per-view counts and drop rule, the accumulating vote kernel), in finish ops.lift_labels_stream_finish (voted, arg-max,
    seen, the per-entry masked 1-NN over "voted").
    ValueError before any kernel of the call: lift_labels' refusals, for points and options at construction and for the chunk at add; a
    chunk whose (H, W), presence of depth (none, a tensor or "render") or device differ from the first chunk's; a chunk that takes the
    views past 65535 in all; finish before any add.  A refused add leaves the stream as it was.  From finish's ONE status read-back, with
    lift_labels' messages and precedence; the out-of-range labels are counted over all chunks, kept in the state and reported by every
    finish.  (RuntimeError from the same read-back: the entry tables hold values outside their range, i.e. somebody wrote into the
    stream's state.)"""

    _CHUNK = ("(H, W)", "the presence of depth (none, tensor or 'render')")

    def __init__(self, points, num_classes, *, ignore_labels=(255,), unlabeled=255, cut_bound=0, vis_thres=0.25, min_visible=0,
                 max_visible=None):
        who = "LiftLabelsStream"
        _check_lift_labels(who, points, None, num_classes, ignore_labels, unlabeled, cut_bound, vis_thres, min_visible, max_visible)
        super().__init__(points, cut_bound, vis_thres, min_visible, max_visible)
        self.num_classes, self.ignore_labels, self.unlabeled = int(num_classes), tuple(ignore_labels), unlabeled
        with torch.cuda.device(self._device), torch.no_grad():
            self._st = ops.lift_labels_stream_begin(_points64(points), self.num_classes)

    def add(self, views):
        """One chunk of views (a LabelViews) onto the votes.  No host synchronisation."""
        who = "LiftLabelsStream.add"
        V, H, W = _check_lift_labels(who, self._points, views, self.num_classes, self.ignore_labels, self.unlabeled, self.cut_bound,
                                     self.vis_thres, self.min_visible, self.max_visible)
        this = ((H, W), _depth_kind(views.depth))
        self._check_chunk(who, this, V)
        L, E, M, K, Dp = views.labels, views.view_entry, views.world_to_camera, views.intrinsics, views.depth
        with torch.cuda.device(self._device), torch.no_grad():
            workspace = self._workspace("add", ops.lift_labels_stream_add_workspace_bytes(V))
            ve, w2c, intr, Dp = _view_args(E, M, K, Dp, self._render_chunk((H, W)))
            vc, vk = ops.lift_labels_stream_add(self._st, L.detach().contiguous(), ve, w2c, intr, Dp, self.cut_bound, float(self.vis_thres),
                                                self.min_visible, _clamped(self.max_visible), ignore_ids=self.ignore_labels, workspace=workspace)
        self._added(this, V, vc, vk)

    def finish(self, fill=True):
        """-> LiftedLabels over the views added so far; the stream goes on.  One host synchronisation (the status read-back)."""
        who = "LiftLabelsStream.finish"
        self._check_started(who)
        with torch.cuda.device(self._device), torch.no_grad():
            r = ops.lift_labels_stream_finish(self._st, unlabeled=self.unlabeled, fill=bool(fill),
                                              workspace=self._workspace("finish", ops.lift_labels_stream_finish_workspace_bytes(self._points.shape[0])))
            votes, count = self._st.votes.clone(), self._st.count.clone()
            view_count, view_keep = self._views_so_far()
            status = ops.readback(r.status)
        _raise_status(who, status, num_classes=self.num_classes, state=True)
        return LiftedLabels(r.labels, votes, r.voted, r.seen.bool(), count, view_count, view_keep)


# ------------------------------------------------------------------------------------------ the mask-embedding lift
MAX_QUERIES = 1024                                          # gp_lift_masks_batched: a view's scores are sorted in LDS
_TABLE_ROWS = 2 ** 24                                       # rows of one ops.segment_tables launch


class MaskViews:
    """The views of a batch of scenes with the X-Decoder form of the VLM's outputs: pred_masks fp32, fp16 or bf16 [V,Q,h,w] (mask logits;
    half logits are read as they are and give the bits of their fp32 copy), pred_logits
    floating [V,Q,C+1] (class logits, the last column "no object"), mask_embed floating [V,Q,D]; view_entry, world_to_camera,
    intrinsics, depth exactly as in Views (a tensor, None or "render"); image_shape = (H, W), required: the reference's cfg.mask_shape, the size the masks are
    resized to and the depths and intrinsics refer to (h <= H and w <= W).  Every view has the same number of queries Q.  lift_masks
    checks the fields."""

    def __init__(self, pred_masks, pred_logits, mask_embed, view_entry, world_to_camera, intrinsics, depth=None, image_shape=None):
        self.pred_masks, self.pred_logits, self.mask_embed = pred_masks, pred_logits, mask_embed
        self.view_entry, self.world_to_camera, self.intrinsics, self.depth, self.image_shape = view_entry, world_to_camera, intrinsics, depth, image_shape


class LiftedMasks:
    """features fp32 [N,D] in the points' row order, seen bool [N], count i32 [N] (the kept views that see the point), view_count i64
    [V], view_keep bool [V], text_features fp32 [C,D] (the NORMALISED text embeddings, as the reference returns them) and logit_scale."""

    def __init__(self, features, seen, count, view_count, view_keep, text_features, logit_scale):
        self.features, self.seen, self.count, self.view_count, self.view_keep = features, seen, count, view_count, view_keep
        self.text_features, self.logit_scale = text_features, logit_scale


_TAPS = {}


def _tap_tables(h, w, H, W, device):
    """bicubic.aa_bicubic_taps of both axes on the device, cached per (h, w, H, W, device).  The upload is from pinned memory and does
    not wait; the pinned source is kept beside the device copy."""
    key = (h, w, H, W, str(device))
    if key not in _TAPS:
        from .bicubic import aa_bicubic_taps
        tx0, twx = aa_bicubic_taps(w, W)
        ty0, twy = aa_bicubic_taps(h, H)
        host = tuple(torch.from_numpy(a).pin_memory() for a in (tx0, twx, ty0, twy))
        _TAPS[key] = (tuple(t.to(device, non_blocking=True) for t in host), host)
    return _TAPS[key][0]


def _check_lift_masks(who, points, views, text_embed, logit_scale, cut_bound, vis_thres, min_visible, max_visible):
    """lift_masks' argument checks, in lift_masks' order; views None: those of the points, the text and the options alone
    (LiftMasksStream's construction).  -> (V, Q, h, w, H, W, C, D), or (C, D) without views"""
    if views is not None and not isinstance(views, MaskViews):
        raise ValueError(f"{who}: views must be a MaskViews, got {type(views).__name__}")
    P = points
    _check_points(who, P)
    if views is not None:
        Pm, Pl, Em = views.pred_masks, views.pred_logits, views.mask_embed
        E, M, K, Dp = views.view_entry, views.world_to_camera, views.intrinsics, views.depth
        if not torch.is_tensor(Pm) or Pm.dim() != 4 or min(Pm.shape) < 1 or Pm.dtype not in ops.ELEM_TAG:
            raise ValueError(f"{who}: views.pred_masks must be fp32, fp16 or bf16 [V, Q, h, w] with V, Q, h, w >= 1, got "
                             f"{(list(Pm.shape), Pm.dtype) if torch.is_tensor(Pm) else type(Pm).__name__}")
        V, Q, h, w = Pm.shape
        _check_view_count(who, V)
        if Q > MAX_QUERIES:
            raise ValueError(f"{who}: {Q} queries per view, at most {MAX_QUERIES} (a view's scores are sorted in LDS)")
    if not torch.is_tensor(text_embed) or text_embed.dim() != 2 or min(text_embed.shape) < 1 or not text_embed.dtype.is_floating_point:
        raise ValueError(f"{who}: text_embed must be floating point [C, D] with C, D >= 1, got "
                         f"{(list(text_embed.shape), text_embed.dtype) if torch.is_tensor(text_embed) else type(text_embed).__name__}")
    C, D = text_embed.shape
    if views is not None:
        if not torch.is_tensor(Pl) or Pl.shape != (V, Q, C + 1) or not Pl.dtype.is_floating_point:
            raise ValueError(f"{who}: views.pred_logits must be floating point [{V}, {Q}, {C + 1}] (C + 1 columns, the last \"no object\"), got "
                             f"{(list(Pl.shape), Pl.dtype) if torch.is_tensor(Pl) else type(Pl).__name__}")
        if not torch.is_tensor(Em) or Em.shape != (V, Q, D) or not Em.dtype.is_floating_point:
            raise ValueError(f"{who}: views.mask_embed must be floating point [{V}, {Q}, {D}], got "
                             f"{(list(Em.shape), Em.dtype) if torch.is_tensor(Em) else type(Em).__name__}")
        _check_poses(who, "views.", V, E, M, K)
        H, W = _image_shape(who, "views.", views.image_shape, () if views.image_shape is None else tuple(views.image_shape),
                            " (the size the masks are resized to)")
        if h > H or w > W:
            raise ValueError(f"{who}: masks of {h} x {w} are larger than image_shape {H} x {W}: the bicubic-antialias resize is evaluated for "
                             "up-sampling only")
        _check_depth(who, Dp, V, H, W)
    _check_visibility_options(who, cut_bound, vis_thres, min_visible, max_visible)
    if isinstance(logit_scale, bool) or not isinstance(logit_scale, (int, float)) or logit_scale != logit_scale:
        raise ValueError(f"{who}: logit_scale={logit_scale!r} must be a number")
    named = ([("views.pred_masks", Pm), ("views.pred_logits", Pl), ("views.mask_embed", Em)] if views is not None else []) + [("text_embed", text_embed)]
    for name, t in named:
        if t.requires_grad:
            raise ValueError(f"{who}: {name} require grad, but the lift takes no gradients (the VLM is frozen, the reference lifts under "
                             "no_grad); detach them")
    _check_one_device(who, "points, text_embed and the views' tensors", [P] + ([Pm, Pl, Em] if views is not None else []) + [text_embed]
                      + ([E, M, K] + ([Dp] if torch.is_tensor(Dp) else []) if views is not None else []))
    return (V, Q, h, w, H, W, C, D) if views is not None else (C, D)


# what lift_masks and LiftMasksStream.add prepare for their kernels, and what both return when no kept view sees a point
def _unit_text(text_embed):
    return torch.nn.functional.normalize(text_embed.detach().float(), dim=-1).contiguous()


def _padded_text(text_norm):
    """the fusion kernel moves rows as float4: tables and rows padded to a multiple of 4 columns (zeros add nothing to a norm or a dot
    product, and a lane's terms stay the lane's)"""
    C, D = text_norm.shape
    text4 = torch.zeros((C, _pad_to(D, 4)), dtype=torch.float32, device=text_norm.device)
    text4[:, :D] = text_norm
    return text4


def _mask_tables(Pl, Em, text_norm, logit_scale, text4=None, f_seg=None, l_seg=None):
    """-> scores fp32 [V,Q] (lift_masks' rule 2) and the segment tables f_seg fp32 [V,Q,d4] / l_seg fp32 [V,Q,C] of the views (rule 5,
    ops.segment_tables over the rows padded to d4 columns).  text4: text_norm padded already (a stream's, made once); f_seg / l_seg:
    the caller's own rows to write (a stream's slices of what it keeps) -- without them fresh ones."""
    (V, Q, D), C, dev = Em.shape, text_norm.shape[0], Em.device
    scores = torch.softmax(Pl.detach().float(), dim=-1)[..., :-1].max(-1).values.contiguous()
    d4 = _pad_to(D, 4)
    emb = torch.zeros((V * Q, d4), dtype=torch.float32, device=dev)
    emb[:, :D] = Em.detach().float().reshape(V * Q, D)
    if text4 is None:
        text4 = _padded_text(text_norm)
    if f_seg is None:
        f_seg = torch.empty((V, Q, d4), dtype=torch.float32, device=dev)
        l_seg = torch.empty((V, Q, C), dtype=torch.float32, device=dev)
    f_rows, l_rows = f_seg.view(V * Q, d4), l_seg.view(V * Q, C)
    for r0 in range(0, V * Q, _TABLE_ROWS):
        r1 = min(r0 + _TABLE_ROWS, V * Q)
        ops.segment_tables(emb[r0:r1], text4, float(logit_scale), f_rows[r0:r1], l_rows[r0:r1])
    return scores, f_seg, l_seg


def _nothing_visible(n, D, dev):
    """features, seen and count of a mask lift in which no kept view sees a point"""
    return (torch.zeros((n, D), dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.bool, device=dev),
            torch.zeros(n, dtype=torch.int32, device=dev))


def lift_masks(points, views, text_embed, logit_scale, *, cut_bound=0, vis_thres=0.25, min_visible=0, max_visible=None, fill=True):
    """The reference's default lift, lift_xdecoder_features (models/affinity_module.py:455-714), for several scenes at once, entries
    never mixing and with no cap on the views of an entry.  points as for lift; views: a MaskViews; text_embed floating [C,D].  Per
    entry b -- its points the rows with batch b in ascending row order, its views those with view_entry == b in ascending view index:
      1. visibility, view_count and view_keep exactly as lift's steps 1-2 (views.depth == "render" included: the rendered maps take
         V * H * W * 8 bytes for the duration of the call and cost no read-back);
      2. score[v,q] = softmax(pred_logits[v,q])[:-1].max() (torch on the device);
      3. the segment of a visible pixel of a kept view: the bicubic-antialias resize of pred_masks[v] to image_shape evaluated at that
         pixel; over the queries with score > 0 the arg-max of score_q * sigmoid(logit_q), the smallest q among equal products; that q
         if sigmoid(logit_q) >= 0.5, else none;
      4. the in-view fill (:604-625): inside a kept view a point without a segment takes the segment of the point of that view that has
         one and minimises (d^2, row), d^2 = (dx*dx + dy*dy) + dz*dz in fp64 over the fp32-rounded xyz; a view where no point has a
         segment keeps none;
      5. f_seg = normalize(mask_embed), logit_seg = logit_scale * f_seg . normalize(text_embed);
      6. fusion (:647-686) over a point's slots = its kept views that see it, in ascending view index: the consensus class is the
         arg-max of the mean logits (the first maximum), the top-min(M,3) slots by that class's logit (the earlier slot among equals)
         are combined with softmax weights; a slot without a segment carries a zero feature and zero logits;
      7. count = the slots, seen = count > 0, unseen rows are zero; with fill an unseen point of an entry that has seen points takes
         the row of the seen point of its entry minimising (d^2, row) -- lift's step 5;
      8. text_features = normalize(text_embed): the reference returns those (:628 rebinds the name).
    The rows are the same bits as HotPath.lift_masks' kernels on each scene by itself.  -> LiftedMasks.  fp16 / bf16 pred_masks are read
    in place: the 16 taps of a pixel are converted to fp32 as they are loaded (exact), the resize, the products and the decision are
    the fp32 call's, so the result is bit for bit lift_masks on pred_masks.float() -- without that copy, and with the call's own
    rank-ordered transposed copy (V * h * w * Q elements of the workspace) in the masks' dtype too: half the bytes.  pred_logits and
    mask_embed are small and upcast by torch.  No gradients: inputs that
    require grad are refused and the points are detached.  Deterministic: no float atomics, no order that depends on arrival.
    Inside: ops.lift_masks_batched_lists (entry tables, ordered visible lists), ops.segment_tables, ops.lift_masks_batched (segments,
    in-view fill, point -> view lists over a bit set of ceil(most views of an entry / 64) words, fusion, per-entry 1-NN), ops.gather_rows.
    D is padded to a multiple of 4 inside (the fusion kernel's rows).  ValueError before any kernel: shape / dtype / device mismatches
    (pred_masks of any dtype but fp32, fp16 and bf16 among them), CPU tensors, inputs that require grad, Q > 1024, more than 65535 views, masks larger than image_shape, N >= 2^31.  TWO read-backs:
    the sizes after the counting pass (entries in all, the most views of an entry) and the status after the last launch (rows whose
    batch index is no integer in 0..65535, views whose entry is outside 0..65535, non-finite coordinates: ValueError)."""
    who = "lift_masks"
    if views is None:
        raise ValueError(f"{who}: views must be a MaskViews, got NoneType")
    V, Q, h, w, H, W, C, D = _check_lift_masks(who, points, views, text_embed, logit_scale, cut_bound, vis_thres, min_visible, max_visible)
    P, Pm, Pl, Em = points, views.pred_masks, views.pred_logits, views.mask_embed
    E, M, K, Dp = views.view_entry, views.world_to_camera, views.intrinsics, views.depth
    n, dev = P.shape[0], P.device
    with torch.cuda.device(dev), torch.no_grad():
        pts = _points64(P)
        ve, w2c, intr, Dp = _view_args(E, M, K, Dp, _render_all(pts, (H, W), cut_bound))
        lists = ops.lift_masks_batched_lists(pts, ve, w2c, intr, Dp, (H, W), cut_bound, float(vis_thres), min_visible,
                                             _clamped(max_visible))              # (the first read-back)
        text_norm = _unit_text(text_embed)
        status = lists.status
        if lists.total == 0:
            feats, seen, count = _nothing_visible(n, D, dev)
        else:
            scores, f_seg, l_seg = _mask_tables(Pl, Em, text_norm, logit_scale)
            r = ops.lift_masks_batched(pts, ve, Pm.detach().contiguous(), scores, _tap_tables(h, w, H, W, dev), (H, W),
                                       (lists.pt, lists.x, lists.y, lists.view), lists.view_off, lists.view_keep, lists.total,
                                       max(1, -(-lists.max_views // 64)), f_seg, l_seg, fill=bool(fill))
            feats = _fill_rows(r.out, f_seg.shape[2], r.nn, D)
            seen, count, status = r.seen.bool(), r.count, r.status
        status = ops.readback(status)                                            # (the second read-back)
    _raise_status(who, status, torn=_LISTS_TORN if lists.total else None)
    return LiftedMasks(feats, seen, count, lists.view_count, lists.view_keep.bool(), text_norm, logit_scale)


MAX_RECORDS = 2 ** 31 - 2                                   # gp_lift_masks_batched's limit on the visible entries of one call


def _grown(t, used, need, shape_tail, dtype, device, most=None):
    """a buffer of at least `need` leading rows that keeps the first `used` of t: t itself while it is large enough, otherwise one of
    max(need, twice the rows of t) rows (at most `most`) -- geometric, so a stream copies every row O(1) times"""
    if t is not None and t.shape[0] >= need:
        return t
    rows = need if t is None else max(need, 2 * t.shape[0])
    if most is not None:
        rows = min(rows, most)
    new = torch.empty((rows,) + tuple(shape_tail), dtype=dtype, device=device)
    if t is not None and used:
        new[:used] = t[:used]
    return new


class LiftMasksStream(_LiftStream):
    """lift_masks with the views arriving in chunks -- the reference's own loop (models/affinity_module.py:495-640: the X-Decoder runs on
    one view, the view's masks become per-point segments, only the small per-point record survives in point_info and the masks are
    freed; the fusion :647-686 alone looks across views), for several scenes at once.  Only one chunk's masks need to exist at a time:

        stream = LiftMasksStream(points, text_embed, logit_scale)
        for chunk in vlm_chunks:                                # a MaskViews: views of any entries, any number of them
            stream.add(chunk)                                   # one read-back: the chunk's sizes
        lifted = stream.finish()                                # -> LiftedMasks; the one status read-back

    points, text_embed, logit_scale and the options are lift_masks'; every chunk is a MaskViews as lift_masks takes it.
      1. After any sequence of add calls, finish(fill=f) returns what lift_masks(points, MaskViews(the chunks concatenated in the order
         added), text_embed, logit_scale, fill=f, ...) returns, bit for bit in features, seen, count, view_count, view_keep and
         text_features (the view fields in arrival order).
      2. An entry's views are taken in their order of arrival; a chunk may hold views of any entries.  The slot order of lift_masks'
         rule 6 ("ascending view index", the earlier slot among equal logits) is arrival order inside the entry, which is what
         lift_masks sees on the concatenation.  view_keep follows from a view's own count, so it is final when the chunk is added.
      3. finish is a snapshot: it writes new tensors and changes nothing the stream keeps, so add and finish may go on alternating.
      4. After add returns the stream holds nothing of the size of the masks (Q x h x w per view).  It keeps: per point the entry
         tables, written once at construction; per view its entry, count, keep flag, record offset and position inside its entry, and
         its rows of the segment tables f_seg [Q, D padded to 4] and logit_seg [Q, C] (ops.segment_tables on the chunk); per visible
         (point, kept view) pair one record (row i32, segment i32 or -1 after the in-view fill), view-major, rows ascending inside a
         view; one view counter per entry in the state; and scratch -- add's workspaces, reused and grown to the largest chunk seen.
         The growing buffers double, so finish concatenates nothing.  A chunk in which no kept view sees anything stores its per-view
         fields alone (its table rows are reserved and never read).
      5. add makes exactly ONE read-back, the counterpart of lift_masks' first: the chunk's visible entries (they size add's
         workspace), those of its kept views (the records it appends) and the most views of one entry so far (the bit set's words in
         finish).  finish makes exactly ONE, the status.  An add without a read-back would have to reserve records for the worst case,
         every point in every view; that is out of scope.
      6. text_embed and logit_scale are fixed at construction; the text is normalised once and returned as text_features.
      7. A chunk's pred_masks may be fp32, fp16 or bf16, chunk by chunk: a chunk leaves (row, segment) records behind, which are the
         same whatever the dtype its logits were read in, and a half chunk's records are those of its fp32 copy.  add's workspace
         holds the chunk's transposed copy in the chunk's dtype.
    Why the bits are lift_masks': visibility and the drop rule, the score sort and the ordered transpose, the segment decision and the
    in-view fill are per view and read no other view -- the chunk goes through lift_masks' own kernels, over a workspace sized by the
    chunk.  The fusion kernel reads a point's slots (view, segment) in ascending position inside the entry with that view's table rows;
    finish rebuilds exactly those lists from the records (the same bit set and popcount kernels) and runs the same fusion and fill.
    Inside: ops.lift_masks_stream_begin at construction; per chunk ops.lift_masks_batched_lists (its counting call, then
    ops.lift_masks_stream_sizes in place of its read-back, then its writing call), ops.segment_tables, ops.lift_masks_stream_add; in
    finish ops.lift_masks_stream_finish and ops.gather_rows.
    ValueError before any kernel of the call: lift_masks' refusals, for points, text and options at construction and for the chunk at
    add; a chunk whose Q, (h, w), image_shape or presence of depth (none, a tensor or "render": three kinds that do not mix) differ from
    the first chunk's (with "render" a chunk's maps are rendered from the stream's entry tables by ops.render_depth_stream into scratch of
    the largest chunk's V * H * W * 8 bytes, with no further read-back; another C, D or device is lift_masks'
    own refusal against the text and the points); a chunk that takes the views past 65535 in all; finish before any add.  After the
    chunk's read-back, before anything is changed: records past 2^31 - 2 in all (lift_masks' limit on the visible entries).  A refused
    add leaves the stream as it was.  From finish's read-back, with lift_masks' messages and precedence: non-finite rows, rows whose
    batch index is no integer in 0..65535 (both counted once, at construction), views whose entry is outside 0..65535 (counted over all
    chunks).  RuntimeError from the same read-back: the state, the per-view arrays or the records hold values outside their range or
    do not hold together, i.e. somebody wrote into what the stream keeps; the kernels force them into range or leave them out first.
    No gradients, as for lift_masks."""

    _CHUNK = ("Q", "(h, w)", "image_shape", "the presence of depth (none, tensor or 'render')")

    def __init__(self, points, text_embed, logit_scale, *, cut_bound=0, vis_thres=0.25, min_visible=0, max_visible=None):
        who = "LiftMasksStream"
        C, D = _check_lift_masks(who, points, None, text_embed, logit_scale, cut_bound, vis_thres, min_visible, max_visible)
        super().__init__(points, cut_bound, vis_thres, min_visible, max_visible)
        self.logit_scale, self.num_classes, self.feature_dim = logit_scale, C, D
        self.num_records = self.most_views = 0
        self._text = text_embed
        # the per-view fields are doubling buffers here (_grown), not the base's per-chunk lists
        self._view_entry = self._view_count = self._view_keep = self._view_pos = self._rec_off = None
        self._f_seg = self._l_seg = self._rec_row = self._rec_seg = None
        with torch.cuda.device(self._device), torch.no_grad():
            self._st = ops.lift_masks_stream_begin(_points64(points))
            self.text_features = _unit_text(text_embed)
            self._d4 = _pad_to(D, 4)
            self._text4 = _padded_text(self.text_features)

    def add(self, views):
        """One chunk of views (a MaskViews).  One host synchronisation (the read-back of the chunk's sizes)."""
        who = "LiftMasksStream.add"
        if views is None:
            raise ValueError(f"{who}: views must be a MaskViews, got NoneType")
        V, Q, h, w, H, W, C, D = _check_lift_masks(who, self._points, views, self._text, self.logit_scale, self.cut_bound, self.vis_thres,
                                                   self.min_visible, self.max_visible)
        this = (Q, (h, w), (H, W), _depth_kind(views.depth))
        self._check_chunk(who, this, V)
        V0, R0 = self.num_views, self.num_records
        Pm, Pl, Em = views.pred_masks, views.pred_logits, views.mask_embed
        E, M, K, Dp = views.view_entry, views.world_to_camera, views.intrinsics, views.depth
        n, dev, st, d4 = self._points.shape[0], self._device, self._st, self._d4
        with torch.cuda.device(dev), torch.no_grad():
            ve, w2c, intr, Dp = _view_args(E, M, K, Dp, self._render_chunk((H, W)))
            found, bufs = {}, {}

            def sizes(got):
                """in place of lift_masks_batched_lists' read-back: the stream's sizes, and the entry arrays out of the scratch"""
                s = ops.readback(ops.lift_masks_stream_sizes(st, ve, got["view_count"], got["view_keep"],
                                                             workspace=self._workspace("sizes", ops.lift_masks_stream_sizes_workspace_bytes(V))))
                total, kept, most = int(s[0]), int(s[1]), int(s[2])
                if R0 + kept > MAX_RECORDS:
                    raise ValueError(f"{who}: {kept} more visible (point, kept view) pairs after {R0}, at most 2^31 - 2 in all")
                found.update(total=total if kept else 0, kept=kept, most=most)
                if found["total"]:
                    pitch = _pad_to(total, 32)                  # (8-byte elements stay 256-byte aligned)
                    ent = self._workspace("entries", 28 * pitch)
                    for i, name in enumerate(("pt", "x", "y")):
                        bufs[name] = ent[8 * pitch * i:8 * pitch * i + 8 * total].view(torch.int64)
                    bufs["view"] = ent[24 * pitch:24 * pitch + 4 * total].view(torch.int32)
                return found["total"], most

            lists = ops.lift_masks_batched_lists(st.points, ve, w2c, intr, Dp, (H, W), self.cut_bound, float(self.vis_thres), self.min_visible,
                                                 _clamped(self.max_visible), buffers=bufs,
                                                 workspace=self._workspace("lists", ops.lift_masks_batched_lists_workspace_bytes(n, V)), sizes=sizes)
            total, kept = found["total"], found["kept"]
            # nothing of the stream has changed so far; from here on nothing is refused
            used = V0 + 1 if V0 else 0
            self._view_entry = _grown(self._view_entry, V0, V0 + V, (), torch.int64, dev)
            self._view_count = _grown(self._view_count, V0, V0 + V, (), torch.int64, dev)
            self._view_keep = _grown(self._view_keep, V0, V0 + V, (), torch.uint8, dev)
            self._view_pos = _grown(self._view_pos, V0, V0 + V, (), torch.int32, dev)
            self._rec_off = _grown(self._rec_off, used, V0 + V + 1, (), torch.int64, dev)
            self._f_seg = _grown(self._f_seg, V0, V0 + V, (Q, d4), torch.float32, dev)
            self._l_seg = _grown(self._l_seg, V0, V0 + V, (Q, C), torch.float32, dev)
            self._view_entry[V0:V0 + V], self._view_count[V0:V0 + V], self._view_keep[V0:V0 + V] = ve, lists.view_count, lists.view_keep
            pm = scores = taps = None
            if total:
                self._rec_row = _grown(self._rec_row, R0, R0 + kept, (), torch.int32, dev, most=MAX_RECORDS)
                self._rec_seg = _grown(self._rec_seg, R0, R0 + kept, (), torch.int32, dev, most=MAX_RECORDS)
                pm, taps = Pm.detach().contiguous(), _tap_tables(h, w, H, W, dev)
                scores = _mask_tables(Pl, Em, self.text_features, self.logit_scale, self._text4, self._f_seg[V0:V0 + V], self._l_seg[V0:V0 + V])[0]
            need = ops.lift_masks_stream_add_workspace_bytes(n, V, Q if total else 1, (h, w) if total else (1, 1), (H, W), total, dtype=Pm.dtype)
            ops.lift_masks_stream_add(st, ve, pm, scores, taps, (H, W), (lists.pt, lists.x, lists.y, lists.view), lists.view_off, lists.view_keep,
                                      total, self._rec_row, self._rec_seg, R0, self._rec_off[V0:V0 + V + 1], self._view_pos[V0:V0 + V],
                                      workspace=self._workspace("add", need))
        self._added(this, V)
        self.num_records, self.most_views = R0 + kept, max(self.most_views, found["most"])

    def finish(self, fill=True):
        """-> LiftedMasks over the views added so far; the stream goes on.  One host synchronisation (the status read-back)."""
        who = "LiftMasksStream.finish"
        self._check_started(who)
        n, D, d4, dev, V, R = self._points.shape[0], self.feature_dim, self._d4, self._device, self.num_views, self.num_records
        with torch.cuda.device(dev), torch.no_grad():
            if R == 0:
                feats, seen, count = _nothing_visible(n, D, dev)
                status = self._st.status
            else:
                words = max(1, -(-self.most_views // 64))
                r = ops.lift_masks_stream_finish(self._st, self._view_entry[:V], self._view_pos[:V], self._view_keep[:V], self._rec_off[:V + 1],
                                                 self._rec_row, self._rec_seg, R, words, self._f_seg, self._l_seg, fill=bool(fill),
                                                 workspace=self._workspace("finish", ops.lift_masks_stream_finish_workspace_bytes(n, V, R, words)))
                feats = _fill_rows(r.out, d4, r.nn, D)
                seen, count, status = r.seen.bool(), r.count, r.status
            view_count, view_keep = self._view_count[:V].clone(), self._view_keep[:V].bool()
            status = ops.readback(status)
        _raise_status(who, status, torn=_STREAM_TORN)
        return LiftedMasks(feats, seen, count, view_count, view_keep, self.text_features, self.logit_scale)


# ------------------------------------------------------------------------------------------ fused-feature files: the chain's end and a start
FUSE_FORMS = ("merged", "chunk")
FUSE_DTYPES = (torch.float16, torch.float32)


def _fuse_points(who, points):
    """the points of fuse / load_fused / dense as contiguous fp64 rows (only the batch column is read)"""
    _check_points(who, points)
    if not points.is_cuda:
        raise ValueError(f"{who}: points must be a CUDA tensor (got {points.device}); there is no CPU path")
    return points.detach().to(torch.float64).contiguous()


class FusedChunks:
    """The fused-feature files of a batch, on the device.  mask_full bool [num_files, N] in the points' row order; feat fp16 or fp32
    [R, D], the rows of file k of entry b are feat[offsets[k, b] : offsets[k, b + 1]] (ascending row order of the entry); offsets i64
    [num_files, B + 1], B = highest batch index + 1; mask bool [R] in feat's row order (the "chunk" form: the row was seen) or None
    (the "merged" form: mask_full holds seen points only).  points: the fp64 [N,4] rows the chunks were made for."""

    def __init__(self, points, mask_full, feat, offsets, mask, form):
        self.points, self.mask_full, self.feat, self.offsets, self.mask, self.form = points, mask_full, feat, offsets, mask, form
        self._offsets = self._rows = None

    @property
    def num_files(self):
        return self.mask_full.shape[0]

    @property
    def num_entries(self):
        return self.offsets.shape[1] - 1

    def _host_offsets(self):
        """offsets as nested lists: one read-back, made once"""
        if self._offsets is None:
            self._offsets = ops.readback(self.offsets)
        return self._offsets

    def _tables(self):
        """(offsets as nested lists, the rows of every entry), made once"""
        if self._rows is None:
            batch = self.points[:, 0]
            self._rows = [torch.nonzero(batch == b).reshape(-1) for b in range(self.num_entries)]
        return self._host_offsets(), self._rows

    def _pair(self, who, b, k):
        if not (isinstance(b, int) and isinstance(k, int) and 0 <= b < self.num_entries and 0 <= k < self.num_files):
            raise ValueError(f"{who}: entry {b!r} / file {k!r} outside 0..{self.num_entries - 1} / 0..{self.num_files - 1}")

    def file(self, b, k=0):
        """The dict the reader loads for file k of entry b (dataset/feature_loader.py:113-192), CPU tensors: "feat" [rows, D],
        "mask_full" bool [n_b], and in the chunk form "mask" bool [rows]."""
        self._pair("FusedChunks.file", b, k)
        off, rows = self._tables()
        lo, hi = off[k][b], off[k][b + 1]
        d = {"feat": self.feat[lo:hi].cpu(), "mask_full": self.mask_full[k].index_select(0, rows[b]).cpu()}
        if self.mask is not None:
            d["mask"] = self.mask[lo:hi].cpu()
        return d

    def save(self, out_dir, scene_names, skip_empty=False):
        """torch.save(self.file(b, k), out_dir/{scene_names[b]}_{k}.pt) for every entry and file -> the paths written.  A file without
        rows is refused (ValueError naming it, before anything is written): the reader drops scenes without files and its decoder
        refuses zero rows; skip_empty=True writes no file for it instead."""
        import os
        who = "FusedChunks.save"
        names = list(scene_names) if isinstance(scene_names, (list, tuple)) else None
        if names is None or len(names) != self.num_entries or not all(isinstance(s, str) and s for s in names):
            raise ValueError(f"{who}: scene_names must be {self.num_entries} names, one per entry 0..{self.num_entries - 1}, got {scene_names!r}")
        off, _ = self._tables()
        empty = [(b, k) for b in range(self.num_entries) for k in range(self.num_files) if off[k][b + 1] == off[k][b]]
        if empty and not skip_empty:
            b, k = empty[0]
            raise ValueError(f"{who}: file {k} of entry {b} ({names[b]}_{k}.pt) has no rows ({len(empty)} such files); skip_empty=True "
                             f"writes no file for them")
        os.makedirs(out_dir, exist_ok=True)
        paths = []
        for b in range(self.num_entries):
            for k in range(self.num_files):
                if (b, k) in empty:
                    continue
                paths.append(os.path.join(out_dir, f"{names[b]}_{k}.pt"))
                torch.save(self.file(b, k), paths[-1])
        return paths

    def dense(self, k=0):
        """(fp32 [N, D], bool [N]) on the device: feat's rows of file k at the points it holds, zero rows elsewhere, and mask_full[k] --
        the reader's evaluation form (dataset/feature_loader.py:119-126) on the unvoxelized points of all entries, ready for
        quantize(points, features).  ops.fuse_dense; read-backs: the offsets (once per FusedChunks) and the status."""
        self._pair("FusedChunks.dense", 0, k)
        with torch.cuda.device(self.points.device), torch.no_grad():
            off = self._host_offsets()
            lo, hi = off[k][0], off[k][-1]
            out, status = ops.fuse_dense(self.points, self.mask_full[k].to(torch.uint8), self.feat[lo:hi])
            st = ops.readback(status)
        if st[0]:
            raise ValueError(f"FusedChunks.dense: {st[0]} rows have a batch index that is no integer in 0..65535")
        if st[4] != hi - lo:
            raise ValueError(f"FusedChunks.dense: mask_full[{k}] selects {st[4]} points but feat holds {hi - lo} rows of file {k}")
        return out, self.mask_full[k]


def fuse(points, lifted, *, n_split_points=None, num_files=1, seed=0, form="merged", dtype=torch.float16):
    """The fused-feature files of a lifted batch: what dataset/feature_loader.py:113-192 reads, written with the settings of
    config/fusion_scannet.yaml:34-35 (n_split_points, num_rand_file_per_scene = num_files).  points [N,4] as lift takes them (only
    the batch column is read); lifted: a Lifted / LiftedMasks, or a (features fp32 | fp16 [N,D], seen bool [N]) pair.  Per entry b --
    its points the rows with batch b in ascending row order, local index i -- and file k:
      chunk_k = every point of the entry when n_split_points is None or n_b <= n_split_points, else the n_split_points points with
      the smallest key h = fmix32(i ^ c), c = fmix32(k ^ fmix32(b ^ fmix32(seed_lo ^ fmix32(seed_hi)))), fmix32 murmur3's 32-bit
      finaliser (x ^= x>>16; x *= 0x85ebca6b; x ^= x>>13; x *= 0xc2b2ae35; x ^= x>>16) -- a bijection, so the keys of one (entry,
      file) are distinct and the chunk has no ties; it depends neither on how the entries' rows interleave nor on any arrival order;
      form "merged" (the two-key file): mask_full = chunk_k & seen, feat = features[mask_full].to(dtype);
      form "chunk" (the three-key file): mask_full = chunk_k, feat = features[chunk_k].to(dtype), mask = seen[chunk_k].
    The conversion is torch's .to(dtype) to the bit (nearest even, inf on overflow, half subnormals kept, -0.0 kept, NaN stays NaN).
    -> FusedChunks (.file, .save, .dense).  No gradients.  Inside: ops.fuse_plan (entry tables, a radix select of the threshold key
    per selecting (file, entry), flags and scans per file), ONE read-back (the plan's status: the sizes that allocate feat and
    offsets, and the bad-row count -- at most the two the interface allows), ops.fuse_write (every source row loaded once, converted
    once, stored to each file that holds it).  Beside the outputs the call holds 4 * num_files * N bytes of scans and about 20 N bytes
    of tables.
    ValueError before any kernel: shape / dtype / device mismatches, CPU tensors, num_files outside 1..16, n_split_points < 1, seed
    outside 0..2^64-1, an unknown form or dtype; from the read-back: rows whose batch index is no integer in 0..65535."""
    who = "fuse"
    P = _fuse_points(who, points)
    n = P.shape[0]
    if isinstance(lifted, (tuple, list)) and len(lifted) == 2:
        Fe, seen = lifted
    elif hasattr(lifted, "features") and hasattr(lifted, "seen"):
        Fe, seen = lifted.features, lifted.seen
    else:
        raise ValueError(f"{who}: lifted must be a Lifted, a LiftedMasks or a (features, seen) pair, got {type(lifted).__name__}")
    if not torch.is_tensor(Fe) or Fe.dim() != 2 or Fe.shape[0] != n or Fe.shape[1] < 1 or Fe.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"{who}: features must be fp32 or fp16 [N, D] with N = {n} point rows, got "
                         f"{(list(Fe.shape), Fe.dtype) if torch.is_tensor(Fe) else type(Fe).__name__}")
    if not torch.is_tensor(seen) or seen.shape != (n,) or seen.dtype != torch.bool:
        raise ValueError(f"{who}: seen must be bool [{n}], got {(list(seen.shape), seen.dtype) if torch.is_tensor(seen) else type(seen).__name__}")
    if Fe.device != P.device or seen.device != P.device:
        raise ValueError(f"{who}: points, features and seen must be on one CUDA device (got {P.device} / {Fe.device} / {seen.device})")
    if isinstance(num_files, bool) or not isinstance(num_files, int) or not 1 <= num_files <= ops.FUSE_MAX_FILES:
        raise ValueError(f"{who}: num_files={num_files!r} outside 1..{ops.FUSE_MAX_FILES}")
    if n_split_points is not None and (isinstance(n_split_points, bool) or not isinstance(n_split_points, int) or n_split_points < 1):
        raise ValueError(f"{who}: n_split_points={n_split_points!r} must be None or an integer >= 1")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: seed={seed!r} outside 0..2^64-1")
    if form not in FUSE_FORMS:
        raise ValueError(f"{who}: form={form!r}, expected one of {FUSE_FORMS}")
    if dtype not in FUSE_DTYPES:
        raise ValueError(f"{who}: dtype={dtype!r}, expected torch.float16 or torch.float32")
    with torch.cuda.device(P.device), torch.no_grad():
        r = ops.fuse_batched(P, Fe.detach().contiguous(), seen.to(torch.uint8).contiguous(), n_split_points, num_files, seed, form, dtype)
    if r.status[0]:
        raise ValueError(f"{who}: {r.status[0]} rows have a batch index that is no integer in 0..65535")
    return FusedChunks(P, r.mask_full.bool(), r.feat, r.offsets, None if r.mask is None else r.mask.bool(), form)


def load_fused(points, files):
    """Fused-feature files back into the batched chain: files holds, per entry 0 .. B-1, a path, a dict as torch.load gives it, or
    None (an entry without a file: no rows).  Either form of dataset/feature_loader.py:113-192 -- "feat" and "mask_full", with "mask"
    (a bool mask or a list of row indices, :129-139) the three-key form -- but one form for all entries.  -> FusedChunks with
    num_files = 1 on the points' device; .dense() then gives what quantize takes.  Host work and copies only (the loader's side of
    the chain); ValueError where a file does not fit its entry's points."""
    who = "load_fused"
    P = _fuse_points(who, points)
    if not isinstance(files, (list, tuple)) or not files:
        raise ValueError(f"{who}: files must be a list with one path, dict or None per entry, got {type(files).__name__}")
    dev, n, B = P.device, P.shape[0], len(files)
    with torch.cuda.device(dev), torch.no_grad():
        batch = P[:, 0]
        mask_full = torch.zeros((1, n), dtype=torch.bool, device=dev)
        feats, masks, sizes, rows_of = [], [], [0], []
        for b in range(B):
            rows_of.append(torch.nonzero(batch == b).reshape(-1))
        covered = sum(int(r.numel()) for r in rows_of)
        if covered != n:
            raise ValueError(f"{who}: {n - covered} rows have a batch index that is no integer in 0..{B - 1} (one file per entry)")
        for b, f in enumerate(files):
            if f is None:
                sizes.append(sizes[-1])
                continue
            d = torch.load(f, map_location="cpu") if isinstance(f, (str, bytes)) or hasattr(f, "__fspath__") else f
            if not isinstance(d, dict) or "feat" not in d or "mask_full" not in d:
                raise ValueError(f"{who}: file of entry {b} must hold 'feat' and 'mask_full', got {sorted(d) if isinstance(d, dict) else type(d).__name__}")
            feat, mf = torch.as_tensor(d["feat"]), torch.as_tensor(d["mask_full"]).bool().reshape(-1)
            nb = int(rows_of[b].numel())
            if feat.dim() != 2 or feat.dtype not in FUSE_DTYPES or mf.shape[0] != nb or int(mf.sum()) != feat.shape[0]:
                raise ValueError(f"{who}: file of entry {b}: feat {list(feat.shape)} {feat.dtype}, mask_full [{mf.shape[0]}] with "
                                 f"{int(mf.sum())} points, for an entry of {nb} points")
            if "mask" in d:
                m = torch.as_tensor(d["mask"])
                if m.dtype != torch.bool:                                        # (a list of row indices, feature_loader.py:129-139)
                    m = torch.zeros(feat.shape[0], dtype=torch.bool).index_fill_(0, m.reshape(-1).long(), True)
                if m.shape != (feat.shape[0],):
                    raise ValueError(f"{who}: file of entry {b}: mask {list(m.shape)} for {feat.shape[0]} rows of feat")
                masks.append(m)
            mask_full[0, rows_of[b]] = mf.to(dev)
            feats.append(feat)
            sizes.append(sizes[-1] + feat.shape[0])
        if not feats:
            raise ValueError(f"{who}: no entry has a file")
        if masks and len(masks) != len(feats):
            raise ValueError(f"{who}: {len(masks)} of {len(feats)} files hold 'mask': one form for all entries")
        if len({(f.dtype, f.shape[1]) for f in feats}) != 1:
            raise ValueError(f"{who}: the files' feat differ in dtype or width: {sorted({(str(f.dtype), f.shape[1]) for f in feats})}")
        feat = torch.cat(feats).to(dev)
        mask = torch.cat(masks).to(dev) if masks else None
        offsets = torch.tensor([sizes], dtype=torch.int64, device=dev)
    return FusedChunks(P, mask_full, feat, offsets, mask, "chunk" if masks else "merged")


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


# ------------------------------------------------------------------------------------------ per-entry kNN, affinity, pooling
def _check_coordinates(who, C):
    if not torch.is_tensor(C) or C.dim() != 2 or C.shape[1] != 4:
        raise ValueError(f"{who}: coordinates must be [N, 4] (batch, x, y, z), got "
                         f"{list(C.shape) if torch.is_tensor(C) else type(C).__name__}")
    if C.dtype.is_floating_point or C.dtype.is_complex or C.dtype == torch.bool:
        raise ValueError(f"{who}: coordinates must be integers, got {C.dtype}")
    if not C.is_cuda:
        raise ValueError(f"{who}: coordinates must be a CUDA tensor (got {C.device}); there is no CPU path")
    if C.shape[0] == 0:
        raise ValueError(f"{who}: empty coordinate set")


def _check_k(who, k):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= GP_KNN_MAX_K:
        raise ValueError(f"{who}: K={k!r} outside 1..{GP_KNN_MAX_K}")


def _ordered_knn(who, C, k, same_as=None, extra=None, lists=True):
    """The checked coordinates C in the sorted order of ops.coords_order_batched -> (perm, rank i32 [N], nbr i32 [N,k] of sorted-row
    numbers).  Every refusal is raised from ONE status read-back (before it: the int32 range read-back of coordinates that are not
    int32 already).  same_as: a second coordinate tensor of C's shape that must equal C.
    extra: a function (perm, rank, keys) -> (i64 [m] device tensor, anything): its words ride in the same read-back, and the result is
    (perm, rank, nbr, keys, the m words as ints, the anything).  lists=False: no kNN (nbr is None), the caller has lists of its own."""
    with torch.cuda.device(C.device):
        C = C.detach()
        if C.dtype != torch.int32:
            # (range-checked before the cast: an int64 coordinate beyond int32 must not wrap into a valid one)
            lo, hi = ops.readback(torch.stack(torch.aminmax(C)).to(torch.int64))
            if lo < -2 ** 31 or hi >= 2 ** 31:
                raise ValueError(f"{who}: coordinates outside the int32 range ({lo} .. {hi})")
            C = C.to(torch.int32)
        C = C.contiguous()
        perm, rank, keys, order_status = ops.coords_order_batched(C)
        if lists:
            nbr, knn_status = ops.knn_batched(keys, perm, k)
        else:
            nbr, knn_status = None, torch.zeros(4, dtype=torch.int32, device=C.device)
        words, kept = extra(perm, rank, keys) if extra is not None else (torch.zeros(0, dtype=torch.int64, device=C.device), None)
        xyz = C[:, 1:]
        extent = (xyz.amax(0).to(torch.int64) - xyz.amin(0).to(torch.int64) + 1)
        differ = (same_as.to(torch.int64) != C.to(torch.int64)).sum() if same_as is not None else torch.zeros((), dtype=torch.int64, device=C.device)
        st = ops.readback(torch.cat([order_status.to(torch.int64), knn_status.to(torch.int64), extent, differ.reshape(1), words]))
    dups, bad_batch, bad_axes, short_rows, short_batch, short_count, axes15 = st[:7]
    extent, differ = st[7:10], st[10]
    if differ:
        raise ValueError(f"{who}: the embeddings' coordinates differ from x.C in {differ} elements (both must be the same rows in the same order)")
    # (range first: a row whose batch index is out of range has a meaningless key, which may equal another row's)
    if bad_batch:
        raise ValueError(f"{who}: {bad_batch} rows have a batch index outside 0..65535")
    if bad_axes:
        axes = [n for a, n in enumerate("xyz") if bad_axes >> a & 1]
        raise ValueError(f"{who}: coordinate extent of 65536 or more along {', '.join(axes)} (16 bits per axis)")
    if dups:
        raise ValueError(f"{who}: {dups} duplicate coordinate rows (MinkowskiEngine would merge them; quantise first)")
    wide = [n for a, n in enumerate("xyz") if extent[a] >= 32768 or axes15 >> a & 1]
    if wide:
        raise ValueError(f"{who}: coordinate extent of 32768 or more along {', '.join(wide)} ({'/'.join(str(e) for e in extent)} voxels; "
                         "squared distances must stay below 2^32)")
    if short_rows:
        raise ValueError(f"{who}: batch entry {short_batch} holds {short_count} voxels, K={k} neighbours need more than K "
                         f"({short_rows} rows are in such entries)")
    return (perm, rank, nbr) if extra is None else (perm, rank, nbr, keys, st[11:], kept)


def knn(coordinates, k):
    """Exact k nearest voxels inside each batch entry.  coordinates: integer [N,4] = batch, x, y, z on the GPU, any row order, unique
    rows.  -> int64 [N,k] of INPUT row numbers in the input's row order: row i lists the k nearest rows of i's entry in (d^2, row)
    order, itself dropped (the rule of ops.knn_lattice and the oracle; rows of other entries never appear, also where entries overlap).
    ValueError for duplicate rows, a batch index outside 0..65535, an axis extent of 32768 or more (over all entries), an entry of k or
    fewer voxels, k outside 1..127.  One status read-back (and a range read-back before it unless the coordinates are int32)."""
    _check_k("knn", k)
    _check_coordinates("knn", coordinates)
    perm, rank, nbr = _ordered_knn("knn", coordinates, k)
    with torch.cuda.device(coordinates.device):
        # sorted rows -> input rows, then the lists into the input's row order
        return perm.long()[nbr.long()].index_select(0, rank.long())


# ------------------------------------------------------------------------------------------ results carried to another cloud
INTERPOLATE_MODES = tuple(ops.KNN_INTERPOLATE_MODES)        # "inverse_distance", "nearest"
INTERPOLATE_DTYPES = tuple(ops.ELEM_TAG)                    # fp32, fp16, bf16


class Neighbors:
    """What knn_query returns and interpolate reads: indices i64 [M,k] (rows of the points, -1 in the slots past the entry's count),
    distances2 f64 [M,k] (the exact fp64 d^2 of the rule, +inf in those slots), num_points (N of the points the rows refer to; None
    for lists made by hand: interpolate then takes the length of index, or of values, as the range)."""

    def __init__(self, indices, distances2, num_points=None):
        self.indices, self.distances2, self.num_points = indices, distances2, num_points

    def transpose(self, index=None, num_rows=None, *, mode="inverse_distance", eps=1e-8):
        """The lists inverted for interpolate(..., differentiable=True): per row of values its references in ascending flat slot, with
        the forward's weights.  index, mode, eps: as the interpolate calls that will use it; num_rows: R of their values (with an
        index it must be given; without one it defaults to num_points).  The lists are constant over a training run: build this
        once and pass transpose= to every step.  -> NeighborsTranspose.  No host synchronisation."""
        who = "Neighbors.transpose"
        I, D2 = _check_lists(who, self)
        if index is not None and (not _is_int_tensor(index) or index.dim() != 1 or index.shape[0] < 1):
            raise ValueError(f"{who}: index must be an integer tensor [N] (point -> row of values), got "
                             f"{(list(index.shape), index.dtype) if torch.is_tensor(index) else type(index).__name__}")
        if num_rows is None and index is None:
            num_rows = self.num_points
        if isinstance(num_rows, bool) or not isinstance(num_rows, int) or not 1 <= num_rows < 2 ** 31:
            raise ValueError(f"{who}: num_rows={num_rows!r} must be the row count of values, an int in 1..2^31-1"
                             f"{' (an index does not tell it)' if index is not None else ''}")
        span, what = (num_rows, "num_rows") if index is None else (index.shape[0], "index")
        if self.num_points is not None and span != self.num_points:
            raise ValueError(f"{who}: {what} {'is' if index is None else 'holds'} {span} rows, the lists name rows of {self.num_points} points")
        _check_mode_eps(who, mode, eps)
        _check_slots(who, I)
        _check_one_device(who, "nb and index", [I, D2] + ([] if index is None else [index]))
        with torch.cuda.device(I.device), torch.no_grad():
            idx = None if index is None else index.detach().to(torch.int64).contiguous()
            return _transpose(I.detach().contiguous(), D2.detach().contiguous(), idx, num_rows, mode, float(eps))


class NeighborsTranspose:
    """What Neighbors.transpose returns and interpolate(differentiable=True) applies in its backward: offsets i64 [R+1], slots i32
    [M*k] (the references of row r of values are the flat slots j * k + s at slots[offsets[r] : offsets[r+1]], ascending; offsets[R]
    counts them), weights f32 [M*k] (the forward's fp32 weights in that order), and what it was built for: M, k, R, mode, eps."""

    def __init__(self, offsets, slots, weights, M, k, R, mode, eps):
        self.offsets, self.slots, self.weights = offsets, slots, weights
        self.M, self.k, self.R, self.mode, self.eps = M, k, R, mode, eps


def _transpose(I, D2, idx, R, mode, eps):
    w = ops.knn_interpolate_weights(I, D2, idx, R, mode, eps)
    offsets, slots, weights = ops.knn_interpolate_transpose(I, w, idx, R, mode)
    return NeighborsTranspose(offsets, slots, weights, I.shape[0], I.shape[1], R, mode, eps)


class _Interpolate(torch.autograd.Function):
    """out = ops.knn_interpolate(values, ...); d values[r] = sum over the references f = j * k + s of r, in ascending f, of w32[f] *
    d out[j] (ops.knn_interpolate_backward over a NeighborsTranspose: fp32, one rounding to the dtype of values)"""

    @staticmethod
    def forward(ctx, values, I, D2, idx, mode, eps, status, transpose):
        ctx.lists, ctx.transpose, ctx.dtype, ctx.R = (I, D2, idx, mode, eps), transpose, values.dtype, values.shape[0]
        return ops.knn_interpolate(values.detach(), I, D2, idx, mode, eps, buffers=None if status is None else {"status": status})

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        with torch.cuda.device(d_out.device):
            g = d_out.float()
            if g.stride(1) != 1 or g.stride(0) < g.shape[1]:
                g = g.contiguous()
            t = ctx.transpose if ctx.transpose is not None else _transpose(*ctx.lists[:3], ctx.R, *ctx.lists[3:])
            return ops.knn_interpolate_backward(g, t.offsets, t.slots, t.weights, t.k, ctx.dtype), None, None, None, None, None, None, None


def _check_lists(who, nb):
    I, D2 = nb.indices, nb.distances2
    if not torch.is_tensor(I) or not torch.is_tensor(D2) or I.dtype != torch.int64 or D2.dtype != torch.float64 or I.dim() != 2 \
            or D2.shape != I.shape or I.shape[0] < 1 or not 1 <= I.shape[1] <= GP_KNN_QUERY_MAX_K:
        raise ValueError(f"{who}: nb must hold indices i64 [M, k] and distances2 f64 [M, k] with M >= 1 and k in 1..{GP_KNN_QUERY_MAX_K}, got "
                         f"{_shape_of(I)} and {_shape_of(D2)}")
    return I, D2


def _check_mode_eps(who, mode, eps):
    if mode not in INTERPOLATE_MODES:
        raise ValueError(f"{who}: mode={mode!r} must be one of {INTERPOLATE_MODES}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0 <= eps < float("inf"):
        raise ValueError(f"{who}: eps={eps!r} must be a finite number >= 0")


def _check_slots(who, I):
    if I.shape[0] * I.shape[1] > ops.KNN_INTERPOLATE_MAX_SLOTS:
        raise ValueError(f"{who}: M * k = {I.shape[0] * I.shape[1]} flat slots, more than 2^31-1: the backward numbers them in i32")


def _check_cloud(who, name, letter, P):
    """_check_points' checks and words for a cloud called `name`"""
    if not torch.is_tensor(P) or P.dim() != 2 or P.shape[1] != 4:
        raise ValueError(f"{who}: {name} must be [{letter}, 4] (batch, x, y, z), got {_shape_of(P)}")
    if P.dtype not in (torch.float64, torch.float32):
        raise ValueError(f"{who}: {name} must be fp64 or fp32, got {P.dtype}")
    n = P.shape[0]
    if n == 0 or n >= 2 ** 31:
        raise ValueError(f"{who}: {n} {name} outside 1..2^31-1")


def knn_query(points, queries, k):
    """The k nearest points of one cloud for every point of another, inside each batch entry, exactly: the way from a working cloud to
    the vertices a benchmark scores on, or from an annotated mesh to the working cloud (the reference's preprocessors keep the two
    apart; its KDTree queries, models/affinity_module.py:445-447, 693-697, are the k = 1, one-scene case).  points [N,4] and queries
    [M,4]: fp64 or fp32, columns batch, x, y, z, on one GPU, any row order; entries may overlap in space and interleave in rows;
    duplicate rows are allowed.  k: an int in 1..32.  -> Neighbors(indices i64 [M,k], distances2 f64 [M,k]).
      The rule, the library's for float clouds (lift's scene-level fill): xyz is rounded to fp32 first; d^2 = (dx*dx + dy*dy) + dz*dz
        in fp64, each operation rounded once; row j lists the points of query j's own entry in ascending (d^2, row).  indices are
        input rows of points, distances2 those exact fp64 values.  A query never matches across entries.  A point that coincides
        with a query is an ordinary neighbour at distance 0: nothing is dropped, unlike knn.
      Short entries.  A query whose entry holds fewer than k points, none included, has -1 and +inf in the slots past the entry's
        count: data, not an error.
    No gradients.  Inside: ops.knn_query (the points' entry table, per entry a bounding box and a uniform grid of at most as many cells
    as it has points, a wave per query walking the grid's shells, the queries it leaves scanning their entry), then ONE status
    read-back, the call's only host synchronisation.  ValueError before any kernel: k that is a bool, no int or outside 1..32; points
    or queries that are no fp64 / fp32 [*, 4] tensor with 1..2^31-1 rows; CPU tensors or two devices; from the read-back: rows of
    points, or of queries, with a value that is not finite or with a batch index that is no integer in 0..65535."""
    who = "knn_query"
    P, Q = points, queries
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= GP_KNN_QUERY_MAX_K:
        raise ValueError(f"{who}: k={k!r} outside 1..{GP_KNN_QUERY_MAX_K}")
    _check_cloud(who, "points", "N", P)
    _check_cloud(who, "queries", "M", Q)
    _check_one_device(who, "points and queries", [P, Q])
    with torch.cuda.device(P.device), torch.no_grad():
        indices, dist2, st = ops.knn_query(_points64(P), _points64(Q), k)
        status = ops.readback(st)
    for name, base in (("points", 0), ("queries", 8)):
        if status[base + 2]:
            raise ValueError(f"{who}: {status[base + 2]} rows of {name} are not finite")
        if status[base]:
            raise ValueError(f"{who}: {status[base]} rows of {name} have a batch index that is no integer in 0..65535")
    return Neighbors(indices, dist2, P.shape[0])


def interpolate(values, nb, *, index=None, mode="inverse_distance", eps=1e-8, unlabeled=255, status=None, differentiable=False,
                transpose=None):
    """Rows carried through the lists of knn_query: purified features or predictions of the working cloud delivered on another
    cloud's points.  nb: the Neighbors of knn_query(points, queries, k).
      values floating [R,D] (fp32, fp16 or bf16; any row stride, unit column stride; read in place) -> fp32 [M,D], contiguous.
        mode "inverse_distance": w_j = 1 / (d^2_j + eps) in fp64 over the valid slots, normalised in fp64 and rounded to fp32; out =
        sum_j w_j v_j accumulated in fp32 in list order.  With eps = 0 a row with zero-distance neighbours takes the mean of exactly
        those.  mode "nearest": slot 0.  A query with no valid slot gives a zero row.  A half input gives the bits of the same call on
        its fp32 upcast.
      values integer [R] (labels, predictions) -> int64 [M]: the value at slot 0 whatever the mode, `unlabeled` where there is none.
      index: an optional integer [N], point -> row of values, as in Rendered.features: pass q.inverse_mapping to read per-voxel rows
        through per-point lists.  Without it R == N.
    A list entry outside -1..N-1 or an index value outside 0..R-1 is never dereferenced: the row comes back zero / `unlabeled` and is
    counted.  The counts stay on the device and nothing is read back: pass status, an int64 [2] tensor on the values' device, to
    receive (rows with such a list entry, rows with such an index value).
    differentiable=False (the default): values.requires_grad is ignored and the result is detached.
    differentiable=True: floating values that require grad, under enabled grad mode, get the same forward bits inside the autograd
      graph; values that need no gradient get the plain result.  backward returns d_values [R,D], contiguous (whatever the pitch of
      values), in the dtype of values.  The rule: a reference is a flat slot f = j*k + s whose forward weight is in effect -- slot s is
      one the mode reads ("nearest": slot 0 only, weight 1), its list entry is valid, its row r = index[indices[j,s]] (or
      indices[j,s]) is valid, and query row j is not excused: a query row with any list entry outside -1..N-1 or any index value
      outside 0..R-1 is a zero row in the forward and contributes no reference.  d_values[r,c] starts at +0.f and takes, over the
      references of r in ascending f, acc = acc + w32[f] * g[j,c] with the product rounded once and the sum rounded once in fp32
      (the library builds with -ffp-contract=off), w32 the forward's own fp32 weight; fp16 / bf16 are rounded once at the end.  A
      row without references gets an explicit zero row.  The result depends on nothing but the inputs: no float atomics, two calls
      give the same bits.  No gradient to nb.distances2, to the weights or to any coordinate; no double backward.
      transpose: a NeighborsTranspose of nb.transpose(index, R, mode=mode, eps=eps), built once for a training run; without it
      every backward builds its own.  ValueError: integer values; M * k > 2^31-1 (flat slots are i32); a transpose whose (M, k,
      R, mode, eps) are not the call's.
    Inside: ops.knn_interpolate (a wave per query row: the list read once, the weights in fp64 by k lanes, the rows gathered by the
    widest loads the row stride allows), no host synchronisation; the backward: ops.knn_interpolate_weights (the forward's device
    code), ops.knn_interpolate_transpose (a stable radix sort of (row, flat slot) pairs), ops.knn_interpolate_backward (a wave per row
    of values walking its list in order).  ValueError: an nb that is no Neighbors; values that are neither
    floating [R,D] of the three dtypes with unit column stride nor integer [R]; an index that is no integer [N]; R (or the index's
    length) other than the N of nb; a mode outside INTERPOLATE_MODES; eps no finite number >= 0; unlabeled no int; CPU tensors or two
    devices."""
    who = "interpolate"
    V = values
    if not isinstance(nb, Neighbors):
        raise ValueError(f"{who}: nb must be the Neighbors of knn_query, got {type(nb).__name__}")
    I, D2 = _check_lists(who, nb)
    labels = _is_int_tensor(V)
    if labels:
        if V.dim() != 1 or V.shape[0] < 1:
            raise ValueError(f"{who}: integer values must be [R] with R >= 1, got {list(V.shape)}")
    elif not torch.is_tensor(V) or V.dtype not in INTERPOLATE_DTYPES or V.dim() != 2 or min(V.shape) < 1:
        raise ValueError(f"{who}: values must be fp32, fp16 or bf16 [R, D] with R, D >= 1, or an integer tensor [R], got "
                         f"{(list(V.shape), V.dtype) if torch.is_tensor(V) else type(V).__name__}")
    elif V.stride(1) != 1 or V.stride(0) < V.shape[1]:
        raise ValueError(f"{who}: values must have unit column stride and a row stride >= D, got strides {V.stride()}")
    if index is not None and (not _is_int_tensor(index) or index.dim() != 1 or index.shape[0] < 1):
        raise ValueError(f"{who}: index must be an integer tensor [N] (point -> row of values), got "
                         f"{(list(index.shape), index.dtype) if torch.is_tensor(index) else type(index).__name__}")
    span, what = (V.shape[0], "values") if index is None else (index.shape[0], "index")
    if nb.num_points is not None and span != nb.num_points:
        raise ValueError(f"{who}: {what} holds {span} rows, the lists name rows of {nb.num_points} points"
                         f"{' (pass index, point -> row of values)' if index is None else ''}")
    _check_mode_eps(who, mode, eps)
    if isinstance(unlabeled, bool) or not isinstance(unlabeled, int) or not -2 ** 63 <= unlabeled < 2 ** 63:
        raise ValueError(f"{who}: unlabeled={unlabeled!r} must be an int")
    if status is not None and (not torch.is_tensor(status) or status.dtype != torch.int64 or status.shape != (2,) or not status.is_contiguous()):
        raise ValueError(f"{who}: status must be a contiguous int64 [2] tensor, got {_shape_of(status)}")
    if not isinstance(differentiable, bool):
        raise ValueError(f"{who}: differentiable={differentiable!r} must be a bool")
    if transpose is not None and not differentiable:
        raise ValueError(f"{who}: transpose goes with differentiable=True")
    if differentiable:
        if labels:
            raise ValueError(f"{who}: differentiable=True takes floating values, got {V.dtype}")
        _check_slots(who, I)
        t = transpose
        if t is not None:
            if not isinstance(t, NeighborsTranspose):
                raise ValueError(f"{who}: transpose must be the NeighborsTranspose of nb.transpose, got {type(t).__name__}")
            mine, its = (I.shape[0], I.shape[1], V.shape[0], mode, float(eps)), (t.M, t.k, t.R, t.mode, float(t.eps))
            if mine != its:
                raise ValueError(f"{who}: transpose was built for (M, k, R, mode, eps) = {its}, this call has {mine}")
    _check_one_device(who, "values, nb, index, status and transpose",
                      [V, I, D2] + [t for t in (index, status) if t is not None] + ([] if transpose is None else [transpose.offsets]))
    idx = None if index is None else index.detach().to(torch.int64).contiguous()
    if differentiable and V.requires_grad and torch.is_grad_enabled():
        with torch.cuda.device(V.device):
            return _Interpolate.apply(V, I.detach().contiguous(), D2.detach().contiguous(), idx, mode, float(eps), status, transpose)
    with torch.cuda.device(V.device), torch.no_grad():
        vals = V.detach().to(torch.int64).contiguous() if labels else V.detach()
        return ops.knn_interpolate(vals, I.detach().contiguous(), D2.detach().contiguous(), idx, mode, float(eps), unlabeled,
                                   buffers=None if status is None else {"status": status})


# ------------------------------------------------------------------------------------------ the geometry columns: normals
def mesh_normals(points, faces):
    """The vertex normals the reference's loader hands the student (dataset/data_loader_ablation.py:162-163), computed the
    reference's way from the scans' meshes (models/utils/dataset_utils.py:198-199 -> vertex_normal, models/utils/mapping_util.py:9-29)
    -- for the meshes of all entries in one call, entries never mixing, bit for bit.  points fp64 or fp32 [N,4] = batch, x, y, z
    exactly as lift takes them; faces integer [F,3] of ROW NUMBERS INTO points, in any order, the faces of different entries
    interleaved at will.  -> normals [N,3] of the points' dtype: for every entry what vertex_normal returns on that entry alone with
    local indices.
      Arithmetic.  All in the dtype of points, every operation rounded once: vec = cross(p1 - p0, p2 - p0) with each product rounded
        before the difference; length = sqrt((vec0^2 + vec1^2) + vec2^2) + 1e-8; the face contributes (vec / length) * (length * 0.5)
        to each of its vertices, once to a vertex it names twice; a vertex sums its faces in ascending face index from 0; normal = sum
        / (sqrt((s0^2 + s1^2) + s2^2) + 1e-8).  A vertex of no face gets a zero row, a zero-area face contributes zeros.
      Order.  A vertex's faces come from a stable sort of (vertex, face) pairs, never from atomics on floats: two calls give the same
        bits, and permuting the face rows changes a vertex's bits only where it changes the order of that vertex's own faces.
    No gradients.  Inside: ops.mesh_normals_batched (a row check, one lane per face, the library's radix sort, one lane per vertex),
    one read-back.  ValueError before any kernel: lift's refusals for points, faces that are no integer [F,3] with F >= 1, CPU tensors
    or two devices; from the ONE status read-back: non-finite rows, rows whose batch index is no integer in 0..65535, faces with an
    index outside 0..N-1, faces whose three rows belong to different entries."""
    who = "mesh_normals"
    P, Fc = points, faces
    _check_points(who, P)
    if not _is_int_tensor(Fc) or Fc.dim() != 2 or Fc.shape[1] != 3:
        raise ValueError(f"{who}: faces must be an integer tensor [F, 3] of rows of points, got "
                         f"{(list(Fc.shape), Fc.dtype) if torch.is_tensor(Fc) else type(Fc).__name__}")
    if Fc.shape[0] == 0:
        raise ValueError(f"{who}: no faces (F = 0): a cloud without a mesh takes estimate_normals")
    if Fc.shape[0] * 3 >= 2 ** 31:
        raise ValueError(f"{who}: {Fc.shape[0]} faces, at most {(2 ** 31 - 1) // 3}")
    _check_one_device(who, "points and faces", [P, Fc])
    with torch.cuda.device(P.device), torch.no_grad():
        normals, st = ops.mesh_normals_batched(P.detach().contiguous(), Fc.detach().to(torch.int64).contiguous())
        status = ops.readback(st)
    _raise_status(who, status)
    if status[6]:
        raise ValueError(f"{who}: {status[6]} faces have an index outside 0..{P.shape[0] - 1}")
    if status[7]:
        raise ValueError(f"{who}: {status[7]} faces name rows of different batch entries")
    return normals


class Normals:
    """normals fp32 [N,3] and variation fp32 [N] per point (its voxel's), voxel_normals fp32 [nv,3] and voxel_variation fp32 [nv] per
    voxel in the row order of quantized.coordinates, positions fp32 [nv,3] (the voxel centroids the covariance was taken over),
    quantized (the Quantized of the points: quantized.inverse_mapping leads from a point to its voxel)."""

    def __init__(self, normals, variation, voxel_normals, voxel_variation, positions, quantized):
        self.normals, self.variation, self.voxel_normals, self.voxel_variation = normals, variation, voxel_normals, voxel_variation
        self.positions, self.quantized = positions, quantized


def estimate_normals(points, *, quantization_size, k=16, toward=None, quantized=None):
    """Normals for a cloud that comes without faces (poses plus a reconstructed cloud, the depth="render" case): per voxel the
    direction of least spread of the voxel's centroid and its k nearest voxels' inside the entry, handed back to every point of the
    voxel -- the stand-in for mesh_normals in the student's geometry columns.  points as lift takes them (fp64 or fp32 [N,4]);
    quantization_size as quantize takes it; 3 <= k <= 127.  toward orients the normals: None (the component of largest magnitude is
    made positive, the lowest axis among equal magnitudes), floating [B,3] (one viewpoint per entry, indexed by the batch column; B
    must exceed the highest batch index), or floating [N,3] (one target per point; a voxel takes that of its lowest point).  A
    per-point target is, for example, the centre of the camera nearest to each point, which a caller has in two lines of torch:
        centres = torch.linalg.inv(world_to_camera)[:, :3, 3]                 # [V,3]
        toward = centres[torch.cdist(points[:, 1:], centres).argmin(1)]       # (per entry where the entries' views differ)
    A vector is flipped where <n, target - centroid> < 0.  (toward of N rows is read per point, of any other length per entry.)
      1. q = quantize(points, xyz as fp32 features, mode="average", quantization_size=...); a caller who quantised the same points at the
         same size already passes quantized=q (with or without features) and saves that call's read-backs.
      2. The voxel centroids are the three averaged columns (with quantized=q, whatever features q holds, xyz is averaged over q's
         voxels by the same kernel in the same order, without a read-back: the same bits).
      3. The lists are knn(q.coordinates, k): exact, inside each entry, so overlapping entries never see each other.
      4. ops.knn_normals on the centroids, fp64 inside.
      5. normals = voxel_normals[q.inverse_mapping].
    -> Normals.  No gradients.  ValueError: lift's refusals for points, k outside 3..127, a toward that is no floating [B,3] / [N,3], a
    quantized of another length; quantize's refusals; knn's, unchanged (an entry of k or fewer voxels, an axis extent of 32768 or more);
    a [B,3] toward with B not above the highest batch index.  Read-backs: quantize's (none with quantized=), knn's one, and one of
    two status words after the kernel."""
    who = "estimate_normals"
    P = points
    _check_points(who, P)
    if isinstance(k, bool) or not isinstance(k, int) or not ops.KNN_NORMALS_MIN_K <= k <= GP_KNN_MAX_K:
        raise ValueError(f"{who}: k={k!r} outside {ops.KNN_NORMALS_MIN_K}..{GP_KNN_MAX_K}")
    N = P.shape[0]
    if toward is not None and (not torch.is_tensor(toward) or not toward.dtype.is_floating_point or toward.dim() != 2 or toward.shape[1] != 3
                               or toward.shape[0] < 1):
        raise ValueError(f"{who}: toward must be None, floating [B, 3] (a viewpoint per entry) or floating [{N}, 3] (a target per point), got "
                         f"{(list(toward.shape), toward.dtype) if torch.is_tensor(toward) else type(toward).__name__}")
    if quantized is not None and (not isinstance(quantized, Quantized) or quantized.inverse_mapping.shape[0] != N):
        raise ValueError(f"{who}: quantized must be the Quantized of these {N} points, got "
                         f"{quantized.inverse_mapping.shape[0] if isinstance(quantized, Quantized) else type(quantized).__name__}"
                         f"{' rows' if isinstance(quantized, Quantized) else ''}")
    _check_one_device(who, "points, toward and quantized",
                      [P] + ([toward] if toward is not None else []) + ([quantized.coordinates] if quantized is not None else []))
    with torch.cuda.device(P.device), torch.no_grad():
        xyz = P.detach()[:, 1:].to(torch.float32)
        q = quantized
        if q is None:
            q = quantize(P.detach(), xyz, mode="average", quantization_size=quantization_size)
            centroids = q.features
        else:
            # the CSR form of q (a voxel's points in ascending row, as quantize reduced them) from what a Quantized keeps
            nv = q.coordinates.shape[0]
            order = torch.argsort(q.inverse_mapping, stable=True)
            seg_start = torch.cat([torch.zeros(1, dtype=torch.int64, device=P.device), torch.cumsum(q.counts.to(torch.int64), 0).clamp(max=N)])
            centroids = torch.empty((nv, 3), dtype=torch.float32, device=P.device)
            ops.scatter_mean_csr(_rows_f32(xyz), 3, order, seg_start, nv, centroids)
        nbr = knn(q.coordinates, k)
        rows = None
        if toward is not None:
            rows = q.unique_index if toward.shape[0] == N else q.coordinates[:, 0]
        status = torch.empty(2, dtype=torch.int64, device=P.device)
        vn, vv = ops.knn_normals(centroids.detach(), nbr, toward, rows, buffers={"status": status})
        bad_list, bad_toward = ops.readback(status)
        if bad_toward:
            raise ValueError(f"{who}: toward holds {toward.shape[0]} viewpoints, but {bad_toward} voxels are in entries beyond them")
        if bad_list:
            raise RuntimeError(f"{who}: {bad_list} neighbour lists name rows outside the voxels: the inputs changed during the call")
        inv = q.inverse_mapping
        return Normals(vn[inv], vv[inv], vn, vv, centroids, q)


_MODE_OF_FAMILY = {"cs": "mfma_cs", "chain": "mfma_chain", "mfma": "mfma", "mfma_persist": "mfma_persist", "tiles": "tiles", "ell": "ell"}


def pool_family(D, K, num_iters, pool_mode="auto"):
    """The pooling kernel family affinity_pool runs at width D: pipeline.resolve_pool_mode's choice at D padded to a multiple of 4, with
    HotPath's default tile and block heights -- the column-sliced matrix-core kernels at 256 / 512 / 768 columns, the fp32 tiles at
    multiples of 512 they do not take -- and the ELL kernel for every other width (the 64-wide tile kernel is config P's own)."""
    from .pipeline import resolve_pool_mode
    Dp = (D + 3) // 4 * 4
    family = resolve_pool_mode(pool_mode, Dp, K, num_iters, 8, 64)
    return "ell" if family == "tiles" and Dp % 512 else family


GRAD_EMBED_WIDTHS = (16, 32, 64, 128)                       # gp_affinity_softmax's


class _PoolGrad(torch.autograd.Function):
    """affinity_pool(differentiable=True) behind the checks: feats [N,D], emb [N,d] in the input's row order -> Y fp32 [N,D].
    Forward: num_iters single applications of ops.pool_ell into one stack [T, N, Dp] of fp32 rows (X_0 .. X_{T-1}, which the weight
    gradient reads).  Backward, in the sorted key order, with G_T = dY and for t = T .. 1:
        dw[i,j] += <G_t[i], X_{t-1}[nbr[i,j]]>                       ops.pool_ell_wgrad
        G_{t-1}[m] = sum over (i,j) with nbr[i,j] = m of w[i,j] G_t[i]  ops.pool_ell_transpose over ops.pool_transpose_build's index
    then d feats = G_0, and d emb through ops.affinity_softmax_backward and ops.l2norm_rows_backward.  The lists are not differentiated."""

    @staticmethod
    def forward(ctx, feats, emb, perm64, rank64, nbr, K, sharpen, num_iters, normalize):
        dev = feats.device
        n, D = feats.shape
        Dp, T = (D + 3) // 4 * 4, num_iters
        stack = torch.empty((T, n, Dp), dtype=torch.float32, device=dev)
        if Dp != D:
            stack[0].zero_()                                             # (the padding columns D .. Dp-1 of X_0; every later X_t is written whole)
        ops.gather_rows(_rows_f32(feats.detach()), D, perm64, out=stack[0])
        e_raw = ops.gather_rows(_rows_f32(emb.detach()), emb.shape[1], perm64)
        e_unit = ops.l2norm_rows_(e_raw.clone()) if normalize else e_raw
        w = ops.affinity_softmax(e_unit, nbr, sharpen)
        for t in range(1, T):
            ops.pool_ell(stack[t - 1], nbr, w, Dp, stack[t])
        out = torch.empty((n, Dp), dtype=torch.float32, device=dev)
        ops.pool_ell(stack[T - 1], nbr, w, Dp, out)
        ctx.save_for_backward(stack, w, nbr, e_raw, e_unit, perm64, rank64)
        ctx.args = (D, Dp, T, K, sharpen, normalize, feats.dtype, emb.dtype)
        return ops.gather_rows(out, D, rank64)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_y):
        stack, w, nbr, e_raw, e_unit, perm64, rank64 = ctx.saved_tensors
        D, Dp, T, K, sharpen, normalize, f_dtype, e_dtype = ctx.args
        need_x, need_e = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dev = w.device
        n = w.shape[0]
        with torch.cuda.device(dev):
            g = torch.zeros((n, Dp), dtype=torch.float32, device=dev) if Dp != D else torch.empty((n, D), dtype=torch.float32, device=dev)
            ops.gather_rows(_rows_f32(d_y), D, perm64, out=g)
            tr_off, tr_slot = ops.pool_transpose_build(nbr)
            dw = torch.empty((n, K), dtype=torch.float32, device=dev) if need_e else None
            spare = torch.empty_like(g) if need_x or (need_e and T > 1) else None
            for t in range(T, 0, -1):
                if need_e:
                    ops.pool_ell_wgrad(g, stack[t - 1], nbr, dw, accumulate=t < T)
                if need_x or (need_e and t > 1):
                    ops.pool_ell_transpose(g, tr_off, tr_slot, w, K, spare)
                    g, spare = spare, g
            d_feats = ops.gather_rows(g, D, rank64).to(f_dtype) if need_x else None
            d_emb = None
            if need_e:
                de = ops.affinity_softmax_backward(e_unit, nbr, w, dw, sharpen, tr_off, tr_slot)
                if normalize:
                    de = ops.l2norm_rows_backward(e_raw, de)
                d_emb = ops.gather_rows(de, de.shape[1], rank64).to(e_dtype)
        return d_feats, d_emb, None, None, None, None, None, None, None


def affinity_pool(x, embeddings, *, K=96, sharpen=20.0, num_iters=19, normalize=True, pool_mode="auto", differentiable=False):
    """The purifying step of evaluate_scene (models/affinity_module.py:1547-1587) over a batched SparseTensor, every batch entry by
    itself.  x: an ME-style SparseTensor (.F [N,D] floating, .C integer [N,4] = batch, x, y, z in any row order, unique rows);
    embeddings: a SparseTensor with the same .C (the student's output) or a tensor [N,d].  Per entry: E = normalize(E) when
    `normalize`, w = softmax_j(sharpen * <E_i, E_nbr(i,j)>) over the K exact nearest voxels of the entry, then num_iters applications
    of the row-stochastic operator (num_iters=0 returns the features).  -> type(x)(features=Y, coordinates=x.C), Y fp32 [N,D] in x's
    row order.
    Like the reference's @torch.no_grad() evaluate_scene this takes NO gradients by default: inputs that require grad are detached, Y
    never requires grad.
    differentiable=True: Y is part of the autograd graph whenever grad mode is on and x.F or the embeddings require grad (otherwise the
    call is the default one).  Gradients reach x.F and the embeddings (a tensor or a SparseTensor's .F) in their row order and dtype;
    the neighbour lists are discrete and not differentiated; no double backward.  num_iters=0: Y carries x.F's values with the identity
    gradient, the embeddings receive none.  The forward then is num_iters single applications of ops.pool_ell that keep X_0 .. X_{T-1}
    for the weight gradient in one fp32 stack of T * N * Dp * 4 bytes (Dp = D padded to a multiple of 4; 5.2 GB at 134k voxels x 512 x
    19) -- there is no recompute mode.  The matrix-core families keep no fp32 intermediates: pool_mode other than "auto" / "ell"
    together with differentiable=True is a ValueError, as is an embedding width outside 16 / 32 / 64 / 128, both before any kernel.
    Inside: the sorted order of ops.coords_order_batched, ops.knn_batched, ops.l2norm_rows_, ops.affinity_softmax and HotPath's pooling
    (pool_family(D, K, num_iters, pool_mode); the operator is built in the key order).  ValueError, all before any pooling kernel and
    from one status read-back: see knn; also num_iters < 0, shape / dtype / device mismatches, embeddings whose coordinates differ."""
    from .pipeline import HotPath
    who = "affinity_pool"
    if not (hasattr(x, "F") and hasattr(x, "C")):
        raise ValueError(f"{who}: x must be a SparseTensor (an object with .F and .C), got {type(x).__name__}")
    Fe, C = x.F, x.C
    _check_k(who, K)
    if isinstance(num_iters, bool) or not isinstance(num_iters, int) or num_iters < 0:
        raise ValueError(f"{who}: num_iters={num_iters!r} must be an integer >= 0")
    _check_coordinates(who, C)
    n = C.shape[0]
    if not torch.is_tensor(Fe) or Fe.dim() != 2 or Fe.shape[0] != n or Fe.shape[1] < 1:
        raise ValueError(f"{who}: features must be [N, D] with N = {n} coordinate rows, got "
                         f"{list(Fe.shape) if torch.is_tensor(Fe) else type(Fe).__name__}")
    E, CE = (embeddings.F, embeddings.C) if hasattr(embeddings, "F") and hasattr(embeddings, "C") else (embeddings, None)
    if not torch.is_tensor(E) or E.dim() != 2 or E.shape[0] != n or E.shape[1] < 1:
        raise ValueError(f"{who}: embeddings must be [N, d] with N = {n} coordinate rows, got "
                         f"{list(E.shape) if torch.is_tensor(E) else type(E).__name__}")
    if not (Fe.dtype.is_floating_point and E.dtype.is_floating_point):
        raise ValueError(f"{who}: features and embeddings must be floating point, got {Fe.dtype} / {E.dtype}")
    if not (Fe.is_cuda and E.is_cuda) or Fe.device != C.device or E.device != C.device:
        raise ValueError(f"{who}: features, embeddings and coordinates must be CUDA tensors on one device (got {Fe.device} / {E.device} / "
                         f"{C.device}); there is no CPU path")
    if CE is not None and CE is not C:
        if not torch.is_tensor(CE) or CE.shape != C.shape or CE.device != C.device or CE.dtype.is_floating_point:
            raise ValueError(f"{who}: the embeddings' coordinates must be x.C ({list(C.shape)} integers on {C.device}), got "
                             f"{list(CE.shape) if torch.is_tensor(CE) else type(CE).__name__}")
    else:
        CE = None
    D = Fe.shape[1]
    if differentiable:
        if pool_mode not in ("auto", "ell"):
            raise ValueError(f"{who}: pool_mode={pool_mode!r} with differentiable=True: the matrix-core families keep no fp32 intermediates, "
                             "gradients run on pool_mode='auto' or 'ell'")
        if E.shape[1] not in GRAD_EMBED_WIDTHS:
            raise ValueError(f"{who}: differentiable=True takes embeddings of width {' / '.join(map(str, GRAD_EMBED_WIDTHS))}, got {E.shape[1]}")
    family = pool_family(D, K, num_iters, pool_mode)                  # (an unknown or inadmissible mode raises here)
    perm, rank, nbr = _ordered_knn(who, C, K, same_as=CE)
    if differentiable and torch.is_grad_enabled() and (Fe.requires_grad or E.requires_grad):
        if num_iters == 0:
            return type(x)(features=Fe.to(torch.float32) if Fe.dtype != torch.float32 else Fe.clone(), coordinates=x.C)
        with torch.cuda.device(C.device):
            Y = _PoolGrad.apply(Fe, E, perm.long(), rank.long(), nbr, K, float(sharpen), num_iters, bool(normalize))
        return type(x)(features=Y, coordinates=x.C)
    with torch.cuda.device(C.device), torch.no_grad():
        dev = C.device
        perm64, Dp = perm.long(), (D + 3) // 4 * 4
        # rows into the key order (ops.gather_rows); the feature columns D .. Dp-1 are zero padding for the row loads of the kernels
        X = torch.zeros((n, Dp), dtype=torch.float32, device=dev) if Dp != D else torch.empty((n, D), dtype=torch.float32, device=dev)
        ops.gather_rows(_rows_f32(Fe.detach()), D, perm64, out=X)
        Es = ops.gather_rows(_rows_f32(E.detach()), E.shape[1], perm64)
        if normalize:
            ops.l2norm_rows_(Es)
        w = ops.affinity_softmax(Es, nbr, float(sharpen))
        hp = HotPath(None, (1, 1), K=K, sharpen=float(sharpen), num_iters=num_iters, device=dev, pool_mode=_MODE_OF_FAMILY[family])
        out = hp._pool(X, nbr, w, n, Dp)
        if hp._chain_ops:
            hp.pool_chain_check()                                        # (a chained launch, selected by name: never hand out rows of one that gave up)
        Y = ops.gather_rows(out, D, rank.long())
    return type(x)(features=Y, coordinates=x.C)


def purify(student, x, *, feature_dim=None, differentiable=False, **kw):
    """student(x) in eval mode under no_grad, then affinity_pool on x.F[:, :feature_dim] with the embeddings it gave (the reference pools
    all columns and slices [:, :512] afterwards; a column never influences another, so the geometry columns are left out before).
    The student's training flag is restored afterwards.  kw: affinity_pool's options.  -> type(x)(features=Y, coordinates=x.C).
    differentiable=True: the student is called as the caller left it -- its mode and the grad state untouched -- and its output feeds
    affinity_pool(..., differentiable=True): a loss on Y reaches the student's parameters and x.F."""
    feats = x.F if feature_dim is None else x.F[:, :int(feature_dim)]
    if differentiable:
        return affinity_pool(type(x)(features=feats, coordinates=x.C), student(x), differentiable=True, **kw)
    was = student.training
    student.eval()
    try:
        with torch.no_grad():
            e = student(x)
    finally:
        student.train(was)
    return affinity_pool(type(x)(features=feats, coordinates=x.C), e, **kw)


# ------------------------------------------------------------------------------------------ labels and per-entry IoU counts
FILLS = {"xyz": 7, "yz": 6, None: 0}                        # the axis mask of ops.nn1_batched (0: no fill)
MAX_COUNT_ELEMENTS = 2 ** 27


class Segmentation:
    """pred i64 (per voxel in the input's row order, or per point with an inverse_mapping), zero bool [N] (rows with sum |F| == 0),
    filled_from i64 [N] (the input row whose label a filled row took, -1 elsewhere), counts i64 [B,3,C] = (I, O, T) per batch entry or
    None, unfilled int (zero rows of entries without a non-zero row: they keep their arg-max)."""

    def __init__(self, pred, zero, filled_from, counts, unfilled):
        self.pred, self.zero, self.filled_from, self.counts, self.unfilled = pred, zero, filled_from, counts, unfilled


def _is_int_tensor(t):
    return torch.is_tensor(t) and not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)


def segment(y, text_features, logit_scale=1.0, *, labels=None, num_classes=None, ignore_labels=(255,), fill="xyz", inverse_mapping=None):
    """The per-scene tail of run/validation.py:413-439 over a batched SparseTensor, every batch entry by itself: classify each row
    against the text embeddings (both normalised, arg-max, first maximum on ties), give rows whose feature is all zero the label of the
    nearest non-zero row OF THEIR ENTRY, count intersection / output / target per entry.
    y: an ME-style SparseTensor (.F [N,D] floating, .C integer [N,4] = batch, x, y, z in any row order, unique rows); text_features
    [C,D].  fill: "xyz" -- the nearest in all three coordinates --, "yz" -- the reference's slice quirk (:422-423: columns 1:4 of an
    [N,3] tensor) --, or None; ties by (d^2, input row), as validation.scene_tail and knn.  labels: i64 [N] per voxel, or [P] per point
    when inverse_mapping ([P], a quantiser's point -> voxel map) is given; counts are then over points, each in the entry of its
    voxel, and pred is per point.  counts has B = highest batch index + 1 blocks (absent entries stay zero), C = num_classes (default:
    the text rows) columns; counts.sum(0) is what sharding.summarize takes.  -> Segmentation.  No gradients: inputs are detached.
    Inside: ops.coords_order_batched, ops.classify_argmax_gemm (more than 32 classes at D % 32 == 0) or ops.classify_argmax on the rows
    as they lie, ops.nn1_batched on the zero flags in sorted order, ops.iou_hist_batched.  ValueError from ONE status read-back
    (and a range read-back before it unless the coordinates are int32): see knn; also text_features not [C, D], num_classes outside
    1..4096, more than 4 ignore labels, labels / inverse_mapping of the wrong length or dtype, an inverse_mapping value outside
    0..N-1, an unknown fill, B * 3 * C above 2^27."""
    who = "segment"
    if not (hasattr(y, "F") and hasattr(y, "C")):
        raise ValueError(f"{who}: y must be a SparseTensor (an object with .F and .C), got {type(y).__name__}")
    Fe, C, T = y.F, y.C, text_features
    if fill not in FILLS:
        raise ValueError(f"{who}: fill={fill!r}, expected one of {tuple(FILLS)}")
    _check_coordinates(who, C)
    n = C.shape[0]
    if not torch.is_tensor(Fe) or Fe.dim() != 2 or Fe.shape[0] != n or Fe.shape[1] < 1:
        raise ValueError(f"{who}: features must be [N, D] with N = {n} coordinate rows, got "
                         f"{list(Fe.shape) if torch.is_tensor(Fe) else type(Fe).__name__}")
    D = Fe.shape[1]
    if not torch.is_tensor(T) or T.dim() != 2 or T.shape[0] < 1 or T.shape[1] != D:
        raise ValueError(f"{who}: text_features must be [C, D] with D = {D} feature columns, got "
                         f"{list(T.shape) if torch.is_tensor(T) else type(T).__name__}")
    if not (Fe.dtype.is_floating_point and T.dtype.is_floating_point):
        raise ValueError(f"{who}: features and text_features must be floating point, got {Fe.dtype} / {T.dtype}")
    if not (Fe.is_cuda and T.is_cuda) or Fe.device != C.device or T.device != C.device:
        raise ValueError(f"{who}: features, text_features and coordinates must be CUDA tensors on one device (got {Fe.device} / {T.device} / "
                         f"{C.device}); there is no CPU path")
    nc = T.shape[0] if num_classes is None else num_classes
    if isinstance(nc, bool) or not isinstance(nc, int) or not 1 <= nc <= 4096:
        raise ValueError(f"{who}: num_classes={nc!r} outside 1..4096")
    ignore = [int(v) for v in ignore_labels]
    if len(ignore) > 4:
        raise ValueError(f"{who}: {len(ignore)} ignore labels, at most 4")
    inv = inverse_mapping
    if inv is not None and (not _is_int_tensor(inv) or inv.dim() != 1 or inv.shape[0] < 1 or inv.device != C.device):
        raise ValueError(f"{who}: inverse_mapping must be an integer tensor [P] on {C.device}, got "
                         f"{(list(inv.shape), inv.dtype, str(inv.device)) if torch.is_tensor(inv) else type(inv).__name__}")
    items = n if inv is None else inv.shape[0]
    if labels is not None and (not _is_int_tensor(labels) or labels.dim() != 1 or labels.shape[0] != items or labels.device != C.device):
        raise ValueError(f"{who}: labels must be an integer tensor [{items}] ({'one per point of inverse_mapping' if inv is not None else 'one per voxel'}) "
                         f"on {C.device}, got {(list(labels.shape), labels.dtype, str(labels.device)) if torch.is_tensor(labels) else type(labels).__name__}")
    axes = FILLS[fill]
    dev = C.device
    with torch.cuda.device(dev), torch.no_grad():
        C = C.detach()
        if C.dtype != torch.int32:
            # (range-checked before the cast: an int64 coordinate beyond int32 must not wrap into a valid one)
            lo, hi = ops.readback(torch.stack(torch.aminmax(C)).to(torch.int64))
            if lo < -2 ** 31 or hi >= 2 ** 31:
                raise ValueError(f"{who}: coordinates outside the int32 range ({lo} .. {hi})")
            C = C.to(torch.int32)
        C = C.contiguous()
        perm, rank, keys, order_status = ops.coords_order_batched(C)
        feats = _rows_f32(Fe.detach())
        text_norm = torch.nn.functional.normalize(T.detach().float(), dim=-1).contiguous()
        if text_norm.shape[0] > 32 and D % 32 == 0:                       # validation.scene_tail's choice
            pred, zero = ops.classify_argmax_gemm(feats, text_norm)
        else:
            pred, zero = ops.classify_argmax(feats, text_norm, float(logit_scale))
        if axes:
            zero_sorted = zero.index_select(0, perm.long())
            nn, fill_status = ops.nn1_batched(keys, perm, 1 - zero_sorted, zero_sorted, axes)
        else:
            nn, fill_status = None, torch.zeros(4, dtype=torch.int32, device=dev)
        xyz = C[:, 1:]
        extent = (xyz.amax(0).to(torch.int64) - xyz.amin(0).to(torch.int64) + 1)
        if inv is not None:
            inv = inv.detach().to(torch.int64).contiguous()
            bad_inv = ((inv < 0) | (inv >= n)).sum().reshape(1)
        else:
            bad_inv = torch.zeros(1, dtype=torch.int64, device=dev)
        st = ops.readback(torch.cat([order_status.to(torch.int64), fill_status.to(torch.int64), extent, C[:, 0].amax().to(torch.int64).reshape(1),
                                     bad_inv]))
        dups, bad_batch, bad_axes = st[:3]
        unfilled, axes15 = st[5], st[6]
        extent, top_batch, bad_inv = st[7:10], st[10], st[11]
        # (range first: a row whose batch index is out of range has a meaningless key, which may equal another row's)
        if bad_batch:
            raise ValueError(f"{who}: {bad_batch} rows have a batch index outside 0..65535")
        if bad_axes:
            names = [a for i, a in enumerate("xyz") if bad_axes >> i & 1]
            raise ValueError(f"{who}: coordinate extent of 65536 or more along {', '.join(names)} (16 bits per axis)")
        if dups:
            raise ValueError(f"{who}: {dups} duplicate coordinate rows (MinkowskiEngine would merge them; quantise first)")
        wide = [a for i, a in enumerate("xyz") if extent[i] >= 32768 or axes15 >> i & 1]
        if wide:
            raise ValueError(f"{who}: coordinate extent of 32768 or more along {', '.join(wide)} ({'/'.join(str(e) for e in extent)} voxels; "
                             "squared distances must stay below 2^32)")
        if bad_inv:
            raise ValueError(f"{who}: {bad_inv} inverse_mapping values outside 0..{n - 1}")
        B = top_batch + 1
        if labels is not None and B * 3 * nc > MAX_COUNT_ELEMENTS:
            raise ValueError(f"{who}: counts [{B}, 3, {nc}] would hold more than 2^27 elements (the highest batch index is {top_batch})")
        if nn is not None:
            # sorted rows -> input rows, in the input's row order; a filled row takes the label its source was classified with
            nn_in = nn.index_select(0, rank.long()).long()
            filled_from = torch.where(nn_in >= 0, perm.long()[nn_in.clamp(min=0)], nn_in)
            pred = torch.where(filled_from >= 0, pred[filled_from.clamp(min=0)], pred)
        else:
            filled_from = torch.full((n,), -1, dtype=torch.int64, device=dev)
        counts = None
        if labels is not None:
            counts = torch.zeros((B, 3, nc), dtype=torch.int64, device=dev)
            ops.iou_hist_batched(pred, C, labels.detach().to(torch.int64).contiguous(), B, nc, ignore, counts, index=inv)
        if inv is not None:
            pred = pred.index_select(0, inv)
    return Segmentation(pred, zero.bool(), filled_from, counts, int(unfilled))


# ------------------------------------------------------------------------------------------ cross-entropy against text embeddings
LOSS_REDUCTIONS = ("item", "entry")
_LOSS_OPTIONS = ("ignore_labels", "inverse_mapping", "reduction", "logits_budget_bytes")


def _pad_to(v, m):
    return (v + m - 1) // m * m


class _TextProducts:
    """The operands of the loss's two products on ops.sparse_conv's exact-fp32 matrix-core GEMM (one dense offset): the normalised text
    rows as [Dp, Cp] for Z = s U T^T and as [Cp, Dq] for dU = s G T, zero padded to the kernel's tiles (Dp = D to 32, Cp = C to 128,
    Dq = D to 128), with s as the epilogue's per-column scale."""

    def __init__(self, text_features, scale, D):
        T = torch.nn.functional.normalize(text_features.detach().float(), dim=-1)
        C, dev = T.shape[0], T.device
        self.C, self.D = C, D
        _, cp, kp = ops.sparse_conv_tiles()
        self.Dp, self.Cp, self.Dq = _pad_to(D, kp), _pad_to(C, cp), _pad_to(D, cp)
        self.to_logits = torch.zeros((self.Dp, self.Cp), dtype=torch.float32, device=dev)
        self.to_logits[:D, :C] = T.t()
        self.to_rows = torch.zeros((self.Cp, self.Dq), dtype=torch.float32, device=dev)
        self.to_rows[:C, :D] = T
        self.scale = scale.to(torch.float32).reshape(1).expand(max(self.Cp, self.Dq)).contiguous()

    def logits(self, u_rows, out):
        """out[r, Cp] = s * u_rows @ T^T (columns C .. Cp-1 are zeros)"""
        return ops.sparse_conv(u_rows, None, self.to_logits, scale=self.scale, out=out)

    def rows(self, g, out):
        """out[r, Dq] = s * g @ T"""
        return ops.sparse_conv(g, None, self.to_rows, scale=self.scale, out=out)


class _SegmentLoss(torch.autograd.Function):
    """The loss and dY are both made by segment_loss's forward kernels; backward hands g * dY to y.F"""

    @staticmethod
    def forward(ctx, feats, loss, d_feats):
        ctx.save_for_backward(d_feats)
        ctx.dtype = feats.dtype
        return loss.clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (d_feats,) = ctx.saved_tensors
        return (g * d_feats).to(ctx.dtype), None, None


def segment_loss(y, text_features, logit_scale=1.0, *, labels, ignore_labels=(255,), inverse_mapping=None, reduction="item",
                 logits_budget_bytes=2 ** 30):
    """The differentiable twin of segment: the classification cross-entropy of y.F against the text embeddings, forward and gradient on
    HIP kernels, deterministic.  y: an ME-style SparseTensor (.F [N,D] floating of any dtype and row stride, .C integer [N,4]; only the
    batch column is used, the rows are taken as they lie); text_features [C,D], 1 <= C <= 4096; labels: integer [N] per voxel, or [P]
    per point when inverse_mapping ([P], a quantiser's point -> voxel map) is given, exactly as segment takes them -- ground truth, or
    segment(x_unpurified, ...).pred for the label-free objective.  With u_i = y_i / max(|y_i|, 1e-12), t_c = normalize(text_c) and
    s = logit_scale: z_ic = s <u_i, t_c> (its arg-max is segment's pred on non-zero rows), lse_i = log sum_c exp(z_ic), and
        loss = sum over the valid items p of w_b(p) (lse_i(p) - z_i(p),l_p).
    An item (a voxel, or a point with row i(p) = inverse_mapping[p]) is valid when 0 <= l_p < C, l_p is none of ignore_labels (at most
    4) and row i(p) is not a zero row (sum |y_i| == 0: segment's zero flag).  reduction "item": w = 1 / V over all V valid items
    (F.cross_entropy's mean); "entry": w_b = 1 / (E V_b), the mean over the E entries that hold valid items of each entry's mean
    (info_nce's "entry").  No valid item: the loss is 0.0 and every gradient exactly zero.
    -> 0-d fp32 loss under autograd with respect to y.F only (the gradient in y.F's dtype, rows without valid items exactly +0.0; no
    double backward); loss.per_entry fp32 [B], every entry's mean, detached, NaN for an entry without valid items, B = the highest
    batch index + 1; loss.valid i64 [B].  The text embeddings and logit_scale are the frozen VLM's: one that requires grad while grad
    mode is on is a ValueError.
    Inside: ops.segment_loss_unit_rows, ops.segment_loss_items (per point: a CSR of the valid items by row), then per chunk of rows
    Z = s U T^T on ops.sparse_conv's exact-fp32 matrix-core GEMM, ops.segment_loss_rows (stable softmax, G = w (m softmax - cnt), lse,
    the row's term) and dU = s G T on the same GEMM, ops.segment_loss_reduce (fixed-order fp64) and ops.l2norm_rows_backward.  The
    logits and G exist for one chunk at a time, at most logits_budget_bytes for the two (G only when a gradient is wanted: a call
    under no_grad, or on features that do not require grad, stores none); the result does not depend on the chunking.
    ValueError before any kernel or from the ONE status read-back (which also carries the highest batch index and V): shape / dtype /
    device mismatches, CPU tensors, an unknown reduction, more than 4 ignore labels, C outside 1..4096, a logit_scale that is not
    finite and positive, a batch index outside 0..65535, an inverse_mapping value outside 0..N-1."""
    who = "segment_loss"
    if not (hasattr(y, "F") and hasattr(y, "C")):
        raise ValueError(f"{who}: y must be a SparseTensor (an object with .F and .C), got {type(y).__name__}")
    Fe, C, T = y.F, y.C, text_features
    if reduction not in LOSS_REDUCTIONS:
        raise ValueError(f"{who}: reduction={reduction!r}, expected one of {LOSS_REDUCTIONS}")
    _check_coordinates(who, C)
    n = C.shape[0]
    if not torch.is_tensor(Fe) or Fe.dim() != 2 or Fe.shape[0] != n or Fe.shape[1] < 1:
        raise ValueError(f"{who}: features must be [N, D] with N = {n} coordinate rows, got "
                         f"{list(Fe.shape) if torch.is_tensor(Fe) else type(Fe).__name__}")
    D = Fe.shape[1]
    if not torch.is_tensor(T) or T.dim() != 2 or T.shape[0] < 1 or T.shape[1] != D:
        raise ValueError(f"{who}: text_features must be [C, D] with D = {D} feature columns, got "
                         f"{list(T.shape) if torch.is_tensor(T) else type(T).__name__}")
    if not (Fe.dtype.is_floating_point and T.dtype.is_floating_point):
        raise ValueError(f"{who}: features and text_features must be floating point, got {Fe.dtype} / {T.dtype}")
    if not (Fe.is_cuda and T.is_cuda) or Fe.device != C.device or T.device != C.device:
        raise ValueError(f"{who}: features, text_features and coordinates must be CUDA tensors on one device (got {Fe.device} / {T.device} / "
                         f"{C.device}); there is no CPU path")
    nc = T.shape[0]
    if not 1 <= nc <= 4096:
        raise ValueError(f"{who}: {nc} text rows (classes) outside 1..4096")
    ignore = [int(v) for v in ignore_labels]
    if len(ignore) > 4:
        raise ValueError(f"{who}: {len(ignore)} ignore labels, at most 4")
    S = logit_scale
    if torch.is_tensor(S):
        if S.numel() != 1 or not S.dtype.is_floating_point or S.device != C.device:
            raise ValueError(f"{who}: a tensor logit_scale must be one floating point value on {C.device}, got {list(S.shape)} {S.dtype} on {S.device}")
    elif isinstance(S, bool) or not isinstance(S, (int, float)) or not (S > 0 and S < float("inf")):
        raise ValueError(f"{who}: logit_scale={S!r} must be finite and positive")
    if torch.is_grad_enabled() and (T.requires_grad or (torch.is_tensor(S) and S.requires_grad)):
        raise ValueError(f"{who}: text_features and logit_scale are not differentiated (the frozen VLM's); detach them, or the gradient "
                         "would be dropped silently")
    inv = inverse_mapping
    if inv is not None and (not _is_int_tensor(inv) or inv.dim() != 1 or inv.shape[0] < 1 or inv.device != C.device):
        raise ValueError(f"{who}: inverse_mapping must be an integer tensor [P] on {C.device}, got "
                         f"{(list(inv.shape), inv.dtype, str(inv.device)) if torch.is_tensor(inv) else type(inv).__name__}")
    items = n if inv is None else inv.shape[0]
    if not _is_int_tensor(labels) or labels.dim() != 1 or labels.shape[0] != items or labels.device != C.device:
        raise ValueError(f"{who}: labels must be an integer tensor [{items}] ({'one per point of inverse_mapping' if inv is not None else 'one per voxel'}) "
                         f"on {C.device}, got {(list(labels.shape), labels.dtype, str(labels.device)) if torch.is_tensor(labels) else type(labels).__name__}")
    if not _is_count(logits_budget_bytes, 1):
        raise ValueError(f"{who}: logits_budget_bytes={logits_budget_bytes!r} must be an integer >= 1")
    dev = C.device
    need_grad = torch.is_grad_enabled() and Fe.requires_grad
    with torch.cuda.device(dev), torch.no_grad():
        C = C.detach()
        bad_range = torch.zeros(1, dtype=torch.int64, device=dev)
        if C.dtype != torch.int32:
            # (only the batch column is read: one outside int32 is outside 0..65535 too and must not wrap into it)
            batch = C[:, 0]
            bad_range = ((batch < 0) | (batch > 65535)).sum().reshape(1)
            C = torch.cat([batch.clamp(-1, 65536).reshape(-1, 1), torch.zeros_like(C[:, 1:])], 1).to(torch.int32)
        C = C.contiguous()
        s_dev = S.detach().to(torch.float32).reshape(1) if torch.is_tensor(S) else torch.full((1,), float(S), dtype=torch.float32, device=dev)
        bad_scale = (~(torch.isfinite(s_dev) & (s_dev > 0))).to(torch.int64)
        tp = _TextProducts(T, s_dev, D)
        feats = _rows_f32(Fe.detach())
        U, zero = ops.segment_loss_unit_rows(feats, D)
        lab = labels.detach().to(torch.int64).contiguous()
        if inv is not None:
            inv = inv.detach().to(torch.int64).contiguous()
        it = ops.segment_loss_items(C, zero, lab, nc, ignore, reduction, index=inv)
        bad_batch, bad_inv, top_batch, V, bad_range, bad_scale = ops.readback(torch.cat([it.status, bad_range, bad_scale]))
        if bad_batch or bad_range:
            raise ValueError(f"{who}: {max(bad_batch, bad_range)} rows have a batch index outside 0..65535")
        if bad_inv:
            raise ValueError(f"{who}: {bad_inv} inverse_mapping values outside 0..{n - 1}")
        if bad_scale:
            raise ValueError(f"{who}: logit_scale must be finite and positive")
        B = top_batch + 1
        valid = it.entry_cnt[:B].clone()
        if V == 0:
            loss = torch.zeros((), dtype=torch.float32, device=dev)
            per_entry = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
            d_feats = torch.zeros((n, D), dtype=torch.float32, device=dev) if need_grad else None
        else:
            chunk = max(1, min(n, logits_budget_bytes // ((8 if need_grad else 4) * tp.Cp), (2 ** 31 - 1) // tp.Cp))
            Z = torch.empty((chunk, tp.Cp), dtype=torch.float32, device=dev)
            G = torch.empty((chunk, tp.Cp), dtype=torch.float32, device=dev) if need_grad else None   # (forward only: no G is stored)
            lse = torch.empty(n, dtype=torch.float32, device=dev)
            term = torch.empty(n, dtype=torch.float64, device=dev)
            dU = torch.empty((n, tp.Dq), dtype=torch.float32, device=dev) if need_grad else None
            for r0 in range(0, n, chunk):
                r = min(chunk, n - r0)
                tp.logits(U[r0:r0 + r], Z[:r])
                ops.segment_loss_rows(Z[:r], nc, C, it, lab, r0, G[:r] if need_grad else None, lse, term)
                if need_grad:
                    tp.rows(G[:r], dU[r0:r0 + r])
            loss, per_entry = ops.segment_loss_reduce(term, C, it.entry_cnt, B, reduction)
            d_feats = None
            if need_grad:
                # the backward of the row normalisation on the padded rows (zero columns change neither the norm nor the products)
                raw = feats
                if tp.Dp != D:
                    raw = torch.zeros((n, tp.Dp), dtype=torch.float32, device=dev)
                    raw[:, :D] = feats
                d_feats = ops.l2norm_rows_backward(raw, dU[:, :tp.Dp])[:, :D]
    if need_grad:
        with torch.cuda.device(dev):
            loss = _SegmentLoss.apply(Fe, loss, d_feats)
    loss.per_entry, loss.valid = per_entry, valid
    return loss


def purified_loss(student, x, text_features, logit_scale=1.0, *, labels, feature_dim=None, **kw):
    """purify(student, x, feature_dim=feature_dim, differentiable=True) followed by segment_loss on what it returns: the objective
    DESIGN.md 5.7 built the differentiable pooling for.  kw is split by name: ignore_labels, inverse_mapping, reduction and
    logits_budget_bytes are segment_loss's, everything else affinity_pool's.  -> the loss of segment_loss, with loss.purified."""
    loss_kw = {k: kw.pop(k) for k in _LOSS_OPTIONS if k in kw}
    purified = purify(student, x, feature_dim=feature_dim, differentiable=True, **kw)
    loss = segment_loss(purified, text_features, logit_scale, labels=labels, **loss_kw)
    loss.purified = purified
    return loss


# ------------------------------------------------------------------------------------------ contrastive pairs and InfoNCE
SIM_ROW_PAD = 4                                             # floats: the ragged rows start 16-byte aligned
MAX_ENTRY_ROWS = 12288 * 256                                # gp_sampler_select_segments: the longest row its groups hold
MAX_CHUNK_ANCHORS = 65535 * 64                              # gp_sim_segments_f16x3: anchor tiles per launch
REDUCTIONS = ("anchor", "entry")


class ContrastivePairs:
    """The sampler's result, everything as INPUT row numbers: anchor i64 [A], positive i64 [A], negative i64 [A, Nn] (the macro
    negatives ascending by (similarity, key row), then the micro ones ascending by (similarity, slot in the neighbour list)), entry
    i64 [A] (the batch index of each anchor), num_rows = N and num_entries = the highest batch index + 1.
    rows i64 [S] (the sorted unique sampled rows) and index i64 [A * (2 + Nn)] (positions in rows of cat(anchor, positive,
    negative.flatten()): the reference's all_sampled_indices and point_to_batch_map, :1196) are made on first use by one torch.unique
    -- which reads S back, as the reference's does."""

    def __init__(self, anchor, positive, negative, entry, num_rows, num_entries):
        self.anchor, self.positive, self.negative, self.entry = anchor, positive, negative, entry
        self.num_rows, self.num_entries = int(num_rows), int(num_entries)
        self._rows = self._index = None

    def _unique(self):
        if self._rows is None:
            self._rows, self._index = torch.unique(torch.cat([self.anchor, self.positive, self.negative.flatten()]), return_inverse=True)
        return self._rows, self._index

    @property
    def rows(self):
        return self._unique()[0]

    @property
    def index(self):
        return self._unique()[1]

    def subset(self, x):
        """the sampled rows of x as a SparseTensor (the reference's :1192-1212 for voxels that are their own samples): row s of it is
        row rows[s] of x; gradients of its features reach x.F"""
        if not (hasattr(x, "F") and hasattr(x, "C")) or x.C.shape[0] != self.num_rows or x.F.shape[0] != self.num_rows:
            raise ValueError(f"ContrastivePairs.subset: x must be the SparseTensor of {self.num_rows} rows the pairs were sampled on")
        rows = self.rows
        return type(x)(features=x.F.index_select(0, rows), coordinates=x.C.index_select(0, rows))


def _is_count(v, lo):
    return not isinstance(v, bool) and isinstance(v, int) and v >= lo


def sample_pairs(coordinates, teacher, *, K=96, num_anchors=4096, num_negatives=63, num_macro=48, anchor_indices=None, neighbors=None,
                 generator=None, sim_budget_bytes=2 ** 33):
    """sample_contrastive_pairs_hybrid (models/affinity_module.py:1099-1136) for every batch entry of a SparseTensor's coordinates at
    once, entries never mixing.  coordinates: integer [N,4] = batch, x, y, z on the GPU, any row order, unique rows; teacher: floating
    [N,Dt], one row per coordinate row.  For an anchor a of entry b, with s_j = <Fn_a, Fn_j>, Fn = F.normalize(teacher, dim=1), over the
    rows j of entry b only:
      positive[a] = arg-max of s_j over j != a;
      negative[a] = the num_macro rows of lowest s_j other than a and positive[a], ascending, then the num_negatives - num_macro lowest
                    of the anchor's K nearest voxels (row a of knn(coordinates, K), a neighbour equal to positive[a] counting as +inf --
                    the reference's in-place mark, :1125-1133), ascending by (value, slot in the list).
    Ties go to the lowest KEY row (the order of ops.coords_order_batched: batch, then Morton code), not to the lowest input row: the
    result then depends on the voxels alone, so permuting the input rows permutes the result and nothing else.  -0 counts as +0, NaN
    orders above +inf (gp_sampler_select).
    anchor_indices: i64 [A] input rows, any count, order and entry; without it min(num_anchors, N_b // 3) rows of every entry are drawn
    without replacement (:1108-1112) on the device -- one torch.rand(N, generator=generator) sorted inside the entries, no loop over
    entries -- and come grouped by entry.  neighbors: i64 [A,K] input rows given together with anchor_indices, used instead of the kNN
    (K is then its width).
    The similarities live in a ragged fp32 buffer (one row of N_b floats per anchor, ops.sim_segments) of at most sim_budget_bytes:
    anchors are processed in chunks that fit; the result does not depend on the chunking.  -> ContrastivePairs.
    Host syncs: ONE status read-back, which also carries the anchor and row counts that size the buffer (and a range read-back before
    it unless the coordinates are int32).  ValueError, all before any kernel of the sampler: what knn refuses; not 1 <= num_macro <=
    num_negatives <= 63 or num_negatives - num_macro > K - 1; an entry that holds an anchor with fewer than num_macro + 2 rows;
    anchors or neighbours outside 0..N-1; a neighbour in another entry than its anchor; a teacher of the wrong shape, dtype or device;
    a budget too small for one anchor row."""
    who = "sample_pairs"
    C, T, AI, NB = coordinates, teacher, anchor_indices, neighbors
    if NB is not None:
        if AI is None:
            raise ValueError(f"{who}: neighbors are given per anchor, together with anchor_indices")
        if not _is_int_tensor(NB) or NB.dim() != 2 or NB.shape[1] < 1:
            raise ValueError(f"{who}: neighbors must be an integer tensor [A, K], got "
                             f"{(list(NB.shape), NB.dtype) if torch.is_tensor(NB) else type(NB).__name__}")
        K = NB.shape[1]
    _check_k(who, K)
    if not (_is_count(num_macro, 1) and _is_count(num_negatives, 1) and num_macro <= num_negatives <= 63):
        raise ValueError(f"{who}: num_macro={num_macro!r}, num_negatives={num_negatives!r}: expected 1 <= num_macro <= num_negatives <= 63")
    num_micro = num_negatives - num_macro
    if num_micro > K - 1:
        raise ValueError(f"{who}: {num_micro} local negatives (num_negatives - num_macro) need K - 1 >= {num_micro} neighbours, K={K}")
    if not _is_count(num_anchors, 1):
        raise ValueError(f"{who}: num_anchors={num_anchors!r} must be an integer >= 1")
    if not _is_count(sim_budget_bytes, 1):
        raise ValueError(f"{who}: sim_budget_bytes={sim_budget_bytes!r} must be an integer >= 1")
    _check_coordinates(who, C)
    n = C.shape[0]
    dev = C.device
    if not torch.is_tensor(T) or T.dim() != 2 or T.shape[0] != n or T.shape[1] < 1:
        raise ValueError(f"{who}: teacher must be [N, Dt] with N = {n} coordinate rows, got "
                         f"{list(T.shape) if torch.is_tensor(T) else type(T).__name__}")
    if not T.dtype.is_floating_point:
        raise ValueError(f"{who}: teacher must be floating point, got {T.dtype}")
    if T.device != dev:
        raise ValueError(f"{who}: teacher and coordinates must be CUDA tensors on one device (got {T.device} / {dev}); there is no CPU path")
    if AI is not None:
        if not _is_int_tensor(AI) or AI.dim() != 1 or AI.shape[0] < 1 or AI.device != dev:
            raise ValueError(f"{who}: anchor_indices must be an integer tensor [A] on {dev}, got "
                             f"{(list(AI.shape), AI.dtype, str(AI.device)) if torch.is_tensor(AI) else type(AI).__name__}")
        if NB is not None and (NB.shape[0] != AI.shape[0] or NB.device != dev):
            raise ValueError(f"{who}: neighbors must be [{AI.shape[0]}, K] (one list per anchor) on {dev}, got {list(NB.shape)} on {NB.device}")
    pad = lambda v: (v + (SIM_ROW_PAD - 1)) // SIM_ROW_PAD * SIM_ROW_PAD

    def extra(perm, rank, keys):
        """entry bounds of every key row, the anchors' descriptors when they are given, and the status words"""
        eb = (keys >> 48) & 0xFFFF                                        # the batch index of every key row, ascending
        first = torch.searchsorted(eb, eb)
        size = torch.searchsorted(eb, eb, right=True) - first
        zero = torch.zeros((), dtype=torch.int64, device=dev)
        bad_a = bad_n = other = zero
        if AI is not None:
            a_in = AI.detach().to(torch.int64)
            bad_a = ((a_in < 0) | (a_in >= n)).sum()
            a_key = rank.long()[a_in.clamp(0, n - 1)]
            a_first, a_len = first[a_key], size[a_key]
            count, floats, longest, shortest = zero + a_in.shape[0], pad(a_len).sum(), a_len.max(), a_len.min()
            nb_key = None
            if NB is not None:
                nb_in = NB.detach().to(torch.int64)
                bad_n = ((nb_in < 0) | (nb_in >= n)).sum()
                nb_key = rank.long()[nb_in.clamp(0, n - 1)]
                other = (first[nb_key] != a_first.unsqueeze(1)).sum()
        else:
            a_key = nb_key = None
            head = first == torch.arange(n, device=dev)                   # one row per entry
            take = torch.clamp(size // 3, max=num_anchors) * head          # :1108: min(num_anchors, N_b // 3) anchors of the entry
            on = take > 0
            count, floats = take.sum(), (take * pad(size)).sum()
            longest = torch.where(on, size, zero).max()
            shortest = torch.where(on, size, zero + n).min()
        words = torch.stack([bad_a, bad_n, other, count, floats, longest, shortest, eb[-1], size.min()])
        return words, (eb, first, size, a_key, nb_key)

    perm, rank, nbr, keys, words, (eb, first, size, a_key, nb_key) = _ordered_knn(who, C, K, extra=extra, lists=NB is None)
    bad_a, bad_n, other, A, floats, longest, shortest, top_batch, smallest = words
    if NB is not None and smallest <= K:                                  # (what the kNN refuses when the lists are its own)
        raise ValueError(f"{who}: a batch entry holds {smallest} voxels, K={K} neighbours need more than K")
    if bad_a:
        raise ValueError(f"{who}: {bad_a} anchor_indices outside 0..{n - 1}")
    if bad_n:
        raise ValueError(f"{who}: {bad_n} neighbors outside 0..{n - 1}")
    if other:
        raise ValueError(f"{who}: {other} neighbors lie in another batch entry than their anchor")
    if A == 0:
        raise ValueError(f"{who}: no entry holds 3 voxels or more: nothing to draw anchors from")
    if shortest < num_macro + 2:
        raise ValueError(f"{who}: a batch entry that holds an anchor has {shortest} voxels, num_macro={num_macro} negatives beside the anchor "
                         f"and its positive need at least {num_macro + 2}")
    if longest > MAX_ENTRY_ROWS:
        raise ValueError(f"{who}: a batch entry that holds an anchor has {longest} voxels, more than the {MAX_ENTRY_ROWS} a row of the selection takes")
    chunk = min(sim_budget_bytes // 4 // pad(longest), MAX_CHUNK_ANCHORS)
    if chunk < 1:
        raise ValueError(f"{who}: sim_budget_bytes={sim_budget_bytes} is less than one anchor's row of {longest} similarities "
                         f"({4 * pad(longest)} bytes)")
    with torch.cuda.device(dev), torch.no_grad():
        perm64 = perm.long()
        if a_key is None:
            # the draw: rows by (entry, a uniform number); the first min(num_anchors, N_b // 3) of every entry are its anchors
            u = torch.rand(n, device=dev, generator=generator)
            by_u = torch.argsort(u)
            order = by_u[torch.argsort(eb[by_u], stable=True)]
            place = torch.arange(n, device=dev) - first[order]
            chosen = place < torch.clamp(size[order] // 3, max=num_anchors)
            a_sorted = order[torch.argsort(~chosen, stable=True)[:A]]     # (A is known from the read-back: no second sync)
            back = None
        else:
            by_key = torch.argsort(a_key)                                 # anchors grouped by entry, as the similarity kernel takes them
            a_sorted = a_key[by_key]
            back = torch.empty_like(by_key)
            back[by_key] = torch.arange(A, device=dev)
        a_first, a_len = first[a_sorted].to(torch.int32), size[a_sorted].to(torch.int32)
        a_row = a_sorted.to(torch.int32)
        offs = torch.cumsum(pad(size[a_sorted]), 0)
        offs = torch.cat([offs.new_zeros(1), offs])                       # [A + 1]: the rows' starts as if all were in one buffer
        if num_micro:
            lists = nbr.index_select(0, a_sorted) if nb_key is None else nb_key.index_select(0, by_key).to(torch.int32)
            lists = lists.contiguous()
        Dt = T.shape[1]
        Dp = (Dt + 31) // 32 * 32
        Tk = torch.zeros((n, Dp), dtype=torch.float32, device=dev) if Dp != Dt else torch.empty((n, Dt), dtype=torch.float32, device=dev)
        ops.gather_rows(_rows_f32(T.detach()), Dt, perm64, out=Tk)         # the teacher rows in the key order, zero columns up to Dp
        hi, lo = ops.normalize_split_f16(Tk)
        del Tk
        buf = torch.empty(min(floats, chunk * pad(longest)), dtype=torch.float32, device=dev)
        positive = torch.empty(A, dtype=torch.int64, device=dev)
        negative = torch.empty((A, num_negatives), dtype=torch.int64, device=dev)
        for a0 in range(0, A, chunk):
            a1 = min(a0 + chunk, A)
            off = (offs[a0:a1] - offs[a0]).contiguous()
            sl = slice(a0, a1)
            ops.sim_segments(hi, lo, a_row[sl], a_first[sl], a_len[sl], off, longest, buf)
            pos, macro = ops.sampler_select_segments(buf, off, a_len[sl], a_first[sl], a_sorted[sl], num_macro, longest)
            positive[sl] = pos
            negative[sl, :num_macro] = macro
            if num_micro:
                negative[sl, num_macro:] = ops.sampler_micro_segments(buf, off, a_first[sl], a_len[sl], lists[sl], pos, num_micro)
        # key rows -> input rows, and the anchors back into the caller's order
        anchor, entry = perm64[a_sorted], eb[a_sorted]
        positive, negative = perm64[positive], perm64[negative]
        if back is not None:
            anchor, entry, positive, negative = anchor[back], entry[back], positive[back], negative[back]
    return ContrastivePairs(anchor, positive, negative, entry, n, top_batch + 1)


class _InfoNCE(torch.autograd.Function):
    """loss = sum_a w_a l_a and dE by ops.infonce_weighted_fwd_bwd in the forward pass; backward hands g * dE to the embeddings"""

    @staticmethod
    def forward(ctx, E, s2v, index, A, Nn, temperature, w):
        loss, per_anchor, dE = ops.infonce_weighted_fwd_bwd(_rows_f32(E.detach()), s2v, index, A, Nn, temperature, w)
        ctx.save_for_backward(dE)
        ctx.dtype = E.dtype
        ctx.mark_non_differentiable(per_anchor)
        return loss, per_anchor

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _):
        (dE,) = ctx.saved_tensors
        return (g * dE).to(ctx.dtype), None, None, None, None, None, None


def info_nce(embeddings, pairs, *, temperature=0.07, reduction="anchor"):
    """The InfoNCE of SonataXAffinityTrainer.forward (models/affinity_module.py:1219-1233) over the pairs of sample_pairs: per anchor
    the cross entropy of (<a, p>, <a, n_1>, ...) / temperature on the normalised embeddings, target 0.  embeddings: a SparseTensor or
    a floating tensor of width <= 256 with S = len(pairs.rows) rows (the student's output on pairs.subset(x)) or N rows (on all of x).
    reduction "anchor": the mean over all anchors -- with one entry the reference's loss; "entry": the mean, over the entries that have
    anchors, of each entry's mean -- what one scene per rank under DDP averages to.  -> 0-d fp32 loss under autograd (backward hands
    g * dE to the embeddings; no double backward); loss.per_entry: fp32 [num_entries], every entry's mean, detached, NaN for an entry
    without anchors.  ValueError before any kernel: a row count that is neither S nor N, a width above 256, an unknown reduction, a
    temperature that is not positive."""
    who = "info_nce"
    if not isinstance(pairs, ContrastivePairs):
        raise ValueError(f"{who}: pairs must be the ContrastivePairs of sample_pairs, got {type(pairs).__name__}")
    if reduction not in REDUCTIONS:
        raise ValueError(f"{who}: reduction={reduction!r}, expected one of {REDUCTIONS}")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not temperature > 0:
        raise ValueError(f"{who}: temperature={temperature!r} must be positive")
    E = embeddings.F if hasattr(embeddings, "F") and hasattr(embeddings, "C") else embeddings
    if not torch.is_tensor(E) or E.dim() != 2 or not E.dtype.is_floating_point:
        raise ValueError(f"{who}: embeddings must be a SparseTensor or a floating tensor [rows, d], got "
                         f"{(list(E.shape), E.dtype) if torch.is_tensor(E) else type(E).__name__}")
    dev = pairs.anchor.device
    if E.device != dev:
        raise ValueError(f"{who}: embeddings and pairs must be on one device (got {E.device} / {dev}); there is no CPU path")
    if not 1 <= E.shape[1] <= 256:
        raise ValueError(f"{who}: embedding width {E.shape[1]} outside 1..256")
    S, N = pairs.rows.shape[0], pairs.num_rows
    if E.shape[0] not in (S, N):
        raise ValueError(f"{who}: embeddings have {E.shape[0]} rows, expected S = {S} (the rows of pairs.subset) or N = {N} (all rows)")
    A, Nn = pairs.negative.shape
    with torch.cuda.device(dev):
        # (S == N: every row was sampled, rows is 0..N-1 and both readings are the same)
        s2v = pairs.rows if E.shape[0] == N else torch.arange(S, device=dev)
        counts = torch.zeros(pairs.num_entries, dtype=torch.float32, device=dev).index_add_(
            0, pairs.entry, torch.ones(A, dtype=torch.float32, device=dev))
        if reduction == "anchor":
            w = torch.full((A,), 1.0 / A, dtype=torch.float32, device=dev)
        else:
            w = 1.0 / ((counts > 0).sum() * counts[pairs.entry])
        loss, per_anchor = _InfoNCE.apply(E, s2v.contiguous(), pairs.index.contiguous(), A, Nn, float(temperature), w.contiguous())
        loss.per_entry = torch.zeros_like(counts).index_add_(0, pairs.entry, per_anchor.detach()) / counts
    return loss


def contrastive_loss(student, x, teacher, *, subset=True, temperature=0.07, reduction="anchor", **kw):
    """sample_pairs on x.C and the teacher rows, the student on the sampled rows (subset=True: pairs.subset(x), as the reference's
    forward runs it on the sampled voxels only, :1192-1212) or on all of x, info_nce on what it returns.  The student is called as the
    caller left it: its mode and the grad state untouched.  kw: sample_pairs's options.  -> the loss of info_nce, with loss.pairs."""
    if not (hasattr(x, "F") and hasattr(x, "C")):
        raise ValueError(f"contrastive_loss: x must be a SparseTensor (an object with .F and .C), got {type(x).__name__}")
    pairs = sample_pairs(x.C, teacher, **kw)
    loss = info_nce(student(pairs.subset(x) if subset else x), pairs, temperature=temperature, reduction=reduction)
    loss.pairs = pairs
    return loss
