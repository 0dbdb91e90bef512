/*
 * geopurify_hip.h -- C ABI of libgeopurify_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for GeoPurify's per-scene hot path.  The reference has no
 * FFI of its own: its hot path calls third-party engines from Python.  Each entry point below
 * replaces one of those call sites (cited as file:line relative to the reference tree); the Python
 * host layer (geopurify_amd/_lib.py) binds them with ctypes, see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - all buffers (outputs and workspaces) are caller-allocated; *_workspace_bytes() gives sizes;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on that stream unless
 *     it documents a synchronisation;
 *   - return value: 0 = ok, negative = error (GP_E*), gp_last_error() gives a message;
 *   - no exceptions, no hidden allocation on the launch path, no torch types.
 *   - rows are fp32 row-major with an explicit leading dimension (in elements) where noted.
 */
#ifndef GEOPURIFY_HIP_H
#define GEOPURIFY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GP_OK 0
#define GP_EINVAL (-22)   /* bad argument / shape */
#define GP_ENOMEM (-12)   /* workspace too small */
#define GP_EHIP (-5)      /* HIP runtime error */
#define GP_ERANGE (-34)   /* coordinate extent not representable */

#define GP_KNN_MAX_K 127  /* K+1 <= 128 */

/* element-type tags of the batched lifts' *_t entry points (feature maps, mask logits) */
#define GP_ELEM_F32 0
#define GP_ELEM_F16 1     /* IEEE binary16 */
#define GP_ELEM_BF16 2    /* bfloat16 */

int gp_version(void);
/* Tuning knobs for experiments (table in csrc/error.hip).  No knob reaches a PRODUCT kernel: the pooling / convolution  */
/* tuning bits (knobs 4 / 3) are honoured only by the *_tuning_kernel twins, the others select a launch shape or a slower, */
/* equally tested kernel.  Unknown keys and undefined values are GP_EINVAL.                                                */
int gp_debug_set(int32_t key, int32_t value);
/* Device buffers for experiments (0: pooling time stamps, 10 x uint64 per wave; NULL, 0 = off).  `bytes` is checked by    */
/* every launch that writes into the buffer.                                                                               */
int gp_debug_ptr(int32_t key, void *device_buffer, size_t bytes);
const char *gp_last_error(void);

/* ------------------------------------------------------------------------------------------ */
/* Rows 1-2: Voxelizer.voxelize + FNV-1 dedupe (dataset/voxelizer.py:103-121,                  */
/*           dataset/voxelization_utils.py:6-18,95-97: np.unique(return_index, return_inverse)) */
/* c = floor([x 1] @ rigid^T[:, :3]); c -= min(c); key = FNV-1(c) ; voxels in ascending key      */
/* order.  rigid_host: 16 doubles row-major (M_r @ M_v).  Outputs: coords_aug f64 [N,3] and inds */
/* i64 [N] hold nv valid rows; inds_reconstruct i64 [N]; *nv_dev receives the voxel count;       */
/* order i64 [N] (optional, may be NULL): point ids sorted by (key, id); seg_start i64 [N+1]     */
/* (optional): CSR offsets of each voxel's points in `order`.                                    */
size_t gp_voxelize_workspace_bytes(int64_t n);
int gp_voxelize_f64(const double *coords, int64_t n, const double *rigid_host,
                    double *coords_aug, int64_t *inds, int64_t *inds_reconstruct, int64_t *nv_dev,
                    int64_t *order, int64_t *seg_start,
                    void *workspace, size_t workspace_bytes, void *stream);
/* FNV-1 hash of integer-valued fp64 coordinates [n,3] -> uint64 [n] (voxelization_utils.py:6-18) */
int gp_fnv_hash_f64(const double *coords, int64_t n, uint64_t *hash, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Row 3: point -> pixel mapping with depth-consistency test                                    */
/* (models/utils/fusion_util.py:99-147 ScanNet, :45-82 Matterport).                              */
/* w2c_host: 16 doubles row-major world->camera (the host passes world_view_transform^T, or     */
/* inv(camera_to_world)); fx,fy,cx,cy: intrinsics at image_dim.  depth f64 [H,W] or NULL.        */
/* mapping i64 [N,3] rows (v,u,1) or (0,0,0).  weight f64 [N] optional (ScanNet variant).         */
int gp_project_points_f64(const double *coords, int64_t n, const double *w2c_host,
                          double fx, double fy, double cx, double cy,
                          const double *depth, int32_t width, int32_t height,
                          int32_t cut_bound, double vis_thres,
                          int64_t *mapping, double *weight, void *stream);
/* Depth "render" mode of the ScanNet mapper (fusion_util.py:126-130, compute_mapping(depth=<str>)):  */
/* depth f64 [H,W] = 999999 everywhere, then the minimum camera-space z over the points with z > 0.2   */
/* that project inside the cut bound; feed it to gp_project_points_f64 for the occlusion test.        */
int gp_render_depth_f64(const double *coords, int64_t n, const double *w2c_host,
                        double fx, double fy, double cx, double cy, int32_t width, int32_t height,
                        int32_t cut_bound, double *depth, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Internal voxel order + lattice grid (shared by kernel-map build and kNN).                     */
/* gp_morton_order: perm i32 [nv] = voxel rows sorted by the Morton code of (coords - min);      */
/* rank i32 [nv] = inverse permutation.  coords i32 [nv,3].                                      */
/* per-axis minimum / maximum of integer coordinates [nv,3] -> mm i32 [6] = (min x,y,z, max x,y,z); no host sync      */
int gp_minmax_i32(const int32_t *coords, int64_t nv, int32_t *mm, void *stream);
size_t gp_morton_order_workspace_bytes(int64_t nv);
int gp_morton_order(const int32_t *coords, int64_t nv, int32_t *perm, int32_t *rank,
                    void *workspace, size_t workspace_bytes, void *stream);
/* gp_grid_build: coords must already be in Morton order (as produced by perm).  The grid lives   */
/* in `grid` (gp_grid_bytes(nv, extent) bytes).  extent_host: 3 ints = max-min+1 per axis,        */
/* origin_host: 3 ints = min per axis.                                                           */
size_t gp_grid_bytes(int64_t nv, const int32_t *extent_host);
int gp_grid_build(const int32_t *coords, int64_t nv, const int32_t *origin_host,
                  const int32_t *extent_host, void *grid, size_t grid_bytes, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Row 8: torch_scatter.scatter_mean(src, index, dim=0) (models/affinity_module.py:1524-1535).   */
/* CSR form (deterministic, sums in ascending point id): seg_start i64 [nv+1], order i64 [n].     */
/* out[v, col0:col0+d] = mean over the voxel's points.  ld_src / ld_out in floats.                */
int gp_scatter_mean_csr(const float *src, int64_t ld_src, int32_t d, const int64_t *order,
                        const int64_t *seg_start, int64_t nv, const int32_t *row_map,
                        float *out, int64_t ld_out, int32_t col0, void *stream);
/* out[p, 0:d] = src[index[p], 0:d]   (final voxel->point gather, affinity_module.py:1589)        */
int gp_gather_rows(const float *src, int64_t ld_src, int32_t d, const int64_t *index, int64_t n,
                   const int32_t *row_map, float *out, int64_t ld_out, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Row 9: MinkowskiEngine submanifold convolution (models/affinity_module.py:36-66,1541-1546).   */
/* gp_kernel_map_build: nbr_map i32 [27,nv]; nbr_map[k][u] = row of voxel coords[u]+o_k or -1,   */
/* k = (dx+1)+3(dy+1)+9(dz+1).  Needs the grid built from the same Morton-ordered coords.         */
int gp_kernel_map_build(const void *grid, const int32_t *coords, int64_t nv, int32_t *nbr_map,
                        void *stream);
/* Batched coordinates (ME's batched_coordinates: int32 [nv,4] = batch, x, y, z, any row order).  key = batch << 48 |           */
/* morton(xyz - min) with 16 bits per axis (gp_morton3's interleave, x lowest; min per axis over all rows), radix-sorted:        */
/* perm / rank as gp_morton_order, keys_sorted u64 [nv].  status i32 [3] (device, written by the call): [0] rows equal to the     */
/* sorted row before them (duplicates), [1] rows whose batch index is outside 0..65535, [2] mask of the axes whose extent       */
/* (max - min + 1) is 65536 or more.  Any nonzero status: the order and keys are undefined.  No host sync.                     */
size_t gp_coords_order_batched_workspace_bytes(int64_t nv);
int gp_coords_order_batched(const int32_t *coords, int64_t nv, int32_t *perm, int32_t *rank, uint64_t *keys_sorted,
                            int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
/* Quantisation of a batched point cloud, the step the reference does by hand in front of the student                           */
/* (models/affinity_module.py:1192-1212: torch.unique(return_inverse) + scatter_mean + ME.SparseTensor; this entry replaces the   */
/* unique / inverse part and hands the reductions their CSR).  coords int32 [n,4] = batch, x, y, z, any row order, duplicate      */
/* rows allowed, 16-byte aligned.  Same key and sort as gp_coords_order_batched.  Outputs, all sized at capacity (nv is only      */
/* known on the device): vox_coords i32 [n,4] the unique rows in ascending key order; unique_index i64 [n] the lowest input row   */
/* of each voxel; inverse i64 [n] input row -> voxel row; order i64 [n] + seg_start i64 [n+1] the CSR gp_scatter_mean_csr takes   */
/* (order ascends in input row inside every voxel); status i32 [3] = (nv, rows whose batch index is outside 0..65535, mask of     */
/* the axes whose extent is 65536 or more).  Rows nv.. of the per-voxel outputs are not written.  A nonzero status[1] or [2]:     */
/* the outputs are defined and in range but meaningless.  1 <= n < 2^31.  No host sync, no float atomics.                         */
size_t gp_quantize_batched_workspace_bytes(int64_t n);
int gp_quantize_batched(const int32_t *coords, int64_t n, int32_t *vox_coords, int64_t *unique_index, int64_t *inverse,
                        int64_t *order, int64_t *seg_start, int32_t *status, void *workspace, size_t workspace_bytes,
                        void *stream);
/* Per-voxel label over the CSR of gp_quantize_batched: labels i64 [n], out i64 [nv].  rule 0 (first): labels[unique_index[v]];   */
/* 1 (differ): ignore_label when any two labels of the voxel differ, else that label (ME's sparse_quantize(labels=,               */
/* ignore_label=)); 2 (count): ignore_label when the voxel holds more than one row (dataset/voxelization_utils.py:86-89).         */
int gp_segment_labels(const int64_t *labels, int64_t n, const int64_t *order, const int64_t *seg_start,
                      const int64_t *unique_index, int64_t nv, int64_t ignore_label, int32_t rule, int64_t *out, void *stream);
/* 27-offset map over the sorted keys of gp_coords_order_batched (same layout and offset order as gp_kernel_map_build):        */
/* nbr_map[k][u] = row of the key of voxel u + o_k in the same batch entry, or -1.  Binary search of the keys.                 */
int gp_kernel_map_sorted(const uint64_t *keys_sorted, int64_t nv, int32_t *nbr_map, void *stream);
/* Y[u, :] = epilogue( sum_k X[nbr_map[k][u], :] @ W[k] ),  W fp32 [kv, cin, cout] row-major,      */
/* kv = 27 (nbr_map [27,nv]) or 1 (nbr_map NULL: identity).  epilogue: y = acc*scale + shift      */
/* (scale/shift fp32 [cout] or NULL), optional residual add (fp32 [nv, ld_res] or NULL), optional  */
/* ReLU.  cin % 8 == 0 (pad channels with zeros), cout % 128 == 0.                                */
int gp_sparse_conv(const float *x, int64_t ld_x, const int32_t *nbr_map, int64_t nv,
                   const float *w, int32_t kv, int32_t cin, int32_t cout,
                   const float *scale, const float *shift, const float *residual, int64_t ld_res,
                   int32_t relu, float *y, int64_t ld_y, void *stream);
/* tiles i32 [3] (host) = gp_sparse_conv's row tile, its column tile (cout is a multiple of it) and its channel step (cin is a      */
/* multiple of it): what a caller pads dense operands to.                                                                          */
int gp_sparse_conv_tiles(int32_t *tiles);
/* Fast path of the same convolution on the f16 matrix cores with fp32-class accuracy (operands     */
/* split x = hi + lo in f16, products hi*hi + hi*lo + lo*hi accumulated in fp32; relative error of   */
/* a product <= 2^-21).  gp_conv_pairs_build compacts the kernel map once per scene: pair_in i32     */
/* [num_pairs] (input row per pair, ordered by (chunk of output rows, k, output row)),                  */
/* pair_pos i32 [kv,nv] (pair index or -1), seg_off i32 [nseg+1] (first pair of each (chunk,k) segment, */
/* nseg = num_chunks*kv; seg_off[nseg] = num_pairs), tile_start i32 [nseg+1] (256-pair tiles before     */
/* each segment).  The chunks are given by their row offsets chunk_row_off (DEVICE i32 [num_chunks+1], */
/* 0 = first, nv = last, ascending): equal heights, or the heights of gp_conv_chunk_plan.              */
/* gp_conv_weights_split: w fp32 [kv,cin,cout] -> w_hi/w_lo f16 [kv,cout,cin] of scale_pow2 * w.       */
/* gp_sparse_conv_f16x3: `partial` = 4 * num_pairs * cout bytes of workspace (the largest chunk's pairs */
/* when chunked) for the partial rows between the two phases -- fp32 rows on the register-staged path   */
/* (x fp32), 24-bit block floating point on the LDS-DMA path (x_hi / x_lo; 3 bytes per element + one    */
/* exponent byte per (pair row, 128 columns): rounded within 2^-22 of the quarter's largest magnitude,   */
/* the rounding of the f16 hi + lo split that follows; an element is u = rint(v 2^(148 - E)) + 2^22 with  */
/* 0 <= u <= 2^23, both ends reached, and E is clamped to >= 22: values below 2^-104 stay below 2^-104; */
/* an Inf / NaN activation row makes the output      */
/* rows that gather it NaN -- so does ONE overflowing element of a partial row: its whole 128-column    */
/* quarter is marked, where fp32 rows kept Inf in that element and finite neighbours.  The 24-bit rows   */
/* use 32-bit byte offsets: a call whose largest chunk holds pairs * cout * 3 >= 4 GiB runs on fp32     */
/* partial rows instead, decided before the first launch); its contents are private to the call.        */
/* Epilogue as gp_sparse_conv (the                                                                       */
/* caller folds 1/scale_pow2 into `scale`).  cin % 32 == 0, cout % 256 == 0, |x| < 65504.              */
size_t gp_conv_pairs_workspace_bytes(int64_t nv, int32_t kv);
int gp_conv_pairs_build(const int32_t *nbr_map, int64_t nv, int32_t kv, int32_t num_chunks, const int32_t *chunk_row_off,
                        int32_t *pair_in, int32_t *pair_pos, int32_t *seg_off, int32_t *tile_start,
                        int32_t *tile_desc /* i32 [num_pairs/256 + nseg, 4]: {k, first pair, count, 0} per tile */,
                        void *workspace, size_t workspace_bytes, void *stream);
/* Chunk heights chosen from the kernel map so that every chunk's phase-1 launch -- sum over the offsets of ceil(pairs / 256)  */
/* row tiles, times col_tiles (= cout / 256) column tiles -- stays within target_tiles (the host passes 3 x the CU count - 16:   */
/* three rounds of one-tile workgroups; equal heights leave 4-8 % of the tile slots of their rounds empty).  Chunks close at multiples of        */
/* granule_rows (>= 64).  Outputs on the DEVICE: chunk_row_off i32 [max_chunks + 1], n_chunks i32 [1]; the caller reads them      */
/* back to size the pair arrays and to pass the host copy to gp_sparse_conv_f16x3.                                               */
size_t gp_conv_chunk_plan_workspace_bytes(int64_t nv, int32_t granule_rows);
int gp_conv_chunk_plan(const int32_t *nbr_map, int64_t nv, int32_t kv, int32_t granule_rows, int32_t col_tiles,
                       int32_t target_tiles, int32_t max_chunks, int32_t *chunk_row_off, int32_t *n_chunks, void *workspace,
                       size_t workspace_bytes, void *stream);
int gp_conv_weights_split(const float *w, int32_t kv, int32_t cin, int32_t cout, float scale_pow2,
                          void *w_hi, void *w_lo, void *stream);
/* Optional pre-split operands: x_hi/x_lo f16 [nv, ld_xh] (from gp_split_f16 or a previous layer's   */
/* y_hi/y_lo) select the LDS-DMA staging path (x may then be NULL); y_hi/y_lo f16 [nv, ld_yh] (or      */
/* NULL) receive the split output for the next layer; with them y may be NULL (no fp32 copy).          */
int gp_split_f16(const float *x, int64_t ld_x, int32_t d, int64_t n, void *hi, void *lo, int64_t ld_h,
                 void *stream);
/* Power-of-two pre-scaling of split operands, so that the f16 lo halves stay NORMAL numbers and x = hi + lo holds to  */
/* 2^-22 RELATIVE also for small magnitudes (unscaled, |x| < 2^-3 leaves lo subnormal: absolute error 2^-25).          */
/* gp_pow2_scale: scale2[0] = s = 2^k with amax(|x[0:n, 0:d]|) * s in [2^13, 2^14), scale2[1] = 1/s (device scalars, */
/* no host sync; workspace >= 4 bytes).  gp_split_f16_scaled: hi + lo = x * s with s = *scale (global, nullable) or,   */
/* when row_inv_scale != NULL, a per-row s(row) chosen the same way, row_inv_scale[row] = 1/s(row).  Exact (powers of  */
/* two); consumers multiply back: gp_pool_mfma_apply(out_scale), gp_sparse_conv_f16x3(x_row_inv_scale).                */
/* gp_split_f16_scaled with lo = NULL: INTERLEAVED rows into hi ([d / 32 steps][hi 32 | lo 32], ld_h >= 2 d): the operand  */
/* form of gp_sparse_conv_f16x3's plane_flags bit 0.                                                                      */
int gp_pow2_scale(const float *x, int64_t ld_x, int32_t d, int64_t n, float *scale2, void *workspace,
                  size_t workspace_bytes, void *stream);
/* dst_row (nullable, i32 [n]): row r of x is written to row dst_row[r] of hi / lo / row_inv_scale (a permutation: gp_rcb_order).   */
int gp_split_f16_scaled(const float *x, int64_t ld_x, int32_t d, int64_t n, void *hi, void *lo, int64_t ld_h,
                        const float *scale, float *row_inv_scale, const int32_t *dst_row, void *stream);
/* gp_voxel_rows_operands: row 8 and what the first layer and the pooling take from it, in one pass (one wave per voxel).  Equal,  */
/* bit for bit, to: x zeroed; gp_scatter_mean_csr(f, d, col0 = 0) and gp_scatter_mean_csr(geo, dg, col0 = d) into x through        */
/* row_map; gp_split_f16_scaled(x, cin_pad, lo = NULL, row_inv_scale) (the interleaved row-scaled operand); gp_pow2_scale(x, d).   */
/* x f32 [nv, ld_x >= cin_pad] is written whole (columns d + dg .. cin_pad - 1 are zeros), rows f16 [nv, ld_rows >= 2 cin_pad],   */
/* row_inv_scale f32 [nv], all at row row_map[v] (nullable: v).  scale2 (nullable, 2 floats) <- [s, 1/s] of max |x[:, 0:d]|, then  */
/* workspace >= 4 bytes.  d % 4 == 0, cin_pad % 32 == 0, d + dg <= cin_pad <= 1024; f and x 16-byte aligned with ld % 4 == 0.     */
/* No host sync.                                                                                                                  */
int gp_voxel_rows_operands(const float *f, int64_t ld_f, int32_t d, const float *geo, int64_t ld_geo, int32_t dg,
                           const int64_t *order, const int64_t *seg_start, int64_t nv, const int32_t *row_map, float *x,
                           int64_t ld_x, int32_t cin_pad, void *rows, int64_t ld_rows, float *row_inv_scale, float *scale2,
                           void *workspace, size_t workspace_bytes, void *stream);
int gp_sparse_conv_f16x3(const float *x, int64_t ld_x, const void *x_hi, const void *x_lo, int64_t ld_xh,
                         const int32_t *pair_in, const int32_t *pair_pos,
                         const int32_t *seg_off, const int32_t *tile_start, const int32_t *tile_desc,
                         int32_t nseg, int64_t num_pairs, int64_t nv, int32_t kv,
                         const void *w_hi, const void *w_lo, int32_t cin, int32_t cout, float *partial,
                         const float *scale, const float *shift, const float *residual, int64_t ld_res,
                         int32_t relu, float *y, int64_t ld_y, void *y_hi, void *y_lo, int64_t ld_yh,
                         int32_t num_chunks, const int32_t *chunk_row_off_host, const int32_t *chunk_tile_off_host,
                         const int32_t *chunk_pair_off_host, const float *x_row_inv_scale, float *y_row_inv_scale,
                         const void *res_hi, const void *res_lo, int64_t ld_rh, const float *res_row_inv_scale, int32_t w_blocked,
                         int32_t plane_flags, void *stream);
/* plane_flags bit 4 (16): ONE offset (kv = 1) whose map holds every output row -- a gather-GEMM y[u] = x[pair_in[u]] @ w[0] (the training   */
/* sampler's anchors x points similarity): phase 1 stores fp32 rows straight into y (contiguous, ld_y = cout; no scale / shift / residual / */
/* ReLU / split output) and phase 2 is not run.                                                                                            */
/* plane_flags (mask): 1 = x_hi is ONE tensor of INTERLEAVED rows, [cin / 32 steps][hi 32 | lo 32] halfs per row (ld_xh >= 2 cin; x_lo  */
/* unused): the LDS-DMA kernel then stages a row and K step as ONE full 128-byte line instead of two half lines; 2 = y_hi receives the   */
/* output in that form (y_lo unused; what the next layer reads); 4 = the residual planes res_hi come in that form.  0: separate planes. */
/* plane_flags bit 5 (32): phase 2 over the 24-bit partial rows walks its output rows ONE AT A TIME (the reference walk) instead of        */
/* keeping the next row's partial rows in flight while a row is reduced (the default up to 512 columns): same bits, for comparisons.      */
/* w_blocked = 1: w_hi / w_lo come from gp_conv_weights_split_blocked -- the same halves as [kv][cout / 256][cin / 32][256][32]: a K   */
/* step's 16 KiB of a column tile contiguous (one 1-KiB run per LDS-DMA instruction instead of 16 half lines), row rho of a tile =     */
/* its column (rho & 128) | (rho & 15) << 3 | (rho >> 4 & 7).  cin % 32 == 0, cout % 256 == 0.  0: the [kv][cout][cin] halves above.    */
/* transpose_flip = 1: the data-gradient operand V[k] = W[kv - 1 - k]^T straight from the forward layer's w: cin / cout are V's (the      */
/* forward layer's cout / cin), w is read as [kv][cout][cin] with the offsets mirrored -- no flipped, transposed fp32 copy in between.  */
int gp_conv_weights_split_blocked(const float *w, int32_t kv, int32_t cin, int32_t cout, float scale_pow2,
                                  void *w_hi, void *w_lo, int32_t transpose_flip, void *stream);
/* res_hi / res_lo f16 [nv, ld_rh] (+ res_row_inv_scale fp32 [nv] or NULL): the residual as the split planes an earlier layer wrote  */
/* (its y_hi / y_lo / y_row_inv_scale) instead of fp32 rows -- (hi + lo) * inv, the value that layer's consumer multiplied with; the    */
/* producer then needs no fp32 copy (y = NULL).  `residual` and res_hi exclude each other.                                             */
/* Chunked execution (num_chunks >= 1, the chunks the pairs were built with): phase 1 / phase 2 alternate  */
/* per chunk so that `partial` (then sized for the largest chunk) stays in the Infinity Cache;             */
/* chunk_row_off_host = HOST copy of the row offsets, chunk_tile_off_host / chunk_pair_off_host =           */
/* tile_start / seg_off at the chunk boundaries, all [num_chunks+1]; num_chunks = 0: none of them.          */
/* in-place row L2 normalisation, F.normalize(p=2, dim=1, eps=1e-12) (affinity_module.py:1547)     */
int gp_l2norm_rows(float *x, int64_t ld, int32_t d, int64_t n, void *stream);
/* The student's 1x1x1 output convolution (hidden -> 128 embedding channels, affinity_module.py:66,71) on the pre-split rows   */
/* the last 3x3x3 layer writes, fused with the row normalisation above (:1547) when l2_normalize != 0:                        */
/* y[r, :] = out_scale * x_row_inv_scale[r] * sum_c (x_hi + x_lo)[r, c] * (w_hi + w_lo)[:, c]   (three exact f16 products per  */
/* element, fp32 accumulation, fixed order).  w_hi / w_lo f16 [cout, cin] from gp_conv_weights_split(kv = 1, scale 2^k),       */
/* out_scale = 2^-k; x_row_inv_scale nullable (unscaled planes).  cout = 128, cin a multiple of 64.                            */
/* e_hi / e_lo (nullable pair, f16 [nv, 128]): also / instead (y may then be NULL) the rows x plane_scale as hi + lo planes --   */
/* the operand of gp_affinity_cs_fragments (plane_scale 1024), written by the same epilogue instead of a separate split pass.    */
int gp_embed_head_f16x3(const void *x_hi, const void *x_lo, int64_t ld_x, const float *x_row_inv_scale, const void *w_hi,
                        const void *w_lo, int64_t nv, int32_t cin, int32_t cout, float out_scale, int32_t l2_normalize,
                        float *y, int64_t ld_y, void *e_hi, void *e_lo, float plane_scale,
                        const int32_t *e_dst_row /* nullable: plane row of input row r (gp_rcb_order's map); y keeps the input order */,
                        void *stream);

/* Row order of the POOLING operator (row 12's matrix-core kernels gather, per block of 128 consecutive rows, the union of the      */
/* rows' neighbours: compact blocks have smaller unions).  gp_rcb_order: inside chunks of chunk_rows (1024 or 2048) consecutive rows   */
/* of the Morton-ordered integer coords [nv, 3], recursive coordinate bisection into leaves of leaf_rows rows (every leaf but a       */
/* chunk's last is full).  sigma i32 [nv]: new position -> row, rho i32 [nv]: row -> new position (both permutations of 0 .. nv - 1   */
/* that keep every chunk in place).  gp_rows_renumber_i32: out[p, j] = rho[nbr[sigma[p], j]] for i32 [nv, k] neighbour lists.           */
/* No reference counterpart: an internal order, composed away before any output (models/affinity_module.py:1575-1589 sees none).        */
int gp_rcb_order(const int32_t *coords, int64_t nv, int32_t chunk_rows, int32_t leaf_rows, int32_t *sigma, int32_t *rho, void *stream);
int gp_rows_renumber_i32(const int32_t *nbr, int64_t nv, int32_t k, const int32_t *sigma, const int32_t *rho, int32_t *out,
                         void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Row 10: faiss.IndexFlatL2.search(K+1) on integer voxel coordinates, self dropped              */
/* (models/affinity_module.py:1551-1557).  Exact; canonical tie rule (d^2, id) ascending where id  */
/* = ids[row] (NULL: the row number).  nbr i32 [nv,K] holds ROW numbers of the given arrays,      */
/* emitted in (d^2, id) order.  coords Morton-ordered + grid as above.  K <= GP_KNN_MAX_K.         */
size_t gp_knn_workspace_bytes(int64_t nv);
int gp_knn_lattice(const void *grid, const int32_t *coords, const int32_t *ids, int64_t nv,
                   int32_t k, int32_t *nbr, void *workspace, size_t workspace_bytes, void *stream);
/* gp_knn_lattice reads a query's candidates once where its first ring holds at most 2048 of them (and nv <= 2^25): their d^2   */
/* and rows stay in registers between the histogram and the emit.  gp_knn_lattice_two_pass: the form that reads them twice (what   */
/* larger blocks take inside gp_knn_lattice as well); same arguments, same lists -- kept for tests and timing.                     */
int gp_knn_lattice_two_pass(const void *grid, const int32_t *coords, const int32_t *ids, int64_t nv,
                            int32_t k, int32_t *nbr, void *workspace, size_t workspace_bytes, void *stream);
/* Row 10 over batched coordinates: the same rule inside every batch entry.  keys_sorted u64 [nv] are the sorted keys of             */
/* gp_coords_order_batched (batch << 48 | morton(xyz - min)), ids i32 [nv] the tie-break id of each sorted row (its perm: ties then     */
/* resolve by the input's row order inside each entry; NULL: the row number).  nbr i32 [nv,K] holds SORTED-ROW numbers: the K+1         */
/* smallest by (d^2, id) among the rows of the query's own entry, self dropped, in that order; exact for every input.  Rows of          */
/* different entries never appear in each other's lists, also where two entries occupy the same coordinates.  No coordinate array       */
/* is read: coordinates are decoded from the keys, 8^3 cells (key >> 9) are found by binary search in a cell table built per call,      */
/* rings 1 and 3 as gp_knn_lattice, then an exhaustive scan of the query's entry alone.  1 <= K <= GP_KNN_MAX_K, 1 <= nv < 2^31.        */
/* status i32 [4] (device, written by the call): [0] queries whose entry holds K or fewer voxels -- their nbr rows are filled with -1; */
/* [1] the lowest such batch index (-1: none); [2] its voxel count; [3] mask of the axes on which a decoded coordinate is 32768 or     */
/* more: the (d^2 << 32 | id) key needs d^2 < 2^32, so with a nonzero mask the lists are undefined (the call still returns, and         */
/* stores only row numbers of the query's entry or -1).  No host sync, nothing read or written outside the given extents.              */
size_t gp_knn_batched_workspace_bytes(int64_t nv);
int gp_knn_batched(const uint64_t *keys_sorted, const int32_t *ids, int64_t nv, int32_t k, int32_t *nbr, int32_t *status,
                   void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Row 11: cosine affinity + sharpened softmax (models/affinity_module.py:1559-1572).             */
/* w[i,j] = softmax_j( sharpen * <E_i, E_nbr[i,j]> ),  E fp32 [nv, ld_e], first d columns.         */
int gp_affinity_softmax(const float *e, int64_t ld_e, int32_t d, const int32_t *nbr, int32_t k,
                        int64_t nv, float sharpen, float *w, void *stream);
/* The same weights, written to w AND -- x 2^10, split hi + lo -- to element dst[i * k + j] of the pooling operator's fragment   */
/* arrays (dst, wa_hi, wa_lo from gp_pool_cs_structure): the value gp_pool_cs_fill would read back from w, so the operator has  */
/* the same bits and no fill pass runs between the student and the 19 applications.                                          */
int gp_affinity_softmax_scatter(const float *e, int64_t ld_e, int32_t d, const int32_t *nbr, int32_t k, int64_t nv,
                                float sharpen, float *w, const int32_t *dst, void *wa_hi, void *wa_lo, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Row 12: one application of the row-stochastic affinity operator, torch.sparse.mm(A, X)        */
/* (models/affinity_module.py:1575-1587) in ELL form: Y[i,0:d] = sum_j w[i,j] * X[nbr[i,j],0:d].   */
/* d % 4 == 0, ld_x/ld_y % 4 == 0.  X and Y must not alias.                                       */
int gp_pool_ell(const float *x, int64_t ld_x, const int32_t *nbr, const float *w, int32_t k,
                int64_t nv, int32_t d, float *y, int64_t ld_y, void *stream);

/* The backward of rows 11 + 12 (models/affinity_module.py:1564-1587), for a loss on the pooled features.  No float atomics: every    */
/* sum runs over a list in a fixed order, the results are bitwise reproducible.  All pitches in floats, multiples of 4 and >= d;      */
/* fp32 row matrices 16-byte aligned; 1 <= k <= 128; nv * k < 2^31; outputs alias no input.                                           */
/* The inverted index of the lists (models/affinity_module.py:1564-1587: the transpose of the operator torch.sparse.mm applies):      */
/* tr_slot[tr_off[m] .. tr_off[m+1]) = the slots i * k + j with nbr[i,j] == m, ascending.  tr_off i64 [nv+1], tr_slot i32 [nv*k]       */
/* (slots whose id lies outside 0..nv-1 come behind tr_off[nv], in no list).  In-degree count, scan, stable radix sort.               */
size_t gp_pool_transpose_workspace_bytes(int64_t nv, int32_t k);
int gp_pool_transpose_build(const int32_t *nbr, int64_t nv, int32_t k, int64_t *tr_off, int32_t *tr_slot, void *workspace,
                            size_t workspace_bytes, void *stream);
/* One application of the transposed operator (models/affinity_module.py:1564-1587):                                                  */
/* out[m,0:d] = sum_p w[slot_p] * g[slot_p / k, 0:d] over the list of m in list order; an empty list writes an exact zero row.        */
int gp_pool_ell_transpose(const float *g, int64_t ld_g, const int64_t *tr_off, const int32_t *tr_slot, const float *w, int32_t k,
                          int64_t nv, int32_t d, float *out, int64_t ld_out, void *stream);
/* The gradient of the weights from one application (models/affinity_module.py:1564-1587): dw[i,j] = <g[i], x_prev[nbr[i,j]]>,        */
/* added to dw when accumulate != 0.  An id outside 0..nv-1 gives 0.                                                                  */
int gp_pool_ell_wgrad(const float *g, int64_t ld_g, const float *x_prev, int64_t ld_x, const int32_t *nbr, int32_t k, int64_t nv,
                      int32_t d, float *dw, int32_t accumulate, void *stream);
/* The backward of gp_affinity_softmax (models/affinity_module.py:1564-1587) on unit rows e_unit:                                     */
/* da[i,j] = sharpen * w[i,j] * (dw[i,j] - sum_k w[i,k] dw[i,k]);                                                                      */
/* de_unit[i] = sum_j da[i,j] e_unit[nbr[i,j]] + sum over the inverted list of i of da[slot] e_unit[slot / k], in that order.          */
size_t gp_affinity_softmax_backward_workspace_bytes(int64_t nv, int32_t k);
int gp_affinity_softmax_backward(const float *e_unit, int64_t ld_e, int32_t d, const int32_t *nbr, const float *w, const float *dw,
                                 int32_t k, int64_t nv, float sharpen, const int64_t *tr_off, const int32_t *tr_slot, float *de_unit,
                                 int64_t ld_de, void *workspace, size_t workspace_bytes, void *stream);
/* The backward of gp_l2norm_rows (F.normalize's, models/affinity_module.py:1564-1587): with u = e / |e|,                              */
/* de_raw = (de_unit - u <u, de_unit>) / |e|, and de_unit / 1e-12 where |e| < 1e-12.                                                   */
int gp_l2norm_rows_backward(const float *e_raw, int64_t ld_e, const float *de_unit, int64_t ld_du, int32_t d, int64_t n,
                            float *de_raw, int64_t ld_de, void *stream);

/* Fast path of the same operator, re-blocked once per scene for the 19 applications: tiles of r     */
/* Morton-adjacent rows (r in {4,8,16}); per tile the union of its rows' neighbours and a dense        */
/* [union, r] weight block.  count: tile_off i64 [ntiles+1] (exclusive scan; last = total entries,     */
/* read it back to size u_row i32 [total] and u_w f32 [total, r]); fill; apply = one application.       */
/* apply: d a multiple of 256 (r = 8, 16) or of 512 (r = 4: a wave keeps 512 columns; d = 256 is       */
/* GP_EINVAL), or d = 64 with r = 4 or 8 (a tile per wave).                                            */
size_t gp_pool_tiles_workspace_bytes(int64_t nv, int32_t r);
int gp_pool_tiles_count(const int32_t *nbr, int64_t nv, int32_t k, int32_t r, int64_t *tile_off,
                        void *workspace, size_t workspace_bytes, void *stream);
int gp_pool_tiles_fill(const int32_t *nbr, const float *w, int64_t nv, int32_t k, int32_t r,
                       const int64_t *tile_off, int32_t *u_row, float *u_w, void *stream);
int gp_pool_tiles_apply(const float *x, int64_t ld_x, const int64_t *tile_off, const int32_t *u_row,
                        const float *u_w, int32_t r, int64_t nv, int32_t d, float *y, int64_t ld_y,
                        void *stream);

/* Matrix-core variant (d = 512): blocks of block_rows (64 or 128) rows, the block's neighbour union    */
/* swept in steps of 32 rows on v_mfma_f32_16x16x32_f16 with split operands (x = hi + lo in f16;        */
/* hi*hi + hi*lo + lo*hi accumulated in fp32).  nblocks = ceil(nv / block_rows), nw = block_rows / 16.   */
/* bu_off i64 [nblocks+1] (padded union rows, multiples of 32), bu_n i32 [nblocks] (unpadded sizes),     */
/* bu_row i32 [total], wa_hi/wa_lo f16 [total/32 * nw * 64 * 8] (weights x 2^10 in MFMA A-fragment order).*/
/* apply: x_hi/x_lo f16 [*, ld_x] -> y_hi/y_lo f16 (nullable pair) and/or y_f32 (nullable).              */
/* min_steps: every row block is padded (zero weights) to at least this many 32-row steps; 0 unless the   */
/* operator is built for gp_pool_mfma_apply_persistent, which needs 9.                                    */
size_t gp_pool_mfma_workspace_bytes(int64_t nv, int32_t block_rows);
int gp_pool_mfma_count(const int32_t *nbr, int64_t nv, int32_t k, int32_t block_rows, int32_t min_steps,
                       int64_t *bu_off, int32_t *bu_n, void *workspace, size_t workspace_bytes, void *stream);
int gp_pool_mfma_fill(const int32_t *nbr, const float *w, int64_t nv, int32_t k, int32_t block_rows,
                      const int64_t *bu_off, const int32_t *bu_n, int64_t total_rows, int32_t *bu_row,
                      void *wa_hi, void *wa_lo, void *stream);
int gp_pool_mfma_apply(const void *x_hi, const void *x_lo, int64_t ld_x, const int64_t *bu_off,
                       const int32_t *bu_row, const void *wa_hi, const void *wa_lo, int64_t nv, int32_t d,
                       int32_t block_rows, void *y_hi, void *y_lo, int64_t ld_y, float *y_f32,
                       int64_t ld_yf, const float *out_scale, void *stream);
/* Persistent form of the same operator (one 512-thread workgroup per CU walks (row block, 256-column half) tiles;  */
/* both column groups of waves share every staged weight fragment; the LDS-DMA ring stays full across row blocks; */
/* the epilogue stores straight from the accumulators).  Extra requirements: min_steps = min over row blocks of   */
/* (bu_off[b+1]-bu_off[b])/32 must be >= 9; the output holds y_rows >= ceil(nv/block_rows)*block_rows rows (rows  */
/* >= nv receive zeros); exactly one of (y_hi,y_lo) / y_f32.  out_scale: optional device scalar multiplied into  */
/* the fp32 output (undoes a power-of-two pre-scaling of the split operands).  queue: 9 x uint32 of device memory, */
/* zero before the first launch and left zero by every launch (per-XCD tile counters: workgroups claim their next */
/* tile dynamically, which keeps neighbouring tiles together in L2); launches sharing a queue must be stream-     */
/* ordered; NULL = static tile lists.  Replaces the 19 torch.sparse.mm calls of                                    */
/* models/affinity_module.py:1584-1587 like gp_pool_mfma_apply.                                                    */
int gp_pool_mfma_apply_persistent(const void *x_hi, const void *x_lo, int64_t ld_x, const int64_t *bu_off,
                                  const int32_t *bu_row, const void *wa_hi, const void *wa_lo, int64_t nv,
                                  int32_t d, int32_t block_rows, int32_t min_steps, void *y_hi, void *y_lo,
                                  int64_t ld_y, float *y_f32, int64_t ld_yf, int64_t y_rows,
                                  const float *out_scale, uint32_t *queue, void *stream);

/* Column-sliced matrix-core variant (d = 256, 512, 768 or 1024; the default from round 3 on): blocks of rows x 256-column */
/* slices (d / 256 per row block: the two halves at d = 512), every                                                        */
/* wave owns all rows x 32 columns; the builder orders a block's union rows by the 16-row groups that use them and         */
/* stores one bit per (32-row step, group): all-zero 16 x 32 weight fragments are neither fetched nor multiplied.        */
/* rows_per_block (16..128, the same value for count, fill and apply; 128 unless there is a reason): the block height.    */
/* nblocks = ceil(nv / rows_per_block).  bu_off i64 [nblocks+1] (padded union rows, multiples of 32), bu_n i32 [nblocks],   */
/* bu_row i32 [total], bu_mask u32 [total/32] (bit g: group g of the step has a non-zero), wa_hi/wa_lo f16               */
/* [total/32 * 8 * 512] (weights x 2^10 in MFMA fragment order; only fragments whose bit is set are defined and read).   */
/* Same numerics and operand conventions as gp_pool_mfma_apply.  Replaces the 19 torch.sparse.mm calls of                */
/* models/affinity_module.py:1575-1589.  gp_pool_cs_count needs the neighbour lists only: a scheduler can run it (and the  */
/* host read-back of bu_off[nblocks] that sizes the arrays) before the affinity weights exist.                            */
size_t gp_pool_cs_workspace_bytes(int64_t nv, int32_t rows_per_block);
/* max_union (device i64, may be NULL): receives the largest block union.  The fill passes take it (max_union argument, 0 = not   */
/* known) to size their LDS tables -- 56 KiB instead of 152 KiB per workgroup on a ScanNet-shaped scene -- together with the      */
/* host read-back of bu_off[nblocks].                                                                                           */
int gp_pool_cs_count(const int32_t *nbr, int64_t nv, int32_t k, int32_t rows_per_block, int64_t *bu_off, int32_t *bu_n,
                     int64_t *max_union, void *workspace, size_t workspace_bytes, void *stream);
int gp_pool_cs_fill(const int32_t *nbr, const float *w, int64_t nv, int32_t k, int32_t rows_per_block, const int64_t *bu_off,
                    int64_t total_rows, int32_t max_union, int32_t *bu_row, uint32_t *bu_mask, void *wa_hi, void *wa_lo, void *stream);
/* gp_pool_cs_fill without the weights: bu_row, bu_mask, zeroed fragments and dst i32 [nv, k] = the element of wa_hi / wa_lo that  */
/* (row, neighbour j) owns; gp_affinity_softmax_scatter completes the operator.  Needs the neighbour lists only (a scheduler runs */
/* it ahead, like gp_pool_cs_count).  total_rows * 128 must fit 32 bits (else: gp_pool_cs_fill).                               */
int gp_pool_cs_structure(const int32_t *nbr, int64_t nv, int32_t k, int32_t rows_per_block, const int64_t *bu_off,
                         int64_t total_rows, int32_t max_union, int32_t *bu_row, uint32_t *bu_mask, void *wa_hi, void *wa_lo,
                         int32_t *dst, void *stream);
/* The structure for gp_affinity_cs_fragments: union rows, fragment masks and valid u32 [total_rows / 32 * 128 + 64]: bit p of  */
/* valid[step * 128 + row] = union row 32 step + p of the row's block is one of that row's neighbours (the last 64 words are     */
/* padding).  No fragment is touched.  Needs the neighbour lists only; their ids must be distinct within a row (k-NN lists are).  */
int gp_pool_cs_structure_valid(const int32_t *nbr, int64_t nv, int32_t k, int32_t rows_per_block, const int64_t *bu_off,
                               int64_t total_rows, int32_t max_union, int32_t *bu_row, uint32_t *bu_mask, uint32_t *bu_valid,
                               void *stream);
/* Row 11 (models/affinity_module.py:1559-1572) fused with the operator fill, on the matrix cores: e_hi / e_lo = the unit          */
/* embeddings x 2^10 as f16 planes [nv, 128] (gp_split_f16_scaled, scale 1024); every (row, union row) similarity of a non-empty   */
/* fragment is computed as hi hi + hi lo + lo hi on v_mfma_f32_16x16x32_f16, the valid ones go through the row's softmax           */
/* (x sharpen), and every non-empty fragment of wa_hi / wa_lo is written whole (weights x 2^10, zeros elsewhere).  d = 128, k <= 96. */
/* Produces no [nv, k] weight matrix (gp_affinity_softmax does).                                                                  */
int gp_affinity_cs_fragments(const void *e_hi, const void *e_lo, int64_t nv, int32_t d, int32_t k, float sharpen,
                             const int64_t *bu_off, const int32_t *bu_row, const uint32_t *bu_mask, const uint32_t *bu_valid,
                             int32_t rows_per_block, void *wa_hi, void *wa_lo, void *stream);
/* One application y = A x.  d = 256, 512, 768 or 1024 (whole 256-column slices; any other d: GP_EINVAL).  The tuning bits of    */
/* knob 4 apply to d = 512 only.                                                                                                 */
int gp_pool_cs_apply(const void *x_hi, const void *x_lo, int64_t ld_x, const int64_t *bu_off, const int32_t *bu_row,
                     const uint32_t *bu_mask, const void *wa_hi, const void *wa_lo, int64_t nv, int32_t d,
                     int32_t rows_per_block, void *y_hi, void *y_lo, int64_t ld_y, float *y_f32, int64_t ld_yf,
                     const float *out_scale, void *stream);
/* ALL `applications` (2..65535) of the operator in ONE launch (the T = 19 torch.sparse.mm calls of                          */
/* models/affinity_module.py:1575-1587 as one kernel): application t reads plane set (t even ? x : p) and writes the other   */
/* one, the last one writes y_f32 (x out_scale[0]) only -- the sequence, planes and bits of `applications` calls of           */
/* gp_pool_cs_apply ping-ponging between x and p; x_hi / x_lo are rewritten from application 1 on.  A row block's tile of     */
/* application t starts when the row blocks of its dependency list have published application t - 1 (per-block flags,         */
/* written-through stores, L1-bypassing gathers); workgroups wait only for workgroups with a smaller index.                   */
/*   gp_pool_cs_deps: dep i32 [nblocks * 64] from the operator's structure (bu_off, bu_row), scratch i32 [nblocks].           */
/*   d: as gp_pool_cs_apply (256, 512, 768 or 1024).                                                                         */
/*   flags u32 [gp_pool_cs_chain_flag_words_d(nv, rows_per_block, d)]: zeroed ONCE at allocation.  Word 0 is the ABORT      */
/*     word: set to 1 by the kernel if a workgroup waited 2 s for a dependency (the launch drains without computing, outputs invalid); the caller reads it   */
/*     at its next synchronisation point and treats non-zero as an error.                                                     */
/*   epoch: kept by the caller per flags array, each call at least `applications` above the previous call's.                  */
/* One flags array serves one launch at a time (do not share it between streams).                                             */
int gp_pool_cs_deps(const int64_t *bu_off, const int32_t *bu_row, int64_t nv, int32_t rows_per_block, int32_t *dep,
                    int32_t *scratch, void *stream);
/* words of the flags array: 32 header words + d / 256 column slices x nblocks (0 for a d or rows_per_block the kernels reject); */
/* gp_pool_cs_chain_flag_words is the d = 512 size.                                                                           */
size_t gp_pool_cs_chain_flag_words(int64_t nv, int32_t rows_per_block);
size_t gp_pool_cs_chain_flag_words_d(int64_t nv, int32_t rows_per_block, int32_t d);
int gp_pool_cs_apply_chain(void *x_hi, void *x_lo, void *p_hi, void *p_lo, int64_t ld, const int64_t *bu_off,
                           const int32_t *bu_row, const uint32_t *bu_mask, const void *wa_hi, const void *wa_lo, int64_t nv,
                           int32_t d, int32_t rows_per_block, int32_t applications, float *y_f32, int64_t ld_yf,
                           const float *out_scale, const int32_t *dep, uint32_t *flags, uint32_t epoch, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Rows 5-7: 2D->3D lift (models/affinity_module.py:416-449, 495-646, 647-696).                   */
/* gp_lift_dense_accum: sum[pt[i], :] += feat2d[:, x[i], y[i]] ; cnt[pt[i]] += 1 for one view.     */
int gp_lift_dense_accum(const float *feat2d, int32_t d, int32_t height, int32_t width,
                        const int64_t *pt, const int64_t *x, const int64_t *y, int64_t n_v,
                        float *sum, int64_t ld_sum, float *cnt, void *stream);
/* gp_lift_dense_bilinear_accum: the LSeg path (affinity_module.py:404-433): feat f32 [d,h,w] is the network's    */
/* low-resolution map; the reference's F.interpolate(bilinear, align_corners=True) to [out_h,out_w] is evaluated   */
/* only at the sampled pixels (x = row, y = col of the full-size image), bit-identical to torch's CPU kernel.      */
int gp_lift_dense_bilinear_accum(const float *feat, int32_t d, int32_t h, int32_t w, int32_t out_h, int32_t out_w,
                                 const int64_t *pt, const int64_t *x, const int64_t *y, int64_t n_v,
                                 float *sum, int64_t ld_sum, float *cnt, void *stream);
/* gp_lift_dense_finish: out = sum / (cnt==0 ? 1e-6 : cnt); seen[p] = cnt > 1e-5 (u8).             */
int gp_lift_dense_finish(float *sum, int64_t ld_sum, int32_t d, const float *cnt, int64_t n,
                         uint8_t *seen, void *stream);
/* gp_lift_masks_view: per visible point pick the segment k* = argmax_q score[q]*sigmoid(m_q(x,y)) */
/* over queries with score>0, where m_q is the bicubic-antialias resize of pred_masks [Q,h,w] to    */
/* mask_shape evaluated only at the sampled pixel (separable taps tap_x0/tap_wx [W,4],              */
/* tap_y0/tap_wy [H,4] precomputed on the host); seg[i] = k* if sigmoid(m_k*) >= 0.5 else -1.       */
/* Equal products: the smallest query index wins.  No query with score > 0: seg = -1, seg_logit = 0. */
/* The arrays must be non-null also when n_v = 0 (GP_EINVAL otherwise; nothing is launched then).    */
size_t gp_lift_masks_workspace_bytes(int32_t q, int32_t h, int32_t w);
int gp_lift_masks_view(const float *pred_masks, int32_t q, int32_t h, int32_t w,
                       const float *scores, const int32_t *tap_x0, const float *tap_wx,
                       const int32_t *tap_y0, const float *tap_wy, int32_t out_h, int32_t out_w,
                       const int64_t *x, const int64_t *y, int64_t n_v, int32_t *seg,
                       float *seg_logit, void *workspace, size_t workspace_bytes, void *stream);
/* gp_lift_masks_views: rows 6-7 up to the point -> (view, segment) lists for ALL views of a scene at once (entries      */
/* from gp_views_visible_lists; pred_masks f32 [nsrc,Q,h,w] and scores f32 [nsrc,Q] stacked over the source views,        */
/* nviews <= nsrc, nviews <= 128).  Per entry the segment of gp_lift_masks_view; then the in-view fill                    */
/* (affinity_module.py:604-625: an entry without a segment takes the one of the nearest entry with a segment in the       */
/* same view, (fp64 squared distance of the fp32 xyz [n,3], entry order) minimum = gp_nn1_masked_f64's rule); then the     */
/* CSR pv_start i64 [n+1], pv_view / pv_seg i32 [total] that gp_fuse_views_top3 reads, a point's entries in ascending      */
/* view order (= gp_pv_count + scan + gp_pv_fill called view by view).  seg i32 [total] out.  Entries of views with       */
/* keep == 0 take no part.  fill_cap: capacity, in fill queries (entries without a segment), of the in-view fill's       */
/* partial-result arrays: 1..total, or 0 = total.  ANY value gives the same results -- queries beyond the capacity are     */
/* answered by one block per 256 of them sweeping the view's whole reference range -- a capacity near the expected query   */
/* count keeps the fill fully parallel and the workspace small (192 B per unit of capacity).                               */
/* Preconditions: Q <= 1024 (a view's scores are sorted in LDS; more: GP_EINVAL -- lift view by view with                  */
/* gp_lift_masks_view, which takes any Q), and scores >= 0 (they are softmax maxima in the reference, :544): the kernel      */
/* visits a pixel's queries in descending score order and stops once the next 64 scores lie below the best                   */
/* score x sigmoid(logit) found, which bounds a candidate only while sigmoid <= 1 multiplies a non-negative score.            */
size_t gp_lift_masks_views_workspace_bytes(int32_t nsrc, int32_t q, int32_t h, int32_t w, int64_t total, int64_t n,
                                           int64_t fill_cap);
int gp_lift_masks_views(const float *pred_masks, int32_t nsrc, int32_t q, int32_t h, int32_t w, const float *scores,
                        const int32_t *tap_x0, const float *tap_wx, const int32_t *tap_y0, const float *tap_wy,
                        int32_t out_h, int32_t out_w, const float *xyz, int64_t n, const int64_t *ent_pt,
                        const int64_t *ent_x, const int64_t *ent_y, const int32_t *ent_view, const int64_t *view_off,
                        const uint8_t *keep, int32_t nviews, int64_t total, int64_t fill_cap, int32_t *seg, int64_t *pv_start,
                        int32_t *pv_view, int32_t *pv_seg, void *workspace, size_t workspace_bytes, void *stream);
/* gp_segment_tables: per view, f_seg[q,:] = normalize(mask_embed[q,:]) and                         */
/* logit_seg[q,c] = logit_scale * <f_seg[q], normalize(text[c])>  (affinity_module.py:627-630;       */
/* every point feature is a segment embedding).                                     */
int gp_segment_tables(const float *mask_embed, int32_t q, int32_t d, const float *text_norm,
                      int32_t c, float logit_scale, float *f_seg, float *logit_seg, void *stream);
/* point -> (view, segment) CSR, replacing the reference's per-point Python dict                       */
/* (affinity_module.py:633-639): gp_pv_count adds 1 to cnt[pt[i]] for one view; after all views an    */
/* exclusive scan gives pv_start; gp_pv_fill appends (view, seg[i]) to every visible point's slot      */
/* list (views must be filled in ascending order on one stream; cursor i32 [n] zero-initialised).     */
int gp_pv_count(const int64_t *pt, int64_t n_v, int64_t *cnt, void *stream);
size_t gp_scan_workspace_bytes(int64_t n);
int gp_exclusive_scan_i64(const int64_t *in, int64_t n, int64_t *out, void *workspace,
                          size_t workspace_bytes, void *stream);
int gp_pv_fill(const int64_t *pt, const int32_t *seg, int64_t n_v, int32_t view,
               const int64_t *pv_start, int32_t *cursor, int32_t *pv_view, int32_t *pv_seg,
               void *stream);
/* gp_fuse_views_top3: CSR over points (pv_start i64 [n+1]; pv_view i32, pv_seg i32 per slot in      */
/* ascending view order; seg -1 = zero feature): consensus class = argmax of the mean logits,        */
/* top-min(M,3) views by agreement, softmax weights, weighted sum of segment features                */
/* f_seg fp32 [V,Q,d], logit_seg fp32 [V,Q,c].  out fp32 [n, ld_out]; seen u8 [n].                    */
/* The rules at equality: the consensus class is the FIRST maximum of the mean logits; among equal    */
/* agreement logits the EARLIER slot (lower view) ranks first, so it is the later one the top-3 cut    */
/* drops.  A seg -1 slot counts in M, has logit 0 for every class (it can be among the top 3), keeps   */
/* its softmax weight and adds a zero feature: a point whose slots are all -1 gets a zero row with     */
/* seen = 1; a point without slots a zero row with seen = 0.  d and ld_out must be multiples of 4      */
/* (rows are moved 16 bytes at a time; GP_EINVAL otherwise), f_seg and out 16-byte aligned.            */
/* The lists are trusted: every pv_view must lie in [0, V) and every pv_seg in [-1, q); a slot left     */
/* unwritten by its producer indexes the tables out of bounds.                                         */
int gp_fuse_views_top3(const int64_t *pv_start, const int32_t *pv_view, const int32_t *pv_seg,
                       int64_t n, const float *f_seg, const float *logit_seg, int32_t q, int32_t d,
                       int32_t c, float *out, int64_t ld_out, uint8_t *seen, void *stream);
/* gp_seen_masks: seen[p] = (pv_start[p + 1] > pv_start[p]), unseen[p] = 1 - seen[p] (u8 [n] each): the reference and query   */
/* masks of the scene-level fill (gp_nn1_masked_f64) from the list offsets alone, so that the search can run before the fusion. */
int gp_seen_masks(const int64_t *pv_start, int64_t n, uint8_t *seen, uint8_t *unseen, void *stream);
/* gp_fuse_views_top3_fill: gp_fuse_views_top3 with the scene-level fill (:687-696) applied while the row is made: row p is     */
/* fused from the list of point nn[p] where 0 <= nn[p] < n (gp_nn1_masked_f64 over gp_seen_masks: the nearest seen point of a   */
/* point without a list), from its own list otherwise.  Same kernel, same loops: out equals gp_fuse_views_top3 followed by      */
/* gp_gather_rows(nn >= 0 ? nn : p) bit for bit, written once.  A point whose own list is empty and whose nn is -1 (no seen     */
/* point anywhere) keeps a zero row.  nn i64 [n]; the other arguments and their alignment as in gp_fuse_views_top3.             */
int gp_fuse_views_top3_fill(const int64_t *pv_start, const int32_t *pv_view, const int32_t *pv_seg,
                            int64_t n, const float *f_seg, const float *logit_seg, int32_t q, int32_t d,
                            int32_t c, const int64_t *nn, float *out, int64_t ld_out, void *stream);
/* gp_nn1_fill_f64: exact 1-NN (fp64 distances on fp32 coordinates, lowest index on ties) from       */
/* query points to reference points; writes nn[i] = index into ref.  (sklearn KDTree k=1,           */
/* affinity_module.py:619-625,693-696; run/validation.py:425-430.)                                   */
size_t gp_nn1_workspace_bytes(int64_t n_ref, int64_t n_query);
int gp_nn1_f64(const float *ref_xyz, int64_t n_ref, const float *query_xyz, int64_t n_query,
               int64_t *nn, void *workspace, size_t workspace_bytes, void *stream);
/* masked form (no host synchronisation): references = points with ref_mask != 0, queries = points  */
/* with query_mask != 0, both subsets of xyz fp32 [n,3]; nn i64 [n] = index into xyz for queries,    */
/* -1 elsewhere.  If there is no reference point nn stays -1 everywhere.                            */
size_t gp_nn1_masked_workspace_bytes(int64_t n);
int gp_nn1_masked_f64(const float *xyz, int64_t n, const uint8_t *ref_mask, const uint8_t *query_mask,
                      int64_t *nn, void *workspace, size_t workspace_bytes, void *stream);
/* Loader glue (dataset/data_loader_ablation.py:257-264,348-351): ordered lists of the visible      */
/* points of one view from its mapping i64 [n,3]: pt (ascending ids), x = pixel row, y = pixel col;  */
/* *count_dev receives n_v.  Outputs must hold n entries.                                           */
size_t gp_visible_lists_workspace_bytes(int64_t n);
int gp_visible_lists(const int64_t *mapping, int64_t n, int64_t *pt, int64_t *x, int64_t *y,
                     int64_t *count_dev, void *workspace, size_t workspace_bytes, void *stream);
/* The same for ALL views of a scene in four launches (instead of V x {gp_project_points_f64, gp_visible_lists}):      */
/* params f64 [V,20] on the DEVICE = row-major world->camera matrix (16) | fx fy cx cy; depth f64 [V,H,W] or NULL.      */
/* Entries (view, point, pixel row, pixel col) come out view-major, ascending point id inside a view -- the               */
/* concatenation of the per-view lists: ent_pt / ent_x / ent_y i64 and ent_view i32 must hold V*n entries; view_off i64   */
/* [V+1] = first entry of each view (+ total); keep u8 [V] = the loader's view-drop rule (data_loader_ablation.py:       */
/* 254-255, 280-288): n_v != 0, n_v >= min_visible, n_v <= val_keep.  V <= 65535, V*n < 2^31.                            */
size_t gp_views_visible_lists_workspace_bytes(int64_t n, int32_t nviews);
int gp_views_visible_lists(const double *coords, int64_t n, const double *params, const double *depth, int32_t nviews,
                           int32_t width, int32_t height, int32_t cut_bound, double vis_thres, int64_t min_visible,
                           int64_t val_keep, int64_t *ent_pt, int64_t *ent_x, int64_t *ent_y, int32_t *ent_view,
                           int64_t *view_off, uint8_t *keep, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Row 13 + caller tail (run/validation.py:413-416, util/util.py:160-177).                        */
/* pred[p] = argmax_c <normalize(F[p]), text_norm[c]> (first max on ties); zero_row[p] = sum|F|==0  */
int gp_classify_argmax(const float *feat, int64_t ld, int32_t d, int64_t n, const float *text_norm,
                       int32_t c, float logit_scale, int64_t *pred, uint8_t *zero_row, void *stream);
/* gp_gather_rows (the final voxel -> point gather, affinity_module.py:1589) and gp_classify_argmax (run/validation.py:413-416) in   */
/* ONE pass: out[p, 0:d] = src[row_map[index[p]], 0:d] and pred / zero_row of those rows -- the per-point matrix is written once    */
/* and not read back.  Same bits and labels as the two calls.  d a multiple of 64 up to 1024, c * d * 4 <= 64 KiB.                 */
int gp_gather_rows_classify(const float *src, int64_t ld_src, int32_t d, const int64_t *index, int64_t n, const int32_t *row_map,
                            float *out, int64_t ld_out, const float *text_norm, int32_t c, float logit_scale, int64_t *pred,
                            uint8_t *zero_row, void *stream);
/* arg-max over the first c columns of logits rows fp32 [n, ld] (e.g. gp_sparse_conv with kv=1 as the   */
/* exact-fp32 MFMA GEMM F @ T^T); zero_row from feat (optional).                                      */
int gp_rows_argmax(const float *logits, int64_t ld, int32_t c, int64_t n, const float *feat, int64_t ld_f,
                   int32_t d, int64_t *pred, uint8_t *zero_row, void *stream);
/* counts i64 [3,C] += (intersection, output, target) histograms with the ignore-id overwrite.      */
int gp_iou_hist_i64(const int64_t *pred, const int64_t *target, int64_t n, int32_t num_classes,
                    const int64_t *ignore_ids_host, int32_t num_ignore, int64_t *counts,
                    void *stream);
/* The zero-row fill of run/validation.py:417-431 (KDTree over the non-zero rows, k = 1) over BATCHED coordinates: masked exact 1-NN    */
/* inside every batch entry.  keys_sorted u64 [nv] and ids i32 [nv] as gp_knn_batched takes them (NULL ids: the row number);            */
/* ref_mask / query_mask u8 [nv] in SORTED-row order (non-zero = set).  nn i32 [nv]: for a query row the SORTED-ROW number of the        */
/* reference row of the SAME entry that minimises (d^2, id), d^2 the integer squared distance over the axes of `axes` (bit 0 = x,       */
/* 1 = y, 2 = z; 1..7 -- 6 is the reference's slice quirk, :422-423); -1 for rows that are no queries and for queries whose entry       */
/* holds no reference.  Equal d^2: the lower id wins; a row set in both masks finds itself; rows of other entries never win, also       */
/* where entries occupy the same coordinates.  No coordinate array is read.  Rings 1 and 3 over an 8^3 cell table of the reference      */
/* keys, accepted only at d^2 strictly below (8R+1)^2, then a scan of the entry's references; axes != 7 scans at once.                  */
/* 1 <= nv < 2^31.  status i32 [4] (device, written by the call): [0] queries; [1] reference rows; [2] queries left at -1 (their entry  */
/* has no reference); [3] mask of the axes on which a decoded coordinate is 32768 or more: the (d^2 << 32 | id) key needs d^2 < 2^32,  */
/* so with a nonzero mask nn is undefined (the call still returns, and stores only rows of the query's entry or -1).  No host sync,   */
/* integer arithmetic only, nothing read or written outside the given extents.                                                          */
size_t gp_nn1_batched_workspace_bytes(int64_t nv);
int gp_nn1_batched(const uint64_t *keys_sorted, const int32_t *ids, const uint8_t *ref_mask, const uint8_t *query_mask, int64_t nv,
                   int32_t axes, int32_t *nn, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
/* counts i64 [B,3,C] += the histograms of gp_iou_hist_i64 (util/util.py:160-177) separated by batch entry, in one pass.  Item p of n  */
/* takes pred[r] and the batch index coords[r,0] of row r = index[p] (index i64 [n]: the per-point form through a quantiser's inverse  */
/* map; NULL: r = p and n must equal rows), coords i32 [rows,4], and target[p].  Same ignore-id overwrite (at most 4 ids), values      */
/* outside 0..C-1 dropped; an item whose row is outside 0..rows-1 or whose batch index is outside 0..B-1 is counted nowhere.           */
/* 1 <= B <= 65536, 1 <= C <= 4096, 1 <= rows < 2^31.  Integer atomics only (LDS counters when B*3*C <= 12288, else 64-bit atomics on  */
/* counts): the result does not depend on arrival order.                                                                               */
int gp_iou_hist_batched_i64(const int64_t *pred, const int32_t *coords, int64_t rows, const int64_t *target, const int64_t *index,
                            int64_t n, int32_t num_batches, int32_t num_classes, const int64_t *ignore_ids_host, int32_t num_ignore,
                            int64_t *counts, void *stream);
/* Classification cross-entropy of SparseTensor rows against text embeddings, forward and gradient (the differentiable twin of the     */
/* labelling above): u_i = y_i / max(|y_i|, 1e-12), z_ic = s <u_i, t_c>, lse_i = log sum_c exp(z_ic),                                   */
/*   loss = sum over the valid items p of w_b(p) (lse_i(p) - z_i(p),l_p),   dz_ic = w_b(i) (m_i softmax_ic - cnt_ic).                  */
/* The products Z = U T^T and dU = s G T are gp_sparse_conv's (kv = 1); the four calls below stand around them.  No float atomics:      */
/* two calls give the same bits.  Nothing is read or written outside the given extents.  Every call refuses an output whose extent      */
/* overlaps an input's or another output's (labels and item_id of gp_segment_loss_rows' per-point form, whose lengths are no argument,  */
/* count from their first element on).  gp_segment_loss_col_step: the columns per lane step of the row kernels (64).                    */
int32_t gp_segment_loss_col_step(void);
/* gp_segment_loss_unit_rows: u f32 [n, ld_u >= d_pad] = the unit rows of y f32 [n, ld_y >= d] with zeros in the columns d .. d_pad-1,   */
/* zero u8 [n] = (sum |y_i| == 0), the zero flag of gp_classify_argmax.  1 <= n < 2^31.                                                 */
int gp_segment_loss_unit_rows(const float *y, int64_t ld_y, int32_t d, int64_t n, float *u, int64_t ld_u, int32_t d_pad, uint8_t *zero,
                              void *stream);
/* gp_segment_loss_items: the valid items.  Item q of p takes the row r = index[q] (index i64 [p], a quantiser's inverse map; NULL:    */
/* r = q and p must equal n) and the label labels[q]; it is valid when 0 <= label < c, the label is none of the ignore ids (at most 4), */
/* r is inside 0..n-1, zero[r] is clear and the batch index coords[r,0] (coords i32 [n,4]) is inside 0..65535.  With an index:           */
/* item_off i64 [n+1] and item_id i32 [p] receive the CSR of the valid items by row, item numbers ascending inside a row (integer        */
/* counts + a scan + a stable sort; the tail of item_id holds the invalid items); without: row_valid u8 [n].  entry_cnt i64 [65536] =    */
/* the valid items V_b per batch entry, entry_w f32 [65536] = 1 / V (reduction 0, "item") or 1 / (E V_b) (1, "entry": E the entries      */
/* with V_b > 0), 0 where V_b = 0.  status i64 [4] (device, written by the call): [0] rows with a batch index outside 0..65535, [1]      */
/* items with a row outside 0..n-1, [2] the highest batch index inside the range, [3] V.  1 <= c <= 4096, 1 <= n, p < 2^31.  No sync.   */
size_t gp_segment_loss_items_workspace_bytes(int64_t n, int64_t p);
int gp_segment_loss_items(const int32_t *coords, const uint8_t *zero, int64_t n, const int64_t *labels, const int64_t *index, int64_t p,
                          int32_t c, const int64_t *ignore_ids_host, int32_t num_ignore, int32_t reduction, uint8_t *row_valid,
                          int64_t *item_off, int32_t *item_id, int64_t *entry_cnt, float *entry_w, int64_t *status, void *workspace,
                          size_t workspace_bytes, void *stream);
/* gp_segment_loss_rows: the row kernel over a chunk of r rows of logits z f32 [r, ld_z >= c], one wave per row.  coords, row_valid,    */
/* item_off, lse and term are the chunk's own rows (pointers advanced to its first row; item_off's values stay positions in the whole   */
/* item_id); labels is indexed by item number (with item_off + item_id) or by chunk row (both NULL: the item of a row is the row        */
/* itself where row_valid is set).  g f32 [r, ld_g >= c_pad] = w_b(i) (m_i softmax_ic - cnt_ic) with exact zeros in the columns         */
/* c .. c_pad-1 (the softmax with the row maximum subtracted; the counts come off as integers in list order before the weight, so one   */
/* class gives exactly 0), lse f32 [r], term f64 [r] = m_i lse_i - sum over the row's items of z_i,l.  A row without items stores       */
/* zeros and reads no logits.  g NULL: lse and term alone (the forward), no g is stored.  1 <= c <= 4096, r * ld < 2^31, pitches         */
/* multiples of 4, z / g 16-byte aligned.                                                                                               */
int gp_segment_loss_rows(const float *z, int64_t ld_z, int64_t r, int32_t c, int32_t c_pad, const int32_t *coords, const uint8_t *row_valid,
                         const int64_t *item_off, const int32_t *item_id, const int64_t *labels, const float *entry_w, float *g,
                         int64_t ld_g, float *lse, double *term, void *stream);
/* gp_segment_loss_reduce: loss f32 (device scalar, overwritten) = sum_b w_b S_b and per_entry f32 [num_entries] = S_b / V_b (NaN where  */
/* V_b = 0), S_b the fp64 sum of term over the rows of entry b in a fixed order (rows sorted by entry, a strided sum per thread, a tree   */
/* over the threads), w_b in fp64 from entry_cnt as above.  num_entries = the highest batch index + 1, 1..65536; 1 <= n < 2^31.           */
size_t gp_segment_loss_reduce_workspace_bytes(int64_t n, int32_t num_entries);
int gp_segment_loss_reduce(const double *term, const int32_t *coords, int64_t n, const int64_t *entry_cnt, int32_t num_entries,
                           int32_t reduction, float *loss, float *per_entry, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* training step of the student (models/affinity_module.py:1138-1237,                */
/* run/train.py:188-198,346-353).  Convolutions forward / dgrad reuse gp_sparse_conv_f16x3 (dgrad   */
/* = the same operator with weights V[k] = W[26-k]^T); these are the remaining pieces.              */
/* gp_col_stats: mean / biased variance of the rows (BatchNorm1d in training mode over voxel rows): ONE sweep, fp64 sums of x and  */
/* x^2 in a fixed order, var = max(E[x^2] - mean^2, 0) in fp64 (53-bit sums of 24-bit data: the cancellation costs                 */
/* log2(mean^2 / var) of ~29 spare bits).                                                                                            */
size_t gp_col_stats_workspace_bytes(int64_t nv, int32_t c);
int gp_col_stats(const float *y, int64_t ld, int64_t nv, int32_t c, float *mean, float *var,
                 void *workspace, size_t workspace_bytes, void *stream);
/* out = [relu]((y-mean)/sqrt(var+eps)*gamma + beta [+ residual]) (out nullable when the planes are asked for); out_hi/out_lo: optional split f16 */
/* copy for the next convolution; running_mean/var (nullable) <- (1-m)*running + m*batch (unbiased var). */
int gp_bn_train_apply(const float *y, int64_t ld, int64_t nv, int32_t c, const float *mean, const float *var,
                      const float *gamma, const float *beta, float eps, const float *residual, int64_t ld_res,
                      int32_t relu, float *out, int64_t ld_out, void *out_hi, void *out_lo, int64_t ld_split,
                      float momentum, float *running_mean, float *running_var, void *stream);
/* dz = dout*mask; dgamma = sum dz*xhat; dbeta = sum dz.  mask: act > 0 (act = the layer's fp32 output); or act NULL and beta_mask given -- a */
/* layer without a residual -- recomputed from y as (y-mean)/sqrt(var+eps)*gamma + beta_mask > 0, the value gp_bn_train_apply evaluated (the  */
/* same float: the activation is then neither read here nor, with out = NULL in gp_bn_train_apply, ever written); both NULL: no mask.        */
/* dy = gamma/sqrt(var+eps)*(dz - dbeta/nv - xhat*dgamma/nv); dz_out (nullable) <- dz.                */
/* dy_scale2 (nullable, 2 floats on the device) <- [s, 1/s] of gp_pow2_scale(dy), taken inside the sweep that writes dy: */
/* the scale of the gradient's f16 split (gp_split_f16_scaled) without another pass over it.                           */
/* SPLIT FORM (dy = NULL, dy_hi / dy_lo f16 [nv + 1, ld_h] and dy_scale2 given; c % 4 == 0, 16-byte aligned rows): the sweep writes    */
/* hi + lo = dy * s itself, row nv zeroed (the weight gradient's padded pairs), dy_scale2 = [s, 1/s] with s the power of two of a BOUND  */
/* of max |dy| -- |gamma| / std x (max |dz| + |sum dz| / n + max |xhat| |sum dz xhat| / n) per column, from maxima taken in the           */
/* reduction pass -- so that no fp32 dy is written and no separate split pass reads it (bound / true maximum: a small factor).          */
/* workspace: gp_bn_train_backward_workspace_bytes(nv, c).                                            */
size_t gp_bn_train_backward_workspace_bytes(int64_t nv, int32_t c);
int gp_bn_train_backward(const float *dout, int64_t ld_dout, const float *act, int64_t ld_act, const float *y,
                         int64_t ld_y, const float *mean, const float *var, float eps, const float *gamma, const float *beta_mask,
                         int64_t nv, int32_t c, float *dy, int64_t ld_dy, float *dz_out, int64_t ld_dz,
                         float *dgamma, float *dbeta, float *dy_scale2, void *dy_hi, void *dy_lo, int64_t ld_h,
                         void *workspace, size_t workspace_bytes, void *stream);
/* SyncBatchNorm pieces (run/train.py:212-213 converts the student to MinkowskiSyncBatchNorm; geopurify_amd/sharding.py     */
/* all-reduces these small vectors over the ranks).  gp_col_sums_f64: mean == NULL -> out[col] = sum_r y[r][col], else         */
/* out[col] = sum_r (y[r][col] - mean[col])^2 (fp64, fixed order).  gp_bn_bwd_sums_f64: sums[0:c] = sum dz,                    */
/* sums[c:2c] = sum dz * xhat.  gp_bn_bwd_apply: the dy formula of gp_bn_train_backward with caller-supplied fp32 sums        */
/* [2c] and the row count n_total they were taken over.  workspace: gp_col_stats_workspace_bytes(nv, c).                     */
int gp_col_sums_f64(const float *y, int64_t ld, int64_t nv, int32_t c, const float *mean, double *out, void *workspace,
                    size_t workspace_bytes, void *stream);
int gp_bn_bwd_sums_f64(const float *dout, int64_t ld_dout, const float *act, int64_t ld_act, const float *y, int64_t ld_y,
                       const float *mean, const float *var, float eps, const float *gamma_mask, const float *beta_mask, int64_t nv, int32_t c,
                       double *sums, void *workspace, size_t workspace_bytes, void *stream);
int gp_bn_bwd_apply(const float *dout, int64_t ld_dout, const float *act, int64_t ld_act, const float *y, int64_t ld_y,
                    const float *mean, const float *var, float eps, const float *gamma, const float *beta_mask, const float *sums,
                    int64_t n_total, int64_t nv, int32_t c, float *dy, int64_t ld_dy, float *dz_out, int64_t ld_dz, float *dy_scale2,
                    void *stream);
/* InfoNCE (affinity_module.py:1219-1233) forward + backward: samples s -> voxel rows sample_to_voxel[s]; */
/* point_to_batch i64 [A*(2+Nn)] = sample ids of (anchors | positives | negatives row-major).           */
/* loss f32 device scalar (overwritten, not accumulated); de f32 [nv, d] = d loss / d e (overwritten;    */
/* rows no sample points at: 0).  d <= 256, 0 <= num_negatives <= 63.  The gradient rows of the samples  */
/* are summed in fp64 (a sample may be many anchors' negative: terms that cancel).                        */
size_t gp_infonce_workspace_bytes(int64_t num_samples, int32_t d);
int gp_infonce_fwd_bwd(const float *e, int64_t ld_e, int64_t nv, int32_t d, const int64_t *sample_to_voxel,
                       int64_t num_samples, const int64_t *point_to_batch, int64_t num_anchors,
                       int32_t num_negatives, float temperature, float *loss, float *de, int64_t ld_de,
                       void *workspace, size_t workspace_bytes, void *stream);
/* The same InfoNCE (affinity_module.py:1219-1233) with a weight per anchor: loss = sum_a weights[a] l_a (weights f32 [A]; 1 / A   */
/* each is the mean of gp_infonce_fwd_bwd), de follows, and anchor_loss f32 [A] receives the l_a.  The reductions over the batch    */
/* entries of a SparseTensor ("anchor": 1 / A; "entry": 1 / (entries with anchors x anchors of a's entry)) are choices of weights.  */
/* Same limits, same workspace, same fp64 gradient accumulation.                                                                     */
int gp_infonce_weighted_fwd_bwd(const float *e, int64_t ld_e, int64_t nv, int32_t d, const int64_t *sample_to_voxel,
                                int64_t num_samples, const int64_t *point_to_batch, int64_t num_anchors, int32_t num_negatives,
                                float temperature, const float *weights, float *loss, float *anchor_loss, float *de, int64_t ld_de,
                                void *workspace, size_t workspace_bytes, void *stream);
/* Weight gradient of a 3x3x3 layer on the matrix cores: dW[k] = X[in_k]^T dY[out_k] (f16 hi/lo operands, fp32    */
/* accumulate).  x_hi/x_lo f16 [nv, ld_x >= cin_pad]; y_hi/y_lo f16 [nv+1, ld_y >= cout] with row nv all zero;       */
/* pair_in/pair_out i32: per offset its (input row, output row) pairs padded to a multiple of 32 with (0, nv);      */
/* segs i32 [num_segments,4] = {offset, first step (32 pairs), steps, 0} ordered by offset; seg_off i32 [kv+1].     */
/* dw f32 [kv, cin_out, cout] = inv_scale[0] * gradient (inv_scale: device scalar, nullable).                       */
size_t gp_conv_wgrad_workspace_bytes(int64_t num_segments, int32_t cin_pad, int32_t cout);
int gp_conv_wgrad_f16x3(const void *x_hi, const void *x_lo, int64_t ld_x, const void *y_hi, const void *y_lo,
                        int64_t ld_y, const int32_t *pair_in, const int32_t *pair_out, const int32_t *segs,
                        int64_t num_segments, const int32_t *seg_off, int32_t kv, int32_t cin_pad, int32_t cin_out,
                        int32_t cout, const float *inv_scale, float *dw, void *workspace, size_t workspace_bytes,
                        void *stream);
/* torch.optim.AdamW update of one flat fp32 tensor (run/train.py:198), step >= 1.                      */
int gp_adamw_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int64_t step, void *stream);
/* K nearest other points of each query row (faiss.IndexFlatL2.search(K+1)[:,1:], affinity_module.py:1157-1166), */
/* order (d^2 in fp64 of the fp32 coordinates, row id).  What is dropped is column 0 of that order, the lowest    */
/* (d^2, id) entry -- the query row itself unless a coincident point has a lower id: then THAT point is dropped   */
/* and the query's own row stays in its list.  1 <= k <= 1023, k + 1 <= n < 2^31 (otherwise GP_EINVAL, nothing is */
/* launched); queries may repeat.  *flag_dev is cleared by every call; != 0 afterwards: some query has more than  */
/* 2048 points inside the distance bin of its (k+1)-th neighbour (massively duplicated points) -- the contents of */
/* out, all rows, are then unspecified.                                                                            */
int gp_knn_points_f32(const float *xyz, int64_t n, const int64_t *queries, int64_t num_queries, int32_t k,
                      int64_t *out, int32_t *flag_dev, void *stream);
/* The sampler's selections on the anchors x points similarity (sample_contrastive_pairs_hybrid, affinity_module.py:1116-1124):    */
/* per row a of sim fp32 [num_anchors, >= n] (leading dimension ld): positive[a] = arg-max over the points other than anchor_idx[a]   */
/* (ties: the lowest index -- torch.argmax after the -inf mark); macro[a, 0:k] = the k points of lowest similarity other than the     */
/* anchor and the positive, ascending by (value, index) (torch.topk(largest=False) after the two +inf marks).  sim is not written.    */
/* 1 <= k < 1024, k + 2 <= n <= 3 145 728 (12 288 groups of at most 256 elements in LDS).  -0 counts as +0; NaNs order above +inf.        */
int gp_sampler_select(const float *sim, int64_t ld, int64_t num_anchors, int64_t n, const int64_t *anchor_idx, int32_t k,
                      int64_t *positive, int64_t *macro, void *stream);
/* The sampler over a batched SparseTensor (affinity_module.py:1099-1136 for several scenes at once): rows live in the key order of    */
/* gp_coords_order_batched, so a batch entry is one contiguous row range, and an anchor is compared with the rows of ITS entry only.  */
/* The similarity (affinity_module.py:1113-1115) is a ragged fp32 buffer: anchor a owns the seg_len[a] floats at out + row_off[a],    */
/* out[row_off[a] + j] = <x[anchor_row[a]], x[seg_first[a] + j]> with x = hi + lo, the f16 planes [*, ld_h] of                        */
/* gp_normalize_split_f16 (d % 32 == 0: pad with zero columns), three products hi.hi + hi.lo + lo.hi accumulated in fp32 on           */
/* v_mfma_f32_16x16x32_f16.  The anchors must be grouped by entry (equal seg_first consecutive); row_off[a] % 4 == 0 (16-byte        */
/* aligned rows) and the extents [row_off[a], row_off[a] + seg_len[a]) must not overlap; floats between them are not written.        */
/* max_len = the largest seg_len; at most 65535 * 64 anchors per call.                                                                */
int gp_sim_segments_f16x3(const void *hi, const void *lo, int64_t ld_h, int32_t d, const int32_t *anchor_row, const int32_t *seg_first,
                          const int32_t *seg_len, const int64_t *row_off, int64_t num_anchors, int64_t max_len, float *out,
                          void *stream);
/* gp_sampler_select (affinity_module.py:1116-1124) over such ragged rows: row a = the row_len[a] floats at sim + row_off[a], element */
/* j standing for index row_base[a] + j; anchor_idx, positive and macro are such indices (global key rows).  Same kernel, same order  */
/* rules.  1 <= k < 1024, every row_len >= k + 2, max_len = the largest row_len <= 3 145 728.                                        */
int gp_sampler_select_segments(const float *sim, const int64_t *row_off, const int32_t *row_len, const int32_t *row_base,
                               int64_t num_anchors, int64_t max_len, const int64_t *anchor_idx, int32_t k, int64_t *positive,
                               int64_t *macro, void *stream);
/* The local negatives (affinity_module.py:1125-1133): micro[a, 0:num_micro] = the entries of nbr[a, 0:k] (i32 key rows, leading      */
/* dimension ld_nbr) with the num_micro lowest similarities in anchor a's ragged row, ascending by (value, slot in the list); an      */
/* entry equal to positive[a] counts as +inf (the reference's in-place mark).  1 <= num_micro <= k <= 128.                           */
int gp_sampler_micro_segments(const float *sim, const int64_t *row_off, const int32_t *seg_first, const int32_t *seg_len,
                              const int32_t *nbr, int64_t ld_nbr, int32_t k, const int64_t *positive, int64_t num_anchors,
                              int32_t num_micro, int64_t *micro, void *stream);
/* F.normalize(x, p=2, dim=1) (affinity_module.py:1114) written as the f16 hi/lo planes of the similarity GEMM's operands:            */
/* hi + lo = x[r] / max(|x[r]|_2, eps) for r < n; rows n <= r < n_pad of the planes are zero.  d % 4 == 0, x 16-byte aligned.         */
int gp_normalize_split_f16(const float *x, int64_t ld_x, int32_t d, int64_t n, int64_t n_pad, float eps, void *hi, void *lo,
                           int64_t ld_h, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* decode of a fused-feature file on the device (dataset/feature_loader.py:113-192). */
/* feat [feat_rows, row_bytes] holds one row per True of mask_chunk u8 [n], in point order (fp16 or  */
/* fp32 elements: rows are copied as bytes); row_keep u8 [feat_rows] (nullable: the three-key form's  */
/* "mask"); vox_ind i64 [nv] = representative point of each voxel.  With p = vox_ind[v],             */
/* in = mask_chunk[p], r = #True in mask_chunk[0..p), keep = in && (row_keep ? row_keep[r] : 1):      */
/*   mode 0 (training forms):   mask_out[v] = keep; out[j] = feat[r] for the j-th kept voxel (compact, */
/*                              voxel order).                                                         */
/*   mode 1 (evaluation forms): mask_out[v] = keep; out[v] = in ? feat[r] : 0 for every voxel.        */
/* out holds nv rows in both modes.  n_sel (device i64 [2]): [0] = number of kept voxels, [1] = number */
/* of True in mask_chunk = the rows a well-formed file holds: the caller MUST compare it with         */
/* feat_rows (the reference's host code raises on a file whose mask and row count disagree; the       */
/* kernel alone would only mask the rows beyond the file's end).                                      */
size_t gp_fused_decode_workspace_bytes(int64_t n, int64_t nv);
int gp_fused_decode(const uint8_t *mask_chunk, int64_t n, const uint8_t *row_keep, const void *feat,
                    int64_t feat_rows, int64_t row_bytes, const int64_t *vox_ind, int64_t nv, int32_t mode,
                    void *out, uint8_t *mask_out, int64_t *n_sel, void *workspace, size_t workspace_bytes,
                    void *stream);

/* ------------------------------------------------------------------------------------------ */
/* The 2D -> 3D lift over BATCHED point clouds: models/affinity_module.py:404-452 (sample each view  */
/* at the visible pixels, mean over views, unseen points take the nearest seen point) with the       */
/* point -> pixel mapping of models/utils/fusion_util.py:45-147 and the view-drop rule of            */
/* dataset/data_loader_ablation.py:254-288, for every batch entry and every view in one sequence of  */
/* launches; entries never mix.  It replaces, per scene, gp_views_visible_lists, one                 */
/* gp_lift_dense_accum / gp_lift_dense_bilinear_accum launch per view, gp_lift_dense_finish and      */
/* gp_nn1_masked_f64, and gives the same bits.                                                       */
/* points f64 [n,4] = batch index, world x, y, z, in any row order.  Entry b's points are the rows   */
/* with batch b in ascending row order, its views the v with view_entry[v] == b in ascending v.      */
/* feat f32 [nviews, h*w, d], PIXEL-MAJOR (a channels_last [V,d,h,w] tensor as it lies; an NCHW one    */
/* through gp_lift_batched_transpose); view_entry i64 [nviews]; w2c f64 [nviews,16] row-major          */
/* world->camera, worded as gp_project_points_f64 words it (the transpose of the reference's          */
/* world_view_transform, or the inverse of a camera-to-world matrix); intrinsics f64 [nviews,4] = fx,  */
/* fy, cx, cy at the image size; depth f64 [nviews,height,width] or NULL (NULL: the p_z > 0 test).     */
/* bilinear = 0: the maps are images (h == height, w == width) and a pixel's row is taken as it is;   */
/* 1: F.interpolate(bilinear, align_corners=True) of the [h,w] map to the image, evaluated at the      */
/* sampled pixels with gp_lift_dense_bilinear_accum's arithmetic.                                     */
/*   view_count i64 [nviews]: the points of the view's entry that the view sees;                      */
/*   view_keep u8 [nviews] = view_count != 0 && min_visible <= view_count <= max_visible;             */
/*   count i32 [n]: the kept views that see the point; seen u8 [n] = count > 0;                        */
/*   out f32 [n, ld_out >= d]: the fp32 sum over those views in ascending v of the sampled column,     */
/*     divided by (count == 0 ? 1e-6 : count) -- zeros for an unseen point;                           */
/*   nn i64 [n] (fill != 0; nullable otherwise): for an unseen point of an entry that has seen points  */
/*     the seen row OF ITS ENTRY that minimises (d^2, row), d^2 = (dx*dx + dy*dy) + dz*dz in fp64 over */
/*     the fp32-rounded xyz (gp_nn1_masked_f64's rule), -1 elsewhere.  out is not rewritten: the       */
/*     caller gathers rows by nn (gp_gather_rows);                                                    */
/*   status i64 [8]: [0] rows whose batch index is no integer in 0..65535, [1] views whose entry is    */
/*     outside 0..65535, [2] rows with a non-finite value, [3] the highest valid batch index, [4] seen */
/*     rows, [5] filled rows.  Rows and views counted in [0] / [1] belong to no entry (count 0, zero   */
/*     rows, nn -1, view_count 0); nothing is read or written outside the extents whatever they hold.  */
/* No float atomics: two calls give the same bits.  1 <= n < 2^31, 1 <= nviews <= 65535, d >= 1,      */
/* cut_bound >= 0.  No output may overlap an input or another output (GP_EINVAL).                     */
/* gp_lift_batched_col_chunk: the channels one pass of the lift kernel holds in registers (wider rows  */
/* take several passes).                                                                              */
int32_t gp_lift_batched_col_chunk(void);
/* src f32 [nviews, d, hw] (NCHW maps) -> dst f32 [nviews, hw, d]; dst must not overlap src.          */
int gp_lift_batched_transpose(const float *src, int32_t nviews, int32_t d, int64_t hw, float *dst, void *stream);
size_t gp_lift_batched_workspace_bytes(int64_t n, int32_t nviews);
int gp_lift_batched(const double *points, int64_t n, const float *feat, int32_t d, int32_t h, int32_t w,
                    const int64_t *view_entry, const double *w2c, const double *intrinsics, const double *depth,
                    int32_t nviews, int32_t height, int32_t width, int32_t bilinear, int32_t cut_bound, double vis_thres,
                    int64_t min_visible, int64_t max_visible, int32_t fill, float *out, int64_t ld_out, uint8_t *seen,
                    int32_t *count, int64_t *view_count, uint8_t *view_keep, int64_t *nn, int64_t *status,
                    void *workspace, size_t workspace_bytes, void *stream);
/* The same calls on maps of another element type, read in place: `elem` names the type of src / dst /   */
/* feat -- GP_ELEM_F32, GP_ELEM_F16 (IEEE binary16) or GP_ELEM_BF16; any other tag is GP_EINVAL.  Every   */
/* loaded element is converted to fp32 (exact for both half types) and then takes the arithmetic of the  */
/* fp32 call, so the outputs are the bits of the fp32 call on the caller's own upcast copy; sums and     */
/* outputs stay fp32.  The transpose keeps the element type (it moves bits).  Half maps need 2-byte      */
/* alignment only; when d is a multiple of 8 (4) and feat is 16 (8) byte aligned a lane reads 8 (4)      */
/* consecutive channels with one load.  Extents and overlap checks count elements of the tag's size.     */
/* The untagged entry points above are these with GP_ELEM_F32.                                           */
int gp_lift_batched_transpose_t(const void *src, int32_t elem, int32_t nviews, int32_t d, int64_t hw, void *dst,
                                void *stream);
int gp_lift_batched_t(const double *points, int64_t n, const void *feat, int32_t elem, int32_t d, int32_t h, int32_t w,
                      const int64_t *view_entry, const double *w2c, const double *intrinsics, const double *depth,
                      int32_t nviews, int32_t height, int32_t width, int32_t bilinear, int32_t cut_bound, double vis_thres,
                      int64_t min_visible, int64_t max_visible, int32_t fill, float *out, int64_t ld_out, uint8_t *seen,
                      int32_t *count, int64_t *view_count, uint8_t *view_keep, int64_t *nn, int64_t *status,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* gp_lift_batched, RESUMABLE: the views arrive in chunks (the VLM's batches), every chunk's maps are  */
/* read once, and after any number of chunks the result is the bits of gp_lift_batched on the          */
/* concatenation of the chunks in the order added.  Points, views, poses, modes and the drop rule are  */
/* worded as in gp_lift_batched; only the relative order of an entry's views matters, and that is the  */
/* order of arrival.  The caller owns, between the calls: state (gp_lift_stream_state_bytes(n)), sums   */
/* f32 [n, ld_sum >= d], count i32 [n] and the running status i64 [8].                                 */
/*                                                                                                    */
/* gp_lift_stream_begin: before the chunk loop of models/affinity_module.py:365-436 (its sum_features /  */
/* counter = zeros).  The points' entry tables (rows sorted stably by entry, offsets) into state, which */
/* no later call writes; sums = +0, count = 0; status [0] rows whose batch index is no integer in       */
/* 0..65535, [2] rows with a non-finite value, [3] the highest valid batch index, the others 0.        */
/*                                                                                                    */
/* gp_lift_stream_add: one pass of the chunk loop, models/affinity_module.py:365-436 (fusion_util.py:   */
/* 45-147, data_loader_ablation.py:254-288), for the nviews views of this chunk, of any entries:        */
/*   view_count i64 [nviews], view_keep u8 [nviews]: as gp_lift_batched, of this chunk's views;          */
/*   sums: every point's row continued with the sampled columns of the chunk's kept views that see it,  */
/*     one fp32 add each in ascending view index; count += their number.  The row of a point that no    */
/*     kept view of the chunk sees is neither read nor written.  No float atomics;                      */
/*   status[1] += the chunk's views whose entry is outside 0..65535 (they belong to no entry).         */
/* It does not synchronise and sizes nothing by device data.  feat f32 [nviews, h*w, d] pixel-major.   */
/*                                                                                                    */
/* gp_lift_stream_finish: the end, models/affinity_module.py:435-449.  Reads state, sums, count and     */
/* status and changes none of them, so it may be called after every chunk:                              */
/*   out f32 [n, ld_out >= d] = sums / (count == 0 ? 1e-6 : count); seen u8 [n] = count > 0;            */
/*   nn i64 [n] (fill != 0; nullable otherwise): as gp_lift_batched, the caller gathers;                */
/*   status_out i64 [8]: [0]..[3] the running status, [4] seen rows, [5] filled rows, [6] values of     */
/*     state that lay outside their range (a state that gp_lift_stream_begin did not write for these    */
/*     points; they are forced into range first: nothing is read or written outside the extents        */
/*     whatever state holds, and add checks every row number and offset it takes from it as well).     */
/* 1 <= n < 2^31, 1 <= nviews <= 65535 per chunk (the caller keeps the total within 65535 if it wants   */
/* gp_lift_batched's limit), d >= 1, cut_bound >= 0.  No output may overlap an input or another output */
/* (GP_EINVAL); sums, count and status are outputs of begin and add and inputs of finish.              */
size_t gp_lift_stream_state_bytes(int64_t n);
size_t gp_lift_stream_begin_workspace_bytes(int64_t n);
int gp_lift_stream_begin(const double *points, int64_t n, int32_t d, void *state, size_t state_bytes, float *sums,
                         int64_t ld_sum, int32_t *count, int64_t *status, void *workspace, size_t workspace_bytes,
                         void *stream);
size_t gp_lift_stream_add_workspace_bytes(int32_t nviews);
int gp_lift_stream_add(const double *points, int64_t n, const void *state, size_t state_bytes, const float *feat,
                       int32_t d, int32_t h, int32_t w, const int64_t *view_entry, const double *w2c,
                       const double *intrinsics, const double *depth, int32_t nviews, int32_t height, int32_t width,
                       int32_t bilinear, int32_t cut_bound, double vis_thres, int64_t min_visible, int64_t max_visible,
                       float *sums, int64_t ld_sum, int32_t *count, int64_t *view_count, uint8_t *view_keep,
                       int64_t *status, void *workspace, size_t workspace_bytes, void *stream);
/* gp_lift_stream_add on maps of element type `elem` (see gp_lift_batched_t); the sums stay fp32, so the */
/* chunks of one stream may differ in type.                                                             */
int gp_lift_stream_add_t(const double *points, int64_t n, const void *state, size_t state_bytes, const void *feat,
                         int32_t elem, int32_t d, int32_t h, int32_t w, const int64_t *view_entry, const double *w2c,
                         const double *intrinsics, const double *depth, int32_t nviews, int32_t height, int32_t width,
                         int32_t bilinear, int32_t cut_bound, double vis_thres, int64_t min_visible, int64_t max_visible,
                         float *sums, int64_t ld_sum, int32_t *count, int64_t *view_count, uint8_t *view_keep,
                         int64_t *status, void *workspace, size_t workspace_bytes, void *stream);
size_t gp_lift_stream_finish_workspace_bytes(int64_t n);
int gp_lift_stream_finish(const double *points, int64_t n, const void *state, size_t state_bytes, const float *sums,
                          int32_t d, int64_t ld_sum, const int32_t *count, const int64_t *status, int32_t fill, float *out,
                          int64_t ld_out, uint8_t *seen, int64_t *nn, int64_t *status_out, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* The mask-embedding lift with top-3 fusion over BATCHED point clouds: models/affinity_module.py:455-714  */
/* (lift_xdecoder_features) for every batch entry and every view in one sequence of launches, entries     */
/* never mixing and with no cap on the views of an entry.  It replaces, per scene,                        */
/* gp_views_visible_lists, gp_lift_masks_views (at most 128 views), gp_fuse_views_top3 and                */
/* gp_nn1_masked_f64, and gives the same bits.  Points, entries, views and poses are worded as in         */
/* gp_lift_batched.                                                                                       */
/*                                                                                                        */
/* gp_lift_masks_batched_lists: the visible lists of all views (fusion_util.py:45-147,                    */
/* data_loader_ablation.py:254-288, affinity_module.py:495-517), view-major: a view tests the rows of its */
/* own entry only and its entries ascend by row (count per block -> scan -> write: no atomic cursor).     */
/*   view_count i64 [nviews], view_keep u8 [nviews]: as gp_lift_batched;                                   */
/*   view_off i64 [nviews+1]: the first entry of every view, view_off[nviews] = the entries in all;        */
/*   ent_pt / ent_x / ent_y i64 [cap], ent_view i32 [cap]: global point row, pixel row, pixel column and   */
/*     view of every entry (dropped views included: gp_lift_masks_batched skips them by view_keep).        */
/*     cap = 0 with null entry arrays: count only (the caller reads status[6] and calls again);            */
/*     entries beyond cap are not written and counted in status[5];                                        */
/*   status i64 [8]: [0]..[3] as gp_lift_batched, [5] entries that did not fit, [6] entries in all,        */
/*     [7] the most views one entry has.                                                                   */
/* 1 <= n < 2^31, 1 <= nviews <= 65535, cut_bound >= 0; no output may overlap an input or another output. */
size_t gp_lift_masks_batched_lists_workspace_bytes(int64_t n, int32_t nviews);
int gp_lift_masks_batched_lists(const double *points, int64_t n, const int64_t *view_entry, const double *w2c,
                                const double *intrinsics, const double *depth, int32_t nviews, int32_t height, int32_t width,
                                int32_t cut_bound, double vis_thres, int64_t min_visible, int64_t max_visible, int64_t cap,
                                int64_t *ent_pt, int64_t *ent_x, int64_t *ent_y, int32_t *ent_view, int64_t *view_off,
                                int64_t *view_count, uint8_t *view_keep, int64_t *status, void *workspace,
                                size_t workspace_bytes, void *stream);
/* gp_lift_masks_batched: from such entries (its own or a caller's: total entries, view_off i64 [nviews+1],*/
/* keep u8 [nviews]) to the fused rows.  Per entry of a kept view the segment of gp_lift_masks_views       */
/* (:526-592: the bicubic-antialias resize of pred_masks f32 [nviews,q,h,w] evaluated at the pixel, arg-max */
/* over scores f32 [nviews,q] > 0 of score x sigmoid, first q among equals, none below sigmoid 0.5), the   */
/* in-view fill (:604-625, (d^2, row) minimum inside the view), then per point its kept views in ascending */
/* view index -- a bit set over the view's position inside its entry, `words` 64-bit words per point,      */
/* words >= ceil(most views of one entry / 64) -- fused by gp_fuse_views_top3's kernel (:647-686) over      */
/* f_seg f32 [nviews,q,d] and logit_seg f32 [nviews,q,c] (gp_segment_tables; d and ld_out multiples of 4), */
/* and the scene-level fill of gp_lift_batched inside every entry (:687-696).                              */
/*   out f32 [n, ld_out >= d]: the fused row, zeros for a point no kept view sees (before the fill);       */
/*   seen u8 [n], count i32 [n] (the kept views that see the point), nn i64 [n] (fill != 0; as             */
/*   gp_lift_batched: the caller gathers), seg i32 [total]: the segment of every entry after the in-view   */
/*   fill, -1 = none;                                                                                      */
/*   status i64 [8]: [0]..[5] as gp_lift_batched, [6] entries that are not what the lists promise (a view  */
/*     that is not the one view_off puts the entry in, a point row outside 0..n-1 or of another batch      */
/*     entry than the view's or not ascending inside the view, a pixel outside the image, a view_off that  */
/*     does not ascend from 0 to total, a tap origin outside the mask), [7] views whose position inside    */
/*     their entry is beyond words x 64.  Such entries and views take no part; nothing is read or written  */
/*     outside the extents whatever the arrays hold.                                                       */
/* fill_cap: as gp_lift_masks_views.  1 <= q <= 1024, 1 <= total < 2^31 - 1, 1 <= words <= 1024.           */
size_t gp_lift_masks_batched_workspace_bytes(int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w, int32_t out_h,
                                             int32_t out_w, int64_t total, int32_t words, int64_t fill_cap);
int gp_lift_masks_batched(const double *points, int64_t n, const int64_t *view_entry, int32_t nviews,
                          const float *pred_masks, int32_t q, int32_t h, int32_t w, const float *scores,
                          const int32_t *tap_x0, const float *tap_wx, const int32_t *tap_y0, const float *tap_wy,
                          int32_t out_h, int32_t out_w, const int64_t *ent_pt, const int64_t *ent_x, const int64_t *ent_y,
                          const int32_t *ent_view, const int64_t *view_off, const uint8_t *keep, int64_t total, int32_t words,
                          int64_t fill_cap, const float *f_seg, const float *logit_seg, int32_t d, int32_t c, int32_t fill,
                          float *out, int64_t ld_out, uint8_t *seen, int32_t *count, int64_t *nn, int32_t *seg, int64_t *status,
                          void *workspace, size_t workspace_bytes, void *stream);
/* The same on pred_masks of element type `elem` (GP_ELEM_F32 / GP_ELEM_F16 / GP_ELEM_BF16, any other    */
/* tag: GP_EINVAL, 0 bytes), read in place: the rank-ordered transposed copy in the workspace keeps the   */
/* masks' type (nviews * h * w * q elements of the tag's size), the 16 taps of a pixel are converted to   */
/* fp32 as they are loaded and the resize, the products and the decision are the fp32 call's: the same    */
/* bits as the fp32 call on the caller's own upcast copy.  The untagged entry points are these with      */
/* GP_ELEM_F32.                                                                                           */
size_t gp_lift_masks_batched_workspace_bytes_t(int32_t elem, int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w,
                                               int32_t out_h, int32_t out_w, int64_t total, int32_t words, int64_t fill_cap);
int gp_lift_masks_batched_t(const double *points, int64_t n, const int64_t *view_entry, int32_t nviews,
                            const void *pred_masks, int32_t elem, int32_t q, int32_t h, int32_t w, const float *scores,
                            const int32_t *tap_x0, const float *tap_wx, const int32_t *tap_y0, const float *tap_wy,
                            int32_t out_h, int32_t out_w, const int64_t *ent_pt, const int64_t *ent_x, const int64_t *ent_y,
                            const int32_t *ent_view, const int64_t *view_off, const uint8_t *keep, int64_t total,
                            int32_t words, int64_t fill_cap, const float *f_seg, const float *logit_seg, int32_t d, int32_t c,
                            int32_t fill, float *out, int64_t ld_out, uint8_t *seen, int32_t *count, int64_t *nn, int32_t *seg,
                            int64_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* gp_lift_masks_batched, RESUMABLE: the views arrive in chunks, every chunk's masks are read once, and   */
/* after any number of chunks the result is the bits of gp_lift_masks_batched on the concatenation of the */
/* chunks in the order added.  Only the relative order of an entry's views matters, and that is the order */
/* of arrival.  The caller owns, between the calls: state (gp_lift_masks_stream_state_bytes(n): the       */
/* points' entry tables and one view counter per entry), the running status i64 [8], and what grows with  */
/* the views -- per view its entry i64, position inside its entry i32 (-1: the view has no entry), keep   */
/* u8 and record offset i64 [views + 1], its rows of f_seg / logit_seg (gp_segment_tables) -- and with    */
/* the visible (point, kept view) pairs: one record (rec_row i32, rec_seg i32 or -1) each, view-major,    */
/* rows ascending inside a view.  Nothing of the size of the masks is kept.                                */
/*                                                                                                        */
/* gp_lift_masks_stream_begin: before the view loop of models/affinity_module.py:495-640.  The entry      */
/* tables into state, the counters 0; status [0] rows whose batch index is no integer in 0..65535, [2]    */
/* rows with a non-finite value, [3] the highest valid batch index, the others 0.                         */
/*                                                                                                        */
/* gp_lift_masks_stream_sizes: what the caller's one read-back per chunk carries, after the counting call */
/* of gp_lift_masks_batched_lists on the chunk (view_count, view_keep): sizes i64 [4] = the chunk's        */
/* visible entries, those of its kept views (the records the chunk appends), the most views one entry has */
/* once the chunk is added (= 64 x words of finish, rounded up), 0.  It changes nothing.                   */
/*                                                                                                        */
/* gp_lift_masks_stream_add: models/affinity_module.py:495-640 for the nviews views of this chunk, of any */
/* entries, from the chunk's visible lists (gp_lift_masks_batched_lists: total entries, view_off, keep):   */
/*   view_pos i32 [nviews]: counter of the view's entry + its rank among the chunk's views of that entry  */
/*     in ascending chunk index; the counters advance; status[4] = the most views of one entry so far;    */
/*   the checked entries, score sort, ordered transpose, segment decision and in-view fill of              */
/*     gp_lift_masks_batched over a workspace sized by the chunk;                                          */
/*   rec_off i64 [nviews + 1] = rec_base + the records of the chunk's kept views before each view;         */
/*     rec_row / rec_seg [rec_base ..): the records (an entry the checks replaced: row -1); nothing is    */
/*     written at or beyond rec_cap;                                                                      */
/*   status[1] += views whose entry is outside 0..65535, [5] += records, [6] += entries that are not what */
/*     the lists promise and counters that lay outside 0..65535.                                          */
/* total = 0 (nothing visible in the chunk; the masks, entry arrays and records may be null) advances the */
/* counters and writes view_pos and rec_off alone.  It does not synchronise.                               */
/*                                                                                                        */
/* gp_lift_masks_stream_finish: the fusion and the fill, models/affinity_module.py:647-714, over all views */
/* added so far (nviews, total records, words >= ceil(most views of one entry / 64)).  Reads everything   */
/* kept and changes none of it, so it may be called after every chunk.  out, seen, count, nn: as          */
/* gp_lift_masks_batched.  status_out i64 [8]: [0]..[3] the running status, [4] seen rows, [5] filled     */
/* rows, [6] the running [6] + values of state, record offsets and records that lay outside their range   */
/* or do not hold together (entry tables; offsets that do not ascend from 0 to total; a record of a view  */
/* that is not kept, with a row outside 0..n-1, of another entry than its view's or not ascending inside  */
/* the view; a segment outside -1..q-1), [7] views of an entry whose position is outside 0..64 x words-1. */
/* All of them are forced into range or left out first: nothing is read or written outside the extents    */
/* whatever the kept arrays hold.                                                                         */
/* 1 <= n < 2^31, 1 <= nviews <= 65535 (per chunk in add, in all in finish), 1 <= q <= 1024, records in  */
/* all < 2^31 - 1.  No output may overlap an input or another output (GP_EINVAL).                         */
size_t gp_lift_masks_stream_state_bytes(int64_t n);
size_t gp_lift_masks_stream_begin_workspace_bytes(int64_t n);
int gp_lift_masks_stream_begin(const double *points, int64_t n, void *state, size_t state_bytes, int64_t *status,
                               void *workspace, size_t workspace_bytes, void *stream);
size_t gp_lift_masks_stream_sizes_workspace_bytes(int32_t nviews);
int gp_lift_masks_stream_sizes(int64_t n, const void *state, size_t state_bytes, const int64_t *status,
                               const int64_t *view_entry, const int64_t *view_count, const uint8_t *view_keep, int32_t nviews,
                               int64_t *sizes, void *workspace, size_t workspace_bytes, void *stream);
size_t gp_lift_masks_stream_add_workspace_bytes(int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w, int32_t out_h,
                                                int32_t out_w, int64_t total, int64_t fill_cap);
int gp_lift_masks_stream_add(const double *points, int64_t n, void *state, size_t state_bytes, const int64_t *view_entry,
                             int32_t nviews, const float *pred_masks, int32_t q, int32_t h, int32_t w, const float *scores,
                             const int32_t *tap_x0, const float *tap_wx, const int32_t *tap_y0, const float *tap_wy,
                             int32_t out_h, int32_t out_w, const int64_t *ent_pt, const int64_t *ent_x, const int64_t *ent_y,
                             const int32_t *ent_view, const int64_t *view_off, const uint8_t *keep, int64_t total,
                             int64_t fill_cap, int32_t *rec_row, int32_t *rec_seg, int64_t rec_base, int64_t rec_cap,
                             int64_t *rec_off, int32_t *view_pos, int64_t *status, void *workspace, size_t workspace_bytes,
                             void *stream);
/* gp_lift_masks_stream_add on pred_masks of element type `elem` (see gp_lift_masks_batched_t); the       */
/* records are the same whatever the type, so the chunks of one stream may differ in type.               */
size_t gp_lift_masks_stream_add_workspace_bytes_t(int32_t elem, int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w,
                                                  int32_t out_h, int32_t out_w, int64_t total, int64_t fill_cap);
int gp_lift_masks_stream_add_t(const double *points, int64_t n, void *state, size_t state_bytes, const int64_t *view_entry,
                               int32_t nviews, const void *pred_masks, int32_t elem, int32_t q, int32_t h, int32_t w,
                               const float *scores, const int32_t *tap_x0, const float *tap_wx, const int32_t *tap_y0,
                               const float *tap_wy, int32_t out_h, int32_t out_w, const int64_t *ent_pt, const int64_t *ent_x,
                               const int64_t *ent_y, const int32_t *ent_view, const int64_t *view_off, const uint8_t *keep,
                               int64_t total, int64_t fill_cap, int32_t *rec_row, int32_t *rec_seg, int64_t rec_base,
                               int64_t rec_cap, int64_t *rec_off, int32_t *view_pos, int64_t *status, void *workspace,
                               size_t workspace_bytes, void *stream);
size_t gp_lift_masks_stream_finish_workspace_bytes(int64_t n, int32_t nviews, int64_t total, int32_t words);
int gp_lift_masks_stream_finish(const double *points, int64_t n, const void *state, size_t state_bytes,
                                const int64_t *view_entry, const int32_t *view_pos, const uint8_t *view_keep,
                                const int64_t *rec_off, int32_t nviews, const int32_t *rec_row, const int32_t *rec_seg,
                                int64_t total, int32_t words, const float *f_seg, const float *logit_seg, int32_t q, int32_t d,
                                int32_t c, const int64_t *status, int32_t fill, float *out, int64_t ld_out, uint8_t *seen,
                                int32_t *count, int64_t *nn, int64_t *status_out, void *workspace, size_t workspace_bytes,
                                void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Rendered depth over BATCHED point clouds: the depth "render" mode of the ScanNet mapper,             */
/* models/utils/fusion_util.py:126-130 (compute_mapping(depth=<str>): the z-buffer of the cloud itself),  */
/* for every view of every batch entry in one sequence of launches; entries never mix.  It replaces, per  */
/* scene and per view, one gp_render_depth_f64 call on the entry's slice of the points (a launch and a    */
/* host-side matrix upload each), and gives the same bits.  Points, entries, views and poses are worded   */
/* as in gp_lift_batched: points f64 [n,4], view_entry i64 [nviews], w2c f64 [nviews,16], intrinsics f64  */
/* [nviews,4].                                                                                            */
/*   depth f64 [nviews,height,width] (8-byte aligned): 999999 everywhere, then per view the minimum        */
/*     camera-space z over the points OF THE VIEW'S ENTRY with z > 0.2 that project inside [cut_bound,     */
/*     width - cut_bound) x [cut_bound, height - cut_bound), pixels rounded half to even -- the depth      */
/*     argument of gp_lift_batched, gp_lift_stream_add and gp_lift_masks_batched_lists;                    */
/*   status i64 [8]: gp_render_depth_batched: [0] rows whose batch index is no integer in 0..65535, [1]    */
/*     views whose entry is outside 0..65535, [2] rows with a non-finite value, [3] the highest valid      */
/*     batch index; gp_render_depth_batched_state: [1] as above, [6] values of state that lay outside      */
/*     their range; the others 0.  Rows counted in [0] are never rendered, the image of a view counted in  */
/*     [1] stays 999999; nothing is read or written outside the extents whatever they hold.                */
/* The minimum is a 64-bit unsigned atomic on the fp64 bit pattern (positive doubles order like their      */
/* bits): it does not depend on arrival order, two calls give the same bits.                               */
/* gp_render_depth_batched sorts the rows by entry itself (the tables of gp_lift_batched, in its           */
/* workspace).  gp_render_depth_batched_state takes the tables from the state that gp_lift_stream_begin    */
/* or gp_lift_masks_stream_begin wrote for these points (state_bytes of at least                           */
/* gp_lift_stream_state_bytes(n); the mask stream's state begins with the same tables), forced into range  */
/* first as gp_lift_stream_finish does, and sorts nothing; it changes no byte of state.                    */
/* 1 <= n < 2^31, 1 <= nviews <= 65535, height, width >= 1, cut_bound >= 0.  No output may overlap an      */
/* input or another output (GP_EINVAL).                                                                    */
size_t gp_render_depth_batched_workspace_bytes(int64_t n, int32_t nviews);
int gp_render_depth_batched(const double *points, int64_t n, const int64_t *view_entry, const double *w2c,
                            const double *intrinsics, int32_t nviews, int32_t height, int32_t width, int32_t cut_bound,
                            double *depth, int64_t *status, void *workspace, size_t workspace_bytes, void *stream);
size_t gp_render_depth_batched_state_workspace_bytes(int64_t n, int32_t nviews);
int gp_render_depth_batched_state(const double *points, int64_t n, const void *state, size_t state_bytes,
                                  const int64_t *view_entry, const double *w2c, const double *intrinsics, int32_t nviews,
                                  int32_t height, int32_t width, int32_t cut_bound, double *depth, int64_t *status,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* The label vote over BATCHED point clouds: integer 2D label maps -- the loader's label_2ds, slot 11 of   */
/* its 20-tuple (dataset/data_loader_ablation.py:296-346) -- voted onto the points.  The reference has no   */
/* such function; every geometric decision is its own: the point -> pixel mapping of                       */
/* models/utils/fusion_util.py:99-147 and the view-drop rule of dataset/data_loader_ablation.py:254-288,   */
/* for every batch entry and every view in one sequence of launches; entries never mix.  Points, entries,  */
/* views, poses, depth, view_count, view_keep, count and seen are worded as in gp_lift_batched and hold    */
/* the same values on the same geometry.                                                                   */
/* labels2d [nviews, height, width] of element type `elem`: GP_LABEL_U8, GP_LABEL_I16, GP_LABEL_I32 or     */
/* GP_LABEL_I64 (any other tag is GP_EINVAL), aligned to its element, read in place and widened to 64 bits */
/* as it is loaded.  ignore_ids: n_ignore <= 16 values in HOST memory.                                      */
/*   votes i32 [n, ld_votes >= num_classes]: votes[p, c] = the kept views that see p and hold class c at    */
/*     the sampled pixel.  A sampled value in ignore_ids casts no vote; any other sampled value outside    */
/*     0..num_classes-1 casts none and is counted in status[7];                                            */
/*   voted i32 [n] = sum_c votes[p, c] (a seen point may have 0);                                          */
/*   labels i64 [n]: the lowest class with the most votes where voted > 0; with fill != 0, in an entry      */
/*     with voted and unvoted points, an unvoted point takes the label of the voted point OF ITS ENTRY     */
/*     that minimises (d^2, row) -- gp_lift_batched's fill with "seen" read as "voted", its votes row       */
/*     staying zero; `unlabeled` (outside 0..num_classes-1) everywhere else;                               */
/*   status i64 [8]: [0]..[3] as gp_lift_batched, [4] voted rows, [5] filled rows, [7] sampled labels out  */
/*     of range.                                                                                           */
/* Integer arithmetic throughout: exact, and independent of any order.  1 <= n < 2^31, 1 <= nviews <=      */
/* 65535, 1 <= num_classes <= 1024, cut_bound >= 0.  No output may overlap an input or another output      */
/* (GP_EINVAL).                                                                                            */
/* gp_lift_labels_batched: the mapper, fusion_util.py:99-147, and the loader's drop rule,                  */
/* data_loader_ablation.py:254-288, over the label_2ds of data_loader_ablation.py:296-346.                 */
#define GP_LABEL_U8 0
#define GP_LABEL_I16 1
#define GP_LABEL_I32 2
#define GP_LABEL_I64 3
size_t gp_lift_labels_batched_workspace_bytes(int64_t n, int32_t nviews);
int gp_lift_labels_batched(const double *points, int64_t n, const void *labels2d, int32_t elem, int32_t num_classes,
                           const int64_t *view_entry, const double *w2c, const double *intrinsics, const double *depth,
                           int32_t nviews, int32_t height, int32_t width, int32_t cut_bound, double vis_thres,
                           int64_t min_visible, int64_t max_visible, const int64_t *ignore_ids, int32_t n_ignore,
                           int64_t unlabeled, int32_t fill, int64_t *labels, int32_t *votes, int64_t ld_votes, int32_t *voted,
                           uint8_t *seen, int32_t *count, int64_t *view_count, uint8_t *view_keep, int64_t *status,
                           void *workspace, size_t workspace_bytes, void *stream);
/* The same vote RESUMABLE, the views in chunks (the loader hands label_2ds out per view,                  */
/* data_loader_ablation.py:296-346; the chunk loop is the one gp_lift_stream_* follows,                    */
/* models/affinity_module.py:365-449).  The caller owns, between the calls: state                          */
/* (gp_lift_labels_stream_state_bytes(n): the entry tables of gp_lift_stream_begin), votes i32 [n, ld_votes */
/* >= num_classes], count i32 [n] and the running status i64 [8].  The sums are integers, so votes, count  */
/* and what follows from them do not depend on the order of the chunks.                                    */
/* gp_lift_labels_stream_begin (before the chunk loop, models/affinity_module.py:365): the tables into     */
/*   state, votes = 0, count = 0, status [0], [2], [3] as gp_lift_stream_begin.                            */
/* gp_lift_labels_stream_add (one pass of the loop, models/affinity_module.py:365-436 with                  */
/*   fusion_util.py:99-147 and data_loader_ablation.py:254-288): view_count / view_keep of this chunk's     */
/*   views; votes and count of every point that a kept view of the chunk sees grow by the chunk's votes    */
/*   (other rows are neither read nor written); status[1] += bad view entries, status[7] += sampled labels */
/*   out of range.  Chunks may differ in elem.  No synchronisation, nothing sized by device data.          */
/* gp_lift_labels_stream_finish (the end, models/affinity_module.py:435-449): reads state, votes, count and */
/*   status and changes none: labels, voted, seen as gp_lift_labels_batched writes them; status_out        */
/*   [0]..[3] and [7] the running words, [4] voted rows, [5] filled rows, [6] values of state outside      */
/*   their range (forced into range before use, as gp_lift_stream_finish does).                            */
size_t gp_lift_labels_stream_state_bytes(int64_t n);
size_t gp_lift_labels_stream_begin_workspace_bytes(int64_t n);
int gp_lift_labels_stream_begin(const double *points, int64_t n, int32_t num_classes, void *state, size_t state_bytes,
                                int32_t *votes, int64_t ld_votes, int32_t *count, int64_t *status, void *workspace,
                                size_t workspace_bytes, void *stream);
size_t gp_lift_labels_stream_add_workspace_bytes(int32_t nviews);
int gp_lift_labels_stream_add(const double *points, int64_t n, const void *state, size_t state_bytes, const void *labels2d,
                              int32_t elem, int32_t num_classes, const int64_t *view_entry, const double *w2c,
                              const double *intrinsics, const double *depth, int32_t nviews, int32_t height, int32_t width,
                              int32_t cut_bound, double vis_thres, int64_t min_visible, int64_t max_visible,
                              const int64_t *ignore_ids, int32_t n_ignore, int32_t *votes, int64_t ld_votes, int32_t *count,
                              int64_t *view_count, uint8_t *view_keep, int64_t *status, void *workspace,
                              size_t workspace_bytes, void *stream);
size_t gp_lift_labels_stream_finish_workspace_bytes(int64_t n);
int gp_lift_labels_stream_finish(const double *points, int64_t n, const void *state, size_t state_bytes, const int32_t *votes,
                                 int32_t num_classes, int64_t ld_votes, const int32_t *count, const int64_t *status,
                                 int64_t unlabeled, int32_t fill, int64_t *labels, int32_t *voted, uint8_t *seen,
                                 int64_t *status_out, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Fused-feature files FROM lifted batched clouds, and back.  The reader is                           */
/* dataset/feature_loader.py:113-192 ({scene}_{k}.pt: feat, mask_full, and mask in the three-key      */
/* form); the writer's settings are config/fusion_scannet.yaml:34-35 (n_split_points,                 */
/* num_rand_file_per_scene).  points f64 [n,4]: only the batch column is read.  Per entry b (its rows  */
/* in ascending row order, local index i) and file k: chunk = all of the entry when n_split_points == 0 */
/* or n_b <= n_split_points, else the n_split_points points with the smallest key                      */
/*   h = fmix32(i ^ fmix32(k ^ fmix32(b ^ fmix32(seed_lo ^ fmix32(seed_hi))))),                         */
/* fmix32 murmur3's finaliser (a bijection: the keys of a pair are distinct, the chunk has no ties).   */
/* form 0 (merged, two keys): mask_full = chunk & seen; form 1 (chunk, three keys): mask_full = chunk, */
/* mask = seen at the file's rows.  feat: the rows of features where mask_full, file after file, in a   */
/* file entry after entry, in an entry by ascending row.                                                */
/* gp_fuse_plan (the settings, config/fusion_scannet.yaml:34-35): mask_full u8 [num_files, n]; state    */
/*   (gp_fuse_state_bytes) for gp_fuse_write; status i64 [8]: [0] rows whose batch index is no integer  */
/*   in 0..65535 (in no file), [3] top batch index, [4] rows of feat over all files.                    */
/* gp_fuse_write (what the reader loads, dataset/feature_loader.py:113-192): features fp32 or fp16      */
/*   [n, d] -> feat fp16 or fp32 [total_rows, d] (GP_ELEM_F32 / GP_ELEM_F16; fp32 -> fp16 rounds to     */
/*   nearest even, overflows to inf, keeps subnormals), mask u8 [total_rows] (form 1; NULL: not         */
/*   written), offsets i64 [num_files, num_entries + 1]: file (k, b) is feat[offsets[k][b] ..           */
/*   offsets[k][b+1]).  num_entries = status[3] + 1, total_rows = status[4] of the plan; a state the    */
/*   plan did not write moves no row outside [0, n) or [0, total_rows).                                 */
/* gp_fuse_dense (the reader's evaluation form, dataset/feature_loader.py:119-126, on unvoxelized       */
/*   points): out fp32 [n, d]: out[p] = mask_full[p] ? feat[rank(p)] : 0, rank(p) the position of p     */
/*   among the rows with mask_full in (entry, row) order; feat [feat_rows, d] the rows of ONE file set  */
/*   (all entries); status [0], [3] as above, [4] = rows with mask_full in a valid entry: the caller    */
/*   compares it with feat_rows (ranks beyond feat_rows read nothing and give zero rows).               */
/* 1 <= n < 2^31 - 1, 1 <= num_files <= 16, d >= 1.  No output may overlap an input or another output.  */
size_t gp_fuse_state_bytes(int64_t n, int32_t num_files);
size_t gp_fuse_workspace_bytes(int64_t n, int32_t num_files, int64_t n_split_points);
int gp_fuse_plan(const double *points, int64_t n, const uint8_t *seen, int32_t num_files, int64_t n_split_points,
                 uint64_t seed, int32_t form, uint8_t *mask_full, void *state, size_t state_bytes, int64_t *status,
                 void *workspace, size_t workspace_bytes, void *stream);
int gp_fuse_write(const void *features, int32_t elem_in, int64_t d, const uint8_t *seen, int64_t n, int32_t num_files,
                  const void *state, size_t state_bytes, int64_t num_entries, void *feat, int32_t elem_out,
                  int64_t total_rows, uint8_t *mask, int64_t *offsets, void *stream);
size_t gp_fuse_dense_workspace_bytes(int64_t n);
int gp_fuse_dense(const double *points, int64_t n, const uint8_t *mask_full, const void *feat, int32_t elem,
                  int64_t feat_rows, int64_t d, float *out, int64_t *status, void *workspace, size_t workspace_bytes,
                  void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Lifted BATCHED point clouds rendered back into their views: per view and pixel the row of the       */
/* front-most visible point of the view's entry (what models/utils/visualization.py:34-48 paints a    */
/* view with, where the last point in row order wins: here the nearest), decided with the mapping of   */
/* models/utils/fusion_util.py:99-147, and the gather that turns that index map into feature maps.     */
/* Points, entries, views, poses and cut_bound are worded as in gp_render_depth_batched.               */
/* depth_mode 0: no depth maps (a point is visible where it projects inside the cut bound with         */
/* p_z > 0), depth NULL; 1: depth f64 [nviews,height,width], the depth argument of gp_lift_batched;    */
/* 2: the maps gp_render_depth_batched makes from these points, rendered into the workspace, depth     */
/* NULL.  A point of view v's entry is a candidate of v when gp_lift_batched would count it in         */
/* view_count[v] (|depth - p_z| <= vis_thres * depth at its pixel, or p_z > 0 without maps) and        */
/* p_z > 0.  It covers the square of side 2 * radius + 1 (0 <= radius <= 4) centred on its pixel,      */
/* clipped to [cut_bound, height - cut_bound) x [cut_bound, width - cut_bound).  A pixel's owner is    */
/* the covering candidate with the smallest p_z (fp64), among equal p_z the lowest row.                */
/*   rows i32 [nviews,height,width]: the owner's row, -1 where nothing covers the pixel;               */
/*   zmin f64 [nviews,height,width] (8-byte aligned): the owner's p_z, 999999 where rows is -1;        */
/*   view_count i64 [nviews]: candidates per view (gp_lift_batched's view_count on the same            */
/*     geometry); pixel_count i64 [nviews]: pixels with an owner;                                      */
/*   status i64 [8]: [0]..[3] as gp_render_depth_batched.  Rows counted in [0] are never rendered,     */
/*     the images of a view counted in [1] stay -1 / 999999.                                           */
/* Two order-free passes (a 64-bit unsigned atomic minimum on the bit pattern of p_z, then a 32-bit    */
/* atomic minimum of the row where the pixel holds the candidate's own p_z): integer minima and sums   */
/* only, so two calls give the same bits in any row order.                                             */
/* gp_render_gather: out [npix, ld_out >= d] of element type elem_out (GP_ELEM_F32 / _F16 / _BF16):    */
/* out[p] = src[index ? index[rows[p]] : rows[p]] converted once (fp16 and bf16: nearest even, every    */
/* bf16 NaN 0x7FC0), a zero row where rows[p] < 0 -- or where rows[p] >= n_index or the source row is   */
/* outside 0..nrows-1, which are never accessed.  rows i32 [npix]; index i64 [n_index] or NULL with    */
/* n_index 0; src fp32 [nrows, ld_src >= d].  Rows whose bases and pitches are multiples of 4 elements */
/* move 16 bytes per load.  1 <= n < 2^31, 1 <= nviews <= 65535; npix, nrows, d >= 1.  No output may   */
/* overlap an input or another output (GP_EINVAL).                                                     */
size_t gp_render_rows_workspace_bytes(int64_t n, int32_t nviews, int32_t height, int32_t width, int32_t depth_mode);
int gp_render_rows(const double *points, int64_t n, const int64_t *view_entry, const double *w2c, const double *intrinsics,
                   int32_t nviews, int32_t height, int32_t width, int32_t cut_bound, int32_t depth_mode, const double *depth,
                   double vis_thres, int32_t radius, int32_t *rows, double *zmin, int64_t *view_count, int64_t *pixel_count,
                   int64_t *status, void *workspace, size_t workspace_bytes, void *stream);
int gp_render_gather(const int32_t *rows, int64_t npix, const int64_t *index, int64_t n_index, const float *src,
                     int64_t nrows, int64_t d, int64_t ld_src, void *out, int32_t elem_out, int64_t ld_out, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* The geometry channels of BATCHED point clouds: vertex normals from meshes, and from neighbour lists */
/* where a cloud has no faces (the student's six geometry columns are colours and vertex normals,      */
/* dataset/data_loader_ablation.py:162-163; the reference takes the normals from the scan's mesh,      */
/* models/utils/dataset_utils.py:198-199 -> vertex_normal, models/utils/mapping_util.py:9-29).         */
/* gp_mesh_normals_batched: mapping_util.py:9-29 for the meshes of several entries at once, bit for    */
/*   bit.  points [n,4] = batch, x, y, z and normals [n,3], both fp32 (fp64 = 0) or both fp64 (1);     */
/*   faces i64 [nfaces,3] of rows of points, in any order, the faces of different entries interleaved  */
/*   at will.  All arithmetic in the points' type, each operation rounded once: vec = cross(p1 - p0,   */
/*   p2 - p0) with each product rounded before the difference (:10-12); length = sqrt((vec0^2 + vec1^2)*/
/*   + vec2^2) + 1e-8 (:13); the contribution (vec / length) * (length * 0.5) (:14-15, :21); a vertex  */
/*   sums the contributions of its faces in ascending face index from 0, a face that names it twice    */
/*   counted once (:23-25, numpy's buffered +=); normal = sum / (sqrt((s0^2 + s1^2) + s2^2) + 1e-8)    */
/*   (:27-28), so a vertex of no face gets a zero row.  The order comes from a stable sort of (vertex, */
/*   face) pairs, never from float atomics: two calls give the same bits.  A face with an index        */
/*   outside 0..n-1 (never dereferenced) or whose three rows are not in one valid entry contributes    */
/*   nothing.  status i64 [8]: [0] rows whose batch index is no integer in 0..65535, [2] rows with a   */
/*   non-finite value, [3] top batch index, [6] faces with an index outside 0..n-1, [7] faces whose    */
/*   rows are not of one entry.  1 <= n < 2^31, 1 <= nfaces <= (2^31 - 1) / 3.                         */
/* gp_knn_normals: for row i, in fp64, over the set i followed by its k listed rows in list order:     */
/*   m = (sum p) / (k + 1), C = sum (p - m)(p - m)^T, l0 <= l1 <= l2 the eigenvalues of C (cyclic      */
/*   Jacobi); normals[i] = the unit eigenvector of l0 -- what stands in for mapping_util.py:19-29      */
/*   where there are no faces --, variation[i] = l0 / (l0 + l1 + l2) (0 where the sum is 0), both      */
/*   rounded to fp32 last.  Every row gets a finite unit vector, also where l0 = l1 or the set is      */
/*   collinear (the direction is then unspecified).  Sign: with toward f64 [m,3] and toward_rows i64   */
/*   [n] the vector is flipped where <n, toward[toward_rows[i]] - p_i> < 0; with toward NULL (m = 0,   */
/*   toward_rows NULL) its component of largest magnitude is made positive, the lowest axis among      */
/*   equal magnitudes.  positions [n, ld_positions >= 3] fp32 (fp64 = 0) or fp64 (1), columns 0..2     */
/*   read in place; neighbors [n,k] i32 (index64 = 0) or i64 (1), 3 <= k <= 127; normals f32 [n,3],    */
/*   variation f32 [n]; status i64 [2]: [0] rows with a list index outside 0..n-1, [1] rows with a     */
/*   toward_rows outside 0..m-1 -- such rows are returned as zeros and the index is never              */
/*   dereferenced.  No workspace.  No output may overlap an input or another output (GP_EINVAL).      */
size_t gp_mesh_normals_batched_workspace_bytes(int64_t n, int64_t nfaces, int32_t fp64);
int gp_mesh_normals_batched(const void *points, int32_t fp64, int64_t n, const int64_t *faces, int64_t nfaces, void *normals,
                            int64_t *status, void *workspace, size_t workspace_bytes, void *stream);
int gp_knn_normals(const void *positions, int32_t fp64, int64_t ld_positions, int64_t n, const void *neighbors, int32_t index64,
                   int32_t k, const double *toward, int64_t m, const int64_t *toward_rows, float *normals, float *variation,
                   int64_t *status, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Results carried from one BATCHED cloud to another: the k nearest points of cloud A for every point  */
/* of cloud B, per batch entry, exactly, and rows interpolated through such lists.  The role of the    */
/* reference's KDTree queries (models/affinity_module.py:445-447, 693-697: the nearest seen point of   */
/* every unseen one), generalised to k neighbours, to a second cloud and to several entries at once.   */
/* gp_knn_query: points f64 [n,4] and queries f64 [m,4] = batch, x, y, z in any row order, duplicates  */
/*   allowed.  xyz rounded to fp32 first; d^2 = (dx*dx + dy*dy) + dz*dz in fp64, each operation        */
/*   rounded once; row j of a query lists the points of the query's own entry in ascending (d^2, row): */
/*   indices i64 [m,k] (rows of points), dist2 f64 [m,k] (those d^2).  A coinciding point is an        */
/*   ordinary neighbour at distance 0.  Slots past the entry's count hold -1 / +inf.  Per entry a      */
/*   uniform grid of ng^3 <= max(count, 1) cubic cells over its fp32 bounding box; one wave per query  */
/*   walks the shells of Chebyshev radius 0..3 around the query's (clamped) cell and stops after shell */
/*   r once it holds k points with d^2_k <= (r h (1 - 1e-9))^2, or the shells cover the grid; the      */
/*   queries left over scan their whole entry, one workgroup each.  1 <= k <= GP_KNN_QUERY_MAX_K.      */
/*   status i64 [16]: [0] rows of points whose batch index is no integer in 0..65535, [2] rows of      */
/*   points with a value that is not finite (in fp64, or xyz in fp32), [3] top batch index of the      */
/*   points; [8], [10]: the same two counts for the queries (such a query gets -1 / +inf);             */
/*   [9] queries whose entry has no points; [11] queries that took the entry scan; [12 + r] queries    */
/*   that stopped after shell r = 0..3.  1 <= n, m < 2^31.  No read-back inside.                        */
/* gp_knn_interpolate: out f32 [m,d], contiguous.  values [nrows, ld_values >= d] of element type elem */
/*   (GP_ELEM_F32 / _F16 / _BF16), read in place; index i64 [n_index] (point -> row of values) or NULL */
/*   with n_index 0; npoints = the range of the list entries (n_index with an index, nrows without).   */
/*   mode 0 (inverse distance): over the slots with indices != -1, w_j = 1 / (d^2_j + eps) in fp64,    */
/*   normalised in fp64, rounded to fp32; where some d^2_j + eps is 0, those slots share the weight    */
/*   equally and the others get 0.  mode 1 (nearest): slot 0 with weight 1.  out = sum_j w_j v_j in    */
/*   fp32 in list order, each product and each sum rounded once.  A row without a valid slot is zero.  */
/*   A list entry outside -1..npoints-1 or an index value outside 0..nrows-1 (of the slots the mode    */
/*   reads) is never dereferenced: the row is zero and counted in status i64 [2]: [0] rows with such a */
/*   list entry, [1] rows with such an index value.                                                     */
/* gp_knn_interpolate_labels: out i64 [m] = values[index ? index[indices[q,0]] : indices[q,0]], or     */
/*   `unlabeled` where slot 0 is -1 or out of range (counted as above).  values i64 [nrows].           */
/* No output may overlap an input or another output (GP_EINVAL).                                       */
#define GP_KNN_QUERY_MAX_K 32
size_t gp_knn_query_workspace_bytes(int64_t n, int64_t m);
int gp_knn_query(const double *points, int64_t n, const double *queries, int64_t m, int32_t k, int64_t *indices, double *dist2,
                 int64_t *status, void *workspace, size_t workspace_bytes, void *stream);
int gp_knn_interpolate(const void *values, int32_t elem, int64_t nrows, int64_t d, int64_t ld_values, const int64_t *index,
                       int64_t n_index, const int64_t *indices, const double *dist2, int64_t m, int32_t k, int64_t npoints,
                       int32_t mode, double eps, float *out, int64_t *status, void *stream);
int gp_knn_interpolate_labels(const int64_t *values, int64_t nrows, const int64_t *index, int64_t n_index, const int64_t *indices,
                              int64_t m, int32_t k, int64_t npoints, int64_t unlabeled, int64_t *out, int64_t *status, void *stream);

/* ---- the backward of gp_knn_interpolate (knn_interpolate_grad.hip) ---------------------------------- */
/* d_values [nrows,d] from g = d_out f32 [m,d]: the role of the autograd the reference gets from torch  */
/* indexing where it carries features through KDTree lists (models/affinity_module.py:445-452,         */
/* 693-714), for k neighbours, weights and an index, exactly and reproducibly: no float atomics.        */
/* A reference is a flat slot f = j*k + s whose forward weight is in effect: s is a slot the mode reads */
/*   (all k; slot 0 for mode 1), its list entry is in 0..npoints-1, its row r = index[entry] (or the    */
/*   entry) in 0..nrows-1, and no slot of query row j that the mode reads holds a list entry outside    */
/*   -1..npoints-1 or an index value outside 0..nrows-1 (such a query row is the forward's zero row).   */
/*   d_values[r,c] starts at +0 and takes, over the references of r in ascending f, acc = acc +         */
/*   w32[f] * g[j,c], the product and the sum each rounded once in fp32; one rounding to the element    */
/*   type at the end; a row without references is written as zeros.                                     */
/* gp_knn_interpolate_weights: weights f32 [m,k] = the forward's own fp32 weight of every reference     */
/*   (the same device code), 0 where the slot is none.  Arguments as gp_knn_interpolate.                */
/* gp_knn_interpolate_transpose: offsets i64 [nrows+1], slots i32 [m*k], sorted_weights f32 [m*k]: the  */
/*   references of row r are slots[offsets[r] .. offsets[r+1]) in ascending f with their weights beside  */
/*   them; offsets[nrows] = the number of references, the slots past it are the flat slots that are     */
/*   none (weight 0).  A stable radix sort of (row, f) pairs over the bits of 0..nrows; weights: what   */
/*   gp_knn_interpolate_weights wrote for the same lists, index, mode and eps.  The result depends on   */
/*   those alone: build it once for a training run.  m * k <= 2^31-1, nrows < 2^31.                     */
/* gp_knn_interpolate_backward: out [nrows,d] of element type out_elem, contiguous; g [m, ld_g >= d].   */
/*   One wave per row of out; offsets and slots are clamped where they are read, so a damaged transpose */
/*   gives wrong numbers and no access outside g.  No output may overlap an input or another output.    */
int gp_knn_interpolate_weights(const int64_t *indices, const double *dist2, const int64_t *index, int64_t n_index, int64_t m, int32_t k,
                               int64_t npoints, int64_t nrows, int32_t mode, double eps, float *weights, void *stream);
size_t gp_knn_interpolate_transpose_workspace_bytes(int64_t m, int32_t k, int64_t nrows);
int gp_knn_interpolate_transpose(const int64_t *indices, const int64_t *index, int64_t n_index, int64_t m, int32_t k, int64_t npoints,
                                 int64_t nrows, int32_t mode, const float *weights, int64_t *offsets, int32_t *slots, float *sorted_weights,
                                 void *workspace, size_t workspace_bytes, void *stream);
int gp_knn_interpolate_backward(const float *g, int64_t ld_g, int64_t m, int64_t d, const int64_t *offsets, const int32_t *slots,
                                const float *sorted_weights, int32_t k, int64_t nrows, void *out, int32_t out_elem, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GEOPURIFY_HIP_H */
