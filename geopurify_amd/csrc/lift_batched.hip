// The 2D -> 3D lift over BATCHED point clouds (geopurify_amd/sparse.py: lift): for every batch entry b, with its points the rows of
// batch b in ascending row order and its views the views with view_entry == b in ascending view index,
//     n_v      = #points of the view's entry that project_point sees in view v                    (view_count)
//     keep_v   = n_v != 0 && n_v >= min_visible && n_v <= max_visible                             (view_keep)
//     sum_p    = fp32 sum over the kept views that see p, in ascending v, of the sampled feature column
//     out_p    = sum_p / (cnt_p == 0 ? 1e-6 : cnt_p),  seen_p = cnt_p > 0                         (features, seen, count)
//     nn_p     = for an unseen p of an entry with seen points: the seen point of ITS entry that minimises (d^2, row), else -1
// -- models/affinity_module.py:404-452 with fusion_util.py:45-147 and data_loader_ablation.py:254-288, for all entries and all views
// in one sequence of launches.  The per-scene path (gp_views_visible_lists, one gp_lift_dense_accum launch per view that
// read-modify-writes [N,D] sums, gp_lift_dense_finish, gp_nn1_masked_f64) computes the same bits one scene at a time.
//
// Structure: (1) rows and views sorted stably by entry (rocPRIM radix sort on 17-bit keys; a bad index sorts behind every entry) and
// the two offset tables by binary search, one thread per entry; (2) the per-view counts: every (view, point of its entry) pair is
// projected, counted per lane, reduced over the wave, one integer atomic per wave and view; (3) the fused lift: one wave per point,
// lane l projects the point through the l-th view of a group of 64 of its entry, a 64-bit ballot is the visible-and-kept mask, its
// set bits are walked in ascending view order with all lanes striding the channels and accumulating in registers; the row is divided
// and stored once.  No float atomics and no read-modify-write of the sums: the fp32 add order is the sequential index_add_'s.  The
// maps are read PIXEL-MAJOR ([V, h*w, D]: one contiguous row of 4 D bytes per sample -- or of 2 D bytes: the maps may be fp16 or bf16
// (gp_map_elem.h, the *_t entry points), every loaded element is converted to fp32, which is exact, and then takes the same adds and
// fmas in the same order, so half maps give the bits of their fp32 copy; aligned half rows are read 8 or 16 bytes per lane); (4) the
// fill: references (seen rows) and
// queries (unseen rows of entries that have seen ones) compacted in the entry-sorted order, so an entry's references are one
// contiguous run; a block of 256 queries streams the runs of its queries' entries through LDS tiles, each query comparing only inside
// its own run.
//
// Bounds: a batch or view entry index is range-checked before every table access (0..65535; the tables hold 65538 words); sorted
// positions come from the offset tables (inside 0..n / 0..nviews by construction of the lower bounds); a pixel is read only after
// project_point found it inside [cut, W-cut) x [cut, H-cut) with cut >= 0; bilinear taps are clamped to the map; channel indices are
// guarded by c < d.  All offsets are 64-bit.
// (The entry tables, the per-view counts with the drop rule and the fill kernels live in gp_lift_entries.h: lift_masks_batched.hip runs
// them too.)
#include "gp_lift_entries.h"
#include "gp_map_elem.h"

namespace {

constexpr int LB_COLS_PER_LANE = 8;
constexpr int LB_COL_CHUNK = GP_WAVE * LB_COLS_PER_LANE;         // channels one pass of the lift kernel holds in registers


// ------------------------------------------------------------------------------------------------ [V, D, hw] -> [V, hw, D]
// (T: float, or uint16_t for both half types -- the elements are moved, never read as numbers)
template <typename T>
__global__ void __launch_bounds__(256) lb_transpose_kernel(const T *__restrict__ src, int rows, int64_t cols, T *__restrict__ dst) {
    __shared__ T tile[64][65];
    const int64_t vo = (int64_t)blockIdx.z * rows * cols;
    const int64_t bx = (int64_t)blockIdx.x * 64;
    const int by = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int row = by + r;
        const int64_t col = bx + tx;
        tile[r][tx] = (row < rows && col < cols) ? src[vo + (int64_t)row * cols + col] : T(0);
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int64_t orow = bx + r;
        const int ocol = by + tx;
        if (orow < cols && ocol < rows) dst[vo + orow * rows + ocol] = tile[tx][r];
    }
}

// ------------------------------------------------------------------------------------------------ the fused lift
// One wave per point.  BILINEAR: the map is [h, w] and the pixel indexes the [H, W] image the reference resizes the map to
// (F.interpolate(bilinear, align_corners=True)); the resize is evaluated at the sampled pixel with the arithmetic of
// lift_dense_bilinear_accum_kernel.  Otherwise (h, w) == (H, W) and the pixel's row is added as it is.
// T: the maps' element type (gp_map_elem.h), converted to fp32 as it is loaded.  VEC: the consecutive columns a lane takes with one
// load.  VEC = 1 is the mapping the kernel was written with (accumulator k of lane l holds column c0 + l + 64 k); with VEC = 4 or 8
// (half maps whose rows are aligned to 8 / 16 bytes) accumulator k holds column c0 + (64 (k / VEC) + l) VEC + k % VEC, one 8- or
// 16-byte load per lane and tap instead of VEC 2-byte ones.  A column is summed by one lane in view order under either mapping: the
// same bits.  The vector forms store their rows as float4 where out and ld_out allow it (a wave-uniform test).
template <typename T, int VEC, bool BILINEAR>
__global__ void __launch_bounds__(256) lb_lift_kernel(const double *__restrict__ points, int64_t n, const T *__restrict__ feat, int d, int h,
                                                      int w, float scale_h, float scale_w, const int32_t *__restrict__ entry_views,
                                                      const int32_t *__restrict__ view_off, const double *__restrict__ w2c,
                                                      const double *__restrict__ intr, const double *__restrict__ depth, int W, int H, int cut,
                                                      double tau, const uint8_t *__restrict__ keep, float *__restrict__ out, int64_t ld_out,
                                                      uint8_t *__restrict__ seen, int32_t *__restrict__ count, int64_t *__restrict__ nn) {
    const int64_t p = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;     // (the same for the whole wave: every exit is wave-uniform)
    if (p >= n) return;
    const int lane = gp_lane();
    const double *P = points + p * 4;
    const double x = P[1], y = P[2], z = P[3];
    const int b = lb_entry_of(P[0]);
    int v0 = 0, v1 = 0;
    if (b >= 0) { v0 = view_off[b]; v1 = view_off[b + 1]; }
    const int64_t map = (int64_t)h * w * d;
    float *orow = out + p * ld_out;
    int cnt = 0;
    for (int c0 = 0; c0 < d; c0 += LB_COL_CHUNK) {
        float acc[LB_COLS_PER_LANE];
#pragma unroll
        for (int k = 0; k < LB_COLS_PER_LANE; ++k) acc[k] = 0.f;
        int seen_by = 0;
        for (int g = v0; g < v1; g += GP_WAVE) {
            int v = 0, px = 0, py = 0;
            bool vis = false;
            if (g + lane < v1) {
                v = entry_views[g + lane];
                if (keep[v]) {
                    const double *M = w2c + (int64_t)v * 16, *K = intr + (int64_t)v * 4;
                    long long ui, vi;
                    vis = project_point(x, y, z, M, M + 4, M + 8, K[0], K[1], K[2], K[3], depth ? depth + (int64_t)v * W * H : nullptr, W, H,
                                        cut, tau, ui, vi);
                    px = (int)ui;
                    py = (int)vi;
                }
            }
            unsigned long long m = __ballot(vis);
            seen_by += __popcll(m);
            while (m) {                                              // ascending view index: the entry's views are sorted stably
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int vj = __shfl(v, j, 64), col = __shfl(px, j, 64), row = __shfl(py, j, 64);
                const T *f = feat + (int64_t)vj * map;
                if (BILINEAR) {
                    int r0, r1, q0, q1;
                    float wr0, wr1, wc0, wc1;
                    bilinear_tap(scale_h, row, h, r0, r1, wr0, wr1);
                    bilinear_tap(scale_w, col, w, q0, q1, wc0, wc1);
                    const T *f00 = f + ((int64_t)r0 * w + q0) * d, *f01 = f + ((int64_t)r0 * w + q1) * d;
                    const T *f10 = f + ((int64_t)r1 * w + q0) * d, *f11 = f + ((int64_t)r1 * w + q1) * d;
                    if constexpr (VEC == 1) {
#pragma unroll
                        for (int k = 0; k < LB_COLS_PER_LANE; ++k) {
                            const int c = c0 + lane + k * GP_WAVE;
                            if (c < d) {
                                const float top = __builtin_fmaf(wc0, gp_to_f32(f00[c]), wc1 * gp_to_f32(f01[c]));
                                const float bot = __builtin_fmaf(wc0, gp_to_f32(f10[c]), wc1 * gp_to_f32(f11[c]));
                                acc[k] += __builtin_fmaf(wr0, top, wr1 * bot);
                            }
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < LB_COLS_PER_LANE / VEC; ++j) {
                            const int c = c0 + (j * GP_WAVE + lane) * VEC;   // (d is a multiple of VEC: the group is inside or outside)
                            if (c < d) {
                                float a00[VEC], a01[VEC], a10[VEC], a11[VEC];
                                gp_load_f32<VEC>(f00 + c, a00);
                                gp_load_f32<VEC>(f01 + c, a01);
                                gp_load_f32<VEC>(f10 + c, a10);
                                gp_load_f32<VEC>(f11 + c, a11);
#pragma unroll
                                for (int i = 0; i < VEC; ++i) {
                                    const float top = __builtin_fmaf(wc0, a00[i], wc1 * a01[i]);
                                    const float bot = __builtin_fmaf(wc0, a10[i], wc1 * a11[i]);
                                    acc[j * VEC + i] += __builtin_fmaf(wr0, top, wr1 * bot);
                                }
                            }
                        }
                    }
                } else {
                    const T *fr = f + ((int64_t)row * w + col) * d;
                    if constexpr (VEC == 1) {
#pragma unroll
                        for (int k = 0; k < LB_COLS_PER_LANE; ++k) {
                            const int c = c0 + lane + k * GP_WAVE;
                            if (c < d) acc[k] += gp_to_f32(fr[c]);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < LB_COLS_PER_LANE / VEC; ++j) {
                            const int c = c0 + (j * GP_WAVE + lane) * VEC;
                            if (c < d) {
                                float a[VEC];
                                gp_load_f32<VEC>(fr + c, a);
#pragma unroll
                                for (int i = 0; i < VEC; ++i) acc[j * VEC + i] += a[i];
                            }
                        }
                    }
                }
            }
        }
        cnt = seen_by;                                               // (every column chunk sees the same views)
        const float den = cnt == 0 ? 1e-6f : (float)cnt;
        if constexpr (VEC == 1) {
#pragma unroll
            for (int k = 0; k < LB_COLS_PER_LANE; ++k) {
                const int c = c0 + lane + k * GP_WAVE;
                if (c < d) orow[c] = acc[k] / den;
            }
        } else {
            const bool wide = (((uintptr_t)out | (uintptr_t)(ld_out * 4)) & 15) == 0;   // (wave-uniform) c is a multiple of 4
#pragma unroll
            for (int j = 0; j < LB_COLS_PER_LANE / VEC; ++j) {
                const int c = c0 + (j * GP_WAVE + lane) * VEC;
                if (c < d) {
#pragma unroll
                    for (int i = 0; i < VEC; i += 4) {
                        const float4 q = make_float4(acc[j * VEC + i] / den, acc[j * VEC + i + 1] / den, acc[j * VEC + i + 2] / den,
                                                     acc[j * VEC + i + 3] / den);
                        if (wide) {
                            *reinterpret_cast<float4 *>(orow + c + i) = q;
                        } else {
                            orow[c + i] = q.x; orow[c + i + 1] = q.y; orow[c + i + 2] = q.z; orow[c + i + 3] = q.w;
                        }
                    }
                }
            }
        }
    }
    if (lane == 0) {
        seen[p] = cnt > 0 ? 1 : 0;
        count[p] = cnt;
        if (nn) nn[p] = -1;
    }
}


struct LbWork {
    uint32_t *k0, *k1, *vk0, *vk1;
    int32_t *r0, *entry_rows, *w0, *entry_views, *entry_off, *view_off, *ref, *qry, *rs, *qs, *rrow, *qpos;
    float *rxyz;
    char *tmp;
    size_t tmp_bytes;
    LbWork(GpCarver &cv, int64_t n, int32_t nviews) {
        const size_t a = lb_sort_bytes(n), b = lb_sort_bytes(nviews), c = lb_scan_bytes(n + 1);
        tmp_bytes = a > b ? (a > c ? a : c) : (b > c ? b : c);
        k0 = cv.take<uint32_t>(n);
        k1 = cv.take<uint32_t>(n);
        r0 = cv.take<int32_t>(n);
        entry_rows = cv.take<int32_t>(n);
        vk0 = cv.take<uint32_t>(nviews);
        vk1 = cv.take<uint32_t>(nviews);
        w0 = cv.take<int32_t>(nviews);
        entry_views = cv.take<int32_t>(nviews);
        entry_off = cv.take<int32_t>(LB_TABLE);
        view_off = cv.take<int32_t>(LB_TABLE);
        ref = cv.take<int32_t>(n + 1);
        qry = cv.take<int32_t>(n + 1);
        rs = cv.take<int32_t>(n + 1);
        qs = cv.take<int32_t>(n + 1);
        rrow = cv.take<int32_t>(n);
        qpos = cv.take<int32_t>(n);
        rxyz = cv.take<float>(3 * n);
        tmp = cv.take<char>(tmp_bytes);
    }
};

}  // namespace

extern "C" int32_t gp_lift_batched_col_chunk(void) { return LB_COL_CHUNK; }

extern "C" int gp_lift_batched_transpose_t(const void *src, int32_t elem, int32_t nviews, int32_t d, int64_t hw, void *dst, void *stream_) {
    GP_CHECK_ARG(src && dst, "gp_lift_batched_transpose: null argument");
    GP_CHECK_ARG(gp_elem_ok(elem), "gp_lift_batched_transpose: element type %d (0 fp32, 1 fp16, 2 bf16)", elem);
    GP_CHECK_ARG(nviews >= 1 && nviews <= 65535 && d >= 1 && hw >= 1 && hw < (1ll << 31), "gp_lift_batched_transpose: %d views of %d x %lld",
                 nviews, d, (long long)hw);
    GP_CHECK_ARG((hw + 63) / 64 < (1ll << 31) && (d + 63) / 64 <= 65535, "gp_lift_batched_transpose: %d channels exceed the grid", d);
    {
        const size_t bytes = (size_t)nviews * (size_t)d * (size_t)hw * gp_elem_size(elem);
        GP_CHECK_ARG(!lb_overlap(dst, bytes, src, bytes), "gp_lift_batched_transpose: dst overlaps src");
    }
    const dim3 grid((unsigned)((hw + 63) / 64), (unsigned)((d + 63) / 64), (unsigned)nviews);
    if (elem == GP_ELEM_F32)
        lb_transpose_kernel<float><<<grid, 256, 0, gp_stream(stream_)>>>(static_cast<const float *>(src), d, hw, static_cast<float *>(dst));
    else
        lb_transpose_kernel<uint16_t><<<grid, 256, 0, gp_stream(stream_)>>>(static_cast<const uint16_t *>(src), d, hw, static_cast<uint16_t *>(dst));
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_lift_batched_transpose(const float *src, int32_t nviews, int32_t d, int64_t hw, float *dst, void *stream_) {
    return gp_lift_batched_transpose_t(src, GP_ELEM_F32, nviews, d, hw, dst, stream_);
}

extern "C" size_t gp_lift_batched_workspace_bytes(int64_t n, int32_t nviews) {
    if (n <= 0 || n >= (1ll << 31) || nviews < 1 || nviews > 65535) return 0;
    GpCarver cv(nullptr, 0);
    LbWork k(cv, n, nviews);
    return cv.off;
}

extern "C" int gp_lift_batched_t(const double *points, int64_t n, const void *feat, int32_t elem, int32_t d, int32_t h, int32_t w,
                                 const int64_t *view_entry, const double *w2c, const double *intrinsics, const double *depth, int32_t nviews,
                                 int32_t height, int32_t width, int32_t bilinear, int32_t cut_bound, double vis_thres, int64_t min_visible,
                                 int64_t max_visible, int32_t fill, float *out, int64_t ld_out, uint8_t *seen, int32_t *count, int64_t *view_count,
                                 uint8_t *view_keep, int64_t *nn, int64_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    GP_CHECK_ARG(points && feat && view_entry && w2c && intrinsics && out && seen && count && view_count && view_keep && status && workspace,
                 "gp_lift_batched: null argument");
    GP_CHECK_ARG(gp_elem_ok(elem), "gp_lift_batched: element type %d (0 fp32, 1 fp16, 2 bf16)", elem);
    GP_CHECK_ARG(elem == GP_ELEM_F32 || (uintptr_t)feat % 2 == 0, "gp_lift_batched: half maps at an odd address");
    GP_CHECK_ARG(n > 0 && n < (1ll << 31), "gp_lift_batched: n=%lld outside 1..2^31-1", (long long)n);
    GP_CHECK_ARG(nviews >= 1 && nviews <= 65535, "gp_lift_batched: %d views outside 1..65535", nviews);
    GP_CHECK_ARG(d >= 1 && h >= 1 && w >= 1 && height >= 1 && width >= 1 && ld_out >= d, "gp_lift_batched: d=%d, map %d x %d, image %d x %d, ld_out=%lld",
                 d, h, w, height, width, (long long)ld_out);
    GP_CHECK_ARG(bilinear == 0 || bilinear == 1, "gp_lift_batched: bilinear=%d (0 nearest, 1 bilinear)", bilinear);
    GP_CHECK_ARG(bilinear || (h == height && w == width), "gp_lift_batched: the nearest mode samples the map itself: map %d x %d, image %d x %d", h, w,
                 height, width);
    GP_CHECK_ARG(cut_bound >= 0, "gp_lift_batched: cut_bound=%d must not be negative", cut_bound);
    GP_CHECK_ARG(fill == 0 || nn, "gp_lift_batched: the fill writes nn");
    {
        // every output against every input and every other output, over their whole extents
        const size_t px = (size_t)height * width, maps = (size_t)nviews * h * w * d * gp_elem_size(elem);
        const void *in[] = {points, feat, view_entry, w2c, intrinsics, depth};
        const size_t in_bytes[] = {(size_t)n * 32, maps, (size_t)nviews * 8, (size_t)nviews * 128, (size_t)nviews * 32, (size_t)nviews * px * 8};
        const void *o[] = {out, seen, count, view_count, view_keep, nn, status, workspace};
        const size_t o_bytes[] = {(size_t)((n - 1) * ld_out + d) * 4, (size_t)n, (size_t)n * 4, (size_t)nviews * 8, (size_t)nviews, (size_t)n * 8,
                                  (size_t)ST_WORDS * 8, workspace_bytes};
        for (int a = 0; a < 8; ++a) {
            for (int i = 0; i < 6; ++i)
                GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], in[i], in_bytes[i]), "gp_lift_batched: an output overlaps an input");
            for (int q = a + 1; q < 8; ++q) GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], o[q], o_bytes[q]), "gp_lift_batched: two outputs overlap");
        }
    }
    GpCarver cv(workspace, workspace_bytes);
    LbWork k(cv, n, nviews);
    if (!cv.ok()) {
        gp_set_error("gp_lift_batched: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    unsigned long long *vc = reinterpret_cast<unsigned long long *>(view_count);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    GP_CHECK_HIP(hipMemsetAsync(view_count, 0, (size_t)nviews * sizeof(int64_t), s));
    const unsigned nb = (unsigned)((n + 255) / 256), vb = (unsigned)((nviews + 255) / 256);
    // (1) entry tables
    lb_row_keys_kernel<<<nb, 256, 0, s>>>(points, n, k.k0, k.r0, st);
    lb_view_keys_kernel<<<vb, 256, 0, s>>>(view_entry, nviews, k.vk0, k.w0, st);
    GP_CHECK_LAUNCH();
    size_t io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(k.tmp, io, k.k0, k.k1, k.r0, k.entry_rows, (size_t)n, 0, LB_KEY_BITS, s));          // (stable)
    io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(k.tmp, io, k.vk0, k.vk1, k.w0, k.entry_views, (size_t)nviews, 0, LB_KEY_BITS, s));  // (stable)
    lb_offsets_kernel<<<(LB_TABLE + 255) / 256, 256, 0, s>>>(k.k1, n, k.entry_off);
    lb_offsets_kernel<<<(LB_TABLE + 255) / 256, 256, 0, s>>>(k.vk1, nviews, k.view_off);
    // (2) per-view counts and the drop rule
    lb_counts_kernel<<<dim3(nb < 64 ? nb : 64, (unsigned)nviews), 256, 0, s>>>(points, k.entry_rows, k.entry_off, view_entry, w2c, intrinsics, depth,
                                                                                width, height, cut_bound, vis_thres, vc);
    lb_keep_kernel<<<vb, 256, 0, s>>>(vc, nviews, min_visible, max_visible, view_keep);
    GP_CHECK_LAUNCH();
    // (3) the fused lift
    // area_pixel_compute_scale<float>(in, out, align_corners=true): (in-1)/(out-1) in fp32, 0 for a single output pixel
    const float sh = height > 1 ? (float)(h - 1) / (float)(height - 1) : 0.f;
    const float sw = width > 1 ? (float)(w - 1) / (float)(width - 1) : 0.f;
    const unsigned lb = (unsigned)((n * 64 + 255) / 256);
    const int vec = gp_elem_vec(feat, d, gp_elem_size(elem));    // (launch-uniform: every sampled row is aligned to the load it names)
#define LB_LIFT(T, VEC)                                                                                                                      \
    do {                                                                                                                                     \
        if (bilinear)                                                                                                                        \
            lb_lift_kernel<T, VEC, true><<<lb, 256, 0, s>>>(points, n, static_cast<const T *>(feat), d, h, w, sh, sw, k.entry_views, k.view_off,  \
                                                            w2c, intrinsics, depth, width, height, cut_bound, vis_thres, view_keep, out, ld_out, \
                                                            seen, count, nn);                                                                \
        else                                                                                                                                 \
            lb_lift_kernel<T, VEC, false><<<lb, 256, 0, s>>>(points, n, static_cast<const T *>(feat), d, h, w, sh, sw, k.entry_views, k.view_off, \
                                                             w2c, intrinsics, depth, width, height, cut_bound, vis_thres, view_keep, out,     \
                                                             ld_out, seen, count, nn);                                                       \
    } while (0)
    if (elem == GP_ELEM_F32) LB_LIFT(float, 1);
    else if (elem == GP_ELEM_F16 && vec == 8) LB_LIFT(gp_f16, 8);
    else if (elem == GP_ELEM_F16 && vec == 4) LB_LIFT(gp_f16, 4);
    else if (elem == GP_ELEM_F16) LB_LIFT(gp_f16, 1);
    else if (vec == 8) LB_LIFT(gp_bf16, 8);
    else if (vec == 4) LB_LIFT(gp_bf16, 4);
    else LB_LIFT(gp_bf16, 1);
#undef LB_LIFT
    GP_CHECK_LAUNCH();
    // (4) the fill
    const unsigned nb1 = (unsigned)((n + 1 + 255) / 256);
    lb_fill_flags_kernel<<<nb1, 256, 0, s>>>(k.k1, k.entry_rows, seen, n, k.ref, k.qry);
    GP_CHECK_LAUNCH();
    io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, io, k.ref, k.rs, (int32_t)0, (size_t)(n + 1), rocprim::plus<int32_t>(), s));
    io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, io, k.qry, k.qs, (int32_t)0, (size_t)(n + 1), rocprim::plus<int32_t>(), s));
    lb_fill_compact_kernel<<<nb, 256, 0, s>>>(points, k.entry_rows, k.ref, k.qry, k.rs, k.qs, n, k.rxyz, k.rrow, k.qpos, st);
    if (fill) lb_fill_kernel<<<nb, 256, 0, s>>>(points, k.k1, k.entry_rows, k.entry_off, k.rs, k.qs, n, k.rxyz, k.rrow, k.qpos, nn, st);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_lift_batched(const double *points, int64_t n, const float *feat, int32_t d, int32_t h, int32_t w, const int64_t *view_entry,
                               const double *w2c, const double *intrinsics, const double *depth, int32_t nviews, int32_t height, int32_t width,
                               int32_t bilinear, int32_t cut_bound, double vis_thres, int64_t min_visible, int64_t max_visible, int32_t fill,
                               float *out, int64_t ld_out, uint8_t *seen, int32_t *count, int64_t *view_count, uint8_t *view_keep, int64_t *nn,
                               int64_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    return gp_lift_batched_t(points, n, feat, GP_ELEM_F32, d, h, w, view_entry, w2c, intrinsics, depth, nviews, height, width, bilinear, cut_bound,
                             vis_thres, min_visible, max_visible, fill, out, ld_out, seen, count, view_count, view_keep, nn, status, workspace,
                             workspace_bytes, stream_);
}
