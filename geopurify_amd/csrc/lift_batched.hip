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
// (The entry tables, the per-view counts with the drop rule and the fill -- kernels, workspace structs and launch sequences -- live in
// gp_lift_entries.h, the sampling body of (3) in gp_lift_sample.h: the other members of the family run them too.)
#include "gp_lift_entries.h"
#include "gp_lift_sample.h"

namespace {

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
// One wave per point.  T, VEC, BILINEAR: the maps' element type, the consecutive columns a lane takes with one load (one 8- or 16-byte
// load per lane and tap instead of VEC 2-byte ones) and the sampling mode, as lb_add_sample and lb_col (gp_lift_sample.h) define them.
// A column is summed by one lane in view order under either column mapping: the same bits.  The vector forms store their rows as float4
// where out and ld_out allow it (a wave-uniform test).
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
                lb_add_sample<T, VEC, BILINEAR>(f, row, col, d, h, w, scale_h, scale_w, c0, lane, acc);
            }
        }
        cnt = seen_by;                                               // (every column chunk sees the same views)
        const float den = cnt == 0 ? 1e-6f : (float)cnt;
        if constexpr (VEC == 1) {
#pragma unroll
            for (int k = 0; k < LB_COLS_PER_LANE; ++k) {
                const int c = lb_col<1>(c0, lane, k);
                if (c < d) orow[c] = acc[k] / den;
            }
        } else {
            const bool wide = (((uintptr_t)out | (uintptr_t)(ld_out * 4)) & 15) == 0;   // (wave-uniform) c is a multiple of 4
#pragma unroll
            for (int j = 0; j < LB_COLS_PER_LANE / VEC; ++j) {
                const int c = lb_col<VEC>(c0, lane, j * VEC);
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
    LbTables t;
    LbFill f;
    char *tmp;
    size_t tmp_bytes;
    LbWork(GpCarver &cv, int64_t n, int32_t nviews) : t(cv, n, nviews), f(cv, n) {
        tmp_bytes = std::max({lb_sort_bytes(n), lb_sort_bytes(nviews), gp_scan_bytes<int32_t>(n + 1)});
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
    if (!lb_n_ok(n) || !lb_nviews_ok(nviews)) return 0;
    GpCarver cv(nullptr, 0);
    LbWork k(cv, n, nviews);
    return cv.off;
}

extern "C" int gp_lift_batched_t(const double *points, int64_t n, const void *feat, int32_t elem, int32_t d, int32_t h, int32_t w,
                                 const int64_t *view_entry, const double *w2c, const double *intrinsics, const double *depth, int32_t nviews,
                                 int32_t height, int32_t width, int32_t bilinear, int32_t cut_bound, double vis_thres, int64_t min_visible,
                                 int64_t max_visible, int32_t fill, float *out, int64_t ld_out, uint8_t *seen, int32_t *count, int64_t *view_count,
                                 uint8_t *view_keep, int64_t *nn, int64_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "gp_lift_batched";
    GP_CHECK_ARG(points && feat && view_entry && w2c && intrinsics && out && seen && count && view_count && view_keep && status && workspace,
                 "%s: null argument", who);
    LB_TRY(lb_check_elem(who, elem, feat, "maps"));
    LB_TRY(lb_check_n(who, n));
    LB_TRY(lb_check_nviews(who, nviews));
    GP_CHECK_ARG(d >= 1 && h >= 1 && w >= 1 && height >= 1 && width >= 1 && ld_out >= d, "%s: d=%d, map %d x %d, image %d x %d, ld_out=%lld", who, d, h,
                 w, height, width, (long long)ld_out);
    LB_TRY(lb_check_sampling(who, bilinear, h, w, height, width));
    LB_TRY(lb_check_cut(who, cut_bound));
    GP_CHECK_ARG(fill == 0 || nn, "%s: the fill writes nn", who);
    {
        const size_t px = (size_t)height * width, maps = (size_t)nviews * h * w * d * gp_elem_size(elem);
        const void *const in[] = {points, feat, view_entry, w2c, intrinsics, depth};
        const size_t in_bytes[] = {(size_t)n * 32, maps, (size_t)nviews * 8, (size_t)nviews * 128, (size_t)nviews * 32, (size_t)nviews * px * 8};
        const void *const o[] = {out, seen, count, view_count, view_keep, nn, status, workspace};
        const size_t o_bytes[] = {(size_t)((n - 1) * ld_out + d) * 4, (size_t)n, (size_t)n * 4, (size_t)nviews * 8, (size_t)nviews, (size_t)n * 8,
                                  (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver cv(workspace, workspace_bytes);
    LbWork k(cv, n, nviews);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    // (1) entry tables, (2) per-view counts and the drop rule
    LB_TRY(lb_entry_tables(points, n, view_entry, nviews, k.t, k.tmp, k.tmp_bytes, st, s));
    LB_TRY(lb_view_counts(points, n, k.t.rows.idx, k.t.rows.off, view_entry, w2c, intrinsics, depth, nviews, width, height, cut_bound,
                          vis_thres, min_visible, max_visible, view_count, view_keep, s));
    // (3) the fused lift
    // area_pixel_compute_scale<float>(in, out, align_corners=true): (in-1)/(out-1) in fp32, 0 for a single output pixel
    const float sh = height > 1 ? (float)(h - 1) / (float)(height - 1) : 0.f;
    const float sw = width > 1 ? (float)(w - 1) / (float)(width - 1) : 0.f;
    const unsigned lb = (unsigned)((n * 64 + 255) / 256);
    lb_sample_dispatch(feat, elem, d, bilinear, [&](auto form) {
        using F = decltype(form);
        using T = typename F::type;
        lb_lift_kernel<T, F::vec, F::bilinear><<<lb, 256, 0, s>>>(points, n, static_cast<const T *>(feat), d, h, w, sh, sw, k.t.views.idx,
                                                                  k.t.views.off, w2c, intrinsics, depth, width, height, cut_bound, vis_thres,
                                                                  view_keep, out, ld_out, seen, count, nn);
    });
    GP_CHECK_LAUNCH();
    // (4) the fill
    return lb_fill(points, n, k.t.rows.k1, k.t.rows.idx, k.t.rows.off, k.f, k.tmp, k.tmp_bytes, seen, fill, nn, st, s);
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
