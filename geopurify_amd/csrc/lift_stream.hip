// The 2D -> 3D lift over BATCHED point clouds, RESUMABLE (geopurify_amd/sparse.py: LiftStream): the views arrive in chunks, every
// chunk's maps are read once and may then be freed, and the result after any number of chunks is the bits of gp_lift_batched on the
// concatenation of the chunks -- the chunk loop of models/affinity_module.py:365-436 (sum_features / counter grown by index_add_ per
// chunk of max_batch_size views) and its end :435-449 (divide, fill), for all entries at once.
//     begin    the points' entry tables (rows sorted stably by entry, offsets), once, into the caller's STATE; sums = +0, count = 0,
//              the status words (bad batch rows, non-finite rows, top batch)
//     add      per chunk: the chunk's view table, n_v and keep_v of the chunk's views from each view's own count (the drop rule needs
//              no other view), then for every point sum_p = (((sum_p + f_v1) + f_v2) + ...) over the chunk's kept views that see it,
//              in ascending view index, cnt_p += their number
//     finish   out_p = sum_p / (cnt_p == 0 ? 1e-6 : cnt_p), seen_p, the per-entry fill's nn_p; sums, counts and state are only read
// Why the bits are gp_lift_batched's: a point's fp32 sum there starts from +0 and takes the kept views that see the point in ascending
// view index, one add each; here the same adds happen in the same order, with a store and a reload of the fp32 partial sum between two
// chunks, which changes no bit; the integer counts add up; keep_v depends on view v's own count alone; division and fill run once.
//
// The accumulating kernel is lb_lift_kernel's walk (lift_batched.hip; both run the sampling body of gp_lift_sample.h): one wave per
// point, lane l projects the point through the l-th view of a group of 64 of its entry's views IN THIS CHUNK, a 64-bit ballot is the
// visible-and-kept mask, its set bits are walked in ascending order with all lanes striding the channels (pixel-major maps: 256
// contiguous bytes per wave load).  The sum row is loaded at the first set bit and stored only if there was one: a point that no
// kept view of the chunk sees costs its projection and no
// row traffic.  One wave owns one point: the row's read-modify-write is its own, there are no float atomics.
//
// Bounds: a batch or view entry index is range-checked before every table access (0..65535; the tables hold 65538 words).  The state
// is written by begin alone, but it is the caller's memory between calls, so nothing read from it is trusted: add's count kernel
// clamps the two offsets to 0..n and skips a sorted row number outside 0..n-1 (and a row of another entry); finish copies the three
// tables into its workspace with keys clamped to 0..65536, row numbers to 0..n-1 and offsets to 0..n, counts what it had to change in
// status[6], and runs the fill of gp_lift_entries.h on the copies, whose indices then stay inside n / n+1 / 3n elements whatever the
// state held.  The chunk's view table lies in add's own workspace (positions inside 0..nviews by construction of the lower bounds).
// A pixel is read only after project_point found it inside [cut, W-cut) x [cut, H-cut) with cut >= 0; bilinear taps are clamped to
// the map; channel indices are guarded by c < d.  All offsets are 64-bit.
#include "gp_lift_stream_state.h"
#include "gp_lift_sample.h"

namespace {

// ------------------------------------------------------------------------------------------------ the accumulating lift
// One wave per point, over the views of the point's entry in this chunk.  T, VEC, BILINEAR as in lb_lift_kernel: the maps' element
// type, the consecutive columns a lane takes with one load and the sampling mode, as lb_add_sample and lb_col (gp_lift_sample.h)
// define them.  The sums stay fp32 whatever T is, so the chunks of one stream may differ in type.
template <typename T, int VEC, bool BILINEAR>
__global__ void __launch_bounds__(256) ls_accum_kernel(const double *__restrict__ points, int64_t n, const T *__restrict__ feat, int d, int h,
                                                       int w, float scale_h, float scale_w, const int32_t *__restrict__ entry_views,
                                                       const int32_t *__restrict__ view_off, const double *__restrict__ w2c,
                                                       const double *__restrict__ intr, const double *__restrict__ depth, int W, int H, int cut,
                                                       double tau, const uint8_t *__restrict__ keep, float *__restrict__ sums, int64_t ld_sum,
                                                       int32_t *__restrict__ count) {
    const int64_t p = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;     // (the same for the whole wave: every exit is wave-uniform)
    if (p >= n) return;
    const int lane = gp_lane();
    const double *P = points + p * 4;
    const int b = lb_entry_of(P[0]);
    if (b < 0) return;
    const int v0 = view_off[b], v1 = view_off[b + 1];
    if (v0 >= v1) return;                                            // the chunk holds no view of this entry
    const double x = P[1], y = P[2], z = P[3];
    const int64_t map = (int64_t)h * w * d;
    float *srow = sums + p * ld_sum;
    // (wave-uniform; the vector forms only) a lane's groups of four columns start at multiples of 4: float4 row traffic where the
    // sums' base and pitch allow it
    const bool wide = VEC > 1 && (((uintptr_t)sums | (uintptr_t)(ld_sum * 4)) & 15) == 0;
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
            if (m && !seen_by) {                                     // (wave-uniform) the first view that sees the point: continue its sum
                if (VEC > 1 && wide) {
#pragma unroll
                    for (int k = 0; k < LB_COLS_PER_LANE; k += 4) {
                        const int c = lb_col<VEC>(c0, lane, k);
                        if (c < d) {
                            const float4 q = *reinterpret_cast<const float4 *>(srow + c);
                            acc[k] = q.x; acc[k + 1] = q.y; acc[k + 2] = q.z; acc[k + 3] = q.w;
                        }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < LB_COLS_PER_LANE; ++k) {
                        const int c = lb_col<VEC>(c0, lane, k);
                        if (c < d) acc[k] = srow[c];
                    }
                }
            }
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
        if (!cnt) return;                                            // unseen by this chunk: the row is neither loaded nor stored
        if (VEC > 1 && wide) {
#pragma unroll
            for (int k = 0; k < LB_COLS_PER_LANE; k += 4) {
                const int c = lb_col<VEC>(c0, lane, k);
                if (c < d) *reinterpret_cast<float4 *>(srow + c) = make_float4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < LB_COLS_PER_LANE; ++k) {
                const int c = lb_col<VEC>(c0, lane, k);
                if (c < d) srow[c] = acc[k];
            }
        }
    }
    if (lane == 0) count[p] += cnt;
}

// ------------------------------------------------------------------------------------------------ the end
// one wave per point: the row divided once, seen, nn = -1 (the fill overwrites the rows it fills)
__global__ void __launch_bounds__(256) ls_divide_kernel(const float *__restrict__ sums, int64_t ld_sum, const int32_t *__restrict__ count,
                                                        int64_t n, int d, float *__restrict__ out, int64_t ld_out, uint8_t *__restrict__ seen,
                                                        int64_t *__restrict__ nn) {
    const int64_t p = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    if (p >= n) return;
    const int lane = gp_lane();
    const int cnt = count[p];
    const float den = cnt == 0 ? 1e-6f : (float)cnt;
    const float *srow = sums + p * ld_sum;
    float *orow = out + p * ld_out;
    for (int c = lane; c < d; c += GP_WAVE) orow[c] = srow[c] / den;
    if (lane == 0) {
        seen[p] = cnt > 0 ? 1 : 0;
        if (nn) nn[p] = -1;
    }
}

}  // namespace

extern "C" size_t gp_lift_stream_state_bytes(int64_t n) { return lb_n_ok(n) ? ls_state_bytes(n) : 0; }

extern "C" size_t gp_lift_stream_begin_workspace_bytes(int64_t n) { return lb_n_ok(n) ? ls_begin_workspace_bytes(n) : 0; }

extern "C" int gp_lift_stream_begin(const double *points, int64_t n, int32_t d, void *state, size_t state_bytes, float *sums, int64_t ld_sum,
                                    int32_t *count, int64_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "gp_lift_stream_begin";
    GP_CHECK_ARG(points && state && sums && count && status && workspace, "%s: null argument", who);
    LB_TRY(lb_check_n(who, n));
    GP_CHECK_ARG(d >= 1 && ld_sum >= d, "%s: d=%d, ld_sum=%lld", who, d, (long long)ld_sum);
    LB_TRY(lb_check_state(who, state_bytes, ls_state_bytes(n)));
    {
        const void *const in[] = {points};
        const size_t in_bytes[] = {(size_t)n * 32};
        const void *const o[] = {state, sums, count, status, workspace};
        const size_t o_bytes[] = {state_bytes, (size_t)((n - 1) * ld_sum + d) * 4, (size_t)n * 4, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver sv(state, state_bytes), cv(workspace, workspace_bytes);
    LsState st(sv, n);
    LsBeginWork k(cv, n);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    GP_CHECK_HIP(hipMemsetAsync(count, 0, (size_t)n * sizeof(int32_t), s));
    GP_CHECK_HIP(hipMemset2DAsync(sums, (size_t)ld_sum * 4, 0, (size_t)d * 4, (size_t)n, s));       // +0 in every sum, the pitch columns untouched
    return ls_begin_tables(points, n, st, k, status, s);
}

extern "C" size_t gp_lift_stream_add_workspace_bytes(int32_t nviews) { return lb_nviews_ok(nviews) ? ls_add_workspace_bytes(nviews) : 0; }

extern "C" int gp_lift_stream_add_t(const double *points, int64_t n, const void *state, size_t state_bytes, const void *feat, int32_t elem,
                                    int32_t d, int32_t h, int32_t w, const int64_t *view_entry, const double *w2c, const double *intrinsics,
                                    const double *depth, int32_t nviews, int32_t height, int32_t width, int32_t bilinear, int32_t cut_bound,
                                    double vis_thres, int64_t min_visible, int64_t max_visible, float *sums, int64_t ld_sum, int32_t *count,
                                    int64_t *view_count, uint8_t *view_keep, int64_t *status, void *workspace, size_t workspace_bytes,
                                    void *stream_) {
    const char *who = "gp_lift_stream_add";
    GP_CHECK_ARG(points && state && feat && view_entry && w2c && intrinsics && sums && count && view_count && view_keep && status && workspace,
                 "%s: null argument", who);
    LB_TRY(lb_check_elem(who, elem, feat, "maps"));
    LB_TRY(lb_check_n(who, n));
    LB_TRY(lb_check_nviews(who, nviews));
    GP_CHECK_ARG(d >= 1 && h >= 1 && w >= 1 && height >= 1 && width >= 1 && ld_sum >= d, "%s: d=%d, map %d x %d, image %d x %d, ld_sum=%lld", who, d, h,
                 w, height, width, (long long)ld_sum);
    LB_TRY(lb_check_sampling(who, bilinear, h, w, height, width));
    LB_TRY(lb_check_cut(who, cut_bound));
    LB_TRY(lb_check_state(who, state_bytes, ls_state_bytes(n)));
    {
        const size_t px = (size_t)height * width, maps = (size_t)nviews * h * w * d * gp_elem_size(elem);
        const void *const in[] = {points, state, feat, view_entry, w2c, intrinsics, depth};
        const size_t in_bytes[] = {(size_t)n * 32,      state_bytes,          maps, (size_t)nviews * 8, (size_t)nviews * 128, (size_t)nviews * 32,
                                   (size_t)nviews * px * 8};
        const void *const o[] = {sums, count, view_count, view_keep, status, workspace};
        const size_t o_bytes[] = {(size_t)((n - 1) * ld_sum + d) * 4, (size_t)n * 4, (size_t)nviews * 8, (size_t)nviews, (size_t)ST_WORDS * 8,
                                  workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver sv(const_cast<void *>(state), state_bytes), cv(workspace, workspace_bytes);
    const LsState st(sv, n);
    LsAddWork k(cv, nviews);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    // (1) the chunk's view table; its bad entries join the running count.  (2) the chunk's per-view counts and the drop rule
    LB_TRY(lb_view_table(view_entry, nviews, k.views, k.tmp, k.tmp_bytes, reinterpret_cast<unsigned long long *>(status), s));
    LB_TRY(ls_view_counts(points, n, st, view_entry, w2c, intrinsics, depth, nviews, width, height, cut_bound, vis_thres, min_visible, max_visible,
                          view_count, view_keep, s));
    // (3) the accumulating lift
    // area_pixel_compute_scale<float>(in, out, align_corners=true): (in-1)/(out-1) in fp32, 0 for a single output pixel
    const float sh = height > 1 ? (float)(h - 1) / (float)(height - 1) : 0.f;
    const float sw = width > 1 ? (float)(w - 1) / (float)(width - 1) : 0.f;
    const unsigned lb = (unsigned)((n * 64 + 255) / 256);
    lb_sample_dispatch(feat, elem, d, bilinear, [&](auto form) {
        using F = decltype(form);
        using T = typename F::type;
        ls_accum_kernel<T, F::vec, F::bilinear><<<lb, 256, 0, s>>>(points, n, static_cast<const T *>(feat), d, h, w, sh, sw, k.views.idx, k.views.off,
                                                                   w2c, intrinsics, depth, width, height, cut_bound, vis_thres, view_keep, sums,
                                                                   ld_sum, count);
    });
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_lift_stream_add(const double *points, int64_t n, const void *state, size_t state_bytes, const float *feat, int32_t d, int32_t h,
                                  int32_t w, const int64_t *view_entry, const double *w2c, const double *intrinsics, const double *depth,
                                  int32_t nviews, int32_t height, int32_t width, int32_t bilinear, int32_t cut_bound, double vis_thres,
                                  int64_t min_visible, int64_t max_visible, float *sums, int64_t ld_sum, int32_t *count, int64_t *view_count,
                                  uint8_t *view_keep, int64_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    return gp_lift_stream_add_t(points, n, state, state_bytes, feat, GP_ELEM_F32, d, h, w, view_entry, w2c, intrinsics, depth, nviews, height, width,
                                bilinear, cut_bound, vis_thres, min_visible, max_visible, sums, ld_sum, count, view_count, view_keep, status,
                                workspace, workspace_bytes, stream_);
}

extern "C" size_t gp_lift_stream_finish_workspace_bytes(int64_t n) {
    if (!lb_n_ok(n)) return 0;
    GpCarver cv(nullptr, 0);
    LsFinishWork k(cv, n);
    return cv.off;
}

extern "C" int gp_lift_stream_finish(const double *points, int64_t n, const void *state, size_t state_bytes, const float *sums, int32_t d,
                                     int64_t ld_sum, const int32_t *count, const int64_t *status, int32_t fill, float *out, int64_t ld_out,
                                     uint8_t *seen, int64_t *nn, int64_t *status_out, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "gp_lift_stream_finish";
    GP_CHECK_ARG(points && state && sums && count && status && out && seen && status_out && workspace, "%s: null argument", who);
    LB_TRY(lb_check_n(who, n));
    GP_CHECK_ARG(d >= 1 && ld_sum >= d && ld_out >= d, "%s: d=%d, ld_sum=%lld, ld_out=%lld", who, d, (long long)ld_sum, (long long)ld_out);
    GP_CHECK_ARG(fill == 0 || nn, "%s: the fill writes nn", who);
    LB_TRY(lb_check_state(who, state_bytes, ls_state_bytes(n)));
    {
        const void *const in[] = {points, state, sums, count, status};
        const size_t in_bytes[] = {(size_t)n * 32, state_bytes, (size_t)((n - 1) * ld_sum + d) * 4, (size_t)n * 4, (size_t)ST_WORDS * 8};
        const void *const o[] = {out, seen, nn, status_out, workspace};
        const size_t o_bytes[] = {(size_t)((n - 1) * ld_out + d) * 4, (size_t)n, (size_t)n * 8, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver sv(const_cast<void *>(state), state_bytes), cv(workspace, workspace_bytes);
    const LsState st(sv, n);
    LsFinishWork k(cv, n);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    LB_TRY(ls_checked_tables(st, n, k.tables, status, LS_CARRY, status_out, s));
    ls_divide_kernel<<<(unsigned)((n * 64 + 255) / 256), 256, 0, s>>>(sums, ld_sum, count, n, d, out, ld_out, seen, nn);
    GP_CHECK_LAUNCH();
    // the fill of gp_lift_batched, over the checked copies of the tables
    return lb_fill(points, n, k.tables.keys, k.tables.rows, k.tables.off, k.fill, k.tmp, k.tmp_bytes, seen, fill, nn,
                   reinterpret_cast<unsigned long long *>(status_out), s);
}
