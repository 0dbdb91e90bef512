// The mask-embedding lift with consensus top-3 fusion over BATCHED point clouds (geopurify_amd/sparse.py: lift_masks) --
// models/affinity_module.py:455-714 (lift_xdecoder_features) for every batch entry and every view in one sequence of launches, with
// no cap on the views of an entry.  Entry b's points are the rows of batch b in ascending row order, its views the views with
// view_entry == b in ascending view index.  The per-scene path (gp_views_visible_lists, gp_lift_masks_views with its two-word view
// mask = at most 128 views, gp_fuse_views_top3, gp_nn1_masked_f64) computes the same bits one scene at a time.
//
// (1) gp_lift_masks_batched_lists: the entry tables of gp_lift_entries.h, then the visible lists by an ORDERED compaction: the rows of
// a view's entry (ascending, the sort is stable) are cut into LML_PARTS contiguous parts, one block each; a block counts its visible
// rows, one exclusive scan over the [view, part] counts gives every block its first entry, and the blocks run the same walk again
// writing (global row, pixel row, pixel column, view) at scan + rank inside the tile (ballot ranks, wave counts through LDS).  No
// atomic cursor: rows ascend inside a view, which both fills rely on.
// (2) gp_lift_masks_batched: entries in (from (1) or from the caller), checked and copied first -- an entry that is not what the lists
// promise is counted in the status and replaced by one that decides nothing --, then the kernels of gp_lift_masks.h (score sort,
// ordered transpose, segment decision, in-view fill: they walk views, any number of them).  (3) the point -> (view, segment) lists: a
// bit set per point over the view's POSITION INSIDE ITS ENTRY (`words` 64-bit words, integer atomic OR), slot = popcount of the lower
// bits: a point's slots come out in ascending view index without the 128-view mask; then gp_fuse_views_top3's kernel.  (4) the
// per-entry scene-level fill of gp_lift_entries.h.
//
// Bounds: batch and view-entry indices are range-checked before every table access; sorted positions come from the offset tables;
// entry arrays are read through checked copies only (point row in 0..n-1, view = the one view_off puts the entry in, pixel inside the
// image, view_off clamped to ascend inside 0..total, tap origins inside the mask); a bit-set word index is < words by the check of the
// view's position; a slot index is start[p] + rank < start[p+1] because rank counts set bits below a set bit; every write of an entry
// is guarded by the capacity.  All offsets are 64-bit.
// (2) to (4) -- kernels, workspace structs and launch sequences -- live in gp_lift_masks_entries.h, on top of gp_lift_masks.h and
// gp_lift_entries.h: lift_masks_stream.hip, the same lift with the views arriving in chunks, runs them too.
#include "gp_lift_masks_entries.h"

namespace {

constexpr int LML_PARTS = 64;                                    // at most this many blocks share a view's rows

// ------------------------------------------------------------------------------------------------ (1) ordered visible lists
// blockIdx.y = view, blockIdx.x = part.  WRITE = false: blkcnt[v * parts + part] = visible rows of the part.  WRITE = true: base =
// the exclusive scan of those counts; the same walk, every visible row written at base + (visible rows before it).
template <bool WRITE>
__global__ void __launch_bounds__(256) lml_walk_kernel(const double *__restrict__ points, const int32_t *__restrict__ entry_rows,
                                                       const int32_t *__restrict__ entry_off, const int64_t *__restrict__ view_entry,
                                                       const double *__restrict__ w2c, const double *__restrict__ intr,
                                                       const double *__restrict__ depth, int W, int H, int cut, double tau, int parts,
                                                       int64_t *__restrict__ blkcnt, const int64_t *__restrict__ base_of, int64_t cap,
                                                       int64_t *__restrict__ ent_pt, int64_t *__restrict__ ent_x, int64_t *__restrict__ ent_y,
                                                       int32_t *__restrict__ ent_view, unsigned long long *__restrict__ status) {
    __shared__ int s_wave[4];
    const int v = blockIdx.y, part = blockIdx.x;
    const int64_t slot = (int64_t)v * parts + part;
    const int64_t e = view_entry[v];
    int64_t s0 = 0, s1 = 0;
    if ((uint64_t)e < (uint64_t)LB_MAX_ENTRIES) {                    // (block-uniform)
        const int64_t r0 = entry_off[e], r1 = entry_off[e + 1];
        const int64_t per = (r1 - r0 + parts - 1) / parts;
        s0 = r0 + part * per < r1 ? r0 + part * per : r1;
        s1 = s0 + per < r1 ? s0 + per : r1;
    }
    const double *M = w2c + (int64_t)v * 16, *K = intr + (int64_t)v * 4;
    const double *dv = depth ? depth + (int64_t)v * W * H : nullptr;
    const int lane = gp_lane(), wave = threadIdx.x >> 6;
    int64_t run = WRITE ? base_of[slot] : 0;
    int lost = 0;
    for (int64_t t = s0; t < s1; t += 256) {                         // (block-uniform trip count)
        const int64_t i = t + threadIdx.x;
        bool vis = false;
        long long ui = 0, vi = 0;
        int64_t row = 0;
        if (i < s1) {
            row = entry_rows[i];
            const double *P = points + row * 4;
            vis = project_point(P[1], P[2], P[3], M, M + 4, M + 8, K[0], K[1], K[2], K[3], dv, W, H, cut, tau, ui, vi);
        }
        const unsigned long long m = __ballot(vis);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = s_wave[k];
            before += k < wave ? c : 0;
            all += c;
        }
        if (WRITE && vis) {
            const int64_t pos = run + before + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < cap) {
                ent_pt[pos] = row;
                ent_x[pos] = vi;                                     // x = pixel row, y = pixel column (gp_views_visible_lists)
                ent_y[pos] = ui;
                ent_view[pos] = v;
            } else {
                ++lost;
            }
        }
        run += all;
        __syncthreads();
    }
    if (!WRITE) {
        if (threadIdx.x == 0) blkcnt[slot] = run;
    } else {
        lost = gp_wave_sum_i(lost);
        if (lane == 0 && lost) atomicAdd(status + ST_LOST, (unsigned long long)lost);
    }
}

// view_off[v] = scan[v * parts], view_count[v] = the difference to the next view, v = 0 .. nviews (view_off only)
__global__ void __launch_bounds__(256) lml_view_off_kernel(const int64_t *__restrict__ scan, int nviews, int parts, int64_t *__restrict__ view_off,
                                                           unsigned long long *__restrict__ view_count,
                                                           unsigned long long *__restrict__ status) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > nviews) return;
    const int64_t o = scan[(int64_t)v * parts];
    view_off[v] = o;
    if (v < nviews) view_count[v] = (unsigned long long)(scan[(int64_t)(v + 1) * parts] - o);
    else status[ST_TOTAL] = (unsigned long long)o;
}

// the most views one entry has (the views' offset table holds 65538 words)
__global__ void __launch_bounds__(256) lml_max_views_kernel(const int32_t *__restrict__ view_off, unsigned long long *__restrict__ status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    int c = b < LB_MAX_ENTRIES ? view_off[b + 1] - view_off[b] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c = max(c, __shfl_xor(c, o, 64));
    if (gp_lane() == 0 && c) atomicMax(status + ST_MAX_VIEWS, (unsigned long long)c);
}

struct LmlWork {
    LbTables t;
    int64_t *blkcnt, *scan;
    char *tmp;
    size_t tmp_bytes;
    int parts;
    LmlWork(GpCarver &cv, int64_t n, int32_t nviews) : t(cv, n, nviews) {
        const int64_t nb = (n + 255) / 256;
        parts = (int)(nb < LML_PARTS ? nb : LML_PARTS);
        const size_t slots = (size_t)nviews * parts + 1;
        tmp_bytes = std::max({lb_sort_bytes(n), lb_sort_bytes(nviews), gp_scan_bytes<int64_t>((int64_t)slots)});
        blkcnt = cv.take<int64_t>(slots);
        scan = cv.take<int64_t>(slots);
        tmp = cv.take<char>(tmp_bytes);
    }
};

struct LmbWork {
    LbTables t;                                                  // the entry tables
    LbFill f;                                                    // the scene-level fill
    int32_t *view_local;                                         // the views' positions inside their entries
    LmbEntries e;                                                // the checked entries
    LvSegWork k;                                                 // the segment decision and the in-view fill
    LmbLists l;                                                  // the point -> (view, segment) lists
    char *tmp;
    size_t tmp_bytes;
    LmbWork(GpCarver &cv, int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w, int32_t out_h, int32_t out_w, int64_t total, int32_t words,
            int64_t fill_cap, size_t esize)
        : t(cv, n, nviews), f(cv, n), view_local(cv.take<int32_t>(nviews)), e(cv, n, nviews, out_h, out_w, total),
          k(cv, nviews, q, h, w, total, fill_cap, esize, (size_t)nviews + 1), l(cv, n, total, words) {
        tmp_bytes = std::max({lb_sort_bytes(n), lb_sort_bytes(nviews), gp_scan_bytes<int32_t>(n + 1), gp_scan_bytes<int32_t>(total + 1), gp_scan_bytes<int64_t>(n + 1)});
        tmp = cv.take<char>(tmp_bytes);
    }
};

}  // namespace

extern "C" size_t gp_lift_masks_batched_lists_workspace_bytes(int64_t n, int32_t nviews) {
    if (!lb_n_ok(n) || !lb_nviews_ok(nviews)) return 0;
    GpCarver cv(nullptr, 0);
    LmlWork k(cv, n, nviews);
    return cv.off;
}

extern "C" int gp_lift_masks_batched_lists(const double *points, int64_t n, const int64_t *view_entry, const double *w2c,
                                           const double *intrinsics, const double *depth, int32_t nviews, int32_t height, int32_t width,
                                           int32_t cut_bound, double vis_thres, int64_t min_visible, int64_t max_visible, int64_t cap,
                                           int64_t *ent_pt, int64_t *ent_x, int64_t *ent_y, int32_t *ent_view, int64_t *view_off,
                                           int64_t *view_count, uint8_t *view_keep, int64_t *status, void *workspace, size_t workspace_bytes,
                                           void *stream_) {
    const char *who = "gp_lift_masks_batched_lists";
    GP_CHECK_ARG(points && view_entry && w2c && intrinsics && view_off && view_count && view_keep && status && workspace, "%s: null argument", who);
    LB_TRY(lb_check_n(who, n));
    LB_TRY(lb_check_nviews(who, nviews));
    GP_CHECK_ARG(height >= 1 && width >= 1 && cut_bound >= 0, "%s: image %d x %d, cut_bound=%d", who, height, width, cut_bound);
    GP_CHECK_ARG(cap >= 0, "%s: cap=%lld must not be negative", who, (long long)cap);
    GP_CHECK_ARG(cap == 0 || (ent_pt && ent_x && ent_y && ent_view), "%s: cap=%lld entries need the entry arrays", who, (long long)cap);
    {
        // (cap == 0: the entry arrays are not written, whatever they point at)
        const size_t px = (size_t)height * width;
        const void *const in[] = {points, view_entry, w2c, intrinsics, depth};
        const size_t in_bytes[] = {(size_t)n * 32, (size_t)nviews * 8, (size_t)nviews * 128, (size_t)nviews * 32, (size_t)nviews * px * 8};
        const void *const o[] = {cap ? ent_pt : nullptr, cap ? ent_x : nullptr, cap ? ent_y : nullptr, cap ? ent_view : nullptr, view_off, view_count,
                                 view_keep, status, workspace};
        const size_t o_bytes[] = {(size_t)cap * 8, (size_t)cap * 8, (size_t)cap * 8, (size_t)cap * 4, ((size_t)nviews + 1) * 8, (size_t)nviews * 8,
                                  (size_t)nviews, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver cv(workspace, workspace_bytes);
    LmlWork k(cv, n, nviews);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    unsigned long long *vc = reinterpret_cast<unsigned long long *>(view_count);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    LB_TRY(lb_entry_tables(points, n, view_entry, nviews, k.t, k.tmp, k.tmp_bytes, st, s));
    const unsigned vb = (unsigned)((nviews + 255) / 256);
    const size_t slots = (size_t)nviews * k.parts + 1;
    const dim3 grid((unsigned)k.parts, (unsigned)nviews);
    GP_CHECK_HIP(hipMemsetAsync(k.blkcnt + (slots - 1), 0, sizeof(int64_t), s));
    lml_walk_kernel<false><<<grid, 256, 0, s>>>(points, k.t.rows.idx, k.t.rows.off, view_entry, w2c, intrinsics, depth, width, height, cut_bound,
                                                vis_thres, k.parts, k.blkcnt, nullptr, 0, nullptr, nullptr, nullptr, nullptr, st);
    GP_CHECK_LAUNCH();
    size_t io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, io, k.blkcnt, k.scan, (int64_t)0, slots, rocprim::plus<int64_t>(), s));
    lml_view_off_kernel<<<(unsigned)((nviews + 1 + 255) / 256), 256, 0, s>>>(k.scan, nviews, k.parts, view_off, vc, st);
    lb_keep_kernel<<<vb, 256, 0, s>>>(vc, nviews, min_visible, max_visible, view_keep);
    lml_max_views_kernel<<<LB_MAX_ENTRIES / 256, 256, 0, s>>>(k.t.views.off, st);
    GP_CHECK_LAUNCH();
    if (cap > 0) {
        lml_walk_kernel<true><<<grid, 256, 0, s>>>(points, k.t.rows.idx, k.t.rows.off, view_entry, w2c, intrinsics, depth, width, height, cut_bound,
                                                   vis_thres, k.parts, nullptr, k.scan, cap, ent_pt, ent_x, ent_y, ent_view, st);
        GP_CHECK_LAUNCH();
    }
    return GP_OK;
}

extern "C" size_t gp_lift_masks_batched_workspace_bytes_t(int32_t elem, int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w, int32_t out_h,
                                                          int32_t out_w, int64_t total, int32_t words, int64_t fill_cap) {
    if (!gp_elem_ok(elem)) return 0;
    if (!lb_n_ok(n) || !lb_nviews_ok(nviews) || q < 1 || q > 1024 || h < 1 || w < 1 || out_h < 1 || out_w < 1 || total < 1 ||
        total >= (int64_t)INT32_MAX || words < 1 || words > 1024 || fill_cap < 0 || fill_cap > total)
        return 0;
    GpCarver cv(nullptr, 0);
    LmbWork k(cv, n, nviews, q, h, w, out_h, out_w, total, words, fill_cap ? fill_cap : total, gp_elem_size(elem));
    return cv.off;
}

extern "C" size_t gp_lift_masks_batched_workspace_bytes(int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w, int32_t out_h, int32_t out_w,
                                                        int64_t total, int32_t words, int64_t fill_cap) {
    return gp_lift_masks_batched_workspace_bytes_t(GP_ELEM_F32, n, nviews, q, h, w, out_h, out_w, total, words, fill_cap);
}

extern "C" int gp_lift_masks_batched_t(const double *points, int64_t n, const int64_t *view_entry, int32_t nviews, const void *pred_masks,
                                       int32_t elem, int32_t q, int32_t h, int32_t w, const float *scores, const int32_t *tap_x0, const float *tap_wx,
                                       const int32_t *tap_y0, const float *tap_wy, int32_t out_h, int32_t out_w, const int64_t *ent_pt,
                                       const int64_t *ent_x, const int64_t *ent_y, const int32_t *ent_view, const int64_t *view_off,
                                       const uint8_t *keep, int64_t total, int32_t words, int64_t fill_cap, const float *f_seg,
                                       const float *logit_seg, int32_t d, int32_t c, int32_t fill, float *out, int64_t ld_out, uint8_t *seen,
                                       int32_t *count, int64_t *nn, int32_t *seg, int64_t *status, void *workspace, size_t workspace_bytes,
                                       void *stream_) {
    const char *who = "gp_lift_masks_batched";
    GP_CHECK_ARG(points && view_entry && pred_masks && scores && tap_x0 && tap_wx && tap_y0 && tap_wy && ent_pt && ent_x && ent_y && ent_view &&
                     view_off && keep && f_seg && logit_seg && out && seen && count && seg && status && workspace,
                 "%s: null argument", who);
    LB_TRY(lb_check_elem(who, elem, pred_masks, "masks"));
    LB_TRY(lb_check_n(who, n));
    LB_TRY(lb_check_nviews(who, nviews));
    LB_TRY(lmb_check_masks(who, q, h, w, out_h, out_w));
    GP_CHECK_ARG(((int64_t)h * w + 63) / 64 < (1ll << 31), "%s: masks of %d x %d exceed the grid", who, h, w);
    GP_CHECK_ARG(total >= 1 && total < (int64_t)INT32_MAX, "%s: %lld entries outside 1..2^31-2", who, (long long)total);
    LB_TRY(lmb_check_words(who, words));
    LB_TRY(lmb_check_fill_cap(who, fill_cap, total));
    LB_TRY(lmb_check_fused(who, d, c, ld_out, f_seg, out, fill, nn));
    if (fill_cap == 0) fill_cap = total;
    {
        const size_t vq = (size_t)nviews * q;
        const void *const in[] = {points, view_entry, pred_masks, scores, tap_x0, tap_wx, tap_y0, tap_wy, ent_pt, ent_x, ent_y, ent_view, view_off,
                                  keep, f_seg, logit_seg};
        const size_t in_bytes[] = {(size_t)n * 32, (size_t)nviews * 8, vq * h * w * gp_elem_size(elem), vq * 4, (size_t)out_w * 4, (size_t)out_w * 16, (size_t)out_h * 4,
                                   (size_t)out_h * 16, (size_t)total * 8, (size_t)total * 8, (size_t)total * 8, (size_t)total * 4,
                                   ((size_t)nviews + 1) * 8, (size_t)nviews, vq * d * 4, vq * c * 4};
        const void *const o[] = {out, seen, count, nn, seg, status, workspace};
        const size_t o_bytes[] = {(size_t)((n - 1) * ld_out + d) * 4, (size_t)n, (size_t)n * 4, (size_t)n * 8, (size_t)total * 4, (size_t)ST_WORDS * 8,
                                  workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver cv(workspace, workspace_bytes);
    LmbWork k(cv, n, nviews, q, h, w, out_h, out_w, total, words, fill_cap, gp_elem_size(elem));
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    // the entry tables, the views' positions inside their entries
    LB_TRY(lb_entry_tables(points, n, view_entry, nviews, k.t, k.tmp, k.tmp_bytes, st, s));
    GP_CHECK_HIP(hipMemsetAsync(k.view_local, 0xff, (size_t)nviews * sizeof(int32_t), s));
    lmb_view_local_kernel<<<(unsigned)((nviews + 255) / 256), 256, 0, s>>>(k.t.views.k1, k.t.views.idx, k.t.views.off, nviews, words, k.view_local, st);
    // the entries, checked; the segment of every entry; the in-view fill
    LB_TRY(lmb_chunk_segments(points, n, view_entry, k.view_local, nviews, pred_masks, elem, q, h, w, scores, tap_x0, tap_wx, tap_y0, tap_wy, out_h,
                              out_w, ent_pt, ent_x, ent_y, ent_view, view_off, keep, total, fill_cap, k.e, k.k, k.tmp, k.tmp_bytes, seg, st, s));
    // point -> (view, segment) lists in ascending view index, consensus top-3 fusion, the scene-level fill inside every entry
    return lmb_fuse_fill(points, n, k.e.c_pt, k.e.c_view, k.e.c_live, k.view_local, seg, total, words, k.l, k.t.rows.k1, k.t.rows.idx, k.t.rows.off,
                         k.f, k.tmp, k.tmp_bytes, f_seg, logit_seg, q, d, c, fill, out, ld_out, seen, count, nn, st, stream_);
}

extern "C" int gp_lift_masks_batched(const double *points, int64_t n, const int64_t *view_entry, int32_t nviews, const float *pred_masks, int32_t q,
                                     int32_t h, int32_t w, const float *scores, const int32_t *tap_x0, const float *tap_wx, const int32_t *tap_y0,
                                     const float *tap_wy, int32_t out_h, int32_t out_w, const int64_t *ent_pt, const int64_t *ent_x,
                                     const int64_t *ent_y, const int32_t *ent_view, const int64_t *view_off, const uint8_t *keep, int64_t total,
                                     int32_t words, int64_t fill_cap, const float *f_seg, const float *logit_seg, int32_t d, int32_t c, int32_t fill,
                                     float *out, int64_t ld_out, uint8_t *seen, int32_t *count, int64_t *nn, int32_t *seg, int64_t *status,
                                     void *workspace, size_t workspace_bytes, void *stream_) {
    return gp_lift_masks_batched_t(points, n, view_entry, nviews, pred_masks, GP_ELEM_F32, q, h, w, scores, tap_x0, tap_wx, tap_y0, tap_wy, out_h,
                                   out_w, ent_pt, ent_x, ent_y, ent_view, view_off, keep, total, words, fill_cap, f_seg, logit_seg, d, c, fill, out,
                                   ld_out, seen, count, nn, seg, status, workspace, workspace_bytes, stream_);
}
