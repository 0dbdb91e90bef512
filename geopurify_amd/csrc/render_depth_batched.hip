// Rendered depth over BATCHED point clouds (geopurify_amd/sparse.py: render_depth, and depth="render" in lift, LiftStream, lift_masks and
// LiftMasksStream): the z-buffer of models/utils/fusion_util.py:126-130 -- the ScanNet mapper with depth given as a str -- for every
// view of every batch entry in one sequence of launches,
//     depth[v, r, c] = min p_z over the points of view v's entry that project to pixel (r, c) inside the cut bound with p_z > 0.2,
//                      999999 where no such point lands
// with the arithmetic of render_depth_kernel (voxelize.hip: gp_render_depth_f64, one scene and one view per call); the decision is
// render_point of gp_project.h, the one definition both kernels run.  Entries never mix: a view renders the rows of its own entry only.
//
// Structure: (1) the entry tables -- gp_render_depth_batched sorts the rows stably by entry with lb_row_table of gp_lift_entries.h
// (lb_row_keys_kernel, the rocPRIM radix sort on 17-bit keys, lb_offsets_kernel), the same notion of "an entry's rows" as the lifts;
// gp_render_depth_batched_state takes them from a stream's state (gp_lift_stream_begin / gp_lift_masks_stream_begin) through
// ls_checked_tables of gp_lift_stream_state.h, every value forced into its range, and sorts nothing; (2) the whole [V, H, W] buffer filled with 999999 by 16-byte
// stores (a scalar head and tail where the buffer starts or ends off a 16-byte boundary); (3) the z-buffer: blockIdx.y = view, a view's
// blocks stride the sorted rows of its entry (lb_counts_kernel's launch shape), one 64-bit unsigned atomicMin on the fp64 bit pattern
// per rendered point.  Positive doubles order like their bit patterns and a minimum does not depend on the order of its operands, so
// two calls give the same bits and the bits are the sequential loop's.
//
// Bounds: a view's entry is range-checked before the offset table is read (0..65535; the table holds 65538 words) -- a view outside
// touches nothing, its image stays 999999, and it is counted in status[1]; sorted positions come from the offset table (inside 0..n
// by construction of the lower bounds, or forced there by ls_tables_kernel together with the row numbers); a row is rendered only when
// its own batch column names the view's entry, so rows with a bad batch index are never rendered and a state that was overwritten
// cannot mix entries; a pixel is written only after render_point found it inside [cut, W-cut) x [cut, H-cut) with cut >= 0.  All
// offsets are 64-bit.  The fill, the z-buffer kernel and their launch sequence (rd_render) are in gp_render_depth.h, shared with
// render_rows.hip.
#include "gp_render_depth.h"

namespace {

struct RdWork {                                                  // gp_render_depth_batched: the entry table and the sort's scratch
    LbTable rows;
    char *tmp;
    size_t tmp_bytes;
    RdWork(GpCarver &cv, int64_t n) : rows(lb_table(cv, n)) {
        tmp_bytes = lb_sort_bytes(n);
        tmp = cv.take<char>(tmp_bytes);
    }
};

int rd_check(const char *who, const double *points, int64_t n, const int64_t *view_entry, const double *w2c, const double *intrinsics,
             int32_t nviews, int32_t height, int32_t width, int32_t cut_bound, const double *depth, const int64_t *status,
             const void *workspace) {
    GP_CHECK_ARG(points && view_entry && w2c && intrinsics && depth && status && workspace, "%s: null argument", who);
    LB_TRY(lb_check_n(who, n));
    LB_TRY(lb_check_nviews(who, nviews));
    LB_TRY(lb_check_image(who, height, width));
    LB_TRY(lb_check_cut(who, cut_bound));
    GP_CHECK_ARG((reinterpret_cast<uintptr_t>(depth) & 7) == 0, "%s: depth is not 8-byte aligned", who);
    return GP_OK;
}

}  // namespace

extern "C" size_t gp_render_depth_batched_workspace_bytes(int64_t n, int32_t nviews) {
    if (!lb_n_ok(n) || !lb_nviews_ok(nviews)) return 0;
    GpCarver cv(nullptr, 0);
    RdWork k(cv, n);
    return cv.off;
}

extern "C" int gp_render_depth_batched(const double *points, int64_t n, const int64_t *view_entry, const double *w2c, const double *intrinsics,
                                       int32_t nviews, int32_t height, int32_t width, int32_t cut_bound, double *depth, int64_t *status,
                                       void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "gp_render_depth_batched";
    LB_TRY(rd_check(who, points, n, view_entry, w2c, intrinsics, nviews, height, width, cut_bound, depth, status, workspace));
    {
        const void *const in[] = {points, view_entry, w2c, intrinsics};
        const size_t in_bytes[] = {(size_t)n * 32, (size_t)nviews * 8, (size_t)nviews * 128, (size_t)nviews * 32};
        const void *const o[] = {depth, status, workspace};
        const size_t o_bytes[] = {(size_t)nviews * height * width * 8, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver cv(workspace, workspace_bytes);
    RdWork k(cv, n);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    LB_TRY(lb_row_table(points, n, k.rows, k.tmp, k.tmp_bytes, st, s));
    return rd_render(points, n, k.rows.idx, k.rows.off, view_entry, w2c, intrinsics, nviews, height, width, cut_bound, depth, st, s);
}

extern "C" size_t gp_render_depth_batched_state_workspace_bytes(int64_t n, int32_t nviews) {
    if (!lb_n_ok(n) || !lb_nviews_ok(nviews)) return 0;
    GpCarver cv(nullptr, 0);
    LsState k(cv, n);
    return cv.off;
}

extern "C" int gp_render_depth_batched_state(const double *points, int64_t n, const void *state, size_t state_bytes, const int64_t *view_entry,
                                             const double *w2c, const double *intrinsics, int32_t nviews, int32_t height, int32_t width,
                                             int32_t cut_bound, double *depth, int64_t *status, void *workspace, size_t workspace_bytes,
                                             void *stream_) {
    const char *who = "gp_render_depth_batched_state";
    LB_TRY(rd_check(who, points, n, view_entry, w2c, intrinsics, nviews, height, width, cut_bound, depth, status, workspace));
    GP_CHECK_ARG(state, "%s: null argument", who);
    LB_TRY(lb_check_state(who, state_bytes, ls_state_bytes(n)));
    {
        const void *const in[] = {points, state, view_entry, w2c, intrinsics};
        const size_t in_bytes[] = {(size_t)n * 32, state_bytes, (size_t)nviews * 8, (size_t)nviews * 128, (size_t)nviews * 32};
        const void *const o[] = {depth, status, workspace};
        const size_t o_bytes[] = {(size_t)nviews * height * width * 8, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver sv(const_cast<void *>(state), state_bytes), cv(workspace, workspace_bytes);
    const LsState tb(sv, n);
    const LsState k(cv, n);                                      // the checked copies of the state's tables
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    LB_TRY(ls_checked_tables(tb, n, k, nullptr, 0, status, s));  // (no running words: the state's owner reports them)
    return rd_render(points, n, k.rows, k.off, view_entry, w2c, intrinsics, nviews, height, width, cut_bound, depth,
                     reinterpret_cast<unsigned long long *>(status), s);
}
