// The label vote over BATCHED point clouds (geopurify_amd/sparse.py: lift_labels, LiftLabelsStream): integer label maps [V, H, W] --
// the loader's label_2ds, slot 11 of its 20-tuple (dataset/data_loader_ablation.py:296-346) -- voted onto the points.  The reference
// has no such function; every geometric decision is its own: the mapper (models/utils/fusion_util.py:99-147, project_point) and the
// view-drop rule (dataset/data_loader_ablation.py:254-288).  For every batch entry b, with its points the rows of batch b and its views
// the views with view_entry == b,
//     n_v, keep_v      = gp_lift_batched's                                                          (view_count, view_keep)
//     cnt_p            = #kept views that see p, seen_p = cnt_p > 0                                  (count, seen)
//     votes[p, c]      = #kept views v that see p with labels[v, py, px] == c, c in 0..C-1; a sampled value in the ignore list
//                        casts no vote; any other sampled value outside 0..C-1 casts none either and is counted in status[7]
//     voted_p          = sum_c votes[p, c]                       (a seen point may have voted_p == 0)
//     labels_p         = the lowest c with the maximal votes[p, c] when voted_p > 0; with fill, in an entry that has voted and unvoted
//                        points, an unvoted point takes the label of the voted point OF ITS ENTRY that minimises (d^2, row) -- the
//                        fill of gp_lift_batched with "seen" read as "voted"; `unlabeled` everywhere else.  A filled point's votes
//                        row stays zero.
// All of it is integer arithmetic: the result is exact and does not depend on any order, which is why the stream's chunks commute.
//
// Structure: gp_lift_batched's (1) entry tables and (2) per-view counts with the drop rule (gp_lift_entries.h), then (3) the vote
// kernel on lb_lift_kernel's skeleton: one wave per point, lane l projects the point through the l-th view of a group of 64 views of
// its entry, and every visible-and-kept lane loads ITS OWN label (1..8 bytes): up to 64 independent loads in flight, not a serial walk
// of the ballot.  The per-point histogram is a slice of C words of LDS per wave (4 waves x C x 4 bytes per block, dynamic), counted with
// LDS integer adds (ds_add_u32; lanes that hit one class serialise inside the LDS, which is exact).  Why LDS and not registers: a
// register histogram over 64 lanes holds class c in accumulator c / 64 of lane c % 64, and the class is data -- a dynamic register
// index, which the compiler turns into scratch memory or into C / 64 predicated adds per sample preceded by a broadcast of every
// sample's label to the owning lane (a serial walk again).  The LDS slice is at most 4 KiB per wave (C <= 1024): 16 KiB per block of
// four waves, ten such blocks fit a CU's 160 KiB, i.e. more than the 32 waves a CU runs; at C = 200 it is 3.2 KiB per block, so LDS
// never limits occupancy and nothing spills.  After the views the wave reads its slice back lane-strided (conflict-free), stores the
// votes row once, coalesced, and reduces (votes desc, class asc) over the wave for the arg-max.  ACCUM (the stream): the slice is
// ADDED to the stored row, and only when some kept view of the chunk sees the point; the labels are taken by ll_labels_kernel at
// finish.  (4) the fill of gp_lift_entries.h over the mask "voted" instead of "seen", then labels[p] = labels[nn[p]].
//
// Bounds: a batch or view entry index is range-checked before every table access (0..65535; the tables hold 65538 words); sorted
// positions come from the offset tables; the pixel is read only after project_point put it inside [cut, W-cut) x [cut, H-cut) with
// cut >= 0; the class is tested against 0 <= lab < C (one unsigned compare of the 64-bit value) before it indexes the LDS slice; the
// stream takes nothing from its state without a check (gp_lift_stream_state.h); nn is tested against 0..n-1 before it indexes labels.
// All offsets are 64-bit.
#include "gp_lift_stream_state.h"

namespace {

enum { ST_BAD_LABEL = 7 };
constexpr int LL_MAX_CLASSES = 1024;
constexpr int LL_MAX_IGNORE = 16;

struct LlIgnore {                                                // the ignore list, by value into the kernel
    int64_t id[LL_MAX_IGNORE];
    int n;
};

inline bool ll_elem_ok(int32_t e) { return e == GP_LABEL_U8 || e == GP_LABEL_I16 || e == GP_LABEL_I32 || e == GP_LABEL_I64; }
inline size_t ll_elem_size(int32_t e) { return e == GP_LABEL_U8 ? 1 : (e == GP_LABEL_I16 ? 2 : (e == GP_LABEL_I32 ? 4 : 8)); }

// (votes desc, class asc) over the wave; every lane gets the winner
__device__ __forceinline__ void ll_wave_argmax(int &bv, int &bc) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ov = __shfl_xor(bv, o, 64), oc = __shfl_xor(bc, o, 64);
        if (ov > bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
    }
}

// ------------------------------------------------------------------------------------------------ the vote
// One wave per point.  T: the label maps' element type, widened to 64 bits as it is loaded.  Dynamic LDS: 4 x C int32.
template <typename T, bool ACCUM>
__global__ void __launch_bounds__(256) ll_vote_kernel(const double *__restrict__ points, int64_t n, const T *__restrict__ labels2d, int C,
                                                      const int32_t *__restrict__ entry_views, const int32_t *__restrict__ view_off,
                                                      const double *__restrict__ w2c, const double *__restrict__ intr,
                                                      const double *__restrict__ depth, int W, int H, int cut, double tau,
                                                      const uint8_t *__restrict__ keep, LlIgnore ign, int32_t *__restrict__ votes, int64_t ld_votes,
                                                      int32_t *__restrict__ count, uint8_t *__restrict__ seen, int32_t *__restrict__ voted,
                                                      uint8_t *__restrict__ has_vote, int64_t *__restrict__ labels, int64_t unlabeled,
                                                      int64_t *__restrict__ nn, unsigned long long *__restrict__ status) {
    extern __shared__ int32_t ll_hist[];
    const int64_t p = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;     // (the same for the whole wave: every exit is wave-uniform)
    if (p >= n) return;
    const int lane = gp_lane();
    int32_t *h = ll_hist + (int)(threadIdx.x >> 6) * C;          // this wave's slice: no other wave touches it
    const double *P = points + p * 4;
    const int b = lb_entry_of(P[0]);
    int v0 = 0, v1 = 0;
    if (b >= 0) { v0 = view_off[b]; v1 = view_off[b + 1]; }
    if (ACCUM && v0 >= v1) return;                               // the chunk holds no view of this entry
    const double x = P[1], y = P[2], z = P[3];
    const int64_t px_per_view = (int64_t)W * H;
    for (int c = lane; c < C; c += GP_WAVE) h[c] = 0;
    gp_wave_sync();
    int cnt = 0, nbad = 0;
    for (int g = v0; g < v1; g += GP_WAVE) {
        bool vis = false, bad = false;
        if (g + lane < v1) {
            const int v = entry_views[g + lane];
            if (keep[v]) {
                const double *M = w2c + (int64_t)v * 16, *K = intr + (int64_t)v * 4;
                long long ui, vi;
                vis = project_point(x, y, z, M, M + 4, M + 8, K[0], K[1], K[2], K[3], depth ? depth + (int64_t)v * px_per_view : nullptr, W, H, cut,
                                    tau, ui, vi);
                if (vis) {                                       // inside the image: the one place a pixel is read
                    const int64_t lab = (int64_t)labels2d[(int64_t)v * px_per_view + (int64_t)vi * W + ui];
                    bool ignored = false;
                    for (int i = 0; i < ign.n; ++i) ignored |= lab == ign.id[i];
                    if (!ignored) {
                        if ((uint64_t)lab < (uint64_t)C) atomicAdd(&h[lab], 1);
                        else bad = true;
                    }
                }
            }
        }
        cnt += __popcll(__ballot(vis));
        nbad += __popcll(__ballot(bad));
    }
    gp_wave_sync();
    if (lane == 0 && nbad) atomicAdd(status + ST_BAD_LABEL, (unsigned long long)nbad);
    int32_t *vrow = votes + p * ld_votes;
    if (ACCUM) {
        if (!cnt) return;                                        // unseen by this chunk: the row is neither loaded nor stored
        for (int c = lane; c < C; c += GP_WAVE) {
            const int a = h[c];
            if (a) vrow[c] += a;                                 // (the wave owns the row)
        }
        if (lane == 0) count[p] += cnt;
    } else {
        int sum = 0, bv = -1, bc = INT32_MAX;
        for (int c = lane; c < C; c += GP_WAVE) {                // ascending c per lane: the strict > keeps the lowest class
            const int a = h[c];
            vrow[c] = a;
            sum += a;
            if (a > bv) { bv = a; bc = c; }
        }
        sum = gp_wave_sum_i(sum);
        ll_wave_argmax(bv, bc);
        if (lane == 0) {
            count[p] = cnt;
            seen[p] = cnt > 0 ? 1 : 0;
            voted[p] = sum;
            has_vote[p] = sum > 0 ? 1 : 0;
            labels[p] = sum > 0 ? (int64_t)bc : unlabeled;
            nn[p] = -1;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the stream's end
// one wave per point over the stored votes row: voted, the arg-max label, seen; nn = -1 (the fill overwrites the rows it fills)
__global__ void __launch_bounds__(256) ll_labels_kernel(const int32_t *__restrict__ votes, int64_t ld_votes, const int32_t *__restrict__ count,
                                                        int64_t n, int C, int64_t unlabeled, int32_t *__restrict__ voted,
                                                        uint8_t *__restrict__ has_vote, uint8_t *__restrict__ seen, int64_t *__restrict__ labels,
                                                        int64_t *__restrict__ nn) {
    const int64_t p = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    if (p >= n) return;
    const int lane = gp_lane();
    const int32_t *vrow = votes + p * ld_votes;
    int sum = 0, bv = -1, bc = INT32_MAX;
    for (int c = lane; c < C; c += GP_WAVE) {
        const int a = vrow[c];
        sum += a;
        if (a > bv) { bv = a; bc = c; }
    }
    sum = gp_wave_sum_i(sum);
    ll_wave_argmax(bv, bc);
    if (lane == 0) {
        seen[p] = count[p] > 0 ? 1 : 0;
        voted[p] = sum;
        has_vote[p] = sum > 0 ? 1 : 0;
        labels[p] = sum > 0 ? (int64_t)bc : unlabeled;
        nn[p] = -1;
    }
}

// labels[p] = labels[nn[p]] for the rows the fill chose a source for: a source is a voted row, which no thread writes
__global__ void __launch_bounds__(256) ll_fill_apply_kernel(const int64_t *__restrict__ nn, int64_t n, int64_t *__restrict__ labels) {
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t j = nn[p];
    if ((uint64_t)j < (uint64_t)n) labels[p] = labels[j];
}

struct LlFill {                                                  // the fill over "voted" and what the label move needs beside it
    LbFill f;
    uint8_t *has_vote;
    int64_t *nn;
    LlFill(GpCarver &cv, int64_t n) : f(cv, n) {
        has_vote = cv.take<uint8_t>(n);
        nn = cv.take<int64_t>(n);
    }
};

struct LlWork {
    LbTables t;
    LlFill f;
    char *tmp;
    size_t tmp_bytes;
    LlWork(GpCarver &cv, int64_t n, int32_t nviews) : t(cv, n, nviews), f(cv, n) {
        tmp_bytes = std::max({lb_sort_bytes(n), lb_sort_bytes(nviews), gp_scan_bytes<int32_t>(n + 1)});
        tmp = cv.take<char>(tmp_bytes);
    }
};

struct LlFinishWork {                                            // the checked copies of the state's tables, the fill
    LsState tables;
    LlFill f;
    char *tmp;
    size_t tmp_bytes;
    LlFinishWork(GpCarver &cv, int64_t n) : tables(cv, n), f(cv, n) {
        tmp_bytes = gp_scan_bytes<int32_t>(n + 1);
        tmp = cv.take<char>(tmp_bytes);
    }
};

int ll_ignore(const char *who, const int64_t *ignore_ids, int32_t n_ignore, LlIgnore &ign) {
    GP_CHECK_ARG(n_ignore >= 0 && n_ignore <= LL_MAX_IGNORE && (n_ignore == 0 || ignore_ids), "%s: %d ignore labels outside 0..%d", who, n_ignore,
                 LL_MAX_IGNORE);
    ign.n = n_ignore;
    for (int i = 0; i < LL_MAX_IGNORE; ++i) ign.id[i] = i < n_ignore ? ignore_ids[i] : 0;
    return GP_OK;
}

// the fill over the mask f.has_vote and the labels it moves; keys / rows / off: the entry tables (the sort's, or the checked copies)
int ll_fill(const double *points, int64_t n, const uint32_t *keys, const int32_t *rows, const int32_t *off, const LlFill &f, char *tmp,
            size_t tmp_bytes, int32_t fill, int64_t *labels, unsigned long long *st, hipStream_t s) {
    LB_TRY(lb_fill(points, n, keys, rows, off, f.f, tmp, tmp_bytes, f.has_vote, fill, f.nn, st, s));
    if (fill) ll_fill_apply_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(f.nn, n, labels);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

// the checks the entry points word alike: the votes' shape
int ll_check_classes(const char *who, int32_t num_classes, int64_t ld_votes) {
    GP_CHECK_ARG(num_classes >= 1 && num_classes <= LL_MAX_CLASSES && ld_votes >= num_classes, "%s: num_classes=%d outside 1..%d, ld_votes=%lld", who,
                 num_classes, LL_MAX_CLASSES, (long long)ld_votes);
    return GP_OK;
}

// the two calls that read label maps: element type and alignment, n, the views, the votes' shape, the image, the cut bound
int ll_check_maps(const char *who, const void *labels2d, int32_t elem, int64_t n, int32_t nviews, int32_t num_classes, int64_t ld_votes,
                  int32_t height, int32_t width, int32_t cut_bound) {
    GP_CHECK_ARG(ll_elem_ok(elem), "%s: label type %d (0 u8, 1 i16, 2 i32, 3 i64)", who, elem);
    GP_CHECK_ARG((uintptr_t)labels2d % ll_elem_size(elem) == 0, "%s: label maps not aligned to their element", who);
    LB_TRY(lb_check_n(who, n));
    LB_TRY(lb_check_nviews(who, nviews));
    LB_TRY(ll_check_classes(who, num_classes, ld_votes));
    LB_TRY(lb_check_image(who, height, width));
    return lb_check_cut(who, cut_bound);
}

// fill is a flag, and `unlabeled` no class
int ll_check_fill(const char *who, int32_t fill, int64_t unlabeled, int32_t num_classes) {
    GP_CHECK_ARG(fill == 0 || fill == 1, "%s: fill=%d (0 or 1)", who, fill);
    GP_CHECK_ARG((uint64_t)unlabeled >= (uint64_t)num_classes, "%s: unlabeled=%lld is a class of 0..%d", who, (long long)unlabeled, num_classes - 1);
    return GP_OK;
}

template <bool ACCUM>
int ll_vote(const double *points, int64_t n, const void *labels2d, int32_t elem, int32_t C, const int32_t *entry_views, const int32_t *view_off,
            const double *w2c, const double *intr, const double *depth, int32_t W, int32_t H, int32_t cut, double tau, const uint8_t *keep,
            const LlIgnore &ign, int32_t *votes, int64_t ld_votes, int32_t *count, uint8_t *seen, int32_t *voted, uint8_t *has_vote,
            int64_t *labels, int64_t unlabeled, int64_t *nn, unsigned long long *st, hipStream_t s) {
    const unsigned blocks = (unsigned)((n * 64 + 255) / 256);
    const size_t lds = (size_t)4 * C * sizeof(int32_t);          // <= 16 KiB: below the 64 KiB a launch may ask for without an attribute
#define LL_VOTE(T)                                                                                                                             \
    ll_vote_kernel<T, ACCUM><<<blocks, 256, lds, s>>>(points, n, static_cast<const T *>(labels2d), C, entry_views, view_off, w2c, intr, depth, W, H, \
                                                      cut, tau, keep, ign, votes, ld_votes, count, seen, voted, has_vote, labels, unlabeled, nn, st)
    if (elem == GP_LABEL_U8) LL_VOTE(uint8_t);
    else if (elem == GP_LABEL_I16) LL_VOTE(int16_t);
    else if (elem == GP_LABEL_I32) LL_VOTE(int32_t);
    else LL_VOTE(int64_t);
#undef LL_VOTE
    GP_CHECK_LAUNCH();
    return GP_OK;
}

}  // namespace

extern "C" size_t gp_lift_labels_batched_workspace_bytes(int64_t n, int32_t nviews) {
    if (!lb_n_ok(n) || !lb_nviews_ok(nviews)) return 0;
    GpCarver cv(nullptr, 0);
    LlWork k(cv, n, nviews);
    return cv.off;
}

extern "C" int gp_lift_labels_batched(const double *points, int64_t n, const void *labels2d, int32_t elem, int32_t num_classes,
                                      const int64_t *view_entry, const double *w2c, const double *intrinsics, const double *depth, int32_t nviews,
                                      int32_t height, int32_t width, int32_t cut_bound, double vis_thres, int64_t min_visible, int64_t max_visible,
                                      const int64_t *ignore_ids, int32_t n_ignore, int64_t unlabeled, int32_t fill, int64_t *labels, int32_t *votes,
                                      int64_t ld_votes, int32_t *voted, uint8_t *seen, int32_t *count, int64_t *view_count, uint8_t *view_keep,
                                      int64_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "gp_lift_labels_batched";
    GP_CHECK_ARG(points && labels2d && view_entry && w2c && intrinsics && labels && votes && voted && seen && count && view_count && view_keep &&
                     status && workspace,
                 "%s: null argument", who);
    LB_TRY(ll_check_maps(who, labels2d, elem, n, nviews, num_classes, ld_votes, height, width, cut_bound));
    LB_TRY(ll_check_fill(who, fill, unlabeled, num_classes));
    LlIgnore ign;
    LB_TRY(ll_ignore(who, ignore_ids, n_ignore, ign));
    {
        const size_t px = (size_t)height * width;
        const void *const in[] = {points, labels2d, view_entry, w2c, intrinsics, depth};
        const size_t in_bytes[] = {(size_t)n * 32,       (size_t)nviews * px * ll_elem_size(elem), (size_t)nviews * 8, (size_t)nviews * 128,
                                   (size_t)nviews * 32, (size_t)nviews * px * 8};
        const void *const o[] = {labels, votes, voted, seen, count, view_count, view_keep, status, workspace};
        const size_t o_bytes[] = {(size_t)n * 8, (size_t)((n - 1) * ld_votes + num_classes) * 4, (size_t)n * 4, (size_t)n, (size_t)n * 4,
                                  (size_t)nviews * 8, (size_t)nviews, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver cv(workspace, workspace_bytes);
    LlWork k(cv, n, nviews);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    // (1) entry tables, (2) per-view counts and the drop rule
    LB_TRY(lb_entry_tables(points, n, view_entry, nviews, k.t, k.tmp, k.tmp_bytes, st, s));
    LB_TRY(lb_view_counts(points, n, k.t.rows.idx, k.t.rows.off, view_entry, w2c, intrinsics, depth, nviews, width, height, cut_bound, vis_thres,
                          min_visible, max_visible, view_count, view_keep, s));
    // (3) the vote
    LB_TRY(ll_vote<false>(points, n, labels2d, elem, num_classes, k.t.views.idx, k.t.views.off, w2c, intrinsics, depth, width, height, cut_bound,
                          vis_thres, view_keep, ign, votes, ld_votes, count, seen, voted, k.f.has_vote, labels, unlabeled, k.f.nn, st, s));
    // (4) the fill over "voted"
    return ll_fill(points, n, k.t.rows.k1, k.t.rows.idx, k.t.rows.off, k.f, k.tmp, k.tmp_bytes, fill, labels, st, s);
}

// ------------------------------------------------------------------------------------------------ the same vote, the views in chunks
extern "C" size_t gp_lift_labels_stream_state_bytes(int64_t n) { return lb_n_ok(n) ? ls_state_bytes(n) : 0; }

extern "C" size_t gp_lift_labels_stream_begin_workspace_bytes(int64_t n) { return lb_n_ok(n) ? ls_begin_workspace_bytes(n) : 0; }

extern "C" int gp_lift_labels_stream_begin(const double *points, int64_t n, int32_t num_classes, void *state, size_t state_bytes, int32_t *votes,
                                           int64_t ld_votes, int32_t *count, int64_t *status, void *workspace, size_t workspace_bytes,
                                           void *stream_) {
    const char *who = "gp_lift_labels_stream_begin";
    GP_CHECK_ARG(points && state && votes && count && status && workspace, "%s: null argument", who);
    LB_TRY(lb_check_n(who, n));
    LB_TRY(ll_check_classes(who, num_classes, ld_votes));
    LB_TRY(lb_check_state(who, state_bytes, ls_state_bytes(n)));
    {
        const void *const in[] = {points};
        const size_t in_bytes[] = {(size_t)n * 32};
        const void *const o[] = {state, votes, count, status, workspace};
        const size_t o_bytes[] = {state_bytes, (size_t)((n - 1) * ld_votes + num_classes) * 4, (size_t)n * 4, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver sv(state, state_bytes), cv(workspace, workspace_bytes);
    LsState st(sv, n);
    LsBeginWork k(cv, n);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    GP_CHECK_HIP(hipMemsetAsync(count, 0, (size_t)n * sizeof(int32_t), s));
    GP_CHECK_HIP(hipMemset2DAsync(votes, (size_t)ld_votes * 4, 0, (size_t)num_classes * 4, (size_t)n, s));   // the pitch columns untouched
    return ls_begin_tables(points, n, st, k, status, s);
}

extern "C" size_t gp_lift_labels_stream_add_workspace_bytes(int32_t nviews) { return lb_nviews_ok(nviews) ? ls_add_workspace_bytes(nviews) : 0; }

extern "C" int gp_lift_labels_stream_add(const double *points, int64_t n, const void *state, size_t state_bytes, const void *labels2d, int32_t elem,
                                         int32_t num_classes, const int64_t *view_entry, const double *w2c, const double *intrinsics,
                                         const double *depth, int32_t nviews, int32_t height, int32_t width, int32_t cut_bound, double vis_thres,
                                         int64_t min_visible, int64_t max_visible, const int64_t *ignore_ids, int32_t n_ignore, int32_t *votes,
                                         int64_t ld_votes, int32_t *count, int64_t *view_count, uint8_t *view_keep, int64_t *status, void *workspace,
                                         size_t workspace_bytes, void *stream_) {
    const char *who = "gp_lift_labels_stream_add";
    GP_CHECK_ARG(points && state && labels2d && view_entry && w2c && intrinsics && votes && count && view_count && view_keep && status && workspace,
                 "%s: null argument", who);
    LB_TRY(ll_check_maps(who, labels2d, elem, n, nviews, num_classes, ld_votes, height, width, cut_bound));
    LB_TRY(lb_check_state(who, state_bytes, ls_state_bytes(n)));
    LlIgnore ign;
    LB_TRY(ll_ignore(who, ignore_ids, n_ignore, ign));
    {
        const size_t px = (size_t)height * width;
        const void *const in[] = {points, state, labels2d, view_entry, w2c, intrinsics, depth};
        const size_t in_bytes[] = {(size_t)n * 32,       state_bytes,          (size_t)nviews * px * ll_elem_size(elem), (size_t)nviews * 8,
                                   (size_t)nviews * 128, (size_t)nviews * 32, (size_t)nviews * px * 8};
        const void *const o[] = {votes, count, view_count, view_keep, status, workspace};
        const size_t o_bytes[] = {(size_t)((n - 1) * ld_votes + num_classes) * 4, (size_t)n * 4, (size_t)nviews * 8, (size_t)nviews,
                                  (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver sv(const_cast<void *>(state), state_bytes), cv(workspace, workspace_bytes);
    const LsState st(sv, n);
    LsAddWork k(cv, nviews);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *sw = reinterpret_cast<unsigned long long *>(status);
    // (1) the chunk's view table; its bad entries join the running count.  (2) the chunk's per-view counts and the drop rule
    LB_TRY(lb_view_table(view_entry, nviews, k.views, k.tmp, k.tmp_bytes, sw, s));
    LB_TRY(ls_view_counts(points, n, st, view_entry, w2c, intrinsics, depth, nviews, width, height, cut_bound, vis_thres, min_visible, max_visible,
                          view_count, view_keep, s));
    // (3) the accumulating vote; the chunk's out-of-range labels join the running count
    return ll_vote<true>(points, n, labels2d, elem, num_classes, k.views.idx, k.views.off, w2c, intrinsics, depth, width, height, cut_bound, vis_thres,
                         view_keep, ign, votes, ld_votes, count, nullptr, nullptr, nullptr, nullptr, 0, nullptr, sw, s);
}

extern "C" size_t gp_lift_labels_stream_finish_workspace_bytes(int64_t n) {
    if (!lb_n_ok(n)) return 0;
    GpCarver cv(nullptr, 0);
    LlFinishWork k(cv, n);
    return cv.off;
}

extern "C" int gp_lift_labels_stream_finish(const double *points, int64_t n, const void *state, size_t state_bytes, const int32_t *votes,
                                            int32_t num_classes, int64_t ld_votes, const int32_t *count, const int64_t *status, int64_t unlabeled,
                                            int32_t fill, int64_t *labels, int32_t *voted, uint8_t *seen, int64_t *status_out, void *workspace,
                                            size_t workspace_bytes, void *stream_) {
    const char *who = "gp_lift_labels_stream_finish";
    GP_CHECK_ARG(points && state && votes && count && status && labels && voted && seen && status_out && workspace, "%s: null argument", who);
    LB_TRY(lb_check_n(who, n));
    LB_TRY(ll_check_classes(who, num_classes, ld_votes));
    LB_TRY(ll_check_fill(who, fill, unlabeled, num_classes));
    LB_TRY(lb_check_state(who, state_bytes, ls_state_bytes(n)));
    {
        const void *const in[] = {points, state, votes, count, status};
        const size_t in_bytes[] = {(size_t)n * 32, state_bytes, (size_t)((n - 1) * ld_votes + num_classes) * 4, (size_t)n * 4, (size_t)ST_WORDS * 8};
        const void *const o[] = {labels, voted, seen, status_out, workspace};
        const size_t o_bytes[] = {(size_t)n * 8, (size_t)n * 4, (size_t)n, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver sv(const_cast<void *>(state), state_bytes), cv(workspace, workspace_bytes);
    const LsState st(sv, n);
    LlFinishWork k(cv, n);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    // the running words into finish's status: those of every stream and the out-of-range labels
    LB_TRY(ls_checked_tables(st, n, k.tables, status, LS_CARRY | (1u << ST_BAD_LABEL), status_out, s));
    ll_labels_kernel<<<(unsigned)((n * 64 + 255) / 256), 256, 0, s>>>(votes, ld_votes, count, n, num_classes, unlabeled, voted, k.f.has_vote, seen,
                                                                       labels, k.f.nn);
    GP_CHECK_LAUNCH();
    // the fill of gp_lift_labels_batched, over the checked copies of the tables
    return ll_fill(points, n, k.tables.keys, k.tables.rows, k.tables.off, k.f, k.tmp, k.tmp_bytes, fill, labels,
                   reinterpret_cast<unsigned long long *>(status_out), s);
}
