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

// the running words into finish's status: bad batch rows, bad view entries, non-finite rows, top batch and the out-of-range labels
__global__ void ll_status_kernel(const int64_t *__restrict__ running, int64_t *__restrict__ status_out) {
    const int i = threadIdx.x;
    if (i < ST_WORDS) status_out[i] = (i <= ST_TOP_BATCH || i == ST_BAD_LABEL) ? running[i] : 0;
}

struct LlFill {                                                  // what the fill needs beside the entry tables
    int32_t *ref, *qry, *rs, *qs, *rrow, *qpos;
    float *rxyz;
    uint8_t *has_vote;
    int64_t *nn;
    LlFill(GpCarver &cv, int64_t n) {
        ref = cv.take<int32_t>(n + 1);
        qry = cv.take<int32_t>(n + 1);
        rs = cv.take<int32_t>(n + 1);
        qs = cv.take<int32_t>(n + 1);
        rrow = cv.take<int32_t>(n);
        qpos = cv.take<int32_t>(n);
        rxyz = cv.take<float>(3 * n);
        has_vote = cv.take<uint8_t>(n);
        nn = cv.take<int64_t>(n);
    }
};

struct LlWork {
    uint32_t *k0, *k1, *vk0, *vk1;
    int32_t *r0, *entry_rows, *w0, *entry_views, *entry_off, *view_off;
    char *tmp;
    size_t tmp_bytes;
    LlFill f;
    static size_t tmp_need(int64_t n, int32_t nviews) {
        const size_t a = lb_sort_bytes(n), b = lb_sort_bytes(nviews), c = lb_scan_bytes(n + 1);
        return a > b ? (a > c ? a : c) : (b > c ? b : c);
    }
    LlWork(GpCarver &cv, int64_t n, int32_t nviews)
        : k0(cv.take<uint32_t>(n)), k1(cv.take<uint32_t>(n)), vk0(cv.take<uint32_t>(nviews)), vk1(cv.take<uint32_t>(nviews)),
          r0(cv.take<int32_t>(n)), entry_rows(cv.take<int32_t>(n)), w0(cv.take<int32_t>(nviews)), entry_views(cv.take<int32_t>(nviews)),
          entry_off(cv.take<int32_t>(LB_TABLE)), view_off(cv.take<int32_t>(LB_TABLE)), tmp_bytes(tmp_need(n, nviews)), f(cv, n) {
        tmp = cv.take<char>(tmp_bytes);
    }
};

struct LlFinishWork {                                            // the checked copies of the state's tables, the fill
    uint32_t *keys;
    int32_t *rows, *off;
    char *tmp;
    size_t tmp_bytes;
    LlFill f;
    LlFinishWork(GpCarver &cv, int64_t n)
        : keys(cv.take<uint32_t>(n)), rows(cv.take<int32_t>(n)), off(cv.take<int32_t>(LB_TABLE)), tmp_bytes(lb_scan_bytes(n + 1)), f(cv, n) {
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
    const unsigned nb = (unsigned)((n + 255) / 256), nb1 = (unsigned)((n + 1 + 255) / 256);
    lb_fill_flags_kernel<<<nb1, 256, 0, s>>>(keys, rows, f.has_vote, n, f.ref, f.qry);
    GP_CHECK_LAUNCH();
    size_t io = tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(tmp, io, f.ref, f.rs, (int32_t)0, (size_t)(n + 1), rocprim::plus<int32_t>(), s));
    io = tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(tmp, io, f.qry, f.qs, (int32_t)0, (size_t)(n + 1), rocprim::plus<int32_t>(), s));
    lb_fill_compact_kernel<<<nb, 256, 0, s>>>(points, rows, f.ref, f.qry, f.rs, f.qs, n, f.rxyz, f.rrow, f.qpos, st);
    if (fill) {
        lb_fill_kernel<<<nb, 256, 0, s>>>(points, keys, rows, off, f.rs, f.qs, n, f.rxyz, f.rrow, f.qpos, f.nn, st);
        ll_fill_apply_kernel<<<nb, 256, 0, s>>>(f.nn, n, labels);
    }
    GP_CHECK_LAUNCH();
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
    if (!ls_n_ok(n) || nviews < 1 || nviews > 65535) return 0;
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
    GP_CHECK_ARG(ll_elem_ok(elem), "%s: label type %d (0 u8, 1 i16, 2 i32, 3 i64)", who, elem);
    GP_CHECK_ARG((uintptr_t)labels2d % ll_elem_size(elem) == 0, "%s: label maps not aligned to their element", who);
    GP_CHECK_ARG(ls_n_ok(n), "%s: n=%lld outside 1..2^31-1", who, (long long)n);
    GP_CHECK_ARG(nviews >= 1 && nviews <= 65535, "%s: %d views outside 1..65535", who, nviews);
    GP_CHECK_ARG(num_classes >= 1 && num_classes <= LL_MAX_CLASSES && ld_votes >= num_classes, "%s: num_classes=%d outside 1..%d, ld_votes=%lld", who,
                 num_classes, LL_MAX_CLASSES, (long long)ld_votes);
    GP_CHECK_ARG(height >= 1 && width >= 1, "%s: image %d x %d", who, height, width);
    GP_CHECK_ARG(cut_bound >= 0, "%s: cut_bound=%d must not be negative", who, cut_bound);
    GP_CHECK_ARG(fill == 0 || fill == 1, "%s: fill=%d (0 or 1)", who, fill);
    GP_CHECK_ARG((uint64_t)unlabeled >= (uint64_t)num_classes, "%s: unlabeled=%lld is a class of 0..%d", who, (long long)unlabeled, num_classes - 1);
    LlIgnore ign;
    if (int rc = ll_ignore(who, ignore_ids, n_ignore, ign)) return rc;
    {
        // every output against every input and every other output, over their whole extents
        const size_t px = (size_t)height * width;
        const void *in[] = {points, labels2d, view_entry, w2c, intrinsics, depth};
        const size_t in_bytes[] = {(size_t)n * 32,       (size_t)nviews * px * ll_elem_size(elem), (size_t)nviews * 8, (size_t)nviews * 128,
                                   (size_t)nviews * 32, (size_t)nviews * px * 8};
        const void *o[] = {labels, votes, voted, seen, count, view_count, view_keep, status, workspace};
        const size_t o_bytes[] = {(size_t)n * 8, (size_t)((n - 1) * ld_votes + num_classes) * 4, (size_t)n * 4, (size_t)n, (size_t)n * 4,
                                  (size_t)nviews * 8, (size_t)nviews, (size_t)ST_WORDS * 8, workspace_bytes};
        for (int a = 0; a < 9; ++a) {
            for (int i = 0; i < 6; ++i) GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], in[i], in_bytes[i]), "%s: an output overlaps an input", who);
            for (int q = a + 1; q < 9; ++q) GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], o[q], o_bytes[q]), "%s: two outputs overlap", who);
        }
    }
    GpCarver cv(workspace, workspace_bytes);
    LlWork k(cv, n, nviews);
    if (!cv.ok()) {
        gp_set_error("%s: workspace too small (%zu < %zu)", who, workspace_bytes, cv.off);
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
    // (3) the vote
    if (int rc = ll_vote<false>(points, n, labels2d, elem, num_classes, k.entry_views, k.view_off, w2c, intrinsics, depth, width, height, cut_bound,
                                vis_thres, view_keep, ign, votes, ld_votes, count, seen, voted, k.f.has_vote, labels, unlabeled, k.f.nn, st, s))
        return rc;
    // (4) the fill over "voted"
    return ll_fill(points, n, k.k1, k.entry_rows, k.entry_off, k.f, k.tmp, k.tmp_bytes, fill, labels, st, s);
}

// ------------------------------------------------------------------------------------------------ the same vote, the views in chunks
extern "C" size_t gp_lift_labels_stream_state_bytes(int64_t n) { return ls_n_ok(n) ? ls_state_bytes(n) : 0; }

extern "C" size_t gp_lift_labels_stream_begin_workspace_bytes(int64_t n) {
    if (!ls_n_ok(n)) return 0;
    GpCarver cv(nullptr, 0);
    LsBeginWork k(cv, n);
    return cv.off;
}

extern "C" int gp_lift_labels_stream_begin(const double *points, int64_t n, int32_t num_classes, void *state, size_t state_bytes, int32_t *votes,
                                           int64_t ld_votes, int32_t *count, int64_t *status, void *workspace, size_t workspace_bytes,
                                           void *stream_) {
    const char *who = "gp_lift_labels_stream_begin";
    GP_CHECK_ARG(points && state && votes && count && status && workspace, "%s: null argument", who);
    GP_CHECK_ARG(ls_n_ok(n), "%s: n=%lld outside 1..2^31-1", who, (long long)n);
    GP_CHECK_ARG(num_classes >= 1 && num_classes <= LL_MAX_CLASSES && ld_votes >= num_classes, "%s: num_classes=%d outside 1..%d, ld_votes=%lld", who,
                 num_classes, LL_MAX_CLASSES, (long long)ld_votes);
    GP_CHECK_ARG(state_bytes >= ls_state_bytes(n), "%s: state too small (%zu < %zu)", who, state_bytes, ls_state_bytes(n));
    {
        const void *o[] = {state, votes, count, status, workspace};
        const size_t o_bytes[] = {state_bytes, (size_t)((n - 1) * ld_votes + num_classes) * 4, (size_t)n * 4, (size_t)ST_WORDS * 8, workspace_bytes};
        for (int a = 0; a < 5; ++a) {
            GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], points, (size_t)n * 32), "%s: an output overlaps an input", who);
            for (int q = a + 1; q < 5; ++q) GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], o[q], o_bytes[q]), "%s: two outputs overlap", who);
        }
    }
    GpCarver sv(state, state_bytes), cv(workspace, workspace_bytes);
    LsState st(sv, n);
    LsBeginWork k(cv, n);
    if (!cv.ok()) {
        gp_set_error("%s: workspace too small (%zu < %zu)", who, workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    GP_CHECK_HIP(hipMemsetAsync(count, 0, (size_t)n * sizeof(int32_t), s));
    GP_CHECK_HIP(hipMemset2DAsync(votes, (size_t)ld_votes * 4, 0, (size_t)num_classes * 4, (size_t)n, s));   // the pitch columns untouched
    lb_row_keys_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(points, n, k.k0, k.r0, reinterpret_cast<unsigned long long *>(status));
    GP_CHECK_LAUNCH();
    size_t io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(k.tmp, io, k.k0, st.keys, k.r0, st.rows, (size_t)n, 0, LB_KEY_BITS, s));             // (stable)
    lb_offsets_kernel<<<(LB_TABLE + 255) / 256, 256, 0, s>>>(st.keys, n, st.off);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" size_t gp_lift_labels_stream_add_workspace_bytes(int32_t nviews) {
    if (nviews < 1 || nviews > 65535) return 0;
    GpCarver cv(nullptr, 0);
    LsAddWork k(cv, nviews);
    return cv.off;
}

extern "C" int gp_lift_labels_stream_add(const double *points, int64_t n, const void *state, size_t state_bytes, const void *labels2d, int32_t elem,
                                         int32_t num_classes, const int64_t *view_entry, const double *w2c, const double *intrinsics,
                                         const double *depth, int32_t nviews, int32_t height, int32_t width, int32_t cut_bound, double vis_thres,
                                         int64_t min_visible, int64_t max_visible, const int64_t *ignore_ids, int32_t n_ignore, int32_t *votes,
                                         int64_t ld_votes, int32_t *count, int64_t *view_count, uint8_t *view_keep, int64_t *status, void *workspace,
                                         size_t workspace_bytes, void *stream_) {
    const char *who = "gp_lift_labels_stream_add";
    GP_CHECK_ARG(points && state && labels2d && view_entry && w2c && intrinsics && votes && count && view_count && view_keep && status && workspace,
                 "%s: null argument", who);
    GP_CHECK_ARG(ll_elem_ok(elem), "%s: label type %d (0 u8, 1 i16, 2 i32, 3 i64)", who, elem);
    GP_CHECK_ARG((uintptr_t)labels2d % ll_elem_size(elem) == 0, "%s: label maps not aligned to their element", who);
    GP_CHECK_ARG(ls_n_ok(n), "%s: n=%lld outside 1..2^31-1", who, (long long)n);
    GP_CHECK_ARG(nviews >= 1 && nviews <= 65535, "%s: %d views outside 1..65535", who, nviews);
    GP_CHECK_ARG(num_classes >= 1 && num_classes <= LL_MAX_CLASSES && ld_votes >= num_classes, "%s: num_classes=%d outside 1..%d, ld_votes=%lld", who,
                 num_classes, LL_MAX_CLASSES, (long long)ld_votes);
    GP_CHECK_ARG(height >= 1 && width >= 1, "%s: image %d x %d", who, height, width);
    GP_CHECK_ARG(cut_bound >= 0, "%s: cut_bound=%d must not be negative", who, cut_bound);
    GP_CHECK_ARG(state_bytes >= ls_state_bytes(n), "%s: state too small (%zu < %zu)", who, state_bytes, ls_state_bytes(n));
    LlIgnore ign;
    if (int rc = ll_ignore(who, ignore_ids, n_ignore, ign)) return rc;
    {
        // every output against every input and every other output, over their whole extents
        const size_t px = (size_t)height * width;
        const void *in[] = {points, state, labels2d, view_entry, w2c, intrinsics, depth};
        const size_t in_bytes[] = {(size_t)n * 32,       state_bytes,          (size_t)nviews * px * ll_elem_size(elem), (size_t)nviews * 8,
                                   (size_t)nviews * 128, (size_t)nviews * 32, (size_t)nviews * px * 8};
        const void *o[] = {votes, count, view_count, view_keep, status, workspace};
        const size_t o_bytes[] = {(size_t)((n - 1) * ld_votes + num_classes) * 4, (size_t)n * 4, (size_t)nviews * 8, (size_t)nviews,
                                  (size_t)ST_WORDS * 8, workspace_bytes};
        for (int a = 0; a < 6; ++a) {
            for (int i = 0; i < 7; ++i) GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], in[i], in_bytes[i]), "%s: an output overlaps an input", who);
            for (int q = a + 1; q < 6; ++q) GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], o[q], o_bytes[q]), "%s: two outputs overlap", who);
        }
    }
    GpCarver sv(const_cast<void *>(state), state_bytes), cv(workspace, workspace_bytes);
    const LsState st(sv, n);
    LsAddWork k(cv, nviews);
    if (!cv.ok()) {
        gp_set_error("%s: workspace too small (%zu < %zu)", who, workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *vc = reinterpret_cast<unsigned long long *>(view_count);
    unsigned long long *sw = reinterpret_cast<unsigned long long *>(status);
    GP_CHECK_HIP(hipMemsetAsync(view_count, 0, (size_t)nviews * sizeof(int64_t), s));
    const unsigned nb = (unsigned)((n + 255) / 256), vb = (unsigned)((nviews + 255) / 256);
    // (1) the chunk's view table; its bad entries join the running count
    lb_view_keys_kernel<<<vb, 256, 0, s>>>(view_entry, nviews, k.vk0, k.w0, sw);
    GP_CHECK_LAUNCH();
    size_t io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(k.tmp, io, k.vk0, k.vk1, k.w0, k.entry_views, (size_t)nviews, 0, LB_KEY_BITS, s));  // (stable)
    lb_offsets_kernel<<<(LB_TABLE + 255) / 256, 256, 0, s>>>(k.vk1, nviews, k.view_off);
    // (2) the chunk's per-view counts and the drop rule
    ls_counts_kernel<<<dim3(nb < 64 ? nb : 64, (unsigned)nviews), 256, 0, s>>>(points, n, st.rows, st.off, view_entry, w2c, intrinsics, depth, width,
                                                                                height, cut_bound, vis_thres, vc);
    lb_keep_kernel<<<vb, 256, 0, s>>>(vc, nviews, min_visible, max_visible, view_keep);
    GP_CHECK_LAUNCH();
    // (3) the accumulating vote; the chunk's out-of-range labels join the running count
    return ll_vote<true>(points, n, labels2d, elem, num_classes, k.entry_views, k.view_off, w2c, intrinsics, depth, width, height, cut_bound, vis_thres,
                         view_keep, ign, votes, ld_votes, count, nullptr, nullptr, nullptr, nullptr, 0, nullptr, sw, s);
}

extern "C" size_t gp_lift_labels_stream_finish_workspace_bytes(int64_t n) {
    if (!ls_n_ok(n)) return 0;
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
    GP_CHECK_ARG(ls_n_ok(n), "%s: n=%lld outside 1..2^31-1", who, (long long)n);
    GP_CHECK_ARG(num_classes >= 1 && num_classes <= LL_MAX_CLASSES && ld_votes >= num_classes, "%s: num_classes=%d outside 1..%d, ld_votes=%lld", who,
                 num_classes, LL_MAX_CLASSES, (long long)ld_votes);
    GP_CHECK_ARG(fill == 0 || fill == 1, "%s: fill=%d (0 or 1)", who, fill);
    GP_CHECK_ARG((uint64_t)unlabeled >= (uint64_t)num_classes, "%s: unlabeled=%lld is a class of 0..%d", who, (long long)unlabeled, num_classes - 1);
    GP_CHECK_ARG(state_bytes >= ls_state_bytes(n), "%s: state too small (%zu < %zu)", who, state_bytes, ls_state_bytes(n));
    {
        const void *in[] = {points, state, votes, count, status};
        const size_t in_bytes[] = {(size_t)n * 32, state_bytes, (size_t)((n - 1) * ld_votes + num_classes) * 4, (size_t)n * 4, (size_t)ST_WORDS * 8};
        const void *o[] = {labels, voted, seen, status_out, workspace};
        const size_t o_bytes[] = {(size_t)n * 8, (size_t)n * 4, (size_t)n, (size_t)ST_WORDS * 8, workspace_bytes};
        for (int a = 0; a < 5; ++a) {
            for (int i = 0; i < 5; ++i) GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], in[i], in_bytes[i]), "%s: an output overlaps an input", who);
            for (int q = a + 1; q < 5; ++q) GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], o[q], o_bytes[q]), "%s: two outputs overlap", who);
        }
    }
    GpCarver sv(const_cast<void *>(state), state_bytes), cv(workspace, workspace_bytes);
    const LsState st(sv, n);
    LlFinishWork k(cv, n);
    if (!cv.ok()) {
        gp_set_error("%s: workspace too small (%zu < %zu)", who, workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *so = reinterpret_cast<unsigned long long *>(status_out);
    const int64_t most = n > LB_TABLE ? n : LB_TABLE;
    ll_status_kernel<<<1, 64, 0, s>>>(status, status_out);
    ls_tables_kernel<<<(unsigned)((most + 255) / 256), 256, 0, s>>>(st.keys, st.rows, st.off, n, k.keys, k.rows, k.off, so);
    ll_labels_kernel<<<(unsigned)((n * 64 + 255) / 256), 256, 0, s>>>(votes, ld_votes, count, n, num_classes, unlabeled, voted, k.f.has_vote, seen,
                                                                       labels, k.f.nn);
    GP_CHECK_LAUNCH();
    // the fill of gp_lift_labels_batched, over the checked copies of the tables
    return ll_fill(points, n, k.keys, k.rows, k.off, k.f, k.tmp, k.tmp_bytes, fill, labels, so, s);
}
