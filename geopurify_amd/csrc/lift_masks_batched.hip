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
// The kernels of (2) and (3) and the entry tables' launch sequence live in gp_lift_masks_entries.h: lift_masks_stream.hip, the same
// lift with the views arriving in chunks, runs them too.
#include "gp_lift_masks_entries.h"
#include "gp_lift_masks.h"

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
    uint32_t *k0, *k1, *vk0, *vk1;
    int32_t *r0, *entry_rows, *w0, *entry_views, *entry_off, *view_off;
    int64_t *blkcnt, *scan;
    char *tmp;
    size_t tmp_bytes;
    int parts;
    static size_t scan64_bytes(int64_t n) { return lmb_scan64_bytes(n); }
    LmlWork(GpCarver &cv, int64_t n, int32_t nviews) {
        const int64_t nb = (n + 255) / 256;
        parts = (int)(nb < LML_PARTS ? nb : LML_PARTS);
        const size_t slots = (size_t)nviews * parts + 1;
        const size_t a = lb_sort_bytes(n), b = lb_sort_bytes(nviews), c = scan64_bytes((int64_t)slots);
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
        blkcnt = cv.take<int64_t>(slots);
        scan = cv.take<int64_t>(slots);
        tmp = cv.take<char>(tmp_bytes);
    }
};

struct LmbWork {
    // entry tables and the scene-level fill (as LbWork)
    uint32_t *k0, *k1, *vk0, *vk1;
    int32_t *r0, *entry_rows, *w0, *entry_views, *entry_off, *view_off, *ref, *qry, *rs, *qs, *rrow, *qpos;
    float *rxyz;
    // the checked entries
    int32_t *view_local, *c_view, *cx0, *cy0;
    int64_t *voff, *c_pt, *c_x, *c_y;
    uint8_t *c_live, *c_keep;
    float *xyz;
    // the segment decision and the in-view fill (as LvWork)
    void *mt;                                                    // (the rank-ordered transposed masks, in the masks' own element type)
    float *sscore, *f_rxyz;
    int32_t *order, *cov, *f_rs, *rent, *qent, *part_i;
    double *part_d;
    int4 *tab;
    // the point -> (view, segment) lists
    unsigned long long *vmask;
    int64_t *cnt, *pv_start;
    int32_t *pv_view, *pv_seg;
    char *tmp;
    size_t tmp_bytes;
    static size_t scan64_bytes(int64_t n) { return LmlWork::scan64_bytes(n); }
    LmbWork(GpCarver &cv, int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w, int32_t out_h, int32_t out_w, int64_t total, int32_t words,
            int64_t fill_cap, size_t esize) {
        size_t t[5] = {lb_sort_bytes(n), lb_sort_bytes(nviews), lb_scan_bytes(n + 1), lb_scan_bytes(total + 1), scan64_bytes(n + 1)};
        tmp_bytes = 0;
        for (size_t b : t) tmp_bytes = b > tmp_bytes ? b : tmp_bytes;
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
        view_local = cv.take<int32_t>(nviews);
        voff = cv.take<int64_t>((size_t)nviews + 1);
        c_pt = cv.take<int64_t>(total);
        c_x = cv.take<int64_t>(total);
        c_y = cv.take<int64_t>(total);
        c_view = cv.take<int32_t>(total);
        c_live = cv.take<uint8_t>(total);
        c_keep = cv.take<uint8_t>(nviews);
        cx0 = cv.take<int32_t>(out_w);
        cy0 = cv.take<int32_t>(out_h);
        xyz = cv.take<float>(3 * n);
        mt = cv.take<char>((size_t)nviews * q * h * w * esize);
        order = cv.take<int32_t>((size_t)nviews * q);
        sscore = cv.take<float>((size_t)nviews * q);
        cov = cv.take<int32_t>(total + 1);
        f_rs = cv.take<int32_t>(total + 1);
        rent = cv.take<int32_t>(total);
        qent = cv.take<int32_t>(total);
        f_rxyz = cv.take<float>(total * 3);
        part_d = cv.take<double>((size_t)FV_CHUNKS * fill_cap);
        part_i = cv.take<int32_t>((size_t)FV_CHUNKS * fill_cap);
        tab = cv.take<int4>((size_t)nviews + 1);
        vmask = cv.take<unsigned long long>((size_t)n * words);
        cnt = cv.take<int64_t>(n + 1);
        pv_start = cv.take<int64_t>(n + 1);
        pv_view = cv.take<int32_t>(total);
        pv_seg = cv.take<int32_t>(total);
        tmp = cv.take<char>(tmp_bytes);
    }
};

}  // namespace

extern "C" size_t gp_lift_masks_batched_lists_workspace_bytes(int64_t n, int32_t nviews) {
    if (n <= 0 || n >= (1ll << 31) || nviews < 1 || nviews > 65535) return 0;
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
    GP_CHECK_ARG(points && view_entry && w2c && intrinsics && view_off && view_count && view_keep && status && workspace,
                 "gp_lift_masks_batched_lists: null argument");
    GP_CHECK_ARG(n > 0 && n < (1ll << 31), "gp_lift_masks_batched_lists: n=%lld outside 1..2^31-1", (long long)n);
    GP_CHECK_ARG(nviews >= 1 && nviews <= 65535, "gp_lift_masks_batched_lists: %d views outside 1..65535", nviews);
    GP_CHECK_ARG(height >= 1 && width >= 1 && cut_bound >= 0, "gp_lift_masks_batched_lists: image %d x %d, cut_bound=%d", height, width, cut_bound);
    GP_CHECK_ARG(cap >= 0, "gp_lift_masks_batched_lists: cap=%lld must not be negative", (long long)cap);
    GP_CHECK_ARG(cap == 0 || (ent_pt && ent_x && ent_y && ent_view), "gp_lift_masks_batched_lists: cap=%lld entries need the entry arrays",
                 (long long)cap);
    {
        const size_t px = (size_t)height * width;
        const void *in[] = {points, view_entry, w2c, intrinsics, depth};
        const size_t in_bytes[] = {(size_t)n * 32, (size_t)nviews * 8, (size_t)nviews * 128, (size_t)nviews * 32, (size_t)nviews * px * 8};
        const void *o[] = {ent_pt, ent_x, ent_y, ent_view, view_off, view_count, view_keep, status, workspace};
        const size_t o_bytes[] = {(size_t)cap * 8, (size_t)cap * 8, (size_t)cap * 8, (size_t)cap * 4, ((size_t)nviews + 1) * 8, (size_t)nviews * 8,
                                  (size_t)nviews, (size_t)ST_WORDS * 8, workspace_bytes};
        for (int a = 0; a < 9; ++a) {
            if (a < 4 && cap == 0) continue;
            for (int i = 0; i < 5; ++i)
                GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], in[i], in_bytes[i]), "gp_lift_masks_batched_lists: an output overlaps an input");
            for (int q = a + 1; q < 9; ++q)
                GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], o[q], o_bytes[q]), "gp_lift_masks_batched_lists: two outputs overlap");
        }
    }
    GpCarver cv(workspace, workspace_bytes);
    LmlWork k(cv, n, nviews);
    if (!cv.ok()) {
        gp_set_error("gp_lift_masks_batched_lists: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    unsigned long long *vc = reinterpret_cast<unsigned long long *>(view_count);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    int rc = lmb_entry_tables(points, n, view_entry, nviews, k.k0, k.k1, k.r0, k.entry_rows, k.vk0, k.vk1, k.w0, k.entry_views, k.entry_off,
                              k.view_off, k.tmp, k.tmp_bytes, st, s);
    if (rc != GP_OK) return rc;
    const unsigned vb = (unsigned)((nviews + 255) / 256);
    const size_t slots = (size_t)nviews * k.parts + 1;
    const dim3 grid((unsigned)k.parts, (unsigned)nviews);
    GP_CHECK_HIP(hipMemsetAsync(k.blkcnt + (slots - 1), 0, sizeof(int64_t), s));
    lml_walk_kernel<false><<<grid, 256, 0, s>>>(points, k.entry_rows, k.entry_off, view_entry, w2c, intrinsics, depth, width, height, cut_bound,
                                                vis_thres, k.parts, k.blkcnt, nullptr, 0, nullptr, nullptr, nullptr, nullptr, st);
    GP_CHECK_LAUNCH();
    size_t io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, io, k.blkcnt, k.scan, (int64_t)0, slots, rocprim::plus<int64_t>(), s));
    lml_view_off_kernel<<<(unsigned)((nviews + 1 + 255) / 256), 256, 0, s>>>(k.scan, nviews, k.parts, view_off, vc, st);
    lb_keep_kernel<<<vb, 256, 0, s>>>(vc, nviews, min_visible, max_visible, view_keep);
    lml_max_views_kernel<<<LB_MAX_ENTRIES / 256, 256, 0, s>>>(k.view_off, st);
    GP_CHECK_LAUNCH();
    if (cap > 0) {
        lml_walk_kernel<true><<<grid, 256, 0, s>>>(points, k.entry_rows, k.entry_off, view_entry, w2c, intrinsics, depth, width, height, cut_bound,
                                                   vis_thres, k.parts, nullptr, k.scan, cap, ent_pt, ent_x, ent_y, ent_view, st);
        GP_CHECK_LAUNCH();
    }
    return GP_OK;
}

extern "C" size_t gp_lift_masks_batched_workspace_bytes_t(int32_t elem, int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w, int32_t out_h,
                                                          int32_t out_w, int64_t total, int32_t words, int64_t fill_cap) {
    if (!gp_elem_ok(elem)) return 0;
    if (n <= 0 || n >= (1ll << 31) || nviews < 1 || nviews > 65535 || q < 1 || q > 1024 || h < 1 || w < 1 || out_h < 1 || out_w < 1 || total < 1 ||
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
    GP_CHECK_ARG(points && view_entry && pred_masks && scores && tap_x0 && tap_wx && tap_y0 && tap_wy && ent_pt && ent_x && ent_y && ent_view &&
                     view_off && keep && f_seg && logit_seg && out && seen && count && seg && status && workspace,
                 "gp_lift_masks_batched: null argument");
    GP_CHECK_ARG(gp_elem_ok(elem), "gp_lift_masks_batched: element type %d (0 fp32, 1 fp16, 2 bf16)", elem);
    GP_CHECK_ARG(elem == GP_ELEM_F32 || (uintptr_t)pred_masks % 2 == 0, "gp_lift_masks_batched: half masks at an odd address");
    GP_CHECK_ARG(n > 0 && n < (1ll << 31), "gp_lift_masks_batched: n=%lld outside 1..2^31-1", (long long)n);
    GP_CHECK_ARG(nviews >= 1 && nviews <= 65535, "gp_lift_masks_batched: %d views outside 1..65535", nviews);
    GP_CHECK_ARG(q >= 1 && q <= 1024, "gp_lift_masks_batched: %d queries outside 1..1024 (the score sort holds 1024)", q);
    GP_CHECK_ARG(h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1 && (int64_t)h * w < (1ll << 31), "gp_lift_masks_batched: masks %d x %d, image %d x %d", h,
                 w, out_h, out_w);
    GP_CHECK_ARG(((int64_t)h * w + 63) / 64 < (1ll << 31), "gp_lift_masks_batched: masks of %d x %d exceed the grid", h, w);
    GP_CHECK_ARG(total >= 1 && total < (int64_t)INT32_MAX, "gp_lift_masks_batched: %lld entries outside 1..2^31-2", (long long)total);
    GP_CHECK_ARG(words >= 1 && words <= 1024, "gp_lift_masks_batched: words=%d outside 1..1024", words);
    GP_CHECK_ARG(fill_cap >= 0 && fill_cap <= total, "gp_lift_masks_batched: fill_cap=%lld outside 0..total", (long long)fill_cap);
    GP_CHECK_ARG(d >= 1 && c >= 1 && d % 4 == 0 && ld_out % 4 == 0 && ld_out >= d, "gp_lift_masks_batched: d=%d and ld_out=%lld must be multiples of 4, c=%d",
                 d, (long long)ld_out, c);
    GP_CHECK_ARG(((uintptr_t)f_seg | (uintptr_t)out) % 16 == 0, "gp_lift_masks_batched: f_seg and out must be 16-byte aligned");
    GP_CHECK_ARG(fill == 0 || nn, "gp_lift_masks_batched: the fill writes nn");
    if (fill_cap == 0) fill_cap = total;
    {
        const size_t vq = (size_t)nviews * q;
        const void *in[] = {points, view_entry, pred_masks, scores, tap_x0, tap_wx, tap_y0, tap_wy, ent_pt, ent_x, ent_y, ent_view, view_off, keep,
                            f_seg, logit_seg};
        const size_t in_bytes[] = {(size_t)n * 32, (size_t)nviews * 8, vq * h * w * gp_elem_size(elem), vq * 4, (size_t)out_w * 4, (size_t)out_w * 16, (size_t)out_h * 4,
                                   (size_t)out_h * 16, (size_t)total * 8, (size_t)total * 8, (size_t)total * 8, (size_t)total * 4,
                                   ((size_t)nviews + 1) * 8, (size_t)nviews, vq * d * 4, vq * c * 4};
        const void *o[] = {out, seen, count, nn, seg, status, workspace};
        const size_t o_bytes[] = {(size_t)((n - 1) * ld_out + d) * 4, (size_t)n, (size_t)n * 4, (size_t)n * 8, (size_t)total * 4, (size_t)ST_WORDS * 8,
                                  workspace_bytes};
        for (int a = 0; a < 7; ++a) {
            for (int i = 0; i < 16; ++i)
                GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], in[i], in_bytes[i]), "gp_lift_masks_batched: an output overlaps an input");
            for (int b = a + 1; b < 7; ++b) GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], o[b], o_bytes[b]), "gp_lift_masks_batched: two outputs overlap");
        }
    }
    GpCarver cv(workspace, workspace_bytes);
    LmbWork k(cv, n, nviews, q, h, w, out_h, out_w, total, words, fill_cap, gp_elem_size(elem));
    if (!cv.ok()) {
        gp_set_error("gp_lift_masks_batched: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    // the entry tables, the views' positions inside their entries, the fp32 xyz
    int rc = lmb_entry_tables(points, n, view_entry, nviews, k.k0, k.k1, k.r0, k.entry_rows, k.vk0, k.vk1, k.w0, k.entry_views, k.entry_off,
                              k.view_off, k.tmp, k.tmp_bytes, st, s);
    if (rc != GP_OK) return rc;
    const unsigned nb = (unsigned)((n + 255) / 256), vb = (unsigned)((nviews + 255) / 256), eb = (unsigned)((total + 1 + 255) / 256);
    GP_CHECK_HIP(hipMemsetAsync(k.view_local, 0xff, (size_t)nviews * sizeof(int32_t), s));
    lmb_view_local_kernel<<<vb, 256, 0, s>>>(k.vk1, k.entry_views, k.view_off, nviews, words, k.view_local, st);
    lmb_xyz_kernel<<<nb, 256, 0, s>>>(points, n, k.xyz);
    // the entries, checked
    lmb_view_off_kernel<<<1, 64, 0, s>>>(view_off, nviews, total, k.voff, st);
    lmb_taps_kernel<<<(unsigned)((out_w + out_h + 255) / 256), 256, 0, s>>>(tap_x0, tap_y0, out_w, out_h, w, h, k.cx0, k.cy0, st);
    lmb_entries_kernel<<<eb, 256, 0, s>>>(points, n, view_entry, k.view_local, k.voff, nviews, out_h, out_w, ent_pt, ent_x, ent_y, ent_view, keep,
                                          total, k.c_pt, k.c_x, k.c_y, k.c_view, k.c_live, st);
    lmb_keep_kernel<<<vb, 256, 0, s>>>(keep, k.view_local, nviews, k.c_keep);
    GP_CHECK_LAUNCH();
    // the segment of every entry (gp_lift_masks.h: the kernels of gp_lift_masks_views)
    const int64_t hw = (int64_t)h * w;
    lv_sort_scores_kernel<<<nviews, 256, 0, s>>>(scores, q, k.order, k.sscore);
    const dim3 tg((unsigned)((hw + 63) / 64), (unsigned)((q + 63) / 64), (unsigned)nviews);
    const unsigned sb = (unsigned)((total * 64 + 255) / 256);
#define LMB_SEGMENTS(T, BITS)                                                                                                                  \
    do {                                                                                                                                       \
        transpose_views_kernel<BITS><<<tg, 256, 0, s>>>(static_cast<const BITS *>(pred_masks), q, (int)hw, static_cast<BITS *>(k.mt), k.order);   \
        lift_masks_views_kernel<T><<<sb, 256, 0, s>>>(static_cast<const T *>(k.mt), q, h, w, k.sscore, k.order, k.cx0, tap_wx, k.cy0, tap_wy,    \
                                                      out_h, out_w, k.c_x, k.c_y, k.c_view, k.c_keep, total, seg);                             \
    } while (0)
    if (elem == GP_ELEM_F32) LMB_SEGMENTS(float, float);
    else if (elem == GP_ELEM_F16) LMB_SEGMENTS(gp_f16, uint16_t);
    else LMB_SEGMENTS(gp_bf16, uint16_t);
#undef LMB_SEGMENTS
    GP_CHECK_LAUNCH();
    // the in-view fill
    fill_flags_kernel<<<eb, 256, 0, s>>>(seg, total, k.cov);
    size_t tb = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, tb, k.cov, k.f_rs, (int32_t)0, (size_t)(total + 1), rocprim::plus<int32_t>(), s));
    fill_compact_kernel<<<eb, 256, 0, s>>>(k.xyz, k.c_pt, seg, k.f_rs, total, k.f_rxyz, k.rent, k.qent);
    const unsigned qb = (unsigned)(total / 256 + nviews + 1);                            // >= sum over views of ceil(queries / 256)
    fill_table_kernel<<<1, 64, 0, s>>>(k.voff, k.f_rs, nviews, k.tab);
    fill_part_kernel<<<dim3(qb, FV_CHUNKS), 256, 0, s>>>(k.xyz, k.c_pt, k.tab, nviews, k.f_rxyz, k.qent, k.part_d, k.part_i, fill_cap, k.rent, seg);
    fill_reduce_kernel<<<qb, 256, 0, s>>>(k.tab, nviews, k.part_d, k.part_i, fill_cap, k.rent, k.qent, seg);
    lmb_dead_kernel<<<eb, 256, 0, s>>>(k.c_live, total, seg);
    GP_CHECK_LAUNCH();
    // point -> (view, segment) lists in ascending view index
    GP_CHECK_HIP(hipMemsetAsync(k.vmask, 0, (size_t)n * words * sizeof(unsigned long long), s));
    lmb_pv_mask_kernel<<<eb, 256, 0, s>>>(k.c_pt, k.c_view, k.c_live, k.view_local, total, words, k.vmask);
    lmb_pv_cnt_kernel<<<(unsigned)((n + 1 + 255) / 256), 256, 0, s>>>(k.vmask, n, words, k.cnt, count, nn);
    tb = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, tb, k.cnt, k.pv_start, (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>(), s));
    lmb_pv_fill_kernel<<<eb, 256, 0, s>>>(k.c_pt, k.c_view, k.c_live, k.view_local, seg, total, words, k.vmask, k.pv_start, k.pv_view, k.pv_seg);
    GP_CHECK_LAUNCH();
    // consensus top-3 fusion: the kernel of the per-scene path
    rc = gp_fuse_views_top3(k.pv_start, k.pv_view, k.pv_seg, n, f_seg, logit_seg, q, d, c, out, ld_out, seen, stream_);
    if (rc != GP_OK) return rc;
    // the scene-level fill inside every entry
    const unsigned nb1 = (unsigned)((n + 1 + 255) / 256);
    lb_fill_flags_kernel<<<nb1, 256, 0, s>>>(k.k1, k.entry_rows, seen, n, k.ref, k.qry);
    GP_CHECK_LAUNCH();
    size_t io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, io, k.ref, k.rs, (int32_t)0, (size_t)(n + 1), rocprim::plus<int32_t>(), s));
    io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, io, k.qry, k.qs, (int32_t)0, (size_t)(n + 1), rocprim::plus<int32_t>(), s));
    lb_fill_compact_kernel<<<nb, 256, 0, s>>>(points, k.entry_rows, k.ref, k.qry, k.rs, k.qs, n, k.rxyz, k.rrow, k.qpos, st);
    if (fill) lb_fill_kernel<<<nb, 256, 0, s>>>(points, k.k1, k.entry_rows, k.entry_off, k.rs, k.qs, n, k.rxyz, k.rrow, k.qpos, nn, st);
    GP_CHECK_LAUNCH();
    return GP_OK;
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
