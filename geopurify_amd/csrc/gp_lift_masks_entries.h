// Shared by the mask-embedding lifts over BATCHED point clouds (lift_masks_batched.hip: gp_lift_masks_batched, all views in one call;
// lift_masks_stream.hip: the same lift with the views arriving in chunks).  Device code: the views' positions inside their entries,
// the checked copies of the visible entries, and the point -> (view, segment) lists over a bit set per point.  Host code, at the end
// of the file: the pipeline of a call's or a chunk's entries (LmbEntries, lmb_chunk_segments: checked entries, the segments of
// gp_lift_masks.h, the in-view fill) and the end both share (LmbLists, lmb_fuse_fill: the lists, the top-3 fusion, the scene-level
// fill of gp_lift_entries.h), with the argument checks the entry points word alike.  One definition for both.
#pragma once
#include "gp_lift_entries.h"
#include "gp_lift_masks.h"

namespace {

enum { ST_LOST = 5, ST_TOTAL = 6, ST_MAX_VIEWS = 7, ST_BAD_ENTRY = 6, ST_BAD_WORDS = 7 };

// ------------------------------------------------------------------------------------------------ (2) the entries, checked
// view_local[v] = the position of view v among the views of its entry (ascending view index: the sort is stable); -1 for a view
// whose entry is outside 0..65535
__global__ void __launch_bounds__(256) lmb_view_local_kernel(const uint32_t *__restrict__ vkeys_sorted, const int32_t *__restrict__ entry_views,
                                                             const int32_t *__restrict__ view_off, int nviews, int words,
                                                             int32_t *__restrict__ view_local, unsigned long long *__restrict__ status) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    bool beyond = false;
    if (s < nviews) {
        const uint32_t b = vkeys_sorted[s];
        const int v = entry_views[s];
        int lp = -1;
        if (b < (uint32_t)LB_MAX_ENTRIES && (unsigned)v < (unsigned)nviews) {
            lp = s - view_off[b];
            beyond = lp < 0 || lp >= words * 64;
            if (beyond) lp = -1;
        }
        if ((unsigned)v < (unsigned)nviews) view_local[v] = lp;
    }
    const int nb = __popcll(__ballot(beyond));
    if (gp_lane() == 0 && nb) atomicAdd(status + ST_BAD_WORDS, (unsigned long long)nb);
}

__global__ void __launch_bounds__(256) lmb_xyz_kernel(const double *__restrict__ points, int64_t n, float *__restrict__ xyz) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (r >= n) return;
    const double *P = points + r * 4;
    xyz[r * 3] = (float)P[1];
    xyz[r * 3 + 1] = (float)P[2];
    xyz[r * 3 + 2] = (float)P[3];
}

// voff[0] = 0, voff[v+1] = view_off[v+1] clamped into [voff[v], total]; anything the clamp changes is counted (one thread: the walk
// is sequential, like fill_table_kernel's)
__global__ void lmb_view_off_kernel(const int64_t *__restrict__ view_off, int nviews, int64_t total, int64_t *__restrict__ voff,
                                    unsigned long long *__restrict__ status) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long bad = view_off[0] != 0 ? 1 : 0;
    int64_t prev = 0;
    voff[0] = 0;
    for (int v = 1; v <= nviews; ++v) {
        int64_t o = view_off[v];
        if (o < prev) { o = prev; ++bad; }
        if (o > total) { o = total; ++bad; }
        voff[v] = o;
        prev = o;
    }
    if (prev != total) ++bad;
    if (bad) atomicAdd(status + ST_BAD_ENTRY, bad);
}

// tap origins inside the mask (the weights are values only)
__global__ void __launch_bounds__(256) lmb_taps_kernel(const int32_t *__restrict__ tx0, const int32_t *__restrict__ ty0, int out_w, int out_h, int w,
                                                       int h, int32_t *__restrict__ cx0, int32_t *__restrict__ cy0,
                                                       unsigned long long *__restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < out_w) {
        const int o = tx0[i];
        bad = o < 0 || o >= w;
        cx0[i] = bad ? 0 : o;
    } else if (i < out_w + out_h) {
        const int o = ty0[i - out_w];
        bad = o < 0 || o >= h;
        cy0[i - out_w] = bad ? 0 : o;
    }
    const int nb = __popcll(__ballot(bad));
    if (gp_lane() == 0 && nb) atomicAdd(status + ST_BAD_ENTRY, (unsigned long long)nb);
}

// One thread per entry e of view pv = the view whose [voff[pv], voff[pv+1]) holds e.  The entry is what the lists promise when its
// view is pv, its point a row of pv's batch entry, above the row of the entry before it in the view, and its pixel inside the image.
// Otherwise it is counted and its copy is (view pv, point 0, a pixel outside the image): in range everywhere, and with c_live = 0 it
// gives no segment, sets no bit and takes no slot.  c_live is also 0 for the entries of a dropped view.
__global__ void __launch_bounds__(256) lmb_entries_kernel(const double *__restrict__ points, int64_t n, const int64_t *__restrict__ view_entry,
                                                          const int32_t *__restrict__ view_local, const int64_t *__restrict__ voff, int nviews,
                                                          int out_h, int out_w, const int64_t *__restrict__ ent_pt,
                                                          const int64_t *__restrict__ ent_x, const int64_t *__restrict__ ent_y,
                                                          const int32_t *__restrict__ ent_view, const uint8_t *__restrict__ keep, int64_t total,
                                                          int64_t *__restrict__ c_pt, int64_t *__restrict__ c_x, int64_t *__restrict__ c_y,
                                                          int32_t *__restrict__ c_view, uint8_t *__restrict__ c_live,
                                                          unsigned long long *__restrict__ status) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    bool bad = false;
    if (e < total) {
        int lo = 0, hi = nviews - 1;                                 // the last view whose first entry is <= e (voff ascends from 0 to total)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (voff[mid] <= e) lo = mid; else hi = mid - 1;
        }
        const int pv = lo;
        const int64_t p = ent_pt[e], x = ent_x[e], y = ent_y[e];
        bad = ent_view[e] != pv || (uint64_t)p >= (uint64_t)n || (uint64_t)x >= (uint64_t)out_h || (uint64_t)y >= (uint64_t)out_w;
        if (!bad) {
            const int64_t b = view_entry[pv];
            bad = (uint64_t)b >= (uint64_t)LB_MAX_ENTRIES || lb_entry_of(points[p * 4]) != (int)b;
            if (!bad && e > voff[pv]) bad = !(ent_pt[e - 1] < p);    // rows ascend inside a view (so a point occurs once in it)
        }
        const bool live = !bad && keep[pv] != 0 && view_local[pv] >= 0;
        c_pt[e] = bad ? 0 : p;
        c_x[e] = bad ? -1 : x;                                       // (a pixel outside the image decides nothing: segment -1)
        c_y[e] = bad ? -1 : y;
        c_view[e] = pv;
        c_live[e] = live ? 1 : 0;
    }
    const int nb = __popcll(__ballot(bad));
    if (gp_lane() == 0 && nb) atomicAdd(status + ST_BAD_ENTRY, (unsigned long long)nb);
}

// keep of a view for the segment kernels: the caller's flag, and the view has a position its entry's bit set holds
__global__ void __launch_bounds__(256) lmb_keep_kernel(const uint8_t *__restrict__ keep, const int32_t *__restrict__ view_local, int nviews,
                                                       uint8_t *__restrict__ c_keep) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < nviews) c_keep[v] = (keep[v] != 0 && view_local[v] >= 0) ? 1 : 0;
}

// an entry that was replaced is uncovered (pixel outside the image) and may have been filled as point 0: it shows no segment
__global__ void __launch_bounds__(256) lmb_dead_kernel(const uint8_t *__restrict__ c_live, int64_t total, int32_t *__restrict__ seg) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e < total && !c_live[e]) seg[e] = -1;
}

// ------------------------------------------------------------------------------------------------ (3) point -> (view, segment) lists
__global__ void __launch_bounds__(256) lmb_pv_mask_kernel(const int64_t *__restrict__ c_pt, const int32_t *__restrict__ c_view,
                                                          const uint8_t *__restrict__ c_live, const int32_t *__restrict__ view_local,
                                                          int64_t total, int words, unsigned long long *__restrict__ vmask) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= total || !c_live[e]) return;
    const int lp = view_local[c_view[e]];                            // 0 <= lp < words * 64 for a live entry
    atomicOr(&vmask[c_pt[e] * words + (lp >> 6)], 1ull << (lp & 63));
}

__global__ void __launch_bounds__(256) lmb_pv_cnt_kernel(const unsigned long long *__restrict__ vmask, int64_t n, int words,
                                                         int64_t *__restrict__ cnt /*[n+1]*/, int32_t *__restrict__ count,
                                                         int64_t *__restrict__ nn) {
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p > n) return;
    int c = 0;
    if (p < n) {
        for (int k = 0; k < words; ++k) c += __popcll(vmask[p * words + k]);
        count[p] = c;
        if (nn) nn[p] = -1;
    }
    cnt[p] = c;
}

__global__ void __launch_bounds__(256) lmb_pv_fill_kernel(const int64_t *__restrict__ c_pt, const int32_t *__restrict__ c_view,
                                                          const uint8_t *__restrict__ c_live, const int32_t *__restrict__ view_local,
                                                          const int32_t *__restrict__ seg, int64_t total, int words,
                                                          const unsigned long long *__restrict__ vmask, const int64_t *__restrict__ start,
                                                          int32_t *__restrict__ pv_view, int32_t *__restrict__ pv_seg) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= total || !c_live[e]) return;
    const int v = c_view[e];
    const int lp = view_local[v];
    const int64_t p = c_pt[e];
    const unsigned long long *m = vmask + p * words;
    int rank = 0;
    for (int k = 0; k < (lp >> 6); ++k) rank += __popcll(m[k]);
    rank += __popcll(m[lp >> 6] & ((1ull << (lp & 63)) - 1ull));
    const int64_t s_ = start[p] + rank;                              // < start[p + 1]: bit lp of the set is this entry's own
    pv_view[s_] = v;
    pv_seg[s_] = seg[e];
}

// ================================================================================================ host side
inline int lmb_check_masks(const char *who, int32_t q, int32_t h, int32_t w, int32_t out_h, int32_t out_w) {
    GP_CHECK_ARG(q >= 1 && q <= 1024, "%s: %d queries outside 1..1024 (the score sort holds 1024)", who, q);
    GP_CHECK_ARG(h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1 && (int64_t)h * w < (1ll << 31), "%s: masks %d x %d, image %d x %d", who, h, w, out_h,
                 out_w);
    return GP_OK;
}
inline int lmb_check_words(const char *who, int32_t words) {
    GP_CHECK_ARG(words >= 1 && words <= 1024, "%s: words=%d outside 1..1024", who, words);
    return GP_OK;
}
inline int lmb_check_fill_cap(const char *who, int64_t fill_cap, int64_t total) {
    GP_CHECK_ARG(fill_cap >= 0 && fill_cap <= total, "%s: fill_cap=%lld outside 0..total", who, (long long)fill_cap);
    return GP_OK;
}
// what the fusion and the scene-level fill ask of the segment tables and the outputs
inline int lmb_check_fused(const char *who, int32_t d, int32_t c, int64_t ld_out, const float *f_seg, const float *out, int32_t fill,
                           const int64_t *nn) {
    GP_CHECK_ARG(d >= 1 && c >= 1 && d % 4 == 0 && ld_out % 4 == 0 && ld_out >= d, "%s: d=%d and ld_out=%lld must be multiples of 4, c=%d", who, d,
                 (long long)ld_out, c);
    GP_CHECK_ARG(((uintptr_t)f_seg | (uintptr_t)out) % 16 == 0, "%s: f_seg and out must be 16-byte aligned", who);
    GP_CHECK_ARG(fill == 0 || nn, "%s: the fill writes nn", who);
    return GP_OK;
}

// ------------------------------------------------------------------------------------------------ a call's or a chunk's entries
// the checked copies of the per-view arrays and of the visible entries; total == 0 (a chunk in which nothing is visible): the per-view
// arrays alone
struct LmbEntries {
    int64_t *voff, *c_pt = nullptr, *c_x = nullptr, *c_y = nullptr;
    int32_t *c_view = nullptr, *cx0 = nullptr, *cy0 = nullptr;
    uint8_t *c_keep, *c_live = nullptr;
    float *xyz = nullptr;
    LmbEntries(GpCarver &cv, int64_t n, int32_t nviews, int32_t out_h, int32_t out_w, int64_t total) {
        voff = cv.take<int64_t>((size_t)nviews + 1);
        c_keep = cv.take<uint8_t>(nviews);
        if (total == 0) return;
        c_pt = cv.take<int64_t>(total);
        c_x = cv.take<int64_t>(total);
        c_y = cv.take<int64_t>(total);
        c_view = cv.take<int32_t>(total);
        c_live = cv.take<uint8_t>(total);
        cx0 = cv.take<int32_t>(out_w);
        cy0 = cv.take<int32_t>(out_h);
        xyz = cv.take<float>(3 * n);
    }
};

// seg[e] = the segment that entry e shows after the in-view fill, -1 for none.  The entries are checked and copied first -- an entry
// that is not what the lists promise is counted in the status and replaced by one that decides nothing --, then the kernels of
// gp_lift_masks.h run on the copies.  view_local: the position of every view inside its entry, -1 for none (lmb_view_local_kernel, or
// a stream's view_pos).  tmp holds gp_scan_bytes<int32_t>(total + 1).
inline int lmb_chunk_segments(const double *points, int64_t n, const int64_t *view_entry, const int32_t *view_local, int32_t nviews,
                              const void *pred_masks, int32_t elem, int32_t q, int32_t h, int32_t w, const float *scores, const int32_t *tap_x0,
                              const float *tap_wx, const int32_t *tap_y0, const float *tap_wy, int32_t out_h, int32_t out_w,
                              const int64_t *ent_pt, const int64_t *ent_x, const int64_t *ent_y, const int32_t *ent_view, const int64_t *view_off,
                              const uint8_t *keep, int64_t total, int64_t fill_cap, const LmbEntries &e, const LvSegWork &k, char *tmp,
                              size_t tmp_bytes, int32_t *seg, unsigned long long *st, hipStream_t s) {
    const unsigned nb = (unsigned)((n + 255) / 256), vb = (unsigned)((nviews + 255) / 256), eb = (unsigned)((total + 1 + 255) / 256);
    lmb_xyz_kernel<<<nb, 256, 0, s>>>(points, n, e.xyz);
    lmb_view_off_kernel<<<1, 64, 0, s>>>(view_off, nviews, total, e.voff, st);
    lmb_taps_kernel<<<(unsigned)((out_w + out_h + 255) / 256), 256, 0, s>>>(tap_x0, tap_y0, out_w, out_h, w, h, e.cx0, e.cy0, st);
    lmb_entries_kernel<<<eb, 256, 0, s>>>(points, n, view_entry, view_local, e.voff, nviews, out_h, out_w, ent_pt, ent_x, ent_y, ent_view, keep,
                                          total, e.c_pt, e.c_x, e.c_y, e.c_view, e.c_live, st);
    lmb_keep_kernel<<<vb, 256, 0, s>>>(keep, view_local, nviews, e.c_keep);
    GP_CHECK_LAUNCH();
#define LMB_SEGMENTS(T, BITS)                                                                                                                \
    lv_segments<T, BITS>(pred_masks, nviews, q, h, w, scores, e.cx0, tap_wx, e.cy0, tap_wy, out_h, out_w, e.xyz, e.c_pt, e.c_x, e.c_y, e.c_view, \
                         e.voff, e.c_keep, total, fill_cap, k, tmp, tmp_bytes, seg, s)
    if (elem == GP_ELEM_F32) LB_TRY(LMB_SEGMENTS(float, float));
    else if (elem == GP_ELEM_F16) LB_TRY(LMB_SEGMENTS(gp_f16, uint16_t));
    else LB_TRY(LMB_SEGMENTS(gp_bf16, uint16_t));
#undef LMB_SEGMENTS
    lmb_dead_kernel<<<eb, 256, 0, s>>>(e.c_live, total, seg);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

// ------------------------------------------------------------------------------------------------ the end: lists, fusion, fill
struct LmbLists {                                                // the point -> (view, segment) lists
    unsigned long long *vmask;
    int64_t *cnt, *pv_start;
    int32_t *pv_view, *pv_seg;
    LmbLists(GpCarver &cv, int64_t n, int64_t total, int32_t words) {
        vmask = cv.take<unsigned long long>((size_t)n * words);
        cnt = cv.take<int64_t>(n + 1);
        pv_start = cv.take<int64_t>(n + 1);
        pv_view = cv.take<int32_t>(total);
        pv_seg = cv.take<int32_t>(total);
    }
};

// From the checked entries (or records) and their segments: every point's (view, segment) list in ascending position of the view
// inside its entry, count, the consensus top-3 fusion (the kernel of the per-scene path: out, seen), and the scene-level fill inside
// every entry over the tables keys / rows / off (nn).  tmp holds gp_scan_bytes<int32_t>(n + 1) and gp_scan_bytes<int64_t>(n + 1).
inline int lmb_fuse_fill(const double *points, int64_t n, const int64_t *c_pt, const int32_t *c_view, const uint8_t *c_live,
                         const int32_t *view_local, const int32_t *seg, int64_t total, int32_t words, const LmbLists &l, const uint32_t *keys,
                         const int32_t *rows, const int32_t *off, const LbFill &f, char *tmp, size_t tmp_bytes, const float *f_seg,
                         const float *logit_seg, int32_t q, int32_t d, int32_t c, int32_t fill, float *out, int64_t ld_out, uint8_t *seen,
                         int32_t *count, int64_t *nn, unsigned long long *st, void *stream_) {
    hipStream_t s = gp_stream(stream_);
    const unsigned eb = (unsigned)((total + 255) / 256);
    GP_CHECK_HIP(hipMemsetAsync(l.vmask, 0, (size_t)n * words * sizeof(unsigned long long), s));
    lmb_pv_mask_kernel<<<eb, 256, 0, s>>>(c_pt, c_view, c_live, view_local, total, words, l.vmask);
    lmb_pv_cnt_kernel<<<(unsigned)((n + 1 + 255) / 256), 256, 0, s>>>(l.vmask, n, words, l.cnt, count, nn);
    size_t tb = tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(tmp, tb, l.cnt, l.pv_start, (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>(), s));
    lmb_pv_fill_kernel<<<eb, 256, 0, s>>>(c_pt, c_view, c_live, view_local, seg, total, words, l.vmask, l.pv_start, l.pv_view, l.pv_seg);
    GP_CHECK_LAUNCH();
    LB_TRY(gp_fuse_views_top3(l.pv_start, l.pv_view, l.pv_seg, n, f_seg, logit_seg, q, d, c, out, ld_out, seen, stream_));
    return lb_fill(points, n, keys, rows, off, f, tmp, tmp_bytes, seen, fill, nn, st, s);
}

}  // namespace
