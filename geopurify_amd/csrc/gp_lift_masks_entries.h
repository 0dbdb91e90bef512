// Device code shared by the mask-embedding lifts over BATCHED point clouds (lift_masks_batched.hip: gp_lift_masks_batched, all views in
// one call; lift_masks_stream.hip: the same lift with the views arriving in chunks): the views' positions inside their entries, the
// checked copies of the visible entries, and the point -> (view, segment) lists over a bit set per point.  One definition for both.
#pragma once
#include "gp_lift_entries.h"

namespace {

enum { ST_LOST = 5, ST_TOTAL = 6, ST_MAX_VIEWS = 7, ST_BAD_ENTRY = 6, ST_BAD_WORDS = 7 };

size_t lmb_scan64_bytes(int64_t n) {
    size_t t = 0;
    (void)rocprim::exclusive_scan(nullptr, t, (int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), 0);
    return t;
}

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

int lmb_entry_tables(const double *points, int64_t n, const int64_t *view_entry, int32_t nviews, uint32_t *k0, uint32_t *k1, int32_t *r0,
                     int32_t *entry_rows, uint32_t *vk0, uint32_t *vk1, int32_t *w0, int32_t *entry_views, int32_t *entry_off, int32_t *view_off,
                     char *tmp, size_t tmp_bytes, unsigned long long *st, hipStream_t s) {
    const unsigned nb = (unsigned)((n + 255) / 256), vb = (unsigned)((nviews + 255) / 256);
    lb_row_keys_kernel<<<nb, 256, 0, s>>>(points, n, k0, r0, st);
    lb_view_keys_kernel<<<vb, 256, 0, s>>>(view_entry, nviews, vk0, w0, st);
    GP_CHECK_LAUNCH();
    size_t io = tmp_bytes;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(tmp, io, k0, k1, r0, entry_rows, (size_t)n, 0, LB_KEY_BITS, s));               // (stable)
    io = tmp_bytes;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(tmp, io, vk0, vk1, w0, entry_views, (size_t)nviews, 0, LB_KEY_BITS, s));       // (stable)
    lb_offsets_kernel<<<(LB_TABLE + 255) / 256, 256, 0, s>>>(k1, n, entry_off);
    lb_offsets_kernel<<<(LB_TABLE + 255) / 256, 256, 0, s>>>(vk1, nviews, view_off);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

}  // namespace
