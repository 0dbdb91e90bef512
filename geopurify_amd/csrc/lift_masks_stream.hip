// The mask-embedding lift with consensus top-3 fusion over BATCHED point clouds, RESUMABLE (geopurify_amd/sparse.py: LiftMasksStream):
// the views arrive in chunks, a chunk's masks are read once and may then be freed, and the result after any number of chunks is the
// bits of gp_lift_masks_batched on the concatenation of the chunks -- the per-view loop of models/affinity_module.py:495-640 (one view's
// masks -> per-point segments -> the small record in point_info, the masks freed) and its end :647-714 (fusion over views, fill), for
// all entries at once.
//     begin    the points' entry tables (gp_lift_stream_state.h) and the per-entry view counters (0) into the caller's STATE, once; the
//              running status words (bad batch rows, non-finite rows, top batch)
//     sizes    between the counting call of gp_lift_masks_batched_lists on the chunk and the caller's one read-back: the chunk's
//              visible entries, those of its kept views (= the records it will append) and the most views one entry will have after
//              the chunk.  Changes nothing.
//     add      per chunk: every view's position inside its entry = the entry's counter + the view's rank among the chunk's views of
//              that entry (ascending chunk index: the sort is stable), the counters advanced; then the kernels of
//              gp_lift_masks_batched up to the in-view fill over a workspace sized by THE CHUNK; then one record (row, segment or -1)
//              per entry of a kept view, appended view-major at the caller's record offset, rows ascending inside a view
//     finish   the bit set per point over the positions, the popcount slots, the scan and the slot lists from the records (the kernels
//              of gp_lift_masks_entries.h), gp_fuse_views_top3, the per-entry fill of gp_lift_entries.h; everything kept is only read
// Why the bits are gp_lift_masks_batched's: visibility, drop rule, score sort, ordered transpose, segment decision and in-view fill
// are per view and read no other view, so a view's records are what the one call holds for it in seg[]; a point's slots are its kept
// views in ascending position inside the entry, which is arrival order here and ascending view index there -- the same lists, the
// same table rows (the accumulated f_seg / logit_seg are indexed by arrival index), the same fusion kernel.
//
// Bounds: a batch or view entry index is range-checked before every table access (0..65535; the tables hold 65538 words).  State,
// per-view arrays and records are the caller's memory between calls, so nothing read from them is trusted.  add forces a counter
// into 0..65535 before it adds to it and gives a view past position 65535 none (-1).  finish copies the entry tables with keys, rows
// and offsets forced into range (ls_tables_kernel), clamps the record offsets to ascend inside 0..total (lmb_view_off_kernel), takes a
// view's position only inside 0..64*words-1 and clamps a segment into -1..Q-1; a record whose row is outside 0..n-1, does not ascend
// inside its view, or lies in another entry than its view's takes no part (no bit, no slot).  Whatever had to be changed or left out
// is counted in status words 6 and 7.  A bit-set word index is < words by the position check; a slot index is start[p] + rank <
// start[p+1] because rank counts set bits below a set bit; an appended record is guarded by the records' capacity.  The chunk's
// entries go through the checked copies of gp_lift_masks_batched.  All offsets are 64-bit.  No float atomics (integer atomicOr / Add / Max).
// (The state's tables and their checked copy are gp_lift_stream_state.h's; the chunk's pipeline and the end shared with
// gp_lift_masks_batched are gp_lift_masks_entries.h's.)
#include "gp_lift_stream_state.h"
#include "gp_lift_masks_entries.h"

namespace {

constexpr int LMS_MAX_POS = 65536;                               // positions inside an entry: 1024 words of 64 (65535 views in all)
enum { LMS_MOST = 4, LMS_RECORDS = 5, LMS_BAD = 6, LMS_BEYOND = 7 };   // running status: most views of one entry, records so far

struct LmsState {                                                // the caller's state buffer
    LsState tables;                                              // the points' entry tables: written by begin, read by finish
    int32_t *views;                                              // [LB_MAX_ENTRIES] the views every entry has so far: advanced by add
    LmsState(GpCarver &cv, int64_t n) : tables(cv, n) { views = cv.take<int32_t>(LB_MAX_ENTRIES); }
};

size_t lms_state_bytes(int64_t n) {
    GpCarver cv(nullptr, 0);
    LmsState s(cv, n);
    return cv.off;
}

struct LmsSizesWork {
    LbTable t;                                                   // the chunk's views sorted stably by entry
    unsigned long long *scratch;                                 // the status words of the table's keys kernel: counted by add, not here
    char *tmp;
    size_t tmp_bytes;
    LmsSizesWork(GpCarver &cv, int32_t nviews) : t(lb_table(cv, nviews)) {
        tmp_bytes = lb_sort_bytes(nviews);
        scratch = cv.take<unsigned long long>(ST_WORDS);
        tmp = cv.take<char>(tmp_bytes);
    }
};

struct LmsAddWork {
    LbTable t;                                                   // the chunk's views sorted stably by entry
    int64_t *loc;
    LmbEntries e;                                                // the checked entries
    LvSegWork k;                                                 // the segment decision and the in-view fill
    int32_t *seg = nullptr;
    char *tmp;
    size_t tmp_bytes;
    LmsAddWork(GpCarver &cv, int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w, int32_t out_h, int32_t out_w, int64_t total,
               int64_t fill_cap, size_t esize)
        : t(lb_table(cv, nviews)), loc(cv.take<int64_t>((size_t)nviews + 1)), e(cv, n, nviews, out_h, out_w, total) {
        if (total > 0) {                                         // (a chunk in which nothing is visible needs the view table alone)
            k = LvSegWork(cv, nviews, q, h, w, total, fill_cap, esize, (size_t)nviews + 1);
            seg = cv.take<int32_t>(total);
        }
        tmp_bytes = std::max(lb_sort_bytes(nviews), gp_scan_bytes<int32_t>(total + 1));
        tmp = cv.take<char>(tmp_bytes);
    }
};

struct LmsFinishWork {
    LsFinishWork base;                                           // the checked entry tables, the scene-level fill, the scans' scratch
    // the checked per-view arrays and records
    int32_t *view_local, *c_view, *c_seg;
    int64_t *voff, *c_pt;
    uint8_t *c_live, *c_keep;
    LmbLists l;                                                  // the point -> (view, segment) lists
    LmsFinishWork(GpCarver &cv, int64_t n, int32_t nviews, int64_t total, int32_t words)
        : base(cv, n, gp_scan_bytes<int64_t>(n + 1)), view_local(cv.take<int32_t>(nviews)), c_view(cv.take<int32_t>(total)),
          c_seg(cv.take<int32_t>(total)), voff(cv.take<int64_t>((size_t)nviews + 1)), c_pt(cv.take<int64_t>(total)),
          c_live(cv.take<uint8_t>(total)), c_keep(cv.take<uint8_t>(nviews)), l(cv, n, total, words) {}
};

// a counter of the state, forced into 0..65535
__device__ __forceinline__ int lms_counter(int c, bool &changed) {
    changed = c < 0 || c >= LMS_MAX_POS;
    return c < 0 ? 0 : (c >= LMS_MAX_POS ? LMS_MAX_POS - 1 : c);
}

// ------------------------------------------------------------------------------------------------ sizes
// sizes[0] = the chunk's visible entries, sizes[1] = those of its kept views (one wave sum, one integer atomic per wave)
__global__ void __launch_bounds__(256) lms_totals_kernel(const int64_t *__restrict__ view_count, const uint8_t *__restrict__ keep, int nviews,
                                                         unsigned long long *__restrict__ sizes) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long all = 0, kept = 0;
    if (v < nviews) {
        const int64_t c = view_count[v];
        all = c > 0 ? (unsigned long long)c : 0;
        kept = keep[v] ? all : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        all += __shfl_xor(all, o, 64);
        kept += __shfl_xor(kept, o, 64);
    }
    if (gp_lane() == 0) {
        if (all) atomicAdd(sizes, all);
        if (kept) atomicAdd(sizes + 1, kept);
    }
}

// sizes[2] = the most views one entry has after the chunk: the running maximum, and counter + the chunk's views for every entry the
// chunk looks at
__global__ void __launch_bounds__(256) lms_most_kernel(const int32_t *__restrict__ view_off, const int32_t *__restrict__ counters,
                                                       const int64_t *__restrict__ running, unsigned long long *__restrict__ sizes) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    int m = 0;
    if (b < LB_MAX_ENTRIES) {
        const int c = view_off[b + 1] - view_off[b];
        bool changed;
        if (c > 0) m = lms_counter(counters[b], changed) + c;
    }
    if (b == 0) {
        const int64_t r = running[LMS_MOST];
        m = max(m, (int)(r < 0 ? 0 : (r > LMS_MAX_POS ? LMS_MAX_POS : r)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    if (gp_lane() == 0 && m) atomicMax(sizes + 2, (unsigned long long)m);
}

// ------------------------------------------------------------------------------------------------ add: positions and counters
// One wave per entry b; its views of this chunk are the sorted positions [view_off[b], view_off[b+1]) in ascending chunk index.
// Every lane reads the counter before lane 0 writes it back (one wave, program order), so position and advance are one kernel:
// view_pos[v] = counter + rank, counter += the chunk's views, the running maximum by one integer atomic per entry that has views.
__global__ void __launch_bounds__(256) lms_positions_kernel(const int32_t *__restrict__ entry_views, const int32_t *__restrict__ view_off,
                                                            int nviews, int32_t *__restrict__ counters, int32_t *__restrict__ view_pos,
                                                            unsigned long long *__restrict__ status) {
    const int b = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;      // (the same for the whole wave: every exit is wave-uniform)
    if (b >= LB_MAX_ENTRIES) return;
    const int s0 = view_off[b], s1 = view_off[b + 1];                // (inside 0..nviews: lower bounds over the chunk's sorted keys)
    if (s1 <= s0) return;
    const int lane = gp_lane();
    bool changed;
    const int base = lms_counter(counters[b], changed);
    for (int s = s0 + lane; s < s1; s += GP_WAVE) {
        const int v = entry_views[s];                                // (0..nviews-1: written by lb_view_keys_kernel in this call)
        const int pos = base + (s - s0);
        if ((unsigned)v < (unsigned)nviews) view_pos[v] = pos < LMS_MAX_POS ? pos : -1;
    }
    if (lane == 0) {
        const int after = base + (s1 - s0);
        counters[b] = after;
        atomicMax(status + LMS_MOST, (unsigned long long)(after < LMS_MAX_POS ? after : LMS_MAX_POS));
        if (changed) atomicAdd(status + LMS_BAD, 1ull);
        if (after > LMS_MAX_POS) atomicAdd(status + LMS_BEYOND, (unsigned long long)(after - LMS_MAX_POS));
    }
}

// ------------------------------------------------------------------------------------------------ add: the records
// loc[v] = the records of the chunk's kept views before v (a kept view has one per entry), rec_off[v] = rec_base + loc[v], v = 0 ..
// nviews; none: nothing is visible in the chunk (one thread: the walk is sequential, like lmb_view_off_kernel's)
__global__ void lms_rec_off_kernel(const int64_t *__restrict__ voff, const uint8_t *__restrict__ c_keep, int nviews, int none, int64_t rec_base,
                                   int64_t *__restrict__ loc, int64_t *__restrict__ rec_off, unsigned long long *__restrict__ status) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t run = 0;
    for (int v = 0; v <= nviews; ++v) {
        loc[v] = run;
        rec_off[v] = rec_base + run;
        if (v < nviews && !none && c_keep[v]) run += voff[v + 1] - voff[v];
    }
    if (run) atomicAdd(status + LMS_RECORDS, (unsigned long long)run);
}

// one thread per entry e of the chunk: the entry of a kept view becomes the record rec_base + loc[view] + (e - the view's first
// entry); an entry that was replaced by the checks carries row -1 and takes no part in finish
__global__ void __launch_bounds__(256) lms_append_kernel(const int64_t *__restrict__ c_pt, const int32_t *__restrict__ c_view,
                                                         const uint8_t *__restrict__ c_live, const uint8_t *__restrict__ c_keep,
                                                         const int64_t *__restrict__ voff, const int64_t *__restrict__ loc,
                                                         const int32_t *__restrict__ seg, int64_t total, int64_t rec_base, int64_t rec_cap,
                                                         int32_t *__restrict__ rec_row, int32_t *__restrict__ rec_seg) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int v = c_view[e];                                         // (0..nviews-1: lmb_entries_kernel's binary search)
    if (!c_keep[v]) return;
    const int64_t dst = rec_base + loc[v] + (e - voff[v]);
    if (dst < 0 || dst >= rec_cap) return;
    const bool live = c_live[e] != 0;
    rec_row[dst] = live ? (int32_t)c_pt[e] : -1;
    rec_seg[dst] = live ? seg[e] : -1;
}

// ------------------------------------------------------------------------------------------------ finish: the checked copies
// view_local[v] = the view's position inside its entry when the entry is one and the bit set holds the position, else -1; c_keep[v] =
// the keep flag of a view that has a position
__global__ void __launch_bounds__(256) lms_views_kernel(const int64_t *__restrict__ view_entry, const int32_t *__restrict__ view_pos,
                                                        const uint8_t *__restrict__ keep, int nviews, int words,
                                                        int32_t *__restrict__ view_local, uint8_t *__restrict__ c_keep,
                                                        unsigned long long *__restrict__ status) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    bool beyond = false;
    if (v < nviews) {
        const bool entry = (uint64_t)view_entry[v] < (uint64_t)LB_MAX_ENTRIES;
        const int pos = view_pos[v];
        const bool ok = entry && pos >= 0 && pos < words * 64;
        beyond = entry && !ok;
        view_local[v] = ok ? pos : -1;
        c_keep[v] = (ok && keep[v] != 0) ? 1 : 0;
    }
    const int nb = __popcll(__ballot(beyond));
    if (gp_lane() == 0 && nb) atomicAdd(status + LMS_BEYOND, (unsigned long long)nb);
}

// One thread per record e of view pv = the view whose [voff[pv], voff[pv+1]) holds e.  The record takes part when its view is kept and
// has a position, its row is a row of pv's batch entry and above the row of the record before it in the view (so a point occurs once
// in a view); its segment is forced into -1..Q-1.  Otherwise it is counted and its copy is (point 0, not live): in range everywhere,
// it sets no bit and takes no slot.
__global__ void __launch_bounds__(256) lms_records_kernel(const double *__restrict__ points, int64_t n, const int64_t *__restrict__ view_entry,
                                                          const uint8_t *__restrict__ c_keep, const int64_t *__restrict__ voff, int nviews, int q,
                                                          const int32_t *__restrict__ rec_row, const int32_t *__restrict__ rec_seg, int64_t total,
                                                          int64_t *__restrict__ c_pt, int32_t *__restrict__ c_view, int32_t *__restrict__ c_seg,
                                                          uint8_t *__restrict__ c_live, unsigned long long *__restrict__ status) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int nbad = 0;
    if (e < total) {
        int lo = 0, hi = nviews - 1;                                 // the last view whose first record is <= e (voff ascends from 0 to total)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (voff[mid] <= e) lo = mid; else hi = mid - 1;
        }
        const int pv = lo;
        const int64_t row = rec_row[e];
        int sg = rec_seg[e];
        bool ok = c_keep[pv] != 0 && (uint64_t)row < (uint64_t)n;    // (c_keep: view_entry[pv] is an entry)
        if (ok) ok = lb_entry_of(points[row * 4]) == (int)view_entry[pv];
        if (ok && e > voff[pv]) ok = (int64_t)rec_row[e - 1] < row;
        if (sg < -1 || sg >= q) {
            sg = -1;
            ++nbad;
        }
        nbad += ok ? 0 : 1;
        c_pt[e] = ok ? row : 0;
        c_view[e] = pv;
        c_seg[e] = sg;
        c_live[e] = ok ? 1 : 0;
    }
    nbad = gp_wave_sum_i(nbad);
    if (gp_lane() == 0 && nbad) atomicAdd(status + LMS_BAD, (unsigned long long)nbad);
}

}  // namespace

extern "C" size_t gp_lift_masks_stream_state_bytes(int64_t n) { return lb_n_ok(n) ? lms_state_bytes(n) : 0; }

extern "C" size_t gp_lift_masks_stream_begin_workspace_bytes(int64_t n) { return lb_n_ok(n) ? ls_begin_workspace_bytes(n) : 0; }

extern "C" int gp_lift_masks_stream_begin(const double *points, int64_t n, void *state, size_t state_bytes, int64_t *status, void *workspace,
                                          size_t workspace_bytes, void *stream_) {
    const char *who = "gp_lift_masks_stream_begin";
    GP_CHECK_ARG(points && state && status && workspace, "%s: null argument", who);
    LB_TRY(lb_check_n(who, n));
    LB_TRY(lb_check_state(who, state_bytes, lms_state_bytes(n)));
    {
        const void *const in[] = {points};
        const size_t in_bytes[] = {(size_t)n * 32};
        const void *const o[] = {state, status, workspace};
        const size_t o_bytes[] = {state_bytes, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver sv(state, state_bytes), cv(workspace, workspace_bytes);
    LmsState st(sv, n);
    LsBeginWork k(cv, n);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    GP_CHECK_HIP(hipMemsetAsync(st.views, 0, (size_t)LB_MAX_ENTRIES * sizeof(int32_t), s));
    return ls_begin_tables(points, n, st.tables, k, status, s);
}

extern "C" size_t gp_lift_masks_stream_sizes_workspace_bytes(int32_t nviews) {
    if (!lb_nviews_ok(nviews)) return 0;
    GpCarver cv(nullptr, 0);
    LmsSizesWork k(cv, nviews);
    return cv.off;
}

extern "C" int gp_lift_masks_stream_sizes(int64_t n, const void *state, size_t state_bytes, const int64_t *status, const int64_t *view_entry,
                                          const int64_t *view_count, const uint8_t *view_keep, int32_t nviews, int64_t *sizes, void *workspace,
                                          size_t workspace_bytes, void *stream_) {
    const char *who = "gp_lift_masks_stream_sizes";
    GP_CHECK_ARG(state && status && view_entry && view_count && view_keep && sizes && workspace, "%s: null argument", who);
    LB_TRY(lb_check_n(who, n));
    LB_TRY(lb_check_nviews(who, nviews));
    LB_TRY(lb_check_state(who, state_bytes, lms_state_bytes(n)));
    {
        // (this entry point holds both outputs against the inputs before it holds them against each other)
        const void *const in[] = {state, status, view_entry, view_count, view_keep};
        const size_t in_bytes[] = {state_bytes, (size_t)ST_WORDS * 8, (size_t)nviews * 8, (size_t)nviews * 8, (size_t)nviews};
        const void *const o[] = {sizes, workspace};
        const size_t o_bytes[] = {4 * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, 5, o, o_bytes, 1));
        LB_TRY(lb_no_overlap(who, in, in_bytes, 5, o + 1, o_bytes + 1, 1));
        LB_TRY(lb_no_overlap(who, in, in_bytes, 0, o, o_bytes, 2));
    }
    GpCarver sv(const_cast<void *>(state), state_bytes), cv(workspace, workspace_bytes);
    const LmsState st(sv, n);
    LmsSizesWork k(cv, nviews);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *sz = reinterpret_cast<unsigned long long *>(sizes);
    GP_CHECK_HIP(hipMemsetAsync(sizes, 0, 4 * sizeof(int64_t), s));
    GP_CHECK_HIP(hipMemsetAsync(k.scratch, 0, ST_WORDS * sizeof(int64_t), s));
    LB_TRY(lb_view_table(view_entry, nviews, k.t, k.tmp, k.tmp_bytes, k.scratch, s));
    lms_totals_kernel<<<(unsigned)((nviews + 255) / 256), 256, 0, s>>>(view_count, view_keep, nviews, sz);
    lms_most_kernel<<<LB_MAX_ENTRIES / 256, 256, 0, s>>>(k.t.off, st.views, status, sz);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" size_t gp_lift_masks_stream_add_workspace_bytes_t(int32_t elem, int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w, int32_t out_h,
                                                             int32_t out_w, int64_t total, int64_t fill_cap) {
    if (!gp_elem_ok(elem)) return 0;
    if (!lb_n_ok(n) || !lb_nviews_ok(nviews) || q < 1 || q > 1024 || h < 1 || w < 1 || out_h < 1 || out_w < 1 || total < 0 ||
        total >= (int64_t)INT32_MAX || fill_cap < 0 || fill_cap > total)
        return 0;
    GpCarver cv(nullptr, 0);
    LmsAddWork k(cv, n, nviews, q, h, w, out_h, out_w, total, fill_cap ? fill_cap : total, gp_elem_size(elem));
    return cv.off;
}

extern "C" size_t gp_lift_masks_stream_add_workspace_bytes(int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w, int32_t out_h, int32_t out_w,
                                                           int64_t total, int64_t fill_cap) {
    return gp_lift_masks_stream_add_workspace_bytes_t(GP_ELEM_F32, n, nviews, q, h, w, out_h, out_w, total, fill_cap);
}

extern "C" int gp_lift_masks_stream_add_t(const double *points, int64_t n, void *state, size_t state_bytes, const int64_t *view_entry,
                                          int32_t nviews, const void *pred_masks, int32_t elem, int32_t q, int32_t h, int32_t w, const float *scores,
                                          const int32_t *tap_x0, const float *tap_wx, const int32_t *tap_y0, const float *tap_wy, int32_t out_h,
                                          int32_t out_w, const int64_t *ent_pt, const int64_t *ent_x, const int64_t *ent_y, const int32_t *ent_view,
                                          const int64_t *view_off, const uint8_t *keep, int64_t total, int64_t fill_cap, int32_t *rec_row,
                                          int32_t *rec_seg, int64_t rec_base, int64_t rec_cap, int64_t *rec_off, int32_t *view_pos, int64_t *status,
                                          void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "gp_lift_masks_stream_add";
    GP_CHECK_ARG(points && state && view_entry && view_off && keep && rec_off && view_pos && status && workspace, "%s: null argument", who);
    LB_TRY(lb_check_elem(who, elem, pred_masks, "masks"));
    LB_TRY(lb_check_n(who, n));
    LB_TRY(lb_check_nviews(who, nviews));
    GP_CHECK_ARG(total >= 0 && total < (int64_t)INT32_MAX, "%s: %lld entries outside 0..2^31-2", who, (long long)total);
    GP_CHECK_ARG(total == 0 || (pred_masks && scores && tap_x0 && tap_wx && tap_y0 && tap_wy && ent_pt && ent_x && ent_y && ent_view && rec_row && rec_seg),
                 "%s: %lld entries need the masks, the scores, the taps, the entry arrays and the records", who, (long long)total);
    LB_TRY(lmb_check_masks(who, q, h, w, out_h, out_w));
    LB_TRY(lmb_check_fill_cap(who, fill_cap, total));
    GP_CHECK_ARG(rec_base >= 0 && rec_cap >= rec_base && rec_cap < (int64_t)INT32_MAX, "%s: records %lld of a capacity of %lld (at most 2^31-2)", who,
                 (long long)rec_base, (long long)rec_cap);
    LB_TRY(lb_check_state(who, state_bytes, lms_state_bytes(n)));
    if (fill_cap == 0) fill_cap = total;
    {
        const size_t vq = (size_t)nviews * q;
        const void *const in[] = {points, view_entry, pred_masks, scores, tap_x0, tap_wx, tap_y0, tap_wy, ent_pt, ent_x, ent_y, ent_view, view_off,
                                  keep};
        const size_t in_bytes[] = {(size_t)n * 32, (size_t)nviews * 8, vq * h * w * gp_elem_size(elem), vq * 4, (size_t)out_w * 4, (size_t)out_w * 16, (size_t)out_h * 4,
                                   (size_t)out_h * 16, (size_t)total * 8, (size_t)total * 8, (size_t)total * 8, (size_t)total * 4,
                                   ((size_t)nviews + 1) * 8, (size_t)nviews};
        const void *const o[] = {state, rec_row, rec_seg, rec_off, view_pos, status, workspace};
        const size_t o_bytes[] = {state_bytes, (size_t)rec_cap * 4, (size_t)rec_cap * 4, ((size_t)nviews + 1) * 8, (size_t)nviews * 4,
                                  (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver sv(state, state_bytes), cv(workspace, workspace_bytes);
    LmsState st(sv, n);
    LmsAddWork k(cv, n, nviews, q, h, w, out_h, out_w, total, fill_cap, gp_elem_size(elem));
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *su = reinterpret_cast<unsigned long long *>(status);
    // the chunk's view table (its bad entries join the running count), the views' positions inside their entries, the counters
    LB_TRY(lb_view_table(view_entry, nviews, k.t, k.tmp, k.tmp_bytes, su, s));
    GP_CHECK_HIP(hipMemsetAsync(view_pos, 0xff, (size_t)nviews * sizeof(int32_t), s));
    lms_positions_kernel<<<LB_MAX_ENTRIES * 64 / 256, 256, 0, s>>>(k.t.idx, k.t.off, nviews, st.views, view_pos, su);
    GP_CHECK_LAUNCH();
    if (total == 0) {
        lms_rec_off_kernel<<<1, 64, 0, s>>>(k.e.voff, k.e.c_keep, nviews, 1, rec_base, k.loc, rec_off, su);
        GP_CHECK_LAUNCH();
        return GP_OK;
    }
    // the pipeline of gp_lift_masks_batched over the chunk (a view's position is its view_local): the entries, checked; the segment
    // of every entry; the in-view fill
    LB_TRY(lmb_chunk_segments(points, n, view_entry, view_pos, nviews, pred_masks, elem, q, h, w, scores, tap_x0, tap_wx, tap_y0, tap_wy, out_h, out_w,
                              ent_pt, ent_x, ent_y, ent_view, view_off, keep, total, fill_cap, k.e, k.k, k.tmp, k.tmp_bytes, k.seg, su, s));
    // the records of the kept views
    lms_rec_off_kernel<<<1, 64, 0, s>>>(k.e.voff, k.e.c_keep, nviews, 0, rec_base, k.loc, rec_off, su);
    lms_append_kernel<<<(unsigned)((total + 1 + 255) / 256), 256, 0, s>>>(k.e.c_pt, k.e.c_view, k.e.c_live, k.e.c_keep, k.e.voff, k.loc, k.seg, total,
                                                                         rec_base, rec_cap, rec_row, rec_seg);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_lift_masks_stream_add(const double *points, int64_t n, void *state, size_t state_bytes, const int64_t *view_entry, int32_t nviews,
                                        const float *pred_masks, int32_t q, int32_t h, int32_t w, const float *scores, const int32_t *tap_x0,
                                        const float *tap_wx, const int32_t *tap_y0, const float *tap_wy, int32_t out_h, int32_t out_w,
                                        const int64_t *ent_pt, const int64_t *ent_x, const int64_t *ent_y, const int32_t *ent_view,
                                        const int64_t *view_off, const uint8_t *keep, int64_t total, int64_t fill_cap, int32_t *rec_row,
                                        int32_t *rec_seg, int64_t rec_base, int64_t rec_cap, int64_t *rec_off, int32_t *view_pos, int64_t *status,
                                        void *workspace, size_t workspace_bytes, void *stream_) {
    return gp_lift_masks_stream_add_t(points, n, state, state_bytes, view_entry, nviews, pred_masks, GP_ELEM_F32, q, h, w, scores, tap_x0, tap_wx,
                                      tap_y0, tap_wy, out_h, out_w, ent_pt, ent_x, ent_y, ent_view, view_off, keep, total, fill_cap, rec_row, rec_seg,
                                      rec_base, rec_cap, rec_off, view_pos, status, workspace, workspace_bytes, stream_);
}

extern "C" size_t gp_lift_masks_stream_finish_workspace_bytes(int64_t n, int32_t nviews, int64_t total, int32_t words) {
    if (!lb_n_ok(n) || !lb_nviews_ok(nviews) || total < 1 || total >= (int64_t)INT32_MAX || words < 1 || words > 1024) return 0;
    GpCarver cv(nullptr, 0);
    LmsFinishWork k(cv, n, nviews, total, words);
    return cv.off;
}

extern "C" int gp_lift_masks_stream_finish(const double *points, int64_t n, const void *state, size_t state_bytes, const int64_t *view_entry,
                                           const int32_t *view_pos, const uint8_t *view_keep, const int64_t *rec_off, int32_t nviews,
                                           const int32_t *rec_row, const int32_t *rec_seg, int64_t total, int32_t words, const float *f_seg,
                                           const float *logit_seg, int32_t q, int32_t d, int32_t c, const int64_t *status, int32_t fill, float *out,
                                           int64_t ld_out, uint8_t *seen, int32_t *count, int64_t *nn, int64_t *status_out, void *workspace,
                                           size_t workspace_bytes, void *stream_) {
    const char *who = "gp_lift_masks_stream_finish";
    GP_CHECK_ARG(points && state && view_entry && view_pos && view_keep && rec_off && rec_row && rec_seg && f_seg && logit_seg && status && out &&
                     seen && count && status_out && workspace,
                 "%s: null argument", who);
    LB_TRY(lb_check_n(who, n));
    LB_TRY(lb_check_nviews(who, nviews));
    GP_CHECK_ARG(q >= 1 && q <= 1024, "%s: %d queries outside 1..1024", who, q);
    GP_CHECK_ARG(total >= 1 && total < (int64_t)INT32_MAX, "%s: %lld records outside 1..2^31-2", who, (long long)total);
    LB_TRY(lmb_check_words(who, words));
    LB_TRY(lmb_check_fused(who, d, c, ld_out, f_seg, out, fill, nn));
    LB_TRY(lb_check_state(who, state_bytes, lms_state_bytes(n)));
    {
        const size_t vq = (size_t)nviews * q;
        const void *const in[] = {points, state, view_entry, view_pos, view_keep, rec_off, rec_row, rec_seg, f_seg, logit_seg, status};
        const size_t in_bytes[] = {(size_t)n * 32,     state_bytes,        (size_t)nviews * 8, (size_t)nviews * 4, (size_t)nviews, ((size_t)nviews + 1) * 8,
                                   (size_t)total * 4, (size_t)total * 4, vq * d * 4,         vq * c * 4,         (size_t)ST_WORDS * 8};
        const void *const o[] = {out, seen, count, nn, status_out, workspace};
        const size_t o_bytes[] = {(size_t)((n - 1) * ld_out + d) * 4, (size_t)n, (size_t)n * 4, (size_t)n * 8, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver sv(const_cast<void *>(state), state_bytes), cv(workspace, workspace_bytes);
    const LmsState st(sv, n);
    LmsFinishWork k(cv, n, nviews, total, words);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *so = reinterpret_cast<unsigned long long *>(status_out);
    // everything kept between the calls, checked; beside the words of every stream, this one carries what add had to change or leave out
    LB_TRY(ls_checked_tables(st.tables, n, k.base.tables, status, LS_CARRY | (1u << LMS_BAD) | (1u << LMS_BEYOND), status_out, s));
    lmb_view_off_kernel<<<1, 64, 0, s>>>(rec_off, nviews, total, k.voff, so);
    lms_views_kernel<<<(unsigned)((nviews + 255) / 256), 256, 0, s>>>(view_entry, view_pos, view_keep, nviews, words, k.view_local, k.c_keep, so);
    lms_records_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(points, n, view_entry, k.c_keep, k.voff, nviews, q, rec_row, rec_seg, total,
                                                                      k.c_pt, k.c_view, k.c_seg, k.c_live, so);
    GP_CHECK_LAUNCH();
    // the end of gp_lift_masks_batched over the records and the checked copies of the tables: point -> (view, segment) lists in ascending
    // position inside the entry, consensus top-3 fusion, the scene-level fill inside every entry
    return lmb_fuse_fill(points, n, k.c_pt, k.c_view, k.c_live, k.view_local, k.c_seg, total, words, k.l, k.base.tables.keys, k.base.tables.rows,
                         k.base.tables.off, k.base.fill, k.base.tmp, k.base.tmp_bytes, f_seg, logit_seg, q, d, c, fill, out, ld_out, seen, count, nn,
                         so, stream_);
}
