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
#include "gp_lift_stream_state.h"
#include "gp_lift_masks_entries.h"
#include "gp_lift_masks.h"

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

struct LmsViewTable {                                            // a chunk's views sorted stably by entry
    uint32_t *vk0, *vk1;
    int32_t *w0, *entry_views, *view_off;
    LmsViewTable(GpCarver &cv, int32_t nviews) {
        vk0 = cv.take<uint32_t>(nviews);
        vk1 = cv.take<uint32_t>(nviews);
        w0 = cv.take<int32_t>(nviews);
        entry_views = cv.take<int32_t>(nviews);
        view_off = cv.take<int32_t>(LB_TABLE);
    }
};

int lms_view_table(const int64_t *view_entry, int32_t nviews, const LmsViewTable &t, char *tmp, size_t tmp_bytes, unsigned long long *st,
                   hipStream_t s) {
    lb_view_keys_kernel<<<(unsigned)((nviews + 255) / 256), 256, 0, s>>>(view_entry, nviews, t.vk0, t.w0, st);
    GP_CHECK_LAUNCH();
    size_t io = tmp_bytes;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(tmp, io, t.vk0, t.vk1, t.w0, t.entry_views, (size_t)nviews, 0, LB_KEY_BITS, s));    // (stable)
    lb_offsets_kernel<<<(LB_TABLE + 255) / 256, 256, 0, s>>>(t.vk1, nviews, t.view_off);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

struct LmsSizesWork {
    LmsViewTable t;
    unsigned long long *scratch;                                 // the status words of the table's keys kernel: counted by add, not here
    char *tmp;
    size_t tmp_bytes;
    LmsSizesWork(GpCarver &cv, int32_t nviews) : t(cv, nviews) {
        tmp_bytes = lb_sort_bytes(nviews);
        scratch = cv.take<unsigned long long>(ST_WORDS);
        tmp = cv.take<char>(tmp_bytes);
    }
};

struct LmsAddWork {
    LmsViewTable t;
    // the checked entries
    int32_t *c_view = nullptr, *cx0 = nullptr, *cy0 = nullptr;
    int64_t *voff, *loc, *c_pt = nullptr, *c_x = nullptr, *c_y = nullptr;
    uint8_t *c_live = nullptr, *c_keep;
    float *xyz = nullptr;
    // the segment decision and the in-view fill (as LmbWork)
    void *mt = nullptr;                                          // (the rank-ordered transposed masks, in the masks' own element type)
    float *sscore = nullptr, *f_rxyz = nullptr;
    int32_t *order = nullptr, *seg = nullptr, *cov = nullptr, *f_rs = nullptr, *rent = nullptr, *qent = nullptr, *part_i = nullptr;
    double *part_d = nullptr;
    int4 *tab = nullptr;
    char *tmp;
    size_t tmp_bytes;
    LmsAddWork(GpCarver &cv, int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w, int32_t out_h, int32_t out_w, int64_t total,
               int64_t fill_cap, size_t esize)
        : t(cv, nviews) {
        const size_t a = lb_sort_bytes(nviews), b = lb_scan_bytes(total + 1);
        tmp_bytes = a > b ? a : b;
        voff = cv.take<int64_t>((size_t)nviews + 1);
        loc = cv.take<int64_t>((size_t)nviews + 1);
        c_keep = cv.take<uint8_t>(nviews);
        if (total > 0) {                                         // (a chunk in which nothing is visible needs the view table alone)
            c_pt = cv.take<int64_t>(total);
            c_x = cv.take<int64_t>(total);
            c_y = cv.take<int64_t>(total);
            c_view = cv.take<int32_t>(total);
            c_live = cv.take<uint8_t>(total);
            cx0 = cv.take<int32_t>(out_w);
            cy0 = cv.take<int32_t>(out_h);
            xyz = cv.take<float>(3 * n);
            mt = cv.take<char>((size_t)nviews * q * h * w * esize);
            order = cv.take<int32_t>((size_t)nviews * q);
            sscore = cv.take<float>((size_t)nviews * q);
            seg = cv.take<int32_t>(total);
            cov = cv.take<int32_t>(total + 1);
            f_rs = cv.take<int32_t>(total + 1);
            rent = cv.take<int32_t>(total);
            qent = cv.take<int32_t>(total);
            f_rxyz = cv.take<float>(total * 3);
            part_d = cv.take<double>((size_t)FV_CHUNKS * fill_cap);
            part_i = cv.take<int32_t>((size_t)FV_CHUNKS * fill_cap);
            tab = cv.take<int4>((size_t)nviews + 1);
        }
        tmp = cv.take<char>(tmp_bytes);
    }
};

struct LmsFinishWork {
    // the checked entry tables and the scene-level fill (as LsFinishWork)
    uint32_t *keys;
    int32_t *rows, *off, *ref, *qry, *rs, *qs, *rrow, *qpos;
    float *rxyz;
    // the checked per-view arrays and records
    int32_t *view_local, *c_view, *c_seg;
    int64_t *voff, *c_pt;
    uint8_t *c_live, *c_keep;
    // the point -> (view, segment) lists
    unsigned long long *vmask;
    int64_t *cnt, *pv_start;
    int32_t *pv_view, *pv_seg;
    char *tmp;
    size_t tmp_bytes;
    LmsFinishWork(GpCarver &cv, int64_t n, int32_t nviews, int64_t total, int32_t words) {
        const size_t a = lb_scan_bytes(n + 1), b = lmb_scan64_bytes(n + 1);
        tmp_bytes = a > b ? a : b;
        keys = cv.take<uint32_t>(n);
        rows = cv.take<int32_t>(n);
        off = cv.take<int32_t>(LB_TABLE);
        ref = cv.take<int32_t>(n + 1);
        qry = cv.take<int32_t>(n + 1);
        rs = cv.take<int32_t>(n + 1);
        qs = cv.take<int32_t>(n + 1);
        rrow = cv.take<int32_t>(n);
        qpos = cv.take<int32_t>(n);
        rxyz = cv.take<float>(3 * n);
        view_local = cv.take<int32_t>(nviews);
        c_keep = cv.take<uint8_t>(nviews);
        voff = cv.take<int64_t>((size_t)nviews + 1);
        c_pt = cv.take<int64_t>(total);
        c_view = cv.take<int32_t>(total);
        c_seg = cv.take<int32_t>(total);
        c_live = cv.take<uint8_t>(total);
        vmask = cv.take<unsigned long long>((size_t)n * words);
        cnt = cv.take<int64_t>(n + 1);
        pv_start = cv.take<int64_t>(n + 1);
        pv_view = cv.take<int32_t>(total);
        pv_seg = cv.take<int32_t>(total);
        tmp = cv.take<char>(tmp_bytes);
    }
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
__global__ void lms_status_kernel(const int64_t *__restrict__ running, int64_t *__restrict__ status_out) {
    const int i = threadIdx.x;
    if (i < ST_WORDS) status_out[i] = (i <= ST_TOP_BATCH || i == LMS_BAD || i == LMS_BEYOND) ? running[i] : 0;
}

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

bool lms_chunk_ok(int32_t nviews) { return nviews >= 1 && nviews <= 65535; }

}  // namespace

extern "C" size_t gp_lift_masks_stream_state_bytes(int64_t n) { return ls_n_ok(n) ? lms_state_bytes(n) : 0; }

extern "C" size_t gp_lift_masks_stream_begin_workspace_bytes(int64_t n) {
    if (!ls_n_ok(n)) return 0;
    GpCarver cv(nullptr, 0);
    LsBeginWork k(cv, n);
    return cv.off;
}

extern "C" int gp_lift_masks_stream_begin(const double *points, int64_t n, void *state, size_t state_bytes, int64_t *status, void *workspace,
                                          size_t workspace_bytes, void *stream_) {
    GP_CHECK_ARG(points && state && status && workspace, "gp_lift_masks_stream_begin: null argument");
    GP_CHECK_ARG(ls_n_ok(n), "gp_lift_masks_stream_begin: n=%lld outside 1..2^31-1", (long long)n);
    GP_CHECK_ARG(state_bytes >= lms_state_bytes(n), "gp_lift_masks_stream_begin: state too small (%zu < %zu)", state_bytes, lms_state_bytes(n));
    {
        const void *o[] = {state, status, workspace};
        const size_t o_bytes[] = {state_bytes, (size_t)ST_WORDS * 8, workspace_bytes};
        for (int a = 0; a < 3; ++a) {
            GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], points, (size_t)n * 32), "gp_lift_masks_stream_begin: an output overlaps an input");
            for (int b = a + 1; b < 3; ++b)
                GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], o[b], o_bytes[b]), "gp_lift_masks_stream_begin: two outputs overlap");
        }
    }
    GpCarver sv(state, state_bytes), cv(workspace, workspace_bytes);
    LmsState st(sv, n);
    LsBeginWork k(cv, n);
    if (!cv.ok()) {
        gp_set_error("gp_lift_masks_stream_begin: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    GP_CHECK_HIP(hipMemsetAsync(st.views, 0, (size_t)LB_MAX_ENTRIES * sizeof(int32_t), s));
    lb_row_keys_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(points, n, k.k0, k.r0, reinterpret_cast<unsigned long long *>(status));
    GP_CHECK_LAUNCH();
    size_t io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(k.tmp, io, k.k0, st.tables.keys, k.r0, st.tables.rows, (size_t)n, 0, LB_KEY_BITS, s));   // (stable)
    lb_offsets_kernel<<<(LB_TABLE + 255) / 256, 256, 0, s>>>(st.tables.keys, n, st.tables.off);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" size_t gp_lift_masks_stream_sizes_workspace_bytes(int32_t nviews) {
    if (!lms_chunk_ok(nviews)) return 0;
    GpCarver cv(nullptr, 0);
    LmsSizesWork k(cv, nviews);
    return cv.off;
}

extern "C" int gp_lift_masks_stream_sizes(int64_t n, const void *state, size_t state_bytes, const int64_t *status, const int64_t *view_entry,
                                          const int64_t *view_count, const uint8_t *view_keep, int32_t nviews, int64_t *sizes, void *workspace,
                                          size_t workspace_bytes, void *stream_) {
    GP_CHECK_ARG(state && status && view_entry && view_count && view_keep && sizes && workspace, "gp_lift_masks_stream_sizes: null argument");
    GP_CHECK_ARG(ls_n_ok(n), "gp_lift_masks_stream_sizes: n=%lld outside 1..2^31-1", (long long)n);
    GP_CHECK_ARG(lms_chunk_ok(nviews), "gp_lift_masks_stream_sizes: %d views outside 1..65535", nviews);
    GP_CHECK_ARG(state_bytes >= lms_state_bytes(n), "gp_lift_masks_stream_sizes: state too small (%zu < %zu)", state_bytes, lms_state_bytes(n));
    {
        const void *in[] = {state, status, view_entry, view_count, view_keep};
        const size_t in_bytes[] = {state_bytes, (size_t)ST_WORDS * 8, (size_t)nviews * 8, (size_t)nviews * 8, (size_t)nviews};
        const void *o[] = {sizes, workspace};
        const size_t o_bytes[] = {4 * 8, workspace_bytes};
        for (int a = 0; a < 2; ++a)
            for (int i = 0; i < 5; ++i)
                GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], in[i], in_bytes[i]), "gp_lift_masks_stream_sizes: an output overlaps an input");
        GP_CHECK_ARG(!lb_overlap(o[0], o_bytes[0], o[1], o_bytes[1]), "gp_lift_masks_stream_sizes: two outputs overlap");
    }
    GpCarver sv(const_cast<void *>(state), state_bytes), cv(workspace, workspace_bytes);
    const LmsState st(sv, n);
    LmsSizesWork k(cv, nviews);
    if (!cv.ok()) {
        gp_set_error("gp_lift_masks_stream_sizes: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *sz = reinterpret_cast<unsigned long long *>(sizes);
    GP_CHECK_HIP(hipMemsetAsync(sizes, 0, 4 * sizeof(int64_t), s));
    GP_CHECK_HIP(hipMemsetAsync(k.scratch, 0, ST_WORDS * sizeof(int64_t), s));
    int rc = lms_view_table(view_entry, nviews, k.t, k.tmp, k.tmp_bytes, k.scratch, s);
    if (rc != GP_OK) return rc;
    lms_totals_kernel<<<(unsigned)((nviews + 255) / 256), 256, 0, s>>>(view_count, view_keep, nviews, sz);
    lms_most_kernel<<<LB_MAX_ENTRIES / 256, 256, 0, s>>>(k.t.view_off, st.views, status, sz);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" size_t gp_lift_masks_stream_add_workspace_bytes_t(int32_t elem, int64_t n, int32_t nviews, int32_t q, int32_t h, int32_t w, int32_t out_h,
                                                             int32_t out_w, int64_t total, int64_t fill_cap) {
    if (!gp_elem_ok(elem)) return 0;
    if (!ls_n_ok(n) || !lms_chunk_ok(nviews) || q < 1 || q > 1024 || h < 1 || w < 1 || out_h < 1 || out_w < 1 || total < 0 ||
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
    GP_CHECK_ARG(points && state && view_entry && view_off && keep && rec_off && view_pos && status && workspace,
                 "gp_lift_masks_stream_add: null argument");
    GP_CHECK_ARG(gp_elem_ok(elem), "gp_lift_masks_stream_add: element type %d (0 fp32, 1 fp16, 2 bf16)", elem);
    GP_CHECK_ARG(elem == GP_ELEM_F32 || (uintptr_t)pred_masks % 2 == 0, "gp_lift_masks_stream_add: half masks at an odd address");
    GP_CHECK_ARG(ls_n_ok(n), "gp_lift_masks_stream_add: n=%lld outside 1..2^31-1", (long long)n);
    GP_CHECK_ARG(lms_chunk_ok(nviews), "gp_lift_masks_stream_add: %d views outside 1..65535", nviews);
    GP_CHECK_ARG(total >= 0 && total < (int64_t)INT32_MAX, "gp_lift_masks_stream_add: %lld entries outside 0..2^31-2", (long long)total);
    GP_CHECK_ARG(total == 0 || (pred_masks && scores && tap_x0 && tap_wx && tap_y0 && tap_wy && ent_pt && ent_x && ent_y && ent_view && rec_row && rec_seg),
                 "gp_lift_masks_stream_add: %lld entries need the masks, the scores, the taps, the entry arrays and the records", (long long)total);
    GP_CHECK_ARG(q >= 1 && q <= 1024, "gp_lift_masks_stream_add: %d queries outside 1..1024 (the score sort holds 1024)", q);
    GP_CHECK_ARG(h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1 && (int64_t)h * w < (1ll << 31), "gp_lift_masks_stream_add: masks %d x %d, image %d x %d",
                 h, w, out_h, out_w);
    GP_CHECK_ARG(fill_cap >= 0 && fill_cap <= total, "gp_lift_masks_stream_add: fill_cap=%lld outside 0..total", (long long)fill_cap);
    GP_CHECK_ARG(rec_base >= 0 && rec_cap >= rec_base && rec_cap < (int64_t)INT32_MAX,
                 "gp_lift_masks_stream_add: records %lld of a capacity of %lld (at most 2^31-2)", (long long)rec_base, (long long)rec_cap);
    GP_CHECK_ARG(state_bytes >= lms_state_bytes(n), "gp_lift_masks_stream_add: state too small (%zu < %zu)", state_bytes, lms_state_bytes(n));
    if (fill_cap == 0) fill_cap = total;
    {
        const size_t vq = (size_t)nviews * q;
        const void *in[] = {points, view_entry, pred_masks, scores, tap_x0, tap_wx, tap_y0, tap_wy, ent_pt, ent_x, ent_y, ent_view, view_off, keep};
        const size_t in_bytes[] = {(size_t)n * 32, (size_t)nviews * 8, vq * h * w * gp_elem_size(elem), vq * 4, (size_t)out_w * 4, (size_t)out_w * 16, (size_t)out_h * 4,
                                   (size_t)out_h * 16, (size_t)total * 8, (size_t)total * 8, (size_t)total * 8, (size_t)total * 4,
                                   ((size_t)nviews + 1) * 8, (size_t)nviews};
        const void *o[] = {state, rec_row, rec_seg, rec_off, view_pos, status, workspace};
        const size_t o_bytes[] = {state_bytes, (size_t)rec_cap * 4, (size_t)rec_cap * 4, ((size_t)nviews + 1) * 8, (size_t)nviews * 4,
                                  (size_t)ST_WORDS * 8, workspace_bytes};
        for (int a = 0; a < 7; ++a) {
            for (int i = 0; i < 14; ++i)
                GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], in[i], in_bytes[i]), "gp_lift_masks_stream_add: an output overlaps an input");
            for (int b = a + 1; b < 7; ++b) GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], o[b], o_bytes[b]), "gp_lift_masks_stream_add: two outputs overlap");
        }
    }
    GpCarver sv(state, state_bytes), cv(workspace, workspace_bytes);
    LmsState st(sv, n);
    LmsAddWork k(cv, n, nviews, q, h, w, out_h, out_w, total, fill_cap, gp_elem_size(elem));
    if (!cv.ok()) {
        gp_set_error("gp_lift_masks_stream_add: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *su = reinterpret_cast<unsigned long long *>(status);
    // the chunk's view table (its bad entries join the running count), the views' positions inside their entries, the counters
    int rc = lms_view_table(view_entry, nviews, k.t, k.tmp, k.tmp_bytes, su, s);
    if (rc != GP_OK) return rc;
    GP_CHECK_HIP(hipMemsetAsync(view_pos, 0xff, (size_t)nviews * sizeof(int32_t), s));
    lms_positions_kernel<<<LB_MAX_ENTRIES * 64 / 256, 256, 0, s>>>(k.t.entry_views, k.t.view_off, nviews, st.views, view_pos, su);
    GP_CHECK_LAUNCH();
    if (total == 0) {
        lms_rec_off_kernel<<<1, 64, 0, s>>>(k.voff, k.c_keep, nviews, 1, rec_base, k.loc, rec_off, su);
        GP_CHECK_LAUNCH();
        return GP_OK;
    }
    const unsigned nb = (unsigned)((n + 255) / 256), vb = (unsigned)((nviews + 255) / 256), eb = (unsigned)((total + 1 + 255) / 256);
    // the entries, checked (the kernels and the order of gp_lift_masks_batched; a view's position is its view_local)
    lmb_xyz_kernel<<<nb, 256, 0, s>>>(points, n, k.xyz);
    lmb_view_off_kernel<<<1, 64, 0, s>>>(view_off, nviews, total, k.voff, su);
    lmb_taps_kernel<<<(unsigned)((out_w + out_h + 255) / 256), 256, 0, s>>>(tap_x0, tap_y0, out_w, out_h, w, h, k.cx0, k.cy0, su);
    lmb_entries_kernel<<<eb, 256, 0, s>>>(points, n, view_entry, view_pos, k.voff, nviews, out_h, out_w, ent_pt, ent_x, ent_y, ent_view, keep, total,
                                          k.c_pt, k.c_x, k.c_y, k.c_view, k.c_live, su);
    lmb_keep_kernel<<<vb, 256, 0, s>>>(keep, view_pos, nviews, k.c_keep);
    GP_CHECK_LAUNCH();
    // the segment of every entry
    const int64_t hw = (int64_t)h * w;
    lv_sort_scores_kernel<<<nviews, 256, 0, s>>>(scores, q, k.order, k.sscore);
    const dim3 tg((unsigned)((hw + 63) / 64), (unsigned)((q + 63) / 64), (unsigned)nviews);
    const unsigned sb = (unsigned)((total * 64 + 255) / 256);
#define LMS_SEGMENTS(T, BITS)                                                                                                                  \
    do {                                                                                                                                       \
        transpose_views_kernel<BITS><<<tg, 256, 0, s>>>(static_cast<const BITS *>(pred_masks), q, (int)hw, static_cast<BITS *>(k.mt), k.order);   \
        lift_masks_views_kernel<T><<<sb, 256, 0, s>>>(static_cast<const T *>(k.mt), q, h, w, k.sscore, k.order, k.cx0, tap_wx, k.cy0, tap_wy,    \
                                                      out_h, out_w, k.c_x, k.c_y, k.c_view, k.c_keep, total, k.seg);                           \
    } while (0)
    if (elem == GP_ELEM_F32) LMS_SEGMENTS(float, float);
    else if (elem == GP_ELEM_F16) LMS_SEGMENTS(gp_f16, uint16_t);
    else LMS_SEGMENTS(gp_bf16, uint16_t);
#undef LMS_SEGMENTS
    GP_CHECK_LAUNCH();
    // the in-view fill
    fill_flags_kernel<<<eb, 256, 0, s>>>(k.seg, total, k.cov);
    size_t tb = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, tb, k.cov, k.f_rs, (int32_t)0, (size_t)(total + 1), rocprim::plus<int32_t>(), s));
    fill_compact_kernel<<<eb, 256, 0, s>>>(k.xyz, k.c_pt, k.seg, k.f_rs, total, k.f_rxyz, k.rent, k.qent);
    const unsigned qb = (unsigned)(total / 256 + nviews + 1);                            // >= sum over views of ceil(queries / 256)
    fill_table_kernel<<<1, 64, 0, s>>>(k.voff, k.f_rs, nviews, k.tab);
    fill_part_kernel<<<dim3(qb, FV_CHUNKS), 256, 0, s>>>(k.xyz, k.c_pt, k.tab, nviews, k.f_rxyz, k.qent, k.part_d, k.part_i, fill_cap, k.rent, k.seg);
    fill_reduce_kernel<<<qb, 256, 0, s>>>(k.tab, nviews, k.part_d, k.part_i, fill_cap, k.rent, k.qent, k.seg);
    lmb_dead_kernel<<<eb, 256, 0, s>>>(k.c_live, total, k.seg);
    GP_CHECK_LAUNCH();
    // the records of the kept views
    lms_rec_off_kernel<<<1, 64, 0, s>>>(k.voff, k.c_keep, nviews, 0, rec_base, k.loc, rec_off, su);
    lms_append_kernel<<<eb, 256, 0, s>>>(k.c_pt, k.c_view, k.c_live, k.c_keep, k.voff, k.loc, k.seg, total, rec_base, rec_cap, rec_row, rec_seg);
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
    if (!ls_n_ok(n) || !lms_chunk_ok(nviews) || total < 1 || total >= (int64_t)INT32_MAX || words < 1 || words > 1024) return 0;
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
    GP_CHECK_ARG(points && state && view_entry && view_pos && view_keep && rec_off && rec_row && rec_seg && f_seg && logit_seg && status && out &&
                     seen && count && status_out && workspace,
                 "gp_lift_masks_stream_finish: null argument");
    GP_CHECK_ARG(ls_n_ok(n), "gp_lift_masks_stream_finish: n=%lld outside 1..2^31-1", (long long)n);
    GP_CHECK_ARG(lms_chunk_ok(nviews), "gp_lift_masks_stream_finish: %d views outside 1..65535", nviews);
    GP_CHECK_ARG(q >= 1 && q <= 1024, "gp_lift_masks_stream_finish: %d queries outside 1..1024", q);
    GP_CHECK_ARG(total >= 1 && total < (int64_t)INT32_MAX, "gp_lift_masks_stream_finish: %lld records outside 1..2^31-2", (long long)total);
    GP_CHECK_ARG(words >= 1 && words <= 1024, "gp_lift_masks_stream_finish: words=%d outside 1..1024", words);
    GP_CHECK_ARG(d >= 1 && c >= 1 && d % 4 == 0 && ld_out % 4 == 0 && ld_out >= d,
                 "gp_lift_masks_stream_finish: d=%d and ld_out=%lld must be multiples of 4, c=%d", d, (long long)ld_out, c);
    GP_CHECK_ARG(((uintptr_t)f_seg | (uintptr_t)out) % 16 == 0, "gp_lift_masks_stream_finish: f_seg and out must be 16-byte aligned");
    GP_CHECK_ARG(fill == 0 || nn, "gp_lift_masks_stream_finish: the fill writes nn");
    GP_CHECK_ARG(state_bytes >= lms_state_bytes(n), "gp_lift_masks_stream_finish: state too small (%zu < %zu)", state_bytes, lms_state_bytes(n));
    {
        const size_t vq = (size_t)nviews * q;
        const void *in[] = {points, state, view_entry, view_pos, view_keep, rec_off, rec_row, rec_seg, f_seg, logit_seg, status};
        const size_t in_bytes[] = {(size_t)n * 32,     state_bytes,        (size_t)nviews * 8, (size_t)nviews * 4, (size_t)nviews, ((size_t)nviews + 1) * 8,
                                   (size_t)total * 4, (size_t)total * 4, vq * d * 4,         vq * c * 4,         (size_t)ST_WORDS * 8};
        const void *o[] = {out, seen, count, nn, status_out, workspace};
        const size_t o_bytes[] = {(size_t)((n - 1) * ld_out + d) * 4, (size_t)n, (size_t)n * 4, (size_t)n * 8, (size_t)ST_WORDS * 8, workspace_bytes};
        for (int a = 0; a < 6; ++a) {
            for (int i = 0; i < 11; ++i)
                GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], in[i], in_bytes[i]), "gp_lift_masks_stream_finish: an output overlaps an input");
            for (int b = a + 1; b < 6; ++b)
                GP_CHECK_ARG(!lb_overlap(o[a], o_bytes[a], o[b], o_bytes[b]), "gp_lift_masks_stream_finish: two outputs overlap");
        }
    }
    GpCarver sv(const_cast<void *>(state), state_bytes), cv(workspace, workspace_bytes);
    const LmsState st(sv, n);
    LmsFinishWork k(cv, n, nviews, total, words);
    if (!cv.ok()) {
        gp_set_error("gp_lift_masks_stream_finish: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *so = reinterpret_cast<unsigned long long *>(status_out);
    const unsigned nb = (unsigned)((n + 255) / 256), nb1 = (unsigned)((n + 1 + 255) / 256), vb = (unsigned)((nviews + 255) / 256);
    const unsigned eb = (unsigned)((total + 255) / 256);
    const int64_t most = n > LB_TABLE ? n : LB_TABLE;
    // everything kept between the calls, checked
    lms_status_kernel<<<1, 64, 0, s>>>(status, status_out);
    ls_tables_kernel<<<(unsigned)((most + 255) / 256), 256, 0, s>>>(st.tables.keys, st.tables.rows, st.tables.off, n, k.keys, k.rows, k.off, so);
    lmb_view_off_kernel<<<1, 64, 0, s>>>(rec_off, nviews, total, k.voff, so);
    lms_views_kernel<<<vb, 256, 0, s>>>(view_entry, view_pos, view_keep, nviews, words, k.view_local, k.c_keep, so);
    lms_records_kernel<<<eb, 256, 0, s>>>(points, n, view_entry, k.c_keep, k.voff, nviews, q, rec_row, rec_seg, total, k.c_pt, k.c_view, k.c_seg,
                                          k.c_live, so);
    GP_CHECK_LAUNCH();
    // point -> (view, segment) lists in ascending position inside the entry (the kernels of gp_lift_masks_batched)
    GP_CHECK_HIP(hipMemsetAsync(k.vmask, 0, (size_t)n * words * sizeof(unsigned long long), s));
    lmb_pv_mask_kernel<<<eb, 256, 0, s>>>(k.c_pt, k.c_view, k.c_live, k.view_local, total, words, k.vmask);
    lmb_pv_cnt_kernel<<<nb1, 256, 0, s>>>(k.vmask, n, words, k.cnt, count, nn);
    size_t tb = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, tb, k.cnt, k.pv_start, (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>(), s));
    lmb_pv_fill_kernel<<<eb, 256, 0, s>>>(k.c_pt, k.c_view, k.c_live, k.view_local, k.c_seg, total, words, k.vmask, k.pv_start, k.pv_view, k.pv_seg);
    GP_CHECK_LAUNCH();
    // consensus top-3 fusion: the kernel of the per-scene path
    int rc = gp_fuse_views_top3(k.pv_start, k.pv_view, k.pv_seg, n, f_seg, logit_seg, q, d, c, out, ld_out, seen, stream_);
    if (rc != GP_OK) return rc;
    // the scene-level fill inside every entry, over the checked copies of the tables
    lb_fill_flags_kernel<<<nb1, 256, 0, s>>>(k.keys, k.rows, seen, n, k.ref, k.qry);
    GP_CHECK_LAUNCH();
    size_t io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, io, k.ref, k.rs, (int32_t)0, (size_t)(n + 1), rocprim::plus<int32_t>(), s));
    io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, io, k.qry, k.qs, (int32_t)0, (size_t)(n + 1), rocprim::plus<int32_t>(), s));
    lb_fill_compact_kernel<<<nb, 256, 0, s>>>(points, k.rows, k.ref, k.qry, k.rs, k.qs, n, k.rxyz, k.rrow, k.qpos, so);
    if (fill) lb_fill_kernel<<<nb, 256, 0, s>>>(points, k.keys, k.rows, k.off, k.rs, k.qs, n, k.rxyz, k.rrow, k.qpos, nn, so);
    GP_CHECK_LAUNCH();
    return GP_OK;
}
