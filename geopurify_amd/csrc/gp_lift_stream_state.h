// What the resumable lifts over BATCHED point clouds keep between their calls (lift_stream.hip: the dense lift in chunks of views;
// lift_masks_stream.hip: the mask-embedding lift in chunks; lift_labels.hip: the label vote in chunks; render_depth_batched.hip reads
// it): the points' entry tables in the caller's STATE, written once by begin (ls_begin_tables), the per-view counts over them
// (ls_view_counts) and their checked copy (ls_checked_tables).  The state is the caller's memory between calls, so nothing read from
// it is trusted: add's counting kernel checks every index it takes from it, and finish copies the tables into its workspace with every
// value forced into its range and carries the running status words over.  One definition for all.
#pragma once
#include "gp_lift_entries.h"

namespace {

enum { ST_BAD_STATE = 6 };
constexpr unsigned LS_CARRY = 0xf;                               // the status words every stream carries from add to finish: 0 .. ST_TOP_BATCH

// The sorted entry tables of the points, carved from the caller's state buffer (written by begin, read by add and finish) or, for their
// checked copy, from a workspace.
struct LsState {
    uint32_t *keys;                                              // [n]   the rows' entries in sorted order (65536: no valid entry)
    int32_t *rows;                                               // [n]   the row of every sorted position
    int32_t *off;                                                // [LB_TABLE] the first sorted position of every entry
    LsState(GpCarver &cv, int64_t n) {
        keys = cv.take<uint32_t>(n);
        rows = cv.take<int32_t>(n);
        off = cv.take<int32_t>(LB_TABLE);
    }
};

size_t ls_state_bytes(int64_t n) {
    GpCarver cv(nullptr, 0);
    LsState s(cv, n);
    return cv.off;
}

struct LsBeginWork {                                             // the unsorted keys and rows; the sort goes straight into the state
    uint32_t *k0;
    int32_t *r0;
    char *tmp;
    size_t tmp_bytes;
    LsBeginWork(GpCarver &cv, int64_t n) {
        tmp_bytes = lb_sort_bytes(n);
        k0 = cv.take<uint32_t>(n);
        r0 = cv.take<int32_t>(n);
        tmp = cv.take<char>(tmp_bytes);
    }
};

size_t ls_begin_workspace_bytes(int64_t n) {
    GpCarver cv(nullptr, 0);
    LsBeginWork k(cv, n);
    return cv.off;
}

// begin: the points' entry tables into the state; the bad batch rows, the non-finite rows and the top batch into status
int ls_begin_tables(const double *points, int64_t n, const LsState &st, const LsBeginWork &k, int64_t *status, hipStream_t s) {
    const LbTable t = {k.k0, st.keys, k.r0, st.rows, st.off};
    return lb_row_table(points, n, t, k.tmp, k.tmp_bytes, reinterpret_cast<unsigned long long *>(status), s);
}

// ------------------------------------------------------------------------------------------------ per-view counts over the state
// lb_counts_kernel with every index of the state checked before use: blockIdx.y = view; the blocks of a view stride the sorted rows
// of its entry.  Integer atomics: the counts do not depend on arrival order.
__global__ void __launch_bounds__(256) ls_counts_kernel(const double *__restrict__ points, int64_t n, const int32_t *__restrict__ entry_rows,
                                                        const int32_t *__restrict__ entry_off, const int64_t *__restrict__ view_entry,
                                                        const double *__restrict__ w2c, const double *__restrict__ intr,
                                                        const double *__restrict__ depth, int W, int H, int cut, double tau,
                                                        unsigned long long *__restrict__ view_count) {
    const int v = blockIdx.y;
    const int64_t e = view_entry[v];
    if ((uint64_t)e >= (uint64_t)LB_MAX_ENTRIES) return;             // (block-uniform)
    int64_t r0 = entry_off[e], r1 = entry_off[e + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > n ? n : r1;
    const double *M = w2c + (int64_t)v * 16, *K = intr + (int64_t)v * 4;
    const double *dv = depth ? depth + (int64_t)v * W * H : nullptr;
    int local = 0;
    for (int64_t i = r0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < r1; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = entry_rows[i];
        if ((uint64_t)row >= (uint64_t)n) continue;
        const double *P = points + row * 4;
        if (lb_entry_of(P[0]) != (int)e) continue;
        long long ui, vi;
        local += project_point(P[1], P[2], P[3], M, M + 4, M + 8, K[0], K[1], K[2], K[3], dv, W, H, cut, tau, ui, vi) ? 1 : 0;
    }
    local = gp_wave_sum_i(local);
    if (gp_lane() == 0 && local) atomicAdd(view_count + v, (unsigned long long)local);
}

// lb_view_counts over the state's tables
int ls_view_counts(const double *points, int64_t n, const LsState &st, const int64_t *view_entry, const double *w2c, const double *intr,
                   const double *depth, int32_t nviews, int32_t W, int32_t H, int32_t cut, double tau, int64_t min_visible, int64_t max_visible,
                   int64_t *view_count, uint8_t *view_keep, hipStream_t s) {
    return lb_counts_and_keep(
        [&](dim3 grid, unsigned long long *vc) {
            ls_counts_kernel<<<grid, 256, 0, s>>>(points, n, st.rows, st.off, view_entry, w2c, intr, depth, W, H, cut, tau, vc);
        },
        n, nviews, min_visible, max_visible, view_count, view_keep, s);
}

// a chunk's view table and the sort's scratch: the workspace of an add that counts and lifts through the state's tables
struct LsAddWork {
    LbTable views;
    char *tmp;
    size_t tmp_bytes;
    LsAddWork(GpCarver &cv, int32_t nviews) : views(lb_table(cv, nviews)) {
        tmp_bytes = lb_sort_bytes(nviews);
        tmp = cv.take<char>(tmp_bytes);
    }
};

size_t ls_add_workspace_bytes(int32_t nviews) {
    GpCarver cv(nullptr, 0);
    LsAddWork k(cv, nviews);
    return cv.off;
}

// status_out[i] = the running word i where bit i of carry is set, else 0 (one wave)
__global__ void ls_status_kernel(const int64_t *__restrict__ running, int64_t *__restrict__ status_out, unsigned carry) {
    const int i = threadIdx.x;
    if (i < ST_WORDS) status_out[i] = ((carry >> i) & 1u) ? running[i] : 0;
}

// the state's tables into the workspace, every value forced into its range; status_out = the running words, [6] = values changed
__global__ void __launch_bounds__(256) ls_tables_kernel(const uint32_t *__restrict__ keys, const int32_t *__restrict__ rows,
                                                        const int32_t *__restrict__ off, int64_t n, uint32_t *__restrict__ keys_out,
                                                        int32_t *__restrict__ rows_out, int32_t *__restrict__ off_out,
                                                        unsigned long long *__restrict__ status_out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int nbad = 0;
    if (i < n) {
        const uint32_t k = keys[i];
        const int32_t r = rows[i];
        const bool ok = (uint64_t)(int64_t)r < (uint64_t)n;
        nbad = (k > (uint32_t)LB_MAX_ENTRIES ? 1 : 0) + (ok ? 0 : 1);
        keys_out[i] = k > (uint32_t)LB_MAX_ENTRIES ? (uint32_t)LB_MAX_ENTRIES : k;
        rows_out[i] = ok ? r : 0;
    }
    if (i < LB_TABLE) {
        const int64_t o = off[i];
        nbad += (o < 0 || o > n) ? 1 : 0;
        off_out[i] = (int32_t)(o < 0 ? 0 : (o > n ? n : o));
    }
    nbad = gp_wave_sum_i(nbad);
    if (gp_lane() == 0 && nbad) atomicAdd(status_out + ST_BAD_STATE, (unsigned long long)nbad);
}

// The checked copy of a state's tables.  running: the stream's status words, of which those in carry (LS_CARRY, plus a stream's own)
// start status_out and the others start at 0; nullptr: status_out is the caller's and stays as it is.  Either way the values the copy
// had to change are added to status_out[ST_BAD_STATE].
int ls_checked_tables(const LsState &st, int64_t n, const LsState &copy, const int64_t *running, unsigned carry, int64_t *status_out,
                      hipStream_t s) {
    const int64_t most = n > LB_TABLE ? n : LB_TABLE;
    if (running) ls_status_kernel<<<1, 64, 0, s>>>(running, status_out, carry);
    ls_tables_kernel<<<(unsigned)((most + 255) / 256), 256, 0, s>>>(st.keys, st.rows, st.off, n, copy.keys, copy.rows, copy.off,
                                                                     reinterpret_cast<unsigned long long *>(status_out));
    GP_CHECK_LAUNCH();
    return GP_OK;
}

// finish: the checked copy of the tables and the scene-level fill over it; tmp_need: what a finish scans beside the fill's flags
struct LsFinishWork {
    LsState tables;
    LbFill fill;
    char *tmp;
    size_t tmp_bytes;
    LsFinishWork(GpCarver &cv, int64_t n, size_t tmp_need = 0) : tables(cv, n), fill(cv, n) {
        tmp_bytes = std::max(gp_scan_bytes<int32_t>(n + 1), tmp_need);
        tmp = cv.take<char>(tmp_bytes);
    }
};

}  // namespace
