// What the resumable lifts over BATCHED point clouds keep between their calls (lift_stream.hip: the dense lift in chunks of views;
// lift_masks_stream.hip: the mask-embedding lift in chunks; lift_labels.hip: the label vote in chunks): the points' entry tables in
// the caller's STATE, written once by begin, the kernel that copies them into a workspace with every value forced into its range --
// the state is the caller's memory between calls, so nothing read from it is trusted -- and, for the two streams that count per view
// (lift_stream.hip, lift_labels.hip), the chunk's view-table workspace and the per-view counts over the state.  One definition for all.
#pragma once
#include "gp_lift_entries.h"

namespace {

enum { ST_BAD_STATE = 6 };

struct LsState {                                                 // the caller's state buffer: written by begin, read by add and finish
    uint32_t *keys;                                              // [n]   the rows' entries in sorted order (65536: no valid entry)
    int32_t *rows;                                               // [n]   the row of every sorted position
    int32_t *off;                                                // [LB_TABLE] the first sorted position of every entry
    LsState(GpCarver &cv, int64_t n) {
        keys = cv.take<uint32_t>(n);
        rows = cv.take<int32_t>(n);
        off = cv.take<int32_t>(LB_TABLE);
    }
};

struct LsBeginWork {
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

// the workspaces of a chunk (its view table) and of the end (the checked copies of the tables, the fill)
struct LsAddWork {
    uint32_t *vk0, *vk1;
    int32_t *w0, *entry_views, *view_off;
    char *tmp;
    size_t tmp_bytes;
    LsAddWork(GpCarver &cv, int32_t nviews) {
        tmp_bytes = lb_sort_bytes(nviews);
        vk0 = cv.take<uint32_t>(nviews);
        vk1 = cv.take<uint32_t>(nviews);
        w0 = cv.take<int32_t>(nviews);
        entry_views = cv.take<int32_t>(nviews);
        view_off = cv.take<int32_t>(LB_TABLE);
        tmp = cv.take<char>(tmp_bytes);
    }
};

struct LsFinishWork {
    uint32_t *keys;
    int32_t *rows, *off, *ref, *qry, *rs, *qs, *rrow, *qpos;
    float *rxyz;
    char *tmp;
    size_t tmp_bytes;
    LsFinishWork(GpCarver &cv, int64_t n) {
        tmp_bytes = lb_scan_bytes(n + 1);
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
        tmp = cv.take<char>(tmp_bytes);
    }
};

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

size_t ls_state_bytes(int64_t n) {
    GpCarver cv(nullptr, 0);
    LsState s(cv, n);
    return cv.off;
}

bool ls_n_ok(int64_t n) { return n > 0 && n < (1ll << 31); }

}  // namespace
