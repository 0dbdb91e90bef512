// What the resumable lifts over BATCHED point clouds keep between their calls (lift_stream.hip: the dense lift in chunks of views;
// lift_masks_stream.hip: the mask-embedding lift in chunks): the points' entry tables in the caller's STATE, written once by begin,
// and the kernel that copies them into a workspace with every value forced into its range -- the state is the caller's memory between
// calls, so nothing read from it is trusted.  One definition for both.
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

size_t ls_state_bytes(int64_t n) {
    GpCarver cv(nullptr, 0);
    LsState s(cv, n);
    return cv.off;
}

bool ls_n_ok(int64_t n) { return n > 0 && n < (1ll << 31); }

}  // namespace
