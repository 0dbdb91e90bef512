// The 8^3 cell table over sorted batched keys (gp_coords_order_batched: batch << 48 | morton(xyz - min)), for knn_batched.hip and
// nn1_batched.hip.  A cell is key >> 9, batch bits included, so a cell's rows are one contiguous run of the sorted order and cells of
// different entries never compare equal.  The table (cell key, first row; the count is the next cell's first row minus this one's) is
// built from head flags on key >> 9 and a rocPRIM scan; KnnKeyCells finds a cell by a binary search of the cell keys and is the cell
// functor of gp_knn_select.h's ring candidates.
#pragma once
#include "gp_grid.h"
#include "gp_scan_bytes.h"

namespace {

// the cell functor of the key table: a cell outside 0..8191 on an axis has no key (it is never re-encoded with wrap-around)
struct KnnKeyCells {
    const uint64_t *cell_key;
    const int32_t *cell_start;
    int64_t nc;
    uint64_t cell_batch;                                             // (key >> 48) << 39
    __device__ __forceinline__ void operator()(int cx, int cy, int cz, int &start, int &cnt) const {
        if ((unsigned)cx <= (unsigned)kMaxCellCoord && (unsigned)cy <= (unsigned)kMaxCellCoord && (unsigned)cz <= (unsigned)kMaxCellCoord) {
            const uint64_t q = cell_batch | gp_morton3((uint32_t)cx, (uint32_t)cy, (uint32_t)cz);
            const int64_t at = lower_bound_u64(cell_key, nc, q);
            if (at < nc && cell_key[at] == q) { start = cell_start[at]; cnt = cell_start[at + 1] - start; }
        }
    }
};

// the table over the first n sorted keys: n = nv, or COUNTED n = min(*count, nv) (keys compacted on the device).
// head[i] = 1 where row i < n opens a cell (key >> 9 differs from the row before it), 0 for n <= i < nv, so the scan runs over nv
// elements whatever n is.  With a status: status[3] |= the axes on which a decoded coordinate has bit 15 set (bits 45..47 of the key:
// gp_morton3 puts bit 15 of x, y, z there).
template <bool COUNTED>
__global__ void key_cell_heads_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ count, int64_t nv,
                                      int32_t *__restrict__ head, int32_t *__restrict__ status) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t n = COUNTED ? min((int64_t)*count, nv) : nv;
    int mask = 0;
    if (i < n) {
        const uint64_t key = keys[i];
        head[i] = (i == 0 || (key >> 9) != (keys[i - 1] >> 9)) ? 1 : 0;
        mask = (int)(key >> 45) & 7;
    } else if (i < nv) {
        head[i] = 0;
    }
    if (!status) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mask |= __shfl_xor(mask, o, 64);
    if (gp_lane() == 0 && mask) atomicOr(&status[3], mask);
}

// cells_before = exclusive scan of head: the head row i writes cell cells_before[i] (< nv); the last row closes the table
template <bool COUNTED>
__global__ void key_cell_table_kernel(const uint64_t *__restrict__ keys, const int32_t *count, const int32_t *__restrict__ head,
                                      const int32_t *__restrict__ cells_before, int64_t nv, uint64_t *__restrict__ cell_key,
                                      int32_t *__restrict__ cell_start, int32_t *ncells) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t n = COUNTED ? min((int64_t)*count, nv) : nv;
    if (i >= n) return;
    const int64_t c = cells_before[i];
    if ((uint64_t)c >= (uint64_t)nv) return;                  // (cannot happen: at most i heads before row i)
    if (head[i]) { cell_key[c] = keys[i] >> 9; cell_start[c] = (int32_t)i; }
    if (i == n - 1) {
        const int64_t nc = c + (head[i] ? 1 : 0);             // 1 .. n
        cell_start[nc] = (int32_t)n;
        *ncells = (int32_t)nc;
    }
}

struct KeyCellWs {
    int32_t *head, *before, *cell_start;
    uint64_t *cell_key;
    char *scan_tmp;
    size_t scan_tmp_bytes;
    KeyCellWs(GpCarver &cv, int64_t nv) : scan_tmp_bytes(gp_scan_bytes<int32_t>(nv)) {
        head = cv.take<int32_t>(nv);
        before = cv.take<int32_t>(nv);
        cell_start = cv.take<int32_t>(nv + 1);
        cell_key = cv.take<uint64_t>(nv);
        scan_tmp = cv.take<char>(scan_tmp_bytes);
    }
};

// three launches: heads, scan, table; *ncells = cells in the table (status may be null, see the heads kernel)
template <bool COUNTED>
int key_cell_table(const uint64_t *keys, const int32_t *count, int64_t nv, const KeyCellWs &t, int32_t *ncells, int32_t *status,
                          hipStream_t s) {
    const int blocks = (int)((nv + 255) / 256);
    key_cell_heads_kernel<COUNTED><<<blocks, 256, 0, s>>>(keys, count, nv, t.head, status);
    GP_CHECK_LAUNCH();
    size_t tmp_io = t.scan_tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(t.scan_tmp, tmp_io, t.head, t.before, (int32_t)0, (size_t)nv, rocprim::plus<int32_t>(), s));
    key_cell_table_kernel<COUNTED><<<blocks, 256, 0, s>>>(keys, count, t.head, t.before, nv, t.cell_key, t.cell_start, ncells);
    return GP_OK;
}

}  // namespace
