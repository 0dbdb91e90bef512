// The fill of run/validation.py:417-431 over BATCHED coordinates: masked exact 1-NN inside each batch entry, canonical (d^2, id) rule.
//
// The input is what gp_knn_batched takes -- the sorted keys of gp_coords_order_batched (batch << 48 | morton(xyz - min)) and the rows'
// ids -- plus two masks in sorted-row order.  Coordinates are decoded from the keys.  The REFERENCE rows are compacted first (flags +
// rocPRIM scan; the compacted keys stay sorted), and the 8^3 cell table of gp_key_cells.h (cell = key >> 9, batch bits included; head
// flags + scan) is built over the reference keys only, so a cell holds nothing but candidates and a cell of another entry never
// compares equal.
//
// One wave per query.  Ring R takes the references of the (2R+1)^3 cells around the query's cell (gp_knn_select.h's candidate table, the
// walk of the kNN kernels, over a binary search of the cell keys) and reduces (d^2 << 32 | id) to its minimum over the wave -- this
// file's own reduction, with its own bound.  The answer is final only when its d^2 is STRICTLY below
// (8R+1)^2: a reference outside the block differs from the query by 8R+1 or more on some axis (the query sits at offset 0..7 of its
// cell, the block ends 8R cells' edges away), so its d^2 is at least (8R+1)^2 -- it cannot beat a smaller d^2, but at equality it can
// hold the lower id.  Ladder: ring 1 for every query, ring 3 for what is left, then a scan of the entry's own reference rows -- the run
// between two lower bounds on the batch bits of the compacted keys -- by one 256-thread block per query.  With an axis mask other than
// 7 a hidden axis can be arbitrarily far, a ring proves nothing, and every query goes to the scan with the masked distance.
//
// Bounds: every compacted index comes from the cell table (runs inside 0 .. nref-1) or from a lower bound inside 0 .. nref, nref <= nv
// by construction of the scan; every sorted row stored in nn is rrow[] of such an index.  Integer arithmetic only; integer atomics only
// (counters and the work lists, whose order does not reach the result).  Nothing waits on memory written by another workgroup.
#include "gp_key_cells.h"
#include "gp_knn_select.h"

namespace {

constexpr unsigned long long kNoKey = ~0ull;

// workspace words (i32): [0] ring-1 failures, [1] ring-3 failures (or all queries with axes != 7), [2] reference rows, [3] cells
enum { W_FAIL1 = 0, W_FAIL3 = 1, W_NREF = 2, W_NCELLS = 3 };

// minimum of (key, row) over the wave by key; every lane returns the winner (kNoKey: no lane held a candidate)
__device__ __forceinline__ void wave_min_key(unsigned long long &key, int &row) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ok = __shfl_xor(key, o, 64);
        const int orow = __shfl_xor(row, o, 64);
        if (ok < key || (ok == key && orow < row)) { key = ok; row = orow; }
    }
}

__global__ void nb_init_kernel(int32_t *__restrict__ words, int32_t *__restrict__ status) {
    if (threadIdx.x < 8) words[threadIdx.x] = 0;
    if (threadIdx.x < 4) status[threadIdx.x] = 0;
}

// flag[i] = row i is a reference; nn[i] = -1; status[0] / [1] += queries / references; status[3] |= the axes with bit 15 set
__global__ void nb_flags_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ ref_mask, const uint8_t *__restrict__ query_mask,
                                int64_t nv, int32_t *__restrict__ flag, int32_t *__restrict__ nn, int32_t *__restrict__ status) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int mask = 0, nq = 0, nr = 0;
    if (i < nv) {
        nr = ref_mask[i] ? 1 : 0;
        nq = query_mask[i] ? 1 : 0;
        flag[i] = nr;
        nn[i] = -1;
        mask = (int)(keys[i] >> 45) & 7;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mask |= __shfl_xor(mask, o, 64);
    nq = gp_wave_sum_i(nq);
    nr = gp_wave_sum_i(nr);
    if (gp_lane() == 0) {
        if (mask) atomicOr(&status[3], mask);
        if (nq) atomicAdd(&status[0], nq);
        if (nr) atomicAdd(&status[1], nr);
    }
}

// before = exclusive scan of flag: reference row i becomes compacted row before[i] (< nv); the last row publishes the count
__global__ void nb_compact_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ flag, const int32_t *__restrict__ before,
                                  int64_t nv, uint64_t *__restrict__ rkeys, int32_t *__restrict__ rrow, int32_t *__restrict__ words) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const int64_t j = before[i];
    if ((uint64_t)j >= (uint64_t)nv) return;                  // (cannot happen: at most i flags before row i)
    if (flag[i]) { rkeys[j] = keys[i]; rrow[j] = (int32_t)i; }
    if (i == nv - 1) words[W_NREF] = (int32_t)(j + (flag[i] ? 1 : 0));
}

// axes != 7: every query goes to the entry scan
__global__ void nb_collect_kernel(const uint8_t *__restrict__ query_mask, int64_t nv, int32_t *__restrict__ list, int32_t *__restrict__ count) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < nv && query_mask[i]) {
        const int p = atomicAdd(count, 1);
        if (p < nv) list[p] = (int32_t)i;
    }
}

template <int R, int WAVES>
__global__ void __launch_bounds__(WAVES * 64)
nn1_batched_ring_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ ids, const uint8_t *__restrict__ query_mask, int64_t nv,
                        const uint64_t *__restrict__ rkeys, const int32_t *__restrict__ rrow, const uint64_t *__restrict__ cell_key,
                        const int32_t *__restrict__ cell_start, const int32_t *__restrict__ words, int32_t *__restrict__ nn,
                        const int32_t *__restrict__ qlist, const int32_t *__restrict__ qcount, int32_t *__restrict__ fail_list,
                        int32_t *__restrict__ fail_count) {
    constexpr unsigned long long BOUND = KnnCfg<R>::B;
    __shared__ int s_cstart[WAVES][KnnCfg<R>::NC], s_coff[WAVES][KnnCfg<R>::NC + 1];

    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t widx = (int64_t)blockIdx.x * WAVES + wv;
    const int64_t total = qlist ? min((int64_t)*qcount, nv) : nv;
    if (widx >= total) return;
    const int qi = __builtin_amdgcn_readfirstlane(qlist ? qlist[widx] : (int)widx);
    if ((uint64_t)(uint32_t)qi >= (uint64_t)nv) return;
    if (!qlist && !query_mask[qi]) return;
    const uint64_t qkey = keys[qi];
    int qx, qy, qz;
    decode_xyz(qkey, qx, qy, qz);
    const int64_t nref = min((int64_t)words[W_NREF], nv);
    // the block's cells' (first compacted row, candidates before) in LDS
    int *cstart = s_cstart[wv], *coff = s_coff[wv];
    const KnnKeyCells cells{cell_key, cell_start, min((int64_t)words[W_NCELLS], nref), (qkey >> 48) << 39};
    const int total_c = knn_ring_candidates<R>(qx >> 3, qy >> 3, qz >> 3, cells, cstart, coff, lane);

    unsigned long long best = kNoKey;
    int best_row = 0x7fffffff;
    for (int j0 = 0; j0 < total_c; j0 += 64) {
        const int j = j0 + lane;
        if (j < total_c) {
            const int64_t r = knn_row_of<R>(cstart, coff, j);       // compacted row, inside its cell's run
            int x, y, z;
            decode_xyz(rkeys[r], x, y, z);
            // (rows of the block's cells: every coordinate difference is below 8 (R + 1))
            const unsigned long long d2 = (unsigned long long)((x - qx) * (x - qx) + (y - qy) * (y - qy) + (z - qz) * (z - qz));
            const int row = rrow[r];
            const unsigned long long key = (d2 << 32) | (unsigned)(ids ? ids[row] : row);
            if (key < best || (key == best && row < best_row)) { best = key; best_row = row; }
        }
    }
    wave_min_key(best, best_row);
    if (best != kNoKey && (best >> 32) < BOUND) {
        if (lane == 0) nn[qi] = best_row;
    } else {
        knn_fail_append(fail_list, fail_count, nv, qi, lane);
    }
}

// the entry scan: one 256-thread block per listed query over the reference rows of the query's entry, masked distance
__global__ void __launch_bounds__(256)
nn1_batched_scan_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ ids, int64_t nv, int axes,
                        const uint64_t *__restrict__ rkeys, const int32_t *__restrict__ rrow, const int32_t *__restrict__ words,
                        int32_t *__restrict__ nn, const int32_t *__restrict__ qlist, const int32_t *__restrict__ qcount,
                        int32_t *__restrict__ status) {
    __shared__ unsigned long long s_key[4];
    __shared__ int s_row[4];
    const int total = (int)min((int64_t)*qcount, nv);
    const int64_t nref = min((int64_t)words[W_NREF], nv);
    const long long ax = axes & 1, ay = (axes >> 1) & 1, az = (axes >> 2) & 1;
    for (int w = blockIdx.x; w < total; w += gridDim.x) {
        const int qi = qlist[w];
        if ((uint64_t)(uint32_t)qi >= (uint64_t)nv) continue;                  // (uniform: qlist[w] is one value for the block)
        const uint64_t qkey = keys[qi];
        int qx, qy, qz;
        decode_xyz(qkey, qx, qy, qz);
        int64_t e0, e1;                                              // the entry's references among the compacted keys
        entry_range_u64(rkeys, nref, qkey, e0, e1);
        if (e1 <= e0) {
            if (threadIdx.x == 0) atomicAdd(&status[2], 1);          // nn[qi] keeps its -1
            continue;
        }
        unsigned long long best = kNoKey;
        int best_row = 0x7fffffff;
        for (int64_t r = e0 + threadIdx.x; r < e1; r += 256) {
            int x, y, z;
            decode_xyz(rkeys[r], x, y, z);
            const long long ex = x - qx, ey = y - qy, ez = z - qz;
            const unsigned long long d2 = (unsigned long long)(ax * ex * ex + ay * ey * ey + az * ez * ez);
            const int row = rrow[r];
            // decoded coordinates below 2^15 (status[3] == 0) keep d2 below 2^32; otherwise the key wraps and the result is undefined,
            // but `row` is a reference row of this entry whatever the key says
            const unsigned long long key = (d2 << 32) | (unsigned)(ids ? ids[row] : row);
            if (key < best || (key == best && row < best_row)) { best = key; best_row = row; }
        }
        wave_min_key(best, best_row);
        if ((threadIdx.x & 63) == 0) { s_key[threadIdx.x >> 6] = best; s_row[threadIdx.x >> 6] = best_row; }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int v = 1; v < 4; ++v)
                if (s_key[v] < best || (s_key[v] == best && s_row[v] < best_row)) { best = s_key[v]; best_row = s_row[v]; }
            // (e1 > e0: lane 0 of wave 0 held row e0, so a winner exists)
            nn[qi] = best_row;
        }
        __syncthreads();
    }
}

struct Nn1BatchedWs {
    int32_t *words, *list_a, *list_b, *rrow;
    uint64_t *rkeys;
    KeyCellWs cells;                                                 // (its head / before / scan_tmp serve the reference flags first)
    Nn1BatchedWs(GpCarver &cv, int64_t nv)
        : words(cv.take<int32_t>(64)), list_a(cv.take<int32_t>(nv)), list_b(cv.take<int32_t>(nv)), rrow(cv.take<int32_t>(nv)),
          rkeys(cv.take<uint64_t>(nv)), cells(cv, nv) {}
};

// ------------------------------------------------------------------------------------------------ per-entry IoU histograms
constexpr int IOU_STAGE_WORDS = 12288;                               // 48 KiB of LDS counters

// STAGED: all B * 3 * C counters of the call fit in LDS (B * 3 * C <= IOU_STAGE_WORDS): LDS integer atomics, one flush per block.
// Otherwise 64-bit integer atomics straight on `counts`.  Either way integer sums: the result does not depend on arrival order.
template <bool STAGED>
__global__ void __launch_bounds__(256)
iou_hist_batched_kernel(const int64_t *__restrict__ pred, const int32_t *__restrict__ coords, int64_t rows, const int64_t *__restrict__ target,
                        const int64_t *__restrict__ index, int64_t n, int B, int C, const int64_t ig0, const int64_t ig1, const int64_t ig2,
                        const int64_t ig3, int nig, unsigned long long *__restrict__ counts) {
    extern __shared__ unsigned int sh[];                             // [B * 3 * C] when STAGED
    const int words = B * 3 * C;
    if (STAGED) {
        for (int i = threadIdx.x; i < words; i += blockDim.x) sh[i] = 0;
        __syncthreads();
    }
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = index ? index[i] : i;
        if ((uint64_t)row >= (uint64_t)rows) continue;               // an index outside the rows is counted nowhere (and read nowhere)
        const int64_t b = coords[row * 4];
        if (b < 0 || b >= B) continue;
        int64_t p = pred[row];
        const int64_t t = target[i];
        if ((nig > 0 && t == ig0) || (nig > 1 && t == ig1) || (nig > 2 && t == ig2) || (nig > 3 && t == ig3)) p = t;
        const int64_t base = b * 3 * C;
        const bool pin = p >= 0 && p < C, tin = t >= 0 && t < C;
        if (STAGED) {
            if (p == t && pin) atomicAdd(&sh[base + p], 1u);
            if (pin) atomicAdd(&sh[base + C + p], 1u);
            if (tin) atomicAdd(&sh[base + 2 * C + t], 1u);
        } else {
            if (p == t && pin) atomicAdd(&counts[base + p], 1ull);
            if (pin) atomicAdd(&counts[base + C + p], 1ull);
            if (tin) atomicAdd(&counts[base + 2 * C + t], 1ull);
        }
    }
    if (STAGED) {
        __syncthreads();
        for (int i = threadIdx.x; i < words; i += blockDim.x)
            if (sh[i]) atomicAdd(&counts[i], (unsigned long long)sh[i]);
    }
}

}  // namespace

extern "C" size_t gp_nn1_batched_workspace_bytes(int64_t nv) {
    if (nv <= 0 || nv >= (1ll << 31)) return 0;
    GpCarver cv(nullptr, 0);
    Nn1BatchedWs ws(cv, nv);
    return cv.off;
}

extern "C" int gp_nn1_batched(const uint64_t *keys_sorted, const int32_t *ids, const uint8_t *ref_mask, const uint8_t *query_mask, int64_t nv,
                              int32_t axes, int32_t *nn, int32_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    GP_CHECK_ARG(keys_sorted && ref_mask && query_mask && nn && status, "gp_nn1_batched: null argument");
    GP_CHECK_ARG(nv > 0 && nv < (1ll << 31), "gp_nn1_batched: nv=%lld out of range (1 .. 2^31 - 1)", (long long)nv);
    GP_CHECK_ARG(axes >= 1 && axes <= 7, "gp_nn1_batched: axes=%d not in 1..7", axes);
    GpCarver cv(workspace, workspace_bytes);
    Nn1BatchedWs ws(cv, nv);
    if (!workspace || !cv.ok()) {
        gp_set_error("gp_nn1_batched: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    const int blocks = (int)((nv + 255) / 256);
    nb_init_kernel<<<1, 64, 0, s>>>(ws.words, status);
    nb_flags_kernel<<<blocks, 256, 0, s>>>(keys_sorted, ref_mask, query_mask, nv, ws.cells.head, nn, status);
    GP_CHECK_LAUNCH();
    size_t tmp_io = ws.cells.scan_tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(ws.cells.scan_tmp, tmp_io, ws.cells.head, ws.cells.before, (int32_t)0, (size_t)nv,
                                         rocprim::plus<int32_t>(), s));
    nb_compact_kernel<<<blocks, 256, 0, s>>>(keys_sorted, ws.cells.head, ws.cells.before, nv, ws.rkeys, ws.rrow, ws.words);
    const int scan_blocks = (int)min((int64_t)2048, nv);
    if (axes == 7) {
        if (int rc = key_cell_table<true>(ws.rkeys, ws.words + W_NREF, nv, ws.cells, ws.words + W_NCELLS, nullptr, s)) return rc;
        constexpr int W1 = 4, W3 = 4;
        // ring 1: every row, the waves of rows that are no query leave at once
        nn1_batched_ring_kernel<1, W1><<<(int)((nv + W1 - 1) / W1), W1 * 64, 0, s>>>(keys_sorted, ids, query_mask, nv, ws.rkeys, ws.rrow, ws.cells.cell_key,
                                                                                  ws.cells.cell_start, ws.words, nn, nullptr, nullptr, ws.list_a,
                                                                                  ws.words + W_FAIL1);
        // ring 3: what ring 1 left (grid sized for the worst case; surplus waves exit immediately)
        nn1_batched_ring_kernel<3, W3><<<(int)((nv + W3 - 1) / W3), W3 * 64, 0, s>>>(keys_sorted, ids, query_mask, nv, ws.rkeys, ws.rrow, ws.cells.cell_key,
                                                                                  ws.cells.cell_start, ws.words, nn, ws.list_a, ws.words + W_FAIL1,
                                                                                  ws.list_b, ws.words + W_FAIL3);
    } else {
        nb_collect_kernel<<<blocks, 256, 0, s>>>(query_mask, nv, ws.list_b, ws.words + W_FAIL3);
    }
    nn1_batched_scan_kernel<<<scan_blocks, 256, 0, s>>>(keys_sorted, ids, nv, axes, ws.rkeys, ws.rrow, ws.words, nn, ws.list_b, ws.words + W_FAIL3,
                                                      status);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_iou_hist_batched_i64(const int64_t *pred, const int32_t *coords, int64_t rows, const int64_t *target, const int64_t *index,
                                       int64_t n, int32_t num_batches, int32_t num_classes, const int64_t *ignore_ids_host, int32_t num_ignore,
                                       int64_t *counts, void *stream_) {
    GP_CHECK_ARG(pred && coords && target && counts, "gp_iou_hist_batched_i64: null argument");
    GP_CHECK_ARG(rows > 0 && rows < (1ll << 31) && n > 0, "gp_iou_hist_batched_i64: rows=%lld / n=%lld out of range", (long long)rows, (long long)n);
    GP_CHECK_ARG(index || n == rows, "gp_iou_hist_batched_i64: without an index n=%lld must equal rows=%lld", (long long)n, (long long)rows);
    GP_CHECK_ARG(num_batches >= 1 && num_batches <= 65536, "gp_iou_hist_batched_i64: num_batches=%d not in 1..65536", num_batches);
    GP_CHECK_ARG(num_classes >= 1 && num_classes <= 4096, "gp_iou_hist_batched_i64: num_classes=%d not in 1..4096", num_classes);
    GP_CHECK_ARG(num_ignore >= 0 && num_ignore <= 4, "gp_iou_hist_batched_i64: at most 4 ignore ids (got %d)", num_ignore);
    GP_CHECK_ARG(num_ignore == 0 || ignore_ids_host, "gp_iou_hist_batched_i64: null ignore ids");
    int64_t ig[4] = {0, 0, 0, 0};
    for (int i = 0; i < num_ignore; ++i) ig[i] = ignore_ids_host[i];
    int blocks = (int)min((n + 255) / 256, (int64_t)1024);
    unsigned long long *out = reinterpret_cast<unsigned long long *>(counts);
    const int64_t words = (int64_t)num_batches * 3 * num_classes;
    if (words <= IOU_STAGE_WORDS)
        iou_hist_batched_kernel<true><<<blocks, 256, words * sizeof(unsigned int), gp_stream(stream_)>>>(
            pred, coords, rows, target, index, n, num_batches, num_classes, ig[0], ig[1], ig[2], ig[3], num_ignore, out);
    else
        iou_hist_batched_kernel<false><<<blocks, 256, 0, gp_stream(stream_)>>>(
            pred, coords, rows, target, index, n, num_batches, num_classes, ig[0], ig[1], ig[2], ig[3], num_ignore, out);
    GP_CHECK_LAUNCH();
    return GP_OK;
}
