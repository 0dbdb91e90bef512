// Row 10 over BATCHED coordinates: exact (K+1)-nearest voxels inside each batch entry, canonical (d^2, id) order, self dropped.
//
// The input is the sorted key array of gp_coords_order_batched (key = batch << 48 | morton(xyz - min), 16 bits per axis) and nothing
// else: coordinates are decoded from the keys, and the lattice grid of gp_knn_lattice is replaced by the CELL TABLE of gp_key_cells.h
// over the keys (cell = key >> 9, batch bits included), built once per call; a query finds each of its (2R+1)^3 cells by a binary
// search of the cell keys, all lanes at once.
//
// Selection is gp_knn_select.h's, the code that knn.hip runs:
//   pass 1  LDS histogram of d^2 (< B = (8R+1)^2)  -> threshold T = d^2 of the (K+1)-th smallest
//   pass 2  emit d^2 < T; collect the ties d^2 == T and keep the smallest ids among them
//   pass 3  rank-sort the K+1 winners by (d^2, id), drop rank 0 (the query itself)
// and so is the ladder: ring 1 for every query, ring 3 for those whose (K+1)-th neighbour is not provably inside the block (or with
// more than KNN_MAXTIE ties), then an exhaustive scan of the query's own entry -- the rows between two lower bounds on the batch bits --
// with a bisection on the (d^2, id) key.  An entry of K or fewer voxels reaches the exhaustive kernel with every query (no block holds
// K+1 candidates), which fills those rows with -1 and reports the entry in `status`.
//
// Bounds: every row number comes from the cell table (first rows and counts of runs inside 0 .. nv-1) or from a lower bound inside
// 0 .. nv, whatever the keys hold; every LDS index is below the count its own histogram gave.  Loops run over candidates (<= nv), the
// cell count (binary search, <= 32 steps) or the 64 bits of the bisection.  Nothing waits on memory written by another workgroup.
#include "gp_key_cells.h"
#include "gp_knn_select.h"

namespace {

// workspace words (i32): [0] ring-1 failures, [1] ring-3 failures, [2..3] one u64: min over the short entries of batch << 32 | count,
// [4] cells in the table
enum { W_FAIL1 = 0, W_FAIL3 = 1, W_SHORT = 2, W_NCELLS = 4 };

__global__ void kb_init_kernel(int32_t *__restrict__ words, int32_t *__restrict__ status) {
    if (threadIdx.x < 8) words[threadIdx.x] = (threadIdx.x == W_SHORT || threadIdx.x == W_SHORT + 1) ? -1 : 0;
    if (threadIdx.x < 4) status[threadIdx.x] = threadIdx.x == 1 ? -1 : 0;
}

template <int R, int WAVES>
__global__ void __launch_bounds__(WAVES * 64)
knn_batched_ring_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ ids, int64_t nv, int k,
                        const uint64_t *__restrict__ cell_key, const int32_t *__restrict__ cell_start, const int32_t *__restrict__ ncells,
                        int32_t *__restrict__ nbr, const int32_t *__restrict__ qlist, const int32_t *__restrict__ qcount,
                        int32_t *__restrict__ fail_list, int32_t *__restrict__ fail_count) {
    constexpr int B = KnnCfg<R>::B, HB = KnnCfg<R>::HB;
    __shared__ int s_hist[WAVES][HB];
    __shared__ unsigned long long s_selkey[WAVES][KNN_MAXSEL];
    __shared__ int s_selrow[WAVES][KNN_MAXSEL];
    __shared__ int s_tieid[WAVES][KNN_MAXTIE];
    __shared__ int s_tierow[WAVES][KNN_MAXTIE];
    __shared__ int s_cnt[WAVES][2];
    __shared__ int s_cstart[WAVES][KnnCfg<R>::NC], s_coff[WAVES][KnnCfg<R>::NC + 1];

    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int64_t widx = (int64_t)blockIdx.x * WAVES + wv;
    int64_t total = qlist ? min((int64_t)*qcount, nv) : nv;
    if (widx >= total) return;
    const int qi = __builtin_amdgcn_readfirstlane(qlist ? qlist[widx] : (int)widx);
    const uint64_t qkey = keys[qi];
    int qx, qy, qz;
    decode_xyz(qkey, qx, qy, qz);
    int *hist = s_hist[wv];
    for (int b = lane; b < HB; b += 64) hist[b] = 0;
    if (lane < 2) s_cnt[wv][lane] = 0;
    // ---- candidate table from the key cells (key >> 9 = batch << 39 | morton(cell coordinates))
    int *cstart = s_cstart[wv], *coff = s_coff[wv];
    const KnnKeyCells cells{cell_key, cell_start, min((int64_t)*ncells, nv), (qkey >> 48) << 39};
    const int total_c = knn_ring_candidates<R>(qx >> 3, qy >> 3, qz >> 3, cells, cstart, coff, lane);
    auto row_of = [&](int j) { return knn_row_of<R>(cstart, coff, j); };
    // (rows of the block's cells: every coordinate difference is below 8 (R + 1), d^2 a small int)
    auto d2_of = [&](int64_t r) {
        int x, y, z;
        decode_xyz(keys[r], x, y, z);
        return (x - qx) * (x - qx) + (y - qy) * (y - qy) + (z - qz) * (z - qz);
    };

    // ---- pass 1: histogram of d^2 over the candidates (two per lane and round: both key loads in flight together)
    for (int j0 = 0; j0 < total_c; j0 += 128) {
        const int ja = j0 + lane, jb = j0 + 64 + lane;
        const bool va = ja < total_c, vb = jb < total_c;
        const int64_t ra = va ? row_of(ja) : qi, rb = vb ? row_of(jb) : qi;
        const int da = d2_of(ra), db = d2_of(rb);
        if (va && da < B) atomicAdd(&hist[da], 1);
        if (vb && db < B) atomicAdd(&hist[db], 1);
    }
    gp_wave_sync();

    // ---- threshold: smallest T with cum(<=T) >= K+1
    const int need = k + 1;
    int T = 0, c_lt = 0;
    if (!knn_threshold<R>(hist, need, lane, T, c_lt)) {
        knn_fail_append(fail_list, fail_count, nv, qi, lane);
        return;
    }

    // ---- pass 2: emit winners below T, collect ties at T
    const KnnSel sel{s_selkey, s_selrow, s_tieid, s_tierow, s_cnt, wv};
    for (int j0 = 0; j0 < total_c; j0 += 64) {
        const int j = j0 + lane;
        if (j < total_c) {
            const int64_t r = row_of(j);
            knn_emit(sel, ids, r, d2_of(r), T);
        }
    }
    // ---- ties by lowest id, then pass 3: rank sort of the K+1 winners, drop rank 0 (self)
    knn_select_finish(sel, T, c_lt, need, lane, nbr + (int64_t)qi * k);
}

// exhaustive fallback: one 256-thread block per failed query, bisection on the 64-bit (d2,id) key over the rows of the query's entry
__global__ void __launch_bounds__(256)
knn_batched_exhaustive_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ ids, int64_t nv, int k,
                              int32_t *__restrict__ nbr, const int32_t *__restrict__ qlist, const int32_t *__restrict__ qcount,
                              int32_t *__restrict__ status, unsigned long long *__restrict__ short_min) {
    __shared__ int s_red[4];
    __shared__ unsigned long long s_selkey[KNN_MAXSEL];
    __shared__ int s_selrow[KNN_MAXSEL];
    __shared__ int s_n;
    const int total = (int)min((int64_t)*qcount, nv);
    for (int w = blockIdx.x; w < total; w += gridDim.x) {
        const int qi = qlist[w];
        const uint64_t qkey = keys[qi];
        int qx, qy, qz;
        decode_xyz(qkey, qx, qy, qz);
        const int need = k + 1;
        int64_t e0, e1;
        entry_range_u64(keys, nv, qkey, e0, e1);
        if (e1 - e0 < need) {
            // an entry of k or fewer voxels has no list: -1 in every slot, and the entry goes into the status (uniform branch: no barrier is skipped)
            for (int t = threadIdx.x; t < k; t += 256) nbr[(int64_t)qi * k + t] = -1;
            if (threadIdx.x == 0) {
                atomicAdd(&status[0], 1);
                atomicMin(short_min, (unsigned long long)((qkey >> 48) << 32) | (unsigned long long)(uint32_t)max(e1 - e0, (int64_t)0));
            }
            continue;
        }
        auto keyof = [&](int64_t r) {
            int x, y, z;
            decode_xyz(keys[r], x, y, z);
            long long ex = x - qx, ey = y - qy, ez = z - qz;
            unsigned long long d2 = (unsigned long long)(ex * ex + ey * ey + ez * ez);
            unsigned id = (unsigned)(ids ? ids[r] : (int)r);
            return (d2 << 32) | id;      // decoded coordinates below 2^15 (status[3] == 0), so d2 < 2^32
        };
        // (status[3] != 0, lists undefined: only the slots that were filled are ranked, and what is stored stays a row of this entry at a
        // slot below k)
        knn_exhaustive_select(e0, e1, need, keyof, s_red, s_selkey, s_selrow, &s_n, nbr + (int64_t)qi * k);
    }
}

__global__ void kb_finish_kernel(const unsigned long long *__restrict__ short_min, int32_t *__restrict__ status) {
    if (threadIdx.x == 0 && status[0] > 0) {
        const unsigned long long p = *short_min;
        status[1] = (int32_t)(p >> 32);
        status[2] = (int32_t)(p & 0xffffffffu);
    }
}

struct KnnBatchedWs {
    int32_t *words, *list_a, *list_b;
    KeyCellWs cells;
    KnnBatchedWs(GpCarver &cv, int64_t nv)
        : words(cv.take<int32_t>(64)), list_a(cv.take<int32_t>(nv)), list_b(cv.take<int32_t>(nv)), cells(cv, nv) {}
};

}  // namespace

extern "C" size_t gp_knn_batched_workspace_bytes(int64_t nv) {
    if (nv <= 0 || nv >= (1ll << 31)) return 0;
    GpCarver cv(nullptr, 0);
    KnnBatchedWs ws(cv, nv);
    return cv.off;
}

extern "C" int gp_knn_batched(const uint64_t *keys_sorted, const int32_t *ids, int64_t nv, int32_t k, int32_t *nbr, int32_t *status,
                              void *workspace, size_t workspace_bytes, void *stream_) {
    GP_CHECK_ARG(keys_sorted && nbr && status, "gp_knn_batched: null argument");
    GP_CHECK_ARG(nv > 0 && nv < (1ll << 31), "gp_knn_batched: nv=%lld out of range (1 .. 2^31 - 1)", (long long)nv);
    GP_CHECK_ARG(k >= 1 && k <= GP_KNN_MAX_K, "gp_knn_batched: k=%d not in 1..%d", k, GP_KNN_MAX_K);
    GpCarver cv(workspace, workspace_bytes);
    KnnBatchedWs ws(cv, nv);
    if (!workspace || !cv.ok()) {
        gp_set_error("gp_knn_batched: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *short_min = reinterpret_cast<unsigned long long *>(ws.words + W_SHORT);
    kb_init_kernel<<<1, 64, 0, s>>>(ws.words, status);
    if (int rc = key_cell_table<false>(keys_sorted, nullptr, nv, ws.cells, ws.words + W_NCELLS, status, s)) return rc;
    constexpr int W1 = 4, W3 = 2;
    // ring 1: all queries
    knn_batched_ring_kernel<1, W1><<<(int)((nv + W1 - 1) / W1), W1 * 64, 0, s>>>(keys_sorted, ids, nv, k, ws.cells.cell_key, ws.cells.cell_start,
                                                                              ws.words + W_NCELLS, nbr, nullptr, nullptr, ws.list_a,
                                                                              ws.words + W_FAIL1);
    // ring 3: failures of ring 1 (grid sized for the worst case; surplus waves exit immediately)
    knn_batched_ring_kernel<3, W3><<<(int)((nv + W3 - 1) / W3), W3 * 64, 0, s>>>(keys_sorted, ids, nv, k, ws.cells.cell_key, ws.cells.cell_start,
                                                                              ws.words + W_NCELLS, nbr, ws.list_a, ws.words + W_FAIL1,
                                                                              ws.list_b, ws.words + W_FAIL3);
    knn_batched_exhaustive_kernel<<<1024, 256, 0, s>>>(keys_sorted, ids, nv, k, nbr, ws.list_b, ws.words + W_FAIL3, status, short_min);
    kb_finish_kernel<<<1, 64, 0, s>>>(short_min, status);
    GP_CHECK_LAUNCH();
    return GP_OK;
}
