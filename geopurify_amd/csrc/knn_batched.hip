// Row 10 over BATCHED coordinates: exact (K+1)-nearest voxels inside each batch entry, canonical (d^2, id) order, self dropped.
//
// The input is the sorted key array of gp_coords_order_batched (key = batch << 48 | morton(xyz - min), 16 bits per axis) and nothing
// else: coordinates are decoded from the keys, and the lattice grid of gp_knn_lattice is replaced by a CELL TABLE over the keys.  An
// 8^3 cell is key >> 9, batch bits included, so a cell's rows are one contiguous run of the sorted order and cells of different
// entries never compare equal.  The table (cell key, first row; the count is the next cell's first row minus this one's) is built once
// per call from head flags on key >> 9 and a rocPRIM scan, as gp_quantize_batched builds its voxel heads; a query finds each of its
// (2R+1)^3 cells by a binary search of the cell keys, all lanes at once.
//
// Selection is knn.hip's, step for step (the two files keep their own copies: gp_knn_lattice's kernels stay as they are):
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
#include <rocprim/device/device_scan.hpp>

#include "gp_grid.h"

namespace {

constexpr int KNN_MAXSEL = 128;   // K+1 <= 128
constexpr int KNN_MAXTIE = 256;   // ties at the threshold distance kept in LDS (more: the query retries on the next ring / exhaustively)
constexpr uint64_t kMorton48 = (1ull << 48) - 1;
constexpr int kMaxCellCoord = 65535 >> 3;

template <int R>
struct KnnCfg {
    static constexpr int B = (8 * R + 1) * (8 * R + 1);
    static constexpr int HB = (B + 63) / 64 * 64;
};

// workspace words (i32): [0] ring-1 failures, [1] ring-3 failures, [2..3] one u64: min over the short entries of batch << 32 | count,
// [4] cells in the table
enum { W_FAIL1 = 0, W_FAIL3 = 1, W_SHORT = 2, W_NCELLS = 4 };

// lower bound of q in a[0, n): the first index whose element is not below q (n when there is none)
__device__ __forceinline__ int64_t lower_bound_u64(const uint64_t *__restrict__ a, int64_t n, uint64_t q) {
    int64_t lo = 0;
    while (n > 0) {
        const int64_t half = n >> 1;
        if (a[lo + half] < q) { lo += half + 1; n -= half + 1; }
        else n = half;
    }
    return lo;
}

__device__ __forceinline__ void decode_xyz(uint64_t key, int &x, int &y, int &z) {
    const uint64_t m = key & kMorton48;
    x = (int)gp_compact3(m);
    y = (int)gp_compact3(m >> 1);
    z = (int)gp_compact3(m >> 2);
}

__global__ void kb_init_kernel(int32_t *__restrict__ words, int32_t *__restrict__ status) {
    if (threadIdx.x < 8) words[threadIdx.x] = (threadIdx.x == W_SHORT || threadIdx.x == W_SHORT + 1) ? -1 : 0;
    if (threadIdx.x < 4) status[threadIdx.x] = threadIdx.x == 1 ? -1 : 0;
}

// head[i] = 1 where the sorted row i opens a cell (key >> 9 differs from the row before it); status[3] |= the axes on which a decoded
// coordinate has bit 15 set (bits 45..47 of the key: gp_morton3 puts bit 15 of x, y, z there)
__global__ void kb_cell_heads_kernel(const uint64_t *__restrict__ keys, int64_t nv, int32_t *__restrict__ head, int32_t *__restrict__ status) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int mask = 0;
    if (i < nv) {
        const uint64_t key = keys[i];
        head[i] = (i == 0 || (key >> 9) != (keys[i - 1] >> 9)) ? 1 : 0;
        mask = (int)(key >> 45) & 7;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mask |= __shfl_xor(mask, o, 64);
    if (gp_lane() == 0 && mask) atomicOr(&status[3], mask);
}

// cells_before = exclusive scan of head: the head row i writes cell cells_before[i] (< nv); the last row closes the table
__global__ void kb_cell_table_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ head, const int32_t *__restrict__ cells_before,
                                     int64_t nv, uint64_t *__restrict__ cell_key, int32_t *__restrict__ cell_start, int32_t *__restrict__ words) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const int64_t c = cells_before[i];
    if ((uint64_t)c >= (uint64_t)nv) return;                  // (cannot happen: at most i heads before row i)
    if (head[i]) { cell_key[c] = keys[i] >> 9; cell_start[c] = (int32_t)i; }
    if (i == nv - 1) {
        const int64_t nc = c + (head[i] ? 1 : 0);             // 1 .. nv
        cell_start[nc] = (int32_t)nv;
        words[W_NCELLS] = (int32_t)nc;
    }
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
    __shared__ int s_cstart[WAVES][(2 * R + 1) * (2 * R + 1) * (2 * R + 1)], s_coff[WAVES][(2 * R + 1) * (2 * R + 1) * (2 * R + 1) + 1];

    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int64_t widx = (int64_t)blockIdx.x * WAVES + wv;
    int64_t total = qlist ? min((int64_t)*qcount, nv) : nv;
    if (widx >= total) return;
    const int qi = __builtin_amdgcn_readfirstlane(qlist ? qlist[widx] : (int)widx);
    const uint64_t qkey = keys[qi];
    int qx, qy, qz;
    decode_xyz(qkey, qx, qy, qz);
    const int cx0 = qx >> 3, cy0 = qy >> 3, cz0 = qz >> 3;
    const uint64_t cell_batch = (qkey >> 48) << 39;                  // key >> 9 = batch << 39 | morton(cell coordinates), 13 bits per axis
    const int64_t nc = min((int64_t)*ncells, nv);
    int *hist = s_hist[wv];
    for (int b = lane; b < HB; b += 64) hist[b] = 0;
    if (lane < 2) s_cnt[wv][lane] = 0;
    // ---- candidate table: the (2R+1)^3 cells' (first row, rows before) in LDS, looked up with all lanes at once, and a flat candidate
    // numbering 0 .. total-1.  A cell outside 0..8191 on an axis has no key (it is never re-encoded with wrap-around): skipped.
    constexpr int SIDE = 2 * R + 1, NC = SIDE * SIDE * SIDE;
    int *cstart = s_cstart[wv], *coff = s_coff[wv];
    int total_c = 0;
    for (int c0 = 0; c0 < NC; c0 += 64) {
        const int c = c0 + lane;
        int start = 0, cnt = 0;
        if (c < NC) {
            const int cx = cx0 + c % SIDE - R, cy = cy0 + (c / SIDE) % SIDE - R, cz = cz0 + c / (SIDE * SIDE) - R;
            if ((unsigned)cx <= (unsigned)kMaxCellCoord && (unsigned)cy <= (unsigned)kMaxCellCoord && (unsigned)cz <= (unsigned)kMaxCellCoord) {
                const uint64_t q = cell_batch | gp_morton3((uint32_t)cx, (uint32_t)cy, (uint32_t)cz);
                const int64_t at = lower_bound_u64(cell_key, nc, q);
                if (at < nc && cell_key[at] == q) { start = cell_start[at]; cnt = cell_start[at + 1] - start; }
            }
        }
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (c < NC) { cstart[c] = start; coff[c] = total_c + incl - cnt; }
        total_c += __shfl(incl, 63, 64);
    }
    if (lane == 0) coff[NC] = total_c;
    gp_wave_sync();
    // candidate j -> row: the cell whose range holds j (binary search over the NC + 1 offsets in LDS)
    auto row_of = [&](int j) {
        int lo = 0, hi = NC - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (coff[mid] <= j) lo = mid; else hi = mid - 1;
        }
        return cstart[lo] + (j - coff[lo]);
    };
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
    constexpr int CH = HB / 64;
    int loc = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) loc += hist[lane * CH + c];
    int incl = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    int tot = __shfl(incl, 63, 64);
    const int need = k + 1;
    bool fail = tot < need;
    int T = 0, c_lt = 0;
    if (!fail) {
        int excl = incl - loc;
        unsigned long long m = __ballot(incl >= need);
        int owner = __ffsll((long long)m) - 1;
        int myT = 0, mylt = 0;
        if (lane == owner) {
            int run = excl;
            for (int c = 0; c < CH; ++c) {
                int h = hist[lane * CH + c];
                if (run + h >= need) { myT = lane * CH + c; mylt = run; break; }
                run += h;
            }
        }
        T = __shfl(myT, owner, 64);
        c_lt = __shfl(mylt, owner, 64);
        if (hist[T] > KNN_MAXTIE) fail = true;
    }
    if (fail) {
        if (lane == 0) {
            int p = atomicAdd(fail_count, 1);
            if (p < nv) fail_list[p] = qi;
        }
        return;
    }

    // ---- pass 2: emit winners below T, collect ties at T
    for (int j0 = 0; j0 < total_c; j0 += 64) {
        const int j = j0 + lane;
        if (j < total_c) {
            const int64_t r = row_of(j);
            const int d2 = d2_of(r);
            if (d2 < T) {
                int id = ids ? ids[r] : (int)r;
                int p = atomicAdd(&s_cnt[wv][0], 1);
                s_selkey[wv][p] = ((unsigned long long)(unsigned)d2 << 32) | (unsigned)id;
                s_selrow[wv][p] = (int)r;
            } else if (d2 == T) {
                int id = ids ? ids[r] : (int)r;
                int p = atomicAdd(&s_cnt[wv][1], 1);
                s_tieid[wv][p] = id;
                s_tierow[wv][p] = (int)r;
            }
        }
    }
    gp_wave_sync();
    const int m_tie = s_cnt[wv][1];
    const int take = need - c_lt;                  // ties to keep: the `take` smallest ids
    for (int t = lane; t < m_tie; t += 64) {
        int id = s_tieid[wv][t];
        int rank = 0;
        for (int u = 0; u < m_tie; ++u) rank += (s_tieid[wv][u] < id);
        if (rank < take) {
            s_selkey[wv][c_lt + rank] = ((unsigned long long)(unsigned)T << 32) | (unsigned)id;
            s_selrow[wv][c_lt + rank] = s_tierow[wv][t];
        }
    }
    gp_wave_sync();

    // ---- pass 3: rank sort of the K+1 winners, drop rank 0 (self)
    for (int t = lane; t < need; t += 64) {
        unsigned long long key = s_selkey[wv][t];
        int rank = 0;
        for (int u = 0; u < need; ++u) rank += (s_selkey[wv][u] < key);
        if (rank > 0) nbr[(int64_t)qi * k + rank - 1] = s_selrow[wv][t];
    }
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
        // the entry's rows: [first key with these batch bits, first key of a higher batch index)
        const uint64_t batch = qkey >> 48;
        const int64_t e0 = lower_bound_u64(keys, nv, batch << 48);
        const int64_t e1 = batch == 65535 ? nv : lower_bound_u64(keys, nv, (batch + 1) << 48);
        if (e1 - e0 < need) {
            // an entry of k or fewer voxels has no list: -1 in every slot, and the entry goes into the status (uniform branch: no barrier is skipped)
            for (int t = threadIdx.x; t < k; t += 256) nbr[(int64_t)qi * k + t] = -1;
            if (threadIdx.x == 0) {
                atomicAdd(&status[0], 1);
                atomicMin(short_min, (unsigned long long)(batch << 32) | (unsigned long long)(uint32_t)max(e1 - e0, (int64_t)0));
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
        // smallest key value t such that count(key <= t) >= need, by bisection over 64 bits
        unsigned long long lo = 0, hi = ~0ull;
        while (lo < hi) {
            unsigned long long mid = lo + ((hi - lo) >> 1);
            int c = 0;
            for (int64_t r = e0 + threadIdx.x; r < e1; r += 256) c += (keyof(r) <= mid);
            c = gp_wave_sum_i(c);
            __syncthreads();
            if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = c;
            __syncthreads();
            int tot = s_red[0] + s_red[1] + s_red[2] + s_red[3];
            if (tot >= need) hi = mid; else lo = mid + 1;
        }
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        for (int64_t r = e0 + threadIdx.x; r < e1; r += 256) {
            unsigned long long key = keyof(r);
            if (key <= lo) {
                int p = atomicAdd(&s_n, 1);
                if (p < KNN_MAXSEL) { s_selkey[p] = key; s_selrow[p] = (int)r; }
            }
        }
        __syncthreads();
        // (s_n == need when the keys are distinct, which d2 < 2^32 and distinct ids make them; otherwise -- status[3] != 0, lists
        // undefined -- only the slots that were filled are ranked, and what is stored stays a row of this entry at a slot below k)
        const int have = min(s_n, KNN_MAXSEL);
        for (int t = threadIdx.x; t < min(need, have); t += 256) {
            unsigned long long key = s_selkey[t];
            int rank = 0;
            for (int u = 0; u < min(need, have); ++u) rank += (s_selkey[u] < key);
            if (rank > 0) nbr[(int64_t)qi * k + rank - 1] = s_selrow[t];
        }
        __syncthreads();
    }
}

__global__ void kb_finish_kernel(const unsigned long long *__restrict__ short_min, int32_t *__restrict__ status) {
    if (threadIdx.x == 0 && status[0] > 0) {
        const unsigned long long p = *short_min;
        status[1] = (int32_t)(p >> 32);
        status[2] = (int32_t)(p & 0xffffffffu);
    }
}

size_t scan_bytes(int64_t n) {
    size_t tmp = 0;
    (void)rocprim::exclusive_scan(nullptr, tmp, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), 0);
    return tmp;
}

struct KnnBatchedWs {
    int32_t *words, *list_a, *list_b, *head, *before, *cell_start;
    uint64_t *cell_key;
    char *scan_tmp;
    size_t scan_tmp_bytes;
    KnnBatchedWs(GpCarver &cv, int64_t nv) : scan_tmp_bytes(scan_bytes(nv)) {
        words = cv.take<int32_t>(64);
        list_a = cv.take<int32_t>(nv);
        list_b = cv.take<int32_t>(nv);
        head = cv.take<int32_t>(nv);
        before = cv.take<int32_t>(nv);
        cell_start = cv.take<int32_t>(nv + 1);
        cell_key = cv.take<uint64_t>(nv);
        scan_tmp = cv.take<char>(scan_tmp_bytes);
    }
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
    const int blocks = (int)((nv + 255) / 256);
    unsigned long long *short_min = reinterpret_cast<unsigned long long *>(ws.words + W_SHORT);
    kb_init_kernel<<<1, 64, 0, s>>>(ws.words, status);
    kb_cell_heads_kernel<<<blocks, 256, 0, s>>>(keys_sorted, nv, ws.head, status);
    GP_CHECK_LAUNCH();
    size_t tmp_io = ws.scan_tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(ws.scan_tmp, tmp_io, ws.head, ws.before, (int32_t)0, (size_t)nv, rocprim::plus<int32_t>(), s));
    kb_cell_table_kernel<<<blocks, 256, 0, s>>>(keys_sorted, ws.head, ws.before, nv, ws.cell_key, ws.cell_start, ws.words);
    constexpr int W1 = 4, W3 = 2;
    // ring 1: all queries
    knn_batched_ring_kernel<1, W1><<<(int)((nv + W1 - 1) / W1), W1 * 64, 0, s>>>(keys_sorted, ids, nv, k, ws.cell_key, ws.cell_start,
                                                                              ws.words + W_NCELLS, nbr, nullptr, nullptr, ws.list_a,
                                                                              ws.words + W_FAIL1);
    // ring 3: failures of ring 1 (grid sized for the worst case; surplus waves exit immediately)
    knn_batched_ring_kernel<3, W3><<<(int)((nv + W3 - 1) / W3), W3 * 64, 0, s>>>(keys_sorted, ids, nv, k, ws.cell_key, ws.cell_start,
                                                                              ws.words + W_NCELLS, nbr, ws.list_a, ws.words + W_FAIL1,
                                                                              ws.list_b, ws.words + W_FAIL3);
    knn_batched_exhaustive_kernel<<<1024, 256, 0, s>>>(keys_sorted, ids, nv, k, nbr, ws.list_b, ws.words + W_FAIL3, status, short_min);
    kb_finish_kernel<<<1, 64, 0, s>>>(short_min, status);
    GP_CHECK_LAUNCH();
    return GP_OK;
}
