// The exact-kNN family's shared steps: knn.hip (one scene, lattice grid), knn_batched.hip (per entry, over sorted keys) and the fill
// of nn1_batched.hip walk the same (2R+1)^3 block of 8^3 cells and, the first two, select by the same counting rule.  Written once:
//   ring candidates   the block's cells' (first row, rows before) in LDS from a CELL FUNCTOR, and candidate j -> row
//   selection         threshold from the d^2 histogram, the fail-list append, emit, ties by lowest id, rank sort without rank 0
//   exhaustive scan   64-step bisection on the (d^2, id) key over a row range, collect, rank sort
// The batched files' cell functor and the table behind it are in gp_key_cells.h (with a rocPRIM scan that knn.hip has no use for).
// The LDS arrays are declared by the kernels (sizes and per-wave slices are theirs); the helpers take pointers to them and are inlined
// into their callers, so the accesses stay LDS accesses.  Every list append is bounded by nv and every device count is clamped to nv
// where it is read, whichever kernel wrote it.
#pragma once
#include "gp_grid.h"

namespace {

constexpr int KNN_MAXSEL = 128;   // K+1 <= 128
constexpr int KNN_MAXTIE = 256;   // ties at the threshold distance kept in LDS (more: the query retries on the next ring / exhaustively)

template <int R>
struct KnnCfg {
    static constexpr int NC = (2 * R + 1) * (2 * R + 1) * (2 * R + 1);
    static constexpr int B = (8 * R + 1) * (8 * R + 1);
    static constexpr int HB = (B + 63) / 64 * 64;
};

// the kernel's selection arrays, one row per wave, and this wave's row (indexed [wv][i] where they are used: a row pointer per array
// kept in registers instead costs the ring kernels two VGPRs)
struct KnnSel {
    unsigned long long (*selkey)[KNN_MAXSEL];
    int (*selrow)[KNN_MAXSEL], (*tieid)[KNN_MAXTIE], (*tierow)[KNN_MAXTIE], (*cnt)[2];                 // cnt: winners, ties
    int wv;
};

__device__ __forceinline__ int knn_wave_incl(int v, int lane) {
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    return incl;
}

// ---- ring candidates: the (2R+1)^3 cells' (first row, rows before) in LDS, looked up with all lanes at once -- one round of dependent
// loads instead of one per cell -- and a flat candidate numbering 0 .. total-1 (returned).  cells(cx, cy, cz, start, cnt) sets the
// cell's first row and row count and leaves both at 0 for a cell that does not exist.
template <int R, class Cells>
__device__ __forceinline__ int knn_ring_candidates(int cx0, int cy0, int cz0, Cells cells, int *cstart, int *coff, int lane) {
    constexpr int SIDE = 2 * R + 1, NC = KnnCfg<R>::NC;
    int total_c = 0;
    for (int c0 = 0; c0 < NC; c0 += 64) {
        const int c = c0 + lane;
        int start = 0, cnt = 0;
        if (c < NC) cells(cx0 + c % SIDE - R, cy0 + (c / SIDE) % SIDE - R, cz0 + c / (SIDE * SIDE) - R, start, cnt);
        const int incl = knn_wave_incl(cnt, lane);
        if (c < NC) { cstart[c] = start; coff[c] = total_c + incl - cnt; }
        total_c += __shfl(incl, 63, 64);
    }
    if (lane == 0) coff[NC] = total_c;
    gp_wave_sync();
    return total_c;
}

// candidate j -> row: the cell whose range holds j (binary search over the NC + 1 offsets in LDS)
template <int R>
__device__ __forceinline__ int knn_row_of(const int *cstart, const int *coff, int j) {
    int lo = 0, hi = KnnCfg<R>::NC - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (coff[mid] <= j) lo = mid; else hi = mid - 1;
    }
    return cstart[lo] + (j - coff[lo]);
}

// ---- selection
// threshold: smallest T with cum(<= T) >= need, and c_lt = cum(< T).  Returns false (the query fails this ring) when the block holds
// fewer than need candidates below B or more than KNN_MAXTIE at T.
template <int R>
__device__ __forceinline__ bool knn_threshold(const int *hist, int need, int lane, int &T, int &c_lt) {
    constexpr int CH = KnnCfg<R>::HB / 64;
    int loc = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) loc += hist[lane * CH + c];
    const int incl = knn_wave_incl(loc, lane);
    if (__shfl(incl, 63, 64) < need) return false;
    const int owner = __ffsll((long long)__ballot(incl >= need)) - 1;
    int myT = 0, mylt = 0;
    if (lane == owner) {
        int run = incl - loc;
        for (int c = 0; c < CH; ++c) {
            int h = hist[lane * CH + c];
            if (run + h >= need) { myT = lane * CH + c; mylt = run; break; }
            run += h;
        }
    }
    T = __shfl(myT, owner, 64);
    c_lt = __shfl(mylt, owner, 64);
    return hist[T] <= KNN_MAXTIE;
}

// the query goes on the next rung's list (the list holds nv entries; the count is clamped where it is read)
__device__ __forceinline__ void knn_fail_append(int32_t *fail_list, int32_t *fail_count, int64_t nv, int qi, int lane) {
    if (lane == 0) {
        const int p = atomicAdd(fail_count, 1);
        if (p < nv) fail_list[p] = qi;
    }
}

// pass 2, one candidate: a winner below T, or a tie at T (every index is below the count its own histogram gave)
__device__ __forceinline__ void knn_emit(const KnnSel &s, const int32_t *ids, int64_t r, int d2, int T) {
    if (d2 < T) {
        int id = ids ? ids[r] : (int)r;
        int p = atomicAdd(&s.cnt[s.wv][0], 1);
        s.selkey[s.wv][p] = ((unsigned long long)(unsigned)d2 << 32) | (unsigned)id;
        s.selrow[s.wv][p] = (int)r;
    } else if (d2 == T) {
        int id = ids ? ids[r] : (int)r;
        int p = atomicAdd(&s.cnt[s.wv][1], 1);
        s.tieid[s.wv][p] = id;
        s.tierow[s.wv][p] = (int)r;
    }
}

// pass 3: rank sort of n winners by (d^2, id), rank 0 (the query itself) dropped; thread `first` of `stride`
__device__ __forceinline__ void knn_rank_store(const unsigned long long *selkey, const int *selrow, int n, int first, int stride,
                                               int32_t *out) {
    for (int t = first; t < n; t += stride) {
        unsigned long long key = selkey[t];
        int rank = 0;
        for (int u = 0; u < n; ++u) rank += (selkey[u] < key);
        if (rank > 0) out[rank - 1] = selrow[t];
    }
}

// after the emits of a wave: keep the need - c_lt smallest ids among the ties, then rank and store the need winners
__device__ __forceinline__ void knn_select_finish(const KnnSel &s, int T, int c_lt, int need, int lane, int32_t *out) {
    gp_wave_sync();
    const int m_tie = s.cnt[s.wv][1];
    const int take = need - c_lt;
    for (int t = lane; t < m_tie; t += 64) {
        int id = s.tieid[s.wv][t];
        int rank = 0;
        for (int u = 0; u < m_tie; ++u) rank += (s.tieid[s.wv][u] < id);
        if (rank < take) {
            s.selkey[s.wv][c_lt + rank] = ((unsigned long long)(unsigned)T << 32) | (unsigned)id;
            s.selrow[s.wv][c_lt + rank] = s.tierow[s.wv][t];
        }
    }
    gp_wave_sync();
    knn_rank_store(s.selkey[s.wv], s.selrow[s.wv], need, lane, 64, out);
}

// ---- exhaustive scan by one 256-thread block: the need smallest keyof(r) over rows [e0, e1) by bisection on the 64-bit key (the smallest
// value t with count(key <= t) >= need), collected and rank-sorted into out.  need == collected when the keys are distinct, which
// d^2 < 2^32 and distinct ids make them; otherwise only the slots that were filled are ranked.  s_red [4], selkey / selrow [KNN_MAXSEL].
template <class KeyOf>
__device__ __forceinline__ void knn_exhaustive_select(int64_t e0, int64_t e1, int need, KeyOf keyof, int *s_red, unsigned long long *selkey,
                                                      int *selrow, int *s_n, int32_t *out) {
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
    if (threadIdx.x == 0) *s_n = 0;
    __syncthreads();
    for (int64_t r = e0 + threadIdx.x; r < e1; r += 256) {
        unsigned long long key = keyof(r);
        if (key <= lo) {
            int p = atomicAdd(s_n, 1);
            if (p < KNN_MAXSEL) { selkey[p] = key; selrow[p] = (int)r; }
        }
    }
    __syncthreads();
    knn_rank_store(selkey, selrow, min(need, min(*s_n, KNN_MAXSEL)), threadIdx.x, 256, out);
    __syncthreads();
}

}  // namespace
