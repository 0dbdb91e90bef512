// Row 10: exact (K+1)-nearest voxels on the integer lattice, canonical (d^2, id) order, self dropped.
//
// One wave per query.  Candidates come from the (2R+1)^3 block of 8^3-voxel cells around the query
// (contiguous runs in the Morton-ordered voxel array), which contains every voxel with
// d^2 < B = (8R+1)^2.  Squared distances are small integers, so selection is a counting problem:
//   pass 1  LDS histogram of d^2 (< B)           -> threshold T = d^2 of the (K+1)-th smallest
//   pass 2  emit d^2 < T; collect the ties d^2 == T and keep the smallest ids among them
//   pass 3  rank-sort the K+1 winners by (d^2, id), drop rank 0 (the query itself)
// Queries whose (K+1)-th neighbour is not provably inside the block (or with too many ties) are
// appended to a retry list for the next, larger ring; the last resort is an exhaustive scan with a
// bisection on the (d^2, id) key, so the result is exact for every input.
//
// The candidate table, the threshold / emit / tie / rank steps, the guarded retry list and the exhaustive scan are gp_knn_select.h's,
// shared with knn_batched.hip and nn1_batched.hip; what is this file's own is the grid's cell functor, the coordinate loads and the
// read-once (KEEP) form of the first ring.
#include "gp_knn_select.h"

namespace {

// KEEP candidates per lane stay in registers between pass 1 and pass 2 (first ring only): blocks of up to 64 KEEP candidates are read
// ONCE -- pass 2 emits from what pass 1 kept, no second cell search and no second coordinate load.  A kept candidate is one word:
// min(d^2, 127) above its row (pass 2 asks d^2 < T and d^2 == T with T < B = 81 only), so rows must stay below 2^25.
constexpr int KNN_KEEP = 32;
constexpr int KNN_KEEP_ROW_BITS = 25;

template <int R, int WAVES, bool KEEP = false>
__global__ void __launch_bounds__(WAVES * 64)
knn_ring_kernel(const void *grid, const int32_t *__restrict__ coords, const int32_t *__restrict__ ids, int64_t nv,
                int k, int32_t *__restrict__ nbr, const int32_t *__restrict__ qlist,
                const int32_t *__restrict__ qcount, int32_t *__restrict__ fail_list, int32_t *__restrict__ fail_count) {
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
    GpGridView g(grid);
    const int qx = coords[(int64_t)qi * 3], qy = coords[(int64_t)qi * 3 + 1], qz = coords[(int64_t)qi * 3 + 2];
    const int cx0 = (qx - g.h->origin[0]) >> 3, cy0 = (qy - g.h->origin[1]) >> 3, cz0 = (qz - g.h->origin[2]) >> 3;
    int *hist = s_hist[wv];
    for (int b = lane; b < HB; b += 64) hist[b] = 0;
    if (lane < 2) s_cnt[wv][lane] = 0;
    // ---- candidate table from the grid's records (a cell outside the grid or without a record holds nothing)
    int *cstart = s_cstart[wv], *coff = s_coff[wv];
    const int total_c = knn_ring_candidates<R>(cx0, cy0, cz0, [g](int cx, int cy, int cz, int &start, int &cnt) {
        const int slot = g.cell_slot(cx, cy, cz);
        if (slot >= 0) { start = g.recs[slot].start; cnt = g.recs[slot].count; }
    }, cstart, coff, lane);
    auto row_of = [&](int j) { return knn_row_of<R>(cstart, coff, j); };

    // ---- pass 1: histogram of d^2 over the candidates (two per lane and round: both coordinate loads in flight together)
    static_assert(!KEEP || KnnCfg<R>::B <= 127, "a kept candidate holds d^2 in 7 bits");
    const bool kept = KEEP && total_c <= 64 * KNN_KEEP;            // (wave-uniform; larger blocks take the two-pass code below)
    unsigned keep[KEEP ? KNN_KEEP : 1];
    if constexpr (KEEP) {
        if (kept) {
#pragma unroll
            for (int i = 0; i < KNN_KEEP; i += 2) {                  // fully unrolled: keep[] is indexed statically
                if (i * 64 < total_c) {
                    const int ja = i * 64 + lane, jb = ja + 64;
                    const bool va = ja < total_c, vb = jb < total_c;
                    const int64_t ra = va ? row_of(ja) : 0, rb = vb ? row_of(jb) : 0;
                    const int ax = coords[ra * 3], ay = coords[ra * 3 + 1], az = coords[ra * 3 + 2];
                    const int bx = coords[rb * 3], by = coords[rb * 3 + 1], bz = coords[rb * 3 + 2];
                    const int da = (ax - qx) * (ax - qx) + (ay - qy) * (ay - qy) + (az - qz) * (az - qz);
                    const int db = (bx - qx) * (bx - qx) + (by - qy) * (by - qy) + (bz - qz) * (bz - qz);
                    if (va && da < B) atomicAdd(&hist[da], 1);
                    if (vb && db < B) atomicAdd(&hist[db], 1);
                    keep[i] = ((unsigned)(va ? min(da, 127) : 127) << KNN_KEEP_ROW_BITS) | (unsigned)ra;
                    keep[i + 1] = ((unsigned)(vb ? min(db, 127) : 127) << KNN_KEEP_ROW_BITS) | (unsigned)rb;
                }
            }
        }
    }
    for (int j0 = kept ? total_c : 0; j0 < total_c; j0 += 128) {
        const int ja = j0 + lane, jb = j0 + 64 + lane;
        const bool va = ja < total_c, vb = jb < total_c;
        const int64_t ra = va ? row_of(ja) : 0, rb = vb ? row_of(jb) : 0;
        const int ax = coords[ra * 3], ay = coords[ra * 3 + 1], az = coords[ra * 3 + 2];
        const int bx = coords[rb * 3], by = coords[rb * 3 + 1], bz = coords[rb * 3 + 2];
        const int da = (ax - qx) * (ax - qx) + (ay - qy) * (ay - qy) + (az - qz) * (az - qz);
        const int db = (bx - qx) * (bx - qx) + (by - qy) * (by - qy) + (bz - qz) * (bz - qz);
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
    auto emit = [&](int64_t r, int d2) { knn_emit(sel, ids, r, d2, T); };
    if constexpr (KEEP) {
        if (kept) {
#pragma unroll
            for (int i = 0; i < KNN_KEEP; ++i)
                if (i * 64 < total_c) emit((int64_t)(keep[i] & ((1u << KNN_KEEP_ROW_BITS) - 1u)), (int)(keep[i] >> KNN_KEEP_ROW_BITS));
        }
    }
    for (int j0 = kept ? total_c : 0; j0 < total_c; j0 += 64) {
        const int j = j0 + lane;
        if (j < total_c) {
            const int64_t r = row_of(j);
            int ex = coords[r * 3] - qx, ey = coords[r * 3 + 1] - qy, ez = coords[r * 3 + 2] - qz;
            emit(r, ex * ex + ey * ey + ez * ez);
        }
    }
    // ---- ties by lowest id, then pass 3: rank sort of the K+1 winners, drop rank 0 (self)
    knn_select_finish(sel, T, c_lt, need, lane, nbr + (int64_t)qi * k);
}

// Measured and left out (round 6; `knn_cell_kernel`, not in the tree): the first ring as one WORKGROUP PER 8^3 CELL -- the 27-cell block staged
// once in LDS (packed coordinates + row ids, <= 2048 candidates) and the cell's ~25-60 queries answered from there by the same histogram /
// threshold / tie / rank steps, the same results (tests) -- to stop re-reading ~19 KB of candidates from L2 twice per query (5 GB per S
// scene: this kernel runs at the L2 ceiling).  0.88 ms with four waves and 48 KiB of LDS per workgroup, 0.54 ms with eight waves and
// 36 KiB (32 waves per CU) against 0.45 ms here: per query the LDS atomics of the histogram, the rank sort and the staging of sparse
// cells' blocks cost more than the L2 reads they replace.
// exhaustive fallback: one 256-thread block per failed query, bisection on the 64-bit (d2,id) key
__global__ void __launch_bounds__(256)
knn_exhaustive_kernel(const int32_t *__restrict__ coords, const int32_t *__restrict__ ids, int64_t nv, int k,
                      int32_t *__restrict__ nbr, const int32_t *__restrict__ qlist, const int32_t *__restrict__ qcount) {
    __shared__ int s_red[4];
    __shared__ unsigned long long s_selkey[KNN_MAXSEL];
    __shared__ int s_selrow[KNN_MAXSEL];
    __shared__ int s_n;
    const int total = (int)min((int64_t)*qcount, nv);
    for (int w = blockIdx.x; w < total; w += gridDim.x) {
        const int qi = qlist[w];
        const int qx = coords[(int64_t)qi * 3], qy = coords[(int64_t)qi * 3 + 1], qz = coords[(int64_t)qi * 3 + 2];
        auto keyof = [&](int64_t r) {
            long long ex = coords[r * 3] - qx, ey = coords[r * 3 + 1] - qy, ez = coords[r * 3 + 2] - qz;
            unsigned long long d2 = (unsigned long long)(ex * ex + ey * ey + ez * ez);
            unsigned id = (unsigned)(ids ? ids[r] : (int)r);
            return (d2 << 32) | id;      // extents are < 2^15 (gp_grid_build), so d2 < 2^32
        };
        knn_exhaustive_select(0, nv, k + 1, keyof, s_red, s_selkey, s_selrow, &s_n, nbr + (int64_t)qi * k);
    }
}

__global__ void zero2_kernel(int32_t *a, int32_t *b) {
    if (threadIdx.x == 0) { *a = 0; *b = 0; }
}

}  // namespace

extern "C" size_t gp_knn_workspace_bytes(int64_t nv) {
    GpCarver cv(nullptr, 0);
    cv.take<int32_t>(64);
    cv.take<int32_t>(nv);
    cv.take<int32_t>(nv);
    return cv.off;
}

static int knn_lattice(bool read_once, const void *grid, const int32_t *coords, const int32_t *ids, int64_t nv, int32_t k,
                       int32_t *nbr, void *workspace, size_t workspace_bytes, void *stream_) {
    GP_CHECK_ARG(grid && coords && nbr && workspace, "gp_knn_lattice: null argument");
    GP_CHECK_ARG(k >= 1 && k <= GP_KNN_MAX_K, "gp_knn_lattice: k=%d not in 1..%d", k, GP_KNN_MAX_K);
    GP_CHECK_ARG(nv > k, "gp_knn_lattice: need more than k voxels (nv=%lld, k=%d)", (long long)nv, k);
    GpCarver cv(workspace, workspace_bytes);
    int32_t *counts = cv.take<int32_t>(64);
    int32_t *list_a = cv.take<int32_t>(nv);
    int32_t *list_b = cv.take<int32_t>(nv);
    if (!cv.ok()) { gp_set_error("gp_knn_lattice: workspace too small (%zu < %zu)", workspace_bytes, cv.off); return GP_ENOMEM; }
    hipStream_t s = gp_stream(stream_);
    zero2_kernel<<<1, 64, 0, s>>>(counts, counts + 1);
    constexpr int W1 = 4, W3 = 2;
    // ring 1: all queries
    if (read_once && nv <= ((int64_t)1 << KNN_KEEP_ROW_BITS))
        knn_ring_kernel<1, W1, true><<<(int)((nv + W1 - 1) / W1), W1 * 64, 0, s>>>(grid, coords, ids, nv, k, nbr, nullptr, nullptr,
                                                                                list_a, counts);
    else
        knn_ring_kernel<1, W1><<<(int)((nv + W1 - 1) / W1), W1 * 64, 0, s>>>(grid, coords, ids, nv, k, nbr, nullptr, nullptr,
                                                                          list_a, counts);
    // ring 3: failures of ring 1 (grid sized for the worst case; surplus waves exit immediately)
    knn_ring_kernel<3, W3><<<(int)((nv + W3 - 1) / W3), W3 * 64, 0, s>>>(grid, coords, ids, nv, k, nbr, list_a, counts,
                                                                      list_b, counts + 1);
    knn_exhaustive_kernel<<<1024, 256, 0, s>>>(coords, ids, nv, k, nbr, list_b, counts + 1);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_knn_lattice(const void *grid, const int32_t *coords, const int32_t *ids, int64_t nv, int32_t k,
                              int32_t *nbr, void *workspace, size_t workspace_bytes, void *stream_) {
    return knn_lattice(true, grid, coords, ids, nv, k, nbr, workspace, workspace_bytes, stream_);
}

extern "C" int gp_knn_lattice_two_pass(const void *grid, const int32_t *coords, const int32_t *ids, int64_t nv, int32_t k,
                                       int32_t *nbr, void *workspace, size_t workspace_bytes, void *stream_) {
    return knn_lattice(false, grid, coords, ids, nv, k, nbr, workspace, workspace_bytes, stream_);
}
