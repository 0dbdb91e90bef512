// Results carried from one BATCHED cloud to another (geopurify_amd/sparse.py: knn_query, interpolate): the k nearest points of cloud A
// for every point of cloud B, per batch entry, exactly; and rows of a matrix interpolated through such lists.  The role of the
// reference's KDTree queries (models/affinity_module.py:445-447, 693-697), generalised to k neighbours, a second cloud and several
// entries in one call.
//
// The rule is the library's rule for float clouds (gp_nn1_masked_f64, lb_fill_kernel): xyz rounded to fp32 first, d^2 = (dx*dx + dy*dy)
// + dz*dz in fp64 with one rounding per operation, a query's list in ascending (d^2, row) over the points of its own entry.
//
// gp_knn_query: the points' entry table (gp_lift_entries.h), per entry the fp32 bounding box (ordered-int atomics) and a uniform grid of
// ng^3 <= max(count, 1) cubic cells, the points bucketed by cell (count, scan, fill; an entry's cells and points stay contiguous).  One
// wave per query walks the shells of Chebyshev radius 0 .. KQ_R1 around the query's clamped cell -- the candidate numbering of
// nn_grid_query_wave_kernel (misc.hip) -- and keeps the k best (d^2, row) sorted in lanes 0 .. k-1, one slot per lane; after shell r
// every unseen point is at least r * h away, so the walk stops once d^2_k <= (r h (1 - 1e-9))^2 or the shells cover the grid.  The queries
// left over are listed and scan their whole entry, one workgroup each, the four waves' lists merged through LDS.  The lists do not
// depend on the order candidates arrive in: the k smallest of a total order.  No kernel waits on another workgroup.
#include "gp_knn_interp.h"
#include "gp_lift_entries.h"

namespace {

constexpr int KQ_MAX_K = GP_KNN_QUERY_MAX_K;
constexpr int KQ_MAX_NG = 1024;                                  // cells per axis: a cell number inside an entry stays below 2^30
constexpr int KQ_R1 = 3;                                         // the grid walk's last shell
constexpr int KQ_WORDS = 16;
constexpr int KQ_CHUNK = 512;                                    // sorted positions per wave of the bounding-box kernel
constexpr int KQ_QUERY_BLOCKS = 8192, KQ_SCAN_BLOCKS = 4096;
enum { KQ_ST_QUERIES = 8, KQ_ST_EMPTY = 9, KQ_ST_SCAN = 11, KQ_ST_SHELL = 12 };   // queries' words: +ST_BAD_BATCH, +ST_NONFINITE as the points'
static_assert(KQ_R1 == 3, "one status word and one packed counter per shell");
static_assert(KQ_MAX_K <= 32, "a list is one slot per lane and half a wave wide in LDS");

struct KqWork {
    LbTable rows;
    char *tmp;
    size_t tmp_bytes;
    int64_t ncap;                                                // cells of all entries together: at most n + LB_MAX_ENTRIES
    float *bb, *exyz, *sxyz;
    int32_t *ng, *cell_cnt, *cell_start, *srow, *pend;
    int64_t *cbase;
    uint32_t *pcell, *pend_count;
    KqWork(GpCarver &cv, int64_t n, int64_t m) : rows(lb_table(cv, n)), ncap(n + LB_MAX_ENTRIES) {
        tmp_bytes = std::max(lb_sort_bytes(n), gp_scan_bytes<int32_t>(ncap + 1));
        tmp = cv.take<char>(tmp_bytes);
        bb = cv.take<float>((size_t)LB_MAX_ENTRIES * 6);
        ng = cv.take<int32_t>(LB_MAX_ENTRIES);
        cbase = cv.take<int64_t>(LB_MAX_ENTRIES);
        exyz = cv.take<float>((size_t)n * 3);
        pcell = cv.take<uint32_t>(n);
        cell_cnt = cv.take<int32_t>(ncap + 1);
        cell_start = cv.take<int32_t>(ncap + 1);
        sxyz = cv.take<float>((size_t)n * 3);
        srow = cv.take<int32_t>(n);
        pend = cv.take<int32_t>(m);
        pend_count = cv.take<uint32_t>(1);
    }
};

// ------------------------------------------------------------------------------------------------ per-entry grids
__global__ void __launch_bounds__(256) kq_bbox_init_kernel(float *__restrict__ bb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < LB_MAX_ENTRIES * 6) bb[i] = (i % 6) < 3 ? INFINITY : -INFINITY;
}

// float atomic min / max through the ordered-int trick of nn_bbox_kernel (misc.hip); NaN never arrives (fminf / fmaxf drop it)
__device__ __forceinline__ void kq_bbox_atomics(float *__restrict__ bb, const float (&lo)[3], const float (&hi)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int *pl = reinterpret_cast<int *>(bb + a), *ph = reinterpret_cast<int *>(bb + 3 + a);
        const int il = __float_as_int(lo[a]), ih = __float_as_int(hi[a]);
        if (lo[a] == lo[a]) { if (il >= 0) atomicMin(pl, il); else atomicMax(reinterpret_cast<unsigned *>(pl), (unsigned)il); }
        if (hi[a] == hi[a]) { if (ih >= 0) atomicMax(ph, ih); else atomicMin(reinterpret_cast<unsigned *>(ph), (unsigned)ih); }
    }
}

// A wave takes KQ_CHUNK consecutive sorted positions.  The keys are sorted, so the chunk is of one entry when its first and last keys
// agree: one reduction and six atomics per chunk; a chunk that straddles entries sends every position's own.  Also writes the fp32 xyz
// in the entry-sorted order, and counts the rows that are finite in fp64 and not in fp32.
__global__ void __launch_bounds__(256) kq_bbox_kernel(const double *__restrict__ points, const uint32_t *__restrict__ keys_sorted,
                                                      const int32_t *__restrict__ rows_sorted, int64_t n, float *__restrict__ bb,
                                                      float *__restrict__ exyz, unsigned long long *__restrict__ status) {
    const int lane = gp_lane();
    const int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * KQ_CHUNK;
    if (base >= n) return;                                           // (wave-uniform)
    const int64_t last = base + KQ_CHUNK <= n ? base + KQ_CHUNK - 1 : n - 1;
    const uint32_t kfirst = keys_sorted[base], klast = keys_sorted[last];
    const bool uniform = kfirst == klast;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int overflow = 0;
    for (int64_t s = base + lane; s <= last; s += 64) {
        const double *P = points + (int64_t)rows_sorted[s] * 4;
        const float v[3] = {(float)P[1], (float)P[2], (float)P[3]};
        exyz[s * 3] = v[0]; exyz[s * 3 + 1] = v[1]; exyz[s * 3 + 2] = v[2];
        const bool fin64 = fabs(P[0]) < INFINITY && fabs(P[1]) < INFINITY && fabs(P[2]) < INFINITY && fabs(P[3]) < INFINITY;
        if (fin64 && !(fabsf(v[0]) < INFINITY && fabsf(v[1]) < INFINITY && fabsf(v[2]) < INFINITY)) ++overflow;
        const uint32_t key = uniform ? kfirst : keys_sorted[s];
        if (key >= (uint32_t)LB_MAX_ENTRIES) continue;
        if (uniform) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], v[a]); hi[a] = fmaxf(hi[a], v[a]); }
        } else {
            kq_bbox_atomics(bb + (size_t)key * 6, v, v);
        }
    }
    overflow = gp_wave_sum_i(overflow);
    if (lane == 0 && overflow) atomicAdd(status + ST_NONFINITE, (unsigned long long)overflow);
    if (uniform && kfirst < (uint32_t)LB_MAX_ENTRIES) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
            for (int o = 32; o > 0; o >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64)); }
        if (lane == 0) kq_bbox_atomics(bb + (size_t)kfirst * 6, lo, hi);
    }
}

// the largest g with g^3 <= v (v >= 1), at most KQ_MAX_NG
__device__ __forceinline__ int kq_icbrt(int64_t v) {
    int g = (int)cbrt((double)v);
    g = g < 1 ? 1 : g;
    while ((int64_t)(g + 1) * (g + 1) * (g + 1) <= v) ++g;
    while (g > 1 && (int64_t)g * g * g > v) --g;
    return g < KQ_MAX_NG ? g : KQ_MAX_NG;
}

// one workgroup of 1024: ng[b] from the entry's count, cbase[b] = the exclusive sum of ng^3 (64 entries per thread, the threads' sums
// scanned in LDS)
__global__ void __launch_bounds__(1024) kq_grid_kernel(const int32_t *__restrict__ off, int32_t *__restrict__ ng, int64_t *__restrict__ cbase) {
    constexpr int PER = LB_MAX_ENTRIES / 1024;
    __shared__ int64_t s_sum[1024];
    const int t = threadIdx.x;
    int64_t local = 0;
    for (int i = 0; i < PER; ++i) {
        const int b = t * PER + i;
        const int64_t cnt = (int64_t)off[b + 1] - off[b];
        const int g = kq_icbrt(cnt > 1 ? cnt : 1);
        ng[b] = g;
        local += (int64_t)g * g * g;
    }
    s_sum[t] = local;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t v = t >= o ? s_sum[t - o] : 0;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    int64_t run = s_sum[t] - local;
    for (int i = 0; i < PER; ++i) {
        const int b = t * PER + i;
        cbase[b] = run;
        run += (int64_t)ng[b] * ng[b] * ng[b];
    }
}

// The grid of entry b with every device-made number clamped where it is read: the point range [p0, p1) inside 0..n, ng inside
// 1..KQ_MAX_NG, the entry's cells inside 0..ncap.  h as nn_grid_of (misc.hip): ext * (1 + 1e-6) / ng, 1 for a zero extent.
struct KqGrid {
    double lo[3], h, inv_h;
    int ng;
    int64_t cbase;
    int p0, p1;
};
__device__ __forceinline__ KqGrid kq_grid_of(int b, const int32_t *__restrict__ off, const float *__restrict__ bb, const int32_t *__restrict__ ng,
                                            const int64_t *__restrict__ cbase, int64_t n, int64_t ncap) {
    KqGrid g;
    int p0 = off[b], p1 = off[b + 1];
    p0 = p0 < 0 ? 0 : (p0 > n ? (int)n : p0);
    p1 = p1 < p0 ? p0 : (p1 > n ? (int)n : p1);
    g.p0 = p0; g.p1 = p1;
    int e = ng[b];
    e = e < 1 ? 1 : (e > KQ_MAX_NG ? KQ_MAX_NG : e);
    int64_t c = cbase[b];
    const int64_t cells = (int64_t)e * e * e;
    if (c < 0 || c + cells > ncap) { c = 0; e = 1; }               // (cannot happen: the sum of ng^3 is at most n + the entries)
    g.ng = e; g.cbase = c;
    double ext = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = bb[(size_t)b * 6 + a];
        const double d = (double)bb[(size_t)b * 6 + 3 + a] - (double)bb[(size_t)b * 6 + a];
        ext = d > ext ? d : ext;
    }
    g.h = (ext > 0 && ext < INFINITY) ? ext * (1.0 + 1e-6) / e : 1.0;
    g.inv_h = 1.0 / g.h;
    return g;
}
__device__ __forceinline__ int kq_cell(const KqGrid &g, double v, int a) {
    const double f = floor((v - g.lo[a]) * g.inv_h);
    return f >= 0.0 ? (f < (double)g.ng ? (int)f : g.ng - 1) : 0;    // (NaN: 0)
}

__global__ void __launch_bounds__(256) kq_cell_count_kernel(const float *__restrict__ exyz, const uint32_t *__restrict__ keys_sorted, int64_t n,
                                                            const int32_t *__restrict__ off, const float *__restrict__ bb,
                                                            const int32_t *__restrict__ ng, const int64_t *__restrict__ cbase, int64_t ncap,
                                                            int32_t *__restrict__ cell_cnt, uint32_t *__restrict__ pcell) {
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = keys_sorted[s];
    if (key >= (uint32_t)LB_MAX_ENTRIES) { pcell[s] = UINT32_MAX; return; }
    const KqGrid g = kq_grid_of((int)key, off, bb, ng, cbase, n, ncap);
    const int64_t c = g.cbase + ((int64_t)kq_cell(g, exyz[s * 3 + 2], 2) * g.ng + kq_cell(g, exyz[s * 3 + 1], 1)) * g.ng + kq_cell(g, exyz[s * 3], 0);
    pcell[s] = (uint32_t)c;                                          // c < ncap <= 2^31 + 65535
    atomicAdd(&cell_cnt[c], 1);
}

// the order inside a cell is the atomics' and differs between calls; the lists do not depend on it
__global__ void __launch_bounds__(256) kq_cell_fill_kernel(const float *__restrict__ exyz, const int32_t *__restrict__ rows_sorted, int64_t n,
                                                           const uint32_t *__restrict__ pcell, int64_t ncap,
                                                           const int32_t *__restrict__ cell_start, int32_t *__restrict__ cursor,
                                                           float *__restrict__ sxyz, int32_t *__restrict__ srow) {
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t c = pcell[s];
    if ((int64_t)c >= ncap) return;
    const int64_t p = (int64_t)cell_start[c] + atomicAdd(&cursor[c], 1);
    if (p < 0 || p >= n) return;
    sxyz[p * 3] = exyz[s * 3]; sxyz[p * 3 + 1] = exyz[s * 3 + 1]; sxyz[p * 3 + 2] = exyz[s * 3 + 2];
    srow[p] = rows_sorted[s];
}

// ------------------------------------------------------------------------------------------------ the k best of a wave
// Lanes 0 .. k-1 hold the list, ascending in (d^2, row), empty slots (+inf, INT32_MAX) last; (kd, kr) is slot k-1, wave-uniform.
__device__ __forceinline__ bool kq_less(double d, int r, double e, int s) { return d < e || (d == e && r < s); }

// a wave-uniform candidate that is less than slot k-1
__device__ __forceinline__ void kq_insert(double cd, int cr, int k, double &ld, int &lr, double &kd, int &kr) {
    const int lane = gp_lane();
    const int p = __popcll(__ballot(lane < k && kq_less(ld, lr, cd, cr)));       // the slots before it: a prefix, p <= k - 1
    const double ud = __shfl_up(ld, 1, 64);
    const int ur = __shfl_up(lr, 1, 64);
    if (lane > p) { ld = ud; lr = ur; }
    else if (lane == p) { ld = cd; lr = cr; }
    kd = __shfl(ld, k - 1, 64);
    kr = __shfl(lr, k - 1, 64);
}

// every lane's candidate (have: the lane holds one); called by all 64 lanes together
__device__ __forceinline__ void kq_offer(bool have, double cd, int cr, int k, double &ld, int &lr, double &kd, int &kr) {
    unsigned long long todo = __ballot(have && kq_less(cd, cr, kd, kr));
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        kq_insert(__shfl(cd, src, 64), __shfl(cr, src, 64), k, ld, lr, kd, kr);
        todo &= todo - 1;
        todo &= __ballot(have && kq_less(cd, cr, kd, kr));
    }
}

__device__ __forceinline__ void kq_write(int64_t q, int k, double ld, int lr, int64_t *__restrict__ indices, double *__restrict__ dist2) {
    const int lane = gp_lane();
    if (lane < k) {
        const bool valid = ld < INFINITY;
        indices[q * k + lane] = valid ? (int64_t)lr : -1;
        dist2[q * k + lane] = valid ? ld : INFINITY;
    }
}

// a query's entry, or -1: the batch column an integer in 0..65535 and the row finite in fp64 and, xyz, in fp32
__device__ __forceinline__ int kq_query_entry(const double *__restrict__ Q, double &qx, double &qy, double &qz, bool &nonfinite, bool &bad) {
    const double b = Q[0];
    const float x = (float)Q[1], y = (float)Q[2], z = (float)Q[3];
    nonfinite = !(fabs(b) < INFINITY && fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY);
    const int e = lb_entry_of(b);
    bad = e < 0 && fabs(b) < INFINITY;
    qx = x; qy = y; qz = z;
    return nonfinite ? -1 : e;
}

// ------------------------------------------------------------------------------------------------ the grid walk
__global__ void __launch_bounds__(256) kq_walk_kernel(const double *__restrict__ queries, int64_t m, int k, const int32_t *__restrict__ off,
                                                      const float *__restrict__ bb, const int32_t *__restrict__ ng,
                                                      const int64_t *__restrict__ cbase, int64_t n, int64_t ncap,
                                                      const int32_t *__restrict__ cell_start, const float *__restrict__ sxyz,
                                                      const int32_t *__restrict__ srow, int64_t *__restrict__ indices,
                                                      double *__restrict__ dist2, int32_t *__restrict__ pend, uint32_t *__restrict__ pend_count,
                                                      unsigned long long *__restrict__ status) {
    __shared__ int s_cs[4][64], s_off[4][65];
    const int lane = gp_lane(), w = threadIdx.x >> 6;
    int *cs_ = s_cs[w], *off_ = s_off[w];
    unsigned c_bad = 0, c_nf = 0, c_empty = 0;
    unsigned long long c_shell01 = 0, c_shell23 = 0;                 // two 32-bit counts each: shells 0, 1 and 2, 3
    for (int64_t q = (int64_t)blockIdx.x * 4 + w; q < m; q += (int64_t)gridDim.x * 4) {
        double qx, qy, qz;
        bool nonfinite, bad;
        const int b = kq_query_entry(queries + q * 4, qx, qy, qz, nonfinite, bad);   // (wave-uniform: one row per wave)
        c_nf += nonfinite ? 1 : 0;
        c_bad += bad ? 1 : 0;
        double ld = INFINITY, kd = INFINITY;
        int lr = INT32_MAX, kr = INT32_MAX;
        bool done = true;
        if (b >= 0) {
            const KqGrid g = kq_grid_of(b, off, bb, ng, cbase, n, ncap);
            if (g.p1 == g.p0) ++c_empty;
            else {
                done = false;
                const int NG = g.ng;
                const int cx = kq_cell(g, qx, 0), cy = kq_cell(g, qy, 1), cz = kq_cell(g, qz, 2);
                for (int r = 0; r <= KQ_R1 && !done; ++r) {
                    // the shell's cells in the order of nn_grid_query_wave_kernel: the two z faces (side^2 each), then per middle slab its
                    // ring of 4 side - 4 cells; 64 cells at a time, a cell's range per lane, a wave prefix sum, the points shared evenly
                    const int z0 = cz - r, y0 = cy - r, x0 = cx - r, side = 2 * r + 1;
                    const int face = side * side, ring = 4 * side - 4;
                    const int nshell = r == 0 ? 1 : 2 * face + (side - 2) * ring;
                    for (int t0 = 0; t0 < nshell; t0 += 64) {
                        const int t = t0 + lane;
                        int c_start = 0, c_cnt = 0;
                        if (t < nshell) {
                            int dz, dy, dx;
                            if (t < face) { dz = 0; dy = t / side; dx = t % side; }
                            else if (t < 2 * face) { const int u = t - face; dz = side - 1; dy = u / side; dx = u % side; }
                            else {
                                const int u = t - 2 * face, v = u % ring;
                                dz = 1 + u / ring;
                                if (v < side) { dy = 0; dx = v; }
                                else if (v < 2 * side) { dy = side - 1; dx = v - side; }
                                else { const int i = v - 2 * side; dy = 1 + (i >> 1); dx = (i & 1) ? side - 1 : 0; }
                            }
                            const int z = z0 + dz, y = y0 + dy, x = x0 + dx;
                            if (z >= 0 && z < NG && y >= 0 && y < NG && x >= 0 && x < NG) {
                                const int64_t c = g.cbase + ((int64_t)z * NG + y) * NG + x;      // < cbase + ng^3 <= ncap
                                int a = cell_start[c], e = cell_start[c + 1];
                                a = a < g.p0 ? g.p0 : (a > g.p1 ? g.p1 : a);                    // an entry's cells hold its own range
                                e = e < a ? a : (e > g.p1 ? g.p1 : e);
                                c_start = a;
                                c_cnt = e - a;
                            }
                        }
                        int incl = c_cnt;
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) {
                            const int v = __shfl_up(incl, o, 64);
                            if (lane >= o) incl += v;
                        }
                        const int total_p = __shfl(incl, 63, 64);            // <= p1 - p0: the cells' ranges are disjoint
                        if (total_p == 0) continue;                          // (wave-uniform)
                        cs_[lane] = c_start;
                        off_[lane] = incl - c_cnt;
                        if (lane == 63) off_[64] = total_p;
                        gp_wave_sync();
                        for (int j0 = 0; j0 < total_p; j0 += 64) {
                            const int j = j0 + lane;
                            const bool have = j < total_p;
                            double d2 = INFINITY;
                            int row = INT32_MAX;
                            if (have) {
                                int lo = 0, hi = 63;
                                while (lo < hi) {
                                    const int mid = (lo + hi + 1) >> 1;
                                    if (off_[mid] <= j) lo = mid; else hi = mid - 1;
                                }
                                const int64_t pj = cs_[lo] + (j - off_[lo]);                     // inside [p0, p1)
                                const double dx = qx - sxyz[pj * 3], dy = qy - sxyz[pj * 3 + 1], dz = qz - sxyz[pj * 3 + 2];
                                d2 = (dx * dx + dy * dy) + dz * dz;
                                row = srow[pj];
                            }
                            kq_offer(have, d2, row, k, ld, lr, kd, kr);
                        }
                        gp_wave_sync();
                    }
                    const double bound = r * g.h * (1.0 - 1e-9);
                    if (kd <= bound * bound ||
                        (x0 <= 0 && y0 <= 0 && z0 <= 0 && cx + r >= NG - 1 && cy + r >= NG - 1 && cz + r >= NG - 1)) {
                        done = true;
                        if (r < 2) c_shell01 += 1ull << (32 * r); else c_shell23 += 1ull << (32 * (r - 2));
                    }
                }
            }
        }
        if (done) kq_write(q, k, ld, lr, indices, dist2);
        else if (lane == 0) {
            const uint32_t slot = atomicAdd(pend_count, 1u);
            if ((int64_t)slot < m) pend[slot] = (int32_t)q;
        }
    }
    if (lane == 0) {
        if (c_bad) atomicAdd(status + KQ_ST_QUERIES + ST_BAD_BATCH, (unsigned long long)c_bad);
        if (c_nf) atomicAdd(status + KQ_ST_QUERIES + ST_NONFINITE, (unsigned long long)c_nf);
        if (c_empty) atomicAdd(status + KQ_ST_EMPTY, (unsigned long long)c_empty);
        const unsigned long long c_shell[4] = {c_shell01 & 0xFFFFFFFFull, c_shell01 >> 32, c_shell23 & 0xFFFFFFFFull, c_shell23 >> 32};
#pragma unroll
        for (int r = 0; r <= KQ_R1; ++r)
            if (c_shell[r]) atomicAdd(status + KQ_ST_SHELL + r, c_shell[r]);
    }
}

// ------------------------------------------------------------------------------------------------ the entry scan
// One workgroup per listed query: the four waves take a quarter of the entry's range each, wave 0 merges the four lists.
__global__ void __launch_bounds__(256) kq_scan_kernel(const double *__restrict__ queries, int64_t m, int k, const int32_t *__restrict__ off,
                                                      int64_t n, const float *__restrict__ sxyz, const int32_t *__restrict__ srow,
                                                      int64_t *__restrict__ indices, double *__restrict__ dist2,
                                                      const int32_t *__restrict__ pend, const uint32_t *__restrict__ pend_count,
                                                      unsigned long long *__restrict__ status) {
    __shared__ double s_d[4][KQ_MAX_K];
    __shared__ int s_r[4][KQ_MAX_K];
    const int lane = gp_lane(), w = threadIdx.x >> 6;
    const int64_t np = (int64_t)*pend_count < m ? (int64_t)*pend_count : m;
    if (blockIdx.x == 0 && threadIdx.x == 0 && np) atomicAdd(status + KQ_ST_SCAN, (unsigned long long)np);
    for (int64_t i = blockIdx.x; i < np; i += gridDim.x) {
        const int64_t q = pend[i];
        if ((uint64_t)q >= (uint64_t)m) continue;                        // (block-uniform)
        double qx, qy, qz;
        bool nonfinite, bad;
        const int b = kq_query_entry(queries + q * 4, qx, qy, qz, nonfinite, bad);
        if (b < 0) continue;                                             // (cannot happen: the walk lists queries of valid entries)
        int p0 = off[b], p1 = off[b + 1];
        p0 = p0 < 0 ? 0 : (p0 > n ? (int)n : p0);
        p1 = p1 < p0 ? p0 : (p1 > n ? (int)n : p1);
        const int quarter = (p1 - p0 + 3) / 4;
        const int a = p0 + w * quarter < p1 ? p0 + w * quarter : p1, e = a + quarter < p1 ? a + quarter : p1;
        double ld = INFINITY, kd = INFINITY;
        int lr = INT32_MAX, kr = INT32_MAX;
        for (int j0 = a; j0 < e; j0 += 64) {
            const int64_t j = (int64_t)j0 + lane;
            const bool have = j < e;
            double d2 = INFINITY;
            int row = INT32_MAX;
            if (have) {
                const double dx = qx - sxyz[j * 3], dy = qy - sxyz[j * 3 + 1], dz = qz - sxyz[j * 3 + 2];
                d2 = (dx * dx + dy * dy) + dz * dz;
                row = srow[j];
            }
            kq_offer(have, d2, row, k, ld, lr, kd, kr);
        }
        if (lane < k) { s_d[w][lane] = ld; s_r[w][lane] = lr; }
        __syncthreads();
        if (w == 0) {
            for (int o = 1; o < 4; ++o) {
                const bool have = lane < k && s_d[o][lane < k ? lane : 0] < INFINITY;
                const double d2 = have ? s_d[o][lane] : INFINITY;
                const int row = have ? s_r[o][lane] : INT32_MAX;
                kq_offer(have, d2, row, k, ld, lr, kd, kr);
            }
            kq_write(q, k, ld, lr, indices, dist2);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ interpolation
enum { KI_WORDS = 2 };
constexpr int KI_BLOCKS = 1 << 16;

// One wave per query row.  Lanes 0 .. slots-1 read the list once, check it and make the weights in fp64 (ki_list_weights of
// gp_knn_interp.h, the backward's definition too); the rows and the fp32 weights go through the wave's LDS slice, and every lane then
// runs the slots in list order over its columns: VEC columns per load where the base and the pitch allow it, the columns past the
// last whole group one by one; wide_store: rows of out are 16-byte aligned.
template <typename T, int VEC>
__global__ void __launch_bounds__(256) ki_kernel(const T *__restrict__ values, int64_t nrows, int64_t d, int64_t ld,
                                                 const int64_t *__restrict__ index, const int64_t *__restrict__ indices,
                                                 const double *__restrict__ dist2, int64_t m, int k, int64_t npoints, int mode, double eps,
                                                 float *__restrict__ out, int wide_store, unsigned long long *__restrict__ status) {
    __shared__ int64_t s_row[4][KQ_MAX_K];
    __shared__ float s_w[4][KQ_MAX_K];
    const int lane = gp_lane(), w = threadIdx.x >> 6;
    const int slots = mode == KI_NEAREST ? 1 : k;                    // <= KQ_MAX_K
    unsigned c_list = 0, c_index = 0;
    for (int64_t q = (int64_t)blockIdx.x * 4 + w; q < m; q += (int64_t)gridDim.x * 4) {
        float wt;
        bool any_list, any_index;
        const int64_t row = ki_list_weights(indices, dist2, index, q, k, slots, npoints, nrows, mode, eps, wt, any_list, any_index);
        c_list += any_list ? 1 : 0;
        c_index += any_index ? 1 : 0;
        gp_wave_sync();                                                  // (the previous row's reads are done)
        if (lane < slots) { s_row[w][lane] = row; s_w[w][lane] = wt; }
        gp_wave_sync();
        float *o = out + q * d;
        const int64_t whole = VEC > 1 ? d / VEC * VEC : 0;
        for (int64_t c = (int64_t)lane * VEC; c < whole; c += 64 * VEC) {
            float acc[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
            for (int j = 0; j < slots; ++j) {
                const int64_t r = s_row[w][j];
                if (r < 0) continue;                                     // (wave-uniform)
                const float wj = s_w[w][j];
                float x[VEC];
                gp_load_f32<VEC>(values + r * ld + c, x);
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] = acc[i] + wj * x[i];
            }
            if (wide_store) {
#pragma unroll
                for (int i = 0; i < VEC; i += 4) {
                    const float y[4] = {acc[i], acc[i + 1 < VEC ? i + 1 : i], acc[i + 2 < VEC ? i + 2 : i], acc[i + 3 < VEC ? i + 3 : i]};
                    gp_store_vec<4>(o + c + i, y);
                }
            } else {
#pragma unroll
                for (int i = 0; i < VEC; ++i) o[c + i] = acc[i];
            }
        }
        for (int64_t c = whole + lane; c < d; c += 64) {
            float acc = 0.f;
            for (int j = 0; j < slots; ++j) {
                const int64_t r = s_row[w][j];
                if (r < 0) continue;
                acc = acc + s_w[w][j] * gp_to_f32(values[r * ld + c]);
            }
            o[c] = acc;
        }
    }
    if (lane == 0) {
        if (c_list) atomicAdd(status, (unsigned long long)c_list);
        if (c_index) atomicAdd(status + 1, (unsigned long long)c_index);
    }
}

template <typename T, int VEC>
int ki_launch(const void *values, int64_t nrows, int64_t d, int64_t ld, const int64_t *index, const int64_t *indices, const double *dist2,
              int64_t m, int k, int64_t npoints, int mode, double eps, float *out, unsigned long long *st, hipStream_t s) {
    const int64_t nb = (m + 3) / 4;
    const int wide_store = (d % 4 == 0 && (uintptr_t)out % 16 == 0) ? 1 : 0;
    ki_kernel<T, VEC><<<(unsigned)(nb < KI_BLOCKS ? nb : KI_BLOCKS), 256, 0, s>>>(static_cast<const T *>(values), nrows, d, ld, index, indices,
                                                                                   dist2, m, k, npoints, mode, eps, out, wide_store, st);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

// the widest load the base and the pitch allow: 16 bytes, for the half types 8 bytes next, else one element
template <typename T>
int ki_run(const void *values, int64_t nrows, int64_t d, int64_t ld, const int64_t *index, const int64_t *indices, const double *dist2,
           int64_t m, int k, int64_t npoints, int mode, double eps, float *out, unsigned long long *st, hipStream_t s) {
    constexpr int WIDE = 16 / sizeof(T);
    if (d >= WIDE && ld % WIDE == 0 && (uintptr_t)values % 16 == 0)
        return ki_launch<T, WIDE>(values, nrows, d, ld, index, indices, dist2, m, k, npoints, mode, eps, out, st, s);
    if (sizeof(T) == 2 && d >= 4 && ld % 4 == 0 && (uintptr_t)values % 8 == 0)
        return ki_launch<T, 4>(values, nrows, d, ld, index, indices, dist2, m, k, npoints, mode, eps, out, st, s);
    return ki_launch<T, 1>(values, nrows, d, ld, index, indices, dist2, m, k, npoints, mode, eps, out, st, s);
}

__global__ void __launch_bounds__(256) ki_labels_kernel(const int64_t *__restrict__ values, int64_t nrows, const int64_t *__restrict__ index,
                                                        const int64_t *__restrict__ indices, int64_t m, int k, int64_t npoints,
                                                        int64_t unlabeled, int64_t *__restrict__ out, unsigned long long *__restrict__ status) {
    const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    bool bad_list = false, bad_index = false;
    if (q < m) {
        int64_t label = unlabeled;
        const int64_t id = indices[q * k];
        if (id != -1) {
            if ((uint64_t)id >= (uint64_t)npoints) bad_list = true;
            else {
                const int64_t row = index ? index[id] : id;
                if ((uint64_t)row >= (uint64_t)nrows) bad_index = true;
                else label = values[row];
            }
        }
        out[q] = label;
    }
    const int nl = __popcll(__ballot(bad_list)), ni = __popcll(__ballot(bad_index));
    if (gp_lane() == 0) {
        if (nl) atomicAdd(status, (unsigned long long)nl);
        if (ni) atomicAdd(status + 1, (unsigned long long)ni);
    }
}

int ki_check_lists(const char *who, int64_t nrows, const int64_t *index, int64_t n_index, int64_t m, int32_t k, int64_t npoints) {
    GP_CHECK_ARG(nrows >= 1 && m >= 1 && m < (1ll << 31), "%s: nrows=%lld, m=%lld: nrows >= 1, m in 1..2^31-1", who, (long long)nrows, (long long)m);
    GP_CHECK_ARG(k >= 1 && k <= KQ_MAX_K, "%s: k=%d not in 1..%d", who, k, KQ_MAX_K);
    GP_CHECK_ARG(index ? n_index >= 1 : n_index == 0, "%s: n_index=%lld %s an index", who, (long long)n_index, index ? "with" : "without");
    GP_CHECK_ARG(npoints == (index ? n_index : nrows), "%s: npoints=%lld is not the length of %s", who, (long long)npoints,
                 index ? "the index" : "values");
    return GP_OK;
}

}  // namespace

extern "C" size_t gp_knn_query_workspace_bytes(int64_t n, int64_t m) {
    if (!lb_n_ok(n) || !lb_n_ok(m)) return 0;
    GpCarver cv(nullptr, 0);
    KqWork k(cv, n, m);
    return cv.off;
}

extern "C" int gp_knn_query(const double *points, int64_t n, const double *queries, int64_t m, int32_t k, int64_t *indices, double *dist2,
                            int64_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "gp_knn_query";
    GP_CHECK_ARG(points && queries && indices && dist2 && status && workspace, "%s: null argument", who);
    LB_TRY(lb_check_n(who, n));
    GP_CHECK_ARG(lb_n_ok(m), "%s: m=%lld outside 1..2^31-1", who, (long long)m);
    GP_CHECK_ARG(k >= 1 && k <= KQ_MAX_K, "%s: k=%d not in 1..%d", who, k, KQ_MAX_K);
    GP_CHECK_ARG((uintptr_t)points % 8 == 0 && (uintptr_t)queries % 8 == 0 && (uintptr_t)indices % 8 == 0 && (uintptr_t)dist2 % 8 == 0 &&
                     (uintptr_t)status % 8 == 0,
                 "%s: an array is not 8-byte aligned", who);
    {
        const void *const in[] = {points, queries};
        const size_t in_bytes[] = {(size_t)n * 32, (size_t)m * 32};
        const void *const o[] = {indices, dist2, status, workspace};
        const size_t o_bytes[] = {(size_t)m * k * 8, (size_t)m * k * 8, (size_t)KQ_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver cv(workspace, workspace_bytes);
    KqWork kw(cv, n, m);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, KQ_WORDS * sizeof(int64_t), s));
    GP_CHECK_HIP(hipMemsetAsync(kw.cell_cnt, 0, (size_t)(kw.ncap + 1) * sizeof(int32_t), s));
    GP_CHECK_HIP(hipMemsetAsync(kw.pend_count, 0, sizeof(uint32_t), s));
    LB_TRY(lb_row_table(points, n, kw.rows, kw.tmp, kw.tmp_bytes, st, s));
    const unsigned nb = (unsigned)((n + 255) / 256);
    kq_bbox_init_kernel<<<LB_MAX_ENTRIES * 6 / 256, 256, 0, s>>>(kw.bb);
    kq_bbox_kernel<<<(unsigned)((n + 4 * KQ_CHUNK - 1) / (4 * KQ_CHUNK)), 256, 0, s>>>(points, kw.rows.k1, kw.rows.idx, n, kw.bb, kw.exyz, st);
    kq_grid_kernel<<<1, 1024, 0, s>>>(kw.rows.off, kw.ng, kw.cbase);
    kq_cell_count_kernel<<<nb, 256, 0, s>>>(kw.exyz, kw.rows.k1, n, kw.rows.off, kw.bb, kw.ng, kw.cbase, kw.ncap, kw.cell_cnt, kw.pcell);
    GP_CHECK_LAUNCH();
    size_t io = kw.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(kw.tmp, io, kw.cell_cnt, kw.cell_start, (int32_t)0, (size_t)(kw.ncap + 1), rocprim::plus<int32_t>(), s));
    GP_CHECK_HIP(hipMemsetAsync(kw.cell_cnt, 0, (size_t)(kw.ncap + 1) * sizeof(int32_t), s));          // now the cells' cursors
    kq_cell_fill_kernel<<<nb, 256, 0, s>>>(kw.exyz, kw.rows.idx, n, kw.pcell, kw.ncap, kw.cell_start, kw.cell_cnt, kw.sxyz, kw.srow);
    const int64_t qb = (m + 3) / 4;
    kq_walk_kernel<<<(unsigned)(qb < KQ_QUERY_BLOCKS ? qb : KQ_QUERY_BLOCKS), 256, 0, s>>>(queries, m, k, kw.rows.off, kw.bb, kw.ng, kw.cbase, n,
                                                                                            kw.ncap, kw.cell_start, kw.sxyz, kw.srow, indices, dist2,
                                                                                            kw.pend, kw.pend_count, st);
    // sized for the worst case, every query listed: the workgroups stride the list
    kq_scan_kernel<<<(unsigned)(m < KQ_SCAN_BLOCKS ? m : KQ_SCAN_BLOCKS), 256, 0, s>>>(queries, m, k, kw.rows.off, n, kw.sxyz, kw.srow, indices,
                                                                                        dist2, kw.pend, kw.pend_count, st);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_knn_interpolate(const void *values, int32_t elem, int64_t nrows, int64_t d, int64_t ld_values, const int64_t *index,
                                  int64_t n_index, const int64_t *indices, const double *dist2, int64_t m, int32_t k, int64_t npoints,
                                  int32_t mode, double eps, float *out, int64_t *status, void *stream_) {
    const char *who = "gp_knn_interpolate";
    GP_CHECK_ARG(values && indices && dist2 && out && status, "%s: null argument", who);
    LB_TRY(lb_check_elem(who, elem, values, "values"));
    LB_TRY(ki_check_lists(who, nrows, index, n_index, m, k, npoints));
    GP_CHECK_ARG(d >= 1 && ld_values >= d, "%s: d=%lld, ld_values=%lld: 1 <= d <= ld_values", who, (long long)d, (long long)ld_values);
    GP_CHECK_ARG(mode == KI_INVERSE_DISTANCE || mode == KI_NEAREST, "%s: mode=%d (0 inverse distance, 1 nearest)", who, mode);
    GP_CHECK_ARG(eps >= 0.0 && eps < INFINITY, "%s: eps=%g must be finite and not negative", who, eps);
    const size_t es = gp_elem_size(elem);
    GP_CHECK_ARG((uintptr_t)values % es == 0 && (uintptr_t)index % 8 == 0 && (uintptr_t)indices % 8 == 0 && (uintptr_t)dist2 % 8 == 0 &&
                     (uintptr_t)out % 4 == 0 && (uintptr_t)status % 8 == 0,
                 "%s: an array is not aligned to its element", who);
    {
        const void *const in[] = {values, index, indices, dist2};
        const size_t in_bytes[] = {((size_t)(nrows - 1) * ld_values + d) * es, (size_t)n_index * 8, (size_t)m * k * 8, (size_t)m * k * 8};
        const void *const o[] = {out, status};
        const size_t o_bytes[] = {(size_t)m * d * 4, (size_t)KI_WORDS * 8};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, KI_WORDS * sizeof(int64_t), s));
    if (elem == GP_ELEM_F32) return ki_run<float>(values, nrows, d, ld_values, index, indices, dist2, m, k, npoints, mode, eps, out, st, s);
    if (elem == GP_ELEM_F16) return ki_run<gp_f16>(values, nrows, d, ld_values, index, indices, dist2, m, k, npoints, mode, eps, out, st, s);
    return ki_run<gp_bf16>(values, nrows, d, ld_values, index, indices, dist2, m, k, npoints, mode, eps, out, st, s);
}

extern "C" int gp_knn_interpolate_labels(const int64_t *values, int64_t nrows, const int64_t *index, int64_t n_index, const int64_t *indices,
                                         int64_t m, int32_t k, int64_t npoints, int64_t unlabeled, int64_t *out, int64_t *status,
                                         void *stream_) {
    const char *who = "gp_knn_interpolate_labels";
    GP_CHECK_ARG(values && indices && out && status, "%s: null argument", who);
    LB_TRY(ki_check_lists(who, nrows, index, n_index, m, k, npoints));
    GP_CHECK_ARG((uintptr_t)values % 8 == 0 && (uintptr_t)index % 8 == 0 && (uintptr_t)indices % 8 == 0 && (uintptr_t)out % 8 == 0 &&
                     (uintptr_t)status % 8 == 0,
                 "%s: an array is not 8-byte aligned", who);
    {
        const void *const in[] = {values, index, indices};
        const size_t in_bytes[] = {(size_t)nrows * 8, (size_t)n_index * 8, (size_t)m * k * 8};
        const void *const o[] = {out, status};
        const size_t o_bytes[] = {(size_t)m * 8, (size_t)KI_WORDS * 8};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, KI_WORDS * sizeof(int64_t), s));
    ki_labels_kernel<<<(unsigned)((m + 255) / 256), 256, 0, s>>>(values, nrows, index, indices, m, k, npoints, unlabeled, out, st);
    GP_CHECK_LAUNCH();
    return GP_OK;
}
