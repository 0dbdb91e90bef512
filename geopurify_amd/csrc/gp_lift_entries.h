// Shared by every lift over BATCHED point clouds (lift_batched.hip, lift_stream.hip, lift_labels.hip -- whose fill passes the mask
// "voted" where the others pass "seen" --, lift_masks_batched.hip, lift_masks_stream.hip, render_depth_batched.hip, render_rows.hip, fuse.hip).
// Device code: the entry tables (rows and views sorted stably by entry, offsets by binary search), the per-view counts with the
// view-drop rule, and the per-entry scene-level fill (references and queries compacted in the entry-sorted order).  Host code, at the
// end of the file: the carve struct and the launch sequence of each of these (LbTable with lb_row_table / lb_view_table,
// lb_view_counts, LbFill with lb_fill), the overlap check of the entry points (lb_no_overlap) and the argument checks they word alike.
// One definition for all: the library's only rocprim::radix_sort_pairs call and its only lb_fill_kernel launch are here.
#pragma once
#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "gp_common.h"
#include "gp_map_elem.h"
#include "gp_project.h"
#include "gp_scan_bytes.h"

namespace {

constexpr int LB_MAX_ENTRIES = 65536;
constexpr int LB_KEY_BITS = 17;                                  // keys 0 .. 65536 (65536: no valid entry)
constexpr int LB_TABLE = LB_MAX_ENTRIES + 2;                     // off[b] for b = 0 .. 65537: off[65536] = first bad row, off[65537] = n
constexpr int LB_TILE = 1024;                                    // references per LDS tile of the fill

enum { ST_BAD_BATCH = 0, ST_BAD_VIEW = 1, ST_NONFINITE = 2, ST_TOP_BATCH = 3, ST_SEEN = 4, ST_QUERIES = 5, ST_WORDS = 8 };

inline bool lb_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// the entry of a point row (its batch column), -1 when it is no integer in 0..65535 (NaN included)
__device__ __forceinline__ int lb_entry_of(double b) {
    return (b >= 0.0 && b <= 65535.0 && b == floor(b)) ? (int)b : -1;
}

// ------------------------------------------------------------------------------------------------ entry tables
__global__ void __launch_bounds__(256) lb_row_keys_kernel(const double *__restrict__ points, int64_t n, uint32_t *__restrict__ keys,
                                                          int32_t *__restrict__ rows, unsigned long long *__restrict__ status) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const bool live = r < n;
    bool nonfinite = false, bad = false;
    int b = -1;
    if (live) {
        const double *P = points + r * 4;
        nonfinite = !(fabs(P[0]) < INFINITY && fabs(P[1]) < INFINITY && fabs(P[2]) < INFINITY && fabs(P[3]) < INFINITY);
        b = lb_entry_of(P[0]);
        bad = b < 0 && fabs(P[0]) < INFINITY;
        keys[r] = b >= 0 ? (uint32_t)b : (uint32_t)LB_MAX_ENTRIES;
        rows[r] = (int32_t)r;
    }
    const int nbad = __popcll(__ballot(bad)), nnf = __popcll(__ballot(nonfinite));
    int top = b;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
    if (gp_lane() == 0) {
        if (nbad) atomicAdd(status + ST_BAD_BATCH, (unsigned long long)nbad);
        if (nnf) atomicAdd(status + ST_NONFINITE, (unsigned long long)nnf);
        if (top >= 0) atomicMax(status + ST_TOP_BATCH, (unsigned long long)top);
    }
}

__global__ void __launch_bounds__(256) lb_view_keys_kernel(const int64_t *__restrict__ view_entry, int nviews, uint32_t *__restrict__ keys,
                                                           int32_t *__restrict__ views, unsigned long long *__restrict__ status) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (v < nviews) {
        const int64_t e = view_entry[v];
        bad = (uint64_t)e >= (uint64_t)LB_MAX_ENTRIES;
        keys[v] = bad ? (uint32_t)LB_MAX_ENTRIES : (uint32_t)e;
        views[v] = v;
    }
    const int nbad = __popcll(__ballot(bad));
    if (gp_lane() == 0 && nbad) atomicAdd(status + ST_BAD_VIEW, (unsigned long long)nbad);
}

// off[b] = the first sorted position whose key is >= b, b = 0 .. 65537 (keys are <= 65536, so off[65537] = n)
__global__ void __launch_bounds__(256) lb_offsets_kernel(const uint32_t *__restrict__ keys_sorted, int64_t n, int32_t *__restrict__ off) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= LB_TABLE) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys_sorted[mid] < (uint32_t)b) lo = mid + 1;
        else hi = mid;
    }
    off[b] = (int32_t)lo;
}

// ------------------------------------------------------------------------------------------------ per-view counts and the drop rule
// blockIdx.y = view; the blocks of a view stride the rows of its entry.  Integer atomics: the counts do not depend on arrival order.
__global__ void __launch_bounds__(256) lb_counts_kernel(const double *__restrict__ points, const int32_t *__restrict__ entry_rows,
                                                        const int32_t *__restrict__ entry_off, const int64_t *__restrict__ view_entry,
                                                        const double *__restrict__ w2c, const double *__restrict__ intr,
                                                        const double *__restrict__ depth, int W, int H, int cut, double tau,
                                                        unsigned long long *__restrict__ view_count) {
    const int v = blockIdx.y;
    const int64_t e = view_entry[v];
    if ((uint64_t)e >= (uint64_t)LB_MAX_ENTRIES) return;             // (block-uniform)
    const int64_t r0 = entry_off[e], r1 = entry_off[e + 1];
    const double *M = w2c + (int64_t)v * 16, *K = intr + (int64_t)v * 4;
    const double *dv = depth ? depth + (int64_t)v * W * H : nullptr;
    int local = 0;
    for (int64_t i = r0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < r1; i += (int64_t)gridDim.x * blockDim.x) {
        const double *P = points + (int64_t)entry_rows[i] * 4;
        long long ui, vi;
        local += project_point(P[1], P[2], P[3], M, M + 4, M + 8, K[0], K[1], K[2], K[3], dv, W, H, cut, tau, ui, vi) ? 1 : 0;
    }
    local = gp_wave_sum_i(local);
    if (gp_lane() == 0 && local) atomicAdd(view_count + v, (unsigned long long)local);
}

// the view-drop rule of the loader (data_loader_ablation.py:254-255, 280-288)
__global__ void lb_keep_kernel(const unsigned long long *__restrict__ view_count, int nviews, int64_t min_visible, int64_t max_visible,
                               uint8_t *__restrict__ keep) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nviews) return;
    const int64_t nv = (int64_t)view_count[v];
    keep[v] = (nv != 0 && nv >= min_visible && nv <= max_visible) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ the fill
// sorted position s: ref[s] = the row is seen (any byte mask: lift_labels.hip passes "voted"); qry[s] = unseen, in a valid entry
// (decided later whether that entry has references)
__global__ void __launch_bounds__(256) lb_fill_flags_kernel(const uint32_t *__restrict__ keys_sorted, const int32_t *__restrict__ entry_rows,
                                                            const uint8_t *__restrict__ seen, int64_t n, int32_t *__restrict__ ref,
                                                            int32_t *__restrict__ qry) {
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s > n) return;
    int r = 0, q = 0;
    if (s < n && keys_sorted[s] < (uint32_t)LB_MAX_ENTRIES) {
        r = seen[entry_rows[s]] ? 1 : 0;
        q = 1 - r;
    }
    ref[s] = r;
    qry[s] = q;
}

// rs / qs: the exclusive scans of the flags over n + 1 elements (rs[n] = references, qs[n] = unseen rows of valid entries)
__global__ void __launch_bounds__(256) lb_fill_compact_kernel(const double *__restrict__ points, const int32_t *__restrict__ entry_rows,
                                                              const int32_t *__restrict__ ref, const int32_t *__restrict__ qry,
                                                              const int32_t *__restrict__ rs, const int32_t *__restrict__ qs, int64_t n,
                                                              float *__restrict__ rxyz, int32_t *__restrict__ rrow, int32_t *__restrict__ qpos,
                                                              unsigned long long *__restrict__ status) {
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s >= n) return;
    if (ref[s]) {
        const int64_t j = rs[s], row = entry_rows[s];
        const double *P = points + row * 4;
        rxyz[j * 3] = (float)P[1];
        rxyz[j * 3 + 1] = (float)P[2];
        rxyz[j * 3 + 2] = (float)P[3];
        rrow[j] = (int32_t)row;
    }
    if (qry[s]) qpos[qs[s]] = (int32_t)s;
    if (s == n - 1) status[ST_SEEN] = (unsigned long long)rs[n];
}

// 256 queries (compacted, in the entry-sorted order) per block.  A query's references are the run [rs[entry_off[b]], rs[entry_off[b+1]])
// of its entry b; the block streams the union of its queries' runs -- one contiguous range, since both lists are entry-sorted --
// through LDS, every query comparing inside its own run only.  d^2 = (dx*dx + dy*dy) + dz*dz in fp64 over the fp32-rounded xyz, the
// first strict minimum wins and a run ascends by row: the (d^2, row) rule of gp_nn1_masked_f64.
__global__ void __launch_bounds__(256) lb_fill_kernel(const double *__restrict__ points, const uint32_t *__restrict__ keys_sorted,
                                                      const int32_t *__restrict__ entry_rows, const int32_t *__restrict__ entry_off,
                                                      const int32_t *__restrict__ rs, const int32_t *__restrict__ qs, int64_t n,
                                                      const float *__restrict__ rxyz, const int32_t *__restrict__ rrow,
                                                      const int32_t *__restrict__ qpos, int64_t *__restrict__ nn,
                                                      unsigned long long *__restrict__ status) {
    __shared__ double sx[LB_TILE], sy[LB_TILE], sz[LB_TILE];
    __shared__ int s_lo, s_hi, s_filled;
    const int64_t nq = qs[n];
    if ((int64_t)blockIdx.x * 256 >= nq) return;                     // (block-uniform)
    if (threadIdx.x == 0) { s_lo = INT32_MAX; s_hi = 0; s_filled = 0; }
    __syncthreads();
    const int64_t qi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int r0 = 0, r1 = 0;
    int64_t row = -1;
    double qx = 0, qy = 0, qz = 0;
    if (qi < nq) {
        const int64_t s = qpos[qi];
        const uint32_t b = keys_sorted[s];                           // < 65536: only rows of valid entries are queries
        r0 = rs[entry_off[b]];
        r1 = rs[entry_off[b + 1]];
        row = entry_rows[s];
        const double *P = points + row * 4;
        qx = (double)(float)P[1]; qy = (double)(float)P[2]; qz = (double)(float)P[3];
        if (r1 > r0) { atomicMin(&s_lo, r0); atomicMax(&s_hi, r1); }
    }
    __syncthreads();
    const int lo = s_lo, hi = s_hi;
    double best = INFINITY;
    int bi = -1;
    for (int t0 = lo; t0 < hi; t0 += LB_TILE) {
        const int tn = hi - t0 < LB_TILE ? hi - t0 : LB_TILE;
        __syncthreads();
        for (int j = threadIdx.x; j < tn; j += 256) {
            sx[j] = rxyz[(int64_t)(t0 + j) * 3]; sy[j] = rxyz[(int64_t)(t0 + j) * 3 + 1]; sz[j] = rxyz[(int64_t)(t0 + j) * 3 + 2];
        }
        __syncthreads();
        const int j0 = r0 > t0 ? r0 - t0 : 0, j1 = r1 - t0 < tn ? r1 - t0 : tn;
        for (int j = j0; j < j1; ++j) {
            const double dx = qx - sx[j], dy = qy - sy[j], dz = qz - sz[j];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < best) { best = d2; bi = t0 + j; }
        }
    }
    if (bi >= 0) {
        nn[row] = rrow[bi];
        atomicAdd(&s_filled, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_filled) atomicAdd(status + ST_QUERIES, (unsigned long long)s_filled);
}

size_t lb_sort_bytes(int64_t n) {
    size_t t = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (size_t)n, 0,
                                    LB_KEY_BITS, 0);
    return t;
}

// ================================================================================================ host side
// ------------------------------------------------------------------------------------------------ argument checks
// Every output against every input and every later output, over their whole extents: for each output first all inputs, then the later
// outputs.  A null pointer overlaps nothing (an optional argument, or an array that a zero capacity leaves unused: pass nullptr).
inline int lb_no_overlap(const char *who, const void *const *in, const size_t *in_bytes, size_t n_in, const void *const *out,
                         const size_t *out_bytes, size_t n_out) {
    for (size_t a = 0; a < n_out; ++a) {
        for (size_t i = 0; i < n_in; ++i)
            GP_CHECK_ARG(!lb_overlap(out[a], out_bytes[a], in[i], in_bytes[i]), "%s: an output overlaps an input", who);
        for (size_t q = a + 1; q < n_out; ++q) GP_CHECK_ARG(!lb_overlap(out[a], out_bytes[a], out[q], out_bytes[q]), "%s: two outputs overlap", who);
    }
    return GP_OK;
}
template <size_t NI, size_t NO>
int lb_no_overlap(const char *who, const void *const (&in)[NI], const size_t (&in_bytes)[NI], const void *const (&out)[NO],
                  const size_t (&out_bytes)[NO]) {
    return lb_no_overlap(who, in, in_bytes, NI, out, out_bytes, NO);
}

// run a check that sets the message itself; leave the entry point with its code when it fails
#define LB_TRY(call)                     \
    do {                                 \
        const int rc_ = (call);          \
        if (rc_ != GP_OK) return rc_;    \
    } while (0)

inline bool lb_n_ok(int64_t n) { return n > 0 && n < (1ll << 31); }
inline bool lb_nviews_ok(int32_t nviews) { return nviews >= 1 && nviews <= 65535; }

inline int lb_check_n(const char *who, int64_t n) {
    GP_CHECK_ARG(lb_n_ok(n), "%s: n=%lld outside 1..2^31-1", who, (long long)n);
    return GP_OK;
}
inline int lb_check_nviews(const char *who, int32_t nviews) {
    GP_CHECK_ARG(lb_nviews_ok(nviews), "%s: %d views outside 1..65535", who, nviews);
    return GP_OK;
}
// elem: GP_ELEM_* of gp_map_elem.h (0 fp32, 1 fp16, 2 bf16); what: "maps" or "masks"
inline int lb_check_elem(const char *who, int32_t elem, const void *p, const char *what) {
    GP_CHECK_ARG(gp_elem_ok(elem), "%s: element type %d (0 fp32, 1 fp16, 2 bf16)", who, elem);
    GP_CHECK_ARG(elem == GP_ELEM_F32 || (uintptr_t)p % 2 == 0, "%s: half %s at an odd address", who, what);
    return GP_OK;
}
inline int lb_check_sampling(const char *who, int32_t bilinear, int32_t h, int32_t w, int32_t height, int32_t width) {
    GP_CHECK_ARG(bilinear == 0 || bilinear == 1, "%s: bilinear=%d (0 nearest, 1 bilinear)", who, bilinear);
    GP_CHECK_ARG(bilinear || (h == height && w == width), "%s: the nearest mode samples the map itself: map %d x %d, image %d x %d", who, h, w,
                 height, width);
    return GP_OK;
}
inline int lb_check_cut(const char *who, int32_t cut_bound) {
    GP_CHECK_ARG(cut_bound >= 0, "%s: cut_bound=%d must not be negative", who, cut_bound);
    return GP_OK;
}
inline int lb_check_image(const char *who, int32_t height, int32_t width) {
    GP_CHECK_ARG(height >= 1 && width >= 1, "%s: image %d x %d", who, height, width);
    return GP_OK;
}
inline int lb_check_state(const char *who, size_t state_bytes, size_t need) {
    GP_CHECK_ARG(state_bytes >= need, "%s: state too small (%zu < %zu)", who, state_bytes, need);
    return GP_OK;
}
inline int lb_check_workspace(const char *who, const GpCarver &cv, size_t workspace_bytes) {
    if (cv.ok()) return GP_OK;
    gp_set_error("%s: workspace too small (%zu < %zu)", who, workspace_bytes, cv.off);
    return GP_ENOMEM;
}

// ------------------------------------------------------------------------------------------------ entry tables
// The rows (or views) sorted stably by entry: (k0, idx0) the keys and indices as the keys kernel wrote them, (k1, idx) sorted, off[b] the
// first sorted position of entry b.  A workspace carves all five; the streams' begin puts k1 / idx / off into the caller's state.
struct LbTable {
    uint32_t *k0, *k1;
    int32_t *idx0, *idx, *off;
};

inline LbTable lb_table(GpCarver &cv, int64_t n) {
    LbTable t;
    t.k0 = cv.take<uint32_t>(n);
    t.k1 = cv.take<uint32_t>(n);
    t.idx0 = cv.take<int32_t>(n);
    t.idx = cv.take<int32_t>(n);
    t.off = cv.take<int32_t>(LB_TABLE);
    return t;
}

// (k0, idx0) -> (k1, idx): stable, so an entry's rows ascend by row and its views by view index
inline int lb_table_sort(const LbTable &t, int64_t n, char *tmp, size_t tmp_bytes, hipStream_t s) {
    size_t io = tmp_bytes;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(tmp, io, t.k0, t.k1, t.idx0, t.idx, (size_t)n, 0, LB_KEY_BITS, s));
    return GP_OK;
}

// the sort and the offsets, for keys that are written (lb_row_table, lb_view_table, or a caller with a keys kernel of its own)
inline int lb_table_finish(const LbTable &t, int64_t n, char *tmp, size_t tmp_bytes, hipStream_t s) {
    LB_TRY(lb_table_sort(t, n, tmp, tmp_bytes, s));
    lb_offsets_kernel<<<(LB_TABLE + 255) / 256, 256, 0, s>>>(t.k1, n, t.off);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

inline int lb_row_table(const double *points, int64_t n, const LbTable &t, char *tmp, size_t tmp_bytes, unsigned long long *st, hipStream_t s) {
    lb_row_keys_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(points, n, t.k0, t.idx0, st);
    GP_CHECK_LAUNCH();
    return lb_table_finish(t, n, tmp, tmp_bytes, s);
}

inline int lb_view_table(const int64_t *view_entry, int32_t nviews, const LbTable &t, char *tmp, size_t tmp_bytes, unsigned long long *st,
                         hipStream_t s) {
    lb_view_keys_kernel<<<(unsigned)((nviews + 255) / 256), 256, 0, s>>>(view_entry, nviews, t.k0, t.idx0, st);
    GP_CHECK_LAUNCH();
    return lb_table_finish(t, nviews, tmp, tmp_bytes, s);
}

// both tables of a call that has all its views at once
struct LbTables {
    LbTable rows, views;
    LbTables(GpCarver &cv, int64_t n, int32_t nviews) : rows(lb_table(cv, n)), views(lb_table(cv, nviews)) {}
};

inline int lb_entry_tables(const double *points, int64_t n, const int64_t *view_entry, int32_t nviews, const LbTables &t, char *tmp,
                           size_t tmp_bytes, unsigned long long *st, hipStream_t s) {
    LB_TRY(lb_row_table(points, n, t.rows, tmp, tmp_bytes, st, s));
    return lb_view_table(view_entry, nviews, t.views, tmp, tmp_bytes, st, s);
}

// ------------------------------------------------------------------------------------------------ per-view counts and the drop rule
// view_count = 0, the counts -- launch_counts(grid, view_count) launches the counting kernel --, keep
template <typename LaunchCounts>
int lb_counts_and_keep(LaunchCounts launch_counts, int64_t n, int32_t nviews, int64_t min_visible, int64_t max_visible, int64_t *view_count,
                       uint8_t *view_keep, hipStream_t s) {
    unsigned long long *vc = reinterpret_cast<unsigned long long *>(view_count);
    GP_CHECK_HIP(hipMemsetAsync(view_count, 0, (size_t)nviews * sizeof(int64_t), s));
    const unsigned nb = (unsigned)((n + 255) / 256);
    launch_counts(dim3(nb < 64 ? nb : 64, (unsigned)nviews), vc);
    lb_keep_kernel<<<(unsigned)((nviews + 255) / 256), 256, 0, s>>>(vc, nviews, min_visible, max_visible, view_keep);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

// over the sort's own tables (the form over a stream's state, every index of it checked: ls_view_counts, gp_lift_stream_state.h)
inline int lb_view_counts(const double *points, int64_t n, const int32_t *entry_rows, const int32_t *entry_off, const int64_t *view_entry,
                          const double *w2c, const double *intr, const double *depth, int32_t nviews, int32_t W, int32_t H, int32_t cut,
                          double tau, int64_t min_visible, int64_t max_visible, int64_t *view_count, uint8_t *view_keep, hipStream_t s) {
    return lb_counts_and_keep(
        [&](dim3 grid, unsigned long long *vc) {
            lb_counts_kernel<<<grid, 256, 0, s>>>(points, entry_rows, entry_off, view_entry, w2c, intr, depth, W, H, cut, tau, vc);
        },
        n, nviews, min_visible, max_visible, view_count, view_keep, s);
}

// ------------------------------------------------------------------------------------------------ the fill
struct LbFill {                                                  // what the fill needs beside the entry tables
    int32_t *ref, *qry, *rs, *qs, *rrow, *qpos;
    float *rxyz;
    LbFill(GpCarver &cv, int64_t n) {
        ref = cv.take<int32_t>(n + 1);
        qry = cv.take<int32_t>(n + 1);
        rs = cv.take<int32_t>(n + 1);
        qs = cv.take<int32_t>(n + 1);
        rrow = cv.take<int32_t>(n);
        qpos = cv.take<int32_t>(n);
        rxyz = cv.take<float>(3 * n);
    }
};

// keys / rows / off: the entry tables (the sort's, or the checked copies of a stream's state); mask: the rows that are references
// ("seen", or "voted"); status words ST_SEEN and ST_QUERIES; fill == 0 stops before the search, nn is then not written.
// tmp holds gp_scan_bytes<int32_t>(n + 1).
inline int lb_fill(const double *points, int64_t n, const uint32_t *keys, const int32_t *rows, const int32_t *off, const LbFill &f, char *tmp,
                   size_t tmp_bytes, const uint8_t *mask, int32_t fill, int64_t *nn, unsigned long long *st, hipStream_t s) {
    const unsigned nb = (unsigned)((n + 255) / 256), nb1 = (unsigned)((n + 1 + 255) / 256);
    lb_fill_flags_kernel<<<nb1, 256, 0, s>>>(keys, rows, mask, n, f.ref, f.qry);
    GP_CHECK_LAUNCH();
    size_t io = tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(tmp, io, f.ref, f.rs, (int32_t)0, (size_t)(n + 1), rocprim::plus<int32_t>(), s));
    io = tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(tmp, io, f.qry, f.qs, (int32_t)0, (size_t)(n + 1), rocprim::plus<int32_t>(), s));
    lb_fill_compact_kernel<<<nb, 256, 0, s>>>(points, rows, f.ref, f.qry, f.rs, f.qs, n, f.rxyz, f.rrow, f.qpos, st);
    if (fill) lb_fill_kernel<<<nb, 256, 0, s>>>(points, keys, rows, off, f.rs, f.qs, n, f.rxyz, f.rrow, f.qpos, nn, st);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

}  // namespace
