// The backward of the rows carried through neighbour lists (geopurify_amd/sparse.py: interpolate(differentiable=True),
// Neighbors.transpose): d_values [R,D] from g = d_out [M,D], exactly and reproducibly.  The role of the autograd that the reference
// gets from torch indexing wherever it carries features between clouds (models/affinity_module.py:445-452, 693-714: gather through
// KDTree lists); here for k neighbours, weights, an index and several entries at once, without float atomics.
//
// The rule.  A reference is a flat slot f = j*k + s whose forward weight is in effect: slot s of query row j is one the mode reads
// (all k, or slot 0 for "nearest"), its list entry and its row r of values are valid, and query row j is not excused (ki_list_rows,
// gp_knn_interp.h -- the forward's own definition).  d_values[r, c] starts at +0.f and takes, over the references of r in ascending f,
// acc = acc + w32[f] * g[j, c]: the product rounded once, the sum rounded once (-ffp-contract=off), w32 the forward's own fp32 weight.
// A row without references is an explicit zero row.  One rounding to the element type of values at the end.
//
// gp_knn_interpolate_weights: one wave per query row, the forward's device code, w32 [M,k] with 0 where no reference.
// gp_knn_interpolate_transpose: the key of a flat slot is its row r, nrows where it is no reference; a stable radix sort of (key, f)
// pairs over the bits of 0..nrows -- the pattern of mn_run (normals.hip) -- leaves every row's references together in ascending f;
// offsets by binary search (as lb_offsets_kernel), the weights gathered into the sorted order.  These lists depend on the lists, the
// index, the mode and eps alone: a training run builds them once.
// gp_knn_interpolate_backward: one wave per row of values, the workgroups striding the rows; lanes cover columns, the row's slots and
// weights are loaded 64 at a time, one per lane, and handed round the wave in order, so a list of any length is walked by the same
// code, serially per column.  No kernel waits on another workgroup; no atomics.
#include "gp_knn_interp.h"
#include "gp_lift_entries.h"

namespace {

constexpr int KG_MAX_K = GP_KNN_QUERY_MAX_K;
constexpr int KG_BLOCKS = 1 << 16;
constexpr int64_t KG_MAX_SLOTS = (1ll << 31) - 1;                // flat slots are i32

// KEYS: keys[f] = the row of flat slot f, nrows where it is no reference, and flat[f] = f; else w32[f] = its weight, 0 where none
template <bool KEYS>
__global__ void __launch_bounds__(256) kg_lists_kernel(const int64_t *__restrict__ indices, const double *__restrict__ dist2,
                                                       const int64_t *__restrict__ index, int64_t m, int k, int64_t npoints, int64_t nrows,
                                                       int mode, double eps, float *__restrict__ w32, uint32_t *__restrict__ keys,
                                                       int32_t *__restrict__ flat) {
    const int lane = gp_lane(), w = threadIdx.x >> 6;
    const int slots = mode == KI_NEAREST ? 1 : k;                    // <= KG_MAX_K
    for (int64_t q = (int64_t)blockIdx.x * 4 + w; q < m; q += (int64_t)gridDim.x * 4) {
        bool any_list, any_index;
        int64_t row;
        float wt = 0.f;
        if (KEYS) {
            double d2;
            row = ki_list_rows(indices, nullptr, index, q, k, slots, npoints, nrows, d2, any_list, any_index);
            if (any_list || any_index) row = -1;
        } else {
            row = ki_list_weights(indices, dist2, index, q, k, slots, npoints, nrows, mode, eps, wt, any_list, any_index);
        }
        if (lane < k) {
            const int64_t f = q * k + lane;                          // <= KG_MAX_SLOTS - 1
            if (KEYS) {
                keys[f] = row >= 0 ? (uint32_t)row : (uint32_t)nrows;
                flat[f] = (int32_t)f;
            } else {
                w32[f] = row >= 0 ? wt : 0.f;
            }
        }
    }
}

// offsets[r] = the first sorted position whose key is >= r, r = 0 .. nrows (keys are <= nrows: offsets[nrows] = the references)
__global__ void __launch_bounds__(256) kg_offsets_kernel(const uint32_t *__restrict__ keys_sorted, int64_t total, int64_t nrows,
                                                         int64_t *__restrict__ offsets) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (r > nrows) return;
    int64_t lo = 0, hi = total;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys_sorted[mid] < (uint32_t)r) lo = mid + 1;
        else hi = mid;
    }
    offsets[r] = lo;
}

// the weights in the sorted order; 0 past the references
__global__ void __launch_bounds__(256) kg_sorted_weights_kernel(const uint32_t *__restrict__ keys_sorted, const int32_t *__restrict__ slots,
                                                                const float *__restrict__ w32, int64_t total, int64_t nrows,
                                                                float *__restrict__ sorted) {
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p >= total) return;
    const int64_t f = slots[p];
    sorted[p] = (keys_sorted[p] < (uint32_t)nrows && (uint64_t)f < (uint64_t)total) ? w32[f] : 0.f;
}

// The references [a, e) of one row over VEC columns at c (live: the lane has such columns): 64 references per trip, lane i loading
// the i-th slot and weight, then in order through the wave.  A slot's query row is clamped where it is read.
template <int VEC>
__device__ __forceinline__ void kg_walk(const float *__restrict__ g, int64_t ldg, int64_t m, int k, const int32_t *__restrict__ slots,
                                        const float *__restrict__ weights, int64_t a, int64_t e, int64_t c, bool live, float (&acc)[VEC]) {
    const int lane = gp_lane();
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
    for (int64_t p0 = a; p0 < e; p0 += 64) {                         // (wave-uniform)
        const int64_t p = p0 + lane;
        int j = 0;
        float wj = 0.f;
        if (p < e) {
            const uint32_t q = (uint32_t)slots[p] / (uint32_t)k;
            if ((int64_t)q < m) { j = (int)q; wj = weights[p]; }     // (else cannot happen: the transpose wrote f < m * k)
        }
        const int cnt = e - p0 < 64 ? (int)(e - p0) : 64;
#pragma unroll 4
        for (int i = 0; i < cnt; ++i) {
            const int ji = __shfl(j, i, 64);
            const float wi = __shfl(wj, i, 64);
            if (live) {
                float x[VEC];
                gp_load_vec<VEC>(g + (int64_t)ji * ldg + c, x);
#pragma unroll
                for (int t = 0; t < VEC; ++t) acc[t] = acc[t] + wi * x[t];
            }
        }
    }
}

// One wave per row of values.  VEC columns per load of g where its base and pitch allow 16 bytes, the columns past the last whole
// group one by one; wide_store: VEC elements of out per store.  offsets are clamped where they are read.
template <typename TO, int VEC>
__global__ void __launch_bounds__(256) kg_backward_kernel(const float *__restrict__ g, int64_t ldg, int64_t m, int64_t d,
                                                          const int64_t *__restrict__ offsets, const int32_t *__restrict__ slots,
                                                          const float *__restrict__ weights, int k, int64_t nrows, int64_t total,
                                                          TO *__restrict__ out, int wide_store) {
    const int lane = gp_lane(), w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t whole = VEC > 1 ? d / VEC * VEC : 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < nrows; r += (int64_t)gridDim.x * 4) {
        int64_t a = offsets[r], e = offsets[r + 1];
        a = a < 0 ? 0 : (a > total ? total : a);
        e = e < a ? a : (e > total ? total : e);
        TO *o = out + r * d;
        for (int64_t cb = 0; cb < whole; cb += 64 * VEC) {           // (wave-uniform)
            const int64_t c = cb + (int64_t)lane * VEC;
            const bool live = c < whole;
            float acc[VEC];
            kg_walk<VEC>(g, ldg, m, k, slots, weights, a, e, c, live, acc);
            if (!live) continue;
            TO y[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) y[i] = gp_cvt<TO, float>(acc[i]);
            if (wide_store) gp_store_vec<VEC>(o + c, y);
            else {
#pragma unroll
                for (int i = 0; i < VEC; ++i) o[c + i] = y[i];
            }
        }
        for (int64_t cb = whole; cb < d; cb += 64) {
            const int64_t c = cb + lane;
            const bool live = c < d;
            float acc[1];
            kg_walk<1>(g, ldg, m, k, slots, weights, a, e, c, live, acc);
            if (live) o[c] = gp_cvt<TO, float>(acc[0]);
        }
    }
}

template <typename TO>
int kg_backward_run(const float *g, int64_t ldg, int64_t m, int64_t d, const int64_t *offsets, const int32_t *slots, const float *weights,
                    int k, int64_t nrows, void *out, hipStream_t s) {
    const int64_t nb = (nrows + 3) / 4, total = m * k;
    const unsigned grid = (unsigned)(nb < KG_BLOCKS ? nb : KG_BLOCKS);
    TO *o = static_cast<TO *>(out);
    if (d >= 4 && ldg % 4 == 0 && (uintptr_t)g % 16 == 0) {
        const int wide_store = (d % 4 == 0 && (uintptr_t)out % (4 * sizeof(TO)) == 0) ? 1 : 0;
        kg_backward_kernel<TO, 4><<<grid, 256, 0, s>>>(g, ldg, m, d, offsets, slots, weights, k, nrows, total, o, wide_store);
    } else {
        kg_backward_kernel<TO, 1><<<grid, 256, 0, s>>>(g, ldg, m, d, offsets, slots, weights, k, nrows, total, o, 0);
    }
    GP_CHECK_LAUNCH();
    return GP_OK;
}

inline int kg_key_bits(int64_t nrows) {                              // keys 0 .. nrows
    int bits = 1;
    while (bits < 32 && (nrows >> bits) != 0) ++bits;
    return bits;
}

size_t kg_sort_bytes(int64_t total, int bits) {
    size_t t = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (size_t)total, 0,
                                    bits, 0);
    return t;
}

struct KgWork {                                                  // the pairs before the sort, the sorted keys, the sort's scratch
    uint32_t *k0, *k1;
    int32_t *f0;
    char *tmp;
    size_t tmp_bytes;
    KgWork(GpCarver &cv, int64_t total, int64_t nrows) {
        k0 = cv.take<uint32_t>(total);
        k1 = cv.take<uint32_t>(total);
        f0 = cv.take<int32_t>(total);
        tmp_bytes = kg_sort_bytes(total, kg_key_bits(nrows));
        tmp = cv.take<char>(tmp_bytes);
    }
};

inline bool kg_sizes_ok(int64_t m, int32_t k, int64_t nrows) {
    return m >= 1 && k >= 1 && k <= KG_MAX_K && m <= KG_MAX_SLOTS / k && nrows >= 1 && nrows < (1ll << 31);
}

int kg_check_lists(const char *who, int64_t nrows, const int64_t *index, int64_t n_index, int64_t m, int32_t k, int64_t npoints, int32_t mode) {
    GP_CHECK_ARG(k >= 1 && k <= KG_MAX_K, "%s: k=%d not in 1..%d", who, k, KG_MAX_K);
    GP_CHECK_ARG(kg_sizes_ok(m, k, nrows), "%s: nrows=%lld, m=%lld, k=%d: nrows in 1..2^31-1, m >= 1, m * k <= 2^31-1", who, (long long)nrows,
                 (long long)m, k);
    GP_CHECK_ARG(index ? n_index >= 1 : n_index == 0, "%s: n_index=%lld %s an index", who, (long long)n_index, index ? "with" : "without");
    GP_CHECK_ARG(npoints == (index ? n_index : nrows), "%s: npoints=%lld is not the length of %s", who, (long long)npoints,
                 index ? "the index" : "values");
    GP_CHECK_ARG(mode == KI_INVERSE_DISTANCE || mode == KI_NEAREST, "%s: mode=%d (0 inverse distance, 1 nearest)", who, mode);
    return GP_OK;
}

inline unsigned kg_list_blocks(int64_t m) {
    const int64_t nb = (m + 3) / 4;
    return (unsigned)(nb < KG_BLOCKS ? nb : KG_BLOCKS);
}

}  // namespace

extern "C" int gp_knn_interpolate_weights(const int64_t *indices, const double *dist2, const int64_t *index, int64_t n_index, int64_t m,
                                          int32_t k, int64_t npoints, int64_t nrows, int32_t mode, double eps, float *weights, void *stream_) {
    const char *who = "gp_knn_interpolate_weights";
    GP_CHECK_ARG(indices && dist2 && weights, "%s: null argument", who);
    LB_TRY(kg_check_lists(who, nrows, index, n_index, m, k, npoints, mode));
    GP_CHECK_ARG(eps >= 0.0 && eps < INFINITY, "%s: eps=%g must be finite and not negative", who, eps);
    GP_CHECK_ARG((uintptr_t)indices % 8 == 0 && (uintptr_t)dist2 % 8 == 0 && (uintptr_t)index % 8 == 0 && (uintptr_t)weights % 4 == 0,
                 "%s: an array is not aligned to its element", who);
    {
        const void *const in[] = {indices, dist2, index};
        const size_t in_bytes[] = {(size_t)m * k * 8, (size_t)m * k * 8, (size_t)n_index * 8};
        const void *const o[] = {weights};
        const size_t o_bytes[] = {(size_t)m * k * 4};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    hipStream_t s = gp_stream(stream_);
    kg_lists_kernel<false><<<kg_list_blocks(m), 256, 0, s>>>(indices, dist2, index, m, k, npoints, nrows, mode, eps, weights, nullptr, nullptr);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" size_t gp_knn_interpolate_transpose_workspace_bytes(int64_t m, int32_t k, int64_t nrows) {
    if (!kg_sizes_ok(m, k, nrows)) return 0;
    GpCarver cv(nullptr, 0);
    KgWork kw(cv, m * k, nrows);
    return cv.off;
}

extern "C" int gp_knn_interpolate_transpose(const int64_t *indices, const int64_t *index, int64_t n_index, int64_t m, int32_t k, int64_t npoints,
                                            int64_t nrows, int32_t mode, const float *weights, int64_t *offsets, int32_t *slots,
                                            float *sorted_weights, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "gp_knn_interpolate_transpose";
    GP_CHECK_ARG(indices && weights && offsets && slots && sorted_weights && workspace, "%s: null argument", who);
    LB_TRY(kg_check_lists(who, nrows, index, n_index, m, k, npoints, mode));
    GP_CHECK_ARG((uintptr_t)indices % 8 == 0 && (uintptr_t)index % 8 == 0 && (uintptr_t)weights % 4 == 0 && (uintptr_t)offsets % 8 == 0 &&
                     (uintptr_t)slots % 4 == 0 && (uintptr_t)sorted_weights % 4 == 0,
                 "%s: an array is not aligned to its element", who);
    const int64_t total = m * k;
    {
        const void *const in[] = {indices, index, weights};
        const size_t in_bytes[] = {(size_t)total * 8, (size_t)n_index * 8, (size_t)total * 4};
        const void *const o[] = {offsets, slots, sorted_weights, workspace};
        const size_t o_bytes[] = {(size_t)(nrows + 1) * 8, (size_t)total * 4, (size_t)total * 4, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver cv(workspace, workspace_bytes);
    KgWork kw(cv, total, nrows);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    kg_lists_kernel<true><<<kg_list_blocks(m), 256, 0, s>>>(indices, nullptr, index, m, k, npoints, nrows, mode, 0.0, nullptr, kw.k0, kw.f0);
    GP_CHECK_LAUNCH();
    size_t io = kw.tmp_bytes;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(kw.tmp, io, kw.k0, kw.k1, kw.f0, slots, (size_t)total, 0, kg_key_bits(nrows), s));
    kg_offsets_kernel<<<(unsigned)((nrows + 1 + 255) / 256), 256, 0, s>>>(kw.k1, total, nrows, offsets);
    kg_sorted_weights_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(kw.k1, slots, weights, total, nrows, sorted_weights);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_knn_interpolate_backward(const float *g, int64_t ld_g, int64_t m, int64_t d, const int64_t *offsets, const int32_t *slots,
                                           const float *sorted_weights, int32_t k, int64_t nrows, void *out, int32_t out_elem, void *stream_) {
    const char *who = "gp_knn_interpolate_backward";
    GP_CHECK_ARG(g && offsets && slots && sorted_weights && out, "%s: null argument", who);
    LB_TRY(lb_check_elem(who, out_elem, out, "out"));
    GP_CHECK_ARG(k >= 1 && k <= KG_MAX_K, "%s: k=%d not in 1..%d", who, k, KG_MAX_K);
    GP_CHECK_ARG(kg_sizes_ok(m, k, nrows), "%s: nrows=%lld, m=%lld, k=%d: nrows in 1..2^31-1, m >= 1, m * k <= 2^31-1", who, (long long)nrows,
                 (long long)m, k);
    GP_CHECK_ARG(d >= 1 && ld_g >= d, "%s: d=%lld, ld_g=%lld: 1 <= d <= ld_g", who, (long long)d, (long long)ld_g);
    const size_t es = gp_elem_size(out_elem);
    GP_CHECK_ARG((uintptr_t)g % 4 == 0 && (uintptr_t)offsets % 8 == 0 && (uintptr_t)slots % 4 == 0 && (uintptr_t)sorted_weights % 4 == 0 &&
                     (uintptr_t)out % es == 0,
                 "%s: an array is not aligned to its element", who);
    const int64_t total = m * k;
    {
        const void *const in[] = {g, offsets, slots, sorted_weights};
        const size_t in_bytes[] = {((size_t)(m - 1) * ld_g + d) * 4, (size_t)(nrows + 1) * 8, (size_t)total * 4, (size_t)total * 4};
        const void *const o[] = {out};
        const size_t o_bytes[] = {(size_t)nrows * d * es};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    hipStream_t s = gp_stream(stream_);
    if (out_elem == GP_ELEM_F32) return kg_backward_run<float>(g, ld_g, m, d, offsets, slots, sorted_weights, k, nrows, out, s);
    if (out_elem == GP_ELEM_F16) return kg_backward_run<gp_f16>(g, ld_g, m, d, offsets, slots, sorted_weights, k, nrows, out, s);
    return kg_backward_run<gp_bf16>(g, ld_g, m, d, offsets, slots, sorted_weights, k, nrows, out, s);
}
