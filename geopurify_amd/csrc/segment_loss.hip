// Classification cross-entropy of SparseTensor rows against text embeddings, forward and gradient (geopurify_amd/sparse.py:
// segment_loss): with u_i = y_i / max(|y_i|, 1e-12), z_ic = s <u_i, t_c> and lse_i = log sum_c exp(z_ic),
//     loss = sum over the valid items p of  w_b(p) (lse_i(p) - z_i(p),l_p)          dz_ic = w_b(i) (m_i softmax_ic - cnt_ic)
// The two products Z = U T^T and dU = s G T run on gp_sparse_conv's exact-fp32 matrix-core GEMM; this file holds what stands around
// them: the unit rows and zero flags, the valid items (per voxel, or per point through a quantiser's inverse map: a CSR of items by
// row from integer counts + a rocPRIM scan + a stable rocPRIM sort, the build of gp_pool_transpose_build), the row kernel (one wave
// per row of a chunk of logits: stable softmax, G, lse and the row's loss term) and the fixed-order fp64 reduction of the row terms
// into the loss and the per-entry means.  No float atomics anywhere: every sum runs in an order that depends on the data alone, so
// two calls give the same bits.
#include "gp_common.h"
#include "gp_scan_bytes.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

constexpr int SL_MAX_ENTRIES = 65536;
constexpr int SL_MAX_CLASSES = 4096;
constexpr int SL_MAX_IGNORE = 4;
constexpr int SL_COL_STEP = GP_WAVE;          // the row kernels: lane l owns the columns l, l + 64, ...

struct SlIgnore {
    int64_t id[SL_MAX_IGNORE];
    int n;
};

inline bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }

// the byte ranges [a, a + na) and [b, b + nb) share a byte (a NULL pointer overlaps nothing)
inline bool sl_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// bytes of r rows of `cols` elements with a pitch of ld elements
inline size_t sl_rows_bytes(int64_t r, int64_t ld, int64_t cols, size_t elem) { return (size_t)((r - 1) * ld + cols) * elem; }

// ------------------------------------------------------------------------------------------------
// u_i = y_i / max(|y_i|, 1e-12) with zero columns d .. d_pad-1, zero_i = (sum |y_i| == 0): one wave per row
__global__ void __launch_bounds__(256) sl_unit_rows_kernel(const float *__restrict__ y, int64_t ld_y, int d, int64_t n,
                                                           float *__restrict__ u, int64_t ld_u, int d_pad, uint8_t *__restrict__ zero) {
    const int64_t r = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    if (r >= n) return;
    const int lane = gp_lane();
    const float *yr = y + r * ld_y;
    float ss = 0.f, sa = 0.f;
    for (int c = lane; c < d; c += SL_COL_STEP) {
        const float v = yr[c];
        ss += v * v;
        sa += fabsf(v);
    }
    ss = gp_wave_sum(ss);
    sa = gp_wave_sum(sa);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
    float *ur = u + r * ld_u;
    for (int c = lane; c < d_pad; c += SL_COL_STEP) ur[c] = c < d ? yr[c] / nrm : 0.f;
    if (lane == 0) zero[r] = sa == 0.f ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// status[0] = rows with a batch index outside 0..65535, status[2] = the highest batch index inside it
// (reduced over the wave first: one atomic per wave and word)
__global__ void __launch_bounds__(256) sl_rows_batch_kernel(const int32_t *__restrict__ coords, int64_t n,
                                                            unsigned long long *__restrict__ status) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const bool live = r < n;
    const int32_t b = live ? coords[r * 4] : 0;
    const bool bad = live && (uint32_t)b >= (uint32_t)SL_MAX_ENTRIES;
    const int nbad = __popcll(__ballot(bad));
    int top = live && !bad ? b : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
    if (gp_lane() == 0) {
        if (nbad) atomicAdd(status + 0, (unsigned long long)nbad);
        if (top >= 0) atomicMax(status + 2, (unsigned long long)top);
    }
}

// valid items: key = the item's row (n for an invalid item: such items sort behind every list and are in none), counts per row and
// per entry by integer atomics (they do not depend on the order of arrival; one atomic per wave and entry)
__global__ void __launch_bounds__(256) sl_items_kernel(const int32_t *__restrict__ coords, const uint8_t *__restrict__ zero, int64_t n,
                                                       const int64_t *__restrict__ labels, const int64_t *__restrict__ index, int64_t p_total,
                                                       int c, SlIgnore ig, uint8_t *__restrict__ row_valid, uint32_t *__restrict__ keys,
                                                       int32_t *__restrict__ ids, unsigned long long *__restrict__ row_cnt,
                                                       unsigned long long *__restrict__ entry_cnt, unsigned long long *__restrict__ status) {
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const bool live = p < p_total;
    bool valid = false;
    int64_t r = 0;
    int32_t b = 0;
    if (live) {
        r = index ? index[p] : p;
        const bool in = (uint64_t)r < (uint64_t)n;
        if (!in) atomicAdd(status + 1, 1ull);
        const int64_t l = labels[p];
        valid = in && l >= 0 && l < c;
        for (int i = 0; i < ig.n; ++i) valid = valid && l != ig.id[i];
        if (valid) {
            b = coords[r * 4];
            valid = !zero[r] && (uint32_t)b < (uint32_t)SL_MAX_ENTRIES;
        }
        if (index) {
            keys[p] = valid ? (uint32_t)r : (uint32_t)n;
            ids[p] = (int32_t)p;
            if (valid) atomicAdd(row_cnt + r, 1ull);
        } else {
            row_valid[p] = valid ? 1 : 0;
        }
    }
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const int32_t bf = __shfl(b, first, 64);
        const unsigned long long same = __ballot(valid && b == bf) & todo;
        if (gp_lane() == first) atomicAdd(entry_cnt + bf, (unsigned long long)__popcll(same));
        todo &= ~same;
    }
}

// V = all valid items, E = the entries that hold one; w_b = 1 / V ("item") or 1 / (E V_b) ("entry"), 0 for an entry without items.
// One block; integer sums.
__global__ void __launch_bounds__(1024) sl_entry_weights_kernel(const unsigned long long *__restrict__ entry_cnt, int reduction,
                                                                float *__restrict__ entry_w, unsigned long long *__restrict__ status) {
    __shared__ unsigned long long tot[2];
    if (threadIdx.x < 2) tot[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long v = 0, e = 0;
    for (int b = threadIdx.x; b < SL_MAX_ENTRIES; b += 1024) {
        const unsigned long long c = entry_cnt[b];
        v += c;
        e += c > 0;
    }
    atomicAdd(&tot[0], v);
    atomicAdd(&tot[1], e);
    __syncthreads();
    const double V = (double)tot[0], E = (double)tot[1];
    for (int b = threadIdx.x; b < SL_MAX_ENTRIES; b += 1024) {
        const unsigned long long c = entry_cnt[b];
        entry_w[b] = c == 0 ? 0.f : (float)(reduction ? 1.0 / (E * (double)c) : 1.0 / V);
    }
    if (threadIdx.x == 0) status[3] = tot[0];
}

int sl_key_bits(int64_t top) {                                   // keys are 0 .. top
    int bits = 1;
    while (bits < 32 && (1ll << bits) <= top) ++bits;
    return bits;
}

size_t sl_sort_bytes(int64_t total, int bits) {
    size_t t = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
                                    (size_t)total, 0, bits, 0);
    return t;
}

// ------------------------------------------------------------------------------------------------
// the row kernel: one wave per row of a chunk of logits z [r, ld_z].  Items of the row: item_off / item_id (a CSR, ascending item
// numbers; labels indexed by item) or, without it, the row itself where row_valid is set (labels indexed by row).
//   g[i,c]  = w_i (m_i softmax_ic - cnt_ic), columns c .. c_pad-1 exact zeros   (m_i p_ic first, then 1 off per item in list order at
//             its label -- integers, so one class gives exactly 0 --, then the weight)
//   lse[i]  = max + log sum exp(z - max),   term[i] = m_i lse_i - sum over the items of z_i,l  (fp64)
// A row without items stores zeros and reads no logits.  g == nullptr: lse and term alone (the forward), nothing else is stored.
__global__ void __launch_bounds__(256) sl_rows_kernel(const float *__restrict__ z, int64_t ld_z, int64_t r_total, int c, int c_pad,
                                                      const int32_t *__restrict__ coords, const uint8_t *__restrict__ row_valid,
                                                      const int64_t *__restrict__ item_off, const int32_t *__restrict__ item_id,
                                                      const int64_t *__restrict__ labels, const float *__restrict__ entry_w,
                                                      float *g, int64_t ld_g, float *__restrict__ lse, double *__restrict__ term) {
    int64_t row = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    if (row >= r_total) return;
    row = __builtin_amdgcn_readfirstlane((int)row);
    const int lane = gp_lane();
    int64_t p0, p1;
    if (item_off) {
        p0 = item_off[row];
        p1 = item_off[row + 1];
    } else {
        p0 = row;
        p1 = row + (row_valid[row] ? 1 : 0);
    }
    float *grow = g ? g + row * ld_g : nullptr;
    const int64_t m = p1 - p0;
    if (m <= 0) {
        if (grow)
            for (int k = lane; k < c_pad; k += SL_COL_STEP) grow[k] = 0.f;
        if (lane == 0) {
            lse[row] = 0.f;
            term[row] = 0.0;
        }
        return;
    }
    const float *zr = z + row * ld_z;
    float mx = -INFINITY;
    for (int k = lane; k < c; k += SL_COL_STEP) mx = fmaxf(mx, zr[k]);
    mx = gp_wave_max(mx);
    float se = 0.f;
    for (int k = lane; k < c; k += SL_COL_STEP) se += expf(zr[k] - mx);
    se = gp_wave_sum(se);
    const float l = mx + logf(se);
    const float fm = (float)m;
    if (grow)
        for (int k = lane; k < c_pad; k += SL_COL_STEP) grow[k] = k < c ? fm * (expf(zr[k] - mx) / se) : 0.f;
    // the items in list order, 64 labels per load; column k belongs to lane k % 64, which wrote it above
    double zs = 0.0;
    for (int64_t q = p0; q < p1; q += GP_WAVE) {
        const int cnt = (int)(p1 - q < GP_WAVE ? p1 - q : GP_WAVE);
        int lab = -1;
        if (lane < cnt) {
            const int64_t v = labels[item_off ? (int64_t)item_id[q + lane] : q + lane];
            lab = (uint64_t)v < (uint64_t)c ? (int)v : -1;
        }
        double zv = lab >= 0 ? (double)zr[lab] : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) zv += __shfl_xor(zv, o, 64);
        zs += zv;
        if (grow)
            for (int t = 0; t < cnt; ++t) {
                const int lt = __shfl(lab, t, 64);
                if (lt >= 0 && lane == (lt & (SL_COL_STEP - 1))) grow[lt] -= 1.f;
            }
    }
    if (grow) {
        const int32_t b = coords[row * 4];
        const float w = entry_w[(uint32_t)b < (uint32_t)SL_MAX_ENTRIES ? b : 0];
        for (int k = lane; k < c; k += SL_COL_STEP) grow[k] *= w;
    }
    if (lane == 0) {
        lse[row] = l;
        term[row] = (double)m * (double)l - zs;
    }
}

// ------------------------------------------------------------------------------------------------
// the reduction: rows sorted by entry (stable), one block per entry sums its rows' terms in fp64 -- thread t the rows t, t + 256, ...
// of the entry's list, then a tree over the threads --, one block sums the weighted entry sums the same way
__global__ void sl_entry_keys_kernel(const int32_t *__restrict__ coords, int64_t n, int num_entries, uint32_t *__restrict__ keys,
                                     int32_t *__restrict__ rows) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int32_t b = coords[r * 4];
    keys[r] = (uint32_t)b < (uint32_t)num_entries ? (uint32_t)b : (uint32_t)num_entries;
    rows[r] = (int32_t)r;
}

__device__ __forceinline__ int64_t sl_lower_bound(const uint32_t *keys, int64_t n, uint32_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double sl_block_sum(double v, double *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

__global__ void __launch_bounds__(256) sl_entry_sums_kernel(const double *__restrict__ term, const uint32_t *__restrict__ keys,
                                                            const int32_t *__restrict__ rows, int64_t n, double *__restrict__ sums) {
    __shared__ double sh[256];
    const uint32_t b = blockIdx.x;
    const int64_t lo = sl_lower_bound(keys, n, b), hi = sl_lower_bound(keys, n, b + 1);
    double v = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) v += term[rows[i]];
    v = sl_block_sum(v, sh);
    if (threadIdx.x == 0) sums[b] = v;
}

__global__ void __launch_bounds__(256) sl_loss_kernel(const double *__restrict__ sums, const unsigned long long *__restrict__ entry_cnt,
                                                      int num_entries, int reduction, float *__restrict__ loss,
                                                      float *__restrict__ per_entry) {
    __shared__ double sh[256];
    __shared__ unsigned long long tot[2];
    if (threadIdx.x < 2) tot[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long v = 0, e = 0;
    for (int b = threadIdx.x; b < num_entries; b += 256) {
        const unsigned long long c = entry_cnt[b];
        v += c;
        e += c > 0;
    }
    atomicAdd(&tot[0], v);
    atomicAdd(&tot[1], e);
    __syncthreads();
    const double V = (double)tot[0], E = (double)tot[1];
    double acc = 0.0;
    for (int b = threadIdx.x; b < num_entries; b += 256) {
        const unsigned long long c = entry_cnt[b];
        if (c > 0) acc += sums[b] * (reduction ? 1.0 / (E * (double)c) : 1.0 / V);
        per_entry[b] = c > 0 ? (float)(sums[b] / (double)c) : __builtin_nanf("");
    }
    acc = sl_block_sum(acc, sh);
    if (threadIdx.x == 0) *loss = (float)acc;
}

}  // namespace

extern "C" int32_t gp_segment_loss_col_step(void) { return SL_COL_STEP; }

extern "C" int gp_segment_loss_unit_rows(const float *y, int64_t ld_y, int32_t d, int64_t n, float *u, int64_t ld_u, int32_t d_pad,
                                         uint8_t *zero, void *stream_) {
    GP_CHECK_ARG(y && u && zero && n > 0 && n < (1ll << 31), "gp_segment_loss_unit_rows: null/empty argument (1 <= n < 2^31)");
    GP_CHECK_ARG(d >= 1 && d_pad >= d && ld_y >= d && ld_u >= d_pad, "gp_segment_loss_unit_rows: d=%d, d_pad=%d, pitches %lld / %lld", d, d_pad,
                 (long long)ld_y, (long long)ld_u);
    GP_CHECK_ARG((uintptr_t)y % 4 == 0 && (uintptr_t)u % 4 == 0, "gp_segment_loss_unit_rows: y/u must be 4-byte aligned");
    {
        const size_t by = sl_rows_bytes(n, ld_y, d, 4), bu = sl_rows_bytes(n, ld_u, d_pad, 4);
        GP_CHECK_ARG(!sl_overlap(u, bu, y, by) && !sl_overlap(zero, (size_t)n, y, by) && !sl_overlap(zero, (size_t)n, u, bu),
                     "gp_segment_loss_unit_rows: the outputs must not overlap y or each other");
    }
    sl_unit_rows_kernel<<<(unsigned)((n * 64 + 255) / 256), 256, 0, gp_stream(stream_)>>>(y, ld_y, d, n, u, ld_u, d_pad, zero);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" size_t gp_segment_loss_items_workspace_bytes(int64_t n, int64_t p) {
    if (n <= 0 || p <= 0 || n >= (1ll << 31) || p >= (1ll << 31)) return 0;
    GpCarver cv(nullptr, 0);
    cv.take<int64_t>(n + 1);
    cv.take<uint32_t>(p);
    cv.take<uint32_t>(p);
    cv.take<int32_t>(p);
    cv.take<char>(gp_scan_bytes<int64_t>(n + 1));
    cv.take<char>(sl_sort_bytes(p, sl_key_bits(n)));
    return cv.off;
}

extern "C" int gp_segment_loss_items(const int32_t *coords, const uint8_t *zero, int64_t n, const int64_t *labels, const int64_t *index,
                                     int64_t p, int32_t c, const int64_t *ignore_ids_host, int32_t num_ignore, int32_t reduction,
                                     uint8_t *row_valid, int64_t *item_off, int32_t *item_id, int64_t *entry_cnt, float *entry_w,
                                     int64_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    GP_CHECK_ARG(coords && zero && labels && entry_cnt && entry_w && status, "gp_segment_loss_items: null argument");
    GP_CHECK_ARG(n > 0 && n < (1ll << 31) && p > 0 && p < (1ll << 31), "gp_segment_loss_items: rows and items must be in 1..2^31-1");
    GP_CHECK_ARG(c >= 1 && c <= SL_MAX_CLASSES, "gp_segment_loss_items: c=%d outside 1..%d", c, SL_MAX_CLASSES);
    GP_CHECK_ARG(num_ignore >= 0 && num_ignore <= SL_MAX_IGNORE && (num_ignore == 0 || ignore_ids_host),
                 "gp_segment_loss_items: %d ignore labels, at most %d", num_ignore, SL_MAX_IGNORE);
    GP_CHECK_ARG(reduction == 0 || reduction == 1, "gp_segment_loss_items: reduction=%d (0 item, 1 entry)", reduction);
    if (index) GP_CHECK_ARG(item_off && item_id && workspace, "gp_segment_loss_items: an index takes item_off, item_id and a workspace");
    else GP_CHECK_ARG(row_valid && p == n, "gp_segment_loss_items: without an index the items are the rows (p == n) and row_valid is written");
    {
        // every output against every input and every other output, over their whole extents
        const void *in[] = {coords, zero, labels, index};
        const size_t in_bytes[] = {(size_t)n * 16, (size_t)n, (size_t)p * 8, (size_t)p * 8};
        const void *out[] = {index ? nullptr : row_valid, index ? item_off : nullptr, index ? item_id : nullptr, entry_cnt, entry_w, status,
                             index ? workspace : nullptr};
        const size_t out_bytes[] = {(size_t)n, (size_t)(n + 1) * 8, (size_t)p * 4, (size_t)SL_MAX_ENTRIES * 8, (size_t)SL_MAX_ENTRIES * 4, 32,
                                    workspace_bytes};
        for (int o = 0; o < 7; ++o) {
            for (int i = 0; i < 4; ++i)
                GP_CHECK_ARG(!sl_overlap(out[o], out_bytes[o], in[i], in_bytes[i]), "gp_segment_loss_items: an output overlaps an input");
            for (int q = o + 1; q < 7; ++q)
                GP_CHECK_ARG(!sl_overlap(out[o], out_bytes[o], out[q], out_bytes[q]), "gp_segment_loss_items: two outputs overlap");
        }
    }
    hipStream_t s = gp_stream(stream_);
    SlIgnore ig;
    ig.n = num_ignore;
    for (int i = 0; i < SL_MAX_IGNORE; ++i) ig.id[i] = i < num_ignore ? ignore_ids_host[i] : 0;
    int64_t *cnt = nullptr;
    uint32_t *k0 = nullptr, *k1 = nullptr;
    int32_t *v0 = nullptr;
    char *ts = nullptr, *tt = nullptr;
    size_t scan_tmp = 0, sort_tmp = 0;
    const int bits = sl_key_bits(n);
    if (index) {
        scan_tmp = gp_scan_bytes<int64_t>(n + 1);
        sort_tmp = sl_sort_bytes(p, bits);
        GpCarver cv(workspace, workspace_bytes);
        cnt = cv.take<int64_t>(n + 1);
        k0 = cv.take<uint32_t>(p);
        k1 = cv.take<uint32_t>(p);
        v0 = cv.take<int32_t>(p);
        ts = cv.take<char>(scan_tmp);
        tt = cv.take<char>(sort_tmp);
        if (!cv.ok()) {
            gp_set_error("gp_segment_loss_items: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
            return GP_ENOMEM;
        }
        GP_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)(n + 1) * sizeof(int64_t), s));
    }
    GP_CHECK_HIP(hipMemsetAsync(entry_cnt, 0, (size_t)SL_MAX_ENTRIES * sizeof(int64_t), s));
    GP_CHECK_HIP(hipMemsetAsync(status, 0, 4 * sizeof(int64_t), s));
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    sl_rows_batch_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(coords, n, st);
    GP_CHECK_LAUNCH();
    sl_items_kernel<<<(unsigned)((p + 255) / 256), 256, 0, s>>>(coords, zero, n, labels, index, p, c, ig, row_valid, k0, v0,
                                                               reinterpret_cast<unsigned long long *>(cnt),
                                                               reinterpret_cast<unsigned long long *>(entry_cnt), st);
    GP_CHECK_LAUNCH();
    sl_entry_weights_kernel<<<1, 1024, 0, s>>>(reinterpret_cast<unsigned long long *>(entry_cnt), reduction, entry_w, st);
    GP_CHECK_LAUNCH();
    if (index) {
        size_t io = scan_tmp;
        GP_CHECK_HIP(rocprim::exclusive_scan(ts, io, cnt, item_off, (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>(), s));
        io = sort_tmp;
        GP_CHECK_HIP(rocprim::radix_sort_pairs(tt, io, k0, k1, v0, item_id, (size_t)p, 0, bits, s));   // (stable: items ascend inside a row)
    }
    return GP_OK;
}

extern "C" int gp_segment_loss_rows(const float *z, int64_t ld_z, int64_t r, int32_t c, int32_t c_pad, const int32_t *coords,
                                    const uint8_t *row_valid, const int64_t *item_off, const int32_t *item_id, const int64_t *labels,
                                    const float *entry_w, float *g, int64_t ld_g, float *lse, double *term, void *stream_) {
    GP_CHECK_ARG(z && coords && labels && entry_w && lse && term && r > 0, "gp_segment_loss_rows: null/empty argument");
    GP_CHECK_ARG((item_off && item_id) || (!item_off && !item_id && row_valid),
                 "gp_segment_loss_rows: items come as item_off + item_id, or as row_valid alone");
    GP_CHECK_ARG(c >= 1 && c <= SL_MAX_CLASSES, "gp_segment_loss_rows: c=%d outside 1..%d", c, SL_MAX_CLASSES);
    GP_CHECK_ARG(c_pad >= c && ld_z >= c && (!g || ld_g >= c_pad), "gp_segment_loss_rows: c=%d, c_pad=%d, pitches %lld / %lld", c, c_pad,
                 (long long)ld_z, (long long)ld_g);
    GP_CHECK_ARG(ld_z % 4 == 0 && aligned16(z) && (!g || (ld_g % 4 == 0 && aligned16(g))), "gp_segment_loss_rows: z/g rows must be 16-byte aligned");
    GP_CHECK_ARG(r * ld_z < (1ll << 31) && (!g || r * ld_g < (1ll << 31)), "gp_segment_loss_rows: r * ld must stay below 2^31 (r=%lld)",
                 (long long)r);
    {
        // every output against every input and every other output, over the extents the call knows: labels and item_id are indexed
        // by item number in the per-point form, their lengths are not arguments, so there they count from their first element on
        const void *in[] = {z, coords, row_valid, item_off, item_id, labels, entry_w};
        const size_t in_bytes[] = {sl_rows_bytes(r, ld_z, c, 4), (size_t)r * 16, (size_t)r, (size_t)(r + 1) * 8, 4,
                                   item_off ? (size_t)8 : (size_t)r * 8, (size_t)SL_MAX_ENTRIES * 4};
        const void *out[] = {g, lse, term};
        const size_t out_bytes[] = {g ? sl_rows_bytes(r, ld_g, c_pad, 4) : 0, (size_t)r * 4, (size_t)r * 8};
        for (int o = 0; o < 3; ++o) {
            for (int i = 0; i < 7; ++i)
                GP_CHECK_ARG(!sl_overlap(out[o], out_bytes[o], in[i], in_bytes[i]), "gp_segment_loss_rows: an output overlaps an input");
            for (int q = o + 1; q < 3; ++q)
                GP_CHECK_ARG(!sl_overlap(out[o], out_bytes[o], out[q], out_bytes[q]), "gp_segment_loss_rows: two outputs overlap");
        }
    }
    sl_rows_kernel<<<(unsigned)((r * 64 + 255) / 256), 256, 0, gp_stream(stream_)>>>(z, ld_z, r, c, c_pad, coords, row_valid, item_off, item_id,
                                                                                    labels, entry_w, g, ld_g, lse, term);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" size_t gp_segment_loss_reduce_workspace_bytes(int64_t n, int32_t num_entries) {
    if (n <= 0 || n >= (1ll << 31) || num_entries < 1 || num_entries > SL_MAX_ENTRIES) return 0;
    GpCarver cv(nullptr, 0);
    cv.take<uint32_t>(n);
    cv.take<uint32_t>(n);
    cv.take<int32_t>(n);
    cv.take<int32_t>(n);
    cv.take<double>(num_entries);
    cv.take<char>(sl_sort_bytes(n, sl_key_bits(num_entries)));
    return cv.off;
}

extern "C" int gp_segment_loss_reduce(const double *term, const int32_t *coords, int64_t n, const int64_t *entry_cnt, int32_t num_entries,
                                      int32_t reduction, float *loss, float *per_entry, void *workspace, size_t workspace_bytes,
                                      void *stream_) {
    GP_CHECK_ARG(term && coords && entry_cnt && loss && per_entry && workspace, "gp_segment_loss_reduce: null argument");
    GP_CHECK_ARG(n > 0 && n < (1ll << 31), "gp_segment_loss_reduce: n=%lld outside 1..2^31-1", (long long)n);
    GP_CHECK_ARG(num_entries >= 1 && num_entries <= SL_MAX_ENTRIES, "gp_segment_loss_reduce: %d entries outside 1..%d", num_entries, SL_MAX_ENTRIES);
    GP_CHECK_ARG(reduction == 0 || reduction == 1, "gp_segment_loss_reduce: reduction=%d (0 item, 1 entry)", reduction);
    {
        const void *in[] = {term, coords, entry_cnt};
        const size_t in_bytes[] = {(size_t)n * 8, (size_t)n * 16, (size_t)num_entries * 8};
        const void *out[] = {loss, per_entry, workspace};
        const size_t out_bytes[] = {4, (size_t)num_entries * 4, workspace_bytes};
        for (int o = 0; o < 3; ++o) {
            for (int i = 0; i < 3; ++i)
                GP_CHECK_ARG(!sl_overlap(out[o], out_bytes[o], in[i], in_bytes[i]), "gp_segment_loss_reduce: an output overlaps an input");
            for (int q = o + 1; q < 3; ++q)
                GP_CHECK_ARG(!sl_overlap(out[o], out_bytes[o], out[q], out_bytes[q]), "gp_segment_loss_reduce: two outputs overlap");
        }
    }
    const int bits = sl_key_bits(num_entries);
    const size_t sort_tmp = sl_sort_bytes(n, bits);
    GpCarver cv(workspace, workspace_bytes);
    uint32_t *k0 = cv.take<uint32_t>(n);
    uint32_t *k1 = cv.take<uint32_t>(n);
    int32_t *v0 = cv.take<int32_t>(n);
    int32_t *v1 = cv.take<int32_t>(n);
    double *sums = cv.take<double>(num_entries);
    char *tt = cv.take<char>(sort_tmp);
    if (!cv.ok()) {
        gp_set_error("gp_segment_loss_reduce: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    sl_entry_keys_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(coords, n, num_entries, k0, v0);
    GP_CHECK_LAUNCH();
    size_t io = sort_tmp;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(tt, io, k0, k1, v0, v1, (size_t)n, 0, bits, s));             // (stable: rows ascend inside an entry)
    sl_entry_sums_kernel<<<(unsigned)num_entries, 256, 0, s>>>(term, k1, v1, n, sums);
    GP_CHECK_LAUNCH();
    sl_loss_kernel<<<1, 256, 0, s>>>(sums, reinterpret_cast<const unsigned long long *>(entry_cnt), num_entries, reduction, loss, per_entry);
    GP_CHECK_LAUNCH();
    return GP_OK;
}
