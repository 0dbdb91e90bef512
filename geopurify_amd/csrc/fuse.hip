// Fused-feature files from lifted BATCHED point clouds, and back: the writer the reader of dataset/feature_loader.py:113-192 never had
// (its settings: config/fusion_scannet.yaml:34-35, n_split_points and num_rand_file_per_scene), for all entries and all files at once.
//
// Per entry b -- its points the rows with batch b in ascending row order, local index i -- and file k:
//     chunk_k = every point of the entry when n_split <= 0 (None) or n_b <= n_split, else the n_split points with the smallest key
//     h = fmix32(i ^ c),  c = fmix32(k ^ fmix32(b ^ fmix32(seed_lo ^ fmix32(seed_hi))))        (fmix32: murmur3's 32-bit finaliser)
// fmix32 is a bijection, so the keys of one (entry, file) are distinct and the chunk is the set {h <= T}, T the key of rank
// n_split - 1: no ties, no dependence on the row interleaving or on any arrival order.
//     merged form: mask_full = chunk & seen;   chunk form: mask_full = chunk, and mask = seen at the file's rows
// feat holds the rows of features where mask_full, file after file, inside a file entry after entry in ascending row order:
// the order of the entry tables of gp_lift_entries.h (rows sorted stably by entry).
//
// gp_fuse_plan:  entry tables -> T per selecting (file, entry) by a radix select over the 32-bit key (four 8-bit passes, keys
//   recomputed from (b, k, i) in every pass -- no [files, n] key array; per-block LDS histograms, integer atomics into [pair, 256]:
//   exact and order-free; a one-block kernel per pair picks the digit and the remaining rank) -> per file: flags in the entry-sorted
//   order, mask_full, an exclusive scan (rocPRIM) kept in the caller's state.  status[4] = the rows of feat.
// gp_fuse_write: offsets [files, entries + 1] from the scans, then one wave per source row: the row is loaded once, converted once and
//   stored to every file that holds it (16 / 8-byte accesses where the width and both bases allow, 4 / 2-byte otherwise).
// gp_fuse_dense: the inverse, the loader's evaluation form (:119-126) on unvoxelized points: out[p] = mask_full[p] ? feat[rank(p)] : 0.
#include "gp_lift_entries.h"
#include "gp_map_elem.h"

namespace {

constexpr int FU_MAX_FILES = 16;
constexpr int FU_HIST_BLOCKS = 64;                               // blocks of 256 keys-per-step that share one pair's histogram
enum { FU_MERGED = 0, FU_CHUNK = 1 };
enum { FU_ROWS = 4, FU_MASK_ROWS = 4 };                          // status words beside ST_BAD_BATCH and ST_TOP_BATCH

__host__ __device__ __forceinline__ uint32_t fu_fmix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}
// cs = fmix32(seed_lo ^ fmix32(seed_hi)) comes from the host
__device__ __forceinline__ uint32_t fu_pair_const(uint32_t cs, uint32_t b, uint32_t k) { return fu_fmix32(k ^ fu_fmix32(b ^ cs)); }

// ------------------------------------------------------------------------------------------------ entry tables (batch column only)
__global__ void __launch_bounds__(256) fu_row_keys_kernel(const double *__restrict__ points, int64_t n, uint32_t *__restrict__ keys,
                                                          int32_t *__restrict__ rows, unsigned long long *__restrict__ status) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    bool bad = false;
    int b = -1;
    if (r < n) {
        b = lb_entry_of(points[r * 4]);
        bad = b < 0;
        keys[r] = b >= 0 ? (uint32_t)b : (uint32_t)LB_MAX_ENTRIES;
        rows[r] = (int32_t)r;
    }
    const int nbad = __popcll(__ballot(bad));
    int top = b;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
    if (gp_lane() == 0) {
        if (nbad) atomicAdd(status + ST_BAD_BATCH, (unsigned long long)nbad);
        if (top >= 0) atomicMax(status + ST_TOP_BATCH, (unsigned long long)top);
    }
}

// ------------------------------------------------------------------------------------------------ the selection
// sel[b] = entry b has more than n_split points (b = 0 .. 65535; sel[65536] = 0 closes the scan)
__global__ void __launch_bounds__(256) fu_sel_flags_kernel(const int32_t *__restrict__ entry_off, int64_t n_split, int32_t *__restrict__ sel) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > LB_MAX_ENTRIES) return;
    sel[b] = (b < LB_MAX_ENTRIES && (int64_t)(entry_off[b + 1] - entry_off[b]) > n_split) ? 1 : 0;
}

// the selecting entries listed; every pair starts at prefix 0 with rank n_split - 1.  sel_idx[b] < cap: cap bounds the entries that
// have more than n_split of the n points
__global__ void __launch_bounds__(256) fu_sel_list_kernel(const int32_t *__restrict__ sel, const int32_t *__restrict__ sel_idx, int64_t n_split,
                                                          int num_files, int64_t cap, int32_t *__restrict__ sel_list,
                                                          uint32_t *__restrict__ prefix, uint32_t *__restrict__ rank) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= LB_MAX_ENTRIES || !sel[b]) return;
    const int64_t j = sel_idx[b];
    if (j >= cap) return;
    sel_list[j] = b;
    for (int k = 0; k < num_files; ++k) {
        prefix[k * cap + j] = 0;
        rank[k * cap + j] = (uint32_t)(n_split - 1);
    }
}

// grid (cap, FU_HIST_BLOCKS, files): the digit histogram, at `shift`, of the keys of pair (k, j) that agree with its prefix above
__global__ void __launch_bounds__(256) fu_hist_kernel(const int32_t *__restrict__ entry_off, const int32_t *__restrict__ sel_list,
                                                      const int32_t *__restrict__ sel_idx, uint32_t cs, const uint32_t *__restrict__ prefix,
                                                      int shift, int64_t cap, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[256];
    const int64_t j = blockIdx.x;
    if (j >= sel_idx[LB_MAX_ENTRIES]) return;                    // (block-uniform)
    const uint32_t b = (uint32_t)sel_list[j], k = blockIdx.z;
    const uint32_t nb = (uint32_t)(entry_off[b + 1] - entry_off[b]);
    if (blockIdx.y * 256u >= nb) return;                         // (block-uniform)
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t c = fu_pair_const(cs, b, k), pfx = prefix[k * cap + j];
    for (uint32_t i = blockIdx.y * 256u + threadIdx.x; i < nb; i += gridDim.y * 256u) {
        const uint32_t key = fu_fmix32(i ^ c);
        if (shift == 24 || (key >> (shift + 8)) == pfx) atomicAdd(&h[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t v = h[threadIdx.x];
    if (v) atomicAdd(hist + ((size_t)k * cap + j) * 256 + threadIdx.x, v);
}

// grid (cap, files), 256 threads = 256 digits: the digit that holds the rank, the rank inside it; the histogram is left zeroed
__global__ void __launch_bounds__(256) fu_pick_kernel(const int32_t *__restrict__ sel_idx, int64_t cap, uint32_t *__restrict__ hist,
                                                      uint32_t *__restrict__ prefix, uint32_t *__restrict__ rank) {
    __shared__ uint32_t wave_sum[4];
    const int64_t j = blockIdx.x;
    if (j >= sel_idx[LB_MAX_ENTRIES]) return;                    // (block-uniform)
    const size_t p = (size_t)blockIdx.y * cap + j;
    const uint32_t v = hist[p * 256 + threadIdx.x];
    hist[p * 256 + threadIdx.x] = 0;
    const uint32_t r = rank[p], pfx = prefix[p];
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, 64);
        if (gp_lane() >= o) incl += t;
    }
    if (gp_lane() == 63) wave_sum[threadIdx.x >> 6] = incl;
    __syncthreads();                                             // (also: every thread has read rank[p] and prefix[p])
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) incl += wave_sum[w];
    const uint32_t excl = incl - v;
    if (excl <= r && r < incl) {
        prefix[p] = (pfx << 8) | threadIdx.x;
        rank[p] = r - excl;
    }
}

// ------------------------------------------------------------------------------------------------ flags of one file, sorted order
__global__ void __launch_bounds__(256) fu_flags_kernel(const uint32_t *__restrict__ keys_sorted, const int32_t *__restrict__ entry_rows,
                                                       const int32_t *__restrict__ entry_off, const int32_t *__restrict__ sel_idx,
                                                       const uint32_t *__restrict__ thresh, const uint8_t *__restrict__ seen, int64_t n,
                                                       int64_t n_split, uint32_t cs, uint32_t k, int form, int64_t cap, int32_t *__restrict__ flag,
                                                       uint8_t *__restrict__ mask_full) {
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s > n) return;
    int f = 0;
    if (s < n) {
        const uint32_t b = keys_sorted[s];
        const int64_t row = entry_rows[s];
        if (b < (uint32_t)LB_MAX_ENTRIES) {
            const int64_t r0 = entry_off[b], nb = entry_off[b + 1] - r0;
            bool in = true;
            if (n_split > 0 && nb > n_split) {
                const int64_t j = sel_idx[b];
                in = j < cap && fu_fmix32((uint32_t)(s - r0) ^ fu_pair_const(cs, b, k)) <= thresh[(size_t)k * cap + j];
            }
            f = (in && (form == FU_CHUNK || seen[row])) ? 1 : 0;
        }
        mask_full[row] = (uint8_t)f;
    }
    flag[s] = f;
}

// base[k] = the first row of file k in feat; status[FU_ROWS] = the rows of feat
__global__ void fu_base_kernel(const int32_t *__restrict__ scan, int64_t n, int num_files, int64_t *__restrict__ base,
                               unsigned long long *__restrict__ status) {
    if (threadIdx.x || blockIdx.x) return;
    int64_t at = 0;
    for (int k = 0; k < num_files; ++k) {
        base[k] = at;
        at += scan[(size_t)k * (n + 1) + n];
    }
    base[num_files] = at;
    status[FU_ROWS] = (unsigned long long)at;
}

__global__ void __launch_bounds__(256) fu_offsets_kernel(const int32_t *__restrict__ scan, const int32_t *__restrict__ entry_off,
                                                         const int64_t *__restrict__ base, int64_t n, int num_files, int64_t entries,
                                                         int64_t *__restrict__ offsets) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= (int64_t)num_files * (entries + 1)) return;
    const int64_t k = t / (entries + 1), b = t % (entries + 1);
    int64_t s = entry_off[b];
    s = s < 0 ? 0 : (s > n ? n : s);
    offsets[t] = base[k] + scan[(size_t)k * (n + 1) + s];
}

// ------------------------------------------------------------------------------------------------ copy and convert
// (the conversion gp_cvt and the wide accesses gp_load_vec / gp_store_vec: gp_map_elem.h)
// One wave per sorted position s.  Lane k < files holds the file's flag and its row inside the file; the source row is loaded once,
// converted once and stored to every flagged file.  A row outside [0, n) or a destination outside [0, total_rows) -- a state that
// gp_fuse_plan did not write -- is skipped, never accessed.
template <typename TI, typename TO, int VEC>
__global__ void __launch_bounds__(256) fu_copy_kernel(const TI *__restrict__ features, int64_t d, const int32_t *__restrict__ entry_rows,
                                                      const int32_t *__restrict__ scan, const int64_t *__restrict__ base, int64_t n,
                                                      int num_files, int64_t total_rows, const uint8_t *__restrict__ seen, TO *__restrict__ feat,
                                                      uint8_t *__restrict__ mask) {
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n) return;                                          // (wave-uniform)
    const int lane = gp_lane();
    const int64_t row = entry_rows[s];
    if ((uint64_t)row >= (uint64_t)n) return;                    // (wave-uniform)
    int32_t pos = 0;
    bool mine = false;
    if (lane < num_files) {
        const int32_t *sc = scan + (size_t)lane * (n + 1) + s;
        pos = sc[0];
        mine = sc[1] == pos + 1 && (uint64_t)(base[lane] + pos) < (uint64_t)total_rows;
    }
    const uint32_t files = (uint32_t)__ballot(mine);
    if (!files) return;                                          // (wave-uniform)
    if (mask && mine) mask[base[lane] + pos] = seen[row] ? 1 : 0;
    const TI *src = features + row * d;
    for (int64_t c0 = 0; c0 < d; c0 += 64 * VEC) {               // (wave-uniform trip count: the shuffles below see every lane)
        const int64_t c = c0 + (int64_t)lane * VEC;
        TO y[VEC];
        if (c < d) {
            TI x[VEC];
            gp_load_vec<VEC>(src + c, x);
#pragma unroll
            for (int i = 0; i < VEC; ++i) y[i] = gp_cvt<TO>(x[i]);
        }
        for (uint32_t rest = files; rest; rest &= rest - 1) {
            const int k = __ffs(rest) - 1;
            const int64_t dst = base[k] + __shfl(pos, k, 64);
            if (c < d) gp_store_vec<VEC>(feat + dst * d + c, y);
        }
    }
}

// the inverse: one wave per sorted position; flag[s] / scan[s] = the row is in the file / its row there
template <typename TI, int VEC>
__global__ void __launch_bounds__(256) fu_dense_kernel(const TI *__restrict__ feat, int64_t d, int64_t feat_rows,
                                                       const int32_t *__restrict__ entry_rows, const int32_t *__restrict__ flag,
                                                       const int32_t *__restrict__ scan, int64_t n, float *__restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n) return;                                          // (wave-uniform)
    const int64_t row = entry_rows[s], r = scan[s];
    const bool in = flag[s] && r < feat_rows;                    // (rows beyond the file's end: outside, the caller compares the counts)
    const TI *src = feat + (in ? r : 0) * d;
    float *dst = out + row * d;
    for (int64_t c = (int64_t)gp_lane() * VEC; c < d; c += 64 * VEC) {
        float y[VEC];
        if (in) {
            TI x[VEC];
            gp_load_vec<VEC>(src + c, x);
#pragma unroll
            for (int i = 0; i < VEC; ++i) y[i] = (float)x[i];
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) y[i] = 0.f;
        }
        gp_store_vec<VEC>(dst + c, y);
    }
}

__global__ void __launch_bounds__(256) fu_dense_flags_kernel(const uint32_t *__restrict__ keys_sorted, const int32_t *__restrict__ entry_rows,
                                                             const uint8_t *__restrict__ mask_full, int64_t n, int32_t *__restrict__ flag) {
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s > n) return;
    flag[s] = (s < n && keys_sorted[s] < (uint32_t)LB_MAX_ENTRIES && mask_full[entry_rows[s]]) ? 1 : 0;
}

__global__ void fu_dense_count_kernel(const int32_t *__restrict__ scan, int64_t n, unsigned long long *__restrict__ status) {
    if (threadIdx.x == 0 && blockIdx.x == 0) status[FU_MASK_ROWS] = (unsigned long long)scan[n];
}

// the widest group of elements both sides may move at once: 16 bytes on the wider side, then 8, then one element
int fu_vec(const void *in, size_t in_size, const void *out, size_t out_size, int64_t d) {
    const size_t wide = in_size > out_size ? in_size : out_size;
    for (int v = (int)(16 / wide); v > 1; v >>= 1)
        if (d % v == 0 && (uintptr_t)in % (v * in_size) == 0 && (uintptr_t)out % (v * out_size) == 0) return v;
    return 1;
}

bool fu_elem_ok(int32_t e) { return e == GP_ELEM_F32 || e == GP_ELEM_F16; }
bool fu_n_ok(int64_t n) { return n >= 1 && n < ((int64_t)1 << 31) - 1; }

// the selecting entries have more than n_split of the n points each
int64_t fu_sel_cap(int64_t n, int64_t n_split) {
    if (n_split <= 0) return 0;
    const int64_t c = n / (n_split + 1);
    return c < LB_MAX_ENTRIES ? c : LB_MAX_ENTRIES;
}

struct FuState {                                                 // what gp_fuse_plan leaves for gp_fuse_write
    int32_t *entry_rows, *entry_off, *scan;
    int64_t *base;
    FuState(GpCarver &cv, int64_t n, int32_t num_files)
        : entry_rows(cv.take<int32_t>(n)), entry_off(cv.take<int32_t>(LB_TABLE)), scan(cv.take<int32_t>((size_t)num_files * (n + 1))),
          base(cv.take<int64_t>(FU_MAX_FILES + 1)) {}
};

struct FuPlanWork {
    uint32_t *k0, *k1, *prefix, *rank, *hist;
    int32_t *r0, *flag, *sel, *sel_idx, *sel_list;
    char *tmp;
    size_t tmp_bytes;
    FuPlanWork(GpCarver &cv, int64_t n, int32_t num_files, int64_t cap)
        : k0(cv.take<uint32_t>(n)), k1(cv.take<uint32_t>(n)), prefix(cv.take<uint32_t>((size_t)num_files * cap)),
          rank(cv.take<uint32_t>((size_t)num_files * cap)), hist(cv.take<uint32_t>((size_t)num_files * cap * 256)), r0(cv.take<int32_t>(n)),
          flag(cv.take<int32_t>(n + 1)), sel(cv.take<int32_t>(LB_MAX_ENTRIES + 1)), sel_idx(cv.take<int32_t>(LB_MAX_ENTRIES + 1)),
          sel_list(cv.take<int32_t>(cap)) {
        tmp_bytes = std::max({lb_sort_bytes(n), gp_scan_bytes<int32_t>(n + 1), gp_scan_bytes<int32_t>(LB_MAX_ENTRIES + 1)});
        tmp = cv.take<char>(tmp_bytes);
    }
};

struct FuDenseWork {
    uint32_t *k0, *k1;
    int32_t *r0, *entry_rows, *flag, *scan;
    char *tmp;
    size_t tmp_bytes;
    FuDenseWork(GpCarver &cv, int64_t n)
        : k0(cv.take<uint32_t>(n)), k1(cv.take<uint32_t>(n)), r0(cv.take<int32_t>(n)), entry_rows(cv.take<int32_t>(n)),
          flag(cv.take<int32_t>(n + 1)), scan(cv.take<int32_t>(n + 1)) {
        tmp_bytes = std::max(lb_sort_bytes(n), gp_scan_bytes<int32_t>(n + 1));
        tmp = cv.take<char>(tmp_bytes);
    }
};

template <typename TI, typename TO>
int fu_copy(int vec, const void *features, int64_t d, const FuState &st, int64_t n, int32_t num_files, int64_t total_rows, const uint8_t *seen,
            void *feat, uint8_t *mask, hipStream_t s) {
    const unsigned grid = (unsigned)((n + 3) / 4);
#define FU_COPY(V)                                                                                                                              \
    fu_copy_kernel<TI, TO, V><<<grid, 256, 0, s>>>(static_cast<const TI *>(features), d, st.entry_rows, st.scan, st.base, n, num_files, total_rows, \
                                                   seen, static_cast<TO *>(feat), mask)
    if (vec == 8) {
        if constexpr (sizeof(TI) == 2 && sizeof(TO) == 2) FU_COPY(8);
    } else if (vec == 4) FU_COPY(4);
    else if (vec == 2) FU_COPY(2);
    else FU_COPY(1);
#undef FU_COPY
    GP_CHECK_LAUNCH();
    return GP_OK;
}

template <typename TI>
int fu_dense(int vec, const void *feat, int64_t d, int64_t feat_rows, const FuDenseWork &k, int64_t n, float *out, hipStream_t s) {
    const unsigned grid = (unsigned)((n + 3) / 4);
#define FU_DENSE(V) fu_dense_kernel<TI, V><<<grid, 256, 0, s>>>(static_cast<const TI *>(feat), d, feat_rows, k.entry_rows, k.flag, k.scan, n, out)
    if (vec == 4) FU_DENSE(4);
    else if (vec == 2) FU_DENSE(2);
    else FU_DENSE(1);
#undef FU_DENSE
    GP_CHECK_LAUNCH();
    return GP_OK;
}

}  // namespace

extern "C" size_t gp_fuse_state_bytes(int64_t n, int32_t num_files) {
    if (!fu_n_ok(n) || num_files < 1 || num_files > FU_MAX_FILES) return 0;
    GpCarver cv(nullptr, 0);
    FuState st(cv, n, num_files);
    return cv.off;
}

extern "C" size_t gp_fuse_workspace_bytes(int64_t n, int32_t num_files, int64_t n_split_points) {
    if (!fu_n_ok(n) || num_files < 1 || num_files > FU_MAX_FILES) return 0;
    GpCarver cv(nullptr, 0);
    FuPlanWork k(cv, n, num_files, fu_sel_cap(n, n_split_points));
    return cv.off;
}

extern "C" int gp_fuse_plan(const double *points, int64_t n, const uint8_t *seen, int32_t num_files, int64_t n_split_points, uint64_t seed,
                            int32_t form, uint8_t *mask_full, void *state, size_t state_bytes, int64_t *status, void *workspace,
                            size_t workspace_bytes, void *stream_) {
    const char *who = "gp_fuse_plan";
    GP_CHECK_ARG(points && seen && mask_full && state && status && workspace, "%s: null argument", who);
    GP_CHECK_ARG(fu_n_ok(n), "%s: n=%lld outside 1..2^31-2", who, (long long)n);
    GP_CHECK_ARG(num_files >= 1 && num_files <= FU_MAX_FILES, "%s: num_files=%d outside 1..%d", who, num_files, FU_MAX_FILES);
    GP_CHECK_ARG(form == FU_MERGED || form == FU_CHUNK, "%s: form=%d (0 merged, 1 chunk)", who, form);
    GP_CHECK_ARG(n_split_points >= 0, "%s: n_split_points=%lld (0: no split)", who, (long long)n_split_points);
    {
        const void *const in[] = {points, seen};
        const size_t in_bytes[] = {(size_t)n * 32, (size_t)n};
        const void *const o[] = {mask_full, state, status, workspace};
        const size_t o_bytes[] = {(size_t)num_files * n, state_bytes, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    const int64_t cap = fu_sel_cap(n, n_split_points);
    GpCarver cs_(state, state_bytes);
    FuState st(cs_, n, num_files);
    GpCarver cv(workspace, workspace_bytes);
    FuPlanWork k(cv, n, num_files, cap);
    if (!cs_.ok() || !cv.ok()) {
        gp_set_error("%s: state or workspace too small (%zu < %zu, %zu < %zu)", who, state_bytes, cs_.off, workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *stw = reinterpret_cast<unsigned long long *>(status);
    const uint32_t cs = fu_fmix32((uint32_t)seed ^ fu_fmix32((uint32_t)(seed >> 32)));
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    const unsigned nb = (unsigned)((n + 255) / 256), nb1 = (unsigned)((n + 1 + 255) / 256);
    // (1) entry tables: the sorted rows and the offsets into the state
    fu_row_keys_kernel<<<nb, 256, 0, s>>>(points, n, k.k0, k.r0, stw);
    GP_CHECK_LAUNCH();
    const LbTable rows = {k.k0, k.k1, k.r0, st.entry_rows, st.entry_off};
    LB_TRY(lb_table_finish(rows, n, k.tmp, k.tmp_bytes, s));
    // (2) the threshold key of every (file, entry) that selects
    if (cap > 0) {
        const unsigned eb = (LB_MAX_ENTRIES + 1 + 255) / 256;
        fu_sel_flags_kernel<<<eb, 256, 0, s>>>(st.entry_off, n_split_points, k.sel);
        size_t io = k.tmp_bytes;
        GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, io, k.sel, k.sel_idx, (int32_t)0, (size_t)(LB_MAX_ENTRIES + 1), rocprim::plus<int32_t>(), s));
        fu_sel_list_kernel<<<eb, 256, 0, s>>>(k.sel, k.sel_idx, n_split_points, num_files, cap, k.sel_list, k.prefix, k.rank);
        GP_CHECK_HIP(hipMemsetAsync(k.hist, 0, (size_t)num_files * cap * 256 * sizeof(uint32_t), s));
        // blocks per pair: about four per 256 keys of an average selecting entry's share, so that many small pairs launch few idle blocks
        const int64_t share = 4 * (int64_t)nb / cap;
        const unsigned by = (unsigned)(share < 1 ? 1 : (share > FU_HIST_BLOCKS ? FU_HIST_BLOCKS : share));
        for (int shift = 24; shift >= 0; shift -= 8) {
            fu_hist_kernel<<<dim3((unsigned)cap, by, (unsigned)num_files), 256, 0, s>>>(st.entry_off, k.sel_list, k.sel_idx, cs, k.prefix, shift, cap,
                                                                                         k.hist);
            fu_pick_kernel<<<dim3((unsigned)cap, (unsigned)num_files), 256, 0, s>>>(k.sel_idx, cap, k.hist, k.prefix, k.rank);
        }
        GP_CHECK_LAUNCH();
    }
    // (3) per file: flags in the entry-sorted order, mask_full, the scan
    for (int f = 0; f < num_files; ++f) {
        fu_flags_kernel<<<nb1, 256, 0, s>>>(k.k1, st.entry_rows, st.entry_off, k.sel_idx, k.prefix, seen, n, cap > 0 ? n_split_points : 0, cs,
                                            (uint32_t)f, form, cap, k.flag, mask_full + (size_t)f * n);
        size_t io = k.tmp_bytes;
        GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, io, k.flag, st.scan + (size_t)f * (n + 1), (int32_t)0, (size_t)(n + 1), rocprim::plus<int32_t>(), s));
    }
    fu_base_kernel<<<1, 64, 0, s>>>(st.scan, n, num_files, st.base, stw);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_fuse_write(const void *features, int32_t elem_in, int64_t d, const uint8_t *seen, int64_t n, int32_t num_files,
                             const void *state, size_t state_bytes, int64_t num_entries, void *feat, int32_t elem_out, int64_t total_rows,
                             uint8_t *mask, int64_t *offsets, void *stream_) {
    const char *who = "gp_fuse_write";
    GP_CHECK_ARG(features && seen && state && offsets, "%s: null argument", who);
    GP_CHECK_ARG(fu_n_ok(n) && d >= 1, "%s: n=%lld outside 1..2^31-2 or d=%lld < 1", who, (long long)n, (long long)d);
    GP_CHECK_ARG(num_files >= 1 && num_files <= FU_MAX_FILES, "%s: num_files=%d outside 1..%d", who, num_files, FU_MAX_FILES);
    GP_CHECK_ARG(fu_elem_ok(elem_in) && fu_elem_ok(elem_out), "%s: element types %d -> %d (0 fp32, 1 fp16)", who, elem_in, elem_out);
    GP_CHECK_ARG(num_entries >= 1 && num_entries <= LB_MAX_ENTRIES, "%s: num_entries=%lld outside 1..%d", who, (long long)num_entries, LB_MAX_ENTRIES);
    GP_CHECK_ARG(total_rows >= 0 && (total_rows == 0 || feat), "%s: total_rows=%lld without feat", who, (long long)total_rows);
    const size_t si = gp_elem_size(elem_in), so = gp_elem_size(elem_out);
    GP_CHECK_ARG((uintptr_t)features % si == 0 && (uintptr_t)feat % so == 0, "%s: rows not aligned to their element", who);
    GpCarver cs_(const_cast<void *>(state), state_bytes);
    FuState st(cs_, n, num_files);
    if (!cs_.ok()) {
        gp_set_error("%s: state too small (%zu < %zu)", who, state_bytes, cs_.off);
        return GP_ENOMEM;
    }
    {
        const void *const in[] = {features, seen, state};
        const size_t in_bytes[] = {(size_t)n * d * si, (size_t)n, state_bytes};
        const void *const o[] = {feat, mask, offsets};
        const size_t o_bytes[] = {(size_t)total_rows * d * so, (size_t)total_rows, (size_t)num_files * (num_entries + 1) * 8};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    hipStream_t s = gp_stream(stream_);
    const int64_t cells = (int64_t)num_files * (num_entries + 1);
    fu_offsets_kernel<<<(unsigned)((cells + 255) / 256), 256, 0, s>>>(st.scan, st.entry_off, st.base, n, num_files, num_entries, offsets);
    GP_CHECK_LAUNCH();
    if (total_rows == 0) return GP_OK;
    const int vec = fu_vec(features, si, feat, so, d);
    if (elem_in == GP_ELEM_F32 && elem_out == GP_ELEM_F16) return fu_copy<float, gp_f16>(vec, features, d, st, n, num_files, total_rows, seen, feat, mask, s);
    if (elem_in == GP_ELEM_F32) return fu_copy<float, float>(vec, features, d, st, n, num_files, total_rows, seen, feat, mask, s);
    if (elem_out == GP_ELEM_F16) return fu_copy<gp_f16, gp_f16>(vec, features, d, st, n, num_files, total_rows, seen, feat, mask, s);
    return fu_copy<gp_f16, float>(vec, features, d, st, n, num_files, total_rows, seen, feat, mask, s);
}

extern "C" size_t gp_fuse_dense_workspace_bytes(int64_t n) {
    if (!fu_n_ok(n)) return 0;
    GpCarver cv(nullptr, 0);
    FuDenseWork k(cv, n);
    return cv.off;
}

extern "C" int gp_fuse_dense(const double *points, int64_t n, const uint8_t *mask_full, const void *feat, int32_t elem, int64_t feat_rows,
                             int64_t d, float *out, int64_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "gp_fuse_dense";
    GP_CHECK_ARG(points && mask_full && out && status && workspace, "%s: null argument", who);
    GP_CHECK_ARG(fu_n_ok(n) && d >= 1, "%s: n=%lld outside 1..2^31-2 or d=%lld < 1", who, (long long)n, (long long)d);
    GP_CHECK_ARG(fu_elem_ok(elem), "%s: element type %d (0 fp32, 1 fp16)", who, elem);
    GP_CHECK_ARG(feat_rows >= 0 && (feat_rows == 0 || feat), "%s: feat_rows=%lld without feat", who, (long long)feat_rows);
    const size_t si = gp_elem_size(elem);
    GP_CHECK_ARG((uintptr_t)feat % si == 0 && (uintptr_t)out % 4 == 0, "%s: rows not aligned to their element", who);
    {
        const void *const in[] = {points, mask_full, feat};
        const size_t in_bytes[] = {(size_t)n * 32, (size_t)n, (size_t)feat_rows * d * si};
        const void *const o[] = {out, status, workspace};
        const size_t o_bytes[] = {(size_t)n * d * 4, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver cv(workspace, workspace_bytes);
    FuDenseWork k(cv, n);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *stw = reinterpret_cast<unsigned long long *>(status);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    const unsigned nb = (unsigned)((n + 255) / 256), nb1 = (unsigned)((n + 1 + 255) / 256);
    fu_row_keys_kernel<<<nb, 256, 0, s>>>(points, n, k.k0, k.r0, stw);
    GP_CHECK_LAUNCH();
    const LbTable rows = {k.k0, k.k1, k.r0, k.entry_rows, nullptr};      // (the sorted rows alone: nothing here reads an entry's offset)
    LB_TRY(lb_table_sort(rows, n, k.tmp, k.tmp_bytes, s));
    fu_dense_flags_kernel<<<nb1, 256, 0, s>>>(k.k1, k.entry_rows, mask_full, n, k.flag);
    size_t io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(k.tmp, io, k.flag, k.scan, (int32_t)0, (size_t)(n + 1), rocprim::plus<int32_t>(), s));
    fu_dense_count_kernel<<<1, 64, 0, s>>>(k.scan, n, stw);
    GP_CHECK_LAUNCH();
    const void *src = feat_rows ? feat : (const void *)out;      // (never read: no row is inside an empty file)
    const int vec = fu_vec(src, si, out, 4, d);
    if (elem == GP_ELEM_F32) return fu_dense<float>(vec, src, d, feat_rows, k, n, out, s);
    return fu_dense<gp_f16>(vec, src, d, feat_rows, k, n, out, s);
}
