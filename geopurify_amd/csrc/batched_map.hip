// Batch-aware voxel order + 27-offset kernel map over sorted 64-bit keys: the coordinate handling of AffinityPredictor.forward
// on an ME-style SparseTensor (int32 [N,4] = batch, x, y, z in any row order).  key = batch << 48 | morton(xyz - min), 16 bits
// per axis with gp_morton3's interleave, so one batch entry with extents below 65536 sorts exactly as gp_morton_order does.  The
// map finds every neighbour by a binary search of the sorted keys (decode, add the offset, re-encode): a pure function of the
// coordinates, and rows of different batch entries never meet because the batch index is part of the key.
// gp_quantize_batched (at the end of the file) merges duplicate rows over the same key: unique voxels, inverse map and CSR.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "gp_grid.h"
#include "gp_scan_bytes.h"

namespace {

__global__ void init_kernel(int32_t *__restrict__ mm, int32_t *__restrict__ status) {
    if (threadIdx.x < 3) mm[threadIdx.x] = INT32_MAX;
    else if (threadIdx.x < 6) mm[threadIdx.x] = INT32_MIN;
    else if (threadIdx.x < 9) status[threadIdx.x - 6] = 0;
}

// per-axis min / max of columns 1..3 of [nv,4]; 256 threads (the LDS reduce assumes 4 waves), one atomic per block and bound
__global__ void minmax4_kernel(const int32_t *__restrict__ c, int64_t nv, int32_t *__restrict__ mm) {
    int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int v = c[i * 4 + 1 + a];
            lo[a] = min(lo[a], v);
            hi[a] = max(hi[a], v);
        }
    }
    __shared__ int s_lo[4][3], s_hi[4][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = min(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = max(hi[a], __shfl_xor(hi[a], o, 64));
        }
        if (gp_lane() == 0) { s_lo[threadIdx.x >> 6][a] = lo[a]; s_hi[threadIdx.x >> 6][a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        atomicMin(&mm[a], min(min(s_lo[0][a], s_lo[1][a]), min(s_lo[2][a], s_lo[3][a])));
        atomicMax(&mm[3 + a], max(max(s_hi[0][a], s_hi[1][a]), max(s_hi[2][a], s_hi[3][a])));
    }
}

// keys + identity values; status[1] += rows whose batch index is outside 0..65535, status[2] = mask of the axes whose extent
// (max - min + 1) is 65536 or more.  Out-of-range rows still get a (meaningless) key so that the sort runs on defined data.
__global__ void batched_keys_kernel(const int32_t *__restrict__ c, int64_t nv, const int32_t *__restrict__ mm,
                                    uint64_t *__restrict__ keys, int32_t *__restrict__ vals, int32_t *__restrict__ status) {
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i == 0) {
        int bad_axes = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if ((int64_t)mm[3 + a] - (int64_t)mm[a] >= 65535) bad_axes |= 1 << a;
        status[2] = bad_axes;
    }
    bool bad = false;
    if (i < nv) {
        const int32_t b = c[i * 4];
        bad = (uint32_t)b > 65535u;
        const uint32_t x = ((uint32_t)c[i * 4 + 1] - (uint32_t)mm[0]) & 0xffffu;
        const uint32_t y = ((uint32_t)c[i * 4 + 2] - (uint32_t)mm[1]) & 0xffffu;
        const uint32_t z = ((uint32_t)c[i * 4 + 3] - (uint32_t)mm[2]) & 0xffffu;
        keys[i] = ((uint64_t)((uint32_t)b & 0xffffu) << 48) | gp_morton3(x, y, z);
        vals[i] = (int32_t)i;
    }
    const int n_bad = gp_wave_sum_i(bad ? 1 : 0);
    if (gp_lane() == 0 && n_bad) atomicAdd(&status[1], n_bad);
}

// status[0] += sorted rows equal to the row before them (one per duplicate beyond the first), and rank = perm^-1
__global__ void dups_rank_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ perm, int64_t nv,
                                 int32_t *__restrict__ rank, int32_t *__restrict__ status) {
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    bool dup = false;
    if (i < nv) {
        rank[perm[i]] = (int32_t)i;
        dup = i > 0 && keys[i] == keys[i - 1];
    }
    const int n_dup = gp_wave_sum_i(dup ? 1 : 0);
    if (gp_lane() == 0 && n_dup) atomicAdd(&status[0], n_dup);
}

// one thread per (row, offset): blockIdx.y = k = (dx+1) + 3(dy+1) + 9(dz+1); nbr_map[k][i] = row of key(i) + o_k or -1
__global__ void kernel_map_sorted_kernel(const uint64_t *__restrict__ keys, int64_t nv, int32_t *__restrict__ nbr_map) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const int k = blockIdx.y;
    int32_t r = (int32_t)i;
    if (k != 13) {
        const uint64_t key = keys[i];
        const uint64_t m = key & kMorton48;
        const int x = (int)gp_compact3(m) + (k % 3) - 1;
        const int y = (int)gp_compact3(m >> 1) + (k / 3 % 3) - 1;
        const int z = (int)gp_compact3(m >> 2) + (k / 9) - 1;
        r = -1;
        if ((uint32_t)x <= 65535u && (uint32_t)y <= 65535u && (uint32_t)z <= 65535u) {
            const uint64_t q = (key & ~kMorton48) | gp_morton3((uint32_t)x, (uint32_t)y, (uint32_t)z);
            // lower bound of q in keys[0, nv)
            int64_t lo = 0, n = nv;
            while (n > 0) {
                const int64_t half = n >> 1;
                if (keys[lo + half] < q) { lo += half + 1; n -= half + 1; }
                else n = half;
            }
            if (lo < nv && keys[lo] == q) r = (int32_t)lo;
        }
    }
    nbr_map[(int64_t)k * nv + i] = r;
}

// gp_quantize_batched, pass 1: head[i] = 1 where the sorted row i opens a voxel (its key differs from the row before it)
__global__ void head_flags_kernel(const uint64_t *__restrict__ keys, int64_t n, int32_t *__restrict__ head) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// gp_quantize_batched, pass 2: heads_before = exclusive scan of head, so the voxel of sorted row i is heads_before[i] + head[i] - 1
// (in 0 .. n-1).  The sorted rows of one voxel are adjacent and, the pair sort being stable, ascend in input row: the head row is
// the voxel's lowest input row, and rows[] is the CSR order as it stands.  Every store is at an index below n, or at nv <= n.
__global__ void quantize_write_kernel(const int32_t *__restrict__ c, const int32_t *__restrict__ rows, const int32_t *__restrict__ head,
                                      const int32_t *__restrict__ heads_before, int64_t n, int32_t *__restrict__ vox_coords,
                                      int64_t *__restrict__ unique_index, int64_t *__restrict__ inverse, int64_t *__restrict__ order,
                                      int64_t *__restrict__ seg_start, int32_t *__restrict__ status) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t r = rows[i];
    const int h = head[i];
    const int64_t v = (int64_t)heads_before[i] + h - 1;
    if ((uint64_t)r >= (uint64_t)n || (uint64_t)v >= (uint64_t)n) return;          // (cannot happen: rows is a permutation of 0 .. n-1)
    order[i] = r;
    inverse[r] = v;
    if (h) {
        *reinterpret_cast<int4 *>(vox_coords + v * 4) = *reinterpret_cast<const int4 *>(c + r * 4);
        unique_index[v] = r;
        seg_start[v] = i;
    }
    if (i == n - 1) {
        seg_start[v + 1] = n;
        status[0] = (int32_t)(v + 1);
    }
}

// one wave per voxel, lanes striding its rows.  rule 0 (first): the label of unique_index[v]; 1 (differ): ignore_label when any two
// labels of the voxel differ; 2 (count): ignore_label when the voxel holds more than one row.
__global__ void segment_labels_kernel(const int64_t *__restrict__ labels, int64_t n, const int64_t *__restrict__ order,
                                      const int64_t *__restrict__ seg, const int64_t *__restrict__ unique_index, int64_t nv,
                                      int64_t ignore_label, int rule, int64_t *__restrict__ out) {
    int64_t v = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    if (v >= nv) return;
    v = __builtin_amdgcn_readfirstlane((int)v);
    const int64_t b = max(seg[v], (int64_t)0), e = min(seg[v + 1], n);            // (no read of order[] past its n rows)
    const int64_t u = unique_index[v];
    const int64_t first = (uint64_t)u < (uint64_t)n ? labels[u] : ignore_label;
    bool differ = false;
    if (rule == 1) {
        for (int64_t j = b + gp_lane(); j < e; j += 64) {
            const int64_t r = order[j];
            differ |= (uint64_t)r >= (uint64_t)n || labels[r] != first;
        }
        differ = __any(differ);
    } else if (rule == 2) {
        differ = e - b > 1;
    }
    if (gp_lane() == 0) out[v] = differ ? ignore_label : first;
}

size_t sort_bytes(int64_t nv) {
    size_t tmp = 0;
    (void)rocprim::radix_sort_pairs(nullptr, tmp, (uint64_t *)nullptr, (uint64_t *)nullptr, (int32_t *)nullptr,
                                    (int32_t *)nullptr, (size_t)nv, 0, 64, 0);
    return tmp;
}

}  // namespace

extern "C" size_t gp_coords_order_batched_workspace_bytes(int64_t nv) {
    if (nv <= 0) return 0;
    GpCarver cv(nullptr, 0);
    cv.take<int32_t>(8);
    cv.take<uint64_t>(nv);
    cv.take<int32_t>(nv);
    cv.take<char>(sort_bytes(nv));
    return cv.off;
}

extern "C" int gp_coords_order_batched(const int32_t *coords, int64_t nv, int32_t *perm, int32_t *rank, uint64_t *keys_sorted,
                                       int32_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    GP_CHECK_ARG(coords && perm && rank && keys_sorted && status, "gp_coords_order_batched: null argument");
    GP_CHECK_ARG(nv > 0 && nv < (1ll << 31), "gp_coords_order_batched: nv=%lld out of range", (long long)nv);
    hipStream_t s = gp_stream(stream_);
    const size_t tmp = sort_bytes(nv);
    GpCarver cv(workspace, workspace_bytes);
    int32_t *mm = cv.take<int32_t>(8);
    uint64_t *k0 = cv.take<uint64_t>(nv);
    int32_t *v0 = cv.take<int32_t>(nv);
    char *t = cv.take<char>(tmp);
    if (!cv.ok()) {
        gp_set_error("gp_coords_order_batched: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    const int blocks = (int)((nv + 255) / 256);
    init_kernel<<<1, 64, 0, s>>>(mm, status);
    minmax4_kernel<<<min(blocks, 64), 256, 0, s>>>(coords, nv, mm);
    batched_keys_kernel<<<blocks, 256, 0, s>>>(coords, nv, mm, k0, v0, status);
    GP_CHECK_LAUNCH();
    size_t tmp_io = tmp;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(t, tmp_io, k0, keys_sorted, v0, perm, (size_t)nv, 0, 64, s));
    dups_rank_kernel<<<blocks, 256, 0, s>>>(keys_sorted, perm, nv, rank, status);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_kernel_map_sorted(const uint64_t *keys_sorted, int64_t nv, int32_t *nbr_map, void *stream_) {
    GP_CHECK_ARG(keys_sorted && nbr_map, "gp_kernel_map_sorted: null argument");
    GP_CHECK_ARG(nv > 0 && nv < (1ll << 31), "gp_kernel_map_sorted: nv=%lld out of range", (long long)nv);
    kernel_map_sorted_kernel<<<dim3((unsigned)((nv + 255) / 256), 27), 256, 0, gp_stream(stream_)>>>(keys_sorted, nv, nbr_map);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Quantisation of a batched point cloud: the key, min / max and pair sort of gp_coords_order_batched, then head flags, a scan
// and one write pass.  No float arithmetic and no float atomics here; the feature reductions are gp_scatter_mean_csr /
// gp_gather_rows over the CSR this entry returns.
namespace {
struct QuantizeWs {
    int32_t *mm, *v0, *v1, *head, *before;
    uint64_t *k0, *k1;
    char *scan_tmp, *sort_tmp;
    size_t scan_tmp_bytes, sort_tmp_bytes;
    QuantizeWs(GpCarver &cv, int64_t n) : scan_tmp_bytes(gp_scan_bytes<int32_t>(n)), sort_tmp_bytes(sort_bytes(n)) {
        mm = cv.take<int32_t>(8);
        k0 = cv.take<uint64_t>(n);
        k1 = cv.take<uint64_t>(n);
        v0 = cv.take<int32_t>(n);
        v1 = cv.take<int32_t>(n);
        head = cv.take<int32_t>(n);
        before = cv.take<int32_t>(n);
        scan_tmp = cv.take<char>(scan_tmp_bytes);
        sort_tmp = cv.take<char>(sort_tmp_bytes);
    }
};
}  // namespace

extern "C" size_t gp_quantize_batched_workspace_bytes(int64_t n) {
    if (n <= 0 || n >= (1ll << 31)) return 0;
    GpCarver cv(nullptr, 0);
    QuantizeWs ws(cv, n);
    return cv.off;
}

extern "C" int gp_quantize_batched(const int32_t *coords, int64_t n, int32_t *vox_coords, int64_t *unique_index, int64_t *inverse,
                                   int64_t *order, int64_t *seg_start, int32_t *status, void *workspace, size_t workspace_bytes,
                                   void *stream_) {
    GP_CHECK_ARG(coords && vox_coords && unique_index && inverse && order && seg_start && status, "gp_quantize_batched: null argument");
    GP_CHECK_ARG(n > 0 && n < (1ll << 31), "gp_quantize_batched: n=%lld out of range (1 .. 2^31 - 1)", (long long)n);
    GP_CHECK_ARG((uintptr_t)coords % 16 == 0 && (uintptr_t)vox_coords % 16 == 0,
                 "gp_quantize_batched: coords and vox_coords must be 16-byte aligned (one row per load / store)");
    hipStream_t s = gp_stream(stream_);
    GpCarver cv(workspace, workspace_bytes);
    QuantizeWs ws(cv, n);
    if (!workspace || !cv.ok()) {
        gp_set_error("gp_quantize_batched: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    const int blocks = (int)((n + 255) / 256);
    init_kernel<<<1, 64, 0, s>>>(ws.mm, status);
    minmax4_kernel<<<min(blocks, 64), 256, 0, s>>>(coords, n, ws.mm);
    batched_keys_kernel<<<blocks, 256, 0, s>>>(coords, n, ws.mm, ws.k0, ws.v0, status);
    GP_CHECK_LAUNCH();
    // (key, row) pairs with row = 0 .. n-1 going in: the radix sort is STABLE, so the rows of equal keys come out in ascending input
    // row.  quantize_write_kernel relies on it twice: unique_index is the head row, and `order` ascends inside every segment.
    size_t tmp_io = ws.sort_tmp_bytes;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(ws.sort_tmp, tmp_io, ws.k0, ws.k1, ws.v0, ws.v1, (size_t)n, 0, 64, s));
    head_flags_kernel<<<blocks, 256, 0, s>>>(ws.k1, n, ws.head);
    GP_CHECK_LAUNCH();
    tmp_io = ws.scan_tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(ws.scan_tmp, tmp_io, ws.head, ws.before, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), s));
    quantize_write_kernel<<<blocks, 256, 0, s>>>(coords, ws.v1, ws.head, ws.before, n, vox_coords, unique_index, inverse, order,
                                                 seg_start, status);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_segment_labels(const int64_t *labels, int64_t n, const int64_t *order, const int64_t *seg_start,
                                 const int64_t *unique_index, int64_t nv, int64_t ignore_label, int32_t rule, int64_t *out,
                                 void *stream_) {
    GP_CHECK_ARG(labels && order && seg_start && unique_index && out, "gp_segment_labels: null argument");
    GP_CHECK_ARG(n > 0 && n < (1ll << 31) && nv > 0 && nv <= n, "gp_segment_labels: n=%lld nv=%lld out of range (1 <= nv <= n < 2^31)",
                 (long long)n, (long long)nv);
    GP_CHECK_ARG(rule >= 0 && rule <= 2, "gp_segment_labels: rule=%d (0 first, 1 differ, 2 count)", rule);
    segment_labels_kernel<<<(unsigned)((nv * 64 + 255) / 256), 256, 0, gp_stream(stream_)>>>(labels, n, order, seg_start, unique_index,
                                                                                             nv, ignore_label, rule, out);
    GP_CHECK_LAUNCH();
    return GP_OK;
}
