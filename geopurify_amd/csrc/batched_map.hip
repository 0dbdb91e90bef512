// Batch-aware voxel order + 27-offset kernel map over sorted 64-bit keys: the coordinate handling of AffinityPredictor.forward
// on an ME-style SparseTensor (int32 [N,4] = batch, x, y, z in any row order).  key = batch << 48 | morton(xyz - min), 16 bits
// per axis with gp_morton3's interleave, so one batch entry with extents below 65536 sorts exactly as gp_morton_order does.  The
// map finds every neighbour by a binary search of the sorted keys (decode, add the offset, re-encode): a pure function of the
// coordinates, and rows of different batch entries never meet because the batch index is part of the key.
#include <rocprim/device/device_radix_sort.hpp>

#include "gp_grid.h"

namespace {

constexpr uint64_t kMorton48 = (1ull << 48) - 1;

// inverse of gp_morton3 for one axis: the bits at 3i (i < 21) of m, packed
__device__ __forceinline__ uint32_t compact3(uint64_t m) {
    m &= 0x1249249249249249ull;
    m = (m ^ (m >> 2)) & 0x10c30c30c30c30c3ull;
    m = (m ^ (m >> 4)) & 0x100f00f00f00f00full;
    m = (m ^ (m >> 8)) & 0x1f0000ff0000ffull;
    m = (m ^ (m >> 16)) & 0x1f00000000ffffull;
    m = (m ^ (m >> 32)) & 0x1fffffull;
    return (uint32_t)m;
}

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
        const int x = (int)compact3(m) + (k % 3) - 1;
        const int y = (int)compact3(m >> 1) + (k / 3 % 3) - 1;
        const int z = (int)compact3(m >> 2) + (k / 9) - 1;
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
