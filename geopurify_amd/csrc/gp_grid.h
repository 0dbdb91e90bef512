// Lattice grid over Morton-ordered voxels: 8x8x8-voxel cells, each occupied cell has a record
// {start row, count, 512-bit occupancy bitmap in local-Morton order}.  Because the voxels are
// sorted by Morton code, a cell's voxels are contiguous and ordered by their 9-bit local code, so
// the row of voxel (x,y,z) is  start + popcount(bitmap below its local code): an exact O(1) lookup
// that serves both the 27-offset kernel map and kNN candidate enumeration (row 10).
#pragma once
#include "gp_common.h"

struct GpGridHeader {
    int32_t origin[3];
    int32_t extent[3];
    int32_t cdim[3];
    int32_t status;      // bit0: input not strictly Morton-increasing (unsorted or duplicate voxels)
    int32_t ncells;      // occupied cells (atomic counter during build)
    int32_t max_cells;
    int64_t nv;
    int64_t cell_index_off;   // byte offsets from the grid base
    int64_t records_off;
};

struct GpCellRec {
    int32_t start;
    int32_t count;
    uint32_t bits[16];
};

__host__ __device__ __forceinline__ uint32_t gp_spread3_10(uint32_t v) {
    // spread the low 10 bits of v so that there are two zero bits between each
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__host__ __device__ __forceinline__ uint64_t gp_morton3(uint32_t x, uint32_t y, uint32_t z) {
    // 21 bits per axis -> 63-bit code (x lowest)
    uint64_t lo = gp_spread3_10(x) | (gp_spread3_10(y) << 1) | (gp_spread3_10(z) << 2);
    uint64_t mid = gp_spread3_10(x >> 10) | (gp_spread3_10(y >> 10) << 1) | (gp_spread3_10(z >> 10) << 2);
    uint64_t hi = gp_spread3_10(x >> 20) | (gp_spread3_10(y >> 20) << 1) | (gp_spread3_10(z >> 20) << 2);
    return lo | (mid << 30) | (hi << 60);
}
// inverse of gp_morton3 for one axis: the bits at 3i (i < 21) of m, packed (y: m >> 1, z: m >> 2)
__host__ __device__ __forceinline__ uint32_t gp_compact3(uint64_t m) {
    m &= 0x1249249249249249ull;
    m = (m ^ (m >> 2)) & 0x10c30c30c30c30c3ull;
    m = (m ^ (m >> 4)) & 0x100f00f00f00f00full;
    m = (m ^ (m >> 8)) & 0x1f0000ff0000ffull;
    m = (m ^ (m >> 16)) & 0x1f00000000ffffull;
    m = (m ^ (m >> 32)) & 0x1fffffull;
    return (uint32_t)m;
}
__device__ __forceinline__ uint32_t gp_local9(int x, int y, int z) {
    return (uint32_t)gp_morton3(x & 7, y & 7, z & 7);
}

// ---- batched keys (gp_coords_order_batched): batch << 48 | gp_morton3(xyz - min), 16 bits per axis.  An 8^3 cell is key >> 9 =
// batch << 39 | morton(cell coordinates), 13 bits per axis.
constexpr uint64_t kMorton48 = (1ull << 48) - 1;
constexpr int kMaxCellCoord = 65535 >> 3;

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

// the rows of key's batch entry in the sorted a[0, n): [first key with these batch bits, first key of a higher batch index)
__device__ __forceinline__ void entry_range_u64(const uint64_t *__restrict__ a, int64_t n, uint64_t key, int64_t &e0, int64_t &e1) {
    const uint64_t batch = key >> 48;
    e0 = lower_bound_u64(a, n, batch << 48);
    e1 = batch == 65535 ? n : lower_bound_u64(a, n, (batch + 1) << 48);
}

struct GpGridView {
    const GpGridHeader *h;
    const int32_t *cell_index;
    const GpCellRec *recs;
    __device__ __forceinline__ GpGridView(const void *grid) {
        h = reinterpret_cast<const GpGridHeader *>(grid);
        const char *b = reinterpret_cast<const char *>(grid);
        cell_index = reinterpret_cast<const int32_t *>(b + h->cell_index_off);
        recs = reinterpret_cast<const GpCellRec *>(b + h->records_off);
    }
    // record slot of cell (cx,cy,cz) or -1
    __device__ __forceinline__ int cell_slot(int cx, int cy, int cz) const {
        if ((unsigned)cx >= (unsigned)h->cdim[0] || (unsigned)cy >= (unsigned)h->cdim[1] ||
            (unsigned)cz >= (unsigned)h->cdim[2])
            return -1;
        return cell_index[((int64_t)cz * h->cdim[1] + cy) * h->cdim[0] + cx];
    }
    // row of the voxel at relative coordinates (rx,ry,rz) or -1
    __device__ __forceinline__ int lookup_rel(int rx, int ry, int rz) const {
        if ((unsigned)rx >= (unsigned)h->extent[0] || (unsigned)ry >= (unsigned)h->extent[1] ||
            (unsigned)rz >= (unsigned)h->extent[2])
            return -1;
        int slot = cell_slot(rx >> 3, ry >> 3, rz >> 3);
        if (slot < 0) return -1;
        const GpCellRec &r = recs[slot];
        uint32_t l = gp_local9(rx, ry, rz);
        uint32_t wi = l >> 5, bi = l & 31;
        uint32_t word = r.bits[wi];
        if (!((word >> bi) & 1u)) return -1;
        int idx = r.start + __popc(word & ((1u << bi) - 1u));
        for (uint32_t j = 0; j < wi; ++j) idx += __popc(r.bits[j]);
        return idx;
    }
};
