// The contrastive sampler over batched SparseTensors (geopurify_amd.sparse.sample_pairs): the anchors x rows similarity of
// sample_contrastive_pairs_hybrid (models/affinity_module.py:1113-1115) computed only INSIDE each anchor's batch entry -- a ragged,
// block-diagonal matrix instead of [A, N] -- and the 15 local negatives of :1125-1133.  The arg-max and the 48 global negatives of a
// ragged row are gp_sampler_select_segments (train.hip: sampler_select_kernel with a row descriptor).
//
// gp_sim_segments_f16x3 is a plain tiled GEMM C = A B^T on v_mfma_f32_16x16x32_f16.  Both operands are rows of the same f16 hi/lo
// planes (gp_normalize_split_f16, rows in key order, d a multiple of 32), K-contiguous: a fragment of either operand is 16 bytes
// of one row, so the tile images in LDS are row-major copies and every fragment is one ds_read_b128.
//   workgroup = 256 threads = 2 x 2 waves, tile = 64 anchors x 64 entry rows, K step 32, each wave 32 x 32 = 2 x 2 accumulators;
//   per K step and wave: 4 fragment pairs (hi, lo) read, 12 MFMAs (hi.hi + hi.lo + lo.hi per accumulator, fp32 accumulation --
//   the arithmetic of the gather-GEMM of sparse_conv_v2.hip); the next step's 16-byte pieces are loaded into registers before the
//   MFMAs of the current one and stored to LDS after them (one image, two barriers per step);
//   LDS rows are 80 bytes apart (64 of data): the 16 rows of a fragment read then start 20 banks apart.
// The grid is (column tiles of the LONGEST entry, anchor tiles).  The anchors arrive sorted by key row, so the anchors of an entry are
// consecutive; an anchor tile that straddles two (or more) entries runs the tile once per entry with the other entries' anchors
// masked, and the rows past an entry's end are masked: nothing is computed into, or stored to, another anchor's extent.
#include "gp_common.h"
#include "gp_gfx950.h"

namespace {

constexpr int SS_TM = 64, SS_TN = 64, SS_TK = 32, SS_PITCH = 40;      // pitch in f16: 80 bytes

// all LDS reads of the step have landed; the fragments are tied to the wait so that no MFMA moves above it
__device__ __forceinline__ void ss_wait_frags(f16x8 (&a)[2][2], f16x8 (&b)[2][2]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(b[0][0]), "+v"(b[0][1]), "+v"(b[1][0]), "+v"(b[1][1])
                 :
                 : "memory");
}

// out[row_off[a] + j] = <x[anchor_row[a]], x[seg_first[a] + j]> for j < seg_len[a], x = hi + lo
__global__ void __launch_bounds__(256)
sim_segments_kernel(const _Float16 *__restrict__ hi, const _Float16 *__restrict__ lo, int64_t ld_h, int d, const int32_t *__restrict__ anchor_row,
                    const int32_t *__restrict__ seg_first, const int32_t *__restrict__ seg_len, const int64_t *__restrict__ row_off,
                    int num_anchors, float *__restrict__ out) {
    // [operand: anchors, rows][plane: hi, lo][tile row][k]
    __shared__ __align__(16) _Float16 img[2][2][SS_TM][SS_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * SS_TM, col0 = blockIdx.x * SS_TN;
    const int m1 = m0 + SS_TM < num_anchors ? m0 + SS_TM : num_anchors;
    // this thread's staging pieces: piece p = tid + 256 q (q = 0, 1) of 512 per operand: plane p >> 8, tile row (p >> 2) & 63, 16 bytes p & 3
    const int prow = (tid >> 2) & 63, pk = (tid & 3) * 8;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)&img[0][0][0][0];
    constexpr uint32_t PLANE = SS_TM * SS_PITCH * 2, OPERAND = 2 * PLANE;
    const uint32_t fa = lds0 + ((wm * 32 + (lane & 15)) * SS_PITCH + (lane >> 4) * 8) * 2;
    const uint32_t fb = lds0 + OPERAND + ((wn * 32 + (lane & 15)) * SS_PITCH + (lane >> 4) * 8) * 2;

    for (int g0 = m0; g0 < m1;) {                          // one pass per entry that has anchors in this tile
        const int first = seg_first[g0], len = seg_len[g0];
        int g1 = g0 + 1;
        while (g1 < m1 && seg_first[g1] == first) ++g1;
        if (col0 < len) {
            // the rows this thread stages: an anchor of the group (or none), an entry row below the entry's end (or none)
            const int am = m0 + prow;
            const bool a_on = am >= g0 && am < g1, b_on = col0 + prow < len;
            const int64_t a_at = a_on ? (int64_t)anchor_row[am] * ld_h + pk : 0;
            const int64_t b_at = b_on ? (int64_t)(first + col0 + prow) * ld_h + pk : 0;
            const i32x4 zero = {0, 0, 0, 0};
            i32x4 ra[2], rb[2];
            auto fetch = [&](int k0) {
                ra[0] = a_on ? *reinterpret_cast<const i32x4 *>(hi + a_at + k0) : zero;
                ra[1] = a_on ? *reinterpret_cast<const i32x4 *>(lo + a_at + k0) : zero;
                rb[0] = b_on ? *reinterpret_cast<const i32x4 *>(hi + b_at + k0) : zero;
                rb[1] = b_on ? *reinterpret_cast<const i32x4 *>(lo + b_at + k0) : zero;
            };
            auto stage = [&]() {
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    *reinterpret_cast<i32x4 *>(&img[0][p][prow][pk]) = ra[p];
                    *reinterpret_cast<i32x4 *>(&img[1][p][prow][pk]) = rb[p];
                }
            };
            f32x4 acc[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            fetch(0);
            for (int k0 = 0; k0 < d; k0 += SS_TK) {
                __syncthreads();                           // every wave is done reading the image of the step before
                stage();
                __syncthreads();
                if (k0 + SS_TK < d) fetch(k0 + SS_TK);
                f16x8 a[2][2], b[2][2];                    // [16-row block][plane]
                gp_lds_rd128_mem<0>(a[0][0], fa);
                gp_lds_rd128_mem<PLANE>(a[0][1], fa);
                gp_lds_rd128_mem<16 * SS_PITCH * 2>(a[1][0], fa);
                gp_lds_rd128_mem<PLANE + 16 * SS_PITCH * 2>(a[1][1], fa);
                gp_lds_rd128_mem<0>(b[0][0], fb);
                gp_lds_rd128_mem<PLANE>(b[0][1], fb);
                gp_lds_rd128_mem<16 * SS_PITCH * 2>(b[1][0], fb);
                gp_lds_rd128_mem<PLANE + 16 * SS_PITCH * 2>(b[1][1], fb);
                ss_wait_frags(a, b);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i][0], b[j][1], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i][1], b[j][0], acc[i][j], 0, 0, 0);
                    }
            }
            // accumulator element r of a lane: tile row 4 (lane >> 4) + r (the anchor), tile column lane & 15 (the entry row)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int am2 = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;
                    if (am2 >= g0 && am2 < g1) {
                        float *orow = out + row_off[am2];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const int c = col0 + wn * 32 + j * 16 + (lane & 15);
                            if (c < len) orow[c] = acc[i][j][r];
                        }
                    }
                }
        }
        g0 = g1;
    }
}

// the order-preserving uint image of a float, as sampler_select_kernel's (train.hip): -0 counts as +0, a NaN with a clear sign bit
// orders above +inf
__device__ __forceinline__ unsigned sm_key(float v) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

// One wave per anchor: the nm lowest of the anchor's k local similarities, ascending by (value, slot in the list), a neighbour that
// is the anchor's positive counting as +inf (affinity_module.py:1125-1133: the gather reads the matrix after the in-place marks).
// k <= 128: two slots per lane, ranked by counting over the 64-bit keys (value | slot), which are unique.
__global__ void __launch_bounds__(256)
sampler_micro_kernel(const float *__restrict__ sim, const int64_t *__restrict__ row_off, const int32_t *__restrict__ seg_first,
                     const int32_t *__restrict__ seg_len, const int32_t *__restrict__ nbr, int64_t ld_nbr, int k,
                     const int64_t *__restrict__ positive, int num_anchors, int nm, int64_t *__restrict__ micro) {
    const int a = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6);
    if (a >= num_anchors) return;
    const int lane = gp_lane();
    const float *row = sim + row_off[a];
    const int first = seg_first[a], len = seg_len[a];
    const int64_t pos = positive[a];
    unsigned long long key[2];
    int who[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = lane + 64 * h;
        key[h] = ~0ull;
        who[h] = -1;
        if (s < k) {
            const int j = nbr[a * ld_nbr + s];
            const int c = j - first;
            // (a list entry outside the anchor's entry is refused before any launch; the test keeps a stray one inside the row)
            float v = INFINITY;
            if (c >= 0 && c < len && (int64_t)j != pos) v = row[c];
            key[h] = ((unsigned long long)sm_key(v) << 32) | (unsigned)s;
            who[h] = j;
        }
    }
    int rank[2] = {0, 0};
    for (int s = 0; s < k; ++s) {
        const int src = s & 63;
        const unsigned long long mine = s < 64 ? key[0] : key[1];
        const unsigned lo32 = __shfl((unsigned)mine, src, 64), hi32 = __shfl((unsigned)(mine >> 32), src, 64);
        const unsigned long long o = ((unsigned long long)hi32 << 32) | lo32;
        rank[0] += o < key[0];
        rank[1] += o < key[1];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (lane + 64 * h < k && rank[h] < nm) micro[(int64_t)a * nm + rank[h]] = who[h];
}

}  // namespace

// The anchors' rows of the similarity of affinity_module.py:1113-1115, each against the rows of its own batch entry only.
extern "C" int gp_sim_segments_f16x3(const void *hi, const void *lo, int64_t ld_h, int32_t d, const int32_t *anchor_row, const int32_t *seg_first,
                                     const int32_t *seg_len, const int64_t *row_off, int64_t num_anchors, int64_t max_len, float *out,
                                     void *stream_) {
    GP_CHECK_ARG(hi && lo && anchor_row && seg_first && seg_len && row_off && out, "gp_sim_segments_f16x3: null argument");
    GP_CHECK_ARG(d > 0 && d % 32 == 0 && ld_h >= d && ld_h % 8 == 0, "gp_sim_segments_f16x3: d=%d must be a positive multiple of 32, ld_h >= d a multiple of 8", d);
    GP_CHECK_ARG(((reinterpret_cast<uintptr_t>(hi) | reinterpret_cast<uintptr_t>(lo) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                 "gp_sim_segments_f16x3: hi, lo and out must be 16-byte aligned");
    GP_CHECK_ARG(num_anchors > 0 && max_len > 0 && max_len < INT32_MAX && (num_anchors + SS_TM - 1) / SS_TM <= 65535,
                 "gp_sim_segments_f16x3: num_anchors=%lld (at most %d per call), max_len=%lld out of range", (long long)num_anchors, 65535 * SS_TM,
                 (long long)max_len);
    dim3 grid((unsigned)((max_len + SS_TN - 1) / SS_TN), (unsigned)((num_anchors + SS_TM - 1) / SS_TM));
    sim_segments_kernel<<<grid, 256, 0, gp_stream(stream_)>>>(static_cast<const _Float16 *>(hi), static_cast<const _Float16 *>(lo), ld_h, d, anchor_row,
                                                              seg_first, seg_len, row_off, (int)num_anchors, out);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

// The local negatives of affinity_module.py:1125-1133 from the anchors' own ragged rows.
extern "C" int gp_sampler_micro_segments(const float *sim, const int64_t *row_off, const int32_t *seg_first, const int32_t *seg_len,
                                         const int32_t *nbr, int64_t ld_nbr, int32_t k, const int64_t *positive, int64_t num_anchors,
                                         int32_t num_micro, int64_t *micro, void *stream_) {
    GP_CHECK_ARG(sim && row_off && seg_first && seg_len && nbr && positive && micro, "gp_sampler_micro_segments: null argument");
    GP_CHECK_ARG(k >= 1 && k <= 128 && ld_nbr >= k && num_micro >= 1 && num_micro <= k, "gp_sampler_micro_segments: k=%d, num_micro=%d out of range (1 <= num_micro <= k <= 128)",
                 k, num_micro);
    GP_CHECK_ARG(num_anchors > 0 && num_anchors < INT32_MAX / 64, "gp_sampler_micro_segments: num_anchors=%lld out of range", (long long)num_anchors);
    sampler_micro_kernel<<<(unsigned)((num_anchors * 64 + 255) / 256), 256, 0, gp_stream(stream_)>>>(sim, row_off, seg_first, seg_len, nbr, ld_nbr, k, positive,
                                                                                                     (int)num_anchors, num_micro, micro);
    GP_CHECK_LAUNCH();
    return GP_OK;
}
