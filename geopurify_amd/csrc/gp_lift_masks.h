// The part of the mask-embedding lift shared by the per-scene path (lift.hip: gp_lift_masks_views) and the batched ones
// (lift_masks_batched.hip: gp_lift_masks_batched; lift_masks_stream.hip: its chunks): the score sort, the ordered transpose, the
// segment decision of a visible pixel on the score-ordered copy, and the in-view fill over view-major entries -- the kernels and, at
// the end of the file, their workspace (LvSegWork) and launch sequence (lv_segments).  One definition, so all paths take the same
// decisions and give the same bits.  The transpose and the segment decision are templates over the masks' element type (gp_map_elem.h): the batched
// paths read fp32, fp16 or bf16 logits, keep the ordered copy in that type and convert the 16 taps of a pixel to fp32 as they are
// loaded; the per-scene path instantiates float alone.
#pragma once
#include <rocprim/device/device_scan.hpp>

#include "gp_common.h"
#include "gp_map_elem.h"

namespace {

// ---- the same for ALL views of a scene: entries e = (view, point, pixel) in view-major order (gp_views_visible_lists); the masks
// of view v are mt + v * h*w*Q, its scores scores + v * Q.  Entries of dropped views get -1.
// (order: the queries of view blockIdx.z by descending score, lv_sort_scores_kernel -- row r of the transposed copy is query order[r])
// T: float, or uint16_t for both half types of the masks (gp_map_elem.h): the copy keeps the input's type, the elements are moved
template <typename T>
__global__ void transpose_views_kernel(const T *__restrict__ src, int rows, int cols, T *__restrict__ dst,
                                       const int32_t *__restrict__ order) {
    __shared__ T tile[64][65];
    const int64_t vo = (int64_t)blockIdx.z * rows * cols;
    const int32_t *ord = order + (int64_t)blockIdx.z * rows;
    int bx = blockIdx.x * 64, by = blockIdx.y * 64;
    int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    __shared__ int s_ord[64];                                  // (one load per tile row instead of a dependent load in front of every read)
    if (threadIdx.x < 64) s_ord[threadIdx.x] = by + threadIdx.x < rows ? ord[by + threadIdx.x] : 0;
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        int row = by + r, col = bx + tx;
        tile[r][tx] = (row < rows && col < cols) ? src[vo + (int64_t)s_ord[r] * cols + col] : T(0);
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        int orow = bx + r, ocol = by + tx;
        if (orow < cols && ocol < rows) dst[vo + (int64_t)orow * rows + ocol] = tile[tx][r];
    }
}
// the queries of every view by (score descending, index ascending): order i32 [V, Q] (rank -> query), sscore f32 [V, Q].  One
// workgroup per view, bitonic sort of 64-bit keys in LDS (Q <= 1024).
__global__ void __launch_bounds__(256) lv_sort_scores_kernel(const float *__restrict__ scores, int Q, int32_t *__restrict__ order,
                                                             float *__restrict__ sscore) {
    __shared__ unsigned long long key[1024];
    const int v = blockIdx.x;
    int np2 = 1;
    while (np2 < Q) np2 <<= 1;
    for (int i = threadIdx.x; i < np2; i += 256) {
        unsigned long long k = ~0ull;
        if (i < Q) {
            unsigned u = __float_as_uint(scores[(int64_t)v * Q + i]);
            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                     // monotone in the float's value
            k = ((unsigned long long)(~u) << 32) | (unsigned)i;                // ascending key = descending score, then ascending index
        }
        key[i] = k;
    }
    __syncthreads();
    for (int kk = 2; kk <= np2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < np2; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long x = key[i], y = key[ixj];
                    if ((x > y) == ((i & kk) == 0)) { key[i] = y; key[ixj] = x; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < Q; i += 256) {
        const int qo = (int)(key[i] & 0xFFFFFFFFull);
        order[(int64_t)v * Q + i] = qo;
        sscore[(int64_t)v * Q + i] = scores[(int64_t)v * Q + qo];
    }
}
// One wave per entry on the score-ordered copy.  The candidates of a pixel are the Q products score_q x sigmoid(logit_q) <= score_q:
// with the queries in descending score order, a pass of 64 can be skipped -- with every pass behind it -- as soon as its LARGEST
// score is strictly below the best product found so far (nothing in it can win or tie).  The decision is the one of
// lift_masks_point (largest product, then smallest query index; the same arithmetic per candidate), reached after 1.1 passes
// instead of 4 on the S scene's synthetic masks (92 % of the pixels stop after the first 64 queries).
// T: the masks' element type (float, gp_f16, gp_bf16); the 16 taps are converted to fp32 as they are loaded, the chain is the same.
template <typename T>
__device__ __forceinline__ void lift_masks_point_sorted(const T *__restrict__ mt /*[h*w, Q] in rank order*/, int Q, int h, int w,
                                                        const float *__restrict__ sscore, const int32_t *__restrict__ order,
                                                        const int32_t *__restrict__ tx0, const float *__restrict__ twx,
                                                        const int32_t *__restrict__ ty0, const float *__restrict__ twy, int out_h, int out_w,
                                                        int row, int col, int lane, int &seg_out) {
    bool inb = (unsigned)row < (unsigned)out_h && (unsigned)col < (unsigned)out_w;
    float best = -1.f, best_logit = 0.f;
    int best_q = -1;
    if (inb) {
        int x0 = tx0[col], y0 = ty0[row];
        float wx[4], wy[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { wx[t] = twx[col * 4 + t]; wy[t] = twy[row * 4 + t]; }
        for (int q0 = 0; q0 < Q; q0 += 64) {
            if (q0 > 0) {                                                     // wave-uniform: can the rest still matter?
                float wb = best;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) wb = fmaxf(wb, __shfl_xor(wb, o, 64));
                if (sscore[q0] < wb) break;
            }
            const int q = q0 + lane;
            if (q < Q) {
                float sc = sscore[q];
                float hr[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int yy = min(y0 + j, h - 1);
                    const T *r = mt + ((int64_t)yy * w) * Q + q;
                    float t = __fmul_rn(gp_to_f32(r[(int64_t)min(x0, w - 1) * Q]), wx[0]);
#pragma unroll
                    for (int a = 1; a < 4; ++a) t = fmaf(gp_to_f32(r[(int64_t)min(x0 + a, w - 1) * Q]), wx[a], t);
                    hr[j] = t;
                }
                float v = __fmul_rn(hr[0], wy[0]);
#pragma unroll
                for (int j = 1; j < 4; ++j) v = fmaf(hr[j], wy[j], v);
                if (sc > 0.f) {
                    float sg = 1.f / (1.f + expf(-v));
                    float pr = __fmul_rn(sc, sg);
                    const int qo = order[q];
                    if (pr > best || (pr == best && qo < best_q)) { best = pr; best_q = qo; best_logit = v; }
                }
            }
        }
    }
    // wave arg-max: larger value, then smaller (original) query index
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ob = __shfl_xor(best, o, 64);
        int oq = __shfl_xor(best_q, o, 64);
        float ol = __shfl_xor(best_logit, o, 64);
        bool take = (oq >= 0) && (best_q < 0 || ob > best || (ob == best && oq < best_q));
        if (take) { best = ob; best_q = oq; best_logit = ol; }
    }
    float sg = 1.f / (1.f + expf(-best_logit));
    seg_out = (best_q >= 0 && sg >= 0.5f) ? best_q : -1;
}
// Measured and left out (round 4): the entries of a view come in POINT order, scattered over the image, and the kernel fetches 4.6 GB
// from beyond L2 per S scene for 0.39 GB of transposed logits (PMC: 53 % L2 hits); with the entries radix-sorted by (view, 8 x 8 pixel
// tile) it takes 524 instead of 545 us and the sort costs 80 us: the wave's 16 taps x Q multiply-adds and their dependent loads
// bound it, not the bytes.  Four consecutive queries per lane with 16-byte loads (Q = 200: one pass of 16 loads on 50 lanes instead of
// four passes of 16 dword loads, the last with 8 live lanes; same bits) is SLOWER: 733 us -- the four passes keep four times as many
// loads in flight.  Round 5: a tile-major form (bins of 16 low-resolution cells staged in LDS from the [Q, h, w] layout): 1.9 ms
// (profiles/r05_lift_tile_major.log); what pays is doing less of the work: the score order above.
template <typename T>
__global__ void lift_masks_views_kernel(const T *__restrict__ mt /*[V, h*w, Q] in rank order*/, int Q, int h, int w,
                                        const float *__restrict__ sscore /*[V,Q]*/, const int32_t *__restrict__ order /*[V,Q]*/,
                                        const int32_t *__restrict__ tx0, const float *__restrict__ twx, const int32_t *__restrict__ ty0,
                                        const float *__restrict__ twy, int out_h, int out_w,
                                        const int64_t *__restrict__ ent_x, const int64_t *__restrict__ ent_y,
                                        const int32_t *__restrict__ ent_view, const uint8_t *__restrict__ keep, int64_t total,
                                        int32_t *__restrict__ seg) {
    int64_t e = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    if (e >= total) return;
    int lane = gp_lane();
    // one wave per entry: its view and pixel are wave-uniform -- said so to the compiler (readfirstlane), the tap tables of the pixel
    // (2 + 8 values) then come through the scalar cache instead of ten 64-lane loads of one address each
    const int v = __builtin_amdgcn_readfirstlane(ent_view[e]);
    const int ex = __builtin_amdgcn_readfirstlane((int)ent_x[e]), ey = __builtin_amdgcn_readfirstlane((int)ent_y[e]);
    int sg = -1;
    if (keep[v])                                                 // wave-uniform
        lift_masks_point_sorted(mt + (int64_t)v * h * w * Q, Q, h, w, sscore + (int64_t)v * Q, order + (int64_t)v * Q, tx0, twx, ty0, twy,
                                out_h, out_w, ex, ey, lane, sg);
    if (lane == 0) seg[e] = sg;
}

// ---- in-view fill for all views (affinity_module.py:604-625): every entry without a segment takes the segment of the
// nearest entry WITH one in the same view -- lexicographic minimum of (squared distance in fp64, entry index), the rule of
// gp_nn1_masked_f64.  Covered entries are compacted (exclusive scan of the flags: view-major order is kept, so a view's
// references are one contiguous range), queries likewise; blocks of 256 queries of one view stream that view's references
// through LDS tiles, the reference range cut into FV_CHUNKS parts for parallelism, then the parts are reduced in order.
constexpr int FV_CHUNKS = 16, FV_TILE = 1024;
__global__ void fill_flags_kernel(const int32_t *__restrict__ seg, int64_t total, int32_t *__restrict__ cov /*[total+1]*/) {
    int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e < total) cov[e] = seg[e] >= 0 ? 1 : 0;
    else if (e == total) cov[e] = 0;
}
__global__ void fill_compact_kernel(const float *__restrict__ xyz, const int64_t *__restrict__ ent_pt, const int32_t *__restrict__ seg,
                                    const int32_t *__restrict__ rs /*[total+1]*/, int64_t total, float *__restrict__ rxyz,
                                    int32_t *__restrict__ rent, int32_t *__restrict__ qent) {
    int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int r = rs[e];
    if (seg[e] >= 0) {
        const int64_t p = ent_pt[e];
        rxyz[(int64_t)r * 3] = xyz[p * 3]; rxyz[(int64_t)r * 3 + 1] = xyz[p * 3 + 1]; rxyz[(int64_t)r * 3 + 2] = xyz[p * 3 + 2];
        rent[r] = (int32_t)e;
    } else {
        qent[e - r] = (int32_t)e;
    }
}
// per-view table for the fill kernels, built once per scene by one small launch: tab[v] = {first query, first reference,
// first 256-query block} (+ a sentinel row): a block finds its view by a binary search over the block column instead of
// walking the view offsets (four dependent global loads per view and block: 0.19 ms per scene in 62k mostly idle blocks)
__global__ void fill_table_kernel(const int64_t *__restrict__ view_off, const int32_t *__restrict__ rs, int nviews, int4 *__restrict__ tab) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int blk = 0;
    for (int v = 0; v <= nviews; ++v) {
        const int64_t o = view_off[v];
        const int r = rs[o], q = (int)(o - r);
        tab[v] = make_int4(q, r, blk, 0);
        if (v < nviews) {
            const int64_t o1 = view_off[v + 1];
            const int q1 = (int)(o1 - rs[o1]);
            blk += (q1 - q + 255) / 256;
        }
    }
}
// block -> (view, block of 256 queries of that view); blocks beyond the last view's exit
__device__ __forceinline__ bool fill_locate(const int4 *__restrict__ tab, int nviews, int bx, int &q0, int &q1, int &r0, int &r1) {
    if (bx >= tab[nviews].z) return false;
    int lo = 0, hi = nviews - 1;
    while (lo < hi) {                                            // last view whose first block is <= bx (empty views share a start)
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].z <= bx) lo = mid; else hi = mid - 1;
    }
    const int4 a = tab[lo], b = tab[lo + 1];
    q0 = a.x + (bx - a.z) * 256;
    q1 = b.x;
    r0 = a.y;
    r1 = b.y;
    return true;
}
// The partial results of the FV_CHUNKS reference parts live in part_d / part_i [FV_CHUNKS][stride], indexed by the QUERY's compact
// index -- so `stride` only has to cover the fill queries (uncovered entries), not every entry (192 B per entry,
// 0.7 GB at config M).  The number of queries is known on the device only; the caller passes a capacity (fill_cap) and a block of
// queries that does not fit below it takes the overflow path: ONE block (blockIdx.y == 0) sweeps the view's whole reference
// range and writes the result itself -- same (d2, index) rule, same result, no partials, just less parallel.
__global__ void __launch_bounds__(256)
fill_part_kernel(const float *__restrict__ xyz, const int64_t *__restrict__ ent_pt, const int4 *__restrict__ tab, int nviews,
                 const float *__restrict__ rxyz, const int32_t *__restrict__ qent,
                 double *__restrict__ part_d, int32_t *__restrict__ part_i, int64_t stride,
                 const int32_t *__restrict__ rent, int32_t *__restrict__ seg) {
    __shared__ double sx[FV_TILE], sy[FV_TILE], sz[FV_TILE];
    int q0, q1, vr0, vr1;
    if (!fill_locate(tab, nviews, blockIdx.x, q0, q1, vr0, vr1)) return;                  // block-uniform
    const int n_ref = vr1 - vr0;
    if (n_ref == 0) return;
    const bool overflow = (int64_t)q0 + 256 > stride;                                     // block-uniform
    if (overflow && blockIdx.y != 0) return;
    const int per = overflow ? n_ref : (n_ref + FV_CHUNKS - 1) / FV_CHUNKS;
    const int r0 = vr0 + blockIdx.y * per, r1 = r0 + per < vr1 ? r0 + per : vr1;
    const int qi = q0 + threadIdx.x;
    const bool live = qi < q1;
    double qx = 0, qy = 0, qz = 0;
    if (live) {
        const int64_t p = ent_pt[qent[qi]];
        qx = xyz[p * 3]; qy = xyz[p * 3 + 1]; qz = xyz[p * 3 + 2];
    }
    double best = INFINITY;
    int bi = -1;
    for (int t0 = r0; t0 < r1; t0 += FV_TILE) {
        int cnt = r1 - t0 < FV_TILE ? r1 - t0 : FV_TILE;
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += 256) {
            sx[j] = rxyz[(int64_t)(t0 + j) * 3]; sy[j] = rxyz[(int64_t)(t0 + j) * 3 + 1]; sz[j] = rxyz[(int64_t)(t0 + j) * 3 + 2];
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            double dx = qx - sx[j], dy = qy - sy[j], dz = qz - sz[j];
            double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < best) { best = d2; bi = t0 + j; }
        }
    }
    if (!live) return;
    if (overflow) {
        if (bi >= 0) seg[qent[qi]] = seg[rent[bi]];              // references keep their segment: no read/write overlap
        return;
    }
    part_d[(int64_t)blockIdx.y * stride + qi] = best;
    part_i[(int64_t)blockIdx.y * stride + qi] = bi;
}
__global__ void fill_reduce_kernel(const int4 *__restrict__ tab, int nviews,
                                   const double *__restrict__ part_d, const int32_t *__restrict__ part_i, int64_t stride,
                                   const int32_t *__restrict__ rent, const int32_t *__restrict__ qent, int32_t *__restrict__ seg) {
    int q0, q1, vr0, vr1;
    if (!fill_locate(tab, nviews, blockIdx.x, q0, q1, vr0, vr1)) return;
    if (vr1 == vr0) return;
    if ((int64_t)q0 + 256 > stride) return;                      // an overflow block wrote its results itself
    const int qi = q0 + threadIdx.x;
    if (qi >= q1) return;
    const int per = (vr1 - vr0 + FV_CHUNKS - 1) / FV_CHUNKS;
    double best = INFINITY;
    int bi = -1;
    for (int c = 0; c < FV_CHUNKS; ++c) {
        if (vr0 + c * per >= vr1) break;                         // chunks beyond the range wrote nothing
        double d = part_d[(int64_t)c * stride + qi];
        int i = part_i[(int64_t)c * stride + qi];
        if (i >= 0 && d < best) { best = d; bi = i; }
    }
    if (bi >= 0) seg[qent[qi]] = seg[rent[bi]];                  // references keep their segment: no read/write overlap
}

// ================================================================================================ host side
// the arrays of the segment decision and the in-view fill.  nsets: the mask sets the ordered copy holds ([nsets, h * w, q] elements of
// esize bytes); fill_cap: the queries the fill's partial results hold; ntab: the rows of the fill's view table (views + 1 at least)
struct LvSegWork {
    void *mt = nullptr;                                          // (the rank-ordered transposed masks, in the masks' own element type)
    float *sscore = nullptr, *rxyz = nullptr;
    int32_t *order = nullptr, *cov = nullptr, *rs = nullptr, *rent = nullptr, *qent = nullptr, *part_i = nullptr;
    double *part_d = nullptr;
    int4 *tab = nullptr;
    LvSegWork() = default;
    LvSegWork(GpCarver &cv, int32_t nsets, int32_t q, int32_t h, int32_t w, int64_t total, int64_t fill_cap, size_t esize, size_t ntab) {
        mt = cv.take<char>((size_t)nsets * q * h * w * esize);
        order = cv.take<int32_t>((size_t)nsets * q);
        sscore = cv.take<float>((size_t)nsets * q);
        cov = cv.take<int32_t>(total + 1);
        rs = cv.take<int32_t>(total + 1);
        rent = cv.take<int32_t>(total);
        qent = cv.take<int32_t>(total);
        rxyz = cv.take<float>(total * 3);
        part_d = cv.take<double>((size_t)FV_CHUNKS * fill_cap);
        part_i = cv.take<int32_t>((size_t)FV_CHUNKS * fill_cap);
        tab = cv.take<int4>(ntab);
    }
};

// seg[e] = the segment of every entry e = (view, point, pixel), view-major with view v's entries at [view_off[v], view_off[v + 1]):
// the score sort, the ordered copy of the masks, the decision at the entry's pixel, then the in-view fill.  T: the masks' element
// type, BITS: the integer or float type of its size that the transpose moves.  tmp holds an int32 scan over total + 1 elements.
template <typename T, typename BITS>
int lv_segments(const void *pred_masks, int32_t nviews, int32_t q, int32_t h, int32_t w, const float *scores, const int32_t *tap_x0,
                const float *tap_wx, const int32_t *tap_y0, const float *tap_wy, int32_t out_h, int32_t out_w, const float *xyz,
                const int64_t *ent_pt, const int64_t *ent_x, const int64_t *ent_y, const int32_t *ent_view, const int64_t *view_off,
                const uint8_t *keep, int64_t total, int64_t fill_cap, const LvSegWork &k, char *tmp, size_t tmp_bytes, int32_t *seg,
                hipStream_t s) {
    const int64_t hw = (int64_t)h * w;
    lv_sort_scores_kernel<<<nviews, 256, 0, s>>>(scores, q, k.order, k.sscore);
    const dim3 tg((unsigned)((hw + 63) / 64), (unsigned)((q + 63) / 64), (unsigned)nviews);
    transpose_views_kernel<BITS><<<tg, 256, 0, s>>>(static_cast<const BITS *>(pred_masks), q, (int)hw, static_cast<BITS *>(k.mt), k.order);
    lift_masks_views_kernel<T><<<(unsigned)((total * 64 + 255) / 256), 256, 0, s>>>(static_cast<const T *>(k.mt), q, h, w, k.sscore, k.order,
                                                                                     tap_x0, tap_wx, tap_y0, tap_wy, out_h, out_w, ent_x, ent_y,
                                                                                     ent_view, keep, total, seg);
    GP_CHECK_LAUNCH();
    // the in-view fill
    const unsigned eb = (unsigned)((total + 1 + 255) / 256);
    fill_flags_kernel<<<eb, 256, 0, s>>>(seg, total, k.cov);
    size_t tb = tmp_bytes;
    GP_CHECK_HIP(rocprim::exclusive_scan(tmp, tb, k.cov, k.rs, (int32_t)0, (size_t)(total + 1), rocprim::plus<int32_t>(), s));
    fill_compact_kernel<<<eb, 256, 0, s>>>(xyz, ent_pt, seg, k.rs, total, k.rxyz, k.rent, k.qent);
    const unsigned qb = (unsigned)(total / 256 + nviews + 1);                            // >= sum over views of ceil(queries / 256)
    fill_table_kernel<<<1, 64, 0, s>>>(view_off, k.rs, nviews, k.tab);
    fill_part_kernel<<<dim3(qb, FV_CHUNKS), 256, 0, s>>>(xyz, ent_pt, k.tab, nviews, k.rxyz, k.qent, k.part_d, k.part_i, fill_cap, k.rent, seg);
    fill_reduce_kernel<<<qb, 256, 0, s>>>(k.tab, nviews, k.part_d, k.part_i, fill_cap, k.rent, k.qent, seg);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

}  // namespace
