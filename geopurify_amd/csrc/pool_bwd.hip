// The backward of the purifying step (models/affinity_module.py:1564-1587): the transposed application of the ELL operator through an
// inverted index of the neighbour lists, the gradient of the affinity weights, the backward of the sharpened softmax over cosine
// similarities and of the row normalisation.  No float atomics anywhere: every sum runs over a list in a fixed order (ascending
// slot i * k + j for the transposed lists), so the gradients are bitwise reproducible.  One wave per destination row (and 256-column
// slab), 16 B per lane, wave-uniform indices and weights -- the shape of pool_ell_kernel.
#include "gp_common.h"
#include "gp_scan_bytes.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

// ------------------------------------------------------------------------------------------------
// inverted index: key = the neighbour id of slot p (nv for an id outside 0..nv-1: such slots sort behind every list and are in none),
// value = p; in-degrees by integer atomics (the counts do not depend on the order of arrival)
__global__ void tr_keys_count_kernel(const int32_t *__restrict__ nbr, int64_t total, int64_t nv, uint32_t *__restrict__ keys,
                                     int32_t *__restrict__ slots, unsigned long long *__restrict__ cnt) {
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p >= total) return;
    const int32_t m = nbr[p];
    const bool ok = (uint64_t)(uint32_t)m < (uint64_t)nv;
    keys[p] = ok ? (uint32_t)m : (uint32_t)nv;
    slots[p] = (int32_t)p;
    if (ok) atomicAdd(cnt + m, 1ull);
}

int tr_key_bits(int64_t nv) {                                    // keys are 0 .. nv
    int bits = 1;
    while (bits < 32 && (1ll << bits) <= nv) ++bits;
    return bits;
}

size_t tr_sort_bytes(int64_t total, int bits) {
    size_t t = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
                                    (size_t)total, 0, bits, 0);
    return t;
}

// ------------------------------------------------------------------------------------------------
// out[m] = sum over the list of m, in list order, of w[slot] * g[slot / k]: one wave per (row, 256-column slab)
template <int UNROLL>
__global__ void __launch_bounds__(256) pool_ell_transpose_kernel(const float *__restrict__ g, int64_t ld_g,
                                                                 const int64_t *__restrict__ tr_off, const int32_t *__restrict__ tr_slot,
                                                                 const float *__restrict__ w, int k, int64_t nv, int d,
                                                                 float *__restrict__ out, int64_t ld_out, int slabs) {
    int64_t wid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    int64_t row = wid / slabs;
    int slab = (int)(wid - row * slabs);
    if (row >= nv) return;
    row = __builtin_amdgcn_readfirstlane((int)row);
    slab = __builtin_amdgcn_readfirstlane(slab);
    const int c = slab * 256 + gp_lane() * 4;
    const bool act = c < d;
    const int64_t b = tr_off[row], e = tr_off[row + 1];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int64_t p = b;
    for (; p + UNROLL <= e; p += UNROLL) {
        float4 t[UNROLL];
        float ww[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int32_t slot = tr_slot[p + u];
            const int64_t r = slot / k;
            ww[u] = w[slot];
            t[u] = act ? *reinterpret_cast<const float4 *>(g + r * ld_g + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            acc.x = fmaf(ww[u], t[u].x, acc.x);
            acc.y = fmaf(ww[u], t[u].y, acc.y);
            acc.z = fmaf(ww[u], t[u].z, acc.z);
            acc.w = fmaf(ww[u], t[u].w, acc.w);
        }
    }
    for (; p < e; ++p) {
        const int32_t slot = tr_slot[p];
        const int64_t r = slot / k;
        const float wj = w[slot];
        if (act) {
            const float4 t = *reinterpret_cast<const float4 *>(g + r * ld_g + c);
            acc.x = fmaf(wj, t.x, acc.x); acc.y = fmaf(wj, t.y, acc.y);
            acc.z = fmaf(wj, t.z, acc.z); acc.w = fmaf(wj, t.w, acc.w);
        }
    }
    if (act) *reinterpret_cast<float4 *>(out + row * ld_out + c) = acc;         // (an empty list: an exact zero row)
}

// ------------------------------------------------------------------------------------------------
// dw[i,j] (+)= <g[i], x[nbr[i,j]]>: one wave per row.  NS > 0: g[i] sits in registers (NS slabs of 256 columns); NS = 0: any width,
// g[i] re-read per neighbour.  Per lane the products are summed in column order over the slabs in slab order, then across the wave.
template <int NS>
__global__ void __launch_bounds__(256) pool_ell_wgrad_kernel(const float *__restrict__ g, int64_t ld_g, const float *__restrict__ x,
                                                             int64_t ld_x, const int32_t *__restrict__ nbr, int k, int64_t nv, int d,
                                                             float *__restrict__ dw, int accumulate) {
    int64_t row = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    if (row >= nv) return;
    row = __builtin_amdgcn_readfirstlane((int)row);
    const int lane = gp_lane();
    const int slabs = (d + 255) / 256;
    const float *grow = g + row * ld_g;
    float4 gr[NS > 0 ? NS : 1];
    if constexpr (NS > 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int c = s * 256 + lane * 4;
            gr[s] = c < d ? *reinterpret_cast<const float4 *>(grow + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const int32_t *nb = nbr + row * k;
    for (int j0 = 0; j0 < k; j0 += 8) {
        float part[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            part[u] = 0.f;
            const int j = j0 + u;
            if (j >= k) continue;
            const int32_t r = nb[j];
            if ((uint64_t)(uint32_t)r >= (uint64_t)nv) continue;                 // (an id outside the rows contributes nothing)
            const float *xr = x + (int64_t)r * ld_x;
            float a = 0.f;
            if constexpr (NS > 0) {
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int c = s * 256 + lane * 4;
                    if (c < d) {
                        const float4 t = *reinterpret_cast<const float4 *>(xr + c);
                        a = fmaf(gr[s].x, t.x, a); a = fmaf(gr[s].y, t.y, a);
                        a = fmaf(gr[s].z, t.z, a); a = fmaf(gr[s].w, t.w, a);
                    }
                }
            } else {
                for (int s = 0; s < slabs; ++s) {
                    const int c = s * 256 + lane * 4;
                    if (c < d) {
                        const float4 q = *reinterpret_cast<const float4 *>(grow + c);
                        const float4 t = *reinterpret_cast<const float4 *>(xr + c);
                        a = fmaf(q.x, t.x, a); a = fmaf(q.y, t.y, a);
                        a = fmaf(q.z, t.z, a); a = fmaf(q.w, t.w, a);
                    }
                }
            }
            part[u] = a;
        }
        float v = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float s = gp_wave_sum(part[u]);
            v = lane == u ? s : v;
        }
        if (lane < 8 && j0 + lane < k) {
            const int64_t at = row * k + j0 + lane;
            dw[at] = accumulate ? dw[at] + v : v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// da[i,j] = sharpen * w[i,j] * (dw[i,j] - sum_k w[i,k] dw[i,k]): one wave per row, k <= 128 (two slots per lane)
__global__ void __launch_bounds__(256) softmax_da_kernel(const float *__restrict__ w, const float *__restrict__ dw, int k, int64_t nv,
                                                         float sharpen, float *__restrict__ da) {
    const int64_t row = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    if (row >= nv) return;
    const int lane = gp_lane();
    const int64_t base = row * k;
    const bool h0 = lane < k, h1 = lane + 64 < k;
    const float w0 = h0 ? w[base + lane] : 0.f, w1 = h1 ? w[base + lane + 64] : 0.f;
    const float g0 = h0 ? dw[base + lane] : 0.f, g1 = h1 ? dw[base + lane + 64] : 0.f;
    const float s = gp_wave_sum(w0 * g0 + w1 * g1);
    if (h0) da[base + lane] = sharpen * w0 * (g0 - s);
    if (h1) da[base + lane + 64] = sharpen * w1 * (g1 - s);
}

// de[i] = sum_j da[i,j] e[nbr[i,j]]  (the row's own list, in list order)  +  sum over the inverted list of i of da[slot] e[slot / k]
__global__ void __launch_bounds__(256) softmax_de_kernel(const float *__restrict__ e, int64_t ld_e, int d, const int32_t *__restrict__ nbr,
                                                         const float *__restrict__ da, int k, int64_t nv,
                                                         const int64_t *__restrict__ tr_off, const int32_t *__restrict__ tr_slot,
                                                         float *__restrict__ de, int64_t ld_de, int slabs) {
    int64_t wid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    int64_t row = wid / slabs;
    int slab = (int)(wid - row * slabs);
    if (row >= nv) return;
    row = __builtin_amdgcn_readfirstlane((int)row);
    slab = __builtin_amdgcn_readfirstlane(slab);
    const int c = slab * 256 + gp_lane() * 4;
    const bool act = c < d;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < k; ++j) {
        const int32_t r = nbr[row * k + j];
        const float a = da[row * k + j];
        if (act && (uint64_t)(uint32_t)r < (uint64_t)nv) {
            const float4 t = *reinterpret_cast<const float4 *>(e + (int64_t)r * ld_e + c);
            acc.x = fmaf(a, t.x, acc.x); acc.y = fmaf(a, t.y, acc.y);
            acc.z = fmaf(a, t.z, acc.z); acc.w = fmaf(a, t.w, acc.w);
        }
    }
    const int64_t b = tr_off[row], end = tr_off[row + 1];
    for (int64_t p = b; p < end; ++p) {
        const int32_t slot = tr_slot[p];
        const int64_t r = slot / k;
        const float a = da[slot];
        if (act) {
            const float4 t = *reinterpret_cast<const float4 *>(e + r * ld_e + c);
            acc.x = fmaf(a, t.x, acc.x); acc.y = fmaf(a, t.y, acc.y);
            acc.z = fmaf(a, t.z, acc.z); acc.w = fmaf(a, t.w, acc.w);
        }
    }
    if (act) *reinterpret_cast<float4 *>(de + row * ld_de + c) = acc;
}

// ------------------------------------------------------------------------------------------------
// backward of l2norm_rows_kernel: u = e / max(|e|, 1e-12);  de = (du - u <u, du>) / |e|, or du / 1e-12 where |e| < 1e-12
__global__ void __launch_bounds__(256) l2norm_rows_backward_kernel(const float *__restrict__ e, int64_t ld_e, const float *__restrict__ du,
                                                                   int64_t ld_du, int d, int64_t n, float *__restrict__ de, int64_t ld_de) {
    const int64_t r = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    if (r >= n) return;
    const int lane = gp_lane();
    float ss = 0.f;
    for (int c = lane; c < d; c += 64) { const float v = e[r * ld_e + c]; ss += v * v; }
    ss = gp_wave_sum(ss);
    const float nrm = sqrtf(ss);
    if (nrm < 1e-12f) {
        for (int c = lane; c < d; c += 64) de[r * ld_de + c] = du[r * ld_du + c] / 1e-12f;
        return;
    }
    float dot = 0.f;
    for (int c = lane; c < d; c += 64) dot += (e[r * ld_e + c] / nrm) * du[r * ld_du + c];
    dot = gp_wave_sum(dot);
    for (int c = lane; c < d; c += 64) {
        const float u = e[r * ld_e + c] / nrm;
        de[r * ld_de + c] = (du[r * ld_du + c] - u * dot) / nrm;
    }
}

inline bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" size_t gp_pool_transpose_workspace_bytes(int64_t nv, int32_t k) {
    if (nv <= 0 || k < 1 || k > 128 || nv * k >= (1ll << 31)) return 0;
    const int64_t total = nv * k;
    GpCarver cv(nullptr, 0);
    cv.take<int64_t>(nv + 1);
    cv.take<uint32_t>(total);
    cv.take<uint32_t>(total);
    cv.take<int32_t>(total);
    cv.take<char>(gp_scan_bytes<int64_t>(nv + 1));
    cv.take<char>(tr_sort_bytes(total, tr_key_bits(nv)));
    return cv.off;
}

extern "C" int gp_pool_transpose_build(const int32_t *nbr, int64_t nv, int32_t k, int64_t *tr_off, int32_t *tr_slot, void *workspace,
                                       size_t workspace_bytes, void *stream_) {
    GP_CHECK_ARG(k >= 1 && k <= 128, "gp_pool_transpose_build: k=%d not in 1..128", k);
    GP_CHECK_ARG(nbr && tr_off && tr_slot && workspace, "gp_pool_transpose_build: null argument");
    GP_CHECK_ARG(nv > 0 && nv * k < (1ll << 31), "gp_pool_transpose_build: nv=%lld, nv * k must stay below 2^31", (long long)nv);
    GP_CHECK_ARG((const void *)tr_slot != (const void *)nbr && (const void *)tr_off != (const void *)nbr,
                 "gp_pool_transpose_build: the outputs must not alias nbr");
    hipStream_t s = gp_stream(stream_);
    const int64_t total = nv * k;
    const int bits = tr_key_bits(nv);
    const size_t scan_tmp = gp_scan_bytes<int64_t>(nv + 1), sort_tmp = tr_sort_bytes(total, bits);
    GpCarver cv(workspace, workspace_bytes);
    int64_t *cnt = cv.take<int64_t>(nv + 1);
    uint32_t *k0 = cv.take<uint32_t>(total);
    uint32_t *k1 = cv.take<uint32_t>(total);
    int32_t *v0 = cv.take<int32_t>(total);
    char *ts = cv.take<char>(scan_tmp);
    char *tt = cv.take<char>(sort_tmp);
    if (!cv.ok()) {
        gp_set_error("gp_pool_transpose_build: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    GP_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)(nv + 1) * sizeof(int64_t), s));
    tr_keys_count_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(nbr, total, nv, k0, v0, reinterpret_cast<unsigned long long *>(cnt));
    GP_CHECK_LAUNCH();
    size_t io = scan_tmp;
    GP_CHECK_HIP(rocprim::exclusive_scan(ts, io, cnt, tr_off, (int64_t)0, (size_t)(nv + 1), rocprim::plus<int64_t>(), s));
    io = sort_tmp;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(tt, io, k0, k1, v0, tr_slot, (size_t)total, 0, bits, s));     // (stable: slots ascend inside a list)
    return GP_OK;
}

extern "C" int gp_pool_ell_transpose(const float *g, int64_t ld_g, const int64_t *tr_off, const int32_t *tr_slot, const float *w,
                                     int32_t k, int64_t nv, int32_t d, float *out, int64_t ld_out, void *stream_) {
    GP_CHECK_ARG(k >= 1 && k <= 128, "gp_pool_ell_transpose: k=%d not in 1..128", k);
    GP_CHECK_ARG(g && tr_off && tr_slot && w && out && nv > 0, "gp_pool_ell_transpose: null/empty argument");
    GP_CHECK_ARG(nv * k < (1ll << 31), "gp_pool_ell_transpose: nv * k must stay below 2^31");
    GP_CHECK_ARG(d > 0 && d % 4 == 0 && ld_g % 4 == 0 && ld_out % 4 == 0 && ld_g >= d && ld_out >= d,
                 "gp_pool_ell_transpose: d and the pitches must be multiples of 4, the pitches at least d");
    GP_CHECK_ARG(aligned16(g) && aligned16(out), "gp_pool_ell_transpose: g/out must be 16-byte aligned");
    GP_CHECK_ARG(g != out && (const void *)w != (const void *)out, "gp_pool_ell_transpose: out must not alias g or w");
    const int slabs = (d + 255) / 256;
    const int64_t waves = nv * slabs;
    pool_ell_transpose_kernel<8><<<(unsigned)((waves * 64 + 255) / 256), 256, 0, gp_stream(stream_)>>>(g, ld_g, tr_off, tr_slot, w, k, nv, d,
                                                                                                      out, ld_out, slabs);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_pool_ell_wgrad(const float *g, int64_t ld_g, const float *x_prev, int64_t ld_x, const int32_t *nbr, int32_t k,
                                 int64_t nv, int32_t d, float *dw, int32_t accumulate, void *stream_) {
    GP_CHECK_ARG(k >= 1 && k <= 128, "gp_pool_ell_wgrad: k=%d not in 1..128", k);
    GP_CHECK_ARG(g && x_prev && nbr && dw && nv > 0, "gp_pool_ell_wgrad: null/empty argument");
    GP_CHECK_ARG(d > 0 && d % 4 == 0 && ld_g % 4 == 0 && ld_x % 4 == 0 && ld_g >= d && ld_x >= d,
                 "gp_pool_ell_wgrad: d and the pitches must be multiples of 4, the pitches at least d");
    GP_CHECK_ARG(aligned16(g) && aligned16(x_prev), "gp_pool_ell_wgrad: g/x_prev must be 16-byte aligned");
    GP_CHECK_ARG(dw != g && dw != x_prev && (const void *)dw != (const void *)nbr, "gp_pool_ell_wgrad: dw must not alias an input");
    const unsigned blocks = (unsigned)((nv * 64 + 255) / 256);
    hipStream_t s = gp_stream(stream_);
    const int slabs = (d + 255) / 256, acc = accumulate ? 1 : 0;
    if (slabs == 1) pool_ell_wgrad_kernel<1><<<blocks, 256, 0, s>>>(g, ld_g, x_prev, ld_x, nbr, k, nv, d, dw, acc);
    else if (slabs == 2) pool_ell_wgrad_kernel<2><<<blocks, 256, 0, s>>>(g, ld_g, x_prev, ld_x, nbr, k, nv, d, dw, acc);
    else if (slabs <= 4) pool_ell_wgrad_kernel<4><<<blocks, 256, 0, s>>>(g, ld_g, x_prev, ld_x, nbr, k, nv, d, dw, acc);
    else pool_ell_wgrad_kernel<0><<<blocks, 256, 0, s>>>(g, ld_g, x_prev, ld_x, nbr, k, nv, d, dw, acc);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" size_t gp_affinity_softmax_backward_workspace_bytes(int64_t nv, int32_t k) {
    if (nv <= 0 || k < 1 || k > 128 || nv * k >= (1ll << 31)) return 0;
    GpCarver cv(nullptr, 0);
    cv.take<float>(nv * k);
    return cv.off;
}

extern "C" int gp_affinity_softmax_backward(const float *e_unit, int64_t ld_e, int32_t d, const int32_t *nbr, const float *w,
                                            const float *dw, int32_t k, int64_t nv, float sharpen, const int64_t *tr_off,
                                            const int32_t *tr_slot, float *de_unit, int64_t ld_de, void *workspace,
                                            size_t workspace_bytes, void *stream_) {
    GP_CHECK_ARG(k >= 1 && k <= 128, "gp_affinity_softmax_backward: k=%d not in 1..128", k);
    GP_CHECK_ARG(e_unit && nbr && w && dw && tr_off && tr_slot && de_unit && workspace && nv > 0,
                 "gp_affinity_softmax_backward: null/empty argument");
    GP_CHECK_ARG(nv * k < (1ll << 31), "gp_affinity_softmax_backward: nv * k must stay below 2^31");
    GP_CHECK_ARG(d > 0 && d % 4 == 0 && ld_e % 4 == 0 && ld_de % 4 == 0 && ld_e >= d && ld_de >= d,
                 "gp_affinity_softmax_backward: d and the pitches must be multiples of 4, the pitches at least d");
    GP_CHECK_ARG(aligned16(e_unit) && aligned16(de_unit), "gp_affinity_softmax_backward: e_unit/de_unit must be 16-byte aligned");
    GP_CHECK_ARG(de_unit != e_unit && de_unit != w && de_unit != dw, "gp_affinity_softmax_backward: de_unit must not alias an input");
    GpCarver cv(workspace, workspace_bytes);
    float *da = cv.take<float>(nv * k);
    if (!cv.ok()) {
        gp_set_error("gp_affinity_softmax_backward: workspace too small (%zu < %zu)", workspace_bytes, cv.off);
        return GP_ENOMEM;
    }
    hipStream_t s = gp_stream(stream_);
    softmax_da_kernel<<<(unsigned)((nv * 64 + 255) / 256), 256, 0, s>>>(w, dw, k, nv, sharpen, da);
    GP_CHECK_LAUNCH();
    const int slabs = (d + 255) / 256;
    const int64_t waves = nv * slabs;
    softmax_de_kernel<<<(unsigned)((waves * 64 + 255) / 256), 256, 0, s>>>(e_unit, ld_e, d, nbr, da, k, nv, tr_off, tr_slot, de_unit, ld_de,
                                                                          slabs);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_l2norm_rows_backward(const float *e_raw, int64_t ld_e, const float *de_unit, int64_t ld_du, int32_t d, int64_t n,
                                       float *de_raw, int64_t ld_de, void *stream_) {
    GP_CHECK_ARG(e_raw && de_unit && de_raw && n > 0, "gp_l2norm_rows_backward: null/empty argument");
    GP_CHECK_ARG(d > 0 && d % 4 == 0 && ld_e % 4 == 0 && ld_du % 4 == 0 && ld_de % 4 == 0 && ld_e >= d && ld_du >= d && ld_de >= d,
                 "gp_l2norm_rows_backward: d and the pitches must be multiples of 4, the pitches at least d");
    GP_CHECK_ARG(aligned16(e_raw) && aligned16(de_unit) && aligned16(de_raw), "gp_l2norm_rows_backward: rows must be 16-byte aligned");
    GP_CHECK_ARG(de_raw != e_raw && de_raw != de_unit, "gp_l2norm_rows_backward: de_raw must not alias an input");
    l2norm_rows_backward_kernel<<<(unsigned)((n * 64 + 255) / 256), 256, 0, gp_stream(stream_)>>>(e_raw, ld_e, de_unit, ld_du, d, n, de_raw,
                                                                                                 ld_de);
    GP_CHECK_LAUNCH();
    return GP_OK;
}
