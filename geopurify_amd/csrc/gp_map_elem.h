// The element types the batched lifts read the VLM's outputs in (feature maps, mask logits): fp32, fp16 and bf16, named in the C-ABI
// by a tag (GP_ELEM_F32 / GP_ELEM_F16 / GP_ELEM_BF16 of include/geopurify_hip.h).  A kernel template over the element type converts
// every loaded element to fp32 -- both conversions are exact -- and then runs the arithmetic of its fp32 instantiation, so a half
// input gives the bits of the same call on the caller's own fp32 copy.  Kernels that only move elements (the transposes) are
// instantiated on the element's size: float and uint16_t.
#pragma once
#include "gp_common.h"

namespace {

typedef _Float16 gp_f16;                                         // v_cvt_f32_f16: exact, subnormals included
struct gp_bf16 { uint16_t bits; };                               // the upper half of the fp32 with the same value

__device__ __forceinline__ float gp_to_f32(float x) { return x; }
__device__ __forceinline__ float gp_to_f32(gp_f16 x) { return (float)x; }
__device__ __forceinline__ float gp_to_f32(gp_bf16 x) { return __uint_as_float((uint32_t)x.bits << 16); }

// VEC consecutive elements at p as fp32, by ONE load of VEC * sizeof(T) bytes; p is aligned to that many bytes (the caller's
// launch-uniform test on the base pointer and the row length)
template <int VEC, typename T>
__device__ __forceinline__ void gp_load_f32(const T *__restrict__ p, float (&x)[VEC]) {
    T raw[VEC];
    __builtin_memcpy(raw, __builtin_assume_aligned(p, VEC * sizeof(T)), VEC * sizeof(T));
#pragma unroll
    for (int i = 0; i < VEC; ++i) x[i] = gp_to_f32(raw[i]);
}

// The conversions of the kernels that write rows in another element type (fuse.hip, render_rows.hip), each element converted once, to
// the bits of torch's .to(dtype).  fp32 -> fp16: v_cvt_f16_f32, nearest even, inf on overflow, subnormals kept.
template <typename TO, typename TI>
__device__ __forceinline__ TO gp_cvt(TI x) { return (TO)x; }
// fp32 -> bf16: nearest even on the bit pattern, every NaN the one quiet NaN 0x7FC0 (the integer rounding alone would turn some NaNs
// into zero or infinity)
template <>
__device__ __forceinline__ gp_bf16 gp_cvt<gp_bf16, float>(float x) {
    const uint32_t u = __float_as_uint(x);
    gp_bf16 y;
    y.bits = x != x ? (uint16_t)0x7FC0 : (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
    return y;
}

// VEC consecutive elements by ONE access of VEC * sizeof(T) bytes; p is aligned to that many bytes
template <int VEC, typename T>
__device__ __forceinline__ void gp_store_vec(T *__restrict__ p, const T (&x)[VEC]) {
    __builtin_memcpy(__builtin_assume_aligned(p, VEC * sizeof(T)), x, VEC * sizeof(T));
}
template <int VEC, typename T>
__device__ __forceinline__ void gp_load_vec(const T *__restrict__ p, T (&x)[VEC]) {
    __builtin_memcpy(x, __builtin_assume_aligned(p, VEC * sizeof(T)), VEC * sizeof(T));
}

inline bool gp_elem_ok(int32_t elem) { return elem == GP_ELEM_F32 || elem == GP_ELEM_F16 || elem == GP_ELEM_BF16; }
inline size_t gp_elem_size(int32_t elem) { return elem == GP_ELEM_F32 ? 4 : 2; }

// the widest load a lane may take from rows of `d` elements of `esize` bytes that start at `base`: 8 elements (16 bytes), 4
// (8 bytes) or 1 -- every row and every group of that many columns is then aligned to the load.  fp32 rows keep the one-element
// mapping they were written with.
inline int gp_elem_vec(const void *base, int64_t d, size_t esize) {
    if (esize != 2) return 1;
    if (d % 8 == 0 && (uintptr_t)base % 16 == 0) return 8;
    if (d % 4 == 0 && (uintptr_t)base % 8 == 0) return 4;
    return 1;
}

}  // namespace
