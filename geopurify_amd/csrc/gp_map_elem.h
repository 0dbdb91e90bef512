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
