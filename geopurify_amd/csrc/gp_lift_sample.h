// The sampling walk of the dense lifts over BATCHED point clouds (lift_batched.hip: lb_lift_kernel; lift_stream.hip: ls_accum_kernel):
// which columns a lane holds, the body that adds one view's sample to them, and the host's choice of the instantiation.  One
// definition for both, so a stream's chunks take the adds of the one call in its order: the same bits.
#pragma once
#include "gp_common.h"
#include "gp_map_elem.h"
#include "gp_project.h"

namespace {

constexpr int LB_COLS_PER_LANE = 8;
constexpr int LB_COL_CHUNK = GP_WAVE * LB_COLS_PER_LANE;         // channels one pass of a walk kernel holds in registers

// the column that accumulator k of a lane holds in the chunk at c0.  VEC: the consecutive columns a lane takes with one load.  VEC = 1
// is the mapping the kernels were written with (column c0 + l + 64 k); with VEC = 4 or 8 (half maps whose rows are aligned to 8 / 16
// bytes) accumulator k holds column c0 + (64 (k / VEC) + l) VEC + k % VEC.  A column is summed by one lane under either mapping.
template <int VEC>
__device__ __forceinline__ int lb_col(int c0, int lane, int k) {
    if constexpr (VEC == 1) return c0 + lane + k * GP_WAVE;
    else return c0 + ((k / VEC) * GP_WAVE + lane) * VEC + k % VEC;
}

// acc += the sample of one view's map f ([h * w, d], pixel-major) at the pixel (row, col).  BILINEAR: the map is [h, w] and the pixel
// indexes the [H, W] image the reference resizes the map to (F.interpolate(bilinear, align_corners=True)); the resize is evaluated at
// the sampled pixel with the arithmetic of lift_dense_bilinear_accum_kernel.  Otherwise (h, w) == (H, W) and the pixel's row is added
// as it is.  T: the maps' element type (gp_map_elem.h), converted to fp32 as it is loaded, which is exact.
template <typename T, int VEC, bool BILINEAR>
__device__ __forceinline__ void lb_add_sample(const T *__restrict__ f, int row, int col, int d, int h, int w, float scale_h, float scale_w,
                                              int c0, int lane, float (&acc)[LB_COLS_PER_LANE]) {
    if (BILINEAR) {
        int r0, r1, q0, q1;
        float wr0, wr1, wc0, wc1;
        bilinear_tap(scale_h, row, h, r0, r1, wr0, wr1);
        bilinear_tap(scale_w, col, w, q0, q1, wc0, wc1);
        const T *f00 = f + ((int64_t)r0 * w + q0) * d, *f01 = f + ((int64_t)r0 * w + q1) * d;
        const T *f10 = f + ((int64_t)r1 * w + q0) * d, *f11 = f + ((int64_t)r1 * w + q1) * d;
        if constexpr (VEC == 1) {
#pragma unroll
            for (int k = 0; k < LB_COLS_PER_LANE; ++k) {
                const int c = lb_col<1>(c0, lane, k);
                if (c < d) {
                    const float top = __builtin_fmaf(wc0, gp_to_f32(f00[c]), wc1 * gp_to_f32(f01[c]));
                    const float bot = __builtin_fmaf(wc0, gp_to_f32(f10[c]), wc1 * gp_to_f32(f11[c]));
                    acc[k] += __builtin_fmaf(wr0, top, wr1 * bot);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < LB_COLS_PER_LANE / VEC; ++j) {
                const int c = lb_col<VEC>(c0, lane, j * VEC);        // (d is a multiple of VEC: the group is inside or outside)
                if (c < d) {
                    float a00[VEC], a01[VEC], a10[VEC], a11[VEC];
                    gp_load_f32<VEC>(f00 + c, a00);
                    gp_load_f32<VEC>(f01 + c, a01);
                    gp_load_f32<VEC>(f10 + c, a10);
                    gp_load_f32<VEC>(f11 + c, a11);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const float top = __builtin_fmaf(wc0, a00[i], wc1 * a01[i]);
                        const float bot = __builtin_fmaf(wc0, a10[i], wc1 * a11[i]);
                        acc[j * VEC + i] += __builtin_fmaf(wr0, top, wr1 * bot);
                    }
                }
            }
        }
    } else {
        const T *fr = f + ((int64_t)row * w + col) * d;
        if constexpr (VEC == 1) {
#pragma unroll
            for (int k = 0; k < LB_COLS_PER_LANE; ++k) {
                const int c = lb_col<1>(c0, lane, k);
                if (c < d) acc[k] += gp_to_f32(fr[c]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < LB_COLS_PER_LANE / VEC; ++j) {
                const int c = lb_col<VEC>(c0, lane, j * VEC);
                if (c < d) {
                    float a[VEC];
                    gp_load_f32<VEC>(fr + c, a);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[j * VEC + i] += a[i];
                }
            }
        }
    }
}

// The instantiation for maps of element type elem at feat with d channels: launch(LbSampleForm<T, VEC, BILINEAR>()) runs once, launch a
// generic lambda that reads the three from its argument's type.  VEC is launch-uniform: every sampled row is aligned to the load it
// names (gp_elem_vec).
template <typename T, int VEC, bool BILINEAR>
struct LbSampleForm {
    using type = T;
    static constexpr int vec = VEC;
    static constexpr bool bilinear = BILINEAR;
};
template <bool BILINEAR, typename Launch>
void lb_sample_dispatch_mode(const void *feat, int32_t elem, int32_t d, Launch launch) {
    const int vec = gp_elem_vec(feat, d, gp_elem_size(elem));
    if (elem == GP_ELEM_F32) launch(LbSampleForm<float, 1, BILINEAR>());
    else if (elem == GP_ELEM_F16 && vec == 8) launch(LbSampleForm<gp_f16, 8, BILINEAR>());
    else if (elem == GP_ELEM_F16 && vec == 4) launch(LbSampleForm<gp_f16, 4, BILINEAR>());
    else if (elem == GP_ELEM_F16) launch(LbSampleForm<gp_f16, 1, BILINEAR>());
    else if (vec == 8) launch(LbSampleForm<gp_bf16, 8, BILINEAR>());
    else if (vec == 4) launch(LbSampleForm<gp_bf16, 4, BILINEAR>());
    else launch(LbSampleForm<gp_bf16, 1, BILINEAR>());
}
template <typename Launch>
void lb_sample_dispatch(const void *feat, int32_t elem, int32_t d, int32_t bilinear, Launch launch) {
    if (bilinear) lb_sample_dispatch_mode<true>(feat, elem, d, launch);
    else lb_sample_dispatch_mode<false>(feat, elem, d, launch);
}

}  // namespace
