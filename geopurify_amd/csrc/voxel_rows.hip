// Row 8 with everything the student's first layer and the pooling take from it, in one pass over the points: the voxel means of the
// lifted features and of the geometry features, the zero pad columns, the fp32 row, its row-scaled interleaved f16 operand and the
// global maximum behind the pooling planes' power of two.  One wave per voxel holds the whole row in registers; the arithmetic is
// that of scatter_mean_csr*_kernel (pool.hip), split_rows_scaled_kernel and amax_kernel (sparse_conv_v2.hip) on the same values, so
// the bits are the same as from those four passes.
#include "gp_common.h"
#include "gp_gfx950.h"

namespace {

// NI float4 per lane: columns lane * 4 + 256 i, i < NI, cover cin_pad <= 256 NI.  d % 4 == 0, so a lane's four columns lie in the
// feature block [0, d) as a whole or behind it (geometry columns [d, d + dg), then zeros up to cin_pad).
template <int NI>
__global__ void voxel_rows_kernel(const float *__restrict__ f, int64_t ld_f, int d, const float *__restrict__ geo, int64_t ld_geo, int dg,
                                  const int64_t *__restrict__ order, const int64_t *__restrict__ seg, int64_t nv,
                                  const int32_t *__restrict__ row_map, float *__restrict__ x, int64_t ld_x, int cin_pad,
                                  _Float16 *__restrict__ rows, int64_t ld_rows, float *__restrict__ row_inv, unsigned *__restrict__ amax_bits) {
    __shared__ float s_m[4];
    const int lane = gp_lane();
    float gmax = 0.f;                                              // max |x[v, 0:d]| over this wave's voxels
    // (grid stride: the workgroups are few enough that their one atomic each does not queue up on the word -- one per 4 voxels did,
    // at twice the kernel's time; a wave without a voxel only joins the reduction)
    for (int64_t v_ = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; v_ < nv; v_ += ((int64_t)gridDim.x * blockDim.x) >> 6) {
        const int64_t v = __builtin_amdgcn_readfirstlane((int)v_);
        const int64_t b = seg[v], e = seg[v + 1];
        const int64_t orow = row_map ? row_map[v] : v;
        const float den = (float)(e - b < 1 ? 1 : e - b);
        float acc[NI][4];
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[i][k] = 0.f;
        // sums in ascending CSR order, every column on its own
        for (int64_t j = b; j < e; ++j) {
            const int64_t r = order[j];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int c = lane * 4 + 256 * i;
                if (c < d) {
                    const float4 t = *reinterpret_cast<const float4 *>(f + r * ld_f + c);
                    acc[i][0] += t.x; acc[i][1] += t.y; acc[i][2] += t.z; acc[i][3] += t.w;
                } else if (c < d + dg) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c + k < d + dg) acc[i][k] += geo[r * ld_geo + (c + k - d)];
                }
            }
        }
        // one division; the fp32 row; the row's maximum over all cin_pad columns
        float rmax = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = lane * 4 + 256 * i;
            if (c < cin_pad) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[i][k] = acc[i][k] / den;
                *reinterpret_cast<float4 *>(x + orow * ld_x + c) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
                const float m = fmaxf(fmaxf(fabsf(acc[i][0]), fabsf(acc[i][1])), fmaxf(fabsf(acc[i][2]), fabsf(acc[i][3])));
                rmax = fmaxf(rmax, m);
                if (c < d) gmax = fmaxf(gmax, m);
            }
        }
        const float s = gp_pow2_for(gp_wave_max(rmax));
        if (lane == 0) row_inv[orow] = 1.f / s;
        // interleaved operand row: [32-column step][hi 32 | lo 32]
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = lane * 4 + 256 * i;
            if (c < cin_pad) {
                const float sv[4] = {acc[i][0] * s, acc[i][1] * s, acc[i][2] * s, acc[i][3] * s};
                f16x4 h, l;
                gp_split_f16<4>(sv, h, l);
                _Float16 *ph = rows + orow * ld_rows + ((c >> 5) << 6) + (c & 31);
                *reinterpret_cast<f16x4 *>(ph) = h;
                *reinterpret_cast<f16x4 *>(ph + 32) = l;
            }
        }
    }
    if (amax_bits) {                                               // one atomic per workgroup (non-negative floats order like their bits)
        gmax = gp_wave_max(gmax);
        if (lane == 0) s_m[threadIdx.x >> 6] = gmax;
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(amax_bits, __float_as_uint(fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]))));
    }
}

__global__ void voxel_rows_scale_kernel(const unsigned *__restrict__ amax_bits, float *__restrict__ out2) {
    const float s = gp_pow2_for(__uint_as_float(amax_bits[0]));
    out2[0] = s;
    out2[1] = 1.f / s;
}

}  // namespace

extern "C" int gp_voxel_rows_operands(const float *f, int64_t ld_f, int32_t d, const float *geo, int64_t ld_geo, int32_t dg,
                                      const int64_t *order, const int64_t *seg_start, int64_t nv, const int32_t *row_map, float *x,
                                      int64_t ld_x, int32_t cin_pad, void *rows, int64_t ld_rows, float *row_inv_scale, float *scale2,
                                      void *workspace, size_t workspace_bytes, void *stream_) {
    GP_CHECK_ARG(f && geo && order && seg_start && x && rows && row_inv_scale && nv > 0, "gp_voxel_rows_operands: null/empty argument");
    GP_CHECK_ARG(d > 0 && d % 4 == 0 && dg > 0 && cin_pad >= d + dg && cin_pad % 32 == 0 && cin_pad <= 1024,
                 "gp_voxel_rows_operands: d %% 4 == 0, cin_pad %% 32 == 0, d + dg <= cin_pad <= 1024");
    GP_CHECK_ARG(ld_f >= d && ld_f % 4 == 0 && ld_geo >= dg && ld_x >= cin_pad && ld_x % 4 == 0 && ld_rows >= 2 * (int64_t)cin_pad && ld_rows % 4 == 0,
                 "gp_voxel_rows_operands: ld_f and ld_x multiples of 4 that hold a row, ld_rows %% 4 == 0 and >= 2 cin_pad");
    GP_CHECK_ARG((uintptr_t)f % 16 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)rows % 8 == 0, "gp_voxel_rows_operands: f and x 16-byte, rows 8-byte aligned");
    GP_CHECK_ARG(!scale2 || (workspace && workspace_bytes >= 4), "gp_voxel_rows_operands: scale2 needs a workspace of 4 bytes");
    hipStream_t s = gp_stream(stream_);
    unsigned *amax = scale2 ? static_cast<unsigned *>(workspace) : nullptr;
    if (amax) GP_CHECK_HIP(hipMemsetAsync(amax, 0, 4, s));
    const int64_t waves = nv < 16384 ? nv : 16384;                 // (as gp_split_f16_scaled: a wave walks its voxels with the grid's stride)
    const unsigned blocks = (unsigned)((waves * 64 + 255) / 256);
    _Float16 *r16 = static_cast<_Float16 *>(rows);
    switch ((cin_pad + 255) / 256) {
    case 1: voxel_rows_kernel<1><<<blocks, 256, 0, s>>>(f, ld_f, d, geo, ld_geo, dg, order, seg_start, nv, row_map, x, ld_x, cin_pad, r16, ld_rows, row_inv_scale, amax); break;
    case 2: voxel_rows_kernel<2><<<blocks, 256, 0, s>>>(f, ld_f, d, geo, ld_geo, dg, order, seg_start, nv, row_map, x, ld_x, cin_pad, r16, ld_rows, row_inv_scale, amax); break;
    case 3: voxel_rows_kernel<3><<<blocks, 256, 0, s>>>(f, ld_f, d, geo, ld_geo, dg, order, seg_start, nv, row_map, x, ld_x, cin_pad, r16, ld_rows, row_inv_scale, amax); break;
    default: voxel_rows_kernel<4><<<blocks, 256, 0, s>>>(f, ld_f, d, geo, ld_geo, dg, order, seg_start, nv, row_map, x, ld_x, cin_pad, r16, ld_rows, row_inv_scale, amax); break;
    }
    if (scale2) voxel_rows_scale_kernel<<<1, 1, 0, s>>>(amax, scale2);
    GP_CHECK_LAUNCH();
    return GP_OK;
}
