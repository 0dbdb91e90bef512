// The z-buffer of the BATCHED point clouds, shared by render_depth_batched.hip (the depth maps themselves) and render_rows.hip (which
// renders them into its workspace for depth="render" before it looks for the owners): the fill with 999999, the z-buffer kernel and
// the launch sequence of the two over entry tables that are ready.  One definition, so both take the same decision and the same bits.
#pragma once
#include "gp_lift_stream_state.h"

namespace {

constexpr double RD_FAR = 999999.0;                              // fusion_util.py:127: the depth of a pixel nothing lands in
constexpr unsigned RD_VIEW_BLOCKS = 64;                          // blocks of 256 threads per view: lb_counts_kernel's launch shape
constexpr int64_t RD_FILL_BLOCKS = 16384;

// depth f64 [total], 8-byte aligned: 999999 everywhere, two values per store from the first 16-byte boundary on
__global__ void __launch_bounds__(256) rd_fill_kernel(double *__restrict__ depth, int64_t total) {
    const int64_t head = (reinterpret_cast<uintptr_t>(depth) & 15) ? 1 : 0;
    const int64_t pairs = (total - head) >> 1;
    double2 *d2 = reinterpret_cast<double2 *>(depth + head);
    const double2 far2 = make_double2(RD_FAR, RD_FAR);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < pairs; i += (int64_t)gridDim.x * blockDim.x) d2[i] = far2;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (head) depth[0] = RD_FAR;
        if ((total - head) & 1) depth[total - 1] = RD_FAR;
    }
}

// blockIdx.y = view; the blocks of a view stride the sorted rows of its entry.  entry_rows / entry_off hold values inside 0..n-1 /
// 0..n (the sort's, or ls_tables_kernel's copies).
__global__ void __launch_bounds__(256) rd_zbuffer_kernel(const double *__restrict__ points, const int32_t *__restrict__ entry_rows,
                                                         const int32_t *__restrict__ entry_off, const int64_t *__restrict__ view_entry,
                                                         const double *__restrict__ w2c, const double *__restrict__ intr, int W, int H, int cut,
                                                         double *__restrict__ depth, unsigned long long *__restrict__ status) {
    const int v = blockIdx.y;
    const int64_t e = view_entry[v];
    if ((uint64_t)e >= (uint64_t)LB_MAX_ENTRIES) {                   // (block-uniform) no entry: nothing is touched
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(status + ST_BAD_VIEW, 1ull);
        return;
    }
    const int64_t r0 = entry_off[e], r1 = entry_off[e + 1];
    const double *M = w2c + (int64_t)v * 16, *K = intr + (int64_t)v * 4;
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    unsigned long long *dv = reinterpret_cast<unsigned long long *>(depth + (int64_t)v * W * H);
    for (int64_t i = r0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < r1; i += (int64_t)gridDim.x * blockDim.x) {
        const double *P = points + (int64_t)entry_rows[i] * 4;
        if (lb_entry_of(P[0]) != (int)e) continue;
        long long ui, vi;
        double p2;
        if (!render_point(P[1], P[2], P[3], M, M + 4, M + 8, fx, fy, cx, cy, W, H, cut, ui, vi, p2)) continue;
        // p2 > 0.2: ordered like the doubles.  (A plain load of the pixel that skips the atomic when p2 is not smaller measured 9 %
        // slower at 4 x 150 000 points and 100 views of 240 x 320, DESIGN.md 5.15: every point goes to the atomic.)
        atomicMin(dv + (vi * W + ui), (unsigned long long)__double_as_longlong(p2));
    }
}

// the fill and the z-buffer over tables that are ready (or being made earlier on the stream)
int rd_render(const double *points, int64_t n, const int32_t *entry_rows, const int32_t *entry_off, const int64_t *view_entry,
              const double *w2c, const double *intrinsics, int32_t nviews, int32_t height, int32_t width, int32_t cut_bound, double *depth,
              unsigned long long *status, hipStream_t s) {
    const int64_t total = (int64_t)nviews * height * width, fb = (total / 2 + 255) / 256;
    rd_fill_kernel<<<(unsigned)(fb < 1 ? 1 : (fb > RD_FILL_BLOCKS ? RD_FILL_BLOCKS : fb)), 256, 0, s>>>(depth, total);
    const int64_t nb = (n + 255) / 256;
    rd_zbuffer_kernel<<<dim3(nb < RD_VIEW_BLOCKS ? (unsigned)nb : RD_VIEW_BLOCKS, (unsigned)nviews), 256, 0, s>>>(
        points, entry_rows, entry_off, view_entry, w2c, intrinsics, width, height, cut_bound, depth, status);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

}  // namespace
