// Device functions shared by the per-scene kernels (voxelize.hip, lift.hip) and the batched lift (lift_batched.hip): the point ->
// pixel mapping with its visibility decision, the z-buffer's decision (voxelize.hip, gp_render_depth.h) and the bilinear tap
// of the LSeg resize.  One definition, so both paths take the same decision and the same bits.
#pragma once
#include "gp_common.h"

__device__ __forceinline__ double dot4_blas(const double *r, double x, double y, double z) {
    // acc = r0*x ; acc = fma(r1,y,acc) ; acc = fma(r2,z,acc) ; acc = fma(r3,1,acc)
    double acc = r[0] * x;
    acc = fma(r[1], y, acc);
    acc = fma(r[2], z, acc);
    acc = fma(r[3], 1.0, acc);
    return acc;
}


// one point through one view: pixel (vi = row, ui = column) and the visibility decision of fusion_util.py:99-147 / :45-82
__device__ __forceinline__ bool project_point(double x, double y, double z, const double *m0, const double *m1, const double *m2,
                                              double fx, double fy, double cx, double cy, const double *__restrict__ depth,
                                              int W, int H, int cut, double tau, long long &ui, long long &vi) {
    double p0 = dot4_blas(m0, x, y, z), p1 = dot4_blas(m1, x, y, z), p2 = dot4_blas(m2, x, y, z);
    double u = (p0 * fx) / p2 + cx;
    double v = (p1 * fy) / p2 + cy;
    double ur = rint(u), vr = rint(v);
    bool finite = (fabs(ur) < 9.0e15) && (fabs(vr) < 9.0e15);      // also false for NaN
    ui = finite ? (long long)ur : -1;
    vi = finite ? (long long)vr : -1;
    bool inside = finite && ui >= cut && vi >= cut && ui < (long long)W - cut && vi < (long long)H - cut;
    if (depth) {
        if (inside) {
            double d = depth[vi * W + ui];
            inside = fabs(d - p2) <= tau * d;
        }
    } else {
        inside = inside && (p2 > 0.0);
    }
    return inside;
}


// one point into the z-buffer of one view (fusion_util.py:126-130, depth given as a str): the pixel it lands in and its camera depth
// p2, true when it projects inside the cut bound with p2 > 0.2 -- the points whose minimum p2 is the pixel's rendered depth
__device__ __forceinline__ bool render_point(double x, double y, double z, const double *m0, const double *m1, const double *m2,
                                             double fx, double fy, double cx, double cy, int W, int H, int cut, long long &ui,
                                             long long &vi, double &p2) {
    double p0 = dot4_blas(m0, x, y, z), p1 = dot4_blas(m1, x, y, z);
    p2 = dot4_blas(m2, x, y, z);
    double u = (p0 * fx) / p2 + cx;
    double v = (p1 * fy) / p2 + cy;
    double ur = rint(u), vr = rint(v);
    bool finite = (fabs(ur) < 9.0e15) && (fabs(vr) < 9.0e15);      // also false for NaN
    ui = finite ? (long long)ur : -1;
    vi = finite ? (long long)vr : -1;
    bool inside = finite && ui >= cut && vi >= cut && ui < (long long)W - cut && vi < (long long)H - cut;
    return inside && p2 > 0.2;
}


// one axis of F.interpolate(bilinear, align_corners=True) at output index i, torch's CPU arithmetic: source = scale*i in fp32,
// lambda clipped to [0,1]
__device__ __forceinline__ void bilinear_tap(float scale, int64_t i, int in_size, int &i0, int &i1, float &w0, float &w1) {
    float real = scale * (float)i;
    int f = (int)floorf(real);
    i0 = f < in_size - 1 ? f : in_size - 1;
    float lam = real - (float)i0;
    lam = lam < 0.f ? 0.f : (lam > 1.f ? 1.f : lam);
    i1 = i0 + 1 < in_size - 1 ? i0 + 1 : in_size - 1;
    w0 = 1.f - lam;
    w1 = lam;
}
