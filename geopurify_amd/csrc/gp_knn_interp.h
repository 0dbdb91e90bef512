// Shared by the interpolation through neighbour lists and its backward (knn_query.hip: ki_kernel; knn_interpolate_grad.hip): what a
// query row's list means -- which slots name a row of values, and with which weight.  One definition, so that the weights the
// backward applies are the forward's own bits and a slot is a reference for both or for neither.
#pragma once
#include "gp_common.h"

namespace {

enum { KI_INVERSE_DISTANCE = 0, KI_NEAREST = 1 };

__device__ __forceinline__ double ki_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The rows of query row q, called by the 64 lanes of a wave together: lane s < slots (1 for KI_NEAREST, else k <= 32) takes slot s.
// -> the row of values that slot names, -1 where the slot is -1, past the slots, or the query row is excused: any_list / any_index
// (wave-uniform) say that some slot holds a list entry outside -1..npoints-1 / an index value outside 0..nrows-1 -- neither is
// dereferenced --, and such a query row names no row at all.  d2: the slot's distance (0 where the entry is -1), when dist2 is given.
__device__ __forceinline__ int64_t ki_list_rows(const int64_t *__restrict__ indices, const double *__restrict__ dist2,
                                                const int64_t *__restrict__ index, int64_t q, int k, int slots, int64_t npoints,
                                                int64_t nrows, double &d2, bool &any_list, bool &any_index) {
    const int lane = gp_lane();
    int64_t row = -1;
    d2 = 0.0;
    bool bad_list = false, bad_index = false;
    if (lane < slots) {
        const int64_t id = indices[q * k + lane];
        if (id != -1) {
            if ((uint64_t)id >= (uint64_t)npoints) bad_list = true;
            else {
                row = index ? index[id] : id;
                if ((uint64_t)row >= (uint64_t)nrows) { bad_index = true; row = -1; }
            }
            if (dist2) d2 = dist2[q * k + lane];
        }
    }
    any_list = __ballot(bad_list) != 0;
    any_index = __ballot(bad_index) != 0;
    return row;
}

// ki_list_rows and the slots' weights: fp64 w_s = 1 / (d^2_s + eps) over the slots that name a row, normalised in fp64 (slots with
// d^2_s + eps == 0 share the weight alone), 1 for the one slot of KI_NEAREST, rounded to fp32 once.  w32 is meaningful where the
// returned row is >= 0.
__device__ __forceinline__ int64_t ki_list_weights(const int64_t *__restrict__ indices, const double *__restrict__ dist2,
                                                   const int64_t *__restrict__ index, int64_t q, int k, int slots, int64_t npoints,
                                                   int64_t nrows, int mode, double eps, float &w32, bool &any_list, bool &any_index) {
    double d2;
    int64_t row = ki_list_rows(indices, dist2, index, q, k, slots, npoints, nrows, d2, any_list, any_index);
    double wt = 0.0;
    if (mode == KI_NEAREST) wt = row >= 0 ? 1.0 : 0.0;
    else {
        const double t = d2 + eps;
        const bool zero = row >= 0 && t == 0.0;
        const bool any_zero = __ballot(zero) != 0;
        const double w0 = row >= 0 ? (any_zero ? (zero ? 1.0 : 0.0) : 1.0 / t) : 0.0;
        const double sum = ki_wave_sum_d(w0);
        wt = sum > 0.0 ? w0 / sum : 0.0;
    }
    if (any_list || any_index) row = -1;                             // a zero row
    w32 = (float)wt;
    return row;
}

}  // namespace
