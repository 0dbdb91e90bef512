// Lifted BATCHED point clouds rendered back into their views (geopurify_amd/sparse.py: render_rows, Rendered.features): per view and
// pixel the row of the front-most visible point of the view's entry -- what models/utils/visualization.py:34-48 paints a view with,
// made exact -- and the gather that turns that index map into channels-last feature maps.
//
// The rule.  A point p of view v's entry is a CANDIDATE of v when project_point of gp_project.h accepts it against the chosen depth
// (none: p_z > 0; the caller's maps; or the maps rd_render of gp_render_depth.h makes from the entry's own points) -- the pairs the
// lifts count in view_count -- and p_z > 0.  A candidate covers the square of side 2 * radius + 1 centred on its pixel, clipped to
// [cut, H - cut) x [cut, W - cut).  A pixel's OWNER is the covering candidate with the smallest p_z (fp64, dot4_blas), the lowest row
// among equal p_z.  Entries never mix.
//
// Why two passes.  A 64-bit atomic cannot hold an fp64 depth and a row together, and rounding p_z to fp32 to pack them changes
// owners.  So: (A) every candidate takes a 64-bit unsigned atomicMin of its p_z bit pattern on every pixel of its footprint in zmin
// (positive doubles order like their bits; p_z > 0 is tested for that reason even where the depth test implies it); a kernel boundary;
// (B) every candidate, re-derived by the same device function and so with the same bits, takes a 32-bit atomicMin of its row on the
// footprint pixels whose zmin bits equal its own.  Only integer minima and integer sums: two calls give the same bits, and so does
// any row order.  A candidate at p_z > 999999 owns nothing, like a point the reference's z-buffer never stores.
//
// Structure: the entry tables (lb_row_table of gp_lift_entries.h); with depth "render", rd_render into the workspace; zmin filled with
// 999999 (rd_fill_kernel) and rows with INT32_MAX (16-byte stores); pass A (which also counts view_count the way lb_counts_kernel
// does); pass B; the finalise kernel (INT32_MAX -> -1, pixel_count by a wave reduction and one integer atomic per wave).  Launch shape
// of A and B: rd_zbuffer_kernel's, blockIdx.y = view, a view's blocks stride the sorted rows of its entry.
//
// Bounds, as render_depth_batched.hip: a view's entry is range-checked before the offset table is read -- a view outside touches
// nothing, its image stays -1 / 999999 and it is counted in status[1]; a row is rendered only when its own batch column names the
// view's entry; a pixel is written only inside the clipped footprint, which lies inside the image for cut >= 0; all offsets 64-bit.
//
// The gather (gp_render_gather): out[p, :] = convert(src[index[rows[p]], :]) or a zero row where rows[p] < 0 (or where an index leaves
// its array: never accessed).  Lane groups of 1 .. 64 lanes per pixel, so a wave handles one pixel of a wide row or several of a
// narrow one; with 64 lanes the owner is wave-uniform.  Rows whose pitches and bases allow it move 4 elements per lane (16-byte
// loads; 16-byte stores of fp32, 8-byte stores of halves) with a scalar tail past the last whole group; any other rows one element.
// Every element is converted once, by gp_cvt of gp_map_elem.h.
#include "gp_map_elem.h"
#include "gp_render_depth.h"

namespace {

constexpr int RR_MAX_RADIUS = 4;
constexpr unsigned RR_FINAL_BLOCKS = 64;                         // blocks of 256 threads per view in the finalise kernel
constexpr int64_t RR_GATHER_BLOCKS = 16384;
enum { RR_DEPTH_NONE = 0, RR_DEPTH_MAPS = 1, RR_DEPTH_RENDER = 2 };

struct RrWork {                                                  // the entry table, the sort's scratch, the rendered depth maps
    LbTable rows;
    char *tmp;
    size_t tmp_bytes;
    double *depth;
    RrWork(GpCarver &cv, int64_t n, int64_t pixels, bool render) : rows(lb_table(cv, n)) {
        tmp_bytes = lb_sort_bytes(n);
        tmp = cv.take<char>(tmp_bytes);
        depth = render ? cv.take<double>((size_t)pixels) : nullptr;
    }
};

// rows i32 [total], 4-byte aligned: INT32_MAX everywhere, four values per store from the first 16-byte boundary on
__global__ void __launch_bounds__(256) rr_fill_kernel(int32_t *__restrict__ rows, int64_t total) {
    int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(rows) & 15)) & 15) >> 2);
    head = head < total ? head : total;
    const int64_t quads = (total - head) >> 2;
    int4 *r4 = reinterpret_cast<int4 *>(rows + head);
    const int4 far4 = make_int4(INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < quads; i += (int64_t)gridDim.x * blockDim.x) r4[i] = far4;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int64_t i = 0; i < head; ++i) rows[i] = INT32_MAX;
        for (int64_t i = head + quads * 4; i < total; ++i) rows[i] = INT32_MAX;
    }
}

// the candidate decision of both passes: the lifts' rule 1 and p_z > 0; its pixel and the bit pattern of its p_z
__device__ __forceinline__ bool rr_candidate(const double *P, const double *M, double fx, double fy, double cx, double cy,
                                             const double *__restrict__ dv, int W, int H, int cut, double tau, long long &ui, long long &vi,
                                             unsigned long long &bits) {
    const bool visible = project_point(P[1], P[2], P[3], M, M + 4, M + 8, fx, fy, cx, cy, dv, W, H, cut, tau, ui, vi);
    const double p2 = dot4_blas(M + 8, P[1], P[2], P[3]);
    bits = (unsigned long long)__double_as_longlong(p2);
    return visible && p2 > 0.0;
}

// blockIdx.y = view; the blocks of a view stride the sorted rows of its entry.  PASS 0: zmin = min p_z bits over the footprints, and
// the candidates counted into view_count; PASS 1: rows = min row over the footprint pixels whose zmin is the candidate's own p_z.
template <int PASS>
__global__ void __launch_bounds__(256) rr_pass_kernel(const double *__restrict__ points, const int32_t *__restrict__ entry_rows,
                                                      const int32_t *__restrict__ entry_off, const int64_t *__restrict__ view_entry,
                                                      const double *__restrict__ w2c, const double *__restrict__ intr,
                                                      const double *__restrict__ depth, int W, int H, int cut, double tau, int radius,
                                                      unsigned long long *zmin, int32_t *__restrict__ rows,
                                                      unsigned long long *__restrict__ view_count, unsigned long long *__restrict__ status,
                                                      int count_bad_views) {
    const int v = blockIdx.y;
    const int64_t e = view_entry[v];
    if ((uint64_t)e >= (uint64_t)LB_MAX_ENTRIES) {                   // (block-uniform) no entry: nothing is touched
        if (PASS == 0 && count_bad_views && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(status + ST_BAD_VIEW, 1ull);
        return;
    }
    const int64_t r0 = entry_off[e], r1 = entry_off[e + 1];
    const double *M = w2c + (int64_t)v * 16, *K = intr + (int64_t)v * 4;
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    const int64_t image = (int64_t)v * W * H;
    const double *dv = depth ? depth + image : nullptr;
    unsigned long long *zv = zmin + image;
    int32_t *rv = rows + image;
    int local = 0;
    for (int64_t i = r0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < r1; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t row = entry_rows[i];
        const double *P = points + (int64_t)row * 4;
        if (lb_entry_of(P[0]) != (int)e) continue;
        long long ui, vi;
        unsigned long long bits;
        if (!rr_candidate(P, M, fx, fy, cx, cy, dv, W, H, cut, tau, ui, vi, bits)) continue;
        ++local;
        // the clipped footprint: (vi, ui) is inside [cut, H - cut) x [cut, W - cut), so neither range is empty
        const long long y0 = vi - radius < cut ? cut : vi - radius, y1 = vi + radius > H - cut - 1 ? H - cut - 1 : vi + radius;
        const long long x0 = ui - radius < cut ? cut : ui - radius, x1 = ui + radius > W - cut - 1 ? W - cut - 1 : ui + radius;
        for (long long y = y0; y <= y1; ++y)
            for (long long x = x0; x <= x1; ++x) {
                if (PASS == 0) atomicMin(zv + (y * W + x), bits);
                else if (zv[y * W + x] == bits) atomicMin(rv + (y * W + x), row);
            }
    }
    if (PASS == 0) {
        local = gp_wave_sum_i(local);
        if (gp_lane() == 0 && local) atomicAdd(view_count + v, (unsigned long long)local);
    }
}

// blockIdx.y = view: INT32_MAX -> -1, the owned pixels counted
__global__ void __launch_bounds__(256) rr_final_kernel(int32_t *__restrict__ rows, int64_t hw, unsigned long long *__restrict__ pixel_count) {
    int32_t *rv = rows + (int64_t)blockIdx.y * hw;
    int local = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < hw; i += (int64_t)gridDim.x * blockDim.x) {
        if (rv[i] == INT32_MAX) rv[i] = -1;
        else ++local;
    }
    local = gp_wave_sum_i(local);
    if (gp_lane() == 0 && local) atomicAdd(pixel_count + blockIdx.y, (unsigned long long)local);
}

// ------------------------------------------------------------------------------------------------ the gather
// Lane groups of 1 << g_shift lanes per pixel; a group's lanes stride the row by (1 << g_shift) * VEC columns.  VEC == 4: every source
// and destination row starts on a boundary of 4 elements (the launch's test on bases and pitches); the columns past the last whole
// group of 4 go one by one.
template <typename TO, int VEC>
__global__ void __launch_bounds__(256) rr_gather_kernel(const int32_t *__restrict__ rows, int64_t npix, const int64_t *__restrict__ index,
                                                        int64_t n_index, const float *__restrict__ src, int64_t nrows, int64_t d,
                                                        int64_t ld_src, TO *__restrict__ out, int64_t ld_out, int g_shift) {
    const int lane = gp_lane(), group = 1 << g_shift, ppw = 64 >> g_shift, sub = lane & (group - 1);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w * ppw < npix; w += nwaves) {
        const int64_t p = w * ppw + (lane >> g_shift);
        if (p >= npix) continue;
        int32_t owner = rows[p];
        if (g_shift == 6) owner = __builtin_amdgcn_readfirstlane(owner);     // one pixel per wave: the owner is wave-uniform
        int64_t r = owner;
        if (index && r >= 0) r = r < n_index ? index[r] : -1;
        const bool own = (uint64_t)r < (uint64_t)nrows;              // ownerless, or an index outside its array: a zero row, nothing read
        const float *s = src + (own ? r : 0) * ld_src;
        TO *o = out + p * ld_out;
        for (int64_t c = (int64_t)sub * VEC; c < d; c += (int64_t)group * VEC) {
            if (VEC > 1 && c + VEC <= d) {
                float x[VEC];
                TO y[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) x[i] = 0.f;
                if (own) gp_load_vec<VEC>(s + c, x);
#pragma unroll
                for (int i = 0; i < VEC; ++i) y[i] = gp_cvt<TO>(x[i]);
                gp_store_vec<VEC>(o + c, y);
            } else {
                for (int64_t i = c; i < d && i < c + VEC; ++i) o[i] = gp_cvt<TO>(own ? s[i] : 0.f);
            }
        }
    }
}

template <typename TO>
int rr_gather(const int32_t *rows, int64_t npix, const int64_t *index, int64_t n_index, const float *src, int64_t nrows, int64_t d,
              int64_t ld_src, void *out_, int64_t ld_out, hipStream_t s) {
    TO *out = static_cast<TO *>(out_);
    const bool wide = d >= 4 && ld_src % 4 == 0 && ld_out % 4 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)out % (4 * sizeof(TO)) == 0;
    const int64_t per_lane = wide ? 4 : 1, groups = (d + per_lane - 1) / per_lane;
    int g_shift = 0;
    while (g_shift < 6 && ((int64_t)1 << g_shift) < groups) ++g_shift;
    const int64_t ppw = 64 >> g_shift, waves = (npix + ppw - 1) / ppw, nb = (waves + 3) / 4;
    const unsigned grid = (unsigned)(nb > RR_GATHER_BLOCKS ? RR_GATHER_BLOCKS : nb);
    if (wide) rr_gather_kernel<TO, 4><<<grid, 256, 0, s>>>(rows, npix, index, n_index, src, nrows, d, ld_src, out, ld_out, g_shift);
    else rr_gather_kernel<TO, 1><<<grid, 256, 0, s>>>(rows, npix, index, n_index, src, nrows, d, ld_src, out, ld_out, g_shift);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

bool rr_sizes_ok(int64_t n, int32_t nviews, int32_t height, int32_t width) {
    return lb_n_ok(n) && lb_nviews_ok(nviews) && height >= 1 && width >= 1;
}

}  // namespace

extern "C" size_t gp_render_rows_workspace_bytes(int64_t n, int32_t nviews, int32_t height, int32_t width, int32_t depth_mode) {
    if (!rr_sizes_ok(n, nviews, height, width) || depth_mode < RR_DEPTH_NONE || depth_mode > RR_DEPTH_RENDER) return 0;
    GpCarver cv(nullptr, 0);
    RrWork k(cv, n, (int64_t)nviews * height * width, depth_mode == RR_DEPTH_RENDER);
    return cv.off;
}

extern "C" int gp_render_rows(const double *points, int64_t n, const int64_t *view_entry, const double *w2c, const double *intrinsics,
                              int32_t nviews, int32_t height, int32_t width, int32_t cut_bound, int32_t depth_mode, const double *depth,
                              double vis_thres, int32_t radius, int32_t *rows, double *zmin, int64_t *view_count, int64_t *pixel_count,
                              int64_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "gp_render_rows";
    GP_CHECK_ARG(points && view_entry && w2c && intrinsics && rows && zmin && view_count && pixel_count && status && workspace,
                 "%s: null argument", who);
    LB_TRY(lb_check_n(who, n));
    LB_TRY(lb_check_nviews(who, nviews));
    LB_TRY(lb_check_image(who, height, width));
    LB_TRY(lb_check_cut(who, cut_bound));
    GP_CHECK_ARG(depth_mode >= RR_DEPTH_NONE && depth_mode <= RR_DEPTH_RENDER, "%s: depth_mode=%d (0 none, 1 maps, 2 render)", who, depth_mode);
    GP_CHECK_ARG((depth_mode == RR_DEPTH_MAPS) == (depth != nullptr), "%s: depth maps go with depth_mode 1 and with no other", who);
    GP_CHECK_ARG(radius >= 0 && radius <= RR_MAX_RADIUS, "%s: radius=%d outside 0..%d", who, radius, RR_MAX_RADIUS);
    GP_CHECK_ARG((reinterpret_cast<uintptr_t>(zmin) & 7) == 0 && (reinterpret_cast<uintptr_t>(rows) & 3) == 0,
                 "%s: depth is not 8-byte aligned or rows not 4-byte aligned", who);
    const int64_t hw = (int64_t)height * width, total = (int64_t)nviews * hw;
    {
        const void *const in[] = {points, view_entry, w2c, intrinsics, depth};
        const size_t in_bytes[] = {(size_t)n * 32, (size_t)nviews * 8, (size_t)nviews * 128, (size_t)nviews * 32, (size_t)total * 8};
        const void *const o[] = {rows, zmin, view_count, pixel_count, status, workspace};
        const size_t o_bytes[] = {(size_t)total * 4, (size_t)total * 8, (size_t)nviews * 8, (size_t)nviews * 8, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver cv(workspace, workspace_bytes);
    RrWork k(cv, n, total, depth_mode == RR_DEPTH_RENDER);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    unsigned long long *vc = reinterpret_cast<unsigned long long *>(view_count), *pc = reinterpret_cast<unsigned long long *>(pixel_count);
    unsigned long long *zm = reinterpret_cast<unsigned long long *>(zmin);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    GP_CHECK_HIP(hipMemsetAsync(view_count, 0, (size_t)nviews * sizeof(int64_t), s));
    GP_CHECK_HIP(hipMemsetAsync(pixel_count, 0, (size_t)nviews * sizeof(int64_t), s));
    LB_TRY(lb_row_table(points, n, k.rows, k.tmp, k.tmp_bytes, st, s));
    if (depth_mode == RR_DEPTH_RENDER) {                             // (counts the bad views: pass A then leaves them alone)
        LB_TRY(rd_render(points, n, k.rows.idx, k.rows.off, view_entry, w2c, intrinsics, nviews, height, width, cut_bound, k.depth, st, s));
        depth = k.depth;
    }
    const int64_t fb = (total / 2 + 255) / 256, rb = (total / 4 + 255) / 256;
    rd_fill_kernel<<<(unsigned)(fb < 1 ? 1 : (fb > RD_FILL_BLOCKS ? RD_FILL_BLOCKS : fb)), 256, 0, s>>>(zmin, total);
    rr_fill_kernel<<<(unsigned)(rb < 1 ? 1 : (rb > RD_FILL_BLOCKS ? RD_FILL_BLOCKS : rb)), 256, 0, s>>>(rows, total);
    const int64_t nb = (n + 255) / 256;
    const dim3 grid(nb < RD_VIEW_BLOCKS ? (unsigned)nb : RD_VIEW_BLOCKS, (unsigned)nviews);
    rr_pass_kernel<0><<<grid, 256, 0, s>>>(points, k.rows.idx, k.rows.off, view_entry, w2c, intrinsics, depth, width, height, cut_bound, vis_thres,
                                           radius, zm, rows, vc, st, depth_mode == RR_DEPTH_RENDER ? 0 : 1);
    rr_pass_kernel<1><<<grid, 256, 0, s>>>(points, k.rows.idx, k.rows.off, view_entry, w2c, intrinsics, depth, width, height, cut_bound, vis_thres,
                                           radius, zm, rows, vc, st, 0);
    const int64_t pb = (hw + 255) / 256;
    rr_final_kernel<<<dim3(pb < RR_FINAL_BLOCKS ? (unsigned)pb : RR_FINAL_BLOCKS, (unsigned)nviews), 256, 0, s>>>(rows, hw, pc);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

extern "C" int gp_render_gather(const int32_t *rows, int64_t npix, const int64_t *index, int64_t n_index, const float *src, int64_t nrows,
                                int64_t d, int64_t ld_src, void *out, int32_t elem_out, int64_t ld_out, void *stream_) {
    const char *who = "gp_render_gather";
    GP_CHECK_ARG(rows && src && out, "%s: null argument", who);
    GP_CHECK_ARG(npix >= 1 && nrows >= 1 && d >= 1, "%s: npix=%lld, nrows=%lld, d=%lld must be >= 1", who, (long long)npix, (long long)nrows,
                 (long long)d);
    GP_CHECK_ARG(ld_src >= d && ld_out >= d, "%s: pitches %lld / %lld below d=%lld", who, (long long)ld_src, (long long)ld_out, (long long)d);
    GP_CHECK_ARG(index ? n_index >= 1 : n_index == 0, "%s: n_index=%lld %s an index", who, (long long)n_index, index ? "with" : "without");
    GP_CHECK_ARG(gp_elem_ok(elem_out), "%s: element type %d (0 fp32, 1 fp16, 2 bf16)", who, elem_out);
    const size_t so = gp_elem_size(elem_out);
    GP_CHECK_ARG((uintptr_t)rows % 4 == 0 && (uintptr_t)index % 8 == 0 && (uintptr_t)src % 4 == 0 && (uintptr_t)out % so == 0,
                 "%s: an array is not aligned to its element", who);
    {
        const void *const in[] = {rows, index, src};
        const size_t in_bytes[] = {(size_t)npix * 4, (size_t)n_index * 8, ((size_t)(nrows - 1) * ld_src + d) * 4};
        const void *const o[] = {out};
        const size_t o_bytes[] = {((size_t)(npix - 1) * ld_out + d) * so};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    hipStream_t s = gp_stream(stream_);
    if (elem_out == GP_ELEM_F32) return rr_gather<float>(rows, npix, index, n_index, src, nrows, d, ld_src, out, ld_out, s);
    if (elem_out == GP_ELEM_F16) return rr_gather<gp_f16>(rows, npix, index, n_index, src, nrows, d, ld_src, out, ld_out, s);
    return rr_gather<gp_bf16>(rows, npix, index, n_index, src, nrows, d, ld_src, out, ld_out, s);
}
