// The geometry channels of BATCHED point clouds (geopurify_amd/sparse.py: mesh_normals, estimate_normals): the vertex normals the
// reference's loader takes from a scan's mesh (dataset/data_loader_ablation.py:162-163 <- models/utils/dataset_utils.py:198-199 <-
// vertex_normal, models/utils/mapping_util.py:9-29), for the meshes of several entries at once and bit for bit, and for clouds that
// come without faces the direction of least spread over given neighbour lists.
//
// gp_mesh_normals_batched.  All arithmetic in the dtype T of the points (fp32 or fp64), every operation rounded once (the Makefile
// passes -ffp-contract=off; sqrt and / of the language are correctly rounded for both types), in the order numpy takes them:
//   face f = (i0, i1, i2):  a = p[i1] - p[i0], b = p[i2] - p[i0]
//     vec = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0)          np.cross: each product rounded, then the difference
//     length = sqrt((vec0^2 + vec1^2) + vec2^2) + T(1e-8)           np.sum over three elements is (x0 + x1) + x2
//     contribution c = (vec / length) * (length * 0.5)             mapping_util.py:14-15, :21
//   vertex v:  s = 0; s += c[f] for every face f that names v, f ascending, ONCE per face whichever corners name v (:24-25: numpy's
//     nv[face[i]] += nf[i] reads, adds and writes back, so a vertex named twice is written twice with the same sum);
//     normal = s / (sqrt((s0^2 + s1^2) + s2^2) + T(1e-8))           :27-28; a vertex of no face: 0 / 1e-8 = 0
// A face names rows of points; since every face stays inside one entry (checked), and an entry's faces keep their order, the result
// for an entry is what vertex_normal returns on that entry alone with local indices.
//
// The per-vertex order comes from a sort, not from arrival: one (vertex, face) pair per distinct corner, written at position 3 f +
// corner -- so the pairs ascend by face --, the pairs of a repeated corner, of a face with an index outside 0..n-1 and of a face whose
// rows belong to different (or to no) entries under the key n; the library's stable radix sort by vertex; a vertex's list is then the
// run of its key (found by binary search, as lb_offsets_kernel finds an entry's), ascending by face.  One lane per vertex walks its
// run and sums: the order is the definition, so the sum is serial whatever the valence, and nothing is sized by it.  Only integer
// atomics (the status counts).
//
// gp_knn_normals.  Row i, in fp64: the set is i followed by its k listed rows; m = (sum p) / (k + 1); C = sum (p - m)(p - m)^T in list
// order; cyclic Jacobi on C in registers (rotations of (0,1), (0,2), (1,2), at most JACOBI_SWEEPS sweeps, an off-diagonal element below
// 1e-18 of its two diagonal elements is set to zero) gives orthonormal eigenvectors whatever the spectrum: a collinear set, a flat
// lattice patch or a single repeated point end in some unit vector.  The eigenvector of the smallest eigenvalue (the lowest column
// among equals) is normalised in fp64, oriented, rounded to fp32; variation = l0 / ((l0 + l1) + l2), 0 where the sum is not positive.
// One lane per row.  A wave stages the lists of its 64 consecutive rows -- one contiguous block of 64 k indices -- through LDS in
// tiles of KN_TILE columns, read with consecutive lanes on consecutive indices; every index is range-checked on the way in (outside
// 0..n-1: stored as -1, the row is counted in status[0] and returned as zeros, nothing is dereferenced).  Each wave owns its tile, so
// the only synchronisation is the wave's own.
#include "gp_lift_entries.h"

namespace {

enum { MN_FACE_RANGE = 6, MN_FACE_MIXED = 7 };                   // status words beside ST_BAD_BATCH, ST_NONFINITE, ST_TOP_BATCH
constexpr int64_t MN_MAX_FACES = ((1ll << 31) - 1) / 3;         // 3 F pairs are numbered in int32

template <typename T>
__device__ __forceinline__ T mn_sqrt(T x);
template <>
__device__ __forceinline__ float mn_sqrt<float>(float x) { return sqrtf(x); }
template <>
__device__ __forceinline__ double mn_sqrt<double>(double x) { return sqrt(x); }

// sqrt((x0^2 + x1^2) + x2^2) + 1e-8, the constant rounded to T
template <typename T>
__device__ __forceinline__ T mn_length(T x0, T x1, T x2) {
    const T q0 = x0 * x0, q1 = x1 * x1, q2 = x2 * x2;
    return mn_sqrt<T>((q0 + q1) + q2) + (T)1.0e-8;
}

// the rows: finite, a batch index in 0..65535 (the counts and the top batch of lb_row_keys_kernel, without its table)
template <typename T>
__global__ void __launch_bounds__(256) mn_rows_kernel(const T *__restrict__ points, int64_t n, unsigned long long *__restrict__ status) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    bool nonfinite = false, bad = false;
    int b = -1;
    if (r < n) {
        const T *P = points + r * 4;
        const double p0 = (double)P[0], p1 = (double)P[1], p2 = (double)P[2], p3 = (double)P[3];
        nonfinite = !(fabs(p0) < INFINITY && fabs(p1) < INFINITY && fabs(p2) < INFINITY && fabs(p3) < INFINITY);
        b = lb_entry_of(p0);
        bad = b < 0 && fabs(p0) < INFINITY;
    }
    const int nbad = __popcll(__ballot(bad)), nnf = __popcll(__ballot(nonfinite));
    int top = b;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
    if (gp_lane() == 0) {
        if (nbad) atomicAdd(status + ST_BAD_BATCH, (unsigned long long)nbad);
        if (nnf) atomicAdd(status + ST_NONFINITE, (unsigned long long)nnf);
        if (top >= 0) atomicMax(status + ST_TOP_BATCH, (unsigned long long)top);
    }
}

// one lane per face: its contribution and its three (vertex, face) pairs
template <typename T>
__global__ void __launch_bounds__(256) mn_faces_kernel(const T *__restrict__ points, int64_t n, const int64_t *__restrict__ faces, int64_t nf,
                                                       T *__restrict__ contrib, uint32_t *__restrict__ keys, int32_t *__restrict__ vals,
                                                       unsigned long long *__restrict__ status) {
    const int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    bool range = false, mixed = false;
    if (f < nf) {
        const int64_t i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        uint32_t k0 = (uint32_t)n, k1 = (uint32_t)n, k2 = (uint32_t)n;
        T c0 = 0, c1 = 0, c2 = 0;
        range = (uint64_t)i0 >= (uint64_t)n || (uint64_t)i1 >= (uint64_t)n || (uint64_t)i2 >= (uint64_t)n;
        if (!range) {                                               // (only rows inside the array are read)
            const T *P0 = points + i0 * 4, *P1 = points + i1 * 4, *P2 = points + i2 * 4;
            const int e0 = lb_entry_of((double)P0[0]), e1 = lb_entry_of((double)P1[0]), e2 = lb_entry_of((double)P2[0]);
            mixed = e0 < 0 || e1 != e0 || e2 != e0;
            if (!mixed) {
                const T a0 = P1[1] - P0[1], a1 = P1[2] - P0[2], a2 = P1[3] - P0[3];
                const T b0 = P2[1] - P0[1], b1 = P2[2] - P0[2], b2 = P2[3] - P0[3];
                const T m0 = a1 * b2, m1 = a2 * b1, m2 = a2 * b0, m3 = a0 * b2, m4 = a0 * b1, m5 = a1 * b0;
                const T v0 = m0 - m1, v1 = m2 - m3, v2 = m4 - m5;
                const T len = mn_length<T>(v0, v1, v2), area = len * (T)0.5;
                c0 = (v0 / len) * area;
                c1 = (v1 / len) * area;
                c2 = (v2 / len) * area;
                k0 = (uint32_t)i0;
                if (i1 != i0) k1 = (uint32_t)i1;
                if (i2 != i0 && i2 != i1) k2 = (uint32_t)i2;
            }
        }
        contrib[f * 3] = c0;
        contrib[f * 3 + 1] = c1;
        contrib[f * 3 + 2] = c2;
        keys[f * 3] = k0;
        keys[f * 3 + 1] = k1;
        keys[f * 3 + 2] = k2;
        vals[f * 3] = vals[f * 3 + 1] = vals[f * 3 + 2] = (int32_t)f;
    }
    const int nr = __popcll(__ballot(range)), nm = __popcll(__ballot(mixed));
    if (gp_lane() == 0) {
        if (nr) atomicAdd(status + MN_FACE_RANGE, (unsigned long long)nr);
        if (nm) atomicAdd(status + MN_FACE_MIXED, (unsigned long long)nm);
    }
}

// one lane per vertex: the run of its key in the sorted pairs, summed in that order (ascending face), then the unit normal
template <typename T>
__global__ void __launch_bounds__(256) mn_sum_kernel(const uint32_t *__restrict__ keys_sorted, const int32_t *__restrict__ faces_sorted,
                                                     int64_t npairs, const T *__restrict__ contrib, int64_t n, T *__restrict__ normals) {
    const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (v >= n) return;
    int64_t lo = 0, hi = npairs;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys_sorted[mid] < (uint32_t)v) lo = mid + 1;
        else hi = mid;
    }
    T s0 = 0, s1 = 0, s2 = 0;
    for (int64_t i = lo; i < npairs && keys_sorted[i] == (uint32_t)v; ++i) {
        const T *c = contrib + (int64_t)faces_sorted[i] * 3;
        s0 = s0 + c[0];
        s1 = s1 + c[1];
        s2 = s2 + c[2];
    }
    const T len = mn_length<T>(s0, s1, s2);
    normals[v * 3] = s0 / len;
    normals[v * 3 + 1] = s1 / len;
    normals[v * 3 + 2] = s2 / len;
}

inline int mn_key_bits(int64_t n) {                                  // keys 0 .. n
    int bits = 1;
    while (bits < 32 && (n >> bits) != 0) ++bits;
    return bits;
}

size_t mn_sort_bytes(int64_t npairs, int bits) {
    size_t t = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (size_t)npairs, 0,
                                    bits, 0);
    return t;
}

struct MnWork {                                                  // the pairs before and after the sort, the contributions, the sort's scratch
    uint32_t *k0, *k1;
    int32_t *f0, *f1;
    void *contrib;
    char *tmp;
    size_t tmp_bytes;
    MnWork(GpCarver &cv, int64_t n, int64_t nf, size_t elem) {
        const int64_t npairs = nf * 3;
        k0 = cv.take<uint32_t>(npairs);
        k1 = cv.take<uint32_t>(npairs);
        f0 = cv.take<int32_t>(npairs);
        f1 = cv.take<int32_t>(npairs);
        contrib = cv.take<char>((size_t)npairs * elem);
        tmp_bytes = mn_sort_bytes(npairs, mn_key_bits(n));
        tmp = cv.take<char>(tmp_bytes);
    }
};

template <typename T>
int mn_run(const T *points, int64_t n, const int64_t *faces, int64_t nf, T *normals, unsigned long long *st, const MnWork &k, hipStream_t s) {
    const int64_t npairs = nf * 3;
    T *contrib = static_cast<T *>(k.contrib);
    mn_rows_kernel<T><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(points, n, st);
    mn_faces_kernel<T><<<(unsigned)((nf + 255) / 256), 256, 0, s>>>(points, n, faces, nf, contrib, k.k0, k.f0, st);
    GP_CHECK_LAUNCH();
    size_t io = k.tmp_bytes;
    GP_CHECK_HIP(rocprim::radix_sort_pairs(k.tmp, io, k.k0, k.k1, k.f0, k.f1, (size_t)npairs, 0, mn_key_bits(n), s));
    mn_sum_kernel<T><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(k.k1, k.f1, npairs, contrib, n, normals);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

// ------------------------------------------------------------------------------------------------ normals from neighbour lists
constexpr int KN_TILE = 32;                                      // list columns per LDS tile
constexpr int KN_PITCH = KN_TILE + 1;                            // words per tile row: lanes reading one column fall on 64 different banks
constexpr int KN_WAVES = 4;
constexpr int JACOBI_SWEEPS = 12;
enum { KN_BAD_LIST = 0, KN_BAD_TOWARD = 1, KN_WORDS = 2 };

// one Jacobi rotation that annihilates a_pq; r is the third index: a_rp, a_rq its row, (v0p, v0q) .. (v2p, v2q) the columns p and q of V
__device__ __forceinline__ void kn_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q, double &v1p,
                                          double &v1q, double &v2p, double &v2q) {
    if (apq == 0.0) return;
    if (fabs(apq) <= 1e-18 * (fabs(app) + fabs(aqq))) {
        apq = 0.0;
        return;
    }
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    double x = v0p, y = v0q;
    v0p = c * x - s * y;
    v0q = s * x + c * y;
    x = v1p, y = v1q;
    v1p = c * x - s * y;
    v1q = s * x + c * y;
    x = v2p, y = v2q;
    v2p = c * x - s * y;
    v2q = s * x + c * y;
}

template <typename T, typename I>
__global__ void __launch_bounds__(64 * KN_WAVES) kn_kernel(const T *__restrict__ pos, int64_t ld, int64_t n, const I *__restrict__ nbr, int k,
                                                           const double *__restrict__ toward, int64_t m, const int64_t *__restrict__ toward_rows,
                                                           float *__restrict__ normals, float *__restrict__ variation,
                                                           unsigned long long *__restrict__ status) {
    __shared__ int32_t tiles[KN_WAVES][64 * KN_PITCH];
    const int lane = gp_lane(), wave = threadIdx.x >> 6;
    int32_t *tile = tiles[wave];
    const int64_t row0 = ((int64_t)blockIdx.x * KN_WAVES + wave) * 64;
    if (row0 >= n) return;                                           // (wave-uniform; the kernel has no block-wide barrier)
    const int64_t i = row0 + lane;
    const bool live = i < n;
    const int64_t rows_here = n - row0 < 64 ? n - row0 : 64;
    double px = 0, py = 0, pz = 0;
    if (live) {
        const T *P = pos + i * ld;
        px = (double)P[0], py = (double)P[1], pz = (double)P[2];
    }
    bool bad = false;
    double sx = px, sy = py, sz = pz, mx = 0, my = 0, mz = 0;
    double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            const double cnt = (double)(k + 1);
            mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
            const double dx = px - mx, dy = py - my, dz = pz - mz;
            c00 = dx * dx, c01 = dx * dy, c02 = dx * dz, c11 = dy * dy, c12 = dy * dz, c22 = dz * dz;
        }
        for (int col0 = 0; col0 < k; col0 += KN_TILE) {
            const int kc = k - col0 < KN_TILE ? k - col0 : KN_TILE;
            if (pass == 0 || k > KN_TILE) {                          // (a list of one tile stays in LDS for the second pass)
                gp_wave_sync();
                const int count = (int)rows_here * kc;
                for (int e = lane; e < count; e += 64) {
                    const int r = e / kc, c = e - r * kc;
                    const int64_t j = (int64_t)nbr[(row0 + r) * k + col0 + c];
                    tile[r * KN_PITCH + c] = (uint64_t)j < (uint64_t)n ? (int32_t)j : -1;
                }
                gp_wave_sync();
            }
            if (live) {
                for (int c = 0; c < kc; ++c) {
                    const int32_t j = tile[lane * KN_PITCH + c];
                    if (j < 0) {
                        bad = true;
                        continue;
                    }
                    const T *Q = pos + (int64_t)j * ld;
                    const double qx = (double)Q[0], qy = (double)Q[1], qz = (double)Q[2];
                    if (pass == 0) {
                        sx += qx, sy += qy, sz += qz;
                    } else {
                        const double dx = qx - mx, dy = qy - my, dz = qz - mz;
                        c00 += dx * dx, c01 += dx * dy, c02 += dx * dz, c11 += dy * dy, c12 += dy * dz, c22 += dz * dz;
                    }
                }
            }
        }
    }
    double tx = 0, ty = 0, tz = 0;
    bool bad_toward = false;
    if (live && toward) {
        const int64_t tr = toward_rows[i];
        bad_toward = (uint64_t)tr >= (uint64_t)m;
        if (!bad_toward) tx = toward[tr * 3] - px, ty = toward[tr * 3 + 1] - py, tz = toward[tr * 3 + 2] - pz;
    }
    const int nbad = __popcll(__ballot(live && bad)), nbt = __popcll(__ballot(live && bad_toward));
    if (lane == 0) {
        if (nbad) atomicAdd(status + KN_BAD_LIST, (unsigned long long)nbad);
        if (nbt) atomicAdd(status + KN_BAD_TOWARD, (unsigned long long)nbt);
    }
    if (!live) return;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, var = 0.f;
    if (!bad && !bad_toward) {
        double a00 = c00, a01 = c01, a02 = c02, a11 = c11, a12 = c12, a22 = c22;
        double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
        for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
            if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
            kn_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);       // (p, q, r) = (0, 1, 2)
            kn_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);       // (0, 2, 1)
            kn_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);       // (1, 2, 0)
        }
        // the smallest eigenvalue, the lowest column among equals; the other two for the variation
        double l0 = a00, e0 = v00, e1 = v10, e2 = v20, la = a11, lb = a22;
        if (a11 < l0) l0 = a11, e0 = v01, e1 = v11, e2 = v21, la = a00, lb = a22;
        if (a22 < l0) l0 = a22, e0 = v02, e1 = v12, e2 = v22, la = a00, lb = a11;
        const double lmid = la < lb ? la : lb, lmax = la < lb ? lb : la;
        const double norm = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
        if (norm > 0.0 && norm < INFINITY) e0 /= norm, e1 /= norm, e2 /= norm;
        else e0 = 1.0, e1 = 0.0, e2 = 0.0;
        const double lpos = l0 > 0.0 ? l0 : 0.0, total = (lpos + lmid) + lmax;
        var = total > 0.0 ? (float)(lpos / total) : 0.f;
        o0 = (float)e0, o1 = (float)e1, o2 = (float)e2;
        bool flip;
        if (toward) {
            flip = (e0 * tx + e1 * ty) + e2 * tz < 0.0;
        } else {                                                     // the component of largest magnitude, the lowest axis among equals
            const float m0 = fabsf(o0), m1 = fabsf(o1), m2 = fabsf(o2);
            float lead = o0, mag = m0;
            if (m1 > mag) lead = o1, mag = m1;
            if (m2 > mag) lead = o2, mag = m2;
            flip = lead < 0.f;
        }
        if (flip) o0 = -o0, o1 = -o1, o2 = -o2;
    }
    normals[i * 3] = o0;
    normals[i * 3 + 1] = o1;
    normals[i * 3 + 2] = o2;
    variation[i] = var;
}

template <typename T, typename I>
int kn_run(const void *pos, int64_t ld, int64_t n, const void *nbr, int k, const double *toward, int64_t m, const int64_t *toward_rows,
           float *normals, float *variation, unsigned long long *st, hipStream_t s) {
    const int64_t rows_per_block = 64 * KN_WAVES;
    kn_kernel<T, I><<<(unsigned)((n + rows_per_block - 1) / rows_per_block), 64 * KN_WAVES, 0, s>>>(
        static_cast<const T *>(pos), ld, n, static_cast<const I *>(nbr), k, toward, m, toward_rows, normals, variation, st);
    GP_CHECK_LAUNCH();
    return GP_OK;
}

inline bool mn_sizes_ok(int64_t n, int64_t nf) { return lb_n_ok(n) && nf >= 1 && nf <= MN_MAX_FACES; }

}  // namespace

extern "C" size_t gp_mesh_normals_batched_workspace_bytes(int64_t n, int64_t nfaces, int32_t fp64) {
    if (!mn_sizes_ok(n, nfaces) || fp64 < 0 || fp64 > 1) return 0;
    GpCarver cv(nullptr, 0);
    MnWork k(cv, n, nfaces, fp64 ? 8 : 4);
    return cv.off;
}

extern "C" int gp_mesh_normals_batched(const void *points, int32_t fp64, int64_t n, const int64_t *faces, int64_t nfaces, void *normals,
                                       int64_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "gp_mesh_normals_batched";
    GP_CHECK_ARG(points && faces && normals && status && workspace, "%s: null argument", who);
    GP_CHECK_ARG(fp64 == 0 || fp64 == 1, "%s: fp64=%d (0: fp32 points and normals, 1: fp64)", who, fp64);
    LB_TRY(lb_check_n(who, n));
    GP_CHECK_ARG(nfaces >= 1 && nfaces <= MN_MAX_FACES, "%s: %lld faces outside 1..%lld", who, (long long)nfaces, (long long)MN_MAX_FACES);
    const size_t elem = fp64 ? 8 : 4;
    GP_CHECK_ARG((uintptr_t)points % elem == 0 && (uintptr_t)normals % elem == 0 && (uintptr_t)faces % 8 == 0 && (uintptr_t)status % 8 == 0,
                 "%s: an array is not aligned to its element", who);
    {
        const void *const in[] = {points, faces};
        const size_t in_bytes[] = {(size_t)n * 4 * elem, (size_t)nfaces * 24};
        const void *const o[] = {normals, status, workspace};
        const size_t o_bytes[] = {(size_t)n * 3 * elem, (size_t)ST_WORDS * 8, workspace_bytes};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    GpCarver cv(workspace, workspace_bytes);
    MnWork k(cv, n, nfaces, elem);
    LB_TRY(lb_check_workspace(who, cv, workspace_bytes));
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, ST_WORDS * sizeof(int64_t), s));
    if (fp64) return mn_run<double>(static_cast<const double *>(points), n, faces, nfaces, static_cast<double *>(normals), st, k, s);
    return mn_run<float>(static_cast<const float *>(points), n, faces, nfaces, static_cast<float *>(normals), st, k, s);
}

extern "C" int gp_knn_normals(const void *positions, int32_t fp64, int64_t ld_positions, int64_t n, const void *neighbors, int32_t index64,
                              int32_t k, const double *toward, int64_t m, const int64_t *toward_rows, float *normals, float *variation,
                              int64_t *status, void *stream_) {
    const char *who = "gp_knn_normals";
    GP_CHECK_ARG(positions && neighbors && normals && variation && status, "%s: null argument", who);
    GP_CHECK_ARG((fp64 == 0 || fp64 == 1) && (index64 == 0 || index64 == 1), "%s: fp64=%d, index64=%d (each 0 or 1)", who, fp64, index64);
    LB_TRY(lb_check_n(who, n));
    GP_CHECK_ARG(k >= 3 && k <= 127, "%s: k=%d outside 3..127", who, k);
    GP_CHECK_ARG(ld_positions >= 3, "%s: ld_positions=%lld below 3", who, (long long)ld_positions);
    GP_CHECK_ARG(toward ? (m >= 1 && toward_rows != nullptr) : (m == 0 && toward_rows == nullptr),
                 "%s: toward [m >= 1, 3] goes with toward_rows [n], and neither without the other (m=%lld)", who, (long long)m);
    const size_t ep = fp64 ? 8 : 4, ei = index64 ? 8 : 4;
    GP_CHECK_ARG((uintptr_t)positions % ep == 0 && (uintptr_t)neighbors % ei == 0 && (uintptr_t)toward % 8 == 0 && (uintptr_t)toward_rows % 8 == 0 &&
                     (uintptr_t)normals % 4 == 0 && (uintptr_t)variation % 4 == 0 && (uintptr_t)status % 8 == 0,
                 "%s: an array is not aligned to its element", who);
    {
        const void *const in[] = {positions, neighbors, toward, toward_rows};
        const size_t in_bytes[] = {((size_t)(n - 1) * ld_positions + 3) * ep, (size_t)n * k * ei, (size_t)m * 24, toward_rows ? (size_t)n * 8 : 0};
        const void *const o[] = {normals, variation, status};
        const size_t o_bytes[] = {(size_t)n * 12, (size_t)n * 4, (size_t)KN_WORDS * 8};
        LB_TRY(lb_no_overlap(who, in, in_bytes, o, o_bytes));
    }
    hipStream_t s = gp_stream(stream_);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(status);
    GP_CHECK_HIP(hipMemsetAsync(status, 0, KN_WORDS * sizeof(int64_t), s));
    if (fp64) {
        if (index64) return kn_run<double, int64_t>(positions, ld_positions, n, neighbors, k, toward, m, toward_rows, normals, variation, st, s);
        return kn_run<double, int32_t>(positions, ld_positions, n, neighbors, k, toward, m, toward_rows, normals, variation, st, s);
    }
    if (index64) return kn_run<float, int64_t>(positions, ld_positions, n, neighbors, k, toward, m, toward_rows, normals, variation, st, s);
    return kn_run<float, int32_t>(positions, ld_positions, n, neighbors, k, toward, m, toward_rows, normals, variation, st, s);
}
