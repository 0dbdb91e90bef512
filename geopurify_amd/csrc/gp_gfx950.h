// gfx950 (CDNA4) device primitives shared by the matrix-core kernels: the vector types of the MFMA fragments, one-instruction
// wrappers around LDS-DMA, the LDS reads and the waits that go with them, the in-kernel clocks, and two small routines (LDS bitonic
// sort, fp32 -> f16 hi + lo split).  Device side only; host helpers and the wave reductions are in gp_common.h.
//
// These are the lines where the hardware rules live (cache-policy bits, the "+v" ties that keep a use behind its wait, what a
// "memory" clobber orders), so each exists ONCE: a lesson learned goes here.  Everything is __forceinline__ in an anonymous
// namespace: including the header adds no symbol and no code to a translation unit that does not use it.
// What stays with its kernel: waits whose operand lists mirror that kernel's registers (cs_wait_a, pq_wait_lgkm3, wg_wait4,
// pg_lgkm0), the LDS writes (pg_wr64 / pg_wr128), the 16-byte sc1 store of pool_mfma_cs.hip, and the hand-over of the convolution's
// STAMP twin (sparse_conv_v2.hip), which waits on two counters and times the barrier apart from the wait.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));      // one A or B fragment of v_mfma_f32_16x16x32_f16
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((vector_size(8)));             // what one transposed LDS read returns: half a fragment
typedef float f32x4 __attribute__((ext_vector_type(4)));         // one 16x16 accumulator tile per lane
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
template <typename T, int N>
using gp_vec = T __attribute__((ext_vector_type(N)));             // (for a width that is a template parameter)

// ------------------------------------------------------------------------------------------------ global -> LDS DMA
// 16 (or 4) bytes per lane straight from global memory into LDS, no VGPR round trip.  The LDS destination is a wave-uniform base +
// lane * 16, not a per-lane scatter (the image is lane-linear); the global address IS per lane -- swizzles go through `g`.
// Counted in vmcnt like any vector load, and loads return in order: gp_handover<N> relies on both.
// AUX: the cache-policy bits of the instruction (0 = default; 16 = sc1: served by L2, never by this CU's L1).
// (the builtin wants its size as a literal, not as a template parameter: hence two functions)
template <int AUX = 0>
__device__ __forceinline__ void gp_glds16(const void *g, void *l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                     (__attribute__((address_space(3))) void *)l, 16, 0, AUX);
}
__device__ __forceinline__ void gp_glds4(const void *g, void *l) {      // 64 lanes x 4 B: a wave's row ids
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                     (__attribute__((address_space(3))) void *)l, 4, 0, 0);
}

// ------------------------------------------------------------------------------------------------ LDS reads, hand-counted
// The reads are inline asm because a compiler-visible LDS read would wait for EVERY outstanding LDS-DMA (the compiler cannot see
// that they target other ring slots) and serialise the ring.  The price: the compiler knows nothing of lgkmcnt here, so every
// result must pass through one of the waits below (or a kernel's own) before its first use, tied with "+v".
// `addr` is the LDS byte address, OFF a 16-bit immediate.
// transposed read: from a row-major f16 image, the K-major half fragment (4 of the 8 k values of this lane)
template <int OFF>
__device__ __forceinline__ void gp_lds_tr16(s16x4 &d, uint32_t addr) {
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}
template <int OFF, typename V>
__device__ __forceinline__ void gp_lds_rd128(V &d, uint32_t addr) {
    static_assert(sizeof(V) == 16, "16-byte read");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}
// the same with a "memory" clobber: for LDS that this kernel also WRITES through inline asm (the compiler must keep the read on
// its side of those writes and of their waits; asm volatile alone orders it only against other asm volatile)
template <int OFF, typename V>
__device__ __forceinline__ void gp_lds_rd128_mem(V &d, uint32_t addr) {
    static_assert(sizeof(V) == 16, "16-byte read");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory");
}
// read and wait in one statement: the value is usable on return (a mailbox read, off the hot path)
template <typename V>
__device__ __forceinline__ void gp_lds_rd128_now(V &d, uint32_t addr) {
    static_assert(sizeof(V) == 16, "16-byte read");
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(d) : "v"(addr) : "memory");
}
// two transposed reads (k rows q and q + 4) -> one fragment
__device__ __forceinline__ f16x8 gp_cat(s16x4 a, s16x4 b) {
    typedef short s16x8 __attribute__((vector_size(16)));
    s16x8 v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(f16x8, v);
}
// all but the youngest N LDS operations have landed; ties the fragment registers of a read group (f[block][plane][half]) to the
// wait so that no use moves above it.  lgkmcnt is a 4-bit counter: groups of 8 reads, at most 11 LDS operations outstanding.
template <int N = 0>
__device__ __forceinline__ void gp_wait_frags(s16x4 (&f)[2][2][2]) {
    asm volatile("s_waitcnt lgkmcnt(%[n])"
                 : "+v"(f[0][0][0]), "+v"(f[0][0][1]), "+v"(f[0][1][0]), "+v"(f[0][1][1]), "+v"(f[1][0][0]), "+v"(f[1][0][1]),
                   "+v"(f[1][1][0]), "+v"(f[1][1][1])
                 : [n] "n"(N));
}
// stage hand-over of an LDS-DMA ring: this wave's DMA has landed except the youngest N instructions (those of the later stages),
// then the workgroup barrier -- after it every wave's share of the stage is in LDS and every wave is done reading the slot that is
// refilled next.  The "memory" clobber keeps compiler-visible accesses on their side of it.
template <int N = 0>
__device__ __forceinline__ void gp_handover() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// ------------------------------------------------------------------------------------------------ in-kernel clocks
// tuning aid of the STAMP instantiations.  Scalar READS of a counter, returned through the scalar data cache: hence the lgkmcnt
// wait inside.  gp_clock: shader cycles of this XCD; gp_clock_real: the constant 100 MHz counter, comparable between XCDs.
__device__ __forceinline__ uint64_t gp_clock() {
    uint64_t t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
__device__ __forceinline__ uint64_t gp_clock_real() {
    uint64_t t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

// ------------------------------------------------------------------------------------------------ small routines
// ascending sort of a[0 .. n_pow2) in LDS by the whole workgroup (every thread calls it; pad with INT32_MAX to a power of two)
__device__ __forceinline__ void gp_bitonic_sort_lds(int *a, int n_pow2, int tid, int nthreads) {
    for (int k = 2; k <= n_pow2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n_pow2; i += nthreads) {
                int ixj = i ^ j;
                if (ixj > i) {
                    int x = a[i], y = a[ixj];
                    bool up = (i & k) == 0;
                    if ((x > y) == up) { a[i] = y; a[ixj] = x; }
                }
            }
            __syncthreads();
        }
}

// x = hi + lo in two f16: hi = x rounded to nearest, lo = the rounded remainder, so hi + lo carries 22 bits of x -- as long as lo
// is a NORMAL f16 (|lo| >= 2^-14): callers pre-scale by a power of two (gp_pow2_for, GP_POOL_CS_WSCALE).  The products
// hi*hi + hi*lo + lo*hi in fp32 then give fp32-class accuracy; the dropped lo*lo term is 2^-22 relative.
// Element i of hi / lo, which are two f16 vectors, arrays or pointers (an element of a vector cannot bind to a reference: hence the
// index).  The statement order is that of the loops this replaced; the instruction schedule of the callers follows it.
// Which form a call site uses is not free for the same reason: the epilogues of cs_pool_kernel / cs_chain_kernel and of
// pool_mfma_persist_kernel keep their instructions only with this element form inside their own unrolled loop (not with the N-wide
// form below), weight_split_kernel and embed_head_kernel only with the reference form.  scripts/isa_compare.py tells.
template <typename H, typename I>
__device__ __forceinline__ void gp_split_f16(float x, H &hi, H &lo, I i) {
    const _Float16 h = (_Float16)x;
    hi[i] = h;
    lo[i] = (_Float16)(x - (float)h);
}
__device__ __forceinline__ void gp_split_f16(float x, _Float16 &hi, _Float16 &lo) {
    _Float16 *ph = &hi, *pl = &lo;
    gp_split_f16(x, ph, pl, 0);
}
// N elements: x is anything indexable that yields float (array, f32x4, float4)
template <int N, typename X, typename H>
__device__ __forceinline__ void gp_split_f16(const X &x, H &hi, H &lo) {
#pragma unroll
    for (int i = 0; i < N; ++i) gp_split_f16(x[i], hi, lo, i);
}
// two float4 -> one fragment's worth
__device__ __forceinline__ void gp_split8_f16(const float4 &u, const float4 &v, f16x8 &hi, f16x8 &lo) {
    const float x[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
    gp_split_f16<8>(x, hi, lo);
}

}  // namespace
