// Device primitives of the hand-scheduled LDS pipelines, shared by every kernel family (GEMM generations, convolution weight gradient, attention, fused
// W-MSA, element-wise row staging): address-space and vector typedefs, LDS-DMA issue (flat-address and buffer-descriptor forms), counted waits, fragment
// reads issued from inline asm and the register ties that hold consumers behind their wait.  These statements ARE the software pipeline -- a divergence
// between two copies is a silent race -- so they exist once, here.  Internal linkage (anonymous namespace) in each translation unit.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_void;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef __attribute__((address_space(3))) float lds_f32;
typedef unsigned long long u64;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((__vector_size__(8 * sizeof(int)))) int i32x8;

// byte address of an LDS object inside the workgroup's allocation (the `v` address operand of the asm reads below)
__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const char*)p;
}

// ---- LDS-DMA: 16 bytes per lane, HBM / L2 -> LDS without VGPR staging ---------------------------------------------------------------------------------
__device__ __forceinline__ void dma16(const void* src, void* lds_dst) {
    __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)lds_dst, 16, 0, 0);
}
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Buffer-descriptor LDS-DMA (buffer_load_dwordx4 ... offen lds).  The resource type and its builtins exist in the device pass only; the host pass, which
// still parses the kernel body to emit its launch stub, sees placeholders.
#if defined(__HIP_DEVICE_COMPILE__)
typedef __amdgpu_buffer_rsrc_t buf_rsrc_t;
__device__ __forceinline__ buf_rsrc_t buf_make(const void* base) {          // 2 GB window, raw (stride 0) addressing, offsets beyond it read zero
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ buf_rsrc_t buf_make_n(const void* base, unsigned bytes) {          // offsets >= bytes read zero
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ void buf_dma16(buf_rsrc_t rs, void* lds_dst, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)lds_dst, 16, voff, soff, 0, 0);
}
#else
struct buf_rsrc_t { int unused; };
__host__ __device__ inline buf_rsrc_t buf_make(const void*) { return buf_rsrc_t{0}; }
__host__ __device__ inline buf_rsrc_t buf_make_n(const void*, unsigned) { return buf_rsrc_t{0}; }
__host__ __device__ inline void buf_dma16(buf_rsrc_t, void*, unsigned, unsigned) {}
#endif

// ---- fragment reads issued only (no wait), counted waits, register ties -------------------------------------------------------------------------------
// N ds_read_b128 at addr + BASE + i * STRIDE, issued only (no wait): outputs are early-clobber so that no destination aliases the address
template <int N, int BASE, int STRIDE> __device__ __forceinline__ void pipe_issue(u32x4 (&f)[N], unsigned addr) {
    static_assert(N == 2 || N == 4, "N");
    if constexpr (N == 4)
        asm volatile("ds_read_b128 %0, %4 offset:%c5\n\tds_read_b128 %1, %4 offset:%c5+%c6\n\tds_read_b128 %2, %4 offset:%c5+%c6*2\n\tds_read_b128 %3, %4 offset:%c5+%c6*3"
                     : "=&v"(f[0]), "=&v"(f[1]), "=&v"(f[2]), "=&v"(f[3]) : "v"(addr), "n"(BASE), "n"(STRIDE) : "memory");
    else
        asm volatile("ds_read_b128 %0, %2 offset:%c3\n\tds_read_b128 %1, %2 offset:%c3+%c4" : "=&v"(f[0]), "=&v"(f[1]) : "v"(addr), "n"(BASE), "n"(STRIDE) : "memory");
}
// transposing reads of NF fragments of a k-major tile (one address register per fragment: the slot swizzle differs per lane; two reads per fragment: K rows
// r and r + 4 of the lane's 8-row block, HO apart), k-step offset KOFF, issued only
template <int NF, int HO, int KOFF> __device__ __forceinline__ void pipe_issue_tr(const unsigned (&a)[NF], u64 (&l)[NF], u64 (&h)[NF]) {
    static_assert(NF == 2 || NF == 4, "NF");
    if constexpr (NF == 4)
        asm volatile("ds_read_b64_tr_b16 %0, %8 offset:%c13\n\tds_read_b64_tr_b16 %1, %8 offset:%c13+%c12\n\t"
                     "ds_read_b64_tr_b16 %2, %9 offset:%c13\n\tds_read_b64_tr_b16 %3, %9 offset:%c13+%c12\n\t"
                     "ds_read_b64_tr_b16 %4, %10 offset:%c13\n\tds_read_b64_tr_b16 %5, %10 offset:%c13+%c12\n\t"
                     "ds_read_b64_tr_b16 %6, %11 offset:%c13\n\tds_read_b64_tr_b16 %7, %11 offset:%c13+%c12"
                     : "=&v"(l[0]), "=&v"(h[0]), "=&v"(l[1]), "=&v"(h[1]), "=&v"(l[2]), "=&v"(h[2]), "=&v"(l[3]), "=&v"(h[3])
                     : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "n"(HO), "n"(KOFF) : "memory");
    else
        asm volatile("ds_read_b64_tr_b16 %0, %4 offset:%c7\n\tds_read_b64_tr_b16 %1, %4 offset:%c7+%c6\n\t"
                     "ds_read_b64_tr_b16 %2, %5 offset:%c7\n\tds_read_b64_tr_b16 %3, %5 offset:%c7+%c6"
                     : "=&v"(l[0]), "=&v"(h[0]), "=&v"(l[1]), "=&v"(h[1]) : "v"(a[0]), "v"(a[1]), "n"(HO), "n"(KOFF) : "memory");
}
template <int CNT> __device__ __forceinline__ void pipe_wait() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(CNT) : "memory"); }
// ties registers to the wait in front of it: consumers of `f` cannot be scheduled above this (empty) statement, which stays behind the wait
template <int N> __device__ __forceinline__ void pipe_tie(u32x4 (&f)[N]) {
    if constexpr (N == 4) asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
    else asm volatile("" : "+v"(f[0]), "+v"(f[1]));
}
template <int N> __device__ __forceinline__ void pipe_tie(u64 (&l)[N], u64 (&h)[N]) {
    if constexpr (N == 4) asm volatile("" : "+v"(l[0]), "+v"(h[0]), "+v"(l[1]), "+v"(h[1]), "+v"(l[2]), "+v"(h[2]), "+v"(l[3]), "+v"(h[3]));
    else asm volatile("" : "+v"(l[0]), "+v"(h[0]), "+v"(l[1]), "+v"(h[1]));
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): indices that stay compile-time constants inside a lambda (a `#pragma unroll` loop over a
// lambda's int parameter left the per-instruction pointer arrays dynamically indexed in the prologue: 64 bytes of scratch per lane)
template <int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (N > 0) {
        static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

}  // namespace
