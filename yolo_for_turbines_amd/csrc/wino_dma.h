// wino_dma.h — device helpers shared by the Winograd GEMM kernels (conv_wino_f32.hip, conv_wino4_f32.hip): LDS-DMA requests
// with a wave-uniform source base, fragment reads, counted waits and a compile-time loop.
#pragma once
#include <type_traits>
#include "common.h"

namespace yolo {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

typedef const __attribute__((address_space(1))) void* wn_gptr;
typedef __attribute__((address_space(3))) void* wn_lptr;
__device__ __forceinline__ void wn_glds16(const void* g, void* l) { __builtin_amdgcn_global_load_lds((wn_gptr)g, (wn_lptr)l, 16, 0, 0); }
// the same request with the source as wave-uniform base (SGPR pair) + 32-bit lane offset, the LDS destination (wave-uniform byte
// address) through M0. Written out because inside the stage loop the compiler's strength reduction turns base + offset back
// into one 64-bit vector add per request.
__device__ __forceinline__ void wn_glds16_s(const void* base_uniform, unsigned lane_off, unsigned lds_addr_uniform) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                 :: "v"(lane_off), "s"(base_uniform), "s"(lds_addr_uniform) : "memory");      // (M0 is written here; the compiler re-loads it before every use of its own)
}
template <int N> __device__ __forceinline__ void wn_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// fragments of one xi: the U row (A operand) and the V row (B operand), channels 2h and 2h + 1 of the stage
template <int OFF>
__device__ __forceinline__ void wn_read2(f32x2& a, f32x2& b, unsigned ua, unsigned va) {
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=&v"(a) : "v"(ua), "n"(OFF));
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=&v"(b) : "v"(va), "n"(OFF));
}

template <int I, int N, class Fn>
__device__ __forceinline__ void wn_for(Fn&& fn) {
    if constexpr (I < N) {
        fn(std::integral_constant<int, I>{});
        wn_for<I + 1, N>(fn);
    }
}

}  // namespace yolo
