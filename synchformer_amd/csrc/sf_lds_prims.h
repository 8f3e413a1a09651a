// The LDS-DMA, wait and barrier primitives of every hand-scheduled kernel (gfx950): ONE definition of each distinct instruction sequence.  Every function is
// __forceinline__, so none of these names reaches a code object; where two forms of one primitive exist, the kernels' device assembly differs between them
// (profiles/lds_prims_refactor.md has the comparison) and the comment names which kernels use which.  The rules, once:
//
//   * LDS-DMA loads are INLINE ASM.  hipcc neither counts these loads nor guards later ds_reads with vmcnt(0) (it does for the builtin once the loop gets
//     complicated - that wait serialised prefetch and compute in the first persistent kernel).  Every wait for them is a hand-placed counted s_waitcnt.
//   * The waits are the BUILTIN (gfx9 encoding: vmcnt[3:0] | expcnt << 4 | lgkmcnt << 8 | vmcnt[5:4] << 14, the other counters left at their maximum), so
//     that hipcc's waitcnt pass sees them and stops inserting its own conservative vmcnt(0) in the loop.
//   * M0 holds the wave-uniform LDS destination of a piece (64 lanes x 16 B = 1 KiB, lane-linear; the dword forms: 64 x 4 B = 256 B).  It is saved and
//     restored inside the asm statement: the compiler does not know that the statement writes it.
//   * An s_nop stands behind every M0 write, in front of the load that reads M0.  `s_nop 0` everywhere, except behind the FIRST M0 write of the two-piece
//     and SGPR-base dword forms of the quadrant-phased kernels, which has `s_nop 3`; the round-2 MXFP8 kernel keeps `s_nop 0` there.  Both are kept as
//     they were measured - a count is part of the instruction sequence, not a detail of this header.
//   * s_barrier stands between two empty asm statements: compiler memory fences (the raw s_barrier builtin alone does not order LDS accesses for the
//     compiler).  It is the RAW barrier: __syncthreads() would also drain the stores in flight.
//   * The lane index is re-derived where it is needed (mbcnt over an opaque zero: neither hoisted nor kept): at 256 registers a thread id kept live across
//     the k-loop or the tile loop is spilled, and its reload sits behind a compiler vmcnt(0) - i.e. behind the whole operand stream (or the epilogue's
//     stores) in flight.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

template <int V> using sf_ic = std::integral_constant<int, V>;   // the constant argument of an unrolled lambda

// ---- waits and barriers ------------------------------------------------------------------------------------------------------------------------------
#define SF_WAITCNT_VM(N) (((N) & 0xF) | (0x7 << 4) | (0xF << 8) | (((N) >> 4) << 14))

// counted wait for this wave's own vector-memory operations (LDS-DMA pieces and whatever else it issued), behind a compiler fence
template <int N>
__device__ __forceinline__ void sf_wait_vmcnt() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(SF_WAITCNT_VM(N));
}
// the same without the fence: sf_gemm_pp.hip, sf_gemm_w4.hip, sf_gemm_tn_pp.hip (the fence changes their schedule: their assembly differs with it)
template <int N>
__device__ __forceinline__ void sf_wait_vmcnt_nofence() {
  __builtin_amdgcn_s_waitcnt(SF_WAITCNT_VM(N));
}
__device__ __forceinline__ void sf_wait_lgkm0() {               // the builtin (not asm): hipcc's own counter tracking sees it
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xF | (0x7 << 4) | (0x0 << 8) | (0x3 << 14));
}
__device__ __forceinline__ void sf_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// counted wait for this wave's own LDS-DMA pieces, then the workgroup barrier
template <int N>
__device__ __forceinline__ void sf_wait_vmcnt_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(SF_WAITCNT_VM(N));
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// this wave's LDS writes retired (an asm wait, which is its own fence), then the workgroup barrier: the epilogue passes of sf_gemm_ln.hip / sf_gemm_ln_mx.hip
__device__ __forceinline__ void sf_lgkm0_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// wave-level ordering of LDS accesses (a wave's own slab): no instruction, fences for the compiler
#define SF_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// ---- small helpers -----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sf_lds_addr(const void* p) {   // LDS byte address of a __shared__ pointer
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)p;
}
__device__ __forceinline__ int sf_lane() {                      // the opaque-zero lane id (rules above)
  int z = 0;
  asm volatile("" : "+v"(z));
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
}
// the same as one asm statement, which the compiler can neither hoist nor fold: sf_gemm_w4.hip (nothing lane-derived stays live across its k-loop or epilogue)
__device__ __forceinline__ int sf_lane_asm() {
  int ln;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
  return ln;
}

// ---- LDS-DMA -------------------------------------------------------------------------------------------------------------------------------------------
// POL is the cache-policy suffix of the load ("" | " nt" | " sc1" | " sc0 sc1"), NOP the count behind the first M0 write: one asm body per form.

// One piece: SGPR base + zero-extended 32-bit lane byte offset (operands below 4 GiB) -> 1 KiB at the wave-uniform LDS byte address `lds`.
#define SF_DEF_DMA1(NAME, POL)                                                                                                        \
  __device__ __forceinline__ void NAME(uint32_t voff, const void* sbase, uint32_t lds) {                                              \
    uint32_t keep;                                                                                                                    \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" POL "\n\ts_mov_b32 m0, %0"       \
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds) : "memory");                                                         \
  }
SF_DEF_DMA1(sf_dma1, "")
SF_DEF_DMA1(sf_dma1_nt, " nt")      // read once: streamed through L2

// One dword per lane (64 lanes x 4 B -> 256 consecutive bytes of LDS), SGPR base + lane offset.  `s_nop 3`: sf_gemm_mx.hip (quadrant-phased kernel),
// sf_gemm_ln_mx.hip - the only users of this form.
__device__ __forceinline__ void sf_dma_dword(uint32_t v0, const void* sbase, uint32_t l0) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 3\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(v0), "s"(sbase), "s"(l0) : "memory");
}
// The same from 64-bit lane addresses (a bias row, keep flags); inactive lanes write nothing.  `s_nop 0`: sf_gemm_pp.hip, sf_gemm_w4.hip, sf_gemm_ln2.hip,
// sf_qkv_tile.h, sf_qkv_time.hip.
__device__ __forceinline__ void sf_dma_dword_addr(const void* gaddr, uint32_t lds) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gaddr), "s"(lds) : "memory");
}

// Two pieces (1 KiB each, consecutive in LDS from the wave-uniform byte address l0): SGPR base + 32-bit lane offsets.
#define SF_DEF_DMA2(NAME, NOP, POL)                                                                                                   \
  __device__ __forceinline__ void NAME(uint32_t v0, uint32_t v1, const void* sbase, uint32_t l0) {                                    \
    uint32_t keep;                                                                                                                    \
    asm volatile(                                                                                                                     \
        "s_mov_b32 %0, m0\n\t"                                                                                                        \
        "s_mov_b32 m0, %4\n\ts_nop " NOP "\n\tglobal_load_lds_dwordx4 %1, %3" POL "\n\t"                                              \
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3" POL "\n\t"                                             \
        "s_mov_b32 m0, %0"                                                                                                            \
        : "=&s"(keep)                                                                                                                 \
        : "v"(v0), "v"(v1), "s"(sbase), "s"(l0)                                                                                       \
        : "memory", "scc");                                                                                                           \
  }
SF_DEF_DMA2(sf_dma2, "3", "")       // sf_gemm_pp.hip, sf_gemm_ln.hip, sf_gemm_ln_mx.hip, the quadrant-phased kernel of sf_gemm_mx.hip
SF_DEF_DMA2(sf_dma2_nop0, "0", "")  // the round-2 persistent kernel of sf_gemm_mx.hip

// Four pieces (1 KiB each, consecutive in LDS from the wave-uniform address l0) as SGPR base + zero-extended 32-bit lane offsets (operands below 4 GiB):
// half the address registers per piece (64-bit lane pointers do not fit next to 128 accumulators + the wider MX fragments: they spilled into the k-loop).
#define SF_DEF_DMA4S(NAME, POL)                                                                                                       \
  __device__ __forceinline__ void NAME(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, const void* sbase, uint32_t l0) {          \
    uint32_t keep;                                                                                                                    \
    asm volatile(                                                                                                                     \
        "s_mov_b32 %0, m0\n\t"                                                                                                        \
        "s_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5" POL "\n\t"                                                    \
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %5" POL "\n\t"                                             \
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %5" POL "\n\t"                                             \
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %5" POL "\n\t"                                             \
        "s_mov_b32 m0, %0"                                                                                                            \
        : "=&s"(keep)                                                                                                                 \
        : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(sbase), "s"(l0)                                                                     \
        : "memory", "scc");                                                                                                           \
  }
SF_DEF_DMA4S(sf_dma4s, "")
SF_DEF_DMA4S(sf_dma4s_nt, " nt")    // the fp32 residual (4 rows x 64 columns per piece) into a wave's landing ring: read once

// The same four pieces from 64-bit lane pointers.
#define SF_DEF_DMA4(NAME, POL)                                                                                                        \
  __device__ __forceinline__ void NAME(const void* g0, const void* g1, const void* g2, const void* g3, uint32_t l0) {                 \
    uint32_t keep;                                                                                                                    \
    asm volatile(                                                                                                                     \
        "s_mov_b32 %0, m0\n\t"                                                                                                        \
        "s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" POL "\n\t"                                                   \
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off" POL "\n\t"                                            \
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, off" POL "\n\t"                                            \
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, off" POL "\n\t"                                            \
        "s_mov_b32 m0, %0"                                                                                                            \
        : "=&s"(keep)                                                                                                                 \
        : "v"(g0), "v"(g1), "v"(g2), "v"(g3), "s"(l0)                                                                                 \
        : "memory", "scc");                                                                                                           \
  }
SF_DEF_DMA4(sf_dma4, "")
SF_DEF_DMA4(sf_dma4_nt, " nt")

// One piece through the BUILTIN, which hipcc counts (the ring-of-stages kernel of sf_gemm.hip, whose loop is simple enough for that to cost nothing).
__device__ __forceinline__ void glds16(const void* gsrc, char* lds_dst_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_dst_wave_base, 16, 0, 0);
}
