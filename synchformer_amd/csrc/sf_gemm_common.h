// Shared pieces of the bf16 GEMM kernels (sf_gemm.hip, sf_gemm_pp.hip, sf_gemm_w4.hip, sf_gemm_tn_pp.hip): the argument block and the measurement switches.
// The LDS-DMA, wait and barrier primitives are sf_lds_prims.h's, the branch-free buffer-op epilogue tail is sf_gemm_epi.h's (both included here).
#pragma once
#include "sf_common.h"
#include "sf_lds_prims.h"
#include "sf_gemm_epi.h"
#include "../../include/synchformer_hip.h"

#ifndef SF_ABL
#define SF_ABL 0   // tools/ablate_gemm.sh builds throwaway variants with -DSF_ABL=mask; the product build is 0
#endif
#define EPI_LD 68                          // fp32 row stride of the epilogue staging slab (64 cols + pad, 16-B aligned)

struct GemmArgs {
  const bf16_t* A; int64_t lda;
  const bf16_t* W; int64_t ldw;
  const float* bias;
  void* C; int64_t ldc;
  void* C2 = nullptr;  // config 11, GELU epilogue: also write the pre-activation here (same dtype and row stride as C)
  const float* R; int64_t ldr;
  RowMap cmap, rmap;
  int64_t M;
  int N, K;
  uint32_t tiles_n, tiles_total;
  uint32_t nchunk;   // persistent kernel: column tiles per sweep (0 = all)
  int64_t wk;        // persistent kernel: elements between consecutive 64-deep k-tiles of a W row (64 row-major, N * 64 k-tile-major)
  // strided batch (blockIdx.y = b0 * batch_inner + b1): element offsets added to A / W / C per batch index
  int batch_inner;
  int64_t sA0, sA1, sW0, sW1, sC0, sC1;
  uint32_t stagger = 0;   // config 11: the workgroups that own one tile fewer than their XCD's first start this many x ~1.2 us late (SF_PP_STAGGER)
};

// The eight <OUT_BF16, GELU, HAS_RES> instantiations of a launcher template, chosen at run time: f(sf_ic<out_bf16>(), sf_ic<gelu>(), sf_ic<res>()) with a generic
// lambda that names the launcher.  (The order of the eight calls is the order in which the kernels reach the code object: keep it.)
template <class F>
static int sf_gemm_dispatch_epi(bool out_bf16, bool gelu, bool res, F f) {
  constexpr sf_ic<0> n{};
  constexpr sf_ic<1> y{};
  if (out_bf16) {
    if (gelu) return res ? f(y, y, y) : f(y, y, n);
    return res ? f(y, n, y) : f(y, n, n);
  }
  if (gelu) return res ? f(n, y, y) : f(n, y, n);
  return res ? f(n, n, y) : f(n, n, n);
}

// GemmArgs::nchunk of configs 7, 11 and 12: the L2 rule of sf_launch_plan.h for bf16 rows, unless SF_GEMM_NCHUNK overrides it (experiments)
static inline uint32_t sf_gemm_nchunk(int64_t K) {
  static const int env_chunk = sf_env_int("SF_GEMM_NCHUNK", -1);
  return env_chunk >= 0 ? (uint32_t)env_chunk : sf_l2_nchunk(K, 512, 1024);
}

// cache-policy bits of the epilogue's buffer ops (aux operand: bit 0 sc0/glc, bit 1 nt/slc, bit 4 sc1)
// Outputs are written once and the fp32 residual is read once: marked non-temporal (nt) so that they do not evict the weight matrix
// (3.5-4.7 MB against a 4 MB L2 per XCD) and the A panels the other column tiles of the same rows are about to read.  Measured on
// M = 175,728: qkv 891 -> 950 TFLOP/s, fc1+GELU 717 -> 744, proj+residual 563 -> 618 (profiles/r01_gemm_configs.md).
#ifndef SF_EPI_STORE_AUX
#define SF_EPI_STORE_AUX 2
#endif
#ifndef SF_EPI_LOAD_AUX
#define SF_EPI_LOAD_AUX 2
#endif
#ifndef SF_DMA_SPREAD
#define SF_DMA_SPREAD 1   // 1 (measured +1-2.6 %): issue the next stage's LDS-DMA behind the first two MFMA clusters instead of right after the barrier
#endif
#ifndef SF_EPI_WIDE
#define SF_EPI_WIDE 1   // persistent kernel, bf16 output without residual: transposed accumulator blocks + 8-byte slab writes + 16-byte row stores
#endif
#ifndef SF_KROT
#define SF_KROT 0      // (measured neutral on every shape: profiles/r02_gemm_ln.md) persistent kernel: workgroup i of an XCD walks its k-loop starting at k-tile (i * SF_KROT) % nk (0 = every workgroup starts at 0)
#endif
#ifndef SF_A_NT
#define SF_A_NT 0      // 1: stream the A operand (activations) through L2 with the nt hint as well
#endif

// config 11 (sf_gemm_pp.hip): the quadrant-phased persistent 256 x 256 x 64 kernel
bool sf_gemm_pp_supported(const GemmArgs& a);
int sf_gemm_pp_dispatch(const GemmArgs& a, bool out_bf16, bool gelu, bool res, hipStream_t s);
// config 12 (sf_gemm_w4.hip): the same tile on four waves with register-resident fragments (bf16 output, optional GELU, no residual)
bool sf_gemm_r4_supported(const GemmArgs& a);
int sf_gemm_r4_dispatch(const GemmArgs& a, bool gelu, hipStream_t s);
