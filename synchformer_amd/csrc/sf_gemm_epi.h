// The branch-free buffer-op epilogue tail of the persistent GEMMs, bf16 (sf_gemm.hip, sf_gemm_pp.hip, sf_gemm_tn_pp.hip) and MXFP8 (sf_gemm_mx.hip) operands
// alike.  Split from sf_gemm_common.h so that the MXFP8 kernels get it without the bf16 argument block.
#pragma once
#include "sf_common.h"
#include "sf_lds_prims.h"

// Tail for one group of NPS x 4 rows x 64 cols per wave (NPS float4 per lane, rows 4 apart): + bias, erf-GELU, + fp32 residual, convert, store.
// Row bounds come for free from the buffer descriptors (num_records = M * ld * esz: rows >= M are dropped by the hardware range check), so there is no
// exec-mask branching and hipcc keeps counted vmcnt waits: stores never wait for earlier stores, and the residual rows of the NEXT group are already in
// flight (loaded before this group's stores were issued).
// OUT: 0 = fp32, 1 = bf16, 2 = MXFP8 (the output is the next MX GEMM's A operand: e4m3 bytes + one E8M0 byte per 32 columns, quantised from the bf16-
// rounded value exactly as sf_quantize_mxfp8 would from a bf16 buffer; a 32-column block = 8 consecutive lanes of the 16-lane row group).
// STORE_AUX / LOAD_AUX: the cache-policy bits of the buffer ops, the caller's own switch (SF_EPI_STORE_AUX, SF_MX_STORE_AUX, ..).
template <int OUT, bool GELU, bool HAS_RES, int NPS, int STORE_AUX>
__device__ __forceinline__ void sf_epi_store(float4 (&v)[NPS], const float4& bias4, const float4 (&res)[NPS], __amdgpu_buffer_rsrc_t rc, uint32_t coff, uint32_t cstep,
                                             __amdgpu_buffer_rsrc_t rsc = __amdgpu_buffer_rsrc_t(), uint32_t sc_off = 0, int rows_left = 0) {
#pragma unroll
  for (int ps = 0; ps < NPS; ++ps) {
    float4 x = v[ps];
    x.x += bias4.x; x.y += bias4.y; x.z += bias4.z; x.w += bias4.w;
    if (GELU) {
      sf_f32x2_t g0 = {x.x, x.y}, g1 = {x.z, x.w};
      gelu_erf4(g0, g1);
      x.x = g0.x; x.y = g0.y; x.z = g1.x; x.w = g1.y;
    }
    if (HAS_RES) { x.x += res[ps].x; x.y += res[ps].y; x.z += res[ps].z; x.w += res[ps].w; }
    if (OUT == 2) {
      const uint32_t p01 = pack_bf2(x.x, x.y), p23 = pack_bf2(x.z, x.w);
      const float f0 = __uint_as_float(p01 << 16), f1 = __uint_as_float(p01 & 0xffff0000u), f2 = __uint_as_float(p23 << 16), f3 = __uint_as_float(p23 & 0xffff0000u);
      float amax = fmaxf(fmaxf(fabsf(f0), fabsf(f1)), fmaxf(fabsf(f2), fabsf(f3)));
      // max over the block's eight lanes on DPP (no LDS traffic): quad_perm [1,0,3,2], quad_perm [2,3,0,1], then row_half_mirror (lane i <-> 7 - i)
      amax = fmaxf(amax, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(amax), 0xB1, 0xF, 0xF, true)));
      amax = fmaxf(amax, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(amax), 0x4E, 0xF, 0xF, true)));
      amax = fmaxf(amax, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(amax), 0x141, 0xF, 0xF, true)));
      int be = sf_mx_be(amax);
      be = be < 1 ? 1 : (be > 254 ? 254 : be);
      const float inv = __uint_as_float((uint32_t)(254 - be) << 23);
      int w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_fmed3f(f0 * inv, 448.f, -448.f), __builtin_amdgcn_fmed3f(f1 * inv, 448.f, -448.f), 0, false);
      w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_fmed3f(f2 * inv, 448.f, -448.f), __builtin_amdgcn_fmed3f(f3 * inv, 448.f, -448.f), w, true);
      __builtin_amdgcn_raw_buffer_store_b32((uint32_t)w, rc, coff + ps * cstep, 0, STORE_AUX);
      // one scale byte per row and 32-column block, from the first lane of the block's eight; every other lane (and rows >= M, which would land in the
      // next plane) gets an out-of-range offset that the buffer range check drops - no exec-mask branch in the store loop
      __builtin_amdgcn_raw_buffer_store_b8((uint8_t)be, rsc, ps * 4 < rows_left ? sc_off + ps * 16 : 0xffffffffu, 0, 0);
    } else if (OUT == 1) {
      u32x2 o; o.x = pack_bf2(x.x, x.y); o.y = pack_bf2(x.z, x.w);
      __builtin_amdgcn_raw_buffer_store_b64(o, rc, coff + ps * cstep, 0, STORE_AUX);
    } else {
      u32x4 o;
      o.x = __float_as_uint(x.x); o.y = __float_as_uint(x.y); o.z = __float_as_uint(x.z); o.w = __float_as_uint(x.w);
      __builtin_amdgcn_raw_buffer_store_b128(o, rc, coff + ps * cstep, 0, STORE_AUX);
    }
  }
}
template <int NPS, int LOAD_AUX>
__device__ __forceinline__ void sf_epi_load_res(float4 (&res)[NPS], __amdgpu_buffer_rsrc_t rr, uint32_t roff, uint32_t rstep) {
#pragma unroll
  for (int ps = 0; ps < NPS; ++ps) {
    const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rr, roff + ps * rstep, 0, LOAD_AUX);
    res[ps] = make_float4(__uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), __uint_as_float(t.w));
  }
}
