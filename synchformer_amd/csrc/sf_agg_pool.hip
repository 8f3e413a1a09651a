// sf_agg_cls_pool: the aggregator layer's attention for its CLS query, pooled in ONE pass over the fp32 residual stream.
//
// Only output row 0 of every aggregator sequence is read (motionformer.py:332), and that row's query comes from the aggregator's CLS token - a parameter.  With
// zn_j the normalised key rows and q_h the constant per-head query, the scores are s_{h,j} = u_h . zn_j + c_h (u_h = scale W_k[h]^T q_h, c_h = scale q_h . b_k[h]) and
// the value side is W_v[h] (sum_j p_{h,j} zn_j) + b_v[h]: neither Q, K nor V of the patch rows has to exist.  This launch reads every token row of X once, applies the
// tower's final norm and the aggregator's norm1 (fp32, the arithmetic of layernorm768_kernel), rounds zn to bf16 (the operand the qkv GEMM used to get), and keeps
// per head a running softmax over the sequence and the weighted sum of zn rows:  G[seq][h][:] = sum_j p_{h,j} zn_j  (12 x 768 per sequence).  G leaves as bf16 hi | lo
// (G[seq][h][0][:] = bf16(G), G[seq][h][1][:] = bf16(G - hi)), the A operand of a K-doubled bf16 GEMM against [W | W]: the old path summed P V in fp32 and rounded
// once after it, and a G rounded to 8 bits BEFORE the value projection costs 1.4 x the old path's error where few keys carry the weight (nothing averages it out).
//
// One 512-thread workgroup per sequence, 16-key chunks (key 0 = the CLS key row zn_cls, keys 1.. = the sequence's tokens); two workgroups share a CU:
//   A  each of the eight waves normalises 2 rows (one row per wave-instruction: lane holds columns i*256 + lane*4 .. +3) and writes them as bf16 into LDS (1552-byte rows);
//      the next chunk's rows are requested before the matrix phases start, so 48 KB of loads per workgroup fly under them
//   B  scores S (16 keys x 16 head slots) = zn x U^T on v_mfma_f32_16x16x32_bf16, the 768-deep contraction split over the eight waves (96 each) and summed in a fixed
//      order through LDS (one score per thread).  U is carried as bf16 hi + lo (two MFMAs into one accumulator): the scores see U at ~16 bits, zn at the bf16 it has anyway
//   C  every wave redoes the (tiny) online softmax for all 12 heads in the A-operand layout of the next product (lane: head l & 15, keys (l >> 4)*4 .. +3): base 2,
//      fp32, masked keys enter as an additive -inf; the denominator sums the bf16-rounded probabilities that the product uses
//   D  acc (16 head slots x 96 columns per wave) = alpha acc + P^T (16 x 16 keys) x zn (16 keys x 96 columns) on v_mfma_f32_16x16x16_bf16; the B fragments (4 keys of
//      one column per lane) come out of the row-major LDS rows through ds_read_b64_tr_b16, as the P V operand of sf_attention.hip does
// Sized by registers: per wave 24 VGPRs of rows in flight, 24 of U fragments and 24 of accumulators leave the two LayerNorms room inside the 128 that four waves per
// SIMD allow (32-key chunks spilled the accumulators around every chunk).
// Deterministic: no atomics, nothing depends on the grid or on n_seq - a sequence's output bits are a function of its own rows only.
#include "sf_common.h"
#include "../../include/synchformer_hip.h"

namespace {

constexpr int AP_D = 768;
constexpr int AP_HEADS = 12;
constexpr int AP_ROWS = 16;                                   // keys per chunk
constexpr int AP_WAVES = 8;                                   // 2 staged rows, 96 contraction columns and 96 output columns per wave
constexpr int AP_WR = AP_ROWS / AP_WAVES, AP_WC = AP_D / AP_WAVES, AP_KS = AP_WC / 32, AP_NT = AP_WC / 16;
constexpr int AP_LD = 776;                                    // bf16 elements per staged row: 1552 B (16-byte aligned rows, 4 dwords of bank shift per row)
constexpr int AP_ZN_BYTES = AP_ROWS * AP_LD * 2;              // 24,832
constexpr int AP_SP_BYTES = AP_WAVES * AP_ROWS * 16 * 4;      // the waves' partial scores, 8,192
constexpr int AP_GB_BYTES = 4 * AP_D * 4;                     // gamma1 | beta1 | gamma2 | beta2, 12,288
constexpr int AP_LDS = AP_ZN_BYTES + AP_SP_BYTES + AP_GB_BYTES + AP_ROWS * 4;   // 45,376 B
constexpr int AP_OUT = 2 * AP_HEADS * AP_D;                   // bf16 elements of a sequence's result: 12 heads x (hi | lo) x 768
static_assert(AP_OUT * 2 <= AP_LDS, "the result is staged over the chunk buffers");

struct AggPoolArgs {
  const float* x; int64_t ldx;
  int64_t seq_rows;
  int row0, n_groups, group_stride, tok_stride, n_tok;
  const float *g1, *b1, *g2, *b2;
  float eps1, eps2;
  const float *u, *c, *zn_cls;
  const uint8_t* key_keep;
  bf16_t* out; int64_t ldo;
};

typedef __attribute__((ext_vector_type(4))) float ap_f32x4;
typedef short ap_s4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) ap_s4 ap_lds_s4;

__device__ __forceinline__ float4 ap_ldg_nt(const float* p) {   // X rows are read by exactly one workgroup, once
  const ap_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const ap_f32x4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}

// Sum over the wave, the same bits in every lane: four DPP adds give every lane its 16-lane row's sum (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror,
// row_mirror), the four row sums are then read as scalars - no ds_bpermute round trips and no lane-address registers (wave_sum's butterfly costs six).
__device__ __forceinline__ float ap_wave_sum(float x) {
  x = sum16_dpp(x);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 48));
  return (r0 + r1) + (r2 + r3);
}

// LayerNorm of AP_WR rows, one per wave-instruction (lane: columns i*256 + lane*4 .. +3), two-pass in registers as layernorm768_kernel (the wave sums in another order).  The rows go through together so
// that a gamma / beta piece read from LDS serves all of them and is dropped again (read per row, the compiler keeps all 24 pieces live).  Rows with on[r] false pass unchanged.
__device__ __forceinline__ void ap_layernorm_rows(float4 (&v)[AP_WR][3], const float* g, const float* b, int lane, float eps, const bool (&on)[AP_WR]) {
  float mean[AP_WR], rstd[AP_WR];
#pragma unroll
  for (int r = 0; r < AP_WR; ++r) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) s += (v[r][i].x + v[r][i].y) + (v[r][i].z + v[r][i].w);
    mean[r] = on[r] ? ap_wave_sum(s) * (1.0f / AP_D) : 0.f;
  }
#pragma unroll
  for (int r = 0; r < AP_WR; ++r) {
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      v[r][i].x -= mean[r]; v[r][i].y -= mean[r]; v[r][i].z -= mean[r]; v[r][i].w -= mean[r];
      q += (v[r][i].x * v[r][i].x + v[r][i].y * v[r][i].y) + (v[r][i].z * v[r][i].z + v[r][i].w * v[r][i].w);
    }
    rstd[r] = rsqrtf(ap_wave_sum(q) * (1.0f / AP_D) + eps);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float4 gg = *reinterpret_cast<const float4*>(g + i * 256 + lane * 4);
    const float4 bb = *reinterpret_cast<const float4*>(b + i * 256 + lane * 4);
#pragma unroll
    for (int r = 0; r < AP_WR; ++r)
      if (on[r]) {
        v[r][i].x = v[r][i].x * rstd[r] * gg.x + bb.x; v[r][i].y = v[r][i].y * rstd[r] * gg.y + bb.y;
        v[r][i].z = v[r][i].z * rstd[r] * gg.z + bb.z; v[r][i].w = v[r][i].w * rstd[r] * gg.w + bb.w;
      }
  }
}

__global__ __launch_bounds__(512, 4) void agg_cls_pool_kernel(AggPoolArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* zn = reinterpret_cast<bf16_t*>(smem);                                          // [16][AP_LD]
  float* sp = reinterpret_cast<float*>(smem + AP_ZN_BYTES);                              // [8 waves][16 keys][16 head slots]
  float* gb = reinterpret_cast<float*>(smem + AP_ZN_BYTES + AP_SP_BYTES);                // [4][768]
  float* sbias = reinterpret_cast<float*>(smem + AP_ZN_BYTES + AP_SP_BYTES + AP_GB_BYTES);   // [16]: 0 for a kept key, -inf for a masked one or a slot past the last key
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                             // scalar: row pointers and the per-row branches stay out of the vector registers
  const int fr = lane & 15, fg = lane >> 4;
  const int64_t sq = blockIdx.x;
  const int g = (int)(sq % p.n_groups);
  const int64_t first = (sq / p.n_groups) * p.seq_rows + p.row0 + (int64_t)g * p.group_stride;   // X row of the sequence's token 0
  const int nk = p.n_tok + 1;                                                            // key 0 is the CLS key
  const int n_chunks = (nk + AP_ROWS - 1) / AP_ROWS;

  for (int i = tid; i < AP_D; i += 64 * AP_WAVES) {
    gb[i] = p.g1[i]; gb[AP_D + i] = p.b1[i]; gb[2 * AP_D + i] = p.g2[i]; gb[3 * AP_D + i] = p.b2[i];
  }

  // B operand of the score product, this wave's 96-deep slice of U^T: lane (fr, fg) holds head slot fr, k = 96 wave + 32 j + 8 fg + 0..7; slots 12..15 are zero
  union Frag { bf16x8 v; uint32_t u[4]; };
  Frag uh[AP_KS], ul[AP_KS];
#pragma unroll
  for (int j = 0; j < AP_KS; ++j) {
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = 0.f;
    if (fr < AP_HEADS) {
      const float* up = p.u + fr * AP_D + AP_WC * wave + 32 * j + 8 * fg;
      const float4 a = *reinterpret_cast<const float4*>(up), b = *reinterpret_cast<const float4*>(up + 4);
      f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t hi = pack_bf2(f[2 * e], f[2 * e + 1]);
      uh[j].u[e] = hi;
      ul[j].u[e] = pack_bf2(f[2 * e] - __uint_as_float(hi << 16), f[2 * e + 1] - __uint_as_float(hi & 0xffff0000u));
    }
  }
  const float c_t = fr < AP_HEADS ? p.c[fr] : 0.f;                                       // thread tid sums the score of key slot tid >> 4, head slot tid & 15 = fr

  // chunk c, slot r holds key c*16 + r; this wave stages slots 2 wave .. +1
  float4 v[AP_WR][3];
  float nb = 0.f;                                                                        // threads 0..15: the score bias of slot tid
  auto request = [&](int c) {
#pragma unroll
    for (int i = 0; i < AP_WR; ++i) {
      const int key = c * AP_ROWS + wave * AP_WR + i;
      if (key >= 1 && key < nk) {
        const float* xr = p.x + (first + (int64_t)(key - 1) * p.tok_stride) * p.ldx + lane * 4;
#pragma unroll
        for (int j = 0; j < 3; ++j) v[i][j] = ap_ldg_nt(xr + j * 256);
      } else if (key == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) v[i][j] = *reinterpret_cast<const float4*>(p.zn_cls + j * 256 + lane * 4);
      } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) v[i][j] = make_float4(0.f, 0.f, 0.f, 0.f);           // P is zero there and must meet finite values
      }
    }
    if (tid < AP_ROWS) {
      const int key = c * AP_ROWS + tid;
      bool keep = key < nk;
      if (keep && key >= 1 && p.key_keep) keep = p.key_keep[first + (int64_t)(key - 1) * p.tok_stride] != 0;   // the CLS key is always kept
      nb = keep ? 0.f : -INFINITY;
    }
  };

  float m_run = -INFINITY, l_run = 0.f;                                                  // head slot fr (the same value in the four lane groups and in all waves)
  f32x4 acc[AP_NT];                                                                      // acc[t][r]: head slot 4 fg + r, column 96 wave + 16 t + fr
#pragma unroll
  for (int t = 0; t < AP_NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  request(0);
  __syncthreads();                                                                       // gamma / beta staged
  for (int c = 0; c < n_chunks; ++c) {
    // ---- A: normalise and stage ----------------------------------------------------------------------
    bool on[AP_WR];
#pragma unroll
    for (int i = 0; i < AP_WR; ++i) { const int key = c * AP_ROWS + wave * AP_WR + i; on[i] = key >= 1 && key < nk; }   // (wave-uniform; the CLS key row arrives normalised)
    ap_layernorm_rows(v, gb, gb + AP_D, lane, p.eps1, on);                                // the tower's final norm (fp32, what the Z buffer held)
    ap_layernorm_rows(v, gb + 2 * AP_D, gb + 3 * AP_D, lane, p.eps2, on);                 // the aggregator's norm1
#pragma unroll
    for (int i = 0; i < AP_WR; ++i) {
      bf16_t* zr = zn + (wave * AP_WR + i) * AP_LD + lane * 4;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        uint2 w; w.x = pack_bf2(v[i][j].x, v[i][j].y); w.y = pack_bf2(v[i][j].z, v[i][j].w);
        *reinterpret_cast<uint2*>(zr + j * 256) = w;
      }
    }
    if (tid < AP_ROWS) sbias[tid] = nb;
    if (c + 1 < n_chunks) request(c + 1);
    __syncthreads();

    // ---- B: partial scores of this wave's 96 columns ---------------------------------------------------
    {
      f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < AP_KS; ++j) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(zn + fr * AP_LD + AP_WC * wave + 32 * j + 8 * fg);
        sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, uh[j].v, sc, 0, 0, 0);
        sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, ul[j].v, sc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) sp[(wave * AP_ROWS + 4 * fg + r) * 16 + fr] = sc[r];       // C layout: column fr, rows 4 fg + r
    }
    __syncthreads();

    // ---- the 16 x 16 scores: one per thread, the eight partials summed in a fixed order, bias and key flag added, in base-2 units; written over wave 0's partial
    // (an element only its own thread reads)
    if (tid < AP_ROWS * 16) {
      float d = 0.f;
#pragma unroll
      for (int w = 0; w < AP_WAVES; ++w) d += sp[w * AP_ROWS * 16 + tid];
      sp[tid] = (d + c_t) * 1.44269504088896f + sbias[tid >> 4];
    }
    __syncthreads();

    // ---- C: online softmax, lane = (head slot fr, keys 4 fg .. +3) --------------------------------------
    float s[4];
    float m_new = m_run;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[e] = sp[(4 * fg + e) * 16 + fr];
      m_new = fmaxf(m_new, s[e]);
    }
    m_new = fmaxf(m_new, __shfl_xor(m_new, 16, 64)); m_new = fmaxf(m_new, __shfl_xor(m_new, 32, 64));   // finite from chunk 0 on: key 0 is never masked
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);                            // chunk 0: exp2(-inf) = 0
    union { bf16x4 v; uint32_t u[2]; } pa;
    float l_add = 0.f;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const uint32_t w = pack_bf2(__builtin_amdgcn_exp2f(s[2 * e] - m_new), __builtin_amdgcn_exp2f(s[2 * e + 1] - m_new));
      pa.u[e] = w;
      l_add += __uint_as_float(w << 16) + __uint_as_float(w & 0xffff0000u);
    }
    l_add += __shfl_xor(l_add, 16, 64); l_add += __shfl_xor(l_add, 32, 64);
    l_run = l_run * alpha + l_add;
    m_run = m_new;

    // ---- D: acc = alpha acc + P^T zn ---------------------------------------------------------------------
    float ar[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ar[r] = __shfl(alpha, 4 * fg + r, 64);                    // lane h (< 16) holds head slot h's factor
    // B fragment of a 16-column tile: keys 4 fg + 0..3 of column fr.  ds_read_b64_tr_b16 transposes a 4 x 16 block inside each 16-lane group (lane i receives element
    // i & 3 of the 8 bytes lanes (i >> 2) + 4 j point at, j = 0..3): pointing lane (fr, fg) at zn[4 fg + (fr >> 2)][16 t + 4 (fr & 3) .. +3] returns zn[4 fg + 0..3][16 t + fr]
    char* zc = smem + ((4 * fg + (fr >> 2)) * AP_LD + AP_WC * wave + 4 * (fr & 3)) * 2;
#pragma unroll
    for (int t = 0; t < AP_NT; ++t) {
      const ap_s4 zb = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ap_lds_s4*)(zc + 32 * t));
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] *= ar[r];
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pa.v, zb, acc[t], 0, 0, 0);
    }
    __syncthreads();                                                                     // zn / sp / sbias are rewritten by the next chunk
  }

  // ---- normalise, stage the 12 x (hi | lo) x 768 bf16 result over the chunk buffers (all dead after the loop's last barrier), store it as whole 16-byte pieces ----
  float li[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) li[r] = 1.0f / __shfl(l_run, 4 * fg + r, 64);
  bf16_t* og = reinterpret_cast<bf16_t*>(smem);                                          // [12][2][768]
  if (fg < 3) {                                                                          // head slots 12..15 are padding
#pragma unroll
    for (int t = 0; t < AP_NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gv = acc[t][r] * li[r];
        const bf16_t hi = f2bf(gv);
        bf16_t* o = og + (4 * fg + r) * 2 * AP_D + AP_WC * wave + 16 * t + fr;
        o[0] = hi;
        o[AP_D] = f2bf(gv - bf2f(hi));
      }
  }
  __syncthreads();
  bf16_t* orow = p.out + sq * p.ldo;
  for (int i = tid; i < AP_OUT / 8; i += 64 * AP_WAVES)
    *reinterpret_cast<uint4*>(orow + i * 8) = *reinterpret_cast<const uint4*>(og + i * 8);
}

}  // namespace

extern "C" int sf_agg_cls_pool(const float* x, int64_t ldx, int64_t n_seq, int64_t seq_rows, int row0, int n_groups, int group_stride, int tok_stride, int n_tok,
                               const float* gamma1, const float* beta1, float eps1, const float* gamma2, const float* beta2, float eps2, const float* u,
                               const float* c, const float* zn_cls, const uint8_t* key_keep, bf16_t* g, int64_t ldg, void* stream) {
  SF_CHECK_ARG(x && gamma1 && beta1 && gamma2 && beta2 && u && c && zn_cls && g, "sf_agg_cls_pool: null pointer");
  SF_CHECK_ARG(ldx >= AP_D && (ldx % 4) == 0 && ldg >= AP_OUT && (ldg % 8) == 0, "sf_agg_cls_pool: ldx must be >= 768 and a multiple of 4, ldg >= 18432 and a multiple of 8");
  SF_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)u % 16) == 0 && ((uintptr_t)zn_cls % 16) == 0,
               "sf_agg_cls_pool: x, g, u and zn_cls must be 16-byte aligned");
  SF_CHECK_ARG(n_seq >= 0 && n_seq < (1ll << 31), "sf_agg_cls_pool: n_seq=%lld out of range", (long long)n_seq);
  SF_CHECK_ARG(n_groups >= 1 && n_tok >= 0 && row0 >= 0 && group_stride >= 0 && tok_stride >= 0 && seq_rows >= 1,
               "sf_agg_cls_pool: bad sequence descriptor (n_groups=%d n_tok=%d row0=%d group_stride=%d tok_stride=%d)", n_groups, n_tok, row0, group_stride, tok_stride);
  SF_CHECK_ARG(n_tok == 0 || (int64_t)row0 + (int64_t)(n_groups - 1) * group_stride + (int64_t)(n_tok - 1) * tok_stride < seq_rows,
               "sf_agg_cls_pool: the descriptor's last token row lies outside its sequence of %lld rows", (long long)seq_rows);
  if (n_seq == 0) return 0;
  AggPoolArgs a;
  a.x = x; a.ldx = ldx; a.seq_rows = seq_rows; a.row0 = row0; a.n_groups = n_groups; a.group_stride = group_stride; a.tok_stride = tok_stride; a.n_tok = n_tok;
  a.g1 = gamma1; a.b1 = beta1; a.g2 = gamma2; a.b2 = beta2; a.eps1 = eps1; a.eps2 = eps2; a.u = u; a.c = c; a.zn_cls = zn_cls; a.key_keep = key_keep;
  a.out = g; a.ldo = ldg;
  if (int rc = sf_prepare_kernel((const void*)agg_cls_pool_kernel, AP_LDS, "sf_agg_cls_pool")) return rc;
  hipLaunchKernelGGL(agg_cls_pool_kernel, dim3((unsigned)n_seq), dim3(64 * AP_WAVES), AP_LDS, (hipStream_t)stream, a);
  SF_LAUNCH_CHECK();
  return 0;
}
