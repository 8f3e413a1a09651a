/*
 * synchformer_hip.h - C ABI of libsynchformer_hip.so: the MI355X (gfx950 / CDNA4) kernels behind
 * Synchformer.forward().
 *
 * This is the drop-in boundary of the build.  The reference has no native
 * layer of its own - every op below is reached in the reference through a torch.nn module call; each entry
 * point cites the reference call sites it replaces (paths relative to v-iashin/Synchformer).
 *
 * Conventions
 *   - plain pointers to DEVICE memory + sizes; no torch / HIP types in signatures (`stream` is a hipStream_t
 *     passed as void*; NULL = the null stream).  The caller owns every buffer; nothing here allocates.
 *   - bf16 operands are raw uint16_t bit patterns; accumulation and all statistics are fp32.
 *   - return 0 on success; non-zero = hipError_t of a failed launch, or -1 for a rejected argument.
 *     `sf_last_error()` returns a thread-local human-readable message for the last non-zero return.
 *   - every launcher is asynchronous on `stream` and re-entrant (no global mutable state but the error string).
 *   - "row map": `const int64_t map[6] = {n12, n2, sA, s1, s2, off}` sends logical row r to physical row
 *         (r / n12) * sA + ((r % n12) / n2) * s1 + (r % n2) * s2 + off          (NULL = identity)
 *     which expresses every reshape / CLS-drop / concat / transpose the reference does with view/cat/einops.
 */
#ifndef SYNCHFORMER_HIP_H
#define SYNCHFORMER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SF_F32 = 0, SF_BF16 = 1, SF_F16 = 2, SF_U8 = 3, SF_I16 = 4, SF_I32 = 5 };   /* element types (SF_I16: PCM input of sf_resample_wave / _mix only; SF_I32: of sf_resample_wave_mix only) */
enum { SF_EPI_NONE = 0, SF_EPI_GELU = 1 };                  /* GEMM epilogue activation */

/* 25, with purely additive entries since (additions under v25): sf_ingest_video_v210, sf_ingest_video_v210_fields; sf_track_pairwise,
 * sf_track_pairwise_gated; nothing that existed at 25 changed */
#define SF_ABI_VERSION 25
int sf_abi_version(void);
const char* sf_last_error(void);
/* "gfx950" + build flags; lets the host assert it loaded the library it built */
const char* sf_build_info(void);
/* C[cmap(m), n] = epi(sum_k A[m,k] * W[n,k] + bias[n]) (+ R[rmap(m), n]);  A: M x K bf16 (row stride lda),
 * W: N x K bf16 (an nn.Linear / flattened conv weight, row stride ldw), bias fp32 or NULL, C bf16|fp32,
 * R fp32 or NULL (may alias C for an in-place residual).  K % 64 == 0.  Exact-erf GELU when SF_EPI_GELU.
 * Alignment: A and W 16 bytes, lda / ldw multiples of 8 elements (checked).  C and R need only their element's alignment, EXCEPT when N % 4 == 0 and ldc
 * (and ldr, with a residual) are multiples of 4: the epilogue then moves four columns per access, so C must be 16-byte aligned for fp32 and 8-byte aligned
 * for bf16, R 16-byte aligned (the caller's obligation: the launcher does not check it).  The GELU epilogue needs identity row maps and N % 64 == 0.
 * Replaces nn.Linear at vit_helper.py:103,155,392-396; modeling_ast.py:142-146,199,263,274;
 * modules/transformer.py:59-61,74,86-91; nn.MultiheadAttention in/out proj + linear1/2 at
 * motionformer.py:329; Conv3d vit_helper.py:436-443 and Conv2d modeling_ast.py:113-117 (after sf_im2col_*);
 * vproj/aproj sync_model.py:55-56; off_head/sync_head sync_model.py:172,189. */
int sf_gemm_bf16(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw, const float* bias, void* C,
                 int c_dtype, int64_t ldc, const int64_t* c_map, const float* R, int64_t ldr, const int64_t* r_map,
                 int epilogue, int64_t M, int64_t N, int64_t K, void* stream);

/* Strided-batched small GEMM (train step: attention backward).  For b0 < batch_outer, b1 < batch_inner:
 * C[b0,b1] (M x N) = A[b0,b1] (M x K) * W[b0,b1]^T (N x K) + bias, X[b0,b1] = X + b0*sX0 + b1*sX1 (element strides).
 * K % 32 == 0 (zero-pad the contraction dimension); any M, N; C bf16|fp32.  Backward of the matmuls at
 * modules/transformer.py:67-70. */
int sf_gemm_bf16_batched(const uint16_t* A, int64_t lda, int64_t sA0, int64_t sA1, const uint16_t* W, int64_t ldw, int64_t sW0,
                         int64_t sW1, const float* bias, void* C, int c_dtype, int64_t ldc, int64_t sC0, int64_t sC1, int64_t M,
                         int64_t N, int64_t K, int batch_outer, int batch_inner, void* stream);

/* Split-K weight-gradient product of the train steps (autograd of every nn.Linear on the path: dW = dY^T X, e.g. the qkv / proj / fc1 / fc2
 * layers of vit_helper.py:87-141 and modeling_ast.py:199-330): part[s] (N x K, fp32) = sum over token rows m in chunk s of dY[m,:]^T X[m,:],
 * chunk s = rows [s*kc, min((s+1)*kc, M)).  dY (M x N) and X (M x K) are the row-major bf16 activations as they are - no transposed copies.
 * N % 128 == 0, K % 128 == 0, kc % 64 == 0, split*kc >= M, ldy >= N, ldx >= K (both % 8 == 0); chunks entirely past M give zero
 * partials.  The caller sums the `split` partials (sf_seqsum).
 * bias_part (split x N, fp32) or NULL: the same chunks' column sums of dY - the bias gradient of the layer - from four extra MFMAs against an
 * all-ones fragment in the workgroups that already hold those dY columns; summed by sf_seqsum(bias_part, N, split, 1, N, ...). */
int sf_gemm_tn_splitk(const uint16_t* dY, int64_t ldy, const uint16_t* X, int64_t ldx, float* part, float* bias_part, int64_t M, int64_t N,
                      int64_t K, int split, int64_t kc, void* stream);
/* The same product on the quadrant-phased 256 x 256 x 64 schedule (sf_gemm_tn_pp.hip) for the big weight gradients: N % 256 == 0, K % 256 == 0, kc % 128 == 0,
 * no empty chunk ((split - 1) * kc < M); rows beyond M contribute zero (buffer range check of the LDS-DMA).  bias_part: (split, N) fp32 or NULL - per-chunk
 * column sums of dY (the bias gradient), summed by sf_seqsum(bias_part, N, split, 1, N, ...). */
int sf_gemm_tn_pp(const uint16_t* dY, int64_t ldy, const uint16_t* X, int64_t ldx, float* part, float* bias_part, int64_t M, int64_t N, int64_t K, int split,
                  int64_t kc, void* stream);
/* dW = sum over the `split` chunk planes of `part` (n_w = N * K floats each) and, in the same launch, db (=|+=) the sum of the `split` rows of bias_part (n_b = N
 * floats each; bias_part may be NULL): the reduction behind sf_gemm_tn_splitk / sf_gemm_tn_pp.  n_w % 4 == 0, n_b % 4 == 0, 16-byte aligned. */
int sf_wgrad_sum(const float* part, int64_t n_w, int split, float* dw, const float* bias_part, int64_t n_b, float* db, int accumulate_bias, void* stream);

/* Full-row projection fused with the residual add and the NEXT LayerNorm (N = 768 fixed):
 *   X[m,:] = A[m,:] W^T + bias + R[m,:]  (fp32; X may alias R),   Y[m,:] = LayerNorm(X[m,:]) * gamma + beta  (bf16; Y may alias A).
 * A: M x K bf16, W: 768 x K bf16 (row stride ldw), or - ldw == 32 - the same weight re-laid out k-step-major as [K/32][768][32] so that the 48 KiB
 * slice of every 32-deep k-step is contiguous (full cache lines); K % 32 == 0; R / X / Y below 4 GiB.  One workgroup owns 128 complete rows, so the fp32 residual
 * stream is read once and written once per sub-layer and the separate sf_layernorm768 launch disappears.  Replaces, inside
 * DividedSpaceTimeBlock.forward (vit_helper.py:364-376), `x + temporal_fc/proj(...)` -> norm1, `x + proj(attn(...))` -> norm2 and
 * `x + mlp.fc2(...)` -> the next block's norm3. */
int sf_gemm_res_ln768(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw, const float* bias, const float* R, int64_t ldr,
                      float* X, int64_t ldx, const float* gamma, const float* beta, float eps, uint16_t* Y, int64_t ldy, int64_t M,
                      int64_t K, void* stream);

/* ---- MX-FP8 path of the frozen feature extractors in the synchronizability fine-tune (BASELINE configs[4]; configs/ft_synchability.yaml:7,19:
 * is_trainable False towers; the reference itself has no fp8 - fp16 autocast only, scripts/train_sync.py:178).  OCP Microscaling MXFP8: e4m3
 * elements, one E8M0 scale byte per 32 consecutive k of a row. ---- */
/* q (rows x K bytes, row stride ldq) and scales <- bf16 x (rows x K); K % 128 == 0.  Scales are STAGE-major for the GEMM's loads: plane k/128 (lds
 * BYTES apart, lds >= rows * 4) holds 4 bytes per row = the E8M0 scales of that row's four 32-blocks in the 128-deep stage. */
int sf_quantize_mxfp8(const uint16_t* x, int64_t ldx, uint8_t* q, int64_t ldq, uint8_t* scales, int64_t lds, int64_t rows, int64_t K, void* stream);
/* sf_gemm_bf16's contract (bias, exact-erf GELU, fp32 residual, bf16|fp32 output, identity row maps) on MXFP8 operands: A (M x K) / W (N x K)
 * e4m3 bytes with their stage-major scale planes sA / sW (K/128 planes, ldsa / ldsw bytes apart, 4 bytes per row, the rows of a plane PADDED to whole
 * 256-row tiles: ldsa >= ceil(M/256) * 1024, ldsw >= ceil(N/256) * 1024, 16-byte aligned - a tile's scales of one stage are fetched as one contiguous KiB); K % 128 == 0, N % 64 == 0.  v_mfma_scale_f32_32x32x64_f8f6f4, fp32 accumulate.
 * (Accuracy: that instruction aligns the products of 8 consecutive k to the largest of them and drops what lies below 2^-13 of it before the fp32 accumulation -
 * asserted by tests/test_gemm_gpu.py::test_mxfp8_mfma_group_alignment, bounded by tests/gemm_oracle.py mx_group_term; operands of narrow dynamic range inside a 32-block, the MX use case, are summed exactly.)
 * Replaces the nn.Linear calls at vit_helper.py:103,155,392-396 (qkv / proj / fc1 / fc2 of the DividedSpaceTimeBlocks) when the engine is built
 * with fp8 towers. */
int sf_gemm_mxfp8(const uint8_t* A, int64_t lda, const uint8_t* sA, int64_t ldsa, const uint8_t* W, int64_t ldw, const uint8_t* sW, int64_t ldsw,
                  const float* bias, void* C, int c_dtype, int64_t ldc, uint8_t* sC, int64_t ldsc, const float* R, int64_t ldr, int epilogue, int64_t M,
                  int64_t N, int64_t K, void* stream);
/* c_dtype SF_U8: the output itself leaves as MXFP8 (C = e4m3 bytes, sC / ldsc = its stage-major scale planes) - the fc1 + GELU hidden activations feeding
 * fc2 - quantised from the bf16-rounded value exactly as sf_quantize_mxfp8 would; N % 128 == 0, no residual. */
/* LayerNorm(768) whose output leaves as MXFP8 (the A operand of the qkv / fc1 MX GEMMs): sf_layernorm768 followed by sf_quantize_mxfp8, in one pass. */
int sf_layernorm768_mxfp8(const float* x, int64_t ldx, const float* gamma, const float* beta, uint8_t* q, int64_t ldq, uint8_t* scales, int64_t lds,
                          int64_t rows, float eps, void* stream);
/* sf_gemm_res_ln768 with a PERIODIC residual: X[m,:] = A[m,:] W^T + bias + R[m % period,:], R a table of `period` (>= 64) rows that is not X; everything else
 * as above (the same kernel body, the product schedule, no measurement hooks).  The patch embedding in one launch - Conv3d vit_helper.py:436-443 on the token-layout
 * im2col rows + the position / time tables (video_model_builder.py:248-254; period = 1569 rows per segment) + block 0's norm3 (vit_helper.py:366): the table is
 * read from cache, its broadcast copy is neither written nor read back. */
int sf_gemm_res_ln768_periodic(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw, const float* bias, const float* R, int64_t ldr, int64_t period,
                               float* X, int64_t ldx, const float* gamma, const float* beta, float eps, uint16_t* Y, int64_t ldy, int64_t M, int64_t K,
                               void* stream);

/* sf_gemm_res_ln768 on MXFP8 operands with an MXFP8 output: X = dq(A) dq(W)^T + bias + R (fp32, 768 columns, X may alias R), (Y, sY) = the MXFP8
 * quantisation of bf16(LayerNorm(X) * gamma + beta) - sf_gemm_mxfp8 with the residual epilogue followed by sf_layernorm768_mxfp8, in one launch
 * (`x = x + proj(...)` / `x = x + fc2(...)` and the LayerNorm that opens the next sub-layer, vit_helper.py:364-376, in the fp8 towers).  A (M x K) / W (768 x K)
 * e4m3 bytes, K % 128 == 0; scale planes as for sf_gemm_mxfp8 with ldsa >= ceil(M/128) * 512, ldsw >= 3072, ldsy >= 4 M (6 planes).  Y / sY may alias
 * A / sA when K == 768. */
int sf_gemm_mx_res_ln768(const uint8_t* A, int64_t lda, const uint8_t* sA, int64_t ldsa, const uint8_t* W, int64_t ldw, const uint8_t* sW, int64_t ldsw,
                         const float* bias, const float* R, int64_t ldr, float* X, int64_t ldx, const float* gamma, const float* beta, float eps,
                         uint8_t* Y, int64_t ldy, uint8_t* sY, int64_t ldsy, int64_t M, int64_t K, void* stream);
/* sf_qkv_time_attention on MXFP8 operands (the temporal qkv projection of the fp8 towers with the 8-frame time attention in its epilogue): X (rows, 768) / W (2304, 768)
 * e4m3 bytes with stage-major scale planes (6 planes, one dword per row, ldsx / ldsw bytes apart); qkv_cls / out bf16 and cls_partial fp32 as in
 * sf_qkv_time_attention.  n_groups % 4 == 0, and n_groups >= 28 unless n_seq <= 2 (a 32-patch tile may touch two sequences at the most: fewer patches per sequence
 * are refused; the bf16 form serves them).  Replaces sf_gemm_mxfp8 (bf16 output) + sf_attention (time groups) + sf_attention_cls on the MX path. */
int sf_qkv_time_attention_mx(const uint8_t* X, int64_t ldx, const uint8_t* sX, int64_t ldsx, const uint8_t* W, int64_t ldw, const uint8_t* sW, int64_t ldsw,
                             const float* bias, const uint16_t* qkv_cls, int64_t ldc, uint16_t* out, int64_t ldo, float* cls_partial, int64_t n_seq, int n_groups,
                             float scale, void* stream);
/* ... with the attention output (patch rows) written as MXFP8 instead of bf16: out_q e4m3 bytes (rows, 768), row stride ldq bytes; out_s the scale planes [6][rows][4],
 * splane bytes apart - byte for byte sf_quantize_mxfp8 of sf_qkv_time_attention_mx's bf16 output.  out_q / out_s must not alias X / sX.  The CLS rows come from
 * sf_attention_cls_combine_mx on cls_partial. */
int sf_qkv_time_attention_mx_q(const uint8_t* X, int64_t ldx, const uint8_t* sX, int64_t ldsx, const uint8_t* W, int64_t ldw, const uint8_t* sW, int64_t ldsw,
                               const float* bias, const uint16_t* qkv_cls, int64_t ldc, uint8_t* out_q, int64_t ldq, uint8_t* out_s, int64_t splane,
                               float* cls_partial, int64_t n_seq, int n_groups, float scale, void* stream);

/* Tuning / test hook (state of the CALLING THREAD only; the launchers stay re-entrant): force the GEMM tile configuration of this thread's subsequent
 * sf_gemm_bf16 calls.  -1 = automatic choice by shape (default); 0 = 128x128x64, 4 waves, two workgroups per CU; 7 = persistent 256x256x64,
 * 8 waves, v_mfma_f32_32x32x16_bf16 (round 2's schedule: one 64-KiB stage of prefetch); 11 = the same tile with the quadrant-phased schedule of round 3
 * (half-tile LDS-DMA stream 1.5 stages ahead, counted waits, staggered wave groups: sf_gemm_pp.hip; K %% 128 == 0) - the automatic choice for the big
 * token GEMMs; 10 = 4 waves of 128x128; 1-6, 8, 9 = the other tilings measured in profiles/r01_gemm_configs.md (tools/bench_gemm.py). */
void sf_gemm_force_config(int cfg);
/* The configuration the automatic choice takes for a row-major, identity-mapped GEMM of this shape (0, 7 or 11): bench.py files its live launch timings
 * under the kernel symbol rocprofv3 reports for that configuration. */
int sf_gemm_bf16_auto_config(int64_t M, int64_t N, int64_t K, int has_residual);
/* fc1 of a trained MLP in one launch (Stage-1 towers; vit_helper.py Mlp / modeling_ast.py ASTIntermediate): pre = A W^T + bias and act = gelu(pre), both bf16 with
 * row stride ldc, both kept for the backward.  Returns SF_NOT_APPLICABLE (-2: no hipError_t, no argument error) without launching when the shape is outside
 * config 11's range (K % 128 == 0, K >= 256, N % 64 == 0, M, N >= 256, aligned): the caller then runs sf_gemm_bf16 + sf_gelu_fwd. */
#define SF_NOT_APPLICABLE (-2)
int sf_gemm_bf16_gelu_dual(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw, const float* bias, uint16_t* pre, uint16_t* act, int64_t ldc,
                           int64_t M, int64_t N, int64_t K, void* stream);
/* The same kind of hook for sf_gemm_res_ln768's main-loop schedule: -1 default (quadrant-phased, round 3), 0 = round 2's loop (one stage of prefetch),
 * 1 = quadrant-phased.  Both sum every accumulator in the same order: bit-identical outputs (the tests compare them).
 * 2 = round 4's 192-row tiles in two 384-column passes on the fused spatial kernel's main loop (row-major W, K % 128 == 0, lda and ldw multiples of
 * 64; other operands fall back to schedule 1): X differs from schedules 0/1 only by fp32 summation order, Y by at most one bf16 rounding.  The
 * environment variable SF_RL_SCHED=2 selects it when nothing is forced. */
void sf_gemm_res_ln_force_schedule(int sched);
void sf_qkv_time_force_schedule(int sched);        /* the same for sf_qkv_time_attention */
void sf_gemm_mx_force_schedule(int sched);         /* ... and for sf_gemm_mxfp8 (quadrant-phased needs K % 256 == 0) */

/* y[omap(r), :] (=|+=) LayerNorm(x[imap(r), :]) * gamma + beta over 768 columns; x fp32, y bf16|fp32.
 * Replaces nn.LayerNorm at vit_helper.py:366-375, motionformer.py:232, modeling_ast.py:301,315,535,
 * sync_model.py:157,169, modules/transformer.py:94-95 and norm1/norm2 inside motionformer.py:329.
 * Contract of the 768-column row launchers (sf_layernorm768, sf_layernorm768_mxfp8, sf_add_scale_ln768, sf_broadcast_rows768, sf_gather_rows768), checked by
 * each of them - a violation returns -1 with sf_last_error set and launches nothing: every row stride is a multiple of 4 elements; every fp32 row pointer, gamma,
 * beta and table is 16-byte aligned, a bf16 output 8-byte aligned (the kernels move 16 bytes per lane and write bf16 rows 8 bytes per lane); with a row map
 * rows < 2^31 (the map works on 32-bit row indices); accumulate needs an fp32 y. */
int sf_layernorm768(const float* x, int64_t ldx, const int64_t* in_map, const float* gamma, const float* beta, void* y,
                    int y_dtype, int64_t ldy, const int64_t* out_map, int accumulate, int64_t rows, float eps,
                    void* stream);

/* dst[(s*dst_seq_rows + l), :] = table[l, :], l < L, s < n_seq (fp32, 768 cols): lays positional tables and
 * CLS/DISTILL/OFF/MOD token rows under every sequence (video_model_builder.py:221-254, modeling_ast.py:84-90,
 * sync_model.py:153-165, motionformer.py:306-307). */
int sf_broadcast_rows768(float* dst, int64_t ld, int64_t dst_seq_rows, const float* table, int64_t L, int64_t n_seq,
                         void* stream);

/* y[r, :] = cast(x[imap(r), :]) (768 cols, x fp32, y bf16|fp32): the x[:, 0] / x[:, 1:] style slicing at
 * motionformer.py:231,332, ast.py:232-236, sync_model.py:172.  ldx % 4 == 0, ldy % 4 == 0 and the alignment contract stated at sf_layernorm768. */
int sf_gather_rows768(const float* x, int64_t ldx, const int64_t* in_map, void* y, int y_dtype, int64_t ldy,
                      int64_t rows, void* stream);

/* Patch gather for Conv3d(3->768, k=s=(2,16,16)) (vit_helper.py:436-444) with extract_vfeats' permute
 * (sync_model.py:74) folded in: vid (n_seg,16,3,224,224) of `dtype` -> out bf16 (n_seg*1568, 1536).
 * dtype SF_U8 additionally applies RGBToHalfToZeroOne + RGBNormalize(0.5,0.5) (dataset/transforms.py:647-669)
 * with the reference's fp16 roundings. */
int sf_im2col_video(const void* vid, int dtype, uint16_t* out, int64_t n_seg, void* stream);

/* Patch gather for Conv2d(1->768, k16, stride 10) (modeling_ast.py:113-117): spec fp32 (n_seg, F, Ta) ->
 * out bf16 (n_seg*nf*nt, 256), nf=(F-16)/10+1, nt=(Ta-16)/10+1, row = (n*nf + fi)*nt + ti. */
int sf_im2col_spec(const float* spec, uint16_t* out, int64_t n_seg, int F, int Ta, void* stream);

/* Grouped multi-head attention, out = softmax(scale * q k^T) v.  q/k/v/out are column slices of packed bf16
 * matrices (head h at columns h*head_dim..); a sequence is `seq_rows` rows; group g of a sequence owns tokens
 * row0 + g*group_stride + i*tok_stride (i < n_tok), plus row `cls_row` as an extra first key when >= 0.
 * n_tok + (cls_row>=0) <= 208; head_dim 64 or 96.  Replaces qkv_attn on the regrouped patches in
 * DividedAttention.forward (vit_helper.py:129-147), ASTSelfAttention (modeling_ast.py:156-176) and
 * SelfAttention (modules/transformer.py:67-70). */
int sf_attention(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t ld, uint16_t* out, int64_t ldo,
                 int64_t n_seq, int64_t seq_rows, int n_groups, int row0, int group_stride, int tok_stride, int n_tok,
                 int cls_row, int heads, int head_dim, float scale, void* stream);

/* sf_attention that ALSO emits, per (sequence, head, group), the partial softmax state (m, l, o[64]; base-2 domain, fp32, 66
 * floats) of the CLS QUERY (row cls_row) over that group's keys - the CLS key itself counted in group 0 only - so the global
 * CLS row of DividedAttention (vit_helper.py:126) costs no second pass over K/V.  Needs cls_row >= 0, head_dim 64 and a free
 * query slot (n_tok <= 8 or n_tok % 16 != 0).  cls_partial: [n_seq][heads][n_groups][66]. */
int sf_attention_cls_partial(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t ld, uint16_t* out, int64_t ldo,
                             int64_t n_seq, int64_t seq_rows, int n_groups, int row0, int group_stride, int tok_stride, int n_tok,
                             int cls_row, int heads, int head_dim, float scale, float* cls_partial, void* stream);
/* Merge those partials: out[seq*out_seq_rows + out_row, head*64 + d] = sum_p o_p[d] 2^(m_p-M) / sum_p l_p 2^(m_p-M). */
int sf_attention_cls_combine(const float* partials, int n_part, uint16_t* out, int64_t ldo, int64_t out_seq_rows, int out_row,
                             int64_t n_seq, int heads, void* stream);
/* The two above writing MXFP8 - e4m3 bytes out_q (rows, heads * 64), row stride ldq bytes, and E8M0 bytes out_s in the scale planes [heads * 64 / 128][rows][4]
 * (plane stride splane bytes): the A-operand layout of sf_gemm_mxfp8 / sf_gemm_mx_res_ln768.  Bytes and scales equal sf_quantize_mxfp8 applied to the bf16 output
 * of sf_attention_cls_partial / sf_attention_cls_combine (the fine-tuning forward's attention output is only ever that operand).  head_dim 64, an even number of
 * heads; sf_attention_cls_partial_mx: 193 <= n_tok <= 207 (192 leaves no free query slot for the CLS query; the 13-key-tile space attention of DividedSpaceTimeBlock, vit_helper.py:368). */
int sf_attention_cls_partial_mx(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t ld, uint8_t* out_q, int64_t ldq, uint8_t* out_s, int64_t splane,
                                int64_t n_seq, int64_t seq_rows, int n_groups, int row0, int group_stride, int tok_stride, int n_tok, int cls_row, int heads,
                                float scale, float* cls_partial, void* stream);
int sf_attention_cls_combine_mx(const float* partials, int n_part, uint8_t* out_q, int64_t ldq, uint8_t* out_s, int64_t splane, int64_t out_seq_rows, int out_row,
                                int64_t n_seq, int heads, void* stream);

/* The spatial half of DividedSpaceTimeBlock in ONE launch (round 4; vit_helper.py:370 `self.attn(self.norm1(x), ..., 'b (f n) d', '(b f) n d')`, DividedAttention.forward
 * vit_helper.py:97-150): qkv projection (vit_helper.py:107) of every PATCH token + the per-frame attention over [CLS key; the frame's 196 patches] in the GEMM's epilogue -
 * the 2304-wide projection never reaches HBM.  Work item = (frame, head pair): the frame's first 192 token rows x q | k | v of two heads on the matrix cores, the four
 * left-over tokens of each frame and the CLS row joined from `side`.
 * X (n_seq * 1569, 768) bf16 = norm1(x), rows [CLS; frame-major patches] per sequence; W (2304, 768) bf16 = qkv.weight, bias 2304 fp32 or NULL;
 * side (n_seq * 33, 2304) bf16 = the same projection (sf_gemm_bf16 on gathered rows) of [the CLS row; for frame f = 0..7 its tokens 192..195]: row seq * 33 and rows
 * seq * 33 + 1 + 4 f + i; out (rows as X, 768) bf16: patch rows only, must not alias X; cls_partial [n_seq][12][8][66] fp32: the CLS query's softmax partial per
 * frame, as sf_attention_cls_partial writes them (merge with sf_attention_cls_combine, n_part = 8).  n_tok must be 196.  Replaces sf_gemm_bf16 (spatial qkv) +
 * sf_attention_cls_partial (space groups). */
int sf_qkv_space_attention(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias, const uint16_t* side, int64_t lds_,
                           uint16_t* out, int64_t ldo, float* cls_partial, int64_t n_seq, int n_tok, float scale, void* stream);
/* ... with TOKEN MASKS (round 5; Synchformer.forward(vis_mask=...), model/sync_model.py:72-80 -> the -inf key masks of vit_helper.py:107-141,
 * video_model_builder.py:185-225): key_keep holds one byte per row of X (what sf_token_mask_video writes); a row with flag 0 is a masked KEY for every query of its
 * frame's group and for the CLS query - its own output row is still computed, as in the reference.  An all-ones mask is bit-identical to sf_qkv_space_attention.
 * Replaces sf_gemm_bf16 + sf_attention_cls_partial_masked on masked forwards. */
int sf_qkv_space_attention_masked(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias, const uint16_t* side, int64_t lds_,
                                  uint16_t* out, int64_t ldo, float* cls_partial, int64_t n_seq, int n_tok, float scale, const uint8_t* key_keep, void* stream);

/* The rows the two fused attention launches do not project themselves, gathered for their small GEMM in ONE launch (round 5; was two sf_copy_rows_bf16 launches, and three
 * torch index ops on the MXFP8 path): out row seq * 33 <- X row seq * (1 + 8 n_tok) (the CLS row), out row seq * 33 + 1 + 4 f + i <- token n_tok - 4 + i of frame f.
 * row_bytes per row (1536 = a bf16 row of 768; 768 = the e4m3 bytes of an MXFP8 operand), strides in BYTES; with sX / sOut the rows' scale dwords of n_planes stage-major
 * planes as well (plane k at sX + k ldsx, one dword per row -> sOut + k ldso).  Reference: the CLS row and the tokens of vit_helper.py:100-158 that 196 = 6 x 32 + 4 = 8 x 24
 * + 4 leaves over. */
int sf_side_rows(const void* X, int64_t ldx_bytes, void* out, int64_t ldo_bytes, int row_bytes, const uint8_t* sX, int64_t ldsx, uint8_t* sOut, int64_t ldso,
                 int n_planes, int64_t n_seq, int n_tok, void* stream);

/* sf_qkv_space_attention on MXFP8 operands (fp8 towers): X (rows, 768) / W (2304, 768) e4m3 bytes with stage-major scale planes (6 planes, one dword per row, ldsx / ldsw
 * bytes apart: what sf_gemm_mx_res_ln768 / sf_quantize_mxfp8 write); side (n_seq * 33, 2304) bf16 from sf_gemm_mxfp8 on gathered copies of the side rows and their scale
 * dwords.  Output EITHER out (bf16) OR out_q / out_s (e4m3 bytes (rows, 768), row stride ldq, + E8M0 bytes in the scale planes [6][rows][4], splane bytes apart: byte for
 * byte sf_quantize_mxfp8 of the bf16 output; buffers of their own, not X / sX); the other pointer NULL.  cls_partial as in sf_qkv_space_attention.  Replaces sf_gemm_mxfp8
 * (spatial qkv, bf16 output) + sf_attention_cls_partial(_mx) on the MX path. */
int sf_qkv_space_attention_mx(const uint8_t* X, int64_t ldx, const uint8_t* sX, int64_t ldsx, const uint8_t* W, int64_t ldw, const uint8_t* sW, int64_t ldsw,
                              const float* bias, const uint16_t* side, int64_t lds_, uint16_t* out, int64_t ldo, uint8_t* out_q, int64_t ldq, uint8_t* out_s,
                              int64_t splane, float* cls_partial, int64_t n_seq, int n_tok, float scale, void* stream);

/* sf_qkv_time_attention on the 192 x 384 main loop of sf_qkv_space_attention (round 4; same reference lines as sf_qkv_time_attention below).  Work item = (sequence,
 * block of 24 patches, head pair): the block's 24 patches x 8 frames x q | k | v of two heads on the matrix cores, then per patch the attention over [CLS key; its 8 frames];
 * the 4 left-over patches of a sequence (196 = 8 x 24 + 4) and the CLS row come from `side`, the (n_seq * 33, 2304) buffer sf_qkv_space_attention takes (row seq * 33 = the
 * CLS row's q | k | v, rows seq * 33 + 1 + 4 f + i = token 192 + i of frame f).  out (rows as X, 768) bf16: patch rows only, must not alias X; cls_partial
 * [n_seq][12][33][66] fp32: the CLS query's softmax partials, four per block (records 4 tb .. 4 tb + 3) + record 32 (the left-over patches and the CLS key itself) -
 * merge with sf_attention_cls_combine, n_part = 33.  n_tok must be 196; ldx and ldw multiples of 64 elements.  Replaces sf_gemm_bf16 (CLS rows) + sf_qkv_time_attention. */
int sf_qkv_time_attention2(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias, const uint16_t* side, int64_t lds_,
                           uint16_t* out, int64_t ldo, float* cls_partial, int64_t n_seq, int n_tok, float scale, void* stream);
/* ... with TOKEN MASKS (round 5; same reference lines as sf_qkv_space_attention_masked): key_keep[row] == 0 masks that KEY for the queries of its patch's 8-frame group
 * and for the CLS query; an all-ones mask is bit-identical to sf_qkv_time_attention2.  Replaces sf_qkv_time_attention_masked on masked forwards. */
int sf_qkv_time_attention2_masked(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias, const uint16_t* side, int64_t lds_,
                                  uint16_t* out, int64_t ldo, float* cls_partial, int64_t n_seq, int n_tok, float scale, const uint8_t* key_keep, void* stream);

/* sf_qkv_time_attention2 on MXFP8 operands (round 5: the temporal half of the fp8 towers on the round-4 schedule; arguments as sf_qkv_space_attention_mx, cls_partial
 * [n_seq][12][33][66]).  Output EITHER out (bf16) OR out_q / out_s (byte for byte sf_quantize_mxfp8 of the bf16 output).  Replaces sf_gemm_mxfp8 (CLS rows) +
 * sf_qkv_time_attention_mx(_q). */
int sf_qkv_time_attention2_mx(const uint8_t* X, int64_t ldx, const uint8_t* sX, int64_t ldsx, const uint8_t* W, int64_t ldw, const uint8_t* sW, int64_t ldsw,
                              const float* bias, const uint16_t* side, int64_t lds_, uint16_t* out, int64_t ldo, uint8_t* out_q, int64_t ldq, uint8_t* out_s,
                              int64_t splane, float* cls_partial, int64_t n_seq, int n_tok, float scale, void* stream);

/* The temporal half of DividedSpaceTimeBlock in ONE launch (vit_helper.py:366 `self.timeattn(self.norm3(x), ..., 'b (f n) d', '(b n) f d')`,
 * DividedAttention.forward vit_helper.py:97-150): qkv projection (vit_helper.py:107) of every PATCH token + the 8-frame attention over
 * [CLS key; the patch's 8 frames] in the GEMM's epilogue - the 2304-wide projection never reaches HBM.
 * X (n_seq * (1 + 8 * n_groups), 768) bf16 = norm3(x), rows [CLS; frame-major patches] per sequence; W (2304, 768) bf16 = qkv.weight, bias 2304 fp32
 * or NULL; qkv_cls (n_seq, 2304) bf16 = the same projection of the CLS rows (sf_gemm_bf16 on the strided CLS rows, lda = seq_rows * ldx);
 * out (rows as X, 768) bf16: patch rows only; cls_partial [n_seq][12][n_groups / 4][66] fp32, records as in sf_attention_cls_partial (one per 4
 * patches) - the CLS row of `out` (vit_helper.py:126) is then written by sf_attention_cls_combine(cls_partial, n_groups / 4, out, ...).
 * 12 heads x 64; n_groups % 4 == 0; X and W below 4 GiB. */
int sf_qkv_time_attention(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias, const uint16_t* qkv_cls, int64_t ldc,
                          uint16_t* out, int64_t ldo, float* cls_partial, int64_t n_seq, int n_groups, float scale, void* stream);

/* One query row per sequence against n_keys consecutive rows (head_dim 64): the Motionformer CLS query
 * (vit_helper.py:126) and the only output row the aggregator layers ever read (motionformer.py:329-332). */
int sf_attention_cls(const uint16_t* q, int64_t q_seq_rows, int q_row, const uint16_t* k, const uint16_t* v, int64_t ld,
                     int64_t kv_seq_rows, int kv_row0, int n_keys, uint16_t* out, int64_t ldo, int64_t out_seq_rows,
                     int out_row, int64_t n_seq, int heads, int head_dim, float scale, void* stream);

/* The aggregator layer's attention for its CLS query, pooled in one pass over the fp32 residual stream (motionformer.py:231-245 final norm + regrouping,
 * 301-334 BaseEncoderLayer of which only output row 0 is read, :332).  That row's query is the layer's cls_token - a parameter - so with zn = norm1(norm(x)) rounded
 * to bf16 the scores are s[h][j] = U[h] . zn_j + c[h]  (U[h] = scale W_k[h]^T q_h, c[h] = scale q_h . b_k[h], prepared once per weight load) and the value side is
 * W_v[h] (sum_j p[h][j] zn_j) + b_v[h]: no Q, K or V of the token rows is formed.  Sequence sq = segment * n_groups + g has the keys [zn_cls; token t = 0 .. n_tok - 1
 * at X row segment * seq_rows + row0 + g * group_stride + t * tok_stride] (the descriptor of sf_attention; visual 1569, 1, 8, 196, 1, 196, audio 74, 2, 6, 1, 6, 12).
 * x fp32 (row stride ldx), read exactly once; gamma1 / beta1 / eps1 the tower's final norm, gamma2 / beta2 / eps2 the aggregator's norm1; u 12 x 768 fp32, c 12 fp32,
 * zn_cls 768 fp32 = norm1(cls_token); key_keep NULL or one byte per row of x (0 = masked key, an additive -inf; the CLS key is always kept; all-ones == NULL bit for bit).
 * g bf16 (n_seq, 12 * 2 * 768), row stride ldg: with G[sq][h][:] = sum_j softmax_j(s[h][.])_j zn_j (fp32), g[sq][h][0][:] = bf16(G) and g[sq][h][1][:] = bf16(G - hi):
 * the A operand of a bf16 GEMM against [W | W] that sees G at ~16 bits.  fp32 base-2 online softmax, deterministic, one workgroup per sequence:
 * a sequence's output bits depend on its own rows only. */
int sf_agg_cls_pool(const float* x, int64_t ldx, int64_t n_seq, int64_t seq_rows, int row0, int n_groups, int group_stride, int tok_stride, int n_tok,
                    const float* gamma1, const float* beta1, float eps1, const float* gamma2, const float* beta2, float eps2, const float* u, const float* c,
                    const float* zn_cls, const uint8_t* key_keep, uint16_t* g, int64_t ldg, void* stream);

/* Audio front-end (dataset/transforms.py:815-889; configs/sync.yaml:183-202): wave fp32 (n_seg, n_samples) ->
 * out fp32 (n_seg, n_mels, pad_to) = ((log(mel(|STFT|^2) + 1e-6), right-padded with 0.0) - mean) / (2 std), the
 * (S, 1, F, Ta) layout Synchformer.forward receives.  STFT: n_fft 1024, periodic Hann(400) centred in the frame, hop 160,
 * center/reflect.  tw_cos/tw_sin: (400, 513) twiddles with the window folded in; fb: (513, n_mels) HTK mel filterbank;
 * fb_lo/fb_hi: per-filter non-zero bin range; power_ws: fp32 workspace (n_seg * min(n_samples/hop+1, pad_to) * 513). */
int sf_mel_frontend(const float* wave, int64_t n_seg, int n_samples, int hop, const float* tw_cos, const float* tw_sin,
                    const float* fb, const int* fb_lo, const int* fb_hi, int n_mels, float* power_ws, float* out, int pad_to,
                    float mean, float std, void* stream);

/* ---- Stage-2 train step (scripts/train_sync.py:153-237, train_utils.py:373-386): backward of vproj/aproj + the sync
 * transformer and the optimizer.  GEMM-shaped work reuses sf_gemm_bf16 / sf_gemm_bf16_batched on transposed copies. ---- */

/* out[b][c][r] = in[b][r][c] (bf16), columns r in [R, R_pad) zero-filled; two-level batch strides in elements. */
int sf_transpose_bf16(const uint16_t* in, int64_t ld_in, int64_t sI0, int64_t sI1, uint16_t* out, int64_t ld_out, int64_t sO0,
                      int64_t sO1, int R, int C, int R_pad, int batch_outer, int batch_inner, void* stream);
/* n_tensors transposes of sf_transpose_bf16's wide kind (C % 8 == 0, R_pad % 8 == 0, 16-byte aligned rows) in one launch: table[t] = { in, out, ld_in, ld_out,
 * R, C, R_pad, ceil(R_pad / 64) } as int64 and tile_prefix[t] = 64 x 64 tiles before tensor t (n_tensors + 1 ints), both in DEVICE memory.  The bf16 W^T
 * operand copies of all trainable weights after an optimizer step. */
int sf_transpose_bf16_multi(const int64_t* table, const int* tile_prefix, int n_tensors, int total_tiles, void* stream);
/* y = bf16(scale * x) for a (rows, cols) fp32 matrix, cols % 4 == 0. */
int sf_cast_bf16(const float* x, int64_t ldx, uint16_t* y, int64_t ldy, int64_t rows, int cols, float scale, void* stream);
/* P[r,:L] = softmax(scale * S[r,:L]) (bf16), P[r,L:L_pad] = 0; L <= 256 (attention probabilities, modules/transformer.py:67-69). */
int sf_softmax_rows(const float* S, int64_t lds, uint16_t* P, int64_t ldp, int64_t rows, int L, int L_pad, float scale, void* stream);
/* dS = scale * P * (dP - rowsum(P * dP)) (bf16, zero-padded): backward of the softmax + 1/sqrt(d) scaling. */
int sf_softmax_bwd_rows(const uint16_t* P, int64_t ldp, const float* dP, int64_t lddp, uint16_t* dS, int64_t ldds, int64_t rows, int L,
                        int L_pad, float scale, void* stream);
/* LayerNorm(768) backward: dx[(dx_map)] (=|+=) ..., dgamma / dbeta (=|+=) column sums; statistics recomputed from x.
 * workspace: fp32, 2 * 768 * ceil(rows / 4) elements. */
int sf_layernorm768_bwd(const float* x, int64_t ldx, const int64_t* x_map, const float* gamma, const float* dy, int64_t lddy,
                        const int64_t* dy_map, float* dx, int64_t lddx, const int64_t* dx_map, int accumulate_dx, float* dgamma,
                        float* dbeta, int accumulate_dparams, float* workspace, int64_t rows, float eps, void* stream);
/* sf_layernorm768_bwd with the incoming gradient dy in bf16 (lddy % 4 == 0, 8-byte aligned rows). */
int sf_layernorm768_bwd_bf16(const float* x, int64_t ldx, const int64_t* x_map, const float* gamma, const uint16_t* dy, int64_t lddy,
                        const int64_t* dy_map, float* dx, int64_t lddx, const int64_t* dx_map, int accumulate_dx, float* dgamma,
                        float* dbeta, int accumulate_dparams, float* workspace, int64_t rows, float eps, void* stream);
/* sf_layernorm768_bwd (identity row maps, dy fp32 or bf16 by dy_dtype) that also writes the head of the NEXT residual branch's backward from the updated dx - what
 * sf_branch_grad would compute in another pass over it: y_next = bf16(seq_scale[row / seq_rows] * dx) (seq_scale NULL = 1: no stochastic depth on that branch) and
 * dbias_next[c] = sum_r seq_scale * dx[r, c] (fp32, assigned).  workspace: fp32, 3 * 768 * ceil(rows / 4) elements. */
int sf_layernorm768_bwd_branch(const float* x, int64_t ldx, const float* gamma, const void* dy, int dy_dtype, int64_t lddy, float* dx, int64_t lddx,
                               int accumulate_dx, float* dgamma, float* dbeta, int accumulate_dparams, uint16_t* y_next, int64_t ldyn, const float* seq_scale,
                               int64_t seq_rows, float* dbias_next, float* workspace, int64_t rows, float eps, void* stream);
/* out[c] (=|+=) sum_r x[r, c] (bias gradients); x fp32|bf16; workspace fp32 cols * ceil(rows / 64). */
int sf_colsum(const void* x, int x_dtype, int64_t ldx, int64_t rows, int cols, float* out, int accumulate, float* workspace, void* stream);
/* out[l, c] (=|+=) sum_b x[b*L + l, c]: gradient of the broadcast positional / token table. */
int sf_seqsum(const float* x, int64_t ldx, int n_seq, int L, int cols, float* out, int accumulate, void* stream);
/* act = gelu_erf(pre) / dpre = dact * gelu_erf'(pre) on bf16 pre-activations (n elements, n % 4 == 0). */
int sf_gelu_fwd(const uint16_t* pre, uint16_t* act, int64_t n, void* stream);
int sf_gelu_bwd(const uint16_t* pre, const float* dact, uint16_t* dpre, int64_t n, void* stream);
/* sf_gelu_bwd with the incoming gradient in bf16 (n % 8 == 0, 16-byte aligned pointers). */
int sf_gelu_bwd_bf16(const uint16_t* pre, const uint16_t* dact, uint16_t* dpre, int64_t n, void* stream);
/* loss = mean cross-entropy of (B, C) logits vs int64 targets (sync_model.py:95-96); dlogits (optional) scaled by grad_scale / B. */
int sf_cross_entropy(const float* logits, int64_t ld, const int64_t* targets, int B, int C, float* loss, float* dlogits, int64_t ldd,
                     float grad_scale, void* stream);
/* y = dropout_p(x) (+ residual): keep(i) = hash(seed, i) >= p * 2^32 over the linear element index i, kept values scaled by
 * 1/(1-p); x, y fp32|bf16 (same dtype), residual fp32 or NULL (fp32 x only).  The same (seed, shape) regenerates the mask in
 * the backward.  Dropout sites: sync_model.py:166, modules/transformer.py:70,73,90. */
int sf_dropout(const void* x, int dtype, int64_t ldx, const float* residual, int64_t ldr, void* y, int64_t ldy, int64_t rows, int cols,
               float p, uint32_t seed, void* stream);
/* Whole-token dropout of the sync transformer's inputs - GlobalTransformer.tok_drop_vis / tok_drop_aud, torch.nn.Dropout1d on (B, S, D) = whole tokens dropped
 * (model/sync_model.py:131-134, 160-161, train mode with tok_pdrop > 0): y[y_map(r), :] (=|+=) row_scale[r] * x[x_map(r), :], fp32, cols % 4 == 0; row_scale[r] is 0 or
 * 1 / (1 - p) per token (sf_dropout over a vector of ones); x_map / y_map = 6-integer row maps or NULL (identity).  Forward: the input LayerNorm's rows into the token
 * matrix on top of the positional table (accumulate = 1); backward: the token matrix's gradient rows, scaled, as the LayerNorm backward's dY (accumulate = 0). */
int sf_scale_rows_map(const float* x, int64_t ldx, const int64_t* x_map, const float* row_scale, float* y, int64_t ldy, const int64_t* y_map, int64_t rows, int cols,
                      int accumulate, void* stream);
/* Head of a residual branch's backward in the Stage-1 towers (the `x = x + drop_path(branch(x))` sites of vit_helper.py:364-376 / modeling_ast.py ASTLayer):
 * y = bf16(s[r / seq_rows] * dx[r, :]) (the dY operand of the branch's output Linear) and dbias (=|+=) the fp32 column sums of the scaled gradient, in one
 * pass over dx (seq_scale may be NULL).  Replaces sf_scale_seq_add -> sf_cast_bf16 -> sf_colsum.  cols % 32 == 0; workspace >= cols * ceil(rows / 64) floats. */
int sf_branch_grad(const float* dx, int64_t ldx, const float* seq_scale, int64_t seq_rows, uint16_t* y, int64_t ldy, int64_t rows, int cols, float* dbias,
                   int accumulate, float* workspace, void* stream);
/* x = residual + seq_scale[r / seq_rows] * branch (fp32; seq_scale may be NULL = 1) and y = bf16(LayerNorm(x) * gamma + beta) in one pass: the stochastic-depth
 * residual add and the next sub-layer's norm of the Stage-1 forward (vit_helper.py:364-376); sf_scale_seq_add followed by sf_layernorm768. */
int sf_add_scale_ln768(const float* branch, int64_t ldb, const float* seq_scale, int64_t seq_rows, const float* residual, int64_t ldr, float* x, int64_t ldx,
                       const float* gamma, const float* beta, uint16_t* y, int64_t ldy, int64_t rows, float eps, void* stream);
/* Stochastic depth of the Stage-1 visual tower (DropPath at vit_helper.py:356,372,375, rates video_model_builder.py:86-87 = linspace(0, 0.2, 12)):
 * y[r,:] = (residual ? residual[r,:] : 0) + seq_scale[r / seq_rows] * x[r,:], fp32, cols % 4 == 0; seq_scale[i] is 0 or 1/keep_prob per
 * segment.  The forward applies it to a residual branch, the backward to the incoming gradient with the same scales. */
int sf_scale_seq_add(const float* x, int64_t ldx, const float* seq_scale, int64_t seq_rows, const float* residual, int64_t ldr, float* y,
                     int64_t ldy, int64_t rows, int cols, void* stream);
/* norm_out[0] = ||g||_2 of a flat fp32 buffer (deterministic two-stage; workspace fp32 1024). */
int sf_grad_norm(const float* g, int64_t n, float* norm_out, float* workspace, void* stream);
/* clip_grad_norm_(max_norm, device-resident norm) + Adam(betas, eps, no weight decay) on flat fp32 buffers; also writes the
 * bf16 copy of the updated parameters when p_bf16 != NULL.  step >= 1 is the Adam step count (bias correction). */
int sf_adam_clip_step(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, const float* norm, float max_norm,
                      float lr, float beta1, float beta2, float eps, int step, void* stream);

/* ---- Stage-1 segment-level contrastive head (train_clip_src/open_clip/model.py:449-585) ------------------------------ */
/* y[r, :768] = mean_j x[r*t + j, :768], then (normalize != 0) divided by max(||.||_2, 1e-12):  AveragePooling 'BS t D -> BS D'
 * (motionformer.py:395-409, ast.py:87-88) and F.normalize (open_clip/model.py:530-531); fp32, row strides % 4 == 0. */
int sf_meanpool_l2norm768(const float* x, int64_t ldx, int t, float* y, int64_t ldy, int normalize, int64_t n, void* stream);
/* out[i, j] = scale * <a_i, b_j> for fp32 a (n, d), b (m, d), d % 16 == 0: sim = feat @ feat_all^T / logit_scale
 * (open_clip/model.py:508-509); kept in fp32 because scale can be as large as 1 / 0.001. */
int sf_similarity_f32(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldo, int n, int m, int d, float scale,
                      void* stream);

/* ---- feature-extractor backward helpers (Stage-1 training; the matmul-shaped parts reuse the GEMM entry points) ------------ */
/* dst[dst_map(r), :cols] = src[src_map(r), :cols] for r < rows (bf16, cols % 8 == 0): builds / scatters the per-group
 * sequences [CLS; group tokens] of divided space-time attention (vit_helper.py:100-158, 341-344). */
int sf_copy_rows_bf16(const uint16_t* src, int64_t ld_src, const int64_t* src_map, uint16_t* dst, int64_t ld_dst, const int64_t* dst_map,
                      int64_t rows, int cols, void* stream);
/* out[s*out_seq_stride + c] (=|+=) sum_{g<G} in[s*in_seq_stride + g*in_group_stride + c]: the CLS row is a key/value of every
 * group, so its dk|dv is the sum over groups (strides in elements). */
int sf_reduce_groups_bf16(const uint16_t* in, int64_t in_seq_stride, int64_t in_group_stride, int G, uint16_t* out, int64_t out_seq_stride,
                          int cols, int64_t n_seq, int accumulate, void* stream);
/* Backward of sf_attention_cls (same addressing): dO row (seq*do_seq_rows + do_row) -> dq at the query row (=), dk / dv at the
 * n_keys key rows (=|+=); head_dim 64, n_keys <= 2048. */
int sf_attention_cls_bwd(const uint16_t* q, int64_t q_seq_rows, int q_row, const uint16_t* k, const uint16_t* v, int64_t ld,
                         int64_t kv_seq_rows, int kv_row0, int n_keys, const uint16_t* dO, int64_t lddo, int64_t do_seq_rows, int do_row,
                         uint16_t* dq, uint16_t* dk, uint16_t* dv, int64_t ldg, int64_t n_seq, int heads, int head_dim, float scale,
                         int accumulate_kv, void* stream);
/* Backward of sf_meanpool_l2norm768: dx[r*t + j, :] = d(mean -> normalize)/dx applied to dy[r, :] (x = the forward input). */
int sf_meanpool_l2norm768_bwd(const float* x, int64_t ldx, int t, const float* dy, int64_t lddy, float* dx, int64_t lddx, int normalize,
                              int64_t n, void* stream);

/* ---- device-side segmenting (dataset/transforms.py:402-500 GenerateMultipleSegments; SURVEY §8f "next" rank 1) ------------------
 * The segments of a clip overlap by 50 % (step_size_seg 0.5): instead of materialising (S, 16, C, H, W) / (S, n_samples) copies on
 * the host and shipping 1.8x the bytes over PCIe, the two front-end gathers read the segment windows straight from the clip:
 * segment (clip, s) = frames [frame0 + s*seg_stride, +16) of vid (n_clips, clip_frames, 3, 224, 224), and samples
 * [sample0 + s*seg_stride, +n_samples) of wave (n_clips, clip_samples).  Reflect padding of the STFT stays inside a segment. */
int sf_im2col_video_clips(const void* vid, int dtype, int64_t n_clips, int64_t clip_frames, int frame0, int seg_stride, int n_seg,
                          uint16_t* out, void* stream);
/* ... into the TOKEN layout: out bf16 (n_clips * n_seg * 1569, 1536), segment n's 1568 patch rows at n * 1569 + 1 .., its row 0 (the CLS slot) zeroed - the
 * patch-embedding GEMM (Conv3d of PatchEmbed3D, motionformer.py) then runs with identity row maps straight onto the (n * 1569, 768) token matrix. */
int sf_im2col_video_tokens(const void* vid, int dtype, int64_t n_clips, int64_t clip_frames, int frame0, int seg_stride, int n_seg, uint16_t* out, void* stream);
int sf_mel_frontend_clips(const float* wave, int64_t n_clips, int64_t clip_samples, int64_t sample0, int64_t seg_stride, int n_seg,
                          int n_samples, int hop, const float* tw_cos, const float* tw_sin, const float* fb, const int* fb_lo,
                          const int* fb_hi, int n_mels, float* power_ws, float* out, int pad_to, float mean, float std, void* stream);

/* ---- train-time inputs from raw clips (TemporalCropAndOffset(ForSyncabilityTraining), RGBSpatialCrop(is_random=True), RandomHorizontalFlip,
 * GenerateMultipleSegments(is_start_random=True); dataset/transforms.py:56-95, 200-215, 242-630) ------------------------------------------
 * Every clip has its own window, drawn on the host (synchformer_amd.augment) and passed as a DEVICE table, so nothing forces a host sync.
 * sf_im2col_video_crops: vid uint8 (n_clips, clip_frames, 3, H, W), H, W >= 224; table int32 [n_clips][table_ld >= 4] = frame0, y0, x0, flip.
 * Segment (clip, s) = frames frame0 + s*seg_stride .. +16, spatial crop [y0, +224) x [x0, +224), mirrored along W when flip != 0, RGB
 * normalisation as in sf_im2col_video.  out: the layout of sf_im2col_video_clips (tok_rows 1568) or sf_im2col_video_tokens (1569).
 * sf_mel_frontend_starts: sf_mel_frontend_clips with a per-clip device array sample0[n_clips] (int64) instead of one start.
 * The launchers cannot read the device tables: the kernels clamp every entry into its clip (a bad row reads wrong data, never out of bounds);
 * the host validates the rows before upload. */
int sf_im2col_video_crops(const uint8_t* vid, int64_t n_clips, int64_t clip_frames, int H, int W, const int* table, int table_ld, int seg_stride,
                          int n_seg, uint16_t* out, int tok_rows, void* stream);
int sf_mel_frontend_starts(const float* wave, int64_t n_clips, int64_t clip_samples, const int64_t* sample0, int64_t seg_stride, int n_seg,
                           int n_samples, int hop, const float* tw_cos, const float* tw_sin, const float* fb, const int* fb_lo,
                           const int* fb_hi, int n_mels, float* power_ws, float* out, int pad_to, float mean, float std, void* stream);

/* ---- Stage-1 train-time augmentations from raw clips (transform_sequence_train of configs/segment_avclip.yaml: RGBSpatialCropSometimesUpscale,
 * GenerateMultipleSegments(is_start_random, audio_jitter_sec), RandomApplyColorDistortion, RandomHorizontalFlip, AudioRandomVolume,
 * AudioRandomLowpassFilter, AudioRandomGaussNoise; dataset/transforms.py:110-218, 402-500, 672-812) ------------------------------------------
 * The host draws the decisions (synchformer_amd.augment.Stage1Sampler) into two int32 DEVICE tables; floats are stored as their bit patterns.
 *   clip table [n_clips][clip_ld >= SF_S1_CLIP_COLS]: frame0, y0, x0, side (224, or 192 = a 192 crop resampled to 224), sample0 (audio jitter included).
 *   segment table [n_clips * n_seg][seg_ld >= SF_S1_SEG_COLS], row of segment (clip, s) at clip * n_seg + s:
 *     [0] colour jitter on;  [1..4] the order of its four ops (torchvision's fn_idx: 0 brightness, 1 contrast, 2 saturation, 3 hue; any other
 *     code is no op; the host sends a permutation - contrast takes the frame mean in front of its FIRST occurrence);
 *     [5, 6] / [7, 8] / [9, 10] brightness / contrast / saturation blend pair r32 = float32(ratio), q32 = float32(1.0 - ratio), the
 *     subtraction in double;  [11] hue shift;  [12] gray;  [13] flip;  [14] audio flags SF_S1_AUDIO_*;  [15] noise seed (uint32).
 * sf_stage1_video_augment: vid uint8 (n_clips, clip_frames, 3, H, W), 4-byte aligned, H, W >= 224 -> out uint8 (n_clips * n_seg, 16, 3, 224, 224),
 *   16-byte aligned (the input of sf_im2col_video): segment (clip, s) = frames frame0 + s*seg_stride .. +16, crop [y0, +side) x [x0, +side).
 *   side 192: bilinear to 224, align_corners=False, no antialias, source coordinate (dst + 0.5) * 192/224 - 0.5 with edges clamped, rounded half to even.
 *   Then, per segment, torchvision 0.15's uint8 tensor arithmetic in fp32 without contraction:
 *     blend(a, b) = trunc(clamp(r32 * a + q32 * b, 0, 255));  gray = trunc(0.2989 r + 0.587 g + 0.114 b), left to right;
 *     brightness = blend(x, 0), saturation = blend(x, gray), contrast = blend(x, mean) with mean = float(sum of gray over the FRAME as it is
 *     when contrast is reached) / 50176;  hue: x / 255 -> RGB->HSV -> h = (h + f) mod 1 -> HSV->RGB -> trunc(v * 255.999);
 *     then gray into all three channels (RandomGrayscale) and the mirror along W.
 *   frame_sums: int32 workspace (n_clips * n_seg * 16), the per-frame gray sums (written for jittered segments only).  Two launches.
 * sf_stage1_audio_augment: wave fp32 (n_clips, clip_samples) -> out fp32 (n_clips * n_seg, n_samples): samples [sample0 + s*seg_stride, +n_samples),
 *   then per segment, in this order: SF_S1_AUDIO_VOLUME clamp(2 x, -1, 1) (Vol(2.0, 'amplitude')); SF_S1_AUDIO_LOWPASS the biquad
 *   y[i] = (b0 x[i] + b1 x[i-1] + b2 x[i-2]) - (a1 y[i-1] + a2 y[i-2]) from zero state, output clamped to [-1, 1] (lowpass_biquad -> lfilter(clamp=True);
 *   coefficients already divided by a0, computed by the host in double); SF_S1_AUDIO_NOISE x + noise_amp * n, n ~ N(0, 1) by Box-Muller from
 *   Philox4x32-10 with key (seed, 0) and counter (sample index, 0, 0, 0): the same seed gives the same noise.  Two launches.
 * AudioRandomReverb and AudioRandomPitchShift (sox effects) are NOT built.
 * The launchers cannot read the device tables: the kernels clamp every entry into its clip (a bad row reads wrong data, never out of bounds);
 * the host validates the rows before upload. */
enum { SF_S1_CLIP_FRAME0 = 0, SF_S1_CLIP_Y0 = 1, SF_S1_CLIP_X0 = 2, SF_S1_CLIP_SIDE = 3, SF_S1_CLIP_SAMPLE0 = 4, SF_S1_CLIP_COLS = 5 };
enum { SF_S1_SEG_JITTER = 0, SF_S1_SEG_OP0 = 1, SF_S1_SEG_BRIGHT_R = 5, SF_S1_SEG_CONTRAST_R = 7, SF_S1_SEG_SATUR_R = 9, SF_S1_SEG_HUE = 11,
       SF_S1_SEG_GRAY = 12, SF_S1_SEG_FLIP = 13, SF_S1_SEG_AUDIO = 14, SF_S1_SEG_SEED = 15, SF_S1_SEG_COLS = 16 };
enum { SF_S1_AUDIO_VOLUME = 1, SF_S1_AUDIO_LOWPASS = 2, SF_S1_AUDIO_NOISE = 4 };
int sf_stage1_video_augment(const uint8_t* vid, int64_t n_clips, int64_t clip_frames, int H, int W, const int* clip_table, int clip_ld,
                            const int* seg_table, int seg_ld, int seg_stride, int n_seg, int* frame_sums, uint8_t* out, void* stream);
int sf_stage1_audio_augment(const float* wave, int64_t n_clips, int64_t clip_samples, const int* clip_table, int clip_ld, const int* seg_table,
                            int seg_ld, int64_t seg_stride, int n_seg, int n_samples, float b0, float b1, float b2, float a1, float a2,
                            float noise_amp, float* out, void* stream);

/* ---- token masks (Synchformer.forward(vis_mask=, aud_mask=), sync_model.py:38-89) -------------------------------
 * content_keep: bool bytes shaped like the input ((n,16,3,224,224) / (n,F,Ta)), 1 = kept.  tok_keep[n*L + t] = 0 iff the masked
 * elements of token t's patch meet filter-0 weights of both signs or a zero weight (the reference's inf -> NaN trick,
 * video_model_builder.py:185-201, modeling_ast.py:515-530); w0_sign = sign of filter 0 per patch element (int8), CLS/DISTILL kept. */
int sf_token_mask_video(const uint8_t* content_keep, int64_t n_seg, const int8_t* w0_sign, uint8_t* tok_keep, void* stream);
int sf_token_mask_spec(const uint8_t* content_keep, int64_t n_seg, int F, int Ta, const int8_t* w0_sign, uint8_t* tok_keep, void* stream);
/* sf_attention / sf_attention_cls with a key mask: key_keep[row] == 0 gives K/V row `row` (same row indexing as k) a score of -inf
 * (qkv_attn tok_mask, vit_helper.py:34-42; ASTSelfAttention, modeling_ast.py:160-163; aggregators' src_mask, motionformer.py:308-329). */
int sf_attention_masked(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t ld, uint16_t* out, int64_t ldo, int64_t n_seq,
                        int64_t seq_rows, int n_groups, int row0, int group_stride, int tok_stride, int n_tok, int cls_row, int heads,
                        int head_dim, float scale, const uint8_t* key_keep, void* stream);
int sf_attention_cls_masked(const uint16_t* q, int64_t q_seq_rows, int q_row, const uint16_t* k, const uint16_t* v, int64_t ld,
                            int64_t kv_seq_rows, int kv_row0, int n_keys, uint16_t* out, int64_t ldo, int64_t out_seq_rows, int out_row,
                            int64_t n_seq, int heads, int head_dim, float scale, const uint8_t* key_keep, void* stream);
/* The masked forward on the fused schedules (round 3): sf_attention_cls_partial and sf_qkv_time_attention with the same key flags (one byte per K/V /
 * token row, 0 = masked: -inf before the softmax, for the patch queries and for the CLS query's partial records; a record whose keys are all masked is
 * (m = -inf, l = 0, o = 0) and drops out in sf_attention_cls_combine).  Reference: vit_helper.py:34-42, 107-141, sync_model.py:72-89. */
int sf_attention_cls_partial_masked(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t ld, uint16_t* out, int64_t ldo, int64_t n_seq,
                                    int64_t seq_rows, int n_groups, int row0, int group_stride, int tok_stride, int n_tok, int cls_row, int heads,
                                    int head_dim, float scale, float* cls_partial, const uint8_t* key_keep, void* stream);
int sf_qkv_time_attention_masked(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias, const uint16_t* qkv_cls, int64_t ldc,
                                 uint16_t* out, int64_t ldo, float* cls_partial, int64_t n_seq, int n_groups, float scale, const uint8_t* key_keep,
                                 void* stream);

/* Stage-1 zero-shot sync check (shift_and_get_preds, train_clip_src/training/train.py:549-579): G = audio-to-video segment similarity
 * (n_clips*S x n_clips*S, fp32, clip-major); per clip, window sims are W-long diagonal sums of its S x S block;
 * preds_a[b, j] = argmax_i, preds_v[b, i] = argmax_j over the S - W + 1 (<= 32) shifts. */
int sf_shift_window_preds(const float* G, int64_t ldg, int n_clips, int S, int W, int64_t* preds_a, int64_t* preds_v, void* stream);

/* Track read-out of a recording: logits (W, C) fp32 (row stride ldl >= C) of W overlapping windows, in time order -> per window the argmax class (lowest index
 * on ties) and its softmax probability (cls_raw, conf_raw), and the Viterbi path under a cost lam >= 0 per class step (cls_path, conf_path = softmax probability
 * of the path's class):  e[w, c] = logits[w, c] - max_c logits[w, .];  s_0 = e[0];  s_w[c] = max_p (s_{w-1}[p] - lam * |p - c|) + e[w, c], lowest p on ties ->
 * backptr[w, c];  s_w -= max_c s_w[c] after every step;  end state = argmax s_{W-1}, lowest index on ties;  backtrace through backptr (W * C bytes, caller-owned
 * workspace).  2 <= C <= 64 (one lane per class); W == 0 launches nothing.  Non-finite logits give unspecified classes, all inside [0, C).  fp32 statistics.
 * Stands next to the reference's single-window read-out, decode_single_video_prediction (example.py:38-56), on the class grid of make_class_grid
 * (dataset/transforms.py:221-239); the reference itself has no recording-level read-out. */
int sf_track_decode(const float* logits, int64_t ldl, int W, int C, float lam, int32_t* cls_raw, float* conf_raw, int32_t* cls_path, float* conf_path,
                    uint8_t* backptr, void* stream);

/* Posterior (forward-backward) read-out of the same chain: the Viterbi path above is the mode of
 *     p(c_0 .. c_{W-1})  ~  exp(sum_w e[w, c_w] - lam sum_{w >= 1} |c_w - c_{w-1}|),        e[w, c] = logits[w, c] - lse_c logits[w, .]   (the TRUE log-softmax),
 * this entry gives its marginals.  logits (W, C) fp32, row stride ldl >= C, rows in time order, 2 <= C <= 64, lam finite and >= 0, grid (C) fp32 = the offsets
 * (seconds) the classes stand for.  With lse = log sum exp:
 *     a_0 = e[0];            a_w[c] = e[w, c] + lse_p (a_{w-1}[p] - lam |p - c|)
 *     b_{W-1} = 0;           b_w[c] = lse_n (b_{w+1}[n] + e[w+1, n] - lam |n - c|)
 *     post[w, c]     = exp(a_w[c] + b_w[c] - lse_c (a_w + b_w))              (W, C) fp32, row stride ldp >= C; rows sum to 1
 *     cls_post[w]    = argmax_c post[w, c], lowest index on ties;            conf_post[w] = post[w, cls_post[w]]
 *     offset_mean[w] = sum_c post[w, c] grid[c]                              ascending c, fp32
 *     log_z[0]       = lse_c a_{W-1}[c]                                      <= 0; 0 at lam = 0 and at W = 1: the log of the probability mass that independent
 *                                                                            per-window softmax draws keep under the smoothness penalty
 * Log domain, fp32; every lse is a max pass and a sum-of-exp pass in ascending index.  After every step the maximum of a_w / b_w is subtracted (a per-row constant
 * cancels in post), so the scores are bounded for any W; the amounts subtracted from a are summed in a double and carried into log_z.  At lam = 0 and at W = 1
 * post[w] = softmax(logits[w]); reversing the rows reverses post and keeps log_z.  A -inf logit is a masked class: in a row with a finite entry it gives post == 0
 * exactly there, finite values elsewhere and no NaN.  Rows with NaN or +inf give unspecified values; cls_post lies in [0, C) always (a NaN never wins `>`).
 * workspace: caller-owned, 2 * W * C floats (a, then b; 8 W C bytes).  Two launches on the caller's stream (the two scans side by side in one launch of two
 * one-wavefront workgroups, then one thread per window), no allocation, no host synchronisation; W == 0 launches nothing and writes nothing. */
int sf_track_posterior(const float* logits, int64_t ldl, int W, int C, float lam, const float* grid, float* post, int64_t ldp, int32_t* cls_post,
                       float* conf_post, float* offset_mean, float* log_z, float* workspace, void* stream);

/* Fixed-lag read-out of a STREAM of window logits: rows l_0, l_1, ... arrive in pushes, in order.  With path_t = sf_track_decode's cls_path and post_t =
 * sf_track_posterior's post on rows 0 .. t (the same emission, renormalisation and tie rules), a push that brings the stream to t + 1 rows returns
 *     cls_raw, conf_raw (n)                      per new row, as sf_track_decode gives them
 *     cls_lag[w] = path_{w+lag}[w]               for every window w whose row w + lag arrived in this push (n_commit of them, from w0 = max(0, rows_done - lag));
 *     conf_lag[w]                                the softmax probability of cls_lag[w] in row w.  Committed once, never revised
 *     post_lag[w, :] = post_{w+lag}[w, :]        (posterior) with cls_post_lag, conf_post_lag, offset_mean_lag as sf_track_posterior defines them; row stride ldp >= C
 *     cls_tail[j] = path_t[t - n_tail + 1 + j]   the path of the whole prefix on the n_tail = min(lag, t + 1) windows not yet committed, conf_tail likewise:
 *                                                cls_tail[n_tail - 1] is the current offset; a later push may change it
 *     log_z[0]                                   (posterior) that of the prefix 0 .. t
 * final != 0 closes the stream: every window not yet committed is committed from the whole prefix (path_t / post_t) and the tail is empty; n may be 0 then.
 * The counts are host arithmetic:  done(T) = max(0, T - lag);  n_commit = (final ? rows_done + n : done(rows_done + n)) - done(rows_done);
 * n_tail = final ? 0 : min(lag, rows_done + n).  The outputs are caller-owned with at least those sizes (a block of size 0 may be null).
 * state: one opaque device buffer per stream of sf_track_stream_bytes(C, lag, posterior) bytes, 16-byte aligned; it is read only when rows_done > 0, so a fresh
 * stream needs no reset.  It holds the scan vectors after the last row (the Viterbi scores; posterior: the normalised forward vector and the double of subtracted
 * maxima) and, of the last `lag` rows, the back pointers, the logits and (posterior) the forward vectors, as rings: its size does not depend on rows_done.
 * rows_done: the rows pushed into this state so far (the caller counts; int64).  workspace: sf_track_stream_workspace_bytes(C, n, posterior) bytes, caller-owned,
 * dead after the push.  2 <= C <= 64, 0 <= lag <= 255, n <= 2^20 rows per push, lam finite and >= 0; -1 and a message otherwise, before anything is launched.
 * Up to four launches on the caller's stream (the row statistics, the two causal scans side by side, one wavefront per committed window plus one for the tail, the
 * rings' update); nothing is read back, allocated or synchronised, so a push can be captured in a graph (rows_done is then part of the capture).  A push with
 * posterior == 0 on a state sized with posterior != 0 (or the reverse) is an error of the caller: the three arguments C, lag, posterior are the state's.
 * Non-finite rows follow the offline rules: every class written lies in [0, C). */
int sf_track_stream_bytes(int C, int lag, int posterior);
int sf_track_stream_workspace_bytes(int C, int n, int posterior);
int sf_track_stream_push(void* state, int C, int lag, int posterior, int64_t rows_done, const float* logits, int64_t ldl, int n, float lam, const float* grid,
                         int final, int32_t* cls_raw, float* conf_raw, int32_t* cls_lag, float* conf_lag, float* post_lag, int64_t ldp, int32_t* cls_post_lag,
                         float* conf_post_lag, float* offset_mean_lag, int32_t* cls_tail, float* conf_tail, float* log_z, void* workspace, void* stream);

/* The same read-out for MANY streams in one call (ABI v20): sf_track_pool_push advances the states of n_active streams that share C, lag and posterior.  For every
 * stream the outputs and the state bytes are those of sf_track_stream_push on that stream alone, bit for bit (the kernels call the same device functions); the number
 * of launches does not depend on n_active: the same at-most-four kinds (row statistics, scans, read-out, rings).
 * states: one caller-owned device buffer of n_slots states, state i at byte i * state_stride; state_stride a multiple of 16 and at least
 *   sf_track_stream_bytes(C, lag, posterior); the layout of one state is sf_track_stream_push's.  A state is read only when its rows_done > 0.
 * table: n_active rows of 8 int64, one per stream of this push:
 *     [0] slot       which state (distinct, < n_slots)            [4] final     != 0 closes the stream (as sf_track_stream_push's final)
 *     [1] rows_done  rows pushed into that state so far           [5] commit0   where its committed block starts in cls_lag .. offset_mean_lag (post_lag: row commit0)
 *     [2] n          its new rows in this push (0 allowed)        [6] tail0     where its tail starts in cls_tail / conf_tail
 *     [3] row0       its rows are rows [row0, row0 + n) of logits [7] unused, 0
 *   passed twice: table_host (the launcher validates it and sizes its grids from it) and table_dev (a device copy the caller has uploaded, in stream order before
 *   this call; the kernels read it).  commit0 / tail0 are the running sums of sf_track_stream_push's n_commit / n_tail in table order: the blocks lie back to back.
 * logits (total_rows, C) fp32 with row stride ldl >= C: the new rows of all streams; the row ranges are disjoint and inside total_rows (gaps are allowed: their
 *   cls_raw / conf_raw are written from whatever the rows hold).  cls_raw / conf_raw (total_rows) are indexed like logits.  log_z (posterior): one float per table row,
 *   written for every stream that holds at least one row after the push.  workspace: sf_track_pool_workspace_bytes(C, total_rows, posterior) bytes, caller-owned,
 *   dead after the push; stream e's part is addressed by its row0.
 * 1 <= n_active <= 4096, total_rows <= 2^20; C, lag, lam as sf_track_stream_push.  -1 and a message, before anything is launched, for: a bad C / lag / lam / stride,
 * n_active out of range, a slot twice or >= n_slots, overlapping or outlying row ranges, commit0 / tail0 that are not the running sums, a null pointer for a block
 * that is not empty.  The launcher reads nothing back, allocates nothing on the device and synchronises nothing.  Block-to-work mapping: blockIdx.y = table row,
 * blockIdx.x = the stream's own work item (scan / committed window or tail / ring row), blocks beyond a stream's count exit at once. */
int sf_track_pool_workspace_bytes(int C, int total_rows, int posterior);
int sf_track_pool_push(void* states, int64_t state_stride, int n_slots, int C, int lag, int posterior, const int64_t* table_host, const int64_t* table_dev,
                       int n_active, const float* logits, int64_t ldl, int total_rows, float lam, const float* grid, int32_t* cls_raw, float* conf_raw,
                       int32_t* cls_lag, float* conf_lag, float* post_lag, int64_t ldp, int32_t* cls_post_lag, float* conf_post_lag, float* offset_mean_lag,
                       int32_t* cls_tail, float* conf_tail, float* log_z, void* workspace, void* stream);

/* The two offline read-outs GATED by synchronizability (ABI v24).  A second, 2-way head (GlobalTransformerWithSyncabilityHead, sync_model.py:176-190;
 * class 1 = synchronizable) reads the same windows: gate_logits (W, 2) fp32, row stride ldg >= 2, beside logits (W, C), row stride ldl >= C.  One chain over the 2C
 * states j = m * C + c (c the offset class, m = 1 synchronizable) joins them:
 *     d = z[w, 1] - z[w, 0];    ls = -softplus(-d);    lu = -softplus(d);    softplus(x) = max(x, 0) + log1p(exp(-|x|))                                  (fp32)
 *     E[w, c, 1] = ls + l[w, c] - lse_c l[w, .];       E[w, c, 0] = lu - log C          (true log-probabilities: every row sums to 1 over the 2C states)
 *     T((p, m') -> (c, m)) = -lam |p - c| - mu [m' != m]                                 lam, mu finite and >= 0
 * A window judged not synchronizable is flat over the offset classes: the chain carries the class across it on the smoothness prior; mu is the flag's hysteresis; a
 * caller's prior on the flag is a constant added to z[:, 1].  2 <= C <= 32 (one lane per state).
 * sf_track_decode_gated: cls_raw / conf_raw as sf_track_decode gives them (from logits alone), sync_raw[w] = sigmoid(d), and the mode of the chain:
 *     S_0 = E[0];   S_w[j] = E[w, j] + max_j' (S_{w-1}[j'] + T(j', j)), the LOWEST predecessor state j' on ties -> backptr[w, j] (one byte);   S_w -= max_j S_w[j];
 *     end state = the lowest state of maximal S_{W-1};   cls_path = j % C, sync_path = j / C (int32) along the backtrace;   conf_path = the softmax probability of
 *     cls_path in the offset row.  backptr: W * 2C bytes, caller-owned.  Three launches.
 * sf_track_posterior_gated: the marginals of the same chain.  With a, b the scans of sf_track_posterior over the 2C states (E, T as above) and post2 = the normalised
 * exp(a + b):
 *     post[w, c] = post2[w, c, 0] + post2[w, c, 1]    (row stride ldp >= C; rows sum to 1);      p_sync[w] = sum_c post2[w, c, 1]    in [0, 1]
 *     cls_post, conf_post, offset_mean from post and log_z[0] = lse_j a_{W-1}[j] <= 0 exactly as sf_track_posterior defines them
 *     reversing the rows reverses post and p_sync and keeps log_z.  workspace: 4 * W * C floats (a, then b, (W, 2C) each), caller-owned.  Two launches.
 * Both: -1 and a message, before anything is launched, for a bad C, stride, lam, mu or a null pointer; W == 0 launches nothing and needs no buffers.  The launchers read
 * nothing back, allocate nothing and synchronise nothing.  Rows with non-finite values give unspecified results, every index inside [0, C) / {0, 1}.  Masked (-inf)
 * classes are not served here. */
int sf_track_decode_gated(const float* logits, int64_t ldl, const float* gate_logits, int64_t ldg, int W, int C, float lam, float mu, int32_t* cls_raw, float* conf_raw,
                          float* sync_raw, int32_t* cls_path, int32_t* sync_path, float* conf_path, uint8_t* backptr, void* stream);
int sf_track_posterior_gated(const float* logits, int64_t ldl, const float* gate_logits, int64_t ldg, int W, int C, float lam, float mu, const float* grid, float* post,
                             int64_t ldp, float* p_sync, int32_t* cls_post, float* conf_post, float* offset_mean, float* log_z, float* workspace, void* stream);

/* Pairwise marginals of neighbouring windows (additions under ABI v25): the joint of (c_w, c_{w+1}) under the chains of sf_track_posterior /
 * sf_track_posterior_gated, given all windows.  With a, b, e as sf_track_posterior defines them, per boundary w = 0 .. W - 2:
 *     t[p, c]      = a_w[p] - lam |p - c| + e[w+1, c] + b_{w+1}[c]
 *     xi[w, p, c]  = exp(t[p, c] - lse_{p,c} t)       (W - 1, C, C) fp32 contiguous, or NULL: not stored.  Sums to 1; its row sums are post[w], its column sums post[w+1]
 *     p_change[w]  = sum_{p != c} xi[w, p, c]          summed directly, not 1 - the diagonal: a small value keeps its digits
 *     jump_abs[w]  = sum xi[w, p, c] |p - c|           the expected class step; sum_w jump_abs = - d log_z / d lam
 *     (top_from[w], top_to[w]) = the off-diagonal pair of largest xi, p_top[w] its mass; ties take the lowest p, then the lowest c: no off-diagonal mass gives (0, 1, 0.0)
 *     log_z[0]     as sf_track_posterior writes it (bit for bit: the same scan)
 * sf_track_pairwise_gated: the pair is over the states (p, m') -> (c, m) with E[w+1, c, m] for e and -lam |p - c| - mu [m' != m] for the transition; the outputs above
 * come from the pair marginal with both flags summed out (xi is the (C, C) class-pair marginal), p_flip[w] = the mass with m' != m; sum_w p_flip = - d log_z / d mu.
 * A pair with a masked (-inf) end is exactly 0 (plain chain; the gated chain does not serve masked classes).  NaN or +inf input: values unspecified, top_from and top_to
 * in [0, C) and different.  Limits as the posterior entries: 2 <= C <= 64 (gated: 32), lam and mu finite and >= 0, ldl >= C, ldg >= 2; -1 and a message before anything
 * is launched otherwise, and for a null pointer (xi excepted; the W - 1 = 0 rows of W == 1 may be null).  W == 0 returns 0 and needs no buffers; W == 1 writes log_z only.
 * workspace: 2 W C floats (gated: 4 W C), caller-owned.  Two launches on the caller's stream: the scan kernel of the posterior entry, unchanged, then one wavefront per
 * boundary (four per block; the lane is the destination state, a_w in LDS; fixed-order wave reductions, no atomics: the same bits from call to call).  Nothing is read
 * back, allocated or synchronised. */
int sf_track_pairwise(const float* logits, int64_t ldl, int W, int C, float lam, float* p_change, float* jump_abs, int32_t* top_from, int32_t* top_to, float* p_top,
                      float* xi, float* log_z, float* workspace, void* stream);
int sf_track_pairwise_gated(const float* logits, int64_t ldl, const float* gate_logits, int64_t ldg, int W, int C, float lam, float mu, float* p_change,
                            float* jump_abs, float* p_flip, int32_t* top_from, int32_t* top_to, float* p_top, float* xi, float* log_z, float* workspace, void* stream);

/* The gated read-outs of a STREAM at a fixed lag (ABI v25): sf_track_stream_push and sf_track_pool_push with the chain over (offset class, synchronizable
 * flag) of sf_track_decode_gated / sf_track_posterior_gated.  Rows (l_t, z_t) arrive in order: l_t the offset logits (C), z_t the gate logits (2) of the start-aligned
 * gate window; E, T, lam, mu and the tie rules are those of the gated offline read-outs.  With path_t = sf_track_decode_gated's (cls_path, sync_path) and post_t, psync_t =
 * sf_track_posterior_gated's post and p_sync on rows 0 .. t, a push that brings the stream to t + 1 rows returns
 *     cls_raw, conf_raw, sync_raw (n)                         per new row, as sf_track_decode_gated gives them
 *     (cls_lag[w], sync_lag[w]) = path_{w+lag}[w]             for every window w whose row w + lag arrived in this push; conf_lag[w] the softmax probability of cls_lag[w]
 *                                                             in offset row w.  Committed once, never revised
 *     post_lag[w, :] = post_{w+lag}[w, :], p_sync_lag[w] = psync_{w+lag}[w]      (posterior) with cls_post_lag, conf_post_lag, offset_mean_lag from post_lag
 *     cls_tail, sync_tail, conf_tail (n_tail)                 path_t on the windows not yet committed
 *     log_z[0]                                                (posterior) that of the prefix 0 .. t
 * final, the counts n_commit / n_tail, rows_done, the block-of-size-0 rule and the launches (row statistics, the two causal scans side by side, one wavefront per
 * committed window plus one for the tail, the rings' update) are sf_track_stream_push's; lag >= t gives the gated offline read-outs bit for bit at the final push.
 * state: one opaque device buffer per stream of sf_track_stream_gated_bytes(C, lag, posterior) bytes (a multiple of 16, independent of rows_done), read only when
 * rows_done > 0.  Layout (TrackGatedStreamLayout in sf_track.hip): [double: subtracted maxima][int32: end state, pad][Viterbi scores: 64 floats][posterior: forward
 * vector: 64 floats][offset logits ring (lag, C) fp32][gate logits ring (lag, 2) fp32][posterior: a ring (lag, 2C) fp32][back pointer ring (lag, 2C) bytes]; row r lies
 * in slot r % lag.  The emission is recomputed from the two logit rings as the offline scans compute it; no emission ring is kept.  A gated state is not an ungated one:
 * the two kinds of push do not mix on one buffer.  workspace: sf_track_stream_gated_workspace_bytes(C, n, posterior) bytes, dead after the push.
 * sf_track_pool_push_gated: the same for n_active streams in one call; the table, its validation, the packed outputs and the block-to-work mapping are
 * sf_track_pool_push's, unchanged; the gate rows of a stream are rows [row0, row0 + n) of gate_logits (total_rows, 2), row stride ldg >= 2; sync_raw is indexed like
 * cls_raw, sync_lag / p_sync_lag like cls_lag, sync_tail like cls_tail.  workspace: sf_track_pool_gated_workspace_bytes(C, total_rows, posterior).
 * 2 <= C <= 32, 0 <= lag <= 255, n (total_rows) <= 2^20, lam and mu finite and >= 0, ldl >= C, ldg >= 2, ldp >= C; -1 and a message before anything is launched for
 * everything sf_track_stream_push / sf_track_pool_push and the gated offline launchers refuse.  Nothing is read back, allocated or synchronised: a single-stream push
 * can be captured in a graph (rows_done is part of the capture).  Non-finite rows: values unspecified, every index written inside [0, C) / {0, 1}. */
int sf_track_stream_gated_bytes(int C, int lag, int posterior);
int sf_track_stream_gated_workspace_bytes(int C, int n, int posterior);
int sf_track_stream_push_gated(void* state, int C, int lag, int posterior, int64_t rows_done, const float* logits, int64_t ldl, const float* gate_logits, int64_t ldg,
                               int n, float lam, float mu, const float* grid, int final, int32_t* cls_raw, float* conf_raw, float* sync_raw, int32_t* cls_lag,
                               int32_t* sync_lag, float* conf_lag, float* post_lag, int64_t ldp, float* p_sync_lag, int32_t* cls_post_lag, float* conf_post_lag,
                               float* offset_mean_lag, int32_t* cls_tail, int32_t* sync_tail, float* conf_tail, float* log_z, void* workspace, void* stream);
int sf_track_pool_gated_workspace_bytes(int C, int total_rows, int posterior);
int sf_track_pool_push_gated(void* states, int64_t state_stride, int n_slots, int C, int lag, int posterior, const int64_t* table_host, const int64_t* table_dev,
                             int n_active, const float* logits, int64_t ldl, const float* gate_logits, int64_t ldg, int total_rows, float lam, float mu,
                             const float* grid, int32_t* cls_raw, float* conf_raw, float* sync_raw, int32_t* cls_lag, int32_t* sync_lag, float* conf_lag, float* post_lag,
                             int64_t ldp, float* p_sync_lag, int32_t* cls_post_lag, float* conf_post_lag, float* offset_mean_lag, int32_t* cls_tail, int32_t* sync_tail,
                             float* conf_tail, float* log_z, void* workspace, void* stream);

/* The WIDE chain (additions under ABI v25): the whole-recording read-outs over S states at unevenly spaced positions - a search over D lags x C classes
 * beyond the class grid.  logits (W, D, C) fp32: window w paired at lag d, row stride ldw >= (D - 1) ldd + C, lag stride ldd >= C, unit class stride; gate_logits
 * (W, D, 2) fp32 with strides ldgw, ldgd likewise, or NULL.  State s (in the caller's order) reads the pair state_src[s] = d * C + c (all distinct, inside [0, D C)) and
 * stands at pos[s] (fp32, finite, non-decreasing: class steps).  Both tables come twice, as sf_track_pool_push takes its table: the HOST copies are validated, the
 * DEVICE copies are what the kernels read.
 *     e[w, s] = logits[w, d, c] - lse_c logits[w, d, .] + g[w, d],     g = -softplus(z0 - z1) (log sigmoid of the gate's margin), 0 without a gate
 * sf_track_decode_wide:  s_0 = e[0];  s_w[c] = max_p (s_{w-1}[p] - lam |pos[p] - pos[c]|) + e[w, c], the lowest p among the maximisers, the end state the lowest argmax,
 *   scores renormalised by a maximum every step.  state_raw[w] = the lowest argmax of e[w, .], conf_raw[w] its softmax probability over all S states; state_path the
 *   path, conf_path that softmax probability at the path's state.  For the path and these probabilities e is taken up to the row constant max_d (g - lse)[w, d], which
 *   changes none of them and keeps the scan exact where it can be (one lag, or rows that agree across the lags: e = the logit).
 * sf_track_posterior_wide:  the recurrences of sf_track_posterior with |p - c| replaced by |pos[p] - pos[c]|: post (W, S) (row stride ldp >= S), state_post / conf_post
 *   its argmax (lowest state on ties) and value, offset_mean[w] = sum_s post[w, s] off[s] (off (S,) fp32 on the device: the states' offsets in seconds), p_lag (W, D)
 *   dense: the sum of post over each lag's states, log_z[0] (<= W log D without a gate, with equality at lam = 0: every window's emissions sum to D over the states).  A -inf logit masks its state.
 * Both: 2 <= S <= 1024, 2 <= C <= 64, 1 <= D <= 1024, S <= D C, lam finite and >= 0; -1 and a message before the device is touched for these, a stride below its
 * bound, a pos that is not finite and ascending, a state_src out of range or repeated, a null pointer when W > 0.  W == 0 returns 0 and writes nothing.  Caller's
 * stream, nothing allocated, read back or synchronised, no atomics: the same bits eager and under graph replay.  workspace: sf_track_wide_workspace_bytes(W, D, S,
 * posterior, &bytes) bytes (posterior = 0 for the decode entry), 16-byte aligned, caller-owned, dead after the call; the back pointers in it are uint16 (W, S).
 * One workgroup of ceil(S / 64) wavefronts, thread s = state s; a step costs O(S) over all states (two scans under a decayed operator, 16 LDS slots and one barrier
 * across the wavefronts).  NaN and +inf: values unspecified, every index written inside [0, S). */
int sf_track_wide_workspace_bytes(int W, int D, int S, int posterior, int64_t* bytes);
int sf_track_decode_wide(const float* logits, int64_t ldw, int64_t ldd, const float* gate_logits, int64_t ldgw, int64_t ldgd, int W, int D, int C, int S,
                         const int32_t* state_src_host, const float* pos_host, const int32_t* state_src_dev, const float* pos_dev, float lam, int32_t* state_raw,
                         float* conf_raw, int32_t* state_path, float* conf_path, void* workspace, void* stream);
int sf_track_posterior_wide(const float* logits, int64_t ldw, int64_t ldd, const float* gate_logits, int64_t ldgw, int64_t ldgd, int W, int D, int C, int S,
                            const int32_t* state_src_host, const float* pos_host, const int32_t* state_src_dev, const float* pos_dev, float lam, const float* off,
                            float* post, int64_t ldp, int32_t* state_post, float* conf_post, float* offset_mean, float* p_lag, float* log_z, void* workspace,
                            void* stream);

/* ---- Ingest of a decoded recording at its native frame rate, size and sample rate: the step the reference leaves to an ffmpeg subprocess in front of its code
 * (example.py:16-53: fps=25, short side 256, even dimensions, -ar 16000), plus the centre 224 crop of RGBSpatialCrop (dataset/transforms.py:68-95).  The host
 * computes the geometry (synchformer_amd.ingest) into DEVICE tables.
 * sf_ingest_video: raw uint8, element (frame f, channel c, row y, column x) at byte f * stride_frame + c * stride_channel + y * stride_row + x * stride_col
 *   (planar (T, 3, H, W): H W, then W, 1; decoder-style (T, H, W, 3): 1, 3 W, 3), n_src frames of H x W.  Output frame j < T_out is source frame frame_table[j]
 *   (int32; repeats and skips allowed, clamped into [0, n_src)), resampled by the separable filter
 *       out[c, r, x] = sum_i y_w[r, i] * sum_k x_w[x, k] * raw[c, y_first[r] + i, x_first[x] + k]        (r, x < 224; horizontal pass first, fp32)
 *   rounded half to even, clamped to [0, 255], written uint8 planar (T_out, 3, 224, 224), 4-byte aligned: the input of sf_im2col_video_clips.  y_first / x_first
 *   int32 (224), y_w / x_w fp32 (224, taps), rows zero-padded to taps: the antialiased bicubic tables of F.interpolate(mode='bicubic', antialias=True), already
 *   sliced to the crop, so the 256-side picture never exists.  Taps that fall outside the picture are skipped (they carry the zero padding); x_first[0] is the lowest
 *   column read, x_first is expected non-decreasing.  1 <= taps <= 35 (a short side up to 2160 at resize side 256), T_out <= 65535 per launch, W + taps_x <= 5108 (four
 *   source rows are staged at a time); -1 otherwise.  One launch; the launcher cannot read the tables: the kernel bounds every address.
 * sf_resample_wave: x (ch, len) fp32 (SF_F32) or int16 PCM (SF_I16, scaled by 1 / 32768), channel stride ld elements, 1 <= ch <= 8 averaged to mono on read ->
 *   y (len_out) fp32, len_out <= ceil(n len / o):  y[p + n q] = sum_{i < taps} xpad[q o + i] * kernel[p, i],  xpad[m] = x[m - width], 0 outside [0, len): the
 *   polyphase windowed-sinc bank of torchaudio.functional.resample (kernel fp32 (n, taps), taps = 2 width + o; ingest.resample_kernel).  The filter is centred: no
 *   delay.  ((255 / n) + 1) o + taps <= 12288 (the input span of 256 outputs is staged in LDS).  fp32 accumulation, taps in ascending order.  One launch. */
int sf_ingest_video(const uint8_t* raw, int64_t stride_frame, int64_t stride_channel, int64_t stride_row, int64_t stride_col, int n_src, int H, int W,
                    const int32_t* frame_table, const int32_t* y_first, const float* y_w, int taps_y, const int32_t* x_first, const float* x_w, int taps_x,
                    uint8_t* out, int T_out, void* stream);
int sf_resample_wave(const void* x, int dtype, int ch, int64_t ld, int64_t len, const float* kernel, int n, int taps, int o, int width, float* y, int64_t len_out,
                     void* stream);

/* sf_resample_wave for several audio PROGRAMMES of one multi-channel wave (an SDI / contribution feed: up to 16 embedded channels, organised as a stereo main mix,
 * a second language, audio description, .. - each checked against the picture on its own).  Input element (channel c, sample s) at x + c * stride_ch + s * stride_s,
 * in elements, both strides >= 1 (planar (ch, len): stride_ch = ld, stride_s = 1; interleaved (len, ch): stride_ch = 1, stride_s = the frame stride >= ch); dtype
 * SF_F32, SF_I16 (scaled by 2^-15) or SF_I32 (the C cast to fp32, times 2^-31: 24-bit audio left-justified in 32 bits, ffmpeg's s32); 1 <= ch <= 16.  mix fp32
 * (P, ch) row-major in DEVICE memory, 1 <= P <= 8 per launch; y fp32 (P, len_out) at row stride ldy >= len_out, len_out <= ceil(n len / o):
 *       m_p[s] = fmaf(mix[p, ch - 1], xf[ch - 1, s], .. fmaf(mix[p, 0], xf[0, s], 0))     (c ascending; xf the scaled fp32 sample; 0 outside [0, len))
 *       y[p, r + n q] = sum_{i < taps} mpad_p[q o + i] * kernel[r, i],  mpad_p[m] = m_p[m - width]      (i ascending, fmaf: sf_resample_wave's rule, the same bank,
 *   centring and zero padding).  Zero weights are multiplied like any other: no skipping.  One workgroup makes 256 consecutive outputs of all P programmes: the
 *   tile's input span is read from memory once, mixed into P fp32 rows in LDS, and each lane walks its phase's taps P times.  The rows take
 *   P (((255 / n) + 1) o + taps) <= 16384 floats (64 KiB of LDS): P = 8 at 8, 16, 22.05, 32, 44.1, 48 and 96 kHz -> 16 kHz; a caller with more programmes, or a
 *   longer span, launches several times.  -1 with a message, before any launch: an unknown dtype, ch or P out of range, strides below 1, len_out above
 *   ceil(n len / o), ldy < len_out, the LDS limit, null pointers with len_out > 0.  The launcher cannot see the buffers' extents: the caller owns them. */
int sf_resample_wave_mix(const void* x, int dtype, int ch, int64_t stride_ch, int64_t stride_s, int64_t len, const float* mix, int P, const float* kernel, int n,
                         int taps, int o, int width, float* y, int64_t ldy, int64_t len_out, void* stream);

/* sf_ingest_video for 8-bit YUV 4:2:0 frames as decoders hand them out (NV12 surfaces, I420 / yuv420p arrays): the planes are resized first and the colour
 * conversion runs on the 224 x 224 result, the order of the reference's ffmpeg step (example.py:16-53 scales in YUV; RGB appears when the 256-side result is
 * decoded).  A frame of even H x W has luma Y (H x W) and chroma U, V (H/2 x W/2 each); with base = raw + f * stride_frame,
 *       Y[y, x] = base[y * stride_row + x],   U[y, x] = base[u_off + y * stride_crow + x * stride_ccol],   V[y, x] = base[v_off + y * stride_crow + x * stride_ccol]
 *   (NV12 at row pitch P: u_off = P H, v_off = u_off + 1, stride_crow = P, stride_ccol = 2;  I420 with contiguous rows: u_off = H W, v_off = H W 5 / 4,
 *   stride_crow = W / 2, stride_ccol = 1).  For output frame j < T_out (source frame frame_table[j], clamped into [0, n_src)) and r, x < 224:
 *       Yr = sum_i y_w[r, i]  * sum_k x_w[x, k]  * Y[y_first[r] + i,  x_first[x] + k]          luma tables: those of sf_ingest_video (H -> Hr, W -> Wr)
 *       Ur = sum_i cy_w[r, i] * sum_k cx_w[x, k] * U[cy_first[r] + i, cx_first[x] + k]         chroma tables: H/2 -> Hr, W/2 -> Wr, sliced at the SAME crop origin;
 *       Vr = the same on V                                                                     chroma is an (H/2, W/2) image under align_corners=False (centre siting;
 *                                                                                              left / top-left siting: tables built with shift=0.25, see below)
 *       out[c, r, x] = clamp(round_half_even(M[c][0] (Yr - o[0]) + M[c][1] (Ur - o[1]) + M[c][2] (Vr - o[2])), 0, 255)
 *   fp32, horizontal pass first, taps ascending, nothing rounded between the resize and the conversion; uint8 planar (T_out, 3, 224, 224), 4-byte aligned.
 *   csc: 12 floats in HOST memory, M row-major (rows R, G, B; columns Y, U, V) then o; they travel as kernel arguments (synchformer_amd.ingest.csc_matrix).
 *   When v_off == u_off + 1 and stride_ccol == 2 the interleaved chroma rows are fetched once and split in registers.  Taps outside a plane are skipped.
 *   -1 on: odd H or W, taps outside 1 .. 35 in any of the four tables, stride_ccol < 1, negative strides or offsets, a row too wide to stage (W + taps_x above
 *   ~5100 or W / 2 + taps_cx above ~2550), T_out outside 0 .. 65535, a null pointer, out not 4-byte aligned.  T_out == 0 launches nothing.  One launch. */
int sf_ingest_video_yuv(const uint8_t* raw, int64_t stride_frame, int64_t stride_row, int64_t u_off, int64_t v_off, int64_t stride_crow, int64_t stride_ccol,
                        int n_src, int H, int W, const int32_t* frame_table, const int32_t* y_first, const float* y_w, int taps_y, const int32_t* x_first,
                        const float* x_w, int taps_x, const int32_t* cy_first, const float* cy_w, int taps_cy, const int32_t* cx_first, const float* cx_w,
                        int taps_cx, const float* csc, uint8_t* out, int T_out, void* stream);

/* sf_ingest_video_yuv for 10-bit YUV 4:2:0 frames in 16-bit little-endian samples (P010 surfaces of hardware decoders, yuv420p10le arrays of libav / PyAV).
 * raw is 2-byte aligned; stride_frame, stride_row, u_off, v_off, stride_crow and stride_ccol are in BYTES and even; the sample value is
 *       v = (word >> shift) & 1023                  (P010: shift 6, the sample sits in the high ten bits; yuv420p10le: shift 0), so stray bits never leave the range;
 *   (P010 at a row pitch of P bytes: u_off = P H, v_off = u_off + 2, stride_crow = P, stride_ccol = 4;  yuv420p10le with contiguous rows: u_off = 2 H W,
 *   v_off = 2 H W 5 / 4, stride_crow = W, stride_ccol = 2).  Everything else is sf_ingest_video_yuv's definition on the 10-bit scale: the same tables, the same
 *   order of operations (fp32, horizontal pass first, taps ascending, fused multiply-adds, nothing rounded before the matrix), csc = M and o on the 10-bit scale
 *   (synchformer_amd.ingest.csc_matrix(bit_depth=10): limited range M = M8 / 4, o = (64, 512, 512)), output uint8 planar (T_out, 3, 224, 224).  Frames that hold
 *   4 v8 give, bit for bit, what sf_ingest_video_yuv gives on v8.  Chroma siting is in the chroma tables (aa_bicubic_table(shift=0.25)), for this entry and for the
 *   8-bit one alike.  When v_off == u_off + 2 and stride_ccol == 4 the interleaved chroma rows are fetched once (16 bytes per four columns) and split in registers.
 *   Serves every width sf_ingest_video_yuv serves (four 16-bit rows of a 3840-wide plane at 35 taps take ~68 KiB of LDS: the kernel raises its dynamic-LDS limit).
 *   -1 on: everything sf_ingest_video_yuv refuses, an odd stride or offset, raw not 2-byte aligned, stride_ccol < 2, shift outside 0 .. 6.  One launch. */
int sf_ingest_video_yuv16(const uint16_t* raw, int64_t stride_frame, int64_t stride_row, int64_t u_off, int64_t v_off, int64_t stride_crow, int64_t stride_ccol,
                          int shift, int n_src, int H, int W, const int32_t* frame_table, const int32_t* y_first, const float* y_w, int taps_y,
                          const int32_t* x_first, const float* x_w, int taps_x, const int32_t* cy_first, const float* cy_w, int taps_cy, const int32_t* cx_first,
                          const float* cx_w, int taps_cx, const float* csc, uint8_t* out, int T_out, void* stream);

/* The general form of sf_ingest_video_yuv and sf_ingest_video_yuv16 (ABI v21): three planes of 1-byte or 2-byte samples at any offsets and strides,
 * chroma planes of Hc x Wc - 4:2:2 as capture cards, mezzanine codecs and hardware surfaces hand it out (uyvy422, yuyv422, yuv422p, nv16, yuv422p10le, p210, y210),
 * the four 4:2:0 layouts of the two entries above, 4:4:4 planar.  With base = raw + f * stride_frame (all strides and offsets in BYTES),
 *       Y[y, x] = base[y_off + y * stride_row  + x * stride_col]       y < H,  x < W
 *       U[y, x] = base[u_off + y * stride_crow + x * stride_ccol]      y < Hc, x < Wc       (V: v_off)
 *       sample  = bytes_per_sample == 1 ? byte : (word >> shift) & 1023
 *   and from there sf_ingest_video_yuv's definition unchanged: the luma tables map H -> Hr and W -> Wr, the chroma tables Hc -> Hr and Wc -> Wr, sliced at the same
 *   crop origin; fp32, horizontal pass first, taps ascending, fused multiply-adds, nothing rounded before the matrix; out = clamp(round_half_even(M (yuv - o)), 0,
 *   255), uint8 planar (T_out, 3, 224, 224).  On a layout the two entries above serve, the output is theirs bit for bit.  With P the row pitch in bytes:
 *       format       bytes  y_off  stride_col  u_off  v_off     stride_crow  stride_ccol  Hc x Wc    shift
 *       uyvy422      1      1      2           0      2         P            4            H x W/2    -
 *       yuyv422      1      0      2           1      3         P            4            H x W/2    -
 *       yuv422p      1      0      1           H W    H W 3/2   W/2          1            H x W/2    -         (contiguous)
 *       nv16         1      0      1           P H    P H + 1   P            2            H x W/2    -
 *       yuv422p10le  2      0      2           2 H W  3 H W     W            2            H x W/2    0         (contiguous)
 *       p210         2      0      2           P H    P H + 2   P            4            H x W/2    6
 *       y210         2      0      4           2      6         P            8            H x W/2    6         (words Y0 U Y1 V)
 *   Staging: interleaved chroma (v_off == u_off + bytes, stride_ccol == 2 bytes: NV12, NV16, P010, P210) is fetched once and split in registers, as in the entries
 *   above.  A packed row (stride_col == 2 bytes, stride_ccol == 4 bytes, v_off == u_off + 2 bytes, |y_off - u_off| == bytes, stride_crow == stride_row, Hc == H, W even,
 *   Wc == W / 2) is fetched as whole 4-sample macropixels with dword or 16-byte loads where the row is 4-byte aligned, once by the luma pass and once by the chroma
 *   pass.  Every other layout, unaligned rows and row ends take one load per sample.  Even H and W are NOT required: the caller's format decides.
 *   -1 before anything is launched on: everything the two entries above refuse (on the given Hc, Wc), bytes_per_sample outside {1, 2}, Hc outside 1 .. H, Wc outside
 *   1 .. W, stride_col or stride_ccol below bytes_per_sample, for 2-byte samples an odd stride or offset or raw not 2-byte aligned, shift outside 0 .. 6, a luma row or
 *   a pair of chroma rows too wide to stage (8-bit 4:4:4 at 3840 columns is).  T_out == 0 launches nothing.  One launch. */
int sf_ingest_video_yuv_planes(const void* raw, int bytes_per_sample, int64_t stride_frame, int64_t y_off, int64_t stride_row, int64_t stride_col, int64_t u_off,
                               int64_t v_off, int64_t stride_crow, int64_t stride_ccol, int shift, int n_src, int H, int W, int Hc, int Wc,
                               const int32_t* frame_table, const int32_t* y_first, const float* y_w, int taps_y, const int32_t* x_first, const float* x_w, int taps_x,
                               const int32_t* cy_first, const float* cy_w, int taps_cy, const int32_t* cx_first, const float* cx_w, int taps_cx, const float* csc,
                               uint8_t* out, int T_out, void* stream);

/* Interlaced recordings (ABI v22): n_src frames of even H x W ARE 2 n_src fields of H / 2 x W.  Field f is rows p, p + 2, .. of frame f >> 1 in every
 * plane, p = (f & 1) ^ bottom_first (bottom_first 0: top field first, 1: bottom field first).  The two entries are sf_ingest_video and sf_ingest_video_yuv_planes on
 * that field recording, with these changes: field_table holds FIELD indices (int32, clamped into [0, 2 n_src)); there are two vertical tables, y_first0 / y_w0 for
 * the fields of parity 0 and y_first1 / y_w1 for parity 1 (cy_*0 / cy_*1 likewise), of one tap count, mapping H / 2 field rows -> Hr with the field's rows placed where
 * they sit in the frame: aa_bicubic_table(H / 2, Hr, shift = 0.25 - p / 2) sliced to the crop (frame row 2 k + p has its centre at frame coordinate 2 k + p + 0.5,
 * which is field coordinate k + 0.5 + 0.25 - p / 2).  Per workgroup the kernel picks the field, moves every plane's base by p stride_row (chroma: p stride_crow) and
 * runs the progressive resize with doubled row strides, H / 2 rows and the tables of parity p: every address is bounded by the field's geometry, and packed rows
 * that the parity offset takes off the 4-byte grid take the per-sample loads.  No deinterlacing filter: one field is resized to the frame's target size.
 * sf_ingest_video_yuv_planes_fields takes layouts with full vertical chroma resolution (Hc == H: the 4:2:2 formats, 4:4:4 planar); interlaced 4:2:0 is out of scope.
 * -1 before anything is launched on: everything the progressive entry refuses, H odd or below 2, Hc != H, bottom_first outside {0, 1}, a null table of either
 * parity, n_src above 2^30 - 1; the LDS geometry is the progressive one at the field's tap counts.  T_out == 0 launches nothing.  One launch. */
int sf_ingest_video_fields(const uint8_t* raw, int64_t stride_frame, int64_t stride_channel, int64_t stride_row, int64_t stride_col, int n_src, int H, int W,
                           const int32_t* field_table, const int32_t* y_first0, const float* y_w0, const int32_t* y_first1, const float* y_w1, int taps_y,
                           const int32_t* x_first, const float* x_w, int taps_x, int bottom_first, uint8_t* out, int T_out, void* stream);
int sf_ingest_video_yuv_planes_fields(const void* raw, int bytes_per_sample, int64_t stride_frame, int64_t y_off, int64_t stride_row, int64_t stride_col, int64_t u_off,
                                      int64_t v_off, int64_t stride_crow, int64_t stride_ccol, int shift, int n_src, int H, int W, int Hc, int Wc,
                                      const int32_t* field_table, const int32_t* y_first0, const float* y_w0, const int32_t* y_first1, const float* y_w1, int taps_y,
                                      const int32_t* x_first, const float* x_w, int taps_x, const int32_t* cy_first0, const float* cy_w0, const int32_t* cy_first1,
                                      const float* cy_w1, int taps_cy, const int32_t* cx_first, const float* cx_w, int taps_cx, const float* csc, int bottom_first,
                                      uint8_t* out, int T_out, void* stream);

/* v210 frames (an addition under ABI v25): 10-bit 4:2:2 as SDI capture cards and QuickTime 'v210' deliver it.  A row of W pixels (W even) is the 10-bit
 * fields Cb0 Y0 Cr0 Y1 Cb1 Y2 Cr1 Y3 .. (the uyvy422 order); field F lies in little-endian 32-bit word F / 3 at bit 10 (F % 3), bits 30 - 31 are unused:
 *       Y [y, x] = (word[y][(2 x + 1) / 3] >> 10 ((2 x + 1) % 3)) & 1023        x < W            word[y] = raw + f * stride_frame + y * stride_row  (strides in BYTES)
 *       Cb[y, j] = (word[y][(4 j)     / 3] >> 10 ((4 j)     % 3)) & 1023        j < W / 2        Cr: field 4 j + 2
 *   A row occupies whole groups of four words (six pixels): stride_row >= 16 ceil(W / 6); the unused fields of a last partial group, the words between it and the
 *   pitch and bits 30 - 31 may hold anything and never influence the output.  From the unpacked samples on this is sf_ingest_video_yuv_planes on yuv422p10le (Hc = H,
 *   Wc = W / 2, shift 0, the 10-bit scale), and the output equals that entry's on the same samples bit for bit; the chroma rows take the luma vertical tables, so
 *   there is no cy_* argument.  An odd H is legal.  Rows are read as aligned dwords.
 *   -1 before anything is launched on: everything sf_ingest_video refuses about T_out, taps and out; n_src < 1, H < 1, W < 2 or odd; stride_row or stride_frame
 *   negative or not a multiple of 4; stride_row < 16 ceil(W / 6); raw not 4-byte aligned; a null pointer with T_out > 0; a row too wide to stage.  T_out == 0 launches
 *   nothing.  One launch.
 * sf_ingest_video_v210_fields: the same on an interlaced recording, as sf_ingest_video_yuv_planes_fields defines fields - field_table holds field indices, the
 *   rows of parity p start p stride_row in and are 2 stride_row apart, y_first0 / y_w0 and y_first1 / y_w1 are the vertical tables of the parities.  Additionally -1
 *   on: H odd or below 2, bottom_first outside {0, 1}, a null table of either parity, n_src above 2^30 - 1. */
int sf_ingest_video_v210(const void* raw, int64_t stride_frame, int64_t stride_row, int n_src, int H, int W, const int32_t* frame_table, const int32_t* y_first,
                         const float* y_w, int taps_y, const int32_t* x_first, const float* x_w, int taps_x, const int32_t* cx_first, const float* cx_w, int taps_cx,
                         const float* csc, uint8_t* out, int T_out, void* stream);
int sf_ingest_video_v210_fields(const void* raw, int64_t stride_frame, int64_t stride_row, int n_src, int H, int W, const int32_t* field_table,
                                const int32_t* y_first0, const float* y_w0, const int32_t* y_first1, const float* y_w1, int taps_y, const int32_t* x_first,
                                const float* x_w, int taps_x, const int32_t* cx_first, const float* cx_w, int taps_cx, const float* csc, int bottom_first, uint8_t* out,
                                int T_out, void* stream);

/* Backward of sf_attention for tiny groups (n_tok <= 8, head_dim 64: Motionformer time attention, vit_helper.py:343-344): same
 * addressing as the forward; dq | dk | dv rows of the group's tokens are written (=), the CLS key's dk | dv of every (seq, group) goes to
 * cls_part (n_seq * n_groups, 2 * heads * 64) bf16 for sf_reduce_groups_bf16. */
int sf_attention_tiny_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t ld, const uint16_t* dO, int64_t lddo, uint16_t* dq,
                          uint16_t* dk, uint16_t* dv, int64_t ldg, uint16_t* cls_part, int64_t n_seq, int64_t seq_rows, int n_groups, int row0,
                          int group_stride, int tok_stride, int n_tok, int cls_row, int heads, int head_dim, float scale, void* stream);

/* out[r] (=|+=) sum_c x[r, c] for a bf16 (rows, cols) matrix (cols % 8 == 0): bias gradients from the transposed gradient copy. */
int sf_rowsum_bf16(const uint16_t* x, int64_t ldx, int rows, int64_t cols, float* out, int accumulate, void* stream);

/* Fused backward of sf_attention for groups of up to 208 keys, head_dim 64 (Motionformer space attention, AST): same addressing and
 * outputs as sf_attention_tiny_bwd; scores / probabilities are recomputed, nothing but dq | dk | dv (and cls_part) touches HBM. */
int sf_attention_group_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t ld, const uint16_t* dO, int64_t lddo, uint16_t* dq,
                           uint16_t* dk, uint16_t* dv, int64_t ldg, uint16_t* cls_part, int64_t n_seq, int64_t seq_rows, int n_groups, int row0,
                           int group_stride, int tok_stride, int n_tok, int cls_row, int heads, int head_dim, float scale, void* stream);

/* sf_attention_group_bwd with the CLS QUERY's backward (sf_attention_cls_bwd's job: vit_helper.py:126, the CLS query attends every key of the sequence) in the same
 * launch: the CLS query rides as one more query row of every group, normalised with the forward's statistics cls_stats [n_seq][heads][2] = (m in the base-2 domain
 * incl. the scale, l) from sf_attention_cls_combine_stats, delta = <dO, o> from the forward's output row o[(seq * seq_rows + cls_row) * ldo + ...].  dk / dv (and
 * cls_part) then hold both contributions - no read-modify-write pass over them - and the CLS query's dq comes out as one partial row per group, dq_cls_part
 * (n_seq * n_groups, heads * 64) bf16: sf_reduce_groups_bf16 sums them into row cls_row of dq.  n_tok % 16 != 0 (a free query slot). */
int sf_attention_group_bwd_clsq(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t ld, const uint16_t* dO, int64_t lddo, uint16_t* dq,
                                uint16_t* dk, uint16_t* dv, int64_t ldg, uint16_t* cls_part, const float* cls_stats, const uint16_t* o, int64_t ldo,
                                uint16_t* dq_cls_part, int64_t n_seq, int64_t seq_rows, int n_groups, int row0, int group_stride, int tok_stride, int n_tok,
                                int cls_row, int heads, int head_dim, float scale, void* stream);
/* The same for the tiny time groups (sf_attention_tiny_bwd; statistics from sf_attention_cls_stats = sf_attention_cls + stats[(seq * heads + head) * 2 + {0, 1}]). */
int sf_attention_tiny_bwd_clsq(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t ld, const uint16_t* dO, int64_t lddo, uint16_t* dq, uint16_t* dk,
                               uint16_t* dv, int64_t ldg, uint16_t* cls_part, const float* cls_stats, const uint16_t* o, int64_t ldo, uint16_t* dq_cls_part,
                               int64_t n_seq, int64_t seq_rows, int n_groups, int row0, int group_stride, int tok_stride, int n_tok, int cls_row, int heads,
                               int head_dim, float scale, void* stream);
int sf_attention_cls_stats(const uint16_t* q, int64_t q_seq_rows, int q_row, const uint16_t* k, const uint16_t* v, int64_t ld, int64_t kv_seq_rows, int kv_row0,
                           int n_keys, uint16_t* out, int64_t ldo, int64_t out_seq_rows, int out_row, int64_t n_seq, int heads, int head_dim, float scale,
                           float* stats, void* stream);
/* sf_attention_cls_combine that also writes the merged softmax statistics stats[(seq * heads + head) * 2 + {0, 1}] = (M, L) of the CLS query. */
int sf_attention_cls_combine_stats(const float* partials, int n_part, uint16_t* out, int64_t ldo, int64_t out_seq_rows, int out_row, int64_t n_seq, int heads,
                                   float* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYNCHFORMER_HIP_H */
