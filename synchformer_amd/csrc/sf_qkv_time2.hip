// Motionformer TIME attention fused into its qkv projection, round 4 (gfx950): sf_qkv_time_attention on the main loop that sf_qkv_space_attention runs (sf_qkv_tile.h).
//
// sf_qkv_time.hip (round 2/3) gives a workgroup 256 token rows x ONE head's q | k | v (192 features) with every wave on 32 rows x all 192 features, so that a wave ends
// with everything its 4 patches need: 28 KiB of LDS fragment reads per wave and 64-deep k-tile for 0.79 MFLOP - 224 KiB per k-tile and CU = 1792 cycles of the LDS port
// against 1546 cycles of MFMAs: the launch is bound by fragment reads (893 TFLOP/s).  This kernel takes the 192 x 384 tile of sf_qkv_tile.h - 2 x 4 waves of
// 96 x 96, 24 KiB of fragment reads per wave for 1.18 MFLOP; stages, pieces, the phase / vmcnt table and the work-item schedule are described there, once, for this
// kernel and sf_qkv_space.hip - and pays with an exchange of q | k | v through LDS before the attention, as the spatial kernel does.
//
//   * Work item = (sequence, PATCH BLOCK tb, HEAD PAIR).  A sequence's 196 patches are 8 blocks of 24 + 4 left over.  The GEMM tile is the block's 24 patches x their 8
//     frames = 192 token rows, frame-major (tile row R = 24 fr + pl <-> X row seq * 1569 + 1 + 196 fr + 24 tb + pl: eight runs of 24 contiguous rows, gathered by the
//     LDS-DMA source addresses - wave w loads frame w: the shared loop's XRUN = 196), x the q | k | v of two heads (384 features).  This kernel's side loads in front of
//     the loop: the bias (waves 0-5) and the 48 chunks of the CLS row's q | k | v (wave 7).  DividedAttention.forward with the '(b n) f d' groups
//     (vit_helper.py:97-150, :343-344): every patch attends [CLS key; its own 8 frames].
//   * Epilogue (1): accumulators (+ bias) -> bf16 -> LDS arrays K | V | Q per head, rows PATCH-major (row' = 8 pl + fr), 128-byte rows with the 16-byte chunks XOR-swizzled
//     by (pl + fr) & 7 - the lanes of a store (consecutive pl of one frame) and the rows of a 16-row fragment read (two patches x 8 frames) both spread over the banks.
//     The sequence's CLS q | k | v (from `side`, landed by LDS-DMA during the main loop) go to row 0 of three 16-row blocks per head (the rest of them zero).
//   * Epilogue (2): a 16-row tile of the arrays = 2 patches x 8 frames is one attention unit on v_mfma_f32_16x16x32_bf16, the arithmetic of attn_mfma_kernel
//     (sf_attention.hip): S^T = K Q^T against key tile {the unit's own 16 rows} and key tile {CLS block}, scores of the other patch and of the block's empty rows
//     masked to -inf, in-lane base-2 softmax, P V with ds_read_b64_tr_b16 V fragments.  24 units per item (2 heads x 12), three per wave, run stage by stage so that
//     their dependency chains overlap.  The CLS QUERY of the sequence (vit_helper.py:126: it attends every token) meets the item's 192 keys in eight pieces - wave w: head
//     w & 1, key tiles 3 (w >> 1) .. + 2 - each writing its softmax partial as record 4 tb + (w >> 1) of cls_partial [seq][head][33][66] (sf_attention_cls_partial's
//     records; sf_attention_cls_combine with n_part = 33 writes the CLS row of `out`).
//   * The 4 left-over patches of a sequence (tokens 192..195 of every frame: rows seq * 33 + 1 + 4 f + i of `side`, the buffer sf_qkv_space_attention takes) are a ninth,
//     GEMM-less item per (sequence, head pair): 32 array rows loaded from `side`, 4 patch units, and the CLS query's record 32 over these 32 keys AND the CLS key itself.
//   * persistent, one workgroup per CU; every XCD owns a contiguous range of (sequence, block) row tiles and sweeps it once per chunk of head pairs.
// Token masks: sf_qkv_time_attention2_masked (template parameter MASK: the key flags become the starting values of the score accumulators).
#include "sf_qkv_tile.h"
#include "../../include/synchformer_hip.h"

#define QT2_NP 196                       // patches per frame
#define QT2_TP 24                        // patches per GEMM tile
#define QT2_ROWS QKT_ROWS                // 24 patches x 8 frames
#ifndef QT2_ABL_HALF
#define QT2_ABL_HALF 0
#endif
#define QT2_ARR (QT2_ROWS * 128)         // one K / V / Q array: 192 rows of 128 B (24 KiB); the six arrays overlay the two operand stages exactly
#define QT2_CB_OFF (6 * QT2_ARR)         // 144 KiB: CLS blocks Kc[2] | Vc[2] | Qc[2], 16 rows of 128 B each, row 0 = the sequence's CLS k / v / q of the head, rows 1..15 zero
static_assert(QT2_CB_OFF + 6 * 2048 == QKT_BIAS_OFF, "the bias sits right behind the CLS blocks");
#define QT2_LAND_OFF (QKT_BIAS_OFF + 1536)         // 768 B: landing area of the CLS row's q | k | v of both heads (48 x 16 B, lane-linear)
// MX variant (fp8 towers): the k-tile's scale dwords need 2 x 2304 B next to two full operand stages - the six 2-KiB CLS blocks shrink to their only non-zero row each
// (CBX: 6 x 128 B) plus ONE shared zero row, rows 1..15 of a block being an address select, and the scales land where the blocks were
#define QT2_CBX_OFF QT2_CB_OFF                      // MX: row 0 of block b (K h0, K h1, V h0, V h1, Q h0, Q h1) at + b * 128
#define QT2_ZROW_OFF (QT2_CB_OFF + 6 * 128)         // MX: 128 zero bytes
#define QT2_SC_OFF (QT2_CB_OFF + 1024)              // MX: 145 KiB, where the k-tile's scale dwords land (two parities of QKT_SC_BYTES)
#define QT2_MASK_OFF (QT2_LAND_OFF + 768)           // MASK variant: one float per array row (patch-major, 192) + the CLS key at index 192: 0 = kept, -inf = masked
#define QT2_NPART 33                     // CLS-query records per (sequence, head): 4 per block (one per wave pair: 3 key tiles each) + 1 of the left-over item
#ifndef QT2_ABL
#define QT2_ABL 0                        // measurement builds (WRONG results): 1 no attention units, 2 no MFMAs in the main loop, 4 no CLS-query units, 8 no patch units, 16 no units in the left-over items, 32 no output stores
#endif

struct Qt2Args {
  const bf16_t* X; int64_t ldx;
  const bf16_t* W; int64_t ldw;
  const float* bias;
  const bf16_t* side; int64_t lds_;      // (n_seq * 33, 2304) bf16: row seq * 33 = the CLS row's q | k | v, row seq * 33 + 1 + 4 f + i = token 192 + i of frame f
  bf16_t* out; int64_t ldo;
  float* cls_part;                       // [n_seq][12][33][66]
  int64_t seq_rows;
  uint32_t n_rt;                         // n_seq * 9 row tiles: (sequence, block 0..7) and the left-over item 8
  uint32_t pair_chunk;                   // head pairs per sweep over an XCD's row tiles (divides 6)
  float scale;
  uint32_t stagger;
  const uint8_t* key_keep = nullptr;     // MASK (template parameter): token flags, one byte per row of X; flag 0 = a masked KEY (for its patch's group and for the CLS query)
  // MX (template parameter): X / W are e4m3 BYTES (ldx / ldw in bytes) with stage-major E8M0 scale planes (one dword per row per 128 k, ldsx / ldsw bytes between planes);
  // the attention output leaves as bf16 `out` OR as MXFP8 (e4m3 bytes, row stride ldq, + E8M0 bytes in the scale planes [6][rows][4], splane bytes apart)
  const uint8_t* sX = nullptr; int64_t ldsx = 0;
  const uint8_t* sW = nullptr; int64_t ldsw = 0;
  uint8_t* out_q = nullptr; int64_t ldq = 0; uint8_t* out_s = nullptr; int64_t splane = 0;
};
// array row (patch-major: row = 8 pl + fr; also a CLS block's row 0..15), 16-byte chunk 0..7 -> byte offset; the chunk slot is XOR-swizzled by (pl + fr) & 7
__device__ __forceinline__ int qt2_arr_off(int row, int chunk) { return row * 128 + ((chunk ^ (((row >> 3) + row) & 7)) << 4); }

template <bool MASK, bool MX = false>
__device__ __forceinline__ void qkv_time2_attn_body(const Qt2Args& p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;                         // 2 x 4 waves, wave tile 96 token rows x 96 features

  const QktSchedule sched(p.n_rt, p.pair_chunk);                   // row tile = (sequence, patch block 0..7 | the left-over item 8)
  uint32_t t = sched.li;
  if (t >= sched.t_end) return;
  // optional start stagger (measurement: do the output-store bursts of 256 workgroups in lockstep cost more than a delayed start?): the groups of `hc` workgroups that share a
  // row tile start (group * 8 + xcd) * stagger * ~1.2 us apart
  for (uint32_t i = 0, n = ((sched.li / sched.hc) * 8u + sched.xcd) * p.stagger; i < n; ++i) __builtin_amdgcn_s_sleep(32);

  // tile row R = 24 fr + pl: the block's 24 patches in frame fr, XRUN = 196 rows of X further down per frame (wave w loads frame w)
  QktTile<MX, QT2_NP, QT2_SC_OFF, (QT2_ABL & 2) != 0> tile(smem, QktOperands{p.X, p.ldx, p.W, p.ldw, p.sX, p.ldsx, p.sW, p.ldsw, p.bias}, wave, lane);
  const uint32_t lds0 = tile.lds0;
  uint32_t cls_voff = 0;                                           // lane offset of the CLS row's LDS-DMA piece: re-derived for every item (not kept live across the attention)

  // the CLS blocks start as zeros; only their row 0 is ever written again
  for (int x = tid; x < (MX ? 1024 : 6 * 2048) / 16; x += 512) *reinterpret_cast<uint4*>(smem + QT2_CB_OFF + x * 16) = make_uint4(0u, 0u, 0u, 0u);
  sf_barrier();                                                   // (a left-over item writes row 0 of the blocks before its first barrier)

  const float sc2 = p.scale * 1.44269504088896f;                   // softmax in base 2
  uint32_t tcount = 0;
  // a CLS block's 16-byte chunk: block blk (0 K | 2 V | 4 Q) of head h, row 0..15 (only row 0 is ever non-zero).  bf16 kernel: six 2-KiB blocks in the arrays' swizzled
  // layout; MX kernel: row 0 of every block in CBX, rows 1..15 all the ONE zero row (an address select per lane)
  auto cb_ptr = [&](int blk, int h, int row, int chunk) -> const char* {
    if (!MX) return smem + QT2_CB_OFF + (blk + h) * 2048 + qt2_arr_off(row, chunk);
    return smem + (row == 0 ? QT2_CBX_OFF + (blk + h) * 128 : QT2_ZROW_OFF) + (chunk << 4);
  };

  for (;;) {
    uint32_t rt; int hp;
    sched.item(t, rt, hp);
    const int64_t seq = rt / 9u; const int tb = (int)(rt - (uint32_t)seq * 9u);
    const bool main_item = tb < 8;                                  // wave-uniform (workgroup-uniform)
    if (main_item) {
      const int dl = tile.begin_item(seq * p.seq_rows + 1 + (int64_t)tb * QT2_TP, hp);
      { const int ch = dl & 7, w3 = (dl >> 3) % 3, hd = (dl >> 3) / 3; cls_voff = (uint32_t)((w3 * QKT_D + hd * 64 + ch * 8) * 2); }   // wave 7, lanes 0..47: the CLS row's q | k | v chunk
      // ---- side loads, in front of the main loop's own pieces (the previous item's attention is over: barrier at the bottom of the loop): bias, the CLS row ----
      tile.issue_bias();
      if (wave == 7) {                                              // CLS row: chunk x = (hd * 3 + which) * 8 + ch, 48 chunks of 16 B
        if (lane < 48) sf_dma1(cls_voff, reinterpret_cast<const char*>(p.side + seq * 33 * p.lds_ + hp * 128), lds0 + QT2_LAND_OFF);
      }
      f32x16 acc[3][3];
      tile.project(acc);

      // ---- epilogue (1): accumulators -> bf16 -> the K | V | Q arrays (they overlay the operand stages), rows patch-major ------------------------------------
      {
        int etid = threadIdx.x;
        asm volatile("" : "+v"(etid));
        const int el31 = etid & 31, ehi = (etid & 63) >> 5;
        // MASK: the item's key flags -> additive score terms (0 / -inf) the S accumulators start from; the byte loads fly under the hand-over stores
        uint8_t kflag = 1;
        if (MASK && etid < QT2_ROWS + 1) {
          const int fr = etid / QT2_TP, pl = etid - fr * QT2_TP;
          kflag = etid == QT2_ROWS ? p.key_keep[seq * p.seq_rows] : p.key_keep[seq * p.seq_rows + 1 + (int64_t)fr * QT2_NP + tb * QT2_TP + pl];
        }
        int rowp[3];                                                // array row of this lane's token of row block i: tile row R = 24 fr + pl -> 8 pl + fr
#pragma unroll
        for (int i = 0; i < 3; ++i) { const int R = wm * 96 + i * 32 + el31, fr = R / QT2_TP; rowp[i] = (R - fr * QT2_TP) * 8 + fr; }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int cb = (wn * 3 + j) * 32;                         // first tile column of the block (wave-uniform)
          const int hd = cb / 192, within = cb - hd * 192, which = within >> 6, feat0 = within & 63;
          const int arr = hd * 3 * QT2_ARR + (which == 1 ? 0 : (which == 2 ? QT2_ARR : 2 * QT2_ARR));      // K | V | Q per head
#pragma unroll
          for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              uint2 w;
              w.x = pack_bf2(acc[j][i][g * 4 + 0], acc[j][i][g * 4 + 1]);
              w.y = pack_bf2(acc[j][i][g * 4 + 2], acc[j][i][g * 4 + 3]);
#if QT2_ABL_HALF   // measurement only (WRONG results): lanes l and l + 8 of a 16-lane store group share a 16-byte chunk slot - here they take different halves of it, which
                   // makes the hand-over stores conflict-free: what do the 2-way conflicts of the product layout cost?  (profiles/r06_attention_fabric.md)
              *reinterpret_cast<uint2*>(smem + arr + qt2_arr_off(rowp[i], (feat0 >> 3) + g) + (ehi ^ ((el31 >> 3) & 1)) * 8) = w;
#else
              *reinterpret_cast<uint2*>(smem + arr + qt2_arr_off(rowp[i], (feat0 >> 3) + g) + ehi * 8) = w;
#endif
            }
          }
        }
        if (etid < 48) {                                            // the CLS row: q -> Qc, k -> Kc, v -> Vc, row 0 of the head's block (row 0: chunk slot = chunk)
          const int ch = etid & 7, w3 = (etid >> 3) % 3, hd = (etid >> 3) / 3;
          const uint4 sv = *reinterpret_cast<const uint4*>(smem + QT2_LAND_OFF + etid * 16);
          *reinterpret_cast<uint4*>(const_cast<char*>(cb_ptr(w3 == 1 ? 0 : (w3 == 2 ? 2 : 4), hd, 0, ch))) = sv;
        }
        if (MASK && etid < QT2_ROWS + 1) {
          const int fr = etid / QT2_TP, pl = etid - fr * QT2_TP;
          reinterpret_cast<float*>(smem + QT2_MASK_OFF)[etid == QT2_ROWS ? QT2_ROWS : pl * 8 + fr] = kflag ? 0.f : -INFINITY;
        }
        sf_barrier();
      }
    } else {
      // ---- the left-over item: 4 patches x 8 frames of q | k | v of both heads from `side` -> array rows 0..31 (row = 8 i + f); the CLS row -> the blocks --------
      int stid = threadIdx.x;
      asm volatile("" : "+v"(stid));
      uint4 sv[3], cv = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int x = stid + e * 512, ch = x & 7, rr = (x >> 3) & 31, w3 = (x >> 8) % 3, hd = (x >> 8) / 3;
        sv[e] = *reinterpret_cast<const uint4*>(p.side + (seq * 33 + 1 + (rr & 7) * 4 + (rr >> 3)) * p.lds_ + w3 * QKT_D + (hp * 2 + hd) * 64 + ch * 8);
      }
      if (stid < 48) {
        const int ch = stid & 7, w3 = (stid >> 3) % 3, hd = (stid >> 3) / 3;
        cv = *reinterpret_cast<const uint4*>(p.side + seq * 33 * p.lds_ + w3 * QKT_D + (hp * 2 + hd) * 64 + ch * 8);
      }
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int x = stid + e * 512, ch = x & 7, rr = (x >> 3) & 31, w3 = (x >> 8) % 3, hd = (x >> 8) / 3;
        *reinterpret_cast<uint4*>(smem + hd * 3 * QT2_ARR + (w3 == 1 ? 0 : (w3 == 2 ? QT2_ARR : 2 * QT2_ARR)) + qt2_arr_off(rr, ch)) = sv[e];
      }
      if (stid < 48) {
        const int ch = stid & 7, w3 = (stid >> 3) % 3, hd = (stid >> 3) / 3;
        *reinterpret_cast<uint4*>(const_cast<char*>(cb_ptr(w3 == 1 ? 0 : (w3 == 2 ? 2 : 4), hd, 0, ch))) = cv;
      }
      if (MASK && stid >= 64 && stid < 64 + 33) {                   // rows 8 i + f = token 192 + i of frame f, and the CLS key
        const int r = stid - 64;
        const uint8_t kf = r == 32 ? p.key_keep[seq * p.seq_rows] : p.key_keep[seq * p.seq_rows + 1 + (int64_t)(r & 7) * QT2_NP + QT2_ROWS + (r >> 3)];
        reinterpret_cast<float*>(smem + QT2_MASK_OFF)[r == 32 ? QT2_ROWS : r] = kf ? 0.f : -INFINITY;
      }
      sf_barrier();
    }

    // ---- epilogue (2): the time attention of the item's patches and the CLS query's partial over the item's keys ------------------------------------------------
    if (!(QT2_ABL & 1)) {
      int atid = threadIdx.x;
      asm volatile("" : "+v"(atid));
      const int alane = atid & 63, fr_ = alane & 15, fg = alane >> 4;
      const int krow = fg * 4 + (fr_ >> 2), c1 = (fr_ & 3) >> 1, hb = (fr_ & 1) * 8;      // this lane's row / chunk / half of a ds_read_b64_tr_b16 V fragment
      const int64_t orow0 = seq * p.seq_rows + 1 + (main_item ? tb * QT2_TP : QT2_ROWS);  // out row of (frame 0, patch 0 of the item)
      // NU 16-row tiles (unit u: head u / 12, tile u % 12; a tile = 2 patches x 8 frames; keys = the same 16 rows, own patch only, + the CLS key), stage by stage over
      // the units: NU independent dependency chains (LDS read -> MFMA -> cross-lane max -> exp2 -> cross-lane sum -> MFMA -> store) overlap in one wave
      auto patch_units = [&](auto NUc, const int u0, const int ustep) {
        constexpr int NU = decltype(NUc)::value;
        const char* k_lds[NU];
        int qt[NU], hh_[NU];
        f32x4 s0[NU], s1[NU];
#pragma unroll
        for (int e = 0; e < NU; ++e) {
          const int u = u0 + e * ustep, h = u >= 12 ? 1 : 0;
          qt[e] = u - 12 * h;
          k_lds[e] = smem + h * 3 * QT2_ARR;
          hh_[e] = h;
          s0[e] = f32x4{0.f, 0.f, 0.f, 0.f}; s1[e] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (MASK) {                                               // rows fg * 4 + r of the unit's tile; row 0 of the CLS block = the CLS key
            const float4 mk = *reinterpret_cast<const float4*>(smem + QT2_MASK_OFF + (qt[e] * 16 + fg * 4) * 4);
            s0[e] = f32x4{mk.x, mk.y, mk.z, mk.w};
            s1[e][0] = reinterpret_cast<const float*>(smem + QT2_MASK_OFF)[QT2_ROWS];
          }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int e = 0; e < NU; ++e) {
            const bf16x8 qf = *reinterpret_cast<const bf16x8*>(k_lds[e] + 2 * QT2_ARR + qt2_arr_off(qt[e] * 16 + fr_, ks * 4 + fg));
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(k_lds[e] + qt2_arr_off(qt[e] * 16 + fr_, ks * 4 + fg));
            const bf16x8 cf = *reinterpret_cast<const bf16x8*>(cb_ptr(0, hh_[e], fr_, ks * 4 + fg));
            s0[e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, s0[e], 0, 0, 0);       // S^T: rows = keys fg * 4 + r of the tile, column = query fr_
            s1[e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cf, qf, s1[e], 0, 0, 0);       // row 0 (fg = 0, r = 0) = the CLS key
          }
        const bool own = (fg >> 1) == (fr_ >> 3);                   // key rows 4 fg .. + 3 belong to patch fg >> 1 of the tile, the query to patch fr_ >> 3
        float m[NU], l[NU], pc[NU];
#pragma unroll
        for (int e = 0; e < NU; ++e) {
          m[e] = fg == 0 ? s1[e][0] : -INFINITY;
#pragma unroll
          for (int r = 0; r < 4; ++r) { s0[e][r] = own ? s0[e][r] : -INFINITY; m[e] = fmaxf(m[e], s0[e][r]); }
        }
#pragma unroll
        for (int e = 0; e < NU; ++e) m[e] = fmaxf(m[e], __shfl_xor(m[e], 16, 64));
#pragma unroll
        for (int e = 0; e < NU; ++e) {                              // (finite without masks: every query sees its own 8 frames and the CLS key)
          m[e] = fmaxf(m[e], __shfl_xor(m[e], 32, 64)) * sc2;
          if (MASK && m[e] == -INFINITY) m[e] = 0.f;                // every key of the group masked: exp2(-inf) = 0 everywhere, l = 0 (a NaN row, as softmax over an all-masked row gives)
        }
#pragma unroll
        for (int e = 0; e < NU; ++e) {
          l[e] = 0.f;
#pragma unroll
          for (int r = 0; r < 4; ++r) { s0[e][r] = __builtin_amdgcn_exp2f(fmaf(s0[e][r], sc2, -m[e])); l[e] += s0[e][r]; }
          pc[e] = fg == 0 ? __builtin_amdgcn_exp2f(fmaf(s1[e][0], sc2, -m[e])) : 0.f;
          l[e] += pc[e];
        }
#pragma unroll
        for (int e = 0; e < NU; ++e) l[e] += __shfl_xor(l[e], 16, 64);
#pragma unroll
        for (int e = 0; e < NU; ++e) l[e] += __shfl_xor(l[e], 32, 64);
        f32x4 o[NU][4];
#pragma unroll
        for (int e = 0; e < NU; ++e) {
          union { bf16x8 v; uint32_t u[4]; } pa;                     // P^T fragment: k slots 8 fg .. + 3 = tile rows 4 fg .. + 3, + 4 .. + 7 = CLS block rows 4 fg .. + 3
          pa.u[0] = pack_bf2(s0[e][0], s0[e][1]); pa.u[1] = pack_bf2(s0[e][2], s0[e][3]);
          pa.u[2] = pack_bf2(pc[e], 0.f); pa.u[3] = 0u;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            union { bf16x8 v; qkt_s4 hh[2]; } vb;
            vb.hh[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((qkt_lds_s4*)(k_lds[e] + QT2_ARR + qt2_arr_off(qt[e] * 16 + krow, dt * 2 + c1) + hb));
            vb.hh[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((qkt_lds_s4*)(cb_ptr(2, hh_[e], krow, dt * 2 + c1) + hb));
            o[e][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vb.v, pa.v, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          }
        }
#ifndef QT2_OUT_LINES
#define QT2_OUT_LINES 1
#endif
#pragma unroll
        for (int e = 0; e < NU; ++e) {
          // query fr_ of the tile = (patch 2 qt + (fr_ >> 3), frame fr_ & 7); this lane holds dims dt * 16 + fg * 4 + r
          const int u = u0 + e * ustep, head = hp * 2 + (u >= 12 ? 1 : 0);
          const float linv = 1.0f / l[e];
          if (QT2_OUT_LINES) {
            // through the unit's own 16 Q rows (dead: only this unit read them): the accumulator layout would store 8 bytes per lane, 32 bytes apart - every 128-byte line
            // of `out` (one token, one head) in 16 pieces over 4 instructions; read back row-wise, 8 lanes x 16 bytes write one complete line
            char* qrows = const_cast<char*>(k_lds[e]) + 2 * QT2_ARR;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
              uint2 w;
              w.x = pack_bf2(o[e][dt][0] * linv, o[e][dt][1] * linv);
              w.y = pack_bf2(o[e][dt][2] * linv, o[e][dt][3] * linv);
              *reinterpret_cast<uint2*>(qrows + qt2_arr_off(qt[e] * 16 + fr_, dt * 2 + (fg >> 1)) + (fg & 1) * 8) = w;
            }
          } else {
            bf16_t* orow = p.out + (orow0 + (int64_t)(fr_ & 7) * QT2_NP + 2 * qt[e] + (fr_ >> 3)) * p.ldo + head * 64 + fg * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
              uint2 w;
              w.x = pack_bf2(o[e][dt][0] * linv, o[e][dt][1] * linv);
              w.y = pack_bf2(o[e][dt][2] * linv, o[e][dt][3] * linv);
              if (!(QT2_ABL & 32) || linv == 12345.678f) *reinterpret_cast<uint2*>(orow + dt * 16) = w;
            }
          }
        }
        if (QT2_OUT_LINES) {
#pragma unroll
          for (int e = 0; e < NU; ++e) {
            const int u = u0 + e * ustep, head = hp * 2 + (u >= 12 ? 1 : 0);
            const char* qrows = k_lds[e] + 2 * QT2_ARR;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const int rr = (alane >> 3) + 8 * j, ch = alane & 7;    // tile row rr = (patch 2 qt + j, frame alane >> 3)
              const uint4 w = *reinterpret_cast<const uint4*>(qrows + qt2_arr_off(qt[e] * 16 + rr, ch));
              if (MX && p.out_q) {
                // MXFP8 output (the A operand of the MX projection that follows), byte for byte sf_quantize_mxfp8 of the bf16 row: the head's 64 dims are two scale blocks,
                // block b = this lane's quad (chunks 4 b .. 4 b + 3); quantised from the bf16-rounded values the bf16 launch would have stored
                const int64_t row = orow0 + (int64_t)(alane >> 3) * QT2_NP + 2 * qt[e] + j;
                float fv[8];
                fv[0] = __uint_as_float(w.x << 16); fv[1] = __uint_as_float(w.x & 0xffff0000u); fv[2] = __uint_as_float(w.y << 16); fv[3] = __uint_as_float(w.y & 0xffff0000u);
                fv[4] = __uint_as_float(w.z << 16); fv[5] = __uint_as_float(w.z & 0xffff0000u); fv[6] = __uint_as_float(w.w << 16); fv[7] = __uint_as_float(w.w & 0xffff0000u);
                float amax = fmaxf(fmaxf(fmaxf(fabsf(fv[0]), fabsf(fv[1])), fmaxf(fabsf(fv[2]), fabsf(fv[3]))), fmaxf(fmaxf(fabsf(fv[4]), fabsf(fv[5])), fmaxf(fabsf(fv[6]), fabsf(fv[7]))));
                amax = fmaxf(amax, __shfl_xor(amax, 1, 64)); amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
                const int be = sf_mx_exp(amax);
                const float inv = sf_mx_inv(be);
                uint2 d; d.x = sf_fp8x4(fv, inv); d.y = sf_fp8x4(fv + 4, inv);
                const int be_hi = __shfl_xor(be, 4, 64);              // the head's other block (lanes ch and ch ^ 4 of the row)
                if (!(QT2_ABL & 32) || l[e] == 12345.678f) {
                  *reinterpret_cast<uint2*>(p.out_q + row * p.ldq + head * 64 + ch * 8) = d;
                  if (ch == 0) *reinterpret_cast<uint16_t*>(p.out_s + (int64_t)(head >> 1) * p.splane + row * 4 + (head & 1) * 2) = (uint16_t)(be | (be_hi << 8));
                }
                continue;
              }
              bf16_t* dst = p.out + (orow0 + (int64_t)(alane >> 3) * QT2_NP + 2 * qt[e] + j) * p.ldo + head * 64 + ch * 8;
#ifndef QT2_OUT_NT
#define QT2_OUT_NT 1   // the attention output with the nt hint: written once, read once by the next launch
#endif
              if (!(QT2_ABL & 32) || l[e] == 12345.678f) {
                typedef unsigned int qt2_u4 __attribute__((ext_vector_type(4)));
                const qt2_u4 wv = {w.x, w.y, w.z, w.w};
                if (QT2_OUT_NT) __builtin_nontemporal_store(wv, reinterpret_cast<qt2_u4*>(dst)); else *reinterpret_cast<qt2_u4*>(dst) = wv;
              }
            }
          }
        }
      };
      // the CLS query of the sequence against NK key tiles of the item from tile kt0 on (+ the CLS key itself when WITH_CLS): unnormalised record `rec` of head h
      auto cls_unit = [&](auto NKc, auto WCc, const int h, const int kt0, const int rec) {
        constexpr int NK = decltype(NKc)::value;
        constexpr bool WITH_CLS = decltype(WCc)::value != 0;
        constexpr int NKT = NK + (WITH_CLS ? 1 : 0);
        const int head = hp * 2 + h;
        const char* k_lds = smem + h * 3 * QT2_ARR;
        const char* v_lds = k_lds + QT2_ARR;
        bf16x8 qf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(cb_ptr(4, h, fr_, ks * 4 + fg));      // column 0 = the CLS query (columns 1..15: zero rows)
        f32x4 s[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
          s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (MASK) {
            if (kt < NK) { const float4 mk = *reinterpret_cast<const float4*>(smem + QT2_MASK_OFF + ((kt0 + kt) * 16 + fg * 4) * 4); s[kt] = f32x4{mk.x, mk.y, mk.z, mk.w}; }
            else s[kt][0] = reinterpret_cast<const float*>(smem + QT2_MASK_OFF)[QT2_ROWS];
          }
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 kf = kt < NK ? *reinterpret_cast<const bf16x8*>(k_lds + qt2_arr_off((kt0 + kt) * 16 + fr_, ks * 4 + fg))
                                      : *reinterpret_cast<const bf16x8*>(cb_ptr(0, h, fr_, ks * 4 + fg));
            s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s[kt], 0, 0, 0);
          }
        }
        if (WITH_CLS) {                                             // of the CLS block only row 0 is a key
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (fg != 0 || r != 0) s[NKT - 1][r] = -INFINITY;
        }
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) m = fmaxf(m, s[kt][r]);
        m = fmaxf(m, __shfl_xor(m, 16, 64)); m = fmaxf(m, __shfl_xor(m, 32, 64));
        const float msc = m * sc2;
        const float msafe = (MASK && m == -INFINITY) ? 0.f : msc;   // every key of the record masked: m = -inf, l = 0 goes to the combine (as sf_attention_cls_partial_masked writes it)
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) { const float e = __builtin_amdgcn_exp2f(fmaf(s[kt][r], sc2, -msafe)); s[kt][r] = e; l += e; }
        l += __shfl_xor(l, 16, 64); l += __shfl_xor(l, 32, 64);
        f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < (NKT + 1) / 2; ++kk) {
          union { bf16x8 v; uint32_t u[4]; } pa;
          pa.u[0] = pack_bf2(s[2 * kk][0], s[2 * kk][1]);
          pa.u[1] = pack_bf2(s[2 * kk][2], s[2 * kk][3]);
          if (2 * kk + 1 < NKT) {
            const int t1 = 2 * kk + 1 < NKT ? 2 * kk + 1 : 0;
            pa.u[2] = pack_bf2(s[t1][0], s[t1][1]);
            pa.u[3] = pack_bf2(s[t1][2], s[t1][3]);
          } else { pa.u[2] = 0u; pa.u[3] = 0u; }
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            union { bf16x8 v; qkt_s4 hh[2]; } vb;
            const int ta = 2 * kk, tb_ = 2 * kk + 1;
            vb.hh[0] = ta < NK ? __builtin_amdgcn_ds_read_tr16_b64_v4i16((qkt_lds_s4*)(v_lds + qt2_arr_off((kt0 + ta) * 16 + krow, dt * 2 + c1) + hb))
                               : __builtin_amdgcn_ds_read_tr16_b64_v4i16((qkt_lds_s4*)(cb_ptr(2, h, krow, dt * 2 + c1) + hb));
            vb.hh[1] = qkt_s4{0, 0, 0, 0};
            if (tb_ < NKT) vb.hh[1] = tb_ < NK ? __builtin_amdgcn_ds_read_tr16_b64_v4i16((qkt_lds_s4*)(v_lds + qt2_arr_off((kt0 + tb_) * 16 + krow, dt * 2 + c1) + hb))
                                               : __builtin_amdgcn_ds_read_tr16_b64_v4i16((qkt_lds_s4*)(cb_ptr(2, h, krow, dt * 2 + c1) + hb));
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vb.v, pa.v, o[dt], 0, 0, 0);
          }
        }
        if (fr_ == 0) {                                             // column 0 = the CLS query
          float* part = p.cls_part + ((seq * 12 + head) * QT2_NPART + rec) * 66;
          if (fg == 0) { part[0] = msc; part[1] = l; }
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[2 + dt * 16 + fg * 4 + r] = o[dt][r];
        }
      };
      const int wr = (wave + (int)tcount) & 7;                      // rotate the roles over the SIMDs from item to item (wave-uniform)
      if (main_item) {
        // every wave: three of the 24 patch units (wr, wr + 8, wr + 16) and a quarter of one head's CLS-query work (key tiles 3 q .. 3 q + 2 -> record 4 tb + q)
        if (!(QT2_ABL & 8)) patch_units(sf_ic<3>{}, wr, 8);
        if (!(QT2_ABL & 4)) cls_unit(sf_ic<3>{}, sf_ic<0>{}, wr & 1, 3 * (wr >> 1), tb * 4 + (wr >> 1));
      } else if (!(QT2_ABL & 16)) {
        if (wr < 2) cls_unit(sf_ic<2>{}, sf_ic<1>{}, wr, 0, 32);
        else if (wr < 6) { const int u = (wr - 2) & 1; patch_units(sf_ic<1>{}, ((wr - 2) >> 1) * 12 + u, 0); }
      }
    }
    sf_barrier();                                                  // every wave is out of the attention arrays: the next item's operands may land
    t += sched.step;
    ++tcount;
    if (t >= sched.t_end) break;
  }
}

__global__ __launch_bounds__(512, 2) void qkv_time2_attn_kernel(Qt2Args p) { qkv_time2_attn_body<false>(p); }
__global__ __launch_bounds__(512, 2) void qkv_time2_attn_masked_kernel(Qt2Args p) { qkv_time2_attn_body<true>(p); }
__global__ __launch_bounds__(512, 2) void qkv_time2_attn_mx_kernel(Qt2Args p) { qkv_time2_attn_body<false, true>(p); }

// X (n_seq * 1569, 768) bf16 = norm3(x), rows [CLS; frame-major patches] per sequence; W (2304, 768) bf16 = timeattn.qkv.weight, bias 2304 fp32 or NULL; side
// (n_seq * 33, 2304) bf16 = the same projection of [the CLS row; per frame f its tokens 192 .. 195] (row seq * 33, rows seq * 33 + 1 + 4 f + i) - the buffer layout of
// sf_qkv_space_attention; out (rows as X, 768) bf16: the PATCH rows are written (row 0 of every sequence comes from sf_attention_cls_combine on cls_partial
// [n_seq][12][33][66] fp32, n_part = 33).  out must not alias X.  Reference: vit_helper.py:97-150 with the '(b n) f d' groups of :343-344, 12 heads x 64, q scaled by `scale`.
static const QktLaunch QT2_BF16 = {"sf_qkv_time_attention2", "196 patches per frame", "a sequence", 1 + 8 * QT2_NP, 9, false};
static const QktLaunch QT2_MX = {"sf_qkv_time_attention2_mx", "196 patches per frame", "a sequence", 1 + 8 * QT2_NP, 9, true};

static int qt2_launch_bf16(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias, const uint16_t* side, int64_t lds_,
                           uint16_t* out, int64_t ldo, float* cls_partial, int64_t n_seq, int n_tok, float scale, const uint8_t* key_keep, void* stream) {
  Qt2Args a;
  a.X = X; a.ldx = ldx; a.W = W; a.ldw = ldw; a.bias = bias; a.side = side; a.lds_ = lds_; a.out = out; a.ldo = ldo; a.cls_part = cls_partial;
  a.scale = scale; a.key_keep = key_keep;
  static const int env_hc = qkt_env_pair_chunk("SF_QT2_PAIR_CHUNK");
  a.pair_chunk = (uint32_t)env_hc;
  static const int env_st = std::max(sf_env_int("SF_QT2_STAGGER", 0), 0);
  a.stagger = (uint32_t)env_st;
  return qkt_launch(QT2_BF16, key_keep ? qkv_time2_attn_masked_kernel : qkv_time2_attn_kernel, a, n_seq, n_tok, stream);
}
extern "C" int sf_qkv_time_attention2(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias, const uint16_t* side, int64_t lds_,
                                      uint16_t* out, int64_t ldo, float* cls_partial, int64_t n_seq, int n_tok, float scale, void* stream) {
  return qt2_launch_bf16(X, ldx, W, ldw, bias, side, lds_, out, ldo, cls_partial, n_seq, n_tok, scale, nullptr, stream);
}
// The same launch with TOKEN MASKS (Synchformer.forward(vis_mask=...), sync_model.py:72-80 -> vit_helper.py:107-141): key_keep holds one byte per row of X; a row with flag
// 0 is a masked KEY for the queries of its patch's 8-frame group and for the CLS query.  The flags become additive terms (0 / -inf) the score accumulators start from:
// an all-ones mask is bit-identical to sf_qkv_time_attention2.
extern "C" int sf_qkv_time_attention2_masked(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias, const uint16_t* side, int64_t lds_,
                                             uint16_t* out, int64_t ldo, float* cls_partial, int64_t n_seq, int n_tok, float scale, const uint8_t* key_keep, void* stream) {
  SF_CHECK_ARG(key_keep, "sf_qkv_time_attention2_masked: null key_keep (call sf_qkv_time_attention2 for an unmasked forward)");
  return qt2_launch_bf16(X, ldx, W, ldw, bias, side, lds_, out, ldo, cls_partial, n_seq, n_tok, scale, key_keep, stream);
}

// The same launch on MXFP8 operands (fp8 towers of the synchronizability fine-tune, round 5: the temporal half gets the schedule the spatial half got in round 4): X (rows,
// 768) e4m3 bytes with its stage-major scale planes sX (6 planes, ldsx bytes apart, one dword per row) - what sf_gemm_mx_res_ln768 / sf_layernorm768_mxfp8 write -, W (2304,
// 768) e4m3 + sW (6 planes of 2304 dwords); side (n_seq * 33, 2304) bf16 as in sf_qkv_time_attention2 (from sf_gemm_mxfp8 on gathered copies of the rows and of their scale
// dwords: sf_side_rows).  The attention runs on the bf16-rounded projection, exactly as sf_qkv_time_attention_mx does.  Output: EITHER out (bf16, patch rows) OR out_q / out_s
// (e4m3 bytes (rows, 768) + the scale planes [6][rows][4], splane bytes apart: byte for byte sf_quantize_mxfp8 of the bf16 output - the A operand of the MX projection that
// follows; buffers of their own, not X / sX).  cls_partial [n_seq][12][33][66] (merge with sf_attention_cls_combine(_mx), n_part = 33).  Replaces sf_gemm_mxfp8 (CLS rows) +
// sf_qkv_time_attention_mx(_q).
extern "C" int sf_qkv_time_attention2_mx(const uint8_t* X, int64_t ldx, const uint8_t* sX, int64_t ldsx, const uint8_t* W, int64_t ldw, const uint8_t* sW, int64_t ldsw,
                                         const float* bias, const uint16_t* side, int64_t lds_, uint16_t* out, int64_t ldo, uint8_t* out_q, int64_t ldq, uint8_t* out_s,
                                         int64_t splane, float* cls_partial, int64_t n_seq, int n_tok, float scale, void* stream) {
  Qt2Args a;
  a.X = reinterpret_cast<const bf16_t*>(X); a.ldx = ldx; a.W = reinterpret_cast<const bf16_t*>(W); a.ldw = ldw; a.bias = bias; a.side = side; a.lds_ = lds_;
  a.out = out; a.ldo = ldo; a.cls_part = cls_partial; a.scale = scale; a.pair_chunk = 6; a.stagger = 0;
  a.sX = sX; a.ldsx = ldsx; a.sW = sW; a.ldsw = ldsw; a.out_q = out_q; a.ldq = ldq; a.out_s = out_s; a.splane = splane;
  return qkt_launch(QT2_MX, qkv_time2_attn_mx_kernel, a, n_seq, n_tok, stream);
}
