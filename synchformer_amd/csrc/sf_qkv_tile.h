// The 192 x 384 x 64 main loop that sf_qkv_space.hip and sf_qkv_time2.hip share (gfx950): 192 token rows of X times the q | k | v of two heads (384 rows of W), as
// 2 x 4 waves of 96 x 96, accumulators transposed (C^T = W X^T: a lane ends with one token's features) and started at the bias.  One copy of the schedule: a wait
// count that is wrong here is wrong for both kernels and for every variant of them, and is searched for in one place.
//
//   * Stages: 64-deep k-tiles (MX: 128 fp8 k - 128 bytes per row either way) in two 72-KiB stages, each A 24 KiB | W0 | W1 | W2 of 16 KiB; W part j = feature
//     block j (32 features) of each of the four wave columns.  The bias (384 floats) sits at 156 KiB, behind everything the kernels overlay on the stages.
//   * Pieces: a wave moves 9 LDS-DMA pieces of 1 KiB per k-tile - A pieces 0..2 (tile rows (3 wave + pc) * 8 .. + 7) and two per W part (part rows
//     (2 wave + pc) * 8 .. + 7) -, MX one more: the k-tile's scale dwords (192 token rows | 3 x 128 part rows of W = 2304 B per parity) are three pieces of which
//     EVERY wave issues one (wave % 3; the copies land the same bytes), so that all waves count the same number of vector-memory operations.
//   * Schedule: THREE phases per k-tile, one feature block each - 12 MFMAs of 32x32x16 (MX: 6 scaled MFMAs of 32x32x64) per wave and phase, the wave's 12 A
//     fragments held in registers.  The pieces run about one stage ahead behind COUNTED waits; the wm = 1 waves run one barrier behind the wm = 0 waves:
//
//         prologue          issue (MX: scales of kt 0,) W0 A0 | W1 A1 A2 | W2 of k-tile 0, W0 A0 of k-tile 1     vmcnt(5): A | W0 | W1 of k-tile 0 (and everything the
//                                                                                                                kernel issued in front: bias, its side loads) landed
//         phase 0 of kt     issue W1, A1, A2 of kt+1                                                              no wait
//         phase 1 of kt     issue (MX: scales of kt+1,) W2 of kt+1                                                vmcnt(9 | MX 10): W2 of kt landed        [last kt: 0]
//         phase 2 of kt     issue W0, A0 of kt+2                                                                  vmcnt(5): A | W0 | W1 (| scales) of kt+1 [kt+2 absent: 2; last: 0]
//
//     Every part is refilled two phases after its last fragment read; data is read one phase after its wait (a barrier lies between).  The counts are counts of
//     THIS wave's operations: whatever a kernel issues per wave in front of the prologue is older than the prologue's pieces and retires with its vmcnt(5).
//   * What differs between the two kernels is a parameter: XRUN (X rows between the starts of two 24-row runs of the tile: 24 = one contiguous run of 192 rows,
//     196 = the same 24 patches in 8 frames), the X row the item starts at, SC_OFF (where the scale dwords land) - and the measurement switches.
//   * Host side: one argument check and one launch (grid computation included) for the four launchers (the bf16 and the MX form of either kernel).
#pragma once
#include "sf_common.h"
#include "sf_lds_prims.h"
#include <stdlib.h>

#define QKT_ROWS 192                     // token rows of the tile
#define QKT_D 768
#define QKT_A_BYTES (QKT_ROWS * 128)     // 24 KiB: 192 rows x 64 k (bf16)
#define QKT_W_PART (128 * 128)           // 16 KiB: 4 wave columns x 32 features x 64 k
#define QKT_STAGE (QKT_A_BYTES + 3 * QKT_W_PART)   // 72 KiB
#define QKT_BIAS_OFF (156 * 1024)        // the tile's 384 bias floats: lives through the main loop AND the kernels' epilogues
#define QKT_SC_BYTES 2304                // MX: the scale dwords of one k-tile
#define QKT_LDS (160 * 1024)

typedef __attribute__((ext_vector_type(8))) int qkt_i32x8;
typedef short qkt_s4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) qkt_s4 qkt_lds_s4;

// Persistent schedule, one workgroup per CU: block b sits on XCD b % 8; every XCD owns a contiguous range of row tiles (frames | patch blocks) and sweeps it once per
// chunk of `hc` head pairs (pair fastest inside a chunk).  A workgroup walks items t = li, li + step, .. < t_end of its XCD.
struct QktSchedule {
  uint32_t xcd, li, step, rt0, hc, chunk_tiles, t_end;
  __device__ __forceinline__ QktSchedule(uint32_t n_rt, uint32_t pair_chunk) {
    xcd = blockIdx.x & 7u; li = blockIdx.x >> 3; step = gridDim.x >> 3;
    const uint32_t r8 = (n_rt + 7u) >> 3;
    rt0 = min(xcd * r8, n_rt);
    const uint32_t rt1 = min(rt0 + r8, n_rt);
    hc = pair_chunk; chunk_tiles = (rt1 - rt0) * hc; t_end = (rt1 - rt0) * 6u;
  }
  __device__ __forceinline__ void item(uint32_t t, uint32_t& rt, int& hp) const {
    const uint32_t c = t / chunk_tiles, r = t - c * chunk_tiles;
    rt = rt0 + r / hc; hp = (int)(c * hc + r % hc);
  }
};

// The operands of the projection: X (rows, 768) and W (2304, 768) bf16, ldx / ldw in elements; MX: e4m3 BYTES (ldx / ldw in bytes) with stage-major E8M0 scale planes
// (one dword per row per 128 k, ldsx / ldsw bytes between planes).  bias: 2304 floats or null.
struct QktOperands {
  const void* X; int64_t ldx;
  const void* W; int64_t ldw;
  const uint8_t* sX; int64_t ldsx;
  const uint8_t* sW; int64_t ldsw;
  const float* bias;
};

// One workgroup's view of the tile.  Per kernel: the constructor; per work item: begin_item(), then the kernel's own side loads (issue_bias() among them), then
// project().  NO_MFMA / NO_PROLOGUE_WAIT: measurement builds (WRONG results) - the main loop without its MFMAs, the prologue without its wait.
template <bool MX, int XRUN, int SC_OFF, bool NO_MFMA = false, bool NO_PROLOGUE_WAIT = false>
struct QktTile {
  static constexpr int ESZ = MX ? 1 : 2;                           // bytes per operand element
  static constexpr int NK = MX ? QKT_D / 128 : QKT_D / 64;         // 12 k-tiles of 64 bf16 / 6 of 128 fp8
  char* const smem;
  const QktOperands o;
  const int wave, lane, wm, wn;                                    // 2 x 4 waves, wave tile 96 token rows x 96 features
  const int sc_seg, sc_lanes;                                      // MX: this wave's scale piece and its lanes (48 + 96 lanes of 16 bytes = three pieces)
  const uint32_t a8, w8;                                           // 8 rows of X / W in bytes
  const uint32_t lds0, lds_a_w, lds_w_w, sc_lds;                   // LDS addresses: smem, this wave's first A piece / W piece of a part, its scale piece
  // per item
  uint32_t voff_a = 0, voff_w[3] = {0, 0, 0}, sc_voff = 0;         // lane offsets of the LDS-DMA pieces: re-derived for every item (not kept live across the kernels' epilogues)
  const char* xbase; const char* wbase;
  int64_t xrow; int hp;

  __device__ __forceinline__ QktTile(char* smem_, const QktOperands& o_, int wave_, int lane_)
      : smem(smem_), o(o_), wave(wave_), lane(lane_), wm(wave_ >> 2), wn(wave_ & 3), sc_seg(wave_ % 3), sc_lanes(sc_seg == 0 ? 48 : (sc_seg == 1 ? 64 : 32)),
        a8((uint32_t)(8 * o_.ldx * ESZ)), w8((uint32_t)(8 * o_.ldw * ESZ)), lds0(__builtin_amdgcn_readfirstlane(sf_lds_addr(smem_))),
        lds_a_w(__builtin_amdgcn_readfirstlane(lds0 + wave_ * 3072)), lds_w_w(__builtin_amdgcn_readfirstlane(lds0 + QKT_A_BYTES + wave_ * 2048)),
        sc_lds(__builtin_amdgcn_readfirstlane(lds0 + SC_OFF + (sc_seg == 0 ? 0 : (sc_seg == 1 ? 768 : 768 + 1024)))) {}

  // The item's tile: tile row R = 24 run + i <-> row xrow_ + XRUN run + i of X; columns = the q | k | v of heads 2 hp_, 2 hp_ + 1.  Derives the lane offsets of the
  // pieces (row strides are multiples of 128 bytes - launcher check -, so the low 7 bits of an offset are its chunk slot: the piece 8 rows further down is
  // (offset ^ 64) + 8 rows, computed at issue time instead of held in a register per piece).  Returns the lane id the offsets were derived from - opaque to the
  // compiler, so that nothing derived from it is hoisted out of the item loop and kept live across the epilogues - for the lane offsets of the kernel's side loads.
  __device__ __forceinline__ int begin_item(int64_t xrow_, int hp_) {
    xrow = xrow_; hp = hp_;
    xbase = reinterpret_cast<const char*>(o.X) + xrow * o.ldx * ESZ;
    wbase = reinterpret_cast<const char*>(o.W) + (int64_t)hp * 128 * o.ldw * ESZ;
    int dtid = threadIdx.x;
    asm volatile("" : "+v"(dtid));
    const int dl = dtid & 63;
    {
      // A piece pc of this wave = tile rows (3 wave + pc) * 8 .. + 7 (run `wave`, rows 8 pc .. + 7 of it); lane (r = lane >> 3, chunk slot = lane & 7) -> LDS
      // row-linear, source chunk XOR-swizzled by the TILE row
      const int r = wave * 3 * 8 + (dl >> 3);
      voff_a = (uint32_t)((int64_t)(wave * XRUN + (dl >> 3)) * o.ldx * ESZ + ((((dl & 7) ^ ((r >> 1) & 7))) << 4));
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      // W part j, piece pc of this wave = part rows (2 wave + pc) * 8 .. + 7; part row pr = 32 wn' + rr <-> tile column wn' * 96 + 32 j + rr <-> row
      // which * 768 + hd * 64 + feat of W (the head pair's offset rides in the SGPR base).  A piece's 8 rows lie in one 16-column group of the tile, so head and
      // q | k | v of the row depend on the wave only: W row = grow_w + (lane >> 3), grow_w wave-uniform (scalar, computed once in front of the item loop)
      const int pr = wave * 2 * 8 + (dl >> 3);
      const int cw = (wave >> 1) * 96 + j * 32 + (wave & 1) * 16;   // tile column of part row 16 wave
      const int hd = cw / 192, within = cw - hd * 192;
      const int grow_w = (within >> 6) * QKT_D + hd * 64 + (within & 63);
      voff_w[j] = (uint32_t)((int64_t)(grow_w + (dl >> 3)) * o.ldw * ESZ + ((((dl & 7) ^ ((pr >> 1) & 7))) << 4));
    }
    if (MX) {
      // the k-tile's scale dwords as 16-byte LDS-DMA lanes: piece 0 = the tile's 192 token rows in tile order (a lane = 4 rows, a run = 6 lanes, of plane kt of sX),
      // pieces 1 | 2 = the tile's 384 W rows (12 runs of 32 rows of plane kt of sW) in part order: area index j * 128 + 32 wn' + rr
      if (sc_seg == 0) sc_voff = XRUN == 24 ? (uint32_t)dl * 16u : (uint32_t)((dl / 6) * XRUN * 4 + (dl % 6) * 16);
      else {
        const int L = (sc_seg == 1 ? 0 : 64) + dl, run = L >> 3, j = run >> 2, wnp = run & 3;
        const int c = wnp * 96 + j * 32 + (L & 7) * 4;
        const int hd = c / 192, within = c - hd * 192;
        sc_voff = (uint32_t)(((within >> 6) * QKT_D + hd * 64 + (within & 63)) * 4);
      }
    }
    return dl;
  }

  __device__ __forceinline__ void issue_sc(int kt) const {
    const char* base = sc_seg == 0 ? reinterpret_cast<const char*>(o.sX) + (int64_t)kt * o.ldsx + xrow * 4
                                   : reinterpret_cast<const char*>(o.sW) + (int64_t)kt * o.ldsw + (int64_t)hp * 512;
    if (lane < sc_lanes) sf_dma1(sc_voff, base, sc_lds + (kt & 1) * QKT_SC_BYTES);
  }
  __device__ __forceinline__ void issue_a(int pc, int S, int kt) const {   // piece pc: 8 pc rows further down; the chunk swizzle flips bit 2 with every 8 rows
    sf_dma1(((pc & 1) ? (voff_a ^ 64u) : voff_a) + (uint32_t)pc * a8, xbase + kt * 128, lds_a_w + S * QKT_STAGE + pc * 1024);
  }
  __device__ __forceinline__ void issue_w(int j, int S, int kt) const {
    sf_dma1(voff_w[j], wbase + kt * 128, lds_w_w + S * QKT_STAGE + j * QKT_W_PART);
    sf_dma1((voff_w[j] ^ 64u) + w8, wbase + kt * 128, lds_w_w + S * QKT_STAGE + j * QKT_W_PART + 1024);
  }
  // 6 x 64 bias floats (waves 0..5): tile columns 64 wave .. + 63 = (head hd = wave / 3, q | k | v = wave % 3).  One of the kernel's side loads, in front of project()
  __device__ __forceinline__ void issue_bias() const {
    if (wave < 6 && o.bias) sf_dma_dword_addr(o.bias + (wave % 3) * QKT_D + (hp * 2 + wave / 3) * 64 + lane, lds0 + QKT_BIAS_OFF + wave * 256);
  }

  // The projection of the item: acc block (j, i) = features 96 wn + 32 j + 8 g + 4 hi + r of the tile, tokens 96 wm + 32 i + l31.  Starts behind the barrier that ended
  // the previous item (both stages are free) and returns behind the barrier after which every wave is done with both stages.
  __device__ __forceinline__ void project(f32x16 (&acc)[3][3]) const {
    // ---- prologue: k-tile 0 and W0 | A0 of k-tile 1 ----
    if (MX) issue_sc(0);
    issue_w(0, 0, 0); issue_a(0, 0, 0);
    issue_w(1, 0, 0); issue_a(1, 0, 0); issue_a(2, 0, 0);
    issue_w(2, 0, 0);
    issue_w(0, 1, 1); issue_a(0, 1, 1);
    if (!NO_PROLOGUE_WAIT) sf_wait_vmcnt<5>();                     // the kernel's side loads, (scales,) A | W0 | W1 of k-tile 0 (this wave's pieces) have landed
    sf_barrier();

    // accumulators start at the bias
    {
      const int hi = lane >> 5;
      const float* bs = reinterpret_cast<const float*>(smem + QKT_BIAS_OFF);
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 b4 = o.bias ? *reinterpret_cast<const float4*>(bs + wn * 96 + j * 32 + g * 8 + hi * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int i = 0; i < 3; ++i) { acc[j][i][g * 4 + 0] = b4.x; acc[j][i][g * 4 + 1] = b4.y; acc[j][i][g * 4 + 2] = b4.z; acc[j][i][g * 4 + 3] = b4.w; }
        }
    }
    int fo[4], fs_x = 0, fs_w = 0, shi = 0;                         // (MX: addresses of this lane's scale dwords - its token row of block 0, row l31 of its W part 0 - and 8 * (lane >> 5))
    {
      int ptid = threadIdx.x;
      asm volatile("" : "+v"(ptid));
      const int pl31 = ptid & 31, phi = (ptid & 63) >> 5;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) fo[kk] = pl31 * 128 + (((kk * 2 + phi) ^ ((pl31 >> 1) & 7)) << 4);
      if (MX) { fs_x = SC_OFF + (wm * 96 + pl31) * 4; fs_w = SC_OFF + 768 + (wn * 32 + pl31) * 4; shi = phi * 8; }
    }
    const int a_base = wm * 96 * 128, w_base = QKT_A_BYTES + wn * 32 * 128;
    // fragments as 32-byte pairs (kk = 2 k2, 2 k2 + 1): the two 16-byte reads a lane supplies to ONE 64-deep scaled MFMA sit in eight consecutive registers, no copies
    union QktFrag { bf16x8 h[2]; qkt_i32x8 v; };
    QktFrag xf[3][2], wf[2];
    uint32_t sx[3] = {0u, 0u, 0u}, sw = 0u;                          // MX: this lane's scale dwords of the k-tile (token row of block i; W row of the current part), >> shi
    auto read_w = [&](const char* st, int j, int par) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) wf[kk >> 1].h[kk & 1] = *reinterpret_cast<const bf16x8*>(st + w_base + j * QKT_W_PART + fo[kk]);
      if (MX) sw = *reinterpret_cast<const uint32_t*>(smem + fs_w + j * 512 + par * QKT_SC_BYTES) >> shi;
    };
    auto mma = [&](auto Jc) {
      constexpr int J = decltype(Jc)::value;
      __builtin_amdgcn_s_setprio(1);
      if constexpr (MX) {
        // a 128-byte LDS row = 128 fp8 k: fragments 2 k2 and 2 k2 + 1 are the 2 x 16 bytes a lane supplies to ONE 64-deep scaled MFMA (as qkv_time_attn_kernel<true, true>)
#pragma unroll
        // scale operands: the k-tile's dword of the row, shifted by 8 * (lane >> 5) so that BYTE 2 k2 is this half-wave's 32-k block of MFMA k2 - selected by the
        // instruction's op_sel (byte index of the scale register), no extraction arithmetic inside the matrix segment
        for (int k2 = 0; k2 < 2; ++k2) {
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            if (k2 == 0) acc[J][i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[0].v, xf[i][0].v, acc[J][i], 0 /* e4m3 */, 0 /* e4m3 */, 0, (int)sw, 0, (int)sx[i]);
            else acc[J][i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[1].v, xf[i][1].v, acc[J][i], 0, 0, 2, (int)sw, 2, (int)sx[i]);
          }
        }
      } else
      if (!NO_MFMA) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int i = 0; i < 3; ++i) acc[J][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[kk >> 1].h[kk & 1], xf[i][kk >> 1].h[kk & 1], acc[J][i], 0, 0, 0);
      } else asm volatile("" :: "v"(wf[0].v), "v"(wf[1].v), "v"(xf[0][0].v), "v"(xf[2][1].v));
      asm volatile("" : "+v"(acc[J][0]), "+v"(acc[J][1]), "+v"(acc[J][2]));   // pins the (pure) MFMAs inside their matrix segment
      __builtin_amdgcn_s_setprio(0);
    };
    // one k-tile held in stage S; ld1 / ld2: k-tiles kt+1 / kt+2 exist
    auto ktile = [&](auto Sc, int kt, bool ld1, bool ld2) {
      constexpr int S = decltype(Sc)::value;
      const char* st = smem + S * QKT_STAGE;
      // ---- phase 0: feature block 0 ----
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) xf[i][kk >> 1].h[kk & 1] = *reinterpret_cast<const bf16x8*>(st + a_base + i * 4096 + fo[kk]);
      read_w(st, 0, S);                                              // (NK is even: the parity of k-tile kt is the stage S)
      if (MX) {
#pragma unroll
        for (int i = 0; i < 3; ++i) sx[i] = *reinterpret_cast<const uint32_t*>(smem + fs_x + i * 128 + S * QKT_SC_BYTES) >> shi;
      }
      __builtin_amdgcn_sched_barrier(0);
      if (ld1) { issue_w(1, S ^ 1, kt + 1); issue_a(1, S ^ 1, kt + 1); issue_a(2, S ^ 1, kt + 1); }      // W1, A1, A2 of k-tile kt+1
      sf_barrier();
      __builtin_amdgcn_sched_barrier(0);
      mma(sf_ic<0>{});
      __builtin_amdgcn_sched_barrier(0);
      sf_barrier();
      // ---- phase 1: feature block 1 ----
      read_w(st, 1, S);
      __builtin_amdgcn_sched_barrier(0);
      // (MX: the scale piece of k-tile kt+1 goes in FRONT of W2 - the phase-2 wait below then retires it with A | W0 | W1 - into the other parity's area, last read in phase 0 of kt-1)
      if (ld1) { if (MX) issue_sc(kt + 1); issue_w(2, S ^ 1, kt + 1); if (MX) sf_wait_vmcnt<10>(); else sf_wait_vmcnt<9>(); } else sf_wait_vmcnt<0>();   // W2 of k-tile kt+1 issued; W2 of this k-tile has landed
      sf_barrier();
      __builtin_amdgcn_sched_barrier(0);
      mma(sf_ic<1>{});
      __builtin_amdgcn_sched_barrier(0);
      sf_barrier();
      // ---- phase 2: feature block 2 ----
      read_w(st, 2, S);
      __builtin_amdgcn_sched_barrier(0);
      if (ld2) { issue_w(0, S, kt + 2); issue_a(0, S, kt + 2); sf_wait_vmcnt<5>(); }                     // W0, A0 of k-tile kt+2; A | W0 | W1 of k-tile kt+1 have landed
      else if (ld1) sf_wait_vmcnt<2>();
      else sf_wait_vmcnt<0>();
      sf_barrier();
      __builtin_amdgcn_sched_barrier(0);
      mma(sf_ic<2>{});
      __builtin_amdgcn_sched_barrier(0);
      sf_barrier();
    };
    if (wm == 1) sf_barrier();                                     // waves 4-7 run one barrier behind waves 0-3
#pragma unroll 1
    for (int kt = 0; kt < NK; kt += 2) {
      ktile(sf_ic<0>{}, kt, true, kt + 2 < NK);
      ktile(sf_ic<1>{}, kt + 1, kt + 2 < NK, kt + 3 < NK);
    }
    if (wm == 0) sf_barrier();                                     // re-align; every wave is done with both stages
  }
};

// ---- host side: the launchers of the two kernels (bf16 and MX form each) ----------------------------------------------------------------------------------------
struct QktLaunch {
  const char* name;                      // the C entry point, for messages
  const char* built_for;                 // what n_tok = 196 means to the kernel
  const char* x_span; int64_t x_span_rows;   // the rows of X one 32-bit lane offset has to span ("a frame": 196, "a sequence": 1569)
  int items_per_seq;                     // row tiles per sequence; times 6 head pairs = work items
  bool mx;                               // X / W are e4m3 bytes with scale planes; the output is bf16 `out` OR MXFP8 out_q / out_s
};

// The argument rules of a launcher, on its filled argument struct (QsArgs / Qt2Args: the same operand fields).  0 or -1 (sf_last_error set); n_seq <= 0 (nothing
// to launch) passes the size checks unseen.
template <class Args>
static int qkt_check_args(const QktLaunch& L, const Args& a, int64_t n_seq, int n_tok) {
  const int esz = L.mx ? 1 : 2;
  if (L.mx) SF_CHECK_ARG(a.X && a.sX && a.W && a.sW && a.side && a.cls_part && ((a.out != nullptr) != (a.out_q != nullptr)), "%s: null pointer (exactly one of out / out_q)", L.name);
  else SF_CHECK_ARG(a.X && a.W && a.side && a.out && a.cls_part, "%s: null pointer", L.name);
  SF_CHECK_ARG(n_tok == 196, "%s: built for %s (8 frames per sequence), got %d", L.name, L.built_for, n_tok);
  // (bf16 form: `out` is an operand like the others; MX form: one of out / out_q, each with rules of its own)
  SF_CHECK_ARG((a.ldx * esz % 128) == 0 && (a.ldw * esz % 128) == 0 && a.ldx >= QKT_D && a.ldw >= QKT_D && (a.lds_ % 8) == 0 && a.lds_ >= 3 * QKT_D &&
                   (L.mx || ((a.ldo % 8) == 0 && a.ldo >= QKT_D)),
               "%s: bad row strides (ldx / ldw multiples of %s: the chunk slot lives in the low 7 bits of a piece's byte offset)", L.name, L.mx ? "128 bytes" : "64 elements");
  SF_CHECK_ARG(((uintptr_t)a.X % 16) == 0 && ((uintptr_t)a.W % 16) == 0 && ((uintptr_t)a.sX % 16) == 0 && ((uintptr_t)a.sW % 16) == 0 && ((uintptr_t)a.side % 16) == 0 &&
                   ((uintptr_t)a.bias % 16) == 0 && ((uintptr_t)a.cls_part % 8) == 0 && (L.mx || ((uintptr_t)a.out % 16) == 0), "%s: operands must be 16-byte aligned", L.name);
  if (L.mx && a.out) SF_CHECK_ARG(((uintptr_t)a.out % 16) == 0 && (a.ldo % 8) == 0 && a.ldo >= QKT_D, "%s: out must be a 16-byte aligned bf16 buffer", L.name);
  if (a.out_q) SF_CHECK_ARG(a.out_s && ((uintptr_t)a.out_q % 8) == 0 && ((uintptr_t)a.out_s % 2) == 0 && (a.ldq % 8) == 0 && a.ldq >= QKT_D && (const void*)a.out_q != (const void*)a.X &&
                                a.out_s != a.sX, "%s: out_q (8-byte aligned, ldq %% 8 == 0) / out_s must be buffers of their own", L.name);
  SF_CHECK_ARG(L.mx || (const void*)a.X != (const void*)a.out, "%s: out must not alias X", L.name);
  if (n_seq <= 0) return 0;
  if (a.out_q) SF_CHECK_ARG(a.splane >= n_seq * a.seq_rows * 4, "%s: a scale plane holds 4 bytes per row", L.name);
  if (L.mx) SF_CHECK_ARG((a.ldsx % 16) == 0 && (a.ldsw % 16) == 0 && a.ldsx >= n_seq * a.seq_rows * 4 && a.ldsw >= 3 * QKT_D * 4, "%s: scale planes must hold one dword per row of X / W", L.name);
  SF_CHECK_ARG(L.x_span_rows * a.ldx * esz < ((int64_t)1 << 32) && (int64_t)3 * QKT_D * a.ldw * esz < ((int64_t)1 << 32) && (int64_t)33 * a.lds_ * 2 < ((int64_t)1 << 32),
               "%s: %s of X, W and a sequence's side rows must stay below 4 GiB (32-bit lane offsets)", L.name, L.x_span);
  SF_CHECK_ARG(n_seq * L.items_per_seq * 6 < ((int64_t)1 << 31), "%s: too many tiles", L.name);
  return 0;
}

// The launch of either kernel in any form, on its argument struct with the operand fields filled: checks them, fills seq_rows and n_rt, prepares `kernel` for its
// 160 KiB of LDS and sizes the grid by the XCD rule (sf_xcd_grid) over n_rt * 6 work items.  0 or the error (sf_last_error set).
template <class Args, class Kernel>
static int qkt_launch(const QktLaunch& L, Kernel kernel, Args& a, int64_t n_seq, int n_tok, void* stream) {
  a.seq_rows = 1 + 8 * 196;
  if (int rc = qkt_check_args(L, a, n_seq, n_tok)) return rc;
  if (n_seq <= 0) return 0;
  if (int rc = sf_prepare_kernel((const void*)kernel, QKT_LDS, L.name)) return rc;
  const int n_cu = sf_cu_count(L.name);
  if (n_cu <= 0) return -1;
  a.n_rt = (uint32_t)(n_seq * L.items_per_seq);
  hipLaunchKernelGGL(kernel, dim3((unsigned)sf_xcd_grid(n_cu, (int64_t)a.n_rt * 6)),dim3(512), QKT_LDS, (hipStream_t)stream, a);
  SF_LAUNCH_CHECK();
  return 0;
}

// SF_QS_PAIR_CHUNK / SF_QT2_PAIR_CHUNK: head pairs per sweep over an XCD's row tiles (a divisor of 6; default and fallback 6).  The
// initialiser of a `static const int` at its two call sites: read once per process, like every knob.
static int qkt_env_pair_chunk(const char* var) {
  const int hc = sf_env_int(var, 6);
  return (hc < 1 || 6 % hc) ? 6 : hc;
}
