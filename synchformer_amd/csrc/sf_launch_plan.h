// The host-side arithmetic of the persistent launchers: ONE definition of each grid, tile-count, column-chunk and measurement-knob rule.  Host only and free of
// HIP: plain integer functions that any C++17 compiler takes alone (tests/launch_plan_main.cpp does, under the address and undefined-behaviour sanitizers), so
// the rules are tested without opening a device.  A launcher keeps what is its own - the argument struct, the kernel choice, the launch and the texts of its
// errors.  The rules, once:
//
//   * A persistent kernel runs ONE workgroup per CU.  The hardware deals consecutive workgroup ids round-robin to the 8 XCDs (blockIdx % 8 is the XCD), and the
//     tile walks give every XCD its own slice of the work (its own rows, its own weight slice in its own L2), so a grid is a WHOLE NUMBER of workgroups per XCD:
//     a multiple of 8, and never empty on a device or partition that reports fewer than 8 CUs.  No more workgroups than work items rounded up to the 8 slots.
//   * The kernels without an XCD schedule (one walk over all row tiles: the fused projection + LayerNorm GEMMs) take one workgroup per CU and no more than tiles.
//   * Tile and work-item indices are 32-bit in the kernels: a launcher refuses a shape whose tile count does not fit 31 bits, with its own entry's text.
//   * Column-chunked sweeps: see sf_l2_nchunk.
//   * A measurement knob (SF_... in the environment) is read ONCE per process, by the initialiser of a function-local `static const int` - which the language
//     makes safe under concurrent host threads, like the mutex of sf_prepare_kernel / sf_cu_count and the thread_local force hooks.  The product never sets one;
//     DESIGN.md lists them with their defaults.
#pragma once
#include <stdint.h>
#include <stdlib.h>

// Workgroups of an XCD-scheduled persistent kernel on a device of n_cu (> 0) CUs: (n_cu / 8) * 8, at least 8.  (sf_gemm_tn_pp takes this form: its workgroups
// find out by themselves that nothing is left.)
static inline int64_t sf_xcd_grid(int n_cu) {
  const int64_t blocks = (n_cu / 8) * 8;
  return blocks < 8 ? 8 : blocks;                // (a device / partition with fewer than 8 CUs: never an empty grid)
}
// ... and at most `items` (>= 0) work items rounded up to the 8 slots
static inline int64_t sf_xcd_grid(int n_cu, int64_t items) {
  const int64_t blocks = sf_xcd_grid(n_cu), need = ((items + 7) / 8) * 8;
  return blocks > need ? need : blocks;
}

// Workgroups of a persistent kernel without an XCD schedule: one per CU, no more than tiles
static inline int64_t sf_cu_grid(int n_cu, int64_t tiles) { return tiles < n_cu ? tiles : n_cu; }

// Column tiles and all tiles of an (M, N) output in BM x BN tiles.  False when the total does not fit the kernels' 31-bit tile index (*tiles_total is then left
// alone): the caller reports "<entry>: too many tiles".
static inline bool sf_tile_counts(int64_t M, int64_t N, int BM, int BN, uint32_t* tiles_n, uint32_t* tiles_total) {
  const int64_t tiles_m = (M + BM - 1) / BM;
  *tiles_n = (uint32_t)((N + BN - 1) / BN);
  const int64_t total = tiles_m * *tiles_n;
  if (total >= ((int64_t)1 << 31)) return false;
  *tiles_total = (uint32_t)total;
  return true;
}

// Column tiles per sweep of a persistent 256-column-tile GEMM (0 = all of them in one sweep).  Column-chunked sweeps keep the weight slice of a sweep (nchunk *
// 256 rows * K elements: bytes_per_k = 512 for bf16, 256 for the e4m3 bytes of MXFP8) within ~2.4 MB of the XCD's 4 MB L2, so that the streamed A panels and
// outputs stop evicting it: PMC on M = 351,456 - qkv 1912 -> 1132 MiB fetched per launch (518 algorithmic), fc1 5604 -> 1167, and +2-4 % speed
// (profiles/r01_gemm_configs.md).  Only for short K (k_max: 1024 bf16, 2048 MXFP8 - the same 2 KiB row): with K = 3072 an A panel is 1.5 MB and re-reading it
// per sweep costs more than it saves (fc2 already fetches its algorithmic bytes).
static inline uint32_t sf_l2_nchunk(int64_t K, int64_t bytes_per_k, int64_t k_max) {
  if (K > k_max) return 0u;
  const int64_t n = 2400000 / (bytes_per_k * K);
  return (uint32_t)(n > 0 ? n : 1);
}

// A measurement knob: the integer value of environment variable `var`, `dflt` when it is unset.  Call it from the initialiser of a `static const int` (with the
// knob's clamp, where it has one) and nowhere else.
static inline int sf_env_int(const char* var, int dflt) {
  const char* e = getenv(var);
  return e ? atoi(e) : dflt;
}
