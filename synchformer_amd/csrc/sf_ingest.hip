// Ingest of a decoded recording at its native geometry: what the reference leaves to an ffmpeg subprocess before any of its code runs
// (example.py:16-53: fps=25, short side 256, even dimensions, -ar 16000) plus the centre 224 crop of RGBSpatialCrop, as two launches.
//   sf_ingest_video:   frame pick (frame_table) + antialiased bicubic resize + crop, uint8 -> uint8 planar (T_out, 3, 224, 224).  The resize is separable and the
//                      two filter tables arrive already sliced to the crop, so only the 224 x 224 outputs are computed: a horizontal pass over the source rows a
//                      tile of output rows needs (fp32, kept in LDS), then the vertical pass over those rows.
//   sf_ingest_video_yuv: the same for 8-bit YUV 4:2:0 frames (NV12, I420): the three planes are resized, the colour matrix runs on the 224 x 224 result.
//   sf_ingest_video_yuv16: the same for 10-bit YUV 4:2:0 frames in 16-bit samples (P010, yuv420p10le): the sample is (raw >> shift) & 1023.
//   sf_ingest_video_yuv_planes: the general form of the two: three planes of 1- or 2-byte samples at any offsets and strides, chroma of Hc x Wc -
//                      4:2:2 packed (uyvy422, yuyv422, y210), semi-planar (nv16, p210) and planar (yuv422p, yuv422p10le), the 4:2:0 layouts, 4:4:4 planar.
//   sf_ingest_video_v210, sf_ingest_video_v210_fields: the same for v210 frames and fields: 10-bit 4:2:2 as SDI capture delivers it, three 10-bit fields
//                      Cb Y Cr Y .. per 32-bit word - unpacked while staging, from there the 16-bit pipeline of yuv422p10le; two kernels of their own.
//   sf_ingest_video_fields, sf_ingest_video_yuv_planes_fields: sf_ingest_video and the general entry on an INTERLACED recording: the table names fields,
//                      each workgroup resizes the rows p, p + 2, .. of its frame with the vertical table of that parity - kernels of their own beside the
//                      progressive ones, which stay the code they were.
//   sf_resample_wave:  zero-delay polyphase windowed-sinc resampler (the bank of ingest.resample_kernel), channels averaged on read, zero padding by bounds checks.
//   sf_resample_wave_mix: the same resampler for P programmes of one multi-channel wave: planar or interleaved fp32 / int16 / int32 input read once
//                      per tile, mixed by a (P, ch) matrix into P fp32 rows in LDS, each row filtered by sf_resample_wave's rule - a kernel of its own.
// All video kernels run ONE resize pipeline, ing_plane_pass, over 1-byte or 2-byte samples (BS): ingest_video_kernel once per workgroup (one channel), the YUV
// kernels twice (luma, then U and V together); the launchers size its LDS with one formula, ing_geometry.
// Host side: the six video entries are argument conversions onto two bodies - ing_rgb (sf_ingest_video, sf_ingest_video_fields) and ing_planes (the four YUV
// entries) - which hold every check, the LDS sizing, the colour matrix and the kernel pick once.  The two 4:2:0 entries reach ing_planes in ING_LEGACY420 mode: it
// keeps their messages, their GEN = 0 instantiations and the trailing kernel arguments they always passed.
// All kernels bound every address they form by the sizes the launcher was given: a table with entries outside the source only changes the picture, never the
// addresses (frame index, first-tap row / column and every tap are clamped or skipped).
#include <initializer_list>

#include "sf_common.h"
#include "../../include/synchformer_hip.h"

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

#define ING_OUT 224            // output rows = columns (the model's input size)
#define ING_TY 8               // output rows per workgroup
#define ING_MAX_TAPS 35        // 2 * ceil(2 * scale) + 1 at scale <= 8.5: a short side up to 2160 at resize_side 256
#define ING_MAX_ROWS 8         // source rows per chunk (4 when the source is wide: the launcher sizes it so that everything fits 64 KiB of LDS)
#define ING_LDS_BYTES 65536
#define ING_PF 20              // staged dwords per lane per chunk at most: NP * R * RP / 4 <= 5120
#define ING_ROW_SLACK 8        // samples behind a staged row that the horizontal pass may read (always against a zero weight)
#define ING_LDS_BYTES16 98304  // the same for 2-byte samples: four staged rows of a 3840-wide luma plane at 35 taps take ~68 KiB (gfx950: 160 KiB per workgroup)
#define ING_PF210 20           // the same for v210 rows (FORM = 3), which fetch 1.5 words per staged dword: see ing_plane_pass
#define ING_PF16 40            // staged dwords per lane per chunk at most for 2-byte samples: NP * R * RP / 2 <= 10240, the row widths the 1-byte kernels serve

// The resize of output rows [r0, r0 + 8) of NP planes of one frame that share their geometry and tables (NP = 1: one RGB channel, or luma; NP = 2: U and V), by the
// 256 threads of a workgroup.  Element (y, x) of plane p is s[p][y * sy + x * sx].  Adds into a0[p] / a1[p]: this lane's 4 columns 4 q .. 4 q + 3 of output rows
// r0 + rg and r0 + rg + 4 (q = tid % 56, rg = tid / 56, lanes < 224).  A caller that runs it twice on the same LDS puts a barrier between the two.
//   LDS:  xw   [TW][224]     fp32   the horizontal table transposed (lane x reads xw[.][x]: no bank conflicts), tap j in row j + 3, zero rows around it
//         yw   [8][taps_y]   fp32   this tile's vertical weights
//         mid  [NP R][224]   fp32   the horizontal pass of the current chunk of R source rows of each plane
//         rows [NP R][RP]    uint8  those source rows from column xlo on, zero beyond the picture (RP = W + taps_x rounded up to 4, + 8); plane p in staged rows
//                                   [p R, (p + 1) R).  R % 4 == 0 and NP R <= 8, so that a horizontal item (4 source rows, one output column) never straddles planes
// Per chunk:
//  (1) staging: a lane fetches 4 neighbouring source bytes of each plane (one dword where the layout allows it, else 4 byte loads at stride sx: 3 for channels-last)
//      and writes one LDS dword per plane; consecutive lanes cover consecutive bytes of the row.  INTER: s1 == s0 + 1 and sx == 2 (NV12) - the 8 bytes
//      U V U V U V U V of four chroma columns are fetched once as two dwords and split into the U and the V dword in registers.  The loads of chunk k + 1 are issued
//      into registers before the horizontal pass of chunk k and written to LDS after its vertical pass: two barriers per chunk, no global latency between them;
//  (2) horizontal pass, lane = output column, four source rows at a time: the taps [off, off + taps_x) are read as the aligned dwords that cover them, and byte
//      k of dword d meets weight row 4 d + k + 3 - (off & 3) - tap j = 4 d + k - (off & 3), or a zero row outside [0, taps_x): sums run in ascending j;
//  (3) vertical pass, lane = four output columns of output rows rg and rg + 4 of the tile: acc += yw[row][y - first] * mid[y], source rows y ascending.
// BS = 2: the samples are 16-bit words that hold 10 bits, v = (word >> shift) & 1023; sy, sx and the planes' addresses stay in BYTES (all even).  What changes:
//   rows [NP R][RP] uint16: two LDS dwords per staged item (one 8-byte store), at most ING_PF16 staged dwords per lane; the staged row starts at xlo rounded down
//      to a multiple of 4 columns, so that rows of an aligned surface are fetched with wide loads at any crop origin: 8 bytes per plane (else two dwords, else
//      2-byte loads); INTER (s1 == s0 + 2, sx == 4: P010) takes the 16 bytes U V U V U V U V of four chroma columns as one 16-byte load (else four dwords);
//   xw: tap j in row j + 1, TW = 2 nd + 1; the horizontal pass reads the nd = (taps_x + 2) / 2 aligned dwords that cover the taps, two samples per dword, half k of
//      dword d against weight row 2 d + k + 1 - (off & 1).  Zero rows only add exact zeros, so the sums - taps ascending, fmaf - are those of BS = 1 term by term.
// FORM = 2: the planes are PACKED into macropixels of 4 BS bytes, Y0 U Y1 V in some order (uyvy422, yuyv422, y210); pk is the byte of plane 0's first
//   sample inside its macropixel, and the launcher has checked that every byte of macropixels [0, W / 2) of a row belongs to the frame.  NP = 1 (luma, sx == 2 BS):
//   the staged row starts at xlo rounded down to 4 columns, a lane's 4 samples lie in two macropixels - 8 or 16 bytes fetched as dwords (one 16-byte load where
//   aligned), every other sample picked with v_perm_b32.  NP = 2 (chroma, s1 == s0 + 2 BS, sx == 4 BS): four chroma columns are four macropixels - 16 or 32 bytes
//   fetched once and split into the U and the V dwords.  Rows that are not 4-byte aligned and row ends take the strided loads.  What reaches LDS is the same either way.
//   BS = 2 fetches twice the dwords it stages, so it stages at most ING_PF16 / 2 per lane and chunk (the launcher sizes R for that): the fetched words of a chunk then
//   fit the registers of the plain form, all loads stay in flight together, and the kernel keeps three workgroups per CU instead of one (12.9 -> 5.0 us per frame).
// FORM = 3, BS = 2: a v210 row - the 10-bit fields Cb0 Y0 Cr0 Y1 Cb1 Y2 Cr1 Y3 .. of a 4:2:2 row, field F in bits [10 (F % 3), 10 (F % 3) + 10) of
//   little-endian word F / 3; s0 is word 0 of row 0 (4-byte aligned), sy the row pitch in bytes, s1 / sx / shift / pk are unused, the row has nw whole words (four
//   per six pixels).  NP = 1 (luma, W columns): the item of columns x .. x + 3 (x % 4 == 0) takes fields 2 x + 1, + 3, + 5, + 7 - three words from (2 x + 1) / 3.
//   NP = 2 (chroma, W = the chroma width): four chroma columns from j take fields 4 j .. 4 j + 14, U on 4 j + 4 i and V two further - six words from 4 j / 3, one
//   fetch for both planes.  Either window starts 0, 1 or 2 fields into its first word, so field t of the window lies in word t / 3 or the next: one select, one
//   shift, one mask.  The words come as one aligned dword load each (every v210 word is 4-byte aligned: no pointer tests), plain where the window lies inside the
//   row, bounded by nw at the row's end (a word at or past nw reads as 0).  Loads of whole 16-byte groups were measured 22 % slower (profiles/ingest_v210.md) and
//   are not here.  Columns at or beyond W are zeroed after the unpacking, so padding fields never reach LDS; what commit() writes is the plain 16-bit row of the
//   yuv422p10le form (shift 0) at the same xlo.  Three words are fetched for two staged dwords, so the
//   form stages at most ING_PF210 dwords per lane and chunk.  FORM = 4 is the same staging with the whole ING_PF16 budget, for rows too wide for four of them to
//   fit ING_PF210 (above ~2500 columns): more registers, one wave per SIMD - rows that wide leave LDS for one or two workgroups per CU anyway.
template <int NWD>
__device__ __forceinline__ uint32_t ing_v210_field(const uint32_t (&d)[NWD], int r, int t) {
  const int p = r + t % 3, lo = t / 3, hi = lo + 1 < NWD ? lo + 1 : NWD - 1;   // t is a constant where this is called: r + t % 3 < 3 whenever lo + 1 == NWD
  return p >= 3 ? (d[hi] >> (10 * (p - 3))) & 1023u : (d[lo] >> (10 * p)) & 1023u;
}

template <int NP, int FORM, int BS>
__device__ __forceinline__ void ing_plane_pass(unsigned char* lds, const uint8_t* __restrict__ s0, const uint8_t* __restrict__ s1, int64_t sy, int64_t sx, int H, int W,
                                               const int32_t* __restrict__ y_first, const float* __restrict__ y_w, int taps_y,
                                               const int32_t* __restrict__ x_first, const float* __restrict__ x_w, int taps_x, int R, int RP, int TW, int r0, int shift,
                                               int pk, float (&a0)[NP][4], float (&a1)[NP][4]) {
  static_assert(BS == 1 || BS == 2, "samples of one or two bytes");
  static_assert(FORM >= 0 && FORM <= 4, "plain, interleaved, packed, v210 or v210 with the whole staging budget");
  static_assert(FORM < 3 || BS == 2, "v210 stages 16-bit samples");
  constexpr bool INTER = FORM == 1;
  constexpr int PAD = BS == 1 ? 3 : 1;                                          // zero rows in front of the transposed table: samples per dword - 1
  constexpr int PF = BS == 1 ? ING_PF : FORM == 3 ? ING_PF210 : FORM == 4 ? ING_PF16 : FORM == 2 ? ING_PF16 / 2 : ING_PF16;   // packed words: twice the staged dwords are fetched, so half are staged
  float* xw = (float*)lds;
  float* yw = xw + TW * ING_OUT;
  float* mid = yw + ING_TY * taps_y;
  uint32_t* rows = (uint32_t*)(mid + NP * R * ING_OUT);
  const int tid = threadIdx.x;

  for (int i = tid; i < TW * ING_OUT; i += 256) {
    const int row = i / ING_OUT;
    if (row < PAD || row >= taps_x + PAD) xw[i] = 0.f;
  }
  for (int i = tid; i < taps_x * ING_OUT; i += 256) {
    const int x = i / taps_x, j = i - x * taps_x;                               // coalesced read of the (224, taps_x) table
    xw[(j + PAD) * ING_OUT + x] = x_w[i];
  }
  for (int i = tid; i < ING_TY * taps_y; i += 256) yw[i] = y_w[(int64_t)r0 * taps_y + i];

  int xlo = x_first[0];
  xlo = xlo < 0 ? 0 : (xlo > W ? W : xlo);
  if (BS == 2 || (FORM == 2 && NP == 1)) xlo &= ~3;
  int ys = y_first[r0], ye = y_first[r0 + ING_TY - 1] + taps_y;
  ys = ys < 0 ? 0 : ys;
  ye = ye > H ? H : ye;                                                        // rows past the picture carry the tables' zero padding: never read

  // vertical pass ownership: lanes 0..223 = (quad q of 4 columns, row pair rg): output rows r0 + rg and r0 + rg + 4
  const int q = tid % 56, rg = tid / 56;
  const bool vert = tid < 224;
  int yf0 = 0, yf1 = 0;
  if (vert) { yf0 = y_first[r0 + rg]; yf1 = y_first[r0 + rg + 4]; }
  const int Q4 = RP >> 2;                                                       // staging items (4 columns) per staged row: BS dwords each
  const int QD = Q4 * BS;                                                       // dwords per staged row
  const int nd = BS == 1 ? (taps_x + 6) >> 2 : (taps_x + 2) >> 1;               // aligned dwords that cover taps_x samples at any offset (TW = 4 nd + 3, 2 nd + 1)
  const int valid_x = W - xlo;
  const int n_stage = R * Q4;                                                   // staging items: 4 columns of one row of every plane; NP BS n_stage <= 256 * PF

  // horizontal pass ownership: items (group of 4 source rows, output column) tid and tid + 256 of (NP R / 4) * 224 <= 448; their table entries are read here, so
  // that the chunk loop issues no global load but the prefetch
  const uint32_t* hp[2];
  const float* hw[2];
  float* hm[2];
  bool hon[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int it = tid + 256 * k;
    hon[k] = it < (NP * R / 4) * ING_OUT;
    const int g = it / ING_OUT, x = it - g * ING_OUT;
    int off = hon[k] ? x_first[x] - xlo : 0;
    off = off < 0 ? 0 : (off > RP - ING_ROW_SLACK - taps_x ? RP - ING_ROW_SLACK - taps_x : off);
    hp[k] = rows + (g * 4) * QD + (BS == 1 ? off >> 2 : off >> 1);
    hw[k] = xw + (PAD - (off & PAD)) * ING_OUT + x;
    hm[k] = mid + (g * 4) * ING_OUT + x;
  }

  // staging of the R source rows of each plane from yc on, through registers: fetch() issues the loads (rows at or beyond ye and columns at or beyond W are
  // zero), commit() writes them to LDS a phase later, so the loads of chunk k + 1 travel under the horizontal pass of chunk k
  uint32_t pf[PF];
  auto fetch = [&](int yc) {
#pragma unroll
    for (int k = 0; k < PF / (NP * BS); ++k) {
      const int it = tid + 256 * k;
      uint32_t v[NP * BS];
#pragma unroll
      for (int p = 0; p < NP * BS; ++p) v[p] = 0;
      if (it < n_stage) {
        const int r = it / Q4, c = (it - r * Q4) * 4;
        const int y = yc + r;
        if (y < ye && c < valid_x) {
          const int64_t o = (int64_t)y * sy + (int64_t)(xlo + c) * sx;
          const bool full = c + 3 < valid_x;
          const uint8_t* gi = s0 + o;
          bool packed = false;
          if constexpr (FORM == 2) {
            const uint8_t* gm = gi - pk;                                        // the first of the item's macropixels
            packed = full && ((uintptr_t)gm & 3) == 0;
            if (packed) {
              const uint32_t sel = 0x01010101u * (uint32_t)(pk / BS);
              if constexpr (BS == 1 && NP == 1) {                               // Y0 . Y1 . | Y2 . Y3 .
                v[0] = __builtin_amdgcn_perm(((const uint32_t*)gm)[1], ((const uint32_t*)gm)[0], 0x06040200u + sel);
              } else if constexpr (BS == 1) {                                   // U . V . of four columns
                uint32_t d[4];
                if (((uintptr_t)gm & 15) == 0) {
                  const u32x4 w = *(const u32x4*)gm;
                  d[0] = w.x; d[1] = w.y; d[2] = w.z; d[3] = w.w;
                } else {
#pragma unroll
                  for (int i = 0; i < 4; ++i) d[i] = ((const uint32_t*)gm)[i];
                }
                const uint32_t lo = __builtin_amdgcn_perm(d[1], d[0], 0x06020400u + sel), hi = __builtin_amdgcn_perm(d[3], d[2], 0x06020400u + sel);   // U U V V
                v[0] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
                v[NP - 1] = __builtin_amdgcn_perm(hi, lo, 0x07060302u);
              } else {                                                          // 16-bit words: half pk / 2 of every other dword
                constexpr int ND = 4 * NP;
                uint32_t d[ND];
                if (((uintptr_t)gm & 15) == 0) {
#pragma unroll
                  for (int i = 0; i < NP; ++i) {
                    const u32x4 w = ((const u32x4*)gm)[i];
                    d[4 * i] = w.x; d[4 * i + 1] = w.y; d[4 * i + 2] = w.z; d[4 * i + 3] = w.w;
                  }
                } else {
#pragma unroll
                  for (int i = 0; i < ND; ++i) d[i] = ((const uint32_t*)gm)[i];
                }
                const uint32_t s16 = 0x05040100u + 2u * sel;
                if constexpr (NP == 1) {                                        // Y0 . Y1 . Y2 . Y3 .
                  v[0] = __builtin_amdgcn_perm(d[1], d[0], s16);
                  v[1] = __builtin_amdgcn_perm(d[3], d[2], s16);
                } else {                                                        // U . V . of four columns
                  v[0] = __builtin_amdgcn_perm(d[2], d[0], s16);
                  v[1] = __builtin_amdgcn_perm(d[ND - 2], d[ND - 4], s16);
                  v[2 * (NP - 1)] = __builtin_amdgcn_perm(d[3], d[1], s16);
                  v[2 * (NP - 1) + 1] = __builtin_amdgcn_perm(d[ND - 1], d[ND - 3], s16);
                }
              }
            }
          }
          if constexpr (FORM >= 3) {
            packed = true;                                                      // (nothing below applies)
            constexpr int NWD = 3 * NP;
            const uint32_t* row = (const uint32_t*)(s0 + (int64_t)y * sy);
            const int nw = 4 * (NP == 1 ? (W + 5) / 6 : (W + 2) / 3);             // whole groups of four words: six luma columns, three chroma columns
            const uint32_t f0 = NP == 1 ? 2u * (uint32_t)(xlo + c) + 1u : 4u * (uint32_t)(xlo + c);
            const int w0 = (int)(f0 / 3u), r = (int)f0 - 3 * w0;
            const bool inside = w0 + NWD <= nw;
            uint32_t d[NWD];
            if (inside) {
#pragma unroll
              for (int i = 0; i < NWD; ++i) d[i] = row[w0 + i];
            } else {                                                            // the last window of a row
#pragma unroll
              for (int i = 0; i < NWD; ++i) d[i] = w0 + i < nw ? row[w0 + i] : 0u;
            }
            uint32_t smp[4 * NP];                                               // luma: Y0 .. Y3; chroma: U0 V0 U1 V1 ..
#pragma unroll
            for (int i = 0; i < 4 * NP; ++i) smp[i] = c + i / NP < valid_x ? ing_v210_field<NWD>(d, r, 2 * i) : 0u;
            if constexpr (NP == 1) {
              v[0] = smp[0] | smp[1] << 16;
              v[1] = smp[2] | smp[3] << 16;
            } else {
              v[0] = smp[0] | smp[2] << 16;
              v[1] = smp[4] | smp[6] << 16;
              v[2 * (NP - 1)] = smp[1] | smp[3] << 16;
              v[2 * (NP - 1) + 1] = smp[5] | smp[7] << 16;
            }
          }
          if (packed) {
          } else if constexpr (BS == 1) {
            if (NP == 2 && INTER && full && ((uintptr_t)gi & 3) == 0) {
              const uint32_t a = ((const uint32_t*)gi)[0], b = ((const uint32_t*)gi)[1];
              v[0] = (a & 0xffu) | ((a >> 8) & 0xff00u) | ((b & 0xffu) << 16) | ((b << 8) & 0xff000000u);
              v[NP - 1] = ((a >> 8) & 0xffu) | ((a >> 16) & 0xff00u) | ((b << 8) & 0xff0000u) | (b & 0xff000000u);
            } else {
#pragma unroll
              for (int p = 0; p < NP; ++p) {
                const uint8_t* g = (p ? s1 : s0) + o;
                if (!INTER && sx == 1 && full && ((uintptr_t)g & 3) == 0) {
                  v[p] = *(const uint32_t*)g;
                } else {
                  uint32_t u = g[0];
                  if (c + 1 < valid_x) u |= (uint32_t)g[sx] << 8;
                  if (c + 2 < valid_x) u |= (uint32_t)g[2 * sx] << 16;
                  if (full) u |= (uint32_t)g[3 * sx] << 24;
                  v[p] = u;
                }
              }
            }
          } else {
            if (NP == 2 && INTER && full && ((uintptr_t)gi & 3) == 0) {         // dword i = U | V << 16 of column c + i
              uint32_t d[4];
              if (((uintptr_t)gi & 15) == 0) {
                const u32x4 w = *(const u32x4*)gi;
                d[0] = w.x; d[1] = w.y; d[2] = w.z; d[3] = w.w;
              } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) d[i] = ((const uint32_t*)gi)[i];
              }
              v[0] = (d[0] & 0xffffu) | (d[1] << 16);
              v[1] = (d[2] & 0xffffu) | (d[3] << 16);
              v[2 * (NP - 1)] = (d[0] >> 16) | (d[1] & 0xffff0000u);
              v[2 * (NP - 1) + 1] = (d[2] >> 16) | (d[3] & 0xffff0000u);
            } else {
#pragma unroll
              for (int p = 0; p < NP; ++p) {
                const uint8_t* g = (p ? s1 : s0) + o;
                if (!INTER && sx == 2 && full && ((uintptr_t)g & 3) == 0) {
                  if (((uintptr_t)g & 7) == 0) {
                    const u32x2 w = *(const u32x2*)g;
                    v[2 * p] = w.x; v[2 * p + 1] = w.y;
                  } else {
                    v[2 * p] = ((const uint32_t*)g)[0]; v[2 * p + 1] = ((const uint32_t*)g)[1];
                  }
                } else {
                  uint32_t u = *(const uint16_t*)g, w = 0;
                  if (c + 1 < valid_x) u |= (uint32_t)*(const uint16_t*)(g + sx) << 16;
                  if (c + 2 < valid_x) w = *(const uint16_t*)(g + 2 * sx);
                  if (full) w |= (uint32_t)*(const uint16_t*)(g + 3 * sx) << 16;
                  v[2 * p] = u; v[2 * p + 1] = w;
                }
              }
            }
          }
        }
      }
#pragma unroll
      for (int p = 0; p < NP * BS; ++p) pf[k * NP * BS + p] = v[p];
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < PF / (NP * BS); ++k) {
      const int it = tid + 256 * k;
      if (it < n_stage) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          if constexpr (BS == 1) {
            rows[p * n_stage + it] = pf[k * NP + p];
          } else {
            u32x2 w;
            w.x = pf[(k * NP + p) * 2]; w.y = pf[(k * NP + p) * 2 + 1];
            *(u32x2*)(rows + 2 * (p * n_stage + it)) = w;
          }
        }
      }
    }
  };

  if (ys < ye) {
    fetch(ys);
    commit();
  }
  __syncthreads();                                                             // rows of the first chunk, xw, yw
  for (int yc = ys; yc < ye; yc += R) {
    const bool more = yc + R < ye;                                             // block-uniform
    if (more) fetch(yc + R);
    // horizontal pass: the taps as aligned dwords against the zero-padded table
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (hon[k]) {
        const uint32_t* p0 = hp[k];
        const float* wp = hw[k];
        float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f;
        for (int d = 0; d < nd; ++d) {
          const uint32_t v0 = p0[d], v1 = p0[QD + d], v2 = p0[2 * QD + d], v3 = p0[3 * QD + d];
          if constexpr (BS == 1) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              const float w = wp[(4 * d + b) * ING_OUT];
              h0 = fmaf(w, (float)((v0 >> (8 * b)) & 255u), h0);
              h1 = fmaf(w, (float)((v1 >> (8 * b)) & 255u), h1);
              h2 = fmaf(w, (float)((v2 >> (8 * b)) & 255u), h2);
              h3 = fmaf(w, (float)((v3 >> (8 * b)) & 255u), h3);
            }
          } else {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              const float w = wp[(2 * d + b) * ING_OUT];
              const int sh = 16 * b + shift;                                   // shift <= 6: the ten bits of half b
              h0 = fmaf(w, (float)((v0 >> sh) & 1023u), h0);
              h1 = fmaf(w, (float)((v1 >> sh) & 1023u), h1);
              h2 = fmaf(w, (float)((v2 >> sh) & 1023u), h2);
              h3 = fmaf(w, (float)((v3 >> sh) & 1023u), h3);
            }
          }
        }
        float* m = hm[k];
        m[0] = h0; m[ING_OUT] = h1; m[2 * ING_OUT] = h2; m[3 * ING_OUT] = h3;
      }
    }
    __syncthreads();                                                           // mid complete; every lane is past its reads of rows
    // vertical pass over the chunk's rows
    if (vert) {
      const int n = ye - yc < R ? ye - yc : R;
      for (int r = 0; r < n; ++r) {
        const int j0 = yc + r - yf0, j1 = yc + r - yf1;
        const bool in0 = j0 >= 0 && j0 < taps_y, in1 = j1 >= 0 && j1 < taps_y;
        if (in0 || in1) {
          const float w0 = in0 ? yw[rg * taps_y + j0] : 0.f, w1 = in1 ? yw[(rg + 4) * taps_y + j1] : 0.f;
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            const f32x4 v = *(const f32x4*)(mid + (p * R + r) * ING_OUT + 4 * q);
            if (in0) { a0[p][0] = fmaf(w0, v.x, a0[p][0]); a0[p][1] = fmaf(w0, v.y, a0[p][1]); a0[p][2] = fmaf(w0, v.z, a0[p][2]); a0[p][3] = fmaf(w0, v.w, a0[p][3]); }
            if (in1) { a1[p][0] = fmaf(w1, v.x, a1[p][0]); a1[p][1] = fmaf(w1, v.y, a1[p][1]); a1[p][2] = fmaf(w1, v.z, a1[p][2]); a1[p][3] = fmaf(w1, v.w, a1[p][3]); }
          }
        }
      }
    }
    if (more) {
      commit();
      __syncthreads();                                                         // rows of the next chunk complete; every lane is past its reads of mid
    }
  }
}

// The source frame of output frame fo, clamped into the recording.
__device__ __forceinline__ int ing_pick_frame(const int32_t* __restrict__ frame_table, int fo, int n_src) {
  const int fs = frame_table[fo];
  return fs < 0 ? 0 : (fs >= n_src ? n_src - 1 : fs);
}

// Interlaced frames: n_src frames of H rows are 2 n_src fields of H / 2 rows; field f is rows p, p + 2, .. of frame f >> 1, p = (f & 1) ^ bottom_first.
// The field of output frame fo, clamped into the recording as ing_pick_frame clamps frames (2 n_src fits an int: the launchers check n_src).
struct IngField { int frame, parity; };
__device__ __forceinline__ IngField ing_pick_field(const int32_t* __restrict__ field_table, int fo, int n_src, int bottom_first) {
  int f = field_table[fo];
  f = f < 0 ? 0 : (f >= 2 * n_src ? 2 * n_src - 1 : f);
  return {f >> 1, (f & 1) ^ (bottom_first & 1)};
}

// Four fp32 levels -> round half to even, clamp to [0, 255], one byte each, column k in byte k.
__device__ __forceinline__ uint32_t ing_pack4(const float (&v)[4]) {
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) w |= (uint32_t)fminf(fmaxf(rintf(v[k]), 0.f), 255.f) << (8 * k);
  return w;
}

// One workgroup = output rows [r0, r0 + 8) of one channel of one output frame (28 row tiles x 3 channels x T_out workgroups): one ing_plane_pass over that channel's
// plane, then one 4-byte store per lane and row: 56 lanes write one full 224-byte line.
__global__ __launch_bounds__(256) void ingest_video_kernel(const uint8_t* __restrict__ raw, int64_t sf, int64_t sc, int64_t sy, int64_t sx, int n_src, int H, int W,
                                                            const int32_t* __restrict__ frame_table, const int32_t* __restrict__ y_first,
                                                            const float* __restrict__ y_w, int taps_y, const int32_t* __restrict__ x_first,
                                                            const float* __restrict__ x_w, int taps_x, uint8_t* __restrict__ out, int R, int RP, int TW) {
  extern __shared__ __align__(16) unsigned char ing_lds[];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * ING_TY, ch = blockIdx.y, fo = blockIdx.z;
  const uint8_t* src = raw + (int64_t)ing_pick_frame(frame_table, fo, n_src) * sf + (int64_t)ch * sc;
  float a0[1][4] = {}, a1[1][4] = {};
  ing_plane_pass<1, 0, 1>(ing_lds, src, src, sy, sx, H, W, y_first, y_w, taps_y, x_first, x_w, taps_x, R, RP, TW, r0, 0, 0, a0, a1);
  if (tid < 224) {
    uint8_t* o = out + (((int64_t)fo * 3 + ch) * ING_OUT + r0 + tid / 56) * ING_OUT + 4 * (tid % 56);
    *(uint32_t*)o = ing_pack4(a0[0]);
    *(uint32_t*)(o + 4 * ING_OUT) = ing_pack4(a1[0]);
  }
}

// ingest_video_kernel on the field that field_table names: the plane starts `parity` rows into the frame, its rows are two frame rows apart, it has H / 2 of them (the
// last one is frame row H - 2 + parity <= H - 1) and the vertical tables are those of its parity (y_first0 / y_w0: the rows 0, 2, ..; y_first1 / y_w1: 1, 3, ..).
__global__ __launch_bounds__(256) void ingest_video_fields_kernel(const uint8_t* __restrict__ raw, int64_t sf, int64_t sc, int64_t sy, int64_t sx, int n_src, int H, int W,
                                                                   const int32_t* __restrict__ field_table, const int32_t* __restrict__ y_first0,
                                                                   const float* __restrict__ y_w0, const int32_t* __restrict__ y_first1, const float* __restrict__ y_w1,
                                                                   int taps_y, const int32_t* __restrict__ x_first, const float* __restrict__ x_w, int taps_x,
                                                                   uint8_t* __restrict__ out, int R, int RP, int TW, int bottom_first) {
  extern __shared__ __align__(16) unsigned char ing_lds[];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * ING_TY, ch = blockIdx.y, fo = blockIdx.z;
  const IngField fl = ing_pick_field(field_table, fo, n_src, bottom_first);
  const uint8_t* src = raw + (int64_t)fl.frame * sf + (int64_t)ch * sc + (int64_t)fl.parity * sy;
  float a0[1][4] = {}, a1[1][4] = {};
  ing_plane_pass<1, 0, 1>(ing_lds, src, src, 2 * sy, sx, H >> 1, W, fl.parity ? y_first1 : y_first0, fl.parity ? y_w1 : y_w0, taps_y, x_first, x_w, taps_x, R, RP, TW, r0,
                          0, 0, a0, a1);
  if (tid < 224) {
    uint8_t* o = out + (((int64_t)fo * 3 + ch) * ING_OUT + r0 + tid / 56) * ING_OUT + 4 * (tid % 56);
    *(uint32_t*)o = ing_pack4(a0[0]);
    *(uint32_t*)(o + 4 * ING_OUT) = ing_pack4(a1[0]);
  }
}

struct IngCsc { float m[9], o[3]; };                                             // M row-major (rows R, G, B; columns Y, U, V), then the offsets

// One workgroup = output rows [r0, r0 + 8) of ALL THREE channels of one output frame: the luma plane through ing_plane_pass (chunks of R source rows), then U and
// V together (chunks of 4 rows of each; their tables replace the luma ones in the same LDS), the three resized 8 x 224 fp32 tiles staying in registers (24 per
// lane); then the colour matrix and three full 224-byte lines per output row.  BS: bytes per sample.  BS = 2 (P010: INTER, shift 6; yuv420p10le: shift 0): csx in
// bytes, v = (word >> shift) & 1023, up to ING_PF16 staging registers per lane - LDS holds two workgroups per CU at the widest rows anyway, so nothing is lost to
// the larger register budget there.  BS = 1 ignores shift.
// GEN = 0: the 4:2:0 entries - luma at the frame base with unit column stride, chroma planes of H / 2 x W / 2; the trailing arguments from y_off on are ignored, so
// these instantiations are what they were before the general entry.  GEN = 1: sf_ingest_video_yuv_planes - luma at y_off with column stride sxl,
// chroma planes of Hc x Wc; CF = 0 (separate planes: any strides) or 1 (interleaved U V: NV12, NV16, P010, P210).  GEN = 2, CF = 2: a packed 4:2:2 row (uyvy422,
// yuyv422, y210), both passes on the packed staging of ing_plane_pass; pky / pkc: the byte of Y0 / of U inside the macropixel.
template <int CF, int BS, int GEN = 0>
__global__ __launch_bounds__(256) void ingest_video_yuv_kernel(const uint8_t* __restrict__ raw, int64_t sf, int64_t sy, int64_t u_off, int64_t v_off, int64_t csy,
                                                                int64_t csx, int n_src, int H, int W, const int32_t* __restrict__ frame_table,
                                                                const int32_t* __restrict__ y_first, const float* __restrict__ y_w, int taps_y,
                                                                const int32_t* __restrict__ x_first, const float* __restrict__ x_w, int taps_x,
                                                                const int32_t* __restrict__ cy_first, const float* __restrict__ cy_w, int taps_cy,
                                                                const int32_t* __restrict__ cx_first, const float* __restrict__ cx_w, int taps_cx, IngCsc csc,
                                                                uint8_t* __restrict__ out, int R, int RP, int TW, int RPc, int TWc, int shift, int64_t y_off,
                                                                int64_t sxl, int Hc, int Wc, int pky, int pkc) {
  static_assert((GEN == 2) == (CF == 2), "the packed luma and chroma forms come together");
  extern __shared__ __align__(16) unsigned char ing_lds[];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * ING_TY, fo = blockIdx.y;
  const uint8_t* src = raw + (int64_t)ing_pick_frame(frame_table, fo, n_src) * sf;
  float ya[1][4] = {}, yb[1][4] = {}, c0[2][4] = {}, c1[2][4] = {};
  if constexpr (GEN == 0)
    ing_plane_pass<1, 0, BS>(ing_lds, src, src, sy, BS, H, W, y_first, y_w, taps_y, x_first, x_w, taps_x, R, RP, TW, r0, shift, 0, ya, yb);
  else
    ing_plane_pass<1, GEN == 2 ? 2 : 0, BS>(ing_lds, src + y_off, src + y_off, sy, sxl, H, W, y_first, y_w, taps_y, x_first, x_w, taps_x, R, RP, TW, r0, shift, pky, ya,
                                            yb);
  __syncthreads();                                                             // every lane is past the LDS of the luma pass
  ing_plane_pass<2, CF, BS>(ing_lds, src + u_off, src + v_off, csy, csx, GEN ? Hc : H >> 1, GEN ? Wc : W >> 1, cy_first, cy_w, taps_cy, cx_first, cx_w, taps_cx, 4, RPc,
                            TWc, r0, shift, GEN == 2 ? pkc : 0, c0, c1);
  if (tid < 224) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float t[3][4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float y = (h ? yb[0][k] : ya[0][k]) - csc.o[0], u = (h ? c1[0][k] : c0[0][k]) - csc.o[1], v = (h ? c1[1][k] : c0[1][k]) - csc.o[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c][k] = fmaf(csc.m[3 * c + 2], v, fmaf(csc.m[3 * c + 1], u, csc.m[3 * c] * y));
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) *(uint32_t*)(out + (((int64_t)fo * 3 + c) * ING_OUT + r0 + tid / 56 + 4 * h) * ING_OUT + 4 * (tid % 56)) = ing_pack4(t[c]);
    }
  }
}

// The end of a YUV workgroup: the colour matrix on the three resized 8 x 224 tiles in registers, three full 224-byte lines per output row.
__device__ __forceinline__ void ing_csc_store(const IngCsc& csc, const float (&ya)[1][4], const float (&yb)[1][4], const float (&c0)[2][4], const float (&c1)[2][4],
                                              uint8_t* __restrict__ out, int fo, int r0, int tid) {
  if (tid < 224) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float t[3][4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float y = (h ? yb[0][k] : ya[0][k]) - csc.o[0], u = (h ? c1[0][k] : c0[0][k]) - csc.o[1], v = (h ? c1[1][k] : c0[1][k]) - csc.o[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c][k] = fmaf(csc.m[3 * c + 2], v, fmaf(csc.m[3 * c + 1], u, csc.m[3 * c] * y));
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) *(uint32_t*)(out + (((int64_t)fo * 3 + c) * ING_OUT + r0 + tid / 56 + 4 * h) * ING_OUT + 4 * (tid % 56)) = ing_pack4(t[c]);
    }
  }
}

// ingest_video_yuv_kernel's general forms (GEN = 1, 2) on the field that field_table names, Hc == H (full vertical chroma resolution): every plane starts `parity`
// rows in - luma by parity sy, chroma by parity csy - with doubled row strides and H / 2 rows; index 0 / 1 of the vertical tables is the parity.  A packed row that the
// parity offset takes off the 4-byte grid goes through the strided loads: ing_plane_pass looks at each pointer it forms.  A kernel of its own, not a flag of
// ingest_video_yuv_kernel: that one's instantiations stay the code they were (sharing its body as an inlined function changed their register allocation).
template <int CF, int BS, int GEN>
__global__ __launch_bounds__(256) void ingest_video_yuv_fields_kernel(const uint8_t* __restrict__ raw, int64_t sf, int64_t sy, int64_t u_off, int64_t v_off, int64_t csy,
                                                                       int64_t csx, int n_src, int H, int W, const int32_t* __restrict__ field_table,
                                                                       const int32_t* __restrict__ y_first0, const float* __restrict__ y_w0,
                                                                       const int32_t* __restrict__ y_first1, const float* __restrict__ y_w1, int taps_y,
                                                                       const int32_t* __restrict__ x_first, const float* __restrict__ x_w, int taps_x,
                                                                       const int32_t* __restrict__ cy_first0, const float* __restrict__ cy_w0,
                                                                       const int32_t* __restrict__ cy_first1, const float* __restrict__ cy_w1, int taps_cy,
                                                                       const int32_t* __restrict__ cx_first, const float* __restrict__ cx_w, int taps_cx, IngCsc csc,
                                                                       uint8_t* __restrict__ out, int R, int RP, int TW, int RPc, int TWc, int shift, int64_t y_off,
                                                                       int64_t sxl, int Wc, int pky, int pkc, int bottom_first) {
  static_assert(GEN != 0, "fields go through the general entry");
  extern __shared__ __align__(16) unsigned char ing_lds[];
  const int fo = blockIdx.y;
  const IngField fl = ing_pick_field(field_table, fo, n_src, bottom_first);
  const uint8_t* src = raw + (int64_t)fl.frame * sf;
  const int64_t py = fl.parity ? sy : 0, pc = fl.parity ? csy : 0;
  const uint8_t* yp = src + y_off + py;
  const int tid = threadIdx.x, r0 = blockIdx.x * ING_TY, Hf = H >> 1;
  float ya[1][4] = {}, yb[1][4] = {}, c0[2][4] = {}, c1[2][4] = {};
  ing_plane_pass<1, GEN == 2 ? 2 : 0, BS>(ing_lds, yp, yp, 2 * sy, sxl, Hf, W, fl.parity ? y_first1 : y_first0, fl.parity ? y_w1 : y_w0, taps_y, x_first, x_w, taps_x, R, RP,
                                          TW, r0, shift, pky, ya, yb);
  __syncthreads();                                                             // every lane is past the LDS of the luma pass
  ing_plane_pass<2, CF, BS>(ing_lds, src + u_off + pc, src + v_off + pc, 2 * csy, csx, Hf, Wc, fl.parity ? cy_first1 : cy_first0, fl.parity ? cy_w1 : cy_w0, taps_cy,
                            cx_first, cx_w, taps_cx, 4, RPc, TWc, r0, shift, GEN == 2 ? pkc : 0, c0, c1);
  ing_csc_store(csc, ya, yb, c0, c1, out, fo, r0, tid);
}

// v210 frames: one workgroup = output rows [r0, r0 + 8) of all three channels of one output frame, as in ingest_video_yuv_kernel - the luma pass, then U
// and V together, both on the v210 staging of ing_plane_pass (FORM = 3) over the same words; the chroma rows are the luma rows and take the luma vertical tables.
// sy: the row pitch in bytes.  Kernels of their own, so that the instantiations above stay the code they were.  FORM: 3, or 4 for wide rows (ing_plane_pass).
template <int FORM>
__global__ __launch_bounds__(256) void ingest_video_v210_kernel(const uint8_t* __restrict__ raw, int64_t sf, int64_t sy, int n_src, int H, int W,
                                                                 const int32_t* __restrict__ frame_table, const int32_t* __restrict__ y_first,
                                                                 const float* __restrict__ y_w, int taps_y, const int32_t* __restrict__ x_first,
                                                                 const float* __restrict__ x_w, int taps_x, const int32_t* __restrict__ cx_first,
                                                                 const float* __restrict__ cx_w, int taps_cx, IngCsc csc, uint8_t* __restrict__ out, int R, int RP, int TW,
                                                                 int RPc, int TWc) {
  extern __shared__ __align__(16) unsigned char ing_lds[];
  const int tid = threadIdx.x, r0 = blockIdx.x * ING_TY, fo = blockIdx.y;
  const uint8_t* src = raw + (int64_t)ing_pick_frame(frame_table, fo, n_src) * sf;
  float ya[1][4] = {}, yb[1][4] = {}, c0[2][4] = {}, c1[2][4] = {};
  ing_plane_pass<1, FORM, 2>(ing_lds, src, src, sy, 0, H, W, y_first, y_w, taps_y, x_first, x_w, taps_x, R, RP, TW, r0, 0, 0, ya, yb);
  __syncthreads();                                                             // every lane is past the LDS of the luma pass
  ing_plane_pass<2, FORM, 2>(ing_lds, src, src, sy, 0, H, W >> 1, y_first, y_w, taps_y, cx_first, cx_w, taps_cx, 4, RPc, TWc, r0, 0, 0, c0, c1);
  ing_csc_store(csc, ya, yb, c0, c1, out, fo, r0, tid);
}

// ingest_video_v210_kernel on the field that field_table names: the rows start `parity` pitches in, are two pitches apart, there are H / 2 of them, and the vertical
// tables are those of the parity.  Every v210 word stays 4-byte aligned at any pitch the launcher admits, so both parities take the same loads.
template <int FORM>
__global__ __launch_bounds__(256) void ingest_video_v210_fields_kernel(const uint8_t* __restrict__ raw, int64_t sf, int64_t sy, int n_src, int H, int W,
                                                                        const int32_t* __restrict__ field_table, const int32_t* __restrict__ y_first0,
                                                                        const float* __restrict__ y_w0, const int32_t* __restrict__ y_first1,
                                                                        const float* __restrict__ y_w1, int taps_y, const int32_t* __restrict__ x_first,
                                                                        const float* __restrict__ x_w, int taps_x, const int32_t* __restrict__ cx_first,
                                                                        const float* __restrict__ cx_w, int taps_cx, IngCsc csc, uint8_t* __restrict__ out, int R, int RP,
                                                                        int TW, int RPc, int TWc, int bottom_first) {
  extern __shared__ __align__(16) unsigned char ing_lds[];
  const int tid = threadIdx.x, r0 = blockIdx.x * ING_TY, fo = blockIdx.y, Hf = H >> 1;
  const IngField fl = ing_pick_field(field_table, fo, n_src, bottom_first);
  const uint8_t* src = raw + (int64_t)fl.frame * sf + (fl.parity ? sy : 0);
  const int32_t* yf = fl.parity ? y_first1 : y_first0;
  const float* yw = fl.parity ? y_w1 : y_w0;
  float ya[1][4] = {}, yb[1][4] = {}, c0[2][4] = {}, c1[2][4] = {};
  ing_plane_pass<1, FORM, 2>(ing_lds, src, src, 2 * sy, 0, Hf, W, yf, yw, taps_y, x_first, x_w, taps_x, R, RP, TW, r0, 0, 0, ya, yb);
  __syncthreads();                                                             // every lane is past the LDS of the luma pass
  ing_plane_pass<2, FORM, 2>(ing_lds, src, src, 2 * sy, 0, Hf, W >> 1, yf, yw, taps_y, cx_first, cx_w, taps_cx, 4, RPc, TWc, r0, 0, 0, c0, c1);
  ing_csc_store(csc, ya, yb, c0, c1, out, fo, r0, tid);
}

// The LDS geometry of ing_plane_pass over `planes` planes of width W: the staged row RP, the padded table's rows TW, the chunk R - what ING_LDS_BYTES leave after
// the padded horizontal table and the tile's vertical weights, over the bytes of one staged row plus one row of the horizontal pass of every plane, at most
// max_rows and at most ING_PF staging registers per lane, rounded down to a multiple of 4 - and the bytes in all.  false: not even 4 rows fit.  bs: bytes per
// sample; 2 takes the padded table, the LDS cap and the register budget of the 16-bit instantiation (RP stays in samples).
struct IngGeom { int RP, TW, R, lds; };
static bool ing_geometry(int W, int taps_y, int taps_x, int planes, int max_rows, int bs, IngGeom* g, int pf = 0) {
  g->RP = ((W + taps_x + 3) & ~3) + ING_ROW_SLACK;
  g->TW = bs == 1 ? 4 * ((taps_x + 6) >> 2) + 3 : 2 * ((taps_x + 2) >> 1) + 1;
  const int fixed = (g->TW * ING_OUT + ING_TY * taps_y) * 4, per_row = planes * (g->RP * bs + ING_OUT * 4);
  const int pf_bytes = 256 * (pf ? pf : bs == 1 ? ING_PF : ING_PF16) * 4;
  int R = ((bs == 1 ? ING_LDS_BYTES : ING_LDS_BYTES16) - fixed) / per_row;
  R = R > max_rows ? max_rows : R;
  if (R > pf_bytes / (planes * g->RP * bs)) R = pf_bytes / (planes * g->RP * bs);
  g->R = R & ~3;
  g->lds = fixed + g->R * per_row;
  return g->R >= 4;
}

// The argument checks all launchers share (0, or -1 with sf_last_error set); out and W are looked at only when there is something to launch.
static int ing_check_args(const char* who, int T_out, std::initializer_list<int> taps, const void* out, int W) {
  SF_CHECK_ARG(T_out >= 0 && T_out <= 65535, "%s: T_out = %d output frames per launch (0 .. 65535: one grid dimension)", who, T_out);
  for (const int t : taps)
    SF_CHECK_ARG(t >= 1 && t <= ING_MAX_TAPS, "%s: %d filter taps out of range (1 .. %d: a short side up to 2160 at resize side 256)", who, t, ING_MAX_TAPS);
  SF_CHECK_ARG(T_out == 0 || ((uintptr_t)out & 3) == 0, "%s: out must be 4-byte aligned", who);
  SF_CHECK_ARG(T_out == 0 || W <= 1 << 20, "%s: W = %d is too wide for four staged source rows in LDS", who, W);
  return 0;
}

// SF_LAUNCH_CHECK under the name each entry has always reported a failed launch with (the macro takes __func__, which is now a shared body).
static int ing_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { sf_set_error("%s: %s", who, hipGetErrorString(e)); return (int)e; }
  return 0;
}

// What the table of an entry names: frames; the fields of an interlaced recording; or frames in the argument form of the two 4:2:0 entries, which
// keep their own kernel instantiations, checks and messages.
enum IngMode { ING_FRAMES, ING_FIELDS, ING_LEGACY420 };

// The two RGB entries.  ING_FIELDS: table holds field indices, y_first / y_w are the tables of parity 0, y_first1 / y_w1 those of parity 1, bottom_first the field
// order; otherwise those three are unused.
static int ing_rgb(const char* who, IngMode mode, const uint8_t* raw, int64_t stride_frame, int64_t stride_channel, int64_t stride_row, int64_t stride_col, int n_src, int H,
                   int W, const int32_t* table, const int32_t* y_first, const float* y_w, const int32_t* y_first1, const float* y_w1, int taps_y, const int32_t* x_first,
                   const float* x_w, int taps_x, int bottom_first, uint8_t* out, int T_out, void* stream) {
  const bool fields = mode == ING_FIELDS;
  if (ing_check_args(who, T_out, {taps_y, taps_x}, out, W)) return -1;
  SF_CHECK_ARG(n_src >= 1 && (!fields || n_src <= 0x3fffffff) && H >= 1 && W >= 1, "%s: source of %d frames %d x %d", who, n_src, H, W);
  SF_CHECK_ARG(!fields || (H >= 2 && H % 2 == 0), "%s: H = %d (two fields take an even H of at least 2)", who, H);
  SF_CHECK_ARG(stride_frame >= 0 && stride_channel >= 0 && stride_row >= 0 && stride_col >= 1, "%s: negative or zero byte stride", who);
  SF_CHECK_ARG(!fields || bottom_first == 0 || bottom_first == 1, "%s: bottom_first = %d (0: top field first, 1: bottom field first)", who, bottom_first);
  if (T_out == 0) return 0;
  SF_CHECK_ARG(raw && table && y_first && y_w && (!fields || (y_first1 && y_w1)) && x_first && x_w && out, "%s: null pointer", who);
  IngGeom g;                                                                    // fields: the field's tap count sizes the LDS
  SF_CHECK_ARG(ing_geometry(W, taps_y, taps_x, 1, ING_MAX_ROWS, 1, &g), "%s: W = %d is too wide for four staged source rows in LDS at taps_x = %d", who, W, taps_x);
  const dim3 grid(ING_OUT / ING_TY, 3, (unsigned)T_out);
  if (fields)
    hipLaunchKernelGGL(ingest_video_fields_kernel, grid, dim3(256), g.lds, (hipStream_t)stream, raw, stride_frame, stride_channel, stride_row, stride_col, n_src, H, W,
                       table, y_first, y_w, y_first1, y_w1, taps_y, x_first, x_w, taps_x, out, g.R, g.RP, g.TW, bottom_first);
  else
    hipLaunchKernelGGL(ingest_video_kernel, grid, dim3(256), g.lds, (hipStream_t)stream, raw, stride_frame, stride_channel, stride_row, stride_col, n_src, H, W, table,
                       y_first, y_w, taps_y, x_first, x_w, taps_x, out, g.R, g.RP, g.TW);
  return ing_launched(who);
}

extern "C" int sf_ingest_video(const uint8_t* raw, int64_t stride_frame, int64_t stride_channel, int64_t stride_row, int64_t stride_col, int n_src, int H, int W,
                               const int32_t* frame_table, const int32_t* y_first, const float* y_w, int taps_y, const int32_t* x_first, const float* x_w,
                               int taps_x, uint8_t* out, int T_out, void* stream) {
  return ing_rgb("sf_ingest_video", ING_FRAMES, raw, stride_frame, stride_channel, stride_row, stride_col, n_src, H, W, frame_table, y_first, y_w, nullptr, nullptr, taps_y,
                 x_first, x_w, taps_x, 0, out, T_out, stream);
}

extern "C" int sf_ingest_video_fields(const uint8_t* raw, int64_t stride_frame, int64_t stride_channel, int64_t stride_row, int64_t stride_col, int n_src, int H, int W,
                                      const int32_t* field_table, const int32_t* y_first0, const float* y_w0, const int32_t* y_first1, const float* y_w1, int taps_y,
                                      const int32_t* x_first, const float* x_w, int taps_x, int bottom_first, uint8_t* out, int T_out, void* stream) {
  return ing_rgb("sf_ingest_video_fields", ING_FIELDS, raw, stride_frame, stride_channel, stride_row, stride_col, n_src, H, W, field_table, y_first0, y_w0, y_first1, y_w1,
                 taps_y, x_first, x_w, taps_x, bottom_first, out, T_out, stream);
}

// ing_geometry for the luma pass and for the chroma pass (four rows of U and four of V per chunk) of a YUV workgroup: 0, or the pass that does not fit (1, 2).
static int ing_geometry_yuv(int W, int Wc, int taps_y, int taps_x, int taps_cy, int taps_cx, int bs, int pf, IngGeom* gy, IngGeom* gc) {
  if (!ing_geometry(W, taps_y, taps_x, 1, ING_MAX_ROWS, bs, gy, pf)) return 1;
  return ing_geometry(Wc, taps_cy, taps_cx, 2, 4, bs, gc, pf) ? 0 : 2;
}

// The YUV kernels by [bytes per sample - 1][form]; form: 0 separate chroma planes, 1 interleaved U V, 2 packed - and for frames, before those three, the two forms of
// the 4:2:0 entries (GEN = 0).
using IngYuvKernel = decltype(&ingest_video_yuv_kernel<0, 1, 0>);
using IngYuvFieldsKernel = decltype(&ingest_video_yuv_fields_kernel<0, 1, 1>);
static const IngYuvKernel ing_yuv_kernels[2][5] = {
    {ingest_video_yuv_kernel<0, 1, 0>, ingest_video_yuv_kernel<1, 1, 0>, ingest_video_yuv_kernel<0, 1, 1>, ingest_video_yuv_kernel<1, 1, 1>, ingest_video_yuv_kernel<2, 1, 2>},
    {ingest_video_yuv_kernel<0, 2, 0>, ingest_video_yuv_kernel<1, 2, 0>, ingest_video_yuv_kernel<0, 2, 1>, ingest_video_yuv_kernel<1, 2, 1>, ingest_video_yuv_kernel<2, 2, 2>}};
static const IngYuvFieldsKernel ing_yuv_fields_kernels[2][3] = {
    {ingest_video_yuv_fields_kernel<0, 1, 1>, ingest_video_yuv_fields_kernel<1, 1, 1>, ingest_video_yuv_fields_kernel<2, 1, 2>},
    {ingest_video_yuv_fields_kernel<0, 2, 1>, ingest_video_yuv_fields_kernel<1, 2, 1>, ingest_video_yuv_fields_kernel<2, 2, 2>}};

// The four YUV entries.  ING_FIELDS: frame_table holds field indices, y_first / y_w / cy_first / cy_w are the tables of parity 0, y_first1 / y_w1 / cy_first1 /
// cy_w1 those of parity 1, bottom_first the field order; otherwise those five are unused.  ING_LEGACY420: the two 4:2:0 entries, whose arguments leave y_off = 0,
// stride_col = one sample and chroma planes of H / 2 x W / 2 implied.
static int ing_planes(const char* who, IngMode mode, const void* raw, int bytes_per_sample, int64_t stride_frame, int64_t y_off, int64_t stride_row, int64_t stride_col,
                      int64_t u_off, int64_t v_off, int64_t stride_crow, int64_t stride_ccol, int shift, int n_src, int H, int W, int Hc, int Wc,
                      const int32_t* frame_table, const int32_t* y_first, const float* y_w, const int32_t* y_first1, const float* y_w1, int taps_y,
                      const int32_t* x_first, const float* x_w, int taps_x, const int32_t* cy_first, const float* cy_w, const int32_t* cy_first1, const float* cy_w1,
                      int taps_cy, const int32_t* cx_first, const float* cx_w, int taps_cx, const float* csc, int bottom_first, uint8_t* out, int T_out, void* stream) {
  const bool fields = mode == ING_FIELDS, legacy = mode == ING_LEGACY420;
  if (ing_check_args(who, T_out, {taps_y, taps_x, taps_cy, taps_cx}, out, W)) return -1;
  const int bs = bytes_per_sample;
  SF_CHECK_ARG(bs == 1 || bs == 2, "%s: bytes_per_sample = %d (1 or 2)", who, bs);
  if (legacy)
    SF_CHECK_ARG(n_src >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "%s: source of %d frames %d x %d (4:2:0 takes even H and W)", who, n_src, H, W);
  else
    SF_CHECK_ARG(n_src >= 1 && H >= 1 && W >= 1, "%s: source of %d frames %d x %d", who, n_src, H, W);
  SF_CHECK_ARG(Hc >= 1 && Hc <= H && Wc >= 1 && Wc <= W, "%s: chroma planes of %d x %d beside a luma plane of %d x %d (1 .. H by 1 .. W)", who, Hc, Wc, H, W);
  const bool strides_ok = stride_frame >= 0 && y_off >= 0 && stride_row >= 0 && u_off >= 0 && v_off >= 0 && stride_crow >= 0 && stride_col >= bs && stride_ccol >= bs;
  if (legacy)
    SF_CHECK_ARG(strides_ok, "%s: negative byte stride or offset, or a chroma column stride below %s", who, bs == 1 ? "1" : "2 bytes");
  else
    SF_CHECK_ARG(strides_ok, "%s: negative byte stride or offset, or a column stride below the %d bytes of a sample", who, bs);
  SF_CHECK_ARG(bs == 1 || ((stride_frame | y_off | stride_row | stride_col | u_off | v_off | stride_crow | stride_ccol) & 1) == 0,
               "%s: odd byte stride or offset (16-bit samples are 2-byte aligned)", who);
  SF_CHECK_ARG(shift >= 0 && shift <= 6, "%s: shift = %d (0 .. 6: ten bits of a 16-bit word)", who, shift);
  if (fields) {
    SF_CHECK_ARG(H >= 2 && H % 2 == 0, "%s: H = %d (two fields take an even H of at least 2)", who, H);
    SF_CHECK_ARG(Hc == H, "%s: chroma planes of %d rows beside %d luma rows (fields take full vertical chroma resolution: 4:2:2, 4:4:4)", who, Hc, H);
    SF_CHECK_ARG(n_src <= 0x3fffffff, "%s: source of %d frames", who, n_src);
    SF_CHECK_ARG(bottom_first == 0 || bottom_first == 1, "%s: bottom_first = %d (0: top field first, 1: bottom field first)", who, bottom_first);
  }
  if (T_out == 0) return 0;
  SF_CHECK_ARG(raw && frame_table && y_first && y_w && x_first && x_w && cy_first && cy_w && cx_first && cx_w && csc && out, "%s: null pointer", who);
  SF_CHECK_ARG(!fields || (y_first1 && y_w1 && cy_first1 && cy_w1), "%s: null pointer", who);
  SF_CHECK_ARG(bs == 1 || ((uintptr_t)raw & 1) == 0, "%s: raw must be 2-byte aligned", who);
  // packed 4:2:2: macropixels of 4 samples, Y0 and U in the first two, Y1 = Y0 + 2 samples, V = U + 2 samples, one row pitch, every byte of the W / 2 macropixels of a
  // row a sample of the frame - so whole macropixels may be fetched
  const int64_t m = y_off < u_off ? y_off : u_off;
  bool packed = stride_col == 2 * bs && stride_ccol == 4 * bs && v_off == u_off + 2 * bs && stride_crow == stride_row && Hc == H && W % 2 == 0 && Wc == W / 2 &&
                (y_off < u_off ? u_off - y_off : y_off - u_off) == bs;
  const bool inter = v_off == u_off + bs && stride_ccol == 2 * bs;               // NV12, NV16, P010, P210: one fetch of the interleaved rows serves both planes
  IngGeom gy, gc;                                                               // fields: the field's tap counts size the LDS
  // the packed 16-bit form stages half as much per chunk; rows too wide for that take the strided loads.  A smaller staging budget never gives ing_geometry a larger
  // R, so a layout that fits at half the budget fits at the whole one: the checks below have nothing to refuse then
  if (packed && bs == 2) packed = ing_geometry_yuv(W, Wc, taps_y, taps_x, taps_cy, taps_cx, bs, ING_PF16 / 2, &gy, &gc) == 0;
  if (!(packed && bs == 2)) {
    const int wide = ing_geometry_yuv(W, Wc, taps_y, taps_x, taps_cy, taps_cx, bs, 0, &gy, &gc);
    SF_CHECK_ARG(wide != 1, "%s: W = %d is too wide for four staged source rows in LDS at taps_x = %d", who, W, taps_x);
    if (legacy)
      SF_CHECK_ARG(wide != 2, "%s: W = %d is too wide for four staged rows of both chroma planes in LDS at taps_cx = %d", who, W, taps_cx);
    else
      SF_CHECK_ARG(wide != 2, "%s: Wc = %d is too wide for four staged rows of both chroma planes in LDS at taps_cx = %d", who, Wc, taps_cx);
  }
  IngCsc k;
  for (int i = 0; i < 9; ++i) k.m[i] = csc[i];
  for (int i = 0; i < 3; ++i) k.o[i] = csc[9 + i];
  const int form = packed ? 2 : inter ? 1 : 0, pky = legacy ? 0 : (int)(y_off - m), pkc = legacy ? 0 : (int)(u_off - m);
  const IngYuvKernel frames_kernel = ing_yuv_kernels[bs - 1][legacy ? form : 2 + form];
  const IngYuvFieldsKernel fields_kernel = ing_yuv_fields_kernels[bs - 1][form];
  if (bs == 2) {                                                                // more LDS than a kernel gets unasked
    const int rc = sf_prepare_kernel(fields ? (const void*)fields_kernel : (const void*)frames_kernel, ING_LDS_BYTES16, who);
    if (rc) return rc;
  }
  const dim3 grid(ING_OUT / ING_TY, (unsigned)T_out);
  const int lds = gy.lds > gc.lds ? gy.lds : gc.lds;
  if (fields)
    hipLaunchKernelGGL(fields_kernel, grid, dim3(256), lds, (hipStream_t)stream, (const uint8_t*)raw, stride_frame, stride_row, u_off, v_off, stride_crow, stride_ccol, n_src,
                       H, W, frame_table, y_first, y_w, y_first1, y_w1, taps_y, x_first, x_w, taps_x, cy_first, cy_w, cy_first1, cy_w1, taps_cy, cx_first, cx_w, taps_cx, k,
                       out, gy.R, gy.RP, gy.TW, gc.RP, gc.TW, shift, y_off, stride_col, Wc, pky, pkc, bottom_first);
  else
    hipLaunchKernelGGL(frames_kernel, grid, dim3(256), lds, (hipStream_t)stream, (const uint8_t*)raw, stride_frame, stride_row, u_off, v_off, stride_crow, stride_ccol, n_src,
                       H, W, frame_table, y_first, y_w, taps_y, x_first, x_w, taps_x, cy_first, cy_w, taps_cy, cx_first, cx_w, taps_cx, k, out, gy.R, gy.RP, gy.TW, gc.RP,
                       gc.TW, shift, y_off, stride_col, Hc, Wc, pky, pkc);
  return ing_launched(legacy ? who : __func__);                                 // (the two general entries have always reported a failed launch under this body's name)
}

extern "C" int sf_ingest_video_yuv(const uint8_t* raw, int64_t stride_frame, int64_t stride_row, int64_t u_off, int64_t v_off, int64_t stride_crow,
                                   int64_t stride_ccol, int n_src, int H, int W, const int32_t* frame_table, const int32_t* y_first, const float* y_w, int taps_y,
                                   const int32_t* x_first, const float* x_w, int taps_x, const int32_t* cy_first, const float* cy_w, int taps_cy,
                                   const int32_t* cx_first, const float* cx_w, int taps_cx, const float* csc, uint8_t* out, int T_out, void* stream) {
  return ing_planes("sf_ingest_video_yuv", ING_LEGACY420, raw, 1, stride_frame, 0, stride_row, 1, u_off, v_off, stride_crow, stride_ccol, 0, n_src, H, W, H / 2, W / 2,
                    frame_table, y_first, y_w, nullptr, nullptr, taps_y, x_first, x_w, taps_x, cy_first, cy_w, nullptr, nullptr, taps_cy, cx_first, cx_w, taps_cx, csc, 0, out,
                    T_out, stream);
}

extern "C" int sf_ingest_video_yuv16(const uint16_t* raw, int64_t stride_frame, int64_t stride_row, int64_t u_off, int64_t v_off, int64_t stride_crow,
                                     int64_t stride_ccol, int shift, int n_src, int H, int W, const int32_t* frame_table, const int32_t* y_first, const float* y_w,
                                     int taps_y, const int32_t* x_first, const float* x_w, int taps_x, const int32_t* cy_first, const float* cy_w, int taps_cy,
                                     const int32_t* cx_first, const float* cx_w, int taps_cx, const float* csc, uint8_t* out, int T_out, void* stream) {
  return ing_planes("sf_ingest_video_yuv16", ING_LEGACY420, raw, 2, stride_frame, 0, stride_row, 2, u_off, v_off, stride_crow, stride_ccol, shift, n_src, H, W, H / 2, W / 2,
                    frame_table, y_first, y_w, nullptr, nullptr, taps_y, x_first, x_w, taps_x, cy_first, cy_w, nullptr, nullptr, taps_cy, cx_first, cx_w, taps_cx, csc, 0, out,
                    T_out, stream);
}

extern "C" int sf_ingest_video_yuv_planes(const void* raw, int bytes_per_sample, int64_t stride_frame, int64_t y_off, int64_t stride_row, int64_t stride_col,
                                          int64_t u_off, int64_t v_off, int64_t stride_crow, int64_t stride_ccol, int shift, int n_src, int H, int W, int Hc, int Wc,
                                          const int32_t* frame_table, const int32_t* y_first, const float* y_w, int taps_y, const int32_t* x_first, const float* x_w,
                                          int taps_x, const int32_t* cy_first, const float* cy_w, int taps_cy, const int32_t* cx_first, const float* cx_w, int taps_cx,
                                          const float* csc, uint8_t* out, int T_out, void* stream) {
  return ing_planes("sf_ingest_video_yuv_planes", ING_FRAMES, raw, bytes_per_sample, stride_frame, y_off, stride_row, stride_col, u_off, v_off, stride_crow, stride_ccol,
                    shift, n_src, H, W, Hc, Wc, frame_table, y_first, y_w, nullptr, nullptr, taps_y, x_first, x_w, taps_x, cy_first, cy_w, nullptr, nullptr, taps_cy, cx_first,
                    cx_w, taps_cx, csc, 0, out, T_out, stream);
}

extern "C" int sf_ingest_video_yuv_planes_fields(const void* raw, int bytes_per_sample, int64_t stride_frame, int64_t y_off, int64_t stride_row, int64_t stride_col,
                                                 int64_t u_off, int64_t v_off, int64_t stride_crow, int64_t stride_ccol, int shift, int n_src, int H, int W, int Hc,
                                                 int Wc, const int32_t* field_table, const int32_t* y_first0, const float* y_w0, const int32_t* y_first1,
                                                 const float* y_w1, int taps_y, const int32_t* x_first, const float* x_w, int taps_x, const int32_t* cy_first0,
                                                 const float* cy_w0, const int32_t* cy_first1, const float* cy_w1, int taps_cy, const int32_t* cx_first,
                                                 const float* cx_w, int taps_cx, const float* csc, int bottom_first, uint8_t* out, int T_out, void* stream) {
  return ing_planes("sf_ingest_video_yuv_planes_fields", ING_FIELDS, raw, bytes_per_sample, stride_frame, y_off, stride_row, stride_col, u_off, v_off, stride_crow,
                    stride_ccol, shift, n_src, H, W, Hc, Wc, field_table, y_first0, y_w0, y_first1, y_w1, taps_y, x_first, x_w, taps_x, cy_first0, cy_w0, cy_first1, cy_w1,
                    taps_cy, cx_first, cx_w, taps_cx, csc, bottom_first, out, T_out, stream);
}

// The two v210 entries, beside ing_planes: that body's checks, messages and kernel picks are not touched.  fields: table holds field indices, y_first /
// y_w are the tables of parity 0, y_first1 / y_w1 those of parity 1, bottom_first the field order; otherwise those three are unused.
static int ing_v210(const char* who, bool fields, const void* raw, int64_t stride_frame, int64_t stride_row, int n_src, int H, int W, const int32_t* table,
                    const int32_t* y_first, const float* y_w, const int32_t* y_first1, const float* y_w1, int taps_y, const int32_t* x_first, const float* x_w, int taps_x,
                    const int32_t* cx_first, const float* cx_w, int taps_cx, const float* csc, int bottom_first, uint8_t* out, int T_out, void* stream) {
  if (ing_check_args(who, T_out, {taps_y, taps_x, taps_cx}, out, W)) return -1;
  SF_CHECK_ARG(n_src >= 1 && H >= 1 && W >= 2 && W % 2 == 0, "%s: source of %d frames %d x %d (v210 takes an even W of at least 2)", who, n_src, H, W);
  SF_CHECK_ARG(stride_frame >= 0 && stride_row >= 0 && ((stride_frame | stride_row) & 3) == 0,
               "%s: stride_frame = %lld, stride_row = %lld bytes (non-negative multiples of 4: v210 rows are 32-bit words)", who, (long long)stride_frame,
               (long long)stride_row);
  const int64_t row_bytes = 16 * (((int64_t)W + 5) / 6);
  SF_CHECK_ARG(stride_row >= row_bytes, "%s: stride_row = %lld bytes below the %lld of a row of %d pixels (16 bytes per 6 pixels, whole groups)", who,
               (long long)stride_row, (long long)row_bytes, W);
  if (fields) {
    SF_CHECK_ARG(H >= 2 && H % 2 == 0, "%s: H = %d (two fields take an even H of at least 2)", who, H);
    SF_CHECK_ARG(n_src <= 0x3fffffff, "%s: source of %d frames", who, n_src);
    SF_CHECK_ARG(bottom_first == 0 || bottom_first == 1, "%s: bottom_first = %d (0: top field first, 1: bottom field first)", who, bottom_first);
  }
  if (T_out == 0) return 0;
  SF_CHECK_ARG(raw && table && y_first && y_w && (!fields || (y_first1 && y_w1)) && x_first && x_w && cx_first && cx_w && csc && out, "%s: null pointer", who);
  SF_CHECK_ARG(((uintptr_t)raw & 3) == 0, "%s: raw must be 4-byte aligned", who);
  IngGeom gy, gc;                                                               // fields: the field's tap count sizes the LDS
  // rows too wide for four of them in ING_PF210 dwords per lane take the instantiation with the plain 16-bit budget: what that geometry fits is never refused
  const bool big = ing_geometry_yuv(W, W / 2, taps_y, taps_x, taps_y, taps_cx, 2, ING_PF210, &gy, &gc) != 0;
  const int wide = big ? ing_geometry_yuv(W, W / 2, taps_y, taps_x, taps_y, taps_cx, 2, 0, &gy, &gc) : 0;
  SF_CHECK_ARG(wide != 1, "%s: W = %d is too wide for four staged source rows in LDS at taps_x = %d", who, W, taps_x);
  SF_CHECK_ARG(wide != 2, "%s: Wc = %d is too wide for four staged rows of both chroma planes in LDS at taps_cx = %d", who, W / 2, taps_cx);
  IngCsc k;
  for (int i = 0; i < 9; ++i) k.m[i] = csc[i];
  for (int i = 0; i < 3; ++i) k.o[i] = csc[9 + i];
  const auto frames_kernel = big ? ingest_video_v210_kernel<4> : ingest_video_v210_kernel<3>;
  const auto fields_kernel = big ? ingest_video_v210_fields_kernel<4> : ingest_video_v210_fields_kernel<3>;
  const int rc = sf_prepare_kernel(fields ? (const void*)fields_kernel : (const void*)frames_kernel, ING_LDS_BYTES16, who);
  if (rc) return rc;                                                            // more LDS than a kernel gets unasked
  const dim3 grid(ING_OUT / ING_TY, (unsigned)T_out);
  const int lds = gy.lds > gc.lds ? gy.lds : gc.lds;
  if (fields)
    hipLaunchKernelGGL(fields_kernel, grid, dim3(256), lds, (hipStream_t)stream, (const uint8_t*)raw, stride_frame, stride_row, n_src, H, W, table,
                       y_first, y_w, y_first1, y_w1, taps_y, x_first, x_w, taps_x, cx_first, cx_w, taps_cx, k, out, gy.R, gy.RP, gy.TW, gc.RP, gc.TW, bottom_first);
  else
    hipLaunchKernelGGL(frames_kernel, grid, dim3(256), lds, (hipStream_t)stream, (const uint8_t*)raw, stride_frame, stride_row, n_src, H, W, table, y_first,
                       y_w, taps_y, x_first, x_w, taps_x, cx_first, cx_w, taps_cx, k, out, gy.R, gy.RP, gy.TW, gc.RP, gc.TW);
  return ing_launched(who);
}

extern "C" int sf_ingest_video_v210(const void* raw, int64_t stride_frame, int64_t stride_row, int n_src, int H, int W, const int32_t* frame_table,
                                    const int32_t* y_first, const float* y_w, int taps_y, const int32_t* x_first, const float* x_w, int taps_x, const int32_t* cx_first,
                                    const float* cx_w, int taps_cx, const float* csc, uint8_t* out, int T_out, void* stream) {
  return ing_v210("sf_ingest_video_v210", false, raw, stride_frame, stride_row, n_src, H, W, frame_table, y_first, y_w, nullptr, nullptr, taps_y, x_first, x_w, taps_x,
                  cx_first, cx_w, taps_cx, csc, 0, out, T_out, stream);
}

extern "C" int sf_ingest_video_v210_fields(const void* raw, int64_t stride_frame, int64_t stride_row, int n_src, int H, int W, const int32_t* field_table,
                                           const int32_t* y_first0, const float* y_w0, const int32_t* y_first1, const float* y_w1, int taps_y, const int32_t* x_first,
                                           const float* x_w, int taps_x, const int32_t* cx_first, const float* cx_w, int taps_cx, const float* csc, int bottom_first,
                                           uint8_t* out, int T_out, void* stream) {
  return ing_v210("sf_ingest_video_v210_fields", true, raw, stride_frame, stride_row, n_src, H, W, field_table, y_first0, y_w0, y_first1, y_w1, taps_y, x_first, x_w,
                  taps_x, cx_first, cx_w, taps_cx, csc, bottom_first, out, T_out, stream);
}

// ---- audio ---------------------------------------------------------------------------------------------------------------------------------------------------
#define RES_TILE 256           // output samples per workgroup, one per lane
#define RES_MAX_SPAN 12288     // floats of input one tile may need (48 KiB of LDS)

// y[p + n q] = sum_i xpad[q o + i] * k[p][i],  xpad[m] = x[m - width] (0 outside [0, len)),  x = the mean of the channels.  One workgroup = 256 consecutive
// outputs; their input span [q_first o - width, q_last o - width + taps) is staged once in LDS (mono, fp32), then lane t walks the taps of its phase in ascending
// order.  T = float or int16_t (scaled by 1 / 32768, exact).
template <typename T>
__global__ __launch_bounds__(RES_TILE) void resample_wave_kernel(const T* __restrict__ x, int ch, int64_t ld, int64_t len, const float* __restrict__ kern, int n,
                                                                  int taps, int o, int width, float* __restrict__ y, int64_t len_out) {
  extern __shared__ __align__(16) float res_lds[];
  const int64_t j0 = (int64_t)blockIdx.x * RES_TILE;
  int64_t j1 = j0 + RES_TILE;
  j1 = j1 > len_out ? len_out : j1;
  const int64_t q0 = j0 / n, q1 = (j1 - 1) / n;
  const int span = (int)(q1 - q0) * o + taps;
  const int64_t s0 = q0 * o - width;
  const float inv = (sizeof(T) == 2 ? 1.0f / 32768.0f : 1.0f) / (float)ch;
  for (int m = threadIdx.x; m < span; m += RES_TILE) {
    const int64_t s = s0 + m;
    float v = 0.f;
    if (s >= 0 && s < len) {
      for (int c = 0; c < ch; ++c) v += (float)x[(int64_t)c * ld + s];
      v *= inv;
    }
    res_lds[m] = v;
  }
  __syncthreads();
  const int64_t j = j0 + threadIdx.x;
  if (j >= j1) return;
  const int64_t qq = j / n;
  const int p = (int)(j - qq * n);
  const float* xs = res_lds + (int)(qq - q0) * o;
  const float* kp = kern + (int64_t)p * taps;
  float acc = 0.f;
  for (int i = 0; i < taps; ++i) acc = fmaf(xs[i], kp[i], acc);
  y[j] = acc;
}

extern "C" int sf_resample_wave(const void* x, int dtype, int ch, int64_t ld, int64_t len, const float* kernel, int n, int taps, int o, int width, float* y,
                                int64_t len_out, void* stream) {
  SF_CHECK_ARG(dtype == SF_F32 || dtype == SF_I16, "sf_resample_wave: dtype %d (fp32 = %d or int16 = %d)", dtype, SF_F32, SF_I16);
  SF_CHECK_ARG(ch >= 1 && ch <= 8, "sf_resample_wave: %d channels out of range (1 .. 8)", ch);
  SF_CHECK_ARG(len >= 0 && len_out >= 0 && ld >= len, "sf_resample_wave: len = %lld, len_out = %lld, channel stride ld = %lld", (long long)len, (long long)len_out,
               (long long)ld);
  SF_CHECK_ARG(n >= 1 && o >= 1 && taps >= 1 && width >= 0, "sf_resample_wave: n = %d phases, o = %d, taps = %d, width = %d", n, o, taps, width);
  SF_CHECK_ARG(len_out <= (len * n + o - 1) / o, "sf_resample_wave: len_out = %lld above ceil(n len / o) = %lld", (long long)len_out,
               (long long)((len * n + o - 1) / o));
  const int64_t span = (int64_t)((RES_TILE - 1) / n + 1) * o + taps;            // q_last - q_first <= (255 / n) + 1
  SF_CHECK_ARG(span <= RES_MAX_SPAN, "sf_resample_wave: a tile of %d outputs spans %lld input samples (o = %d, n = %d, taps = %d), above %d", RES_TILE,
               (long long)span, o, n, taps, RES_MAX_SPAN);
  SF_CHECK_ARG((len_out + RES_TILE - 1) / RES_TILE <= 0x7fffffffLL, "sf_resample_wave: len_out = %lld is too long for one launch", (long long)len_out);
  if (len_out == 0) return 0;
  SF_CHECK_ARG(x && kernel && y, "sf_resample_wave: null pointer");
  const dim3 grid((unsigned)((len_out + RES_TILE - 1) / RES_TILE));
  const int lds = (int)span * 4;
  if (dtype == SF_F32)
    hipLaunchKernelGGL(resample_wave_kernel<float>, grid, dim3(RES_TILE), lds, (hipStream_t)stream, (const float*)x, ch, ld, len, kernel, n, taps, o, width, y, len_out);
  else
    hipLaunchKernelGGL(resample_wave_kernel<int16_t>, grid, dim3(RES_TILE), lds, (hipStream_t)stream, (const int16_t*)x, ch, ld, len, kernel, n, taps, o, width, y,
                       len_out);
  SF_LAUNCH_CHECK();
  return 0;
}

// ---- audio, several programmes -----------------------------------------------------------------------------------------------------------------
#define MIX_MAX_CH 16          // channels of the input
#define MIX_MAX_P 8            // programmes (output rows) per launch
#define MIX_MAX_FLOATS 16384   // P * span: the mixed rows of one tile (64 KiB of LDS)
#define MIX_CHUNK RES_TILE     // input samples staged at a time
#define MIX_PITCH (MIX_CHUNK + 1)   // floats between two channels of the staged chunk: lane = sample reads without bank conflicts, c-fastest writes spread over the banks
#define MIX_LDS_BYTES (MIX_MAX_FLOATS * 4 + MIX_MAX_CH * MIX_PITCH * 4)

__device__ __forceinline__ float mix_sample(float v) { return v; }
__device__ __forceinline__ float mix_sample(int16_t v) { return (float)v * (1.0f / 32768.0f); }
__device__ __forceinline__ float mix_sample(int32_t v) { return (float)v * (1.0f / 2147483648.0f); }

// m_p[s] = sum_c mix[p][c] * xf[c][s] (fmaf, c ascending, from 0; 0 outside [0, len)),  y[p][r + n q] = sum_i mpad_p[q o + i] * k[r][i]: sf_resample_wave's rule per
// programme.  Element (c, s) of the input is x[c * stride_ch + s * stride_s].  One workgroup = 256 consecutive outputs of ALL P programmes:
//   (1) the tile's input span is read once, 256 samples at a time, into stage[ch][MIX_PITCH] (fp32, scaled): item i of a chunk is (sample i / ch, channel i % ch) when
//       the channels of a sample lie closer than the samples of a channel (interleaved) and (channel i / 256, sample i % 256) otherwise (planar), so neighbouring
//       lanes touch neighbouring addresses in either layout;
//   (2) lane t mixes sample t of the chunk into the P rows rows[p][span_ld];
//   (3) after the last chunk lane t walks the taps of its phase once per programme, ascending.
// T = float, int16_t (scaled by 2^-15) or int32_t (cast to fp32, scaled by 2^-31).
template <typename T>
__global__ __launch_bounds__(RES_TILE) void resample_wave_mix_kernel(const T* __restrict__ x, int ch, int64_t stride_ch, int64_t stride_s, int64_t len,
                                                                      const float* __restrict__ mix, int P, const float* __restrict__ kern, int n, int taps, int o,
                                                                      int width, float* __restrict__ y, int64_t ldy, int64_t len_out, int span_ld) {
  extern __shared__ __align__(16) float mix_lds[];
  float* rows = mix_lds;                                                          // [P][span_ld]
  float* stage = mix_lds + P * span_ld;                                           // [ch][MIX_PITCH]
  const int tid = threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.x * RES_TILE;
  int64_t j1 = j0 + RES_TILE;
  j1 = j1 > len_out ? len_out : j1;
  const int64_t q0 = j0 / n, q1 = (j1 - 1) / n;
  int span = (int)(q1 - q0) * o + taps;
  span = span > span_ld ? span_ld : span;                                         // (the launcher's bound: never in force)
  const int64_t s0 = q0 * o - width;
  const bool c_fast = stride_ch < stride_s;
  for (int m0 = 0; m0 < span; m0 += MIX_CHUNK) {
    const int cnt = span - m0 < MIX_CHUNK ? span - m0 : MIX_CHUNK;
    const int items = c_fast ? cnt * ch : MIX_CHUNK * ch;
    for (int i = tid; i < items; i += RES_TILE) {
      int c, m;
      if (c_fast) { m = i / ch; c = i - m * ch; } else { c = i / MIX_CHUNK; m = i - c * MIX_CHUNK; }
      const int64_t s = s0 + m0 + m;
      float v = 0.f;
      if (m < cnt && s >= 0 && s < len) v = mix_sample(x[(int64_t)c * stride_ch + s * stride_s]);
      stage[c * MIX_PITCH + m] = v;
    }
    __syncthreads();
    if (tid < cnt) {
      const int64_t s = s0 + m0 + tid;
      const bool inside = s >= 0 && s < len;
      for (int p = 0; p < P; ++p) {
        const float* mp = mix + p * ch;
        float acc = 0.f;
        for (int c = 0; c < ch; ++c) acc = fmaf(mp[c], stage[c * MIX_PITCH + tid], acc);
        rows[p * span_ld + m0 + tid] = inside ? acc : 0.f;
      }
    }
    __syncthreads();
  }
  const int64_t j = j0 + tid;
  if (j >= j1) return;
  const int64_t qq = j / n;
  const int r = (int)(j - qq * n);
  const float* kp = kern + (int64_t)r * taps;
  const int off = (int)(qq - q0) * o;
  for (int p = 0; p < P; ++p) {
    const float* xs = rows + p * span_ld + off;
    float acc = 0.f;
    for (int i = 0; i < taps; ++i) acc = fmaf(xs[i], kp[i], acc);
    y[(int64_t)p * ldy + j] = acc;
  }
}

extern "C" int sf_resample_wave_mix(const void* x, int dtype, int ch, int64_t stride_ch, int64_t stride_s, int64_t len, const float* mix, int P, const float* kernel,
                                    int n, int taps, int o, int width, float* y, int64_t ldy, int64_t len_out, void* stream) {
  SF_CHECK_ARG(dtype == SF_F32 || dtype == SF_I16 || dtype == SF_I32, "sf_resample_wave_mix: dtype %d (fp32 = %d, int16 = %d or int32 = %d)", dtype, SF_F32, SF_I16,
               SF_I32);
  SF_CHECK_ARG(ch >= 1 && ch <= MIX_MAX_CH, "sf_resample_wave_mix: %d channels out of range (1 .. %d)", ch, MIX_MAX_CH);
  SF_CHECK_ARG(P >= 1 && P <= MIX_MAX_P, "sf_resample_wave_mix: %d programmes out of range (1 .. %d per launch)", P, MIX_MAX_P);
  SF_CHECK_ARG(len >= 0 && len_out >= 0 && stride_ch >= 1 && stride_s >= 1, "sf_resample_wave_mix: len = %lld, len_out = %lld, strides %lld (channel) and %lld (sample)",
               (long long)len, (long long)len_out, (long long)stride_ch, (long long)stride_s);
  SF_CHECK_ARG(n >= 1 && o >= 1 && taps >= 1 && width >= 0, "sf_resample_wave_mix: n = %d phases, o = %d, taps = %d, width = %d", n, o, taps, width);
  SF_CHECK_ARG(len_out <= (len * n + o - 1) / o, "sf_resample_wave_mix: len_out = %lld above ceil(n len / o) = %lld", (long long)len_out,
               (long long)((len * n + o - 1) / o));
  SF_CHECK_ARG(ldy >= len_out, "sf_resample_wave_mix: row stride ldy = %lld below len_out = %lld", (long long)ldy, (long long)len_out);
  const int64_t span = (int64_t)((RES_TILE - 1) / n + 1) * o + taps;            // q_last - q_first <= (255 / n) + 1
  SF_CHECK_ARG((int64_t)P * span <= MIX_MAX_FLOATS, "sf_resample_wave_mix: a tile of %d outputs spans %lld input samples (o = %d, n = %d, taps = %d); %d programmes "
               "of them are above the %d floats of LDS: at most %lld programmes per launch", RES_TILE, (long long)span, o, n, taps, P, MIX_MAX_FLOATS,
               (long long)(MIX_MAX_FLOATS / span));
  SF_CHECK_ARG((len_out + RES_TILE - 1) / RES_TILE <= 0x7fffffffLL, "sf_resample_wave_mix: len_out = %lld is too long for one launch", (long long)len_out);
  if (len_out == 0) return 0;
  SF_CHECK_ARG(x && mix && kernel && y, "sf_resample_wave_mix: null pointer");
  const dim3 grid((unsigned)((len_out + RES_TILE - 1) / RES_TILE));
  const int lds = ((int)(P * span) + ch * MIX_PITCH) * 4;
  int rc = 0;
  auto launch = [&](auto kern, auto* xs) {
    if ((rc = sf_prepare_kernel((const void*)kern, MIX_LDS_BYTES, "sf_resample_wave_mix")) != 0) return;
    hipLaunchKernelGGL(kern, grid, dim3(RES_TILE), lds, (hipStream_t)stream, xs, ch, stride_ch, stride_s, len, mix, P, kernel, n, taps, o, width, y, ldy, len_out,
                       (int)span);
  };
  if (dtype == SF_F32) launch(resample_wave_mix_kernel<float>, (const float*)x);
  else if (dtype == SF_I16) launch(resample_wave_mix_kernel<int16_t>, (const int16_t*)x);
  else launch(resample_wave_mix_kernel<int32_t>, (const int32_t*)x);
  if (rc != 0) return rc;
  SF_LAUNCH_CHECK();
  return 0;
}
