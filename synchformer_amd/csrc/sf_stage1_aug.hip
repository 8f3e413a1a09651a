// Stage-1 (AVCLIP pre-training) train-time augmentations on the device: the pixel and sample operations of transform_sequence_train of
// configs/segment_avclip.yaml (dataset/transforms.py:110-218, 402-500, 672-812), restated.  The host draws the DECISIONS
// (synchformer_amd.augment.Stage1Sampler) and uploads two int32 tables; the layouts are in include/synchformer_hip.h.
//
//   video:  uint8 clips (n_clips, clip_frames, 3, H, W)  ->  uint8 segments (n_clips * n_seg, 16, 3, 224, 224)
//     crop at (y0, x0), 224 or a 192 crop resampled bilinearly to 224 (RGBSpatialCropSometimesUpscale), segmenting (GenerateMultipleSegments),
//     per segment ColorJitter(0.8, 0.8, 0.8, 0.2) in a drawn order + RandomGrayscale (RandomApplyColorDistortion), RandomHorizontalFlip.
//     The arithmetic is torchvision 0.15's tensor path on uint8: every op truncates back to uint8, blends are r * a + q * b in fp32 with each
//     product and the sum rounded separately - so FP CONTRACTION IS OFF in this file (an FMA changes truncations).
//     Contrast blends with the PER-FRAME mean of the gray image as it is when contrast is reached: pass 0 (one workgroup per frame of a jittered
//     segment) sums that gray image exactly in int32, pass 1 recomputes the chain from the source with the mean and writes the segment.
//   audio:  fp32 wave (n_clips, clip_samples)  ->  fp32 segments (n_clips * n_seg, n_samples)
//     gather of the windows, then per segment Vol(2.0, 'amplitude'), lowpass_biquad(100 Hz, Q 0.707) and Gaussian noise 0.01 * N(0, 1) from
//     Philox4x32-10 keyed by the segment's seed and counted by the sample index (no generator state in memory).
// The tables are on the device, so the launchers cannot check them: rows are validated on the host before upload and the kernels CLAMP every
// entry into its clip - a bad row reads wrong pixels / samples, never outside the clip.
#include "sf_common.h"
#include "../../include/synchformer_hip.h"

#pragma clang fp contract(off)

#define S1_PIX (224 * 224)              // 50176 pixels per frame
#define S1_RUNS (224 * 14)              // 16-pixel runs per frame
#define S1_SMALL 192

struct S1Clip {
  int64_t frame;                        // first frame of the segment, absolute in the clips tensor
  int y0, x0, side;
};

__device__ __forceinline__ S1Clip s1_clip_row(const int* __restrict__ clip_table, int clip_ld, int64_t n, int n_seg_clip, int64_t clip_frames, int H,
                                              int W, int seg_stride) {
  const int64_t clip = n / n_seg_clip, sidx = n - clip * n_seg_clip;
  const int* row = clip_table + clip * clip_ld;
  const int span = (n_seg_clip - 1) * seg_stride + 16;
  S1Clip c;
  c.side = row[3] == S1_SMALL ? S1_SMALL : 224;
  const int frame0 = min(max(row[0], 0), (int)(clip_frames - span));
  c.y0 = min(max(row[1], 0), H - c.side);
  c.x0 = min(max(row[2], 0), W - c.side);
  c.frame = clip * clip_frames + frame0 + sidx * seg_stride;
  return c;
}

// 16 consecutive bytes from any address: the 4-byte-aligned words that cover them, funnel-shifted into place (as im2col_video_crops_kernel).  The
// fifth word is read only when the run is misaligned, and through byte loads where it would cross `end` (a tensor whose size is no multiple of 4).
__device__ __forceinline__ void s1_load16(const uint8_t* __restrict__ p, const uint8_t* __restrict__ end, float* __restrict__ v) {
  const int sh = (int)((uintptr_t)p & 3);
  const uint32_t* base = reinterpret_cast<const uint32_t*>(p - sh);
  typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
  const u32x4a4 lo = *reinterpret_cast<const u32x4a4*>(base);
  uint32_t hi = 0u;
  if (sh) {
    const uint8_t* h = reinterpret_cast<const uint8_t*>(base + 4);
    if (h + 4 <= end) hi = base[4];
    else
      for (int k = 0; k < 3; ++k)
        if (h + k < end) hi |= (uint32_t)h[k] << (8 * k);
  }
  uint32_t s[4];
  s[0] = __builtin_amdgcn_alignbyte(lo.y, lo.x, sh);
  s[1] = __builtin_amdgcn_alignbyte(lo.z, lo.y, sh);
  s[2] = __builtin_amdgcn_alignbyte(lo.w, lo.z, sh);
  s[3] = __builtin_amdgcn_alignbyte(hi, lo.w, sh);
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = (float)((s[j >> 2] >> (8 * (j & 3))) & 0xffu);
}

// The 16-pixel run w of row y of one frame, all three channels, as integer-valued floats: the 224 crop, or the 192 crop resampled to 224 as
// F.interpolate(mode='bilinear', align_corners=False) does in fp32 (source coordinate scale * (dst + 0.5) - 0.5 clamped at 0, the two-tap weights
// 1 - lambda and lambda, rows combined after columns), rounded half to even.
__device__ __forceinline__ void s1_load_px(const uint8_t* __restrict__ vid, const uint8_t* __restrict__ end, const S1Clip& c, int f, int y, int w, int H,
                                           int W, float* __restrict__ r, float* __restrict__ g, float* __restrict__ b) {
  const uint8_t* fr = vid + (c.frame + f) * 3 * (int64_t)H * W;
  const int64_t plane = (int64_t)H * W;
  if (c.side == 224) {
    const uint8_t* p = fr + (int64_t)(c.y0 + y) * W + c.x0 + 16 * w;
    s1_load16(p, end, r);
    s1_load16(p + plane, end, g);
    s1_load16(p + 2 * plane, end, b);
    return;
  }
  const float scale = (float)S1_SMALL / 224.0f;
  float sy = scale * ((float)y + 0.5f) - 0.5f;
  sy = sy < 0.f ? 0.f : sy;
  const int iy0 = min((int)sy, S1_SMALL - 1), iy1 = iy0 + (iy0 < S1_SMALL - 1 ? 1 : 0);
  const float hy1 = fminf(fmaxf(sy - (float)iy0, 0.f), 1.f), hy0 = 1.f - hy1;
  const uint8_t* r0 = fr + (int64_t)(c.y0 + iy0) * W + c.x0;
  const uint8_t* r1 = fr + (int64_t)(c.y0 + iy1) * W + c.x0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    float sx = scale * ((float)(16 * w + j) + 0.5f) - 0.5f;
    sx = sx < 0.f ? 0.f : sx;
    const int ix0 = min((int)sx, S1_SMALL - 1), ix1 = ix0 + (ix0 < S1_SMALL - 1 ? 1 : 0);
    const float wx1 = fminf(fmaxf(sx - (float)ix0, 0.f), 1.f), wx0 = 1.f - wx1;
    float o[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float p00 = (float)r0[ch * plane + ix0], p01 = (float)r0[ch * plane + ix1];
      const float p10 = (float)r1[ch * plane + ix0], p11 = (float)r1[ch * plane + ix1];
      o[ch] = rintf(hy0 * (wx0 * p00 + wx1 * p01) + hy1 * (wx0 * p10 + wx1 * p11));
    }
    r[j] = o[0]; g[j] = o[1]; b[j] = o[2];
  }
}

// torchvision _blend on uint8: (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 255).to(uint8); rr = float32(ratio), qq = float32(1.0 - ratio)
__device__ __forceinline__ float s1_blend(float rr, float a, float qq, float b) {
  const float t = rr * a, u = qq * b;
  return truncf(fminf(fmaxf(t + u, 0.f), 255.f));
}

// rgb_to_grayscale on uint8: (0.2989 * r + 0.587 * g + 0.114 * b).to(uint8), evaluated left to right
__device__ __forceinline__ float s1_gray(float r, float g, float b) {
  const float t = 0.2989f * r + 0.587f * g;
  return truncf(t + 0.114f * b);
}

// adjust_hue on uint8: x / 255 -> _rgb2hsv -> h = (h + f) mod 1 -> _hsv2rgb -> trunc(v * (255 + 1 - 1e-3)), in fp32
__device__ __forceinline__ void s1_hue(float& R, float& G, float& B, float hf) {
  const float r = R / 255.0f, g = G / 255.0f, b = B / 255.0f;
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.0f : maxc);
  const float crd = eqc ? 1.0f : cr;
  const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
  const float hr = maxc == r ? bc - gc : 0.f;
  const float hg = (maxc == g && maxc != r) ? 2.0f + rc - bc : 0.f;
  const float hb = (maxc != g && maxc != r) ? 4.0f + gc - rc : 0.f;
  float h = hr + hg + hb;
  h = h / 6.0f + 1.0f;
  h = h - truncf(h);                                    // torch.fmod(h / 6 + 1, 1): the argument is positive
  h = h + hf;
  h = h - floorf(h);                                    // Python's % 1.0 (torch.remainder): exact for h >= 0, h + 1 rounded for h < 0 - both as here
  const float h6 = h * 6.0f, fi = floorf(h6), f = h6 - fi;
  const int i = ((int)fi) % 6;                          // h may round up to exactly 1: sector 6 is sector 0
  const float v = maxc;
  const float p = fminf(fmaxf(v * (1.0f - s), 0.f), 1.f);
  const float q = fminf(fmaxf(v * (1.0f - s * f), 0.f), 1.f);
  const float t = fminf(fmaxf(v * (1.0f - s * (1.0f - f)), 0.f), 1.f);
  const float o0 = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
  const float o1 = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
  const float o2 = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
  R = truncf(o0 * 255.999f); G = truncf(o1 * 255.999f); B = truncf(o2 * 255.999f);
}

// ops k_lo .. k_hi - 1 of a segment's jitter order on a 16-pixel run.  Codes as torchvision's fn_idx: 0 brightness, 1 contrast, 2 saturation,
// 3 hue; anything else is no op.  `mean` is used by contrast only.
__device__ __forceinline__ void s1_apply_ops(float* __restrict__ r, float* __restrict__ g, float* __restrict__ b, const int* __restrict__ row, int k_lo,
                                             int k_hi, float mean) {
#pragma unroll 1
  for (int k = k_lo; k < k_hi; ++k) {
    const int op = row[SF_S1_SEG_OP0 + k];
    if (op == 0) {
      const float rr = __int_as_float(row[SF_S1_SEG_BRIGHT_R]), qq = __int_as_float(row[SF_S1_SEG_BRIGHT_R + 1]);
#pragma unroll
      for (int j = 0; j < 16; ++j) { r[j] = s1_blend(rr, r[j], qq, 0.f); g[j] = s1_blend(rr, g[j], qq, 0.f); b[j] = s1_blend(rr, b[j], qq, 0.f); }
    } else if (op == 1) {
      const float rr = __int_as_float(row[SF_S1_SEG_CONTRAST_R]), qq = __int_as_float(row[SF_S1_SEG_CONTRAST_R + 1]);
#pragma unroll
      for (int j = 0; j < 16; ++j) { r[j] = s1_blend(rr, r[j], qq, mean); g[j] = s1_blend(rr, g[j], qq, mean); b[j] = s1_blend(rr, b[j], qq, mean); }
    } else if (op == 2) {
      const float rr = __int_as_float(row[SF_S1_SEG_SATUR_R]), qq = __int_as_float(row[SF_S1_SEG_SATUR_R + 1]);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float y = s1_gray(r[j], g[j], b[j]);
        r[j] = s1_blend(rr, r[j], qq, y); g[j] = s1_blend(rr, g[j], qq, y); b[j] = s1_blend(rr, b[j], qq, y);
      }
    } else if (op == 3) {
      const float hf = __int_as_float(row[SF_S1_SEG_HUE]);
#pragma unroll
      for (int j = 0; j < 16; ++j) s1_hue(r[j], g[j], b[j], hf);
    }
  }
}

// position of the (first) contrast op in the order, 4 when there is none
__device__ __forceinline__ int s1_contrast_pos(const int* __restrict__ row) {
  int kc = 4;
  for (int k = 3; k >= 0; --k)
    if (row[SF_S1_SEG_OP0 + k] == 1) kc = k;
  return kc;
}

// pass 0: grid (16 frames, segments).  sums[n * 16 + f] = sum over the frame of the gray image in front of the contrast op (exact in int32).
__global__ __launch_bounds__(256) void s1_video_mean_kernel(const uint8_t* __restrict__ vid, const uint8_t* __restrict__ end, const int* __restrict__ clip_table,
                                                             int clip_ld, const int* __restrict__ seg_table, int seg_ld, int* __restrict__ sums, int n_seg_clip,
                                                             int64_t clip_frames, int H, int W, int seg_stride) {
  __shared__ int part[4];
  const int f = blockIdx.x;
  const int64_t n = blockIdx.y;
  const int* row = seg_table + n * seg_ld;
  if (row[SF_S1_SEG_JITTER] == 0) return;
  const int kc = s1_contrast_pos(row);
  if (kc == 4) return;
  const S1Clip c = s1_clip_row(clip_table, clip_ld, n, n_seg_clip, clip_frames, H, W, seg_stride);
  int acc = 0;
  for (int i = threadIdx.x; i < S1_RUNS; i += 256) {
    const int y = i / 14, w = i - y * 14;
    float r[16], g[16], b[16];
    s1_load_px(vid, end, c, f, y, w, H, W, r, g, b);
    s1_apply_ops(r, g, b, row, 0, kc, 0.f);
#pragma unroll
    for (int j = 0; j < 16; ++j) acc += (int)s1_gray(r[j], g[j], b[j]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) sums[n * 16 + f] = part[0] + part[1] + part[2] + part[3];
}

// pass 1: grid (196, segments), one 16-pixel run of all three channels per thread.
__global__ __launch_bounds__(256) void s1_video_augment_kernel(const uint8_t* __restrict__ vid, const uint8_t* __restrict__ end, const int* __restrict__ clip_table,
                                                                int clip_ld, const int* __restrict__ seg_table, int seg_ld, const int* __restrict__ sums,
                                                                uint8_t* __restrict__ out, int n_seg_clip, int64_t clip_frames, int H, int W, int seg_stride) {
  const int item = blockIdx.x * 256 + threadIdx.x;          // < 16 * 3136 = 196 * 256
  const int64_t n = blockIdx.y;
  const int w = item % 14, y = (item / 14) % 224, f = item / S1_RUNS;
  const int* row = seg_table + n * seg_ld;
  const S1Clip c = s1_clip_row(clip_table, clip_ld, n, n_seg_clip, clip_frames, H, W, seg_stride);
  float r[16], g[16], b[16];
  s1_load_px(vid, end, c, f, y, w, H, W, r, g, b);
  if (row[SF_S1_SEG_JITTER] != 0) {
    const float mean = s1_contrast_pos(row) < 4 ? (float)sums[n * 16 + f] / (float)S1_PIX : 0.f;
    s1_apply_ops(r, g, b, row, 0, 4, mean);
  }
  if (row[SF_S1_SEG_GRAY] != 0) {
#pragma unroll
    for (int j = 0; j < 16; ++j) r[j] = g[j] = b[j] = s1_gray(r[j], g[j], b[j]);
  }
  const bool flip = row[SF_S1_SEG_FLIP] != 0;
  uint8_t* o = out + (((n * 16 + f) * 3) * 224 + y) * (int64_t)224 + 16 * (flip ? 13 - w : w);
  const float* ch[3] = {r, g, b};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    uint32_t q[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const float* s = ch[k] + 4 * d;
      q[d] = flip ? ((uint32_t)s[3] | (uint32_t)s[2] << 8 | (uint32_t)s[1] << 16 | (uint32_t)s[0] << 24)
                  : ((uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24);
    }
    *reinterpret_cast<uint4*>(o + (int64_t)k * S1_PIX) = flip ? make_uint4(q[3], q[2], q[1], q[0]) : make_uint4(q[0], q[1], q[2], q[3]);
  }
}

extern "C" int sf_stage1_video_augment(const uint8_t* vid, int64_t n_clips, int64_t clip_frames, int H, int W, const int* clip_table, int clip_ld,
                                       const int* seg_table, int seg_ld, int seg_stride, int n_seg, int* frame_sums, uint8_t* out, void* stream) {
  SF_CHECK_ARG(vid && clip_table && seg_table && frame_sums && out, "sf_stage1_video_augment: null pointer");
  SF_CHECK_ARG(((uintptr_t)vid & 3) == 0 && ((uintptr_t)out & 15) == 0, "sf_stage1_video_augment: vid must be 4-byte and out 16-byte aligned");
  SF_CHECK_ARG(H >= 224 && W >= 224 && clip_ld >= SF_S1_CLIP_COLS && seg_ld >= SF_S1_SEG_COLS,
               "sf_stage1_video_augment: frames %dx%d smaller than the 224 crop, or table rows of %d / %d entries (>= %d / %d)", H, W, clip_ld, seg_ld,
               SF_S1_CLIP_COLS, SF_S1_SEG_COLS);
  SF_CHECK_ARG(n_seg >= 1 && seg_stride >= 0 && (int64_t)(n_seg - 1) * seg_stride + 16 <= clip_frames,
               "sf_stage1_video_augment: %d segments of stride %d do not fit %lld frames", n_seg, seg_stride, (long long)clip_frames);
  SF_CHECK_ARG(clip_frames < (1 << 30) && n_clips >= 0 && n_clips * n_seg < 65536, "sf_stage1_video_augment: at most 65535 segments per call");
  if (n_clips == 0) return 0;
  const uint8_t* end = vid + n_clips * clip_frames * 3 * (int64_t)H * W;
  const unsigned N = (unsigned)(n_clips * n_seg);
  hipLaunchKernelGGL(s1_video_mean_kernel, dim3(16, N), dim3(256), 0, (hipStream_t)stream, vid, end, clip_table, clip_ld, seg_table, seg_ld, frame_sums,
                     n_seg, clip_frames, H, W, seg_stride);
  SF_LAUNCH_CHECK();
  hipLaunchKernelGGL(s1_video_augment_kernel, dim3(16 * S1_RUNS / 256, N), dim3(256), 0, (hipStream_t)stream, vid, end, clip_table, clip_ld, seg_table,
                     seg_ld, frame_sums, out, n_seg, clip_frames, H, W, seg_stride);
  SF_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------
// audio
// ------------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11): counter (idx, 0, 0, 0), key (seed, 0) -> two of the four output words -> one Box-Muller normal.
__device__ __forceinline__ float s1_normal(uint32_t seed, uint32_t idx) {
  uint32_t c0 = idx, c1 = 0u, c2 = 0u, c3 = 0u, k0 = seed, k1 = 0u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  const float u1 = ((float)(c0 >> 8) + 1.0f) * (1.0f / 16777216.0f);      // (0, 1]
  const float u2 = (float)(c1 >> 8) * (1.0f / 16777216.0f);              // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

__device__ __forceinline__ int64_t s1_audio_start(const int* __restrict__ clip_table, int clip_ld, int64_t n, int n_seg_clip, int64_t clip_samples,
                                                   int64_t seg_stride, int n_samples) {
  const int64_t clip = n / n_seg_clip, sidx = n - clip * n_seg_clip;
  const int64_t max_start = clip_samples - ((int64_t)(n_seg_clip - 1) * seg_stride + n_samples);
  const int64_t s0 = min(max((int64_t)clip_table[clip * clip_ld + SF_S1_CLIP_SAMPLE0], (int64_t)0), max_start);
  return clip * clip_samples + s0 + sidx * seg_stride;
}

// gather + volume (+ the noise of segments without a lowpass; with one, the noise follows the filter in the next launch).  grid (blocks, segments)
__global__ __launch_bounds__(256) void s1_audio_gather_kernel(const float* __restrict__ wave, const int* __restrict__ clip_table, int clip_ld,
                                                               const int* __restrict__ seg_table, int seg_ld, float* __restrict__ out, int n_seg_clip,
                                                               int64_t clip_samples, int64_t seg_stride, int n_samples, float noise_amp) {
  const int64_t n = blockIdx.y;
  const int* row = seg_table + n * seg_ld;
  const int flags = row[SF_S1_SEG_AUDIO];
  const uint32_t seed = (uint32_t)row[SF_S1_SEG_SEED];
  const float* src = wave + s1_audio_start(clip_table, clip_ld, n, n_seg_clip, clip_samples, seg_stride, n_samples);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_samples; i += gridDim.x * 256) {
    float x = src[i];
    if (flags & SF_S1_AUDIO_VOLUME) x = fminf(fmaxf(2.0f * x, -1.f), 1.f);
    if ((flags & (SF_S1_AUDIO_LOWPASS | SF_S1_AUDIO_NOISE)) == SF_S1_AUDIO_NOISE) x = x + noise_amp * s1_normal(seed, (uint32_t)i);
    out[n * n_samples + i] = x;
  }
}

// lowpass_biquad in place, one workgroup of 64 per flagged segment: chunks of 1024 samples go through LDS (coalesced in and out), lane 0 runs the
// recurrence  y[i] = (b0 x[i] + b1 x[i-1] + b2 x[i-2]) - (a1 y[i-1] + a2 y[i-2])  from zero state, eight samples per trip with the loads in front
// (input and output live in separate arrays, so the next loads do not wait for the stores); the output is clamped to [-1, 1] (lfilter(clamp=True))
// on the way out - the recurrence itself runs on the unclamped values - and the noise is added there.
#define S1_LP_CHUNK 1024
__global__ __launch_bounds__(64) void s1_audio_lowpass_kernel(const int* __restrict__ seg_table, int seg_ld, float* __restrict__ out, int n_samples, float b0,
                                                              float b1, float b2, float a1, float a2, float noise_amp) {
  __shared__ float xin[S1_LP_CHUNK], yout[S1_LP_CHUNK];
  const int64_t n = blockIdx.x;
  const int* row = seg_table + n * seg_ld;
  const int flags = row[SF_S1_SEG_AUDIO];
  if (!(flags & SF_S1_AUDIO_LOWPASS)) return;
  const uint32_t seed = (uint32_t)row[SF_S1_SEG_SEED];
  float* x = out + n * n_samples;
  float x1 = 0.f, x2 = 0.f, y1 = 0.f, y2 = 0.f;
  for (int c0 = 0; c0 < n_samples; c0 += S1_LP_CHUNK) {
    const int len = min(S1_LP_CHUNK, n_samples - c0);
    for (int i = threadIdx.x; i < S1_LP_CHUNK; i += 64) xin[i] = i < len ? x[c0 + i] : 0.f;      // a short chunk is the LAST one: its zero tail gives unused outputs and a state nobody reads
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 0; i < len; i += 8) {
        float xv[8], yv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) xv[k] = xin[i + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float fx = b0 * xv[k] + b1 * x1 + b2 * x2;
          const float fy = a1 * y1 + a2 * y2;
          yv[k] = fx - fy;
          x2 = x1; x1 = xv[k]; y2 = y1; y1 = yv[k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) yout[i + k] = yv[k];
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < len; i += 64) {
      float v = fminf(fmaxf(yout[i], -1.f), 1.f);
      if (flags & SF_S1_AUDIO_NOISE) v = v + noise_amp * s1_normal(seed, (uint32_t)(c0 + i));
      x[c0 + i] = v;
    }
    __syncthreads();
  }
}

extern "C" int sf_stage1_audio_augment(const float* wave, int64_t n_clips, int64_t clip_samples, const int* clip_table, int clip_ld, const int* seg_table,
                                       int seg_ld, int64_t seg_stride, int n_seg, int n_samples, float b0, float b1, float b2, float a1, float a2,
                                       float noise_amp, float* out, void* stream) {
  SF_CHECK_ARG(wave && clip_table && seg_table && out, "sf_stage1_audio_augment: null pointer");
  SF_CHECK_ARG(clip_ld >= SF_S1_CLIP_COLS && seg_ld >= SF_S1_SEG_COLS, "sf_stage1_audio_augment: table rows of %d / %d entries (>= %d / %d)", clip_ld, seg_ld,
               SF_S1_CLIP_COLS, SF_S1_SEG_COLS);
  SF_CHECK_ARG(n_seg >= 1 && n_samples >= 1 && seg_stride >= 0 && (int64_t)(n_seg - 1) * seg_stride + n_samples <= clip_samples,
               "sf_stage1_audio_augment: %d segments [s*%lld, +%d) do not fit %lld samples", n_seg, (long long)seg_stride, n_samples, (long long)clip_samples);
  SF_CHECK_ARG(clip_samples < ((int64_t)1 << 31) && n_clips >= 0 && n_clips * n_seg < 65536, "sf_stage1_audio_augment: clip too long or more than 65535 segments");
  if (n_clips == 0) return 0;
  const unsigned N = (unsigned)(n_clips * n_seg);
  hipLaunchKernelGGL(s1_audio_gather_kernel, dim3((unsigned)min((n_samples + 255) / 256, 64), N), dim3(256), 0, (hipStream_t)stream, wave, clip_table, clip_ld,
                     seg_table, seg_ld, out, n_seg, clip_samples, seg_stride, n_samples, noise_amp);
  SF_LAUNCH_CHECK();
  hipLaunchKernelGGL(s1_audio_lowpass_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, seg_table, seg_ld, out, n_samples, b0, b1, b2, a1, a2, noise_amp);
  SF_LAUNCH_CHECK();
  return 0;
}
