// Track read-out of a recording's per-window logits: per-window argmax / confidence and a Viterbi path under a cost on class changes.
// The logits of W overlapping windows (engine.sync_windows) are W noisy votes on an offset that changes slowly; the per-window argmax flickers
// between neighbouring classes, the path that maximises
//     sum_w e[w, c_w] - lam * sum_{w >= 1} |c_w - c_{w-1}|,        e[w, c] = logits[w, c] - max_c logits[w, .]
// does not.  e is log-softmax up to a row constant (a row constant cannot change the path), and for dyadic logits / lam every operation below is exact in fp32.
// Three launches on the caller's stream, all latency-bound (W x C <= W x 64 floats):
//   1. track_rows_kernel<false>: one thread per window: argmax (lowest index on ties), softmax probability of that class (fp32 statistics);
//   2. track_viterbi_kernel:     ONE wavefront, lane c = class c, the previous step's scores in LDS: the forward scan over W, then the backtrace;
//   3. track_rows_kernel<true>:  one thread per window: softmax probability of the path's class.
// Reference read-out this stands next to: decode_single_video_prediction (example.py:38-56: softmax + top-k of ONE window) on the class grid of
// make_class_grid (dataset/transforms.py:221-239); the reference has no recording-level read-out.
//
// sf_track_posterior (below the Viterbi launcher) reads the same chain out as marginals: the path above is the mode of
//     p(c_0 .. c_{W-1})  ~  exp(sum_w e[w, c_w] - lam * sum_w |c_w - c_{w-1}|),        e = the true log-softmax,
// and the forward-backward algorithm gives post[w, c] = p(c_w = c) and log_z = log of the sum over all paths.  Two launches:
//   1. track_fb_scan_kernel:     TWO workgroups of one wavefront each, side by side: block 0 the forward scan (a, and log_z), block 1 the backward scan (b);
//   2. track_fb_combine_kernel:  one thread per window: post = softmax_c (a + b), its argmax and value, the posterior mean of the grid.
#include "sf_common.h"
#include "../../include/synchformer_hip.h"
#include <cmath>

#define TRACK_MAX_C 64

// Per-window row statistics.  PATH = false: cls[w] = argmax (first maximum wins), conf[w] = its softmax probability = 1 / sum_c exp(l_c - max).
// PATH = true: cls[w] is given (the Viterbi path), conf[w] = exp(l_cls - max) / sum.  A NaN never wins a `>` comparison, so the argmax of a row of NaNs is 0.
template <bool PATH>
__global__ __launch_bounds__(256) void track_rows_kernel(const float* __restrict__ logits, int64_t ldl, int W, int C, int32_t* __restrict__ cls,
                                                          float* __restrict__ conf) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  const float* row = logits + (int64_t)w * ldl;
  int best = 0;
  float m = row[0];
  for (int c = 1; c < C; ++c) {
    const float l = row[c];
    if (l > m) { m = l; best = c; }
  }
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf(row[c] - m);
  if (PATH) {
    int c = cls[w];
    c = c < 0 ? 0 : (c >= C ? C - 1 : c);
    conf[w] = expf(row[c] - m) / sum;
  } else {
    cls[w] = best;
    conf[w] = 1.0f / sum;
  }
}

// One wavefront.  Lane c < C owns class c; lanes >= C run along with -inf scores so that every cross-lane operation sees a full EXEC mask.
//   s_0 = e[0];   s_w[c] = max_p (s_{w-1}[p] - lam * |p - c|) + e[w, c]   (lowest p on ties -> backptr[w, c]);   s_w -= max_c s_w[c]   (bounds the scores for any W)
// The end state is argmax s_{W-1} (lowest index on ties); the backtrace follows backptr from there.  Non-finite logits give NaN scores: a NaN never wins `>`, so the
// predecessor stays 0, and the backtrace clamps what it reads: every backptr entry and every class written lies in [0, C).
__global__ __launch_bounds__(64) void track_viterbi_kernel(const float* __restrict__ logits, int64_t ldl, int W, int C, float lam, int32_t* __restrict__ cls_path,
                                                            uint8_t* __restrict__ backptr) {
  __shared__ float s_prev[TRACK_MAX_C];
  const int c = threadIdx.x;
  const bool live = c < C;
  const float ninf = -INFINITY;
  float l = live ? logits[c] : ninf;
  float s = l - wave_max(l);                                 // s_0 = e[0]; -inf - finite = -inf in the idle lanes (NaN there when the row maximum is +-inf: never read)
  s_prev[c] = s;
  __syncthreads();
  float l_next = (live && W > 1) ? logits[ldl + c] : ninf;
  for (int w = 1; w < W; ++w) {
    l = l_next;
    if (w + 1 < W) l_next = live ? logits[(int64_t)(w + 1) * ldl + c] : ninf;      // the next row's load travels under this step's scan
    const float e = l - wave_max(l);
    float best = s_prev[0] - lam * (float)c;
    int bp = 0;
    for (int p = 1; p < C; ++p) {
      const float cand = s_prev[p] - lam * fabsf((float)(p - c));
      if (cand > best) { best = cand; bp = p; }
    }
    s = live ? best + e : ninf;
    s -= wave_max(s);
    if (live) backptr[(int64_t)w * C + c] = (uint8_t)bp;
    __syncthreads();                                               // every lane has read s_prev
    s_prev[c] = s;
    __syncthreads();
  }
  // (the barriers above order this wave's backptr stores before its loads below)
  int cur = 0;
  {
    float m = s_prev[0];
    for (int p = 1; p < C; ++p) if (s_prev[p] > m) { m = s_prev[p]; cur = p; }
  }
  // backtrace: lane c loads backptr[w, c] of eight rows at a time (independent of the chain), the chain itself is eight wave-uniform shuffles
  for (int w0 = W - 1; w0 >= 1; w0 -= 8) {
    int b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = (live && w0 - j >= 1) ? (int)backptr[(int64_t)(w0 - j) * C + c] : 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (w0 - j >= 1) {                                           // wave-uniform
        if (c == 0) cls_path[w0 - j] = cur;
        const int p = __shfl(b[j], cur, 64);
        cur = p < C ? p : C - 1;
      }
    }
  }
  if (c == 0) cls_path[0] = cur;
}

extern "C" int sf_track_decode(const float* logits, int64_t ldl, int W, int C, float lam, int32_t* cls_raw, float* conf_raw, int32_t* cls_path, float* conf_path,
                               uint8_t* backptr, void* stream) {
  SF_CHECK_ARG(W >= 0, "sf_track_decode: W = %d windows", W);
  SF_CHECK_ARG(C >= 2 && C <= TRACK_MAX_C, "sf_track_decode: C = %d classes out of range (2 .. %d: one lane per class)", C, TRACK_MAX_C);
  SF_CHECK_ARG(ldl >= C, "sf_track_decode: row stride ldl = %lld below C = %d", (long long)ldl, C);
  SF_CHECK_ARG(std::isfinite(lam) && lam >= 0.f, "sf_track_decode: lam must be finite and >= 0 (the cost of a class change)");
  if (W == 0) return 0;
  SF_CHECK_ARG(logits && cls_raw && conf_raw && cls_path && conf_path && backptr, "sf_track_decode: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((W + 255) / 256));
  hipLaunchKernelGGL(track_rows_kernel<false>, grid, dim3(256), 0, s, logits, ldl, W, C, cls_raw, conf_raw);
  SF_LAUNCH_CHECK();
  hipLaunchKernelGGL(track_viterbi_kernel, dim3(1), dim3(64), 0, s, logits, ldl, W, C, lam, cls_path, backptr);
  SF_LAUNCH_CHECK();
  hipLaunchKernelGGL(track_rows_kernel<true>, grid, dim3(256), 0, s, logits, ldl, W, C, cls_path, conf_path);
  SF_LAUNCH_CHECK();
  return 0;
}

// ---- forward-backward (posterior) read-out --------------------------------------------------------------------------------------------------------------
// Log domain throughout (a scaled linear-domain recursion underflows: exp(-lam * 20 steps) is 0 in fp32 at lam = 8).  -inf is a masked class: every
// subtraction that could meet (-inf) - (-inf) is guarded (fb_finite_or_zero on the subtrahend), so a row with one finite logit produces no NaN.

__device__ __forceinline__ float fb_finite_or_zero(float m) { return (m > -INFINITY && m < INFINITY) ? m : 0.f; }      // false for NaN too

// lse_p (u[p] - lam * |p - c|) over the C4 = C rounded up to 4 entries of u (LDS; entries >= C hold -inf and add exp(-inf) = +0: the sum is the sum over
// p < C in ascending p, bit for bit).  A max pass, then a sum-of-exp pass.  All lanes read the same address: the LDS broadcasts.
__device__ __forceinline__ float fb_transition_lse(const float* u, int C4, int c, float lam) {
  float mx = -INFINITY;
  for (int p = 0; p < C4; p += 4) {
    const float4 v = *reinterpret_cast<const float4*>(u + p);
    mx = fmaxf(mx, v.x - lam * fabsf((float)(p - c)));
    mx = fmaxf(mx, v.y - lam * fabsf((float)(p + 1 - c)));
    mx = fmaxf(mx, v.z - lam * fabsf((float)(p + 2 - c)));
    mx = fmaxf(mx, v.w - lam * fabsf((float)(p + 3 - c)));
  }
  const float sub = fb_finite_or_zero(mx);
  float sum = 0.f;
  for (int p = 0; p < C4; p += 4) {
    const float4 v = *reinterpret_cast<const float4*>(u + p);
    sum += expf(v.x - lam * fabsf((float)(p - c)) - sub);
    sum += expf(v.y - lam * fabsf((float)(p + 1 - c)) - sub);
    sum += expf(v.z - lam * fabsf((float)(p + 2 - c)) - sub);
    sum += expf(v.w - lam * fabsf((float)(p + 3 - c)) - sub);
  }
  return sub + logf(sum);                                          // every predecessor masked: 0 + log 0 = -inf
}

// e = l - lse_c l over the wave (idle lanes carry -inf and stay -inf).
__device__ __forceinline__ float fb_log_softmax(float l) {
  const float m = fb_finite_or_zero(wave_max(l));
  return l - (m + logf(wave_sum(expf(l - m))));
}

// Block 0, the forward scan over rows 0 .. W-1:   a_0 = e[0];        a_w[c] = e[w, c] + lse_p (a_{w-1}[p] - lam |p - c|);
// block 1, the backward scan over rows W-1 .. 0:  b_{W-1} = 0;       b_w[c] = lse_n (b_{w+1}[n] + e[w+1, n] - lam |n - c|).
// One wavefront each, lane c = class c, the vector the transition reads (a_{w-1}, or b_{w+1} + e[w+1]) in LDS, the next row's load under the current step.
// After every step the vector's maximum is subtracted (scores stay within [-(lam (C - 1) + row range), 0] for any W: a per-row constant cancels in post)
// and, in the forward block, added to a double: log_z = the subtracted maxima + lse_c of the last, normalised a.  ws = a (W, C) then b (W, C), fp32.
__global__ __launch_bounds__(64) void track_fb_scan_kernel(const float* __restrict__ logits, int64_t ldl, int W, int C, float lam, float* __restrict__ ws,
                                                            float* __restrict__ log_z) {
  __shared__ __attribute__((aligned(16))) float s_u[TRACK_MAX_C];
  const int c = threadIdx.x;
  const bool live = c < C;
  const bool back = blockIdx.x == 1;                              // wave-uniform
  const int C4 = (C + 3) & ~3;
  const float ninf = -INFINITY;
  float* out = ws + (back ? (int64_t)W * C : 0);
  const int64_t row0 = back ? W - 1 : 0, step = back ? -1 : 1;     // scan position k reads row row0 + step * k
  double shifted = 0.0;

  float e = fb_log_softmax(live ? logits[row0 * ldl + c] : ninf);
  float v = back ? (live ? 0.f : ninf) : e;
  float m = fb_finite_or_zero(wave_max(v));
  v -= m;
  shifted += (double)m;
  if (live) out[row0 * C + c] = v;
  s_u[c] = back ? v + e : v;
  __syncthreads();
  float l_next = (live && W > 1) ? logits[(row0 + step) * ldl + c] : ninf;
  for (int k = 1; k < W; ++k) {
    const int64_t row = row0 + step * k;
    const float l = l_next;
    if (k + 1 < W) l_next = live ? logits[(row + step) * ldl + c] : ninf;
    e = fb_log_softmax(l);
    const float r = fb_transition_lse(s_u, C4, c, lam);
    v = live ? (back ? r : r + e) : ninf;
    m = fb_finite_or_zero(wave_max(v));
    v -= m;
    shifted += (double)m;
    if (live) out[row * C + c] = v;
    __syncthreads();                                               // every lane has read s_u
    s_u[c] = back ? v + e : v;
    __syncthreads();
  }
  if (!back) {
    const float z = logf(wave_sum(expf(v)));                       // the normalised a_{W-1}: maximum 0 (idle and masked lanes add exp(-inf) = 0)
    if (c == 0) log_z[0] = (float)(shifted + (double)z);
  }
}

// One thread per window:  s = a_w + b_w;  post[w, c] = exp(s[c] - lse_c s);  cls_post = argmax_c post (first maximum wins; a NaN never wins `>`), conf_post its
// value;  offset_mean = sum_c post[w, c] grid[c] in ascending c.
__global__ __launch_bounds__(256) void track_fb_combine_kernel(const float* __restrict__ ws, int W, int C, const float* __restrict__ grid, float* __restrict__ post,
                                                               int64_t ldp, int32_t* __restrict__ cls_post, float* __restrict__ conf_post,
                                                               float* __restrict__ offset_mean) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  const float* a = ws + (int64_t)w * C;
  const float* b = a + (int64_t)W * C;
  float m = -INFINITY;
  for (int c = 0; c < C; ++c) m = fmaxf(m, a[c] + b[c]);
  m = fb_finite_or_zero(m);
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf(a[c] + b[c] - m);
  const float lse = fb_finite_or_zero(m + logf(sum));
  float* prow = post + (int64_t)w * ldp;
  int best = 0;
  float pbest = 0.f, mean = 0.f;
  for (int c = 0; c < C; ++c) {
    const float p = expf(a[c] + b[c] - lse);
    prow[c] = p;
    mean += p * grid[c];
    if (c == 0 || p > pbest) { pbest = p; best = c; }
  }
  cls_post[w] = best;
  conf_post[w] = pbest;
  offset_mean[w] = mean;
}

extern "C" int sf_track_posterior(const float* logits, int64_t ldl, int W, int C, float lam, const float* grid, float* post, int64_t ldp, int32_t* cls_post,
                                  float* conf_post, float* offset_mean, float* log_z, float* workspace, void* stream) {
  SF_CHECK_ARG(W >= 0, "sf_track_posterior: W = %d windows", W);
  SF_CHECK_ARG(C >= 2 && C <= TRACK_MAX_C, "sf_track_posterior: C = %d classes out of range (2 .. %d: one lane per class)", C, TRACK_MAX_C);
  SF_CHECK_ARG(ldl >= C, "sf_track_posterior: row stride ldl = %lld below C = %d", (long long)ldl, C);
  SF_CHECK_ARG(ldp >= C, "sf_track_posterior: post row stride ldp = %lld below C = %d", (long long)ldp, C);
  SF_CHECK_ARG(std::isfinite(lam) && lam >= 0.f, "sf_track_posterior: lam must be finite and >= 0 (the cost of a class change)");
  if (W == 0) return 0;
  SF_CHECK_ARG(logits && grid && post && cls_post && conf_post && offset_mean && log_z && workspace, "sf_track_posterior: null pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(track_fb_scan_kernel, dim3(2), dim3(64), 0, s, logits, ldl, W, C, lam, workspace, log_z);
  SF_LAUNCH_CHECK();
  hipLaunchKernelGGL(track_fb_combine_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, s, (const float*)workspace, W, C, grid, post, ldp, cls_post,
                     conf_post, offset_mean);
  SF_LAUNCH_CHECK();
  return 0;
}
