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
