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
//
// sf_track_stream_push (further below) reads a stream of rows out at a fixed lag with carried state; sf_track_pool_push (at the end) does that for many streams
// in one call: the same launches over a descriptor table, blockIdx.y = the stream, every block running the single-stream device functions on its stream's context.
// sf_track_decode_gated / sf_track_posterior_gated (after the pool) are the two offline read-outs of one chain over (offset class, synchronizable flag), fed by a
// second head; sf_track_stream_push_gated / sf_track_pool_push_gated (last) read that chain out of a stream at a fixed lag, from a carried state 2C wide: the stream's
// four kinds of launch around the gated kernels' own step functions.
#include "sf_common.h"
#include "../../include/synchformer_hip.h"
#include <algorithm>
#include <cmath>

#define TRACK_MAX_C 64

// Per-window row statistics.  PATH = false: cls[w] = argmax (first maximum wins), conf[w] = its softmax probability = 1 / sum_c exp(l_c - max).
// PATH = true: cls[w] is given (the Viterbi path), conf[w] = exp(l_cls - max) / sum.  A NaN never wins a `>` comparison, so the argmax of a row of NaNs is 0.
// The statistics of one row, by one thread: the argmax (first maximum wins), the maximum and sum_c exp(l_c - max), in ascending c.
__device__ __forceinline__ void track_row_stats(const float* __restrict__ row, int C, int& best, float& m, float& sum) {
  best = 0;
  m = row[0];
  for (int c = 1; c < C; ++c) {
    const float l = row[c];
    if (l > m) { m = l; best = c; }
  }
  sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf(row[c] - m);
}
// The softmax probability of class `c` (clamped into [0, C)) given the row's statistics.
__device__ __forceinline__ float track_row_conf(const float* __restrict__ row, int C, int c, float m, float sum) {
  c = c < 0 ? 0 : (c >= C ? C - 1 : c);
  return expf(row[c] - m) / sum;
}

template <bool PATH>
__global__ __launch_bounds__(256) void track_rows_kernel(const float* __restrict__ logits, int64_t ldl, int W, int C, int32_t* __restrict__ cls,
                                                          float* __restrict__ conf) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  const float* row = logits + (int64_t)w * ldl;
  int best;
  float m, sum;
  track_row_stats(row, C, best, m, sum);
  if (PATH) {
    conf[w] = track_row_conf(row, C, cls[w], m, sum);
  } else {
    cls[w] = best;
    conf[w] = 1.0f / sum;
  }
}

// One step of the Viterbi scan, by the whole wavefront: l = this row's logit of class c (-inf in the idle lanes), s_prev = the previous scores (LDS) ->
// the new, renormalised score of class c; bp = the predecessor (lowest p on ties).
__device__ __forceinline__ float track_viterbi_step(const float* s_prev, int C, int c, bool live, float lam, float l, int& bp) {
  const float e = l - wave_max(l);
  float best = s_prev[0] - lam * (float)c;
  bp = 0;
  for (int p = 1; p < C; ++p) {
    const float cand = s_prev[p] - lam * fabsf((float)(p - c));
    if (cand > best) { best = cand; bp = p; }
  }
  float s = live ? best + e : -INFINITY;
  s -= wave_max(s);
  return s;
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
    int bp;
    s = track_viterbi_step(s_prev, C, c, live, lam, l, bp);
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

// One step of either scan, by the whole wavefront: u (LDS) = the vector the transition reads, e = this row's log-softmax (joins the lse in the forward scan only)
// -> the new vector's entry of class c with the vector's maximum m (0 when that is not finite) subtracted.
__device__ __forceinline__ float fb_scan_step(const float* u, int C4, int c, bool live, bool back, float lam, float e, float& m) {
  const float r = fb_transition_lse(u, C4, c, lam);
  float v = live ? (back ? r : r + e) : -INFINITY;
  m = fb_finite_or_zero(wave_max(v));
  return v - m;
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
    v = fb_scan_step(s_u, C4, c, live, back, lam, e, m);
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

// One window, by one thread: prow[c] = exp(a[c] + b[c] - lse_c (a + b)); best = its argmax (first maximum wins), pbest its value; mean = sum_c prow[c] grid[c].
__device__ __forceinline__ void fb_combine_row(const float* a, const float* b, int C, const float* __restrict__ grid, float* __restrict__ prow, int& best,
                                               float& pbest, float& mean) {
  float m = -INFINITY;
  for (int c = 0; c < C; ++c) m = fmaxf(m, a[c] + b[c]);
  m = fb_finite_or_zero(m);
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf(a[c] + b[c] - m);
  const float lse = fb_finite_or_zero(m + logf(sum));
  best = 0;
  pbest = 0.f;
  mean = 0.f;
  for (int c = 0; c < C; ++c) {
    const float p = expf(a[c] + b[c] - lse);
    prow[c] = p;
    mean += p * grid[c];
    if (c == 0 || p > pbest) { pbest = p; best = c; }
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
  int best;
  float pbest, mean;
  fb_combine_row(a, a + (int64_t)W * C, C, grid, post + (int64_t)w * ldp, best, pbest, mean);
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

// ---- fixed-lag read-out of a stream (sf_track_stream_push) -------------------------------------------------------------------------------------------------
// Rows arrive in pushes; window w is committed by the push that delivers row w + lag, as path_{w+lag}[w] / post_{w+lag}[w] (the offline read-outs of the prefix
// 0 .. w + lag), and never revised.  Both scans are causal, so what a push needs of the past is the scan vectors after the last row (s; with the posterior a and
// the double of subtracted maxima) and, of the last `lag` rows, the back pointers, the logits (conf_lag, and the backward recursion's log-softmax, which is
// recomputed from them as the offline scan does) and - posterior - the normalised a.  The state buffer holds exactly that, the per-row parts as rings (row r in
// slot r % lag); its size does not depend on how many rows have passed.  A push of n rows is three or four launches on the caller's stream:
//   1. track_rows_kernel<false>:     cls_raw / conf_raw of the new rows (the offline kernel);
//   2. track_stream_scan_kernel:     one wavefront per scan, side by side (block 0 Viterbi, block 1 forward): loads the carried vector, runs the n rows with the next
//                                    row's load under the current step, writes back pointers / a and every row's end state (argmax s_r) into the push's workspace,
//                                    stores the carried vectors;
//   3. track_stream_readout_kernel:  one wavefront per window that becomes committed: its own backtrace from the end state of row w + lag (eight rows of back
//                                    pointers per round, wave-uniform shuffles), with the posterior its own backward recursion over rows w + lag .. w + 1 and the
//                                    combine of row w; one more wavefront backtraces the tail from the last row.  The windows are independent: a catch-up push of
//                                    1000 rows spreads over the chip instead of running n * lag dependent steps in one wavefront;
//   4. track_stream_keep_kernel:     copies the last min(lag, n) new rows into the rings (after 3, which still reads the slots they replace).
// Rows before the push live in the rings, rows of the push in the caller's logits and the workspace: TrackStreamRows resolves a row index to either.
struct TrackStreamRows {
  const float* lg_new;  int64_t ldl;      // the push's logits
  const uint8_t* bp_new;                  // workspace: back pointers (n, C)
  const float* a_new;                     // workspace: normalised a (n, C); posterior only
  const int32_t* end_new;                 // workspace: argmax s_r per new row
  const float* lg_ring;  const uint8_t* bp_ring;  const float* a_ring;      // state: (lag, C) each
  const int32_t* end_last;                // state: argmax s of the last row pushed
  int64_t t_old;                          // rows before this push
  int lag, C;
  __device__ __forceinline__ const float* logits(int64_t r) const { return r >= t_old ? lg_new + (r - t_old) * ldl : lg_ring + (r % lag) * C; }
  __device__ __forceinline__ const uint8_t* backptr(int64_t r) const { return r >= t_old ? bp_new + (r - t_old) * C : bp_ring + (r % lag) * C; }
  __device__ __forceinline__ const float* a(int64_t r) const { return r >= t_old ? a_new + (r - t_old) * C : a_ring + (r % lag) * C; }
  __device__ __forceinline__ int end(int64_t r) const { return r >= t_old ? end_new[r - t_old] : end_last[0]; }
  __device__ __forceinline__ int width() const { return C; }
};

// the state buffer: [double shifted][int32 end_last, pad][s: 64 floats][posterior: a: 64 floats][logits ring][posterior: a ring][back pointer ring]
struct TrackStreamLayout {
  int64_t s, a, lg_ring, a_ring, bp_ring, total;
  __host__ __device__ TrackStreamLayout(int C, int lag, bool posterior) {
    s = 16;
    a = s + TRACK_MAX_C * 4;
    lg_ring = a + (posterior ? TRACK_MAX_C * 4 : 0);
    a_ring = lg_ring + (int64_t)lag * C * 4;
    bp_ring = a_ring + (posterior ? (int64_t)lag * C * 4 : 0);
    total = (bp_ring + (int64_t)lag * C + 15) & ~(int64_t)15;
  }
};

// The end state of a row: the lowest class whose renormalised score is the maximum, 0.  (No such lane - NaN scores - gives class 0, as a NaN never wins `>`.)
__device__ __forceinline__ int track_wave_end_state(float s, bool live) {
  const unsigned long long hit = __ballot(live && s == 0.f);
  return hit ? __ffsll((long long)hit) - 1 : 0;
}

// The scan of one stream's push, by one wavefront: fwd = false the Viterbi scan, fwd = true the forward scan (wave-uniform).  s_u: TRACK_MAX_C floats of LDS, 16-byte
// aligned.  The single-stream kernel and the pool's kernel (sf_track_pool_push) both run this body: one stream's arithmetic is the same in either.
__device__ __forceinline__ void track_stream_scan_body(const float* __restrict__ logits, int64_t ldl, int n, int C, float lam, int64_t t_old,
                                                       unsigned char* __restrict__ state, int lag, int posterior, uint8_t* __restrict__ bp_new,
                                                       float* __restrict__ a_new, int32_t* __restrict__ end_new, float* __restrict__ log_z, bool fwd, float* s_u) {
  const TrackStreamLayout lay(C, lag, posterior != 0);
  const int c = threadIdx.x;
  const bool live = c < C;
  const int C4 = (C + 3) & ~3;
  const float ninf = -INFINITY;
  float* carried = reinterpret_cast<float*>(state + (fwd ? lay.a : lay.s));
  double* st_shifted = reinterpret_cast<double*>(state);
  int32_t* st_end = reinterpret_cast<int32_t*>(state + 8);
  double shifted = (fwd && t_old > 0) ? st_shifted[0] : 0.0;
  float v = (t_old > 0 && live) ? carried[c] : ninf;
  int k = 0;
  float l_next = (live && n > 0) ? logits[c] : ninf;
  if (t_old == 0 && n > 0) {                                       // the first row of the stream: s_0 = e[0] / a_0 = e[0], as the offline scans begin
    const float l = l_next;
    if (n > 1) l_next = live ? logits[ldl + c] : ninf;
    if (fwd) {
      v = fb_log_softmax(l);
      const float m = fb_finite_or_zero(wave_max(v));
      v -= m;
      shifted += (double)m;
      if (live) a_new[c] = v;
    } else {
      v = l - wave_max(l);
      if (live) bp_new[c] = 0;                                     // never followed: the backtrace stops at row 1
      const int end = track_wave_end_state(v, live);               // (the ballot needs the whole wavefront)
      if (c == 0) end_new[0] = end;
    }
    k = 1;
  }
  s_u[c] = v;
  __syncthreads();
  for (; k < n; ++k) {
    const float l = l_next;
    if (k + 1 < n) l_next = live ? logits[(int64_t)(k + 1) * ldl + c] : ninf;       // the next row's load travels under this step
    if (fwd) {
      float m;
      v = fb_scan_step(s_u, C4, c, live, false, lam, fb_log_softmax(l), m);
      shifted += (double)m;
      if (live) a_new[(int64_t)k * C + c] = v;
    } else {
      int bp;
      v = track_viterbi_step(s_u, C, c, live, lam, l, bp);
      if (live) bp_new[(int64_t)k * C + c] = (uint8_t)bp;
      const int end = track_wave_end_state(v, live);
      if (c == 0) end_new[k] = end;
    }
    __syncthreads();                                               // every lane has read s_u
    s_u[c] = v;
    __syncthreads();
  }
  if (n > 0) {
    const int end = track_wave_end_state(v, live);
    if (live) carried[c] = v;
    if (c == 0) {
      if (fwd) st_shifted[0] = shifted;
      else st_end[0] = end;
    }
  }
  if (fwd) {
    const float z = logf(wave_sum(expf(v)));                       // the normalised a of the last row: maximum 0
    if (c == 0) log_z[0] = (float)(shifted + (double)z);
  }
}

__global__ __launch_bounds__(64) void track_stream_scan_kernel(const float* __restrict__ logits, int64_t ldl, int n, int C, float lam, int64_t t_old,
                                                                unsigned char* __restrict__ state, int lag, int posterior, uint8_t* __restrict__ bp_new,
                                                                float* __restrict__ a_new, int32_t* __restrict__ end_new, float* __restrict__ log_z) {
  __shared__ __attribute__((aligned(16))) float s_u[TRACK_MAX_C];
  track_stream_scan_body(logits, ldl, n, C, lam, t_old, state, lag, posterior, bp_new, a_new, end_new, log_z, blockIdx.x == 1, s_u);      // block 1: the forward scan
}

// Follows the back pointers of rows R .. w + 1 from class `cur` (the class at row R) -> the class at row w.  Lane c loads backptr[r, c] of eight rows at a time, the
// chain itself is eight wave-uniform shuffles.  KEEP: tail[r - w] = the class at row r, for every r in [w, R] (LDS, written by lane 0).
template <bool KEEP, class Rows>
__device__ __forceinline__ int track_stream_backtrace(const Rows& rows, int64_t R, int64_t w, int cur, int c, bool live, int* tail) {
  const int C = rows.width();                                      // entries of one row of back pointers (the gated chain: 2C states)
  for (int64_t r0 = R; r0 > w; r0 -= 8) {
    int b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = (live && r0 - j > w) ? (int)rows.backptr(r0 - j)[c] : 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (r0 - j > w) {                                            // wave-uniform
        if (KEEP && c == 0) tail[r0 - j - w] = cur;
        const int p = __shfl(b[j], cur, 64);
        cur = p < C ? p : C - 1;
      }
    }
  }
  if (KEEP && c == 0) tail[0] = cur;
  return cur;
}

// Block i < n_commit: window w = w0 + i, read from the prefix that ends at row R = min(w + lag, t_last).  Block n_commit (if n_tail > 0): the tail, the path of the
// whole prefix on the last n_tail rows.
// bx = the block's index among the stream's n_commit + (n_tail > 0) blocks; s_u (16-byte aligned) / s_b: TRACK_MAX_C floats of LDS each, s_tail: 256 ints.
template <bool POST>
__device__ __forceinline__ void track_stream_readout_body(const TrackStreamRows& rows, float lam, const float* __restrict__ grid, int64_t w0, int n_commit, int n_tail,
                                                          int64_t t_last, int32_t* __restrict__ cls_lag, float* __restrict__ conf_lag,
                                                          float* __restrict__ post_lag, int64_t ldp, int32_t* __restrict__ cls_post_lag,
                                                          float* __restrict__ conf_post_lag, float* __restrict__ offset_mean_lag,
                                                          int32_t* __restrict__ cls_tail, float* __restrict__ conf_tail, int bx, float* s_u, float* s_b, int* s_tail) {
  const int c = threadIdx.x;
  const int C = rows.C;
  const bool live = c < C;
  if (bx == n_commit) {                                            // the tail
    const int64_t w = t_last - (n_tail - 1);
    int cur = rows.end(t_last);
    cur = cur < 0 ? 0 : (cur >= C ? C - 1 : cur);
    track_stream_backtrace<true>(rows, t_last, w, cur, c, live, s_tail);
    __syncthreads();
    for (int i = c; i < n_tail; i += 64) {
      const float* row = rows.logits(w + i);
      int best;
      float m, sum;
      track_row_stats(row, C, best, m, sum);
      cls_tail[i] = s_tail[i];
      conf_tail[i] = track_row_conf(row, C, s_tail[i], m, sum);
    }
    return;
  }
  const int i = bx;
  const int64_t w = w0 + i;
  const int64_t R = w + rows.lag < t_last ? w + rows.lag : t_last;
  int cur = rows.end(R);
  cur = cur < 0 ? 0 : (cur >= C ? C - 1 : cur);
  cur = track_stream_backtrace<false>(rows, R, w, cur, c, live, nullptr);
  if (c == 0) {
    const float* row = rows.logits(w);
    int best;
    float m, sum;
    track_row_stats(row, C, best, m, sum);
    cls_lag[i] = cur;
    conf_lag[i] = track_row_conf(row, C, cur, m, sum);
  }
  if (POST) {
    // the backward scan of the prefix 0 .. R, from its end down to row w:  b_R = 0;  b_r[c] = lse_n (b_{r+1}[n] + e[r+1, n] - lam |n - c|), renormalised per step
    const int C4 = (C + 3) & ~3;
    const float ninf = -INFINITY;
    float v = live ? 0.f : ninf;
    float l_next = live ? rows.logits(R)[c] : ninf;
    for (int64_t r = R; r > w; --r) {                              // b_{r-1} from b_r and row r
      const float l = l_next;
      if (r - 1 > w) l_next = live ? rows.logits(r - 1)[c] : ninf;
      const float e = fb_log_softmax(l);
      __syncthreads();                                             // every lane has read s_u
      s_u[c] = v + e;
      __syncthreads();
      float m;
      v = fb_scan_step(s_u, C4, c, live, true, lam, 0.f, m);
    }
    s_b[c] = v;
    __syncthreads();
    if (c == 0) {
      int best;
      float pbest, mean;
      fb_combine_row(rows.a(w), s_b, C, grid, post_lag + (int64_t)i * ldp, best, pbest, mean);
      cls_post_lag[i] = best;
      conf_post_lag[i] = pbest;
      offset_mean_lag[i] = mean;
    }
  }
}

template <bool POST>
__global__ __launch_bounds__(64) void track_stream_readout_kernel(TrackStreamRows rows, float lam, const float* __restrict__ grid, int64_t w0, int n_commit, int n_tail,
                                                                   int64_t t_last, int32_t* __restrict__ cls_lag, float* __restrict__ conf_lag,
                                                                   float* __restrict__ post_lag, int64_t ldp, int32_t* __restrict__ cls_post_lag,
                                                                   float* __restrict__ conf_post_lag, float* __restrict__ offset_mean_lag,
                                                                   int32_t* __restrict__ cls_tail, float* __restrict__ conf_tail) {
  __shared__ __attribute__((aligned(16))) float s_u[TRACK_MAX_C];
  __shared__ float s_b[TRACK_MAX_C];
  __shared__ int s_tail[256];
  track_stream_readout_body<POST>(rows, lam, grid, w0, n_commit, n_tail, t_last, cls_lag, conf_lag, post_lag, ldp, cls_post_lag, conf_post_lag, offset_mean_lag, cls_tail,
                                  conf_tail, (int)blockIdx.x, s_u, s_b, s_tail);
}

// Ring row j of a push: new row k = k0 + j (row t_old + k of the stream) into slot (t_old + k) % lag of the rings.
__device__ __forceinline__ void track_stream_keep_body(const float* __restrict__ logits, int64_t ldl, const uint8_t* __restrict__ bp_new, const float* __restrict__ a_new,
                                                       int k0, int64_t t_old, int C, int lag, int posterior, unsigned char* __restrict__ state, int j) {
  const TrackStreamLayout lay(C, lag, posterior != 0);
  const int c = threadIdx.x;
  if (c >= C) return;
  const int64_t k = k0 + (int64_t)j;
  const int64_t slot = ((t_old + k) % lag) * C + c;
  reinterpret_cast<float*>(state + lay.lg_ring)[slot] = logits[k * ldl + c];
  (state + lay.bp_ring)[slot] = bp_new[k * C + c];
  if (posterior) reinterpret_cast<float*>(state + lay.a_ring)[slot] = a_new[k * C + c];
}

// Block j: ring row j.
__global__ __launch_bounds__(64) void track_stream_keep_kernel(const float* __restrict__ logits, int64_t ldl, const uint8_t* __restrict__ bp_new,
                                                                const float* __restrict__ a_new, int k0, int64_t t_old, int C, int lag, int posterior,
                                                                unsigned char* __restrict__ state) {
  track_stream_keep_body(logits, ldl, bp_new, a_new, k0, t_old, C, lag, posterior, state, (int)blockIdx.x);
}

static bool track_stream_shape_ok(const char* who, int C, int lag) {
  if (C < 2 || C > TRACK_MAX_C) { sf_set_error("%s: C = %d classes out of range (2 .. %d: one lane per class)", who, C, TRACK_MAX_C); return false; }
  if (lag < 0 || lag > 255) { sf_set_error("%s: lag = %d windows out of range (0 .. 255)", who, lag); return false; }
  return true;
}

extern "C" int sf_track_stream_bytes(int C, int lag, int posterior) {
  if (!track_stream_shape_ok("sf_track_stream_bytes", C, lag)) return -1;
  return (int)TrackStreamLayout(C, lag, posterior != 0).total;     // at most 16 + 512 + 255 * 64 * 9
}

// the workspace of a push: [posterior: a (n, C) fp32][end (n) int32][back pointers (n, C) bytes]
#define TRACK_STREAM_MAX_PUSH (1 << 20)
extern "C" int sf_track_stream_workspace_bytes(int C, int n, int posterior) {
  SF_CHECK_ARG(C >= 2 && C <= TRACK_MAX_C, "sf_track_stream_workspace_bytes: C = %d classes out of range (2 .. %d)", C, TRACK_MAX_C);
  SF_CHECK_ARG(n >= 0 && n <= TRACK_STREAM_MAX_PUSH, "sf_track_stream_workspace_bytes: n = %d rows in one push (0 .. %d)", n, TRACK_STREAM_MAX_PUSH);
  return (int)(((posterior ? (int64_t)n * C * 4 : 0) + (int64_t)n * 4 + (int64_t)n * C + 15) & ~(int64_t)15);      // at most 2^20 * 324
}

extern "C" int sf_track_stream_push(void* state, int C, int lag, int posterior, int64_t rows_done, const float* logits, int64_t ldl, int n, float lam,
                                    const float* grid, int final, int32_t* cls_raw, float* conf_raw, int32_t* cls_lag, float* conf_lag, float* post_lag, int64_t ldp,
                                    int32_t* cls_post_lag, float* conf_post_lag, float* offset_mean_lag, int32_t* cls_tail, float* conf_tail, float* log_z,
                                    void* workspace, void* stream) {
  if (!track_stream_shape_ok("sf_track_stream_push", C, lag)) return -1;
  SF_CHECK_ARG(state, "sf_track_stream_push: null state");
  SF_CHECK_ARG(n >= 0 && n <= TRACK_STREAM_MAX_PUSH, "sf_track_stream_push: n = %d rows in one push (0 .. %d: split a longer catch-up)", n, TRACK_STREAM_MAX_PUSH);
  SF_CHECK_ARG(rows_done >= 0 && rows_done <= (INT64_MAX >> 1), "sf_track_stream_push: %lld rows pushed so far", (long long)rows_done);
  SF_CHECK_ARG(std::isfinite(lam) && lam >= 0.f, "sf_track_stream_push: lam must be finite and >= 0 (the cost of a class change)");
  SF_CHECK_ARG(n == 0 || ldl >= C, "sf_track_stream_push: row stride ldl = %lld below C = %d", (long long)ldl, C);
  const int64_t t_old = rows_done, t_new = rows_done + n;
  const int64_t done_old = t_old > lag ? t_old - lag : 0;                                   // windows committed before this push
  const int64_t done_new = final ? t_new : (t_new > lag ? t_new - lag : 0);
  const int64_t n_commit = done_new - done_old, n_tail = t_new - done_new;
  if (t_new == 0) return 0;
  SF_CHECK_ARG(n == 0 || (logits && cls_raw && conf_raw && workspace), "sf_track_stream_push: null pointer (new rows)");
  SF_CHECK_ARG(n_commit == 0 || (cls_lag && conf_lag), "sf_track_stream_push: null pointer (committed block)");
  SF_CHECK_ARG(n_tail == 0 || (cls_tail && conf_tail), "sf_track_stream_push: null pointer (tail)");
  if (posterior) {
    SF_CHECK_ARG(log_z, "sf_track_stream_push: null log_z");
    SF_CHECK_ARG(n_commit == 0 || (grid && post_lag && cls_post_lag && conf_post_lag && offset_mean_lag && ldp >= C),
                 "sf_track_stream_push: null pointer or post row stride ldp = %lld below C = %d (posterior block)", (long long)ldp, C);
  }
  hipStream_t s = (hipStream_t)stream;
  const TrackStreamLayout lay(C, lag, posterior != 0);
  unsigned char* st = static_cast<unsigned char*>(state);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  float* a_new = reinterpret_cast<float*>(ws);
  int32_t* end_new = reinterpret_cast<int32_t*>(ws + (posterior ? (int64_t)n * C * 4 : 0));
  uint8_t* bp_new = reinterpret_cast<uint8_t*>(end_new + n);
  if (n > 0) {
    hipLaunchKernelGGL(track_rows_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, logits, ldl, n, C, cls_raw, conf_raw);
    SF_LAUNCH_CHECK();
  }
  if (n > 0 || posterior) {                                        // (n == 0 with the posterior: log_z of the prefix so far, from the carried a)
    hipLaunchKernelGGL(track_stream_scan_kernel, dim3(posterior ? 2 : 1), dim3(64), 0, s, logits, ldl, n, C, lam, t_old, st, lag, posterior, bp_new, a_new, end_new,
                       log_z);
    SF_LAUNCH_CHECK();
  }
  if (n_commit + n_tail > 0) {
    TrackStreamRows rows;
    rows.lg_new = logits;  rows.ldl = ldl;  rows.bp_new = bp_new;  rows.a_new = a_new;  rows.end_new = end_new;
    rows.lg_ring = reinterpret_cast<const float*>(st + lay.lg_ring);  rows.bp_ring = st + lay.bp_ring;  rows.a_ring = reinterpret_cast<const float*>(st + lay.a_ring);
    rows.end_last = reinterpret_cast<const int32_t*>(st + 8);
    rows.t_old = t_old;  rows.lag = lag;  rows.C = C;
    const dim3 g((unsigned)(n_commit + (n_tail > 0 ? 1 : 0)));
    if (posterior)
      hipLaunchKernelGGL(track_stream_readout_kernel<true>, g, dim3(64), 0, s, rows, lam, grid, done_old, (int)n_commit, (int)n_tail, t_new - 1, cls_lag, conf_lag, post_lag,
                         ldp, cls_post_lag, conf_post_lag, offset_mean_lag, cls_tail, conf_tail);
    else
      hipLaunchKernelGGL(track_stream_readout_kernel<false>, g, dim3(64), 0, s, rows, lam, grid, done_old, (int)n_commit, (int)n_tail, t_new - 1, cls_lag, conf_lag, post_lag,
                         ldp, cls_post_lag, conf_post_lag, offset_mean_lag, cls_tail, conf_tail);
    SF_LAUNCH_CHECK();
  }
  const int keep = n < lag ? n : lag;
  if (keep > 0) {
    hipLaunchKernelGGL(track_stream_keep_kernel, dim3((unsigned)keep), dim3(64), 0, s, logits, ldl, (const uint8_t*)bp_new, (const float*)a_new, n - keep, t_old, C, lag,
                       posterior, st);
    SF_LAUNCH_CHECK();
  }
  return 0;
}

// ---- the same read-out for many streams in one call (sf_track_pool_push) ---------------------------------------------------------------------------------------
// n_active streams that share C, lag and posterior, named by a descriptor table of 8 int64 per stream (slot, rows_done, n, row0, final, commit0, tail0, unused): the
// states lie state_stride bytes apart in one buffer, the new rows of all streams in one logits matrix (stream e: rows [row0, row0 + n)), the committed blocks and
// the tails back to back in table order.  The same four kinds of launch as one stream's push, each over all streams: blockIdx.y = the table row, blockIdx.x = that
// stream's own work item (its scan / committed window or tail / ring row); the grid's x extent is the largest count in the table and a block beyond its stream's
// count exits at once (a stream brings 0 .. n rows and commits 0 .. k windows: the mapping is ragged, an idle block costs one table read).  Every block builds its
// stream's context from the table's DEVICE copy and runs the single-stream bodies above: one stream's bits do not depend on who shares the push.
#define TRACK_POOL_MAX_ACTIVE 4096
#define TRACK_POOL_ROW 8

// One table row and sf_track_stream_push's counts for it (host and device: the launcher sizes the grids from the same arithmetic).
struct TrackPoolEntry {
  int64_t slot, t_old, n, row0, final, commit0, tail0;
  int64_t t_new, done_old, n_commit, n_tail;
  __host__ __device__ TrackPoolEntry(const int64_t* table, int64_t e, int lag) {
    const int64_t* r = table + e * TRACK_POOL_ROW;
    slot = r[0];  t_old = r[1];  n = r[2];  row0 = r[3];  final = r[4];  commit0 = r[5];  tail0 = r[6];
    t_new = t_old + n;
    done_old = t_old > lag ? t_old - lag : 0;
    const int64_t done_new = final ? t_new : (t_new > lag ? t_new - lag : 0);
    n_commit = done_new - done_old;
    n_tail = t_new - done_new;
  }
  __host__ __device__ int64_t readout_blocks() const { return t_new == 0 ? 0 : n_commit + (n_tail > 0 ? 1 : 0); }
  __host__ __device__ int64_t keep(int lag) const { return n < lag ? n : lag; }
};

// the workspace of a pool push: sf_track_stream_push's three arrays over total_rows rows; stream e's part starts at its row0
struct TrackPoolWorkspace {
  float* a;  int32_t* end;  uint8_t* bp;
  __host__ __device__ TrackPoolWorkspace(unsigned char* ws, int C, int total_rows, bool posterior) {
    a = reinterpret_cast<float*>(ws);
    end = reinterpret_cast<int32_t*>(ws + (posterior ? (int64_t)total_rows * C * 4 : 0));
    bp = reinterpret_cast<uint8_t*>(end + total_rows);
  }
};

// grid (posterior ? 2 : 1, n_active): block (0, e) the Viterbi scan of stream e, block (1, e) its forward scan
__global__ __launch_bounds__(64) void track_pool_scan_kernel(const int64_t* __restrict__ table, unsigned char* __restrict__ states, int64_t state_stride,
                                                              const float* __restrict__ logits, int64_t ldl, int C, float lam, int lag, int posterior,
                                                              unsigned char* __restrict__ workspace, int total_rows, float* __restrict__ log_z) {
  __shared__ __attribute__((aligned(16))) float s_u[TRACK_MAX_C];
  const TrackPoolEntry e(table, blockIdx.y, lag);
  const bool fwd = blockIdx.x == 1;
  if (e.t_new == 0 || (e.n == 0 && !fwd)) return;                  // an empty stream; nothing to scan (n == 0 with the posterior: log_z from the carried a)
  const TrackPoolWorkspace ws(workspace, C, total_rows, posterior != 0);
  track_stream_scan_body(logits + e.row0 * ldl, ldl, (int)e.n, C, lam, e.t_old, states + e.slot * state_stride, lag, posterior, ws.bp + e.row0 * C, ws.a + e.row0 * C,
                         ws.end + e.row0, log_z + blockIdx.y, fwd, s_u);
}

// grid (the largest n_commit + (n_tail > 0) of the table, n_active)
template <bool POST>
__global__ __launch_bounds__(64) void track_pool_readout_kernel(const int64_t* __restrict__ table, const unsigned char* __restrict__ states, int64_t state_stride,
                                                                 const float* __restrict__ logits, int64_t ldl, int C, float lam, int lag,
                                                                 const float* __restrict__ grid, const unsigned char* __restrict__ workspace, int total_rows,
                                                                 int32_t* __restrict__ cls_lag, float* __restrict__ conf_lag, float* __restrict__ post_lag, int64_t ldp,
                                                                 int32_t* __restrict__ cls_post_lag, float* __restrict__ conf_post_lag,
                                                                 float* __restrict__ offset_mean_lag, int32_t* __restrict__ cls_tail, float* __restrict__ conf_tail) {
  __shared__ __attribute__((aligned(16))) float s_u[TRACK_MAX_C];
  __shared__ float s_b[TRACK_MAX_C];
  __shared__ int s_tail[256];
  const TrackPoolEntry e(table, blockIdx.y, lag);
  if ((int64_t)blockIdx.x >= e.readout_blocks()) return;
  const TrackStreamLayout lay(C, lag, POST);
  const TrackPoolWorkspace ws(const_cast<unsigned char*>(workspace), C, total_rows, POST);
  const unsigned char* st = states + e.slot * state_stride;
  TrackStreamRows rows;
  rows.lg_new = logits + e.row0 * ldl;  rows.ldl = ldl;  rows.bp_new = ws.bp + e.row0 * C;  rows.a_new = ws.a + e.row0 * C;  rows.end_new = ws.end + e.row0;
  rows.lg_ring = reinterpret_cast<const float*>(st + lay.lg_ring);  rows.bp_ring = st + lay.bp_ring;  rows.a_ring = reinterpret_cast<const float*>(st + lay.a_ring);
  rows.end_last = reinterpret_cast<const int32_t*>(st + 8);
  rows.t_old = e.t_old;  rows.lag = lag;  rows.C = C;
  track_stream_readout_body<POST>(rows, lam, grid, e.done_old, (int)e.n_commit, (int)e.n_tail, e.t_new - 1, cls_lag + e.commit0, conf_lag + e.commit0,
                                  post_lag + e.commit0 * ldp, ldp, cls_post_lag + e.commit0, conf_post_lag + e.commit0, offset_mean_lag + e.commit0,
                                  cls_tail + e.tail0, conf_tail + e.tail0, (int)blockIdx.x, s_u, s_b, s_tail);
}

// grid (the largest min(n, lag) of the table, n_active)
__global__ __launch_bounds__(64) void track_pool_keep_kernel(const int64_t* __restrict__ table, unsigned char* __restrict__ states, int64_t state_stride,
                                                              const float* __restrict__ logits, int64_t ldl, int C, int lag, int posterior,
                                                              const unsigned char* __restrict__ workspace, int total_rows) {
  const TrackPoolEntry e(table, blockIdx.y, lag);
  const int64_t keep = e.keep(lag);
  if ((int64_t)blockIdx.x >= keep) return;
  const TrackPoolWorkspace ws(const_cast<unsigned char*>(workspace), C, total_rows, posterior != 0);
  track_stream_keep_body(logits + e.row0 * ldl, ldl, ws.bp + e.row0 * C, ws.a + e.row0 * C, (int)(e.n - keep), e.t_old, C, lag, posterior,
                         states + e.slot * state_stride, (int)blockIdx.x);
}

// What a pool push's table adds up to; track_pool_table_check validates the HOST copy of the table (slots, row ranges, running sums) before anything is launched and
// fills this in.  Shared by sf_track_pool_push and sf_track_pool_push_gated: the table is the same.
struct TrackPoolTotals { int64_t sum_n, sum_commit, sum_tail, max_read, max_keep;  bool scan; };
static int track_pool_table_check(const char* who, const int64_t* table_host, int n_active, int n_slots, int total_rows, int lag, int posterior, TrackPoolTotals& tot) {
  struct Span { int64_t row0, n; };
  static thread_local int64_t slots[TRACK_POOL_MAX_ACTIVE];
  static thread_local Span spans[TRACK_POOL_MAX_ACTIVE];
  int64_t sum_n = 0, sum_commit = 0, sum_tail = 0, max_read = 0, max_keep = 0;
  int n_spans = 0;
  bool scan = false;
  for (int i = 0; i < n_active; ++i) {
    const int64_t* r = table_host + (int64_t)i * TRACK_POOL_ROW;
    SF_CHECK_ARG(r[0] >= 0 && r[0] < n_slots, "%s: table row %d: slot %lld outside the %d slots", who, i, (long long)r[0], n_slots);
    SF_CHECK_ARG(r[1] >= 0 && r[1] <= (INT64_MAX >> 1), "%s: table row %d: %lld rows pushed so far", who, i, (long long)r[1]);
    SF_CHECK_ARG(r[2] >= 0 && r[3] >= 0 && r[2] <= total_rows && r[3] <= total_rows - r[2],
                 "%s: table row %d: rows [%lld, %lld + %lld) outside the %d rows of the push", who, i, (long long)r[3], (long long)r[3], (long long)r[2], total_rows);
    const TrackPoolEntry e(table_host, i, lag);
    SF_CHECK_ARG(e.commit0 == sum_commit && e.tail0 == sum_tail,
                 "%s: table row %d: commit0 = %lld, tail0 = %lld, the counts of the rows before it give %lld, %lld", who, i, (long long)e.commit0,
                 (long long)e.tail0, (long long)sum_commit, (long long)sum_tail);
    slots[i] = e.slot;
    if (e.n > 0) spans[n_spans++] = Span{e.row0, e.n};
    if (e.t_new > 0) {
      sum_commit += e.n_commit;
      sum_tail += e.n_tail;
      if (e.readout_blocks() > max_read) max_read = e.readout_blocks();
      if (e.keep(lag) > max_keep) max_keep = e.keep(lag);
      scan = scan || e.n > 0 || posterior;
    }
    sum_n += e.n;
  }
  std::sort(slots, slots + n_active);
  for (int i = 1; i < n_active; ++i) SF_CHECK_ARG(slots[i] != slots[i - 1], "%s: slot %lld named twice in one push", who, (long long)slots[i]);
  std::sort(spans, spans + n_spans, [](const Span& a, const Span& b) { return a.row0 < b.row0; });
  for (int i = 1; i < n_spans; ++i)
    SF_CHECK_ARG(spans[i - 1].row0 + spans[i - 1].n <= spans[i].row0, "%s: the rows [%lld, +%lld) and [%lld, +%lld) of two streams overlap", who,
                 (long long)spans[i - 1].row0, (long long)spans[i - 1].n, (long long)spans[i].row0, (long long)spans[i].n);
  tot = TrackPoolTotals{sum_n, sum_commit, sum_tail, max_read, max_keep, scan};
  return 0;
}

extern "C" int sf_track_pool_workspace_bytes(int C, int total_rows, int posterior) {
  SF_CHECK_ARG(C >= 2 && C <= TRACK_MAX_C, "sf_track_pool_workspace_bytes: C = %d classes out of range (2 .. %d)", C, TRACK_MAX_C);
  SF_CHECK_ARG(total_rows >= 0 && total_rows <= TRACK_STREAM_MAX_PUSH, "sf_track_pool_workspace_bytes: %d rows in one push (0 .. %d)", total_rows, TRACK_STREAM_MAX_PUSH);
  return sf_track_stream_workspace_bytes(C, total_rows, posterior);
}

extern "C" int sf_track_pool_push(void* states, int64_t state_stride, int n_slots, int C, int lag, int posterior, const int64_t* table_host, const int64_t* table_dev,
                                  int n_active, const float* logits, int64_t ldl, int total_rows, float lam, const float* grid, int32_t* cls_raw, float* conf_raw,
                                  int32_t* cls_lag, float* conf_lag, float* post_lag, int64_t ldp, int32_t* cls_post_lag, float* conf_post_lag,
                                  float* offset_mean_lag, int32_t* cls_tail, float* conf_tail, float* log_z, void* workspace, void* stream) {
  if (!track_stream_shape_ok("sf_track_pool_push", C, lag)) return -1;
  SF_CHECK_ARG(std::isfinite(lam) && lam >= 0.f, "sf_track_pool_push: lam must be finite and >= 0 (the cost of a class change)");
  SF_CHECK_ARG(n_active >= 1 && n_active <= TRACK_POOL_MAX_ACTIVE, "sf_track_pool_push: n_active = %d streams in one push (1 .. %d)", n_active, TRACK_POOL_MAX_ACTIVE);
  SF_CHECK_ARG(n_slots >= 1, "sf_track_pool_push: n_slots = %d", n_slots);
  SF_CHECK_ARG(states && table_host && table_dev, "sf_track_pool_push: null pointer (states or table)");
  const TrackStreamLayout lay(C, lag, posterior != 0);
  SF_CHECK_ARG(state_stride >= lay.total && state_stride % 16 == 0, "sf_track_pool_push: state stride %lld: a multiple of 16, at least %lld bytes", (long long)state_stride,
               (long long)lay.total);
  SF_CHECK_ARG(total_rows >= 0 && total_rows <= TRACK_STREAM_MAX_PUSH, "sf_track_pool_push: total_rows = %d rows in one push (0 .. %d)", total_rows, TRACK_STREAM_MAX_PUSH);
  TrackPoolTotals tot;
  if (track_pool_table_check("sf_track_pool_push", table_host, n_active, n_slots, total_rows, lag, posterior, tot)) return -1;
  const int64_t sum_n = tot.sum_n, sum_commit = tot.sum_commit, sum_tail = tot.sum_tail, max_read = tot.max_read, max_keep = tot.max_keep;
  const bool scan = tot.scan;
  SF_CHECK_ARG(sum_n == 0 || ldl >= C, "sf_track_pool_push: row stride ldl = %lld below C = %d", (long long)ldl, C);
  SF_CHECK_ARG(sum_n == 0 || (logits && cls_raw && conf_raw && workspace), "sf_track_pool_push: null pointer (new rows)");
  SF_CHECK_ARG(sum_commit == 0 || (cls_lag && conf_lag), "sf_track_pool_push: null pointer (committed block)");
  SF_CHECK_ARG(sum_tail == 0 || (cls_tail && conf_tail), "sf_track_pool_push: null pointer (tail)");
  if (posterior) {
    SF_CHECK_ARG(!scan || log_z, "sf_track_pool_push: null log_z");
    SF_CHECK_ARG(sum_commit == 0 || (grid && post_lag && cls_post_lag && conf_post_lag && offset_mean_lag && ldp >= C),
                 "sf_track_pool_push: null pointer or post row stride ldp = %lld below C = %d (posterior block)", (long long)ldp, C);
  }
  hipStream_t s = (hipStream_t)stream;
  unsigned char* st = static_cast<unsigned char*>(states);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  if (sum_n > 0) {                                                 // one thread per row of the packed matrix (rows between two streams' ranges: their own argmax, unread)
    hipLaunchKernelGGL(track_rows_kernel<false>, dim3((unsigned)((total_rows + 255) / 256)), dim3(256), 0, s, logits, ldl, total_rows, C, cls_raw, conf_raw);
    SF_LAUNCH_CHECK();
  }
  if (scan) {
    hipLaunchKernelGGL(track_pool_scan_kernel, dim3(posterior ? 2 : 1, (unsigned)n_active), dim3(64), 0, s, table_dev, st, state_stride, logits, ldl, C, lam, lag, posterior,
                       ws, total_rows, log_z);
    SF_LAUNCH_CHECK();
  }
  if (max_read > 0) {
    const dim3 g((unsigned)max_read, (unsigned)n_active);
    if (posterior)
      hipLaunchKernelGGL(track_pool_readout_kernel<true>, g, dim3(64), 0, s, table_dev, (const unsigned char*)st, state_stride, logits, ldl, C, lam, lag, grid,
                         (const unsigned char*)ws, total_rows, cls_lag, conf_lag, post_lag, ldp, cls_post_lag, conf_post_lag, offset_mean_lag, cls_tail, conf_tail);
    else
      hipLaunchKernelGGL(track_pool_readout_kernel<false>, g, dim3(64), 0, s, table_dev, (const unsigned char*)st, state_stride, logits, ldl, C, lam, lag, grid,
                         (const unsigned char*)ws, total_rows, cls_lag, conf_lag, post_lag, ldp, cls_post_lag, conf_post_lag, offset_mean_lag, cls_tail, conf_tail);
    SF_LAUNCH_CHECK();
  }
  if (max_keep > 0) {
    hipLaunchKernelGGL(track_pool_keep_kernel, dim3((unsigned)max_keep, (unsigned)n_active), dim3(64), 0, s, table_dev, st, state_stride, logits, ldl, C, lag, posterior,
                       (const unsigned char*)ws, total_rows);
    SF_LAUNCH_CHECK();
  }
  return 0;
}

// ---- the read-outs gated by synchronizability (sf_track_decode_gated, sf_track_posterior_gated) ----------------------------------------------------
// A second, 2-way head (class 1 = synchronizable) reads the same windows; one chain over the 2C states j = m * C + c (c the offset class, m the flag) joins the two:
//     d = z[w, 1] - z[w, 0];   ls = -softplus(-d) = log sigmoid(d);   lu = -softplus(d);   softplus(x) = max(x, 0) + log1p(exp(-|x|))
//     E[w, c, 1] = ls + l[w, c] - lse_c l[w, .];     E[w, c, 0] = lu - log C          (a true log-probability: every row sums to 1 over the 2C states)
//     T((p, m') -> (c, m)) = -lam |p - c| - mu [m' != m]
// A window judged not synchronizable says nothing about the offset (plane 0 is flat) and the chain carries the class across it on the smoothness prior.
// One wavefront per scan as above, lane j = state j, lanes >= 2C idle with -inf.  A lane scans the C predecessors of its OWN plane and takes the other plane's best
// (Viterbi) / lse (forward-backward) from its partner lane (m, c) <-> (1 - m, c), which has just computed exactly that: max_p (s[p, 1-m] - lam |p - c|) - mu.
#define TRACK_GATE_MAX_C 32

__device__ __forceinline__ float gate_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// What a lane of the gated scans is: its state's plane m and class c, its partner's lane.  Idle lanes (j >= 2C) act as state 0 and are their own partner.
struct TrackGatedLane {
  int j, m, c, partner;
  bool live;
  __device__ __forceinline__ TrackGatedLane(int C) {
    j = threadIdx.x;
    live = j < 2 * C;
    m = (live && j >= C) ? 1 : 0;
    c = live ? j - m * C : 0;
    partner = live ? (m ? j - C : j + C) : j;
  }
};

// E[w, c, m] of the lane's state, by the whole wavefront: l1 = the row's offset logit of class c in the lanes of plane 1 and -inf in every other lane, z0 / z1 the
// row's gate logits (wave-uniform).  -inf in the idle lanes.
__device__ __forceinline__ float track_gated_emission(const TrackGatedLane& ln, float l1, float z0, float z1, float log_c) {
  const float d = z1 - z0;
  const float e1 = fb_log_softmax(l1);
  const float e = ln.m ? -gate_softplus(-d) + e1 : -gate_softplus(d) - log_c;
  return ln.live ? e : -INFINITY;
}

// One step of the gated Viterbi scan, by the whole wavefront: s_prev (LDS, 2C floats, state-major) = the previous, renormalised scores, e = this row's emission of
// the lane's state -> the new renormalised score; bp = the predecessor STATE (one byte).  The lane scans the C predecessors of its own plane (lowest p on ties), takes
// the other plane's best from its partner, subtracts mu, and settles the tie between the planes (m' = 0 wins).  The offline kernel and the stream's scan both call
// this: the arithmetic is shared, not copied.
__device__ __forceinline__ float track_gated_viterbi_step(const TrackGatedLane& ln, const float* s_prev, int C, float lam, float mu, float e, int& bp) {
  const float* sp = s_prev + ln.m * C;                             // the lane's own plane
  float best = sp[0] - lam * (float)ln.c;
  bp = 0;
  for (int p = 1; p < C; ++p) {
    const float cand = sp[p] - lam * fabsf((float)(p - ln.c));
    if (cand > best) { best = cand; bp = p; }
  }
  const float other = __shfl(best, ln.partner, 64) - mu;           // max_p (S[p, 1 - m] - lam |p - c|) - mu, and the p that gave it
  const int other_bp = __shfl(bp, ln.partner, 64);
  const bool cross = ln.m ? other >= best : other > best;          // ties between the planes: m' = 0 wins
  bp = cross ? (1 - ln.m) * C + other_bp : ln.m * C + bp;
  float s = ln.live ? (cross ? other : best) + e : -INFINITY;
  s -= wave_max(s);
  return s;
}

// One step of either gated forward-backward scan, by the whole wavefront: s_u (LDS, two planes of 32 floats, entries >= C hold -inf) = the vector the transition
// reads, e = this row's emission (joins the lse in the forward scan only) -> the new vector's entry of the lane's state with the vector's maximum m (0 when that is
// not finite) subtracted.  lse over the 2C predecessors = logaddexp(lse over the own plane, the partner's lse over its own plane - mu).
__device__ __forceinline__ float track_gated_fb_step(const TrackGatedLane& ln, const float* s_u, int C4, bool back, float lam, float mu, float e, float& m) {
  const float own = fb_transition_lse(s_u + ln.m * 32, C4, ln.c, lam);
  const float other = __shfl(own, ln.partner, 64) - mu;
  const float mx = fb_finite_or_zero(fmaxf(own, other));
  const float r = mx + logf(expf(own - mx) + expf(other - mx));
  const float v = ln.live ? (back ? r : r + e) : -INFINITY;
  m = fb_finite_or_zero(wave_max(v));
  return v - m;
}

// One thread per window: cls_raw / conf_raw as track_rows_kernel<false> gives them, sync_raw = sigmoid(z1 - z0).
__global__ __launch_bounds__(256) void track_gated_rows_kernel(const float* __restrict__ logits, int64_t ldl, const float* __restrict__ gate, int64_t ldg, int W, int C,
                                                                int32_t* __restrict__ cls_raw, float* __restrict__ conf_raw, float* __restrict__ sync_raw) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  int best;
  float m, sum;
  track_row_stats(logits + (int64_t)w * ldl, C, best, m, sum);
  cls_raw[w] = best;
  conf_raw[w] = 1.0f / sum;
  const float d = gate[(int64_t)w * ldg + 1] - gate[(int64_t)w * ldg];
  sync_raw[w] = 1.0f / (1.0f + expf(-d));
}

// One wavefront, lane j = state j = m * C + c.   S_0 = E[0];   S_w[j] = E[w, j] + max_j' (S_{w-1}[j'] + T(j', j)), the LOWEST predecessor state on ties -> backptr[w, j]
// (one byte);   S_w -= max_j S_w[j].  Inside a plane the lowest p wins (strict `>` in ascending p); between the planes m' = 0 wins: a lane of plane 0 takes the other
// plane's candidate only when it is strictly larger, a lane of plane 1 also when it is equal.  (The partner picks its p BEFORE mu is subtracted, a scan over all 2C
// predecessors would pick after: the two differ only where fp32 rounds two different candidates of the other plane to one value by subtracting mu - the partner then
// keeps the truly larger one.  With exact arithmetic, e.g. dyadic inputs, they are the same rule.)  The end state is the lowest state whose score is the maximum; the
// backtrace is track_viterbi_kernel's (eight rows of back pointers per load) and writes cls_path = j % C, sync_path = j / C.  NaN scores never win a comparison, and
// the backtrace clamps what it reads: every byte and every index written lies in [0, 2C) / [0, C) / {0, 1}.
__global__ __launch_bounds__(64) void track_gated_viterbi_kernel(const float* __restrict__ logits, int64_t ldl, const float* __restrict__ gate, int64_t ldg, int W, int C,
                                                                  float lam, float mu, int32_t* __restrict__ cls_path, int32_t* __restrict__ sync_path,
                                                                  uint8_t* __restrict__ backptr) {
  __shared__ float s_prev[64];
  const TrackGatedLane ln(C);
  const int S = 2 * C;
  const float ninf = -INFINITY;
  const float log_c = logf((float)C);
  const bool loads = ln.live && ln.m;                              // the lanes of plane 1 carry the offset logits
  float s = track_gated_emission(ln, loads ? logits[ln.c] : ninf, gate[0], gate[1], log_c);
  s -= wave_max(s);
  s_prev[ln.j] = s;
  __syncthreads();
  float l_next = (loads && W > 1) ? logits[ldl + ln.c] : ninf;
  float z0_next = W > 1 ? gate[ldg] : 0.f, z1_next = W > 1 ? gate[ldg + 1] : 0.f;
  for (int w = 1; w < W; ++w) {
    const float l = l_next, z0 = z0_next, z1 = z1_next;
    if (w + 1 < W) {                                               // the next row's loads travel under this step's scan
      l_next = loads ? logits[(int64_t)(w + 1) * ldl + ln.c] : ninf;
      z0_next = gate[(int64_t)(w + 1) * ldg];
      z1_next = gate[(int64_t)(w + 1) * ldg + 1];
    }
    int bp;
    s = track_gated_viterbi_step(ln, s_prev, C, lam, mu, track_gated_emission(ln, l, z0, z1, log_c), bp);
    if (ln.live) backptr[(int64_t)w * S + ln.j] = (uint8_t)bp;
    __syncthreads();                                               // every lane has read s_prev
    s_prev[ln.j] = s;
    __syncthreads();
  }
  // (the barriers above order this wave's backptr stores before its loads below)
  int cur = track_wave_end_state(s, ln.live);
  for (int w0 = W - 1; w0 >= 1; w0 -= 8) {
    int b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) b[i] = (ln.live && w0 - i >= 1) ? (int)backptr[(int64_t)(w0 - i) * S + ln.j] : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (w0 - i >= 1) {                                           // wave-uniform
        if (ln.j == 0) { cls_path[w0 - i] = cur % C;  sync_path[w0 - i] = cur / C; }
        const int p = __shfl(b[i], cur, 64);
        cur = p < S ? p : S - 1;
      }
    }
  }
  if (ln.j == 0) { cls_path[0] = cur % C;  sync_path[0] = cur / C; }
}

static bool track_gated_args_ok(const char* who, int W, int C, int64_t ldl, int64_t ldg, float lam, float mu) {
  if (W < 0) { sf_set_error("%s: W = %d windows", who, W); return false; }
  if (C < 2 || C > TRACK_GATE_MAX_C) { sf_set_error("%s: C = %d classes out of range (2 .. %d: one lane per (class, flag) state)", who, C, TRACK_GATE_MAX_C); return false; }
  if (ldl < C) { sf_set_error("%s: row stride ldl = %lld below C = %d", who, (long long)ldl, C); return false; }
  if (ldg < 2) { sf_set_error("%s: gate row stride ldg = %lld below 2", who, (long long)ldg); return false; }
  if (!(std::isfinite(lam) && lam >= 0.f)) { sf_set_error("%s: lam must be finite and >= 0 (the cost of a class change)", who); return false; }
  if (!(std::isfinite(mu) && mu >= 0.f)) { sf_set_error("%s: mu must be finite and >= 0 (the cost of a change of the synchronizable flag)", who); return false; }
  return true;
}

extern "C" int sf_track_decode_gated(const float* logits, int64_t ldl, const float* gate_logits, int64_t ldg, int W, int C, float lam, float mu, int32_t* cls_raw,
                                     float* conf_raw, float* sync_raw, int32_t* cls_path, int32_t* sync_path, float* conf_path, uint8_t* backptr, void* stream) {
  if (!track_gated_args_ok("sf_track_decode_gated", W, C, ldl, ldg, lam, mu)) return -1;
  if (W == 0) return 0;
  SF_CHECK_ARG(logits && gate_logits && cls_raw && conf_raw && sync_raw && cls_path && sync_path && conf_path && backptr, "sf_track_decode_gated: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((W + 255) / 256));
  hipLaunchKernelGGL(track_gated_rows_kernel, grid, dim3(256), 0, s, logits, ldl, gate_logits, ldg, W, C, cls_raw, conf_raw, sync_raw);
  SF_LAUNCH_CHECK();
  hipLaunchKernelGGL(track_gated_viterbi_kernel, dim3(1), dim3(64), 0, s, logits, ldl, gate_logits, ldg, W, C, lam, mu, cls_path, sync_path, backptr);
  SF_LAUNCH_CHECK();
  hipLaunchKernelGGL(track_rows_kernel<true>, grid, dim3(256), 0, s, logits, ldl, W, C, cls_path, conf_path);
  SF_LAUNCH_CHECK();
  return 0;
}

// The two scans of 3.14 over the 2C states: block 0 forward (a, and log_z), block 1 backward (b), one wavefront each.
//     a_0 = E[0];        a_w[j] = E[w, j] + lse_j' (a_{w-1}[j'] + T(j', j));        b_{W-1} = 0;        b_w[j] = lse_n (b_{w+1}[n] + E[w+1, n] + T(j, n))
// The vector the transition reads lies in LDS as two planes of 32 floats (entries >= C hold -inf, so fb_transition_lse's float4 reads stay aligned and add +0);
// lse over the 2C predecessors = logaddexp(lse over the own plane, the partner's lse over its own plane - mu).  The maximum is subtracted after every step and, in the
// forward block, summed in a double.  ws = a (W, 2C) then b (W, 2C), fp32, state-major rows j = m * C + c.
__global__ __launch_bounds__(64) void track_gated_fb_scan_kernel(const float* __restrict__ logits, int64_t ldl, const float* __restrict__ gate, int64_t ldg, int W, int C,
                                                                  float lam, float mu, float* __restrict__ ws, float* __restrict__ log_z) {
  __shared__ __attribute__((aligned(16))) float s_u[64];
  const TrackGatedLane ln(C);
  const int S = 2 * C;
  const bool back = blockIdx.x == 1;                              // wave-uniform
  const int C4 = (C + 3) & ~3;
  const float ninf = -INFINITY;
  const float log_c = logf((float)C);
  const bool loads = ln.live && ln.m;
  const int slot = ln.m * 32 + ln.c;
  float* out = ws + (back ? (int64_t)W * S : 0);
  const int64_t row0 = back ? W - 1 : 0, step = back ? -1 : 1;     // scan position k reads row row0 + step * k
  double shifted = 0.0;

  s_u[threadIdx.x] = ninf;
  __syncthreads();
  float e = track_gated_emission(ln, loads ? logits[row0 * ldl + ln.c] : ninf, gate[row0 * ldg], gate[row0 * ldg + 1], log_c);
  float v = back ? (ln.live ? 0.f : ninf) : e;
  float m = fb_finite_or_zero(wave_max(v));
  v -= m;
  shifted += (double)m;
  if (ln.live) {
    out[row0 * S + ln.j] = v;
    s_u[slot] = back ? v + e : v;
  }
  __syncthreads();
  float l_next = (loads && W > 1) ? logits[(row0 + step) * ldl + ln.c] : ninf;
  float z0_next = W > 1 ? gate[(row0 + step) * ldg] : 0.f, z1_next = W > 1 ? gate[(row0 + step) * ldg + 1] : 0.f;
  for (int k = 1; k < W; ++k) {
    const int64_t row = row0 + step * k;
    const float l = l_next, z0 = z0_next, z1 = z1_next;
    if (k + 1 < W) {
      l_next = loads ? logits[(row + step) * ldl + ln.c] : ninf;
      z0_next = gate[(row + step) * ldg];
      z1_next = gate[(row + step) * ldg + 1];
    }
    e = track_gated_emission(ln, l, z0, z1, log_c);
    v = track_gated_fb_step(ln, s_u, C4, back, lam, mu, e, m);
    shifted += (double)m;
    if (ln.live) out[row * S + ln.j] = v;
    __syncthreads();                                               // every lane has read s_u
    if (ln.live) s_u[slot] = back ? v + e : v;
    __syncthreads();
  }
  if (!back) {
    const float z = logf(wave_sum(expf(v)));                       // the normalised a_{W-1}: maximum 0 (idle lanes add exp(-inf) = 0)
    if (ln.j == 0) log_z[0] = (float)(shifted + (double)z);
  }
}

// One window, by one thread: a, b (2C floats each, state-major) -> prow[c] = post2[c, 0] + post2[c, 1] with post2 = exp(a + b - lse_j (a + b)); ps = sum_c post2[c, 1]
// clamped at 1; best = argmax_c prow (first maximum wins), pbest its value; mean = sum_c prow[c] grid[c] in ascending c.
__device__ __forceinline__ void track_gated_combine_row(const float* a, const float* b, int C, const float* __restrict__ grid, float* __restrict__ prow, int& best,
                                                        float& pbest, float& mean, float& ps) {
  const int S = 2 * C;
  float m = -INFINITY;
  for (int j = 0; j < S; ++j) m = fmaxf(m, a[j] + b[j]);
  m = fb_finite_or_zero(m);
  float sum = 0.f;
  for (int j = 0; j < S; ++j) sum += expf(a[j] + b[j] - m);
  const float lse = fb_finite_or_zero(m + logf(sum));
  best = 0;
  pbest = 0.f;
  mean = 0.f;
  ps = 0.f;
  for (int c = 0; c < C; ++c) {
    const float p1 = expf(a[C + c] + b[C + c] - lse);
    const float p = expf(a[c] + b[c] - lse) + p1;
    prow[c] = p;
    ps += p1;
    mean += p * grid[c];
    if (c == 0 || p > pbest) { pbest = p; best = c; }
  }
  ps = fminf(ps, 1.f);
}

// One thread per window:  s = a_w + b_w over the 2C states;  post2 = exp(s - lse_j s);  post[w, c] = post2[c, 0] + post2[c, 1];  p_sync[w] = sum_c post2[c, 1] (at most
// 1);  cls_post = argmax_c post (first maximum wins; a NaN never wins `>`), conf_post its value;  offset_mean = sum_c post[w, c] grid[c] in ascending c.
__global__ __launch_bounds__(256) void track_gated_fb_combine_kernel(const float* __restrict__ ws, int W, int C, const float* __restrict__ grid, float* __restrict__ post,
                                                                      int64_t ldp, float* __restrict__ p_sync, int32_t* __restrict__ cls_post,
                                                                      float* __restrict__ conf_post, float* __restrict__ offset_mean) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  const int S = 2 * C;
  const float* a = ws + (int64_t)w * S;
  int best;
  float pbest, mean, ps;
  track_gated_combine_row(a, a + (int64_t)W * S, C, grid, post + (int64_t)w * ldp, best, pbest, mean, ps);
  p_sync[w] = ps;
  cls_post[w] = best;
  conf_post[w] = pbest;
  offset_mean[w] = mean;
}

extern "C" int sf_track_posterior_gated(const float* logits, int64_t ldl, const float* gate_logits, int64_t ldg, int W, int C, float lam, float mu, const float* grid,
                                        float* post, int64_t ldp, float* p_sync, int32_t* cls_post, float* conf_post, float* offset_mean, float* log_z,
                                        float* workspace, void* stream) {
  if (!track_gated_args_ok("sf_track_posterior_gated", W, C, ldl, ldg, lam, mu)) return -1;
  SF_CHECK_ARG(ldp >= C, "sf_track_posterior_gated: post row stride ldp = %lld below C = %d", (long long)ldp, C);
  if (W == 0) return 0;
  SF_CHECK_ARG(logits && gate_logits && grid && post && p_sync && cls_post && conf_post && offset_mean && log_z && workspace, "sf_track_posterior_gated: null pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(track_gated_fb_scan_kernel, dim3(2), dim3(64), 0, s, logits, ldl, gate_logits, ldg, W, C, lam, mu, workspace, log_z);
  SF_LAUNCH_CHECK();
  hipLaunchKernelGGL(track_gated_fb_combine_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, s, (const float*)workspace, W, C, grid, post, ldp, p_sync, cls_post,
                     conf_post, offset_mean);
  SF_LAUNCH_CHECK();
  return 0;
}

// ---- the gated read-outs of a stream at a fixed lag (sf_track_stream_push_gated, sf_track_pool_push_gated) -----------------------------------------
// sf_track_stream_push's definition with the gated offline read-outs in place of the ungated ones: window w is committed by the push that delivers row w + lag as
// path_{w+lag}[w] / post_{w+lag}[w] of sf_track_decode_gated / sf_track_posterior_gated on the prefix 0 .. w + lag.  The carried state is 2C wide: the scan vectors
// over the states j = m * C + c, rings of back pointers (2C bytes a row) and of a (2C floats a row), and rings of BOTH inputs - the offset logits (C) and the gate
// logits (2) - from which the emission is recomputed exactly as the offline scans compute it (no emission ring).  The same four kinds of launch, the per-step
// arithmetic that of the offline kernels (track_gated_viterbi_step, track_gated_fb_step, track_gated_emission, track_gated_combine_row).
struct TrackGatedStreamRows {
  const float* lg_new;  int64_t ldl;      // the push's offset logits
  const float* gz_new;  int64_t ldg;      // the push's gate logits
  const uint8_t* bp_new;                  // workspace: back pointers (n, 2C)
  const float* a_new;                     // workspace: normalised a (n, 2C); posterior only
  const int32_t* end_new;                 // workspace: the end state per new row
  const float* lg_ring;  const float* gz_ring;  const uint8_t* bp_ring;  const float* a_ring;      // state: (lag, C), (lag, 2), (lag, 2C), (lag, 2C)
  const int32_t* end_last;                // state: the end state of the last row pushed
  int64_t t_old;                          // rows before this push
  int lag, C;
  __device__ __forceinline__ const float* logits(int64_t r) const { return r >= t_old ? lg_new + (r - t_old) * ldl : lg_ring + (r % lag) * C; }
  __device__ __forceinline__ const float* gate(int64_t r) const { return r >= t_old ? gz_new + (r - t_old) * ldg : gz_ring + (r % lag) * 2; }
  __device__ __forceinline__ const uint8_t* backptr(int64_t r) const { return r >= t_old ? bp_new + (r - t_old) * 2 * C : bp_ring + (r % lag) * 2 * C; }
  __device__ __forceinline__ const float* a(int64_t r) const { return r >= t_old ? a_new + (r - t_old) * 2 * C : a_ring + (r % lag) * 2 * C; }
  __device__ __forceinline__ int end(int64_t r) const { return r >= t_old ? end_new[r - t_old] : end_last[0]; }
  __device__ __forceinline__ int width() const { return 2 * C; }
};

// the gated state buffer:
//   [double shifted][int32 end_last, pad][s: 64 floats][posterior: a: 64 floats][offset logits ring (lag, C) fp32][gate logits ring (lag, 2) fp32]
//   [posterior: a ring (lag, 2C) fp32][back pointer ring (lag, 2C) bytes], rounded up to 16 bytes.  Row r of the stream lies in slot r % lag of every ring.
struct TrackGatedStreamLayout {
  int64_t s, a, lg_ring, gz_ring, a_ring, bp_ring, total;
  __host__ __device__ TrackGatedStreamLayout(int C, int lag, bool posterior) {
    s = 16;
    a = s + 64 * 4;
    lg_ring = a + (posterior ? 64 * 4 : 0);
    gz_ring = lg_ring + (int64_t)lag * C * 4;
    a_ring = gz_ring + (int64_t)lag * 2 * 4;
    bp_ring = a_ring + (posterior ? (int64_t)lag * 2 * C * 4 : 0);
    total = (bp_ring + (int64_t)lag * 2 * C + 15) & ~(int64_t)15;
  }
};

// One stream's view of its rows: the rings of its state and its part of the push (host and device: the single-stream launcher and the pool's kernels build it).
__host__ __device__ __forceinline__ void track_gated_rows_fill(TrackGatedStreamRows& rows, const TrackGatedStreamLayout& lay, const unsigned char* st, const float* logits,
                                                               int64_t ldl, const float* gate, int64_t ldg, const uint8_t* bp, const float* a, const int32_t* end,
                                                               int64_t t_old, int lag, int C) {
  rows.lg_new = logits;  rows.ldl = ldl;  rows.gz_new = gate;  rows.ldg = ldg;  rows.bp_new = bp;  rows.a_new = a;  rows.end_new = end;
  rows.lg_ring = reinterpret_cast<const float*>(st + lay.lg_ring);  rows.gz_ring = reinterpret_cast<const float*>(st + lay.gz_ring);
  rows.bp_ring = st + lay.bp_ring;  rows.a_ring = reinterpret_cast<const float*>(st + lay.a_ring);
  rows.end_last = reinterpret_cast<const int32_t*>(st + 8);
  rows.t_old = t_old;  rows.lag = lag;  rows.C = C;
}

// The scan of one stream's push, by one wavefront: fwd = false the Viterbi scan, fwd = true the forward scan (wave-uniform).  s_u: 64 floats of LDS, 16-byte aligned:
// the Viterbi scores state-major, the forward vector as two planes of 32 (entries >= C hold -inf), as the offline kernels keep them.
__device__ __forceinline__ void track_gated_stream_scan_body(const float* __restrict__ logits, int64_t ldl, const float* __restrict__ gate, int64_t ldg, int n, int C,
                                                             float lam, float mu, int64_t t_old, unsigned char* __restrict__ state, int lag, int posterior,
                                                             uint8_t* __restrict__ bp_new, float* __restrict__ a_new, int32_t* __restrict__ end_new,
                                                             float* __restrict__ log_z, bool fwd, float* s_u) {
  const TrackGatedStreamLayout lay(C, lag, posterior != 0);
  const TrackGatedLane ln(C);
  const int S = 2 * C;
  const int C4 = (C + 3) & ~3;
  const float ninf = -INFINITY;
  const float log_c = logf((float)C);
  const bool loads = ln.live && ln.m;                              // the lanes of plane 1 carry the offset logits
  const int slot = fwd ? ln.m * 32 + ln.c : ln.j;
  float* carried = reinterpret_cast<float*>(state + (fwd ? lay.a : lay.s));
  double* st_shifted = reinterpret_cast<double*>(state);
  int32_t* st_end = reinterpret_cast<int32_t*>(state + 8);
  double shifted = (fwd && t_old > 0) ? st_shifted[0] : 0.0;
  float v = (t_old > 0 && ln.live) ? carried[ln.j] : ninf;
  int k = 0;
  float l_next = (loads && n > 0) ? logits[ln.c] : ninf;
  float z0_next = n > 0 ? gate[0] : 0.f, z1_next = n > 0 ? gate[1] : 0.f;
  s_u[threadIdx.x] = ninf;
  __syncthreads();
  if (t_old == 0 && n > 0) {                                       // the first row of the stream: S_0 = E[0] / a_0 = E[0], as the offline scans begin
    const float l = l_next, z0 = z0_next, z1 = z1_next;
    if (n > 1) {
      l_next = loads ? logits[ldl + ln.c] : ninf;
      z0_next = gate[ldg];
      z1_next = gate[ldg + 1];
    }
    const float e = track_gated_emission(ln, l, z0, z1, log_c);
    if (fwd) {
      v = e;
      const float m = fb_finite_or_zero(wave_max(v));
      v -= m;
      shifted += (double)m;
      if (ln.live) a_new[ln.j] = v;
    } else {
      v = e;
      v -= wave_max(v);
      if (ln.live) bp_new[ln.j] = 0;                               // never followed: the backtrace stops at row 1
      const int end = track_wave_end_state(v, ln.live);            // (the ballot needs the whole wavefront)
      if (ln.j == 0) end_new[0] = end;
    }
    k = 1;
  }
  if (ln.live) s_u[slot] = v;
  __syncthreads();
  for (; k < n; ++k) {
    const float l = l_next, z0 = z0_next, z1 = z1_next;
    if (k + 1 < n) {                                               // the next row's loads travel under this step
      l_next = loads ? logits[(int64_t)(k + 1) * ldl + ln.c] : ninf;
      z0_next = gate[(int64_t)(k + 1) * ldg];
      z1_next = gate[(int64_t)(k + 1) * ldg + 1];
    }
    const float e = track_gated_emission(ln, l, z0, z1, log_c);
    if (fwd) {
      float m;
      v = track_gated_fb_step(ln, s_u, C4, false, lam, mu, e, m);
      shifted += (double)m;
      if (ln.live) a_new[(int64_t)k * S + ln.j] = v;
    } else {
      int bp;
      v = track_gated_viterbi_step(ln, s_u, C, lam, mu, e, bp);
      if (ln.live) bp_new[(int64_t)k * S + ln.j] = (uint8_t)bp;
      const int end = track_wave_end_state(v, ln.live);
      if (ln.j == 0) end_new[k] = end;
    }
    __syncthreads();                                               // every lane has read s_u
    if (ln.live) s_u[slot] = v;
    __syncthreads();
  }
  if (n > 0) {
    const int end = track_wave_end_state(v, ln.live);
    if (ln.live) carried[ln.j] = v;
    if (ln.j == 0) {
      if (fwd) st_shifted[0] = shifted;
      else st_end[0] = end;
    }
  }
  if (fwd) {
    const float z = logf(wave_sum(expf(v)));                       // the normalised a of the last row: maximum 0
    if (ln.j == 0) log_z[0] = (float)(shifted + (double)z);
  }
}

__global__ __launch_bounds__(64) void track_gated_stream_scan_kernel(const float* __restrict__ logits, int64_t ldl, const float* __restrict__ gate, int64_t ldg, int n,
                                                                      int C, float lam, float mu, int64_t t_old, unsigned char* __restrict__ state, int lag,
                                                                      int posterior, uint8_t* __restrict__ bp_new, float* __restrict__ a_new,
                                                                      int32_t* __restrict__ end_new, float* __restrict__ log_z) {
  __shared__ __attribute__((aligned(16))) float s_u[64];
  track_gated_stream_scan_body(logits, ldl, gate, ldg, n, C, lam, mu, t_old, state, lag, posterior, bp_new, a_new, end_new, log_z, blockIdx.x == 1, s_u);
}

// Every pointer of the committed block and the tail of one stream's read-out.
struct TrackGatedStreamOut {
  int32_t* cls_lag;  int32_t* sync_lag;  float* conf_lag;
  float* post_lag;  int64_t ldp;  float* p_sync_lag;  int32_t* cls_post_lag;  float* conf_post_lag;  float* offset_mean_lag;
  int32_t* cls_tail;  int32_t* sync_tail;  float* conf_tail;
  // the same block `commit0` committed windows / `tail0` tail entries further on (a pool's packed outputs)
  __host__ __device__ TrackGatedStreamOut at(int64_t commit0, int64_t tail0) const {
    TrackGatedStreamOut o = *this;
    o.cls_lag += commit0;  o.sync_lag += commit0;  o.conf_lag += commit0;
    o.post_lag += commit0 * ldp;  o.p_sync_lag += commit0;  o.cls_post_lag += commit0;  o.conf_post_lag += commit0;  o.offset_mean_lag += commit0;
    o.cls_tail += tail0;  o.sync_tail += tail0;  o.conf_tail += tail0;
    return o;
  }
};

// Block i < n_commit: window w = w0 + i, read from the prefix that ends at row R = min(w + lag, t_last); block n_commit (if n_tail > 0): the tail.  The backtrace is
// track_stream_backtrace over rows of 2C back pointers (every index read clamped below 2C); the state j it arrives at is written as cls = j % C, sync = j / C.
// s_u (16-byte aligned) / s_b: 64 floats of LDS each, s_tail: 256 ints.
template <bool POST>
__device__ __forceinline__ void track_gated_stream_readout_body(const TrackGatedStreamRows& rows, float lam, float mu, const float* __restrict__ grid, int64_t w0,
                                                                int n_commit, int n_tail, int64_t t_last, const TrackGatedStreamOut& out, int bx, float* s_u, float* s_b,
                                                                int* s_tail) {
  const int C = rows.C, S = 2 * C;
  const TrackGatedLane ln(C);
  if (bx == n_commit) {                                            // the tail
    const int64_t w = t_last - (n_tail - 1);
    int cur = rows.end(t_last);
    cur = cur < 0 ? 0 : (cur >= S ? S - 1 : cur);
    track_stream_backtrace<true>(rows, t_last, w, cur, ln.j, ln.live, s_tail);
    __syncthreads();
    for (int i = threadIdx.x; i < n_tail; i += 64) {
      const float* row = rows.logits(w + i);
      int best;
      float m, sum;
      track_row_stats(row, C, best, m, sum);
      const int cls = s_tail[i] % C;
      out.cls_tail[i] = cls;
      out.sync_tail[i] = s_tail[i] / C;
      out.conf_tail[i] = track_row_conf(row, C, cls, m, sum);
    }
    return;
  }
  const int i = bx;
  const int64_t w = w0 + i;
  const int64_t R = w + rows.lag < t_last ? w + rows.lag : t_last;
  int cur = rows.end(R);
  cur = cur < 0 ? 0 : (cur >= S ? S - 1 : cur);
  cur = track_stream_backtrace<false>(rows, R, w, cur, ln.j, ln.live, nullptr);
  if (ln.j == 0) {
    const float* row = rows.logits(w);
    int best;
    float m, sum;
    track_row_stats(row, C, best, m, sum);
    out.cls_lag[i] = cur % C;
    out.sync_lag[i] = cur / C;
    out.conf_lag[i] = track_row_conf(row, C, cur % C, m, sum);
  }
  if (POST) {
    // the backward scan of the prefix 0 .. R, from its end down to row w:  b_R = 0;  b_r[j] = lse_n (b_{r+1}[n] + E[r+1, n] + T(j, n)), renormalised per step
    const int C4 = (C + 3) & ~3;
    const float ninf = -INFINITY;
    const float log_c = logf((float)C);
    const bool loads = ln.live && ln.m;
    const int slot = ln.m * 32 + ln.c;
    s_u[threadIdx.x] = ninf;                                       // (ordered before the planes' stores by the loop's first barrier)
    float v = ln.live ? 0.f : ninf;
    float l_next = loads ? rows.logits(R)[ln.c] : ninf;
    float z0_next = rows.gate(R)[0], z1_next = rows.gate(R)[1];
    for (int64_t r = R; r > w; --r) {                              // b_{r-1} from b_r and row r
      const float l = l_next, z0 = z0_next, z1 = z1_next;
      if (r - 1 > w) {
        l_next = loads ? rows.logits(r - 1)[ln.c] : ninf;
        z0_next = rows.gate(r - 1)[0];
        z1_next = rows.gate(r - 1)[1];
      }
      const float e = track_gated_emission(ln, l, z0, z1, log_c);
      __syncthreads();                                             // every lane has read s_u
      if (ln.live) s_u[slot] = v + e;
      __syncthreads();
      float m;
      v = track_gated_fb_step(ln, s_u, C4, true, lam, mu, 0.f, m);
    }
    if (ln.live) s_b[ln.j] = v;
    __syncthreads();
    if (ln.j == 0) {
      int best;
      float pbest, mean, ps;
      track_gated_combine_row(rows.a(w), s_b, C, grid, out.post_lag + (int64_t)i * out.ldp, best, pbest, mean, ps);
      out.p_sync_lag[i] = ps;
      out.cls_post_lag[i] = best;
      out.conf_post_lag[i] = pbest;
      out.offset_mean_lag[i] = mean;
    }
  }
}

template <bool POST>
__global__ __launch_bounds__(64) void track_gated_stream_readout_kernel(TrackGatedStreamRows rows, float lam, float mu, const float* __restrict__ grid, int64_t w0,
                                                                         int n_commit, int n_tail, int64_t t_last, TrackGatedStreamOut out) {
  __shared__ __attribute__((aligned(16))) float s_u[64];
  __shared__ float s_b[64];
  __shared__ int s_tail[256];
  track_gated_stream_readout_body<POST>(rows, lam, mu, grid, w0, n_commit, n_tail, t_last, out, (int)blockIdx.x, s_u, s_b, s_tail);
}

// Ring row j of a push: new row k = k0 + j (row t_old + k of the stream) into slot (t_old + k) % lag of the rings: C offset logits, 2 gate logits, 2C back pointers
// and (posterior) 2C entries of a, one lane per entry.
__device__ __forceinline__ void track_gated_stream_keep_body(const float* __restrict__ logits, int64_t ldl, const float* __restrict__ gate, int64_t ldg,
                                                             const uint8_t* __restrict__ bp_new, const float* __restrict__ a_new, int k0, int64_t t_old, int C, int lag,
                                                             int posterior, unsigned char* __restrict__ state, int j) {
  const TrackGatedStreamLayout lay(C, lag, posterior != 0);
  const int c = threadIdx.x;
  const int S = 2 * C;
  if (c >= S) return;
  const int64_t k = k0 + (int64_t)j;
  const int64_t ring = (t_old + k) % lag;
  if (c < C) reinterpret_cast<float*>(state + lay.lg_ring)[ring * C + c] = logits[k * ldl + c];
  if (c < 2) reinterpret_cast<float*>(state + lay.gz_ring)[ring * 2 + c] = gate[k * ldg + c];
  (state + lay.bp_ring)[ring * S + c] = bp_new[k * S + c];
  if (posterior) reinterpret_cast<float*>(state + lay.a_ring)[ring * S + c] = a_new[k * S + c];
}

// Block j: ring row j.
__global__ __launch_bounds__(64) void track_gated_stream_keep_kernel(const float* __restrict__ logits, int64_t ldl, const float* __restrict__ gate, int64_t ldg,
                                                                      const uint8_t* __restrict__ bp_new, const float* __restrict__ a_new, int k0, int64_t t_old, int C,
                                                                      int lag, int posterior, unsigned char* __restrict__ state) {
  track_gated_stream_keep_body(logits, ldl, gate, ldg, bp_new, a_new, k0, t_old, C, lag, posterior, state, (int)blockIdx.x);
}

// What sf_track_stream_push and track_gated_args_ok refuse, for the two gated stream launchers: C (2 .. 32), lag, lam, mu and - when there are rows - the strides.
static bool track_gated_stream_args_ok(const char* who, int C, int lag, int n, int64_t ldl, int64_t ldg, float lam, float mu) {
  if (lag < 0 || lag > 255) { sf_set_error("%s: lag = %d windows out of range (0 .. 255)", who, lag); return false; }
  if (n < 0 || n > TRACK_STREAM_MAX_PUSH) { sf_set_error("%s: n = %d rows in one push (0 .. %d: split a longer catch-up)", who, n, TRACK_STREAM_MAX_PUSH); return false; }
  return track_gated_args_ok(who, n, C, n ? ldl : (int64_t)C, n ? ldg : (int64_t)2, lam, mu);
}

extern "C" int sf_track_stream_gated_bytes(int C, int lag, int posterior) {
  if (!track_gated_stream_args_ok("sf_track_stream_gated_bytes", C, lag, 0, 0, 0, 0.f, 0.f)) return -1;
  return (int)TrackGatedStreamLayout(C, lag, posterior != 0).total;      // at most 16 + 512 + 255 * (32 * 4 + 8 + 64 * 4 + 64)
}

// the workspace of a gated push: [posterior: a (n, 2C) fp32][end (n) int32][back pointers (n, 2C) bytes] - TrackPoolWorkspace over rows of 2C
extern "C" int sf_track_stream_gated_workspace_bytes(int C, int n, int posterior) {
  if (!track_gated_stream_args_ok("sf_track_stream_gated_workspace_bytes", C, 0, n, C, 2, 0.f, 0.f)) return -1;
  return (int)(((posterior ? (int64_t)n * 2 * C * 4 : 0) + (int64_t)n * 4 + (int64_t)n * 2 * C + 15) & ~(int64_t)15);      // at most 2^20 * 324
}

extern "C" int sf_track_pool_gated_workspace_bytes(int C, int total_rows, int posterior) { return sf_track_stream_gated_workspace_bytes(C, total_rows, posterior); }

extern "C" int sf_track_stream_push_gated(void* state, int C, int lag, int posterior, int64_t rows_done, const float* logits, int64_t ldl, const float* gate_logits,
                                          int64_t ldg, int n, float lam, float mu, const float* grid, int final, int32_t* cls_raw, float* conf_raw, float* sync_raw,
                                          int32_t* cls_lag, int32_t* sync_lag, float* conf_lag, float* post_lag, int64_t ldp, float* p_sync_lag, int32_t* cls_post_lag,
                                          float* conf_post_lag, float* offset_mean_lag, int32_t* cls_tail, int32_t* sync_tail, float* conf_tail, float* log_z,
                                          void* workspace, void* stream) {
  const char* who = "sf_track_stream_push_gated";
  if (!track_gated_stream_args_ok(who, C, lag, n, ldl, ldg, lam, mu)) return -1;
  SF_CHECK_ARG(state, "%s: null state", who);
  SF_CHECK_ARG(rows_done >= 0 && rows_done <= (INT64_MAX >> 1), "%s: %lld rows pushed so far", who, (long long)rows_done);
  const int64_t t_old = rows_done, t_new = rows_done + n;
  const int64_t done_old = t_old > lag ? t_old - lag : 0;                                   // windows committed before this push
  const int64_t done_new = final ? t_new : (t_new > lag ? t_new - lag : 0);
  const int64_t n_commit = done_new - done_old, n_tail = t_new - done_new;
  if (t_new == 0) return 0;
  SF_CHECK_ARG(n == 0 || (logits && gate_logits && cls_raw && conf_raw && sync_raw && workspace), "%s: null pointer (new rows)", who);
  SF_CHECK_ARG(n_commit == 0 || (cls_lag && sync_lag && conf_lag), "%s: null pointer (committed block)", who);
  SF_CHECK_ARG(n_tail == 0 || (cls_tail && sync_tail && conf_tail), "%s: null pointer (tail)", who);
  if (posterior) {
    SF_CHECK_ARG(log_z, "%s: null log_z", who);
    SF_CHECK_ARG(n_commit == 0 || (grid && post_lag && p_sync_lag && cls_post_lag && conf_post_lag && offset_mean_lag && ldp >= C),
                 "%s: null pointer or post row stride ldp = %lld below C = %d (posterior block)", who, (long long)ldp, C);
  }
  hipStream_t s = (hipStream_t)stream;
  const TrackGatedStreamLayout lay(C, lag, posterior != 0);
  unsigned char* st = static_cast<unsigned char*>(state);
  const TrackPoolWorkspace ws(static_cast<unsigned char*>(workspace), 2 * C, n, posterior != 0);
  if (n > 0) {
    hipLaunchKernelGGL(track_gated_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, logits, ldl, gate_logits, ldg, n, C, cls_raw, conf_raw, sync_raw);
    SF_LAUNCH_CHECK();
  }
  if (n > 0 || posterior) {                                        // (n == 0 with the posterior: log_z of the prefix so far, from the carried a)
    hipLaunchKernelGGL(track_gated_stream_scan_kernel, dim3(posterior ? 2 : 1), dim3(64), 0, s, logits, ldl, gate_logits, ldg, n, C, lam, mu, t_old, st, lag, posterior,
                       ws.bp, ws.a, ws.end, log_z);
    SF_LAUNCH_CHECK();
  }
  if (n_commit + n_tail > 0) {
    TrackGatedStreamRows rows;
    track_gated_rows_fill(rows, lay, st, logits, ldl, gate_logits, ldg, ws.bp, ws.a, ws.end, t_old, lag, C);
    const TrackGatedStreamOut out{cls_lag, sync_lag, conf_lag, post_lag, ldp, p_sync_lag, cls_post_lag, conf_post_lag, offset_mean_lag, cls_tail, sync_tail, conf_tail};
    const dim3 g((unsigned)(n_commit + (n_tail > 0 ? 1 : 0)));
    if (posterior)
      hipLaunchKernelGGL(track_gated_stream_readout_kernel<true>, g, dim3(64), 0, s, rows, lam, mu, grid, done_old, (int)n_commit, (int)n_tail, t_new - 1, out);
    else
      hipLaunchKernelGGL(track_gated_stream_readout_kernel<false>, g, dim3(64), 0, s, rows, lam, mu, grid, done_old, (int)n_commit, (int)n_tail, t_new - 1, out);
    SF_LAUNCH_CHECK();
  }
  const int keep = n < lag ? n : lag;
  if (keep > 0) {
    hipLaunchKernelGGL(track_gated_stream_keep_kernel, dim3((unsigned)keep), dim3(64), 0, s, logits, ldl, gate_logits, ldg, (const uint8_t*)ws.bp, (const float*)ws.a,
                       n - keep, t_old, C, lag, posterior, st);
    SF_LAUNCH_CHECK();
  }
  return 0;
}

// The pool's kernels: sf_track_pool_push's mapping (blockIdx.y = the table row, blockIdx.x = the stream's own work item), every block running the gated bodies above on
// its stream's context.  Stream e's gate rows are rows [row0, row0 + n) of the gate matrix, as its offset rows are of logits.
__global__ __launch_bounds__(64) void track_gated_pool_scan_kernel(const int64_t* __restrict__ table, unsigned char* __restrict__ states, int64_t state_stride,
                                                                    const float* __restrict__ logits, int64_t ldl, const float* __restrict__ gate, int64_t ldg, int C,
                                                                    float lam, float mu, int lag, int posterior, unsigned char* __restrict__ workspace, int total_rows,
                                                                    float* __restrict__ log_z) {
  __shared__ __attribute__((aligned(16))) float s_u[64];
  const TrackPoolEntry e(table, blockIdx.y, lag);
  const bool fwd = blockIdx.x == 1;
  if (e.t_new == 0 || (e.n == 0 && !fwd)) return;                  // an empty stream; nothing to scan (n == 0 with the posterior: log_z from the carried a)
  const TrackPoolWorkspace ws(workspace, 2 * C, total_rows, posterior != 0);
  track_gated_stream_scan_body(logits + e.row0 * ldl, ldl, gate + e.row0 * ldg, ldg, (int)e.n, C, lam, mu, e.t_old, states + e.slot * state_stride, lag, posterior,
                               ws.bp + e.row0 * 2 * C, ws.a + e.row0 * 2 * C, ws.end + e.row0, log_z + blockIdx.y, fwd, s_u);
}

template <bool POST>
__global__ __launch_bounds__(64) void track_gated_pool_readout_kernel(const int64_t* __restrict__ table, const unsigned char* __restrict__ states, int64_t state_stride,
                                                                       const float* __restrict__ logits, int64_t ldl, const float* __restrict__ gate, int64_t ldg, int C,
                                                                       float lam, float mu, int lag, const float* __restrict__ grid,
                                                                       const unsigned char* __restrict__ workspace, int total_rows, TrackGatedStreamOut out) {
  __shared__ __attribute__((aligned(16))) float s_u[64];
  __shared__ float s_b[64];
  __shared__ int s_tail[256];
  const TrackPoolEntry e(table, blockIdx.y, lag);
  if ((int64_t)blockIdx.x >= e.readout_blocks()) return;
  const TrackGatedStreamLayout lay(C, lag, POST);
  const TrackPoolWorkspace ws(const_cast<unsigned char*>(workspace), 2 * C, total_rows, POST);
  TrackGatedStreamRows rows;
  track_gated_rows_fill(rows, lay, states + e.slot * state_stride, logits + e.row0 * ldl, ldl, gate + e.row0 * ldg, ldg, ws.bp + e.row0 * 2 * C, ws.a + e.row0 * 2 * C,
                        ws.end + e.row0, e.t_old, lag, C);
  track_gated_stream_readout_body<POST>(rows, lam, mu, grid, e.done_old, (int)e.n_commit, (int)e.n_tail, e.t_new - 1, out.at(e.commit0, e.tail0), (int)blockIdx.x, s_u, s_b,
                                        s_tail);
}

__global__ __launch_bounds__(64) void track_gated_pool_keep_kernel(const int64_t* __restrict__ table, unsigned char* __restrict__ states, int64_t state_stride,
                                                                    const float* __restrict__ logits, int64_t ldl, const float* __restrict__ gate, int64_t ldg, int C,
                                                                    int lag, int posterior, const unsigned char* __restrict__ workspace, int total_rows) {
  const TrackPoolEntry e(table, blockIdx.y, lag);
  const int64_t keep = e.keep(lag);
  if ((int64_t)blockIdx.x >= keep) return;
  const TrackPoolWorkspace ws(const_cast<unsigned char*>(workspace), 2 * C, total_rows, posterior != 0);
  track_gated_stream_keep_body(logits + e.row0 * ldl, ldl, gate + e.row0 * ldg, ldg, ws.bp + e.row0 * 2 * C, ws.a + e.row0 * 2 * C, (int)(e.n - keep), e.t_old, C, lag,
                               posterior, states + e.slot * state_stride, (int)blockIdx.x);
}

extern "C" int sf_track_pool_push_gated(void* states, int64_t state_stride, int n_slots, int C, int lag, int posterior, const int64_t* table_host,
                                        const int64_t* table_dev, int n_active, const float* logits, int64_t ldl, const float* gate_logits, int64_t ldg, int total_rows,
                                        float lam, float mu, const float* grid, int32_t* cls_raw, float* conf_raw, float* sync_raw, int32_t* cls_lag, int32_t* sync_lag,
                                        float* conf_lag, float* post_lag, int64_t ldp, float* p_sync_lag, int32_t* cls_post_lag, float* conf_post_lag,
                                        float* offset_mean_lag, int32_t* cls_tail, int32_t* sync_tail, float* conf_tail, float* log_z, void* workspace, void* stream) {
  const char* who = "sf_track_pool_push_gated";
  SF_CHECK_ARG(total_rows >= 0 && total_rows <= TRACK_STREAM_MAX_PUSH, "%s: total_rows = %d rows in one push (0 .. %d)", who, total_rows, TRACK_STREAM_MAX_PUSH);
  if (!track_gated_stream_args_ok(who, C, lag, 0, 0, 0, lam, mu)) return -1;
  SF_CHECK_ARG(n_active >= 1 && n_active <= TRACK_POOL_MAX_ACTIVE, "%s: n_active = %d streams in one push (1 .. %d)", who, n_active, TRACK_POOL_MAX_ACTIVE);
  SF_CHECK_ARG(n_slots >= 1, "%s: n_slots = %d", who, n_slots);
  SF_CHECK_ARG(states && table_host && table_dev, "%s: null pointer (states or table)", who);
  const TrackGatedStreamLayout lay(C, lag, posterior != 0);
  SF_CHECK_ARG(state_stride >= lay.total && state_stride % 16 == 0, "%s: state stride %lld: a multiple of 16, at least %lld bytes", who, (long long)state_stride,
               (long long)lay.total);
  TrackPoolTotals tot;
  if (track_pool_table_check(who, table_host, n_active, n_slots, total_rows, lag, posterior, tot)) return -1;
  SF_CHECK_ARG(tot.sum_n == 0 || ldl >= C, "%s: row stride ldl = %lld below C = %d", who, (long long)ldl, C);
  SF_CHECK_ARG(tot.sum_n == 0 || ldg >= 2, "%s: gate row stride ldg = %lld below 2", who, (long long)ldg);
  SF_CHECK_ARG(tot.sum_n == 0 || (logits && gate_logits && cls_raw && conf_raw && sync_raw && workspace), "%s: null pointer (new rows)", who);
  SF_CHECK_ARG(tot.sum_commit == 0 || (cls_lag && sync_lag && conf_lag), "%s: null pointer (committed block)", who);
  SF_CHECK_ARG(tot.sum_tail == 0 || (cls_tail && sync_tail && conf_tail), "%s: null pointer (tail)", who);
  if (posterior) {
    SF_CHECK_ARG(!tot.scan || log_z, "%s: null log_z", who);
    SF_CHECK_ARG(tot.sum_commit == 0 || (grid && post_lag && p_sync_lag && cls_post_lag && conf_post_lag && offset_mean_lag && ldp >= C),
                 "%s: null pointer or post row stride ldp = %lld below C = %d (posterior block)", who, (long long)ldp, C);
  }
  hipStream_t s = (hipStream_t)stream;
  unsigned char* st = static_cast<unsigned char*>(states);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  if (tot.sum_n > 0) {                                             // one thread per row of the packed matrices
    hipLaunchKernelGGL(track_gated_rows_kernel, dim3((unsigned)((total_rows + 255) / 256)), dim3(256), 0, s, logits, ldl, gate_logits, ldg, total_rows, C, cls_raw,
                       conf_raw, sync_raw);
    SF_LAUNCH_CHECK();
  }
  if (tot.scan) {
    hipLaunchKernelGGL(track_gated_pool_scan_kernel, dim3(posterior ? 2 : 1, (unsigned)n_active), dim3(64), 0, s, table_dev, st, state_stride, logits, ldl, gate_logits, ldg,
                       C, lam, mu, lag, posterior, ws, total_rows, log_z);
    SF_LAUNCH_CHECK();
  }
  if (tot.max_read > 0) {
    const TrackGatedStreamOut out{cls_lag, sync_lag, conf_lag, post_lag, ldp, p_sync_lag, cls_post_lag, conf_post_lag, offset_mean_lag, cls_tail, sync_tail, conf_tail};
    const dim3 g((unsigned)tot.max_read, (unsigned)n_active);
    if (posterior)
      hipLaunchKernelGGL(track_gated_pool_readout_kernel<true>, g, dim3(64), 0, s, table_dev, (const unsigned char*)st, state_stride, logits, ldl, gate_logits, ldg, C, lam, mu,
                         lag, grid, (const unsigned char*)ws, total_rows, out);
    else
      hipLaunchKernelGGL(track_gated_pool_readout_kernel<false>, g, dim3(64), 0, s, table_dev, (const unsigned char*)st, state_stride, logits, ldl, gate_logits, ldg, C, lam, mu,
                         lag, grid, (const unsigned char*)ws, total_rows, out);
    SF_LAUNCH_CHECK();
  }
  if (tot.max_keep > 0) {
    hipLaunchKernelGGL(track_gated_pool_keep_kernel, dim3((unsigned)tot.max_keep, (unsigned)n_active), dim3(64), 0, s, table_dev, st, state_stride, logits, ldl, gate_logits,
                       ldg, C, lag, posterior, (const unsigned char*)ws, total_rows);
    SF_LAUNCH_CHECK();
  }
  return 0;
}
