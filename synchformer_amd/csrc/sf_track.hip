// Track read-out of a recording's per-window logits: per-window argmax / confidence and a Viterbi path under a cost on class changes.
// The logits of W overlapping windows (engine.sync_windows) are W noisy votes on an offset that changes slowly; the per-window argmax flickers
// between neighbouring classes, the path that maximises
//     sum_w e[w, c_w] - lam * sum_{w >= 1} |c_w - c_{w-1}|,        e[w, c] = logits[w, c] - max_c logits[w, .]
// does not.  e is log-softmax up to a row constant (a row constant cannot change the path), and for dyadic logits / lam every operation below is exact in fp32.
// sf_track_decode: three launches on the caller's stream, all latency-bound (W x C <= W x 64 floats):
//   1. track_rows_kernel<false>: one thread per window: argmax (lowest index on ties), softmax probability of that class (fp32 statistics);
//   2. track_viterbi_kernel:     ONE wavefront, lane c = class c, the previous step's scores in LDS: the forward scan over W, then the backtrace;
//   3. track_rows_kernel<true>:  one thread per window: softmax probability of the path's class.
// Reference read-out this stands next to: decode_single_video_prediction (example.py:38-56: softmax + top-k of ONE window) on the class grid of
// make_class_grid (dataset/transforms.py:221-239); the reference has no recording-level read-out.
//
// sf_track_posterior reads the same chain out as marginals: the path above is the mode of
//     p(c_0 .. c_{W-1})  ~  exp(sum_w e[w, c_w] - lam * sum_w |c_w - c_{w-1}|),        e = the true log-softmax,
// and the forward-backward algorithm gives post[w, c] = p(c_w = c) and log_z = log of the sum over all paths.  Two launches:
//   1. track_fb_scan_kernel:     TWO workgroups of one wavefront each, side by side: block 0 the forward scan (a, and log_z), block 1 the backward scan (b);
//   2. track_fb_combine_kernel:  one thread per window: post = softmax_c (a + b), its argmax and value, the posterior mean of the grid.
// sf_track_pairwise combines the two scans across a boundary (track_pairwise_kernel, track_pairwise_gated_kernel): the joint marginal of neighbouring windows, its off-diagonal mass (the
// probability that the offset changed there) and the expected class step - what a fit of lam / mu needs.
// The _gated forms read out one chain over (offset class, synchronizable flag), fed by a second head.
//
// The file has three parts.  First the arithmetic: the rows kernels and the step functions of the plain and the gated chain.  Then the two chains: a chain is a small
// policy struct (TrackChainPlain over the C offset classes, TrackChainGated over the 2C states) that says what a lane, a row's inputs, a step, an LDS slot and a ring
// are, around those step functions.  Everything after them is written ONCE, as templates on a chain, but for two pieces that measured slower folded and say so where
// they stand (the plain chain's own Viterbi kernel, the two pairwise kernels; a chain names its kernel through launch_viterbi / launch_pairwise): the
// whole-recording kernels (Viterbi scan + backtrace, the two forward-backward scans, the combine) with the three launchers of the whole-recording entries, and the
// read-out of live feeds at a fixed lag with carried state - the rows struct, the state layout, the scan / read-out / keep bodies, the three stream and three pool
// kernels and their two launchers.  sf_track_stream_push(_gated) read
// one stream, sf_track_pool_push(_gated) many in one call: the same launches over a descriptor table, blockIdx.y = the stream, every block running the single-stream
// bodies on its stream's context.  Every extern "C" entry packs its arguments (a chain's Src, a TrackStreamOut) and calls a launcher template.
#include "sf_common.h"
#include "sf_track_math.h"
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

// ---- forward-backward (posterior) read-out --------------------------------------------------------------------------------------------------------------
// Log domain throughout (a scaled linear-domain recursion underflows: exp(-lam * 20 steps) is 0 in fp32 at lam = 8).  -inf is a masked class: every
// subtraction that could meet (-inf) - (-inf) is guarded (fb_finite_or_zero on the subtrahend), so a row with one finite logit produces no NaN.

// (fb_finite_or_zero: sf_track_math.h, shared with the wide chain)

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

// The end state of a row: the lowest class whose renormalised score is the maximum, 0.  (No such lane - NaN scores - gives class 0, as a NaN never wins `>`.)
__device__ __forceinline__ int track_wave_end_state(float s, bool live) {
  const unsigned long long hit = __ballot(live && s == 0.f);
  return hit ? __ffsll((long long)hit) - 1 : 0;
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

// (gate_softplus: sf_track_math.h, shared with the wide chain)

// What a lane of the gated scans is: its state's plane m and class c, its partner's lane.  Idle lanes (j >= 2C) act as state 0 and are their own partner.
// lane: the thread's lane in its wavefront - threadIdx.x in the one-wave blocks of the scans.
struct TrackGatedLane {
  int j, m, c, partner;
  bool live;
  __device__ __forceinline__ TrackGatedLane(int C, int lane = threadIdx.x) {
    j = lane;
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
// the other plane's best from its partner, subtracts mu, and settles the tie between the planes (m' = 0 wins).  The whole-recording kernel and the stream's scan both call
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

// ---- pairwise marginals of neighbouring windows (sf_track_pairwise, sf_track_pairwise_gated) --------------------------------------------------------
// With a, b the two forward-backward scans (left in the workspace by track_fb_scan_kernel) the joint marginal of windows w and w + 1 is
//     xi_w[p, c] = exp(t[p, c] - lse_{p,c} t),        t[p, c] = a_w[p] - lam |p - c| + e[w+1, c] + b_{w+1}[c]
// (the constants the scans subtracted per row cancel), over the states (p, m') -> (c, m) with - mu [m' != m] for the gated chain.  The two pairwise kernels (below the
// chains) walk it, one wavefront per boundary; these are the pieces of them that do not depend on the chain.  Every wave reduction is a butterfly in a fixed order; no
// atomics: the outputs are the same bits from call to call.

// What a lane gathers in walk 2: sum = all of its column, off = the entries with p != c, jump = sum |p - c| x; best / bp = its largest off-diagonal entry, the lowest p
// on ties (strict `>` in ascending p; a NaN never wins).  bp starts at the lowest p != c, so a column without mass still names an off-diagonal pair.
struct TrackPairAcc {
  float sum, off, jump, best;
  int bp;
  __device__ __forceinline__ TrackPairAcc(int c) : sum(0.f), off(0.f), jump(0.f), best(0.f), bp(c == 0 ? 1 : 0) {}
  __device__ __forceinline__ void add(float x, int p, int c) {
    sum += x;
    if (p != c) {
      off += x;
      jump += x * fabsf((float)(p - c));
      if (x > best) { best = x; bp = p; }
    }
  }
};

// The wave's best off-diagonal pair from the lanes' candidates (x, p, c): the largest x, then the lowest p, then the lowest c - a total order, so the butterfly leaves
// the same triple in every lane.  Lanes that hold no column pass x = -1 and never win.
__device__ __forceinline__ void track_pair_top(float& x, int& p, int& c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float x2 = __shfl_xor(x, o, 64);
    const int p2 = __shfl_xor(p, o, 64), c2 = __shfl_xor(c, o, 64);
    if (x2 > x || (x2 == x && (p2 < p || (p2 == p && c2 < c)))) { x = x2; p = p2; c = c2; }
  }
}

// The boundary's scalars, by lane 0 of its wave.  z = the sum over all pairs of exp(t - max t) (>= 1 unless every pair is masked).  Whatever the input held, bp and
// bc lie in [0, C) and differ: a candidate replaces a lane's first one (the lowest p != c) only through `x > best` with p != c, which neither a NaN nor the +0 of an
// entry beyond C passes, and the winning lane is one that holds a column (C >= 2 of them pass best >= 0, the others -1).
__device__ __forceinline__ void track_pair_write(int w, float z, float off, float jump, float best, int bp, int bc, float* __restrict__ p_change,
                                                 float* __restrict__ jump_abs, int32_t* __restrict__ top_from, int32_t* __restrict__ top_to, float* __restrict__ p_top) {
  p_change[w] = off / z;
  jump_abs[w] = jump / z;
  top_from[w] = bp;
  top_to[w] = bc;
  p_top[w] = best / z;
}

// ---- the two chains ------------------------------------------------------------------------------------------------------------------------------------------
// The kernels and launchers below this section are templates on a CHAIN (two pieces excepted, which say why where they stand).  A chain says how many states a row has, what a lane of the scanning wavefront is (the chain
// object itself, built per thread), what the inputs of a row are and how they are loaded (Src: pointers and strides positioned at a row; In: one row's values in a
// lane), the first row of the Viterbi scan, the emission, the two steps, where a lane's entry lies in LDS, how one row is combined,
// what the keep step copies of the inputs, how a path state is written out and which rows, Viterbi and pairwise kernels are its own.  The arithmetic is that of the step functions above: a
// chain calls them, it does not restate them.  A new chain (say, a third state dimension) is a new policy struct; nothing below it changes.

// Every pointer of the committed block and the tail of one stream's read-out; the offline posterior entries fill in the posterior block alone, one entry per window.
// The plain chain leaves the sync pointers null and never touches them.
struct TrackStreamOut {
  int32_t* cls_lag;  int32_t* sync_lag;  float* conf_lag;
  float* post_lag;  int64_t ldp;  float* p_sync_lag;  int32_t* cls_post_lag;  float* conf_post_lag;  float* offset_mean_lag;
  int32_t* cls_tail;  int32_t* sync_tail;  float* conf_tail;
  // the same block `commit0` committed windows / `tail0` tail entries further on (a pool's packed outputs)
  __host__ __device__ TrackStreamOut at(int64_t commit0, int64_t tail0) const {
    TrackStreamOut o = *this;
    o.cls_lag += commit0;  o.sync_lag += commit0;  o.conf_lag += commit0;
    o.post_lag += commit0 * ldp;  o.p_sync_lag += commit0;  o.cls_post_lag += commit0;  o.conf_post_lag += commit0;  o.offset_mean_lag += commit0;
    o.cls_tail += tail0;  o.sync_tail += tail0;  o.conf_tail += tail0;
    return o;
  }
};

// The chain over the C offset classes (sf_track_decode / sf_track_posterior): lane j = class j, one logit per row and lane, the scan vectors contiguous in LDS (the
// idle lanes store their -inf, which is what fb_transition_lse reads behind class C - 1).
struct TrackChainPlain {
  static constexpr int MAX_C = TRACK_MAX_C;
  static constexpr int GATE_WIDTH = 0;                             // floats of a row's second input: none
  static constexpr bool LDS_PREFILL = false;
  static constexpr bool VITERBI_TAKES_EMISSION = false;            // track_viterbi_step takes the logit: its e = l - max is its own
  static constexpr const char* LANE_IS = "class";
  __host__ __device__ static int states(int C) { return C; }
  struct Src {
    const float* lg;  int64_t ldl;
    __host__ __device__ Src at(int64_t r) const { return Src{lg + r * ldl, ldl}; }
    bool ok() const { return lg != nullptr; }
    bool strides_ok(const char* who, int C) const {
      if (ldl < C) { sf_set_error("%s: row stride ldl = %lld below C = %d", who, (long long)ldl, C); return false; }
      return true;
    }
  };
  struct In { float l; };
  static bool sync_ok(const void*) { return true; }                // the chain has no sync outputs: nothing to refuse
  static void launch_rows(const Src& src, int n, int C, int32_t* cls_raw, float* conf_raw, float*, hipStream_t s) {
    hipLaunchKernelGGL(track_rows_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src.lg, src.ldl, n, C, cls_raw, conf_raw);
  }
  // the chain's Viterbi and pairwise kernels of a whole recording (defined below them: which are templates on the chain and which are not, and why)
  static void launch_viterbi(const Src& src, int W, int C, float lam, float mu, int32_t* cls_path, int32_t* sync_path, uint8_t* backptr, hipStream_t s);
  static void launch_pairwise(const Src& src, const float* ws, int W, int C, float lam, float mu, float* p_change, float* jump_abs, float* p_flip, int32_t* top_from,
                              int32_t* top_to, float* p_top, float* xi, hipStream_t s);

  int j;
  bool live;
  __device__ __forceinline__ TrackChainPlain(int C, int lane = threadIdx.x) : j(lane), live(j < C) {}
  __device__ __forceinline__ In load(const Src& row, bool have) const { return In{(live && have) ? row.lg[j] : -INFINITY}; }
  template <class Rows>
  __device__ __forceinline__ In load_row(const Rows& rows, int64_t r) const { return In{live ? rows.logits(r)[j] : -INFINITY}; }
  __device__ __forceinline__ float first_viterbi(const In& in, float) const { return in.l - wave_max(in.l); }      // s_0 = e[0]; -inf in the idle lanes
  __device__ __forceinline__ float emission(const In& in) const { return fb_log_softmax(in.l); }
  __device__ __forceinline__ float viterbi_step(const float* s_u, int C, float lam, float, const In& in, float, int& bp) const {
    return track_viterbi_step(s_u, C, j, live, lam, in.l, bp);
  }
  __device__ __forceinline__ float fb_step(const float* s_u, int C4, bool back, float lam, float, float e, float& m) const {
    return fb_scan_step(s_u, C4, j, live, back, lam, e, m);
  }
  __device__ __forceinline__ void put(float* s_u, bool, float v) const { s_u[j] = v; }
  __device__ __forceinline__ static int put_state(int state, int, int32_t* cls, int32_t*, int64_t i) { cls[i] = state;  return state; }
  __device__ __forceinline__ static void combine(const float* a, const float* b, int C, const float* __restrict__ grid, const TrackStreamOut& out, int i) {
    int best;
    float pbest, mean;
    fb_combine_row(a, b, C, grid, out.post_lag + (int64_t)i * out.ldp, best, pbest, mean);
    out.cls_post_lag[i] = best;
    out.conf_post_lag[i] = pbest;
    out.offset_mean_lag[i] = mean;
  }
  __device__ __forceinline__ static void keep_inputs(const Src& row, float* lg_slot, float*, int c, int) { lg_slot[c] = row.lg[c]; }
};

// The chain over the 2C states j = m * C + c (sf_track_decode_gated / sf_track_posterior_gated): a lane is a TrackGatedLane, a row brings the offset logit (in the
// lanes of plane 1) and the two gate logits (wave-uniform), the Viterbi scores lie state-major in LDS and the forward vector as two planes of 32 over a -inf fill.
struct TrackChainGated : TrackGatedLane {
  static constexpr int MAX_C = TRACK_GATE_MAX_C;
  static constexpr int GATE_WIDTH = 2;
  static constexpr bool LDS_PREFILL = true;
  static constexpr bool VITERBI_TAKES_EMISSION = true;             // both scans of a row start from one emission
  static constexpr const char* LANE_IS = "(class, flag) state";
  __host__ __device__ static int states(int C) { return 2 * C; }
  struct Src {
    const float* lg;  int64_t ldl;  const float* gz;  int64_t ldg;
    __host__ __device__ Src at(int64_t r) const { return Src{lg + r * ldl, ldl, gz + r * ldg, ldg}; }
    bool ok() const { return lg != nullptr && gz != nullptr; }
    bool strides_ok(const char* who, int C) const {
      if (ldl < C) { sf_set_error("%s: row stride ldl = %lld below C = %d", who, (long long)ldl, C); return false; }
      if (ldg < 2) { sf_set_error("%s: gate row stride ldg = %lld below 2", who, (long long)ldg); return false; }
      return true;
    }
  };
  struct In { float l, z0, z1; };
  static bool sync_ok(const void* p) { return p != nullptr; }
  static void launch_rows(const Src& src, int n, int C, int32_t* cls_raw, float* conf_raw, float* sync_raw, hipStream_t s) {
    hipLaunchKernelGGL(track_gated_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src.lg, src.ldl, src.gz, src.ldg, n, C, cls_raw, conf_raw, sync_raw);
  }
  static void launch_viterbi(const Src& src, int W, int C, float lam, float mu, int32_t* cls_path, int32_t* sync_path, uint8_t* backptr, hipStream_t s);
  static void launch_pairwise(const Src& src, const float* ws, int W, int C, float lam, float mu, float* p_change, float* jump_abs, float* p_flip, int32_t* top_from,
                              int32_t* top_to, float* p_top, float* xi, hipStream_t s);

  float log_c;
  bool loads;                                                      // the lanes of plane 1 carry the offset logits
  __device__ __forceinline__ TrackChainGated(int C, int lane = threadIdx.x) : TrackGatedLane(C, lane), log_c(logf((float)C)), loads(live && m) {}
  __device__ __forceinline__ In load(const Src& row, bool have) const {
    return In{(loads && have) ? row.lg[c] : -INFINITY, have ? row.gz[0] : 0.f, have ? row.gz[1] : 0.f};
  }
  template <class Rows>
  __device__ __forceinline__ In load_row(const Rows& rows, int64_t r) const {
    const float* gz = rows.gate(r);
    return In{loads ? rows.logits(r)[c] : -INFINITY, gz[0], gz[1]};
  }
  __device__ __forceinline__ float emission(const In& in) const { return track_gated_emission(*this, in.l, in.z0, in.z1, log_c); }
  __device__ __forceinline__ float first_viterbi(const In&, float e) const { return e - wave_max(e); }      // S_0 = E[0]
  __device__ __forceinline__ float viterbi_step(const float* s_u, int C, float lam, float mu, const In&, float e, int& bp) const {
    return track_gated_viterbi_step(*this, s_u, C, lam, mu, e, bp);
  }
  __device__ __forceinline__ float fb_step(const float* s_u, int C4, bool back, float lam, float mu, float e, float& mx) const {
    return track_gated_fb_step(*this, s_u, C4, back, lam, mu, e, mx);
  }
  __device__ __forceinline__ void put(float* s_u, bool fwd, float v) const {
    if (live) s_u[fwd ? m * 32 + c : j] = v;
  }
  __device__ __forceinline__ static int put_state(int state, int C, int32_t* cls, int32_t* sync, int64_t i) {
    cls[i] = state % C;
    sync[i] = state / C;
    return state % C;
  }
  __device__ __forceinline__ static void combine(const float* a, const float* b, int C, const float* __restrict__ grid, const TrackStreamOut& out, int i) {
    int best;
    float pbest, mean, ps;
    track_gated_combine_row(a, b, C, grid, out.post_lag + (int64_t)i * out.ldp, best, pbest, mean, ps);
    out.p_sync_lag[i] = ps;
    out.cls_post_lag[i] = best;
    out.conf_post_lag[i] = pbest;
    out.offset_mean_lag[i] = mean;
  }
  __device__ __forceinline__ static void keep_inputs(const Src& row, float* lg_slot, float* gz_slot, int c, int C) {
    if (c < C) lg_slot[c] = row.lg[c];
    if (c < 2) gz_slot[c] = row.gz[c];
  }
};

// Follows the back pointers of rows R .. w + 1 from state `cur` (the state at row R) -> the state at row w.  Lane c loads backptr[r, c] of eight rows at a time, the
// chain itself is eight wave-uniform shuffles.  rows: .width() the entries of one row of back pointers (the gated chain: 2C states; every index read is clamped below
// it), .backptr(r) row r of them.  sink(r, state) is called by the whole wavefront for every r in [w, R], in descending r: what to do with the state at row r.
template <class Rows, class Sink>
__device__ __forceinline__ int track_backtrace(const Rows& rows, int64_t R, int64_t w, int cur, int c, bool live, const Sink& sink) {
  const int S = rows.width();
  for (int64_t r0 = R; r0 > w; r0 -= 8) {
    int b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = (live && r0 - j > w) ? (int)rows.backptr(r0 - j)[c] : 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (r0 - j > w) {                                            // wave-uniform
        sink(r0 - j, cur);
        const int p = __shfl(b[j], cur, 64);
        cur = p < S ? p : S - 1;
      }
    }
  }
  sink(w, cur);
  return cur;
}

// ---- the read-outs of a whole recording (sf_track_decode, sf_track_posterior, sf_track_pairwise and their _gated forms) ----------------

// The back pointers of a recording: row r of S bytes.
struct TrackPathRows {
  const uint8_t* bp;  int S;
  __device__ __forceinline__ int width() const { return S; }
  __device__ __forceinline__ const uint8_t* backptr(int64_t r) const { return bp + r * S; }
};

// One wavefront, lane j = state j of the chain; lanes beyond the chain's states run along with -inf scores so that every cross-lane operation sees a full EXEC mask.
//   s_0 = E[0];   s_w[j] = max_j' (s_{w-1}[j'] + T(j', j)) + E[w, j]   (the lowest predecessor on ties -> backptr[w, j], one byte);   s_w -= max_j s_w[j]
// (the renormalisation bounds the scores for any W).  T = -lam |p - c|, and -mu [m' != m] between the planes of the gated chain.  Inside a plane the lowest p wins
// (strict `>` in ascending p); between the planes m' = 0 wins: a lane of plane 0 takes the other plane's candidate only when it is strictly larger, a lane of plane 1
// also when it is equal.  (The partner picks its p BEFORE mu is subtracted, a scan over all 2C predecessors would pick after: the two differ only where fp32 rounds two
// different candidates of the other plane to one value by subtracting mu - the partner then keeps the truly larger one.  With exact arithmetic, e.g. dyadic inputs,
// they are the same rule.)  The end state is the lowest state whose score is the maximum, 0 after the renormalisation; the backtrace follows backptr from there (the
// barriers of the scan order this wave's backptr stores before its loads) and the chain writes the path: cls_path alone, or cls_path = j % C and sync_path = j / C.
// Non-finite logits give NaN scores: a NaN never wins a comparison, so the predecessor stays 0, and the backtrace clamps what it reads: every byte and every index
// written lies in [0, S) / [0, C) / {0, 1}.
template <class Chain>
__global__ __launch_bounds__(64) void track_viterbi_kernel(typename Chain::Src src, int W, int C, float lam, float mu, int32_t* __restrict__ cls_path,
                                                            int32_t* __restrict__ sync_path, uint8_t* __restrict__ backptr) {
  __shared__ float s_u[TRACK_MAX_C];
  const Chain ch(C);
  const unsigned S = Chain::states(C);                             // (unsigned: a row index times S needs no sign word)
  typename Chain::In in = ch.load(src, true);
  typename Chain::In next = ch.load(src.at(1), W > 1);
  float s = ch.first_viterbi(in, Chain::VITERBI_TAKES_EMISSION ? ch.emission(in) : 0.f);
  ch.put(s_u, false, s);
  __syncthreads();
  for (int w = 1; w < W; ++w) {
    in = next;
    if (w + 1 < W) next = ch.load(src.at(w + 1), true);            // the next row's loads travel under this step's scan
    int bp;
    s = ch.viterbi_step(s_u, C, lam, mu, in, Chain::VITERBI_TAKES_EMISSION ? ch.emission(in) : 0.f, bp);
    if (ch.live) backptr[(int64_t)w * S + ch.j] = (uint8_t)bp;
    __syncthreads();                                               // every lane has read s_u
    ch.put(s_u, false, s);
    __syncthreads();
  }
  track_backtrace(TrackPathRows{backptr, (int)S}, W - 1, 0, track_wave_end_state(s, ch.live), ch.j, ch.live,
                  [&](int64_t r, int state) { if (ch.j == 0) Chain::put_state(state, C, cls_path, sync_path, r); });
}

// The plain chain does NOT run the template above: it keeps this kernel, which is the template written out for it by hand, with loose pointers for arguments, a
// serial scan of LDS for the end state and a backtrace of its own over 32-bit row indices.  The template's plain instantiation gives the same bytes and measured 1.7 %
// slower over 4096 rows (2.1 % before a no-op moved its scan loop, which had landed 4 bytes early, back); the cause of the rest was not found - an int row index in
// the shared backtrace made it worse - so the piece stays doubled (profiles/track_offline_refactor.md).  s_prev is what the template calls s_u.
__global__ __launch_bounds__(64) void track_viterbi_plain_kernel(const float* __restrict__ logits, int64_t ldl, int W, int C, float lam, int32_t* __restrict__ cls_path,
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

void TrackChainPlain::launch_viterbi(const Src& src, int W, int C, float lam, float, int32_t* cls_path, int32_t*, uint8_t* backptr, hipStream_t s) {
  hipLaunchKernelGGL(track_viterbi_plain_kernel, dim3(1), dim3(64), 0, s, src.lg, src.ldl, W, C, lam, cls_path, backptr);
}
void TrackChainGated::launch_viterbi(const Src& src, int W, int C, float lam, float mu, int32_t* cls_path, int32_t* sync_path, uint8_t* backptr, hipStream_t s) {
  hipLaunchKernelGGL(track_viterbi_kernel<TrackChainGated>, dim3(1), dim3(64), 0, s, src, W, C, lam, mu, cls_path, sync_path, backptr);
}

// Block 0, the forward scan over rows 0 .. W-1:   a_0 = E[0];        a_w[j] = E[w, j] + lse_j' (a_{w-1}[j'] + T(j', j));
// block 1, the backward scan over rows W-1 .. 0:  b_{W-1} = 0;       b_w[j] = lse_n (b_{w+1}[n] + E[w+1, n] + T(j, n)).
// One wavefront each, lane j = state j, the vector the transition reads (a_{w-1}, or b_{w+1} + E[w+1]) in LDS as the chain lays it out (contiguous; the gated chain:
// two planes of 32 floats over a -inf fill, so fb_transition_lse's float4 reads stay aligned and add +0), the next row's loads under the current step.
// After every step the vector's maximum is subtracted (scores stay within [-(lam (C - 1) + row range), 0] for any W: a per-row constant cancels in post)
// and, in the forward block, added to a double: log_z = the subtracted maxima + lse of the last, normalised a.  ws = a (W, S) then b (W, S), fp32, state-major rows.
template <class Chain>
__global__ __launch_bounds__(64) void track_fb_scan_kernel(typename Chain::Src src, int W, int C, float lam, float mu, float* __restrict__ ws,
                                                            float* __restrict__ log_z) {
  __shared__ __attribute__((aligned(16))) float s_u[TRACK_MAX_C];
  const Chain ch(C);
  const unsigned S = Chain::states(C);
  const bool back = blockIdx.x == 1;                              // wave-uniform
  const int C4 = (C + 3) & ~3;
  const float ninf = -INFINITY;
  float* out = ws + (back ? (int64_t)W * S : 0);
  const int64_t row0 = back ? W - 1 : 0, step = back ? -1 : 1;     // scan position k reads row row0 + step * k
  double shifted = 0.0;

  if (Chain::LDS_PREFILL) {
    s_u[threadIdx.x] = ninf;
    __syncthreads();
  }
  float e = ch.emission(ch.load(src.at(row0), true));
  float v = back ? (ch.live ? 0.f : ninf) : e;
  float m = fb_finite_or_zero(wave_max(v));
  v -= m;
  shifted += (double)m;
  if (ch.live) out[row0 * S + ch.j] = v;
  ch.put(s_u, true, back ? v + e : v);
  __syncthreads();
  typename Chain::In next = ch.load(src.at(row0 + step), W > 1);
  for (int k = 1; k < W; ++k) {
    const int64_t row = row0 + step * k;
    const typename Chain::In in = next;
    if (k + 1 < W) next = ch.load(src.at(row + step), true);
    e = ch.emission(in);
    v = ch.fb_step(s_u, C4, back, lam, mu, e, m);
    shifted += (double)m;
    if (ch.live) out[row * S + ch.j] = v;
    __syncthreads();                                               // every lane has read s_u
    ch.put(s_u, true, back ? v + e : v);
    __syncthreads();
  }
  if (!back) {
    const float z = logf(wave_sum(expf(v)));                       // the normalised a_{W-1}: maximum 0 (idle and masked lanes add exp(-inf) = 0)
    if (ch.j == 0) log_z[0] = (float)(shifted + (double)z);
  }
}

// One thread per window: the chain's combine of a_w + b_w (fb_combine_row / track_gated_combine_row) into entry w of the posterior block.
template <class Chain>
__global__ __launch_bounds__(256) void track_fb_combine_kernel(const float* __restrict__ ws, int W, int C, const float* __restrict__ grid, TrackStreamOut out) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  const unsigned S = Chain::states(C);
  const float* a = ws + (int64_t)w * S;
  Chain::combine(a, a + (int64_t)W * S, C, grid, out, w);
}

// The pairwise kernels are NOT a template on the chain: folded onto chain hooks (a lane's term, which lanes gather) they walk a_w one float per LDS read where these
// read float4s, and the gated one needs a block barrier more to lay a_w out through put(); measured, the folded kernels took 9.7 us where these take 8.4 us (plain)
// and 14.6 us where these take 13.7 us (gated) at W = 173 (profiles/track_offline_refactor.md).  What they share is shared as functions: TrackPairAcc, track_pair_top,
// track_pair_write, the emissions.  One wavefront per boundary, four boundaries per 256-thread block; the lane is the DESTINATION state, a_w lies in the wave's LDS
// slice (entries beyond C hold -inf and add +0) and is read as a broadcast while the lane walks the predecessors: walk 1 the maximum, walk 2 the sums and the lane's
// best off-diagonal pair, walk 3 (only with xi) the stores, lane c writing column c of row p.
__global__ __launch_bounds__(256) void track_pairwise_kernel(const float* __restrict__ logits, int64_t ldl, const float* __restrict__ ws, int W, int C, float lam,
                                                             float* __restrict__ p_change, float* __restrict__ jump_abs, int32_t* __restrict__ top_from,
                                                             int32_t* __restrict__ top_to, float* __restrict__ p_top, float* __restrict__ xi) {
  __shared__ __attribute__((aligned(16))) float s_a[4][TRACK_MAX_C];
  const int wv = threadIdx.x >> 6, c = threadIdx.x & 63;
  const int wb = blockIdx.x * 4 + wv;
  const bool active = wb < W - 1;                                  // wave-uniform; an idle wave walks the last boundary again and stores nothing
  const int64_t w = active ? wb : W - 2;
  const bool live = c < C;
  const int C4 = (C + 3) & ~3;
  const float ninf = -INFINITY;
  float* u = s_a[wv];
  u[c] = live ? ws[w * C + c] : ninf;                              // a_w
  const float e = fb_log_softmax(live ? logits[(w + 1) * ldl + c] : ninf);
  const float d = live ? e + ws[((int64_t)W + w + 1) * C + c] : ninf;   // e[w+1, c] + b_{w+1}[c]
  __syncthreads();
  float mx = ninf;
  for (int p = 0; p < C4; p += 4) {
    const float4 v = *reinterpret_cast<const float4*>(u + p);
    mx = fmaxf(mx, v.x - lam * fabsf((float)(p - c)));
    mx = fmaxf(mx, v.y - lam * fabsf((float)(p + 1 - c)));
    mx = fmaxf(mx, v.z - lam * fabsf((float)(p + 2 - c)));
    mx = fmaxf(mx, v.w - lam * fabsf((float)(p + 3 - c)));
  }
  const float sub = fb_finite_or_zero(wave_max(mx + d));
  TrackPairAcc acc(c);
  for (int p = 0; p < C4; p += 4) {
    const float4 v = *reinterpret_cast<const float4*>(u + p);
    acc.add(expf(v.x - lam * fabsf((float)(p - c)) + d - sub), p, c);
    acc.add(expf(v.y - lam * fabsf((float)(p + 1 - c)) + d - sub), p + 1, c);
    acc.add(expf(v.z - lam * fabsf((float)(p + 2 - c)) + d - sub), p + 2, c);
    acc.add(expf(v.w - lam * fabsf((float)(p + 3 - c)) + d - sub), p + 3, c);
  }
  const float z = wave_sum(acc.sum), off = wave_sum(acc.off), jump = wave_sum(acc.jump);
  float best = live ? acc.best : -1.f;
  int bp = acc.bp, bc = c;
  track_pair_top(best, bp, bc);
  if (!active) return;
  if (c == 0) track_pair_write((int)w, z, off, jump, best, bp, bc, p_change, jump_abs, top_from, top_to, p_top);
  if (xi && live) {
    float* out = xi + w * C * C + c;
    for (int p = 0; p < C; ++p) out[(int64_t)p * C] = expf(u[p] - lam * fabsf((float)(p - c)) + d - sub) / z;
  }
}

// The same over the 2C states: lane j = (m, c) is the destination state, a_w lies in LDS as two planes of 32 floats.  The lane walks its own plane and the other plane
// minus mu; y = the two added = the mass of (p, any flag) -> (c, m).  The class pair (p -> c) is y + the partner lane's y (the same bits in both lanes: the sum
// commutes); the lanes of plane 0 gather the class outputs and store xi, every live lane gathers the mass that changes the flag.
__global__ __launch_bounds__(256) void track_pairwise_gated_kernel(const float* __restrict__ logits, int64_t ldl, const float* __restrict__ gate, int64_t ldg,
                                                                   const float* __restrict__ ws, int W, int C, float lam, float mu, float* __restrict__ p_change,
                                                                   float* __restrict__ jump_abs, float* __restrict__ p_flip, int32_t* __restrict__ top_from,
                                                                   int32_t* __restrict__ top_to, float* __restrict__ p_top, float* __restrict__ xi) {
  __shared__ __attribute__((aligned(16))) float s_a[4][64];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wb = blockIdx.x * 4 + wv;
  const bool active = wb < W - 1;                                  // wave-uniform; an idle wave walks the last boundary again and stores nothing
  const int64_t w = active ? wb : W - 2;
  const int S = 2 * C;
  const int C4 = (C + 3) & ~3;
  const float ninf = -INFINITY;
  const TrackGatedLane ln(C, lane);
  const bool live = ln.live;
  const int m = ln.m, c = ln.c, partner = ln.partner;
  float* u = s_a[wv];
  u[lane] = (lane & 31) < C ? ws[w * S + (lane >> 5) * C + (lane & 31)] : ninf;       // a_w: slot (m', p) = m' * 32 + p
  const float em = track_gated_emission(ln, (live && m) ? logits[(w + 1) * ldl + c] : ninf, gate[(w + 1) * ldg], gate[(w + 1) * ldg + 1], logf((float)C));
  const float d = live ? em + ws[((int64_t)W + w + 1) * S + lane] : ninf;               // E[w+1, j] + b_{w+1}[j]
  __syncthreads();
  const float* own = u + m * 32;
  const float* oth = u + (1 - m) * 32;
  float mx = ninf;
  for (int p = 0; p < C4; p += 4) {
    const float4 v = *reinterpret_cast<const float4*>(own + p), o = *reinterpret_cast<const float4*>(oth + p);
    mx = fmaxf(mx, fmaxf(v.x, o.x - mu) - lam * fabsf((float)(p - c)));
    mx = fmaxf(mx, fmaxf(v.y, o.y - mu) - lam * fabsf((float)(p + 1 - c)));
    mx = fmaxf(mx, fmaxf(v.z, o.z - mu) - lam * fabsf((float)(p + 2 - c)));
    mx = fmaxf(mx, fmaxf(v.w, o.w - mu) - lam * fabsf((float)(p + 3 - c)));
  }
  const float sub = fb_finite_or_zero(wave_max(mx + d));
  const bool gathers = live && m == 0;
  TrackPairAcc acc(c);
  float flip = 0.f;
  for (int p = 0; p < C; ++p) {
    const float pen = lam * fabsf((float)(p - c));
    const float x_oth = expf(oth[p] - mu - pen + d - sub);
    const float y = expf(own[p] - pen + d - sub) + x_oth;
    flip += x_oth;
    const float yc = y + __shfl(y, partner, 64);
    if (gathers) acc.add(yc, p, c);
  }
  const float z = wave_sum(acc.sum), off = wave_sum(acc.off), jump = wave_sum(acc.jump), flips = wave_sum(flip);
  float best = gathers ? acc.best : -1.f;
  int bp = acc.bp, bc = c;
  track_pair_top(best, bp, bc);
  if (!active) return;
  if (lane == 0) {
    track_pair_write((int)w, z, off, jump, best, bp, bc, p_change, jump_abs, top_from, top_to, p_top);
    p_flip[w] = flips / z;
  }
  if (xi) {                                                        // wave-uniform: every lane takes part in the shuffle, plane 0 stores
    float* out = xi + w * C * C + c;
    for (int p = 0; p < C; ++p) {
      const float pen = lam * fabsf((float)(p - c));
      const float y = expf(own[p] - pen + d - sub) + expf(oth[p] - mu - pen + d - sub);
      const float yc = y + __shfl(y, partner, 64);
      if (gathers) out[(int64_t)p * C] = yc / z;
    }
  }
}

void TrackChainPlain::launch_pairwise(const Src& src, const float* ws, int W, int C, float lam, float, float* p_change, float* jump_abs, float*, int32_t* top_from,
                                      int32_t* top_to, float* p_top, float* xi, hipStream_t s) {
  hipLaunchKernelGGL(track_pairwise_kernel, dim3((unsigned)((W - 1 + 3) / 4)), dim3(256), 0, s, src.lg, src.ldl, ws, W, C, lam, p_change, jump_abs, top_from, top_to, p_top,
                     xi);
}
void TrackChainGated::launch_pairwise(const Src& src, const float* ws, int W, int C, float lam, float mu, float* p_change, float* jump_abs, float* p_flip,
                                      int32_t* top_from, int32_t* top_to, float* p_top, float* xi, hipStream_t s) {
  hipLaunchKernelGGL(track_pairwise_gated_kernel, dim3((unsigned)((W - 1 + 3) / 4)), dim3(256), 0, s, src.lg, src.ldl, src.gz, src.ldg, ws, W, C, lam, mu, p_change,
                     jump_abs, p_flip, top_from, top_to, p_top, xi);
}

// What every entry of a chain refuses before it looks at a pointer, in two parts: W, C (one lane per state) and the strides; then the costs (the plain entries pass
// mu = 0).  In two parts because the two posterior entries differ in where they check `ldp`: sf_track_posterior between the parts, sf_track_posterior_gated after both.
template <class Chain>
static bool track_shape_ok(const char* who, int W, int C, const typename Chain::Src& src) {
  if (W < 0) { sf_set_error("%s: W = %d windows", who, W); return false; }
  if (C < 2 || C > Chain::MAX_C) { sf_set_error("%s: C = %d classes out of range (2 .. %d: one lane per %s)", who, C, Chain::MAX_C, Chain::LANE_IS); return false; }
  return src.strides_ok(who, C);
}
static bool track_costs_ok(const char* who, float lam, float mu) {
  if (!(std::isfinite(lam) && lam >= 0.f)) { sf_set_error("%s: lam must be finite and >= 0 (the cost of a class change)", who); return false; }
  if (!(std::isfinite(mu) && mu >= 0.f)) { sf_set_error("%s: mu must be finite and >= 0 (the cost of a change of the synchronizable flag)", who); return false; }
  return true;
}
template <class Chain>
static bool track_args_ok(const char* who, int W, int C, const typename Chain::Src& src, float lam, float mu) {
  return track_shape_ok<Chain>(who, W, C, src) && track_costs_ok(who, lam, mu);
}

// Three launches on the caller's stream, all latency-bound (W x S <= W x 64 floats): the chain's rows kernel (cls_raw / conf_raw, sync_raw), the Viterbi scan with
// its backtrace, and track_rows_kernel<true>: the softmax probability of the path's class.
template <class Chain>
static int track_decode_impl(const char* who, const typename Chain::Src& src, int W, int C, float lam, float mu, int32_t* cls_raw, float* conf_raw, float* sync_raw,
                             int32_t* cls_path, int32_t* sync_path, float* conf_path, uint8_t* backptr, void* stream) {
  if (!track_args_ok<Chain>(who, W, C, src, lam, mu)) return -1;
  if (W == 0) return 0;
  SF_CHECK_ARG(src.ok() && cls_raw && conf_raw && Chain::sync_ok(sync_raw) && cls_path && Chain::sync_ok(sync_path) && conf_path && backptr, "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  Chain::launch_rows(src, W, C, cls_raw, conf_raw, sync_raw, s);
  SF_LAUNCH_CHECK_AS(who);
  Chain::launch_viterbi(src, W, C, lam, mu, cls_path, sync_path, backptr, s);
  SF_LAUNCH_CHECK_AS(who);
  hipLaunchKernelGGL(track_rows_kernel<true>, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, s, src.lg, src.ldl, W, C, cls_path, conf_path);
  SF_LAUNCH_CHECK_AS(who);
  return 0;
}

// Two launches: both scans side by side (two workgroups of one wavefront), then one thread per window.  out: the posterior block, entry w = window w.
// ldp_first: whether the entry checks `ldp` before the costs (sf_track_posterior) or after them (sf_track_posterior_gated), as each always did.
template <class Chain>
static int track_posterior_impl(const char* who, const typename Chain::Src& src, int W, int C, float lam, float mu, const float* grid, const TrackStreamOut& out,
                                bool ldp_first, float* log_z, float* workspace, void* stream) {
  if (!track_shape_ok<Chain>(who, W, C, src)) return -1;
  if (ldp_first) SF_CHECK_ARG(out.ldp >= C, "%s: post row stride ldp = %lld below C = %d", who, (long long)out.ldp, C);
  if (!track_costs_ok(who, lam, mu)) return -1;
  SF_CHECK_ARG(out.ldp >= C, "%s: post row stride ldp = %lld below C = %d", who, (long long)out.ldp, C);
  if (W == 0) return 0;
  SF_CHECK_ARG(src.ok() && grid && out.post_lag && Chain::sync_ok(out.p_sync_lag) && out.cls_post_lag && out.conf_post_lag && out.offset_mean_lag && log_z && workspace,
               "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(track_fb_scan_kernel<Chain>, dim3(2), dim3(64), 0, s, src, W, C, lam, mu, workspace, log_z);
  SF_LAUNCH_CHECK_AS(who);
  hipLaunchKernelGGL(track_fb_combine_kernel<Chain>, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, s, (const float*)workspace, W, C, grid, out);
  SF_LAUNCH_CHECK_AS(who);
  return 0;
}

// The scans of the posterior (they leave a, b in the workspace and log_z), then one wavefront per boundary.  A single window has log_z and no boundary.
template <class Chain>
static int track_pairwise_impl(const char* who, const typename Chain::Src& src, int W, int C, float lam, float mu, float* p_change, float* jump_abs, float* p_flip,
                               int32_t* top_from, int32_t* top_to, float* p_top, float* xi, float* log_z, float* workspace, void* stream) {
  if (!track_args_ok<Chain>(who, W, C, src, lam, mu)) return -1;
  if (W == 0) return 0;
  SF_CHECK_ARG(src.ok() && log_z && workspace && (W == 1 || (p_change && jump_abs && Chain::sync_ok(p_flip) && top_from && top_to && p_top)), "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(track_fb_scan_kernel<Chain>, dim3(2), dim3(64), 0, s, src, W, C, lam, mu, workspace, log_z);
  SF_LAUNCH_CHECK_AS(who);
  if (W == 1) return 0;
  Chain::launch_pairwise(src, (const float*)workspace, W, C, lam, mu, p_change, jump_abs, p_flip, top_from, top_to, p_top, xi, s);
  SF_LAUNCH_CHECK_AS(who);
  return 0;
}

extern "C" int sf_track_decode(const float* logits, int64_t ldl, int W, int C, float lam, int32_t* cls_raw, float* conf_raw, int32_t* cls_path, float* conf_path,
                               uint8_t* backptr, void* stream) {
  return track_decode_impl<TrackChainPlain>("sf_track_decode", TrackChainPlain::Src{logits, ldl}, W, C, lam, 0.f, cls_raw, conf_raw, nullptr, cls_path, nullptr,
                                            conf_path, backptr, stream);
}

extern "C" int sf_track_decode_gated(const float* logits, int64_t ldl, const float* gate_logits, int64_t ldg, int W, int C, float lam, float mu, int32_t* cls_raw,
                                     float* conf_raw, float* sync_raw, int32_t* cls_path, int32_t* sync_path, float* conf_path, uint8_t* backptr, void* stream) {
  return track_decode_impl<TrackChainGated>("sf_track_decode_gated", TrackChainGated::Src{logits, ldl, gate_logits, ldg}, W, C, lam, mu, cls_raw, conf_raw, sync_raw,
                                            cls_path, sync_path, conf_path, backptr, stream);
}

extern "C" int sf_track_posterior(const float* logits, int64_t ldl, int W, int C, float lam, const float* grid, float* post, int64_t ldp, int32_t* cls_post,
                                  float* conf_post, float* offset_mean, float* log_z, float* workspace, void* stream) {
  const TrackStreamOut out{nullptr, nullptr, nullptr, post, ldp, nullptr, cls_post, conf_post, offset_mean, nullptr, nullptr, nullptr};
  return track_posterior_impl<TrackChainPlain>("sf_track_posterior", TrackChainPlain::Src{logits, ldl}, W, C, lam, 0.f, grid, out, true, log_z, workspace, stream);
}

extern "C" int sf_track_posterior_gated(const float* logits, int64_t ldl, const float* gate_logits, int64_t ldg, int W, int C, float lam, float mu, const float* grid,
                                        float* post, int64_t ldp, float* p_sync, int32_t* cls_post, float* conf_post, float* offset_mean, float* log_z,
                                        float* workspace, void* stream) {
  const TrackStreamOut out{nullptr, nullptr, nullptr, post, ldp, p_sync, cls_post, conf_post, offset_mean, nullptr, nullptr, nullptr};
  return track_posterior_impl<TrackChainGated>("sf_track_posterior_gated", TrackChainGated::Src{logits, ldl, gate_logits, ldg}, W, C, lam, mu, grid, out, false,
                                               log_z, workspace, stream);
}

extern "C" int sf_track_pairwise(const float* logits, int64_t ldl, int W, int C, float lam, float* p_change, float* jump_abs, int32_t* top_from, int32_t* top_to,
                                 float* p_top, float* xi, float* log_z, float* workspace, void* stream) {
  return track_pairwise_impl<TrackChainPlain>("sf_track_pairwise", TrackChainPlain::Src{logits, ldl}, W, C, lam, 0.f, p_change, jump_abs, nullptr, top_from, top_to,
                                              p_top, xi, log_z, workspace, stream);
}

extern "C" int sf_track_pairwise_gated(const float* logits, int64_t ldl, const float* gate_logits, int64_t ldg, int W, int C, float lam, float mu, float* p_change,
                                       float* jump_abs, float* p_flip, int32_t* top_from, int32_t* top_to, float* p_top, float* xi, float* log_z, float* workspace,
                                       void* stream) {
  return track_pairwise_impl<TrackChainGated>("sf_track_pairwise_gated", TrackChainGated::Src{logits, ldl, gate_logits, ldg}, W, C, lam, mu, p_change, jump_abs, p_flip,
                                              top_from, top_to, p_top, xi, log_z, workspace, stream);
}

// ---- fixed-lag read-out of live feeds (sf_track_stream_push, sf_track_pool_push and their _gated forms) --------------------------------
// Rows arrive in pushes; window w is committed by the push that delivers row w + lag, as path_{w+lag}[w] / post_{w+lag}[w] (the offline read-outs of the prefix
// 0 .. w + lag: sf_track_decode / sf_track_posterior, or their gated forms), and never revised.  Both scans are causal, so what a push needs of the past is the scan
// vectors after the last row (s; with the posterior a and the double of subtracted maxima) and, of the last `lag` rows, the back pointers, the inputs (conf_lag, and
// the backward recursion's emission, which is recomputed from them as the offline scan does: no emission ring) and - posterior - the normalised a.  The state buffer
// holds exactly that, the per-row parts as rings (row r in slot r % lag); its size does not depend on how many rows have passed.  A push of n rows is three or four
// launches on the caller's stream:
//   1. the chain's rows kernel:      cls_raw / conf_raw (/ sync_raw) of the new rows (the offline kernel);
//   2. track_stream_scan_kernel:     one wavefront per scan, side by side (block 0 Viterbi, block 1 forward): loads the carried vector, runs the n rows with the next
//                                    row's loads under the current step, writes back pointers / a and every row's end state (argmax s_r) into the push's workspace,
//                                    stores the carried vectors;
//   3. track_stream_readout_kernel:  one wavefront per window that becomes committed: its own backtrace from the end state of row w + lag (eight rows of back
//                                    pointers per round, wave-uniform shuffles), with the posterior its own backward recursion over rows w + lag .. w + 1 and the
//                                    combine of row w; one more wavefront backtraces the tail from the last row.  The windows are independent: a catch-up push of
//                                    1000 rows spreads over the chip instead of running n * lag dependent steps in one wavefront;
//   4. track_stream_keep_kernel:     copies the last min(lag, n) new rows into the rings (after 3, which still reads the slots they replace).
// All of it is templated on a chain (above), as the whole-recording kernels are, and runs a row through the same hooks in the same order as they do.

// the state buffer: [double shifted][int32 end_last, pad][s: 64 floats][posterior: a: 64 floats][offset logits ring (lag, C) fp32][gated: gate logits ring (lag, 2) fp32]
//   [posterior: a ring (lag, S) fp32][back pointer ring (lag, S) bytes], rounded up to 16 bytes; S = the chain's states.  Row r of the stream lies in slot r % lag of
//   every ring.
template <class Chain>
struct TrackStreamLayout {
  int64_t s, a, lg_ring, gz_ring, a_ring, bp_ring, total;
  __host__ __device__ TrackStreamLayout(int C, int lag, bool posterior) {
    const int64_t S = Chain::states(C);
    s = 16;
    a = s + TRACK_MAX_C * 4;
    lg_ring = a + (posterior ? TRACK_MAX_C * 4 : 0);
    gz_ring = lg_ring + (int64_t)lag * C * 4;
    a_ring = gz_ring + (int64_t)lag * Chain::GATE_WIDTH * 4;
    bp_ring = a_ring + (posterior ? (int64_t)lag * S * 4 : 0);
    total = (bp_ring + (int64_t)lag * S + 15) & ~(int64_t)15;
  }
};
using TrackGatedStreamLayout = TrackStreamLayout<TrackChainGated>;      // (the name the header's description of the gated state uses)

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

// the workspace of a push of total_rows rows of S states: [posterior: a (total_rows, S) fp32][end (total_rows) int32][back pointers (total_rows, S) bytes]; in a pool
// push stream e's part starts at its row0
struct TrackPoolWorkspace {
  float* a;  int32_t* end;  uint8_t* bp;
  __host__ __device__ TrackPoolWorkspace(unsigned char* ws, int S, int total_rows, bool posterior) {
    a = reinterpret_cast<float*>(ws);
    end = reinterpret_cast<int32_t*>(ws + (posterior ? (int64_t)total_rows * S * 4 : 0));
    bp = reinterpret_cast<uint8_t*>(end + total_rows);
  }
  __host__ __device__ TrackPoolWorkspace at(int64_t row0, int S) const {
    TrackPoolWorkspace w = *this;
    w.a += row0 * S;  w.end += row0;  w.bp += row0 * S;
    return w;
  }
};
static int64_t track_workspace_bytes(int S, int n, int posterior) {
  return ((posterior ? (int64_t)n * S * 4 : 0) + (int64_t)n * 4 + (int64_t)n * S + 15) & ~(int64_t)15;      // at most 2^20 * 324
}

// Rows before the push live in the rings of the state, rows of the push in the caller's inputs and the workspace: TrackStreamRows resolves a row index to either.
template <class Chain>
struct TrackStreamRows {
  typename Chain::Src src;                // the push's inputs
  const uint8_t* bp_new;                  // workspace: back pointers (n, S)
  const float* a_new;                     // workspace: normalised a (n, S); posterior only
  const int32_t* end_new;                 // workspace: the end state (argmax s_r) per new row
  const float* lg_ring;  const float* gz_ring;       // state: the rings of the inputs, (lag, C) and - gated - (lag, 2)
  const uint8_t* bp_ring;  const float* a_ring;      // state: (lag, S) each
  const int32_t* end_last;                // state: the end state of the last row pushed
  int64_t t_old;                          // rows before this push
  int lag, C;
  __device__ __forceinline__ int width() const { return Chain::states(C); }
  __device__ __forceinline__ const float* logits(int64_t r) const { return r >= t_old ? src.lg + (r - t_old) * src.ldl : lg_ring + (r % lag) * C; }
  __device__ __forceinline__ const float* gate(int64_t r) const { return r >= t_old ? src.gz + (r - t_old) * src.ldg : gz_ring + (r % lag) * 2; }      // (gated only)
  __device__ __forceinline__ const uint8_t* backptr(int64_t r) const { return r >= t_old ? bp_new + (r - t_old) * width() : bp_ring + (r % lag) * width(); }
  __device__ __forceinline__ const float* a(int64_t r) const { return r >= t_old ? a_new + (r - t_old) * width() : a_ring + (r % lag) * width(); }
  __device__ __forceinline__ int end(int64_t r) const { return r >= t_old ? end_new[r - t_old] : end_last[0]; }
};

// One stream's view of its rows: the rings of its state and its part of the push (host and device: the single-stream launcher and the pool's kernels build it).
template <class Chain>
__host__ __device__ __forceinline__ TrackStreamRows<Chain> track_stream_rows(const unsigned char* st, const typename Chain::Src& src, const TrackPoolWorkspace& ws,
                                                                             int64_t t_old, int lag, int C, bool posterior) {
  const TrackStreamLayout<Chain> lay(C, lag, posterior);
  TrackStreamRows<Chain> rows;
  rows.src = src;  rows.bp_new = ws.bp;  rows.a_new = ws.a;  rows.end_new = ws.end;
  rows.lg_ring = reinterpret_cast<const float*>(st + lay.lg_ring);  rows.gz_ring = reinterpret_cast<const float*>(st + lay.gz_ring);
  rows.bp_ring = st + lay.bp_ring;  rows.a_ring = reinterpret_cast<const float*>(st + lay.a_ring);
  rows.end_last = reinterpret_cast<const int32_t*>(st + 8);
  rows.t_old = t_old;  rows.lag = lag;  rows.C = C;
  return rows;
}

// The scan of one stream's push, by one wavefront: fwd = false the Viterbi scan, fwd = true the forward scan (wave-uniform).  s_u: TRACK_MAX_C floats of LDS, 16-byte
// aligned, laid out as the chain's offline kernels keep them.  The single-stream kernel and the pool's kernel both run this body: one stream's arithmetic is the same
// in either.
template <class Chain>
__device__ __forceinline__ void track_stream_scan_body(const typename Chain::Src& src, int n, int C, float lam, float mu, int64_t t_old,
                                                       unsigned char* __restrict__ state, int lag, int posterior, uint8_t* __restrict__ bp_new,
                                                       float* __restrict__ a_new, int32_t* __restrict__ end_new, float* __restrict__ log_z, bool fwd, float* s_u) {
  const TrackStreamLayout<Chain> lay(C, lag, posterior != 0);
  const Chain ch(C);
  const unsigned S = Chain::states(C);                             // (unsigned: a row index times S needs no sign word)
  const int C4 = (C + 3) & ~3;
  const float ninf = -INFINITY;
  float* carried = reinterpret_cast<float*>(state + (fwd ? lay.a : lay.s));
  double* st_shifted = reinterpret_cast<double*>(state);
  int32_t* st_end = reinterpret_cast<int32_t*>(state + 8);
  double shifted = (fwd && t_old > 0) ? st_shifted[0] : 0.0;
  float v = (t_old > 0 && ch.live) ? carried[ch.j] : ninf;
  int k = 0;
  typename Chain::In next = ch.load(src, n > 0);
  if (Chain::LDS_PREFILL) {
    s_u[threadIdx.x] = ninf;
    __syncthreads();
  }
  if (t_old == 0 && n > 0) {                                       // the first row of the stream: s_0 / a_0 = the emission of row 0, as the offline scans begin
    const typename Chain::In in = next;
    if (n > 1) next = ch.load(src.at(1), true);
    const float e = (Chain::VITERBI_TAKES_EMISSION || fwd) ? ch.emission(in) : 0.f;
    if (fwd) {
      v = e;
      const float m = fb_finite_or_zero(wave_max(v));
      v -= m;
      shifted += (double)m;
      if (ch.live) a_new[ch.j] = v;
    } else {
      v = ch.first_viterbi(in, e);
      if (ch.live) bp_new[ch.j] = 0;                               // never followed: the backtrace stops at row 1
      const int end = track_wave_end_state(v, ch.live);            // (the ballot needs the whole wavefront)
      if (ch.j == 0) end_new[0] = end;
    }
    k = 1;
  }
  ch.put(s_u, fwd, v);
  __syncthreads();
  // One 4-byte no-op, executed once per push.  The loop below is one wavefront running n dependent steps, and its time depends on where its 8-byte instructions lie
  // against an 8-byte boundary: with the loop heads 4 bytes off, the plain scan of 1000 rows measured 1143 us against 1112 us (kernel trace, MI355X).  The kernel
  // arguments are loaded by 20 bytes less code than before the kernels became templates; this puts the loops of all four scan kernels back where they lay
  // (profiles/track_refactor.md has the loop heads' offsets and the times).  Whoever changes the code in front of the loop checks the offsets again.
  asm volatile("s_nop 0");
  for (; k < n; ++k) {
    const typename Chain::In in = next;
    if (k + 1 < n) next = ch.load(src.at(k + 1), true);            // the next row's loads travel under this step
    const float e = (Chain::VITERBI_TAKES_EMISSION || fwd) ? ch.emission(in) : 0.f;
    if (fwd) {
      float m;
      v = ch.fb_step(s_u, C4, false, lam, mu, e, m);
      shifted += (double)m;
      if (ch.live) a_new[(int64_t)k * S + ch.j] = v;
    } else {
      int bp;
      v = ch.viterbi_step(s_u, C, lam, mu, in, e, bp);
      if (ch.live) bp_new[(int64_t)k * S + ch.j] = (uint8_t)bp;
      const int end = track_wave_end_state(v, ch.live);
      if (ch.j == 0) end_new[k] = end;
    }
    __syncthreads();                                               // every lane has read s_u
    ch.put(s_u, fwd, v);
    __syncthreads();
  }
  if (n > 0) {
    const int end = track_wave_end_state(v, ch.live);
    if (ch.live) carried[ch.j] = v;
    if (ch.j == 0) {
      if (fwd) st_shifted[0] = shifted;
      else st_end[0] = end;
    }
  }
  if (fwd) {
    const float z = logf(wave_sum(expf(v)));                       // the normalised a of the last row: maximum 0
    if (ch.j == 0) log_z[0] = (float)(shifted + (double)z);
  }
}

template <class Chain>
__global__ __launch_bounds__(64) void track_stream_scan_kernel(typename Chain::Src src, int n, int C, float lam, float mu, int64_t t_old,
                                                                unsigned char* __restrict__ state, int lag, int posterior, uint8_t* __restrict__ bp_new,
                                                                float* __restrict__ a_new, int32_t* __restrict__ end_new, float* __restrict__ log_z) {
  __shared__ __attribute__((aligned(16))) float s_u[TRACK_MAX_C];
  track_stream_scan_body<Chain>(src, n, C, lam, mu, t_old, state, lag, posterior, bp_new, a_new, end_new, log_z, blockIdx.x == 1, s_u);      // block 1: the forward scan
}

// Block i < n_commit: window w = w0 + i, read from the prefix that ends at row R = min(w + lag, t_last).  Block n_commit (if n_tail > 0): the tail, the path of the
// whole prefix on the last n_tail rows.  The backtrace runs over rows of S back pointers (every index read clamped below S); the state it arrives at is written by the
// chain (cls alone, or cls = j % C and sync = j / C).
// bx = the block's index among the stream's n_commit + (n_tail > 0) blocks; s_u (16-byte aligned) / s_b: TRACK_MAX_C floats of LDS each, s_tail: 256 ints.
template <class Chain, bool POST>
__device__ __forceinline__ void track_stream_readout_body(const TrackStreamRows<Chain>& rows, float lam, float mu, const float* __restrict__ grid, int64_t w0,
                                                          int n_commit, int n_tail, int64_t t_last, const TrackStreamOut& out, int bx, float* s_u, float* s_b,
                                                          int* s_tail) {
  const int C = rows.C, S = Chain::states(C);
  const Chain ch(C);
  if (bx == n_commit) {                                            // the tail
    const int64_t w = t_last - (n_tail - 1);
    int cur = rows.end(t_last);
    cur = cur < 0 ? 0 : (cur >= S ? S - 1 : cur);
    track_backtrace(rows, t_last, w, cur, ch.j, ch.live, [&](int64_t r, int state) { if (ch.j == 0) s_tail[r - w] = state; });
    __syncthreads();
    for (int i = threadIdx.x; i < n_tail; i += 64) {
      const float* row = rows.logits(w + i);
      int best;
      float m, sum;
      track_row_stats(row, C, best, m, sum);
      const int cls = Chain::put_state(s_tail[i], C, out.cls_tail, out.sync_tail, i);
      out.conf_tail[i] = track_row_conf(row, C, cls, m, sum);
    }
    return;
  }
  const int i = bx;
  const int64_t w = w0 + i;
  const int64_t R = w + rows.lag < t_last ? w + rows.lag : t_last;
  int cur = rows.end(R);
  cur = cur < 0 ? 0 : (cur >= S ? S - 1 : cur);
  cur = track_backtrace(rows, R, w, cur, ch.j, ch.live, [](int64_t, int) {});
  if (ch.j == 0) {
    const float* row = rows.logits(w);
    int best;
    float m, sum;
    track_row_stats(row, C, best, m, sum);
    const int cls = Chain::put_state(cur, C, out.cls_lag, out.sync_lag, i);
    out.conf_lag[i] = track_row_conf(row, C, cls, m, sum);
  }
  if (POST) {
    // the backward scan of the prefix 0 .. R, from its end down to row w:  b_R = 0;  b_r[j] = lse_n (b_{r+1}[n] + E[r+1, n] + T(j, n)), renormalised per step
    const int C4 = (C + 3) & ~3;
    const float ninf = -INFINITY;
    if (Chain::LDS_PREFILL) s_u[threadIdx.x] = ninf;               // (ordered before the lanes' stores by the loop's first barrier)
    float v = ch.live ? 0.f : ninf;
    typename Chain::In next = ch.load_row(rows, R);
    for (int64_t r = R; r > w; --r) {                              // b_{r-1} from b_r and row r
      const typename Chain::In in = next;
      if (r - 1 > w) next = ch.load_row(rows, r - 1);
      const float e = ch.emission(in);
      __syncthreads();                                             // every lane has read s_u
      ch.put(s_u, true, v + e);
      __syncthreads();
      float m;
      v = ch.fb_step(s_u, C4, true, lam, mu, 0.f, m);
    }
    if (ch.live) s_b[ch.j] = v;                                    // (the combine reads the S live entries only)
    __syncthreads();
    if (ch.j == 0) Chain::combine(rows.a(w), s_b, C, grid, out, i);
  }
}

template <class Chain, bool POST>
__global__ __launch_bounds__(64) void track_stream_readout_kernel(TrackStreamRows<Chain> rows, float lam, float mu, const float* __restrict__ grid, int64_t w0,
                                                                   int n_commit, int n_tail, int64_t t_last, TrackStreamOut out) {
  __shared__ __attribute__((aligned(16))) float s_u[TRACK_MAX_C];
  __shared__ float s_b[TRACK_MAX_C];
  __shared__ int s_tail[256];
  track_stream_readout_body<Chain, POST>(rows, lam, mu, grid, w0, n_commit, n_tail, t_last, out, (int)blockIdx.x, s_u, s_b, s_tail);
}

// Ring row j of a push: new row k = k0 + j (row t_old + k of the stream) into slot (t_old + k) % lag of the rings: the row's inputs (what the chain keeps of them), S
// back pointers and (posterior) S entries of a, one lane per entry.
template <class Chain>
__device__ __forceinline__ void track_stream_keep_body(const typename Chain::Src& src, const uint8_t* __restrict__ bp_new, const float* __restrict__ a_new, int k0,
                                                       int64_t t_old, int C, int lag, int posterior, unsigned char* __restrict__ state, int j) {
  const TrackStreamLayout<Chain> lay(C, lag, posterior != 0);
  const int c = threadIdx.x;
  const int S = Chain::states(C);
  if (c >= S) return;
  const int64_t k = k0 + (int64_t)j;
  const int64_t ring = (t_old + k) % lag;
  Chain::keep_inputs(src.at(k), reinterpret_cast<float*>(state + lay.lg_ring) + ring * C, reinterpret_cast<float*>(state + lay.gz_ring) + ring * Chain::GATE_WIDTH, c, C);
  (state + lay.bp_ring)[ring * S + c] = bp_new[k * S + c];
  if (posterior) reinterpret_cast<float*>(state + lay.a_ring)[ring * S + c] = a_new[k * S + c];
}

// Block j: ring row j.
template <class Chain>
__global__ __launch_bounds__(64) void track_stream_keep_kernel(typename Chain::Src src, const uint8_t* __restrict__ bp_new, const float* __restrict__ a_new, int k0,
                                                                int64_t t_old, int C, int lag, int posterior, unsigned char* __restrict__ state) {
  track_stream_keep_body<Chain>(src, bp_new, a_new, k0, t_old, C, lag, posterior, state, (int)blockIdx.x);
}

static bool track_stream_shape_ok(const char* who, int C, int lag) {
  if (C < 2 || C > TRACK_MAX_C) { sf_set_error("%s: C = %d classes out of range (2 .. %d: one lane per class)", who, C, TRACK_MAX_C); return false; }
  if (lag < 0 || lag > 255) { sf_set_error("%s: lag = %d windows out of range (0 .. 255)", who, lag); return false; }
  return true;
}

// What sf_track_stream_push and the gated chain's track_args_ok refuse, for the two gated launchers: C (2 .. 32), lag, lam, mu and - when there are rows - the strides.
#define TRACK_STREAM_MAX_PUSH (1 << 20)
static bool track_gated_stream_args_ok(const char* who, int C, int lag, int n, int64_t ldl, int64_t ldg, float lam, float mu) {
  if (lag < 0 || lag > 255) { sf_set_error("%s: lag = %d windows out of range (0 .. 255)", who, lag); return false; }
  if (n < 0 || n > TRACK_STREAM_MAX_PUSH) { sf_set_error("%s: n = %d rows in one push (0 .. %d: split a longer catch-up)", who, n, TRACK_STREAM_MAX_PUSH); return false; }
  return track_args_ok<TrackChainGated>(who, n, C, TrackChainGated::Src{nullptr, n ? ldl : (int64_t)C, nullptr, n ? ldg : (int64_t)2}, lam, mu);
}

extern "C" int sf_track_stream_bytes(int C, int lag, int posterior) {
  if (!track_stream_shape_ok("sf_track_stream_bytes", C, lag)) return -1;
  return (int)TrackStreamLayout<TrackChainPlain>(C, lag, posterior != 0).total;      // at most 16 + 512 + 255 * 64 * 9
}

extern "C" int sf_track_stream_gated_bytes(int C, int lag, int posterior) {
  if (!track_gated_stream_args_ok("sf_track_stream_gated_bytes", C, lag, 0, 0, 0, 0.f, 0.f)) return -1;
  return (int)TrackGatedStreamLayout(C, lag, posterior != 0).total;      // at most 16 + 512 + 255 * (32 * 4 + 8 + 64 * 4 + 64)
}

extern "C" int sf_track_stream_workspace_bytes(int C, int n, int posterior) {
  SF_CHECK_ARG(C >= 2 && C <= TRACK_MAX_C, "sf_track_stream_workspace_bytes: C = %d classes out of range (2 .. %d)", C, TRACK_MAX_C);
  SF_CHECK_ARG(n >= 0 && n <= TRACK_STREAM_MAX_PUSH, "sf_track_stream_workspace_bytes: n = %d rows in one push (0 .. %d)", n, TRACK_STREAM_MAX_PUSH);
  return (int)track_workspace_bytes(C, n, posterior);
}

extern "C" int sf_track_stream_gated_workspace_bytes(int C, int n, int posterior) {
  if (!track_gated_stream_args_ok("sf_track_stream_gated_workspace_bytes", C, 0, n, C, 2, 0.f, 0.f)) return -1;
  return (int)track_workspace_bytes(2 * C, n, posterior);
}

// One stream's push, after the entry's own checks of C, lag, n, the strides and the costs: the counts, the null checks and the launches.  `who` names the entry.
template <class Chain>
static int track_stream_push_impl(const char* who, void* state, int C, int lag, int posterior, int64_t rows_done, const typename Chain::Src& src, int n, float lam,
                                  float mu, const float* grid, int final, int32_t* cls_raw, float* conf_raw, float* sync_raw, const TrackStreamOut& out, float* log_z,
                                  void* workspace, void* stream) {
  const int64_t t_old = rows_done, t_new = rows_done + n;
  const int64_t done_old = t_old > lag ? t_old - lag : 0;                                   // windows committed before this push
  const int64_t done_new = final ? t_new : (t_new > lag ? t_new - lag : 0);
  const int64_t n_commit = done_new - done_old, n_tail = t_new - done_new;
  if (t_new == 0) return 0;
  SF_CHECK_ARG(n == 0 || (src.ok() && cls_raw && conf_raw && Chain::sync_ok(sync_raw) && workspace), "%s: null pointer (new rows)", who);
  SF_CHECK_ARG(n_commit == 0 || (out.cls_lag && Chain::sync_ok(out.sync_lag) && out.conf_lag), "%s: null pointer (committed block)", who);
  SF_CHECK_ARG(n_tail == 0 || (out.cls_tail && Chain::sync_ok(out.sync_tail) && out.conf_tail), "%s: null pointer (tail)", who);
  if (posterior) {
    SF_CHECK_ARG(log_z, "%s: null log_z", who);
    SF_CHECK_ARG(n_commit == 0 || (grid && out.post_lag && Chain::sync_ok(out.p_sync_lag) && out.cls_post_lag && out.conf_post_lag && out.offset_mean_lag && out.ldp >= C),
                 "%s: null pointer or post row stride ldp = %lld below C = %d (posterior block)", who, (long long)out.ldp, C);
  }
  hipStream_t s = (hipStream_t)stream;
  unsigned char* st = static_cast<unsigned char*>(state);
  const TrackPoolWorkspace ws(static_cast<unsigned char*>(workspace), Chain::states(C), n, posterior != 0);
  if (n > 0) {
    Chain::launch_rows(src, n, C, cls_raw, conf_raw, sync_raw, s);
    SF_LAUNCH_CHECK_AS(who);
  }
  if (n > 0 || posterior) {                                        // (n == 0 with the posterior: log_z of the prefix so far, from the carried a)
    hipLaunchKernelGGL(track_stream_scan_kernel<Chain>, dim3(posterior ? 2 : 1), dim3(64), 0, s, src, n, C, lam, mu, t_old, st, lag, posterior, ws.bp, ws.a, ws.end, log_z);
    SF_LAUNCH_CHECK_AS(who);
  }
  if (n_commit + n_tail > 0) {
    const TrackStreamRows<Chain> rows = track_stream_rows<Chain>(st, src, ws, t_old, lag, C, posterior != 0);
    const dim3 g((unsigned)(n_commit + (n_tail > 0 ? 1 : 0)));
    if (posterior)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(track_stream_readout_kernel<Chain, true>), g, dim3(64), 0, s, rows, lam, mu, grid, done_old, (int)n_commit, (int)n_tail, t_new - 1,
                         out);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(track_stream_readout_kernel<Chain, false>), g, dim3(64), 0, s, rows, lam, mu, grid, done_old, (int)n_commit, (int)n_tail, t_new - 1,
                         out);
    SF_LAUNCH_CHECK_AS(who);
  }
  const int keep = n < lag ? n : lag;
  if (keep > 0) {
    hipLaunchKernelGGL(track_stream_keep_kernel<Chain>, dim3((unsigned)keep), dim3(64), 0, s, src, (const uint8_t*)ws.bp, (const float*)ws.a, n - keep, t_old, C, lag,
                       posterior, st);
    SF_LAUNCH_CHECK_AS(who);
  }
  return 0;
}

extern "C" int sf_track_stream_push(void* state, int C, int lag, int posterior, int64_t rows_done, const float* logits, int64_t ldl, int n, float lam,
                                    const float* grid, int final, int32_t* cls_raw, float* conf_raw, int32_t* cls_lag, float* conf_lag, float* post_lag, int64_t ldp,
                                    int32_t* cls_post_lag, float* conf_post_lag, float* offset_mean_lag, int32_t* cls_tail, float* conf_tail, float* log_z,
                                    void* workspace, void* stream) {
  const char* who = "sf_track_stream_push";
  if (!track_stream_shape_ok(who, C, lag)) return -1;
  SF_CHECK_ARG(state, "%s: null state", who);
  SF_CHECK_ARG(n >= 0 && n <= TRACK_STREAM_MAX_PUSH, "%s: n = %d rows in one push (0 .. %d: split a longer catch-up)", who, n, TRACK_STREAM_MAX_PUSH);
  SF_CHECK_ARG(rows_done >= 0 && rows_done <= (INT64_MAX >> 1), "%s: %lld rows pushed so far", who, (long long)rows_done);
  SF_CHECK_ARG(std::isfinite(lam) && lam >= 0.f, "%s: lam must be finite and >= 0 (the cost of a class change)", who);
  SF_CHECK_ARG(n == 0 || ldl >= C, "%s: row stride ldl = %lld below C = %d", who, (long long)ldl, C);
  const TrackStreamOut out{cls_lag, nullptr, conf_lag, post_lag, ldp, nullptr, cls_post_lag, conf_post_lag, offset_mean_lag, cls_tail, nullptr, conf_tail};
  return track_stream_push_impl<TrackChainPlain>(who, state, C, lag, posterior, rows_done, TrackChainPlain::Src{logits, ldl}, n, lam, 0.f, grid, final, cls_raw, conf_raw,
                                                 nullptr, out, log_z, workspace, stream);
}

extern "C" int sf_track_stream_push_gated(void* state, int C, int lag, int posterior, int64_t rows_done, const float* logits, int64_t ldl, const float* gate_logits,
                                          int64_t ldg, int n, float lam, float mu, const float* grid, int final, int32_t* cls_raw, float* conf_raw, float* sync_raw,
                                          int32_t* cls_lag, int32_t* sync_lag, float* conf_lag, float* post_lag, int64_t ldp, float* p_sync_lag, int32_t* cls_post_lag,
                                          float* conf_post_lag, float* offset_mean_lag, int32_t* cls_tail, int32_t* sync_tail, float* conf_tail, float* log_z,
                                          void* workspace, void* stream) {
  const char* who = "sf_track_stream_push_gated";
  if (!track_gated_stream_args_ok(who, C, lag, n, ldl, ldg, lam, mu)) return -1;
  SF_CHECK_ARG(state, "%s: null state", who);
  SF_CHECK_ARG(rows_done >= 0 && rows_done <= (INT64_MAX >> 1), "%s: %lld rows pushed so far", who, (long long)rows_done);
  const TrackStreamOut out{cls_lag, sync_lag, conf_lag, post_lag, ldp, p_sync_lag, cls_post_lag, conf_post_lag, offset_mean_lag, cls_tail, sync_tail, conf_tail};
  return track_stream_push_impl<TrackChainGated>(who, state, C, lag, posterior, rows_done, TrackChainGated::Src{logits, ldl, gate_logits, ldg}, n, lam, mu, grid, final,
                                                 cls_raw, conf_raw, sync_raw, out, log_z, workspace, stream);
}

// ---- the same read-out for many streams in one call (sf_track_pool_push, sf_track_pool_push_gated) --------------------------------------------------------------
// n_active streams that share C, lag and posterior, named by a descriptor table of 8 int64 per stream (slot, rows_done, n, row0, final, commit0, tail0, unused): the
// states lie state_stride bytes apart in one buffer, the new rows of all streams in one logits matrix (stream e: rows [row0, row0 + n); its gate rows are the same rows
// of the gate matrix), the committed blocks and the tails back to back in table order.  The same four kinds of launch as one stream's push, each over all streams:
// blockIdx.y = the table row, blockIdx.x = that stream's own work item (its scan / committed window or tail / ring row); the grid's x extent is the largest count in the
// table and a block beyond its stream's count exits at once (a stream brings 0 .. n rows and commits 0 .. k windows: the mapping is ragged, an idle block costs one
// table read).  Every block builds its stream's context from the table's DEVICE copy and runs the single-stream bodies above: one stream's bits do not depend on who
// shares the push.  (TrackPoolEntry and TrackPoolWorkspace, above the bodies, are the table row and the workspace of either kind of push.)

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

// grid (posterior ? 2 : 1, n_active): block (0, e) the Viterbi scan of stream e, block (1, e) its forward scan
template <class Chain>
__global__ __launch_bounds__(64) void track_pool_scan_kernel(const int64_t* __restrict__ table, unsigned char* __restrict__ states, int64_t state_stride,
                                                              typename Chain::Src src, int C, float lam, float mu, int lag, int posterior,
                                                              unsigned char* __restrict__ workspace, int total_rows, float* __restrict__ log_z) {
  __shared__ __attribute__((aligned(16))) float s_u[TRACK_MAX_C];
  const TrackPoolEntry e(table, blockIdx.y, lag);
  const bool fwd = blockIdx.x == 1;
  if (e.t_new == 0 || (e.n == 0 && !fwd)) return;                  // an empty stream; nothing to scan (n == 0 with the posterior: log_z from the carried a)
  const int S = Chain::states(C);
  const TrackPoolWorkspace ws = TrackPoolWorkspace(workspace, S, total_rows, posterior != 0).at(e.row0, S);
  track_stream_scan_body<Chain>(src.at(e.row0), (int)e.n, C, lam, mu, e.t_old, states + e.slot * state_stride, lag, posterior, ws.bp, ws.a, ws.end, log_z + blockIdx.y,
                                fwd, s_u);
}

// grid (the largest n_commit + (n_tail > 0) of the table, n_active)
template <class Chain, bool POST>
__global__ __launch_bounds__(64) void track_pool_readout_kernel(const int64_t* __restrict__ table, const unsigned char* __restrict__ states, int64_t state_stride,
                                                                 typename Chain::Src src, int C, float lam, float mu, int lag, const float* __restrict__ grid,
                                                                 const unsigned char* __restrict__ workspace, int total_rows, TrackStreamOut out) {
  __shared__ __attribute__((aligned(16))) float s_u[TRACK_MAX_C];
  __shared__ float s_b[TRACK_MAX_C];
  __shared__ int s_tail[256];
  const TrackPoolEntry e(table, blockIdx.y, lag);
  if ((int64_t)blockIdx.x >= e.readout_blocks()) return;
  const int S = Chain::states(C);
  const TrackPoolWorkspace ws = TrackPoolWorkspace(const_cast<unsigned char*>(workspace), S, total_rows, POST).at(e.row0, S);
  const TrackStreamRows<Chain> rows = track_stream_rows<Chain>(states + e.slot * state_stride, src.at(e.row0), ws, e.t_old, lag, C, POST);
  track_stream_readout_body<Chain, POST>(rows, lam, mu, grid, e.done_old, (int)e.n_commit, (int)e.n_tail, e.t_new - 1, out.at(e.commit0, e.tail0), (int)blockIdx.x, s_u,
                                         s_b, s_tail);
}

// grid (the largest min(n, lag) of the table, n_active)
template <class Chain>
__global__ __launch_bounds__(64) void track_pool_keep_kernel(const int64_t* __restrict__ table, unsigned char* __restrict__ states, int64_t state_stride,
                                                              typename Chain::Src src, int C, int lag, int posterior, const unsigned char* __restrict__ workspace,
                                                              int total_rows) {
  const TrackPoolEntry e(table, blockIdx.y, lag);
  const int64_t keep = e.keep(lag);
  if ((int64_t)blockIdx.x >= keep) return;
  const int S = Chain::states(C);
  const TrackPoolWorkspace ws = TrackPoolWorkspace(const_cast<unsigned char*>(workspace), S, total_rows, posterior != 0).at(e.row0, S);
  track_stream_keep_body<Chain>(src.at(e.row0), ws.bp, ws.a, (int)(e.n - keep), e.t_old, C, lag, posterior, states + e.slot * state_stride, (int)blockIdx.x);
}

extern "C" int sf_track_pool_workspace_bytes(int C, int total_rows, int posterior) {
  SF_CHECK_ARG(C >= 2 && C <= TRACK_MAX_C, "sf_track_pool_workspace_bytes: C = %d classes out of range (2 .. %d)", C, TRACK_MAX_C);
  SF_CHECK_ARG(total_rows >= 0 && total_rows <= TRACK_STREAM_MAX_PUSH, "sf_track_pool_workspace_bytes: %d rows in one push (0 .. %d)", total_rows, TRACK_STREAM_MAX_PUSH);
  return sf_track_stream_workspace_bytes(C, total_rows, posterior);
}

extern "C" int sf_track_pool_gated_workspace_bytes(int C, int total_rows, int posterior) { return sf_track_stream_gated_workspace_bytes(C, total_rows, posterior); }

// A pool's push, after the entry's own checks of C, lag, total_rows and the costs: the table, the strides, the null checks and the launches.  `who` names the entry.
template <class Chain>
static int track_pool_push_impl(const char* who, void* states, int64_t state_stride, int n_slots, int C, int lag, int posterior, const int64_t* table_host,
                                const int64_t* table_dev, int n_active, const typename Chain::Src& src, int total_rows, float lam, float mu, const float* grid,
                                int32_t* cls_raw, float* conf_raw, float* sync_raw, const TrackStreamOut& out, float* log_z, void* workspace, void* stream) {
  SF_CHECK_ARG(n_active >= 1 && n_active <= TRACK_POOL_MAX_ACTIVE, "%s: n_active = %d streams in one push (1 .. %d)", who, n_active, TRACK_POOL_MAX_ACTIVE);
  SF_CHECK_ARG(n_slots >= 1, "%s: n_slots = %d", who, n_slots);
  SF_CHECK_ARG(states && table_host && table_dev, "%s: null pointer (states or table)", who);
  const TrackStreamLayout<Chain> lay(C, lag, posterior != 0);
  SF_CHECK_ARG(state_stride >= lay.total && state_stride % 16 == 0, "%s: state stride %lld: a multiple of 16, at least %lld bytes", who, (long long)state_stride,
               (long long)lay.total);
  TrackPoolTotals tot;
  if (track_pool_table_check(who, table_host, n_active, n_slots, total_rows, lag, posterior, tot)) return -1;
  if (tot.sum_n > 0 && !src.strides_ok(who, C)) return -1;
  SF_CHECK_ARG(tot.sum_n == 0 || (src.ok() && cls_raw && conf_raw && Chain::sync_ok(sync_raw) && workspace), "%s: null pointer (new rows)", who);
  SF_CHECK_ARG(tot.sum_commit == 0 || (out.cls_lag && Chain::sync_ok(out.sync_lag) && out.conf_lag), "%s: null pointer (committed block)", who);
  SF_CHECK_ARG(tot.sum_tail == 0 || (out.cls_tail && Chain::sync_ok(out.sync_tail) && out.conf_tail), "%s: null pointer (tail)", who);
  if (posterior) {
    SF_CHECK_ARG(!tot.scan || log_z, "%s: null log_z", who);
    SF_CHECK_ARG(tot.sum_commit == 0 || (grid && out.post_lag && Chain::sync_ok(out.p_sync_lag) && out.cls_post_lag && out.conf_post_lag && out.offset_mean_lag && out.ldp >= C),
                 "%s: null pointer or post row stride ldp = %lld below C = %d (posterior block)", who, (long long)out.ldp, C);
  }
  hipStream_t s = (hipStream_t)stream;
  unsigned char* st = static_cast<unsigned char*>(states);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  if (tot.sum_n > 0) {                                             // one thread per row of the packed matrices (rows between two streams' ranges: their own argmax, unread)
    Chain::launch_rows(src, total_rows, C, cls_raw, conf_raw, sync_raw, s);
    SF_LAUNCH_CHECK_AS(who);
  }
  if (tot.scan) {
    hipLaunchKernelGGL(track_pool_scan_kernel<Chain>, dim3(posterior ? 2 : 1, (unsigned)n_active), dim3(64), 0, s, table_dev, st, state_stride, src, C, lam, mu, lag,
                       posterior, ws, total_rows, log_z);
    SF_LAUNCH_CHECK_AS(who);
  }
  if (tot.max_read > 0) {
    const dim3 g((unsigned)tot.max_read, (unsigned)n_active);
    if (posterior)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(track_pool_readout_kernel<Chain, true>), g, dim3(64), 0, s, table_dev, (const unsigned char*)st, state_stride, src, C, lam, mu, lag,
                         grid, (const unsigned char*)ws, total_rows, out);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(track_pool_readout_kernel<Chain, false>), g, dim3(64), 0, s, table_dev, (const unsigned char*)st, state_stride, src, C, lam, mu, lag,
                         grid, (const unsigned char*)ws, total_rows, out);
    SF_LAUNCH_CHECK_AS(who);
  }
  if (tot.max_keep > 0) {
    hipLaunchKernelGGL(track_pool_keep_kernel<Chain>, dim3((unsigned)tot.max_keep, (unsigned)n_active), dim3(64), 0, s, table_dev, st, state_stride, src, C, lag, posterior,
                       (const unsigned char*)ws, total_rows);
    SF_LAUNCH_CHECK_AS(who);
  }
  return 0;
}

extern "C" int sf_track_pool_push(void* states, int64_t state_stride, int n_slots, int C, int lag, int posterior, const int64_t* table_host, const int64_t* table_dev,
                                  int n_active, const float* logits, int64_t ldl, int total_rows, float lam, const float* grid, int32_t* cls_raw, float* conf_raw,
                                  int32_t* cls_lag, float* conf_lag, float* post_lag, int64_t ldp, int32_t* cls_post_lag, float* conf_post_lag,
                                  float* offset_mean_lag, int32_t* cls_tail, float* conf_tail, float* log_z, void* workspace, void* stream) {
  const char* who = "sf_track_pool_push";
  if (!track_stream_shape_ok(who, C, lag)) return -1;
  SF_CHECK_ARG(std::isfinite(lam) && lam >= 0.f, "%s: lam must be finite and >= 0 (the cost of a class change)", who);
  SF_CHECK_ARG(total_rows >= 0 && total_rows <= TRACK_STREAM_MAX_PUSH, "%s: total_rows = %d rows in one push (0 .. %d)", who, total_rows, TRACK_STREAM_MAX_PUSH);
  const TrackStreamOut out{cls_lag, nullptr, conf_lag, post_lag, ldp, nullptr, cls_post_lag, conf_post_lag, offset_mean_lag, cls_tail, nullptr, conf_tail};
  return track_pool_push_impl<TrackChainPlain>(who, states, state_stride, n_slots, C, lag, posterior, table_host, table_dev, n_active, TrackChainPlain::Src{logits, ldl},
                                               total_rows, lam, 0.f, grid, cls_raw, conf_raw, nullptr, out, log_z, workspace, stream);
}

extern "C" int sf_track_pool_push_gated(void* states, int64_t state_stride, int n_slots, int C, int lag, int posterior, const int64_t* table_host,
                                        const int64_t* table_dev, int n_active, const float* logits, int64_t ldl, const float* gate_logits, int64_t ldg, int total_rows,
                                        float lam, float mu, const float* grid, int32_t* cls_raw, float* conf_raw, float* sync_raw, int32_t* cls_lag, int32_t* sync_lag,
                                        float* conf_lag, float* post_lag, int64_t ldp, float* p_sync_lag, int32_t* cls_post_lag, float* conf_post_lag,
                                        float* offset_mean_lag, int32_t* cls_tail, int32_t* sync_tail, float* conf_tail, float* log_z, void* workspace, void* stream) {
  const char* who = "sf_track_pool_push_gated";
  SF_CHECK_ARG(total_rows >= 0 && total_rows <= TRACK_STREAM_MAX_PUSH, "%s: total_rows = %d rows in one push (0 .. %d)", who, total_rows, TRACK_STREAM_MAX_PUSH);
  if (!track_gated_stream_args_ok(who, C, lag, 0, 0, 0, lam, mu)) return -1;
  const TrackStreamOut out{cls_lag, sync_lag, conf_lag, post_lag, ldp, p_sync_lag, cls_post_lag, conf_post_lag, offset_mean_lag, cls_tail, sync_tail, conf_tail};
  return track_pool_push_impl<TrackChainGated>(who, states, state_stride, n_slots, C, lag, posterior, table_host, table_dev, n_active,
                                               TrackChainGated::Src{logits, ldl, gate_logits, ldg}, total_rows, lam, mu, grid, cls_raw, conf_raw, sync_raw, out, log_z,
                                               workspace, stream);
}
