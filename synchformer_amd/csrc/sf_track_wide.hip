// The wide chain: the track read-outs of a recording over S <= 1024 states at unevenly spaced positions.
// A search over D lags x C classes reads window w at lag d as logits[w, d, :]; state s stands for the pair state_src[s] = d * C + c at the position pos[s] (in class
// steps; non-decreasing in s), and the chain is
//     p(s_0 .. s_{W-1})  ~  exp(sum_w e[w, s_w] - lam sum_{w >= 1} |pos[s_w] - pos[s_{w-1}]|)
//     e[w, s] = logits[w, d, c] - lse_c logits[w, d, .] + g[w, d],        g = -softplus(z0 - z1) = log sigmoid of the gate's margin, 0 without a gate.
// sf_track_decode_wide is its mode (Viterbi), sf_track_posterior_wide its marginals (forward-backward).  The entries of sf_track.hip put one state per lane of ONE
// wavefront and walk all predecessors per step, O(S^2); here thread s of ONE workgroup of ceil(S / 64) wavefronts is state s and a step costs O(S) over all states:
// because the positions ascend,
//     max_p (u[p] - lam |pos[p] - pos[c]|)  =  max( max_{p <= c} (u[p] - lam (pos[c] - pos[p])),  max_{p >= c} (u[p] - lam (pos[p] - pos[c])) )
// and each half is a scan under the DECAYED operator  (v, x) o (v', x') = (max(v - lam (x' - x), v'), x'),  x <= x'  (lse in place of max for the posterior).  The
// partial that reaches lane c from o lanes away always ends at lane c -+ o, so its decay lam |pos[c] - pos[c -+ o]| is a constant of the lane: six per direction, set up
// once; the scan carries values (and indices), never positions.  Across the wavefronts: every wave leaves its two totals in one of at most 16 LDS slots, ONE barrier,
// and every wave folds the slots of the waves before (behind) it, decayed over the distances between the waves' end (first) positions.  The slots are double-buffered
// by the parity of the step, which is what makes one barrier per step enough; the renormalisation (s -= max s) is applied one step late for the same reason: the
// maximum of the vector a step reads travels through the slots with that step's totals.
// Launches (caller's stream, no allocation, no host synchronisation, no atomics: the same bits from call to call and under graph replay):
//   sf_track_decode_wide:     track_wide_rows_kernel (norm[w, d] = g - lse_c; state_raw / conf_raw), track_wide_viterbi_kernel (scan + backtrace from back pointers
//                             staged in LDS a block of rows at a time), track_wide_conf_kernel (conf_path);
//   sf_track_posterior_wide:  track_wide_rows_kernel (norm only), track_wide_inverse_kernel ((d, c) -> state), track_wide_fb_kernel (two workgroups of one launch: the
//                             forward and the backward scan), track_wide_combine_kernel (one workgroup per window: post, state_post, offset_mean, p_lag).
#include "sf_common.h"
#include "sf_track_math.h"
#include "../../include/synchformer_hip.h"
#include <cmath>
#include <cstring>

#define TRACK_WIDE_MAX_S 1024
#define TRACK_WIDE_MAX_C 64
#define TRACK_WIDE_MAX_D 1024
#define TRACK_WIDE_MAX_WAVES (TRACK_WIDE_MAX_S / 64)
#define TRACK_WIDE_BP_STAGE 16384                                   // back pointers staged in LDS per block of rows (32 KB): 16 rows at S = 1024, 780 at S = 21

// Where everything lies in the caller's workspace (bytes from its start, every part 16-byte aligned).  decode: norm (W, D) fp32, the rows' (max, sum) (W, 2) fp32,
// back pointers (W, S) uint16.  posterior: norm (W, D) fp32, inverse (D, 64) int32, a (W, S) fp32, b (W, S) fp32.
// The two entries' norm are NOT the same numbers: the posterior entry stores g - lse_c, the decode entry that minus its row maximum max_d (g - lse_c)[w, .] (a row
// constant the path and the softmax probabilities do not see: track_wide_rows_kernel says why).  A workspace of one entry is never read by the other.
struct TrackWideLayout {
  int64_t norm, stat, back, inv, ab, total;
  TrackWideLayout(int64_t W, int64_t D, int64_t S, int posterior) {
    auto up = [](int64_t b) { return (b + 15) & ~(int64_t)15; };
    norm = 0;
    int64_t at = up(W * D * 4);
    stat = back = inv = ab = 0;
    if (posterior) {
      inv = at;  at = up(at + D * TRACK_WIDE_MAX_C * 4);
      ab = at;   at = up(at + 2 * W * S * 4);
    } else {
      stat = at; at = up(at + 2 * W * 4);
      back = at; at = up(at + W * S * 2);
    }
    total = at;
  }
};

// ---- reductions of a 256-thread workgroup, in a fixed order (wave butterfly, then the four waves in ascending order) ---------------------------------------------
__device__ __forceinline__ float wide_block_max(float v, float* s_red) {
  v = wave_max(v);
  __syncthreads();                                                 // the slots' previous use is over
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}
__device__ __forceinline__ float wide_block_sum(float v, float* s_red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}
// The largest value and, among equals, the lowest index; a NaN never wins.  Every thread gets the same pair.
__device__ __forceinline__ void wide_block_argmax(float& v, int& i, float* s_red, int* s_idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { s_red[threadIdx.x >> 6] = v; s_idx[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = s_red[0];
  i = s_idx[0];
  for (int k = 1; k < 4; ++k)
    if (s_red[k] > v || (s_red[k] == v && s_idx[k] < i)) { v = s_red[k]; i = s_idx[k]; }
}

// ---- rows: one 256-thread workgroup per window ------------------------------------------------------------------------------------------------------------------
// norm[w, d] = g[w, d] - lse_c logits[w, d, .] (0 where that lse is not finite: a lag whose row is all -inf keeps e = -inf), so that
// e[w, s] = logits[w, d, c] + norm[w, d].  With state_raw (the decode entry): norm minus its row maximum (see below), the lowest argmax of e[w, .] over the S states
// and its softmax probability over all S states (1 / sum_s exp(e - max)); stat[w] = (max, sum) for track_wide_conf_kernel.  Without (the posterior entry): norm alone.
__global__ __launch_bounds__(256) void track_wide_rows_kernel(const float* __restrict__ logits, int64_t ldw, int64_t ldd, const float* __restrict__ gate, int64_t ldgw,
                                                               int64_t ldgd, int D, int C, int S, const int32_t* __restrict__ src, float* __restrict__ norm,
                                                               float* __restrict__ stat, int32_t* __restrict__ state_raw, float* __restrict__ conf_raw) {
  __shared__ float s_n[TRACK_WIDE_MAX_D];
  __shared__ float s_red[4];
  __shared__ int s_idx[4];
  const int w = blockIdx.x, t = threadIdx.x;
  for (int d = t; d < D; d += 256) {
    const float* row = logits + (int64_t)w * ldw + (int64_t)d * ldd;
    float m = row[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, row[c]);
    const float sub = fb_finite_or_zero(m);
    // The sum and the logarithm in double: norm is common to all states of a lag, so an error of it goes into every path and adds up along the windows in log_z.  A
    // serial fp32 sum rounds the tail of a softmax (terms around half an ulp of the partial sum) the same way in every window - integer logits repeat them exactly:
    // with it log_z of one lag, C = 64, W = 300, lam = 0 (true value 0) came out at 3.5e-5, with the double at 2.0e-6.  D C exps per window: the cost is not visible.
    double sum = 0.0;
    for (int c = 0; c < C; ++c) sum += (double)expf(row[c] - sub);
    const double lse = (double)sub + log(sum);
    float g = 0.f;
    if (gate) {
      const float* z = gate + (int64_t)w * ldgw + (int64_t)d * ldgd;
      g = -gate_softplus(z[0] - z[1]);
    }
    const float n = (lse > -(double)INFINITY && lse < (double)INFINITY) ? (float)((double)g - lse) : 0.f;
    s_n[d] = n;
    norm[(int64_t)w * D + d] = n;
  }
  if (!state_raw) return;                                          // uniform
  // The decode entry reads e up to a row constant: norm -= max_d norm (0 when that is not finite).  A row constant changes neither the path nor a softmax over the
  // states, and with it the arithmetic of the Viterbi scan is EXACT where it can be: one lag, or rows that agree across the lags, leave e = the logit itself.
  {
    float nm = -INFINITY;
    for (int d = t; d < D; d += 256) nm = fmaxf(nm, s_n[d]);
    nm = fb_finite_or_zero(wide_block_max(nm, s_red));
    for (int d = t; d < D; d += 256) {
      const float n = s_n[d] - nm;
      s_n[d] = n;
      norm[(int64_t)w * D + d] = n;
    }
  }
  __syncthreads();
  const float* lw = logits + (int64_t)w * ldw;
  float best = -INFINITY;
  int bi = S;                                                      // above every state: the first candidate of a thread replaces it even at -inf
  for (int s = t; s < S; s += 256) {
    const int sc = src[s], d = sc / C, c = sc - d * C;
    const float e = lw[(int64_t)d * ldd + c] + s_n[d];
    if (e > best || bi == S) { best = e; bi = s; }
  }
  if (bi == S) bi = S - 1;                                         // (a thread without a state: never below a real candidate of the same value unless all are -inf)
  float m = best;
  int mi = bi;
  if (t >= S) { m = -INFINITY; mi = S - 1; }
  wide_block_argmax(m, mi, s_red, s_idx);
  const float sub = fb_finite_or_zero(m);
  float sum = 0.f;
  for (int s = t; s < S; s += 256) {
    const int sc = src[s], d = sc / C, c = sc - d * C;
    sum += expf(lw[(int64_t)d * ldd + c] + s_n[d] - sub);
  }
  sum = wide_block_sum(sum, s_red);
  if (t == 0) {
    state_raw[w] = mi < S ? mi : S - 1;
    conf_raw[w] = expf(m - sub) / sum;
    stat[2 * (int64_t)w] = sub;
    stat[2 * (int64_t)w + 1] = sum;
  }
}

// conf_path[w] = exp(e[w, state_path[w]] - max) / sum: one thread per window.
__global__ __launch_bounds__(256) void track_wide_conf_kernel(const float* __restrict__ logits, int64_t ldw, int64_t ldd, const float* __restrict__ norm,
                                                               const float* __restrict__ stat, int W, int D, int C, int S, const int32_t* __restrict__ src,
                                                               const int32_t* __restrict__ state_path, float* __restrict__ conf_path) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  int s = state_path[w];
  s = s < 0 ? 0 : (s >= S ? S - 1 : s);
  const int sc = src[s], d = sc / C, c = sc - d * C;
  const float e = logits[(int64_t)w * ldw + (int64_t)d * ldd + c] + norm[(int64_t)w * D + d];
  conf_path[w] = expf(e - stat[2 * (int64_t)w]) / stat[2 * (int64_t)w + 1];
}

// inv[d, c] (row stride 64) = the state that reads (d, c), -1 where no state does.  One workgroup: fill, barrier, scatter (state_src has no repeats).
__global__ __launch_bounds__(1024) void track_wide_inverse_kernel(const int32_t* __restrict__ src, int D, int C, int S, int32_t* __restrict__ inv) {
  for (int i = threadIdx.x; i < D * TRACK_WIDE_MAX_C; i += 1024) inv[i] = -1;
  __syncthreads();
  for (int s = threadIdx.x; s < S; s += 1024) {
    const int sc = src[s], d = sc / C, c = sc - d * C;
    inv[d * TRACK_WIDE_MAX_C + c] = s;
  }
}

// ---- what a thread of the two scan kernels is ---------------------------------------------------------------------------------------------------------------------
// Thread t = state t (threads beyond S act as state S - 1's position with a score of -inf, so every cross-lane operation sees a full EXEC mask and a decay of 0).
// dl[k] / dr[k]: lam times the distance to the lane 2^k to the left / right inside the wavefront.  cl / cr: lam times the distance to the last position of the wave
// before / the first position of the wave behind.  s_dend[k] = lam (end[k] - end[k-1]), s_dbeg[k] = lam (beg[k+1] - beg[k]): the decays between the waves' slots.
struct TrackWideLane {
  int t, lane, wv, nw, d, c;
  bool live;
  float dl[6], dr[6], cl, cr;
  __device__ __forceinline__ TrackWideLane(int S, int C, const int32_t* __restrict__ src, const float* __restrict__ pos, float lam, float* s_dend, float* s_dbeg) {
    t = threadIdx.x;  lane = t & 63;  wv = t >> 6;  nw = blockDim.x >> 6;
    live = t < S;
    const int sc = live ? t : S - 1;
    const float x = pos[sc];
    const int f = src[sc];
    d = f / C;
    c = f - d * C;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      dl[k] = lam * (x - __shfl_up(x, 1u << k, 64));
      dr[k] = lam * (__shfl_down(x, 1u << k, 64) - x);
    }
    const int prev_end = wv * 64 - 1, next_beg = (wv + 1) * 64;
    cl = wv > 0 ? lam * (x - pos[prev_end]) : 0.f;                   // (prev_end < S: every wave holds at least one state)
    cr = wv + 1 < nw ? lam * (pos[next_beg < S ? next_beg : S - 1] - x) : 0.f;
    if (lane == 0) {
      const int e1 = wv * 64 + 63 < S ? wv * 64 + 63 : S - 1;
      s_dend[wv] = wv > 0 ? lam * (pos[e1] - pos[prev_end]) : 0.f;
      s_dbeg[wv] = wv + 1 < nw ? lam * (pos[next_beg < S ? next_beg : S - 1] - x) : 0.f;
    }
  }
};

// ---- Viterbi ----------------------------------------------------------------------------------------------------------------------------------------------------
//   s_0 = e[0];   s_w[c] = max_p (s_{w-1}[p] - lam |pos[p] - pos[c]|) + e[w, c]   (the lowest p among the maximisers -> backptr[w, c], uint16);   s_w -= max s_{w-1}
// (the renormalisation runs one step late, see the head of the file; it bounds the scores all the same: max s_w >= the emission of the previous maximum's state).
// Ties: inside the prefix half the partial from the left (lower indices) wins `>=`; inside the suffix half the partial from the right wins only `>`; the prefix half
// wins `>=` against the suffix half: the lowest maximiser overall.  A NaN loses every comparison it could win an out-of-range index with, and the backtrace clamps.
// The end state is the lowest argmax of the last scores.  Backtrace: blocks of rows of back pointers are copied into LDS by the whole workgroup (contiguous uint16),
// thread 0 follows them there.
__global__ __launch_bounds__(1024) void track_wide_viterbi_kernel(const float* __restrict__ logits, int64_t ldw, int64_t ldd, const float* __restrict__ norm, int W, int D,
                                                                   int C, int S, const int32_t* __restrict__ src, const float* __restrict__ pos, float lam,
                                                                   int32_t* __restrict__ state_path, uint16_t* __restrict__ backptr) {
  __shared__ float s_pv[2][TRACK_WIDE_MAX_WAVES], s_sv[2][TRACK_WIDE_MAX_WAVES], s_mx[2][TRACK_WIDE_MAX_WAVES];
  __shared__ int s_pi[2][TRACK_WIDE_MAX_WAVES], s_si[2][TRACK_WIDE_MAX_WAVES];
  __shared__ float s_dend[TRACK_WIDE_MAX_WAVES], s_dbeg[TRACK_WIDE_MAX_WAVES];
  __shared__ uint16_t s_bp[TRACK_WIDE_BP_STAGE];
  const TrackWideLane ln(S, C, src, pos, lam, s_dend, s_dbeg);
  const int t = ln.t, lane = ln.lane, wv = ln.wv, nw = ln.nw;
  const float ninf = -INFINITY;
  const int64_t lo = (int64_t)ln.d * ldd + ln.c;
  float s = ln.live ? logits[lo] + norm[ln.d] : ninf;
  float l_next = (ln.live && W > 1) ? logits[ldw + lo] : ninf, n_next = (ln.live && W > 1) ? norm[D + ln.d] : 0.f;
  __syncthreads();                                                 // s_dend / s_dbeg
  for (int w = 1; w < W; ++w) {
    const int buf = w & 1;
    const float e = l_next + n_next;
    if (w + 1 < W && ln.live) {                                    // the next row's loads travel under this step's scans
      l_next = logits[(int64_t)(w + 1) * ldw + lo];
      n_next = norm[(int64_t)(w + 1) * D + ln.d];
    }
    float pv = s, sv = s;
    int pi = t, si = t;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int o = 1 << k;
      const float v2 = __shfl_up(pv, o, 64) - ln.dl[k];
      const int i2 = __shfl_up(pi, o, 64);
      if (lane >= o && v2 >= pv) { pv = v2; pi = i2; }
      const float v3 = __shfl_down(sv, o, 64) - ln.dr[k];
      const int i3 = __shfl_down(si, o, 64);
      if (lane + o < 64 && v3 > sv) { sv = v3; si = i3; }
    }
    const float wm = wave_max(s);
    if (lane == 63) { s_pv[buf][wv] = pv; s_pi[buf][wv] = pi; }
    if (lane == 0) { s_sv[buf][wv] = sv; s_si[buf][wv] = si; s_mx[buf][wv] = wm; }
    __syncthreads();
    float mx = s_mx[buf][0];
    for (int k = 1; k < nw; ++k) mx = fmaxf(mx, s_mx[buf][k]);
    if (wv > 0) {                                                  // the waves before this one, folded left to right: the carry stands at the end of wave k
      float cv = s_pv[buf][0];
      int ci = s_pi[buf][0];
      for (int k = 1; k < wv; ++k) {
        cv -= s_dend[k];
        const float tv = s_pv[buf][k];
        if (!(cv >= tv)) { cv = tv; ci = s_pi[buf][k]; }
      }
      cv -= ln.cl;
      if (cv >= pv) { pv = cv; pi = ci; }
    }
    if (wv + 1 < nw) {                                             // the waves behind it, folded right to left: the carry stands at the first position of wave k
      float cv = s_sv[buf][nw - 1];
      int ci = s_si[buf][nw - 1];
      for (int k = nw - 2; k > wv; --k) {
        cv -= s_dbeg[k];
        const float tv = s_sv[buf][k];
        if (!(cv > tv)) { cv = tv; ci = s_si[buf][k]; }
      }
      cv -= ln.cr;
      if (cv > sv) { sv = cv; si = ci; }
    }
    const bool pre = pv >= sv;
    const float best = pre ? pv : sv;
    int bp = pre ? pi : si;
    bp = bp < S ? bp : S - 1;
    if (ln.live) backptr[(int64_t)w * S + t] = (uint16_t)bp;
    s = ln.live ? best + e - fb_finite_or_zero(mx) : ninf;
  }
  // the end state: the lowest argmax of the last scores
  __syncthreads();                                                 // the last step's slots have been read
  {
    const float wm = wave_max(s);
    const unsigned long long hit = __ballot(ln.live && s == wm);
    if (lane == 0) { s_sv[0][wv] = wm; s_si[0][wv] = wv * 64 + (hit ? __ffsll((long long)hit) - 1 : 0); }
  }
  __syncthreads();                                                 // also orders the scan's backptr stores before the loads below
  if (t == 0) {
    float m = s_sv[0][0];
    int cur = s_si[0][0];
    for (int k = 1; k < nw; ++k)
      if (s_sv[0][k] > m) { m = s_sv[0][k]; cur = s_si[0][k]; }
    cur = cur < S ? cur : S - 1;
    state_path[W - 1] = cur;
    s_pi[0][0] = cur;
  }
  const int rb = TRACK_WIDE_BP_STAGE / S;                          // rows per staged block (>= 16)
  for (int r1 = W - 1; r1 >= 1; r1 -= rb) {                        // rows r1 .. r0 of the back pointers, r0 >= 1
    const int r0 = r1 - rb + 1 > 1 ? r1 - rb + 1 : 1;
    const int n = (r1 - r0 + 1) * S;
    const uint16_t* from = backptr + (int64_t)r0 * S;
    __syncthreads();                                               // the stage's previous block has been walked; s_pi[0][0] is written
    for (int i = t; i < n; i += blockDim.x) s_bp[i] = from[i];
    __syncthreads();
    if (t == 0) {
      int cur = s_pi[0][0];
      for (int r = r1; r >= r0; --r) {
        const int p = s_bp[(r - r0) * S + cur];
        cur = p < S ? p : S - 1;
        state_path[r - 1] = cur;
      }
      s_pi[0][0] = cur;
    }
  }
}

// ---- forward-backward -------------------------------------------------------------------------------------------------------------------------------------------
// log(exp(a) + exp(b)); -inf when both are.
__device__ __forceinline__ float wide_lae(float a, float b) {
  const float m = fmaxf(a, b), n = fminf(a, b);
  return m == -INFINITY ? m : m + log1pf(expf(n - m));
}

// Block 0, rows 0 .. W-1:   a_0 = e[0];      a_w[c] = e[w, c] + lse_p (a_{w-1}[p] - lam |pos[p] - pos[c]|);
// block 1, rows W-1 .. 0:   b_{W-1} = 0;     b_w[c] = lse_n (b_{w+1}[n] + e[w+1, n] - lam |pos[n] - pos[c]|).
// u = the vector the transition reads (a_{w-1}, or b_{w+1} + e[w+1]).  The lse over all predecessors = lae(inclusive prefix scan, EXCLUSIVE suffix scan) under the decayed
// operator with lae in place of max.  The maximum of u (0 when it is not finite) is subtracted from the new vector - the per-row constant cancels in post - and, in the
// forward block, added to a double: log_z = the subtracted maxima + lse of the last vector.  ws = a (W, S) then b (W, S), fp32.
__global__ __launch_bounds__(1024) void track_wide_fb_kernel(const float* __restrict__ logits, int64_t ldw, int64_t ldd, const float* __restrict__ norm, int W, int D, int C,
                                                              int S, const int32_t* __restrict__ src, const float* __restrict__ pos, float lam, float* __restrict__ ws,
                                                              float* __restrict__ log_z) {
  __shared__ float s_pv[2][TRACK_WIDE_MAX_WAVES], s_sv[2][TRACK_WIDE_MAX_WAVES], s_mx[2][TRACK_WIDE_MAX_WAVES];
  __shared__ float s_dend[TRACK_WIDE_MAX_WAVES], s_dbeg[TRACK_WIDE_MAX_WAVES];
  const TrackWideLane ln(S, C, src, pos, lam, s_dend, s_dbeg);
  const int t = ln.t, lane = ln.lane, wv = ln.wv, nw = ln.nw;
  const bool back = blockIdx.x == 1;                               // uniform
  const float ninf = -INFINITY;
  const int64_t lo = (int64_t)ln.d * ldd + ln.c;
  float* out = ws + (back ? (int64_t)W * S : 0);
  const int64_t row0 = back ? W - 1 : 0, step = back ? -1 : 1;     // scan position k reads row row0 + step * k
  double shifted = 0.0;
  float e = ln.live ? logits[row0 * ldw + lo] + norm[row0 * D + ln.d] : ninf;
  float v = back ? (ln.live ? 0.f : ninf) : e;
  if (ln.live) out[row0 * S + t] = v;
  float u = back ? v + e : v;
  float l_next = (ln.live && W > 1) ? logits[(row0 + step) * ldw + lo] : ninf, n_next = (ln.live && W > 1) ? norm[(row0 + step) * D + ln.d] : 0.f;
  __syncthreads();                                                 // s_dend / s_dbeg
  for (int k = 1; k < W; ++k) {
    const int buf = k & 1;
    const int64_t row = row0 + step * k;
    e = l_next + n_next;
    if (k + 1 < W && ln.live) {
      l_next = logits[(row + step) * ldw + lo];
      n_next = norm[(row + step) * D + ln.d];
    }
    float pv = u, sv = u;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int o = 1 << j;
      const float v2 = __shfl_up(pv, o, 64) - ln.dl[j];
      if (lane >= o) pv = wide_lae(v2, pv);
      const float v3 = __shfl_down(sv, o, 64) - ln.dr[j];
      if (lane + o < 64) sv = wide_lae(sv, v3);
    }
    const float wm = wave_max(u);
    float sx = __shfl_down(sv, 1, 64) - ln.dr[0];                  // exclusive: the suffix of the lanes to the right
    if (lane == 63) sx = ninf;
    if (lane == 63) s_pv[buf][wv] = pv;
    if (lane == 0) { s_sv[buf][wv] = sv; s_mx[buf][wv] = wm; }
    __syncthreads();
    float mx = s_mx[buf][0];
    for (int j = 1; j < nw; ++j) mx = fmaxf(mx, s_mx[buf][j]);
    mx = fb_finite_or_zero(mx);
    if (wv > 0) {
      float cv = s_pv[buf][0];
      for (int j = 1; j < wv; ++j) cv = wide_lae(cv - s_dend[j], s_pv[buf][j]);
      pv = wide_lae(cv - ln.cl, pv);
    }
    if (wv + 1 < nw) {
      float cv = s_sv[buf][nw - 1];
      for (int j = nw - 2; j > wv; --j) cv = wide_lae(s_sv[buf][j], cv - s_dbeg[j]);
      sx = wide_lae(sx, cv - ln.cr);
    }
    const float r = wide_lae(pv, sx) - mx;
    v = ln.live ? (back ? r : r + e) : ninf;
    shifted += (double)mx;
    if (ln.live) out[row * S + t] = v;
    u = back ? v + e : v;
  }
  if (!back) {                                                     // log_z = the subtracted maxima + lse of the last vector, its waves in ascending order
    const float wm = wave_max(v);
    __syncthreads();
    if (lane == 0) s_mx[0][wv] = wm;
    __syncthreads();
    float mx = s_mx[0][0];
    for (int j = 1; j < nw; ++j) mx = fmaxf(mx, s_mx[0][j]);
    mx = fb_finite_or_zero(mx);
    const float ws_sum = wave_sum(expf(v - mx));
    if (lane == 0) s_pv[0][wv] = ws_sum;
    __syncthreads();
    if (t == 0) {
      float sum = s_pv[0][0];
      for (int j = 1; j < nw; ++j) sum += s_pv[0][j];
      log_z[0] = (float)(shifted + (double)mx + (double)logf(sum));
    }
  }
}

// One 256-thread workgroup per window: post[w, s] = exp(a + b - lse_s (a + b)); state_post = its argmax (lowest state on ties), conf_post its value; offset_mean =
// sum_s post off[s]; p_lag[w, d] = sum_c post[w, inv[d, c]] in ascending c.  Sums in a fixed order: a thread's states ascending, a wave butterfly, the waves ascending.
__global__ __launch_bounds__(256) void track_wide_combine_kernel(const float* __restrict__ ws, int W, int D, int C, int S, const int32_t* __restrict__ inv,
                                                                  const float* __restrict__ off, float* __restrict__ post, int64_t ldp, int32_t* __restrict__ state_post,
                                                                  float* __restrict__ conf_post, float* __restrict__ offset_mean, float* __restrict__ p_lag) {
  __shared__ float s_p[TRACK_WIDE_MAX_S];
  __shared__ float s_red[4];
  __shared__ int s_idx[4];
  const int w = blockIdx.x, t = threadIdx.x;
  const float* a = ws + (int64_t)w * S;
  const float* b = a + (int64_t)W * S;
  float m = -INFINITY;
  for (int s = t; s < S; s += 256) {
    const float x = a[s] + b[s];
    s_p[s] = x;
    m = fmaxf(m, x);
  }
  m = fb_finite_or_zero(wide_block_max(m, s_red));
  float sum = 0.f;
  for (int s = t; s < S; s += 256) sum += expf(s_p[s] - m);
  sum = wide_block_sum(sum, s_red);
  const float lse = fb_finite_or_zero(m + logf(sum));
  float best = -1.f, mean = 0.f;
  int bi = S - 1;
  for (int s = t; s < S; s += 256) {
    const float p = expf(s_p[s] - lse);
    s_p[s] = p;
    post[(int64_t)w * ldp + s] = p;
    mean += p * off[s];
    if (p > best) { best = p; bi = s; }
  }
  mean = wide_block_sum(mean, s_red);
  wide_block_argmax(best, bi, s_red, s_idx);                       // (its barriers also publish s_p)
  if (t == 0) {
    state_post[w] = bi;
    conf_post[w] = best < 0.f ? 0.f : best;
    offset_mean[w] = mean;
  }
  for (int d = t; d < D; d += 256) {
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
      const int s = inv[d * TRACK_WIDE_MAX_C + c];
      if (s >= 0) acc += s_p[s];
    }
    p_lag[(int64_t)w * D + d] = acc;
  }
}

// ---- the launchers ----------------------------------------------------------------------------------------------------------------------------------------------
// What both entries refuse before they look at a device pointer: the sizes, the strides, lam, and the HOST copies of the two tables (pos finite and non-decreasing,
// state_src inside [0, D C) without repeats).  The kernels read the DEVICE copies; that the two agree is the caller's business, as with sf_track_pool_push's table.
static int track_wide_args_ok(const char* who, int64_t ldw, int64_t ldd, const float* gate, int64_t ldgw, int64_t ldgd, int W, int D, int C, int S,
                              const int32_t* src_host, const float* pos_host, float lam) {
  SF_CHECK_ARG(W >= 0, "%s: W = %d windows", who, W);
  SF_CHECK_ARG(S >= 2 && S <= TRACK_WIDE_MAX_S, "%s: S = %d states out of range (2 .. %d: one thread per state, one workgroup)", who, S, TRACK_WIDE_MAX_S);
  SF_CHECK_ARG(C >= 2 && C <= TRACK_WIDE_MAX_C, "%s: C = %d classes out of range (2 .. %d)", who, C, TRACK_WIDE_MAX_C);
  SF_CHECK_ARG(D >= 1 && D <= TRACK_WIDE_MAX_D, "%s: D = %d lags out of range (1 .. %d)", who, D, TRACK_WIDE_MAX_D);
  SF_CHECK_ARG((int64_t)S <= (int64_t)D * C, "%s: S = %d states for D * C = %lld pairs", who, S, (long long)D * C);
  SF_CHECK_ARG(ldd >= C && ldw >= (int64_t)(D - 1) * ldd + C, "%s: lag stride ldd = %lld below C = %d, or row stride ldw = %lld below (D - 1) ldd + C", who, (long long)ldd, C,
               (long long)ldw);
  if (gate) SF_CHECK_ARG(ldgd >= 2 && ldgw >= (int64_t)(D - 1) * ldgd + 2, "%s: gate lag stride ldgd = %lld below 2, or gate row stride ldgw = %lld below (D - 1) ldgd + 2", who,
                         (long long)ldgd, (long long)ldgw);
  SF_CHECK_ARG(std::isfinite(lam) && lam >= 0.f, "%s: lam must be finite and >= 0 (the cost of a class step)", who);
  if (W == 0 && !(src_host && pos_host)) return 0;                 // nothing to do and no tables to look at
  SF_CHECK_ARG(src_host && pos_host, "%s: null pointer (the host copies of state_src / pos)", who);
  uint64_t seen[TRACK_WIDE_MAX_D * TRACK_WIDE_MAX_C / 64];
  memset(seen, 0, sizeof(uint64_t) * (size_t)(((int64_t)D * C + 63) / 64));
  for (int s = 0; s < S; ++s) {
    SF_CHECK_ARG(std::isfinite(pos_host[s]) && (s == 0 || pos_host[s] >= pos_host[s - 1]), "%s: pos[%d] = %g: the positions are finite and ascending", who, s,
                 (double)pos_host[s]);
    const int f = src_host[s];
    SF_CHECK_ARG(f >= 0 && f < D * C, "%s: state_src[%d] = %d outside [0, D C = %d)", who, s, f, D * C);
    SF_CHECK_ARG(!(seen[f >> 6] >> (f & 63) & 1), "%s: state_src[%d] = %d repeats an earlier state", who, s, f);
    seen[f >> 6] |= 1ull << (f & 63);
  }
  return 0;
}

extern "C" int sf_track_wide_workspace_bytes(int W, int D, int S, int posterior, int64_t* bytes) {
  SF_CHECK_ARG(bytes != nullptr, "sf_track_wide_workspace_bytes: null pointer");
  SF_CHECK_ARG(W >= 0 && D >= 1 && D <= TRACK_WIDE_MAX_D && S >= 2 && S <= TRACK_WIDE_MAX_S, "sf_track_wide_workspace_bytes: W = %d, D = %d, S = %d", W, D, S);
  *bytes = TrackWideLayout(W > 0 ? W : 1, D, S, posterior).total;
  return 0;
}

extern "C" int sf_track_decode_wide(const float* logits, int64_t ldw, int64_t ldd, const float* gate_logits, int64_t ldgw, int64_t ldgd, int W, int D, int C, int S,
                                    const int32_t* state_src_host, const float* pos_host, const int32_t* state_src_dev, const float* pos_dev, float lam,
                                    int32_t* state_raw, float* conf_raw, int32_t* state_path, float* conf_path, void* workspace, void* stream) {
  const char* who = "sf_track_decode_wide";
  if (track_wide_args_ok(who, ldw, ldd, gate_logits, ldgw, ldgd, W, D, C, S, state_src_host, pos_host, lam)) return -1;
  if (W == 0) return 0;
  SF_CHECK_ARG(logits && state_src_dev && pos_dev && state_raw && conf_raw && state_path && conf_path && workspace, "%s: null pointer", who);
  const TrackWideLayout L(W, D, S, 0);
  unsigned char* ws = (unsigned char*)workspace;
  float* norm = (float*)(ws + L.norm);
  float* stat = (float*)(ws + L.stat);
  uint16_t* back = (uint16_t*)(ws + L.back);
  hipStream_t s = (hipStream_t)stream;
  const unsigned threads = (unsigned)((S + 63) / 64) * 64;
  hipLaunchKernelGGL(track_wide_rows_kernel, dim3((unsigned)W), dim3(256), 0, s, logits, ldw, ldd, gate_logits, ldgw, ldgd, D, C, S, state_src_dev, norm, stat, state_raw,
                     conf_raw);
  SF_LAUNCH_CHECK_AS(who);
  hipLaunchKernelGGL(track_wide_viterbi_kernel, dim3(1), dim3(threads), 0, s, logits, ldw, ldd, (const float*)norm, W, D, C, S, state_src_dev, pos_dev, lam, state_path, back);
  SF_LAUNCH_CHECK_AS(who);
  hipLaunchKernelGGL(track_wide_conf_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, s, logits, ldw, ldd, (const float*)norm, (const float*)stat, W, D, C, S,
                     state_src_dev, (const int32_t*)state_path, conf_path);
  SF_LAUNCH_CHECK_AS(who);
  return 0;
}

extern "C" int sf_track_posterior_wide(const float* logits, int64_t ldw, int64_t ldd, const float* gate_logits, int64_t ldgw, int64_t ldgd, int W, int D, int C, int S,
                                       const int32_t* state_src_host, const float* pos_host, const int32_t* state_src_dev, const float* pos_dev, float lam,
                                       const float* off, float* post, int64_t ldp, int32_t* state_post, float* conf_post, float* offset_mean, float* p_lag, float* log_z,
                                       void* workspace, void* stream) {
  const char* who = "sf_track_posterior_wide";
  if (track_wide_args_ok(who, ldw, ldd, gate_logits, ldgw, ldgd, W, D, C, S, state_src_host, pos_host, lam)) return -1;
  SF_CHECK_ARG(ldp >= S, "%s: post row stride ldp = %lld below S = %d", who, (long long)ldp, S);
  if (W == 0) return 0;
  SF_CHECK_ARG(logits && state_src_dev && pos_dev && off && post && state_post && conf_post && offset_mean && p_lag && log_z && workspace, "%s: null pointer", who);
  const TrackWideLayout L(W, D, S, 1);
  unsigned char* ws = (unsigned char*)workspace;
  float* norm = (float*)(ws + L.norm);
  int32_t* inv = (int32_t*)(ws + L.inv);
  float* ab = (float*)(ws + L.ab);
  hipStream_t s = (hipStream_t)stream;
  const unsigned threads = (unsigned)((S + 63) / 64) * 64;
  hipLaunchKernelGGL(track_wide_rows_kernel, dim3((unsigned)W), dim3(256), 0, s, logits, ldw, ldd, gate_logits, ldgw, ldgd, D, C, S, state_src_dev, norm, (float*)nullptr,
                     (int32_t*)nullptr, (float*)nullptr);
  SF_LAUNCH_CHECK_AS(who);
  hipLaunchKernelGGL(track_wide_inverse_kernel, dim3(1), dim3(1024), 0, s, state_src_dev, D, C, S, inv);
  SF_LAUNCH_CHECK_AS(who);
  hipLaunchKernelGGL(track_wide_fb_kernel, dim3(2), dim3(threads), 0, s, logits, ldw, ldd, (const float*)norm, W, D, C, S, state_src_dev, pos_dev, lam, ab, log_z);
  SF_LAUNCH_CHECK_AS(who);
  hipLaunchKernelGGL(track_wide_combine_kernel, dim3((unsigned)W), dim3(256), 0, s, (const float*)ab, W, D, C, S, (const int32_t*)inv, off, post, ldp, state_post, conf_post,
                     offset_mean, p_lag);
  SF_LAUNCH_CHECK_AS(who);
  return 0;
}
