"""Float64 oracle of the gated fixed-lag read-out of a stream (sf_track_stream_push_gated).  numpy only: nothing here imports synchformer_amd.

The outputs are DEFINED through the gated offline read-outs of prefixes (track_gated_oracle: E, T, the tie rules): with path_t = TG.viterbi on rows 0 .. t and
post_t = TG.posterior on rows 0 .. t,

    (cls_lag[w], sync_lag[w]) = path_{w+lag}[w]      post_lag[w] = post_{w+lag}['post'][w]      p_sync_lag[w] = post_{w+lag}['p_sync'][w]
    tail after row t = path_t[max(0, t + 1 - lag) .. t]                                         log_z after row t = that of the prefix 0 .. t

committed by the push that delivers row w + lag (or by the final push, from the whole recording).  by_definition() computes exactly that, one offline read-out per
prefix; GatedStreamOracle is the second, incremental statement - a 2C-wide carried state and rings of the last `lag` rows - that a CPU test holds against the first
and the long GPU run is compared with.

Exact ties are the rule in this chain (plane 0 of the emission is flat), so an fp32 path is not comparable index by index with float64 on random input.  The
criterion that survives ties is the MAX-MARGINAL: max_marginals() gives M_t[w, j], the best score of any path of the prefix 0 .. t through state j at row w; a
committed (cls, sync) is correct iff max_j M[w, j] - M[w, cls + C sync] is within the fp32 margin.  gaps() evaluates that for a whole read-out."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_gated_oracle as TG  # noqa: E402
from track_stream_oracle import counts, softmax  # noqa: E402,F401


def prefix_readouts(logits: np.ndarray, gate: np.ndarray, lam: float, mu: float, grid=None):
    """(paths, posts): TG.viterbi / TG.posterior of every prefix 0 .. t (posts None without a grid); by_definition(pre=...) takes them, so several lags share them."""
    l, z = np.asarray(logits, np.float64), np.asarray(gate, np.float64)
    W = l.shape[0]
    paths = [TG.viterbi(l[:t + 1], z[:t + 1], lam, mu) for t in range(W)]
    posts = [TG.posterior(l[:t + 1], z[:t + 1], lam, mu, grid) for t in range(W)] if grid is not None else None
    return paths, posts


def by_definition(logits: np.ndarray, gate: np.ndarray, lam: float, mu: float, lag: int, pushes, grid=None, pre=None):
    """pushes: [(n, final), ...] whose n sum to W -> one dict per push: w0, cls_raw, conf_raw, sync_raw (n,), cls_lag, sync_lag, conf_lag (k,), cls_tail, sync_tail,
    conf_tail (m,), and with a grid post_lag (k, C), p_sync_lag, cls_post_lag, conf_post_lag, offset_mean_lag (k,), log_z (float; 0.0 while nothing was pushed)."""
    l, z = np.asarray(logits, np.float64), np.asarray(gate, np.float64)
    W, C = l.shape
    assert sum(n for n, _ in pushes) == W and z.shape == (W, 2)
    p = softmax(l) if W else np.zeros_like(l)
    paths, posts = prefix_readouts(l, z, lam, mu, grid) if pre is None else pre
    out, rows = [], 0
    for n, final in pushes:
        w0, k, m = counts(rows, n, lag, final)
        t = rows + n - 1
        new = np.arange(rows, rows + n)
        ws = np.arange(w0, w0 + k)
        ends = np.minimum(ws + lag, t)
        wt = np.arange(t + 1 - m, t + 1)
        d = dict(w0=w0, cls_raw=l[new].argmax(1), conf_raw=p[new].max(1), sync_raw=1.0 / (1.0 + np.exp(-(z[new, 1] - z[new, 0]))))
        d['cls_lag'] = np.array([paths[r]['cls_path'][w] for w, r in zip(ws, ends)], np.int64)
        d['sync_lag'] = np.array([paths[r]['sync_path'][w] for w, r in zip(ws, ends)], np.int64)
        d['conf_lag'] = p[ws, d['cls_lag']]
        d['cls_tail'] = paths[t]['cls_path'][wt] if m else np.zeros(0, np.int64)
        d['sync_tail'] = paths[t]['sync_path'][wt] if m else np.zeros(0, np.int64)
        d['conf_tail'] = p[wt, d['cls_tail']]
        if grid is not None:
            d['post_lag'] = np.array([posts[r]['post'][w] for w, r in zip(ws, ends)]).reshape(k, C)
            for name, key in (('p_sync_lag', 'p_sync'), ('cls_post_lag', 'cls_post'), ('conf_post_lag', 'conf_post'), ('offset_mean_lag', 'offset_mean')):
                d[name] = np.array([posts[r][key][w] for w, r in zip(ws, ends)])
            d['log_z'] = posts[t]['log_z'] if t >= 0 else 0.0
        out.append(d)
        rows += n
    return out


class GatedStreamOracle:
    """The same outputs with carried state: the Viterbi scores S (2C) and the forward vector a (2C, float64,
    unnormalised) and, of the last `lag` rows, the back pointers (2C), BOTH logit rows (C and 2: the emission is recomputed from them) and a (2C).
    push(rows, gate_rows, final) -> the dict of by_definition for that push."""

    def __init__(self, C: int, lam: float, mu: float, lag: int, grid=None):
        self.C, self.lam, self.mu, self.lag = C, float(lam), float(mu), lag
        self.grid = None if grid is None else np.asarray(grid, np.float64)
        self.T = TG.transition(C, lam, mu)
        self.rows, self.s, self.a, self.end = 0, None, None, 0
        self.bp, self.lg, self.gz, self.av = {}, {}, {}, {}                         # row index -> ...: rings of `lag` rows

    def held(self) -> int:
        return max(len(self.bp), len(self.lg), len(self.gz), len(self.av))

    @staticmethod
    def _trace(r: int, w: int, bp, end) -> list:
        cur, out = end[r], []
        for q in range(r, w, -1):
            out.append(cur)
            cur = bp[q][cur]
        out.append(cur)
        return out[::-1]

    def push(self, rows: np.ndarray, gate_rows: np.ndarray, final: bool = False) -> dict:
        C, S = self.C, 2 * self.C
        x, g = np.asarray(rows, np.float64).reshape(-1, C), np.asarray(gate_rows, np.float64).reshape(-1, 2)
        n = x.shape[0]
        assert g.shape[0] == n
        w0, k, m = counts(self.rows, n, self.lag, final)
        bp, lg, gz, av, end = dict(self.bp), dict(self.lg), dict(self.gz), dict(self.av), {self.rows - 1: self.end}
        for i in range(n):
            r = self.rows + i
            e = TG.emission(x[i:i + 1], g[i:i + 1])[0]
            if r == 0:
                self.s, bp[r] = e.copy(), np.zeros(S, np.int64)
            else:
                cand = self.s[:, None] + self.T
                bp[r] = cand.argmax(0)                                              # the first maximum = the lowest predecessor state
                self.s = cand.max(0) + e                                            # (no renormalisation, as TG.viterbi: float64 carries it, and the ties break alike)
            end[r] = int(self.s.argmax())
            lg[r], gz[r] = x[i], g[i]
            if self.grid is not None:
                self.a = e if r == 0 else e + TG.lse(self.a[:, None] + self.T, axis=0)
                av[r] = self.a
        t = self.rows + n - 1
        ws = list(range(w0, w0 + k))
        p = {r: softmax(lg[r][None])[0] for r in lg}
        d = dict(w0=w0, cls_raw=x.argmax(1), conf_raw=softmax(x).max(1) if n else np.zeros(0), sync_raw=1.0 / (1.0 + np.exp(-(g[:, 1] - g[:, 0]))))
        lagged = np.array([self._trace(min(w + self.lag, t), w, bp, end)[0] for w in ws], np.int64)
        tail = np.array(self._trace(t, t + 1 - m, bp, end) if m else [], np.int64)
        d['cls_lag'], d['sync_lag'] = lagged % C, lagged // C
        d['conf_lag'] = np.array([p[w][c] for w, c in zip(ws, d['cls_lag'])])
        d['cls_tail'], d['sync_tail'] = tail % C, tail // C
        d['conf_tail'] = np.array([p[t + 1 - m + j][c] for j, c in enumerate(d['cls_tail'])])
        if self.grid is not None:
            post2 = np.zeros((k, S))
            for j, w in enumerate(ws):
                b = np.zeros(S)
                for r in range(min(w + self.lag, t), w, -1):                        # b_{r-1} from b_r and row r, its emission recomputed from the two logit rows
                    b = TG.lse((b + TG.emission(lg[r][None], gz[r][None])[0])[None, :] + self.T, axis=1)
                sc = av[w] + b
                post2[j] = np.exp(sc - TG.lse(sc))
            post = post2[:, :C] + post2[:, C:]
            cls = post.argmax(1) if k else np.zeros(0, np.int64)
            d.update(post_lag=post, p_sync_lag=post2[:, C:].sum(1), cls_post_lag=cls, conf_post_lag=post[np.arange(k), cls], offset_mean_lag=post @ self.grid,
                     log_z=float(TG.lse(self.a)) if t >= 0 else 0.0)
        self.rows += n
        self.end = end[t] if t >= 0 else 0
        keep = range(max(0, self.rows - self.lag), self.rows)
        self.bp, self.lg, self.gz = {r: bp[r] for r in keep}, {r: lg[r] for r in keep}, {r: gz[r] for r in keep}
        self.av = {r: av[r] for r in keep if r in av}
        return d


def max_marginals(logits: np.ndarray, gate: np.ndarray, lam: float, mu: float) -> np.ndarray:
    """M (W, 2C): M[w, j] = the best TG.path_score of any state path of these W rows that is in state j at row w = a max-forward plus a max-backward pass."""
    E = TG.emission(logits, gate)
    W, S = E.shape
    T = TG.transition(S // 2, lam, mu)
    F, B = np.empty((W, S)), np.zeros((W, S))
    F[0] = E[0]
    for w in range(1, W):
        F[w] = E[w] + (F[w - 1][:, None] + T).max(0)
    for w in range(W - 2, -1, -1):
        B[w] = ((B[w + 1] + E[w + 1])[None, :] + T).max(1)
    return F + B


def prefix_max_marginals(logits: np.ndarray, gate: np.ndarray, lam: float, mu: float) -> list:
    """[M_t for every prefix 0 .. t]; gaps(mm=...) takes them, so several lags and chunkings share them."""
    l, z = np.asarray(logits, np.float64), np.asarray(gate, np.float64)
    return [max_marginals(l[:t + 1], z[:t + 1], lam, mu) for t in range(l.shape[0])]


def gap(M: np.ndarray, w: int, cls: int, sync: int) -> float:
    """How far below the best path through row w the best path through (cls, sync) at row w lies; 0 for a correct decision."""
    C = M.shape[1] // 2
    return float(M[w].max() - M[w, int(cls) + C * int(sync)])


def gaps(mm: list, lag: int, pushes, outs):
    """mm: prefix_max_marginals; pushes [(n, final), ...]; outs: per push an object or dict with cls_lag, sync_lag, cls_tail, sync_tail (array-likes) ->
    (lagged, tail): lists of (w, t, gap) - window w judged on the prefix 0 .. t - over every committed window and every push's tail."""
    get = (lambda o, k: o[k]) if isinstance(outs[0], dict) else getattr
    lagged, tail, rows = [], [], 0
    for (n, final), o in zip(pushes, outs):
        w0, k, m = counts(rows, n, lag, final)
        t = rows + n - 1
        cl, sl, ct, st = (np.asarray(get(o, name)).astype(np.int64) for name in ('cls_lag', 'sync_lag', 'cls_tail', 'sync_tail'))
        assert cl.shape == sl.shape == (k,) and ct.shape == st.shape == (m,), (cl.shape, ct.shape, k, m)
        for i in range(k):
            r = min(w0 + i + lag, t)
            lagged.append((w0 + i, r, gap(mm[r], w0 + i, cl[i], sl[i])))
        for i in range(m):
            tail.append((t + 1 - m + i, t, gap(mm[t], t + 1 - m + i, ct[i], st[i])))
        rows += n
    return lagged, tail


def stream_inputs(seed: int, W: int, C: int, scale: float = 3.0):
    """(logits (W, C), gate logits (W, 2)): scale * randn, fp32 - the random inputs of the stream tests."""
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((W, C))).astype(np.float32), (scale * rng.standard_normal((W, 2))).astype(np.float32)


def discriminations(logits: np.ndarray, gate: np.ndarray, lam: float, mu: float, lag: int, pre=None, mm=None) -> dict:
    """How many windows of a one-push-and-final read-out at `lag` violate the max-marginal bound when the committed block is replaced by a plausible wrong answer,
    from the oracle alone: 'offline' = the path of the whole input, 'lag+1' = the read-out at lag + 1, 'argmax' = the per-row argmax with the gate's own sign;
    'oracle' = the float64 read-out at `lag` itself (0: the criterion accepts the definition).  A test asserts the first three are >= 1 on ITS inputs: an input
    on which a wrong read-out passes proves nothing."""
    l, z = np.asarray(logits, np.float64), np.asarray(gate, np.float64)
    W, C = l.shape
    paths = prefix_readouts(l, z, lam, mu)[0] if pre is None else pre[0]
    mm = prefix_max_marginals(l, z, lam, mu) if mm is None else mm
    subs = dict(oracle=[paths[min(w + lag, W - 1)]['states'][w] for w in range(W)], offline=list(paths[W - 1]['states']),
                argmax=list(l.argmax(1) + C * (z[:, 1] > z[:, 0])))
    subs['lag+1'] = [paths[min(w + lag + 1, W - 1)]['states'][w] for w in range(W)]
    out = {}
    for name, states in subs.items():
        out[name] = sum(gap(mm[min(w + lag, W - 1)], w, states[w] % C, states[w] // C) > path_tol(min(w + lag, W - 1)) for w in range(W))
    return out


def path_tol(t: int) -> float:
    """The margin of a decision on the prefix 0 .. t: (t + 1) * 2^-13, tests/test_track_gated_gpu.py's PATH_TOL per window (scores below 2^9, one ulp 2^-15, four
    rounded operations per window; a real defect costs more than 0.1)."""
    return (t + 1) * 2.0 ** -13
