"""Float64 oracle of the fixed-lag read-out of a stream of window logits (sf_track_stream_push).  numpy only: nothing here imports synchformer_amd.

The outputs are DEFINED through the offline read-outs of prefixes: with path_t = the Viterbi path of rows 0 .. t (the recurrence of sf_track_decode, restated
below as tests/test_track_gpu.py restates it) and post_t = track_posterior_oracle.posterior on rows 0 .. t,

    cls_lag[w]  = path_{w+lag}[w]          post_lag[w] = post_{w+lag}[w]          committed by the push that delivers row w + lag (or by the final push, from
                                                                                   the whole recording: path_{W-1}[w], post_{W-1}[w])
    tail after row t = path_t[max(0, t + 1 - lag) .. t]                            log_z after row t = that of the prefix 0 .. t

by_definition() computes exactly that, one offline read-out per prefix (O(W^2)); StreamOracle is the second, incremental statement - carried scan vectors and the
last `lag` rows only - that a CPU test holds against the first and that the long GPU run (W = 4096) is compared with."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_posterior_oracle as TP  # noqa: E402


def viterbi(logits: np.ndarray, lam: float) -> np.ndarray:
    """e[w, c] = l[w, c] - max_c l[w, .];  s_0 = e[0];  s_w[c] = max_p (s_{w-1}[p] - lam |p - c|) + e[w, c], lowest p on ties -> bp[w, c];  s_w -= max_c s_w[c];
    end = argmax s_{W-1}, lowest index on ties;  backtrace through bp."""
    l = np.asarray(logits, np.float64)
    e = l - l.max(1, keepdims=True)
    W, C = e.shape
    d = np.abs(np.arange(C)[:, None] - np.arange(C)[None, :]).astype(np.float64)   # d[p, c]
    s = e[0].copy()
    bp = np.zeros((W, C), np.int64)
    for w in range(1, W):
        cand = s[:, None] - float(lam) * d
        bp[w] = cand.argmax(0)                                                      # first maximum = lowest p
        s = cand.max(0) + e[w]
        s = s - s.max()
    path = np.zeros(W, np.int64)
    path[-1] = s.argmax()
    for w in range(W - 1, 0, -1):
        path[w - 1] = bp[w, path[w]]
    return path


def softmax(logits: np.ndarray) -> np.ndarray:
    l = np.asarray(logits, np.float64)
    p = np.exp(l - l.max(1, keepdims=True))
    return p / p.sum(1, keepdims=True)


def counts(rows: int, n: int, lag: int, final: bool):
    """(w0, n_commit, n_tail) of a push of n rows onto `rows` rows."""
    done_old = max(0, rows - lag)
    done_new = rows + n if final else max(0, rows + n - lag)
    return done_old, done_new - done_old, rows + n - done_new


def prefix_readouts(logits: np.ndarray, lam: float, grid=None):
    """(paths, posts): the offline read-outs of every prefix 0 .. t (posts None without a grid); by_definition(pre=...) takes them, so several lags share them."""
    x = np.asarray(logits, np.float64)
    W = x.shape[0]
    return [viterbi(x[:t + 1], lam) for t in range(W)], ([TP.posterior(x[:t + 1], lam, grid) for t in range(W)] if grid is not None else None)


def by_definition(logits: np.ndarray, lam: float, lag: int, pushes, grid=None, pre=None):
    """pushes: [(n, final), ...] whose n sum to W -> one dict per push: w0, cls_raw, conf_raw (n,), cls_lag, conf_lag (k,), cls_tail, conf_tail (m,), and with a
    grid post_lag (k, C), cls_post_lag, conf_post_lag, offset_mean_lag (k,), log_z (float; 0.0 while nothing was pushed)."""
    x = np.asarray(logits, np.float64)
    W = x.shape[0]
    assert sum(n for n, _ in pushes) == W
    p = softmax(x) if W else np.zeros_like(x)
    paths, posts = prefix_readouts(x, lam, grid) if pre is None else pre
    out, rows = [], 0
    for n, final in pushes:
        w0, k, m = counts(rows, n, lag, final)
        t = rows + n - 1                                                            # the last row pushed so far
        new = np.arange(rows, rows + n)
        ws = np.arange(w0, w0 + k)
        ends = np.minimum(ws + lag, t)                                              # the prefix that commits window w (t: only in a final push)
        wt = np.arange(t + 1 - m, t + 1)
        d = dict(w0=w0, cls_raw=x[new].argmax(1), conf_raw=p[new].max(1))
        d['cls_lag'] = np.array([paths[r][w] for w, r in zip(ws, ends)], np.int64)
        d['conf_lag'] = p[ws, d['cls_lag']]
        d['cls_tail'] = paths[t][wt] if m else np.zeros(0, np.int64)
        d['conf_tail'] = p[wt, d['cls_tail']]
        if grid is not None:
            d['post_lag'] = np.array([posts[r]['post'][w] for w, r in zip(ws, ends)]).reshape(k, x.shape[1])
            for name, key in (('cls_post_lag', 'cls_post'), ('conf_post_lag', 'conf_post'), ('offset_mean_lag', 'offset_mean')):
                d[name] = np.array([posts[r][key][w] for w, r in zip(ws, ends)])
            d['log_z'] = posts[t]['log_z'] if t >= 0 else 0.0
        out.append(d)
        rows += n
    return out


class StreamOracle:
    """The same outputs with carried state: the Viterbi scores s, the (unnormalised, float64) forward vector a, and of the last `lag` rows the back pointers, the
    logits and a.  push(rows, final) -> the dict of by_definition for that push."""

    def __init__(self, C: int, lam: float, lag: int, grid=None):
        self.C, self.lam, self.lag = C, float(lam), lag
        self.grid = None if grid is None else np.asarray(grid, np.float64)
        self.pen = self.lam * np.abs(np.arange(C)[:, None] - np.arange(C)[None, :]).astype(np.float64)     # pen[p, c]
        self.rows, self.s, self.a, self.end = 0, None, None, 0
        self.bp, self.lg, self.av = {}, {}, {}                                      # row index -> back pointers / logits / a: rings of `lag` rows

    def held(self) -> int:
        return max(len(self.bp), len(self.lg), len(self.av))

    def _trace(self, r: int, w: int, bp, end) -> list:
        """the classes at rows w .. r of the path that ends in end[r]"""
        cur, out = end[r], []
        for q in range(r, w, -1):
            out.append(cur)
            cur = bp[q][cur]
        out.append(cur)
        return out[::-1]

    def push(self, rows: np.ndarray, final: bool = False) -> dict:
        x = np.asarray(rows, np.float64).reshape(-1, self.C)
        n = x.shape[0]
        w0, k, m = counts(self.rows, n, self.lag, final)
        bp, lg, av, end = dict(self.bp), dict(self.lg), dict(self.av), {self.rows - 1: self.end}
        for i in range(n):
            r = self.rows + i
            e = x[i] - x[i].max()
            if r == 0:
                self.s, bp[r] = e.copy(), np.zeros(self.C, np.int64)
            else:
                cand = self.s[:, None] - self.pen
                bp[r] = cand.argmax(0)
                self.s = cand.max(0) + e
                self.s = self.s - self.s.max()
            end[r] = int(self.s.argmax())
            lg[r] = x[i]
            if self.grid is not None:
                el = x[i] - TP.lse(x[i])
                self.a = el if r == 0 else el + TP.lse(self.a[:, None] - self.pen, axis=0)
                av[r] = self.a
        t = self.rows + n - 1
        ws = list(range(w0, w0 + k))
        p = {r: softmax(lg[r][None])[0] for r in lg}
        d = dict(w0=w0, cls_raw=x.argmax(1), conf_raw=softmax(x).max(1) if n else np.zeros(0))
        d['cls_lag'] = np.array([self._trace(min(w + self.lag, t), w, bp, end)[0] for w in ws], np.int64)
        d['conf_lag'] = np.array([p[w][c] for w, c in zip(ws, d['cls_lag'])])
        d['cls_tail'] = np.array(self._trace(t, t + 1 - m, bp, end) if m else [], np.int64)
        d['conf_tail'] = np.array([p[t + 1 - m + j][c] for j, c in enumerate(d['cls_tail'])])
        if self.grid is not None:
            post = np.zeros((k, self.C))
            for j, w in enumerate(ws):
                b = np.zeros(self.C)
                for r in range(min(w + self.lag, t), w, -1):                        # b_{r-1} from b_r and row r
                    b = TP.lse((b + lg[r] - TP.lse(lg[r]))[:, None] - self.pen, axis=0)
                sc = av[w] + b
                post[j] = np.exp(sc - TP.lse(sc))
            cls = post.argmax(1) if k else np.zeros(0, np.int64)
            d.update(post_lag=post, cls_post_lag=cls, conf_post_lag=post[np.arange(k), cls], offset_mean_lag=post @ self.grid,
                     log_z=float(TP.lse(self.a)) if t >= 0 else 0.0)
        self.rows += n
        self.end = end[t] if t >= 0 else 0
        keep = range(max(0, self.rows - self.lag), self.rows)                       # the last `lag` rows
        self.bp, self.lg, self.av = {r: bp[r] for r in keep}, {r: lg[r] for r in keep}, {r: av[r] for r in keep if r in av}
        return d


CHUNKINGS = ('whole', 'ones', 'ragged', 'long_after_short')


def chunking(name: str, W: int, lag: int):
    """Row counts per push for W rows: all at once; one at a time; 3, 1, 5, 2, ... repeated; several short pushes, then one longer than lag + 1, then the rest."""
    if name == 'whole':
        return [W]
    if name == 'ones':
        return [1] * W
    out, left, i = [], W, 0
    if name == 'ragged':
        pattern = (3, 1, 5, 2)
    else:
        assert name == 'long_after_short'
        pattern = (2, 1, 2, lag + 3, 1, 4)
    while left:
        out.append(min(pattern[i % len(pattern)], left))
        left -= out[-1]
        i += 1
    return out
