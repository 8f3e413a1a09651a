"""Float64 oracle of the wide chain (sf_track_decode_wide / sf_track_posterior_wide).  numpy only: nothing here imports synchformer_amd.

    states s = 0 .. S-1 read the pair state_src[s] = d * C + c of logits (W, D, C) and stand at pos[s] (non-decreasing)
    e[w, s] = logits[w, d, c] - lse_c logits[w, d, .] + g[w, d],      g = -softplus(z0 - z1), 0 without a gate
    p(s_0 .. s_{W-1})  ~  exp(sum_w e[w, s_w] - lam sum_{w >= 1} |pos[s_w] - pos[s_{w-1}]|)

states(): the table of a search over lags.  emission(): e.  viterbi(): the O(S^2) mode with the contract's tie rules.  posterior(): the O(S^2) forward-backward,
literally (no renormalisation).  brute_force(): every one of the S^W paths."""
import itertools

import numpy as np

from track_posterior_oracle import lse


def states(lags, grid, seg_sec=0.32):
    """-> (state_src, pos, off, lag_of, cls_of): state (lag index d, class c) stands for seg_sec * lags[d] + grid[c], taken to the microsecond; sorted by
    (offset, d, c); pos = offset / (grid[1] - grid[0]); off float64 seconds."""
    grid = np.asarray(grid, np.float64)
    C = grid.shape[0]
    step = int(round(float(grid[1] - grid[0]) * 1e6))
    rows = sorted((int(round((seg_sec * int(lag) + float(grid[c])) * 1e6)), d, c) for d, lag in enumerate(lags) for c in range(C))
    key = np.array([r[0] for r in rows], np.float64)
    lag_of = np.array([r[1] for r in rows], np.int64)
    cls_of = np.array([r[2] for r in rows], np.int64)
    return lag_of * C + cls_of, key / step, key / 1e6, lag_of, cls_of


def _norm(logits, gate):
    """g - lse_c per (w, d), float64."""
    l = np.asarray(logits, np.float64)
    n = -lse(l, axis=2)
    if gate is not None:
        z = np.asarray(gate, np.float64)
        x = z[..., 0] - z[..., 1]
        n = n - (np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))))
    return n


def emission(logits, state_src, gate=None, row_constant=True):
    """e (W, S) float64.  row_constant=False: e minus the row constant max_d (g - lse)[w, d], added as l + (n - max n): what the path is read from - exact where the
    rows agree across the lags (n - max n = 0) - and the same path as e gives."""
    l = np.asarray(logits, np.float64)
    W, D, C = l.shape
    src = np.asarray(state_src, np.int64)
    n = _norm(l, gate)
    with np.errstate(invalid='ignore'):
        n = np.where(np.isfinite(n), n, 0.0)                                   # a lag whose row is all -inf: its states stay at -inf
    if not row_constant:
        n = n - n.max(axis=1, keepdims=True)
    return l.reshape(W, D * C)[:, src] + n[:, src // C]


def viterbi(e, pos, lam):
    """The mode of the chain from e (W, S): s_0 = e[0]; s_w[c] = max_p (s_{w-1}[p] - lam |pos[p] - pos[c]|) + e[w, c], the lowest p among the maximisers; s_w -= max
    s_w; the end state the lowest argmax -> (state_raw (W,), state_path (W,)); state_raw the lowest argmax of each row."""
    e = np.asarray(e, np.float64)
    pos = np.asarray(pos, np.float64)
    W, S = e.shape
    pen = float(lam) * np.abs(pos[:, None] - pos[None, :])                     # pen[p, c]
    s = e[0].copy()
    back = np.zeros((W, S), np.int64)
    for w in range(1, W):
        cand = s[:, None] - pen
        back[w] = cand.argmax(0)                                               # numpy: the first maximum = the lowest p
        s = cand.max(0) + e[w]
        m = s.max()
        if np.isfinite(m):
            s = s - m
    path = np.zeros(W, np.int64)
    path[W - 1] = int(s.argmax())
    for w in range(W - 1, 0, -1):
        path[w - 1] = back[w, path[w]]
    return e.argmax(1), path


def path_score(e, pos, lam, path):
    """sum_w e[w, path_w] - lam sum |pos step|, float64."""
    e = np.asarray(e, np.float64)
    pos = np.asarray(pos, np.float64)
    path = np.asarray(path, np.int64)
    return float(e[np.arange(e.shape[0]), path].sum() - float(lam) * np.abs(np.diff(pos[path])).sum())


def posterior(e, pos, lam, off, lag_of, D):
    """-> dict(post (W, S), state_post, conf_post, offset_mean (W,), p_lag (W, D), log_z):
        a_0 = e[0];          a_w[c] = e[w, c] + lse_p (a_{w-1}[p] - lam |pos[p] - pos[c]|)
        b_{W-1} = 0;         b_w[c] = lse_n (b_{w+1}[n] + e[w+1, n] - lam |pos[n] - pos[c]|)
        post = softmax_s (a + b);  offset_mean = post @ off;  p_lag[w, d] = sum of post over the states of lag d;  log_z = lse_s a_{W-1}"""
    e = np.asarray(e, np.float64)
    pos = np.asarray(pos, np.float64)
    W, S = e.shape
    pen = float(lam) * np.abs(pos[:, None] - pos[None, :])
    a = np.empty((W, S))
    b = np.empty((W, S))
    a[0] = e[0]
    for w in range(1, W):
        a[w] = e[w] + lse(a[w - 1][:, None] - pen, axis=0)
    b[W - 1] = 0.0
    for w in range(W - 2, -1, -1):
        b[w] = lse((b[w + 1] + e[w + 1])[:, None] - pen, axis=0)
    s = a + b
    post = np.exp(s - lse(s, axis=1)[:, None])
    st = post.argmax(1)
    p_lag = np.zeros((W, D))
    np.add.at(p_lag, (slice(None), np.asarray(lag_of, np.int64)), post)
    return dict(post=post, state_post=st, conf_post=post[np.arange(W), st], offset_mean=post @ np.asarray(off, np.float64), p_lag=p_lag,
                log_z=float(lse(a[W - 1])))


def brute_force(e, pos, lam):
    """Every one of the S^W paths -> (post (W, S), log_z, the best score, the best path: the lexicographically lowest among equals, read backwards - the path the
    tie rules of viterbi() pick is checked against the SCORE, not against this)."""
    e = np.asarray(e, np.float64)
    pos = np.asarray(pos, np.float64)
    W, S = e.shape
    paths = np.array(list(itertools.product(range(S), repeat=W)), np.int64)
    score = e[np.arange(W)[None, :], paths].sum(1) - float(lam) * np.abs(np.diff(pos[paths], axis=1)).sum(1)
    log_z = float(lse(score))
    with np.errstate(invalid='ignore'):
        p = np.exp(score - log_z)
    post = np.zeros((W, S))
    for w in range(W):
        np.add.at(post[w], paths[:, w], p)
    return post, log_z, float(score.max()), paths[int(score.argmax())]
