"""Float64 oracle of the posterior (forward-backward) read-out of a recording's window logits (sf_track_posterior).  numpy only: nothing here
imports synchformer_amd.  Two independent statements of the same chain

    p(c_0 .. c_{W-1})  ~  exp(sum_w e[w, c_w] - lam sum_{w >= 1} |c_w - c_{w-1}|),        e[w, c] = logits[w, c] - lse_c logits[w, .]

posterior(): the recurrences of the contract, literally (no renormalisation: float64 carries W = 4096 with 1e-12 to spare);
brute_force(): every one of the C^W paths, summed."""
import itertools

import numpy as np


def lse(x: np.ndarray, axis=None) -> np.ndarray:
    """log sum exp along `axis`: a max pass, then a sum-of-exp pass; -inf where every entry is -inf (the guard of (-inf) - (-inf))."""
    x = np.asarray(x, np.float64)
    m = x.max(axis=axis, keepdims=True)
    sub = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide='ignore'):
        out = sub + np.log(np.exp(x - sub).sum(axis=axis, keepdims=True))
    return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


def log_softmax(logits: np.ndarray) -> np.ndarray:
    l = np.asarray(logits, np.float64)
    return l - lse(l, axis=1)[:, None]


def posterior(logits: np.ndarray, lam: float, grid: np.ndarray):
    """-> dict(post (W, C), cls_post (W,), conf_post (W,), offset_mean (W,), log_z float), all float64 / int64.
        a_0 = e[0];          a_w[c] = e[w, c] + lse_p (a_{w-1}[p] - lam |p - c|)
        b_{W-1} = 0;         b_w[c] = lse_n (b_{w+1}[n] + e[w+1, n] - lam |n - c|)
        post[w, c] = exp(a_w[c] + b_w[c] - lse_c (a_w + b_w));   cls_post = argmax_c post (lowest index on ties), conf_post its value
        offset_mean[w] = sum_c post[w, c] grid[c];               log_z = lse_c a_{W-1}[c]"""
    e = log_softmax(logits)
    W, C = e.shape
    grid = np.asarray(grid, np.float64)
    assert W >= 1 and grid.shape == (C,)
    pen = float(lam) * np.abs(np.arange(C)[:, None] - np.arange(C)[None, :]).astype(np.float64)       # pen[p, c]
    a = np.empty((W, C))
    b = np.empty((W, C))
    a[0] = e[0]
    for w in range(1, W):
        a[w] = e[w] + lse(a[w - 1][:, None] - pen, axis=0)
    b[W - 1] = 0.0
    for w in range(W - 2, -1, -1):
        b[w] = lse((b[w + 1] + e[w + 1])[:, None] - pen, axis=0)
    s = a + b
    post = np.exp(s - lse(s, axis=1)[:, None])
    cls = post.argmax(1)                                                                              # numpy: the first maximum
    return dict(post=post, cls_post=cls, conf_post=post[np.arange(W), cls], offset_mean=post @ grid, log_z=float(lse(a[W - 1])))


def brute_force(logits: np.ndarray, lam: float):
    """Marginals and log_z by enumeration of all C^W paths -> (post (W, C), log_z)."""
    e = log_softmax(logits)
    W, C = e.shape
    paths = np.array(list(itertools.product(range(C), repeat=W)), np.int64)                           # (C^W, W)
    score = e[np.arange(W)[None, :], paths].sum(1) - float(lam) * np.abs(np.diff(paths, axis=1)).sum(1)
    log_z = float(lse(score))
    p = np.exp(score - log_z)
    post = np.zeros((W, C))
    for w in range(W):
        np.add.at(post[w], paths[:, w], p)
    return post, log_z
