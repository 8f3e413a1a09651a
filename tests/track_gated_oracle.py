"""Float64 oracle of the read-outs gated by synchronizability (sf_track_decode_gated, sf_track_posterior_gated).  numpy only: nothing here imports
synchformer_amd.  States are j = m * C + c (c the offset class, m = 1 synchronizable); l = the offset logits (W, C), z = the gate logits (W, 2):

    d = z[w, 1] - z[w, 0];   ls = -softplus(-d);   lu = -softplus(d);   softplus(x) = max(x, 0) + log1p(exp(-|x|))
    E[w, c, 1] = ls + l[w, c] - lse_c l[w, .];     E[w, c, 0] = lu - log C                  (every row sums to 1 over the 2C states)
    T((p, m') -> (c, m)) = -lam |p - c| - mu [m' != m]
    p(j_0 .. j_{W-1})  ~  exp(sum_w E[w, j_w] + sum_{w >= 1} T(j_{w-1}, j_w))

viterbi(): the mode, the lowest predecessor state (and the lowest end state) on ties;  posterior(): the forward-backward recurrences, literally (no
renormalisation);  path_score(): the log-weight of any state path;  brute_force(): every one of the (2C)^W paths."""
import itertools

import numpy as np


def lse(x: np.ndarray, axis=None) -> np.ndarray:
    """log sum exp along `axis`: a max pass, then a sum-of-exp pass."""
    x = np.asarray(x, np.float64)
    m = x.max(axis=axis, keepdims=True)
    sub = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide='ignore'):
        out = sub + np.log(np.exp(x - sub).sum(axis=axis, keepdims=True))
    return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


def softplus(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def emission(logits: np.ndarray, gate: np.ndarray) -> np.ndarray:
    """E (W, 2C), column j = m * C + c."""
    l, z = np.asarray(logits, np.float64), np.asarray(gate, np.float64)
    W, C = l.shape
    assert z.shape == (W, 2)
    d = z[:, 1] - z[:, 0]
    e1 = -softplus(-d)[:, None] + (l - lse(l, axis=1)[:, None])
    e0 = np.repeat((-softplus(d) - np.log(C))[:, None], C, axis=1)
    return np.concatenate([e0, e1], axis=1)


def transition(C: int, lam: float, mu: float) -> np.ndarray:
    """T (2C, 2C): T[j', j], the log-weight of the step j' -> j."""
    c, m = np.arange(2 * C) % C, np.arange(2 * C) // C
    return -float(lam) * np.abs(c[:, None] - c[None, :]).astype(np.float64) - float(mu) * (m[:, None] != m[None, :])


def path_score(logits: np.ndarray, gate: np.ndarray, lam: float, mu: float, states: np.ndarray) -> float:
    """The log-weight of the state path `states` (W,) with entries j = sync * C + cls."""
    E = emission(logits, gate)
    T = transition(E.shape[1] // 2, lam, mu)
    s = np.asarray(states, np.int64)
    assert s.shape == (E.shape[0],) and s.min() >= 0 and s.max() < E.shape[1]
    return float(E[np.arange(len(s)), s].sum() + T[s[:-1], s[1:]].sum())


def viterbi(logits: np.ndarray, gate: np.ndarray, lam: float, mu: float):
    """-> dict(states (W,), cls_path, sync_path, score): S_0 = E[0]; S_w[j] = E[w, j] + max_j' (S_{w-1}[j'] + T[j', j]), the lowest j' on ties; the end state is the
    lowest state of maximal S_{W-1}; score = that maximum = path_score(states) (no renormalisation: float64 carries it)."""
    E = emission(logits, gate)
    W, S = E.shape
    C = S // 2
    T = transition(C, lam, mu)
    s = E[0].copy()
    bp = np.zeros((W, S), np.int64)
    for w in range(1, W):
        cand = s[:, None] + T
        bp[w] = cand.argmax(0)                                                   # numpy: the first maximum = the lowest predecessor state
        s = cand.max(0) + E[w]
    states = np.zeros(W, np.int64)
    states[-1] = s.argmax()
    for w in range(W - 1, 0, -1):
        states[w - 1] = bp[w, states[w]]
    return dict(states=states, cls_path=states % C, sync_path=states // C, score=float(s.max()))


def posterior(logits: np.ndarray, gate: np.ndarray, lam: float, mu: float, grid: np.ndarray):
    """-> dict(post2 (W, 2C), post (W, C), p_sync (W,), cls_post, conf_post, offset_mean (W,), log_z float):
        a_0 = E[0];          a_w[j] = E[w, j] + lse_j' (a_{w-1}[j'] + T[j', j])
        b_{W-1} = 0;         b_w[j] = lse_n (b_{w+1}[n] + E[w+1, n] + T[j, n])
        post2 = exp(a + b - lse_j (a + b));   post[w, c] = post2[w, c] + post2[w, C + c];   p_sync[w] = sum_c post2[w, C + c]
        cls_post = argmax_c post (lowest index on ties), conf_post its value;   offset_mean = post @ grid;   log_z = lse_j a_{W-1}[j]"""
    E = emission(logits, gate)
    W, S = E.shape
    C = S // 2
    grid = np.asarray(grid, np.float64)
    assert W >= 1 and grid.shape == (C,)
    T = transition(C, lam, mu)
    a, b = np.empty((W, S)), np.empty((W, S))
    a[0] = E[0]
    for w in range(1, W):
        a[w] = E[w] + lse(a[w - 1][:, None] + T, axis=0)
    b[W - 1] = 0.0
    for w in range(W - 2, -1, -1):
        b[w] = lse((b[w + 1] + E[w + 1])[None, :] + T, axis=1)
    s = a + b
    post2 = np.exp(s - lse(s, axis=1)[:, None])
    post = post2[:, :C] + post2[:, C:]
    cls = post.argmax(1)
    return dict(post2=post2, post=post, p_sync=post2[:, C:].sum(1), cls_post=cls, conf_post=post[np.arange(W), cls], offset_mean=post @ grid,
                log_z=float(lse(a[W - 1])))


def brute_force(logits: np.ndarray, gate: np.ndarray, lam: float, mu: float):
    """Every one of the (2C)^W state paths -> dict(best (the maximal path score), post2 (W, 2C), log_z)."""
    E = emission(logits, gate)
    W, S = E.shape
    T = transition(S // 2, lam, mu)
    paths = np.array(list(itertools.product(range(S), repeat=W)), np.int64)      # ((2C)^W, W)
    score = E[np.arange(W)[None, :], paths].sum(1) + T[paths[:, :-1], paths[:, 1:]].sum(1)
    log_z = float(lse(score))
    p = np.exp(score - log_z)
    post2 = np.zeros((W, S))
    for w in range(W):
        np.add.at(post2[w], paths[:, w], p)
    return dict(best=float(score.max()), post2=post2, log_z=log_z)


def ungated_viterbi(logits: np.ndarray, lam: float) -> np.ndarray:
    """The chain without the gate (sf_track_decode's recurrence in float64, lowest index on ties) -> cls_path (W,)."""
    l = np.asarray(logits, np.float64)
    e = l - l.max(1, keepdims=True)
    W, C = e.shape
    pen = float(lam) * np.abs(np.arange(C)[:, None] - np.arange(C)[None, :]).astype(np.float64)
    s = e[0].copy()
    bp = np.zeros((W, C), np.int64)
    for w in range(1, W):
        cand = s[:, None] - pen
        bp[w] = cand.argmax(0)
        s = cand.max(0) + e[w]
        s = s - s.max()
    path = np.zeros(W, np.int64)
    path[-1] = s.argmax()
    for w in range(W - 1, 0, -1):
        path[w - 1] = bp[w, path[w]]
    return path


def gap_scenario(W: int = 60, C: int = 21, gap=(22, 37), cls: int = 13, decoy: int = 2, vote: float = 6.0, d: float = 6.0):
    """The scenario of DESIGN 3.20: W windows voting `cls` with a +vote logit, the windows [gap) voting `decoy` instead (a music bed: confident and wrong); the gate
    says synchronizable (+d) outside the gap and not (-d) inside -> (logits (W, C), gate_logits (W, 2))."""
    l = np.zeros((W, C))
    l[:, cls] = vote
    l[gap[0]:gap[1], cls] = 0.0
    l[gap[0]:gap[1], decoy] = vote
    z = np.zeros((W, 2))
    z[:, 1] = d
    z[gap[0]:gap[1], 1] = -d
    return l, z
