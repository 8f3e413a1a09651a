"""Float64 oracle of the pairwise read-out of a recording's offset track (sf_track_pairwise, sf_track_pairwise_gated).  numpy only: nothing here imports
synchformer_amd.  The chains are those of tests/track_posterior_oracle.py (plain, C classes) and tests/track_gated_oracle.py (2C states j = m * C + c); per boundary
w = 0 .. W - 2, with a, b the forward / backward scans and S the log-weight of a step,

    t[j', j] = a_w[j'] + S[j', j] + E[w+1, j] + b_{w+1}[j];        xi2[w, j', j] = exp(t[j', j] - lse_{j',j} t) = P(state_w = j', state_{w+1} = j | all windows)

pairwise() / pairwise_gated(): the contract, literally (no renormalisation: float64 carries W = 4096);  brute_force(): every path, summed;  sample_path(): one draw
from the chain by forward filtering and backward sampling (the labels a fit of lam / mu is tested on)."""
import itertools

import numpy as np

import track_gated_oracle as TG
import track_posterior_oracle as TP

lse = TP.lse


def _plain_chain(logits, lam):
    """-> (E (W, C), S (C, C)): emissions and step log-weights of the plain chain."""
    E = TP.log_softmax(logits)
    C = E.shape[1]
    return E, -float(lam) * np.abs(np.arange(C)[:, None] - np.arange(C)[None, :]).astype(np.float64)


def _scans(E, S):
    """a_0 = E[0];  a_w[j] = E[w, j] + lse_j' (a_{w-1}[j'] + S[j', j]);  b_{W-1} = 0;  b_w[j] = lse_n (b_{w+1}[n] + E[w+1, n] + S[j, n])."""
    W = E.shape[0]
    a, b = np.empty_like(E), np.empty_like(E)
    a[0] = E[0]
    for w in range(1, W):
        a[w] = E[w] + lse(a[w - 1][:, None] + S, axis=0)
    b[W - 1] = 0.0
    for w in range(W - 2, -1, -1):
        b[w] = lse((b[w + 1] + E[w + 1])[None, :] + S, axis=1)
    return a, b


def _state_pairs(E, S):
    """-> (xi2 (W-1, n, n), log_z): the pair marginals over the chain's own states."""
    a, b = _scans(E, S)
    t = a[:-1, :, None] + S[None] + (E[1:] + b[1:])[:, None, :]                            # a masked (-inf) end gives -inf: only sums, no difference of infinities
    n = E.shape[1]
    z = lse(t.reshape(t.shape[0], n * n), axis=1) if t.shape[0] else np.zeros(0)
    return np.exp(t - z[:, None, None]), float(lse(a[-1]))


def _class_outputs(xi, log_z):
    """The outputs the contract derives from the class-pair marginal xi (W-1, C, C)."""
    n, C = xi.shape[0], xi.shape[1]
    dist = np.abs(np.arange(C)[:, None] - np.arange(C)[None, :]).astype(np.float64)
    offd = dist > 0
    masked = np.where(offd[None], xi, -1.0).reshape(n, C * C)
    top = masked.argmax(1) if n else np.zeros(0, np.int64)                                 # numpy: the first maximum = the lowest p, then the lowest c
    return dict(xi=xi, p_change=(xi * offd[None]).sum((1, 2)), jump_abs=(xi * dist[None]).sum((1, 2)), top_from=top // C, top_to=top % C,
                p_top=masked[np.arange(n), top] if n else np.zeros(0), log_z=log_z)


def pairwise(logits: np.ndarray, lam: float):
    """-> dict(xi (W-1, C, C), p_change, jump_abs, p_top (W-1,) float64, top_from, top_to (W-1,) int64, log_z float):
        xi[w, p, c] = exp(t - lse t),  t[p, c] = a_w[p] - lam |p - c| + e[w+1, c] + b_{w+1}[c];     p_change = sum_{p != c} xi;     jump_abs = sum xi |p - c|
        (top_from, top_to) = the off-diagonal pair of largest xi (the lowest p, then the lowest c on ties), p_top its mass."""
    E, S = _plain_chain(logits, lam)
    return _class_outputs(*_state_pairs(E, S))


def pairwise_gated(logits: np.ndarray, gate: np.ndarray, lam: float, mu: float):
    """The same over the states (p, m') -> (c, m) with TG.emission and TG.transition -> pairwise()'s dict from the class-pair marginal (both flags summed out), plus
    p_flip (W-1,): the mass with m' != m, and xi2 (W-1, 2C, 2C)."""
    E = TG.emission(logits, gate)
    C = E.shape[1] // 2
    xi2, log_z = _state_pairs(E, TG.transition(C, lam, mu))
    out = _class_outputs(xi2[:, :C, :C] + xi2[:, :C, C:] + xi2[:, C:, :C] + xi2[:, C:, C:], log_z)
    out.update(p_flip=xi2[:, :C, C:].sum((1, 2)) + xi2[:, C:, :C].sum((1, 2)), xi2=xi2)
    return out


def brute_force(logits: np.ndarray, lam: float, gate: np.ndarray = None, mu: float = 0.0):
    """Every path of the plain chain (gate None) or of the gated chain -> (xi2 (W-1, n, n) over the chain's own states, log_z)."""
    E, S = _plain_chain(logits, lam) if gate is None else (TG.emission(logits, gate), TG.transition(np.shape(logits)[1], lam, mu))
    W, n = E.shape
    paths = np.array(list(itertools.product(range(n), repeat=W)), np.int64)
    score = E[np.arange(W)[None, :], paths].sum(1) + S[paths[:, :-1], paths[:, 1:]].sum(1)
    log_z = float(lse(score))
    p = np.exp(score - log_z)
    xi2 = np.zeros((W - 1, n, n))
    for w in range(W - 1):
        np.add.at(xi2[w], (paths[:, w], paths[:, w + 1]), p)
    return xi2, log_z


def sample_path(rng: np.random.Generator, logits: np.ndarray, lam: float, gate: np.ndarray = None, mu: float = 0.0) -> np.ndarray:
    """One path (W,) int64 drawn from the chain (states j = m * C + c with a gate): the forward scan, then state_{W-1} ~ softmax(a_{W-1}) and
    state_w ~ softmax_j' (a_w[j'] + S[j', state_{w+1}]) backwards."""
    E, S = _plain_chain(logits, lam) if gate is None else (TG.emission(logits, gate), TG.transition(np.shape(logits)[1], lam, mu))
    W, n = E.shape
    a = np.empty_like(E)
    a[0] = E[0]
    for w in range(1, W):
        a[w] = E[w] + lse(a[w - 1][:, None] + S, axis=0)
    path = np.empty(W, np.int64)

    def draw(s):
        p = np.exp(s - lse(s))
        return int(rng.choice(n, p=p / p.sum()))

    path[W - 1] = draw(a[W - 1])
    for w in range(W - 2, -1, -1):
        path[w] = draw(a[w] + S[:, path[w + 1]])
    return path
