"""GPU: the wide chain (sf_track_decode_wide / sf_track_posterior_wide) against the float64 oracle of tests/track_wide_oracle.py: exactness on
dyadic inputs (ties included), the reduction to the plain chain, float inputs within measured bars, identities, the engine's lagged windows and the tracker.

THE BARS ARE MEASURED, as tests/test_track_posterior_gpu.py measures its own.  The yardstick is the contract's O(S^2) recurrences, literally, in torch fp32 on the
CPU (_yard_posterior, _yard_viterbi below), compared with the float64 oracle on the very inputs a test uses; per quantity

    post:   max |post - oracle|                       mean:   max |offset_mean - oracle| / grid step          p_lag:  max |p_lag - oracle|
    log_z:  |log_z - oracle| / max(1, |oracle|)       path:   (the oracle's optimum - the float64 score of the returned path) / max(1, |optimum|)

the kernel may be at most 4x the yardstick's worst value over the inputs of this file that carry a bar - the float inputs and the reduction inputs (computed once,
in `refs`) - with an absolute floor of 1e-6 for post and p_lag.  CEIL holds a fixed ceiling per quantity - those worst values rounded up to one digit - and the yardstick counts with at most its ceiling, so the bars cannot
float with the CPU's libm.  The yardstick's worst post / mean / p_lag come from W = 4096 (it does not renormalise), its worst log_z from the reduction inputs (one
lag, W = 300, lam = 0: log_z = 0 is small against the scores it is the lse of), its worst path from one near-tie; on most inputs it finds the float64 optimum itself.
state_post is compared wherever the oracle's two largest marginals differ by more than the post bar; on the float inputs those windows are fewer than 1 % (asserted;
the integer logits of the reduction inputs tie on purpose).

One identity of the issue is NOT asserted as stated: 'log_z <= log D without a gate'.  Every window's emissions sum to D over the states (one softmax per lag), so
Z <= D^W with equality at lam = 0 (the oracle and the brute force of tests/test_track_wide_cpu.py show it); the bound that holds, log_z <= W log D, is asserted."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_wide_oracle as TW  # noqa: E402

pytestmark = pytest.mark.gpu

QUANT = ('post', 'mean', 'p_lag', 'log_z', 'path')
# the yardstick's worst (post, mean in grid steps, p_lag, log_z, path) over the float inputs below, rounded up to one digit (measured: see DESIGN 3.24)
CEIL = (4e-4, 5e-3, 4e-4, 7e-6, 8e-11)         # measured 3.99e-4, 4.37e-3, 3.98e-4, 6.68e-6, 7.2e-11


# ---- tables -------------------------------------------------------------------------------------------------------------------------------------------------
def _lag_tables(D: int, C: int = 21):
    """The states of D lags centred on 0 over the default grid, as ops.track_wide_states makes them (fp32 tables: the oracle reads the same numbers)."""
    from synchformer_amd import ops
    from synchformer_amd.postprocess import class_grid
    lags = tuple(range(-(D // 2), D - D // 2))
    src, pos, off, lag_of, cls_of = ops.track_wide_states(lags, class_grid(-2, 2, C))
    return dict(D=D, C=C, src=src, pos=pos, off=off, lag_of=lag_of.numpy().astype(np.int64), step=0.2)


def _plain_tables(C: int):
    """One lag, pos = arange(C), the classes on linspace(-2, 2, C): the plain chain of ops.track_decode / ops.track_posterior as a wide one."""
    return dict(D=1, C=C, src=torch.arange(C, dtype=torch.int32), pos=torch.arange(C, dtype=torch.float32), off=torch.linspace(-2, 2, C),
                lag_of=np.zeros(C, np.int64), step=4.0 / (C - 1))


def _dev_tables(gpu, t: dict):
    from synchformer_amd import ops
    return ops.track_wide_tables(t['src'], t['pos'], t['off'], t['D'], t['C'], gpu)


# ---- the yardsticks: the contract's recurrences in torch fp32 on the CPU ---------------------------------------------------------------------------------------
def _lse32(x: torch.Tensor, dim: int) -> torch.Tensor:
    m = x.max(dim, keepdim=True).values
    sub = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    return (sub + torch.log(torch.exp(x - sub).sum(dim, keepdim=True))).squeeze(dim)


def _emission32(x: np.ndarray, z, t: dict) -> torch.Tensor:
    l = torch.from_numpy(x)
    assert l.dtype == torch.float32
    n = -_lse32(l, 2)
    if z is not None:
        n = n - torch.nn.functional.softplus(torch.from_numpy(z)[..., 0] - torch.from_numpy(z)[..., 1])
    n = torch.where(torch.isfinite(n), n, torch.zeros_like(n))
    src = t['src'].long()
    return l.reshape(l.shape[0], -1)[:, src] + n[:, src // t['C']]


def _yard_posterior(x, z, t: dict, lam: float):
    e = _emission32(x, z, t)
    W, S = e.shape
    pos, off = t['pos'], t['off']
    pen = torch.tensor(lam, dtype=torch.float32) * (pos[:, None] - pos[None, :]).abs()
    a, b = torch.empty(W, S), torch.empty(W, S)
    a[0] = e[0]
    for w in range(1, W):
        a[w] = e[w] + _lse32(a[w - 1][:, None] - pen, 0)
    b[W - 1] = 0
    for w in range(W - 2, -1, -1):
        b[w] = _lse32((b[w + 1] + e[w + 1])[:, None] - pen, 0)
    s = a + b
    post = torch.exp(s - _lse32(s, 1)[:, None])
    p_lag = torch.zeros(W, t['D']).index_add_(1, torch.from_numpy(t['lag_of']), post)
    return dict(post=post.numpy(), offset_mean=(post @ off).numpy(), p_lag=p_lag.numpy(), log_z=float(_lse32(a[W - 1], 0)))


def _yard_viterbi(x, z, t: dict, lam: float) -> np.ndarray:
    e = _emission32(x, z, t)
    W, S = e.shape
    pos = t['pos']
    pen = torch.tensor(lam, dtype=torch.float32) * (pos[:, None] - pos[None, :]).abs()
    s = e[0].clone()
    back = torch.zeros(W, S, dtype=torch.int64)
    for w in range(1, W):
        best, back[w] = (s[:, None] - pen).max(0)
        s = best + e[w]
        s = s - s.max()
    path = [int(s.argmax())]
    for w in range(W - 1, 0, -1):
        path.append(int(back[w, path[-1]]))
    return np.array(path[::-1])


def _errors(got: dict, ref: dict, step: float, rows=None):
    """(post, mean, p_lag, log_z) errors of `got` against the float64 `ref`; rows: compare only these windows."""
    sel = slice(None) if rows is None else rows
    return (float(np.abs(got['post'].astype(np.float64) - ref['post'])[sel].max()),
            float(np.abs(got['offset_mean'].astype(np.float64) - ref['offset_mean'])[sel].max()) / step,
            float(np.abs(got['p_lag'].astype(np.float64) - ref['p_lag'])[sel].max()),
            abs(float(got['log_z']) - ref['log_z']) / max(1.0, abs(ref['log_z'])))


def _deficit(case: dict, path: np.ndarray) -> float:
    return (case['best'] - TW.path_score(case['e'], case['pos64'], case['lam'], path)) / max(1.0, abs(case['best']))


# ---- the float inputs: made once, with their oracle and yardstick, and never changed ----------------------------------------------------------------------------
def _randn(seed: int, shape, scale: float) -> np.ndarray:
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def _float_case(seed, D, W, lam, scale, gate):
    return dict(x=_randn(seed, (W, D, 21), scale), z=_randn(seed + 1, (W, D, 2), 2.0) if gate else None, D=D, lam=lam)


def _masked_case():
    c = _float_case(31, 3, 40, 1.0, 3.0, False)
    c['x'][:, 1, 4] = -np.inf                                                    # a state masked in every window
    c['x'][5:17, 0, 11] = -np.inf                                                # and one masked in some
    c['x'][33, 2, :] = -np.inf                                                   # and a whole lag of one window
    return c


# every listed value of (D, C), W, lam, the scale and the gate occurs; the large S = 1008 meets W = 300 once (its O(S^2) float64 reference is the slow one)
_INPUTS = {
    ('f', 3, 9, 0.0, 3.0, False): _float_case(101, 3, 9, 0.0, 3.0, False),
    ('f', 3, 300, 1.0, 3.0, True): _float_case(102, 3, 300, 1.0, 3.0, True),
    ('f', 3, 300, 8.0, 50.0, False): _float_case(103, 3, 300, 8.0, 50.0, False),
    ('f', 3, 300, 0.0, 50.0, True): _float_case(104, 3, 300, 0.0, 50.0, True),
    ('f', 25, 9, 8.0, 50.0, True): _float_case(105, 25, 9, 8.0, 50.0, True),
    ('f', 25, 300, 1.0, 3.0, False): _float_case(106, 25, 300, 1.0, 3.0, False),
    ('f', 25, 9, 0.0, 3.0, True): _float_case(107, 25, 9, 0.0, 3.0, True),
    ('f', 48, 9, 1.0, 3.0, True): _float_case(108, 48, 9, 1.0, 3.0, True),
    ('f', 48, 9, 8.0, 50.0, False): _float_case(109, 48, 9, 8.0, 50.0, False),
    ('f', 48, 300, 8.0, 3.0, False): _float_case(111, 48, 300, 8.0, 3.0, False),
    ('f', 3, 300, 0.0, 3.0, False): _float_case(112, 3, 300, 0.0, 3.0, False),     # lam = 0 without a gate: log_z reaches W log D
    ('f', 25, 300, 8.0, 3.0, True): _float_case(113, 25, 300, 8.0, 3.0, True),
    ('f', 25, 300, 1.0, 50.0, True): _float_case(114, 25, 300, 1.0, 50.0, True),    # 50 * randn along 300 windows at many lags: where an underflow in the lse scans would show
    ('f', 48, 300, 8.0, 50.0, True): _float_case(115, 48, 300, 8.0, 50.0, True),
    # lam = 0 at 48 lags, with a gate: without one the windows are independent softmaxes spread over 48 lags, whose two largest marginals (a few 1e-2 each) lie
    # closer than the post bar in most windows - the 1 % cap on undecided windows below does not admit that input at W = 300
    ('f', 48, 9, 0.0, 3.0, True): _float_case(110, 48, 9, 0.0, 3.0, True),
    ('strided',): _float_case(41, 3, 130, 0.5, 3.0, True),
    ('drift',): _float_case(42, 3, 4096, 1.0, 3.0, False),
    ('masked',): _masked_case(),
}
FLOAT_KEYS = [k for k in _INPUTS if k[0] == 'f']


def _plain_case(C: int, W: int, lam: float):
    """An exactness input of the reduction to the plain chain: integer logits in [-8, 8], one lag."""
    return dict(x=np.random.default_rng(50 * C + W).integers(-8, 9, (W, 1, C)).astype(np.float32), z=None, D=1, lam=lam, t=_plain_tables(C))


PLAIN_KEYS = [('plain', C, W, lam) for C in (2, 21, 64) for W in (1, 2, 9, 300) for lam in (0.0, 0.5, 1.0, 4.0)]
_INPUTS.update({k: _plain_case(*k[1:]) for k in PLAIN_KEYS})                     # the yardstick runs on these too: they are inputs of this file


def _make_refs():
    out, tabs = {}, {}
    for key, c in _INPUTS.items():
        t = c['t'] if 't' in c else tabs.setdefault(c['D'], _lag_tables(c['D']))
        pos64, off64 = t['pos'].double().numpy(), t['off'].double().numpy()
        x64 = c['x'].astype(np.float64)
        z64 = None if c['z'] is None else c['z'].astype(np.float64)
        e = TW.emission(x64, t['src'].numpy(), z64)
        ref = TW.posterior(e, pos64, c['lam'], off64, t['lag_of'], c['D'])
        case = dict(c, t=t, e=e, pos64=pos64, ref=ref)
        case['raw'], case['path'] = TW.viterbi(TW.emission(x64, t['src'].numpy(), z64, row_constant=False), pos64, c['lam'])
        case['best'] = TW.path_score(e, pos64, c['lam'], case['path'])
        case['yard'] = _errors(_yard_posterior(c['x'], c['z'], t, c['lam']), ref, t['step']) + (_deficit(case, _yard_viterbi(c['x'], c['z'], t, c['lam'])),)
        out[key] = case
    worst = [max(v['yard'][q] for v in out.values()) for q in range(5)]
    print('yardstick worst: ' + '  '.join(f'{n} {w:.3e}' for n, w in zip(QUANT, worst)) + f' (ceilings {CEIL})')
    worst = [min(w, c) for w, c in zip(worst, CEIL)]                                                 # the bars do not float
    out['bar'] = (max(4 * worst[0], 1e-6), 4 * worst[1], max(4 * worst[2], 1e-6), 4 * worst[3], 4 * worst[4])
    return out


@pytest.fixture(scope='module')
def refs():
    """key -> the case with its tables, float64 oracle (posterior, optimum) and the yardstick's errors; 'bar' -> the bar per quantity."""
    return _make_refs()


def _dev3(gpu, a: np.ndarray, ld):
    """a (W, D, K) on the device; ld = (row stride, lag stride) of a strided view whose padding holds a value that would win every maximum."""
    if ld is None:
        return torch.from_numpy(a).to(gpu)
    W, D, K = a.shape
    assert ld[1] >= K and ld[0] >= D * ld[1]
    buf = torch.full((W, ld[0]), 1e30, device=gpu, dtype=torch.float32)
    view = buf.as_strided((W, D, K), (ld[0], ld[1], 1))
    view.copy_(torch.from_numpy(a).to(gpu))
    return view


def _run(gpu, x, z, tables, lam, ld=None, ldg=None, ldp=None, posterior=True):
    from synchformer_amd import ops
    W, S, D = x.shape[0], tables.S, tables.D
    xd = _dev3(gpu, x, ld)
    zd = None if z is None else _dev3(gpu, z, ldg)
    dec = ops.track_decode_wide(xd, tables, lam, zd)
    assert [t.dtype for t in dec] == [torch.int32, torch.float32, torch.int32, torch.float32] and all(t.shape == (W,) for t in dec)
    got = dict(zip(('state_raw', 'conf_raw', 'state_path', 'conf_path'), (t.cpu().numpy() for t in dec)))
    if posterior:
        pbuf = None if ldp is None else torch.full((W, ldp), -7.0, device=gpu, dtype=torch.float32)
        out = ops.track_posterior_wide(xd, tables, lam, zd, post=None if pbuf is None else pbuf[:, :S])
        post, state_post, conf_post, mean, p_lag, log_z = out
        assert [t.dtype for t in out] == [torch.float32, torch.int32, torch.float32, torch.float32, torch.float32, torch.float32]
        assert post.shape == (W, S) and state_post.shape == conf_post.shape == mean.shape == (W,) and p_lag.shape == (W, D) and log_z.shape == (1,)
        if pbuf is not None:
            assert (pbuf[:, S:] == -7.0).all(), 'the padding of post was written'
        got.update(post=post.cpu().numpy(), state_post=state_post.cpu().numpy(), conf_post=conf_post.cpu().numpy(), offset_mean=mean.cpu().numpy(),
                   p_lag=p_lag.cpu().numpy(), log_z=float(log_z.item()))
    torch.cuda.synchronize()
    return got


def _check(got: dict, case: dict, bar, rows=None, what=''):
    """Errors within the bars; the path's float64 score within its bar of the optimum; rows of post and p_lag sum to 1; conf_post is post at state_post; state_post is
    the oracle's argmax wherever that is decided by more than the bar; log_z <= W log D without a gate."""
    ref, (W, D, _) = case['ref'], case['x'].shape
    S = case['e'].shape[1]
    err = _errors(got, ref, case['t']['step'], rows) + (_deficit(case, got['state_path']),)
    print(f'{what} lam {case["lam"]}: ' + '  '.join(f'{n} {e:.3e} (yardstick {y:.3e}, bar {b:.3e})' for n, e, y, b in zip(QUANT, err, case['yard'], bar)))
    sel = np.arange(W) if rows is None else rows
    assert all(np.isfinite(got[k]).all() for k in ('post', 'conf_post', 'offset_mean', 'p_lag', 'conf_raw', 'conf_path')) and np.isfinite(got['log_z'])
    assert all(e <= b for e, b in zip(err, bar)), (err, bar)
    assert err[4] >= -1e-9, 'a path above the optimum'
    for k in ('state_raw', 'state_path', 'state_post'):
        assert got[k].min() >= 0 and got[k].max() < S, k
    assert np.abs(got['post'].sum(1) - 1)[sel].max() <= 1e-5 and np.abs(got['p_lag'].sum(1) - 1)[sel].max() <= 1e-5
    if case['z'] is None:
        assert got['log_z'] <= W * math.log(D) + bar[3] * max(1.0, W * math.log(D))
    assert np.array_equal(got['conf_post'], got['post'][np.arange(W), got['state_post']])
    top = np.sort(ref['post'], 1)
    decided = (top[:, -1] - top[:, -2] > bar[0])[sel]
    assert np.array_equal(got['state_post'][sel][decided], ref['state_post'][sel][decided])
    # the raw read-out: the oracle's argmax wherever its two largest emissions differ by more than fp32 resolves, and the softmax probabilities over all S states
    es = np.sort(case['e'], 1)
    clear = (es[:, -1] - es[:, -2] > 1e-5 * np.maximum(1.0, np.abs(es[:, -1])))[sel]
    assert np.array_equal(got['state_raw'][sel][clear], case['raw'][sel][clear])
    with np.errstate(invalid='ignore'):
        p = np.exp(case['e'] - case['e'].max(1, keepdims=True))
    p = p / p.sum(1, keepdims=True)
    tol = 2e-6 + 8 * 2.0 ** -24 * np.abs(case['e'][np.isfinite(case['e'])]).max()     # a probability's error is that of its exponent: a few fp32 roundings of |e|
    assert np.abs(got['conf_raw'] - p[np.arange(W), got['state_raw']])[sel].max() <= tol
    assert np.abs(got['conf_path'] - p[np.arange(W), got['state_path']])[sel].max() <= tol


def test_argmax_is_decided_in_the_oracle(refs):
    """Fewer than 1 % of the windows have the oracle's two largest marginals closer than the post bar: the state_post check covers the rest."""
    close = total = 0
    for key, case in refs.items():
        if key == 'bar' or key[0] == 'plain':                                    # (integer logits tie on purpose)
            continue
        top = np.sort(case['ref']['post'], 1)
        close += int((top[:, -1] - top[:, -2] <= refs['bar'][0]).sum())
        total += top.shape[0]
    print(f'{close} of {total} windows undecided at the bar')
    assert close < 0.01 * total


@pytest.mark.parametrize('key', FLOAT_KEYS, ids=lambda k: f'D{k[1]}-W{k[2]}-lam{k[3]}-x{k[4]}-{"gate" if k[5] else "plain"}')
def test_float_inputs_against_oracle(gpu, refs, key):
    case = refs[key]
    tables = _dev_tables(gpu, case['t'])
    got = _run(gpu, case['x'], case['z'], tables, case['lam'])
    _check(got, case, refs['bar'], what=str(key))
    flipped = _run(gpu, case['x'][::-1].copy(), None if case['z'] is None else case['z'][::-1].copy(), tables, case['lam'])
    assert np.abs(flipped['post'][::-1] - got['post']).max() <= 2 * refs['bar'][0]                      # reversed rows: reversed marginals, the same partition sum
    assert abs(flipped['log_z'] - got['log_z']) <= 2 * refs['bar'][3] * max(1.0, abs(case['ref']['log_z']))


def test_strided_equals_dense(gpu, refs):
    """Row and lag strides above the dense ones for logits and gate logits (the padding would win every maximum if read) and a post of row stride S + 5 (its padding
    stays as it was): within the bars, and bit-equal to the dense call."""
    case = refs[('strided',)]
    tables = _dev_tables(gpu, case['t'])
    got = _run(gpu, case['x'], case['z'], tables, case['lam'], ld=(3 * 24 + 7, 24), ldg=(11, 3), ldp=case['e'].shape[1] + 5)
    _check(got, case, refs['bar'], what='strided')
    dense = _run(gpu, case['x'], case['z'], tables, case['lam'])
    assert all(np.array_equal(got[k], dense[k]) for k in got if k != 'log_z') and got['log_z'] == dense['log_z']


def test_does_not_drift(gpu, refs):
    """W = 4096: the per-step renormalisation keeps the scores bounded, the double accumulator keeps log_z to fp32 precision, the staged backtrace walks 4096 rows."""
    case = refs[('drift',)]
    _check(_run(gpu, case['x'], case['z'], _dev_tables(gpu, case['t']), case['lam']), case, refs['bar'], what='W 4096')


def test_masked_states(gpu, refs):
    case = refs[('masked',)]
    got = _run(gpu, case['x'], case['z'], _dev_tables(gpu, case['t']), case['lam'])
    _check(got, case, refs['bar'], what='masked')
    masked = np.isneginf(case['e'])
    assert masked.any(0).sum() >= 23 and masked.all(0).sum() == 1
    assert (got['post'][masked] == 0).all() and not masked[np.arange(masked.shape[0]), got['state_path']].any()


def test_non_finite_rows_stay_in_range(gpu):
    """A row of NaN and a row with +inf: values are unspecified, the calls return and every index written lies in [0, S)."""
    t = _lag_tables(3)
    x = _randn(3, (40, 3, 21), 3.0)
    x[11] = np.nan
    x[23, 1, 5] = np.inf
    got = _run(gpu, x, None, _dev_tables(gpu, t), 1.0)
    for k in ('state_raw', 'state_path', 'state_post'):
        assert got[k].shape == (40,) and got[k].min() >= 0 and got[k].max() < 63, (k, got[k])


def test_no_windows_and_rejections(gpu):
    from synchformer_amd import ops
    t = _lag_tables(3)
    tables = _dev_tables(gpu, t)
    dec = ops.track_decode_wide(torch.empty(0, 3, 21, device=gpu), tables, 1.0)
    post, state_post, conf_post, mean, p_lag, log_z = ops.track_posterior_wide(torch.empty(0, 3, 21, device=gpu), tables, 1.0)
    torch.cuda.synchronize()
    assert all(x.shape == (0,) for x in dec) and post.shape == (0, 63) and p_lag.shape == (0, 3) and log_z.shape == (1,) and log_z.item() == 0
    with pytest.raises(AssertionError):
        ops.track_decode_wide(torch.zeros(3, 2, 21, device=gpu), tables, 1.0)                           # logits of another number of lags
    with pytest.raises(RuntimeError, match='lam must be finite'):
        ops.track_decode_wide(torch.zeros(3, 3, 21, device=gpu), tables, -1.0)
    bad = ops.track_wide_tables(t['src'], t['pos'].flip(0), t['off'], 3, 21, gpu)
    with pytest.raises(RuntimeError, match='ascending'):
        ops.track_posterior_wide(torch.zeros(3, 3, 21, device=gpu), bad, 1.0)
    with pytest.raises(ValueError):
        ops.track_wide_tables(torch.arange(1025, dtype=torch.int32), torch.zeros(1025), torch.zeros(1025), 17, 64, gpu)


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------------------------
def _exact_tables(S: int, seed: int):
    """S states over D = ceil(S / C) lags of C classes in a random order, at dyadic positions with repeats.  (C = 2 for S = 2, else 64.)"""
    rng = np.random.default_rng(seed)
    C = 2 if S == 2 else 64
    D = -(-S // C)
    src = rng.permutation(D * C)[:S].astype(np.int32)
    pos = np.cumsum(rng.choice([0.0, 0.0, 0.5, 1.0, 1.5], S)).astype(np.float32)
    return dict(D=D, C=C, src=torch.from_numpy(src), pos=torch.from_numpy(pos), off=torch.from_numpy(0.2 * pos), lag_of=(src // C).astype(np.int64))


def _exact_logits(W: int, t: dict, seed: int) -> np.ndarray:
    """Integer logits in [-8, 8], every window's row the same at every lag: the emission's normalisation is one constant per window, which the path does not see, and
    every operation of the scan is exact in fp32 (scores are multiples of 1/8 bounded by 8 + 4 x the span of the positions)."""
    row = np.random.default_rng(seed).integers(-8, 9, (W, 1, t['C'])).astype(np.float32)
    return np.repeat(row, t['D'], axis=1)


def _expect_exact(gpu, x: np.ndarray, t: dict, lam: float):
    e = TW.emission(x.astype(np.float64), t['src'].numpy(), row_constant=False)
    assert np.array_equal(e, np.round(e)), 'the emission is not the integer logit'
    raw, path = TW.viterbi(e, t['pos'].double().numpy(), lam)
    got = _run(gpu, x, None, _dev_tables(gpu, t), lam, posterior=False)
    assert np.array_equal(got['state_raw'], raw), np.nonzero(got['state_raw'] != raw)
    assert np.array_equal(got['state_path'], path), np.nonzero(got['state_path'] != path)
    return got


@pytest.mark.parametrize('lam', [0.0, 0.5, 1.0, 4.0])
@pytest.mark.parametrize('W', [1, 2, 9, 300])
@pytest.mark.parametrize('S', [2, 63, 64, 65, 130, 1024])
def test_exact_on_dyadic_inputs(gpu, S, W, lam):
    t = _exact_tables(S, 1000 + S)
    _expect_exact(gpu, _exact_logits(W, t, 7 * S + W + int(2 * lam)), t, lam)


def test_ties_across_a_wave_boundary(gpu):
    """S = 130 (three wavefronts).  (a) Flat logits: every predecessor ties at every step, state 0 wins everywhere, through the carries of both later waves.
    (b) States 63 and 64 - the last lane of wave 0 and the first of wave 1 - share a position and hold the only large logit of row 0, row 1 is flat and row 2 votes for
    state 100: every state from 63 to 100 ties as the predecessor of 100 (the cost of the detour is the same) and the lowest, 63, must win: the carry from wave 0
    against wave 1's own prefix; then 63 ties with 64 as its own predecessor: the prefix half against the suffix half."""
    S, C = 130, 64
    pos = 0.5 * np.arange(S, dtype=np.float32)
    pos[64:] -= 0.5                                                              # pos[63] == pos[64]
    t = dict(D=3, C=C, src=torch.arange(S, dtype=torch.int32), pos=torch.from_numpy(pos), off=torch.from_numpy(0.2 * pos), lag_of=np.arange(S) // C)
    for lam in (0.0, 1.0):
        got = _expect_exact(gpu, np.zeros((9, 3, C), np.float32), t, lam)
        assert (got['state_path'] == 0).all() and (got['state_raw'] == 0).all()
    # (b): the rows agree across the lags (so the emission is exact) and state_src gives class 1 to states 63 and 64 alone, class 2 to state 100 alone
    src = np.zeros(S, np.int64)
    others = [d * C + c for c in [0] + list(range(3, C)) for d in range(3)]          # 186 pairs of the classes 0, 3 .. 63
    src[[63, 64, 100]] = [0 * C + 1, 1 * C + 1, 1 * C + 2]
    src[[s for s in range(S) if s not in (63, 64, 100)]] = others[:S - 3]
    t = dict(t, src=torch.from_numpy(src.astype(np.int32)), lag_of=src // C)
    row = np.full((3, 1, C), -8.0, np.float32)
    row[0, 0, 1] = 8.0
    row[1] = 0.0
    row[2, 0, 2] = 8.0
    got = _expect_exact(gpu, np.repeat(row, 3, axis=1), t, 0.125)
    assert got['state_path'].tolist() == [63, 63, 100], got['state_path']


# ---- the reduction to the plain chain ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [2, 21, 64])
def test_one_lag_is_the_plain_chain(gpu, refs, C):
    """D = 1, pos = arange(C), on the exactness inputs: state_raw / state_path are the oracle's and ops.track_decode's cls_raw / cls_path bit for bit; the posterior
    lies within the bars of the oracle, and post, offset_mean and log_z agree with ops.track_posterior within the bars."""
    from synchformer_amd import ops
    bar = refs['bar']
    tables = _dev_tables(gpu, _plain_tables(C))
    for key in [k for k in PLAIN_KEYS if k[1] == C]:
        case = refs[key]
        W, lam, step = key[2], key[3], case['t']['step']
        got = _run(gpu, case['x'], None, tables, lam)
        _check(got, case, bar, what=str(key))
        assert np.array_equal(got['state_raw'], case['raw']) and np.array_equal(got['state_path'], case['path']), key
        x = torch.from_numpy(case['x'][:, 0]).to(gpu)
        cls_raw, _, cls_path, _ = ops.track_decode(x, lam)
        assert np.array_equal(got['state_raw'], cls_raw.cpu().numpy()) and np.array_equal(got['state_path'], cls_path.cpu().numpy()), key
        post, _, _, mean, log_z = ops.track_posterior(x, lam, case['t']['off'].to(gpu))
        assert np.abs(got['post'] - post.cpu().numpy()).max() <= bar[0] and np.abs(got['offset_mean'] - mean.cpu().numpy()).max() / step <= bar[1]
        assert abs(got['log_z'] - log_z.item()) <= bar[3] * max(1.0, abs(case['ref']['log_z'])) and np.abs(got['p_lag'] - 1).max() <= 1e-5


# ---- graph replay -----------------------------------------------------------------------------------------------------------------------------------------------
def test_under_graph_capture(gpu):
    """Both entries captured on a single stream and replayed equal the eager calls bit for bit: the launchers neither synchronise nor allocate, and no sum depends on
    an order that could change."""
    from synchformer_amd import ops
    t = _lag_tables(25)
    tables = _dev_tables(gpu, t)
    x = torch.from_numpy(_randn(9, (9, 25, 21), 3.0)).to(gpu)
    z = torch.from_numpy(_randn(10, (9, 25, 2), 2.0)).to(gpu)
    eager = [o.clone() for o in ops.track_decode_wide(x, tables, 1.0, z) + ops.track_posterior_wide(x, tables, 1.0, z)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = ops.track_decode_wide(x, tables, 1.0, z) + ops.track_posterior_wide(x, tables, 1.0, z)
    for o in captured:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, captured))
    assert eager[4].sum().item() == pytest.approx(9.0, abs=1e-4)


# ---- the engine's lagged windows --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def engines(gpu):
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    eng = SynchformerEngine(synth.make_state_dict(1337), gpu, seg_chunk=5)
    gate_sd = {k: v for k, v in synth.make_state_dict(4242, head='sync_head', n_pos=184, n_out=2).items() if not k.startswith(('vfeat_extractor.', 'afeat_extractor.'))}
    gate = SynchformerEngine(gate_sd, gpu, towers=False)
    g = torch.Generator().manual_seed(12)
    return eng, gate, torch.randn(24, 8, 768, generator=g).to(gpu), torch.randn(24, 6, 768, generator=g).to(gpu)


@pytest.mark.parametrize('hop', [1, 2])
def test_lagged_windows_equal_sliced_banks(gpu, engines, hop):
    """sync_windows_lagged(...)[:, j] is sync_windows on the banks sliced by hand - visual [v0, ..), audio [v0 + d, ..) - bit for bit, for the offset engine and for a
    towers=False 2-way gate engine with its own window."""
    eng, gate, vbank, abank = engines
    lags = (-3, 0, 2)
    for e, nwin in ((eng, 14), (gate, gate.n_window)):
        got = e.sync_windows_lagged(vbank, abank, lags, hop=hop, win_chunk=4, n_window=nwin)
        W = (24 - nwin - 3 - 2) // hop + 1
        assert got.shape == (W, 3, e.n_out) and got.dtype == torch.float32
        n = (W - 1) * hop + nwin
        for j, d in enumerate(lags):
            want = e.sync_windows(vbank[3:3 + n], abank[3 + d:3 + d + n], hop=hop, win_chunk=4, n_window=nwin)
            assert want.shape == (W, e.n_out) and torch.equal(got[:, j], want), (hop, nwin, d)
    with pytest.raises(ValueError):
        eng.sync_windows_lagged(vbank[:18], abank[:18], lags)
    with pytest.raises(ValueError):
        eng.sync_windows_lagged(vbank, abank, (0, 0))


# ---- the tracker ------------------------------------------------------------------------------------------------------------------------------------------------
def test_tracker_one_lag_is_track_features(gpu, engines):
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.track import OffsetTracker, WideOffsetTrack
    eng, gate, vbank, abank = engines
    tracker = OffsetTracker(eng, MelFrontend(gpu), lam=0.5, posterior=True)
    plain, wide = tracker.track_features(vbank, abank), tracker.track_features_wide(vbank, abank, (0,))
    assert isinstance(wide, WideOffsetTrack) and wide.lags == (0,) and wide.first_segment == 0 and wide.n_segments == 24
    assert torch.equal(wide.logits[:, 0], plain.logits) and torch.equal(wide.t_sec, plain.t_sec)
    assert torch.equal(wide.cls_path, plain.cls_path) and torch.equal(wide.offset_sec_path, plain.offset_sec_path)
    assert torch.equal(wide.cls_raw, plain.cls_raw) and torch.equal(wide.offset_sec_raw, plain.offset_sec_raw) and (wide.lag_path == 0).all()
    assert wide.spans() == plain.spans()


def test_tracker_fields_are_the_ops(gpu, engines):
    from synchformer_amd import ops
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.track import OffsetTracker
    eng, gate, vbank, abank = engines
    lags = (-3, 0, 2)
    for g in (None, gate):
        tracker = OffsetTracker(eng, MelFrontend(gpu), lam=0.5, posterior=True, gate=g)
        tr = tracker.track_features_wide(vbank, abank, lags, win_chunk=4)
        W = 24 - 14 - 3 - 2 + 1
        assert tr.logits.shape == (W, 3, 21) and tr.first_segment == 3 and tr.lags == lags
        assert torch.equal(tr.logits, eng.sync_windows_lagged(vbank, abank, lags))
        assert (tr.gate_logits is None) == (g is None)
        if g is not None:
            assert torch.equal(tr.gate_logits, gate.sync_windows_lagged(vbank, abank, lags, n_window=gate.n_window)[:W])
        assert (tr.t_sec.cpu().double() - ((torch.arange(W, dtype=torch.float64) * 8 + 60) / 25 + 0.96)).abs().max() <= 1e-6
        src, pos, off, lag_of, cls_of = ops.track_wide_states(lags, tracker.grid)
        tables = ops.track_wide_tables(src, pos, off, 3, 21, gpu)
        state_raw, conf_raw, state_path, conf_path = ops.track_decode_wide(tr.logits, tables, 0.5, tr.gate_logits)
        post, state_post, conf_post, mean, p_lag, log_z = ops.track_posterior_wide(tr.logits, tables, 0.5, tr.gate_logits)
        lag_val = torch.tensor(lags, dtype=torch.int32)[lag_of.long()].to(gpu)
        assert torch.equal(tr.state_path, state_path) and torch.equal(tr.conf_path, conf_path) and torch.equal(tr.conf_raw, conf_raw)
        assert torch.equal(tr.lag_path, lag_val[state_path.long()]) and torch.equal(tr.cls_path, cls_of.to(gpu)[state_path.long()])
        assert torch.equal(tr.lag_raw, lag_val[state_raw.long()]) and torch.equal(tr.cls_raw, cls_of.to(gpu)[state_raw.long()])
        assert torch.equal(tr.offset_sec_path, off.to(gpu)[state_path.long()]) and torch.equal(tr.offset_sec_raw, off.to(gpu)[state_raw.long()])
        assert torch.equal(tr.post, post) and torch.equal(tr.state_post, state_post) and torch.equal(tr.conf_post, conf_post) and torch.equal(tr.p_lag, p_lag)
        assert torch.equal(tr.offset_sec_mean, mean) and torch.equal(tr.log_z, log_z) and torch.equal(tr.offset_sec_post, off.to(gpu)[state_post.long()])
        assert tr.lag_path.dtype == torch.int32 and set(tr.lag_path.tolist()) <= set(lags)
    none = OffsetTracker(eng, MelFrontend(gpu)).track_features_wide(vbank, abank, lags)
    assert none.post is None and none.p_lag is None and none.log_z is None


def test_planted_jump_between_lags(gpu, engines):
    """Planted logits: unit noise everywhere and a vote of 6 on one state per window - lag -3 / class 4 (offset -2.16 s) in the first half, lag +2 / class 17 (+2.04 s) in
    the second.  Through OffsetTracker.track_logits_wide (ops.track_decode_wide and the tracker's mapping tables), lag_path, offset_sec_path and spans() show the jump where it was planted."""
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.track import OffsetTracker
    eng = engines[0]
    lags, W = (-3, 0, 2), 60
    x = _randn(77, (W, 3, 21), 1.0)
    x[:30, 0, 4] += 6.0
    x[30:, 2, 17] += 6.0
    tr = OffsetTracker(eng, MelFrontend(gpu), lam=1.0).track_logits_wide(torch.from_numpy(x).to(gpu), lags)
    assert tr.n_segments == 3 + 2 + 14 + 59 and tr.first_segment == 3 and tr.post is None
    assert tr.lag_path.tolist() == [-3] * 30 + [2] * 30 and tr.cls_path.tolist() == [4] * 30 + [17] * 30
    want = [0.32 * -3 + (-2 + 0.2 * 4)] * 30 + [0.32 * 2 + (-2 + 0.2 * 17)] * 30
    assert np.abs(tr.offset_sec_path.cpu().numpy() - np.array(want)).max() <= 1e-6
    spans = tr.spans()
    assert len(spans) == 2 and abs(spans[0][2] + 2.16) <= 1e-6 and abs(spans[1][2] - 2.04) <= 1e-6
    t = tr.t_sec.cpu().double()
    assert spans[0][0] == t[0].item() and spans[1][1] == t[-1].item() and spans[0][1] == spans[1][0] == 0.5 * (t[29].item() + t[30].item())
    assert abs(t[0].item() - (60 / 25 + 0.96)) <= 1e-6
