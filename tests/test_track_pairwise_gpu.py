"""GPU: sf_track_pairwise / sf_track_pairwise_gated (the pairwise marginals of neighbouring windows) against the float64 oracle of
tests/track_pairwise_oracle.py, their identities, masked and non-finite input, strides, graph capture, the OffsetTracker integration and track.fit_smoothness on
the device.

THE BAR IS MEASURED, the way tests/test_track_posterior_gpu.py measures its own.  The yardstick is the contract, literally (no renormalisation), in torch fp32 on the
CPU (_yardstick below), compared with the float64 oracle on the very inputs a test uses; per quantity

    xi, p_change, p_flip, p_top:  max |got - oracle|             jump:   max |jump_abs - oracle|, in classes
    log_z:  |log_z - oracle| / max(1, |oracle log_z|)

the kernel may be at most 4x the yardstick's worst value over all inputs of this file (computed once, in `refs`), with a floor of 1e-6 per quantity.  CEIL holds a
fixed ceiling per quantity - those worst values rounded up to one digit - and the yardstick counts with at most its ceiling, so the bar cannot float with the CPU's
libm.  The yardstick does not renormalise: its worst values come from W = 4096, where its scores reach -11000 and an ulp is 1e-3.
The top pair has no exclusions: the oracle's xi at the kernel's (top_from, top_to) must be at least the oracle's best off-diagonal mass times (1 - r), r = 4x the
yardstick's worst relative error of p_top (R_CEIL: measured the same way, rounded up to one digit)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_pairwise_oracle as PW  # noqa: E402

pytestmark = pytest.mark.gpu

QUANT = ('xi', 'p_change', 'p_flip', 'p_top', 'jump', 'log_z')
# the yardstick's worst value per quantity over the inputs below, rounded up to one digit (measured 7.9e-4, 7.8e-4, 7.1e-5, 6.6e-4, 3.8e-3 classes, 1.1e-5: DESIGN 3.23;
# all but p_flip and log_z at W = 4096, those two in the gated grid at W = 300), and its worst relative error of p_top likewise (measured 2.8e-3, at W = 4096)
CEIL = (8e-4, 8e-4, 8e-5, 7e-4, 4e-3, 2e-5)
R_CEIL = 3e-3


# ---- the yardstick: the contract in torch fp32 on the CPU ------------------------------------------------------------------------------------------------------------
def _lse32(x: torch.Tensor, dim: int) -> torch.Tensor:
    m = x.max(dim, keepdim=True).values
    sub = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    return (sub + torch.log(torch.exp(x - sub).sum(dim, keepdim=True))).squeeze(dim)


def _softplus32(x: torch.Tensor) -> torch.Tensor:
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


def _yardstick(x: np.ndarray, lam: float, gate: np.ndarray = None, mu: float = 0.0):
    """a, b and xi as the oracle states them in float64, in fp32 -> the oracle's dict (numpy)."""
    l = torch.from_numpy(x)
    assert l.dtype == torch.float32
    W, C = l.shape
    idx = torch.arange(C)
    dist = (idx[:, None] - idx[None, :]).abs().float()
    e = l - _lse32(l, 1)[:, None]
    if gate is None:
        E, S = e, -torch.tensor(lam, dtype=torch.float32) * dist
    else:
        z = torch.from_numpy(gate)
        assert z.dtype == torch.float32
        d = z[:, 1] - z[:, 0]
        E = torch.cat([(-_softplus32(d) - torch.log(torch.tensor(float(C))))[:, None].expand(W, C), -_softplus32(-d)[:, None] + e], 1)
        m = torch.arange(2 * C) // C
        S = -torch.tensor(lam, dtype=torch.float32) * dist.repeat(2, 2) - torch.tensor(mu, dtype=torch.float32) * (m[:, None] != m[None, :]).float()
    n = E.shape[1]
    a, b = torch.empty(W, n), torch.empty(W, n)
    a[0] = E[0]
    for w in range(1, W):
        a[w] = E[w] + _lse32(a[w - 1][:, None] + S, 0)
    b[W - 1] = 0
    for w in range(W - 2, -1, -1):
        b[w] = _lse32((b[w + 1] + E[w + 1])[None, :] + S, 1)
    t = a[:-1, :, None] + S[None] + E[1:, None, :] + b[1:, None, :]
    xi2 = torch.exp(t - _lse32(t.reshape(W - 1, n * n), 1)[:, None, None])
    out = {}
    if gate is None:
        xi = xi2
    else:
        xi = xi2[:, :C, :C] + xi2[:, :C, C:] + xi2[:, C:, :C] + xi2[:, C:, C:]
        out['p_flip'] = (xi2[:, :C, C:].sum((1, 2)) + xi2[:, C:, :C].sum((1, 2))).numpy()
    offd = dist > 0
    masked = torch.where(offd[None], xi, torch.tensor(-1.0)).reshape(W - 1, C * C)
    top = masked.argmax(1)
    out.update(xi=xi.numpy(), p_change=(xi * offd[None]).sum((1, 2)).numpy(), jump_abs=(xi * dist[None]).sum((1, 2)).numpy(), top_from=(top // C).numpy(),
               top_to=(top % C).numpy(), p_top=masked.gather(1, top[:, None])[:, 0].numpy(), log_z=float(_lse32(a[W - 1], 0)))
    return out


def _errors(got: dict, ref: dict):
    """The six errors of `got` against the float64 `ref` (p_flip: 0 for the plain chain)."""
    def worst(k):
        d = np.abs(got[k].astype(np.float64) - ref[k])
        return float(d.max()) if d.size else 0.0

    return (worst('xi'), worst('p_change'), worst('p_flip') if 'p_flip' in ref else 0.0, worst('p_top'), worst('jump_abs'),
            abs(got['log_z'] - ref['log_z']) / max(1.0, abs(ref['log_z'])))


def _rel_top(got: dict, ref: dict) -> float:
    """The worst relative error of p_top."""
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.abs(got['p_top'].astype(np.float64) - ref['p_top']) / ref['p_top']
    return float(np.nan_to_num(r, nan=0.0).max()) if r.size else 0.0                        # 0 / 0: no off-diagonal mass in either


# ---- the inputs: made once, with their oracle and yardstick, and never changed ---------------------------------------------------------------------------------------
WS = (2, 3, 5, 9, 300)                                                               # 5: one boundary past a full block of four
LAMS = (0.0, 0.5, 1.0, 8.0)
PLAIN_CASES = [(W, C, lam) for W in WS for C in (2, 21, 64) for lam in LAMS]          # 21: the round-up to 4; 64 fills the wave
GATED_CASES = [(W, C, lam, mu) for W in WS for C in (2, 21, 32) for lam in LAMS for mu in (0.0, 2.0)]


def _randn(seed: int, W: int, C: int, scale: float) -> np.ndarray:
    return (scale * np.random.default_rng(seed).standard_normal((W, C))).astype(np.float32)


def _masked_input():
    x = _randn(31, 40, 21, 3.0)
    x[:, 4] = -np.inf                                                            # a class masked in every window
    x[5:17, 11] = -np.inf                                                        # and one masked in some
    x[33, 11] = -np.inf
    return x


def jump_scenario():
    """One jump from class 8 to class 13 at window 20 of 40: a vote of 6.0 on unit noise, seed 5."""
    x = np.random.default_rng(5).standard_normal((40, 21))
    x[:20, 8] += 6.0
    x[20:, 13] += 6.0
    return x.astype(np.float32)


_INPUTS = {('plain', W, C, lam): (_randn(7 + 1000 * W + 10 * C + int(2 * lam), W, C, 3.0), lam, None, 0.0) for W, C, lam in PLAIN_CASES}
_INPUTS.update({('gated', W, C, lam, mu): (_randn(8 + 1000 * W + 10 * C + int(2 * lam), W, C, 3.0), lam, _randn(9 + 1000 * W + C + int(mu), W, 2, 2.0), mu)
                for W, C, lam, mu in GATED_CASES})
_INPUTS[('strided',)] = (_randn(41, 130, 21, 3.0), 0.5, None, 0.0)
_INPUTS[('strided_gated',)] = (_randn(41, 130, 21, 3.0), 0.5, _randn(44, 130, 2, 2.0), 2.0)
_INPUTS[('drift',)] = (_randn(42, 4096, 21, 3.0), 1.0, None, 0.0)
_INPUTS[('wide',)] = (_randn(43, 300, 21, 50.0), 8.0, None, 0.0)
_INPUTS[('masked',)] = (_masked_input(), 1.0, None, 0.0)
_INPUTS[('jump',)] = (jump_scenario(), 1.0, None, 0.0)


def _oracle(x, lam, gate, mu):
    x64 = x.astype(np.float64)
    return PW.pairwise(x64, lam) if gate is None else PW.pairwise_gated(x64, gate.astype(np.float64), lam, mu)


@pytest.fixture(scope='module')
def refs():
    """key -> dict(x, lam, gate, mu, ref = float64 oracle, yard = the yardstick's errors, yard_r = its relative error of p_top); 'bar' -> the bar per quantity, 'r'."""
    out = {}
    for key, (x, lam, gate, mu) in _INPUTS.items():
        ref, yard = _oracle(x, lam, gate, mu), _yardstick(x, lam, gate, mu)
        out[key] = dict(x=x, lam=lam, gate=gate, mu=mu, ref=ref, yard=_errors(yard, ref), yard_r=_rel_top(yard, ref))
    worst = [max(v['yard'][q] for v in out.values()) for q in range(len(QUANT))]
    worst_r = max(v['yard_r'] for v in out.values())
    print('yardstick worst: ' + '  '.join(f'{n} {w:.3e}' for n, w in zip(QUANT, worst)) + f'  p_top relative {worst_r:.3e} (ceilings {CEIL}, {R_CEIL})')
    out['bar'] = tuple(max(4 * min(w, c), 1e-6) for w, c in zip(worst, CEIL))
    out['r'] = 4 * min(worst_r, R_CEIL)
    return out


def _dev_input(gpu, x: np.ndarray, ld=None):
    """x on the device; ld: as a view of a wider buffer whose extra columns hold a value that would win every maximum."""
    if ld is None:
        return torch.from_numpy(x).to(gpu)
    buf = torch.full((x.shape[0], ld), 1e30, device=gpu, dtype=torch.float32)
    buf[:, :x.shape[1]] = torch.from_numpy(x).to(gpu)
    return buf[:, :x.shape[1]]


def _run(gpu, x, lam, gate=None, mu=0.0, xi=True, ldl=None, ldg=None):
    from synchformer_amd import ops
    W, C = x.shape
    if gate is None:
        out = ops.track_pairwise(_dev_input(gpu, x, ldl), lam, xi=xi)
        names = ('p_change', 'jump_abs', 'top_from', 'top_to', 'p_top', 'xi', 'log_z')
    else:
        out = ops.track_pairwise_gated(_dev_input(gpu, x, ldl), _dev_input(gpu, gate, ldg), lam, mu, xi=xi)
        names = ('p_change', 'jump_abs', 'p_flip', 'top_from', 'top_to', 'p_top', 'xi', 'log_z')
    torch.cuda.synchronize()
    got = dict(zip(names, out))
    n = max(W - 1, 0)
    for k, t in got.items():
        if k == 'xi':
            assert (t is None) if not xi else (t.dtype == torch.float32 and t.shape == (n, C, C) and t.is_contiguous())
        elif k == 'log_z':
            assert t.dtype == torch.float32 and t.shape == (1,)
        else:
            assert t.shape == (n,) and t.dtype == (torch.int32 if k.startswith('top_') else torch.float32), k
    return {k: (None if t is None else float(t.item()) if k == 'log_z' else t.cpu().numpy()) for k, t in got.items()}


def _same(a: dict, b: dict, skip=()):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a if k not in skip and a[k] is not None and b[k] is not None)


def _check(got: dict, case: dict, refs, what=''):
    """Errors within the bar; the top pair's true mass within (1 - r) of the best; xi sums to 1 and p_change is its off-diagonal sum."""
    ref, bar = case['ref'], refs['bar']
    C = case['x'].shape[1]
    err = _errors(got, ref)
    print(f'{what}: ' + '  '.join(f'{n} {e:.3e} (yardstick {y:.3e}, bar {b:.3e})' for n, e, y, b in zip(QUANT, err, case['yard'], bar)))
    assert all(np.isfinite(got[k]).all() for k in got if got[k] is not None and k not in ('top_from', 'top_to'))
    assert all(e <= b for e, b in zip(err, bar)), (err, bar)
    n = got['p_change'].shape[0]
    kf, kt = got['top_from'].astype(np.int64), got['top_to'].astype(np.int64)
    assert ((0 <= kf) & (kf < C) & (0 <= kt) & (kt < C) & (kf != kt)).all()
    at, best = ref['xi'][np.arange(n), kf, kt], ref['p_top']
    print(f'{what}: top pair {int((kf != ref["top_from"]).sum() + ((kf == ref["top_from"]) & (kt != ref["top_to"])).sum())} of {n} differ from the oracle, '
          f'worst true mass / best {float((at / np.where(best > 0, best, 1)).min()) if n else 1:.6f} (r {refs["r"]:.3e})')
    assert (at >= best * (1 - refs['r'])).all()
    assert np.abs(got['p_top'] - got['xi'][np.arange(n), kf, kt]).max(initial=0) <= 1e-6                # p_top is the returned xi at the pair
    assert np.abs(got['xi'].astype(np.float64).sum((1, 2)) - 1).max(initial=0) <= 1e-5
    offd = ~np.eye(C, dtype=bool)
    assert np.abs((got['xi'].astype(np.float64) * offd[None]).sum((1, 2)) - got['p_change']).max(initial=0) <= 1e-5


@pytest.mark.parametrize('W, C, lam', PLAIN_CASES)
def test_pairwise_against_oracle(gpu, refs, W, C, lam):
    from synchformer_amd import ops
    case = refs[('plain', W, C, lam)]
    got = _run(gpu, case['x'], lam)
    _check(got, case, refs, what=f'W {W} C {C} lam {lam}')
    post, _, _, _, log_z = ops.track_posterior(torch.from_numpy(case['x']).to(gpu), lam, torch.linspace(-2, 2, C, device=gpu))
    post = post.cpu().numpy()
    assert float(log_z.item()) == got['log_z']                                               # the same scan: bit for bit
    assert np.abs(got['xi'].sum(2) - post[:-1]).max() <= 2 * refs['bar'][0] and np.abs(got['xi'].sum(1) - post[1:]).max() <= 2 * refs['bar'][0]
    assert _same(got, _run(gpu, case['x'], lam, xi=False))                                             # xi = False: every other output, bit for bit
    if lam == 0.0:                                                                                     # independent windows: the outer product of the softmaxes
        p = torch.softmax(torch.from_numpy(case['x']).double(), 1).numpy()
        assert np.abs(got['xi'] - p[:-1, :, None] * p[1:, None, :]).max() <= refs['bar'][0]


@pytest.mark.parametrize('W, C, lam, mu', GATED_CASES)
def test_pairwise_gated_against_oracle(gpu, refs, W, C, lam, mu):
    from synchformer_amd import ops
    case = refs[('gated', W, C, lam, mu)]
    got = _run(gpu, case['x'], lam, case['gate'], mu)
    _check(got, case, refs, what=f'gated W {W} C {C} lam {lam} mu {mu}')
    post, _, _, _, _, log_z = ops.track_posterior_gated(torch.from_numpy(case['x']).to(gpu), torch.from_numpy(case['gate']).to(gpu), lam, mu,
                                                        torch.linspace(-2, 2, C, device=gpu))
    post = post.cpu().numpy()
    assert float(log_z.item()) == got['log_z']
    assert np.abs(got['xi'].sum(2) - post[:-1]).max() <= 2 * refs['bar'][0] and np.abs(got['xi'].sum(1) - post[1:]).max() <= 2 * refs['bar'][0]
    assert _same(got, _run(gpu, case['x'], lam, case['gate'], mu, xi=False))
    assert (got['p_flip'] >= 0).all() and (got['p_flip'] <= 1 + 1e-5).all()


def test_pairwise_strided(gpu, refs):
    """ldl = C + 3 (and ldg = 5), the extra columns holding 1e30: bit-equal to the dense call."""
    case = refs[('strided',)]
    got = _run(gpu, case['x'], case['lam'], ldl=24)
    _check(got, case, refs, what='strided')
    assert _same(got, _run(gpu, case['x'], case['lam']))
    case = refs[('strided_gated',)]
    got = _run(gpu, case['x'], case['lam'], case['gate'], case['mu'], ldl=24, ldg=5)
    _check(got, case, refs, what='strided gated')
    assert _same(got, _run(gpu, case['x'], case['lam'], case['gate'], case['mu']))


def test_pairwise_does_not_drift(gpu, refs):
    """W = 4096: the scans renormalise per step, and the constants cancel in xi."""
    case = refs[('drift',)]
    _check(_run(gpu, case['x'], case['lam']), case, refs, what='W 4096')


def test_pairwise_wide_dynamic_range(gpu, refs):
    """50 * randn at lam = 8: the log-domain pair stays finite and accurate."""
    case = refs[('wide',)]
    _check(_run(gpu, case['x'], case['lam']), case, refs, what='wide')


def test_pairwise_masked_classes(gpu, refs):
    case = refs[('masked',)]
    got = _run(gpu, case['x'], case['lam'])
    _check(got, case, refs, what='masked')
    masked = np.isneginf(case['x'])
    assert masked[:, 4].all() and 0 < masked[:, 11].sum() < masked.shape[0]
    dead = masked[:-1, :, None] | masked[1:, None, :]                                                  # a pair with a masked end
    assert dead.any() and (got['xi'][dead] == 0).all()


def test_pairwise_non_finite_rows_stay_in_range(gpu):
    """A row of NaN and a +inf: values are unspecified, the call returns, every pair written lies in [0, C) and off the diagonal."""
    x = _randn(3, 40, 21, 3.0)
    x[11, :] = np.nan
    x[23, 5] = np.inf
    for gate in (None, _randn(4, 40, 2, 2.0)):
        got = _run(gpu, x, 1.0, gate, 2.0)
        kf, kt = got['top_from'], got['top_to']
        assert kf.shape == (39,) and kf.min() >= 0 and kf.max() < 21 and kt.min() >= 0 and kt.max() < 21 and (kf != kt).all(), (kf, kt)
    z = _randn(4, 40, 2, 2.0)
    z[7, 0] = np.nan
    z[19, 1] = np.inf
    got = _run(gpu, _randn(3, 40, 21, 3.0), 1.0, z, 2.0)
    assert got['top_from'].min() >= 0 and got['top_from'].max() < 21 and got['top_to'].min() >= 0 and got['top_to'].max() < 21
    assert (got['top_from'] != got['top_to']).all()


def test_gate_that_always_says_synchronizable_gives_the_plain_chain(gpu, refs):
    """z1 - z0 = 30 in every row and mu = 8: the flag never leaves 1 - the class outputs are the plain chain's within the bar, p_flip <= 1e-6."""
    x = _randn(51, 60, 21, 3.0)
    z = np.zeros((60, 2), np.float32)
    z[:, 1] = 30.0
    plain, gated = _run(gpu, x, 1.0), _run(gpu, x, 1.0, z, 8.0)
    bar = dict(zip(QUANT, refs['bar']))
    for k, q in (('xi', 'xi'), ('p_change', 'p_change'), ('p_top', 'p_top'), ('jump_abs', 'jump')):
        assert np.abs(gated[k].astype(np.float64) - plain[k]).max() <= bar[q], k
    assert gated['p_flip'].max() <= 1e-6
    assert abs(gated['log_z'] - plain['log_z']) <= bar['log_z'] * max(1.0, abs(plain['log_z']))


def test_pairwise_is_reproducible_and_captures(gpu):
    """Two calls are bit-equal; one call captured on a single stream and replayed equals the eager call bit for bit: nothing is synchronised or allocated inside."""
    from synchformer_amd import ops
    x, z = torch.from_numpy(_randn(9, 9, 21, 3.0)).to(gpu), torch.from_numpy(_randn(10, 9, 2, 2.0)).to(gpu)
    for call in (lambda: ops.track_pairwise(x, 1.0, xi=True), lambda: ops.track_pairwise_gated(x, z, 1.0, 2.0, xi=True)):
        eager = [t.clone() for t in call()]
        again = call()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, again))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            captured = call()
        for t in captured:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, captured))
        assert eager[-2].sum().item() == pytest.approx(8.0, abs=1e-4)


def test_pairwise_of_one_and_of_no_windows(gpu):
    from synchformer_amd import ops
    x, z = torch.from_numpy(_randn(1, 1, 21, 3.0)).to(gpu), torch.from_numpy(_randn(2, 1, 2, 2.0)).to(gpu)
    for W in (1, 0):
        out = ops.track_pairwise(x[:W], 1.0, xi=True)
        gout = ops.track_pairwise_gated(x[:W], z[:W], 1.0, 2.0, xi=True)
        torch.cuda.synchronize()
        assert [tuple(t.shape) for t in out] == [(0,)] * 5 + [(0, 21, 21), (1,)] and [tuple(t.shape) for t in gout] == [(0,)] * 6 + [(0, 21, 21), (1,)]
        assert ops.track_pairwise(x[:W], 1.0)[5] is None
        # one window: log_z = 0 (the emissions are log-probabilities); none: zero-filled
        assert abs(out[6].item()) <= 1e-6 and abs(gout[7].item()) <= 1e-6 and (W == 1 or (out[6].item() == 0.0 and gout[7].item() == 0.0))
    with pytest.raises(RuntimeError, match='lam must be finite'):
        ops.track_pairwise(torch.zeros(3, 21, device=gpu), -1.0)
    with pytest.raises(RuntimeError, match='mu must be finite'):
        ops.track_pairwise_gated(torch.zeros(3, 21, device=gpu), torch.zeros(3, 2, device=gpu), 1.0, float('nan'))
    with pytest.raises(AssertionError):
        ops.track_pairwise_gated(torch.zeros(3, 21, device=gpu), torch.zeros(2, 2, device=gpu), 1.0, 2.0)


def test_the_jump_is_found(gpu, refs):
    """One jump from class 8 to class 13 at window 20 of 40, lam = 1: boundary 19 carries it, every other boundary stays low, changes(0.5) is that one entry."""
    from types import SimpleNamespace
    from synchformer_amd.track import OffsetTracker
    case = refs[('jump',)]
    got = _run(gpu, case['x'], 1.0)
    _check(got, case, refs, what='jump')
    assert int(got['p_change'].argmax()) == 19 and got['p_change'][19] > 0.9 and (got['top_from'][19], got['top_to'][19]) == (8, 13)
    assert np.delete(got['p_change'], 19).max() < 0.2
    tracker = OffsetTracker(SimpleNamespace(n_out=21, n_window=14, dev=torch.device(gpu)), None, lam=1.0, pairwise=True)
    tr = tracker._track_of(torch.from_numpy(case['x']).to(gpu), 53)
    ch = tr.changes(0.5)
    grid = tracker.grid.cpu().double().tolist()
    assert len(ch) == 1 and ch[0][1] == grid[8] and ch[0][2] == grid[13] and ch[0][3] == float(got['p_change'][19]) and ch[0][4] == float(got['p_top'][19])
    assert ch[0][0] == pytest.approx(0.5 * (tr.t_sec[19].item() + tr.t_sec[20].item()), abs=1e-5)
    assert tr.expected_changes() == pytest.approx(float(got['p_change'].astype(np.float64).sum()), abs=1e-6) and 1.0 < tr.expected_changes() < 1.6
    assert tr.changes(0.0)[5][0] == pytest.approx(tr.t_change[5].item()) and len(tr.changes(0.0)) == 39


def test_tracker_pairwise_fields(gpu):
    """OffsetTracker(pairwise=True) on a 20-segment bank (7 windows), plain and gated: every field of before is bit-equal to the pairwise=False track, the new
    attributes are the ops on the track's own logits, bit for bit."""
    from synchformer_amd import ops, synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.track import OffsetTracker
    eng, mel = SynchformerEngine(synth.make_state_dict(1337), gpu), MelFrontend(gpu)
    gate_sd = {k: v for k, v in synth.make_state_dict(4242, head='sync_head', n_pos=184, n_out=2).items() if not k.startswith(('vfeat_extractor.', 'afeat_extractor.'))}
    gate = SynchformerEngine(gate_sd, gpu, towers=False)
    g = torch.Generator().manual_seed(12)
    vbank, abank = torch.randn(20, 8, 768, generator=g).to(gpu), torch.randn(20, 6, 768, generator=g).to(gpu)
    old = ('t_sec', 'logits', 'cls_raw', 'conf_raw', 'cls_path', 'conf_path', 'offset_sec_raw', 'offset_sec_path', 'post', 'cls_post', 'conf_post', 'offset_sec_post',
           'offset_sec_mean', 'log_z', 'gate_logits', 'sync_raw', 'sync_path', 'p_sync')
    new = ('t_change', 'p_change', 'jump_abs', 'p_change_top', 'change_from_sec', 'change_to_sec', 'p_flip')

    def same(a, b):
        return (a is None and b is None) or torch.equal(a, b)

    for gt in (None, gate):
        before = OffsetTracker(eng, mel, lam=0.5, posterior=True, gate=gt, mu=1.5).track_features(vbank, abank)
        tracker = OffsetTracker(eng, mel, lam=0.5, posterior=True, gate=gt, mu=1.5, pairwise=True)
        tr = tracker.track_features(vbank, abank)
        torch.cuda.synchronize()
        assert tr.logits.shape == (7, 21) and tr.n_segments == before.n_segments == 20
        assert all(same(getattr(tr, n), getattr(before, n)) for n in old) and all(getattr(before, n) is None for n in new)
        if gt is None:
            p_change, jump_abs, top_from, top_to, p_top, _, _ = ops.track_pairwise(tr.logits, 0.5)
            assert tr.p_flip is None
        else:
            p_change, jump_abs, p_flip, top_from, top_to, p_top, _, _ = ops.track_pairwise_gated(tr.logits, tr.gate_logits, 0.5, 1.5)
            assert torch.equal(tr.p_flip, p_flip) and tr.p_flip.shape == (6,)
        assert torch.equal(tr.p_change, p_change) and torch.equal(tr.jump_abs, jump_abs) and torch.equal(tr.p_change_top, p_top)
        assert torch.equal(tr.change_from_sec, tracker.grid[top_from.long()]) and torch.equal(tr.change_to_sec, tracker.grid[top_to.long()])
        assert torch.equal(tr.t_change, 0.5 * (tr.t_sec[:-1] + tr.t_sec[1:])) and tr.t_change.shape == tr.p_change.shape == (6,)
        assert 0 <= tr.expected_changes() <= 6 and all(len(row) == 5 for row in tr.changes(0.0))


def test_fit_smoothness_on_the_device(gpu):
    """fit_smoothness with its default `stats` (the device read-out) on the W = 2000, lam = 1 case of tests/test_track_fit_cpu.py against the fit driven by the
    float64 oracle: the two differ by at most the larger of the bisection's resolution lam_max / 2^iters and 4x what the fp32 yardstick's fit differs by - and in any
    case by less than 0.1 se_lam: the numerical error is small against the statistical one."""
    from synchformer_amd.track import fit_smoothness
    from test_track_fit_cpu import labelled_recording, oracle_stats
    x, y = labelled_recording(1.0)
    x32 = x.astype(np.float32)
    iters, lam_max = 20, 16.0

    def yard_stats(logits, gate_logits, lam, mu):
        o = _yardstick(logits, lam)
        return float(o['jump_abs'].astype(np.float64).sum()), 0.0, o['log_z']

    ref = fit_smoothness([(x32.astype(np.float64), y)], lam_max=lam_max, iters=iters, stats=oracle_stats)
    yard = fit_smoothness([(x32, y)], lam_max=lam_max, iters=iters, stats=yard_stats)
    got = fit_smoothness([(torch.from_numpy(x32).to(gpu), torch.from_numpy(y).to(gpu))], lam_max=lam_max, iters=iters)
    print(f'oracle fit {ref.lam:.6f} +- {ref.se_lam:.4f};  device {got.lam:.6f} (off by {abs(got.lam - ref.lam) / ref.se_lam:.4f} se), fp32 yardstick {yard.lam:.6f} '
          f'(off by {abs(yard.lam - ref.lam) / ref.se_lam:.4f} se);  E[J] device {got.jumps_expected:.3f}, oracle {ref.jumps_expected:.3f}')
    assert abs(got.lam - ref.lam) <= max(lam_max / 2 ** iters, 4 * abs(yard.lam - ref.lam))
    assert abs(got.lam - ref.lam) < 0.1 * ref.se_lam
    assert not got.at_bound and got.jumps_observed == ref.jumps_observed and got.evaluations == ref.evaluations
    assert abs(got.se_lam - ref.se_lam) <= 0.02 * ref.se_lam and abs(got.log_likelihood - ref.log_likelihood) <= 1e-4 * abs(ref.log_likelihood)
