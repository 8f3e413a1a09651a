"""GPU: sf_track_decode_gated / sf_track_posterior_gated (the read-outs of one chain over (offset class, synchronizable flag)) against the float64
oracle of tests/track_gated_oracle.py, their identities, strided and non-finite input, a replay under graph capture, and the OffsetTracker(gate=...) integration.

THE PATH is not compared index by index on random input: plane 0 of the emission is flat, exact ties are the rule, and an fp32 and a float64 restatement break
them differently.  Instead the oracle's path_score of the kernel's path must lie within W * 2^-13 of the oracle's optimum: the renormalised scores of these inputs
lie below 2^9 in magnitude, so one ulp is 2^-15; a decision can go the other way only inside a few ulp, and each such flip costs at most that margin once per
window.  A real defect costs mu, lam or an emission gap per window: more than 0.1.  (Measured on the MI355X: the worst gap over the grid is 1.1e-12, at W = 4096
1.8e-12 - float64 rounding: the kernel's path is an optimum everywhere; test_decode_gated_path_is_optimal prints it, DESIGN 3.20 records it.)
Where the margins are whole logits - the gap scenario, a gate at d = +30 - indices are compared exactly.

THE POSTERIOR BAR IS MEASURED, by the method of tests/test_track_posterior_gpu.py.  The yardstick is the contract's recurrences, literally (no renormalisation), in
torch fp32 on the CPU (_yardstick below), compared with the float64 oracle on the very inputs a test uses; per quantity

    post:    max |post - oracle|                 p_sync:  max |p_sync - oracle|                 mean:  max |offset_mean - oracle| / grid step
    log_z:   |log_z - oracle| / max(1, |oracle log_z|)

the kernel may be at most 4x the yardstick's worst value over all inputs of this file (computed once, in `refs`), with an absolute floor of 1e-6 for post.  CEIL
holds a fixed ceiling per quantity - those worst values, rounded up to one digit - and the yardstick counts with at most its ceiling, so the bar cannot float with
the CPU's libm.  cls_post is checked free of ties: the oracle's marginal of the chosen class lies within the post bar of the oracle's maximum."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_gated_oracle as TG  # noqa: E402

pytestmark = pytest.mark.gpu

QUANT = ('post', 'p_sync', 'mean', 'log_z')
# the yardstick's worst (post, p_sync, mean in grid steps, log_z) over the inputs below, rounded up to one digit (measured 7.15e-4, 6.18e-4, 2.12e-2,
# 1.33e-5: post and p_sync from W = 4096, the mean from W = 300, C = 32 at lam = 8, mu = 16, log_z from W = 300, C = 21 at lam = mu = 0)
CEIL = (8e-4, 7e-4, 3e-2, 2e-5)
PATH_TOL = 2.0 ** -13                                                            # per window


def _grid(C: int) -> np.ndarray:
    return np.linspace(-2, 2, C).astype(np.float32)


def _lse32(x: torch.Tensor, dim: int) -> torch.Tensor:
    m = x.max(dim, keepdim=True).values
    sub = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    return (sub + torch.log(torch.exp(x - sub).sum(dim, keepdim=True))).squeeze(dim)


def _softplus32(x: torch.Tensor) -> torch.Tensor:
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def _yardstick(x: np.ndarray, z: np.ndarray, lam: float, mu: float, grid: np.ndarray):
    """The recurrences of the contract in torch fp32 on the CPU, as the oracle states them in float64."""
    l, zz, g = torch.from_numpy(x), torch.from_numpy(z), torch.from_numpy(grid)
    assert l.dtype == zz.dtype == g.dtype == torch.float32
    W, C = l.shape
    d = zz[:, 1] - zz[:, 0]
    e1 = -_softplus32(-d)[:, None] + (l - _lse32(l, 1)[:, None])
    e0 = (-_softplus32(d) - torch.log(torch.tensor(float(C))))[:, None].expand(W, C)
    E = torch.cat([e0, e1], 1)
    T = torch.from_numpy(TG.transition(C, lam, mu)).float()                      # T[j', j]
    a, b = torch.empty(W, 2 * C), torch.empty(W, 2 * C)
    a[0] = E[0]
    for w in range(1, W):
        a[w] = E[w] + _lse32(a[w - 1][:, None] + T, 0)
    b[W - 1] = 0
    for w in range(W - 2, -1, -1):
        b[w] = _lse32((b[w + 1] + E[w + 1])[None, :] + T, 1)
    s = a + b
    post2 = torch.exp(s - _lse32(s, 1)[:, None])
    post = post2[:, :C] + post2[:, C:]
    p_sync, mean = torch.zeros(W), torch.zeros(W)
    for c in range(C):                                                           # ascending c, fp32
        p_sync = p_sync + post2[:, C + c]
        mean = mean + post[:, c] * g[c]
    return dict(post=post.numpy(), p_sync=p_sync.numpy(), offset_mean=mean.numpy(), log_z=float(_lse32(a[W - 1], 0)))


def _errors(got: dict, ref: dict, grid: np.ndarray):
    """(post, p_sync, mean, log_z) errors of `got` against the float64 `ref`."""
    step = float(grid[1] - grid[0])
    return (float(np.abs(got['post'].astype(np.float64) - ref['post']).max()),
            float(np.abs(got['p_sync'].astype(np.float64) - ref['p_sync']).max()),
            float(np.abs(got['offset_mean'].astype(np.float64) - ref['offset_mean']).max()) / step,
            abs(float(got['log_z']) - ref['log_z']) / max(1.0, abs(ref['log_z'])))


# ---- the inputs: made once, with their oracle and yardstick, and never changed ---------------------------------------------------------------------
GRID_CASES = [(W, C, lam, mu) for W in (1, 2, 9, 300) for C in (2, 21, 32) for lam in (0.0, 0.5, 1.0, 8.0) for mu in (0.0, 2.0, 16.0)]
SHAPES = [(W, C) for W in (1, 2, 9, 300) for C in (2, 21, 32)]


def _randn(seed: int, W: int, C: int, scale: float):
    """(logits (W, C), gate logits (W, 2)), scale * randn, fp32."""
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((W, C))).astype(np.float32), (scale * rng.standard_normal((W, 2))).astype(np.float32)


_INPUTS = {('grid', W, C, lam, mu): (*_randn(11 + 1000 * W + 10 * C + int(2 * lam) + 100000 * int(mu), W, C, 3.0), lam, mu) for W, C, lam, mu in GRID_CASES}
_INPUTS[('strided',)] = (*_randn(41, 130, 21, 3.0), 0.5, 2.0)
_INPUTS[('drift',)] = (*_randn(42, 4096, 21, 3.0), 1.0, 2.0)
_INPUTS[('wide',)] = (*_randn(43, 300, 21, 50.0), 8.0, 2.0)


@pytest.fixture(scope='module')
def refs():
    """key -> dict(x, z, lam, mu, grid, ref = float64 oracle, vit = the oracle's Viterbi, yard = the yardstick's errors); 'bar' -> the bar per quantity."""
    out = {}
    for key, (x, z, lam, mu) in _INPUTS.items():
        grid = _grid(x.shape[1])
        x64, z64 = x.astype(np.float64), z.astype(np.float64)
        ref = TG.posterior(x64, z64, lam, mu, grid.astype(np.float64))
        out[key] = dict(x=x, z=z, lam=lam, mu=mu, grid=grid, ref=ref, vit=TG.viterbi(x64, z64, lam, mu), yard=_errors(_yardstick(x, z, lam, mu, grid), ref, grid))
    worst = [max(v['yard'][q] for v in out.values()) for q in range(4)]
    print('yardstick worst: ' + '  '.join(f'{n} {w:.3e}' for n, w in zip(QUANT, worst)) + f' (ceilings {CEIL})')
    worst = [min(w, c) for w, c in zip(worst, CEIL)]                             # the bar does not float
    out['bar'] = (max(4 * worst[0], 1e-6), 4 * worst[1], 4 * worst[2], 4 * worst[3])
    return out


def _dev_inputs(gpu, x: np.ndarray, z: np.ndarray, ldl=None, ldg=None):
    """Dense device copies, or strided views whose padding holds a value that would win every maximum."""
    W, C = x.shape
    if ldl is None:
        return torch.from_numpy(x).to(gpu), torch.from_numpy(z).to(gpu)
    xb = torch.full((W, ldl), 1e30, device=gpu, dtype=torch.float32)
    zb = torch.full((W, ldg), 1e30, device=gpu, dtype=torch.float32)
    xb[:, :C] = torch.from_numpy(x).to(gpu)
    zb[:, :2] = torch.from_numpy(z).to(gpu)
    return xb[:, :C], zb[:, :2]


def _decode(gpu, x, z, lam, mu, ldl=None, ldg=None):
    from synchformer_amd import ops
    W = x.shape[0]
    out = ops.track_decode_gated(*_dev_inputs(gpu, x, z, ldl, ldg), lam, mu)
    torch.cuda.synchronize()
    assert [t.dtype for t in out] == [torch.int32, torch.float32, torch.float32, torch.int32, torch.int32, torch.float32] and all(t.shape == (W,) for t in out)
    return dict(zip(('cls_raw', 'conf_raw', 'sync_raw', 'cls_path', 'sync_path', 'conf_path'), (t.cpu().numpy() for t in out)))


def _posterior(gpu, x, z, lam, mu, grid, ldl=None, ldg=None, ldp=None):
    from synchformer_amd import ops
    W, C = x.shape
    pbuf = None if ldp is None else torch.full((W, ldp), -7.0, device=gpu, dtype=torch.float32)
    out = ops.track_posterior_gated(*_dev_inputs(gpu, x, z, ldl, ldg), lam, mu, torch.from_numpy(grid).to(gpu), post=None if pbuf is None else pbuf[:, :C])
    torch.cuda.synchronize()
    post, p_sync, cls_post, conf_post, mean, log_z = out
    assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.int32, torch.float32, torch.float32, torch.float32]
    assert post.shape == (W, C) and p_sync.shape == cls_post.shape == conf_post.shape == mean.shape == (W,) and log_z.shape == (1,)
    if pbuf is not None:
        assert (pbuf[:, C:] == -7.0).all(), 'the padding of post was written'
    return dict(post=post.cpu().numpy(), p_sync=p_sync.cpu().numpy(), cls_post=cls_post.cpu().numpy(), conf_post=conf_post.cpu().numpy(),
                offset_mean=mean.cpu().numpy(), log_z=float(log_z.item()))


def _softmax64(x: np.ndarray) -> np.ndarray:
    p = np.exp(x.astype(np.float64) - x.astype(np.float64).max(1, keepdims=True))
    return p / p.sum(1, keepdims=True)


def _check_decode(got: dict, case: dict, what=''):
    """The raw read-outs against float64, every index in range, the path within PATH_TOL per window of the oracle's optimum -> the gap."""
    x, z, lam, mu = case['x'], case['z'], case['lam'], case['mu']
    W, C = x.shape
    p = _softmax64(x)
    assert np.array_equal(got['cls_raw'], x.argmax(1)), 'cls_raw'
    assert np.abs(got['conf_raw'] - p[np.arange(W), got['cls_raw']]).max() <= 4e-6               # up to 32 terms (wide logits: 1 of them), fp32 exp and sum
    d = z[:, 1].astype(np.float64) - z[:, 0].astype(np.float64)
    assert np.abs(got['sync_raw'] - 1 / (1 + np.exp(-d))).max() <= 4e-6
    assert got['cls_path'].min() >= 0 and got['cls_path'].max() < C and set(np.unique(got['sync_path'])) <= {0, 1}
    assert np.abs(got['conf_path'] - p[np.arange(W), got['cls_path']]).max() <= 4e-6
    states = got['sync_path'].astype(np.int64) * C + got['cls_path']
    gap = case['vit']['score'] - TG.path_score(x.astype(np.float64), z.astype(np.float64), lam, mu, states)
    print(f'{what} lam {lam} mu {mu}: optimum - score of the kernel\'s path = {gap:.3e} (allowed {W * PATH_TOL:.3e}); '
          f'{int((states != case["vit"]["states"]).sum())} of {W} indices differ from the oracle\'s')
    assert -1e-9 <= gap <= W * PATH_TOL, gap
    return gap


def _check_posterior(got: dict, case: dict, bar, what=''):
    ref, (W, C) = case['ref'], case['x'].shape
    err = _errors(got, ref, case['grid'])
    print(f'{what} lam {case["lam"]} mu {case["mu"]}: ' + '  '.join(f'{n} {e:.3e} (yardstick {y:.3e}, bar {b:.3e})' for n, e, y, b in zip(QUANT, err, case['yard'], bar)))
    assert all(np.isfinite(got[k]).all() for k in ('post', 'p_sync', 'conf_post', 'offset_mean')) and np.isfinite(got['log_z'])
    assert all(e <= b for e, b in zip(err, bar)), (err, bar)
    assert np.abs(got['post'].sum(1) - 1).max() <= 1e-5
    assert got['log_z'] <= 1e-5
    assert got['p_sync'].min() >= 0 and got['p_sync'].max() <= 1
    assert got['cls_post'].min() >= 0 and got['cls_post'].max() < C
    assert np.array_equal(got['conf_post'], got['post'][np.arange(W), got['cls_post']])
    assert (ref['post'][np.arange(W), got['cls_post']] >= ref['post'].max(1) - bar[0]).all()     # the chosen class is the oracle's best, or within the bar of it


@pytest.mark.parametrize('W, C', SHAPES)
def test_decode_gated_path_is_optimal(gpu, refs, W, C):
    worst = 0.0
    for lam in (0.0, 0.5, 1.0, 8.0):
        for mu in (0.0, 2.0, 16.0):
            case = refs[('grid', W, C, lam, mu)]
            worst = max(worst, _check_decode(_decode(gpu, case['x'], case['z'], lam, mu), case, what=f'W {W} C {C}'))
    print(f'W {W} C {C}: worst gap {worst:.3e}')


@pytest.mark.parametrize('W, C', SHAPES)
def test_posterior_gated_against_oracle(gpu, refs, W, C):
    bar = refs['bar']
    for lam in (0.0, 0.5, 1.0, 8.0):
        for mu in (0.0, 2.0, 16.0):
            case = refs[('grid', W, C, lam, mu)]
            got = _posterior(gpu, case['x'], case['z'], lam, mu, case['grid'])
            _check_posterior(got, case, bar, what=f'W {W} C {C}')
            flipped = _posterior(gpu, case['x'][::-1].copy(), case['z'][::-1].copy(), lam, mu, case['grid'])       # reversed rows: reversed marginals, the same log_z
            assert np.abs(flipped['post'][::-1] - got['post']).max() <= 2 * bar[0] and np.abs(flipped['p_sync'][::-1] - got['p_sync']).max() <= 2 * bar[1]
            assert abs(flipped['log_z'] - got['log_z']) <= 2 * bar[3] * max(1.0, abs(case['ref']['log_z']))


def test_gated_strided(gpu, refs):
    """ldl = C + 3, ldg = 5 (the columns beyond the width would win every maximum if read) and a post of row stride C + 5 (its padding stays as it was); bit-equal
    to the dense calls."""
    case = refs[('strided',)]
    x, z, lam, mu, grid = (case[k] for k in ('x', 'z', 'lam', 'mu', 'grid'))
    got = _posterior(gpu, x, z, lam, mu, grid, ldl=24, ldg=5, ldp=26)
    _check_posterior(got, case, refs['bar'], what='strided')
    dense = _posterior(gpu, x, z, lam, mu, grid)
    assert all(np.array_equal(got[k], dense[k]) for k in ('post', 'p_sync', 'cls_post', 'conf_post', 'offset_mean')) and got['log_z'] == dense['log_z']
    dec = _decode(gpu, x, z, lam, mu, ldl=24, ldg=5)
    _check_decode(dec, case, what='strided')
    dense = _decode(gpu, x, z, lam, mu)
    assert all(np.array_equal(dec[k], dense[k]) for k in dec)


def test_gated_does_not_drift(gpu, refs):
    """W = 4096: the per-step renormalisation keeps the scores bounded, the double accumulator keeps log_z to fp32 precision, and the path stays optimal."""
    case = refs[('drift',)]
    _check_posterior(_posterior(gpu, case['x'], case['z'], case['lam'], case['mu'], case['grid']), case, refs['bar'], what='W 4096')
    _check_decode(_decode(gpu, case['x'], case['z'], case['lam'], case['mu']), case, what='W 4096')


def test_posterior_gated_wide_dynamic_range(gpu, refs):
    """50 * randn at lam = 8: logits 300 apart inside a row and gate logits 100 apart - the log-domain recursion stays finite and accurate."""
    case = refs[('wide',)]
    _check_posterior(_posterior(gpu, case['x'], case['z'], case['lam'], case['mu'], case['grid']), case, refs['bar'], what='wide')


@pytest.mark.parametrize('mu', [0.0, 2.0, 16.0])
@pytest.mark.parametrize('lam', [0.5, 1.0])
def test_gap_scenario(gpu, refs, lam, mu):
    """The music bed of DESIGN 3.20 (margins of whole logits: indices are compared exactly): the joint path holds class 13 and flags exactly the gap, while the
    ungated read-out of the same logits follows the decoy.  The posterior agrees on the flag: p_sync below 1 % in the gap and above 99 % outside (the oracle:
    5.8e-4 / 0.9995 at worst); the class marginal inside the gap is spread by the flat plane (the oracle gives class 13 a marginal of 0.09 .. 0.16 there), so it is
    compared with the oracle like any other input."""
    from synchformer_amd import ops
    l, z = TG.gap_scenario()
    ref = TG.viterbi(l, z, lam, mu)
    got = _decode(gpu, l.astype(np.float32), z.astype(np.float32), lam, mu)
    assert np.array_equal(got['cls_path'], ref['cls_path']) and np.array_equal(got['sync_path'], ref['sync_path'])
    assert (got['cls_path'] == 13).all() and np.array_equal(np.flatnonzero(got['sync_path'] == 0), np.arange(22, 37))
    plain = ops.track_decode(torch.from_numpy(l.astype(np.float32)).to(gpu), lam)[2].cpu().numpy()
    assert (plain[22:37] == 2).all() and (plain[:22] == 13).all() and (plain[37:] == 13).all()
    grid = _grid(21)
    post = _posterior(gpu, l.astype(np.float32), z.astype(np.float32), lam, mu, grid)
    assert post['p_sync'][22:37].max() < 0.01 and post['p_sync'][:22].min() > 0.99 and post['p_sync'][37:].min() > 0.99
    case = dict(x=l.astype(np.float32), z=z.astype(np.float32), lam=lam, mu=mu, grid=grid, ref=TG.posterior(l, z, lam, mu, grid.astype(np.float64)), yard=(0, 0, 0, 0))
    _check_posterior(post, case, refs['bar'], what='gap')
    assert (post['cls_post'][:22] == 13).all() and (post['cls_post'][37:] == 13).all()


@pytest.mark.parametrize('lam', [0.0, 0.5, 1.0, 8.0])
def test_confident_gate_gives_the_ungated_path(gpu, lam):
    """d = +30 everywhere: the joint path is the ungated path (the oracle's and sf_track_decode's) with the flag set in every window."""
    from synchformer_amd import ops
    l, z = TG.gap_scenario()
    z[:, 0], z[:, 1] = 0.0, 30.0
    got = _decode(gpu, l.astype(np.float32), z.astype(np.float32), lam, 2.0)
    assert (got['sync_path'] == 1).all() and np.array_equal(got['cls_path'], TG.ungated_viterbi(l, lam))
    assert np.array_equal(got['cls_path'], ops.track_decode(torch.from_numpy(l.astype(np.float32)).to(gpu), lam)[2].cpu().numpy())


def test_gated_non_finite_rows_stay_in_range(gpu):
    """Rows of NaN and rows with infinities, in either input: values are unspecified, the calls return and every index written lies in range."""
    from synchformer_amd import ops
    x, z = _randn(3, 40, 21, 3.0)
    x[11, :] = np.nan
    x[23, 5] = np.inf
    x[29, 7] = -np.inf
    z[5, 1] = np.nan
    z[17, 0] = np.inf
    z[31, :] = -np.inf
    xd, zd = torch.from_numpy(x).to(gpu), torch.from_numpy(z).to(gpu)
    dec = ops.track_decode_gated(xd, zd, 1.0, 2.0)
    post = ops.track_posterior_gated(xd, zd, 1.0, 2.0, torch.from_numpy(_grid(21)).to(gpu))
    torch.cuda.synchronize()
    for cls in (dec[0], dec[3], post[2]):
        c = cls.cpu().numpy()
        assert c.shape == (40,) and c.min() >= 0 and c.max() < 21, c
    assert set(np.unique(dec[4].cpu().numpy())) <= {0, 1}
    assert np.array_equal(dec[0].cpu().numpy()[:11], x[:11].argmax(1))           # rows before the first non-finite one are untouched in the raw read-out


def test_gated_of_no_windows(gpu):
    from synchformer_amd import ops
    grid = torch.from_numpy(_grid(21)).to(gpu)
    x, z = torch.empty(0, 21, device=gpu), torch.empty(0, 2, device=gpu)
    dec = ops.track_decode_gated(x, z, 1.0, 2.0)
    post, p_sync, cls_post, conf_post, mean, log_z = ops.track_posterior_gated(x, z, 1.0, 2.0, grid)
    torch.cuda.synchronize()
    assert all(t.shape == (0,) for t in dec) and post.shape == (0, 21) and p_sync.shape == cls_post.shape == conf_post.shape == mean.shape == (0,)
    assert log_z.shape == (1,) and log_z.item() == 0.0
    with pytest.raises(AssertionError):
        ops.track_decode_gated(torch.zeros(3, 21, device=gpu), torch.zeros(4, 2, device=gpu), 1.0, 2.0)            # gate logits of another length
    with pytest.raises(RuntimeError, match='mu must be finite'):
        ops.track_decode_gated(torch.zeros(3, 21, device=gpu), torch.zeros(3, 2, device=gpu), 1.0, -1.0)
    with pytest.raises(RuntimeError, match='classes out of range'):
        ops.track_posterior_gated(torch.zeros(3, 33, device=gpu), torch.zeros(3, 2, device=gpu), 1.0, 2.0, torch.zeros(33, device=gpu))


def test_gated_under_graph_capture(gpu):
    """One call of each launcher captured on a single stream and replayed once equals the eager call bit for bit: the launchers neither synchronise nor allocate."""
    from synchformer_amd import ops
    x, z = (torch.from_numpy(t).to(gpu) for t in _randn(9, 9, 21, 3.0))
    grid = torch.from_numpy(_grid(21)).to(gpu)
    eager = [t.clone() for t in ops.track_decode_gated(x, z, 1.0, 2.0) + ops.track_posterior_gated(x, z, 1.0, 2.0, grid)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = ops.track_decode_gated(x, z, 1.0, 2.0) + ops.track_posterior_gated(x, z, 1.0, 2.0, grid)
    for t in captured:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert len(eager) == 12 and all(torch.equal(a, b) for a, b in zip(eager, captured))
    assert eager[6].sum().item() == pytest.approx(9.0, abs=1e-4)


# ----------------------------------------------------------------------------------------------------------------------------------------------
# end to end: the 17-segment recording and seg_chunk = 5 engine of tests/test_track_gpu.py, and a synthetic 184-token gate engine without towers
# ----------------------------------------------------------------------------------------------------------------------------------------------
T_REC, N_REC, N_SEG = 144, 92160, 17
TRACK_FIELDS = ('t_sec', 'logits', 'cls_raw', 'conf_raw', 'cls_path', 'conf_path', 'offset_sec_raw', 'offset_sec_path')
POST_FIELDS = ('post', 'cls_post', 'conf_post', 'offset_sec_post', 'offset_sec_mean', 'log_z')
GATE_FIELDS = ('gate_logits', 'sync_raw', 'sync_path', 'p_sync')


@pytest.fixture(scope='module')
def rec(gpu):
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    eng = SynchformerEngine(synth.make_state_dict(1337), gpu, seg_chunk=5)
    gate_sd = {k: v for k, v in synth.make_state_dict(4242, head='sync_head', n_pos=184, n_out=2).items() if not k.startswith(('vfeat_extractor.', 'afeat_extractor.'))}
    gate = SynchformerEngine(gate_sd, gpu, towers=False)                         # the state dict holds no tower keys
    mel = MelFrontend(gpu)
    g = torch.Generator().manual_seed(99)
    frames = torch.randint(0, 256, (T_REC, 3, 224, 224), generator=g, dtype=torch.uint8).to(gpu)
    wave = synth.make_wave(1, 1, 99, n=N_REC).reshape(N_REC).to(gpu)
    vbank, abank = eng.extract_recording(frames, wave, mel)
    torch.cuda.synchronize()
    return dict(eng=eng, gate=gate, mel=mel, frames=frames, wave=wave, vbank=vbank, abank=abank)


def _same(a, b, names):
    return all(torch.equal(getattr(a, n), getattr(b, n)) for n in names)


def test_sync_only_engine(gpu, rec):
    eng, gate = rec['eng'], rec['gate']
    assert (eng.n_window, eng.n_out, eng.towers) == (14, 21, True) and (gate.n_window, gate.n_out, gate.towers) == (13, 2, False)
    with pytest.raises(RuntimeError, match='towers=False'):
        gate.extract_recording(rec['frames'], rec['wave'], rec['mel'])
    with pytest.raises(RuntimeError, match='towers=False'):
        gate.extract_vfeats(torch.zeros(1, 1, 16, 3, 224, 224, device=gpu, dtype=torch.uint8))


def test_tracker_gate_fields(gpu, rec):
    """The gate's logits are the 2-way head on the explicit 13-segment slices of the SAME bank, start-aligned with the offset windows, bit for bit; the gated fields
    are the two new ops on (logits, gate_logits), bit for bit; a tracker without a gate gives what it gave before."""
    from synchformer_amd import ops
    from synchformer_amd.track import OffsetTracker
    eng, gate, mel, vbank, abank = (rec[k] for k in ('eng', 'gate', 'mel', 'vbank', 'abank'))
    plain = OffsetTracker(eng, mel, lam=0.5, posterior=True).track(rec['frames'], rec['wave'])
    tracker = OffsetTracker(eng, mel, lam=0.5, posterior=True, gate=gate, mu=1.5)
    tr = tracker.track(rec['frames'], rec['wave'])
    torch.cuda.synchronize()
    W = N_SEG - 14 + 1
    assert tr.logits.shape == (W, 21) and tr.gate_logits.shape == (W, 2) and tr.gate_logits.dtype == torch.float32 and tr.n_segments == N_SEG
    for w in range(W):
        one = gate.sync_transformer(vbank[None, w:w + 13], abank[None, w:w + 13])[0]
        assert torch.equal(tr.gate_logits[w], one), (w, (tr.gate_logits[w] - one).abs().max().item())
    assert not torch.equal(tr.gate_logits[0], tr.gate_logits[1])
    cls_raw, conf_raw, sync_raw, cls_path, sync_path, conf_path = ops.track_decode_gated(tr.logits, tr.gate_logits, 0.5, 1.5)
    assert torch.equal(tr.cls_raw, cls_raw) and torch.equal(tr.conf_raw, conf_raw) and torch.equal(tr.sync_raw, sync_raw) and torch.equal(tr.cls_path, cls_path)
    assert torch.equal(tr.sync_path, sync_path) and torch.equal(tr.conf_path, conf_path) and torch.equal(tr.offset_sec_path, tracker.grid[cls_path.long()])
    post, p_sync, cls_post, conf_post, mean, log_z = ops.track_posterior_gated(tr.logits, tr.gate_logits, 0.5, 1.5, tracker.grid)
    assert torch.equal(tr.post, post) and torch.equal(tr.p_sync, p_sync) and torch.equal(tr.cls_post, cls_post) and torch.equal(tr.conf_post, conf_post)
    assert torch.equal(tr.offset_sec_mean, mean) and torch.equal(tr.log_z, log_z) and torch.equal(tr.offset_sec_post, tracker.grid[cls_post.long()])
    assert tr.sync_path.dtype == torch.int32 and tr.sync_raw.shape == tr.p_sync.shape == (W,)
    # what does not depend on the gate is what the tracker without one gives; track_features on the bank is the same track
    assert _same(tr, plain, ('t_sec', 'logits', 'cls_raw', 'conf_raw', 'offset_sec_raw'))
    assert _same(tracker.track_features(vbank, abank), tr, TRACK_FIELDS + POST_FIELDS + GATE_FIELDS)
    assert len(tr.spans()) >= 1 and tr.spans()[0][0] == pytest.approx(2.4) and tr.spans()[-1][1] == pytest.approx(2.4 + 0.32 * (W - 1))
    # without a gate: the fields of before, bit for bit the two ungated ops on the track's logits, and no gate fields
    assert all(getattr(plain, n) is None for n in GATE_FIELDS)
    dec = ops.track_decode(plain.logits, 0.5)
    assert all(torch.equal(getattr(plain, n), t) for n, t in zip(('cls_raw', 'conf_raw', 'cls_path', 'conf_path'), dec))
    pst = ops.track_posterior(plain.logits, 0.5, tracker.grid)
    assert all(torch.equal(getattr(plain, n), t) for n, t in zip(('post', 'cls_post', 'conf_post', 'offset_sec_mean', 'log_z'), pst))
    assert torch.equal(plain.offset_sec_path, tracker.grid[dec[2].long()]) and torch.equal(plain.offset_sec_post, tracker.grid[pst[1].long()])
    no_post = OffsetTracker(eng, mel, lam=0.5, gate=gate, mu=1.5).track_features(vbank, abank)
    assert _same(no_post, tr, TRACK_FIELDS + ('gate_logits', 'sync_raw', 'sync_path')) and no_post.p_sync is None and no_post.post is None


def test_tracker_gate_hop_and_raw(gpu, rec):
    """hop = 3 (2 windows: segments 0 and 3 start both kinds of window) and track_raw through an identity ingest honour the gate."""
    from synchformer_amd import ops
    from synchformer_amd.ingest import RecordingIngest
    from synchformer_amd.track import OffsetTracker
    eng, gate, mel, vbank, abank = (rec[k] for k in ('eng', 'gate', 'mel', 'vbank', 'abank'))
    tr = OffsetTracker(eng, mel, hop_segments=3, gate=gate).track_features(vbank, abank)
    assert tr.logits.shape == (2, 21) and tr.gate_logits.shape == (2, 2)
    for w in range(2):
        assert torch.equal(tr.gate_logits[w], gate.sync_transformer(vbank[None, 3 * w:3 * w + 13], abank[None, 3 * w:3 * w + 13])[0])
    ing = RecordingIngest(gpu, 25, (224, 224), 16000)
    tracker = OffsetTracker(eng, mel, gate=gate)
    raw, raw_plain = tracker.track_raw(rec['frames'], rec['wave'], ing), OffsetTracker(eng, mel).track_raw(rec['frames'], rec['wave'], ing)
    assert _same(raw, raw_plain, ('t_sec', 'logits', 'cls_raw', 'conf_raw')) and raw.gate_logits.shape == (raw.logits.shape[0], 2) and raw_plain.sync_path is None
    dec = ops.track_decode_gated(raw.logits, raw.gate_logits, tracker.lam, tracker.mu)
    assert torch.equal(raw.cls_path, dec[3]) and torch.equal(raw.sync_path, dec[4]) and torch.equal(raw.sync_raw, dec[2])


def test_tracker_gate_programmes(gpu, rec):
    """The programme form with P = 2 equals two single calls, field for field."""
    from synchformer_amd.track import OffsetTracker
    eng, gate, mel, vbank, abank = (rec[k] for k in ('eng', 'gate', 'mel', 'vbank', 'abank'))
    abank2 = abank.flip(0).contiguous()                                          # a second programme: the same features in another order
    tracker = OffsetTracker(eng, mel, lam=0.5, posterior=True, gate=gate)
    both = tracker.track_features_programmes(vbank, torch.stack([abank, abank2]))
    assert len(both) == 2
    for got, ab in zip(both, (abank, abank2)):
        assert _same(got, tracker.track_features(vbank, ab), TRACK_FIELDS + POST_FIELDS + GATE_FIELDS)
    assert not torch.equal(both[0].gate_logits, both[1].gate_logits)
