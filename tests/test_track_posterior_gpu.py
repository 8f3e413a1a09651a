"""GPU: sf_track_posterior (the forward-backward read-out of a recording's window logits) against the float64 oracle of
tests/track_posterior_oracle.py, its identities, masked and non-finite input, the OffsetTracker integration and a replay under graph capture.

THE BAR IS MEASURED.  The yardstick is the contract's recurrences, literally (no renormalisation), in torch fp32 on the CPU (_yardstick below), compared with
the float64 oracle on the very inputs a test uses; per quantity

    post:    max |post - oracle|                                   mean:  max |offset_mean - oracle| / grid step
    log_z:   |log_z - oracle| / max(1, |oracle log_z|)

the kernel may be at most 4x the yardstick's worst value over all inputs of this file (computed once, in `refs`), with an absolute floor of 1e-6 for post.
The factor covers another expf / logf and another summation order, not another recurrence (1e-2 and above).  The yardstick does not renormalise, so its
scores grow with W and with the range of the logits: its worst post / mean values come from W = 4096 (50 * randn is next), its worst log_z from the grid
(W = 300, where |log_z| is small against the scores it is the lse of).  CEIL holds a fixed ceiling per quantity - those worst values, rounded up to one
digit - and the yardstick counts with at most its ceiling, so the bar cannot float with the CPU's libm.
cls_post is compared wherever the oracle's two largest marginals differ by more than the post bar; those windows are fewer than 1 % (asserted)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_posterior_oracle as TP  # noqa: E402

pytestmark = pytest.mark.gpu

QUANT = ('post', 'mean', 'log_z')
# the yardstick's worst (post, mean in grid steps, log_z) over the inputs below, rounded up to one digit (measured 9.8e-4, 8.6e-3, 4.9e-6: DESIGN 3.14)
CEIL = (1e-3, 9e-3, 5e-6)


def _grid(C: int) -> np.ndarray:
    return np.linspace(-2, 2, C).astype(np.float32)


def _lse32(x: torch.Tensor, dim: int) -> torch.Tensor:
    m = x.max(dim, keepdim=True).values
    sub = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    return (sub + torch.log(torch.exp(x - sub).sum(dim, keepdim=True))).squeeze(dim)


def _yardstick(x: np.ndarray, lam: float, grid: np.ndarray):
    """The recurrences of the contract in torch fp32 on the CPU, as the oracle states them in float64."""
    l, g = torch.from_numpy(x), torch.from_numpy(grid)
    assert l.dtype == torch.float32 and g.dtype == torch.float32
    e = l - _lse32(l, 1)[:, None]
    W, C = e.shape
    idx = torch.arange(C)
    pen = torch.tensor(lam, dtype=torch.float32) * (idx[:, None] - idx[None, :]).abs().float()        # pen[p, c]
    a, b = torch.empty(W, C), torch.empty(W, C)
    a[0] = e[0]
    for w in range(1, W):
        a[w] = e[w] + _lse32(a[w - 1][:, None] - pen, 0)
    b[W - 1] = 0
    for w in range(W - 2, -1, -1):
        b[w] = _lse32((b[w + 1] + e[w + 1])[:, None] - pen, 0)
    s = a + b
    post = torch.exp(s - _lse32(s, 1)[:, None])
    mean = torch.zeros(W)
    for c in range(C):                                                                               # ascending c, fp32
        mean = mean + post[:, c] * g[c]
    return dict(post=post.numpy(), offset_mean=mean.numpy(), log_z=float(_lse32(a[W - 1], 0)))


def _errors(got: dict, ref: dict, grid: np.ndarray, rows=None):
    """(post, mean, log_z) errors of `got` against the float64 `ref`; rows: compare only these windows (the others hold unspecified values)."""
    step = float(grid[1] - grid[0])
    sel = slice(None) if rows is None else rows
    return (float(np.abs(got['post'].astype(np.float64) - ref['post'])[sel].max()),
            float(np.abs(got['offset_mean'].astype(np.float64) - ref['offset_mean'])[sel].max()) / step,
            abs(float(got['log_z']) - ref['log_z']) / max(1.0, abs(ref['log_z'])))


# ---- the inputs: made once, with their oracle and yardstick, and never changed ---------------------------------------------------------------------
GRID_CASES = [(W, C, lam) for W in (1, 2, 9, 300) for C in (2, 21, 64) for lam in (0.0, 0.5, 1.0, 8.0)]


def _randn(seed: int, W: int, C: int, scale: float) -> np.ndarray:
    return (scale * np.random.default_rng(seed).standard_normal((W, C))).astype(np.float32)


def _masked_input():
    x = _randn(31, 40, 21, 3.0)
    x[:, 4] = -np.inf                                                            # a class masked in every window
    x[5:17, 11] = -np.inf                                                        # and one masked in some
    x[33, 11] = -np.inf
    return x


_INPUTS = {('grid', W, C, lam): (_randn(7 + 1000 * W + 10 * C + int(2 * lam), W, C, 3.0), lam) for W, C, lam in GRID_CASES}
_INPUTS[('strided',)] = (_randn(41, 130, 21, 3.0), 0.5)
_INPUTS[('drift',)] = (_randn(42, 4096, 21, 3.0), 1.0)
_INPUTS[('wide',)] = (_randn(43, 300, 21, 50.0), 8.0)
_INPUTS[('masked',)] = (_masked_input(), 1.0)


@pytest.fixture(scope='module')
def refs():
    """key -> dict(x, lam, grid, ref = float64 oracle, yard = the yardstick's (post, mean, log_z) errors); 'bar' -> the bar per quantity."""
    out = {}
    for key, (x, lam) in _INPUTS.items():
        grid = _grid(x.shape[1])
        ref = TP.posterior(x.astype(np.float64), lam, grid.astype(np.float64))
        out[key] = dict(x=x, lam=lam, grid=grid, ref=ref, yard=_errors(_yardstick(x, lam, grid), ref, grid))
    worst = [max(v['yard'][q] for v in out.values()) for q in range(3)]
    print(f'yardstick worst: post {worst[0]:.3e}  mean {worst[1]:.3e} steps  log_z {worst[2]:.3e} (ceilings {CEIL})')
    worst = [min(w, c) for w, c in zip(worst, CEIL)]                                                 # the bar does not float
    out['bar'] = (max(4 * worst[0], 1e-6), 4 * worst[1], 4 * worst[2])
    return out


def _run(gpu, x: np.ndarray, lam: float, grid: np.ndarray, ldl=None, ldp=None):
    from synchformer_amd import ops
    W, C = x.shape
    if ldl is None:
        xd = torch.from_numpy(x).to(gpu)
    else:                                                                        # a strided view: columns beyond C hold a value that would win every maximum
        buf = torch.full((W, ldl), 1e30, device=gpu, dtype=torch.float32)
        buf[:, :C] = torch.from_numpy(x).to(gpu)
        xd = buf[:, :C]
    pbuf = None if ldp is None else torch.full((W, ldp), -7.0, device=gpu, dtype=torch.float32)
    out = ops.track_posterior(xd, lam, torch.from_numpy(grid).to(gpu), post=None if pbuf is None else pbuf[:, :C])
    torch.cuda.synchronize()
    post, cls_post, conf_post, mean, log_z = out
    assert [t.dtype for t in out] == [torch.float32, torch.int32, torch.float32, torch.float32, torch.float32]
    assert post.shape == (W, C) and cls_post.shape == conf_post.shape == mean.shape == (W,) and log_z.shape == (1,)
    if pbuf is not None:
        assert (pbuf[:, C:] == -7.0).all(), 'the padding of post was written'
    return dict(post=post.cpu().numpy(), cls_post=cls_post.cpu().numpy(), conf_post=conf_post.cpu().numpy(), offset_mean=mean.cpu().numpy(),
                log_z=float(log_z.item()))


def _check(got: dict, case: dict, bar, rows=None, what=''):
    """Errors within the bar; rows of post sum to 1; conf_post is post at cls_post; cls_post is the oracle's argmax wherever that is decided by more than the bar."""
    ref, W = case['ref'], case['x'].shape[0]
    err = _errors(got, ref, case['grid'], rows)
    print(f'{what} lam {case["lam"]}: ' + '  '.join(f'{n} {e:.3e} (yardstick {y:.3e}, bar {b:.3e})' for n, e, y, b in zip(QUANT, err, case['yard'], bar)))
    sel = np.arange(W) if rows is None else rows
    assert all(np.isfinite(got[k]).all() for k in ('post', 'conf_post', 'offset_mean')) and np.isfinite(got['log_z'])
    assert all(e <= b for e, b in zip(err, bar)), (err, bar)
    assert np.abs(got['post'].sum(1) - 1)[sel].max() <= 1e-5
    assert got['log_z'] <= 1e-5
    assert got['cls_post'].min() >= 0 and got['cls_post'].max() < case['x'].shape[1]
    assert np.array_equal(got['conf_post'], got['post'][np.arange(W), got['cls_post']])
    top = np.sort(ref['post'], 1)
    decided = (top[:, -1] - top[:, -2] > bar[0])[sel]
    assert np.array_equal(got['cls_post'][sel][decided], ref['cls_post'][sel][decided])


def test_argmax_is_decided_in_the_oracle(refs):
    """Fewer than 1 % of the windows have the oracle's two largest marginals closer than the post bar (continuous random logits): the cls_post check covers the rest."""
    close = total = 0
    for key, case in refs.items():
        if key == 'bar':
            continue
        top = np.sort(case['ref']['post'], 1)
        close += int((top[:, -1] - top[:, -2] <= refs['bar'][0]).sum())
        total += top.shape[0]
    print(f'{close} of {total} windows undecided at the bar')
    assert close < 0.01 * total


@pytest.mark.parametrize('W, C, lam', GRID_CASES)
def test_posterior_against_oracle(gpu, refs, W, C, lam):
    case = refs[('grid', W, C, lam)]
    bar = refs['bar']
    got = _run(gpu, case['x'], lam, case['grid'])
    _check(got, case, bar, what=f'W {W} C {C}')
    if lam == 0.0 or W == 1:                                                     # independent windows: the softmax of each row, log_z = 0
        x = case['x'].astype(np.float64)
        p = np.exp(x - x.max(1, keepdims=True))
        assert np.abs(got['post'] - p / p.sum(1, keepdims=True)).max() <= bar[0] and abs(got['log_z']) <= bar[2], got['log_z']
    else:
        assert got['log_z'] < 0
    flipped = _run(gpu, case['x'][::-1].copy(), lam, case['grid'])                 # reversed rows: reversed marginals, the same partition sum
    assert np.abs(flipped['post'][::-1] - got['post']).max() <= 2 * bar[0]
    assert abs(flipped['log_z'] - got['log_z']) <= 2 * bar[2] * max(1.0, abs(case['ref']['log_z']))


def test_posterior_strided(gpu, refs):
    """ldl = C + 3 (the columns beyond C would win every maximum if read) and a post of row stride C + 5 (its padding stays as it was); bit-equal to the dense call."""
    case = refs[('strided',)]
    got = _run(gpu, case['x'], case['lam'], case['grid'], ldl=24, ldp=26)
    _check(got, case, refs['bar'], what='strided')
    dense = _run(gpu, case['x'], case['lam'], case['grid'])
    assert all(np.array_equal(got[k], dense[k]) for k in ('post', 'cls_post', 'conf_post', 'offset_mean')) and got['log_z'] == dense['log_z']


def test_posterior_does_not_drift(gpu, refs):
    """W = 4096: the per-step renormalisation keeps the scores bounded and the double accumulator keeps log_z (-11349.5 here) to fp32 precision."""
    case = refs[('drift',)]
    _check(_run(gpu, case['x'], case['lam'], case['grid']), case, refs['bar'], what='W 4096')


def test_posterior_wide_dynamic_range(gpu, refs):
    """50 * randn at lam = 8: logits 300 apart inside a row, exp(-160) = 0 in fp32 - the log-domain recursion stays finite and accurate."""
    case = refs[('wide',)]
    _check(_run(gpu, case['x'], case['lam'], case['grid']), case, refs['bar'], what='wide')


def test_posterior_masked_classes(gpu, refs):
    case = refs[('masked',)]
    got = _run(gpu, case['x'], case['lam'], case['grid'])
    _check(got, case, refs['bar'], what='masked')
    masked = np.isneginf(case['x'])
    assert masked[:, 4].all() and 0 < masked[:, 11].sum() < masked.shape[0]
    assert (got['post'][masked] == 0).all()


def test_posterior_non_finite_rows_stay_in_range(gpu):
    """A row of NaN and a row with +inf: values are unspecified, the call returns and every class written lies in [0, C)."""
    from synchformer_amd import ops
    x = _randn(3, 40, 21, 3.0)
    x[11, :] = np.nan
    x[23, 5] = np.inf
    out = ops.track_posterior(torch.from_numpy(x).to(gpu), 1.0, torch.from_numpy(_grid(21)).to(gpu))
    torch.cuda.synchronize()
    cls = out[1].cpu().numpy()
    assert cls.shape == (40,) and cls.min() >= 0 and cls.max() < 21, cls


def test_posterior_of_no_windows(gpu):
    from synchformer_amd import ops
    post, cls_post, conf_post, mean, log_z = ops.track_posterior(torch.empty(0, 21, device=gpu), 1.0, torch.from_numpy(_grid(21)).to(gpu))
    torch.cuda.synchronize()
    assert post.shape == (0, 21) and cls_post.shape == conf_post.shape == mean.shape == (0,) and log_z.shape == (1,)
    with pytest.raises(AssertionError):
        ops.track_posterior(torch.zeros(3, 21, device=gpu), 1.0, torch.from_numpy(_grid(20)).to(gpu))       # a grid of another length
    with pytest.raises(RuntimeError, match='lam must be finite'):
        ops.track_posterior(torch.zeros(3, 21, device=gpu), -1.0, torch.from_numpy(_grid(21)).to(gpu))


def test_posterior_under_graph_capture(gpu):
    """One call captured on a single stream and replayed equals the eager call bit for bit: the launcher neither synchronises nor allocates."""
    from synchformer_amd import ops
    x = torch.from_numpy(_randn(9, 9, 21, 3.0)).to(gpu)
    grid = torch.from_numpy(_grid(21)).to(gpu)
    eager = [t.clone() for t in ops.track_posterior(x, 1.0, grid)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = ops.track_posterior(x, 1.0, grid)
    for t in captured:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, captured))
    assert eager[0].sum().item() == pytest.approx(9.0, abs=1e-4)


def test_tracker_posterior_fields(gpu):
    """OffsetTracker(posterior=True) on a 20-segment bank (7 windows): every field of before is bit-equal to the posterior=False track, the new fields are
    ops.track_posterior on the track's own logits, bit for bit."""
    from synchformer_amd import ops, synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.track import OffsetTracker
    eng, mel = SynchformerEngine(synth.make_state_dict(1337), gpu), MelFrontend(gpu)
    g = torch.Generator().manual_seed(12)
    vbank, abank = torch.randn(20, 8, 768, generator=g).to(gpu), torch.randn(20, 6, 768, generator=g).to(gpu)
    plain = OffsetTracker(eng, mel, lam=0.5).track_features(vbank, abank)
    tracker = OffsetTracker(eng, mel, lam=0.5, posterior=True)
    tr = tracker.track_features(vbank, abank)
    torch.cuda.synchronize()
    old = ('t_sec', 'logits', 'cls_raw', 'conf_raw', 'cls_path', 'conf_path', 'offset_sec_raw', 'offset_sec_path')
    assert tr.logits.shape == (7, 21) and tr.n_segments == plain.n_segments == 20
    assert all(torch.equal(getattr(tr, n), getattr(plain, n)) for n in old)
    assert all(getattr(plain, n) is None for n in ('post', 'cls_post', 'conf_post', 'offset_sec_post', 'offset_sec_mean', 'log_z'))
    post, cls_post, conf_post, mean, log_z = ops.track_posterior(tr.logits, 0.5, tracker.grid)
    assert torch.equal(tr.post, post) and torch.equal(tr.cls_post, cls_post) and torch.equal(tr.conf_post, conf_post)
    assert torch.equal(tr.offset_sec_mean, mean) and torch.equal(tr.log_z, log_z) and torch.equal(tr.offset_sec_post, tracker.grid[cls_post.long()])
    assert tr.post.shape == (7, 21) and tr.cls_post.dtype == torch.int32 and tr.log_z.shape == (1,)
    assert tracker.grid.min() <= tr.offset_sec_mean.min() and tr.offset_sec_mean.max() <= tracker.grid.max()
    assert (tr.post.sum(1) - 1).abs().max().item() <= 1e-5 and tr.log_z.item() <= 1e-5
