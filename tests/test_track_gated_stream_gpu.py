"""GPU: sf_track_stream_push_gated / sf_track_pool_push_gated (the fixed-lag read-outs of a live feed over (offset class, synchronizable flag)) against
the float64 oracle of tests/track_gated_stream_oracle.py, and the gated stream / pool / programme feeds of OffsetTracker.

THE PATH is judged by the MAX-MARGINAL, not index by index: plane 0 of the emission is flat, exact ties are the rule.  A committed (cls, sync) of
window w, read from the prefix 0 .. t, is correct iff the best path of that prefix through it lies within (t + 1) * 2^-13 of the prefix's optimum - PATH_TOL of
tests/test_track_gated_gpu.py per window of the prefix, with that file's derivation.  test_the_inputs_discriminate asserts from the oracle alone that the offline
path, the read-out at lag + 1 and the per-row argmax each VIOLATE that bound on this file's input, so the input cannot quietly become one that proves nothing.
Where the margins are whole logits (the gap scenario: >= 0.5 logit between the best and the second-best state over all prefixes,
test_track_gated_stream_cpu.py::test_gap_scenario_margins) indices are compared exactly.

THE POSTERIOR BAR is built by the method of DESIGN 3.14 / 3.20: the contract's recurrences in torch fp32 on the CPU (test_track_gated_gpu._yardstick) on every
prefix of this file's posterior inputs, against float64; the kernel may be at most 4x the yardstick's worst, each yardstick value capped by that file's CEIL, with
an absolute floor of 1e-6 for post."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_track_gated_gpu as G  # noqa: E402  (PATH_TOL, CEIL, _yardstick, _errors, _dev_inputs, the end-to-end recording)
import track_gated_oracle as TG  # noqa: E402
import track_gated_stream_oracle as GS  # noqa: E402
import track_stream_oracle as TS  # noqa: E402
from test_track_gated_gpu import rec  # noqa: E402,F401  (the 17-segment recording, the seg_chunk = 5 engine, the synthetic 184-token gate)

pytestmark = pytest.mark.gpu

W_RUN = 70
LAMS, MUS = (0.0, 0.5, 2.0, 8.0), (0.0, 2.0, 16.0)
COMMITTED = ('cls_lag', 'sync_lag', 'conf_lag')
POSTERIOR = ('post_lag', 'p_sync_lag', 'cls_post_lag', 'conf_post_lag', 'offset_mean_lag')
RAW = ('cls_raw', 'conf_raw', 'sync_raw')
assert GS.path_tol(0) == G.PATH_TOL


def _inputs(C: int):
    return GS.stream_inputs(100 * C, W_RUN, C)                                   # (C = 21: seed 2100, the input test_track_gated_stream_cpu.py judges too)


_MM = {}


def _mm(C: int, W: int, lam: float, mu: float):
    """The max-marginals of every prefix of the first W rows of _inputs(C): computed once, shared by every lag and chunking."""
    key = (C, lam, mu)
    if key not in _MM:
        _MM[key] = GS.prefix_max_marginals(*_inputs(C), lam, mu)
    return _MM[key][:W]                                                          # (a prefix of the input has the prefixes of the input)


def _np(out) -> dict:
    return {k: (v if v is None or isinstance(v, int) else v.cpu().numpy()) for k, v in out._asdict().items()}


def _pushes(chunks):
    return [(n, False) for n in chunks] + [(0, True)]


def _run(gpu, x, z, lam, mu, lag, pushes, posterior=False, strided=False):
    """One gated stream over the rows of (x, z) in `pushes` -> (state, [dict of numpy per push])."""
    from synchformer_amd import ops
    C = x.shape[1]
    state = ops.track_stream_state_gated(C, lag, posterior, gpu)
    xd, zd = G._dev_inputs(gpu, x, z, *((C + 3, 5) if strided else (None, None)))
    grid = torch.from_numpy(G._grid(C)).to(gpu) if posterior else None
    size, outs, row = state.buf.numel(), [], 0
    for n, final in pushes:
        outs.append(ops.track_stream_push_gated(state, xd[row:row + n], zd[row:row + n], lam, mu, grid, final=final))
        row += n
    torch.cuda.synchronize()
    assert state.buf.numel() == size and state.rows == row and row == x.shape[0]
    return state, [_np(o) for o in outs]


def _cat(outs, keys):
    return {k: np.concatenate([o[k] for o in outs]) for k in keys}


def _in_range(outs, C):
    for o in outs:
        for k in ('cls_raw', 'cls_lag', 'cls_tail', 'cls_post_lag'):
            if o[k] is not None and o[k].size:
                assert o[k].min() >= 0 and o[k].max() < C, (k, o[k])
        for k in ('sync_lag', 'sync_tail'):
            assert set(np.unique(o[k])) <= {0, 1}, (k, o[k])


def _worst_gap(mm, lag, pushes, outs):
    """Asserts the max-marginal criterion on every committed window and every push's tail -> the worst gap."""
    lagged, tail = GS.gaps(mm, lag, pushes, outs)
    for w, t, g in lagged + tail:
        assert -1e-9 <= g <= GS.path_tol(t), (w, t, g, GS.path_tol(t))
    return max([g for _, _, g in lagged + tail], default=0.0)


@pytest.mark.parametrize('lam', [0.5, 1.0, 2.0])
def test_the_inputs_discriminate(lam):
    """From the oracle alone, on THIS file's input at C = 21: the float64 read-out at `lag` satisfies the bound everywhere; the offline path, the read-out at
    lag + 1 and the per-row argmax each violate it in at least one window - for every lag <= 9 the tests below use."""
    l, z = _inputs(21)
    pre, mm = GS.prefix_readouts(l, z, lam, 2.0), GS.prefix_max_marginals(l, z, lam, 2.0)
    for lag in (0, 1, 7, 8, 9):
        bad = GS.discriminations(l, z, lam, 2.0, lag, pre, mm)
        print(f'lam {lam} lag {lag}: windows that violate the bound: {bad}')
        assert bad['oracle'] == 0 and bad['offline'] >= 1 and bad['lag+1'] >= 1 and bad['argmax'] >= 1, (lam, lag, bad)


@pytest.mark.parametrize('lag', [0, 1, 7, 8, 9, 63])
@pytest.mark.parametrize('C', [2, 21, 32])
def test_max_marginal_criterion_and_chunking_invariance(gpu, C, lag):
    """W = 70 over lam x mu x four chunkings: every committed window and every push's tail is an optimum of its prefix within the margin; all chunkings give
    bit-equal classes, flags and floats (the tails: equal to the one-row-per-push run's at every common boundary).  W in {lag, lag + 1, lag + 2}: the same at
    the edge where nothing / one / two windows are committed before the flush."""
    x, z = _inputs(C)
    worst = 0.0
    for lam in LAMS:
        for mu in MUS:
            mm = _mm(C, W_RUN, lam, mu)
            ref = ones_tails = None
            for name in ('ones', 'whole', 'ragged', 'long_after_short'):         # (one row per push first: it has the tail after every row)
                pushes = _pushes(TS.chunking(name, W_RUN, lag))
                _, outs = _run(gpu, x, z, lam, mu, lag, pushes)
                _in_range(outs, C)
                worst = max(worst, _worst_gap(mm, lag, pushes, outs))
                got = _cat(outs, COMMITTED + RAW)
                tails, row = {}, 0
                for (n, final), o in zip(pushes, outs):
                    row += n
                    if not final:
                        tails[row] = (o['cls_tail'], o['sync_tail'], o['conf_tail'])
                if ref is None:
                    ref, ones_tails = got, tails
                    assert got['cls_lag'].shape == (W_RUN,) and np.array_equal(got['cls_raw'], x.argmax(1))
                else:
                    assert all(np.array_equal(got[k], ref[k]) for k in got), (name, lam, mu)
                    assert all(np.array_equal(a, b) for row, t in tails.items() for a, b in zip(t, ones_tails[row])), (name, lam, mu)
    for W in sorted({max(lag, 1), lag + 1, lag + 2}):
        for name in ('whole', 'ones'):
            pushes = _pushes(TS.chunking(name, W, lag))
            _, outs = _run(gpu, x[:W], z[:W], 0.5, 2.0, lag, pushes)
            _in_range(outs, C)
            worst = max(worst, _worst_gap(_mm(C, W, 0.5, 2.0), lag, pushes, outs))
            assert sum(len(o['cls_lag']) for o in outs) == W and sum(len(o['cls_lag']) for o in outs[:-1]) == max(0, W - lag)
    print(f'C {C} lag {lag}: worst max-marginal gap {worst:.3e} (allowed per window of the prefix {G.PATH_TOL:.3e})')


def test_strided_views_with_poisoned_padding(gpu):
    """ldl = C + 3, ldg = 5, the columns beyond the width holding 1e30: bit-equal to the dense run, with and without the posterior."""
    x, z = _inputs(21)
    pushes = _pushes(TS.chunking('ragged', W_RUN, 8))
    for posterior in (False, True):
        _, dense = _run(gpu, x, z, 0.5, 2.0, 8, pushes, posterior)
        _, strided = _run(gpu, x, z, 0.5, 2.0, 8, pushes, posterior, strided=True)
        for a, b in zip(dense, strided):
            assert all(np.array_equal(a[k], b[k]) for k in a if a[k] is not None and not isinstance(a[k], int))


# ---- the posterior: the bar, made once -------------------------------------------------------------------------------------------------------------------------
POST_CASES = [(2, 0.5, 2.0), (2, 8.0, 16.0), (21, 0.0, 0.0), (21, 0.5, 2.0), (21, 2.0, 0.0), (21, 8.0, 16.0), (32, 0.5, 2.0), (32, 8.0, 16.0)]
POST_LAGS = (0, 1, 7, 8, 9, 63)


@pytest.fixture(scope='module')
def post_refs():
    """(C, lam, mu) -> dict(pre = the float64 read-outs of every prefix, yard = the yardstick's worst errors over the prefixes); 'bar' -> the bar per quantity."""
    out = {}
    for C, lam, mu in POST_CASES:
        x, z = _inputs(C)
        grid = G._grid(C)
        pre = GS.prefix_readouts(x, z, lam, mu, grid.astype(np.float64))
        yard = np.max([G._errors(G._yardstick(x[:t + 1], z[:t + 1], lam, mu, grid), pre[1][t], grid) for t in range(W_RUN)], axis=0)
        out[(C, lam, mu)] = dict(pre=pre, yard=tuple(float(v) for v in yard))
    worst = [max(v['yard'][q] for v in out.values()) for q in range(4)]
    print('yardstick worst: ' + '  '.join(f'{n} {w:.3e}' for n, w in zip(G.QUANT, worst)) + f' (ceilings {G.CEIL})')
    worst = [min(w, c) for w, c in zip(worst, G.CEIL)]                           # the bar does not float
    out['bar'] = (max(4 * worst[0], 1e-6), 4 * worst[1], 4 * worst[2], 4 * worst[3])
    return out


def _posterior_errors(outs, want, grid):
    """(post, p_sync, mean in grid steps, log_z relative) of a run's pushes against by_definition's."""
    step = float(grid[1] - grid[0])
    err = [0.0, 0.0, 0.0, 0.0]
    for o, d in zip(outs, want):
        if len(d['cls_lag']):
            err[0] = max(err[0], float(np.abs(o['post_lag'].astype(np.float64) - d['post_lag']).max()))
            err[1] = max(err[1], float(np.abs(o['p_sync_lag'].astype(np.float64) - d['p_sync_lag']).max()))
            err[2] = max(err[2], float(np.abs(o['offset_mean_lag'].astype(np.float64) - d['offset_mean_lag']).max()) / step)
        err[3] = max(err[3], abs(float(o['log_z'][0]) - d['log_z']) / max(1.0, abs(d['log_z'])))
    return err


@pytest.mark.parametrize('C, lam, mu', POST_CASES)
def test_posterior_under_a_lag(gpu, post_refs, C, lam, mu):
    """post_lag, p_sync_lag, offset_mean_lag and every push's log_z against the float64 read-outs of the prefixes, under the measured bar; the four chunkings are
    bit-equal; the Viterbi block does not depend on the posterior."""
    x, z = _inputs(C)
    grid, bar, case = G._grid(C), post_refs['bar'], post_refs[(C, lam, mu)]
    worst = [0.0] * 4
    for lag in POST_LAGS:
        ref = None
        for name in TS.CHUNKINGS:
            pushes = _pushes(TS.chunking(name, W_RUN, lag))
            _, outs = _run(gpu, x, z, lam, mu, lag, pushes, posterior=True)
            _in_range(outs, C)
            got = _cat(outs, COMMITTED + POSTERIOR)
            got['log_z'] = outs[-1]['log_z']
            if ref is None:
                ref = got
                want = GS.by_definition(x, z, lam, mu, lag, pushes, grid.astype(np.float64), case['pre'])
                err = _posterior_errors(outs, want, grid)
                worst = [max(a, b) for a, b in zip(worst, err)]
                assert all(e <= b for e, b in zip(err, bar)), (lag, err, bar)
                assert np.isfinite(got['post_lag']).all() and np.abs(got['post_lag'].sum(1) - 1).max() <= 1e-5
                assert got['p_sync_lag'].min() >= 0 and got['p_sync_lag'].max() <= 1 and all(float(o['log_z'][0]) <= 1e-5 for o in outs)
                assert np.array_equal(got['conf_post_lag'], got['post_lag'][np.arange(W_RUN), got['cls_post_lag']])
                full = np.concatenate([d['post_lag'] for d in want])
                assert (full[np.arange(W_RUN), got['cls_post_lag']] >= full.max(1) - bar[0]).all()      # the chosen class: the oracle's best, or within the bar of it
                _, plain = _run(gpu, x, z, lam, mu, lag, pushes, posterior=False)
                assert all(np.array_equal(_cat(plain, COMMITTED)[k], got[k]) for k in COMMITTED)
            else:
                assert all(np.array_equal(got[k], ref[k]) for k in got), (name, lag)
    print(f'C {C} lam {lam} mu {mu}: kernel worst ' + '  '.join(f'{n} {e:.3e} (yardstick {y:.3e}, bar {b:.3e})' for n, e, y, b in zip(G.QUANT, worst, case['yard'], bar)))


def test_long_run(gpu, post_refs):
    """W = 4096, lag = 16, 64 rows per push: log_z after every push against the float64 forward pass under the same relative bar, p_sync_lag and post_lag on every
    64th window, and the state buffer's size unchanged at the end."""
    from synchformer_amd import ops
    W, C, lag, lam, mu = 4096, 21, 16, 1.0, 2.0
    x, z = GS.stream_inputs(4096, W, C)
    grid, bar = G._grid(C), post_refs['bar']
    l64, z64 = x.astype(np.float64), z.astype(np.float64)
    E, T = TG.emission(l64, z64), TG.transition(C, lam, mu)
    a = np.empty((W, 2 * C))
    a[0] = E[0]
    for w in range(1, W):
        a[w] = E[w] + TG.lse(a[w - 1][:, None] + T, axis=0)
    log_z = TG.lse(a, axis=1)
    state = ops.track_stream_state_gated(C, lag, True, gpu)
    size = state.buf.numel()
    xd, zd, gd = torch.from_numpy(x).to(gpu), torch.from_numpy(z).to(gpu), torch.from_numpy(grid).to(gpu)
    outs = [ops.track_stream_push_gated(state, xd[r:r + 64], zd[r:r + 64], lam, mu, gd) for r in range(0, W, 64)]
    outs.append(ops.track_stream_push_gated(state, xd[:0], zd[:0], lam, mu, gd, final=True))
    torch.cuda.synchronize()
    assert state.buf.numel() == size == ops._lib.load().sf_track_stream_gated_bytes(C, lag, 1) and state.rows == W
    outs = [_np(o) for o in outs]
    _in_range(outs, C)
    worst_z = max(abs(float(o['log_z'][0]) - log_z[64 * (i + 1) - 1]) / max(1.0, abs(log_z[64 * (i + 1) - 1])) for i, o in enumerate(outs[:-1]))
    got = _cat(outs, COMMITTED + POSTERIOR)
    assert got['cls_lag'].shape == (W,)
    worst_p = worst_s = 0.0
    for w in range(0, W, 64):
        R = min(w + lag, W - 1)
        b = np.zeros(2 * C)
        for r in range(R, w, -1):
            b = TG.lse((b + E[r])[None, :] + T, axis=1)
        post2 = np.exp(a[w] + b - TG.lse(a[w] + b))
        worst_p = max(worst_p, float(np.abs(got['post_lag'][w] - (post2[:C] + post2[C:])).max()))
        worst_s = max(worst_s, abs(float(got['p_sync_lag'][w]) - post2[C:].sum()))
    print(f'W 4096: log_z {worst_z:.3e} (bar {bar[3]:.3e})  post {worst_p:.3e} (bar {bar[0]:.3e})  p_sync {worst_s:.3e} (bar {bar[1]:.3e})')
    assert worst_z <= bar[3] and worst_p <= bar[0] and worst_s <= bar[1]


# ---- scenarios with margins of whole logits: exact indices -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mu', [0.0, 2.0, 16.0])
@pytest.mark.parametrize('lam', [0.5, 1.0])
def test_gap_scenario_under_a_lag(gpu, lam, mu):
    """The music bed of DESIGN 3.20 read live: compared exactly with the oracle's prefix Viterbi at every lag (margins >= 0.5 logit).  mu in {0, 2}, every lag: class
    13 in all 60 windows, flag 0 exactly on windows 22 .. 36, while the ungated stream of the same logits follows the decoy on 15 windows - those 15, except at
    lam = 1, lag = 0, where a decision without look-ahead needs two decoy rows to pay for the switch and the 15 are 23 .. 37 (the float64 ungated oracle says so).
    mu = 16, lag <= 1: the flag lags by one to three windows - the oracle says so, and the kernel agrees."""
    from synchformer_amd import ops
    l, z = TG.gap_scenario()
    x32, z32 = l.astype(np.float32), z.astype(np.float32)
    W = l.shape[0]
    pre = GS.prefix_readouts(l, z, lam, mu)
    ungated = [TS.viterbi(l[:t + 1], lam) for t in range(W)]
    late = 0
    for lag in (0, 1, 4, 16, 59):
        pushes = _pushes(TS.chunking('ragged', W, lag))
        want = GS.by_definition(l, z, lam, mu, lag, pushes, pre=pre)
        _, outs = _run(gpu, x32, z32, lam, mu, lag, pushes)
        for o, d in zip(outs, want):
            assert all(np.array_equal(o[k], d[k]) for k in ('cls_lag', 'sync_lag', 'cls_tail', 'sync_tail', 'cls_raw')), (lag, o, d)
        got = _cat(outs, COMMITTED)
        gap = np.flatnonzero(got['sync_lag'] == 0)
        if mu < 16 or lag >= 4:
            assert (got['cls_lag'] == 13).all() and np.array_equal(gap, np.arange(22, 37)), (lag, got)
        elif not np.array_equal(gap, np.arange(22, 37)):
            late += 1
            assert 1 <= gap[0] - 22 <= 3, gap
        state = ops.track_stream_state(21, lag, False, gpu)
        xd = torch.from_numpy(x32).to(gpu)
        plain, row = [], 0
        for n, final in pushes:
            plain.append(ops.track_stream_push(state, xd[row:row + n], lam, final=final).cls_lag.cpu().numpy())
            row += n
        plain = np.concatenate(plain)
        assert np.array_equal(plain, [ungated[min(w + lag, W - 1)][w] for w in range(W)])
        decoy = np.flatnonzero(plain == 2)
        assert np.array_equal(decoy, np.arange(23, 38) if (lam, lag) == (1.0, 0) else np.arange(22, 37)), (lag, decoy)
    assert late == (0 if mu < 16 else (2 if lam == 0.5 else 1)), late


@pytest.mark.parametrize('lam', [0.5, 1.0, 8.0])
def test_a_confident_gate_changes_nothing(gpu, lam):
    """d = +30 everywhere: sync_lag == 1 and cls_lag is the ungated stream's on the same logits, at every lag."""
    from synchformer_amd import ops
    l, z = TG.gap_scenario()
    z[:, 0], z[:, 1] = 0.0, 30.0
    x32, z32 = l.astype(np.float32), z.astype(np.float32)
    for lag in (0, 1, 4, 16):
        pushes = _pushes(TS.chunking('ragged', l.shape[0], lag))
        _, outs = _run(gpu, x32, z32, lam, 2.0, lag, pushes)
        got = _cat(outs, COMMITTED)
        state, xd, plain, row = ops.track_stream_state(21, lag, False, gpu), torch.from_numpy(x32).to(gpu), [], 0
        for n, final in pushes:
            plain.append(ops.track_stream_push(state, xd[row:row + n], lam, final=final).cls_lag.cpu().numpy())
            row += n
        assert (got['sync_lag'] == 1).all() and np.array_equal(got['cls_lag'], np.concatenate(plain)), lag
        assert all((o['sync_tail'] == 1).all() for o in outs)


@pytest.mark.parametrize('C', [2, 21, 32])
def test_offline_limit(gpu, C):
    """lag = 255 >= W: the flush gives ops.track_decode_gated / ops.track_posterior_gated on the whole input, every field bit for bit."""
    from synchformer_amd import ops
    x, z = _inputs(C)
    xd, zd, grid = torch.from_numpy(x).to(gpu), torch.from_numpy(z).to(gpu), torch.from_numpy(G._grid(C)).to(gpu)
    for lam, mu in ((0.5, 2.0), (8.0, 0.0)):
        for name in ('whole', 'ragged'):
            _, outs = _run(gpu, x, z, lam, mu, 255, _pushes(TS.chunking(name, W_RUN, 255)), posterior=True)
            assert all(len(o['cls_lag']) == 0 for o in outs[:-1])
            last = outs[-1]
            dec = [t.cpu().numpy() for t in ops.track_decode_gated(xd, zd, lam, mu)]
            post = [t.cpu().numpy() for t in ops.track_posterior_gated(xd, zd, lam, mu, grid)]
            assert np.array_equal(last['cls_lag'], dec[3]) and np.array_equal(last['sync_lag'], dec[4]) and np.array_equal(last['conf_lag'], dec[5])
            assert np.array_equal(_cat(outs, RAW)['sync_raw'], dec[2]) and np.array_equal(_cat(outs, RAW)['conf_raw'], dec[1])
            for k, t in zip(('post_lag', 'p_sync_lag', 'cls_post_lag', 'conf_post_lag', 'offset_mean_lag', 'log_z'), post):
                assert np.array_equal(last[k], t), (k, name, lam, mu)
            # the tail before the flush is the offline path too
            assert np.array_equal(outs[-2]['cls_tail'], dec[3]) and np.array_equal(outs[-2]['sync_tail'], dec[4])


def test_interleaved_streams(gpu):
    """Two streams pushed alternately equal the two pushed one after the other: a push touches its own state only."""
    from synchformer_amd import ops
    xa, za = _inputs(21)
    xb, zb = GS.stream_inputs(77, W_RUN, 21)
    pushes = _pushes(TS.chunking('ragged', W_RUN, 7))
    _, alone_a = _run(gpu, xa, za, 0.5, 2.0, 7, pushes, posterior=True)
    _, alone_b = _run(gpu, xb, zb, 0.5, 2.0, 7, pushes, posterior=True)
    grid = torch.from_numpy(G._grid(21)).to(gpu)
    dev = [tuple(torch.from_numpy(t).to(gpu) for t in pair) for pair in ((xa, za), (xb, zb))]
    states = [ops.track_stream_state_gated(21, 7, True, gpu) for _ in range(2)]
    got, row = ([], []), 0
    for n, final in pushes:
        for i in range(2):
            got[i].append(_np(ops.track_stream_push_gated(states[i], dev[i][0][row:row + n], dev[i][1][row:row + n], 0.5, 2.0, grid, final=final)))
        row += n
    for mine, alone in zip(got, (alone_a, alone_b)):
        for a, b in zip(mine, alone):
            assert all(np.array_equal(a[k], b[k]) for k in a if not isinstance(a[k], int))


def test_a_push_under_graph_capture(gpu):
    """One single-stream push captured on one stream and replayed once equals the eager push: outputs and state bytes."""
    from synchformer_amd import ops
    x, z = _inputs(21)
    xd, zd, grid = torch.from_numpy(x).to(gpu), torch.from_numpy(z).to(gpu), torch.from_numpy(G._grid(21)).to(gpu)
    a, b = (ops.track_stream_state_gated(21, 8, True, gpu) for _ in range(2))
    for st in (a, b):
        ops.track_stream_push_gated(st, xd[:13], zd[:13], 0.5, 2.0, grid)
    assert torch.equal(a.buf, b.buf)
    eager = ops.track_stream_push_gated(a, xd[13:24], zd[13:24], 0.5, 2.0, grid)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = ops.track_stream_push_gated(b, xd[13:24], zd[13:24], 0.5, 2.0, grid)
    for t in captured[1:]:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert captured.w0 == eager.w0 == 5 and all(torch.equal(p, q) for p, q in zip(eager[1:], captured[1:]))
    assert torch.equal(a.buf, b.buf) and a.rows == b.rows == 24
    assert eager.cls_lag.shape == (11,) and eager.cls_tail.shape == (8,)


def test_non_finite_rows_stay_in_range(gpu):
    """Rows of NaN and rows with infinities, in either input: values are unspecified, every index written lies in [0, C) / {0, 1}."""
    x, z = GS.stream_inputs(3, 40, 21)
    x[11, :] = np.nan
    x[23, 5] = np.inf
    x[29, 7] = -np.inf
    z[5, 1] = np.nan
    z[17, 0] = np.inf
    z[31, :] = -np.inf
    for lag in (0, 7, 255):
        for name in ('whole', 'ragged'):
            _, outs = _run(gpu, x, z, 1.0, 2.0, lag, _pushes(TS.chunking(name, 40, lag)), posterior=True)
            _in_range(outs, 21)
            assert sum(len(o['cls_lag']) for o in outs) == 40
            assert np.array_equal(_cat(outs, RAW)['cls_raw'][:11], x[:11].argmax(1))


def test_pool_equals_single_streams(gpu):
    """5 streams with unequal counts - 0 rows and a final among them - pushed in one call equal track_stream_push_gated on each stream alone, bit for bit, state
    bytes included; a reopened slot starts fresh."""
    from synchformer_amd import ops
    C, lag, lam, mu = 21, 7, 0.5, 2.0
    grid = torch.from_numpy(G._grid(C)).to(gpu)
    data = [tuple(torch.from_numpy(t).to(gpu) for t in GS.stream_inputs(500 + i, 60, C)) for i in range(5)]
    slots = [3, 0, 6, 1, 4]
    ticks = [([3, 0, 20, 7, 1], ()), ([2, 5, 0, 30, 4], (0, 1)), ([9, 0, 11, 0, 2], (6,))]      # counts per stream (in `slots` order), the slots that close
    for posterior in (False, True):
        pool = ops.track_pool_state_gated(7, C, lag, posterior, gpu)
        singles = [ops.track_stream_state_gated(C, lag, posterior, gpu) for _ in range(5)]
        rows = [0] * 5
        for counts, final in ticks:
            live = [i for i in range(5) if not pool.closed[slots[i]]]
            xs = torch.cat([data[i][0][rows[i]:rows[i] + counts[i]] for i in live])
            zs = torch.cat([data[i][1][rows[i]:rows[i] + counts[i]] for i in live])
            outs = ops.track_pool_push_gated(pool, [slots[i] for i in live], xs, zs, [counts[i] for i in live], lam, mu, grid if posterior else None, final=final)
            for i, out in zip(live, outs):
                one = ops.track_stream_push_gated(singles[i], data[i][0][rows[i]:rows[i] + counts[i]], data[i][1][rows[i]:rows[i] + counts[i]], lam, mu,
                                                  grid if posterior else None, final=slots[i] in final)
                a, b = _np(out), _np(one)
                assert all(np.array_equal(a[k], b[k]) if a[k] is not None else b[k] is None for k in a), (posterior, i, counts)
                assert torch.equal(pool.buf[slots[i]], singles[i].buf), (posterior, i)
                rows[i] += counts[i]
        # slot 0 (closed above) is reopened: the stale bytes are not read, the new stream is a fresh one
        pool.reopen(0)
        fresh = ops.track_stream_state_gated(C, lag, posterior, gpu)
        out = ops.track_pool_push_gated(pool, [0], data[0][0][:12], data[0][1][:12], [12], lam, mu, grid if posterior else None)[0]
        one = ops.track_stream_push_gated(fresh, data[0][0][:12], data[0][1][:12], lam, mu, grid if posterior else None)
        a, b = _np(out), _np(one)
        assert all(np.array_equal(a[k], b[k]) if a[k] is not None else b[k] is None for k in a)
        torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------------------------------
# end to end: the 17-segment recording, the seg_chunk = 5 engine and the synthetic 184-token gate of tests/test_track_gated_gpu.py
# ----------------------------------------------------------------------------------------------------------------------------------------------
UPDATE_TENSORS = ('logits', 'cls_raw', 'conf_raw', 't_sec', 'cls_lag', 'conf_lag', 'offset_sec_lag', 't_sec_tail', 'cls_tail', 'conf_tail', 'offset_sec_tail', 'post_lag',
                  'cls_post_lag', 'conf_post_lag', 'offset_sec_post_lag', 'offset_sec_mean_lag', 'log_z')
UPDATE_GATE = ('gate_logits', 'sync_raw', 'sync_lag', 'sync_tail', 'p_sync_lag')
RAGGED = [(40, 20000), (0, 30000), (57, 0), (30, 30000), (17, 12160)]           # frames, samples per push: 144 frames and 92160 samples in all, at their own pace


def _same_update(a, b, names):
    for n in names:
        x, y = getattr(a, n), getattr(b, n)
        if (x is None) != (y is None) or (x is not None and not torch.equal(x, y)):
            return False
    return a.w_new == b.w_new and a.w0 == b.w0


def _feed(stream, frames, wave):
    """The ragged pushes plus flush -> the list of updates; held <= held_bound after every push."""
    upds, f, s = [], 0, 0
    for df, ds in RAGGED:
        upds.append(stream.push(frames[f:f + df], wave[s:s + ds]))
        f, s = f + df, s + ds
        assert all(stream.held[k] <= stream.held_bound[k] for k in stream.held), (stream.held, stream.held_bound)
    upds.append(stream.flush())
    return upds


@pytest.mark.parametrize('lag', [0, 3, 16])
def test_stream_gated_end_to_end(gpu, rec, lag):
    """Ragged pushes plus flush through stream(lag, gated=True) give track()'s logits and gate_logits bit for bit; with lag >= 3 (the recording has 4 windows) also its
    cls_path, sync_path and p_sync.  gated=False on the same tracker equals a tracker without a gate, field for field."""
    from synchformer_amd.track import OffsetTracker
    eng, gate, mel, frames, wave = (rec[k] for k in ('eng', 'gate', 'mel', 'frames', 'wave'))
    tracker = OffsetTracker(eng, mel, lam=0.5, posterior=True, gate=gate, mu=1.5)
    track = tracker.track(frames, wave)
    upds = _feed(tracker.stream(lag, gated=True), frames, wave)
    cat = lambda name: torch.cat([getattr(u, name) for u in upds])
    assert torch.equal(cat('logits'), track.logits) and torch.equal(cat('gate_logits'), track.gate_logits) and torch.equal(cat('sync_raw'), track.sync_raw)
    assert torch.equal(cat('cls_raw'), track.cls_raw) and cat('cls_lag').shape == (4,) and cat('sync_lag').dtype == torch.int32
    assert all(u.sync_tail.shape == u.cls_tail.shape and u.p_sync_lag.shape == u.cls_lag.shape for u in upds)
    if lag >= 3:
        assert torch.equal(cat('cls_lag'), track.cls_path) and torch.equal(cat('sync_lag'), track.sync_path) and torch.equal(cat('p_sync_lag'), track.p_sync)
        assert torch.equal(cat('conf_lag'), track.conf_path) and torch.equal(cat('post_lag'), track.post) and torch.equal(upds[-1].log_z, track.log_z)
    plain = _feed(OffsetTracker(eng, mel, lam=0.5, posterior=True).stream(lag), frames, wave)
    ungated = _feed(tracker.stream(lag, gated=False), frames, wave)
    for a, b in zip(ungated, plain):
        assert _same_update(a, b, UPDATE_TENSORS) and all(getattr(a, n) is None for n in UPDATE_GATE)


def test_pool_gated_end_to_end(gpu, rec):
    """A 3-feed pool(gated=True) equals three gated streams, field for field (the feeds at their own pace, one of them flushed early)."""
    from synchformer_amd.track import OffsetTracker
    eng, gate, mel, frames, wave = (rec[k] for k in ('eng', 'gate', 'mel', 'frames', 'wave'))
    tracker = OffsetTracker(eng, mel, lam=0.5, posterior=True, gate=gate, mu=1.5)
    feeds_data = [(frames, wave), (frames.flip(0).contiguous(), wave.flip(0).contiguous()), (frames[:136], wave[:87040])]
    cuts = [[(0, 0), (128, 81920), (144, 92160)], [(0, 0), (136, 87040), (144, 92160)], [(0, 0), (120, 76800), (136, 87040)]]
    pool = tracker.pool(3, lag=2, gated=True)
    handles = [pool.open() for _ in range(3)]
    streams = [tracker.stream(2, gated=True) for _ in range(3)]
    for tick in range(2):
        data = {h: (fr[c[tick][0]:c[tick + 1][0]], wv[c[tick][1]:c[tick + 1][1]]) for h, (fr, wv), c in zip(handles, feeds_data, cuts)}
        got = pool.push(data, flush=[handles[2]] if tick == 1 else ())
        for h, s in zip(handles, streams):
            want = s.push(*data[h])
            if tick == 1 and h is handles[2]:
                last = s.flush()                                                 # the pool's flush tick = the stream's push and flush: the committed blocks back to back
                assert torch.equal(got[h].cls_lag, torch.cat([want.cls_lag, last.cls_lag])) and torch.equal(got[h].sync_lag, torch.cat([want.sync_lag, last.sync_lag]))
                assert torch.equal(got[h].p_sync_lag, torch.cat([want.p_sync_lag, last.p_sync_lag])) and torch.equal(got[h].gate_logits, want.gate_logits)
            else:
                assert _same_update(got[h], want, UPDATE_TENSORS + UPDATE_GATE), (tick, h.slot)
            assert all(h.held[k] <= h.held_bound[k] for k in h.held)


def test_programme_stream_gated_end_to_end(gpu, rec):
    """A ProgrammeStream with P = 2 (two mono programmes of a 2-channel wave) equals two gated streams fed those channels."""
    from synchformer_amd.ingest import RecordingIngest
    from synchformer_amd.track import OffsetTracker
    eng, gate, mel, frames, wave = (rec[k] for k in ('eng', 'gate', 'mel', 'frames', 'wave'))
    tracker = OffsetTracker(eng, mel, lam=0.5, posterior=True, gate=gate, mu=1.5)
    waves = torch.stack([wave, wave.flip(0)])
    ing = RecordingIngest(gpu, 25, (224, 224), 16000, audio_channels=2, programmes=[0, 1])
    prog = tracker.stream(lag=2, ingest=ing, gated=True)
    singles = [tracker.stream(lag=2, ingest=RecordingIngest(gpu, 25, (224, 224), 16000), gated=True) for _ in range(2)]
    f = s = 0
    for df, ds in RAGGED + [(None, None)]:
        if df is None:
            got, want = prog.flush(), [x.flush() for x in singles]
        else:
            got = prog.push(frames[f:f + df], waves[:, s:s + ds])
            want = [x.push(frames[f:f + df], waves[p, s:s + ds]) for p, x in enumerate(singles)]
            f, s = f + df, s + ds
            assert all(prog.held[k] <= prog.held_bound[k] for k in prog.held), (prog.held, prog.held_bound)
        assert len(got) == 2 and all(_same_update(a, b, UPDATE_TENSORS + UPDATE_GATE) for a, b in zip(got, want))
