"""GPU: sf_track_stream_push (the fixed-lag read-out of a stream of window logits) against the float64 oracle of tests/track_stream_oracle.py:
exact on integer logits, bit-equal across chunkings on real ones, the posterior block under the measured bars of tests/test_track_posterior_gpu.py, non-finite
rows, two interleaved streams and a push replayed from a captured graph."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_track_posterior_gpu as PG  # noqa: E402   (the yardstick, its ceilings and the masked / wide inputs: the bars here are built the way that file builds its own)
import track_posterior_oracle as TP  # noqa: E402
import track_stream_oracle as TS  # noqa: E402

pytestmark = pytest.mark.gpu

C21 = 21
INT_KEYS = ('cls_raw', 'cls_lag', 'cls_tail')
CONF_KEYS = ('conf_raw', 'conf_lag', 'conf_tail')
POST_KEYS = ('post_lag', 'cls_post_lag', 'conf_post_lag', 'offset_mean_lag', 'log_z')


def _pushes(sizes):
    """every push of `sizes`, then the flush: an empty final push"""
    return [(n, False) for n in sizes] + [(0, True)]


def _device_rows(gpu, x: np.ndarray, ldl=None) -> torch.Tensor:
    if ldl is None:
        return torch.from_numpy(x.astype(np.float32)).to(gpu)
    buf = torch.full((x.shape[0], ldl), 1e30, device=gpu, dtype=torch.float32)   # a strided view: columns beyond C hold a value that would win every argmax
    buf[:, :x.shape[1]] = torch.from_numpy(x.astype(np.float32)).to(gpu)
    return buf[:, :x.shape[1]]


def _stream(gpu, x: np.ndarray, lam: float, lag: int, pushes, grid=None, ldl=None):
    """Runs the pushes [(n, final)] over the rows of x -> one dict of numpy arrays per push (read back once, after the last push)."""
    from synchformer_amd import ops
    xd = _device_rows(gpu, x, ldl)
    gd = None if grid is None else torch.from_numpy(grid.astype(np.float32)).to(gpu)
    state = ops.track_stream_state(x.shape[1], lag, grid is not None, gpu)
    outs, rows = [], 0
    for n, final in pushes:
        outs.append(ops.track_stream_push(state, xd[rows:rows + n], lam, gd, final=final))
        rows += n
        assert state.rows == rows and state.closed == final
    torch.cuda.synchronize()
    res = []
    for o in outs:
        d = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in o._asdict().items()}
        assert d['cls_raw'].dtype == d['cls_lag'].dtype == d['cls_tail'].dtype == np.int32 and d['conf_lag'].dtype == np.float32
        if grid is not None:
            d['log_z'] = float(d['log_z'][0])
        res.append(d)
    return res


def _check_exact(got, ref, C, what):
    """classes equal the oracle exactly, probabilities within 2e-6 (C terms, fp32 exp and sum: the bar of tests/test_track_gpu.py), every push"""
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g['w0'] == r['w0'], (what, i)
        for k in INT_KEYS:
            assert g[k].shape == r[k].shape and np.array_equal(g[k], r[k]), (what, i, k, g[k], r[k])
        for k in CONF_KEYS:
            assert g[k].shape == r[k].shape and (g[k].size == 0 or np.abs(g[k] - r[k]).max() <= 2e-6), (what, i, k)


def _cat(outs, key):
    return np.concatenate([d[key] for d in outs])


def _bit_equal(a, b, keys, what):
    """two chunkings of the same rows: the committed blocks and the raw read-out concatenate to the same bits, and so does the tail after the same row"""
    for k in keys:
        if k == 'log_z':
            continue
        assert np.array_equal(_cat(a, k), _cat(b, k), equal_nan=True), (what, k)


@pytest.mark.parametrize('lam', [0.0, 0.5, 2.0, 64.0])
@pytest.mark.parametrize('lag', [0, 1, 7, 8, 9, 63])
def test_stream_exact(gpu, lag, lam):
    """Integer logits in [-8, 8], dyadic lam: every operation of the recurrence is exact in fp32, so cls_lag, every push's cls_tail and cls_raw equal the float64
    oracle exactly.  W around the lag (nothing, one, two windows committed before the flush) and 70; every chunking.  At W = 70, lam = 2 the fixed-lag classes
    differ from the offline path and from the argmax (counts from the oracle; tests/test_track_stream_cpu.py pins them): a stream that returned either, or that
    ignored `lag`, fails here."""
    for W in sorted({1, 2, lag, lag + 1, lag + 2, 70} - {0}):
        x = np.random.default_rng(1000 * W + int(2 * lam)).integers(-8, 9, (W, C21)).astype(np.float64)      # the seed rule of test_decode_exact
        pre = TS.prefix_readouts(x, lam)
        for name in TS.CHUNKINGS:
            pushes = _pushes(TS.chunking(name, W, lag))
            ref = TS.by_definition(x, lam, lag, pushes, pre=pre)
            got = _stream(gpu, x, lam, lag, pushes)
            _check_exact(got, ref, C21, (W, lag, lam, name))
        if W == 70 and lam == 2.0:
            cls, offline, raw = _cat(got, 'cls_lag'), pre[0][-1], x.argmax(1)
            n_off, n_raw = int((cls != offline).sum()), int((cls != raw).sum())
            print(f'lag {lag}: cls_lag differs from the offline path in {n_off} windows, from the argmax in {n_raw}')
            assert n_off == int((_cat(ref, 'cls_lag') != offline).sum())
            assert (n_off > 0) == (lag < 63) and n_raw >= 47
            if lag in (7, 8, 9):                                                # and from its neighbours' lags
                other = _cat(TS.by_definition(x, lam, lag - 1, _pushes([W]), pre=pre), 'cls_lag')
                assert (cls != other).any()


def test_stream_two_classes_all_lanes_and_strided(gpu):
    rng = np.random.default_rng(78)
    for C, W, lag, lam in ((2, 257, 8, 0.5), (2, 257, 255, 2.0), (64, 66, 9, 2.0), (64, 66, 63, 0.5)):
        x = rng.integers(-8, 9, (W, C)).astype(np.float64)
        pre = TS.prefix_readouts(x, lam)
        for name in ('whole', 'ragged', 'long_after_short'):
            pushes = _pushes(TS.chunking(name, W, lag))
            _check_exact(_stream(gpu, x, lam, lag, pushes), TS.by_definition(x, lam, lag, pushes, pre=pre), C, (C, W, lag, name))
    x = rng.integers(-8, 9, (130, C21)).astype(np.float64)                       # ldl = 37 > C: the poisoned columns beyond C must not be read, in any launch
    pushes = _pushes(TS.chunking('ragged', 130, 7))
    grid = PG._grid(C21)
    got = _stream(gpu, x, 0.5, 7, pushes, grid=grid, ldl=37)
    _check_exact(got, TS.by_definition(x, 0.5, 7, pushes), C21, 'strided')
    dense = _stream(gpu, x, 0.5, 7, pushes, grid=grid)
    _bit_equal(got, dense, INT_KEYS + CONF_KEYS + POST_KEYS, 'strided vs dense')
    assert np.isfinite(_cat(got, 'post_lag')).all() and [d['log_z'] for d in got] == [d['log_z'] for d in dense]


def _real_valued():
    """the input of tests/test_track_gpu.py::test_decode_real_valued"""
    W = 200
    rng = np.random.default_rng(2024)
    x = rng.standard_normal((W, C21))
    true = np.round(np.linspace(5, 15, W)).astype(np.int64)
    x[np.arange(W), true] += 1.5
    return x.astype(np.float32)


@pytest.mark.parametrize('lam', [0.25, 1.0, 3.0])
def test_stream_real_valued(gpu, lam):
    """Real-valued logits round, so the oracle is not compared class by class.  (1) The carried state is the scan's own fp32 values: every chunking gives the same
    bits, classes and floats, with and without the posterior.  (2) With lag = 255 >= W - 1 the flushed classes are a path of the whole recording: its float64
    score lies within test_decode_real_valued's bound of the float64 optimum."""
    x = _real_valued()
    W = x.shape[0]
    grid = PG._grid(C21)
    for lag in (16, 255):
        runs = {name: _stream(gpu, x, lam, lag, _pushes(TS.chunking(name, W, lag)), grid=grid) for name in TS.CHUNKINGS}
        for name in TS.CHUNKINGS[1:]:
            _bit_equal(runs['whole'], runs[name], INT_KEYS[:2] + CONF_KEYS[:2] + POST_KEYS, (lam, lag, name))
            assert runs[name][-1]['log_z'] == runs['whole'][-1]['log_z']
            assert np.array_equal(runs[name][-2]['cls_tail'], runs['whole'][-2]['cls_tail']) and np.array_equal(runs[name][-2]['conf_tail'], runs['whole'][-2]['conf_tail'])
        plain = _stream(gpu, x, lam, lag, _pushes(TS.chunking('ragged', W, lag)))
        _bit_equal(plain, runs['ragged'], INT_KEYS + CONF_KEYS, 'posterior on / off')
    path = _cat(runs['whole'], 'cls_lag')
    assert np.array_equal(_cat(runs['whole'], 'cls_raw'), x.argmax(1))
    e = x.astype(np.float64) - x.astype(np.float64).max(1, keepdims=True)
    bound = 2 * W * 3 * 2.0 ** -24 * (np.abs(e).max() + lam * C21)
    score = float(e[np.arange(W), path].sum() - lam * np.abs(np.diff(path.astype(np.int64))).sum())
    d = np.abs(np.arange(C21)[:, None] - np.arange(C21)[None, :]).astype(np.float64)
    s = e[0].copy()
    for w in range(1, W):
        s = (s[:, None] - lam * d).max(0) + e[w]
    best = float(s.max())
    print(f'lam {lam}: flushed path score {score:.6f}, float64 optimum {best:.6f}, bound {bound:.2e}')
    assert best - score <= bound and score <= best + 1e-9, (score, best, bound)
    p = TS.softmax(x)
    assert np.abs(_cat(runs['whole'], 'conf_lag') - p[np.arange(W), path]).max() <= 2e-6


# ---- the posterior block ----------------------------------------------------------------------------------------------------------------------------
POST_CASES = [(W, C, lam) for W in (1, 2, 9, 70) for C in (2, 21, 64) for lam in (0.0, 0.5, 8.0)]
POST_LAGS = (0, 1, 8, 20)
_POST_INPUTS = {('grid', W, C, lam): (PG._randn(11 + 1000 * W + 10 * C + int(2 * lam), W, C, 3.0), lam) for W, C, lam in POST_CASES}
_POST_INPUTS[('masked',)] = (PG._masked_input(), 1.0)
_POST_INPUTS[('wide',)] = (PG._randn(43, 70, 21, 50.0), 8.0)                      # the first 70 rows of that file's wide-range input (scale 50)


def _yardstick_lag(prefixes, lag: int):
    """The contract's recurrences in torch fp32 on the CPU (prefixes[r] = PG._yardstick on rows 0 .. r), read out at a fixed lag: post[w] from the prefix
    0 .. min(w + lag, W - 1)."""
    W = len(prefixes)
    ends = [min(w + lag, W - 1) for w in range(W)]
    return dict(post=np.stack([prefixes[r]['post'][w] for w, r in enumerate(ends)]), offset_mean=np.array([prefixes[r]['offset_mean'][w] for w, r in enumerate(ends)]),
                log_z=prefixes[-1]['log_z'])


@pytest.fixture(scope='module')
def post_refs():
    """key -> dict(x, lam, grid, pre = the float64 read-outs of every prefix, yard[lag] = the yardstick's (post, mean, log_z) errors); 'bar' -> the bar per
    quantity: 4 x the yardstick's worst value over the inputs of this file, each at most its ceiling in PG.CEIL, with PG's absolute floor of 1e-6 for post."""
    out = {}
    for key, (x, lam) in _POST_INPUTS.items():
        grid = PG._grid(x.shape[1])
        x64, g64 = x.astype(np.float64), grid.astype(np.float64)
        pre = TS.prefix_readouts(x64, lam, g64)
        yard, prefixes = {}, [PG._yardstick(x[:r + 1], lam, grid) for r in range(x.shape[0])]
        for lag in POST_LAGS:
            d = TS.by_definition(x64, lam, lag, [(x.shape[0], True)], g64, pre=pre)[0]
            ref = dict(post=d['post_lag'], offset_mean=d['offset_mean_lag'], log_z=d['log_z'])
            yard[lag] = PG._errors(_yardstick_lag(prefixes, lag), ref, grid)
        out[key] = dict(x=x, lam=lam, grid=grid, pre=pre, yard=yard)
    worst = [max(v['yard'][lag][q] for v in out.values() for lag in POST_LAGS) for q in range(3)]
    print(f'yardstick worst: post {worst[0]:.3e}  mean {worst[1]:.3e} steps  log_z {worst[2]:.3e} (ceilings {PG.CEIL})')
    worst = [min(w, c) for w, c in zip(worst, PG.CEIL)]
    out['bar'] = (max(4 * worst[0], 1e-6), 4 * worst[1], 4 * worst[2])
    return out


def _check_posterior(gpu, case, bar, lag, what):
    x, lam, grid = case['x'], case['lam'], case['grid']
    W, C = x.shape
    x64, g64 = x.astype(np.float64), grid.astype(np.float64)
    runs = {}
    for name in TS.CHUNKINGS:
        pushes = _pushes(TS.chunking(name, W, lag))
        runs[name] = got = _stream(gpu, x, lam, lag, pushes, grid=grid)
        ref = TS.by_definition(x64, lam, lag, pushes, g64, pre=case['pre'])
        gp, rp = _cat(got, 'post_lag'), _cat(ref, 'post_lag')
        step = float(grid[1] - grid[0])
        e_post = float(np.abs(gp - rp).max())
        e_mean = float(np.abs(_cat(got, 'offset_mean_lag') - _cat(ref, 'offset_mean_lag')).max()) / step
        e_z = max(abs(g['log_z'] - r['log_z']) / max(1.0, abs(r['log_z'])) for g, r in zip(got, ref))        # after EVERY push: the prefix's
        if name == 'whole':
            print(f'{what} lag {lag} lam {lam}: ' + '  '.join(f'{n} {e:.3e} (yardstick {y:.3e}, bar {b:.3e})'
                                                            for n, e, y, b in zip(PG.QUANT, (e_post, e_mean, e_z), case['yard'][lag], bar)))
        assert gp.shape == (W, C) and np.isfinite(gp).all()
        assert e_post <= bar[0] and e_mean <= bar[1] and e_z <= bar[2], (name, (e_post, e_mean, e_z), bar)
        assert np.abs(gp.sum(1) - 1).max() <= 1e-5
        assert all(g['log_z'] <= 1e-5 for g in got)
        cls = _cat(got, 'cls_post_lag')
        assert cls.min() >= 0 and cls.max() < C
        assert np.array_equal(_cat(got, 'conf_post_lag'), gp[np.arange(W), cls])
        top = np.sort(rp, 1)
        decided = top[:, -1] - top[:, -2] > bar[0]
        assert np.array_equal(cls[decided], _cat(ref, 'cls_post_lag')[decided])
        assert [g['w0'] for g in got] == [r['w0'] for r in ref]
    for name in TS.CHUNKINGS[1:]:
        _bit_equal(runs['whole'], runs[name], INT_KEYS[:2] + CONF_KEYS[:2] + POST_KEYS, (what, lag, name))
    return runs['whole']


def test_posterior_argmax_is_decided_in_the_oracle(post_refs):
    """At least 99 % of the committed windows have the oracle's two largest marginals further apart than the post bar: the cls_post_lag check covers them."""
    close = total = 0
    for key, case in post_refs.items():
        if key == 'bar':
            continue
        for lag in POST_LAGS:
            W = case['x'].shape[0]
            rp = TS.by_definition(case['x'].astype(np.float64), case['lam'], lag, [(W, True)], case['grid'].astype(np.float64), pre=case['pre'])[0]['post_lag']
            top = np.sort(rp, 1)
            close += int((top[:, -1] - top[:, -2] <= post_refs['bar'][0]).sum())
            total += W
    print(f'{close} of {total} windows undecided at the bar')
    assert close <= 0.01 * total


@pytest.mark.parametrize('W, C, lam', POST_CASES)
def test_stream_posterior_against_oracle(gpu, post_refs, W, C, lam):
    case = post_refs[('grid', W, C, lam)]
    for lag in POST_LAGS:
        got = _check_posterior(gpu, case, post_refs['bar'], lag, f'W {W} C {C}')
        if lam == 0.0:                                                           # independent windows: the lag changes nothing, post is each row's softmax
            assert np.abs(_cat(got, 'post_lag') - TS.softmax(case['x'])).max() <= post_refs['bar'][0]


def test_stream_posterior_masked_and_wide(gpu, post_refs):
    for lag in POST_LAGS:
        got = _check_posterior(gpu, post_refs[('masked',)], post_refs['bar'], lag, 'masked')
        assert (_cat(got, 'post_lag')[np.isneginf(post_refs[('masked',)]['x'])] == 0).all()
        _check_posterior(gpu, post_refs[('wide',)], post_refs['bar'], lag, 'wide')


def test_stream_does_not_drift(gpu):
    """W = 4096 rows at lag = 16, 64 rows per push: the carried double keeps log_z to fp32 precision after every push (the bar: 4 x the fp32 yardstick's error at
    the end of the run, at most PG.CEIL's), and the committed marginals and classes stay with the incremental float64 oracle."""
    x = PG._randn(42, 4096, C21, 3.0)                                            # that file's drift input
    lam, lag, grid = 1.0, 16, PG._grid(C21)
    pushes = [(64, False)] * 64 + [(0, True)]
    got = _stream(gpu, x, lam, lag, pushes, grid=grid)
    ref = TP.posterior(x.astype(np.float64), lam, grid.astype(np.float64))
    yard = PG._errors(PG._yardstick(x, lam, grid), ref, grid)
    bar_post, bar_z = max(4 * min(yard[0], PG.CEIL[0]), 1e-6), 4 * min(yard[2], PG.CEIL[2])
    inc = TS.StreamOracle(C21, lam, lag, grid.astype(np.float64))
    e_z = e_post = 0.0
    rows = 0
    for (n, final), g in zip(pushes, got):
        r = inc.push(x[rows:rows + n].astype(np.float64), final)
        rows += n
        e_z = max(e_z, abs(g['log_z'] - r['log_z']) / max(1.0, abs(r['log_z'])))
        if len(r['post_lag']):
            e_post = max(e_post, float(np.abs(g['post_lag'] - r['post_lag']).max()))
        assert g['w0'] == r['w0'] and g['cls_lag'].shape == r['cls_lag'].shape
    print(f'W 4096: log_z {got[-1]["log_z"]:.3f} (float64 {ref["log_z"]:.3f}); worst relative error over the pushes {e_z:.3e} (yardstick {yard[2]:.3e}, bar {bar_z:.3e}); '
          f'post_lag {e_post:.3e} (yardstick {yard[0]:.3e}, bar {bar_post:.3e})')
    assert e_z <= bar_z and e_post <= bar_post
    assert sum(len(g['cls_lag']) for g in got) == 4096


# ---- safety and isolation -----------------------------------------------------------------------------------------------------------------------------
def test_stream_non_finite_rows_stay_in_range(gpu):
    """One row of NaN and one row of +inf: any classes may come out, every class written lies in [0, C), in the committed blocks and in every tail."""
    x = np.random.default_rng(3).standard_normal((40, C21)).astype(np.float32)
    x[11, :] = np.nan
    x[23, :] = np.inf
    for lag in (0, 3, 9):
        for name in ('whole', 'ragged'):
            got = _stream(gpu, x, 1.0, lag, _pushes(TS.chunking(name, 40, lag)), grid=PG._grid(C21))
            for k in INT_KEYS + ('cls_post_lag',):
                c = _cat(got, k)
                assert c.size or (k == 'cls_tail' and lag == 0), (lag, name, k)        # (no tail at lag 0: every window is committed by its own push)
                assert c.size == 0 or (c.min() >= 0 and c.max() < C21), (lag, name, k, c)
            assert np.array_equal(_cat(got, 'cls_raw')[:11], x[:11].argmax(1))
            assert sum(len(g['cls_lag']) for g in got) == 40


def test_two_streams_do_not_share_state(gpu):
    """Two streams pushed alternately equal the same two streams pushed one after the other."""
    from synchformer_amd import ops
    rng = np.random.default_rng(5)
    xs = [torch.from_numpy(rng.standard_normal((50, C21)).astype(np.float32)).to(gpu) for _ in range(2)]
    grid = torch.from_numpy(PG._grid(C21)).to(gpu)
    sizes = TS.chunking('ragged', 50, 5)

    def run(order):
        states = [ops.track_stream_state(C21, 5, True, gpu) for _ in range(2)]
        outs = ([], [])
        for i, j in order:                                                       # stream i, its j-th push
            r0 = sum(sizes[:j])
            outs[i].append(ops.track_stream_push(states[i], xs[i][r0:r0 + sizes[j]], 0.5 + i, grid, final=(j == len(sizes) - 1)))
        torch.cuda.synchronize()
        return outs

    alternate = run([(i, j) for j in range(len(sizes)) for i in range(2)])
    serial = run([(i, j) for i in range(2) for j in range(len(sizes))])
    for i in range(2):
        for a, b in zip(alternate[i], serial[i]):
            assert a.w0 == b.w0 and all(torch.equal(u, v) for u, v in zip(a[1:], b[1:]))
    assert not torch.equal(torch.cat([o.cls_lag for o in serial[0]]), torch.cat([o.cls_lag for o in serial[1]]))


def test_push_under_graph_capture(gpu):
    """One push (rows 5 .. 11 of a stream at lag 3: a committed block, a tail and the rings' update) captured on a single stream and replayed equals the eager push
    bit for bit, outputs and state: the launcher neither synchronises, allocates nor reads anything back."""
    from synchformer_amd import ops
    x = torch.from_numpy(PG._randn(9, 12, C21, 3.0)).to(gpu)
    grid = torch.from_numpy(PG._grid(C21)).to(gpu)

    def fresh():
        st = ops.track_stream_state(C21, 3, True, gpu)
        ops.track_stream_push(st, x[:5], 1.0, grid)
        return st

    eager_state = fresh()
    eager = ops.track_stream_push(eager_state, x[5:], 1.0, grid)
    st = fresh()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = ops.track_stream_push(st, x[5:], 1.0, grid)
    for t in captured[1:]:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert captured.w0 == eager.w0 == 2 and captured.cls_lag.shape == (7,) and captured.cls_tail.shape == (3,)
    assert all(torch.equal(a, b) for a, b in zip(eager[1:], captured[1:]))
    assert torch.equal(st.buf, eager_state.buf)
    last = [ops.track_stream_push(s, x[:0], 1.0, grid, final=True) for s in (st, eager_state)]
    torch.cuda.synchronize()
    assert last[0].cls_lag.shape == (3,) and all(torch.equal(a, b) for a, b in zip(last[0][1:], last[1][1:]))


# ---- end to end: OffsetTracker.stream against track / track_raw on the finished recording ----------------------------------------------------------------
T_REC, N_REC, N_SEG, N_WIN = 144, 92160, 17, 4                                   # the fixture geometry of tests/test_track_gpu.py


@pytest.fixture(scope='module')
def rec(gpu):
    """One engine (synthetic weights, seg_chunk = 5: the un-fused schedule, where a segment's features do not depend on its place in a launch), one 17-segment
    recording as 256 x 256 raw frames, its centre crop, and the offline tracks - computed once, read-only."""
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.track import OffsetTracker
    eng = SynchformerEngine(synth.make_state_dict(1337), gpu, seg_chunk=5)
    mel = MelFrontend(gpu)
    g = torch.Generator().manual_seed(99)
    raw = torch.randint(0, 256, (T_REC, 3, 256, 256), generator=g, dtype=torch.uint8)
    wave = synth.make_wave(1, 1, 99, n=N_REC).reshape(N_REC)
    crop = raw[:, :, 16:240, 16:240].contiguous()
    tracker = OffsetTracker(eng, mel, lam=0.5, posterior=True)
    ref = tracker.track(crop.to(gpu), wave.to(gpu))
    torch.cuda.synchronize()
    assert ref.logits.shape == (N_WIN, C21) and ref.n_segments == N_SEG
    return dict(eng=eng, mel=mel, tracker=tracker, raw=raw, wave=wave, crop=crop, ref=ref)


def _ragged(total_f: int, total_a: int, f_runs=(1, 7, 40, 0, 3, 25), a_runs=(16000, 0, 333, 40000, 5120, 0, 1)):
    """[(f0, f1, a0, a1)]: frames in runs of 1, 7, 40, ..., samples in unrelated runs, some pushes empty on one side, until both are through."""
    out, f, a, i = [], 0, 0, 0
    while f < total_f or a < total_a:
        nf, na = min(f_runs[i % len(f_runs)], total_f - f), min(a_runs[i % len(a_runs)], total_a - a)
        out.append((f, f + nf, a, a + na))
        f, a, i = f + nf, a + na, i + 1
    return out


def _run_stream(stream, frames, wave, pieces):
    ups = []
    for f0, f1, a0, a1 in pieces:
        ups.append(stream.push(frames[f0:f1], wave[..., a0:a1]))
        held, bound = stream.held, stream.held_bound
        assert all(held[k] <= bound[k] for k in bound), (held, bound)
    ups.append(stream.flush())
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='closed'):
        stream.push(frames[:0], wave[..., :0])
    return ups


def _check_stream_against(ups, ref, lag):
    from synchformer_amd.postprocess import class_grid
    grid = class_grid(-2, 2, C21)
    cat = lambda name: torch.cat([getattr(u, name) for u in ups])                 # noqa: E731
    W = ref.logits.shape[0]
    assert torch.equal(cat('logits'), ref.logits), (cat('logits') - ref.logits).abs().max().item()
    assert torch.equal(cat('cls_raw'), ref.cls_raw) and torch.equal(cat('conf_raw'), ref.conf_raw)
    assert [u.w0 for u in ups][0] == 0 and sum(u.cls_lag.shape[0] for u in ups) == W
    assert torch.equal(cat('t_sec').float(), ref.t_sec.cpu()) and cat('t_sec').dtype == torch.float64
    if lag >= W - 1:                                                             # every window is committed from the whole recording: the offline read-outs
        assert torch.equal(cat('cls_lag'), ref.cls_path) and torch.equal(cat('offset_sec_lag'), ref.offset_sec_path)
        assert torch.equal(cat('conf_lag'), ref.conf_path)
        assert torch.equal(cat('cls_post_lag'), ref.cls_post) and (cat('post_lag') - ref.post).abs().max().item() <= 1e-5
        assert abs(ups[-1].log_z.item() - ref.log_z.item()) <= 1e-5 * max(1.0, abs(ref.log_z.item()))
    rows = 0
    for u in ups[:-1]:                                                           # every push's tail: the last min(lag, rows) windows so far, at their own times
        rows += u.logits.shape[0]
        m = u.cls_tail.shape[0]
        assert m == min(lag, rows) and u.w_new == rows - u.logits.shape[0]
        assert torch.equal(u.t_sec_tail.float(), ref.t_sec.cpu()[rows - m:rows]) and torch.equal(u.offset_sec_tail.cpu(), grid[u.cls_tail.cpu().long()])
        if rows == W and m:                                                      # once every window is in (an ingest may hold the last one back until flush):
            assert torch.equal(u.cls_tail, ref.cls_path[W - m:])                 # the tail is the offline path's end
    assert ups[-1].cls_tail.shape[0] == 0 and rows + ups[-1].logits.shape[0] == W


@pytest.mark.parametrize('lag', [3, 16, 1])
def test_offset_stream_equals_track(gpu, rec, lag):
    """Ragged pushes plus flush() give the logits of track() on the finished recording bit for bit (the un-fused tower schedule is position-independent, the
    windows of a stream are row-map views of the held features), the same t_sec, and with lag >= W - 1 = 3 the offline path; what the stream holds stays
    within its stated bound after every push; a push after flush() raises.  Frames on the device and samples in host memory, then the reverse."""
    frames, wave = rec['crop'], rec['wave']
    pieces = _ragged(T_REC, N_REC)
    assert any(f0 == f1 and a1 > a0 for f0, f1, a0, a1 in pieces) and any(a0 == a1 and f1 > f0 for f0, f1, a0, a1 in pieces)
    for fr, wv in ((frames.to(gpu), wave), (frames, wave.to(gpu))):
        stream = rec['tracker'].stream(lag=lag)
        ups = _run_stream(stream, fr, wv, pieces)
        _check_stream_against(ups, rec['ref'], lag)
        assert stream.n_segments == N_SEG and stream.n_windows == N_WIN and stream.held['segments'] <= 13
    if lag == 1:                                                                 # the fixed lag is in force: window w was committed from windows 0 .. w + 1 only
        x = rec['ref'].logits.cpu().numpy().astype(np.float64)
        want = np.concatenate([d['cls_lag'] for d in TS.by_definition(x, 0.5, 1, [(N_WIN, False), (0, True)])])
        got = torch.cat([u.cls_lag for u in ups]).cpu().numpy()
        print(f'lag 1: committed {got}, float64 fixed-lag {want}, offline {rec["ref"].cls_path.cpu().numpy()}')
        assert got.shape == want.shape


def test_offset_stream_from_decoded_input(gpu, rec):
    """ingest=RecordingIngest(...): the identity geometry (25 fps, 256 x 256, 16 kHz) against track_raw, and 50 fps channels-last frames with 48 kHz stereo audio
    against track_raw on the whole recording."""
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 25, (256, 256), 16000)
    ref = rec['tracker'].track_raw(rec['raw'].to(gpu), rec['wave'].to(gpu), ing)
    assert torch.equal(ref.logits, rec['ref'].logits)
    ups = _run_stream(rec['tracker'].stream(lag=3, ingest=ing), rec['raw'], rec['wave'], _ragged(T_REC, N_REC))
    _check_stream_against(ups, ref, 3)
    raw50 = rec['raw'].repeat_interleave(2, 0).permute(0, 2, 3, 1).contiguous()                          # (288, 256, 256, 3)
    wave48 = torch.rand(2, 3 * N_REC, generator=torch.Generator().manual_seed(48)) * 2 - 1
    ing50 = RecordingIngest(gpu, 50, (256, 256), 48000, channels_last=True)
    ref50 = rec['tracker'].track_raw(raw50, wave48, ing50)
    pieces = _ragged(2 * T_REC, 3 * N_REC, f_runs=(1, 7, 40, 0, 3, 50), a_runs=(48000, 0, 1001, 120000, 15360, 0, 1))
    ups = _run_stream(rec['tracker'].stream(lag=16, ingest=ing50), raw50, wave48, pieces)
    assert ref50.logits.shape[0] >= N_WIN
    _check_stream_against(ups, ref50, 16)
