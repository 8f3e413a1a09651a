"""GPU: sf_track_pool_push (the fixed-lag read-out of many streams in one call) against sf_track_stream_push stream by stream - every output block and
the state bytes after every tick, bit for bit - and against the float64 oracle of tests/track_stream_oracle.py; OffsetStreamPool against OffsetTracker.stream and
track() / track_raw() on the finished recordings."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_track_posterior_gpu as PG  # noqa: E402   (the fp32 yardstick, its ceilings, the seeded inputs)
import test_track_stream_gpu as SG  # noqa: E402      (the stream tests' end-to-end geometry and push patterns)
import track_stream_oracle as TS  # noqa: E402
from test_track_stream_gpu import rec  # noqa: E402,F401   (the module-scoped engine / recording fixture of the stream tests)

pytestmark = pytest.mark.gpu

C21 = 21
W70 = 70
FIELDS = ('cls_raw', 'conf_raw', 'cls_lag', 'conf_lag', 'cls_tail', 'conf_tail', 'post_lag', 'cls_post_lag', 'conf_post_lag', 'offset_mean_lag', 'log_z')


def _same(a, b):
    """the same bits (floats compared as their bit patterns: a NaN equals the same NaN); None only equals None"""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def _run_ticks(gpu, xs, ticks, slot_of, lag, lam, grid=None, n_slots=7, ldl=None, ldp=None):
    """xs: {stream: float32 numpy (W, C)}; ticks: [[(stream, n, final), ...], ...] - one pool push per tick, the entries in table order; slot_of: {stream: slot}.
    Every tick runs once through ops.track_pool_push and once, stream by stream, through ops.track_stream_push; after every tick every output block of every
    stream and its state bytes must be equal.  ldl / ldp: row strides of the packed logits / of post_lag, the padding poisoned with
    NaN.  -> ({stream: [TrackStreamOut per push]}, the pool state)."""
    from synchformer_amd import ops
    C = next(iter(xs.values())).shape[1]
    xd = {s: torch.from_numpy(x).to(gpu) for s, x in xs.items()}
    gd = None if grid is None else torch.from_numpy(grid.astype(np.float32)).to(gpu)
    pool = ops.track_pool_state(n_slots, C, lag, grid is not None, gpu)
    nbytes = pool.buf.shape[1]
    solo = {s: ops.track_stream_state(C, lag, grid is not None, gpu) for s in xs}
    assert all(st.buf.numel() == nbytes for st in solo.values())
    pos = {s: 0 for s in xs}
    outs = {s: [] for s in xs}
    for t, entries in enumerate(ticks):
        rows = [xd[s][pos[s]:pos[s] + n] for s, n, _ in entries]
        total = sum(n for _, n, _ in entries)
        packed = torch.cat(rows) if rows else torch.empty(0, C, device=gpu)
        if ldl is not None:
            wide = torch.full((total, ldl), float('nan'), device=gpu)
            wide[:, :C] = packed
            packed = wide[:, :C]
        slots, counts, final = [slot_of[s] for s, _, _ in entries], [n for _, n, _ in entries], [slot_of[s] for s, _, f in entries if f]
        post = None
        if ldp is not None:
            K = ops.track_pool_plan([pool.rows[x] for x in slots], counts, lag, [x in final for x in slots]).total_commit
            post_wide = torch.full((K, ldp), float('nan'), device=gpu)
            post = post_wide[:, :C]
        got = ops.track_pool_push(pool, slots, packed, counts, lam, gd, final=final, post=post)
        if ldp is not None:
            assert torch.isnan(post_wide[:, C:]).all() and torch.isfinite(post).all(), 'post_lag: the padding beyond C was written, or a NaN was read from the logits'
        assert len(got) == len(entries)
        for (s, n, f), g in zip(entries, got):
            want = ops.track_stream_push(solo[s], xd[s][pos[s]:pos[s] + n], lam, gd, final=f)
            pos[s] += n
            assert g.w0 == want.w0, (t, s)
            for k in FIELDS:
                assert _same(getattr(g, k), getattr(want, k)), (t, s, k, getattr(g, k), getattr(want, k))
            assert pool.rows[slot_of[s]] == solo[s].rows == pos[s] and pool.closed[slot_of[s]] == solo[s].closed == f
            if pos[s] > 0:                                                           # (a state is read only once its stream holds rows)
                assert torch.equal(pool.buf[slot_of[s]], solo[s].buf), (t, s, 'state bytes')
            outs[s].append(g)
    torch.cuda.synchronize()
    return outs, pool


def _cat(outs, key):
    return torch.cat([getattr(o, key) for o in outs]).cpu().numpy()


def _ints(seed: int, W: int, C: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(-8, 9, (W, C)).astype(np.float32)


def _five_streams(lag: int):
    """Per stream its pushes, one per tick it takes part in (None: not named in that tick) - 70 rows each, the chunkings unrelated: empty pushes, a push longer than
    the lag, a stream that joins at tick 3, streams closed at different ticks - 'a' by its last rows, 'b' and 'd' by an empty final push."""
    rest = lambda done, step: [min(step, W70 - r) for r in range(done, W70, step)]          # noqa: E731
    a = TS.chunking('ragged', W70, lag)
    long_b = min(W70 - 2, lag + 2)
    b = [0, 2, long_b] + rest(2 + long_b, 9) + [0]
    c = [None] * 3 + TS.chunking('long_after_short', W70, lag)
    d = [None, W70, 0, 0, None, 0, 0]
    e = [7, 0, 7, 7, None, 7, 0, 7, 7, None, None, 7, 7, 7, 7]
    per = dict(a=[(n, i == len(a) - 1) for i, n in enumerate(a)], b=[(n, i == len(b) - 1) for i, n in enumerate(b)],
               c=[None if n is None else (n, i == len(c) - 1) for i, n in enumerate(c)], d=[None if n is None else (n, i == len(d) - 1) for i, n in enumerate(d)],
               e=[None if n is None else (n, False) for n in e] + [(0, True)])
    assert all(sum(p[0] for p in v if p) == W70 for v in per.values())
    assert any(p and p[0] > lag for p in per['b']) and per['b'][-1] == (0, True) and per['a'][-1][0] > 0 and per['a'][-1][1]
    ticks = []
    for t in range(max(len(v) for v in per.values())):
        ticks.append([(s, *v[t]) for s, v in per.items() if t < len(v) and v[t] is not None])
    assert len({len(v) for v in per.values()}) >= 4                                       # closed at different ticks
    return per, [tk for tk in ticks if tk]


_PRE = {}


def _pre(s, x, lam, grid=None):
    key = (s, lam, grid is not None)
    if key not in _PRE:
        _PRE[key] = TS.prefix_readouts(x.astype(np.float64), lam, None if grid is None else grid.astype(np.float64))
    return _PRE[key]


SLOTS5 = dict(a=5, b=0, c=3, d=6, e=2)


@pytest.mark.parametrize('lam', [0.0, 0.5, 2.0])
@pytest.mark.parametrize('lag', [0, 1, 8, 63])
def test_pool_exact(gpu, lag, lam):
    """Integer logits in [-8, 8] and dyadic lam (every operation exact in fp32): 5 streams in a pool of 7 slots, C = 21; after every tick every output block and the
    state slot equal the single-stream call, and the concatenated cls_lag / cls_raw equal the float64 definition."""
    xs = {s: _ints(100 + i, W70, C21) for i, s in enumerate('abcde')}
    per, ticks = _five_streams(lag)
    outs, pool = _run_ticks(gpu, xs, ticks, SLOTS5, lag, lam)
    assert pool.buf[1].eq(0).all() and pool.buf[4].eq(0).all() and all(pool.closed[SLOTS5[s]] for s in xs)      # the two idle slots were never written
    for s, x in xs.items():
        pushes = [p for p in per[s] if p is not None]
        ref = TS.by_definition(x.astype(np.float64), lam, lag, pushes, pre=_pre(s, x, lam))
        assert len(ref) == len(outs[s]) and [o.w0 for o in outs[s]] == [r['w0'] for r in ref]
        for k in ('cls_lag', 'cls_raw'):
            assert np.array_equal(_cat(outs[s], k), np.concatenate([r[k] for r in ref])), (s, k)
        for o, r in zip(outs[s], ref):
            assert np.array_equal(o.cls_tail.cpu().numpy(), r['cls_tail'])
        assert _cat(outs[s], 'cls_lag').shape == (W70,)


def test_reopened_slot_equals_a_fresh_stream(gpu):
    """Slot 5 carries stream 'a' to its final push, is re-opened and carries 'f' next to a stream that goes on: 'f' equals a fresh single stream in every output
    (the stale bytes of 'a' are never read: a state is read only when rows_done > 0)."""
    from synchformer_amd import ops
    lag, lam, grid = 8, 0.5, PG._grid(C21)
    xs = dict(a=_ints(1, 30, C21), b=_ints(2, 60, C21), f=_ints(3, 30, C21))
    first = [[('a', 10, False), ('b', 10, False)], [('b', 10, False), ('a', 20, True)]]
    outs, pool = _run_ticks(gpu, dict(a=xs['a'], b=xs['b']), first, dict(a=5, b=1), lag, lam, grid)
    assert pool.closed[5] and pool.rows[5] == 30 and not pool.buf[5].eq(0).all()
    with pytest.raises(RuntimeError, match='closed'):
        ops.track_pool_push(pool, [5], torch.zeros(1, C21, device=gpu), [1], lam, torch.from_numpy(grid).to(gpu))
    pool.reopen(5)
    assert pool.rows[5] == 0 and not pool.closed[5]
    b_rest = xs['b'][20:]
    second = [[('f', 3, False), ('b2', 20, False)], [('f', 0, False)], [('b2', 20, True), ('f', 27, False)], [('f', 0, True)]]
    # 'b2' continues 'b' in slot 1 (rows 20 .. 59); per tick only 'f' is compared, 'b' as a whole below
    gd = torch.from_numpy(grid).to(gpu)
    solo = ops.track_stream_state(C21, lag, True, gpu)
    fd, bd = torch.from_numpy(xs['f']).to(gpu), torch.from_numpy(b_rest).to(gpu)
    fpos = bpos = 0
    for entries in second:
        rows, slots, counts, final = [], [], [], []
        for s, n, f in entries:
            src, p = (fd, fpos) if s == 'f' else (bd, bpos)
            rows.append(src[p:p + n])
            slots.append(5 if s == 'f' else 1)
            counts.append(n)
            final += [slots[-1]] if f else []
        got = ops.track_pool_push(pool, slots, torch.cat(rows), counts, lam, gd, final=final)
        for (s, n, f), g in zip(entries, got):
            if s == 'f':
                want = ops.track_stream_push(solo, fd[fpos:fpos + n], lam, gd, final=f)
                fpos += n
                assert g.w0 == want.w0 and all(_same(getattr(g, k), getattr(want, k)) for k in FIELDS), (entries, [k for k in FIELDS if not _same(getattr(g, k), getattr(want, k))])
            else:
                bpos += n
    assert fpos == 30 and pool.closed[5] and pool.closed[1]
    # stream 'b' was never disturbed by its neighbours: all 60 rows through the pool above equal one single stream over the same pushes
    whole = ops.track_stream_state(C21, lag, True, gpu)
    ref = [ops.track_stream_push(whole, torch.from_numpy(xs['b'][r0:r0 + n]).to(gpu), lam, gd, final=f) for r0, n, f in ((0, 10, False), (10, 10, False), (20, 20, False), (40, 20, True))]
    assert torch.equal(torch.cat([o.cls_lag for o in outs['b']]), torch.cat([o.cls_lag for o in ref[:2]]))
    assert torch.equal(pool.buf[1], whole.buf)


@pytest.mark.parametrize('C, lag, lam', [(2, 8, 0.5), (2, 255, 2.0), (64, 9, 2.0), (64, 63, 0.5), (21, 7, 0.5)])
def test_pool_two_classes_all_lanes_and_strided(gpu, C, lag, lam):
    """C = 2 and C = 64 (every lane a class), the packed logits with row stride ldl > C and post_lag with ldp > C, both paddings NaN: nothing beyond column C is
    read or written, every block equals the single stream's dense call, the classes equal the float64 definition."""
    xs = {s: _ints(200 + 10 * C + i, 66, C) for i, s in enumerate('abc')}
    per = dict(a=[(n, False) for n in TS.chunking('ragged', 66, lag)] + [(0, True)], b=[(66, False), (0, False), (0, True)],
               c=[None, None] + [(n, i == 5) for i, n in enumerate((1, 0, 30, 5, 29, 1))])
    ticks = [[(s, *v[t]) for s, v in per.items() if t < len(v) and v[t] is not None] for t in range(max(len(v) for v in per.values()))]
    grid = PG._grid(C)
    outs, _ = _run_ticks(gpu, xs, ticks, dict(a=2, b=0, c=1), lag, lam, grid, n_slots=3, ldl=C + 16, ldp=C + 3)
    for s, x in xs.items():
        ref = TS.by_definition(x.astype(np.float64), lam, lag, [p for p in per[s] if p is not None])
        for k in ('cls_lag', 'cls_raw'):
            assert np.array_equal(_cat(outs[s], k), np.concatenate([r[k] for r in ref])), (s, k)
        assert np.isfinite(_cat(outs[s], 'post_lag')).all() and np.abs(_cat(outs[s], 'post_lag').sum(1) - 1).max() <= 1e-5


# ---- the posterior on real-valued logits ------------------------------------------------------------------------------------------------------------------
# two inputs of tests/test_track_stream_gpu.py: 3 randn and 50 randn ('wide'), 70 rows, lam = 8
REAL = {'grid': SG._POST_INPUTS[('grid', 70, 21, 8.0)], 'wide': SG._POST_INPUTS[('wide',)]}


@pytest.fixture(scope='module')
def real_refs():
    """Per input and lag the float64 definition and the fp32 yardstick's error against it, built as tests/test_track_stream_gpu.py builds its own; the bar per
    quantity is 4 x the yardstick's worst value over THESE two inputs, each at most its ceiling in PG.CEIL, with the floor of 1e-6 for post.  The two inputs are
    among that file's, so this bar is at most that file's: a result under it is under the stream tests' bar."""
    out = {}
    for key, (x, lam) in REAL.items():
        assert x.shape == (70, 21) and lam == 8.0
        grid = PG._grid(21)
        x64, g64 = x.astype(np.float64), grid.astype(np.float64)
        pre = TS.prefix_readouts(x64, lam, g64)
        prefixes = [PG._yardstick(x[:r + 1], lam, grid) for r in range(70)]
        yard = {}
        for lag in (8, 20):
            d = TS.by_definition(x64, lam, lag, [(70, True)], g64, pre=pre)[0]
            yard[lag] = PG._errors(SG._yardstick_lag(prefixes, lag), dict(post=d['post_lag'], offset_mean=d['offset_mean_lag'], log_z=d['log_z']), grid)
        out[key] = dict(x=x, lam=lam, grid=grid, pre=pre, yard=yard)
    worst = [min(max(v['yard'][lag][q] for v in out.values() for lag in (8, 20)), PG.CEIL[q]) for q in range(3)]
    out['bar'] = (max(4 * worst[0], 1e-6), 4 * worst[1], 4 * worst[2])
    print(f'yardstick worst over the two inputs (ceilings applied): {worst}, bar {out["bar"]}')
    return out


@pytest.mark.parametrize('lag', [8, 20])
def test_pool_posterior_real_valued(gpu, real_refs, lag):
    """Both inputs in one pool, pushed in unrelated chunkings (a third stream between them): bit-equal to the single-stream call in every field, log_z included
    (asserted per tick by _run_ticks), and the committed marginals, the posterior mean and log_z after every push under the bar against the float64 definition."""
    grid = PG._grid(21)
    xs = dict(g=REAL['grid'][0], x=_ints(9, 70, 21), w=REAL['wide'][0])
    per = dict(g=[(n, False) for n in TS.chunking('ragged', 70, lag)] + [(0, True)], x=[(70, True)],
               w=[None] + [(n, i == len(TS.chunking('long_after_short', 70, lag)) - 1) for i, n in enumerate(TS.chunking('long_after_short', 70, lag))])
    ticks = [[(s, *v[t]) for s, v in per.items() if t < len(v) and v[t] is not None] for t in range(max(len(v) for v in per.values()))]
    outs, _ = _run_ticks(gpu, xs, ticks, dict(g=1, x=2, w=0), lag, 8.0, grid, n_slots=3)
    bar, step = real_refs['bar'], float(grid[1] - grid[0])
    for s, key in (('g', 'grid'), ('w', 'wide')):
        case = real_refs[key]
        ref = TS.by_definition(case['x'].astype(np.float64), 8.0, lag, [p for p in per[s] if p is not None], grid.astype(np.float64), pre=case['pre'])
        gp, rp = _cat(outs[s], 'post_lag'), np.concatenate([r['post_lag'] for r in ref])
        e_post = float(np.abs(gp - rp).max())
        e_mean = float(np.abs(_cat(outs[s], 'offset_mean_lag') - np.concatenate([r['offset_mean_lag'] for r in ref])).max()) / step
        e_z = max(abs(o.log_z.item() - r['log_z']) / max(1.0, abs(r['log_z'])) for o, r in zip(outs[s], ref))
        print(f'{key} lag {lag}: ' + '  '.join(f'{n} {e:.3e} (yardstick {y:.3e}, bar {b:.3e})' for n, e, y, b in zip(PG.QUANT, (e_post, e_mean, e_z), case['yard'][lag], bar)))
        assert gp.shape == (70, 21) and np.isfinite(gp).all() and np.abs(gp.sum(1) - 1).max() <= 1e-5
        assert e_post <= bar[0] and e_mean <= bar[1] and e_z <= bar[2], (key, (e_post, e_mean, e_z), bar)
        assert all(o.log_z.item() <= 1e-5 for o in outs[s])


# ---- isolation -----------------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_rows_stay_inside_their_stream(gpu):
    """Stream 'n' carries a row of NaN and a row of +inf: its classes stay in [0, C), and its neighbours in the same pushes are bit-equal to a run without it."""
    rng = np.random.default_rng(3)
    xs = {s: rng.standard_normal((40, C21)).astype(np.float32) for s in 'anb'}
    xs['n'][11, :] = np.nan
    xs['n'][23, :] = np.inf
    grid = PG._grid(C21)
    for lag in (0, 3, 9):
        sizes = TS.chunking('ragged', 40, lag)
        ticks = [[(s, n, i == len(sizes) - 1) for s in 'anb'] for i, n in enumerate(sizes)]
        with_n, _ = _run_ticks(gpu, xs, ticks, dict(a=0, n=1, b=2), lag, 1.0, grid, n_slots=3)
        without, _ = _run_ticks(gpu, dict(a=xs['a'], b=xs['b']), [[e for e in tk if e[0] != 'n'] for tk in ticks], dict(a=0, b=2), lag, 1.0, grid, n_slots=3)
        for s in 'ab':
            for u, v in zip(with_n[s], without[s]):
                assert u.w0 == v.w0 and all(_same(getattr(u, k), getattr(v, k)) for k in FIELDS), (lag, s)
            assert np.isfinite(_cat(with_n[s], 'post_lag')).all()
        for k in ('cls_raw', 'cls_lag', 'cls_tail', 'cls_post_lag'):
            c = _cat(with_n['n'], k)
            assert c.size == 0 or (c.min() >= 0 and c.max() < C21), (lag, k, c)
        assert _cat(with_n['n'], 'cls_lag').shape == (40,) and np.array_equal(_cat(with_n['n'], 'cls_raw')[:11], xs['n'][:11].argmax(1))


def test_table_and_slot_order_do_not_matter(gpu):
    """The same ticks with the table rows permuted (so every stream's rows, committed block and tail lie elsewhere in the packed buffers) and the streams in other
    slots: the same per-stream results."""
    lag, lam, grid = 8, 0.5, PG._grid(C21)
    xs = {s: PG._randn(300 + i, W70, C21, 3.0) for i, s in enumerate('abcde')}
    _, ticks = _five_streams(lag)
    one, _ = _run_ticks(gpu, xs, ticks, SLOTS5, lag, lam, grid)
    rng = np.random.default_rng(8)
    shuffled = [[tk[i] for i in rng.permutation(len(tk))] for tk in ticks]
    assert any(a != b for a, b in zip(ticks, shuffled))
    two, _ = _run_ticks(gpu, xs, shuffled, dict(a=1, b=6, c=0, d=2, e=4), lag, lam, grid)
    for s in xs:
        assert len(one[s]) == len(two[s])
        for u, v in zip(one[s], two[s]):
            assert u.w0 == v.w0 and all(_same(getattr(u, k), getattr(v, k)) for k in FIELDS), s


# ---- end to end: OffsetStreamPool against OffsetTracker.stream and track / track_raw on the finished recordings ----------------------------------------------
def _equal_updates(a, b, what):
    for f in dataclasses.fields(a):
        u, v = getattr(a, f.name), getattr(b, f.name)
        if isinstance(u, torch.Tensor):
            assert isinstance(v, torch.Tensor) and u.shape == v.shape and u.dtype == v.dtype and u.device == v.device and torch.equal(u, v), (what, f.name, u, v)
        else:
            assert u == v, (what, f.name, u, v)


def _joined(push_upd, flush_upd):
    """What one final push WITH data returns, from a stream's push of the same data and its flush(): the committed blocks one after the other (a window is read
    from the same prefix either way), the push's new windows, the flush's (empty) tail and log_z."""
    kw = {}
    for f in dataclasses.fields(push_upd):
        u, v = getattr(push_upd, f.name), getattr(flush_upd, f.name)
        if f.name in ('w_new', 'logits', 'cls_raw', 'conf_raw', 'w0'):
            kw[f.name] = u
        elif f.name in ('t_sec_tail', 'cls_tail', 'conf_tail', 'offset_sec_tail', 'log_z'):
            kw[f.name] = v
        else:
            kw[f.name] = None if u is None else torch.cat([u, v])
    assert flush_upd.logits.shape[0] == 0 and flush_upd.w0 == push_upd.w0 + push_upd.cls_lag.shape[0]
    return type(push_upd)(**kw)


def test_offset_stream_pool_equals_streams_and_tracks(gpu, rec):
    """Three feeds in a pool of three slots on the un-fused tower schedule (seg_chunk = 5, lam = 0.5, posterior on), ragged unrelated pushes: 'ing' the fixture's
    recording as 50 fps channels-last frames with 48 kHz stereo sound through an ingest, 'two' a second seeded recording opened late, 'short' that one again 40
    frames shorter (104 frames: 12 segments, it never completes a window) flushed early with its last data; 'late' re-opens its slot with the fixture's recording.
    Every update of every feed equals the same pushes through tracker.stream(...), each feed's logits those of track() / track_raw() on its finished recording."""
    from synchformer_amd import synth
    from synchformer_amd.ingest import RecordingIngest
    tracker, lag = rec['tracker'], 2
    T, N = SG.T_REC, SG.N_REC
    raw50 = rec['raw'].repeat_interleave(2, 0).permute(0, 2, 3, 1).contiguous()                              # (288, 256, 256, 3)
    wave48 = torch.rand(2, 3 * N, generator=torch.Generator().manual_seed(48)) * 2 - 1
    ing50 = RecordingIngest(gpu, 50, (256, 256), 48000, channels_last=True)
    crop2 = torch.randint(0, 256, (T, 3, 224, 224), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    wave2 = synth.make_wave(1, 1, 7, n=N).reshape(N)
    src = dict(ing=(raw50, wave48, SG._ragged(2 * T, 3 * N, f_runs=(1, 7, 40, 0, 3, 50), a_runs=(48000, 0, 1001, 120000, 15360, 0, 1)), ing50),
               two=(crop2.to(gpu), wave2, SG._ragged(T, N, f_runs=(30, 0, 9, 64), a_runs=(0, 30000, 7, 50000)), None),
               short=(crop2[:T - 40], wave2.to(gpu), SG._ragged(T - 40, N, f_runs=(5, 50, 0, 20), a_runs=(20000, 1, 0, 40000, 12000)), None),
               late=(rec['crop'], rec['wave'].to(gpu), SG._ragged(T, N), None))
    first_tick = dict(ing=0, short=0, two=2)
    pool = tracker.pool(3, lag=lag)
    feeds, ups, left = {}, {k: [] for k in src}, {k: list(v[2]) for k, v in src.items()}
    flushed_with_data = set()
    tick = 0
    while any(left.values()) or any(not f.closed for f in feeds.values()):
        assert tick < 60
        for name, t0 in first_tick.items():
            if t0 == tick:
                feeds[name] = pool.open(ingest=src[name][3])
        if tick == 2:
            with pytest.raises(RuntimeError, match='slots are taken'):
                pool.open()
        if 'late' not in feeds and 'short' in feeds and feeds['short'].closed:
            feeds['late'] = pool.open()
            assert feeds['late'].slot == feeds['short'].slot                      # the freed slot, re-opened
        data, flush = {}, []
        for name, f in feeds.items():
            if f.closed:
                continue
            if left[name]:
                f0, f1, a0, a1 = left[name].pop(0)
                data[f] = (src[name][0][f0:f1], src[name][1][..., a0:a1])
                if name == 'short' and not left[name]:
                    flush.append(f)                                               # flushed with its last data, early: the others go on
                    flushed_with_data.add(name)
            else:
                flush.append(f)                                                   # flushed without data, one tick after its last push
        got = pool.push(data, flush=flush)
        assert set(got) == set(data) | set(flush)
        for name, f in feeds.items():
            if f in got:
                ups[name].append(got[f])
                assert all(f.held[k] <= f.held_bound[k] for k in f.held_bound), (name, f.held, f.held_bound)
                assert f.closed == (f in flush)
        tick += 1
    torch.cuda.synchronize()
    assert flushed_with_data == {'short'} and all(f.closed for f in feeds.values()) and len(feeds) == 4 and not pool.feeds
    with pytest.raises(RuntimeError, match='closed'):
        pool.push({feeds['two']: (crop2[:0], wave2[:0])})
    # the same pushes through a stream of its own, feed by feed
    for name, (frames, wave, pieces, ing) in src.items():
        stream = tracker.stream(lag=lag, ingest=ing)
        want = [stream.push(frames[f0:f1], wave[..., a0:a1]) for f0, f1, a0, a1 in pieces] + [stream.flush()]
        if name in flushed_with_data:
            want = want[:-2] + [_joined(want[-2], want[-1])]
        assert len(want) == len(ups[name]), (name, len(want), len(ups[name]))
        for i, (u, v) in enumerate(zip(ups[name], want)):
            _equal_updates(u, v, (name, i))
        assert feeds[name].n_segments == stream.n_segments and feeds[name].n_windows == stream.n_windows
    # and the finished recordings
    refs = dict(ing=tracker.track_raw(raw50, wave48, ing50), two=tracker.track(crop2.to(gpu), wave2.to(gpu)), late=rec['ref'])
    for name, ref in refs.items():
        logits = torch.cat([u.logits for u in ups[name]])
        assert logits.shape[0] >= SG.N_WIN and torch.equal(logits, ref.logits), name
        assert torch.equal(torch.cat([u.cls_raw for u in ups[name]]), ref.cls_raw) and sum(u.cls_lag.shape[0] for u in ups[name]) == ref.logits.shape[0]
    assert not torch.equal(refs['two'].logits, refs['late'].logits)
    assert feeds['short'].n_segments == 12 and sum(u.logits.shape[0] + u.cls_lag.shape[0] for u in ups['short']) == 0
    with pytest.raises(ValueError):
        tracker.track(crop2[:T - 40].to(gpu), wave2.to(gpu))
