"""Many live feeds on one device: A = one OffsetStream per feed, pushed in a loop (what a monitor had before the pool) against B = one
OffsetStreamPool, in one process, alternating, and the read-out alone (ops.track_pool_push against a loop of ops.track_stream_push).  One JSON line per result.

    python tools/track_pool.py [--feeds 16] [--seconds 20] [--stream 1.0] [--lag 16] [--posterior] [--reps 3] [--seg-chunk N] [--stages] [--gate [--mu X]]

Inputs are synthetic feeds from seeds (random frames and samples on the device, feed i from seed i, every feed a little shorter than the one before: content and
length differ per feed; the weights are synth.make_state_dict's).  Every tick hands each feed that still has data its next `--stream` seconds (25 fps frames,
16 kHz samples); a feed that ran out is flushed.  A run is timed by the host clock around all its ticks with a device synchronise after every tick inside the
window (a monitor reads the committed offsets every tick); one untimed run of each side first, then `--reps` runs of each, A and B alternating.  Reported per side:
ms per tick, segments / s and the feeds one device carries in real time (feeds x tick seconds / tick time), each as the median with min and max over the runs.
--stages adds one more, untimed-for-the-comparison run per side with a synchronise around the towers, the windows and the read-out: the per-stage split.
The read-out alone: 256 streams x 1 row per tick at C = 21 after 300 rows of history each, the same alternation.
--gate: a third side G = the pool of a tracker with a synthetic 2-way syncability engine (towers=False), pool(gated=True), in the same alternation:
what the gate adds per tick beside B of this run (its 13-segment windows through a second sync transformer and the 2C-wide read-out), the committed windows flagged
not synchronizable, and the gated read-out alone (ops.track_pool_push_gated) beside ops.track_pool_push."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def _stats(values, digits=3):
    return dict(median=round(statistics.median(values), digits), min=round(min(values), digits), max=round(max(values), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--feeds', type=int, default=16)
    ap.add_argument('--seconds', type=float, default=20.0)
    ap.add_argument('--stream', type=float, default=1.0, help='seconds of feed per tick')
    ap.add_argument('--lag', type=int, default=16)
    ap.add_argument('--posterior', action='store_true')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--seg-chunk', type=int, default=None, help="the engine's seg_chunk (default: the engine's own)")
    ap.add_argument('--stages', action='store_true')
    ap.add_argument('--readout-streams', type=int, default=256)
    ap.add_argument('--readout-ticks', type=int, default=100)
    ap.add_argument('--gate', action='store_true', help='also run the pool gated by a synthetic 2-way syncability engine (towers=False)')
    ap.add_argument('--mu', type=float, default=2.0, help='cost of one change of the synchronizable flag (with --gate)')
    args = ap.parse_args()
    if args.reps < 3:
        ap.error('--reps: at least three repetitions of each side')
    from synchformer_amd import ops, synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.track import OffsetTracker
    dev = torch.device('cuda:0')
    eng = SynchformerEngine(synth.make_state_dict(1337), dev) if args.seg_chunk is None else SynchformerEngine(synth.make_state_dict(1337), dev, seg_chunk=args.seg_chunk)
    mel = MelFrontend(dev)
    tracker = OffsetTracker(eng, mel, lam=1.0, posterior=args.posterior)
    gated_tracker = None
    if args.gate:
        gate = SynchformerEngine(synth.make_state_dict(4242, head='sync_head', n_pos=184, n_out=2), dev, towers=False)
        gated_tracker = OffsetTracker(eng, mel, lam=1.0, posterior=args.posterior, gate=gate, mu=args.mu)
    base = dict(tool='track_pool', feeds=args.feeds, seconds=args.seconds, stream_s=args.stream, lag=args.lag, posterior=args.posterior, seg_chunk=eng.seg_chunk,
                device=torch.cuda.get_device_name(0))

    # ---- the feeds -------------------------------------------------------------------------------------------------------------------------------------
    feeds = []
    for i in range(args.feeds):
        g = torch.Generator(device=dev).manual_seed(i)
        sec = args.seconds * (1.0 - 0.4 * i / max(1, args.feeds))               # feed i is 2.5 % x i shorter than the first (at 16 feeds)
        nf, na = int(25 * sec), int(16000 * sec) - 137 * i
        feeds.append((torch.randint(0, 256, (nf, 3, 224, 224), device=dev, dtype=torch.uint8, generator=g), torch.rand(na, device=dev, generator=g) * 2 - 1))
    tf, ta = int(round(25 * args.stream)), int(round(16000 * args.stream))
    n_ticks = max((max(f.shape[0] // tf, w.shape[0] // ta) + 1) for f, w in feeds)
    piece = lambda i, t: (feeds[i][0][t * tf:(t + 1) * tf], feeds[i][1][t * ta:(t + 1) * ta])      # noqa: E731
    has = lambda i, t: t * tf < feeds[i][0].shape[0] or t * ta < feeds[i][1].shape[0]               # noqa: E731

    def run_a():
        streams = [tracker.stream(lag=args.lag) for _ in feeds]
        segs = wins = ticks = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(n_ticks + 1):
            live = [i for i, s in enumerate(streams) if not s.closed]
            if not live:
                break
            for i in live:
                u = streams[i].push(*piece(i, t)) if has(i, t) else streams[i].flush()
                wins += u.logits.shape[0]
            torch.cuda.synchronize()
            ticks += 1
        dt = time.perf_counter() - t0
        segs = sum(s.n_segments for s in streams)
        return dt, ticks, segs, wins

    flagged = [0]

    def run_b(gated=False):
        pool = gated_tracker.pool(args.feeds, lag=args.lag, gated=True) if gated else tracker.pool(args.feeds, lag=args.lag)
        handles = [pool.open() for _ in feeds]
        wins = ticks = 0
        zero = torch.zeros((), device=dev, dtype=torch.int64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(n_ticks + 1):
            live = [i for i, f in enumerate(handles) if not f.closed]
            if not live:
                break
            ups = pool.push({handles[i]: piece(i, t) for i in live if has(i, t)}, flush=[handles[i] for i in live if not has(i, t)])
            wins += sum(u.logits.shape[0] for u in ups.values())
            if gated:
                for u in ups.values():
                    zero += (u.sync_lag == 0).sum()
            torch.cuda.synchronize()
            ticks += 1
        dt = time.perf_counter() - t0
        flagged[0] = int(zero.item())
        return dt, ticks, sum(f.n_segments for f in handles), wins

    run_a()
    run_b()
    res = dict(A=[], B=[], G=[])
    if args.gate:
        run_b(gated=True)
    for _ in range(args.reps):
        res['A'].append(run_a())
        res['B'].append(run_b())
        if args.gate:
            res['G'].append(run_b(gated=True))
    assert len({r[1:] for r in res['A'] + res['B'] + res['G']}) == 1, 'the sides did not do the same work'
    _, ticks, segs, wins = res['A'][0]
    out = {}
    for side, what in (('A', 'one OffsetStream per feed, pushed in a loop'), ('B', 'one OffsetStreamPool')):
        ms = [1e3 * r[0] / ticks for r in res[side]]
        out[side] = dict(what=what, ms_per_tick=_stats(ms), segments_per_s=_stats([segs / r[0] for r in res[side]], 1),
                         feeds_in_real_time=_stats([args.feeds * 1e3 * args.stream / m for m in ms], 1))
        print(json.dumps(dict(base, side=side, ticks=ticks, segments=segs, windows=wins, reps=args.reps, **out[side])), flush=True)
    a_ms, b_ms = out['A']['ms_per_tick'], out['B']['ms_per_tick']
    spread = a_ms['max'] - a_ms['min']
    print(json.dumps(dict(base, what='end_to_end', speedup_median=round(a_ms['median'] / b_ms['median'], 3), a_spread_ms=round(spread, 3),
                          gain_ms=round(a_ms['median'] - b_ms['median'], 3), b_beats_a_by_more_than_a_spread=bool(a_ms['min'] - b_ms['max'] > 0 and
                                                                                                                  a_ms['median'] - b_ms['median'] > spread))), flush=True)

    if args.gate:
        g_ms = _stats([1e3 * r[0] / ticks for r in res['G']])
        print(json.dumps(dict(base, side='G', what='one OffsetStreamPool, gated', mu=args.mu, ticks=ticks, windows=wins, reps=args.reps, ms_per_tick=g_ms,
                              gate_adds_ms_per_tick=round(g_ms['median'] - b_ms['median'], 3), gate_adds_fraction=round(g_ms['median'] / b_ms['median'] - 1, 4),
                              windows_not_synchronizable=flagged[0])), flush=True)

    # ---- the per-stage split ----------------------------------------------------------------------------------------------------------------------------
    if args.stages:
        acc = {}

        def timed(name, fn):
            def wrapped(*a, **k):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn(*a, **k)
                torch.cuda.synchronize()
                acc[name] = acc.get(name, 0.0) + time.perf_counter() - t0
                return r
            return wrapped

        saved = (eng.both_towers, eng.sync_windows, eng.sync_transformer, ops.track_stream_push, ops.track_pool_push)
        eng.both_towers, eng.sync_windows, eng.sync_transformer = timed('towers', saved[0]), timed('windows', saved[1]), timed('windows', saved[2])
        ops.track_stream_push, ops.track_pool_push = timed('readout', saved[3]), timed('readout', saved[4])
        try:
            for side, run in (('A', run_a), ('B', run_b)):
                acc.clear()
                dt, ticks, _, _ = run()
                print(json.dumps(dict(base, what='stages', side=side, ms_per_tick={k: round(1e3 * v / ticks, 3) for k, v in acc.items()},
                                      other_ms_per_tick=round(1e3 * (dt - sum(acc.values())) / ticks, 3))), flush=True)
        finally:
            eng.both_towers, eng.sync_windows, eng.sync_transformer, ops.track_stream_push, ops.track_pool_push = saved

    # ---- the read-out alone -----------------------------------------------------------------------------------------------------------------------------
    S, C, T = args.readout_streams, 21, args.readout_ticks
    gen = torch.Generator(device=dev).manual_seed(3)
    grid = torch.linspace(-2, 2, C, device=dev) if args.posterior else None
    history = 3 * torch.randn(S, 300, C, device=dev, generator=gen)
    rows = 3 * torch.randn(T, S, C, device=dev, generator=gen)

    def readout_a():
        states = [ops.track_stream_state(C, args.lag, args.posterior, dev) for _ in range(S)]
        for i, st in enumerate(states):
            ops.track_stream_push(st, history[i], 1.0, grid)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(T):
            for i, st in enumerate(states):
                ops.track_stream_push(st, rows[t, i:i + 1], 1.0, grid)
            torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / T

    def readout_b():
        state = ops.track_pool_state(S, C, args.lag, args.posterior, dev)
        ops.track_pool_push(state, range(S), history.reshape(S * 300, C), [300] * S, 1.0, grid)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(T):
            ops.track_pool_push(state, range(S), rows[t], [1] * S, 1.0, grid)
            torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / T

    gate_history, gate_rows = 3 * torch.randn(S, 300, 2, device=dev, generator=gen), 3 * torch.randn(T, S, 2, device=dev, generator=gen)

    def readout_g():
        state = ops.track_pool_state_gated(S, C, args.lag, args.posterior, dev)
        ops.track_pool_push_gated(state, range(S), history.reshape(S * 300, C), gate_history.reshape(S * 300, 2), [300] * S, 1.0, args.mu, grid)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(T):
            ops.track_pool_push_gated(state, range(S), rows[t], gate_rows[t], [1] * S, 1.0, args.mu, grid)
            torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / T

    readout_a()
    readout_b()
    ra, rb, rg = [], [], []
    if args.gate:
        readout_g()
    for _ in range(args.reps):
        ra.append(readout_a())
        rb.append(readout_b())
        if args.gate:
            rg.append(readout_g())
    sa, sb = _stats(ra, 4), _stats(rb, 4)
    print(json.dumps(dict(tool='track_pool', what='readout_alone', streams=S, rows_per_tick=1, classes=C, lag=args.lag, posterior=args.posterior, ticks=T, reps=args.reps,
                          a_stream_push_loop_ms_per_tick=sa, b_pool_push_ms_per_tick=sb, speedup_median=round(sa['median'] / sb['median'], 2),
                          b_beats_a_by_more_than_a_spread=bool(sa['min'] > sb['max'] and sa['median'] - sb['median'] > sa['max'] - sa['min']))), flush=True)
    if args.gate:
        sg = _stats(rg, 4)
        print(json.dumps(dict(tool='track_pool', what='readout_alone_gated', streams=S, rows_per_tick=1, classes=C, lag=args.lag, posterior=args.posterior, mu=args.mu, ticks=T,
                              reps=args.reps, g_pool_push_gated_ms_per_tick=sg, b_pool_push_ms_per_tick=sb, gate_adds_ms_per_tick=round(sg['median'] - sb['median'], 4))),
              flush=True)


if __name__ == '__main__':
    main()
