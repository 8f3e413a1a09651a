"""Per-push time of the fixed-lag read-out (sf_track_stream_push) next to the one alternative that exists: ops.track_decode (+ ops.track_posterior)
re-run on every row so far.  Prints one JSON line per configuration.

    python tools/track_stream_readout.py [--classes 21] [--reps 200] [--gate [--mu 2.0]]

A stream of random logits is pushed n rows at a time (n = 1: a live feed at one window per push; n = 1000: a catch-up) after `history` rows are already in, at
lag 16 and 255, with and without the posterior; a push is timed by device events around `reps` consecutive pushes on one stream (no synchronisation between
them: the state advances in stream order), after a warm-up of the same pushes.  The offline re-run is timed the same way at W = 1000 and 100000 rows.  Output
allocation (the ops allocate their outputs) is inside both sides' times.
--gate: instead, the one-row and the 1000-row push at lag 16 through ops.track_stream_push and ops.track_stream_push_gated side by side - the same
binary, the same process, the two alternating five times each; median, min and max of the five per side."""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--classes', type=int, default=21)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--gate', action='store_true', help='time the gated push beside the ungated one (lag 16), alternating')
    ap.add_argument('--mu', type=float, default=2.0)
    args = ap.parse_args()
    from synchformer_amd import ops
    dev = torch.device('cuda:0')
    C = args.classes
    gen = torch.Generator(device=dev).manual_seed(3)
    grid = torch.linspace(-2, 2, C, device=dev)

    def events(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    if args.gate:
        import statistics
        for posterior in (False, True):
            for n in (1, 1000):
                reps = args.reps if n == 1 else max(10, args.reps // 10)
                g = grid if posterior else None
                x, z = 3 * torch.randn(n, C, device=dev, generator=gen), 3 * torch.randn(n, 2, device=dev, generator=gen)
                hx, hz = 3 * torch.randn(300, C, device=dev, generator=gen), 3 * torch.randn(300, 2, device=dev, generator=gen)
                plain, gated = ops.track_stream_state(C, 16, posterior, dev), ops.track_stream_state_gated(C, 16, posterior, dev)
                ops.track_stream_push(plain, hx, 1.0, g)                         # history: the rings are full
                ops.track_stream_push_gated(gated, hx, hz, 1.0, args.mu, g)
                push_a = lambda: ops.track_stream_push(plain, x, 1.0, g)         # noqa: E731
                push_b = lambda: ops.track_stream_push_gated(gated, x, z, 1.0, args.mu, g)      # noqa: E731
                for _ in range(10):
                    push_a()
                    push_b()
                a, b = [], []
                for _ in range(5):
                    a.append(events(push_a, reps))
                    b.append(events(push_b, reps))
                stat = lambda v: {'median': round(1e3 * statistics.median(v), 2), 'min': round(1e3 * min(v), 2), 'max': round(1e3 * max(v), 2)}      # noqa: E731
                print(json.dumps({'tool': 'track_stream_readout', 'what': 'push_gated_vs_ungated', 'classes': C, 'posterior': posterior, 'lag': 16, 'rows_per_push': n,
                                  'reps': reps, 'runs_per_side': 5, 'ungated_us_per_push': stat(a), 'gated_us_per_push': stat(b), 'mu': args.mu,
                                  'state_bytes': [int(plain.buf.numel()), int(gated.buf.numel())]}), flush=True)
        return
    for posterior in (False, True):
        for lag in (16, 255):
            for n in (1, 1000):
                reps = args.reps if n == 1 else max(10, args.reps // 10)
                x = 3 * torch.randn(n, C, device=dev, generator=gen)
                state = ops.track_stream_state(C, lag, posterior, dev)
                ops.track_stream_push(state, 3 * torch.randn(300, C, device=dev, generator=gen), 1.0, grid if posterior else None)     # history: the rings are full
                for _ in range(10):
                    ops.track_stream_push(state, x, 1.0, grid if posterior else None)
                ms = events(lambda: ops.track_stream_push(state, x, 1.0, grid if posterior else None), reps)
                print(json.dumps({'tool': 'track_stream_readout', 'what': 'push', 'classes': C, 'posterior': posterior, 'lag': lag, 'rows_per_push': n,
                                  'reps': reps, 'ms_per_push': round(ms, 4), 'us_per_row': round(1e3 * ms / n, 3), 'state_bytes': int(state.buf.numel())}), flush=True)
    for W in (1000, 100000):
        x = 3 * torch.randn(W, C, device=dev, generator=gen)
        reps = 20 if W == 1000 else 3
        ms_d = events(lambda: ops.track_decode(x, 1.0), reps)
        ms_p = events(lambda: ops.track_posterior(x, 1.0, grid), reps)
        print(json.dumps({'tool': 'track_stream_readout', 'what': 'offline_rerun', 'classes': C, 'rows': W, 'reps': reps, 'track_decode_ms': round(ms_d, 3),
                          'track_posterior_ms': round(ms_p, 3)}), flush=True)


if __name__ == '__main__':
    main()
