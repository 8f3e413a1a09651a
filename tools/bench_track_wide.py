"""First measurement of the wide chain (profiles/track_wide.md): time per step of ops.track_decode_wide / ops.track_posterior_wide at S = 21, 210, 1008
states (D = 1, 10, 48 lags of 21 classes) and W = 173, 11000 windows, beside ops.track_decode / ops.track_posterior at C = 21 on the lag-0 rows of the same logits;
and engine.sync_windows_lagged at D = 25 beside 25 calls of engine.sync_windows on banks sliced by hand.  The calls alternate inside one process; a round is a batch
of calls between two device events; median (min .. max) of the rounds.  One JSON line per measurement.

    python tools/bench_track_wide.py [--rounds 9] [--no-engine]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rounds_of(fns, batch: int, rounds: int, warmup: int = 3):
    """fns: name -> callable.  Alternates the callables round by round -> name -> sorted per-call times (s) of the rounds."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e-3 / batch)
    return {name: sorted(v) for name, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--no-engine', action='store_true', help='skip the sync_windows_lagged comparison')
    args = ap.parse_args()
    from synchformer_amd import ops
    from synchformer_amd.postprocess import class_grid
    dev = torch.device('cuda:0')
    grid = class_grid(-2, 2, 21)
    gd = grid.to(dev)
    for W, batch in ((173, 40), (11000, 2)):
        for D in (1, 10, 48):
            lags = tuple(range(-(D // 2), D - D // 2))
            src, pos, off, lag_of, cls_of = ops.track_wide_states(lags, grid)
            tables = ops.track_wide_tables(src, pos, off, D, 21, dev)
            x = 3 * torch.randn(W, D, 21, generator=torch.Generator().manual_seed(W + D)).to(dev)
            x0 = x[:, D // 2].contiguous()                                       # the rows of lag 0
            res = rounds_of({'decode_wide': lambda: ops.track_decode_wide(x, tables, 1.0), 'posterior_wide': lambda: ops.track_posterior_wide(x, tables, 1.0),
                             'decode_plain_C21': lambda: ops.track_decode(x0, 1.0), 'posterior_plain_C21': lambda: ops.track_posterior(x0, 1.0, gd)}, batch, args.rounds)
            for name, v in res.items():
                print(json.dumps({'what': name, 'W': W, 'D': D, 'S': D * 21, 'call_us': round(statistics.median(v) * 1e6, 1), 'min_us': round(v[0] * 1e6, 1),
                                  'max_us': round(v[-1] * 1e6, 1), 'step_us': round(statistics.median(v) * 1e6 / W, 4)}), flush=True)
    if args.no_engine:
        return
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    eng = SynchformerEngine(synth.make_state_dict(1337), dev)
    lags = tuple(range(-12, 13))
    N = 14 + 12 + 12 + 172                                                       # 173 windows at every lag
    g = torch.Generator().manual_seed(5)
    vbank, abank = torch.randn(N, 8, 768, generator=g).to(dev), torch.randn(N, 6, 768, generator=g).to(dev)
    n = 172 + 14

    def by_hand():
        return [eng.sync_windows(vbank[12:12 + n], abank[12 + d:12 + d + n]) for d in lags]

    res = rounds_of({'sync_windows_lagged_D25': lambda: eng.sync_windows_lagged(vbank, abank, lags), 'sync_windows_x25': by_hand,
                     'sync_windows_x1': lambda: eng.sync_windows(vbank[12:12 + n], abank[12:12 + n])}, 2, args.rounds)
    for name, v in res.items():
        print(json.dumps({'what': name, 'W': 173, 'call_ms': round(statistics.median(v) * 1e3, 3), 'min_ms': round(v[0] * 1e3, 3), 'max_ms': round(v[-1] * 1e3, 3)}), flush=True)


if __name__ == '__main__':
    main()
