"""Fit OffsetTracker's lam (and, with a gate, mu) on labelled recordings: track.fit_smoothness driven by the pairwise read-out on the device.

    python tools/fit_track.py [--windows 2000] [--classes 21] [--lam 1.0] [--scale 3.0] [--seed 0] [--gate [--mu 2.0]] [--recordings 1]
    python tools/fit_track.py --npz FILE [--gate]

Without --npz the tool checks itself: it draws `scale * randn` logits (with --gate also 2 * randn gate logits), samples the labels of every window from the chain at
the known --lam (--mu) by forward filtering and backward sampling in float64 on the host, fits, and prints one JSON line: truth, fit, standard error, the distance
in standard errors, observed and expected class steps (flag changes), the log-likelihood and the milliseconds per evaluation of the read-out (one
ops.track_pairwise(_gated) call per recording, its sums read back: wall clock around the whole fit over the evaluations - launches, allocations and the two read-backs,
not kernel time).

--npz FILE fits a user's arrays: `logits` (W, C) fp32 and `labels` (W,) int - e.g. OffsetTrack.logits of an in-sync recording whose audio was shifted by a known amount,
and the class of that shift in every window; with --gate also `gate_logits` (W, 2) and `sync_labels` (W,) in {0, 1}.  Several recordings: the same names with a suffix
_0, _1, ...  The line then has no truth to compare with."""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def _lse(x: torch.Tensor, dim: int) -> torch.Tensor:
    return torch.logsumexp(x, dim)


def sample_states(g: torch.Generator, logits: torch.Tensor, lam: float, gate_logits=None, mu: float = 0.0) -> torch.Tensor:
    """One path (W,) from the chain, float64 on the host (states j = m * C + c with a gate): the forward scan, then backward sampling."""
    l = logits.double()
    W, C = l.shape
    e = l - _lse(l, 1)[:, None]
    idx = torch.arange(C)
    dist = (idx[:, None] - idx[None, :]).abs().double()
    if gate_logits is None:
        E, S = e, -lam * dist
    else:
        d = gate_logits.double()[:, 1] - gate_logits.double()[:, 0]
        E = torch.cat([(torch.nn.functional.logsigmoid(-d) - math.log(C))[:, None].expand(W, C), torch.nn.functional.logsigmoid(d)[:, None] + e], 1)
        m = torch.arange(2 * C) // C
        S = -lam * dist.repeat(2, 2) - mu * (m[:, None] != m[None, :]).double()
    a = torch.empty_like(E)
    a[0] = E[0]
    for w in range(1, W):
        a[w] = E[w] + _lse(a[w - 1][:, None] + S, 0)
    path = torch.empty(W, dtype=torch.int64)
    path[W - 1] = torch.multinomial(torch.softmax(a[W - 1], 0), 1, generator=g)
    for w in range(W - 2, -1, -1):
        path[w] = torch.multinomial(torch.softmax(a[w] + S[:, path[w + 1]], 0), 1, generator=g)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--npz', default=None, help='fit these arrays instead of the self-check: logits, labels (gate_logits, sync_labels), optionally with suffixes _0, _1, ...')
    ap.add_argument('--windows', type=int, default=2000)
    ap.add_argument('--classes', type=int, default=21)
    ap.add_argument('--recordings', type=int, default=1)
    ap.add_argument('--lam', type=float, default=1.0, help='the lam the labels are sampled at')
    ap.add_argument('--mu', type=float, default=2.0, help='the mu the labels are sampled at (with --gate)')
    ap.add_argument('--scale', type=float, default=3.0, help='standard deviation of the synthetic logits')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--gate', action='store_true', help='fit the chain over (offset class, synchronizable flag): lam and mu')
    ap.add_argument('--lam-max', type=float, default=16.0)
    ap.add_argument('--mu-max', type=float, default=16.0)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--sweeps', type=int, default=4)
    args = ap.parse_args()
    from synchformer_amd.track import fit_smoothness
    assert torch.cuda.is_available(), 'the fit runs the pairwise read-out on the device'
    dev = torch.device('cuda:0')
    recs, truth = [], {}
    if args.npz is not None:
        import numpy as np
        data = np.load(args.npz)
        suffixes = [''] if 'logits' in data else sorted({k[len('logits'):] for k in data.files if k.startswith('logits_')})
        for s in suffixes:
            item = [torch.from_numpy(data['logits' + s]).float().to(dev), torch.from_numpy(data['labels' + s])]
            if args.gate:
                item += [torch.from_numpy(data['gate_logits' + s]).float().to(dev), torch.from_numpy(data['sync_labels' + s])]
            recs.append(tuple(item))
    else:
        g = torch.Generator().manual_seed(args.seed)
        truth = {'lam_true': args.lam, **({'mu_true': args.mu} if args.gate else {})}
        for _ in range(args.recordings):
            logits = (args.scale * torch.randn(args.windows, args.classes, generator=g)).float()
            gate_logits = (2 * torch.randn(args.windows, 2, generator=g)).float() if args.gate else None
            states = sample_states(g, logits, args.lam, gate_logits, args.mu)
            recs.append((logits.to(dev), states % args.classes, gate_logits.to(dev), states // args.classes) if args.gate else (logits.to(dev), states))
    fit_smoothness(recs, gated=args.gate, lam_max=args.lam_max, mu_max=args.mu_max, iters=2, sweeps=1)          # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f = fit_smoothness(recs, gated=args.gate, lam_max=args.lam_max, mu_max=args.mu_max, iters=args.iters, sweeps=args.sweeps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    line = {'tool': 'fit_track', 'recordings': len(recs), 'windows': [int(r[0].shape[0]) for r in recs], 'classes': int(recs[0][0].shape[1]), 'gated': bool(args.gate),
            **truth, 'lam': round(f.lam, 6), 'se_lam': round(f.se_lam, 6), 'lam_at_bound': f.lam_at_bound}
    if 'lam_true' in truth:
        line['lam_off_by_se'] = round((f.lam - args.lam) / f.se_lam, 3)
    if args.gate:
        line.update({'mu': round(f.mu, 6), 'se_mu': round(f.se_mu, 6), 'mu_at_bound': f.mu_at_bound})
        if 'mu_true' in truth:
            line['mu_off_by_se'] = round((f.mu - args.mu) / f.se_mu, 3)
    line.update({'jumps_observed': f.jumps_observed, 'jumps_expected': round(f.jumps_expected, 3), 'flips_observed': f.flips_observed,
                 'flips_expected': round(f.flips_expected, 3), 'log_likelihood': round(f.log_likelihood, 3), 'evaluations': f.evaluations,
                 'ms_per_evaluation': round(1e3 * dt / f.evaluations, 4)})
    print(json.dumps(line))


if __name__ == '__main__':
    main()
