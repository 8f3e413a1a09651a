"""Fixture of tests/test_track_pinned_gpu.py: the SHA-256 of everything the fixed-lag read-outs of live feeds write - sf_track_stream_push, sf_track_pool_push and their
gated forms (csrc/sf_track.hip behind ops.track_stream_push / track_pool_push / track_stream_push_gated / track_pool_push_gated).  The oracle tests of these read-outs
judge the path by its score and the posterior within a bar; they would pass a changed order of a sum, a fused multiply-add that was two operations before, or a state
byte that moved.  This file pins the BYTES: every tensor of every push's result in field order (w0 as an int64) and the state buffer after every push (unwritten ring
slots and padding are zero in a fresh state, so these bytes are deterministic; the workspace is not digested).

The file is recorded ONCE, on the GPU, from the tree AND the library of the commit it names - the PARENT of the change under test (ops.py is part of what is pinned, so
the library alone is not enough): an export of that commit, built in place, put first on sys.path:

    git worktree add ../parent <commit> && (cd ../parent && python -c "import __graft_entry__ as g; g.build()")
    python tests/golden/make_track_stream_digests.py --tree ../parent --commit <commit>

It records every case twice and refuses to write unless the two recordings are equal.  All inputs are drawn on the CPU under fixed seeds; each case's input digest is
stored next to its output digest, so that a changed random stream shows as an input mismatch and not as a kernel regression.  No input holds a NaN (NaN payload bits
are no contract; the non-finite tests of the oracle files cover those rows).

Stream cases, plain and gated: C in {2, 21, 32} (64 too for the plain chain) x lag in {0, 1, 16, 255} x posterior off / on x two ways to close.  The rows - 3 * randn
logits, 3 * randn gate logits - go in through one chunk pattern (chunks(lag)): 0 rows on the empty stream, the first row alone, a push shorter than the lag (lag // 2),
one equal to it, one longer that wraps the rings (lag + 7), 0 rows in mid-stream, the rest; closed by final=True on the rest, or by a final push of 0 rows after it.
A case has 300 rows; at lag 255 the pattern needs more than 300 (1 + 127 + 255 + 262) and the case has 665, so that no push of the pattern is cut short.
Two more inputs at C = 21, lag 16: one class masked with -inf in every third row; logits and gate logits as strided views (row strides C + 3 and 5) whose padding
holds a finite poison.

Pool cases, plain and gated: C = 21, lag in {0, 16}, posterior off / on, 5 slots, 4 ticks (POOL_TICKS): the active slots named out of order, ragged counts with zeros,
a named slot that is still empty, a slot closed in tick 2 and reopened in tick 3, and in tick 3 a `post=` whose row stride is wider than C."""
import argparse
import functools
import hashlib
import json
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
OUT = HERE / 'track_stream_digests.json'
ROWS = 300
LAM, MU = 0.7, 1.3                       # not dyadic: a product that is rounded once instead of twice shows in the bytes
POISON = 1000.0                          # the padding of the strided inputs and of the pool's strided `post`
POOL_C, POOL_SLOTS = 21, 5
# (slots, counts, final, reopen before the tick): slot 0 is named in tick 1 with 0 rows while it is still empty; slot 4 closes in tick 2 and reopens in tick 3
POOL_TICKS = (((3, 0, 4, 1), (5, 0, 20, 1), (), ()),
              ((1, 4, 2), (17, 0, 9), (4,), ()),
              ((4, 0, 3, 2), (6, 3, 30, 0), (), (4,)),
              ((2, 1, 0, 3, 4), (1, 0, 12, 2, 25), (0, 3), ()))
POOL_STRIDED_POST_TICK = 2


def chunks(lag: int):
    """The sizes of the pushes of a stream case, in order; None = the rest of the rows."""
    return (0, 1, lag // 2, lag, lag + 7, 0, None)


def n_rows(lag: int) -> int:
    return max(ROWS, sum(c for c in chunks(lag) if c) + 20)


class Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, t):
        self.h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())

    def add_result(self, out):
        """Every field of a TrackStreamOut / TrackGatedStreamOut, in field order: the name, then the bytes (an int as int64, nothing for None)."""
        for name, v in out._asdict().items():
            self.h.update(name.encode())
            if v is not None:
                self.add(torch.tensor([v], dtype=torch.int64) if isinstance(v, int) else v)

    def hexdigest(self):
        return self.h.hexdigest()


def _randn(*shape, seed):
    return 3.0 * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _inputs(C: int, n: int, variant):
    """(logits (n, C), gate logits (n, 2), grid (C,)) on the CPU."""
    x, z = _randn(n, C, seed=7000 + C), _randn(n, 2, seed=8000 + C)
    if variant == 'masked':
        x[::3, C // 4] = float('-inf')
    return x, z, torch.linspace(-2.0, 2.0, C)


def _padded(t, ld, dev):
    buf = torch.full((t.shape[0], ld), POISON, device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf[:, :t.shape[1]]


class StreamCase:
    def __init__(self, gated, C, lag, posterior, close, variant=None):
        self.gated, self.C, self.lag, self.posterior, self.close, self.variant = gated, C, lag, posterior, close, variant

    def inputs(self):
        x, z, grid = _inputs(self.C, n_rows(self.lag), self.variant)
        return [x, z, grid] if self.gated else [x, grid]

    def run(self, dev) -> str:
        from synchformer_amd import ops
        x, z, grid = _inputs(self.C, n_rows(self.lag), self.variant)
        C, strided = self.C, self.variant == 'strided'
        xd, zd = (_padded(x, C + 3, dev), _padded(z, 5, dev)) if strided else (x.to(dev), z.to(dev))
        gd = grid.to(dev) if self.posterior else None
        state = (ops.track_stream_state_gated if self.gated else ops.track_stream_state)(C, self.lag, self.posterior, dev)
        pushes = [[n, False] for n in chunks(self.lag)]
        pushes[-1][0] = x.shape[0] - sum(n for n, _ in pushes[:-1])
        if self.close == 'empty':
            pushes.append([0, False])
        pushes[-1][1] = True
        d, row = Digest(), 0
        for n, final in pushes:
            if self.gated:
                out = ops.track_stream_push_gated(state, xd[row:row + n], zd[row:row + n], LAM, MU, gd, final=final)
            else:
                out = ops.track_stream_push(state, xd[row:row + n], LAM, gd, final=final)
            row += n
            d.add_result(out)
            d.add(state.buf)
        assert row == x.shape[0] and state.closed
        return d.hexdigest()


class PoolCase:
    def __init__(self, gated, lag, posterior):
        self.gated, self.lag, self.posterior = gated, lag, posterior

    def inputs(self):
        x, z, grid = _inputs(POOL_C, sum(sum(t[1]) for t in POOL_TICKS), 'pool')
        return [x, z, grid] if self.gated else [x, grid]

    def run(self, dev) -> str:
        from synchformer_amd import ops
        C = POOL_C
        x, z, grid = _inputs(C, sum(sum(t[1]) for t in POOL_TICKS), 'pool')
        xd, zd, gd = x.to(dev), z.to(dev), grid.to(dev) if self.posterior else None
        state = (ops.track_pool_state_gated if self.gated else ops.track_pool_state)(POOL_SLOTS, C, self.lag, self.posterior, dev)
        d, row = Digest(), 0
        for tick, (slots, counts, final, reopen) in enumerate(POOL_TICKS):
            for s in reopen:
                state.reopen(s)
            n = sum(counts)
            post = None
            if self.posterior and tick == POOL_STRIDED_POST_TICK:
                K = ops.track_pool_plan([state.rows[s] for s in slots], counts, self.lag, [s in final for s in slots]).total_commit
                post = torch.full((K, C + 5), POISON, device=dev)[:, :C]
            if self.gated:
                outs = ops.track_pool_push_gated(state, slots, xd[row:row + n], zd[row:row + n], counts, LAM, MU, gd, final=final, post=post)
            else:
                outs = ops.track_pool_push(state, slots, xd[row:row + n], counts, LAM, gd, final=final, post=post)
            row += n
            for out in outs:
                d.add_result(out)
            d.add(state.buf)
        return d.hexdigest()


# name -> a case: .inputs() the CPU tensors it is fed from, .run(device) the digest of what it wrote
CASES = {}
for _g in (False, True):
    _kind = 'gated' if _g else 'plain'
    for _C in (2, 21, 32) + (() if _g else (64,)):
        for _lag in (0, 1, 16, 255):
            for _p in (False, True):
                for _close in ('rows', 'empty'):
                    CASES[f'stream_{_kind}_C{_C}_lag{_lag}_post{int(_p)}_close_{_close}'] = StreamCase(_g, _C, _lag, _p, _close)
    for _p in (False, True):
        for _v in ('masked', 'strided'):
            CASES[f'stream_{_kind}_C21_lag16_post{int(_p)}_{_v}'] = StreamCase(_g, 21, 16, _p, 'rows', _v)
        for _lag in (0, 16):
            CASES[f'pool_{_kind}_lag{_lag}_post{int(_p)}'] = PoolCase(_g, _lag, _p)


def input_digest(name: str) -> str:
    d = Digest()
    for t in CASES[name].inputs():
        d.add(t)
    return d.hexdigest()


def record(dev):
    cases = {}
    for name, case in CASES.items():
        cases[name] = dict(input=input_digest(name), output=case.run(dev))
        print(f'{name}: input {cases[name]["input"][:16]}  output {cases[name]["output"][:16]}', flush=True)
    return cases


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--tree', type=Path, default=HERE.parent.parent, help='the built tree whose synchformer_amd (ops.py and the library) is recorded')
    ap.add_argument('--commit', required=True, help='the commit that tree is an export of')
    ap.add_argument('--out', type=Path, default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, str(args.tree.resolve()))
    import synchformer_amd
    from synchformer_amd import _lib
    print(f'recording from {synchformer_amd.__file__} and {_lib.lib_path()}')
    assert Path(synchformer_amd.__file__).resolve().parent.parent == args.tree.resolve(), 'synchformer_amd was imported from another tree'
    dev = torch.device('cuda:0')
    first, second = record(dev), record(dev)
    differ = [n for n in first if first[n] != second[n]]
    assert not differ, f'two recordings differ: {differ}'
    args.out.write_text(json.dumps(dict(recorded_from=args.commit, cases=first), indent=1) + '\n')
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
