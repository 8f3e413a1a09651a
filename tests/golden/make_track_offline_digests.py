"""Fixture of tests/test_track_offline_pinned_gpu.py: the SHA-256 of everything the whole-recording track read-outs return - sf_track_decode, sf_track_posterior,
sf_track_pairwise and their gated forms (csrc/sf_track.hip behind ops.track_decode / track_posterior / track_pairwise / track_decode_gated / track_posterior_gated /
track_pairwise_gated).  The oracle tests of these read-outs judge the path by its score and the marginals within a bar; they would pass a changed order of a sum or a
fused multiply-add that was two operations before.  This file pins the BYTES: every tensor the three calls of a case return, in order (a None - xi when it was not asked
for - adds its position only; the back pointers and the workspace are scratch and are not digested).  Where `post` is a strided view, the whole buffer behind it
is digested too, and its padding must still hold the poison.

The file is recorded ONCE, on the GPU, from the tree AND the library of the commit it names - the PARENT of the change under test - exactly as
make_track_stream_digests.py describes:

    git worktree add ../parent <commit> && (cd ../parent && python -c "import __graft_entry__ as g; g.build()")
    python tests/golden/make_track_offline_digests.py --tree ../parent --commit <commit>

It records every case twice and refuses to write unless the two recordings are equal.  All inputs are drawn on the CPU under fixed seeds (3 * randn logits, 3 * randn
gate logits, linspace(-2, 2, C) as grid); each case's input digest is stored next to its output digest.  No input holds a NaN.

A case is (chain, C, W): C in {2, 21, 32} (C4 pads 2 to 4 and 21 to 24; 32 gated fills the 64 lanes), 64 too for the plain chain; W in {1, 2, 5, 6, 9, 10, 257}:
    1        no scan step, the pairwise early return;
    2        one step, no prefetch;
    5, 6     exactly four boundaries fill a pairwise block, then a fifth leaves three idle waves;
    9, 10    the backtrace is exactly one round of eight rows, then one more;
    257      the one-thread-per-window kernels cross a 256-thread block.
Three more inputs at C = 21, W = 65: one class masked with -inf in every third row (plain chain only: the header does not serve masked classes on the gated chain);
logits, gate logits and `post` as strided views (row strides C + 3, 5 and C + 5) whose padding holds a finite poison; track_pairwise with xi=False."""
import argparse
import functools
import hashlib
import json
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
OUT = HERE / 'track_offline_digests.json'
LAM, MU = 0.7, 1.3                       # not dyadic: a product that is rounded once instead of twice shows in the bytes
POISON = 1000.0                          # the padding of the strided inputs and of the strided `post`
WS = (1, 2, 5, 6, 9, 10, 257)
EXTRA_C, EXTRA_W = 21, 65


class Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, t):
        self.h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())

    def add_result(self, call: str, out):
        """Every tensor a call returned, in order: the call's name and the position, then the bytes (nothing for None)."""
        for i, v in enumerate(out):
            self.h.update(f'{call}[{i}]'.encode())
            if v is not None:
                self.add(v)

    def hexdigest(self):
        return self.h.hexdigest()


def _randn(*shape, seed):
    return 3.0 * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _inputs(C: int, W: int, variant):
    """(logits (W, C), gate logits (W, 2), grid (C,)) on the CPU."""
    x, z = _randn(W, C, seed=17000 + 300 * C + W), _randn(W, 2, seed=18000 + 300 * C + W)
    if variant == 'masked':
        x[::3, C // 4] = float('-inf')
    return x, z, torch.linspace(-2.0, 2.0, C)


def _padded(t, ld, dev):
    buf = torch.full((t.shape[0], ld), POISON, device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf[:, :t.shape[1]]


class OfflineCase:
    def __init__(self, gated, C, W, variant=None):
        self.gated, self.C, self.W, self.variant = gated, C, W, variant

    def inputs(self):
        x, z, grid = _inputs(self.C, self.W, self.variant)
        return [x, z, grid] if self.gated else [x, grid]

    def run(self, dev) -> str:
        from synchformer_amd import ops
        x, z, grid = _inputs(self.C, self.W, self.variant)
        C, W, strided = self.C, self.W, self.variant == 'strided'
        xd, zd = (_padded(x, C + 3, dev), _padded(z, 5, dev)) if strided else (x.to(dev), z.to(dev))
        gd = grid.to(dev)
        post_buf = torch.full((W, C + 5), POISON, device=dev) if strided else None
        post = post_buf[:, :C] if strided else None
        xi = self.variant != 'no_xi'
        d = Digest()
        if self.gated:
            d.add_result('decode', ops.track_decode_gated(xd, zd, LAM, MU))
            d.add_result('posterior', ops.track_posterior_gated(xd, zd, LAM, MU, gd, post=post))
            d.add_result('pairwise', ops.track_pairwise_gated(xd, zd, LAM, MU, xi=xi))
        else:
            d.add_result('decode', ops.track_decode(xd, LAM))
            d.add_result('posterior', ops.track_posterior(xd, LAM, gd, post=post))
            d.add_result('pairwise', ops.track_pairwise(xd, LAM, xi=xi))
        if strided:                      # the whole buffer behind `post`, padding included: nothing beyond column C may be written
            assert bool((post_buf[:, C:] == POISON).all()), 'the padding of the strided post was written'
            d.add(post_buf)
        return d.hexdigest()


# name -> a case: .inputs() the CPU tensors it is fed from, .run(device) the digest of what the three calls returned
CASES = {}
for _g in (False, True):
    _kind = 'gated' if _g else 'plain'
    for _C in (2, 21, 32) + (() if _g else (64,)):
        for _W in WS:
            CASES[f'{_kind}_C{_C}_W{_W}'] = OfflineCase(_g, _C, _W)
    for _v in (('strided', 'no_xi') if _g else ('masked', 'strided', 'no_xi')):
        CASES[f'{_kind}_C{EXTRA_C}_W{EXTRA_W}_{_v}'] = OfflineCase(_g, EXTRA_C, EXTRA_W, _v)


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
