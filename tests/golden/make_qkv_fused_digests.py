"""Fixture of test_kernels_gpu.py::test_qkv_fused_outputs_are_pinned: the SHA-256 of what the fused qkv + attention launches of csrc/sf_qkv_space.hip and
csrc/sf_qkv_time2.hip write (the parity tests allow a bf16 ulp and would not see a race that a wrong wait count opens, nor a changed order of the k sum).

The file is recorded ONCE, from the library of the commit it names - the PARENT of the change under test, built in a second worktree and selected through
SYNCHFORMER_HIP_LIB (the Python layer is the working tree's: ops.py and _lib.py do not change):

    git worktree add ../parent <commit> && python -c "import sys; sys.path.insert(0, '../parent'); import __graft_entry__ as g; g.build()"
    SYNCHFORMER_HIP_LIB=../parent/synchformer_amd/lib/libsynchformer_hip.so python tests/golden/make_qkv_fused_digests.py --commit <commit>     # needs the GPU

It records every case twice and refuses to write unless the two recordings are equal.  Inputs come from CPU generators under the seeds of the parity tests; each
input's own digest is stored too, so that a change of the random stream shows as an input mismatch and not as a kernel regression."""
import argparse
import functools
import hashlib
import json
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
OUT = HERE / 'qkv_fused_digests.json'
L, D = 1569, 768
FILL = 7.0                 # `out` starts at a constant: the launches leave the CLS rows alone, their bytes are part of the digest


def sha256(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def _bf16_inputs(kernel, n_seq):
    """(x, w, bias) on the CPU under the seeds of test_qkv_space_attention / test_qkv_time_attention2"""
    s = 150 if kernel == 'space' else 160
    return _randn(n_seq * L, D, seed=s).bfloat16(), _randn(3 * D, D, seed=s + 1, scale=0.05).bfloat16(), 0.1 * _randn(3 * D, seed=s + 2)


@functools.lru_cache(maxsize=None)
def _mx_inputs(kernel, n_seq):
    """(x, w, bias) on the CPU as test_qkv_space_attention_mx / test_qkv_time_attention2_mx draw them: block scales that differ widely along K and across rows"""
    s = 190 if kernel == 'space' else 290
    g = torch.Generator().manual_seed(s + n_seq)
    x = (torch.randn(n_seq * L, D, generator=g) * torch.exp2(torch.randint(-3, 3, (n_seq * L, D // 32), generator=g).float()).repeat_interleave(32, 1)).bfloat16()
    w = (torch.randn(3 * D, D, generator=g) * 0.03 * torch.exp2(torch.randint(-2, 2, (3 * D, D // 32), generator=g).float()).repeat_interleave(32, 1)).bfloat16()
    return x, w, 0.1 * _randn(3 * D, seed=s + 2)


@functools.lru_cache(maxsize=None)
def _mask(n_seq):
    """uint8 (n_seq * L): about 20 % random zeros, one fully masked frame, one patch masked in all its 8 frames (a time group left with the CLS key only), a left-over
    patch (tokens 192..195 travel through the side rows) and a masked CLS key - each in a sequence of its own where there are several"""
    keep = torch.rand(n_seq, L, generator=torch.Generator().manual_seed(163)) > 0.2
    keep[1 % n_seq, 1 + 3 * 196:1 + 4 * 196] = False
    keep[2 % n_seq, 1 + 50::196] = False
    keep[0, 1 + 194::196] = False
    keep[3 % n_seq, 0] = False
    return keep.reshape(-1).to(torch.uint8)


def _strided(t, ld):
    """t as a column slice of a wider buffer (row stride ld elements); the columns past t hold a constant the kernels must never read into their result"""
    buf = torch.full((t.shape[0], ld), 3, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _n_part(kernel):
    return 8 if kernel == 'space' else 33


def _bf16_case(kernel, n_seq, masked=False, bias=True, ld=None):
    def run(dev):
        from synchformer_amd import ops
        x, w, b = _bf16_inputs(kernel, n_seq)
        b = b if bias else None
        keep = _mask(n_seq) if masked else None
        xd, wd, bd = x.to(dev), w.to(dev), b.to(dev) if bias else None
        side_in = torch.empty(n_seq * 33, D, device=dev, dtype=torch.bfloat16)
        ops.space_side_rows(xd, side_in, n_seq)
        side = torch.empty(n_seq * 33, 3 * D, device=dev, dtype=torch.bfloat16)
        ops.gemm(side_in, wd, bd, side)
        if ld:
            xd, wd = _strided(xd, ld), _strided(wd, ld)
        out = torch.full((n_seq * L, D), FILL, device=dev, dtype=torch.bfloat16)
        part = torch.zeros(n_seq * 12 * _n_part(kernel) * 66, device=dev)
        fn = ops.qkv_space_attention if kernel == 'space' else ops.qkv_time_attention2
        fn(xd, wd, bd, side, out, part, n_seq=n_seq, scale=0.125, key_keep=keep.to(dev) if masked else None)
        return [t for t in (x, w, b, keep) if t is not None], [out, part]
    return run


def _mx_case(kernel, n_seq, mx_out=False, bias=True, ld=None):
    def run(dev):
        from synchformer_amd import ops
        x, w, b = _mx_inputs(kernel, n_seq)
        b = b if bias else None
        rows = n_seq * L
        bd = b.to(dev) if bias else None
        xq, xs = torch.empty(rows, D, device=dev, dtype=torch.uint8), ops.mx_scale_planes(rows, D, dev)
        wq, ws = torch.empty(3 * D, D, device=dev, dtype=torch.uint8), ops.mx_scale_planes(3 * D, D, dev)
        ops.quantize_mxfp8(x.to(dev), xq, xs)
        ops.quantize_mxfp8(w.to(dev), wq, ws)
        sq, ss = torch.zeros(n_seq * 33, D, device=dev, dtype=torch.uint8), ops.mx_scale_planes(n_seq * 33, D, dev)
        ops.space_side_rows_mx(xq, xs, sq, ss, n_seq)
        side = torch.empty(n_seq * 33, 3 * D, device=dev, dtype=torch.bfloat16)
        ops.gemm_mxfp8(sq, ss, wq, ws, bd, side)
        if ld:
            xq, wq = _strided(xq, ld), _strided(wq, ld)
        part = torch.zeros(n_seq * 12 * _n_part(kernel) * 66, device=dev)
        fn = ops.qkv_space_attention_mx if kernel == 'space' else ops.qkv_time_attention2_mx
        if mx_out:
            out, out_s = torch.full((rows, D), int(FILL), device=dev, dtype=torch.uint8), ops.mx_scale_planes(rows, D, dev)
            fn(xq, xs, wq, ws, bd, side, out, part, n_seq=n_seq, scale=0.125, out_scales=out_s)
            outs = [out, out_s, part]
        else:
            out = torch.full((rows, D), FILL, device=dev, dtype=torch.bfloat16)
            fn(xq, xs, wq, ws, bd, side, out, part, n_seq=n_seq, scale=0.125)
            outs = [out, part]
        return [t for t in (x, w, b) if t is not None], outs
    return run


# name -> run(device) -> (the inputs as generated on the CPU, the tensors the launch wrote, on the device)
CASES = {}
for _k in ('space', 'time2'):
    # n_seq = 1: fewer work items than workgroups (time: 9 row tiles over 8 XCDs, XCDs 5-7 own nothing); n_seq = 7: 42 | 48 items per XCD against 32 workgroups - some
    # run a second item: the unit rotation, the re-derived lane offsets, and in the time kernel a left-over item followed by a main item
    for _n in (1, 7):
        CASES[f'{_k}_n{_n}'] = _bf16_case(_k, _n)
        CASES[f'{_k}_masked_n{_n}'] = _bf16_case(_k, _n, masked=True)
        CASES[f'{_k}_mx_n{_n}'] = _mx_case(_k, _n)
        CASES[f'{_k}_mx_mxout_n{_n}'] = _mx_case(_k, _n, mx_out=True)
    CASES[f'{_k}_nobias_n1'] = _bf16_case(_k, 1, bias=False)
    CASES[f'{_k}_mx_nobias_n1'] = _mx_case(_k, 1, bias=False)
    CASES[f'{_k}_ld832_n1'] = _bf16_case(_k, 1, ld=832)                  # the lane offsets of the LDS-DMA pieces depend on the row strides
    CASES[f'{_k}_mx_ld896_n1'] = _mx_case(_k, 1, ld=896)


def record(dev):
    cases = {}
    for name, run in CASES.items():
        src, out = run(dev)
        torch.cuda.synchronize()
        cases[name] = dict(input=sha256(*src), output=sha256(*out))
        print(f'{name}: input {cases[name]["input"]}  output {cases[name]["output"]}', flush=True)
    return cases


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--commit', required=True, help='the commit the library under record was built from')
    ap.add_argument('--out', type=Path, default=OUT)
    args = ap.parse_args()
    from synchformer_amd import _lib
    print(f'recording from {_lib.lib_path()}')
    dev = torch.device('cuda:0')
    first, second = record(dev), record(dev)
    differ = [n for n in first if first[n] != second[n]]
    assert not differ, f'two recordings differ: {differ}'
    args.out.write_text(json.dumps(dict(recorded_from=args.commit, cases=first), indent=1) + '\n')
    print(f'wrote {args.out}')


if __name__ == '__main__':
    import sys
    sys.path.insert(0, str(HERE.parent.parent))
    main()
