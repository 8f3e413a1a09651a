"""A few launches of ONE of the six fused qkv + attention kernels (csrc/sf_qkv_space.hip, csrc/sf_qkv_time2.hip on the main loop of csrc/sf_qkv_tile.h) at the model's
size, on the tensors of tools/bench_qkv_space.py / bench_qkv_time2.py - for a kernel trace, not for host timing (run on the GPU box):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/time_qkv_fused.py {space|time2}[_masked|_mx] [n_segments] [launches]

SYNCHFORMER_HIP_LIB selects another build of the library (profiles/qkv_tile_refactor.md: the parent's and the new one alternating)."""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from synchformer_amd import ops

dev = torch.device('cuda:0')


def main():
    which = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 224
    launches = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    kernel, _, form = which.partition('_')
    assert kernel in ('space', 'time2') and form in ('', 'masked', 'mx'), which
    L, D = 1569, 768
    rows = n * L
    x = torch.randn(rows, D, device=dev).bfloat16()
    w = (torch.randn(3 * D, D, device=dev) * 0.05).bfloat16()
    b = torch.randn(3 * D, device=dev) * 0.1
    out = torch.empty(rows, D, device=dev, dtype=torch.bfloat16)
    part = torch.empty(n * 12 * (8 if kernel == 'space' else 33) * 66, device=dev)
    side = torch.empty(n * 33, 3 * D, device=dev, dtype=torch.bfloat16)
    if form == 'mx':
        xq, xs = torch.empty(rows, D, device=dev, dtype=torch.uint8), ops.mx_scale_planes(rows, D, dev)
        wq, ws = torch.empty(3 * D, D, device=dev, dtype=torch.uint8), ops.mx_scale_planes(3 * D, D, dev)
        ops.quantize_mxfp8(x, xq, xs)
        ops.quantize_mxfp8(w, wq, ws)
        sq, ss = torch.zeros(n * 33, D, device=dev, dtype=torch.uint8), ops.mx_scale_planes(n * 33, D, dev)
        ops.space_side_rows_mx(xq, xs, sq, ss, n)
        ops.gemm_mxfp8(sq, ss, wq, ws, b, side)
        fn = ops.qkv_space_attention_mx if kernel == 'space' else ops.qkv_time_attention2_mx
        launch = lambda: fn(xq, xs, wq, ws, b, side, out, part, n_seq=n, scale=0.125)
    else:
        side_in = torch.empty(n * 33, D, device=dev, dtype=torch.bfloat16)
        ops.space_side_rows(x, side_in, n)
        ops.gemm(side_in, w, b, side)
        keep = (torch.rand(rows, device=dev) > 0.3).to(torch.uint8) if form == 'masked' else None
        fn = ops.qkv_space_attention if kernel == 'space' else ops.qkv_time_attention2
        launch = lambda: fn(x, w, b, side, out, part, n_seq=n, scale=0.125, key_keep=keep)
    torch.cuda.synchronize()
    for _ in range(launches):
        launch()
    torch.cuda.synchronize()
    print(f'{which}: {launches} launches at {n} segments')


if __name__ == '__main__':
    main()
