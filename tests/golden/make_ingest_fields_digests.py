"""Fixture of test_ingest_fields_gpu.py::test_field_outputs_are_pinned: the SHA-256 of what the field kernels of csrc/sf_ingest.hip write for cases of
the oracle test (the pixel test allows one level against float64 and would not see a changed summation order or a changed address inside a constant region).

    python tests/golden/make_ingest_fields_digests.py --commit $(git rev-parse HEAD)        # needs the GPU; writes tests/golden/ingest_fields_digests.json

The inputs are those of test_fields_match_oracle (ingest_fields_oracle.rgb_frames / yuv_planes, from CPU generators); each input's own digest is stored too, so that a
change of the random stream shows as an input mismatch and not as a kernel regression.  The file is recorded ONCE, on the commit it names, after those cases pass the
oracle; a digest that differs later means the arithmetic or the addressing changed."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent.parent)]
import ingest_fields_oracle as F  # noqa: E402

OUT = HERE / 'ingest_fields_digests.json'


def sha256(t: torch.Tensor) -> str:
    return hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def ingest(dev, H, W, pix_fmt, order, channels_last=False):
    """The RecordingIngest of a GPU case: the colour setting of ingest_fields_oracle.CASES, the field pick [0, 1, 1, 4, 7] over 4 frames."""
    from synchformer_amd.ingest import RecordingIngest
    cs, full, loc, _, _ = F.CASES[(H, W)]
    kw = dict(channels_last=channels_last) if pix_fmt == 'rgb24' else dict(pix_fmt=pix_fmt, colorspace=cs, full_range=full, chroma_loc=loc)
    ing = RecordingIngest(dev, 25, (H, W), 16000, field_order=order, **kw)
    ing._tables = {4: torch.tensor(F.TABLE, dtype=torch.int32)}
    return ing


def raw_frames(H, W, pix_fmt, channels_last=False):
    """The raw frames of a GPU case on the host."""
    if pix_fmt == 'rgb24':
        raw = F.rgb_frames(H, W)
        return raw.permute(0, 2, 3, 1).contiguous() if channels_last else raw
    return F.pack(F.yuv_planes(H, W, 10 if pix_fmt in F.FMTS_16 else 8), pix_fmt)


def _case(H, W, pix_fmt, order, channels_last=False):
    def run(dev):
        raw = raw_frames(H, W, pix_fmt, channels_last)
        return raw, ingest(dev, H, W, pix_fmt, order, channels_last).frames(raw.to(dev), 0, len(F.TABLE))
    return run


# name -> run(device) -> (the input as generated on the CPU, the uint8 output on the device)
CASES = {
    'rgb_planar_270x480_tff': _case(270, 480, 'rgb24', 'tff'),                     # 5 vertical taps on a field of 135 rows
    'rgb_channels_last_480x202_bff': _case(480, 202, 'rgb24', 'bff', True),        # column stride 3, portrait, the other order
    'uyvy422_270x480_tff': _case(270, 480, 'uyvy422', 'tff'),                      # packed 8-bit: dword loads on both parities
    'yuyv422_480x202_bff': _case(480, 202, 'yuyv422', 'bff'),                      # chroma width 101: row ends on the strided loads
    'yuv422p_480x202_tff': _case(480, 202, 'yuv422p', 'tff'),                      # planar chroma rows of 101 bytes: every other field row unaligned
    'nv16_270x480_bff': _case(270, 480, 'nv16', 'bff'),                            # the interleaved chroma fetch
    'yuv422p10le_270x480_tff': _case(270, 480, 'yuv422p10le', 'tff'),
    'p210_480x202_bff': _case(480, 202, 'p210', 'bff'),
    'y210_270x480_bff': _case(270, 480, 'y210', 'bff'),                            # packed 16-bit
    'uyvy422_1080x1920_tff': _case(1080, 1920, 'uyvy422', 'tff'),                  # 11-tap field filter, wide-row chunks
    'y210_1080x1920_bff': _case(1080, 1920, 'y210', 'bff'),                        # the halved staging of the packed 16-bit form
}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--commit', required=True, help='the commit the library under record was built from')
    ap.add_argument('--out', type=Path, default=OUT)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    cases = {}
    for name, run in CASES.items():
        src, out = run(dev)
        torch.cuda.synchronize()
        assert out.dtype == torch.uint8 and out.shape == (len(F.TABLE), 3, 224, 224), (name, out.dtype, out.shape)
        cases[name] = dict(input=sha256(src), output=sha256(out))
        print(f'{name}: input {tuple(src.shape)} {cases[name]["input"]}  output {tuple(out.shape)} {cases[name]["output"]}', flush=True)
    args.out.write_text(json.dumps(dict(recorded_from=args.commit, cases=cases), indent=1) + '\n')
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
