"""Fixture of test_ingest_gpu.py::test_ingest_outputs_are_pinned: the SHA-256 of what ops.ingest_video / ops.ingest_video_yuv write for the smallest inputs that
reach every branch of the resize pipeline of csrc/sf_ingest.hip (the pixel tests allow one level against float64 and would not see a changed summation order).

    python tests/golden/make_ingest_digests.py --commit $(git rev-parse HEAD)        # needs the GPU; writes tests/golden/ingest_digests.json

Inputs come from CPU generators (ingest_oracle.random_frames, ingest_yuv_oracle.random_planes) under the seeds of the pixel tests; each input's own digest is
printed and stored too, so that a change of the random stream shows as an input mismatch and not as a kernel regression.  The file is recorded ONCE, on the commit
it names; a digest that differs later means the arithmetic or the addressing changed."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent.parent)]
import ingest_oracle as R  # noqa: E402
import ingest_yuv_oracle as Y  # noqa: E402

OUT = HERE / 'ingest_digests.json'


def sha256(t: torch.Tensor) -> str:
    return hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()


def _rgb(H, W, channels_last=False, side=256, window=False):
    """5 source frames through RecordingIngest's tables and the frame pick [0, 0, 2, 4, 4]; window: the frames sit at (2, 30) of a (H + 3, 517) buffer of 255."""
    def run(dev):
        from synchformer_amd import ops
        from synchformer_amd.ingest import RecordingIngest
        raw = R.random_frames(5, H, W, H * 10000 + W + side)
        ing = RecordingIngest(dev, 25, (H, W), 16000, channels_last=channels_last, resize_side=side)
        src = raw.permute(0, 2, 3, 1).contiguous() if channels_last else raw
        if window:
            buf = torch.full((5, 3, H + 3, 517), 255, dtype=torch.uint8)
            buf[:, :, 2:2 + H, 30:30 + W] = raw
            src = buf.to(dev)[:, :, 2:2 + H, 30:30 + W]
        pick = torch.tensor(R.TABLE, dtype=torch.int32, device=dev)
        return raw, ops.ingest_video(src.to(dev), channels_last, pick, ing.y_first, ing.y_w, ing.x_first, ing.x_w)
    return run


def _tables(dev, H, W, Wr):
    """The anisotropic resize to 256 x Wr, sliced to the centre crop: [y_first, y_w, x_first, x_w] on the device."""
    from synchformer_amd.ingest import aa_bicubic_table
    x0 = (Wr - 224) // 2
    yf, yw, _ = aa_bicubic_table(H, 256)
    xf, xw, _ = aa_bicubic_table(W, Wr)
    return [t.contiguous().to(dev) for t in (yf[16:240], yw[16:240], xf[x0:x0 + 224], xw[x0:x0 + 224])]


def _rgb_taps(H, W, Wr):
    """3 source frames, the pick [2, 0, 1], through ops.ingest_video with its own tables (test_ingest_video_many_taps)."""
    def run(dev):
        from synchformer_amd import ops
        raw = R.random_frames(3, H, W, H + W)
        pick = torch.tensor([2, 0, 1], dtype=torch.int32, device=dev)
        return raw, ops.ingest_video(raw.to(dev), False, pick, *_tables(dev, H, W, Wr))
    return run


def _yuv(H, W, pix_fmt, pitch=None):
    """5 source frames in the colour setting of ingest_yuv_oracle.CASES, the frame pick [0, 0, 2, 4, 4]; pitch: the NV12 frames sit in rows of `pitch` bytes."""
    def run(dev):
        from synchformer_amd import ops
        from synchformer_amd.ingest import RecordingIngest
        cs, full, _, _ = Y.CASES[(H, W)]
        raw = Y.pack(*Y.random_planes(5, H, W, H * 10000 + W + 256), pix_fmt)
        ing = RecordingIngest(dev, 25, (H, W), 16000, pix_fmt=pix_fmt, colorspace=cs, full_range=full)
        src = raw.to(dev)
        if pitch:
            buf = torch.full((5, H * 3 // 2, pitch), 255, dtype=torch.uint8)
            buf[:, :, :W] = raw
            src = buf.to(dev)[:, :, :W]
        pick = torch.tensor(R.TABLE, dtype=torch.int32, device=dev)
        return raw, ops.ingest_video_yuv(src, pix_fmt, pick, ing.y_first, ing.y_w, ing.x_first, ing.x_w, ing.cy_first, ing.cy_w, ing.cx_first, ing.cx_w, ing.csc)
    return run


def _yuv_taps(H, W, pix_fmt):
    """2 source frames, the pick [1, 0], to 256 x 256 through ops.ingest_video_yuv with its own tables (test_yuv_many_taps)."""
    def run(dev):
        from synchformer_amd import ops
        from synchformer_amd.ingest import csc_matrix
        raw = Y.pack(*Y.random_planes(2, H, W, H + W), pix_fmt)
        M, off = csc_matrix('bt601', False)
        pick = torch.tensor([1, 0], dtype=torch.int32, device=dev)
        return raw, ops.ingest_video_yuv(raw.to(dev), pix_fmt, pick, *_tables(dev, H, W, 256), *_tables(dev, H // 2, W // 2, 256), torch.cat([M.reshape(9), off]).float())
    return run


# name -> run(device) -> (the input bytes as generated on the CPU, the uint8 output on the device)
CASES = {
    'rgb_planar_144x176': _rgb(144, 176),                                         # upscale, 5 taps, rows narrower than one staging sweep
    'rgb_planar_301x517': _rgb(301, 517),                                         # odd width: the dword and the byte path of the staging mix
    'rgb_channels_last_360x202': _rgb(360, 202, channels_last=True),              # column stride 3, portrait
    'rgb_window_270x480_in_517': _rgb(270, 480, window=True),                     # row and frame strides, unaligned row starts
    'rgb_planar_2160x260_to_256x256': _rgb_taps(2160, 260, 256),                  # 35 vertical taps, 13 chunks per tile
    'rgb_planar_260x3400_to_256x400': _rgb_taps(260, 3400, 400),                  # 35 horizontal taps, chunks of 4 rows
    'rgb_planar_270x480_side224': _rgb(270, 480, side=224),                       # filter rows clamped at the picture's edge
    'nv12_270x480': _yuv(270, 480, 'nv12'),                                       # bt601 limited; the interleaved chroma fetch
    'yuv420p_270x480': _yuv(270, 480, 'yuv420p'),                                 # the U plane ends in the middle of a row
    'nv12_360x202': _yuv(360, 202, 'nv12'),                                       # bt709 full; chroma width 101: unaligned chroma rows, byte path
    'yuv420p_360x202': _yuv(360, 202, 'yuv420p'),
    'nv12_270x480_pitch512': _yuv(270, 480, 'nv12', pitch=512),                   # a pitched surface read in place
    'nv12_2160x260_to_256x256': _yuv_taps(2160, 260, 'nv12'),                     # 35 / 19 taps
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
        assert out.dtype == torch.uint8 and out.shape[1:] == (3, 224, 224), (name, out.dtype, out.shape)
        cases[name] = dict(input=sha256(src), output=sha256(out))
        print(f'{name}: input {tuple(src.shape)} {cases[name]["input"]}  output {tuple(out.shape)} {cases[name]["output"]}', flush=True)
    args.out.write_text(json.dumps(dict(recorded_from=args.commit, cases=cases), indent=1) + '\n')
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
