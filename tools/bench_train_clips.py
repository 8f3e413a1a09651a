"""Stage-2 train step from raw clips (synchformer_amd.augment): what the device-side crop / flip / offset front-end costs.

    python tools/bench_train_clips.py [--clips 16] [--steps 10] [--warmup 3] [--out FILE.json]

Three numbers at 16 clips x 14 segments (configs/sync.yaml geometry, dropout 0.1 as in bench.py --workload train):
  * step_hbm_ms:        SyncTrainer.train_step_clips from raw 10 s 256 x 256 uint8 clips + 16 kHz waves already in HBM, against
    step_presegmented_ms: MelFrontend on the materialised waveform segments + train_step on pre-segmented (B, 14, 16, 3, 224, 224) uint8 inputs -
    the same work minus the crop path;
  * step_pinned_ms:     the same step fed from PINNED host memory through ClipTrainPipeline (trimmed windows: 120 frames of 256 x 256 + 76,800
    samples per clip cross PCIe, under the previous step);
  * im2col_crops_us / im2col_tokens_us: sf_im2col_video_crops against sf_im2col_video_tokens over the same 224 segments, by HIP events.
Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import random
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--clips', type=int, default=16)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--side', type=int, default=256)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from synchformer_amd import ops, synth
    from synchformer_amd.augment import ClipSampler, ClipTrainPipeline
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.train import SyncTrainer
    dev = torch.device('cuda:0')
    B, S, side, T, NS = args.clips, 14, args.side, 250, 160000
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (B, T, 3, side, side), dtype=torch.uint8, generator=g)
    wave = torch.randn(B, NS, generator=g) * 0.1
    sampler = ClipSampler('grid')
    batch = sampler.sample(random.Random(0), [T] * B, [NS] * B, side, side, torch.Generator().manual_seed(0))
    fw, ww, rel = batch.trim(frames, wave)
    mel = MelFrontend(dev)
    tr = SyncTrainer(synth.make_state_dict(1337), dev, embd_pdrop=0.1, resid_pdrop=0.1, attn_pdrop=0.1, seed=1337)
    out = {'clips': B, 'segments': S, 'side': side, 'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup}

    # (1) raw clips in HBM vs pre-segmented inputs
    f_d, w_d, b_d = frames.to(dev), wave.to(dev), batch.to(dev)
    tb = batch.table
    vis = torch.stack([torch.stack([frames[b, f0 + s * 8:f0 + s * 8 + 16, :, y0:y0 + 224, x0:x0 + 224] for s in range(S)]).flip(-1) if fl else
                       torch.stack([frames[b, f0 + s * 8:f0 + s * 8 + 16, :, y0:y0 + 224, x0:x0 + 224] for s in range(S)])
                       for b, (f0, y0, x0, fl) in enumerate(tb.tolist())]).contiguous().to(dev)
    segs = torch.stack([torch.stack([wave[b, a + s * 5120:a + s * 5120 + 10240] for s in range(S)]) for b, a in enumerate(batch.sample0.tolist())]).to(dev)
    out['step_presegmented_ms'] = _time(lambda: tr.train_step(vis, mel(segs), b_d.targets), args.steps, args.warmup)
    out['step_hbm_ms'] = _time(lambda: tr.train_step_clips(f_d, w_d, mel, b_d), args.steps, args.warmup)
    del vis, segs, f_d, w_d

    # (2) pinned host memory through the two-slot pipeline (the same pinned batch re-staged every step: the transfer is what is measured)
    f_pin, w_pin, r_pin = fw.pin_memory(), ww.pin_memory(), rel.pin_memory()
    pipe = ClipTrainPipeline(tr, mel, B, n_seg=S, H=side, W=side)
    pipe.stage(f_pin, w_pin, r_pin)
    out['step_pinned_ms'] = _time(lambda: pipe.step(f_pin, w_pin, r_pin), args.steps, args.warmup)
    pipe.step()
    out['h2d_mb_per_clip'] = round((fw[0].numel() + ww[0].numel() * 4) / 1e6, 2)

    # (3) the gather kernels alone, over the same B * S segments
    f_d = fw.to(dev)
    t_d = rel.table.to(dev)
    seg_in = torch.randint(0, 256, (B * S, 16, 3, 224, 224), dtype=torch.uint8, device=dev)
    patches = torch.empty(B * S * 1569, 1536, device=dev, dtype=torch.bfloat16)
    out['im2col_crops_us'] = 1e3 * _time(lambda: ops.im2col_video_crops(f_d, t_d, patches, 8, S), 20, 3)
    out['im2col_tokens_us'] = 1e3 * _time(lambda: ops.im2col_video_tokens(seg_in, patches), 20, 3)
    out['clips_per_s_hbm'] = B / out['step_hbm_ms'] * 1e3
    out['clips_per_s_pinned'] = B / out['step_pinned_ms'] * 1e3
    out['clips_per_s_presegmented'] = B / out['step_presegmented_ms'] * 1e3
    line = json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in out.items()})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
