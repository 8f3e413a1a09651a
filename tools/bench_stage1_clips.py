"""Stage-1 (AVCLIP) train step from raw clips (synchformer_amd.augment.Stage1Sampler): what the device-side augmentations cost.

    python tools/bench_stage1_clips.py [--clips 2] [--steps 10] [--warmup 3] [--repeats 3] [--out FILE.json]

At 2 clips x 14 segments (configs/segment_avclip.yaml geometry), 10 s 256 x 256 uint8 clips + 16 kHz waves already in HBM, `--repeats` times in turn
(every figure is reported as the list of its repeats, so the run-to-run spread is in the output):
  * step_clips_config_ms:  AVCLIPTrainer.train_step_clips with decisions drawn at the config's rates (upscale 0.2, colour jitter 0.2, gray 0.2, flip 0.5,
    audio augs 0.2 each), a ring of 8 pre-drawn batches;
  * step_clips_all_on_ms:  the same with every augmentation forced on in every segment (the worst case: upscale, jitter, gray, flip, volume, lowpass, noise);
  * step_materialised_ms:  train_step (forward, backward, optimizer - the whole step, as the two legs above) on materialised (B, 14, 16, 3, 224, 224)
    uint8 segments and finished log-mels - the same work minus the new launches;
  * fb_clips_config_ms / fb_materialised_ms: forward_backward_clips at the config's rates against forward_backward on the materialised inputs (no
    optimizer step: the same difference over a shorter base);
  * video_*_us / audio_*_us: HIP-event times of the two new entry points alone (sf_stage1_video_augment = the frame-mean launch + the augment launch,
    sf_stage1_audio_augment = the gather launch + the lowpass launch) with everything off, at the config's rates and with everything on.
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
    ap.add_argument('--clips', type=int, default=2)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--side', type=int, default=256)
    ap.add_argument('--seed', type=int, default=3, help='of the decisions; 3 puts the ring of 8 batches next to the configured rates (its counts are in the output)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from synchformer_amd import ops, synth
    from synchformer_amd.augment import Stage1Sampler
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.stage1 import AVCLIPTrainer
    dev = torch.device('cuda:0')
    B, S, side, T, NS = args.clips, 14, args.side, 250, 160000
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (B, T, 3, side, side), dtype=torch.uint8, generator=g).to(dev)
    wave = (torch.randn(B, NS, generator=g) * 0.1).to(dev)
    rng, gen = random.Random(args.seed), torch.Generator().manual_seed(args.seed)
    draw = lambda sampler: sampler.sample(rng, [T] * B, [NS] * B, side, side, gen).to(dev)
    ring = [draw(Stage1Sampler()) for _ in range(8)]
    all_on = [draw(Stage1Sampler(sometimes_p=1, p_color_jitter=1, p_gray_scale=1, p_flip=1, p_audio_aug=1)) for _ in range(8)]
    all_off = [draw(Stage1Sampler(sometimes_p=0, p_color_jitter=0, p_gray_scale=0, p_flip=0, p_audio_aug=0)) for _ in range(8)]
    mel = MelFrontend(dev)
    sd = {k: v for k, v in synth.make_state_dict(1337).items() if k.startswith(('vfeat_extractor.', 'afeat_extractor.'))}
    tr = AVCLIPTrainer(sd, dev, lr=1e-4)
    out = {'clips': B, 'segments': S, 'side': side, 'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats}
    vis, aud = (t.clone() for t in tr.augment_clips(frames, wave, mel, ring[0]))
    seg = torch.empty(B * S, 16, 3, 224, 224, dtype=torch.uint8, device=dev)
    sums = torch.empty(B * S * 16, dtype=torch.int32, device=dev)
    seg_wave = torch.empty(B * S, 10240, dtype=torch.float32, device=dev)
    it = [0]

    def nxt(batches):
        it[0] += 1
        return batches[it[0] % len(batches)]

    def video(batches):
        b = nxt(batches)
        ops.stage1_video_augment(frames, b.clip_table, b.seg_table, seg, sums, b.v_stride, S)

    def audio(batches):
        b = nxt(batches)
        ops.stage1_audio_augment(wave, b.clip_table, b.seg_table, seg_wave, b.a_stride, S, b.lowpass, b.noise_amp)

    legs = {
        'step_materialised_ms': (lambda: tr.train_step(vis, aud), args.steps, args.warmup, 1.0),
        'step_clips_config_ms': (lambda: tr.train_step_clips(frames, wave, mel, nxt(ring)), args.steps, args.warmup, 1.0),
        'step_clips_all_on_ms': (lambda: tr.train_step_clips(frames, wave, mel, nxt(all_on)), args.steps, args.warmup, 1.0),
        'fb_materialised_ms': (lambda: tr.forward_backward(vis, aud), args.steps, args.warmup, 1.0),
        'fb_clips_config_ms': (lambda: tr.forward_backward_clips(frames, wave, mel, nxt(ring)), args.steps, args.warmup, 1.0),
        'video_off_us': (lambda: video(all_off), 40, 8, 1e3), 'video_config_us': (lambda: video(ring), 40, 8, 1e3),
        'video_all_on_us': (lambda: video(all_on), 40, 8, 1e3),
        'audio_off_us': (lambda: audio(all_off), 40, 8, 1e3), 'audio_config_us': (lambda: audio(ring), 40, 8, 1e3),
        'audio_all_on_us': (lambda: audio(all_on), 40, 8, 1e3),
    }
    for k in legs:
        out[k] = []
    for _ in range(args.repeats):                                     # the legs in turn, so a drift of the box hits all of them alike
        for k, (fn, steps, warmup, scale) in legs.items():
            out[k].append(round(scale * _time(fn, steps, warmup), 3))
    out['jittered_segments_in_ring'] = [int(b.seg_table[:, 0].sum()) for b in ring]
    out['upscaled_clips_in_ring'] = [int((b.clip_table[:, 3] == 192).sum()) for b in ring]
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
