"""Audio programmes, measured: the kernel on its own, and the feature against what it replaces.  Prints JSON lines.

    python tools/bench_programmes.py kernel [--seconds 60] [--windows 5] [--calls 20]
    python tools/bench_programmes.py feature --side {A,B} [--tree PATH] [--seconds 60] [--size 1080x1920] [--windows 5] [--calls 3] [--programmes 1,2,4,8]

kernel   sf_resample_wave_mix on --seconds of 16-channel 48 kHz, P = 1, 4, 8, planar and interleaved, s16 and s32 (12 cases; fp32 is left out: the feeds carry
         PCM), and sf_resample_wave beside it on the 8-channel planar case it can take.  Per case: windows of --calls back-to-back calls between device events;
         milliseconds per call, input + output bytes per second.
feature  --seconds of uyvy422 at 30000/1001 with an 8-channel 48 kHz int16 wave in device memory.  Side A is what a user does without the feature: track_raw once
         per programme, each on the programme's pre-selected channels (planar, selected outside the timed region) - it uses only entry points the parent commit has,
         so `--tree PATH` can point it at a checkout of the parent with its own build.  Side B is one track_raw_programmes call on the interleaved wave.  Per P:
         windows of --calls calls between device synchronisations; seconds per call."""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

PROGRAMMES = [(0, 1), (2, 3), (4, 5), (6, 7), 0, 2, 4, 6]                         # of 8 channels: four stereo pairs, then four single channels


def events_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def kernel(args):
    from synchformer_amd import ops
    from synchformer_amd.ingest import RecordingIngest
    dev = torch.device('cuda:0')
    ing = RecordingIngest(dev, 25, (256, 256), 48000)
    n = int(args.seconds * 48000)
    gen = torch.Generator().manual_seed(3)
    x16 = torch.randint(-32768, 32768, (16, n), generator=gen, dtype=torch.int32).to(torch.int16).to(dev)
    inputs = {('s16', 'planar'): x16, ('s16', 'interleaved'): x16.t().contiguous(), ('s32', 'planar'): x16.to(torch.int32) << 16}
    inputs[('s32', 'interleaved')] = inputs[('s32', 'planar')].t().contiguous()
    mix = torch.rand(8, 16, generator=gen).to(dev) / 16
    n_out = ing.n_samples(n)

    def run(name, fn, nbytes):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = sorted(events_ms(fn, args.calls) for _ in range(args.windows))
        print(json.dumps({'tool': 'bench_programmes', 'mode': 'kernel', 'case': name, 'ms_min': round(ms[0], 4), 'ms_median': round(ms[len(ms) // 2], 4),
                          'ms_max': round(ms[-1], 4), 'bytes': nbytes, 'GBps_median': round(nbytes / ms[len(ms) // 2] / 1e6, 1)}), flush=True)

    x8 = x16[:8].contiguous()
    run('sf_resample_wave s16 planar 8ch -> mono', lambda: ops.resample_wave(x8, ing.kernel, ing.o, ing.width), 8 * n * 2 + n_out * 4)
    run('sf_resample_wave_mix s16 planar 8ch P=1', lambda: ops.resample_wave_mix(x8, mix[:1, :8].contiguous(), ing.kernel, ing.o, ing.width), 8 * n * 2 + n_out * 4)
    for (fmt, layout), x in inputs.items():
        for P in (1, 4, 8):
            m = mix[:P].contiguous()
            run(f'sf_resample_wave_mix {fmt} {layout} 16ch P={P}', lambda: ops.resample_wave_mix(x, m, ing.kernel, ing.o, ing.width, layout == 'interleaved'),
                x.numel() * x.element_size() + P * n_out * 4)


def feature(args):
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.ingest import RecordingIngest
    from synchformer_amd.track import OffsetTracker
    dev = torch.device('cuda:0')
    H, W = (int(v) for v in args.size.lower().split('x'))
    fps = (30000, 1001)
    T_raw, n_raw = int(args.seconds * 30000 / 1001), int(args.seconds * 48000)
    eng = SynchformerEngine(synth.make_state_dict(1337), dev)
    tracker = OffsetTracker(eng, MelFrontend(dev))
    raw = torch.randint(0, 256, (T_raw, H, W, 2), generator=torch.Generator(device=dev).manual_seed(7), dtype=torch.uint8, device=dev)
    wave = torch.stack([synth.make_wave(1, 1, 300 + c, n=n_raw).reshape(n_raw) for c in range(8)])
    wave = (wave / wave.abs().max() * 30000).round().to(torch.int16)            # (8, n) planar; the feed's own layout is its transpose
    for P in (int(v) for v in args.programmes.split(',')):
        progs = PROGRAMMES[:P]
        if args.side == 'A':
            ing = RecordingIngest(dev, fps, (H, W), 48000, pix_fmt='uyvy422')
            sel = [wave[[p] if isinstance(p, int) else list(p)].contiguous().to(dev) for p in progs]
            fn = lambda: [tracker.track_raw(raw, s, ing) for s in sel]          # noqa: E731
        else:
            ing = RecordingIngest(dev, fps, (H, W), 48000, pix_fmt='uyvy422', audio_channels=8, audio_interleaved=True, programmes=progs)
            wil = wave.t().contiguous().to(dev)
            fn = lambda: tracker.track_raw_programmes(raw, wil, ing)            # noqa: E731
        tracks = fn()
        torch.cuda.synchronize()
        secs = []
        for _ in range(args.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            secs.append((time.perf_counter() - t0) / args.calls)
        digest = [round(float(t.logits.double().sum().item()), 4) for t in tracks]
        print(json.dumps({'tool': 'bench_programmes', 'mode': 'feature', 'side': args.side, 'P': P, 'windows': int(tracks[0].logits.shape[0]),
                          'segments': tracks[0].n_segments, 's_per_call': [round(s, 5) for s in secs], 's_median': round(sorted(secs)[len(secs) // 2], 5),
                          'logit_sums': digest}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'feature'])
    ap.add_argument('--side', choices=['A', 'B'], default='B')
    ap.add_argument('--tree', default=None, help='import synchformer_amd from this checkout (side A: the parent commit with its own build)')
    ap.add_argument('--seconds', type=float, default=60.0)
    ap.add_argument('--size', default='1080x1920')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--calls', type=int, default=None)
    ap.add_argument('--programmes', default='1,2,4,8')
    args = ap.parse_args()
    args.calls = args.calls or (20 if args.mode == 'kernel' else 3)
    root = Path(args.tree).resolve() if args.tree else Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root))
    (kernel if args.mode == 'kernel' else feature)(args)


if __name__ == '__main__':
    main()
