"""Offset tracking along a synthetic recording: the bank path (every segment through the towers once, windows as row-map views of the bank)
beside the same windows through forward_clips on explicit 120-frame slices.  Prints one JSON line.

    python tools/track_recording.py [--seconds 60] [--hop 1] [--seg-chunk 224] [--host] [--clip-windows 8]

forward_clips is timed on at most --clip-windows windows (spread over the recording) and scaled to all W; both sides include the mel front-end and
are timed by wall clock around a device synchronisation, after one warm-up pass each.  Synthetic weights and inputs: the numbers are throughput only."""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=60.0)
    ap.add_argument('--hop', type=int, default=1)
    ap.add_argument('--seg-chunk', type=int, default=224)
    ap.add_argument('--win-chunk', type=int, default=256)
    ap.add_argument('--clip-windows', type=int, default=8, help='windows timed through forward_clips (scaled to all of them)')
    ap.add_argument('--host', action='store_true', help='keep the recording in pinned host memory (uploaded chunk by chunk)')
    args = ap.parse_args()
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend, recording_geometry
    from synchformer_amd.track import OffsetTracker
    dev = torch.device('cuda:0')
    T, n = int(args.seconds * 25), int(args.seconds * 16000)
    g = recording_geometry(T, n, args.hop)
    N, W = g['n_segments'], g['n_windows']
    if W < 1:
        raise SystemExit(f'{args.seconds} s hold {N} segments: below one window')
    eng = SynchformerEngine(synth.make_state_dict(1337), dev, seg_chunk=args.seg_chunk)
    mel = MelFrontend(dev)
    gen = torch.Generator().manual_seed(7)
    frames = torch.randint(0, 256, (T, 3, 224, 224), generator=gen, dtype=torch.uint8)
    wave = torch.rand(n, generator=gen) * 2 - 1
    fd, wd = frames.to(dev), wave.to(dev)
    src = (frames.pin_memory(), wave.pin_memory()) if args.host else (fd, wd)
    tracker = OffsetTracker(eng, mel, hop_segments=args.hop)

    def timed(fn, reps=1):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, out

    t_bank, (vbank, abank) = timed(lambda: eng.extract_recording(*src, mel))
    t_win, track = timed(lambda: tracker.track_features(vbank, abank, win_chunk=args.win_chunk), reps=3)
    k = min(W, max(1, args.clip_windows))
    picks = [round(i * (W - 1) / max(1, k - 1)) for i in range(k)]

    def clips():
        return torch.stack([eng.forward_clips(fd[None, 8 * args.hop * w:8 * args.hop * w + 120], wd[None, 5120 * args.hop * w:5120 * args.hop * w + 76800], mel)[0]
                            for w in picks])

    t_clips, ref = timed(clips)
    t_clips_all = t_clips * W / k
    err = (track.logits[picks] - ref).abs().max().item()
    print(json.dumps({
        'tool': 'track_recording', 'seconds': args.seconds, 'hop_segments': args.hop, 'segments': N, 'windows': W, 'host_input': bool(args.host),
        'seg_chunk': args.seg_chunk, 'bank_s': round(t_bank, 4), 'segments_per_s': round(N / t_bank, 1), 'windows_s': round(t_win, 5),
        'windows_per_s': round(W / t_win, 1), 'track_total_s': round(t_bank + t_win, 4),
        'forward_clips_windows_timed': k, 'forward_clips_s_scaled': round(t_clips_all, 3), 'speedup_vs_forward_clips': round(t_clips_all / (t_bank + t_win), 2),
        'max_abs_logit_diff_vs_forward_clips': round(err, 6), 'path_changes': int((track.cls_path[1:] != track.cls_path[:-1]).sum().item()),
        'raw_changes': int((track.cls_raw[1:] != track.cls_raw[:-1]).sum().item())}))


if __name__ == '__main__':
    main()
