"""Offset tracking along a synthetic recording: the bank path (every segment through the towers once, windows as row-map views of the bank)
beside the same windows through forward_clips on explicit 120-frame slices.  Prints one JSON line.

    python tools/track_recording.py [--seconds 60] [--hop 1] [--seg-chunk 224] [--host] [--clip-windows 8] [--fps 30000/1001 --size 1080x1920 --rate 48000]
                                    [--pix-fmt {rgb24,nv12,yuv420p,p010,yuv420p10le,uyvy422,yuyv422,yuv422p,nv16,yuv422p10le,p210,y210,v210}]
                                    [--chroma-loc {center,left,topleft}] [--field-order {progressive,tff,bff}] [--posterior] [--pairwise]
                                    [--stream SECONDS [--lag N]] [--gate [--mu X]]
                                    [--audio-channels N [--audio-interleaved] [--sample-fmt {flt,s16,s32}] --programmes 0+1,2+3,4]

With --fps / --size / --rate the recording is synthesised RAW at that geometry (channels-last uint8 frames, stereo int16 PCM, in device memory) and goes through
the ingest stage: the line then also carries the ingest time alone (the same chunks the bank asks for, plus the wave) and the bank from raw
frames next to the bank from frames ingested beforehand.  With --pix-fmt nv12 / yuv420p the raw frames are 8-bit YUV 4:2:0 in that layout: half
the bytes per frame, which the line reports next to the times (with --host they are what is uploaded).  With --pix-fmt p010 / yuv420p10le they are 10-bit
4:2:0 in 16-bit samples: the bytes of RGB again.  With a 4:2:2 layout the raw frames are (H, W, 2) for the packed uyvy422 / yuyv422
(uint8) and y210 (uint16), (2 H, W) for yuv422p / nv16 (uint8) and yuv422p10le / p210 (uint16): 2 H W bytes per frame in 8 bits, 4 H W in 16.  --chroma-loc sites the chroma samples of a YUV layout (tables only: no cost on the device).
With --pix-fmt v210 the raw frames are int32 (H, v210_row_words(W)): random words, 10-bit 4:2:2 at 128 ceil(W / 48) bytes per row (5120 at 1920).
With --field-order tff / bff the raw frames are interlaced (rgb24, the 4:2:2 layouts and v210): --fps stays the frame rate, every 25 fps frame is the one field
nearest its slot resized on its own, and the line reports the field order, the fields shown and the field's vertical taps (half the source rows are read).

With --posterior the windows are also read out as marginals: the line then carries the mean and minimum of conf_post, log_z per window step
(log_z / max(W - 1, 1)), the largest |offset_sec_mean - offset_sec_path| and the time of the two extra launches (the read-out alone, on the track's logits).

With --pairwise the boundaries between neighbouring windows are read out too (OffsetTracker(pairwise=True)): the line then carries
OffsetTrack.expected_changes(), OffsetTrack.changes() (time s, from s, to s, p_change, p_top per boundary with p_change >= 0.5) and the time of the two extra launches
(ops.track_pairwise alone, on the track's logits); with --gate also the gated track's expected changes of the offset and of the flag.

With --gate a synthetic 2-way syncability engine without towers (184 position rows: windows of 13 segments) reads the same bank and the windows are
read out over (offset class, synchronizable flag) at --mu: the line then carries, of this same run, the time of the offset windows and of the ungated read-out beside
the time of the gate's windows and of the gated read-out (with --posterior both read-outs include their posterior launches), what the gate adds to track_total_s, the
windows flagged not synchronizable, and the spans (start s, end s, offset s or null) of OffsetTrack.spans().  With --stream as well the recording is pushed a second
time through the gated stream (OffsetTracker.stream(lag, gated=True)): 'stream_gated' carries the same per-stage times plus the gate's windows, the
committed windows flagged not synchronizable, whether logits and gate_logits equal the offline track's, and what the gate adds per push beside 'stream' of this run.

With --lags A:B[:STEP] (written --lags=-12:12 when A is negative) the same bank is also read out over the audio lags A .. B (whole segments of 0.32 s: offsets beyond the +-2 s class grid) through
OffsetTracker.track_features_wide: 'wide' carries the lags, the states, the windows every lag shares, the time of the wide track beside the plain track's of this run
(and of its lagged windows alone), and the spans (start s, end s, offset s) of WideOffsetTrack.spans(), which are printed to stderr as well.

With --stream SECONDS the recording is also pushed through OffsetTracker.stream(lag) in pieces of that many seconds (from raw input when --fps /
--size / --rate are given): the line then carries, per push, the milliseconds of the bank (the towers on the segments the push completed), the windows (the sync
transformer on the windows it completed) and the read-out (ops.track_stream_push) - each timed by wall clock between device synchronisations, which a
production stream would not place - their sum over the recording against the offline track_total_s, and whether the streamed logits equal the offline ones.

With --programmes (implies the raw path) the wave has --audio-channels channels, every channel a differently seeded synth.make_wave so that the
programmes differ, planar (ch, n) or with --audio-interleaved (n, ch), as --sample-fmt flt (fp32), s16 or s32 (the s16 values << 16).  `0+1,2+3,4` are three
programmes: two averaged pairs and a single channel.  The recording goes through OffsetTracker.track_raw_programmes - the picture once, the audio tower once per
programme - and ONE JSON LINE PER PROGRAMME is printed: its channels, the time of the whole call and of P separate track_raw calls on the programme's channels
alone, whether the programme's logits equal that separate call's, and its path.  With --stream the recording is also pushed through the ProgrammeStream and each
line says whether the streamed logits equal the offline ones.  Nothing else of the tool runs in this mode.

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
    ap.add_argument('--fps', default=None, help='raw frame rate, e.g. 30, 29.97 or 30000/1001 (default: 25, no ingest)')
    ap.add_argument('--size', default=None, help='raw frame size HxW, e.g. 1080x1920')
    ap.add_argument('--rate', type=int, default=None, help='raw sample rate in Hz, e.g. 48000')
    ap.add_argument('--pix-fmt', choices=['rgb24', 'nv12', 'yuv420p', 'p010', 'yuv420p10le', 'uyvy422', 'yuyv422', 'yuv422p', 'nv16', 'yuv422p10le', 'p210', 'y210', 'v210'],
                    default=None, help='layout of the raw frames (default: rgb24, channels-last); 4:2:2: uyvy422 / yuyv422 / y210 frames are (H, W, 2), the others (2 H, W); v210: int32 (H, words per row)')
    ap.add_argument('--chroma-loc', choices=['center', 'left', 'topleft'], default='center', help='where the chroma samples of a YUV layout sit')
    ap.add_argument('--field-order', choices=['progressive', 'tff', 'bff'], default='progressive',
                    help='interlaced raw frames, top / bottom field first: the field nearest each 25 fps slot is ingested on its own (rgb24, 4:2:2 layouts and v210)')
    ap.add_argument('--posterior', action='store_true', help='also read the windows out as marginals (forward-backward)')
    ap.add_argument('--pairwise', action='store_true', help='also read out the boundaries between windows: change probabilities, expected number of changes')
    ap.add_argument('--stream', type=float, default=None, metavar='SECONDS', help='also push the recording through OffsetTracker.stream in pieces of this length')
    ap.add_argument('--lag', type=int, default=16, help='decision lag of the stream, in windows')
    ap.add_argument('--gate', action='store_true', help='also gate the track by a synthetic 2-way syncability engine (towers=False) on the same bank')
    ap.add_argument('--mu', type=float, default=2.0, help='cost of one change of the synchronizable flag (with --gate)')
    ap.add_argument('--lags', default=None, metavar='A:B[:STEP]', help='also read the bank out over the audio lags A .. B (segments of 0.32 s): offsets beyond +-2 s; write --lags=-12:12 when A is negative')
    ap.add_argument('--programmes', default=None, help="audio programmes of the wave's channels, e.g. 0+1,2+3,4: one offset track per programme against one pass of the picture")
    ap.add_argument('--audio-channels', type=int, default=None, help='channels of the raw wave (with --programmes; default: the highest channel named + 1)')
    ap.add_argument('--audio-interleaved', action='store_true', help='the raw wave is (n, ch), as a feed delivers it (with --programmes)')
    ap.add_argument('--sample-fmt', choices=['flt', 's16', 's32'], default='s16', help='sample type of the raw wave (with --programmes)')
    args = ap.parse_args()
    from synchformer_amd import ops, synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend, recording_geometry
    from synchformer_amd.ingest import PIX_FMTS_422, PIX_FMTS_422_16, PIX_FMTS_PACKED, PIX_FMTS_V210, RecordingIngest, v210_row_words
    from synchformer_amd.track import OffsetTracker
    dev = torch.device('cuda:0')
    if args.programmes is not None:
        return programmes_main(args, dev)
    if args.audio_channels is not None or args.audio_interleaved:
        raise SystemExit('--audio-channels / --audio-interleaved describe the wave of --programmes')
    raw_mode = args.fps is not None or args.size is not None or args.rate is not None or args.pix_fmt is not None or args.field_order != 'progressive'
    ing = None
    if raw_mode:
        fps = tuple(int(v) for v in args.fps.split('/')) if args.fps and '/' in args.fps else float(args.fps or 25)
        RH, RW = (int(v) for v in (args.size or '256x256').lower().split('x'))
        pix_fmt = args.pix_fmt or 'rgb24'
        ing = RecordingIngest(dev, fps, (RH, RW), args.rate or 16000, channels_last=pix_fmt == 'rgb24', pix_fmt=pix_fmt, chroma_loc=args.chroma_loc,
                              field_order=args.field_order)
        deep = pix_fmt in ('p010', 'yuv420p10le') + PIX_FMTS_422_16
        # random bits are a valid frame in every layout (stray bits of a 16-bit word are dropped)
        raw_shape = (RH, RW, 3) if pix_fmt == 'rgb24' else (RH, RW, 2) if pix_fmt in PIX_FMTS_PACKED else (2 * RH, RW) if pix_fmt in PIX_FMTS_422 else (RH * 3 // 2, RW)
        frame_bytes = RH * RW * 3 if pix_fmt == 'rgb24' else RH * RW * (2 if pix_fmt in PIX_FMTS_422 else 3) // (1 if pix_fmt in PIX_FMTS_422 else 2) * (2 if deep else 1)
        if pix_fmt in PIX_FMTS_V210:                                              # rows of 32-bit words at the conventional pitch; random words are a valid frame
            raw_shape = (RH, v210_row_words(RW))
            frame_bytes = 4 * raw_shape[0] * raw_shape[1]
        T_raw, n_raw = int(args.seconds * ing.fps_in), int(args.seconds * ing.rate_in)
        T, n = ing.n_frames(T_raw), ing.n_samples(n_raw)
    else:
        T, n = int(args.seconds * 25), int(args.seconds * 16000)
    g = recording_geometry(T, n, args.hop)
    N, W = g['n_segments'], g['n_windows']
    if W < 1:
        raise SystemExit(f'{args.seconds} s hold {N} segments: below one window')
    eng = SynchformerEngine(synth.make_state_dict(1337), dev, seg_chunk=args.seg_chunk)
    mel = MelFrontend(dev)
    gen = torch.Generator().manual_seed(7)
    if raw_mode:
        dgen = torch.Generator(device=dev).manual_seed(7)
        if pix_fmt in PIX_FMTS_V210:
            raw = torch.randint(-(1 << 31), (1 << 31) - 1, (T_raw, *raw_shape), generator=dgen, dtype=torch.int32, device=dev)
        elif deep:
            raw = torch.randint(-32768, 32768, (T_raw, *raw_shape), generator=dgen, dtype=torch.int16, device=dev).view(torch.uint16)
        else:
            raw = torch.randint(0, 256, (T_raw, *raw_shape), generator=dgen, dtype=torch.uint8, device=dev)
        raw_wave = torch.randint(-32768, 32768, (2, n_raw), generator=gen, dtype=torch.int32).to(torch.int16).to(dev)
        fd, wd = ing.frames(raw, 0, T), ing.wave(raw_wave)                      # materialised for the comparisons below only
        if args.host:
            raw, raw_wave = raw.cpu().pin_memory(), raw_wave.cpu().pin_memory()
        src = (fd.cpu().pin_memory(), wd.cpu().pin_memory()) if args.host else (fd, wd)
    else:
        frames = torch.randint(0, 256, (T, 3, 224, 224), generator=gen, dtype=torch.uint8)
        wave = torch.rand(n, generator=gen) * 2 - 1
        fd, wd = frames.to(dev), wave.to(dev)
        src = (frames.pin_memory(), wave.pin_memory()) if args.host else (fd, wd)
    tracker = OffsetTracker(eng, mel, hop_segments=args.hop, posterior=args.posterior, pairwise=args.pairwise)

    def timed(fn, reps=1):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, out

    t_bank, (vbank, abank) = timed(lambda: eng.extract_recording(*src, mel))
    extra = {}
    if raw_mode:
        chunks = [(8 * s0, 8 * (min(args.seg_chunk, N - s0) + s0 - 1) + 16) for s0 in range(0, N, args.seg_chunk)]      # the bank's own frame slices

        def ingest_only():
            ing.wave(raw_wave)
            for f0, f1 in chunks:
                ing.frames(raw, f0, f1)

        t_ing, _ = timed(ingest_only, reps=3)
        t_one, _ = timed(lambda: ing.frames(raw, 0, T), reps=3)                  # the whole recording in one launch
        t_wave, _ = timed(lambda: ing.wave(raw_wave), reps=3)
        t_raw, (vb_raw, ab_raw) = timed(lambda: eng.extract_recording_from(lambda f0, f1: ing.frames(raw, f0, f1), T, ing.wave(raw_wave), mel))
        table = ing.frame_table(T_raw)
        src_frames = int(torch.unique(table).numel()) / (2 if ing.interlaced else 1)          # interlaced: the table holds fields, half a frame's bytes each
        extra = {'raw_fps': float(ing.fps_in), 'raw_size': [RH, RW], 'raw_rate': ing.rate_in, 'pix_fmt': pix_fmt, 'chroma_loc': args.chroma_loc,
                 'field_order': ing.field_order, 'raw_frames': T_raw, 'raw_bytes_per_frame': frame_bytes,
                 'raw_bytes': T_raw * frame_bytes, 'frames_25fps': T, 'taps': [ing.taps_y, ing.taps_x],
                 'ingest_s': round(t_ing, 5), 'ingest_frames_per_s': round(sum(f1 - f0 for f0, f1 in chunks) / t_ing, 1),
                 'ingest_video_one_launch_s': round(t_one, 5), 'ingest_video_one_launch_frames_per_s': round(T / t_one, 1),
                 'ingest_video_one_launch_source_GBps': round(src_frames * frame_bytes / t_one / 1e9, 1), 'resample_wave_s': round(t_wave, 6),
                 'bank_from_raw_s': round(t_raw, 4), 'bank_from_raw_equals_bank': bool(torch.equal(vb_raw, vbank) and torch.equal(ab_raw, abank))}
    t_win, track = timed(lambda: tracker.track_features(vbank, abank, win_chunk=args.win_chunk), reps=3)
    if args.posterior:
        t_post, _ = timed(lambda: ops.track_posterior(track.logits, tracker.lam, tracker.grid), reps=20)
        extra.update({'conf_post_mean': round(track.conf_post.mean().item(), 4), 'conf_post_min': round(track.conf_post.min().item(), 4),
                      'log_z_per_step': round(track.log_z.item() / max(W - 1, 1), 4),
                      'max_abs_mean_minus_path_s': round((track.offset_sec_mean - track.offset_sec_path).abs().max().item(), 4),
                      'posterior_s': round(t_post, 6)})
    if args.pairwise:
        t_pair, _ = timed(lambda: ops.track_pairwise(track.logits, tracker.lam), reps=20)
        extra.update({'expected_changes': round(track.expected_changes(), 3), 'changes': [[round(v, 3) for v in row] for row in track.changes()],
                      'pairwise_s': round(t_pair, 6)})
    if args.gate:
        gate = SynchformerEngine(synth.make_state_dict(4242, head='sync_head', n_pos=184, n_out=2), dev, towers=False)
        gated = OffsetTracker(eng, mel, hop_segments=args.hop, posterior=args.posterior, gate=gate, mu=args.mu, pairwise=args.pairwise)
        gtrack = gated.track_features(vbank, abank, win_chunk=args.win_chunk)
        grid = gated.grid

        def plain_readout():
            ops.track_decode(track.logits, gated.lam)
            if args.posterior:
                ops.track_posterior(track.logits, gated.lam, grid)

        def gated_readout():
            ops.track_decode_gated(gtrack.logits, gtrack.gate_logits, gated.lam, gated.mu)
            if args.posterior:
                ops.track_posterior_gated(gtrack.logits, gtrack.gate_logits, gated.lam, gated.mu, grid)

        t_ow, _ = timed(lambda: eng.sync_windows(vbank, abank, hop=args.hop, win_chunk=args.win_chunk), reps=5)
        t_gw, _ = timed(lambda: gate.sync_windows(vbank, abank, hop=args.hop, win_chunk=args.win_chunk, n_window=gate.n_window), reps=5)
        t_pr, _ = timed(plain_readout, reps=20)
        t_gr, _ = timed(gated_readout, reps=20)
        spans = gtrack.spans()
        extra['gate'] = {'mu': args.mu, 'gate_n_window': gate.n_window, 'offset_windows_s': round(t_ow, 6), 'ungated_readout_s': round(t_pr, 6),
                         'gate_windows_s': round(t_gw, 6), 'gated_readout_s': round(t_gr, 6),
                         'gate_adds_fraction_of_track_total': round((t_gw + t_gr - t_pr) / (t_bank + t_win), 5),
                         'logits_equal_ungated': bool(torch.equal(gtrack.logits, track.logits)),
                         'windows_not_synchronizable': int((gtrack.sync_path == 0).sum().item()), 'sync_raw_mean': round(gtrack.sync_raw.mean().item(), 4),
                         'spans': [[round(t0, 2), round(t1, 2), None if off is None else round(off, 3)] for t0, t1, off in spans]}
        if args.posterior:
            extra['gate']['p_sync_mean'] = round(gtrack.p_sync.mean().item(), 4)
        if args.pairwise:
            extra['gate'].update({'expected_changes': round(gtrack.expected_changes(), 3), 'expected_flips': round(gtrack.p_flip.double().sum().item(), 3)})
        for t0, t1, off in spans:
            print(f'span {t0:8.2f} s .. {t1:8.2f} s  ' + ('not synchronizable' if off is None else f'offset {off:+.2f} s'), file=sys.stderr)
    if args.lags is not None:                                                    # the wide read-out: a search over audio lags beyond the class grid
        lo, hi, *st = [int(x) for x in args.lags.split(':')]
        lags = tuple(range(lo, hi + 1, st[0] if st else 1))
        t_wide, wtrack = timed(lambda: tracker.track_features_wide(vbank, abank, lags, win_chunk=args.win_chunk), reps=3)
        t_lw, _ = timed(lambda: eng.sync_windows_lagged(vbank, abank, lags, hop=args.hop, win_chunk=args.win_chunk), reps=3)
        wspans = wtrack.spans()
        extra['wide'] = {'lags': [lags[0], lags[-1], lags[1] - lags[0] if len(lags) > 1 else 1], 'states': len(lags) * int(tracker.grid.numel()),
                         'windows': int(wtrack.logits.shape[0]), 'first_segment': wtrack.first_segment, 'wide_track_s': round(t_wide, 5), 'plain_track_s': round(t_win, 5),
                         'lagged_windows_s': round(t_lw, 5), 'wide_readout_s': round(t_wide - t_lw, 6),
                         'spans': [[round(t0, 2), round(t1, 2), round(off, 3)] for t0, t1, off in wspans]}
        print(f'wide read-out over lags {lags[0]} .. {lags[-1]}: {t_wide * 1e3:.2f} ms (plain track {t_win * 1e3:.2f} ms)', file=sys.stderr)
        for t0, t1, off in wspans:
            print(f'wide span {t0:8.2f} s .. {t1:8.2f} s  offset {off:+.2f} s', file=sys.stderr)
    if args.stream is not None:
        source = (raw, raw_wave, ing) if raw_mode else (src[0], src[1], None)
        extra['stream'] = stream_timing(args, tracker, eng, ops, source, track)
        if args.gate:
            extra['stream_gated'] = stream_timing(args, gated, eng, ops, source, gtrack, gated=True)
            extra['stream_gated']['gate_adds_ms_per_push'] = round(extra['stream_gated']['push']['mean_ms'] - extra['stream']['push']['mean_ms'], 3)
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
        'raw_changes': int((track.cls_raw[1:] != track.cls_raw[:-1]).sum().item()), **extra}))


def programmes_main(args, dev):
    """--programmes: one recording, P audio programmes, one line per programme."""
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.ingest import PIX_FMTS_422, PIX_FMTS_422_16, PIX_FMTS_PACKED, PIX_FMTS_V210, RecordingIngest, v210_row_words
    from synchformer_amd.track import OffsetTracker
    progs = [tuple(int(c) for c in part.split('+')) for part in args.programmes.split(',')]
    progs = [p[0] if len(p) == 1 else p for p in progs]
    ch = args.audio_channels or 1 + max(c for p in progs for c in ((p,) if isinstance(p, int) else p))
    fps = tuple(int(v) for v in args.fps.split('/')) if args.fps and '/' in args.fps else float(args.fps or 25)
    RH, RW = (int(v) for v in (args.size or '256x256').lower().split('x'))
    pix_fmt = args.pix_fmt or 'rgb24'
    geo = dict(channels_last=pix_fmt == 'rgb24', pix_fmt=pix_fmt, chroma_loc=args.chroma_loc, field_order=args.field_order)
    ing = RecordingIngest(dev, fps, (RH, RW), args.rate or 16000, audio_channels=ch, audio_interleaved=args.audio_interleaved, programmes=progs, **geo)
    plain = RecordingIngest(dev, fps, (RH, RW), args.rate or 16000, **geo)
    deep = pix_fmt in ('p010', 'yuv420p10le') + PIX_FMTS_422_16
    raw_shape = (RH, RW, 3) if pix_fmt == 'rgb24' else (RH, RW, 2) if pix_fmt in PIX_FMTS_PACKED else (2 * RH, RW) if pix_fmt in PIX_FMTS_422 else (RH * 3 // 2, RW)
    T_raw, n_raw = int(args.seconds * ing.fps_in), int(args.seconds * ing.rate_in)
    dgen = torch.Generator(device=dev).manual_seed(7)
    if pix_fmt in PIX_FMTS_V210:
        raw = torch.randint(-(1 << 31), (1 << 31) - 1, (T_raw, RH, v210_row_words(RW)), generator=dgen, dtype=torch.int32, device=dev)
    elif deep:
        raw = torch.randint(-32768, 32768, (T_raw, *raw_shape), generator=dgen, dtype=torch.int16, device=dev).view(torch.uint16)
    else:
        raw = torch.randint(0, 256, (T_raw, *raw_shape), generator=dgen, dtype=torch.uint8, device=dev)
    wave = torch.stack([synth.make_wave(1, 1, 100 + c, n=n_raw).reshape(n_raw) for c in range(ch)])      # every channel its own signal: the programmes differ
    wave = wave / wave.abs().max()
    pcm = (wave * 30000).round().to(torch.int16)
    planar = wave if args.sample_fmt == 'flt' else pcm if args.sample_fmt == 's16' else pcm.to(torch.int32) << 16
    single = planar if args.sample_fmt != 's32' else pcm                         # track_raw takes fp32 or int16: the same samples
    raw_wave = planar.t().contiguous() if args.audio_interleaved else planar
    if args.host:
        raw, raw_wave, single = raw.cpu().pin_memory(), raw_wave.pin_memory(), single.pin_memory()
    else:
        raw_wave, single = raw_wave.to(dev), single.to(dev)
    eng = SynchformerEngine(synth.make_state_dict(1337), dev, seg_chunk=args.seg_chunk)
    tracker = OffsetTracker(eng, MelFrontend(dev), hop_segments=args.hop, posterior=args.posterior)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    t_all, tracks = timed(lambda: tracker.track_raw_programmes(raw, raw_wave, ing, win_chunk=args.win_chunk))
    rows = [[p] if isinstance(p, int) else list(p) for p in progs]
    t_sep, refs = timed(lambda: [tracker.track_raw(raw, single[r], plain, win_chunk=args.win_chunk) for r in rows])
    streamed = None
    if args.stream is not None:
        stream = tracker.stream(lag=args.lag, ingest=ing)
        ups, f, a, i, t = [], 0, 0, 1, 0 if args.audio_interleaved else 1
        while f < raw.shape[0] or a < raw_wave.shape[t]:
            f1, a1 = min(raw.shape[0], round(i * args.stream * float(ing.fps_in))), min(raw_wave.shape[t], round(i * args.stream * ing.rate_in))
            ups.append(stream.push(raw[f:f1], raw_wave.narrow(t, a, a1 - a)))
            f, a, i = f1, a1, i + 1
        ups.append(stream.flush())
        streamed = [torch.cat([u[p].logits for u in ups]) for p in range(len(progs))]
    for p, (prog, tr, ref) in enumerate(zip(progs, tracks, refs)):
        line = {'tool': 'track_recording', 'programme': p, 'channels': rows[p], 'programmes': len(progs), 'audio_channels': ch, 'sample_fmt': args.sample_fmt,
                'audio_interleaved': bool(args.audio_interleaved), 'seconds': args.seconds, 'segments': tr.n_segments, 'windows': int(tr.logits.shape[0]),
                'track_raw_programmes_s': round(t_all, 4), 'track_raw_per_programme_s': round(t_sep, 4), 'ratio': round(t_all / t_sep, 3),
                'logits_equal_track_raw': bool(torch.equal(tr.logits, ref.logits)), 'max_abs_logit_diff_vs_track_raw': round((tr.logits - ref.logits).abs().max().item(), 6),
                'path_changes': int((tr.cls_path[1:] != tr.cls_path[:-1]).sum().item()), 'offset_sec_path_first': round(tr.offset_sec_path[0].item(), 3)}
        if streamed is not None:
            line['stream'] = {'piece_s': args.stream, 'lag': args.lag, 'held_after': stream.held,
                              'logits_equal_offline': bool(streamed[p].shape == tr.logits.shape and torch.equal(streamed[p], tr.logits))}
        print(json.dumps(line))


def stream_timing(args, tracker, eng, ops, source, track, gated=False):
    """Pushes the recording through tracker.stream(lag) in pieces of args.stream seconds, twice (the first pass warms up); the three stages are timed by wrapping
    the calls OffsetStream makes (engine.extract_segments_from, engine.sync_windows, ops.track_stream_push) between device synchronisations.  gated: through
    tracker.stream(lag, gated=True) - the read-out is ops.track_stream_push_gated and the gate's own sync_windows is a fourth stage."""
    frames, wave, ing = source
    fps, rate = (float(ing.fps_in), ing.rate_in) if ing is not None else (25.0, 16000)
    ms = {}

    def staged(obj, name, key):
        fn = getattr(obj, name)

        def wrapped(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            ms[key] = ms.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
            return out
        setattr(obj, name, wrapped)
        return fn

    saved = [(eng, 'extract_segments_from', staged(eng, 'extract_segments_from', 'bank')), (eng, 'sync_windows', staged(eng, 'sync_windows', 'windows')),
             (ops, 'track_stream_push', staged(ops, 'track_stream_push', 'readout'))]
    if gated:
        setattr(ops, 'track_stream_push', saved[-1][2])
        saved[-1] = (ops, 'track_stream_push_gated', staged(ops, 'track_stream_push_gated', 'readout'))
        saved.append((tracker.gate, 'sync_windows', staged(tracker.gate, 'sync_windows', 'gate_windows')))
    try:
        for _ in range(2):
            stream = tracker.stream(lag=args.lag, ingest=ing, gated=True) if gated else tracker.stream(lag=args.lag, ingest=ing)
            rows, logits, gate_logits, flagged, f, a, i = [], [], [], 0, 0, 0, 1
            t_start = time.perf_counter()
            while f < frames.shape[0] or a < wave.shape[-1]:
                f1, a1 = min(frames.shape[0], round(i * args.stream * fps)), min(wave.shape[-1], round(i * args.stream * rate))
                ms.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                upd = stream.push(frames[f:f1], wave[..., a:a1])
                torch.cuda.synchronize()
                rows.append(dict(ms, push=(time.perf_counter() - t0) * 1e3, windows_new=int(upd.logits.shape[0]), committed=int(upd.cls_lag.shape[0])))
                logits.append(upd.logits)
                if gated:
                    gate_logits.append(upd.gate_logits)
                    flagged += int((upd.sync_lag == 0).sum().item())
                    rows[-1]['not_synchronizable'] = int((upd.sync_lag == 0).sum().item())
                f, a, i = f1, a1, i + 1
            upd = stream.flush()
            logits.append(upd.logits)
            if gated:
                gate_logits.append(upd.gate_logits)
                flagged += int((upd.sync_lag == 0).sum().item())
            torch.cuda.synchronize()
            total = time.perf_counter() - t_start
    finally:
        for obj, name, fn in saved:
            setattr(obj, name, fn)
    for r in rows:
        print('push ' + '  '.join(f'{k} {v:.2f} ms' if isinstance(v, float) else f'{k} {v}' for k, v in r.items()), file=sys.stderr)
    busy = [r for r in rows if r['windows_new']]

    def stat(key):
        v = [r.get(key, 0.0) for r in busy]
        return {'mean_ms': round(sum(v) / max(len(v), 1), 3), 'max_ms': round(max(v, default=0.0), 3)}

    got = torch.cat(logits)
    more = {}
    if gated:
        gz = torch.cat(gate_logits)
        more = {'gate_windows': stat('gate_windows'), 'windows_not_synchronizable': flagged,
                'gate_logits_equal_offline': bool(gz.shape == track.gate_logits.shape and torch.equal(gz, track.gate_logits))}
    return {**more, 'piece_s': args.stream, 'lag': args.lag, 'pushes': len(rows), 'pushes_with_windows': len(busy), 'bank': stat('bank'), 'windows': stat('windows'),
            'readout': stat('readout'), 'push': stat('push'), 'held_after': stream.held, 'total_s': round(total, 4),
            'logits_equal_offline': bool(got.shape == track.logits.shape and torch.equal(got, track.logits)),
            'max_abs_logit_diff_vs_offline': round((got - track.logits).abs().max().item(), 6) if got.shape == track.logits.shape else None}


if __name__ == '__main__':
    main()
