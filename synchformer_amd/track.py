"""Track the audio-visual offset along a recording.

The inference entry points take one window (14 segments, ~4.8 s) and return one answer; a recording is a sequence of overlapping windows.  Sliding
`forward_clips` over it sends every segment through both towers once per window that contains it - 14 times at a hop of one segment - and the towers
are 99.8 % of the FLOPs.  Here every segment crosses the towers once (`engine.extract_recording`: the segment feature bank), the windows are row-map
views of the bank (`engine.sync_windows`), and the W logit rows are read out on the device (`ops.track_decode`: per-window argmax and a Viterbi path
under a cost on class changes; with `posterior=True` also `ops.track_posterior`, DESIGN 3.14: the marginals of the chain whose mode is that path - a
confidence that carries the evidence of the whole recording, and an offset finer than the class grid).

    tracker = OffsetTracker(engine, MelFrontend(dev))
    track = tracker.track(frames, wave)           # frames (T, 3, 224, 224) uint8, wave (n,) fp32 16 kHz; device or host
    track = tracker.track_raw(raw_frames, raw_wave, RecordingIngest(dev, (30000, 1001), (1080, 1920), 48000, channels_last=True))   # as decoded
    track.t_sec, track.offset_sec_path            # where in the recording, which offset
    track = OffsetTracker(engine, mel, posterior=True).track(frames, wave)
    track.conf_post, track.offset_sec_mean        # how sure given every window, the posterior mean offset

Out of scope (one recording per call): batching several recordings, double-buffered host-to-device transfer of the chunks, de-duplicating the
overlapped tubelets inside the patch embedding.
"""
from dataclasses import dataclass
from typing import Optional

import torch

from . import ops
from .frontend import recording_geometry
from .postprocess import class_grid


def window_times(n_windows: int, hop_segments: int = 1, v_fps: float = 25.0, **segment_kw) -> torch.Tensor:
    """Centres (seconds, fp32) of the windows of a recording: window w covers frames [8 hop w, 8 hop w + 120) at 25 fps -> (8 hop w + 60) / 25."""
    g = recording_geometry(0, 0, hop_segments, **segment_kw)
    span = (g['n_window'] - 1) * g['v_stride'] + g['v_size']                    # frames of one window (120)
    w = torch.arange(n_windows, dtype=torch.float64)
    return ((g['v_stride'] * hop_segments * w + span / 2) / v_fps).float()


@dataclass
class OffsetTrack:
    """Read-out of one recording: W windows in time order, tensors on the engine's device."""
    t_sec: torch.Tensor              # (W,) fp32: window centres, (8 hop w + 60) / 25
    logits: torch.Tensor             # (W, C) fp32
    cls_raw: torch.Tensor            # (W,) int32: per-window argmax
    conf_raw: torch.Tensor           # (W,) fp32: its softmax probability
    cls_path: torch.Tensor           # (W,) int32: Viterbi path
    conf_path: torch.Tensor          # (W,) fp32: softmax probability of the path's class
    offset_sec_raw: torch.Tensor     # (W,) fp32: grid[cls_raw]
    offset_sec_path: torch.Tensor    # (W,) fp32: grid[cls_path]
    n_segments: int                  # segments in the bank
    # the posterior read-out (OffsetTracker(posterior=True), ops.track_posterior); None without it
    post: Optional[torch.Tensor] = None              # (W, C) fp32: marginal of class c in window w given all windows; rows sum to 1
    cls_post: Optional[torch.Tensor] = None          # (W,) int32: argmax_c post
    conf_post: Optional[torch.Tensor] = None         # (W,) fp32: post[w, cls_post[w]]
    offset_sec_post: Optional[torch.Tensor] = None   # (W,) fp32: grid[cls_post]
    offset_sec_mean: Optional[torch.Tensor] = None   # (W,) fp32: sum_c post[w, c] grid[c]
    log_z: Optional[torch.Tensor] = None             # (1,) fp32: log partition sum against independent softmax draws, <= 0 (0: the windows agree)


class OffsetTracker:
    """engine: a SynchformerEngine; mel: a frontend.MelFrontend on the same device; hop_segments: windows advance by this many segments (1 = 0.32 s);
    lam: cost of one class step between neighbouring windows in the Viterbi read-out, in logit units (0 = the per-window argmax; large = one class for the
    whole recording).  lam = 1.0 is a DEFAULT, NOT A TUNED VALUE: nobody has measured it on real recordings (no trained checkpoint ships with this
    repository) - choose it on held-out recordings of the domain.  grid: the offsets (seconds) the classes stand for, default class_grid(-2, 2, 21); its
    length must be the engine's n_out (an engine with the 2-way syncability head takes a 2-element grid, e.g. torch.tensor([0., 1.])).  posterior: also
    read the windows out as marginals under the same lam (two more launches; fills OffsetTrack.post .. log_z)."""

    def __init__(self, engine, mel, hop_segments: int = 1, lam: float = 1.0, grid: Optional[torch.Tensor] = None, posterior: bool = False):
        if hop_segments < 1:
            raise ValueError(f'hop_segments = {hop_segments}')
        if not (lam >= 0 and lam != float('inf')):
            raise ValueError(f'lam = {lam}: the cost of a class change is finite and >= 0')
        grid = class_grid(-2, 2, 21) if grid is None else torch.as_tensor(grid, dtype=torch.float32)
        if grid.dim() != 1 or grid.numel() != engine.n_out:
            raise ValueError(f'a grid of {tuple(grid.shape)} classes for an engine with {engine.n_out} outputs')
        self.eng, self.mel, self.hop, self.lam = engine, mel, int(hop_segments), float(lam)
        self.grid = grid.to(engine.dev)
        self.posterior = bool(posterior)

    def track_features(self, vbank: torch.Tensor, abank: torch.Tensor, win_chunk: int = 256) -> OffsetTrack:
        """Segment feature banks (N, 8, 768) / (N, 6, 768) (engine.extract_recording, or features the caller already holds) -> OffsetTrack."""
        logits = self.eng.sync_windows(vbank, abank, hop=self.hop, win_chunk=win_chunk)
        cls_raw, conf_raw, cls_path, conf_path = ops.track_decode(logits, self.lam)
        track = OffsetTrack(t_sec=window_times(logits.shape[0], self.hop).to(self.eng.dev), logits=logits, cls_raw=cls_raw, conf_raw=conf_raw,
                            cls_path=cls_path, conf_path=conf_path, offset_sec_raw=self.grid[cls_raw.long()], offset_sec_path=self.grid[cls_path.long()],
                            n_segments=int(vbank.shape[0]))
        if self.posterior:
            track.post, track.cls_post, track.conf_post, track.offset_sec_mean, track.log_z = ops.track_posterior(logits, self.lam, self.grid)
            track.offset_sec_post = self.grid[track.cls_post.long()]
        return track

    def track(self, frames: torch.Tensor, wave: torch.Tensor, seg_chunk: Optional[int] = None, win_chunk: int = 256) -> OffsetTrack:
        """frames (T, 3, 224, 224) uint8, wave (n,) fp32 16 kHz, on the device or in host memory -> OffsetTrack; ValueError below one window (120 frames,
        76800 samples)."""
        return self.track_features(*self.eng.extract_recording(frames, wave, self.mel, seg_chunk), win_chunk=win_chunk)

    def track_raw(self, raw_frames: torch.Tensor, raw_wave: torch.Tensor, ingest, seg_chunk: Optional[int] = None, win_chunk: int = 256) -> OffsetTrack:
        """The recording as a decoder hands it out: raw_frames uint8 (T, 3, H, W) or channels-last (T, H, W, 3) at the native frame rate and
        size, raw_wave fp32 or int16 (n,) / (ch, n) at the native rate, device or host; `ingest` an ingest.RecordingIngest of that geometry -> OffsetTrack.
        Each tower chunk's 25 fps, 224 x 224 frames are made from the raw ones right before the chunk runs; the resized recording is never materialised.
        ValueError below one window after conversion, or when the frames do not have the ingest's size."""
        ingest._check_frames(raw_frames)
        wave = ingest.wave(raw_wave)
        banks = self.eng.extract_recording_from(lambda f0, f1: ingest.frames(raw_frames, f0, f1), ingest.n_frames(raw_frames.shape[0]), wave, self.mel, seg_chunk)
        return self.track_features(*banks, win_chunk=win_chunk)
