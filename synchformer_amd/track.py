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

    gate = SynchformerEngine(syncability_sd, dev, towers=False)        # the 2-way syncability head of the same towers (checkpoint.same_towers)
    track = OffsetTracker(engine, mel, gate=gate).track(frames, wave)  # the read-outs run over (offset class, synchronizable flag): silence, music beds and
    track.sync_path, track.p_sync, track.spans()                       # cutaways are flagged instead of being read as an offset

    stream = tracker.stream(lag=16)               # a live feed: push what arrived, get the windows that became final
    upd = stream.push(frames_1s, wave_1s)         # upd.cls_lag / offset_sec_lag: committed, never revised; upd.offset_sec_tail[-1]: the offset now
    upd = stream.flush()                          # end of the feed: the tail is committed

    gated = OffsetTracker(engine, mel, gate=gate).stream(lag=16, gated=True)      # the live feed read over (offset class, synchronizable flag)
    upd = gated.push(frames_1s, wave_1s)          # upd.sync_lag: 0 where the committed window says 'nothing to read here'; upd.p_sync_lag with posterior=True

    pool = tracker.pool(n_feeds=64, lag=16)       # many live feeds on one device: one tick = one batched pass for all of them
    a, b = pool.open(), pool.open()
    upds = pool.push({a: (frames_a, wave_a), b: (frames_b, wave_b)})     # {feed: OffsetUpdate}, each what the feed's own stream would return
    upds = pool.push({a: (frames_a2, wave_a2)}, flush=[b])               # b's final push; its slot is free again

    ing = RecordingIngest(dev, 25, (1080, 1920), 48000, audio_channels=8, audio_interleaved=True, programmes=[(0, 1), (2, 3), 4])
    tracks = tracker.track_raw_programmes(raw_frames, raw_wave, ing)     # one OffsetTrack per audio programme; the picture crosses its tower once
    upds = tracker.stream(ingest=ing).push(raw_frames_1s, raw_wave_1s)   # a ProgrammeStream: one OffsetUpdate per programme

Out of scope (one recording per call): batching several recordings offline, double-buffered host-to-device transfer of the chunks, de-duplicating the
overlapped tubelets inside the patch embedding.
"""
from dataclasses import dataclass
from typing import List, Optional

import torch

from . import ops
from .frontend import recording_geometry, stream_geometry
from .postprocess import class_grid


def window_times64(n_windows: int, hop_segments: int = 1, v_fps: float = 25.0, first_window: int = 0, **segment_kw) -> torch.Tensor:
    """Centres (seconds, float64) of windows first_window .. first_window + n_windows - 1: window w covers frames [8 hop w, 8 hop w + 120) at 25 fps ->
    (8 hop w + 60) / 25, computed at the absolute window index (a stream's day-old windows keep their milliseconds)."""
    g = recording_geometry(0, 0, hop_segments, **segment_kw)
    span = (g['n_window'] - 1) * g['v_stride'] + g['v_size']                    # frames of one window (120)
    w = torch.arange(first_window, first_window + n_windows, dtype=torch.float64)
    return (g['v_stride'] * hop_segments * w + span / 2) / v_fps


def window_times(n_windows: int, hop_segments: int = 1, v_fps: float = 25.0, **segment_kw) -> torch.Tensor:
    """Centres (seconds, fp32) of the windows of a recording: window w covers frames [8 hop w, 8 hop w + 120) at 25 fps -> (8 hop w + 60) / 25."""
    return window_times64(n_windows, hop_segments, v_fps, **segment_kw).float()


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
    # the gate (OffsetTracker(gate=...), ops.track_decode_gated / track_posterior_gated); None without it.  Optional attributes, set by the tracker and
    # deliberately NOT dataclass fields: the field list and the positional constructor above stay what they were
    gate_logits = None               # (W, 2) fp32: the syncability head on the windows' first gate.n_window segments, class 1 = synchronizable
    sync_raw = None                  # (W,) fp32: sigmoid(z1 - z0), the gate's own per-window probability
    sync_path = None                 # (W,) int32: the flag along the joint Viterbi path (cls_path is that path's class), 1 = synchronizable
    p_sync = None                    # (W,) fp32: the flag's marginal given all windows (with posterior=True)
    # the pairwise read-out (OffsetTracker(pairwise=True), ops.track_pairwise / track_pairwise_gated); None without it.  Plain attributes as the gate's:
    # one row per boundary between windows w and w + 1
    t_change = None                  # (W-1,) fp32: the boundary's time, half-way between the two window centres
    p_change = None                  # (W-1,) fp32: the probability, given all windows, that the offset class changes at the boundary
    jump_abs = None                  # (W-1,) fp32: the expected class step |c_{w+1} - c_w|
    p_change_top = None              # (W-1,) fp32: the probability of the likeliest change, change_from_sec -> change_to_sec
    change_from_sec = None           # (W-1,) fp32: grid[top_from]
    change_to_sec = None             # (W-1,) fp32: grid[top_to]
    p_flip = None                    # (W-1,) fp32: the probability that the synchronizable flag changes at the boundary (with a gate)

    def changes(self, min_prob: float = 0.5):
        """Host side (OffsetTracker(pairwise=True)): the boundaries where the offset changed with probability p_change >= min_prob, as a list of
        (t_sec, from_sec, to_sec, p_change, p_top) in time order - from_sec -> to_sec the likeliest change there, p_top its probability.  Overlapping windows
        SMEAR a change over neighbouring boundaries (a window that straddles it votes for either side), and each of them can stay under min_prob although the
        change is certain: expected_changes() does not have that problem, the probability of a change within an interval is not built.  Synchronises."""
        if self.p_change is None:
            raise ValueError('OffsetTrack.changes: no pairwise read-out on this track (OffsetTracker(..., pairwise=True))')
        cols = [x.detach().cpu().double().tolist() for x in (self.t_change, self.change_from_sec, self.change_to_sec, self.p_change, self.p_change_top)]
        return [row for row in zip(*cols) if row[3] >= min_prob]

    def expected_changes(self) -> float:
        """Host side (OffsetTracker(pairwise=True)): the expected number of offset changes along the recording, sum_w p_change[w].  A change that overlapping
        windows smear over neighbouring boundaries, each under changes()'s min_prob, still counts here with its whole mass; the probability of a change
        within an interval is not built.  Synchronises."""
        if self.p_change is None:
            raise ValueError('OffsetTrack.expected_changes: no pairwise read-out on this track (OffsetTracker(..., pairwise=True))')
        return float(self.p_change.detach().double().sum().item())

    def spans(self):
        """Host side: the runs of constant (sync_path, cls_path) as a list of (t0_sec, t1_sec, offset_sec or None), in time order - None where the path says 'not
        synchronizable'.  Neighbouring spans meet half-way between their windows' centres; the first starts at t_sec[0], the last ends at t_sec[-1].  Without a
        gate every window counts as synchronizable.  Synchronises (the path is copied to the host)."""
        t = self.t_sec.detach().cpu().double().tolist()
        cls = self.cls_path.detach().cpu().tolist()
        off = self.offset_sec_path.detach().cpu().tolist()
        sync = [1] * len(cls) if self.sync_path is None else self.sync_path.detach().cpu().tolist()
        out, a = [], 0
        for w in range(1, len(cls) + 1):
            if w == len(cls) or (sync[w], cls[w]) != (sync[a], cls[a]):
                t0 = t[a] if a == 0 else 0.5 * (t[a - 1] + t[a])
                t1 = t[w - 1] if w == len(cls) else 0.5 * (t[w - 1] + t[w])
                out.append((t0, t1, float(off[a]) if sync[a] else None))
                a = w
        return out


@dataclass
class WideOffsetTrack:
    """Read-out of one recording over a search of audio lags (OffsetTracker.track_features_wide): W windows in time order, D lags, S = D C states;
    tensors on the engine's device.  State (lag d, class c) stands for the offset 0.32 d + grid[c] seconds (a_start = v_start + offset_sec)."""
    t_sec: torch.Tensor              # (W,) fp32: centres of the windows' PICTURE, window_times + 0.32 first_segment
    lags: tuple                      # the D lags, in segments of 0.32 s, ascending
    logits: torch.Tensor             # (W, D, C) fp32: window w paired at lag lags[j]
    gate_logits: Optional[torch.Tensor]   # (W, D, 2) fp32 with a gate (class 1 = synchronizable), else None
    lag_raw: torch.Tensor            # (W,) int32: the lag (segments) of the per-window argmax over all states
    cls_raw: torch.Tensor            # (W,) int32: its class
    conf_raw: torch.Tensor           # (W,) fp32: its softmax probability over all states
    offset_sec_raw: torch.Tensor     # (W,) fp32: its offset
    state_path: torch.Tensor         # (W,) int32: the Viterbi path, as states of the table (ops.track_wide_states)
    lag_path: torch.Tensor           # (W,) int32: the path's lag (segments)
    cls_path: torch.Tensor           # (W,) int32: the path's class
    conf_path: torch.Tensor          # (W,) fp32: the softmax probability of the path's state
    offset_sec_path: torch.Tensor    # (W,) fp32: the path's offset
    n_segments: int                  # segments in the bank
    first_segment: int               # v0: the visual segment window 0 starts at (max(0, -lags[0]))
    # the posterior read-out (OffsetTracker(posterior=True), ops.track_posterior_wide); None without it
    post: Optional[torch.Tensor] = None              # (W, S) fp32: marginal of state s in window w given all windows
    p_lag: Optional[torch.Tensor] = None             # (W, D) fp32: marginal of each lag
    state_post: Optional[torch.Tensor] = None        # (W,) int32: argmax_s post
    conf_post: Optional[torch.Tensor] = None         # (W,) fp32: its value
    offset_sec_post: Optional[torch.Tensor] = None   # (W,) fp32: the offset of state_post
    offset_sec_mean: Optional[torch.Tensor] = None   # (W,) fp32: sum_s post[w, s] offset[s]
    log_z: Optional[torch.Tensor] = None             # (1,) fp32: log partition sum, <= W log D without a gate

    def spans(self):
        """Host side, as OffsetTrack.spans over offset_sec_path: the runs of a constant path state as (t0_sec, t1_sec, offset_sec), in time order; neighbouring spans
        meet half-way between their windows' centres.  Two states of one offset (0.32 * 5 - 1.6 = 0.0) are one run.  Synchronises."""
        t = self.t_sec.detach().cpu().double().tolist()
        off = self.offset_sec_path.detach().cpu().tolist()
        out, a = [], 0
        for w in range(1, len(off) + 1):
            if w == len(off) or off[w] != off[a]:
                t0 = t[a] if a == 0 else 0.5 * (t[a - 1] + t[a])
                t1 = t[w - 1] if w == len(off) else 0.5 * (t[w - 1] + t[w])
                out.append((t0, t1, float(off[a])))
                a = w
        return out


class OffsetTracker:
    """engine: a SynchformerEngine; mel: a frontend.MelFrontend on the same device; hop_segments: windows advance by this many segments (1 = 0.32 s);
    lam: cost of one class step between neighbouring windows in the Viterbi read-out, in logit units (0 = the per-window argmax; large = one class for the
    whole recording).  lam = 1.0 is a DEFAULT, NOT A TUNED VALUE: nobody has measured it on real recordings (no trained checkpoint ships with this
    repository) - choose it on held-out recordings of the domain.  grid: the offsets (seconds) the classes stand for, default class_grid(-2, 2, 21); its
    length must be the engine's n_out (an engine with the 2-way syncability head takes a 2-element grid, e.g. torch.tensor([0., 1.])).  posterior: also
    read the windows out as marginals under the same lam (two more launches; fills OffsetTrack.post .. log_z).
    gate: an engine with the 2-way syncability head (n_out == 2, class 1 = synchronizable; SynchformerEngine(sd, dev, towers=False) suffices) on the
    same device, of the SAME towers as `engine` (checkpoint.same_towers - nothing here can check it).  Gate window w is segments [w hop, w hop + gate.n_window) of
    the same banks, start-aligned with offset window w; cls_path, conf_path, offset_sec_path and the posterior fields then come from the chain over (offset class,
    synchronizable flag), and gate_logits, sync_raw, sync_path, p_sync are filled.  mu: the cost of one change of the flag between neighbouring windows, in logit
    units.  mu = 2.0 is a DEFAULT, NOT A TUNED VALUE, as lam: choose both on held-out recordings of the domain.  A prior on the flag is a constant added to
    gate_logits[:, 1] by the caller.  stream() and pool() read a live feed through the same chain with gated=True (a carried state 2C wide) or, with
    gated=False, as a tracker without a gate does; on a tracker with a gate the choice is explicit.
    pairwise: also read out the boundaries between neighbouring windows (ops.track_pairwise, with a gate ops.track_pairwise_gated; two more launches):
    fills OffsetTrack.t_change .. change_to_sec (p_flip with a gate) for OffsetTrack.changes() / expected_changes().  fit_smoothness (below) fits lam and mu on
    labelled recordings."""

    def __init__(self, engine, mel, hop_segments: int = 1, lam: float = 1.0, grid: Optional[torch.Tensor] = None, posterior: bool = False, gate=None,
                 mu: float = 2.0, pairwise: bool = False):
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
        if not (mu >= 0 and mu != float('inf')):
            raise ValueError(f'mu = {mu}: the cost of a change of the synchronizable flag is finite and >= 0')
        if gate is not None:
            if gate.n_out != 2:
                raise ValueError(f'gate: an engine with {gate.n_out} outputs, the syncability head has 2 (class 1 = synchronizable)')
            if torch.device(gate.dev) != torch.device(engine.dev):
                raise ValueError(f'gate: on {gate.dev}, the engine on {engine.dev}')
            if engine.n_out > 32:
                raise ValueError(f'gate: the gated read-outs serve at most 32 classes, the engine has {engine.n_out}')
            if not 1 <= gate.n_window <= engine.n_window:
                raise ValueError(f'gate: its window of {gate.n_window} segments does not fit the offset window of {engine.n_window} it is start-aligned with')
        self.gate, self.mu = gate, float(mu)
        self.pairwise = bool(pairwise)
        self._wide_cache = {}                                                    # lags -> the wide read-outs' tables on the device (_wide_tables)

    def track_features(self, vbank: torch.Tensor, abank: torch.Tensor, win_chunk: int = 256) -> OffsetTrack:
        """Segment feature banks (N, 8, 768) / (N, 6, 768) (engine.extract_recording, or features the caller already holds) -> OffsetTrack."""
        logits = self.eng.sync_windows(vbank, abank, hop=self.hop, win_chunk=win_chunk)
        gate_logits = None
        if self.gate is not None:                                                # the same banks, start-aligned windows of the gate's own length: exactly W rows
            gate_logits = self.gate.sync_windows(vbank, abank, hop=self.hop, win_chunk=win_chunk, n_window=self.gate.n_window)[:logits.shape[0]]
        return self._track_of(logits, int(vbank.shape[0]), gate_logits)

    def _track_of(self, logits: torch.Tensor, n_segments: int, gate_logits: Optional[torch.Tensor] = None) -> OffsetTrack:
        """The read-out of one recording's window logits (W, C); with a gate, over (offset class, synchronizable flag) with its logits (W, 2) of the same windows."""
        sync_raw = sync_path = None
        if gate_logits is None:
            cls_raw, conf_raw, cls_path, conf_path = ops.track_decode(logits, self.lam)
        else:
            cls_raw, conf_raw, sync_raw, cls_path, sync_path, conf_path = ops.track_decode_gated(logits, gate_logits, self.lam, self.mu)
        track = OffsetTrack(t_sec=window_times(logits.shape[0], self.hop).to(self.eng.dev), logits=logits, cls_raw=cls_raw, conf_raw=conf_raw,
                            cls_path=cls_path, conf_path=conf_path, offset_sec_raw=self.grid[cls_raw.long()], offset_sec_path=self.grid[cls_path.long()],
                            n_segments=n_segments)
        track.gate_logits, track.sync_raw, track.sync_path = gate_logits, sync_raw, sync_path
        if self.posterior and gate_logits is None:
            track.post, track.cls_post, track.conf_post, track.offset_sec_mean, track.log_z = ops.track_posterior(logits, self.lam, self.grid)
        elif self.posterior:
            track.post, track.p_sync, track.cls_post, track.conf_post, track.offset_sec_mean, track.log_z = ops.track_posterior_gated(logits, gate_logits, self.lam,
                                                                                                                                       self.mu, self.grid)
        if self.posterior:
            track.offset_sec_post = self.grid[track.cls_post.long()]
        if self.pairwise:
            if gate_logits is None:
                track.p_change, track.jump_abs, top_from, top_to, track.p_change_top, _, _ = ops.track_pairwise(logits, self.lam)
            else:
                track.p_change, track.jump_abs, track.p_flip, top_from, top_to, track.p_change_top, _, _ = ops.track_pairwise_gated(logits, gate_logits, self.lam,
                                                                                                                                   self.mu)
            track.t_change = 0.5 * (track.t_sec[:-1] + track.t_sec[1:])
            track.change_from_sec, track.change_to_sec = self.grid[top_from.long()], self.grid[top_to.long()]
        return track

    WIDE_TABLES_KEPT = 8                                                         # sets of lags whose tables stay on the device (the oldest goes first)

    def _wide_tables(self, lags):
        """The states of a search over `lags` (ops.track_wide_states on the tracker's grid) and their tables on the device, kept for the last WIDE_TABLES_KEPT sets
        of lags -> (lags as a tuple, ops.TrackWideTables, lag values (S,) int32, classes (S,) int32 on the device)."""
        lags = tuple(int(d) for d in lags)
        if lags not in self._wide_cache:
            src, pos, off, lag_of, cls_of = ops.track_wide_states(lags, self.grid)
            tables = ops.track_wide_tables(src, pos, off, len(lags), int(self.grid.numel()), self.eng.dev)
            lag_val = torch.tensor(lags, dtype=torch.int32)[lag_of.long()]
            while len(self._wide_cache) >= self.WIDE_TABLES_KEPT:
                self._wide_cache.pop(next(iter(self._wide_cache)))
            self._wide_cache[lags] = (lags, tables, lag_val.to(self.eng.dev), cls_of.to(self.eng.dev))
        return self._wide_cache[lags]

    def track_features_wide(self, vbank: torch.Tensor, abank: torch.Tensor, lags, win_chunk: int = 256) -> WideOffsetTrack:
        """track_features beyond the class grid: the banks are read at every lag of `lags` (strictly ascending integers, segments of 0.32 s; D lags x C
        classes <= 1024 states) through engine.sync_windows_lagged - no tower runs again - and the (W, D, C) logits are read out by track_logits_wide; `lam` keeps
        its meaning, the cost of one class step.  A tracker with a gate passes its logits at the same lags as the emission's gate term.  What the model's logits look
        like at a lag whose residual lies outside the grid is NOT known here (no trained checkpoint): the read-out is the chain's, whatever it is fed."""
        lags = tuple(int(d) for d in lags)
        logits = self.eng.sync_windows_lagged(vbank, abank, lags, hop=self.hop, win_chunk=win_chunk)
        gate_logits = None
        if self.gate is not None:                                                # start-aligned windows of the gate's own length at the same lags: the first W rows
            gate_logits = self.gate.sync_windows_lagged(vbank, abank, lags, hop=self.hop, win_chunk=win_chunk, n_window=self.gate.n_window)
            if gate_logits.shape[0] < logits.shape[0]:
                raise ValueError(f'track_features_wide: the gate\'s window of {self.gate.n_window} segments gives {gate_logits.shape[0]} windows at these lags, the offset '
                                 f'window of {self.eng.n_window} segments {logits.shape[0]}: the gate\'s window must not be the longer one')
            gate_logits = gate_logits[:logits.shape[0]]
        return self.track_logits_wide(logits, lags, gate_logits, n_segments=int(vbank.shape[0]))

    def track_logits_wide(self, logits: torch.Tensor, lags, gate_logits: Optional[torch.Tensor] = None, n_segments: Optional[int] = None) -> WideOffsetTrack:
        """The read-out of window logits the caller already holds: logits fp32 (W, D, C) on the engine's device, window w paired at lag lags[j] (what
        engine.sync_windows_lagged returns), gate_logits fp32 (W, D, 2) or None -> WideOffsetTrack, through ops.track_decode_wide (with posterior=True also
        ops.track_posterior_wide) over the states (lag, class) at the offsets 0.32 lag + grid[c].  n_segments: the bank's length, for the track's record (default: the
        shortest bank that holds these windows)."""
        lags, tables, lag_val, cls_val = self._wide_tables(lags)
        if logits.dim() != 3 or tuple(logits.shape[1:]) != (len(lags), int(self.grid.numel())):
            raise ValueError(f'track_logits_wide: logits {tuple(logits.shape)} for {len(lags)} lags x {int(self.grid.numel())} classes')
        v0 = max(0, -lags[0])
        if n_segments is None:
            n_segments = v0 + max(0, lags[-1]) + self.eng.n_window + self.hop * max(0, logits.shape[0] - 1)
        state_raw, conf_raw, state_path, conf_path = ops.track_decode_wide(logits, tables, self.lam, gate_logits)
        raw, path = state_raw.long(), state_path.long()
        seg_sec = 0.32
        track = WideOffsetTrack(t_sec=(window_times64(logits.shape[0], self.hop) + seg_sec * v0).float().to(self.eng.dev), lags=lags, logits=logits,
                                gate_logits=gate_logits, lag_raw=lag_val[raw], cls_raw=cls_val[raw], conf_raw=conf_raw, offset_sec_raw=tables.off[raw],
                                state_path=state_path, lag_path=lag_val[path], cls_path=cls_val[path], conf_path=conf_path, offset_sec_path=tables.off[path],
                                n_segments=int(n_segments), first_segment=v0)
        if self.posterior:
            track.post, track.state_post, track.conf_post, track.offset_sec_mean, track.p_lag, track.log_z = ops.track_posterior_wide(logits, tables, self.lam,
                                                                                                                                       gate_logits)
            track.offset_sec_post = tables.off[track.state_post.long()]
        return track

    def track_wide(self, frames: torch.Tensor, wave: torch.Tensor, lags, seg_chunk: Optional[int] = None, win_chunk: int = 256) -> WideOffsetTrack:
        """track() over a search of audio lags: inputs as track(), `lags` as track_features_wide -> WideOffsetTrack."""
        return self.track_features_wide(*self.eng.extract_recording(frames, wave, self.mel, seg_chunk), lags, win_chunk=win_chunk)

    def track_raw_wide(self, raw_frames: torch.Tensor, raw_wave: torch.Tensor, ingest, lags, seg_chunk: Optional[int] = None, win_chunk: int = 256) -> WideOffsetTrack:
        """track_raw() over a search of audio lags: inputs as track_raw(), `lags` as track_features_wide -> WideOffsetTrack."""
        if getattr(ingest, 'programmes', None) is not None:
            raise ValueError(f'track_raw_wide: the ingest has {len(ingest.programmes)} audio programmes; the wide read-out serves one')
        ingest._check_frames(raw_frames)
        wave = ingest.wave(raw_wave)
        banks = self.eng.extract_recording_from(lambda f0, f1: ingest.frames(raw_frames, f0, f1), ingest.n_frames(raw_frames.shape[0]), wave, self.mel, seg_chunk)
        return self.track_features_wide(*banks, lags, win_chunk=win_chunk)

    def track_features_programmes(self, vbank: torch.Tensor, abanks: torch.Tensor, win_chunk: int = 256) -> List[OffsetTrack]:
        """One visual bank (N, 8, 768) and the audio banks of P programmes (P, N, 6, 768) (engine.extract_recording_programmes_from) -> one OffsetTrack per
        programme, each what track_features gives for (vbank, abanks[p]); vproj runs over the visual bank once (engine.sync_windows_programmes)."""
        logits = self.eng.sync_windows_programmes(vbank, abanks, hop=self.hop, win_chunk=win_chunk)
        gate_logits = [None] * logits.shape[0]
        if self.gate is not None:
            gate_logits = self.gate.sync_windows_programmes(vbank, abanks, hop=self.hop, win_chunk=win_chunk, n_window=self.gate.n_window)[:, :logits.shape[1]]
        return [self._track_of(logits[p], int(vbank.shape[0]), gate_logits[p]) for p in range(logits.shape[0])]

    def track_raw_programmes(self, raw_frames: torch.Tensor, raw_wave: torch.Tensor, ingest, seg_chunk: Optional[int] = None, win_chunk: int = 256) -> List[OffsetTrack]:
        """track_raw for the audio programmes of one recording: `ingest` an ingest.RecordingIngest with programmes, raw_wave its multi-channel wave
        ((ch, n), or (n, ch) interleaved; fp32, int16 or int32) -> one OffsetTrack per programme, in the order of ingest.programmes, each identical in every field
        to track_raw on that programme alone.  The frames are resized once and cross the visual tower once; the audio tower runs once per programme."""
        if getattr(ingest, 'programmes', None) is None:
            raise ValueError('track_raw_programmes: the ingest has no programmes (RecordingIngest(..., audio_channels=, programmes=[...])): use track_raw')
        ingest._check_frames(raw_frames)
        waves = ingest.waves(raw_wave)
        banks = self.eng.extract_recording_programmes_from(lambda f0, f1: ingest.frames(raw_frames, f0, f1), ingest.n_frames(raw_frames.shape[0]), waves, self.mel,
                                                           seg_chunk)
        return self.track_features_programmes(*banks, win_chunk=win_chunk)

    def track(self, frames: torch.Tensor, wave: torch.Tensor, seg_chunk: Optional[int] = None, win_chunk: int = 256) -> OffsetTrack:
        """frames (T, 3, 224, 224) uint8, wave (n,) fp32 16 kHz, on the device or in host memory -> OffsetTrack; ValueError below one window (120 frames,
        76800 samples)."""
        return self.track_features(*self.eng.extract_recording(frames, wave, self.mel, seg_chunk), win_chunk=win_chunk)

    def track_raw(self, raw_frames: torch.Tensor, raw_wave: torch.Tensor, ingest, seg_chunk: Optional[int] = None, win_chunk: int = 256) -> OffsetTrack:
        """The recording as a decoder hands it out: raw_frames uint8 (T, 3, H, W) or channels-last (T, H, W, 3) at the native frame rate and
        size, raw_wave fp32 or int16 (n,) / (ch, n) at the native rate, device or host; `ingest` an ingest.RecordingIngest of that geometry -> OffsetTrack.
        Each tower chunk's 25 fps, 224 x 224 frames are made from the raw ones right before the chunk runs; the resized recording is never materialised.
        ValueError below one window after conversion, or when the frames do not have the ingest's size, or for an ingest with programmes (track_raw_programmes)."""
        if getattr(ingest, 'programmes', None) is not None:
            raise ValueError(f'track_raw: the ingest has {len(ingest.programmes)} audio programmes, one track cannot hold them: use track_raw_programmes')
        ingest._check_frames(raw_frames)
        wave = ingest.wave(raw_wave)
        banks = self.eng.extract_recording_from(lambda f0, f1: ingest.frames(raw_frames, f0, f1), ingest.n_frames(raw_frames.shape[0]), wave, self.mel, seg_chunk)
        return self.track_features(*banks, win_chunk=win_chunk)

    def stream(self, lag: int = 16, seg_chunk: Optional[int] = None, ingest=None, gated: Optional[bool] = None):
        """A live feed: push frames and samples as they arrive, get per push the windows that became final.  lag: window w is committed once
        `lag` more windows have arrived (0 .. 255), as the class of w on the Viterbi path of everything up to window w + lag - a decision delay of
        lag * hop * 0.32 s.  lag = 16 is a DEFAULT, NOT A TUNED VALUE (as lam): how far back a later window still changes the decision depends on lam and on
        the domain's logits; choose it on held-out recordings.  lag >= the number of windows gives the offline path at flush().  seg_chunk: as in track().
        ingest: an ingest.RecordingIngest - push then takes frames and samples as decoded (native frame rate, size, sample rate; track_raw's layouts).  An ingest
        with programmes gives a ProgrammeStream: push / flush return one OffsetUpdate per programme.
        gated, on a tracker with a gate: True reads the feed out over (offset class, synchronizable flag) - the committed windows are those of the gated
        offline read-out of the prefix 0 .. w + lag, and every OffsetUpdate carries gate_logits, sync_raw, sync_lag, sync_tail (p_sync_lag with the posterior);
        False gives the stream of a tracker without a gate; None (the default) raises NotImplementedError: the choice is explicit.  On a tracker without a gate
        gated=True is a ValueError."""
        gated = self._gate_choice('stream', gated)
        if getattr(ingest, 'programmes', None) is not None:
            return ProgrammeStream(self, lag, seg_chunk, ingest, gated=gated)
        return OffsetStream(self, lag, seg_chunk, ingest, gated=gated)

    def pool(self, n_feeds: int, lag: int = 16, seg_chunk: Optional[int] = None, gated: Optional[bool] = None) -> 'OffsetStreamPool':
        """Up to `n_feeds` live feeds at once: each feed is what stream(lag, seg_chunk) is, but one push() advances all named feeds together - their
        new segments share the towers' launch groups, their new windows the sync transformer's passes, their read-outs one ops.track_pool_push.  gated: as stream()'s
        (True: the gate's 13-segment windows cross its sync transformer in passes of their own, the read-out is one ops.track_pool_push_gated)."""
        return OffsetStreamPool(self, n_feeds, lag, seg_chunk, gated=self._gate_choice('pool', gated))

    def _gate_choice(self, who: str, gated: Optional[bool]) -> bool:
        """Whether a live read-out runs through the gate: an explicit choice on a tracker that has one."""
        if self.gate is None:
            if gated:
                raise ValueError(f'OffsetTracker.{who}(gated=True): the tracker has no gate (OffsetTracker(..., gate=<an engine with the syncability head>))')
            return False
        if gated is None:
            raise NotImplementedError(f'OffsetTracker.{who}: this tracker has a gate, and the offline read-out of DESIGN 3.20 does not decide how a live feed is read: '
                                      f'pass gated=True for the fixed-lag read-out over (offset class, synchronizable flag) (DESIGN 3.21, a carried state 2C wide) or '
                                      f'gated=False for the one a tracker without a gate gives')
        return bool(gated)


@dataclass
class OffsetUpdate:
    """What one push (or the flush) of an OffsetStream adds; tensors on the engine's device, times float64 on the host."""
    # the windows this push completed (n of them, from window w_new)
    w_new: int
    logits: torch.Tensor             # (n, C) fp32
    cls_raw: torch.Tensor            # (n,) int32: per-window argmax
    conf_raw: torch.Tensor           # (n,) fp32
    # the committed block: windows w0 .. w0 + k - 1, final - a later push never revises them
    w0: int
    t_sec: torch.Tensor              # (k,) float64: window centres at the absolute window index
    cls_lag: torch.Tensor            # (k,) int32: the class of window w on the Viterbi path of windows 0 .. w + lag
    conf_lag: torch.Tensor           # (k,) fp32: its softmax probability in window w
    offset_sec_lag: torch.Tensor     # (k,) fp32: grid[cls_lag]
    # the tail: the windows not yet committed, on the path of everything so far; [-1] is the current offset and may change with the next push
    t_sec_tail: torch.Tensor         # (m,) float64
    cls_tail: torch.Tensor           # (m,) int32
    conf_tail: torch.Tensor          # (m,) fp32
    offset_sec_tail: torch.Tensor    # (m,) fp32
    # OffsetTracker(posterior=True): the marginals of the committed windows given windows 0 .. w + lag; None without it
    post_lag: Optional[torch.Tensor] = None            # (k, C) fp32
    cls_post_lag: Optional[torch.Tensor] = None        # (k,) int32
    conf_post_lag: Optional[torch.Tensor] = None       # (k,) fp32
    offset_sec_post_lag: Optional[torch.Tensor] = None  # (k,) fp32: grid[cls_post_lag]
    offset_sec_mean_lag: Optional[torch.Tensor] = None  # (k,) fp32
    log_z: Optional[torch.Tensor] = None               # (1,) fp32: that of all the windows so far
    # the gate (stream / pool with gated=True); None without it.  Optional attributes set by the feed and deliberately NOT dataclass fields, as
    # OffsetTrack's: the field list and the positional constructor above stay what they were.  cls_lag, conf_lag, cls_tail, the posterior fields then come from the
    # chain over (offset class, synchronizable flag)
    gate_logits = None               # (n, 2) fp32: the syncability head on the new windows' first gate.n_window segments
    sync_raw = None                  # (n,) fp32: sigmoid(z1 - z0)
    sync_lag = None                  # (k,) int32: the flag of the committed windows, 1 = synchronizable (0: nothing to read here)
    sync_tail = None                 # (m,) int32: the flag along the tail
    p_sync_lag = None                # (k,) fp32: the flag's marginal given windows 0 .. w + lag (with posterior=True)


def pool_schedule(feeds, hop: int = 1, seg_chunk: int = 224, win_chunk: int = 256) -> dict:
    """The host schedule of one pool tick (OffsetStreamPool.push), pure arithmetic.  feeds: one dict per feed taking part, in feed order, AFTER its new frames and
    samples were accepted: n_frames, n_samples (totals so far), n_segments (segments already through the towers), f0, a0, s0 (the recording's index of the first held
    frame / sample / segment feature) ->
        geometry   per feed: stream_geometry(n_frames, n_samples, n_segments, hop) - each feed's own, nothing is shared
        segments   the staging order of the towers: (feed, s, frame_lo, sample_lo) for every new segment of every feed, feeds in order, s ascending; frame_lo /
                   sample_lo index the feed's HELD buffers (v_stride s - f0, a_stride s - a0)
        groups     (i0, i1) ranges of `segments`: launch groups of at most seg_chunk segments, whatever feed they come from
        windows    the gather order of the sync transformer: (feed, w, feat_lo) for every new window, feat_lo = hop w - s0 indexing the held features (after the new
                   segments were appended); passes = (i0, i1) ranges of at most win_chunk windows
        counts     per feed: its new windows (the rows it brings to ops.track_pool_push)
        trims      per feed: (frames_from, samples_from, features_from) of its geometry"""
    if seg_chunk < 1 or win_chunk < 1:
        raise ValueError(f'pool_schedule: seg_chunk = {seg_chunk}, win_chunk = {win_chunk}')
    geometry, segments, windows, counts, trims = [], [], [], [], []
    for i, f in enumerate(feeds):
        g = stream_geometry(f['n_frames'], f['n_samples'], f['n_segments'], hop)
        (s0, s1), (w0, w1) = g['new_segments'], g['new_windows']
        geometry.append(g)
        segments += [(i, s, g['v_stride'] * s - f['f0'], g['a_stride'] * s - f['a0']) for s in range(s0, s1)]
        windows += [(i, w, hop * w - f['s0']) for w in range(w0, w1)]
        counts.append(w1 - w0)
        trims.append((g['frames_from'], g['samples_from'], g['features_from']))
    groups = [(i0, min(i0 + seg_chunk, len(segments))) for i0 in range(0, len(segments), seg_chunk)]
    passes = [(i0, min(i0 + win_chunk, len(windows))) for i0 in range(0, len(windows), win_chunk)]
    return dict(geometry=geometry, segments=segments, groups=groups, windows=windows, passes=passes, counts=counts, trims=trims)


class _Feed:
    """What one live feed carries on the host and the steps of one advance - accept, (towers), (windows), (read-out), trim, update - shared by OffsetStream (one feed,
    its own launches) and OffsetStreamPool (many feeds, the three device steps batched across them)."""

    def __init__(self, tracker: 'OffsetTracker', ingest=None, gated: bool = False):
        if gated and tracker.gate is None:
            raise ValueError('a gated feed needs a tracker with a gate')
        self.tracker, self.gated = tracker, bool(gated)
        dev = tracker.eng.dev
        self._ingest = None if ingest is None else ingest.stream()
        self._frames = torch.empty(0, 3, 224, 224, device=dev, dtype=torch.uint8)
        self._wave = torch.empty(0, device=dev, dtype=torch.float32)
        self._vfeat = self._afeat = None
        self.n_frames = self.n_samples = self.n_segments = self.n_windows = 0    # totals so far
        self._f0 = self._a0 = self._s0 = 0                                       # the recording's index of the first held frame / sample / segment
        self.closed = False

    def _state_bytes(self) -> int:
        raise NotImplementedError

    @property
    def held(self) -> dict:
        """The sizes of the carried buffers: frames, samples, segments (features) and state_bytes."""
        return dict(frames=int(self._frames.shape[0]), samples=int(self._wave.numel()), segments=0 if self._vfeat is None else int(self._vfeat.shape[0]),
                    state_bytes=self._state_bytes())

    @property
    def held_bound(self) -> dict:
        """The bound on `held` after a push, from the totals so far (see the class docstring; one push's own frames and samples pass through on top of it)."""
        g = recording_geometry(self.n_frames, self.n_samples, self.tracker.hop)
        nv = max(0, (self.n_frames - g['v_size']) // g['v_stride'] + 1)
        na = max(0, (self.n_samples - g['a_size']) // g['a_stride'] + 1)
        return dict(frames=g['v_size'] - 1 + g['v_stride'] * (nv - g['n_segments']), samples=g['a_size'] - 1 + g['a_stride'] * (na - g['n_segments']),
                    segments=g['n_window'] - 1 + self.tracker.hop - 1, state_bytes=self._state_bytes())

    def _empty_input(self):
        dev = self.tracker.eng.dev
        return torch.empty(0, 3, 224, 224, device=dev, dtype=torch.uint8), torch.empty(0, device=dev, dtype=torch.float32)

    def _accept(self, frames: torch.Tensor, wave: torch.Tensor, who: str = 'OffsetStream.push'):
        """Appends what arrived (25 fps, 224 x 224, 16 kHz: after the ingest) to the held frames and samples and counts it."""
        eng = self.tracker.eng
        if frames.dim() != 4 or frames.dtype != torch.uint8 or tuple(frames.shape[1:]) != (3, 224, 224) or wave.shape[:-1] != self._wave.shape[:-1]:
            raise ValueError(f'{who}: expected uint8 frames (t, 3, 224, 224) and a {"1-D wave" if self._wave.dim() == 1 else f"wave ({self._wave.shape[0]}, m)"}, got '
                             f'{frames.dtype} {tuple(frames.shape)} / {tuple(wave.shape)}')
        if frames.shape[0]:
            self._frames = torch.cat([self._frames, frames.to(eng.dev, non_blocking=True)])
        if wave.shape[-1]:                                                       # (the samples are the last axis: a ProgrammeStream holds P rows of them)
            self._wave = torch.cat([self._wave, wave.to(eng.dev, torch.float32, non_blocking=True)], -1)
        self.n_frames += int(frames.shape[0])
        self.n_samples += int(wave.shape[-1])

    def _add_features(self, vf: torch.Tensor, af: torch.Tensor):
        self._vfeat = vf if self._vfeat is None else torch.cat([self._vfeat, vf])
        self._afeat = af if self._afeat is None else torch.cat([self._afeat, af])

    def _trim(self, g: dict):
        """Drops what no later segment / window reads and moves the totals on (g: this advance's stream_geometry)."""
        self._frames, self._f0 = self._frames[g['frames_from'] - self._f0:], g['frames_from']
        self._wave, self._a0 = self._wave[..., g['samples_from'] - self._a0:], g['samples_from']
        if self._vfeat is not None:
            k = g['features_from'] - self._s0
            self._vfeat, self._afeat, self._s0 = self._vfeat[k:], self._afeat[k:], g['features_from']
        self.n_segments, self.n_windows = g['new_segments'][1], g['new_windows'][1]

    def _update(self, out, logits: torch.Tensor, w0: int, w1: int, gate_logits: Optional[torch.Tensor] = None) -> 'OffsetUpdate':
        """The read-out of this advance (an ops.TrackStreamOut, or TrackGatedStreamOut with the gate's logits of the same windows) and its logits (windows
        w0 .. w1 - 1) -> OffsetUpdate."""
        tr = self.tracker
        k, m = out.cls_lag.shape[0], out.cls_tail.shape[0]
        upd = OffsetUpdate(w_new=w0, logits=logits, cls_raw=out.cls_raw, conf_raw=out.conf_raw, w0=out.w0, t_sec=window_times64(k, tr.hop, first_window=out.w0),
                           cls_lag=out.cls_lag, conf_lag=out.conf_lag, offset_sec_lag=tr.grid[out.cls_lag.long()],
                           t_sec_tail=window_times64(m, tr.hop, first_window=w1 - m), cls_tail=out.cls_tail, conf_tail=out.conf_tail,
                           offset_sec_tail=tr.grid[out.cls_tail.long()])
        if tr.posterior:
            upd.post_lag, upd.cls_post_lag, upd.conf_post_lag, upd.offset_sec_mean_lag, upd.log_z = (out.post_lag, out.cls_post_lag, out.conf_post_lag,
                                                                                                       out.offset_mean_lag, out.log_z)
            upd.offset_sec_post_lag = tr.grid[out.cls_post_lag.long()]
        if self.gated:
            upd.gate_logits, upd.sync_raw, upd.sync_lag, upd.sync_tail, upd.p_sync_lag = gate_logits, out.sync_raw, out.sync_lag, out.sync_tail, out.p_sync_lag
        return upd


class _Stream(_Feed):
    """A feed with launches of its own: the bodies of push() and flush() around the subclass's _advance(frames, wave, final); `who` is the class named in the
    messages.  (A PoolFeed has neither: its pool advances it.)"""

    def _push(self, who: str, frames: torch.Tensor, wave: torch.Tensor):
        if self.closed:
            raise RuntimeError(f'{who}.push: the stream was closed by flush()')
        if self._ingest is not None:
            frames, wave = self._ingest.push(frames, wave)
        return self._advance(frames, wave, final=False)

    def _flush(self, who: str):
        if self.closed:
            raise RuntimeError(f'{who}.flush: the stream is closed')
        upd = self._advance(*(self._empty_input() if self._ingest is None else self._ingest.flush()), final=True)
        self.closed = True
        return upd


class OffsetStream(_Stream):
    """OffsetTracker.stream(): the recording path for a feed that does not end.  push() takes what arrived - uint8 frames (t, 3, 224, 224) at 25 fps and fp32
    samples (m,) at 16 kHz, device or host, either possibly empty, the two at their own pace (with `ingest`: as decoded) - runs the towers on the segments that
    became complete, the sync transformer on the windows that became complete (engine.sync_windows on the held features: 13 old segments and n new ones give
    exactly the n new windows) and the fixed-lag read-out (ops.track_stream_push).  What the stream carries is bounded, whatever has passed (`held`):
        frames   from 8 N on (N = segments done): at most 15, plus what the video is ahead of the audio, plus one push
        samples  from 5120 N on: at most 10239, plus what the audio is ahead of the video, plus one push
        segment features from the next window's first segment on: at most 13 + hop - 1
        the read-out state: ops.track_stream_state's bytes (gated: ops.track_stream_state_gated's)
    With gated=True the gate's logits of the same n new windows come from the same held features (gate.sync_windows with n_window = gate.n_window,
    start-aligned, the first n rows: what track_features does offline) and the read-out is ops.track_stream_push_gated.
    The segment grid is the recording's (anchored at frame 0), so the windows, their logits (bit for bit where the tower schedule is position-independent: the
    un-fused one) and t_sec are those track() gives for the finished recording."""

    def __init__(self, tracker: OffsetTracker, lag: int = 16, seg_chunk: Optional[int] = None, ingest=None, gated: bool = False):
        super().__init__(tracker, ingest, gated)
        self.lag, self.seg_chunk = int(lag), seg_chunk
        self.state = (ops.track_stream_state_gated if self.gated else ops.track_stream_state)(tracker.eng.n_out, self.lag, tracker.posterior, tracker.eng.dev)

    def _state_bytes(self) -> int:
        return int(self.state.buf.numel())

    def push(self, frames: torch.Tensor, wave: torch.Tensor) -> OffsetUpdate:
        return self._push('OffsetStream', frames, wave)

    def flush(self) -> OffsetUpdate:
        """End of the feed: whatever the ingest still held becomes final, the tail is committed from everything pushed, the stream closes (a later push raises)."""
        return self._flush('OffsetStream')

    def _advance(self, frames: torch.Tensor, wave: torch.Tensor, final: bool) -> OffsetUpdate:
        tr, eng = self.tracker, self.tracker.eng
        self._accept(frames, wave)
        g = stream_geometry(self.n_frames, self.n_samples, self.n_segments, tr.hop)
        (s0, s1), (w0, w1) = g['new_segments'], g['new_windows']
        if s1 > s0:                                                              # the towers, on the segments this push completed
            self._add_features(*eng.extract_segments_from(lambda f0, f1: self._frames[f0 - self._f0:f1 - self._f0], self._wave, tr.mel, s0, s1 - s0, self.seg_chunk,
                                                          sample0=self._a0))
        if w1 > w0:                                                              # the windows whose last segment arrived: the held features hold exactly these
            lo = tr.hop * w0 - self._s0
            logits = eng.sync_windows(self._vfeat[lo:], self._afeat[lo:], hop=tr.hop)
            assert logits.shape[0] == w1 - w0, (logits.shape, w0, w1)
        else:
            logits = torch.empty(0, eng.n_out, device=eng.dev, dtype=torch.float32)
        gate_logits = None
        if self.gated:
            gate = tr.gate
            if w1 > w0:                                                          # start-aligned windows of the gate's own length: exactly the n new rows
                gate_logits = gate.sync_windows(self._vfeat[lo:], self._afeat[lo:], hop=tr.hop, n_window=gate.n_window)[:w1 - w0]
            else:
                gate_logits = torch.empty(0, 2, device=eng.dev, dtype=torch.float32)
            out = ops.track_stream_push_gated(self.state, logits, gate_logits, tr.lam, tr.mu, tr.grid if tr.posterior else None, final=final)
        else:
            out = ops.track_stream_push(self.state, logits, tr.lam, tr.grid if tr.posterior else None, final=final)
        self._trim(g)
        return self._update(out, logits, w0, w1, gate_logits)


class ProgrammeStream(_Stream):
    """OffsetTracker.stream(ingest=<an ingest with programmes>): OffsetStream for the P audio programmes of one feed.  push(raw_frames, raw_wave) and
    flush() return one OffsetUpdate per programme, in the order of ingest.programmes; each is what a plain OffsetStream fed that programme's channels returns,
    field for field (bit for bit on the un-fused tower schedule).  The picture is resized once and crosses the visual tower once per segment; the stream holds ONE
    set of frames and ONE visual feature buffer, P wave rows and P audio feature buffers, and one ops.track_pool_state(P, ..) advanced by one ops.track_pool_push
    per push.  The host arithmetic is _Feed's.  The bound on `held` is OffsetStream's with the audio entries scaled by P:
        frames          at most 15, plus what the video is ahead of the audio, plus one push
        samples         P x (at most 10239, plus what the audio is ahead of the video, plus one push)
        segments        visual features: at most 13 + hop - 1
        audio_segments  P x segments
        state_bytes     P x ops.track_stream_state's bytes"""

    def __init__(self, tracker: OffsetTracker, lag: int = 16, seg_chunk: Optional[int] = None, ingest=None, gated: bool = False):
        if getattr(ingest, 'programmes', None) is None:
            raise ValueError('ProgrammeStream: an ingest with programmes is required (RecordingIngest(..., audio_channels=, programmes=[...]))')
        super().__init__(tracker, ingest, gated)
        self.P = len(ingest.programmes)
        self.lag, self.seg_chunk = int(lag), seg_chunk
        self._wave = torch.empty(self.P, 0, device=tracker.eng.dev, dtype=torch.float32)
        self.state = (ops.track_pool_state_gated if self.gated else ops.track_pool_state)(self.P, tracker.eng.n_out, self.lag, tracker.posterior, tracker.eng.dev)

    def _state_bytes(self) -> int:
        return int(self.state.buf.numel())

    @property
    def held(self) -> dict:
        h = super().held                                                         # (samples: the elements of the (P, m) wave rows)
        h['audio_segments'] = self.P * h['segments']
        return h

    @property
    def held_bound(self) -> dict:
        b = super().held_bound
        b['samples'], b['audio_segments'] = self.P * b['samples'], self.P * b['segments']
        return b

    def push(self, frames: torch.Tensor, wave: torch.Tensor) -> List[OffsetUpdate]:
        return self._push('ProgrammeStream', frames, wave)

    def flush(self) -> List[OffsetUpdate]:
        """End of the feed: what the ingest still held becomes final, every programme's tail is committed, the stream closes (a later push raises)."""
        return self._flush('ProgrammeStream')

    def _advance(self, frames: torch.Tensor, waves: torch.Tensor, final: bool) -> List[OffsetUpdate]:
        tr, eng, P = self.tracker, self.tracker.eng, self.P
        self._accept(frames, waves, 'ProgrammeStream.push')
        g = stream_geometry(self.n_frames, self.n_samples, self.n_segments, tr.hop)
        (s0, s1), (w0, w1) = g['new_segments'], g['new_windows']
        if s1 > s0:                                                              # the towers: the picture once, the audio once per programme
            vf, af = eng.extract_segments_programmes_from(lambda f0, f1: self._frames[f0 - self._f0:f1 - self._f0], self._wave, tr.mel, s0, s1 - s0, self.seg_chunk,
                                                          sample0=self._a0)
            self._add_features(vf, af.transpose(0, 1))                           # held audio features: (segments, P, 6, 768), trimmed along the segments
        if w1 > w0:
            lo = tr.hop * w0 - self._s0
            logits = eng.sync_windows_programmes(self._vfeat[lo:], self._afeat[lo:].transpose(0, 1), hop=tr.hop)
            assert logits.shape[:2] == (P, w1 - w0), (logits.shape, w0, w1)
        else:
            logits = torch.empty(P, 0, eng.n_out, device=eng.dev, dtype=torch.float32)
        slots = list(range(P))
        gate_logits = [None] * P
        if self.gated:
            gate = tr.gate
            if w1 > w0:
                gate_logits = gate.sync_windows_programmes(self._vfeat[lo:], self._afeat[lo:].transpose(0, 1), hop=tr.hop, n_window=gate.n_window)[:, :w1 - w0].contiguous()
            else:
                gate_logits = torch.empty(P, 0, 2, device=eng.dev, dtype=torch.float32)
            outs = ops.track_pool_push_gated(self.state, slots, logits.reshape(P * (w1 - w0), eng.n_out), gate_logits.reshape(P * (w1 - w0), 2), [w1 - w0] * P, tr.lam,
                                             tr.mu, tr.grid if tr.posterior else None, final=slots if final else ())
        else:
            outs = ops.track_pool_push(self.state, slots, logits.reshape(P * (w1 - w0), eng.n_out), [w1 - w0] * P, tr.lam, tr.grid if tr.posterior else None,
                                       final=slots if final else ())
        self._trim(g)
        return [self._update(out, logits[p], w0, w1, gate_logits[p]) for p, out in enumerate(outs)]


class PoolFeed(_Feed):
    """One feed of an OffsetStreamPool (pool.open()): the handle push() is keyed by.  `held` / `held_bound` / the totals as an OffsetStream's."""

    def __init__(self, pool: 'OffsetStreamPool', slot: int, ingest=None):
        super().__init__(pool.tracker, ingest, pool.gated)
        self.pool, self.slot = pool, slot

    def _state_bytes(self) -> int:
        return int(self.pool.state.buf.shape[1])


class OffsetStreamPool:
    """OffsetTracker.pool(): many live feeds on one device, advanced together.  open() takes a free slot and returns the feed's handle; one push() is
    one tick: every feed named in it accepts what arrived for it (through its own ingest, if it has one), then
        towers    the new segments of all feeds, in feed order, are gathered into staging tensors (n, 16, 3, 224, 224) / (n, 10240) and cross the towers as n
                  one-segment clips, in launch groups of at most seg_chunk segments, whatever feed they come from;
        windows   the new windows of all feeds are gathered from the held features into (nw, 14, t, 768) and cross the sync transformer in passes of at most
                  win_chunk = 256;
        read-out  one ops.track_pool_push for all feeds (gated=True, DESIGN 3.21: the windows' first gate.n_window segments are gathered as well and cross the
                  gate's sync transformer in the same passes; one ops.track_pool_push_gated);
    and every feed trims its buffers as its own stream would.  Per feed the host arithmetic is OffsetStream's (the same code), `held <= held_bound` holds per
    feed, and on the un-fused tower schedule (the engine's seg_chunk < 6) every field of every update equals the same feed through its own OffsetStream bit for
    bit.  A feed named in `flush` gets its final push in that tick (with or without data) and its slot becomes free; feeds not named are untouched."""

    def __init__(self, tracker: OffsetTracker, n_feeds: int, lag: int = 16, seg_chunk: Optional[int] = None, win_chunk: int = 256, gated: bool = False):
        if n_feeds < 1:
            raise ValueError(f'OffsetStreamPool: n_feeds = {n_feeds}')
        if gated and tracker.gate is None:
            raise ValueError('OffsetStreamPool: gated=True needs a tracker with a gate')
        self.tracker, self.n_feeds, self.lag, self.seg_chunk, self.win_chunk, self.gated = tracker, int(n_feeds), int(lag), seg_chunk, int(win_chunk), bool(gated)
        self.state = (ops.track_pool_state_gated if self.gated else ops.track_pool_state)(self.n_feeds, tracker.eng.n_out, self.lag, tracker.posterior, tracker.eng.dev)
        self._free = list(range(self.n_feeds - 1, -1, -1))                       # slot 0 first
        self.feeds = {}                                                          # slot -> the open feed

    def open(self, ingest=None) -> PoolFeed:
        """A new feed in a free slot (ingest: an ingest.RecordingIngest, as OffsetTracker.stream's); RuntimeError when every slot is taken; ValueError for an ingest
        with programmes."""
        if getattr(ingest, 'programmes', None) is not None:
            raise ValueError('OffsetStreamPool.open: an ingest with audio programmes is not served by a pool (one feed with several read-out slots is out of '
                             'scope): use OffsetTracker.stream(ingest=...) for that feed')
        if not self._free:
            raise RuntimeError(f'OffsetStreamPool.open: all {self.n_feeds} slots are taken (flush a feed first)')
        slot = self._free.pop()
        self.state.reopen(slot)
        feed = self.feeds[slot] = PoolFeed(self, slot, ingest)
        return feed

    def push(self, data: dict, flush=()) -> dict:
        """One tick.  data: {feed: (frames, wave)} - what arrived for each feed since its last push (OffsetStream.push's inputs); flush: feeds that end in this
        tick -> {feed: OffsetUpdate}, for every feed named in either."""
        tr, eng = self.tracker, self.tracker.eng
        flush = list(flush)
        feeds = list(data) + [f for f in flush if f not in data]
        if len(set(feeds)) != len(feeds) or len(set(flush)) != len(flush):
            raise ValueError('OffsetStreamPool.push: a feed named twice')
        for f in feeds:
            if not isinstance(f, PoolFeed) or f.pool is not self:
                raise ValueError('OffsetStreamPool.push: not a feed of this pool')
            if f.closed:
                raise RuntimeError(f'OffsetStreamPool.push: the feed in slot {f.slot} was closed by a flush')
        if not feeds:
            return {}
        # accept: per feed, through its own ingest
        for f in feeds:
            frames, wave = data[f] if f in data else f._empty_input()
            if f._ingest is not None:
                parts = ([f._ingest.push(frames, wave)] if f in data else []) + ([f._ingest.flush()] if f in flush else [])
                frames, wave = (parts[0] if len(parts) == 1 else (torch.cat([p[0].to(eng.dev) for p in parts]), torch.cat([p[1].to(eng.dev) for p in parts])))
            f._accept(frames, wave, 'OffsetStreamPool.push')
        chunk = eng.seg_chunk if self.seg_chunk is None else int(self.seg_chunk)
        plan = pool_schedule([dict(n_frames=f.n_frames, n_samples=f.n_samples, n_segments=f.n_segments, f0=f._f0, a0=f._a0, s0=f._s0) for f in feeds], tr.hop, chunk,
                             self.win_chunk)
        # towers: launch groups over the new segments of all feeds
        if plan['segments']:
            g0 = plan['geometry'][0]
            vz, vs, az, as_ = g0['v_size'], g0['v_stride'], g0['a_size'], g0['a_stride']
            new_v, new_a = [[] for _ in feeds], [[] for _ in feeds]
            for i0, i1 in plan['groups']:
                n = i1 - i0
                fst = torch.empty(n, vz, 3, 224, 224, device=eng.dev, dtype=torch.uint8)
                wst = torch.empty(n, az, device=eng.dev, dtype=torch.float32)
                for j, (i, _, flo, alo) in enumerate(plan['segments'][i0:i1]):
                    fst[j].copy_(feeds[i]._frames[flo:flo + vz])
                    wst[j].copy_(feeds[i]._wave[alo:alo + az])
                aud = tr.mel.segments(wst, 0, as_, 1, az)
                vf, af = eng.both_towers(lambda: eng.extract_vfeats_clips(fst, 0, vs, 1), aud)
                for j, (i, _, _, _) in enumerate(plan['segments'][i0:i1]):
                    new_v[i].append(vf[j])
                    new_a[i].append(af[j])
            for f, v, a in zip(feeds, new_v, new_a):
                if v:
                    f._add_features(torch.cat(v), torch.cat(a))
        # windows: gathered from the held features of all feeds
        nw = len(plan['windows'])
        logits = torch.empty(nw, eng.n_out, device=eng.dev, dtype=torch.float32)
        gate_logits = torch.empty(nw, 2, device=eng.dev, dtype=torch.float32) if self.gated else None
        if nw:
            nwin = plan['geometry'][0]['n_window']
            for i0, i1 in plan['passes']:
                vwin = torch.stack([feeds[i]._vfeat[lo:lo + nwin] for i, _, lo in plan['windows'][i0:i1]])
                awin = torch.stack([feeds[i]._afeat[lo:lo + nwin] for i, _, lo in plan['windows'][i0:i1]])
                logits[i0:i1].copy_(eng.sync_transformer(vwin, awin))
                if self.gated:                                                   # the gate's start-aligned windows: the first gate.n_window segments of the same gather
                    gate_logits[i0:i1].copy_(tr.gate.sync_transformer(vwin[:, :tr.gate.n_window].contiguous(), awin[:, :tr.gate.n_window].contiguous()))
        # read-out: one call for all feeds
        if self.gated:
            outs = ops.track_pool_push_gated(self.state, [f.slot for f in feeds], logits, gate_logits, plan['counts'], tr.lam, tr.mu,
                                             tr.grid if tr.posterior else None, final=[f.slot for f in flush])
        else:
            outs = ops.track_pool_push(self.state, [f.slot for f in feeds], logits, plan['counts'], tr.lam, tr.grid if tr.posterior else None,
                                       final=[f.slot for f in flush])
        res, row = {}, 0
        for f, g, n, out in zip(feeds, plan['geometry'], plan['counts'], outs):
            f._trim(g)
            res[f] = f._update(out, logits[row:row + n], g['new_windows'][0], g['new_windows'][1], gate_logits[row:row + n] if self.gated else None)
            row += n
        for f in flush:
            f.closed = True
            del self.feeds[f.slot]
            self._free.append(f.slot)
        return res


# ---- fitting lam and mu on labelled recordings ---------------------------------------------------------------------------------------------------------
@dataclass
class SmoothnessFit:
    """What fit_smoothness found.  J = sum_w |c_{w+1} - c_w| (class steps), F = the number of changes of the synchronizable flag, summed over the recordings."""
    lam: float
    mu: Optional[float]              # None for the plain chain
    lam_at_bound: bool               # the likelihood still rises at 0 or at lam_max: lam is that bound, not a maximum (labels that never change: lam_max)
    mu_at_bound: bool
    jumps_observed: float            # J* of the labels
    jumps_expected: float            # E[J] under the chain at the fit; equal to J* at an interior maximum
    flips_observed: float            # F* (0 for the plain chain)
    flips_expected: float
    log_likelihood: float            # sum_r (score of the labelled path - log_z) at the fit, <= 0
    se_lam: float                    # 1 / sqrt(-d E[J] / d lam) by a central difference at the fit (the curvature of the log-likelihood along lam); inf when flat
    se_mu: Optional[float]
    evaluations: int                 # calls of `stats` per recording

    @property
    def at_bound(self) -> bool:
        return self.lam_at_bound or self.mu_at_bound


def _device_stats(logits, gate_logits, lam: float, mu: float):
    """fit_smoothness's default `stats`: the pairwise read-out on the device, summed in float64 on the host."""
    if gate_logits is None:
        out = ops.track_pairwise(logits, lam)
        return float(out[1].double().sum().item()), 0.0, float(out[6].item())
    out = ops.track_pairwise_gated(logits, gate_logits, lam, mu)
    return float(out[1].double().sum().item()), float(out[2].double().sum().item()), float(out[7].item())


def _host64(x) -> torch.Tensor:
    return (x.detach().cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(x)).double()


def _bisect_decreasing(g, hi: float, iters: int):
    """The root of a decreasing g on [0, hi] by `iters` halvings -> (x, at_bound): 0 when g(0) <= 0, hi when g(hi) >= 0, both with at_bound."""
    if g(0.0) <= 0:
        return 0.0, True
    if g(hi) >= 0:
        return float(hi), True
    lo = 0.0
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        if g(mid) > 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi), False


def fit_smoothness(recordings, gated: bool = False, lam_max: float = 16.0, mu_max: float = 16.0, iters: int = 30, sweeps: int = 4, stats=None) -> SmoothnessFit:
    """Fit OffsetTracker's lam (gated: and mu) on labelled recordings by maximum conditional likelihood.
    recordings: a list of (logits (W, C) fp32, labels (W,) int) - the window logits of a recording (OffsetTrack.logits) and the true class of every window; with
    gated=True each item is (logits, labels, gate_logits (W, 2), sync_labels (W,) in {0, 1}).  The class label is required in every window: for an in-sync recording
    whose audio was shifted by a known amount it is known whether or not the window is synchronizable.
    The chain is a conditional random field, p(path | logits) ~ exp(sum e - lam J - mu F); its log-likelihood sum_r (score of the labels - log_z) is concave in
    (lam, mu) with the gradient (E[J] - J*, E[F] - F*), and the expectations are the sums of jump_abs / p_flip of the pairwise read-out.  Plain chain: `iters`
    halvings of [0, lam_max] on E[J] - J*, which decreases in lam.  Gated: `sweeps` rounds of that for lam at fixed mu, then for mu on E[F] - F* at fixed lam
    (coordinate ascent, from mu = min(2, mu_max)).  A parameter whose gradient does not change sign inside its interval ends at the bound, flagged.
    stats(logits, gate_logits or None, lam, mu) -> (sum_w jump_abs, sum_w p_flip, log_z): by default ops.track_pairwise(_gated) on the device the logits lie on,
    summed in float64; anything with the same contract serves (the tests pass a float64 oracle and run this function without a GPU).
    ValueError for no recordings, mismatched lengths, or labels outside [0, C) / {0, 1}."""
    stats = _device_stats if stats is None else stats
    if not (lam_max > 0 and mu_max > 0 and iters >= 1 and sweeps >= 1):
        raise ValueError(f'fit_smoothness: lam_max = {lam_max}, mu_max = {mu_max}, iters = {iters}, sweeps = {sweeps}')
    recs, j_obs, f_obs, emit = [], 0.0, 0.0, 0.0
    for r, item in enumerate(recordings):
        if len(item) != (4 if gated else 2):
            raise ValueError(f'fit_smoothness: recording {r} has {len(item)} entries, expected ' + ('(logits, labels, gate_logits, sync_labels)' if gated else '(logits, labels)'))
        logits, labels = item[0], torch.as_tensor(item[1]).detach().cpu().reshape(-1).long()
        if len(logits.shape) != 2 or labels.numel() != logits.shape[0]:
            raise ValueError(f'fit_smoothness: recording {r}: {labels.numel()} labels for logits of {tuple(logits.shape)}')
        W, C = logits.shape
        if W and (labels.min() < 0 or labels.max() >= C):
            raise ValueError(f'fit_smoothness: recording {r}: labels outside [0, {C})')
        e = torch.log_softmax(_host64(logits), 1)[torch.arange(W), labels]
        gate_logits = None
        if gated:
            gate_logits, sync = item[2], torch.as_tensor(item[3]).detach().cpu().reshape(-1).long()
            if tuple(gate_logits.shape) != (W, 2) or sync.numel() != W:
                raise ValueError(f'fit_smoothness: recording {r}: gate logits of {tuple(gate_logits.shape)} and {sync.numel()} sync labels for {W} windows')
            if W and (sync.min() < 0 or sync.max() > 1):
                raise ValueError(f'fit_smoothness: recording {r}: sync labels outside {{0, 1}}')
            z = _host64(gate_logits)
            d = z[:, 1] - z[:, 0]
            e = torch.where(sync == 1, torch.nn.functional.logsigmoid(d) + e, torch.nn.functional.logsigmoid(-d) - torch.log(torch.tensor(float(C), dtype=torch.float64)))
            f_obs += float((sync[1:] - sync[:-1]).abs().sum())
        j_obs += float((labels[1:] - labels[:-1]).abs().sum())
        emit += float(e.sum())
        if W:
            recs.append((logits, gate_logits))
    if not recs:
        raise ValueError('fit_smoothness: no recordings')
    count = [0]

    def totals(lam: float, mu: float):
        count[0] += 1
        out = [stats(l, g, float(lam), float(mu)) for l, g in recs]
        return tuple(float(sum(o[k] for o in out)) for k in range(3))

    def stderr(which: int, lam: float, mu: float, top: float):
        x = (lam, mu)[which]
        h = max(0.02 * x, 0.005)
        lo, hi = max(x - h, 0.0), min(x + h, top)
        at = (lambda v: (v, mu)) if which == 0 else (lambda v: (lam, v))
        slope = (totals(*at(hi))[which] - totals(*at(lo))[which]) / (hi - lo)
        return float('inf') if not slope < 0 else (-slope) ** -0.5

    mu, mu_bound, se_mu = (min(2.0, float(mu_max)), False, None) if gated else (0.0, False, None)
    for _ in range(sweeps if gated else 1):
        lam, lam_bound = _bisect_decreasing(lambda x: totals(x, mu)[0] - j_obs, float(lam_max), iters)
        if gated:
            mu, mu_bound = _bisect_decreasing(lambda x: totals(lam, x)[1] - f_obs, float(mu_max), iters)
    j_exp, f_exp, log_z = totals(lam, mu)
    se_lam = stderr(0, lam, mu, float(lam_max))
    if gated:
        se_mu = stderr(1, lam, mu, float(mu_max))
    return SmoothnessFit(lam=lam, mu=mu if gated else None, lam_at_bound=lam_bound, mu_at_bound=mu_bound, jumps_observed=j_obs, jumps_expected=j_exp,
                         flips_observed=f_obs, flips_expected=f_exp, log_likelihood=emit - lam * j_obs - (mu * f_obs if gated else 0.0) - log_z, se_lam=se_lam,
                         se_mu=se_mu, evaluations=count[0])
