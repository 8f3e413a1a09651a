"""Stage-2 train-time inputs from raw clips: the random offset, crop, flip and segment start of the reference's train transform chain,
drawn on the host and applied on the device.

The reference builds every Stage-2 / synchronizability fine-tune example on a CPU DataLoader (configs/sync.yaml:120-202,
configs/ft_synchability.yaml):

    EqualifyFromRight -> RGBSpatialCrop(is_random=True) -> TemporalCropAndOffset / ...ForSyncabilityTraining -> RandomHorizontalFlip
    -> GenerateMultipleSegments(is_start_random=True) -> RGBToHalfToZeroOne -> RGBNormalize -> log-mel          (dataset/transforms.py)

and ships 67 MB of fp16 per clip.  Here `ClipSampler` makes only the random DECISIONS of that chain - per clip a table row
(frame0, y0, x0, flip), an audio start `sample0` and the target - and the device does the rest: `sf_im2col_video_crops` (crop, flip,
segmenting, RGB normalisation, patch gather in one pass) and `sf_mel_frontend_starts` (log-mel of every clip's own audio window).

Python `random` draws come from a caller-supplied `random.Random` in exactly the reference's order - crop `randint` x2, offset `choice`
(syncability mode: `random()` first), `uniform`, jitter `randint`, segment-start `randint` - so the same seed reproduces what the reference
draws for the same item (tests/golden/train_crops.npz pins it).  The flip is one Bernoulli(p_flip) per clip from a `torch.Generator`; its
stream is NOT the reference's torch RNG stream: there the p = 0 colour and audio augs of sync.yaml consume `torch.rand` draws of their own,
so a replay would mean restating them.  The flip rate and independence are what matter for training, and those are the same.

Rows are validated here, on the host, before they are uploaded: the launchers cannot read a device table without a sync, so the kernels only
clamp a row into its clip (a bad row would read the wrong pixels, never outside the clip); a row this module builds is always in bounds.

    sampler = ClipSampler('grid')                                   # configs/sync.yaml; 'syncability' for configs/ft_synchability.yaml
    batch = sampler.sample(rng, v_lens, a_lens, H, W, gen)           # or sampler.fixed(offset_sec, v_start_i_sec, v_lens, a_lens, H, W)
    frames_win, wave_win, rel = batch.trim(frames_host, wave_host)  # only the frames / samples the segments read
    loss = trainer.train_step_clips(frames_win.to(dev), wave_win.to(dev), mel, rel.to(dev))

Stage 1 (AVCLIP pre-training, configs/segment_avclip.yaml) has its own pair at the end of this module: `Stage1Sampler` draws that chain's decisions -
per clip crop / upscale / segment start / audio jitter, per SEGMENT colour jitter, gray, flip, volume, lowpass, noise - into a `Stage1Batch` of two
int32 tables, and `AVCLIPTrainer.train_step_clips` applies them on the device (sf_stage1_video_augment, sf_stage1_audio_augment).
"""
import math
import random
from dataclasses import dataclass, field, replace
from typing import List, Optional, Sequence

import numpy as np
import torch

TABLE_COLS = 4          # frame0, y0, x0, flip; the kernel takes the row stride, so a row can grow (e.g. per-clip colour augs) without an ABI change


def _sec2frames(sec, fps):          # dataset/transforms.py:12-16
    return int(sec * fps)


def _frames2sec(frames, fps):
    return frames / fps


def class_grid(max_off_sec: float = 2.0, grid_size: int = 21) -> torch.Tensor:
    """make_class_grid(-max_off_sec, max_off_sec, grid_size) (dataset/transforms.py:218-230): fp32, as the reference keeps it."""
    return torch.from_numpy(np.linspace(-max_off_sec, max_off_sec, grid_size)).float()


@dataclass
class ClipBatch:
    """The per-clip parameters of one batch.  `table` int32 (B, 4) = frame0, y0, x0, flip; `sample0` int64 (B,); `targets` int64 (B,) - on the
    host after sampling, on the device after `.to(device)`.  Segment s of clip b = frames table[b, 0] + s*v_stride .. +16 and samples
    sample0[b] + s*a_stride .. +a_size of that clip.  offset_sec / v_start_i_sec / a_jitter_i are kept for logging (the reference's
    item['targets'] / item['meta'])."""
    table: torch.Tensor
    sample0: torch.Tensor
    targets: torch.Tensor
    n_seg: int
    v_stride: int = 8
    a_stride: int = 5120
    a_size: int = 10240
    offset_sec: List[float] = field(default_factory=list)
    v_start_i_sec: List[float] = field(default_factory=list)
    a_jitter_i: List[int] = field(default_factory=list)

    @property
    def v_span(self) -> int:
        """Frames the n_seg segments of a clip read (120 for 14 half-overlapping 16-frame segments)."""
        return (self.n_seg - 1) * self.v_stride + 16

    @property
    def a_span(self) -> int:
        return (self.n_seg - 1) * self.a_stride + self.a_size

    def windows(self):
        """(frame_lo, sample_lo) int64 arrays: clip b needs frames [frame_lo[b], + v_span) and samples [sample_lo[b], + a_span) only - what a host
        loader has to decode / ship (v_span frames at full resolution instead of the whole clip)."""
        return self.table[:, 0].cpu().numpy().astype(np.int64), self.sample0.cpu().numpy().astype(np.int64)

    def validate(self, clip_frames: int, clip_samples: int, H: int, W: int):
        """Raise ValueError unless every row's windows lie inside a (clip_frames, 3, H, W) clip / clip_samples waveform (host tensors only)."""
        t, s0 = self.table.cpu(), self.sample0.cpu()
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] < TABLE_COLS or t.shape[0] != s0.shape[0]:
            raise ValueError(f'ClipBatch: table must be int32 (B, >= {TABLE_COLS}) with one sample0 per row, got {t.dtype} {tuple(t.shape)}')
        f0, y0, x0 = t[:, 0].long(), t[:, 1].long(), t[:, 2].long()
        bad = (f0 < 0) | (f0 + self.v_span > clip_frames) | (y0 < 0) | (y0 + 224 > H) | (x0 < 0) | (x0 + 224 > W) | (s0 < 0) | \
              (s0 + self.a_span > clip_samples)
        if bool(bad.any()):
            b = int(bad.nonzero()[0, 0])
            raise ValueError(f'ClipBatch: row {b} (frame0, y0, x0, flip = {t[b].tolist()}, sample0 {int(s0[b])}) leaves the clip of {clip_frames} frames '
                             f'{H}x{W}, {clip_samples} samples ({self.n_seg} segments read {self.v_span} frames / {self.a_span} samples)')

    def trim(self, frames: torch.Tensor, wave: torch.Tensor, pin: bool = False):
        """Host clips frames (B, T, 3, H, W) uint8 / wave (B, n) -> (frames (B, v_span, 3, H, W), wave (B, a_span), batch relative to them): the
        windows only, so the host-to-device transfer carries v_span frames per clip at full resolution instead of the whole clip."""
        self.validate(frames.shape[1], wave.shape[1], frames.shape[3], frames.shape[4])
        f_lo, s_lo = self.windows()
        fw = torch.empty((frames.shape[0], self.v_span) + tuple(frames.shape[2:]), dtype=frames.dtype, pin_memory=pin)
        ww = torch.empty((wave.shape[0], self.a_span), dtype=torch.float32, pin_memory=pin)
        for b in range(frames.shape[0]):
            fw[b].copy_(frames[b, f_lo[b]:f_lo[b] + self.v_span])
            ww[b].copy_(wave[b, s_lo[b]:s_lo[b] + self.a_span])
        table = self.table.clone()
        table[:, 0] = 0
        return fw, ww, replace(self, table=table, sample0=torch.zeros_like(self.sample0))

    def to(self, device, non_blocking: bool = False) -> 'ClipBatch':
        return replace(self, table=self.table.to(device, non_blocking=non_blocking), sample0=self.sample0.to(device, non_blocking=non_blocking),
                       targets=self.targets.to(device, non_blocking=non_blocking))

    def pin_memory(self) -> 'ClipBatch':
        return replace(self, table=self.table.pin_memory(), sample0=self.sample0.pin_memory(), targets=self.targets.pin_memory())


class ClipSampler:
    """The random part of the Stage-2 train transform chain, per clip (see the module docstring).

    mode 'grid': TemporalCropAndOffset(offset_type='grid') of configs/sync.yaml - offset drawn from the 21-point grid over +-max_off_sec,
    target = its grid index.  mode 'syncability': TemporalCropAndOffsetForSyncabilityTraining (dataset/transforms.py:502-630) of
    configs/ft_synchability.yaml - with p = 0.5 a grid offset, otherwise +-crop_len_sec; target = sync_target = int(offset_is_syncable).
    Defaults are those two configs' (14 / 13 segments of 16 frames, 50 % overlap, 25 fps, 16 kHz, 5 s crop, 0.05 s audio wiggle, p_flip 0.5)."""

    def __init__(self, mode: str = 'grid', n_segments: Optional[int] = None, crop_len_sec: float = 5.0, max_off_sec: float = 2.0,
                 grid_size: int = 21, max_wiggle_sec: float = 0.05, segment_size_vframes: int = 16, step_size_seg: float = 0.5,
                 input_size: int = 224, p_flip: float = 0.5, clip_max_len_sec: float = 10, v_fps: int = 25, a_fps: int = 16000):
        if mode not in ('grid', 'syncability'):
            raise ValueError(f"ClipSampler: mode must be 'grid' or 'syncability', got {mode!r}")
        if input_size != 224:
            raise ValueError('ClipSampler: the crop kernel serves 224 x 224 crops')
        self.mode = mode
        self.n_segments = n_segments if n_segments is not None else (14 if mode == 'grid' else 13)
        self.max_wiggle_sec, self.seg_v, self.step = max_wiggle_sec, segment_size_vframes, step_size_seg
        self.input_size, self.p_flip, self.clip_max_len_sec = input_size, float(p_flip), clip_max_len_sec
        self.v_fps, self.a_fps = v_fps, a_fps
        self.grid = class_grid(max_off_sec, grid_size)
        self._grid_list = self.grid.tolist()
        if mode == 'syncability':                                     # transforms.py:507-510
            seg_size_sec = segment_size_vframes / v_fps
            trim_size_in_seg = self.n_segments - (1 - step_size_seg) * (self.n_segments - 1)
            self.crop_len_sec = round(trim_size_in_seg * seg_size_sec, 2)
        else:
            self.crop_len_sec = crop_len_sec
        if max_wiggle_sec is not None and max_wiggle_sec - 1e-6 > (self._grid_list[1] - self._grid_list[0]) / 2:
            raise ValueError(f'ClipSampler: max_wiggle_sec {max_wiggle_sec} exceeds half the grid step')
        # GenerateMultipleSegments geometry (transforms.py:421-439)
        self.seg_a = _sec2frames(_frames2sec(segment_size_vframes, v_fps), a_fps)
        self.v_stride, self.a_stride = int(step_size_seg * segment_size_vframes), int(step_size_seg * self.seg_a)

    # ---- the reference's transforms, one clip at a time -----------------------------------------------------------------------------------
    def _equalify(self, v_len: int, a_len: int):
        """EqualifyFromRight (transforms.py:19-57)."""
        min_len = min(self.clip_max_len_sec, a_len / self.a_fps, v_len / self.v_fps)
        v_len_frames = int(self.v_fps * min_len)
        a_len_frames = int((self.a_fps // self.v_fps) * v_len_frames)
        if not (a_len_frames <= a_len and v_len_frames <= v_len):
            raise ValueError(f'EqualifyFromRight: {a_len_frames} / {v_len_frames} exceed {a_len} / {v_len}')
        return v_len_frames, a_len_frames

    def _crop(self, rng, H: int, W: int, random_crop: bool):
        """RGBSpatialCrop (transforms.py:68-95): (y0, x0)."""
        th = tw = self.input_size
        if H < th or W < tw:
            raise ValueError(f'frames {H}x{W} are smaller than the {th} crop')
        if not random_crop:
            return int(round((H - th) / 2.)), int(round((W - tw) / 2.))
        if W == tw and H == th:
            return 0, 0
        return rng.randint(0, H - th), rng.randint(0, W - tw)

    def _jitter(self, rng, a_start_i: int, a_len: int, a_crop: int):
        """apply_a_jitter (transforms.py:242-254)."""
        max_a_start_i = a_len - a_crop
        max_j = _sec2frames(self.max_wiggle_sec, self.a_fps)
        left, right = min(a_start_i, max_j), min(max_a_start_i - a_start_i, max_j)
        a_jitter_i = rng.randint(-left, right)
        a_start_i = a_start_i + a_jitter_i
        if not 0 <= a_start_i <= max_a_start_i:
            raise ValueError(f'audio jitter {a_jitter_i} leaves [0, {max_a_start_i}]')
        return a_start_i, a_jitter_i

    def _fix_negative(self, a_start_i: int) -> int:
        """The `a_start_i < 0` fix-up (transforms.py:352-362, 594-604): a rounding-sized underflow is moved to 0, anything larger raises."""
        if a_start_i < 0:
            if abs(a_start_i) <= self.a_fps / self.v_fps:
                return a_start_i + abs(a_start_i)
            raise ValueError(f'a_start_i {a_start_i} is negative beyond one video frame')
        return a_start_i

    def _offset(self, rng, v_len: int, a_len: int, fixed):
        """TemporalCropAndOffset / ...ForSyncabilityTraining: (v_start_i, a_start_i, offset_sec, v_start_i_sec, a_jitter_i, target)."""
        v_fps, a_fps = self.v_fps, self.a_fps
        v_crop, a_crop = _sec2frames(self.crop_len_sec, v_fps), _sec2frames(self.crop_len_sec, a_fps)
        wiggle = self.max_wiggle_sec is not None and self.max_wiggle_sec > 0 and fixed is None
        a_jitter_i, syncable = 0, None
        if fixed is None:
            if self.mode == 'syncability':
                syncable = rng.random() < 0.5
                offset_sec = rng.choice(self._grid_list) if syncable else rng.choice([-self.crop_len_sec, self.crop_len_sec])
            else:
                offset_sec = rng.choice(self._grid_list)
            offset_sec = round(offset_sec, 2)
            v_start_max_sec = _frames2sec(v_len - v_crop, v_fps)
            if not v_start_max_sec > 0:
                raise ValueError(f'clip of {v_len} frames is too short for a {v_crop}-frame crop')
            v_start_sec = rng.uniform(max(0, -offset_sec), min(v_start_max_sec, v_start_max_sec - offset_sec))
            if not 0 <= v_start_sec <= v_start_max_sec:
                raise ValueError(f'v_start_sec {v_start_sec} outside [0, {v_start_max_sec}]')
            v_start_i = _sec2frames(v_start_sec, v_fps)
            v_start_i_sec = _frames2sec(v_start_i, v_fps)
        else:
            offset_sec, v_start_i_sec = round(fixed[0], 2), fixed[1]
            v_start_i = _sec2frames(v_start_i_sec, v_fps)
        a_start_i = _sec2frames(v_start_i_sec + offset_sec, a_fps)
        if self.mode == 'syncability':                                # jitter first, then the fix-up (transforms.py:564-604)
            if wiggle:
                a_start_i, a_jitter_i = self._jitter(rng, a_start_i, a_len, a_crop)
            a_start_i = self._fix_negative(a_start_i)
        else:                                                         # the fix-up first, then the jitter (transforms.py:352-368)
            a_start_i = self._fix_negative(a_start_i)
            if wiggle:
                a_start_i, a_jitter_i = self._jitter(rng, a_start_i, a_len, a_crop)
        if not (a_len >= a_start_i + a_crop and v_len >= v_start_i + v_crop):
            raise ValueError(f'crop [{v_start_i}, +{v_crop}) / [{a_start_i}, +{a_crop}) leaves the clip of {v_len} frames / {a_len} samples')
        if self.mode == 'syncability':
            target = int(syncable)
        else:
            target = int((self.grid - offset_sec).abs().argmin())    # quantize_offset (transforms.py:233-238), on the fp32 grid like the reference
        return v_start_i, a_start_i, offset_sec, v_start_i_sec, a_jitter_i, target, v_crop, a_crop

    def _segments(self, rng, v_len: int, a_len: int, random_start: bool):
        """GenerateMultipleSegments (transforms.py:421-500) on the v_len / a_len crop: the start (frames, samples) of segment 0."""
        n_max = min((v_len - self.seg_v) // self.v_stride + 1, (a_len - self.seg_a) // self.a_stride + 1)
        if self.n_segments > n_max:
            raise ValueError(f'cant make {self.n_segments} segs of len {self.seg_v} in a vid of len {v_len}')
        seg_seq_len = self.n_segments * self.step + (1 - self.step)
        max_v_start_i = v_len - int(seg_seq_len * self.seg_v)
        v_start_i = rng.randint(0, max_v_start_i) if random_start else max_v_start_i // 2
        a_start_i = _sec2frames(_frames2sec(v_start_i, self.v_fps), self.a_fps)
        if a_start_i + (self.n_segments - 1) * self.a_stride + self.seg_a > a_len:
            raise ValueError('audio segment ranges out of bounds')
        return v_start_i, a_start_i

    def _clip(self, rng, v_len, a_len, H, W, fixed):
        v_len, a_len = self._equalify(int(v_len), int(a_len))
        y0, x0 = self._crop(rng, H, W, random_crop=fixed is None)
        v0, a0, off, vsec, jit, tgt, v_crop, a_crop = self._offset(rng, v_len, a_len, fixed)
        sv, sa = self._segments(rng, v_crop, a_crop, random_start=fixed is None)
        return (v0 + sv, y0, x0), a0 + sa, off, vsec, jit, tgt

    def _batch(self, rows, flips):
        table = torch.tensor([list(r[0]) + [int(f)] for r, f in zip(rows, flips)], dtype=torch.int32).view(len(rows), TABLE_COLS)
        return ClipBatch(table=table, sample0=torch.tensor([r[1] for r in rows], dtype=torch.int64),
                         targets=torch.tensor([r[5] for r in rows], dtype=torch.int64), n_seg=self.n_segments, v_stride=self.v_stride,
                         a_stride=self.a_stride, a_size=self.seg_a, offset_sec=[r[2] for r in rows], v_start_i_sec=[r[3] for r in rows],
                         a_jitter_i=[r[4] for r in rows])

    # ---- public -----------------------------------------------------------------------------------------------------------------------------
    def sample(self, rng: random.Random, v_lens: Sequence[int], a_lens: Sequence[int], H: int, W: int,
               gen: Optional[torch.Generator] = None) -> ClipBatch:
        """Train-time draws for B clips of v_lens[b] frames / a_lens[b] samples (lengths may differ; the frames tensor is (B, max T, 3, H, W)).
        Python draws from `rng` clip by clip in the reference's order; the flips from `gen` (torch.rand(B) < p_flip) after them."""
        if len(v_lens) != len(a_lens):
            raise ValueError('ClipSampler.sample: one audio length per clip')
        rows = [self._clip(rng, v, a, H, W, None) for v, a in zip(v_lens, a_lens)]
        flips = (torch.rand(len(rows), generator=gen) < self.p_flip).tolist()
        batch = self._batch(rows, flips)
        batch.validate(max(v_lens), max(a_lens), H, W)
        return batch

    def fixed(self, offset_sec: Sequence[float], v_start_i_sec: Sequence[float], v_lens: Sequence[int], a_lens: Sequence[int], H: int,
              W: int) -> ClipBatch:
        """The valid / test split (load_fixed_offsets_on, configs/sync.yaml:115): offsets and video starts from the CSV, centre crop, no audio
        wiggle, middle segment start, no flip - transform_sequence_test (configs/sync.yaml:204-225).  Grid mode only: the fine-tune config
        loads no fixed offsets and its transform defines no sync target for them."""
        if self.mode != 'grid':
            raise ValueError('ClipSampler.fixed: fixed offsets exist for the grid mode only (configs/ft_synchability.yaml: load_fixed_offsets_on [])')
        if not (len(offset_sec) == len(v_start_i_sec) == len(v_lens) == len(a_lens)):
            raise ValueError('ClipSampler.fixed: one offset, video start and length pair per clip')
        rows = [self._clip(None, v, a, H, W, (o, s)) for o, s, v, a in zip(offset_sec, v_start_i_sec, v_lens, a_lens)]
        batch = self._batch(rows, [0] * len(rows))
        batch.validate(max(v_lens), max(a_lens), H, W)
        return batch


class ClipTrainPipeline:
    """Raw clips from HOST memory to train steps, with the host-to-device transfer of batch i+1 under the step of batch i - the training
    counterpart of frontend.HostClipPipeline (same two-slot shape).  The host hands over the trimmed windows of a batch (ClipBatch.trim:
    uint8 frames (B, v_span, 3, H, W) at full resolution, fp32 wave (B, a_span)) and the batch's parameter table, all PINNED; frames, wave,
    table, sample0 and targets go H2D on a copy stream into one of two device slots while the compute stream trains on the other.  Events hand
    off in both directions; nothing in step() waits on the host.

        pipe = ClipTrainPipeline(trainer, MelFrontend(dev), B, H=256, W=256)
        pipe.stage(frames0, wave0, batch0)                                # pinned; batch0 relative to the windows (ClipBatch.trim)
        for f, w, b in batches[1:]:
            loss = pipe.step(f, w, b)                                     # step of the staged batch || H2D of the next one
        loss = pipe.step()
    LIFETIME OF THE HOST BUFFERS: as in HostClipPipeline, the copies are only enqueued - call `wait_staged()` (or synchronize the event stage()
    returns) before overwriting the pinned buffers of the most recent stage().  The returned loss is the trainer's device scalar, valid on the
    compute stream and overwritten by the next step."""

    def __init__(self, trainer, mel, B: int, n_seg: int = 14, H: int = 256, W: int = 256, v_stride: int = 8, a_stride: int = 5120,
                 a_size: int = 10240, lr: Optional[float] = None):
        self.tr, self.mel, self.dev, self.lr = trainer, mel, trainer.engine.dev, lr
        span_v, span_a = (n_seg - 1) * v_stride + 16, (n_seg - 1) * a_stride + a_size
        self.geom = dict(n_seg=n_seg, v_stride=v_stride, a_stride=a_stride, a_size=a_size)
        self.frames = [torch.empty(B, span_v, 3, H, W, device=self.dev, dtype=torch.uint8) for _ in range(2)]
        self.wave = [torch.empty(B, span_a, device=self.dev, dtype=torch.float32) for _ in range(2)]
        self.batch = [ClipBatch(table=torch.empty(B, TABLE_COLS, device=self.dev, dtype=torch.int32),
                                sample0=torch.empty(B, device=self.dev, dtype=torch.int64),
                                targets=torch.empty(B, device=self.dev, dtype=torch.int64), **self.geom) for _ in range(2)]
        self.copy_stream = torch.cuda.Stream(device=self.dev)
        self.loaded = [torch.cuda.Event(), torch.cuda.Event()]
        self.released = [torch.cuda.Event(), torch.cuda.Event()]
        self._fresh = [True, True]
        self._staged = None
        self._next = 0
        self._last_loaded = None

    def stage(self, frames_host: torch.Tensor, wave_host: torch.Tensor, batch_host: ClipBatch) -> 'torch.cuda.Event':
        """Start the transfer of one batch into the free slot; returns the event recorded behind the copies."""
        if self._staged is not None and self._next == self._staged:
            raise RuntimeError('ClipTrainPipeline: both slots are in use - call step() before staging another batch')
        if frames_host.shape != self.frames[0].shape or frames_host.dtype != torch.uint8 or wave_host.shape != self.wave[0].shape or \
                wave_host.dtype != torch.float32:
            raise ValueError(f'ClipTrainPipeline: expected uint8 frames {tuple(self.frames[0].shape)} and fp32 wave {tuple(self.wave[0].shape)}, got '
                             f'{frames_host.dtype} {tuple(frames_host.shape)}, {wave_host.dtype} {tuple(wave_host.shape)}')
        if any(getattr(batch_host, k) != v for k, v in self.geom.items()):
            raise ValueError(f'ClipTrainPipeline: batch geometry differs from {self.geom}')
        batch_host.validate(frames_host.shape[1], wave_host.shape[1], frames_host.shape[3], frames_host.shape[4])
        i = self._next
        slot = self.batch[i]
        with torch.cuda.stream(self.copy_stream):
            if not self._fresh[i]:
                self.copy_stream.wait_event(self.released[i])
            self.frames[i].copy_(frames_host, non_blocking=True)
            self.wave[i].copy_(wave_host, non_blocking=True)
            slot.table.copy_(batch_host.table, non_blocking=True)
            slot.sample0.copy_(batch_host.sample0, non_blocking=True)
            slot.targets.copy_(batch_host.targets, non_blocking=True)
            self.loaded[i].record(self.copy_stream)
        slot.offset_sec, slot.v_start_i_sec, slot.a_jitter_i = batch_host.offset_sec, batch_host.v_start_i_sec, batch_host.a_jitter_i
        if self._staged is None:
            self._staged = i
        self._next = i ^ 1
        self._last_loaded = self.loaded[i]
        return self.loaded[i]

    def wait_staged(self):
        """Block the HOST until the most recent stage() has left the caller's host buffers (they may be recycled afterwards)."""
        if self._last_loaded is not None:
            self._last_loaded.synchronize()

    def step(self, next_frames_host: torch.Tensor = None, next_wave_host: torch.Tensor = None, next_batch_host: ClipBatch = None) -> torch.Tensor:
        """Train step of the staged batch; if a next batch is given its transfer is issued FIRST so that it runs under this step."""
        if self._staged is None:
            raise RuntimeError('ClipTrainPipeline: nothing staged')
        i = self._staged
        if next_frames_host is not None:
            self._next = i ^ 1
            self.stage(next_frames_host, next_wave_host, next_batch_host)
        main = torch.cuda.current_stream(self.dev)
        main.wait_event(self.loaded[i])
        loss = self.tr.train_step_clips(self.frames[i], self.wave[i], self.mel, self.batch[i], lr=self.lr)
        self.released[i].record(main)
        self._fresh[i] = False
        self._staged = (i ^ 1) if next_frames_host is not None else None
        return loss


# ---- Stage 1 (AVCLIP pre-training): transform_sequence_train of configs/segment_avclip.yaml ----------------------------------------------------------
# The two device tables of sf_stage1_video_augment / sf_stage1_audio_augment (include/synchformer_hip.h has the same layout; floats as bit patterns)
S1_CLIP_COLS = 5        # frame0, y0, x0, side (224 | 192), sample0 (audio jitter included)
S1_SEG_COLS = 16        # jitter, op0..op3, (r32, q32) of brightness / contrast / saturation, hue, gray, flip, audio flags, noise seed
S1_JITTER, S1_OP0, S1_BRIGHT, S1_CONTRAST, S1_SATUR, S1_HUE, S1_GRAY, S1_FLIP, S1_AUDIO, S1_SEED = 0, 1, 5, 7, 9, 11, 12, 13, 14, 15
S1_OP_BRIGHTNESS, S1_OP_CONTRAST, S1_OP_SATURATION, S1_OP_HUE = 0, 1, 2, 3      # torchvision ColorJitter's fn_idx
S1_AUDIO_VOLUME, S1_AUDIO_LOWPASS, S1_AUDIO_NOISE = 1, 2, 4


def f32_bits(x) -> torch.Tensor:
    """float32 values -> their bit patterns as int32 (how the tables carry floats)."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.int32).copy())


def bits_f32(t: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(t.cpu().contiguous().numpy().view(np.float32).copy())


def blend_pair(ratio):
    """(r32, q32) = (float32(ratio), float32(1.0 - ratio)) with the subtraction in double: what torch makes of the Python scalars `ratio` and
    `1.0 - ratio` of torchvision's _blend when they meet a float32 tensor."""
    r = np.asarray(ratio, dtype=np.float64)
    return r.astype(np.float32), (1.0 - r).astype(np.float32)


def lowpass_coeffs(sample_rate: float = 16000, cutoff_freq: float = 100, Q: float = 0.707):
    """torchaudio.functional.lowpass_biquad's RBJ coefficients divided by a0, in double: (b0, b1, b2, a1, a2)."""
    w0 = 2 * math.pi * cutoff_freq / sample_rate
    alpha = math.sin(w0) / 2 / Q
    b0, b1, b2 = (1 - math.cos(w0)) / 2, 1 - math.cos(w0), (1 - math.cos(w0)) / 2
    a0, a1, a2 = 1 + alpha, -2 * math.cos(w0), 1 - alpha
    return b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0


@dataclass
class Stage1Batch:
    """The decisions of one Stage-1 batch.  `clip_table` int32 (B, 5) = frame0, y0, x0, side, sample0 and `seg_table` int32 (B * n_seg, 16), row of
    segment (b, s) at b * n_seg + s (columns: the S1_* constants above) - on the host after sampling, on the device after `.to(device)`.
    Segment s of clip b = frames clip_table[b, 0] + s*v_stride .. +16 and samples clip_table[b, 4] + s*a_stride .. +a_size.  `lowpass` = the
    biquad's (b0, b1, b2, a1, a2); a_jitter_i is kept for logging."""
    clip_table: torch.Tensor
    seg_table: torch.Tensor
    n_seg: int
    v_stride: int = 16
    a_stride: int = 10240
    a_size: int = 10240
    lowpass: tuple = field(default_factory=lowpass_coeffs)
    noise_amp: float = 0.01
    a_jitter_i: List[int] = field(default_factory=list)

    @property
    def v_span(self) -> int:
        return (self.n_seg - 1) * self.v_stride + 16

    @property
    def a_span(self) -> int:
        return (self.n_seg - 1) * self.a_stride + self.a_size

    def windows(self):
        """(frame_lo, sample_lo) int64 arrays: clip b needs frames [frame_lo[b], + v_span) and samples [sample_lo[b], + a_span) only."""
        t = self.clip_table.cpu().numpy().astype(np.int64)
        return t[:, 0], t[:, 4]

    def validate(self, clip_frames: int, clip_samples: int, H: int, W: int):
        """Raise ValueError unless every clip row's windows lie inside a (clip_frames, 3, H, W) clip / clip_samples waveform and every segment row
        holds flags, a permutation of the four ops and finite factors (host tensors only)."""
        c, s = self.clip_table.cpu(), self.seg_table.cpu()
        if c.dtype != torch.int32 or c.dim() != 2 or c.shape[1] < S1_CLIP_COLS or s.dtype != torch.int32 or s.dim() != 2 or s.shape[1] < S1_SEG_COLS or \
                s.shape[0] != c.shape[0] * self.n_seg:
            raise ValueError(f'Stage1Batch: tables must be int32 (B, >= {S1_CLIP_COLS}) and (B * {self.n_seg}, >= {S1_SEG_COLS}), got {c.dtype} '
                             f'{tuple(c.shape)}, {s.dtype} {tuple(s.shape)}')
        f0, y0, x0, side, s0 = (c[:, i].long() for i in range(5))
        bad = (f0 < 0) | (f0 + self.v_span > clip_frames) | ((side != 224) & (side != 192)) | (y0 < 0) | (y0 + side > H) | (x0 < 0) | (x0 + side > W) | \
              (s0 < 0) | (s0 + self.a_span > clip_samples)
        if bool(bad.any()):
            b = int(bad.nonzero()[0, 0])
            raise ValueError(f'Stage1Batch: clip row {b} (frame0, y0, x0, side, sample0 = {c[b, :5].tolist()}) leaves the clip of {clip_frames} frames '
                             f'{H}x{W}, {clip_samples} samples ({self.n_seg} segments read {self.v_span} frames / {self.a_span} samples)')
        flags = s[:, [S1_JITTER, S1_GRAY, S1_FLIP]]
        ops_ok = (s[:, S1_OP0:S1_OP0 + 4].sort(1).values == torch.arange(4, dtype=torch.int32)).all(1)
        fac = bits_f32(s[:, S1_BRIGHT:S1_HUE + 1])
        bad = ((flags != 0) & (flags != 1)).any(1) | ~ops_ok | (s[:, S1_AUDIO] < 0) | (s[:, S1_AUDIO] > 7) | ~torch.isfinite(fac).all(1)
        if bool(bad.any()):
            r = int(bad.nonzero()[0, 0])
            raise ValueError(f'Stage1Batch: segment row {r} = {s[r, :S1_SEG_COLS].tolist()} is no valid row (0/1 flags, a permutation of the ops 0..3, '
                             f'finite factors, audio flags 0..7)')

    def trim(self, frames: torch.Tensor, wave: torch.Tensor, pin: bool = False):
        """Host clips frames (B, T, 3, H, W) uint8 / wave (B, n) -> (frames (B, v_span, 3, H, W), wave (B, a_span), batch relative to them)."""
        self.validate(frames.shape[1], wave.shape[1], frames.shape[3], frames.shape[4])
        f_lo, s_lo = self.windows()
        fw = torch.empty((frames.shape[0], self.v_span) + tuple(frames.shape[2:]), dtype=frames.dtype, pin_memory=pin)
        ww = torch.empty((wave.shape[0], self.a_span), dtype=torch.float32, pin_memory=pin)
        for b in range(frames.shape[0]):
            fw[b].copy_(frames[b, f_lo[b]:f_lo[b] + self.v_span])
            ww[b].copy_(wave[b, s_lo[b]:s_lo[b] + self.a_span])
        table = self.clip_table.clone()
        table[:, 0] = 0
        table[:, 4] = 0
        return fw, ww, replace(self, clip_table=table)

    def to(self, device, non_blocking: bool = False) -> 'Stage1Batch':
        return replace(self, clip_table=self.clip_table.to(device, non_blocking=non_blocking), seg_table=self.seg_table.to(device, non_blocking=non_blocking))

    def pin_memory(self) -> 'Stage1Batch':
        return replace(self, clip_table=self.clip_table.pin_memory(), seg_table=self.seg_table.pin_memory())


class Stage1Sampler:
    """The random DECISIONS of the Stage-1 train transform chain (configs/segment_avclip.yaml: transform_sequence_train), one clip at a time:

        EqualifyFromRight -> RGBSpatialCropSometimesUpscale -> GenerateMultipleSegments(is_start_random, audio_jitter_sec) -> per SEGMENT
        RandomApplyColorDistortion, RandomHorizontalFlip, AudioRandomVolume, AudioRandomLowpassFilter, AudioRandomGaussNoise

    The device applies them (sf_stage1_video_augment, sf_stage1_audio_augment).  Defaults are that file's: 14 segments of 16 frames, step 1.0
    (v_stride 16, a_stride 10240), 25 fps, 16 kHz, sometimes_upscale_p 0.2 (a 192 crop upscaled to 224), p_color_jitter 0.2, p_gray_scale 0.2,
    p_horizontal_flip 0.5, p_audio_aug 0.2, audio_jitter_sec 0.05.

    RNG.  Python `random` draws come from the caller's `random.Random` in exactly the reference's order - crop `randint` x2 (none when the frame
    is the crop size), segment-start `randint`, jitter `randint` - so the same seed gives the reference's crop corner, start and jitter
    (tests/golden/stage1_crops.npz pins it).  The Bernoulli, uniform and permutation draws - upscale per clip; per segment jitter on, op order,
    the three blend factors ~ U[0.2, 1.8], hue ~ U[-0.2, 0.2] (ColorJitter(0.8, 0.8, 0.8, 0.2), s = 1), gray, flip, volume, lowpass, noise and
    a 32-bit noise seed - come from the caller's `torch.Generator`.  Their stream is NOT the reference's global torch stream; the rates, the
    ranges and the independence of the draws are the contract.

    AudioRandomReverb and AudioRandomPitchShift are sox effects (torchaudio.sox_effects) and are not built: p_reverb / p_pitch must stay 0."""

    def __init__(self, n_segments: int = 14, segment_size_vframes: int = 16, step_size_seg: float = 1.0, input_size: int = 224,
                 smaller_input_size: int = 192, sometimes_p: float = 0.2, p_color_jitter: float = 0.2, p_gray_scale: float = 0.2, p_flip: float = 0.5,
                 p_audio_aug: float = 0.2, audio_jitter_sec: float = 0.05, p_reverb: float = 0.0, p_pitch: float = 0.0, is_random: bool = True,
                 clip_max_len_sec: float = 10, v_fps: int = 25, a_fps: int = 16000, lowpass_cutoff: float = 100, lowpass_Q: float = 0.707,
                 noise_amp: float = 0.01):
        if p_reverb or p_pitch:
            raise ValueError('Stage1Sampler: AudioRandomReverb / AudioRandomPitchShift are sox effects (torchaudio.sox_effects) and are not built: '
                             'p_reverb and p_pitch must be 0')
        if input_size != 224 or smaller_input_size != 192 or segment_size_vframes != 16:
            raise ValueError('Stage1Sampler: the augmentation kernels serve 16-frame segments of 224 crops and the 192 -> 224 upscale')
        for name, p in (('sometimes_p', sometimes_p), ('p_color_jitter', p_color_jitter), ('p_gray_scale', p_gray_scale), ('p_flip', p_flip),
                        ('p_audio_aug', p_audio_aug)):
            if not 0 <= p <= 1:
                raise ValueError(f'Stage1Sampler: {name} = {p} is no probability')
        self.n_segments, self.seg_v, self.step = n_segments, segment_size_vframes, step_size_seg
        self.input_size, self.small, self.sometimes_p, self.is_random = input_size, smaller_input_size, float(sometimes_p), is_random
        self.p_jitter, self.p_gray, self.p_flip, self.p_audio = float(p_color_jitter), float(p_gray_scale), float(p_flip), float(p_audio_aug)
        self.audio_jitter_sec, self.clip_max_len_sec, self.v_fps, self.a_fps = audio_jitter_sec, clip_max_len_sec, v_fps, a_fps
        self.seg_a = _sec2frames(_frames2sec(segment_size_vframes, v_fps), a_fps)
        self.v_stride, self.a_stride = int(step_size_seg * segment_size_vframes), int(step_size_seg * self.seg_a)
        self.lowpass, self.noise_amp = lowpass_coeffs(a_fps, lowpass_cutoff, lowpass_Q), noise_amp

    # ---- the reference's transforms, one clip at a time ----------------------------------------------------------------------------------------
    def _equalify(self, v_len: int, a_len: int):
        """EqualifyFromRight (transforms.py:19-57)."""
        min_len = min(self.clip_max_len_sec, a_len / self.a_fps, v_len / self.v_fps)
        v_len_frames = int(self.v_fps * min_len)
        a_len_frames = int((self.a_fps // self.v_fps) * v_len_frames)
        if not (a_len_frames <= a_len and v_len_frames <= v_len):
            raise ValueError(f'EqualifyFromRight: {a_len_frames} / {v_len_frames} exceed {a_len} / {v_len}')
        return v_len_frames, a_len_frames

    def _crop(self, rng, H: int, W: int, side: int):
        """RGBSpatialCrop (transforms.py:68-95) of `side`: (y0, x0)."""
        if H < side or W < side:
            raise ValueError(f'frames {H}x{W} are smaller than the {side} crop')
        if not self.is_random:
            return int(round((H - side) / 2.)), int(round((W - side) / 2.))
        if W == side and H == side:
            return 0, 0
        return rng.randint(0, H - side), rng.randint(0, W - side)

    def _segments(self, rng, v_len: int, a_len: int):
        """GenerateMultipleSegments (transforms.py:421-500): (frame0, sample0 with the jitter, jitter)."""
        n_max = min((v_len - self.seg_v) // self.v_stride + 1, (a_len - self.seg_a) // self.a_stride + 1)
        if self.n_segments > n_max:
            raise ValueError(f'cant make {self.n_segments} segs of len {self.seg_v} in a vid of len {v_len}')
        seg_seq_len = self.n_segments * self.step + (1 - self.step)
        v_seq, a_seq = int(seg_seq_len * self.seg_v), int(seg_seq_len * self.seg_a)
        max_v_start_i = v_len - v_seq
        v_start_i = rng.randint(0, max_v_start_i) if self.is_random else max_v_start_i // 2
        a_start_i = _sec2frames(_frames2sec(v_start_i, self.v_fps), self.a_fps)
        jitter = 0
        if self.audio_jitter_sec > 0:
            j = min(_sec2frames(self.audio_jitter_sec, self.a_fps), a_start_i, a_len - a_start_i - a_seq)
            jitter = rng.randint(-j, j)                              # j < 0 (audio too short): ValueError, as the reference's randint
        s0 = a_start_i + jitter
        if s0 < 0 or s0 + (self.n_segments - 1) * self.a_stride + self.seg_a > a_len:
            raise ValueError('audio segment ranges out of bounds')
        return v_start_i, s0, jitter

    def _clip(self, rng, v_len, a_len, H, W, upscale: bool):
        v_len, a_len = self._equalify(int(v_len), int(a_len))
        side = self.small if upscale else self.input_size
        y0, x0 = self._crop(rng, H, W, side)
        frame0, s0, jitter = self._segments(rng, v_len, a_len)
        return [frame0, y0, x0, side, s0], jitter

    def _segment_rows(self, n: int, gen) -> torch.Tensor:
        """The per-segment table of n segments, every draw from `gen` (column by column, so the stream does not depend on the outcomes)."""
        def bern(p):
            return (torch.rand(n, generator=gen) < p).to(torch.int32)
        t = torch.zeros(n, S1_SEG_COLS, dtype=torch.int32)
        t[:, S1_JITTER] = bern(self.p_jitter)
        t[:, S1_OP0:S1_OP0 + 4] = torch.rand(n, 4, generator=gen).argsort(1).to(torch.int32)      # a uniform permutation of the four ops
        ratio = torch.empty(n, 3, dtype=torch.float32).uniform_(0.2, 1.8, generator=gen).numpy()   # ColorJitter draws fp32 and passes float(.)
        r32, q32 = blend_pair(ratio)
        for i, col in enumerate((S1_BRIGHT, S1_CONTRAST, S1_SATUR)):
            t[:, col], t[:, col + 1] = f32_bits(r32[:, i]), f32_bits(q32[:, i])
        t[:, S1_HUE] = f32_bits(torch.empty(n, dtype=torch.float32).uniform_(-0.2, 0.2, generator=gen).numpy())
        t[:, S1_GRAY], t[:, S1_FLIP] = bern(self.p_gray), bern(self.p_flip)
        t[:, S1_AUDIO] = bern(self.p_audio) * S1_AUDIO_VOLUME + bern(self.p_audio) * S1_AUDIO_LOWPASS + bern(self.p_audio) * S1_AUDIO_NOISE
        seed = torch.randint(0, 2 ** 32, (n,), generator=gen, dtype=torch.int64)
        t[:, S1_SEED] = torch.where(seed >= 2 ** 31, seed - 2 ** 32, seed).to(torch.int32)
        return t

    # ---- public ------------------------------------------------------------------------------------------------------------------------------
    def sample(self, rng: random.Random, v_lens: Sequence[int], a_lens: Sequence[int], H: int, W: int,
               gen: Optional[torch.Generator] = None) -> Stage1Batch:
        """Train-time draws for B clips of v_lens[b] frames / a_lens[b] samples (the frames tensor is (B, max T, 3, H, W)).  From `gen` first the B
        upscale decisions, then the segment table; from `rng` clip by clip in the reference's order."""
        if len(v_lens) != len(a_lens):
            raise ValueError('Stage1Sampler.sample: one audio length per clip')
        B = len(v_lens)
        upscale = (torch.rand(B, generator=gen) < self.sometimes_p).tolist()
        seg_table = self._segment_rows(B * self.n_segments, gen)
        rows = [self._clip(rng, v, a, H, W, u) for v, a, u in zip(v_lens, a_lens, upscale)]
        batch = Stage1Batch(clip_table=torch.tensor([r[0] for r in rows], dtype=torch.int32).view(B, S1_CLIP_COLS), seg_table=seg_table,
                            n_seg=self.n_segments, v_stride=self.v_stride, a_stride=self.a_stride, a_size=self.seg_a, lowpass=self.lowpass,
                            noise_amp=self.noise_amp, a_jitter_i=[r[1] for r in rows])
        batch.validate(max(v_lens), max(a_lens), H, W)
        return batch
