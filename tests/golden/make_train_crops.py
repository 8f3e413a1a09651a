"""Fixture for synchformer_amd.augment.ClipSampler: the REAL reference train transforms (dataset/transforms.py) run on index-valued synthetic
items under random.seed(k), recording the draws they make.

    python tests/golden/make_train_crops.py        # writes tests/golden/train_crops.npz

Chain per item (configs/sync.yaml:120-202 / configs/ft_synchability.yaml, without the torch-RNG transforms):
    EqualifyFromRight -> RGBSpatialCrop(is_random) -> TemporalCropAndOffset(offset_type='grid') / ...ForSyncabilityTraining
    -> GenerateMultipleSegments(is_start_random)
The video holds value t * 10^6 + y * 10^3 + x at frame t, pixel (y, x) and the audio sample i holds i, so the outputs give back the crop corner,
the temporal crop start and the segment-0 frame / sample.  Only integers are stored (offsets as round(100 * offset_sec)).
"""
import random
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import ref_import  # noqa: E402

N_SEEDS = 200
# case id -> (mode, n_segments, v_len, a_len, H, W)
CASES = [
    ('grid', 14, 250, 160000, 256, 256),          # 10 s, 256-side (configs/sync.yaml: size_before_crop 256)
    ('grid', 14, 250, 160000, 256, 340),          # 10 s, non-square
    ('grid', 14, 175, 112000, 256, 256),          # just long enough for +-2 s around a 5 s crop
    ('grid', 14, 260, 150000, 257, 300),          # audio shorter than video: EqualifyFromRight trims both
    ('grid', 14, 150, 96000, 256, 256),           # too short for the large offsets: some draws assert
    ('grid', 14, 125, 80000, 256, 256),           # exactly one crop long: v_start_max_sec == 0 asserts
    ('grid', 14, 250, 160000, 224, 224),          # no spatial draws when the frame is the crop size
    ('syncability', 13, 250, 160000, 256, 256),   # configs/ft_synchability.yaml: 13 segments, +-crop_len offsets
    ('syncability', 13, 250, 160000, 256, 340),
    ('syncability', 13, 200, 128000, 256, 256),
]
# fixed offsets (load_fixed_offsets_on valid/test): (offset_sec, v_start_i_sec) on a 10 s 256 x 340 clip, transform_sequence_test
FIXED = [(0.0, 2.0), (-2.0, 2.0), (2.0, 0.0), (-1.5, 1.48), (0.4, 1.2), (-0.2, 3.0), (1.8, 3.16), (0.6, 4.96), (-1.0, 0.96), (2.0, 5.0),
         (-2.0, 1.0), (1.0, 6.0)]
COLUMNS = ['case', 'seed', 'ok', 'y0', 'x0', 'v_start_i', 'a_start_i_seg0', 'frame_seg0', 'offset_sec_x100', 'target', 'a_jitter_i']


def _item(v_len, a_len, H, W, targets=None, split='train'):
    t = torch.arange(v_len, dtype=torch.int32).view(v_len, 1, 1, 1) * 1000000
    y = torch.arange(H, dtype=torch.int32).view(1, 1, H, 1) * 1000
    x = torch.arange(W, dtype=torch.int32).view(1, 1, 1, W)
    return dict(video=(t + y + x).expand(v_len, 3, H, W), audio=torch.arange(a_len, dtype=torch.float64), path='synthetic', split=split,
                meta=dict(video=dict(fps=[25.0]), audio=dict(framerate=[16000.0])), targets=dict(targets or {}))


def main():
    ref_import.import_reference_avclip()                  # late shims: dataset.transforms imports torchvision / torchaudio
    with ref_import._cwd(ref_import.REF):
        from dataset.transforms import (EqualifyFromRight, GenerateMultipleSegments, RGBSpatialCrop, TemporalCropAndOffset,
                                        TemporalCropAndOffsetForSyncabilityTraining)

    def chain(mode, n_seg, train):
        if mode == 'grid':
            tco = TemporalCropAndOffset(crop_len_sec=5, max_off_sec=2, max_wiggle_sec=0.05 if train else 0.0, do_offset=True, offset_type='grid',
                                        grid_size=21, segment_size_vframes=16, n_segments=n_seg, step_size_seg=0.5, vfps=25)
        else:
            tco = TemporalCropAndOffsetForSyncabilityTraining(max_off_sec=2, max_wiggle_sec=0.05, do_offset=True, grid_size=21,
                                                              segment_size_vframes=16, n_segments=n_seg, step_size_seg=0.5, vfps=25)
        return [EqualifyFromRight(clip_max_len_sec=10), RGBSpatialCrop(224, is_random=train), tco,
                GenerateMultipleSegments(segment_size_vframes=16, n_segments=n_seg, is_start_random=train, step_size_seg=0.5)]

    def run(ts, item, mode):
        item = ts[0](item)
        item = ts[1](item)
        v = int(item['video'][0, 0, 0, 0])
        y0, x0 = (v % 1000000) // 1000, v % 1000
        item = ts[2](item)
        v_start_i = int(item['video'][0, 0, 0, 0]) // 1000000
        item = ts[3](item)
        frame0 = int(item['video'][0, 0, 0, 0, 0]) // 1000000
        a0 = int(item['audio'][0, 0])
        tg = item['targets']
        target = int(tg['sync_target']) if mode == 'syncability' else int(tg['offset_target'])
        return [1, y0, x0, v_start_i, a0, frame0, int(round(tg['offset_sec'] * 100)), target, int(item['meta'].get('a_jitter_i', 0))]

    rows = []
    for ci, (mode, n_seg, v_len, a_len, H, W) in enumerate(CASES):
        ts = chain(mode, n_seg, True)
        n_ok = 0
        for k in range(N_SEEDS):
            random.seed(k)
            try:
                r = run(ts, _item(v_len, a_len, H, W), mode)
                n_ok += 1
            except Exception:       # AssertionError, Exception or ValueError: the reference's asserts / raise Exception / an empty randint range
                r = [0] + [0] * 8
            rows.append([ci, k] + r)
        print(f'case {ci} {CASES[ci]}: {n_ok}/{N_SEEDS} items built')
    ts = chain('grid', 14, False)
    for fi, (off, vs) in enumerate(FIXED):
        try:
            r = run(ts, _item(250, 160000, 256, 340, dict(offset_sec=off, v_start_i_sec=vs), split='valid'), 'grid')
        except Exception:
            r = [0] + [0] * 8
        rows.append([len(CASES) + fi, -1] + r)
        print('fixed', (off, vs), r)
    np.savez_compressed(HERE / 'train_crops.npz', rows=np.array(rows, dtype=np.int64), columns=np.array(COLUMNS),
                        cases=np.array([[0 if m == 'grid' else 1, n, v, a, h, w] for m, n, v, a, h, w in CASES], dtype=np.int64),
                        fixed_x100=np.array([[int(round(o * 100)), int(round(s * 100))] for o, s in FIXED], dtype=np.int64))


if __name__ == '__main__':
    main()
