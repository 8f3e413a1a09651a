"""Fixture for synchformer_amd.augment.Stage1Sampler: the REAL reference functions behind the Python-`random` draws of the Stage-1 train
transforms (configs/segment_avclip.yaml), run on seeded items, recording what they return.

    python tests/golden/make_stage1_crops.py        # writes tests/golden/stage1_crops.npz

Per item, under random.seed(k), in the order of transform_sequence_train:
    EqualifyFromRight -> RGBSpatialCrop.get_random_crop_sides(video, (side, side)) -> GenerateMultipleSegments(segment_size_vframes=16, n_segments=14,
    is_start_random=True, audio_jitter_sec=0.05, step_size_seg=1.0).get_sequential_seg_ranges(...)
`side` is 224, or 192 for the items RGBSpatialCropSometimesUpscale would send through the smaller crop - that decision is a torch.rand draw, not part
of the Python stream, so it is an input here (odd seeds take the 192 crop).  The classes that build torchvision objects (RGBSpatialCropSometimesUpscale,
RandomApplyColorDistortion, ...) cannot be instantiated under the import shims; the two functions above can.  Only integers are stored.
"""
import random
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import ref_import  # noqa: E402

N_SEEDS = 60
# case id -> (v_len, a_len, H, W)
CASES = [
    (250, 160000, 256, 256),          # 10 s, 256-side
    (250, 160000, 256, 340),          # non-square
    (224, 143360, 256, 256),          # exactly 14 segments: max_v_start_i = 0, the jitter clamps to 0
    (260, 150000, 257, 300),          # audio shorter than video: EqualifyFromRight trims both
    (230, 147200, 224, 224),          # no 224 crop draws when the frame is the crop size (the 192 crop still draws)
    (225, 144000, 256, 256),          # one spare frame: the jitter clamps to 0 from the left (start 0) or from the right (start 1)
    (200, 128000, 256, 256),          # too short for 14 segments: asserts
]
COLUMNS = ['case', 'seed', 'ok', 'side', 'y0', 'x0', 'frame0', 'sample0', 'a_jitter_i']


def main():
    ref_import.import_reference_avclip()                  # late shims: dataset.transforms imports torchvision / torchaudio
    with ref_import._cwd(ref_import.REF):
        from dataset.transforms import EqualifyFromRight, GenerateMultipleSegments, RGBSpatialCrop
    eq = EqualifyFromRight(clip_max_len_sec=10)
    gms = GenerateMultipleSegments(segment_size_vframes=16, n_segments=14, is_start_random=True, audio_jitter_sec=0.05, step_size_seg=1.0)

    def run(v_len, a_len, H, W, side):
        item = dict(video=torch.zeros(v_len, 1, 1, 1, dtype=torch.uint8).expand(v_len, 3, H, W), audio=torch.arange(a_len, dtype=torch.float64),
                    path='synthetic', split='train', meta=dict(video=dict(fps=[25.0]), audio=dict(framerate=[16000.0])))
        item = eq(item)
        y0, x0, _, _ = RGBSpatialCrop.get_random_crop_sides(item['video'], (side, side))
        v_len, a_len = item['video'].shape[0], item['audio'].shape[0]
        seg_a = int(16 / 25 * 16000)
        # GenerateMultipleSegments.forward's own check in front of get_sequential_seg_ranges (transforms.py:436-444)
        assert 14 <= min((v_len - 16) // 16 + 1, (a_len - seg_a) // seg_a + 1)
        v_ranges, a_ranges = gms.get_sequential_seg_ranges(v_len, a_len, 25, 16000, 14, seg_a)
        frame0, sample0 = int(v_ranges[0, 0]), int(a_ranges[0, 0])
        assert [int(v) for v in v_ranges[:, 0]] == [frame0 + 16 * i for i in range(14)] and [int(a) for a in a_ranges[:, 0]] == [sample0 + seg_a * i for i in range(14)]
        return [1, side, y0, x0, frame0, sample0, sample0 - int(frame0 / 25 * 16000)]

    rows = []
    for ci, (v_len, a_len, H, W) in enumerate(CASES):
        n_ok = 0
        for k in range(N_SEEDS):
            random.seed(k)
            side = 192 if k % 2 else 224
            try:
                r = run(v_len, a_len, H, W, side)
                n_ok += 1
            except (AssertionError, ValueError):       # the reference's asserts / an empty randint range
                r = [0, side, 0, 0, 0, 0, 0]
            rows.append([ci, k] + r)
        print(f'case {ci} {CASES[ci]}: {n_ok}/{N_SEEDS} items built')
    np.savez_compressed(HERE / 'stage1_crops.npz', rows=np.array(rows, dtype=np.int64), columns=np.array(COLUMNS), cases=np.array(CASES, dtype=np.int64))


if __name__ == '__main__':
    main()
