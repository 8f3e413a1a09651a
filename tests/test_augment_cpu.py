"""CPU: synchformer_amd.augment.ClipSampler reproduces the REAL reference train transforms draw for draw (tests/golden/train_crops.npz,
written by tests/golden/make_train_crops.py), raises where they raise, and its batches validate / trim on the host."""
import random
from pathlib import Path

import numpy as np
import pytest
import torch

GOLD = Path(__file__).resolve().parent / 'golden'


def _load():
    g = np.load(GOLD / 'train_crops.npz')
    cols = [str(c) for c in g['columns']]
    return g, cols


def _sampler(mode_id, n_seg):
    from synchformer_amd.augment import ClipSampler
    return ClipSampler('grid' if mode_id == 0 else 'syncability', n_segments=int(n_seg))


def _check(batch, r, c, v_len, a_len):
    assert batch.table.dtype == torch.int32 and batch.table.shape == (1, 4)
    frame0, y0, x0, _ = batch.table[0].tolist()
    got = dict(y0=y0, x0=x0, frame_seg0=frame0, a_start_i_seg0=int(batch.sample0[0]), target=int(batch.targets[0]),
               offset_sec_x100=int(round(batch.offset_sec[0] * 100)), v_start_i=int(round(batch.v_start_i_sec[0] * 25)),
               a_jitter_i=int(batch.a_jitter_i[0]))
    want = {k: int(r[c.index(k)]) for k in got}
    assert got == want, (got, want)


def test_sampler_reproduces_reference_draws():
    from synchformer_amd.augment import ClipSampler  # noqa: F401
    g, c = _load()
    rows, cases = g['rows'], g['cases']
    n_ok = n_raise = n_left = n_right = 0
    for r in rows:
        ci, seed, ok = int(r[0]), int(r[1]), int(r[2])
        if ci >= len(cases):
            continue
        mode_id, n_seg, v_len, a_len, H, W = (int(x) for x in cases[ci])
        s = _sampler(mode_id, n_seg)
        rng = random.Random(seed)
        if not ok:
            with pytest.raises(ValueError):
                s.sample(rng, [v_len], [a_len], H, W, torch.Generator().manual_seed(0))
            n_raise += 1
            continue
        b = s.sample(rng, [v_len], [a_len], H, W, torch.Generator().manual_seed(0))
        _check(b, r, c, v_len, a_len)
        n_ok += 1
        # which reference branches the row went through (recomputed from the recorded values)
        off, v0 = int(r[c.index('offset_sec_x100')]) / 100, int(r[c.index('v_start_i')])
        a_raw = int((v0 / 25 + off) * 16000)
        a_fixed = max(a_raw, 0) if mode_id == 0 else a_raw
        crop_a = 80000 if mode_id == 0 else int(round(7 * 0.64, 2) * 16000)
        a_len_eq = int(640 * int(25 * min(10, a_len / 16000, v_len / 25)))
        n_left += a_fixed < 800
        n_right += (a_len_eq - crop_a) - a_fixed < 800
    assert n_ok >= 1500 and n_raise >= 250, (n_ok, n_raise)
    assert n_left >= 1 and n_right >= 1, (n_left, n_right)     # the jitter clamped at both ends (the a_start_i < 0 fix-up: the fixed-offset test)


def test_sampler_fixed_offsets_match_reference():
    from synchformer_amd.augment import ClipSampler
    g, c = _load()
    rows, cases, fixed = g['rows'], g['cases'], g['fixed_x100']
    s = ClipSampler('grid')
    seen_fixup = False
    for r in rows:
        fi = int(r[0]) - len(cases)
        if fi < 0:
            continue
        off, vs = int(fixed[fi][0]) / 100, int(fixed[fi][1]) / 100
        if not int(r[2]):
            with pytest.raises(ValueError):
                s.fixed([off], [vs], [250], [160000], 256, 340)
            continue
        b = s.fixed([off], [vs], [250], [160000], 256, 340)
        _check(b, r, c, 250, 160000)
        assert int(b.table[0, 3]) == 0
        seen_fixup |= int((vs + off) * 16000) < 0
    assert seen_fixup
    with pytest.raises(ValueError):
        ClipSampler('syncability').fixed([0.0], [1.0], [250], [160000], 256, 256)


def test_sampler_batches_draw_clip_by_clip():
    """A batch of clips of different lengths draws clip after clip from one rng: the same rows as one-clip calls in sequence."""
    from synchformer_amd.augment import ClipSampler
    s = ClipSampler('grid')
    lens = [(250, 160000), (175, 112000), (240, 155000)]
    b = s.sample(random.Random(5), [v for v, _ in lens], [a for _, a in lens], 256, 340, torch.Generator().manual_seed(3))
    rng = random.Random(5)
    for i, (v, a) in enumerate(lens):
        one = s.sample(rng, [v], [a], 256, 340, torch.Generator().manual_seed(0))
        assert b.table[i, :3].tolist() == one.table[0, :3].tolist() and int(b.sample0[i]) == int(one.sample0[0])
        assert int(b.targets[i]) == int(one.targets[0])
    assert b.n_seg == 14 and b.v_span == 120 and b.a_span == 76800 and b.a_size == 10240


def test_flip_rate_and_generator():
    from synchformer_amd.augment import ClipSampler
    s = ClipSampler('grid')
    b = s.sample(random.Random(0), [250] * 400, [160000] * 400, 256, 256, torch.Generator().manual_seed(11))
    f = b.table[:, 3]
    assert set(f.tolist()) <= {0, 1} and 160 < int(f.sum()) < 240
    b2 = s.sample(random.Random(0), [250] * 400, [160000] * 400, 256, 256, torch.Generator().manual_seed(11))
    assert torch.equal(b.table, b2.table)
    assert int(ClipSampler('grid', p_flip=0.0).sample(random.Random(0), [250] * 50, [160000] * 50, 256, 256).table[:, 3].sum()) == 0


def test_validate_and_trim():
    from synchformer_amd.augment import ClipSampler
    s = ClipSampler('syncability')
    b = s.sample(random.Random(1), [250, 250], [160000, 160000], 256, 300, torch.Generator().manual_seed(1))
    frames = torch.randint(0, 256, (2, 250, 3, 256, 300), dtype=torch.uint8)
    wave = torch.randn(2, 160000)
    fw, ww, rel = b.trim(frames, wave)
    assert fw.shape == (2, b.v_span, 3, 256, 300) and ww.shape == (2, b.a_span)
    assert rel.table[:, 0].tolist() == [0, 0] and rel.sample0.tolist() == [0, 0] and torch.equal(rel.table[:, 1:], b.table[:, 1:])
    for i in range(2):
        f0, s0 = int(b.table[i, 0]), int(b.sample0[i])
        assert torch.equal(fw[i], frames[i, f0:f0 + b.v_span]) and torch.equal(ww[i], wave[i, s0:s0 + b.a_span])
    rel.validate(b.v_span, b.a_span, 256, 300)
    for col, val in ((0, 1), (1, 33), (2, 77), (2, -1)):
        bad = rel.table.clone()
        bad[0, col] = val
        with pytest.raises(ValueError):
            type(rel)(table=bad, sample0=rel.sample0, targets=rel.targets, n_seg=rel.n_seg).validate(b.v_span, b.a_span, 256, 300)
    with pytest.raises(ValueError):
        type(rel)(table=rel.table, sample0=rel.sample0 + 1, targets=rel.targets, n_seg=rel.n_seg).validate(b.v_span, b.a_span, 256, 300)
