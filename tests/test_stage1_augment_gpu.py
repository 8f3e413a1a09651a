"""GPU: the Stage-1 train-time augmentations from raw clips (sf_stage1_video_augment, sf_stage1_audio_augment, AVCLIPTrainer.train_step_clips)
against the CPU oracle of tests/stage1_augment_oracle.py.  Inputs: 2 clips of 40 frames, 232 x 250 (W no multiple of 4), odd x0, origins at 0 and
at the far edge, 2 segments per clip, content that differs per frame; the clip tensors are views into larger allocations, so a missing clamp
could not leave them."""
import numpy as np
import pytest
import torch

import stage1_augment_oracle as R
from synchformer_amd import augment as A

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope='module')
def dev_clips(gpu):
    big = torch.zeros(R.clips().numel() + 2 * 65536, dtype=torch.uint8, device=gpu)
    view = big[65536:65536 + R.clips().numel()].view(R.clips().shape)
    view.copy_(R.clips())
    return view


@pytest.fixture(scope='module')
def dev_waves(gpu):
    big = torch.zeros(R.waves().numel() + 2 * 16384, dtype=torch.float32, device=gpu)
    view = big[16384:16384 + R.waves().numel()].view(R.waves().shape)
    view.copy_(R.waves())
    return view


def _video(frames, clip_table, seg_table, n_seg, v_stride):
    from synchformer_amd import ops
    n = frames.shape[0] * n_seg
    out = torch.full((n, 16, 3, 224, 224), 77, dtype=torch.uint8, device=frames.device)
    sums = torch.full((n * 16,), -1, dtype=torch.int32, device=frames.device)
    ops.stage1_video_augment(frames, clip_table.to(frames.device), seg_table.to(frames.device), out, sums, v_stride, n_seg)
    torch.cuda.synchronize()
    return out.cpu()


def _audio(wave, clip_table, seg_table, n_seg, a_stride=10240, a_size=10240):
    from synchformer_amd import ops
    out = torch.full((wave.shape[0] * n_seg, a_size), 9.0, dtype=torch.float32, device=wave.device)
    ops.stage1_audio_augment(wave, clip_table.to(wave.device), seg_table.to(wave.device), out, a_stride, n_seg, A.lowpass_coeffs(), 0.01)
    torch.cuda.synchronize()
    return out.cpu()


def test_crop_flip_gray_bit_identical_to_host_slicing(dev_clips):
    """Case 1: no arithmetic but the gray - bit-identical to slicing on the host."""
    for rows in (R.CROP_ROWS, [[8, 8, 26, 224, 0], [0, 0, 0, 224, 0]]):
        clip_table = R.clip_rows(rows)
        seg_table = R.seg_rows(4, gray=[0, 1, 0, 1], flip=[0, 0, 1, 1])
        got = _video(dev_clips, clip_table, seg_table, 2, 16)
        want = R.video_augment(R.clips(), clip_table, seg_table, 2, 16, F32)
        assert torch.equal(got, want)
        # the oracle's no-op path is plain slicing
        f0, y0, x0 = rows[0][:3]
        assert torch.equal(got[0], R.clips()[0, f0:f0 + 16, :, y0:y0 + 224, x0:x0 + 224])
        assert torch.equal(got[2], R.clips()[1, rows[1][0]:rows[1][0] + 16, :, rows[1][1]:rows[1][1] + 224, rows[1][2]:rows[1][2] + 224].flip(-1))


@pytest.mark.parametrize('op', ['brightness', 'saturation', 'contrast'])
def test_blend_ops_alone_bit_identical_to_fp32_oracle(dev_clips, op):
    """Case 2: each blend op alone (the other three are in the order with a ratio of 1 / a hue shift of 0, which change nothing - asserted on the
    oracle), ratios at both ends of the range and inside it."""
    code = dict(brightness=0, contrast=1, saturation=2)[op]
    order = [code] + [c for c in range(4) if c != code]
    ratios = [0.2, 0.6431, 1.3127, 1.8]
    key = dict(brightness='bright', contrast='contrast', saturation='satur')[op]
    seg_table = R.seg_rows(4, jitter=[1] * 4, order=[order] * 4, flip=[0, 1, 0, 0], **{key: ratios})
    clip_table = R.clip_rows(R.CROP_ROWS)
    got = _video(dev_clips, clip_table, seg_table, 2, 16)
    want = R.video_augment(R.clips(), clip_table, seg_table, 2, 16, F32)
    assert torch.equal(got, want)
    x = R.crop(R.clips()[0, 0:16], 0, 13, 224, F32)
    alone = getattr(R, op)(x, float(np.float32(ratios[0])), F32)
    assert torch.equal(want[0], alone) and not torch.equal(alone, x)


def test_contrast_mean_is_per_frame_and_of_the_modified_image(dev_clips):
    """Case 3: contrast behind brightness (and behind saturation + brightness): the mean is the frame's own, of the image as contrast finds it."""
    seg_table = R.seg_rows(4, jitter=[1] * 4, order=[[0, 1, 2, 3], [0, 1, 2, 3], [2, 0, 1, 3], [3, 0, 1, 2]], bright=[1.7, 0.4, 1.5, 0.8],
                           contrast=[0.3, 1.75, 0.5, 1.4], satur=[1.0, 1.0, 1.6, 1.0])
    clip_table = R.clip_rows(R.CROP_ROWS)
    got = _video(dev_clips, clip_table, seg_table, 2, 16)
    want = R.video_augment(R.clips(), clip_table, seg_table, 2, 16, F32)
    assert torch.equal(got, want)
    # the test can tell: the frames of the segment differ strongly in brightness, and a mean of the unmodified image or of the whole segment is another result
    x = R.crop(R.clips()[0, 0:16], 0, 13, 224, F32)
    b = R.brightness(x, float(np.float32(1.7)), F32)
    means = R.gray(b, F32).float().mean(dim=(1, 2, 3))
    assert float(means.max() / means.min()) > 3
    r = float(np.float32(0.3))
    whole = R.blend(b, R.gray(b, F32).float().mean(), r, F32)
    unmodified = R.blend(b, R.gray(x, F32).float().mean(dim=(1, 2, 3), keepdim=True), r, F32)
    assert not torch.equal(want[0], whole) and not torch.equal(want[0], unmodified)


def test_hue_alone(dev_clips):
    """Case 4: within 1 level of the fp64 oracle at every pixel, differing from the fp32 oracle on <= 1e-3 of the pixels."""
    clip_table, seg_table, n_seg, v_stride = R.hue_case()
    got = _video(dev_clips, clip_table, seg_table, n_seg, v_stride)
    d64, s64 = R.compare(got, R.reference('hue', 'float64'))
    d32, s32 = R.compare(got, R.reference('hue', 'float32'))
    print(f'hue: vs fp64 max {d64} level(s), share {s64:.3e}; vs fp32 max {d32}, share {s32:.3e}')
    assert d64 <= 1 and s32 <= 1e-3, (d64, s64, d32, s32)
    assert not torch.equal(got[0], R.crop(R.clips()[0, 0:16], 0, 13, 224, F32))


def test_upscaled_crop(dev_clips):
    """Case 5: within 1 level of F.interpolate(x.double(), 224, 'bilinear', align_corners=False).round() at every pixel, differing on <= 1e-2."""
    clip_table, seg_table, n_seg, v_stride = R.upscale_case()
    got = _video(dev_clips, clip_table, seg_table, n_seg, v_stride)
    want = R.reference('upscale', 'float64')
    x = R.clips()[1, 8:24, :, 40:232, 58:250].double()
    assert torch.equal(want[2], torch.nn.functional.interpolate(x, 224, mode='bilinear', align_corners=False).round().to(torch.uint8))
    d, share = R.compare(got, want)
    d32, s32 = R.compare(got, R.reference('upscale', 'float32'))
    print(f'upscale: vs fp64 max {d} level(s), share {share:.3e}; vs fp32 max {d32}, share {s32:.3e}')
    assert d <= 1 and share <= 1e-2, (d, share)


def test_all_24_orders(dev_clips):
    """Case 6: 24 segments, one op order each, random factors, mixed with gray, flip and the 192 crop (clip 1), checked on 4 of each segment's 16
    frames (a frame does not depend on the others).  Per segment, the share of pixels that differ from the fp32 oracle stays under the cap of the one
    inexact op in front of the chain - 1e-3 (hue, case 4), or 1e-2 behind the resampling (case 5) - so a wrong order, mean or factor, which changes
    nearly every pixel, cannot pass.  Against fp64 the chain cannot be held to one level at EVERY pixel: an op's one-level disagreement is carried
    through the ops behind it and amplified, and the fp32 oracle itself ends up to 9 levels from the fp64 one on these inputs
    (tests/test_stage1_augment_cpu.py::test_oracle_chained_ops_carry_a_level_along); what is asserted is that the share of pixels more than one
    level from fp64 stays under the same caps."""
    clip_table, seg_table, n_seg, v_stride = R.orders_case()
    got = _video(dev_clips, clip_table, seg_table, n_seg, v_stride)[:, list(R.ORDER_FRAMES)]
    w32, w64 = R.reference('orders', 'float32'), R.reference('orders', 'float64')
    worst = {}
    for n in range(24):
        side = int(clip_table[n // n_seg, 3])
        cap = 1e-2 if side == 192 else 1e-3
        d32, s32 = R.compare(got[n], w32[n])
        over = float(((got[n].to(torch.int16) - w64[n].to(torch.int16)).abs() > 1).float().mean())
        worst[side] = max(worst.get(side, (0, 0)), (s32, over))
        assert s32 <= cap and over <= cap, (n, side, d32, s32, over)
    print(f'orders: worst (share differing from fp32, share more than 1 level from fp64) per crop side: {worst}')


def test_out_of_range_rows_equal_the_clamped_rows(dev_clips, dev_waves):
    """Case 7: every clip entry out of range in both directions, a side that is no crop size, op codes outside 0..3 (no op)."""
    seg_table = R.seg_rows(4, jitter=[1] * 4, order=[[0, 7, 2, -1], [4, 0, 9, 2], [0, 1, 2, 3], [5, 6, 7, 8]], bright=[1.3] * 4, satur=[0.5] * 4,
                           contrast=[1.2] * 4, audio=[1, 0, 1, 0])
    for bad in ([[-5, -3, -9, 224, -7], [99, 500, 300, 100, 10 ** 6]], [[10 ** 6, 10 ** 6, 10 ** 6, 192, 2 ** 31 - 1], [-2 ** 31, -1, 251, 0, -2 ** 31]]):
        bad = R.clip_rows(bad)
        ok, _ = R.clamp_tables(bad, seg_table, 2, 16, 10240, 10240, R.T, R.N_SAMPLES, R.H, R.W)
        A.Stage1Batch(clip_table=ok, seg_table=R.seg_rows(4), n_seg=2).validate(R.T, R.N_SAMPLES, R.H, R.W)
        assert torch.equal(_video(dev_clips, bad, seg_table, 2, 16), _video(dev_clips, ok, seg_table, 2, 16))
        assert torch.equal(_audio(dev_waves, bad, seg_table, 2), _audio(dev_waves, ok, seg_table, 2))
    ok = R.clip_rows(R.CROP_ROWS)
    got = _video(dev_clips, ok, seg_table, 2, 16)
    assert torch.equal(got, R.video_augment(R.clips(), ok, seg_table, 2, 16, F32))
    x0 = R.crop(R.clips()[0, 0:16], 0, 13, 224, F32)
    assert torch.equal(got[0], R.saturation(R.brightness(x0, float(np.float32(1.3)), F32), float(np.float32(0.5)), F32))      # codes 7 and -1 skipped
    assert torch.equal(got[3], R.clips()[1, 24:40, :, 8:232, 26:250])                   # four unknown codes: the crop


def test_audio_gather_volume_lowpass(dev_waves):
    """Case 8, first half: the gather (with the jitter in sample0) and the volume are exact, untouched segments are the input bit for bit, the
    lowpass stays within 4 x the fp32 CPU recurrence's own error of the fp64 oracle (floor 1e-6; the factor allows another rounding order)."""
    clip_table = R.clip_rows(R.CROP_ROWS)                              # sample0 3 and the last possible start
    seg_table = R.seg_rows(4, audio=[0, A.S1_AUDIO_VOLUME, A.S1_AUDIO_LOWPASS, A.S1_AUDIO_VOLUME | A.S1_AUDIO_LOWPASS])
    got = _audio(dev_waves, clip_table, seg_table, 2)
    x = R.audio_gather(R.waves(), clip_table, 2, 10240, 10240)
    assert torch.equal(x[0], R.waves()[0, 3:3 + 10240]) and torch.equal(x[3], R.waves()[1, R.N_SAMPLES - 10240:])
    assert torch.equal(got[0], x[0])
    assert torch.equal(got[1], R.volume(x[1])) and float(got[1].abs().max()) == 1.0 and not torch.equal(got[1], x[1])
    pre = torch.stack([x[2], R.volume(x[3])]).numpy()
    y64, y32 = R.lowpass(pre, A.lowpass_coeffs(), np.float64), R.lowpass(pre, A.lowpass_coeffs(), np.float32)
    bound = max(4 * float(np.abs(y32 - y64).max()), 1e-6)
    err = float(np.abs(got[2:4].numpy().astype(np.float64) - y64).max())
    print(f'lowpass: max |gpu - fp64| {err:.3e}, bound {bound:.3e} (fp32 CPU recurrence {bound / 4:.3e}); output peak {np.abs(y64).max():.3f}')
    assert err <= bound and np.abs(y64).max() > 0.05, (err, bound)


def test_audio_noise(dev_waves):
    """Case 8, second half: the same seed gives the same noise, segments differ, sample mean and std within 5 standard errors of 0 and 0.01, no
    correlation with the neighbouring sample beyond 5 / sqrt(N); the noise rides on the lowpass output too."""
    clip_table = R.clip_rows(R.CROP_ROWS)
    seg_table = R.seg_rows(4, audio=[A.S1_AUDIO_NOISE] * 3 + [A.S1_AUDIO_NOISE | A.S1_AUDIO_LOWPASS], seed=[12345, -7, 12345, 12345])
    quiet = R.seg_rows(4, audio=[0, 0, 0, A.S1_AUDIO_LOWPASS])
    got, base = _audio(dev_waves, clip_table, seg_table, 2), _audio(dev_waves, clip_table, quiet, 2)
    assert torch.equal(got, _audio(dev_waves, clip_table, seg_table, 2))
    noise = (got.double() - base.double()).numpy()
    N = noise.shape[1]
    assert np.abs(noise[0] - noise[2]).max() < 3e-7 and np.abs(noise[0] - noise[3]).max() < 3e-7      # one seed, one noise (up to the fp32 adds: 2 x 2^-24 x 2)
    assert np.abs(noise[0] - noise[1]).max() > 0.01
    for n in (0, 1):
        z = noise[n]
        assert abs(z.mean()) <= 5 * 0.01 / np.sqrt(N), z.mean()
        assert abs(z.std() - 0.01) <= 5 * 0.01 / np.sqrt(2 * N), z.std()
        zc = (z - z.mean()) / z.std()
        assert abs(float((zc[1:] * zc[:-1]).mean())) <= 5 / np.sqrt(N)
        assert abs(float((zc ** 4).mean()) - 3) <= 5 * np.sqrt(96 / N) and np.abs(zc).max() < 6           # a normal's kurtosis, no wild samples
    z0, z1 = (noise[0] - noise[0].mean()) / noise[0].std(), (noise[1] - noise[1].mean()) / noise[1].std()
    assert abs(float((z0 * z1).mean())) <= 5 / np.sqrt(N)


@pytest.mark.parametrize('two_streams', [True, False])
def test_train_step_clips(gpu, dev_clips, dev_waves, two_streams):
    """Case 9, B = 1, S = 2: with every augmentation off train_step_clips gives the loss and the gradients of train_step on the host-sliced segments
    and MelFrontend of the host-sliced waves, bit for bit; with augmentations on, those of train_step fed the device-augmented buffers."""
    from synchformer_amd import ops, synth
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.stage1 import AVCLIPTrainer
    sd = {k: v for k, v in synth.make_state_dict(1337).items() if k.startswith(('vfeat_extractor.', 'afeat_extractor.'))}
    tr, ref = AVCLIPTrainer(sd, gpu, lr=1e-4), AVCLIPTrainer(sd, gpu, lr=1e-4)
    tr.two_streams = ref.two_streams = two_streams
    mel = MelFrontend(gpu)
    frames, wave = dev_clips[1:2], dev_waves[1:2]
    clip_table = R.clip_rows([[8, 8, 25, 224, 777]])

    def same(what):
        torch.cuda.synchronize()
        assert torch.equal(tr.loss, ref.loss) and torch.isfinite(tr.loss).all(), what
        assert torch.equal(tr.flat_g, ref.flat_g) and float(tr.flat_g.abs().max()) > 0, what

    off = A.Stage1Batch(clip_table=clip_table, seg_table=R.seg_rows(2), n_seg=2)
    off.validate(R.T, R.N_SAMPLES, R.H, R.W)
    tr.train_step_clips(frames, wave, mel, off.to(gpu))
    vis = torch.stack([R.clips()[1, 8 + 16 * s:8 + 16 * s + 16, :, 8:232, 25:249] for s in range(2)]).unsqueeze(0)
    wav = torch.stack([R.waves()[1, 777 + 10240 * s:777 + 10240 * (s + 1)] for s in range(2)]).unsqueeze(0)
    ref.train_step(vis.to(gpu), mel(wav.to(gpu)))
    same('augmentations off')

    on = A.Stage1Batch(clip_table=R.clip_rows([[3, 40, 57, 192, 5000]]), n_seg=2,
                       seg_table=R.seg_rows(2, jitter=[1, 1], order=[[2, 0, 3, 1], [1, 3, 0, 2]], bright=[1.4, 0.7], contrast=[0.6, 1.5], satur=[1.6, 0.4],
                                            hue=[0.15, -0.1], gray=[0, 1], flip=[1, 0], audio=[7, 3], seed=[42, 43]))
    on.validate(R.T, R.N_SAMPLES, R.H, R.W)
    dev_on = on.to(gpu)
    tr.train_step_clips(frames, wave, mel, dev_on)
    seg = torch.empty(2, 16, 3, 224, 224, dtype=torch.uint8, device=gpu)
    ops.stage1_video_augment(frames, dev_on.clip_table, dev_on.seg_table, seg, torch.empty(32, dtype=torch.int32, device=gpu), 16, 2)
    seg_wave = torch.empty(2, 10240, dtype=torch.float32, device=gpu)
    ops.stage1_audio_augment(wave, dev_on.clip_table, dev_on.seg_table, seg_wave, 10240, 2, on.lowpass, on.noise_amp)
    assert not torch.equal(seg.cpu(), vis[0])
    ref.train_step(seg.unsqueeze(0), mel(seg_wave.unsqueeze(0)))
    same('augmentations on')
    assert torch.equal(tr.flat_p, ref.flat_p)
