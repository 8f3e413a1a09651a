"""GPU: Stage-2 train inputs from raw clips (synchformer_amd.augment, sf_im2col_video_crops, sf_mel_frontend_starts, train_step_clips).

The crop / flip / segment gather and the per-clip log-mel must be BIT-identical to the existing kernels on the same inputs materialised with
torch slicing + flip(-1); a train step from raw clips must equal train_step on the materialised inputs (bit for bit unless train_step itself
differs from run to run - then within that spread, measured here)."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

N_CLIPS, T, H, W = 3, 250, 256, 340


def _clips(dev, seed=0, n=N_CLIPS, t=T, h=H, w=W):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (n, t, 3, h, w), dtype=torch.uint8, generator=g)
    wave = torch.randn(n, 160000, generator=g) * 0.1
    return frames.to(dev), wave.to(dev)


def _segments(frames, table, stride, n_seg):
    """(B, n_seg, 16, 3, 224, 224) uint8: the crops materialised with torch slicing (+ flip(-1))."""
    out = []
    for b, (f0, y0, x0, fl) in enumerate(table.tolist()):
        segs = torch.stack([frames[b, f0 + s * stride:f0 + s * stride + 16, :, y0:y0 + 224, x0:x0 + 224] for s in range(n_seg)])
        out.append(segs.flip(-1) if fl else segs)
    return torch.stack(out).contiguous()


# every crop corner / flip combination: x0 = 0, W - 224 and odd; y0 = 0, H - 224 and odd; frame0 at both ends of the clip
TABLES = [
    [[0, 0, 0, 0], [130, H - 224, W - 224, 1], [57, 7, 37, 0]],
    [[0, 0, 0, 1], [130, H - 224, W - 224, 0], [57, 7, 37, 1]],
    [[3, 31, 1, 0], [64, 1, 115, 1], [129, 0, 113, 1]],
]


@pytest.mark.parametrize('ti', range(len(TABLES)))
def test_im2col_video_crops_bit_identical(gpu, ti):
    from synchformer_amd import ops
    frames, _ = _clips(gpu, seed=ti)
    n_seg, stride = 14, 8
    table = torch.tensor(TABLES[ti], dtype=torch.int32)
    segs = _segments(frames, table, stride, n_seg).view(N_CLIPS * n_seg, 16, 3, 224, 224)
    tdev = table.to(gpu)
    n = N_CLIPS * n_seg
    for tokens, rows in ((True, 1569), (False, 1568)):
        got = torch.full((n * rows, 1536), float('nan'), device=gpu, dtype=torch.bfloat16)
        ops.im2col_video_crops(frames, tdev, got, stride, n_seg, tokens=tokens)
        want = torch.empty_like(got)
        if tokens:
            ops.im2col_video_tokens(segs, want)
        else:
            ops.im2col_video(segs, want)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (ti, tokens)


def test_im2col_video_crops_square_and_exact_size(gpu):
    """H = W = 256 (the configs' size_before_crop) and frames already 224 x 224 (crop at 0, 0); 13 segments (fine-tune)."""
    from synchformer_amd import ops
    for h, w, rows in ((256, 256, [[0, 32, 32, 1], [100, 0, 31, 0]]), (224, 224, [[5, 0, 0, 1], [0, 0, 0, 0]])):
        frames, _ = _clips(gpu, seed=h, n=2, t=120, h=h, w=w)
        table = torch.tensor(rows, dtype=torch.int32)
        n_seg = 13
        rows_ok = [[min(r[0], 120 - 112)] + r[1:] for r in rows]
        segs = _segments(frames, torch.tensor(rows_ok, dtype=torch.int32), 8, n_seg).view(2 * n_seg, 16, 3, 224, 224)
        got = torch.empty((2 * n_seg * 1569, 1536), device=gpu, dtype=torch.bfloat16)
        ops.im2col_video_crops(frames, torch.tensor(rows_ok, dtype=torch.int32, device=gpu), got, 8, n_seg)
        want = torch.empty_like(got)
        ops.im2col_video_tokens(segs, want)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (h, w)


def test_im2col_video_crops_clamps_rows_into_the_clip(gpu):
    """The launcher cannot read the device table: a row outside the clip is clamped into it by the kernel (reads stay inside the clip)."""
    from synchformer_amd import ops
    frames, _ = _clips(gpu, seed=5, n=2, t=130)
    bad = torch.tensor([[10 ** 6, -5, W + 50, 1], [-3, H, -7, 0]], dtype=torch.int32)
    clamped = torch.tensor([[130 - 120, 0, W - 224, 1], [0, H - 224, 0, 0]], dtype=torch.int32)
    got = torch.empty((2 * 14 * 1569, 1536), device=gpu, dtype=torch.bfloat16)
    want = torch.empty_like(got)
    ops.im2col_video_crops(frames, bad.to(gpu), got, 8, 14)
    ops.im2col_video_crops(frames, clamped.to(gpu), want, 8, 14)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    with pytest.raises(RuntimeError):
        ops.im2col_video_crops(frames[:, :100].contiguous(), clamped.to(gpu), got, 8, 14)         # 14 segments need 120 frames


def test_mel_frontend_starts_bit_identical(gpu):
    from synchformer_amd.frontend import MelFrontend
    _, wave = _clips(gpu, seed=1)
    mel = MelFrontend(gpu)
    n_seg, stride, size = 14, 5120, 10240
    starts = [0, 12345, 160000 - (n_seg - 1) * stride - size]
    s0 = torch.tensor(starts, dtype=torch.int64, device=gpu)
    got = mel.segments_at(wave, s0, stride, n_seg, size)
    segs = torch.stack([torch.stack([wave[b, a + s * stride:a + s * stride + size] for s in range(n_seg)]) for b, a in enumerate(starts)])
    want = mel(segs.contiguous())
    torch.cuda.synchronize()
    assert got.shape == want.shape == (N_CLIPS, n_seg, 1, 128, 66)
    assert torch.equal(got, want)
    # equal starts: the same as the one-start launcher
    same = mel.segments_at(wave, torch.full((N_CLIPS,), 2560, dtype=torch.int64, device=gpu), stride, n_seg, size)
    assert torch.equal(same, mel.segments(wave, 2560, stride, n_seg, size))


def _materialised(frames, wave, mel, batch):
    tb = batch.table.cpu()
    vis = _segments(frames, tb, batch.v_stride, batch.n_seg)
    s0 = batch.sample0.cpu().tolist()
    segs = torch.stack([torch.stack([wave[b, a + s * batch.a_stride:a + s * batch.a_stride + batch.a_size] for s in range(batch.n_seg)])
                        for b, a in enumerate(s0)])
    return vis, mel(segs.contiguous())


def _trainers(sd, gpu, n, **kw):
    from synchformer_amd.train import SyncTrainer
    return [SyncTrainer(sd, gpu, seed=1337, **kw) for _ in range(n)]


def _steps_agree(sd, gpu, sampler, n_steps, seed, **kw):
    """Trainer A: train_step on materialised inputs; B: train_step_clips from the raw clips; C: train_step again (the run-to-run spread)."""
    from synchformer_amd.frontend import MelFrontend
    mel = MelFrontend(gpu)
    A, B, C = _trainers(sd, gpu, 3, **kw)
    rng, gen = random.Random(seed), torch.Generator().manual_seed(seed)
    for step in range(n_steps):
        frames, wave = _clips(gpu, seed=seed * 10 + step)
        batch = sampler.sample(rng, [T] * N_CLIPS, [160000] * N_CLIPS, H, W, gen)
        bd = batch.to(gpu)
        vis, aud = _materialised(frames, wave, mel, bd)
        la = A.train_step(vis, aud, bd.targets).item()
        lb = B.train_step_clips(frames, wave, mel, bd).item()
        lc = C.train_step(vis, aud, bd.targets).item()
        ga, gb, gc = A.flat_g.clone(), B.flat_g.clone(), C.flat_g.clone()
        loss_bar, grad_bar = abs(la - lc), (ga - gc).abs().max().item()
        print(f'step {step}: loss {la:.6f} / clips {lb:.6f}; spread of train_step: loss {loss_bar:.3g}, grad {grad_bar:.3g}; '
              f'clips vs train_step: loss {abs(la - lb):.3g}, grad {(ga - gb).abs().max().item():.3g}')
        assert abs(la - lb) <= loss_bar and (ga - gb).abs().max().item() <= grad_bar, step
        assert torch.equal(A.flat_p, B.flat_p) or (A.flat_p - B.flat_p).abs().max().item() <= (A.flat_p - C.flat_p).abs().max().item()


def test_train_step_clips_matches_train_step(gpu):
    from synchformer_amd import synth
    from synchformer_amd.augment import ClipSampler
    _steps_agree(synth.make_state_dict(1337), gpu, ClipSampler('grid'), 2, seed=3)


def test_train_step_clips_matches_train_step_ft(gpu):
    """The fine-tune configuration: MXFP8 extractor GEMMs, 13 segments, 2-way sync head, syncability offsets."""
    from synchformer_amd import synth
    from synchformer_amd.augment import ClipSampler
    _steps_agree(synth.make_state_dict(1337, n_pos=184, n_out=2, head='sync_head'), gpu, ClipSampler('syncability'), 1, seed=4, fp8_towers=True)


def test_forward_crops_fixed_offsets_matches_forward(gpu):
    """The valid / test path: fixed offsets, centre crop, middle segments - forward_crops == forward on the materialised inputs."""
    from synchformer_amd import synth
    from synchformer_amd.augment import ClipSampler
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    eng, mel = SynchformerEngine(synth.make_state_dict(1337), gpu), MelFrontend(gpu)
    frames, wave = _clips(gpu, seed=9)
    bd = ClipSampler('grid').fixed([0.0, -1.5, 2.0], [2.0, 1.48, 3.0], [T] * 3, [160000] * 3, H, W).to(gpu)
    vis, aud = _materialised(frames, wave, mel, bd)
    got, want = eng.forward_crops(frames, wave, mel, bd), eng.forward(vis, aud)
    torch.cuda.synchronize()
    assert torch.equal(got, want), (got - want).abs().max().item()


def test_clip_train_pipeline_matches_device_resident_steps(gpu):
    """Three consecutive batches through the pinned-host two-slot pipeline (one set of pinned host buffers, refilled after wait_staged())
    give the losses of train_step_clips on the same trimmed windows already in HBM."""
    from synchformer_amd import synth
    from synchformer_amd.augment import ClipSampler, ClipTrainPipeline
    from synchformer_amd.frontend import MelFrontend
    sd = synth.make_state_dict(1337)
    P, R, R2 = _trainers(sd, gpu, 3)
    mel = MelFrontend(gpu)
    sampler, nb = ClipSampler('grid'), 2
    rng, gen = random.Random(11), torch.Generator().manual_seed(11)
    host = []
    for i in range(3):
        g = torch.Generator().manual_seed(100 + i)
        frames = torch.randint(0, 256, (nb, T, 3, H, W), dtype=torch.uint8, generator=g)
        wave = torch.randn(nb, 160000, generator=g) * 0.1
        host.append(sampler.sample(rng, [T] * nb, [160000] * nb, H, W, gen).trim(frames, wave))
    ref, spread = [], []
    for fw, ww, b in host:
        bd = b.to(gpu)
        ref.append(R.train_step_clips(fw.to(gpu), ww.to(gpu), mel, bd).item())
        spread.append(abs(ref[-1] - R2.train_step_clips(fw.to(gpu), ww.to(gpu), mel, bd).item()))
    pipe = ClipTrainPipeline(P, mel, nb, n_seg=14, H=H, W=W)
    f_pin, w_pin, b_pin = host[0][0].pin_memory(), host[0][1].pin_memory(), host[0][2].pin_memory()

    def fill(i):
        f_pin.copy_(host[i][0]); w_pin.copy_(host[i][1])
        b_pin.table.copy_(host[i][2].table); b_pin.sample0.copy_(host[i][2].sample0); b_pin.targets.copy_(host[i][2].targets)

    pipe.stage(f_pin, w_pin, b_pin)
    got = []
    for i in (1, 2):
        pipe.wait_staged()                  # the previous stage() has left the pinned buffers: recycle them
        fill(i)
        got.append(pipe.step(f_pin, w_pin, b_pin).item())
    got.append(pipe.step().item())
    print('pipeline', got, 'device-resident', ref, 'spread', spread)
    for g_, r_, s_ in zip(got, ref, spread):
        assert abs(g_ - r_) <= s_, (got, ref, spread)
