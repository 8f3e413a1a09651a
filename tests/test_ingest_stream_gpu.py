"""GPU: ingest.IngestStream - the frames and samples it emits over any chunking concatenate to RecordingIngest.frames / .wave on the finished recording, bit for
bit: the frame-rate rule's last slot waits for the next source frame, the resampler runs on each chunk with its left context."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _push_all(stream, frames=None, wave=None, f_runs=(1,), a_runs=(1,)):
    fs, ws, f, a, i = [], [], 0, 0, 0
    nf_total = 0 if frames is None else frames.shape[0]
    na_total = 0 if wave is None else wave.shape[-1]
    while f < nf_total or a < na_total:
        nf, na = min(f_runs[i % len(f_runs)], nf_total - f), min(a_runs[i % len(a_runs)], na_total - a)
        out_f, out_w = stream.push(None if frames is None else frames[f:f + nf], None if wave is None else wave[..., a:a + na])
        fs.append(out_f)
        ws.append(out_w)
        assert stream.held['frames'] <= 1
        f, a, i = f + nf, a + na, i + 1
    out_f, out_w = stream.flush()
    with pytest.raises(RuntimeError, match='closed'):
        stream.push(None, None)
    return torch.cat(fs + [out_f]), torch.cat(ws + [out_w])


def _raw_frames(pix_fmt: str, n: int, H: int, W: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    if pix_fmt == 'rgb24':
        return torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)                       # channels-last, as decoders hand them out
    if pix_fmt == 'nv12':
        return torch.randint(0, 256, (n, 3 * H // 2, W), generator=g, dtype=torch.uint8)
    x = (torch.randint(0, 1024, (n, 3 * H // 2, W), generator=g, dtype=torch.int32) << 6).numpy().astype(np.uint16)     # P010: ten bits at the top of each word
    return torch.from_numpy(x.view(np.int16))


@pytest.mark.parametrize('fps, pix_fmt', [((30000, 1001), 'rgb24'), (50, 'rgb24'), ((30000, 1001), 'nv12'), (50, 'p010')])
def test_streamed_frames_equal_offline(gpu, fps, pix_fmt):
    from synchformer_amd.ingest import RecordingIngest
    n, H, W = 40, 270, 480
    raw = _raw_frames(pix_fmt, n, H, W, 5)
    ing = RecordingIngest(gpu, fps, (H, W), 16000, channels_last=(pix_fmt == 'rgb24'), pix_fmt=pix_fmt)
    ref = ing.frames(raw, 0, ing.n_frames(n))
    for runs in ((1,), (3, 0, 7, 1, 12)):
        got, _ = _push_all(ing.stream(), frames=raw, f_runs=runs)
        torch.cuda.synchronize()
        assert got.shape == ref.shape and got.dtype == torch.uint8 and torch.equal(got, ref), (fps, pix_fmt, runs)
    got, _ = _push_all(ing.stream(), frames=raw.to(gpu), f_runs=(40,))                                    # one push, from the device
    assert torch.equal(got, ref) and ref.shape[0] > 0 and not torch.equal(ref[0], ref[-1])


@pytest.mark.parametrize('rate, ch, dtype', [(48000, 2, torch.int16), (44100, 1, torch.float32), (8000, 1, torch.float32)])
def test_streamed_wave_equals_offline(gpu, rate, ch, dtype):
    from synchformer_amd.ingest import RecordingIngest
    n = 4411
    x = torch.rand(ch, n, generator=torch.Generator().manual_seed(rate)) * 2 - 1
    x = (x * 32767).to(torch.int16) if dtype == torch.int16 else x
    x = x[0] if ch == 1 else x
    ing = RecordingIngest(gpu, 25, (256, 256), rate)
    ref = ing.wave(x.to(gpu))
    assert ref.shape == (ing.n_samples(n),)
    for chunk in (1, 100, 1000):
        stream = ing.stream()
        _, got = _push_all(stream, wave=x, a_runs=(chunk,))
        torch.cuda.synchronize()
        assert got.shape == ref.shape and torch.equal(got, ref), (rate, chunk, (got - ref).abs().max().item() if got.shape == ref.shape else got.shape)
        assert stream.held['samples'] <= chunk + 2 * (ing.width + ing.o)
    ident = RecordingIngest(gpu, 25, (256, 256), 16000)                          # a mono fp32 wave at 16 kHz passes as it is
    y = torch.rand(5000, generator=torch.Generator().manual_seed(1))
    _, got = _push_all(ident.stream(), wave=y, a_runs=(777,))
    assert torch.equal(got.cpu(), y)
