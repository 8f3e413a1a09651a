"""GPU: sf_resample_wave_mix against the float64 oracle of tests/ingest_programmes_oracle.py - rates, lengths, channel and programme counts, the
three sample types, planar and interleaved views with poisoned padding - its tile edges at 44.1 kHz, its bit-for-bit relations to sf_resample_wave and to
itself, and IngestStream over an interleaved int16 feed."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_programmes_oracle as PO  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 1e-5                                                                       # the resampler's bar (tests/test_ingest_gpu.py): inputs and mix rows are bounded by 1
NP_DT = {'f32': np.float32, 's16': np.int16, 's32': np.int32}
POISON = {'f32': float('nan'), 's16': 0x7fff, 's32': 0x7fff7fff}


@functools.lru_cache(maxsize=None)
def _bank(gpu_index, rate):
    """(kernel fp32 on the device, width, o, n): RecordingIngest's own bank (the identity bank at 16 kHz)."""
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(torch.device('cuda', gpu_index), 25, (256, 256), rate)
    return ing.kernel, ing.width, ing.o, ing.n


def _samples(fmt, ch, length, seed) -> np.ndarray:
    """planar (ch, length): U(-1, 1) noise, or full-scale integers (both ends of the range among them)"""
    rng = np.random.default_rng(seed)
    if fmt == 'f32':
        return rng.uniform(-1, 1, (ch, length)).astype(np.float32)
    info = np.iinfo(NP_DT[fmt])
    x = rng.integers(info.min, info.max, (ch, length), dtype=np.int64, endpoint=True)
    if length >= 2:
        x[0, 0], x[-1, -1] = info.min, info.max
    return x.astype(NP_DT[fmt])


def _mix(P, ch, seed) -> np.ndarray:
    """random rows scaled to an absolute sum <= 1; a negative and a zero weight wherever the matrix has room for both"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1, 1, (P, ch))
    if m.size >= 2:
        m.flat[0] = -abs(m.flat[0]) - 0.1
        m.flat[m.size - 1] = 0.0
    elif seed % 2:
        m.flat[0] = -abs(m.flat[0]) - 0.1
    m = m / np.maximum(np.abs(m).sum(1, keepdims=True), 1.0) * rng.uniform(0.5, 1.0, (P, 1))
    m = m.astype(np.float32)
    assert (np.abs(m.astype(np.float64)).sum(1) <= 1.0).all() and (m.size < 2 or ((m < 0).any() and (m == 0).any()))
    return m


def _view(gpu, x: np.ndarray, fmt, interleaved: bool) -> torch.Tensor:
    """x (ch, len) on the device as a strided view whose padding is poisoned: planar with a channel stride of len + 5, or interleaved (len, ch) with a frame stride
    of ch + 3"""
    ch, length = x.shape
    t = torch.from_numpy(x)
    if interleaved:
        buf = torch.full((length, ch + 3), POISON[fmt], dtype=t.dtype)
        buf[:, :ch] = t.t()
        return buf.to(gpu)[:, :ch]
    buf = torch.full((ch, length + 5), POISON[fmt], dtype=t.dtype)
    buf[:, :length] = t
    return buf.to(gpu)[:, :length]


def _launch_padded(xv, mix, bank, interleaved, len_out, pad=3):
    """The launcher itself, writing into rows of stride len_out + pad filled with NaN -> the whole (P, len_out + pad) buffer."""
    from synchformer_amd import _lib, ops
    kernel, width, o, n = bank
    x2 = xv.t() if interleaved else xv
    ch, length = x2.shape
    P = mix.shape[0]
    y = torch.full((P, len_out + pad), float('nan'), device=xv.device, dtype=torch.float32)
    rc = _lib.load().sf_resample_wave_mix(xv.data_ptr(), ops._MIX_DT[xv.dtype], ch, x2.stride(0) if ch > 1 else 1, x2.stride(1) if length > 1 else 1, length,
                                          mix.data_ptr(), P, kernel.data_ptr(), n, kernel.shape[1], o, width, y.data_ptr(), len_out + pad, len_out,
                                          torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'sf_resample_wave_mix')
    return y


@pytest.mark.parametrize('fmt', ['f32', 's16', 's32'])
@pytest.mark.parametrize('rate', [48000, 44100, 8000, 16000])
def test_mix_matches_float64(gpu, rate, fmt):
    """Every length, channel count, programme count and layout at this rate and sample type: max |gpu - float64| <= 1e-5, the output finite although every byte of
    the input's stride padding is NaN / 0x7fff.., the NaN behind each output row untouched, and ops.resample_wave_mix the same bits as the bare launcher."""
    from synchformer_amd import ops
    bank = _bank(gpu.index or 0, rate)
    kernel, width, o, n = bank
    worst = 0.0
    for length in (4411, 100, 1, 0):
        for ch in (1, 2, 3, 16):
            x = _samples(fmt, ch, length, 1000 * ch + length + rate)
            for P in (1, 3, 8):
                m = _mix(P, ch, 31 * P + ch + length)
                ref = PO.mix_resample64(x, m, rate)
                md = torch.from_numpy(m).to(gpu)
                for interleaved in (False, True):
                    xv = _view(gpu, x, fmt, interleaved)
                    assert length < 2 or ((xv.stride(1), xv.stride(0)) if interleaved else xv.stride()) == ((1, ch + 3) if interleaved else (length + 5, 1))
                    y = _launch_padded(xv, md, bank, interleaved, ref.shape[1])
                    got = ops.resample_wave_mix(xv, md, kernel, o, width, interleaved)
                    yc = y.cpu()
                    assert got.shape == ref.shape == (P, -(-n * length // o)) and got.dtype == torch.float32
                    assert torch.isnan(yc[:, ref.shape[1]:]).all(), 'the padding behind the output rows was written'
                    assert torch.equal(yc[:, :ref.shape[1]], got.cpu())
                    if ref.size:
                        assert torch.isfinite(got).all(), (length, ch, P, interleaved)
                        worst = max(worst, float(np.abs(got.cpu().double().numpy() - ref).max()))
    print(f'{rate} Hz {fmt}: max |gpu - float64| {worst:.3e} (bar {BAR:.0e})')
    assert worst <= BAR, worst


@pytest.mark.parametrize('len_out', [255, 256, 257, 513])
def test_tile_edges_at_44k1(gpu, len_out):
    """n = 160, o = 441: one tile, exactly one, one output into the second, one into the third.  The input is the shortest that gives len_out outputs, so the last
    tile's span runs past the end of the input (the right zero padding) and the first tile starts width samples before it (the left one)."""
    from synchformer_amd import ops
    kernel, width, o, n = _bank(gpu.index or 0, 44100)
    assert (n, o) == (160, 441)
    length = -(-len_out * o // n)                                                # the shortest input with ceil(n len / o) >= len_out
    while -(-n * (length - 1) // o) >= len_out:
        length -= 1
    assert -(-n * length // o) >= len_out > -(-n * (length - 1) // o)
    q_last = (len_out - 1) // n
    assert q_last * o - width + kernel.shape[1] > length and width > 0          # the last tile reads past the input, the first before it
    for fmt in ('f32', 's16'):
        x = _samples(fmt, 3, length, len_out)
        m = _mix(3, 3, len_out)
        ref = PO.mix_resample64(x, m, 44100)[:, :len_out]
        md = torch.from_numpy(m).to(gpu)
        for interleaved in (False, True):
            xv = _view(gpu, x, fmt, interleaved)
            got = ops.resample_wave_mix(xv, md, kernel, o, width, interleaved, len_out=len_out)
            err = float(np.abs(got.cpu().double().numpy() - ref).max())
            print(f'len_out {len_out} {fmt} {"interleaved" if interleaved else "planar"}: {length} samples, max |gpu - float64| {err:.3e}')
            assert got.shape == (3, len_out) and err <= BAR, err
            y = _launch_padded(xv, md, (kernel, width, o, n), interleaved, len_out).cpu()
            assert torch.equal(y[:, :len_out], got.cpu()) and torch.isnan(y[:, len_out:]).all()


@pytest.mark.parametrize('rate', [44100, 48000, 16000])
def test_single_channel_and_pair_equal_resample_wave(gpu, rate):
    """A programme that is one channel at weight 1 is ops.resample_wave on that channel alone, bit for bit, planar and interleaved, fp32 and int16 (the other 15
    weights are zeros, multiplied like any weight: fmaf(0, x, acc) = acc).  An equal-weight pair on int16 is ops.resample_wave on the two channels: both sides
    are exact before the filter (the products by 2^-16 and the sums of two int16 are exact in fp32) - which is why int16, not fp32, is used here."""
    from synchformer_amd import ops
    from synchformer_amd.ingest import programme_matrix
    kernel, width, o, n = _bank(gpu.index or 0, rate)
    ch, length = 16, 4411
    for fmt in ('f32', 's16'):
        x = _samples(fmt, ch, length, rate + ch)
        xd = torch.from_numpy(x).to(gpu)
        progs = [5, 0, 15] + ([(3, 9), (14, 15)] if fmt == 's16' else [])
        md = programme_matrix(progs, ch).to(gpu)
        for interleaved in (False, True):
            got = ops.resample_wave_mix(_view(gpu, x, fmt, interleaved), md, kernel, o, width, interleaved)
            for p, prog in enumerate(progs):
                rows = [prog] if isinstance(prog, int) else list(prog)
                ref = ops.resample_wave(xd[rows].contiguous(), kernel, o, width)
                assert torch.equal(got[p], ref), (rate, fmt, interleaved, prog, (got[p] - ref).abs().max().item())
    assert not torch.equal(got[0], got[1])


def test_layouts_types_and_launch_splits_agree_bit_for_bit(gpu):
    """Interleaved equals its planar copy; int32 holding int16 << 16 equals the int16 run; 11 programmes (two launches of 8 and 3) equal the same programmes run
    one at a time; a transposed (non-contiguous) mix and a view with a zero stride are taken too."""
    from synchformer_amd import ops
    kernel, width, o, n = _bank(gpu.index or 0, 44100)
    ch, length = 6, 3000
    x16 = _samples('s16', ch, length, 7)
    m = torch.from_numpy(_mix(11, ch, 11)).to(gpu)
    planar = torch.from_numpy(x16).to(gpu)
    base = ops.resample_wave_mix(planar, m, kernel, o, width)
    assert base.shape == (11, -(-n * length // o))
    inter = planar.t().contiguous()
    assert torch.equal(ops.resample_wave_mix(inter, m, kernel, o, width, interleaved=True), base)
    assert torch.equal(ops.resample_wave_mix(_view(gpu, x16, 's16', True), m, kernel, o, width, interleaved=True), base)
    x32 = torch.from_numpy(x16.astype(np.int32) << 16).to(gpu)
    assert torch.equal(ops.resample_wave_mix(x32, m, kernel, o, width), base)
    assert torch.equal(ops.resample_wave_mix(x32.t().contiguous(), m, kernel, o, width, interleaved=True), base)
    for p in range(11):
        assert torch.equal(ops.resample_wave_mix(planar, m[p:p + 1], kernel, o, width)[0], base[p]), p
    assert torch.equal(ops.resample_wave_mix(planar, m.t().contiguous().t(), kernel, o, width), base)
    same = planar[:1].expand(ch, length)                                         # stride 0 over the channels: copied once
    assert torch.equal(ops.resample_wave_mix(same, m, kernel, o, width), ops.resample_wave_mix(same.contiguous(), m, kernel, o, width))
    xf = torch.from_numpy(_samples('f32', ch, length, 8)).to(gpu)                # fp32: layouts and splits (not the exactness argument of int16)
    bf = ops.resample_wave_mix(xf, m, kernel, o, width)
    assert torch.equal(ops.resample_wave_mix(xf.t().contiguous(), m, kernel, o, width, interleaved=True), bf)
    assert all(torch.equal(ops.resample_wave_mix(xf, m[p:p + 1], kernel, o, width)[0], bf[p]) for p in range(11))


def test_waves_at_16k_is_the_mix_to_the_last_bit(gpu):
    """At 16 kHz nothing is passed through: the identity bank goes through the kernel and the rows are fmaf(mix[p, c], x[c], ..) in channel order, bit for bit -
    restated here in numpy fp32 (products of int16 samples by these dyadic weights and their sums are exact, so the order does not matter for them)."""
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 25, (256, 256), 16000, audio_channels=4, audio_interleaved=True, programmes=[0, (2, 3), {1: 1.0}, {0: 0.5, 3: -0.25}])
    x = _samples('s16', 4, 5000, 16)
    got = ing.waves(torch.from_numpy(x.T.copy()))
    xf = x.astype(np.float32) / np.float32(32768)
    want = np.stack([xf[0], (xf[2] + xf[3]) * np.float32(0.5), xf[1], xf[0] * np.float32(0.5) - xf[3] * np.float32(0.25)])
    assert got.shape == (4, 5000) and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    xr = _samples('f32', 4, 777, 17)                                             # fp32: a single channel at weight 1 passes to the bit
    assert np.array_equal(ing.waves(torch.from_numpy(xr.T.copy()))[0].cpu().numpy(), xr[0])
    with pytest.raises(ValueError, match=r'\.waves\(\)'):
        ing.wave(torch.from_numpy(x))


def test_ingest_stream_programmes_equal_waves(gpu):
    """4-channel interleaved int16 at 44.1 kHz, 3 programmes, pushed in the ragged sample runs of tests/test_track_stream_gpu.py: the (P, m) pieces concatenate to
    .waves() on the whole input bit for bit, and the stream never holds more raw samples than the plan's bound, 2 (width + o) (resample_stream_plan keeps the
    left context of the next output group: fewer than width + o samples behind it and fewer than width + o not yet usable)."""
    from test_track_stream_gpu import _ragged
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 25, (256, 256), 44100, audio_channels=4, audio_interleaved=True, programmes=[0, (2, 3), {1: 1.0}])
    total = 130000
    raw = torch.from_numpy(_samples('s16', 4, total, 44).T.copy())               # (n, 4)
    whole = ing.waves(raw)
    assert whole.shape == (3, ing.n_samples(total))
    for src in (raw, raw.to(gpu)):
        st = ing.stream()
        outs = []
        pieces = _ragged(0, total, a_runs=(44100, 0, 919, 40000, 14112, 0, 1))
        assert len(pieces) > 5 and any(a0 == a1 for _, _, a0, a1 in pieces)
        for _, _, a0, a1 in pieces:
            frames, w = st.push(None, src[a0:a1])
            assert w.shape[0] == 3 and frames.shape[0] == 0
            outs.append(w)
            assert st.held['samples'] <= 2 * (ing.width + ing.o), (st.held, ing.width, ing.o)
        outs.append(st.flush()[1])
        assert st.held['samples'] == 0 or st.held['samples'] <= 2 * (ing.width + ing.o)
        assert torch.equal(torch.cat(outs, 1), whole)
        with pytest.raises(RuntimeError, match='closed'):
            st.push(None, src[:0])
    planar = RecordingIngest(gpu, 25, (256, 256), 44100, audio_channels=4, programmes=[0, (2, 3), {1: 1.0}])
    st = planar.stream()
    outs = [st.push(None, raw.t()[:, a0:a1])[1] for _, _, a0, a1 in pieces] + [st.flush()[1]]
    assert torch.equal(torch.cat(outs, 1), whole)
