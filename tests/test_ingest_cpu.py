"""No GPU: the host geometry of the ingest stage (synchformer_amd.ingest) against restatements that do not call it (tests/ingest_oracle.py), the
ABI entries of its two launchers and the argument handling of RecordingIngest and of the launchers (rejected before the device is touched)."""
import ctypes
import math
import os
import sys
from fractions import Fraction

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_oracle as R  # noqa: E402


def test_frame_table_identity_and_halving():
    from synchformer_amd.ingest import fps_frame_table
    for fps in (25, 25.0, (25, 1), (50, 2)):
        t = fps_frame_table(40, fps)
        assert t.dtype == torch.int32 and torch.equal(t, torch.arange(40, dtype=torch.int32)), fps
    t = fps_frame_table(41, 50)                                                  # p_i = floor(i / 2 + 1 / 2): slot j is reached last by frame 2 j
    assert t.numel() == 21 and torch.equal(t, 2 * torch.arange(21, dtype=torch.int32))
    t = fps_frame_table(40, 50)                                                  # an even count: frame 39 alone lands on the last slot, p_39 = 20
    assert t.numel() == 21 and torch.equal(t[:20], 2 * torch.arange(20, dtype=torch.int32)) and int(t[20]) == 39
    assert fps_frame_table(0, 30).numel() == 0
    with pytest.raises(ValueError):
        fps_frame_table(10, 0)


@pytest.mark.parametrize('fps', [(30000, 1001), 30, 24, 12.5, 60])
def test_frame_table_follows_the_near_rule(fps):
    from synchformer_amd.ingest import fps_frame_table
    n_in = 40
    fi = Fraction(*fps) if isinstance(fps, tuple) else Fraction(fps).limit_denominator(1001)
    t = fps_frame_table(n_in, fps)
    ref = R.frame_table_bruteforce(n_in, fi)
    assert t.dtype == torch.int32 and t.tolist() == ref, (fps, t.tolist(), ref)
    assert (t[1:] >= t[:-1]).all() and int(t[-1]) == n_in - 1
    for j, i in enumerate(t.tolist()):                                           # the frame shown at j / 25 was taken within half an output period plus one input period
        assert abs(Fraction(i) / fi - Fraction(j, 25)) <= Fraction(1, 50) + 1 / fi, (fps, j, i)
    # a float names the same rate as its fraction
    if isinstance(fps, tuple):
        assert torch.equal(t, fps_frame_table(n_in, fps[0] / fps[1]))


def test_resized_dims():
    from synchformer_amd.ingest import resized_dims
    assert resized_dims(1080, 1920) == (256, 454)            # 1920 * 256 // 1080 = 455 -> even
    assert resized_dims(1920, 1080) == (454, 256)
    assert resized_dims(256, 256) == (256, 256) and resized_dims(270, 480) == (256, 454) and resized_dims(360, 202) == (456, 256)
    assert resized_dims(144, 176) == (256, 312) and resized_dims(301, 517, 224) == (224, 384)
    with pytest.raises(ValueError):
        resized_dims(0, 10)


def _apply_tables(x64, H, W, Hr, Wr, dtype):
    from synchformer_amd.ingest import aa_bicubic_table
    yf, yw, ty = aa_bicubic_table(H, Hr, dtype)
    xf, xw, tx = aa_bicubic_table(W, Wr, dtype)
    xp = torch.nn.functional.pad(x64, (0, tx, 0, ty))                            # the zero-padded taps may point past the edge
    h = sum(xw[:, j].double()[None, :] * xp[:, (xf.long() + j)] for j in range(tx))                 # (H + ty, Wr)
    return sum(yw[:, i].double()[:, None] * h[(yf.long() + i)] for i in range(ty))                   # (Hr, Wr)


@pytest.mark.parametrize('H, W', R.SIZES)
def test_aa_bicubic_table_is_interpolate(H, W):
    """The tables applied in float64 (horizontal pass first) against F.interpolate on float64, uniform random levels in [0, 255].
    The float64 weights: within 1e-9 (measured 5e-13).  The stored fp32 weights: each is its float64 value rounded, <= 2^-25 relative; a row's absolute mass
    is <= 1.3 (the cubic's negative lobes), two passes, values <= 255:  2 * 1.3^2 * 255 * 2^-25 = 2.6e-5."""
    from synchformer_amd import ingest
    Hr, Wr = ingest.resized_dims(H, W)
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.randint(0, 256, (H, W), generator=g).double()
    ref = R.resize64(x, (Hr, Wr))
    yf, yw, ty = ingest.aa_bicubic_table(H, Hr)
    xf, xw, tx = ingest.aa_bicubic_table(W, Wr)
    assert yf.dtype == xf.dtype == torch.int32 and yw.dtype == xw.dtype == torch.float32 and yw.shape == (Hr, ty) and xw.shape == (Wr, tx)
    for n_in, n_out, taps in ((H, Hr, ty), (W, Wr, tx)):
        s = n_in / n_out
        assert taps == 2 * math.ceil(2 * s if s >= 1 else 2) + 1
    for f, w, n_in in ((yf, yw, H), (xf, xw, W)):
        assert (w.double().sum(1) - 1).abs().max() <= w.shape[1] * 2.0 ** -24                       # rows sum to 1 (fp32 rounding of each weight)
        assert (w.abs().double().sum(1) <= 1.3).all()
        assert (f >= 0).all() and (f[1:] >= f[:-1]).all()
        last = ((w != 0).long() * torch.arange(1, w.shape[1] + 1)).max(1).values
        assert ((f.long() + last) <= n_in).all()                                                    # no non-zero tap outside the input
    e64 = (_apply_tables(x, H, W, Hr, Wr, torch.float64) - ref).abs().max().item()
    e32 = (_apply_tables(x, H, W, Hr, Wr, torch.float32) - ref).abs().max().item()
    print(f'{H} x {W} -> {Hr} x {Wr}: taps {ty} x {tx}, max |tables - F.interpolate float64|: float64 weights {e64:.3e}, fp32 weights {e32:.3e}')
    assert e64 <= 1e-9, e64
    assert e32 <= 2.6e-5, e32


def test_aa_bicubic_identity_at_scale_one():
    from synchformer_amd.ingest import aa_bicubic_table
    f, w, taps = aa_bicubic_table(256, 256)
    assert taps == 5
    x = torch.arange(256, dtype=torch.float64) * 3 + 1
    xp = torch.cat([x, torch.zeros(taps, dtype=torch.float64)])
    got = sum(w[:, j].double() * xp[f.long() + j] for j in range(taps))
    assert torch.equal(got, x)
    assert ((w == 0) | (w == 1)).all() and (w.sum(1) == 1).all()                 # exact 0 / 1 weights: the kernel's fp32 sums are exact on them


@pytest.mark.parametrize('rate, n, taps', [(48000, 1, 41), (44100, 160, 475), (22050, 320, 459), (8000, 2, 15)])
def test_resample_kernel_shape_and_tone(rate, n, taps):
    """A 1 kHz tone resampled with the bank (float64 sums) against the analytic sinusoid at the output sample times, away from 200 edge samples: within 2e-3
    (the windowed sinc's own pass-band error measures 4.4e-4; a one-sample delay would give 2 sin(pi 1000 / 16000) = 0.39)."""
    from synchformer_amd.ingest import resample_kernel
    k, width, o, nn = resample_kernel(rate)
    assert k.dtype == torch.float32 and k.shape == (n, taps) and nn == n and taps == 2 * width + o and o == rate // math.gcd(rate, 16000)
    n_in = rate // 4                                                             # 0.25 s
    x = torch.sin(2 * math.pi * 1000 * torch.arange(n_in, dtype=torch.float64) / rate)
    xp = torch.nn.functional.pad(x, (width, width + o))
    n_out = -(-n * n_in // o)
    j = torch.arange(n_out)
    q, p = j // n, j % n
    y = torch.zeros(n_out, dtype=torch.float64)
    for i in range(taps):
        y += xp[q * o + i] * k[p, i].double()
    want = torch.sin(2 * math.pi * 1000 * j.double() / 16000)
    err = (y - want)[200:-200].abs().max().item()
    print(f'{rate} Hz: {n} phases x {taps} taps, 1 kHz tone max error {err:.3e}')
    assert n_out == 4000 and err <= 2e-3, err
    # and the bank is the float64 restatement's, to fp32 rounding of the weights
    ref = R.resample64(x, rate)
    assert (y - ref).abs().max().item() <= taps * 2.0 ** -24, (y - ref).abs().max().item()


def test_abi_lists_the_ingest_launchers():
    from synchformer_amd import _lib
    assert _lib.ABI_VERSION >= 15
    assert len(_lib.SIGNATURES['sf_ingest_video']) == 18 and len(_lib.SIGNATURES['sf_resample_wave']) == 13
    for lib in (_lib.load(), _lib.load_ablation()):
        assert hasattr(lib, 'sf_ingest_video') and hasattr(lib, 'sf_resample_wave') and lib.sf_abi_version() >= 15


def test_recording_ingest_argument_validation():
    import synchformer_amd as sa
    from synchformer_amd import ingest
    assert sa.RecordingIngest is ingest.RecordingIngest
    cpu = torch.device('cpu')
    with pytest.raises(ValueError, match='resize_side'):
        ingest.RecordingIngest(cpu, 25, (270, 480), 16000, resize_side=200)
    with pytest.raises(ValueError, match='taps'):
        ingest.RecordingIngest(cpu, 25, (2400, 4000), 48000)                     # scale 9.4: 39 taps
    with pytest.raises(ValueError, match='crop'):
        ingest.RecordingIngest(cpu, 25, (270, 480), 16000, crop=112)
    with pytest.raises(ValueError):
        ingest.RecordingIngest(cpu, 0, (270, 480), 16000)
    ing = ingest.RecordingIngest(cpu, (30000, 1001), (1080, 1920), 48000, channels_last=True)
    assert (ing.Hr, ing.Wr, ing.y0, ing.x0, ing.taps_y, ing.taps_x) == (256, 454, 16, 115, 19, 19)
    assert ing.y_first.shape == ing.x_first.shape == (224,) and ing.y_w.shape == (224, 19) and (ing.o, ing.n, ing.width) == (3, 1, 19)
    assert ing.n_frames(300) == int(math.floor(299 * Fraction(25 * 1001, 30000) + Fraction(1, 2))) + 1 and ing.n_samples(48000) == 16000
    with pytest.raises(ValueError, match='raw frames'):
        ing.frames(torch.zeros(4, 3, 1080, 1920, dtype=torch.uint8), 0, 1)       # planar given, channels-last declared
    with pytest.raises(ValueError, match='raw wave'):
        ing.wave(torch.zeros(9, 100))
    # the 2160 short side is inside the range
    assert ingest.RecordingIngest(cpu, 25, (2160, 3840), 48000).taps_y == 35


def test_launchers_reject_bad_arguments_without_gpu():
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    v = dict(raw=p, sf=100, sc=1, sy=10, sx=1, n_src=1, H=10, W=10, ft=p, yf=p, yw=p, ty=5, xf=p, xw=p, tx=5, out=p, T=1)

    def video(**kw):
        a = dict(v, **kw)
        return lib.sf_ingest_video(a['raw'], a['sf'], a['sc'], a['sy'], a['sx'], a['n_src'], a['H'], a['W'], a['ft'], a['yf'], a['yw'], a['ty'], a['xf'], a['xw'],
                                   a['tx'], a['out'], a['T'], None)

    assert video(ty=36) == -1 and b'out of range' in lib.sf_last_error()
    assert video(tx=0) == -1 and b'out of range' in lib.sf_last_error()
    assert video(raw=None) == -1 and b'null pointer' in lib.sf_last_error()
    assert video(out=p + 1) == -1 and b'aligned' in lib.sf_last_error()
    assert video(sx=0) == -1 and b'stride' in lib.sf_last_error()
    assert video(W=70000) == -1 and b'too wide' in lib.sf_last_error()
    assert video(T=-1) == -1 and video(H=0) == -1
    assert video(T=0) == 0                                                       # nothing to do: returns before any launch
    r = dict(x=p, dt=0, ch=1, ld=100, len=100, k=p, n=1, taps=41, o=3, width=19, y=p, len_out=34)

    def wave(**kw):
        a = dict(r, **kw)
        return lib.sf_resample_wave(a['x'], a['dt'], a['ch'], a['ld'], a['len'], a['k'], a['n'], a['taps'], a['o'], a['width'], a['y'], a['len_out'], None)

    assert wave(dt=1) == -1 and b'dtype' in lib.sf_last_error()
    assert wave(ch=9) == -1 and b'channels' in lib.sf_last_error()
    assert wave(len_out=35) == -1 and b'above ceil' in lib.sf_last_error()
    assert wave(o=50000, taps=50038, len_out=0) == -1 and b'spans' in lib.sf_last_error()
    assert wave(x=None) == -1 and b'null pointer' in lib.sf_last_error()
    assert wave(len_out=0) == 0 and wave(len=0, ld=0, len_out=0) == 0
