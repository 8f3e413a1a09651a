"""CPU: the host side of audio programmes - programme_matrix, RecordingIngest's refusals, the LDS limit of sf_resample_wave_mix as arithmetic, the
launcher's argument checks (they return before any launch), the library's export and ABI, and the float64 oracle of tests/ingest_programmes_oracle.py against the
existing restatement of sf_resample_wave (tests/ingest_oracle.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_oracle as R  # noqa: E402
import ingest_programmes_oracle as PO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES_P8 = (8000, 16000, 22050, 32000, 44100, 48000, 96000)                      # the rates at which 8 programmes fit one launch


def test_programme_matrix_values():
    from synchformer_amd.ingest import programme_matrix
    M = programme_matrix([0, (2, 3), {1: 1.0}, {0: 0.5, 3: -0.25}, (1, 2, 3), [4]], 5)
    want = torch.tensor([[1, 0, 0, 0, 0], [0, 0, .5, .5, 0], [0, 1, 0, 0, 0], [.5, 0, 0, -.25, 0], [0, 1 / 3, 1 / 3, 1 / 3, 0], [0, 0, 0, 0, 1]], dtype=torch.float32)
    assert M.dtype == torch.float32 and M.shape == (6, 5) and torch.equal(M, want)
    assert torch.equal(programme_matrix([(0, 1)], 2), torch.tensor([[0.5, 0.5]]))  # the stereo pair as sf_resample_wave averages it
    assert torch.equal(programme_matrix([{0: 0.0}], 1), torch.zeros(1, 1))         # a zero weight is a weight


@pytest.mark.parametrize('programmes, n_channels, match', [
    ([], 4, 'non-empty'), (None, 4, 'non-empty'), ([()], 4, 'empty'), ([{}], 4, 'empty'), ([4], 4, 'channel'), ([-1], 4, 'channel'), ([(0, 4)], 4, 'channel'),
    ([{7: 1.0}], 4, 'channel'), ([(1, 1)], 4, 'twice'), ([{0: float('nan')}], 4, 'finite'), ([{0: float('inf')}], 4, 'finite'), ([{0: 'x'}], 4, 'finite'),
    (['a'], 4, 'int'), ([0.5], 4, 'int'), ([(0.0,)], 4, 'channel'), ([0], 0, 'n_channels')])
def test_programme_matrix_refusals(programmes, n_channels, match):
    from synchformer_amd.ingest import programme_matrix
    with pytest.raises(ValueError, match=match):
        programme_matrix(programmes, n_channels)


def test_recording_ingest_programmes_constructor():
    from synchformer_amd.ingest import RecordingIngest
    cpu = torch.device('cpu')
    plain = RecordingIngest(cpu, 25, (256, 256), 48000)
    assert plain.programmes is None and 'programmes' not in vars(plain) and 'mix' not in vars(plain) and 'audio_channels' not in vars(plain)
    for kw in (dict(audio_channels=4), dict(audio_interleaved=True)):
        with pytest.raises(ValueError, match='programmes'):
            RecordingIngest(cpu, 25, (256, 256), 48000, **kw)
    for ch in (None, 0, 17):
        with pytest.raises(ValueError, match='audio_channels'):
            RecordingIngest(cpu, 25, (256, 256), 48000, audio_channels=ch, programmes=[0])
    with pytest.raises(ValueError, match='channel'):
        RecordingIngest(cpu, 25, (256, 256), 48000, audio_channels=4, programmes=[4])
    with pytest.raises(ValueError, match='non-empty'):
        RecordingIngest(cpu, 25, (256, 256), 48000, audio_channels=4, programmes=[])
    ing = RecordingIngest(cpu, 25, (256, 256), 48000, audio_channels=4, audio_interleaved=True, programmes=[0, (2, 3), {1: 1.0}])
    assert ing.audio_channels == 4 and ing.audio_interleaved and ing.programmes == [0, (2, 3), {1: 1.0}]
    assert torch.equal(ing.mix, torch.tensor([[1, 0, 0, 0], [0, 0, .5, .5], [0, 1, 0, 0]], dtype=torch.float32))
    assert (ing.o, ing.n, ing.width) == (plain.o, plain.n, plain.width) and torch.equal(ing.kernel, plain.kernel)
    with pytest.raises(ValueError, match=r'\.waves\(\)'):
        ing.wave(torch.zeros(4, 100))
    with pytest.raises(ValueError, match=r'\.wave\(\)'):
        plain.waves(torch.zeros(4, 100))
    for bad in (torch.zeros(4, 100), torch.zeros(100, 3), torch.zeros(100, 4, dtype=torch.float64), torch.zeros(100), torch.zeros(100, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='raw wave'):
            ing.waves(bad)
    with pytest.raises(RuntimeError, match='device'):                            # the right shape on the CPU: refused at the op, before any launch
        ing.waves(torch.zeros(100, 4, dtype=torch.int16))
    assert RecordingIngest(cpu, 25, (256, 256), 16000, audio_channels=16, programmes=[15]).kernel.shape == (1, 1)


def test_ops_resample_wave_mix_refuses_cpu_tensors_and_bad_shapes():
    from synchformer_amd import ops
    from synchformer_amd.ingest import resample_kernel
    k, width, o, n = resample_kernel(48000)
    with pytest.raises(RuntimeError, match='device'):
        ops.resample_wave_mix(torch.zeros(2, 100), torch.ones(1, 2), k, o, width)
    with pytest.raises(ValueError):
        ops.resample_wave_mix(torch.zeros(17, 100), torch.ones(1, 17), k, o, width)
    with pytest.raises(ValueError):
        ops.resample_wave_mix(torch.zeros(2, 100), torch.ones(1, 3), k, o, width)
    with pytest.raises(ValueError):
        ops.resample_wave_mix(torch.zeros(2, 100, dtype=torch.float64), torch.ones(1, 2), k, o, width)
    with pytest.raises(ValueError):
        ops.resample_wave_mix(torch.zeros(100, 2), torch.ones(1, 2), k, o, width, interleaved=False)


def test_lds_limit_admits_eight_programmes_at_the_seven_rates():
    """P * span <= 16384 floats, span = ((255 // n) + 1) o + taps: by the oracle's own bank geometry, by ingest.resample_kernel's, and by ops.resample_mix_span."""
    from synchformer_amd import ops
    from synchformer_amd.ingest import resample_kernel
    header = open(os.path.join(ROOT, 'include', 'synchformer_hip.h')).read()
    assert '16384 floats' in header and ops.MIX_MAX_FLOATS == 16384 and ops.MIX_MAX_P == 8 and ops.MIX_MAX_CH == 16 and ops.MIX_TILE == 256
    spans = {}
    for rate in RATES_P8:
        k, width, o, n = (torch.ones(1, 1), 0, 1, 1) if rate == 16000 else resample_kernel(rate)
        spans[rate] = ((255 // n) + 1) * o + k.shape[1]
        assert spans[rate] == PO.span(rate) == ops.resample_mix_span(n, o, k.shape[1])
        assert 8 * spans[rate] <= 16384, (rate, spans[rate])
    print('span of one tile:', spans)
    assert spans[48000] == 809 and spans[44100] == 1357 and spans[96000] == 1616 and spans[16000] == 257
    assert 8 * PO.span(192000) > 16384 and 16384 // PO.span(192000) == 5         # a rate at which the op has to split: 5 programmes per launch


def test_library_exports_the_mix_launcher_at_abi_23():
    from synchformer_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'synchformer_hip.h')).read()
    assert int(re.search(r'#define SF_ABI_VERSION (\d+)', header).group(1)) >= 23 and re.search(r'SF_I32 = 5\b', header) and ops.SF_I32 == 5
    assert len(_lib.SIGNATURES['sf_resample_wave_mix']) == 17 and len(_lib.SIGNATURES['sf_resample_wave']) == 13
    for lib in (_lib.load(), _lib.load_ablation()):
        assert hasattr(lib, 'sf_resample_wave_mix') and lib.sf_abi_version() >= 23
    assert 'resample_wave_mix' not in ops.DISPATCHER_OPS and 'resample_wave' not in ops.DISPATCHER_OPS


def test_mix_launcher_rejects_bad_arguments_without_gpu():
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    r = dict(x=p, dt=4, ch=2, sc=1, ss=2, len=100, mix=p, P=3, k=p, n=1, taps=41, o=3, width=19, y=p, ldy=34, len_out=34)

    def mix(**kw):
        a = dict(r, **kw)
        return lib.sf_resample_wave_mix(a['x'], a['dt'], a['ch'], a['sc'], a['ss'], a['len'], a['mix'], a['P'], a['k'], a['n'], a['taps'], a['o'], a['width'], a['y'],
                                        a['ldy'], a['len_out'], None)

    for dt in (1, 2, 3, 6, -1):
        assert mix(dt=dt) == -1 and b'dtype' in lib.sf_last_error()
    assert mix(ch=0) == -1 and b'channels' in lib.sf_last_error() and mix(ch=17) == -1 and b'channels' in lib.sf_last_error()
    assert mix(P=0) == -1 and b'programmes' in lib.sf_last_error() and mix(P=9) == -1 and b'programmes' in lib.sf_last_error()
    assert mix(ss=0) == -1 and b'strides' in lib.sf_last_error() and mix(sc=-1) == -1 and b'strides' in lib.sf_last_error()
    assert mix(len_out=35, ldy=35) == -1 and b'above ceil' in lib.sf_last_error()
    assert mix(ldy=33) == -1 and b'ldy' in lib.sf_last_error()
    assert mix(P=8, o=12, taps=158, width=73, len_out=0) == -1 and b'floats of LDS' in lib.sf_last_error()      # 192 kHz: 8 x 3230 floats
    assert mix(P=5, o=12, taps=158, width=73, len_out=0) == 0
    for name in ('x', 'mix', 'k', 'y'):
        assert mix(**{name: None}) == -1 and b'null pointer' in lib.sf_last_error()
    assert mix(len_out=0, x=None, y=None, mix=None, k=None) == 0 and mix(len=0, len_out=0, ldy=0) == 0          # nothing to do: returns before any launch
    for dt in (0, 4, 5):
        assert mix(dt=dt, len_out=0) == 0


@pytest.mark.parametrize('rate', [48000, 44100, 8000, 22050])
def test_oracle_reproduces_the_mono_restatement(rate):
    """mix = [[1 / ch] * ch] is sf_resample_wave's average: the oracle equals tests/ingest_oracle.py's resample64 on the channel mean (both float64; they share no
    code: a loop over the bank's definition here, F.conv1d there)."""
    rng = np.random.default_rng(rate)
    for ch, length in ((1, 1000), (2, 4411), (3, 100), (8, 1)):
        x = rng.uniform(-1, 1, (ch, length)).astype(np.float32)
        got = PO.mix_resample64(x, np.full((1, ch), 1.0 / ch), rate)
        ref = R.resample64(torch.from_numpy(x).double().mean(0), rate).numpy()
        assert got.shape == (1, ref.shape[0]), (got.shape, ref.shape)
        err = np.abs(got[0] - ref).max()
        assert err <= 1e-12, (rate, ch, length, err)
    k, width, o, n = PO.bank64(rate)
    from synchformer_amd.ingest import resample_kernel
    k32 = resample_kernel(rate)
    assert (width, o, n) == k32[1:] and np.abs(k - k32[0].double().numpy()).max() <= 2.0 ** -24


def test_oracle_identity_bank_and_integer_scales():
    x = np.array([[-32768, 16384, 1], [32767, -1, 0]], dtype=np.int16)
    mixm = np.array([[1.0, 0.0], [0.5, -0.25]])
    got = PO.mix_resample64(x, mixm, 16000)
    assert np.array_equal(got, mixm @ (x.astype(np.float64) / 32768.0))
    assert np.array_equal(PO.mix_resample64(x.astype(np.int32) << 16, mixm, 16000), got)
    assert PO.mix_resample64(np.zeros((2, 0), dtype=np.float32), mixm, 48000).shape == (2, 0)
