"""No GPU: sf_track_decode's argument handling (rejected before the device is touched) and the segment / window geometry of a recording."""
import ctypes

import pytest
import torch


def _ptr(buf):
    p = ctypes.addressof(buf)
    return p + (-p) % 16


def test_track_decode_argument_validation_without_gpu():
    """The launcher's convention (test_argument_validation_without_gpu): -1 plus a message, nothing launched - safe on a box without a device."""
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = _ptr(buf)
    good = dict(logits=p, ldl=21, W=3, C=21, lam=1.0, cls_raw=p, conf_raw=p, cls_path=p, conf_path=p, backptr=p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sf_track_decode(a['logits'], a['ldl'], a['W'], a['C'], a['lam'], a['cls_raw'], a['conf_raw'], a['cls_path'], a['conf_path'], a['backptr'], None)

    for name in ('logits', 'cls_raw', 'conf_raw', 'cls_path', 'conf_path', 'backptr'):
        assert call(**{name: None}) == -1 and b'null pointer' in lib.sf_last_error(), name
    for C in (1, 0, -3, 65):
        assert call(C=C, ldl=128) == -1 and b'classes out of range' in lib.sf_last_error(), C
    assert call(ldl=20) == -1 and b'row stride' in lib.sf_last_error()
    for lam in (-0.5, float('inf'), float('-inf'), float('nan')):
        assert call(lam=lam) == -1 and b'lam must be finite' in lib.sf_last_error(), lam
    assert call(W=-1) == -1 and b'windows' in lib.sf_last_error()
    assert call(W=0) == 0                                                       # nothing to do: returns before any launch


def test_abi_lists_track_decode():
    from synchformer_amd import _lib
    assert _lib.ABI_VERSION >= 14 and len(_lib.SIGNATURES['sf_track_decode']) == 11
    assert hasattr(_lib.load(), 'sf_track_decode') and hasattr(_lib.load_ablation(), 'sf_track_decode')


@pytest.mark.parametrize('T, n, N, W1, W2', [
    (120, 76800, 14, 1, 1),          # exactly one window
    (144, 92160, 17, 4, 2),
    (400, 92160, 17, 4, 2),          # the audio is the shorter stream
    (144, 200000, 17, 4, 2),         # the video is the shorter stream
    (151, 97279, 17, 4, 2),          # one frame / one sample short of an 18th segment
    (152, 97280, 18, 5, 3),
    (119, 76800, 13, 0, 0),          # below one window
    (120, 76799, 13, 0, 0),
    (8, 100, 0, 0, 0),
])
def test_recording_geometry(T, n, N, W1, W2):
    from synchformer_amd.frontend import recording_geometry
    g1, g2 = recording_geometry(T, n), recording_geometry(T, n, 2)
    assert (g1['n_segments'], g1['n_windows'], g2['n_segments'], g2['n_windows']) == (N, W1, N, W2)
    assert (g1['v_stride'], g1['v_size'], g1['a_stride'], g1['a_size'], g1['n_window']) == (8, 16, 5120, 10240, 14)
    # every window lies inside both streams
    if W1:
        assert 8 * (W1 - 1) + 120 <= T and 5120 * (W1 - 1) + 76800 <= n


def test_one_window_recording_is_segment_ranges_own_clip():
    from synchformer_amd.frontend import recording_geometry, segment_ranges
    g, r = recording_geometry(120, 76800), segment_ranges(120, 76800)
    assert r['v_start'] == 0 and r['a_start'] == 0 and g['n_segments'] == r['n_segments'] == 14 and g['n_windows'] == 1
    assert all(g[k] == r[k] for k in ('v_stride', 'v_size', 'a_stride', 'a_size'))
    with pytest.raises(ValueError):
        recording_geometry(120, 76800, 0)


def test_window_centres():
    from synchformer_amd.track import window_times
    for hop, W in ((1, 4), (2, 2), (3, 7)):
        want = torch.tensor([(8 * hop * w + 60) / 25 for w in range(W)], dtype=torch.float64).float()
        got = window_times(W, hop)
        assert got.dtype == torch.float32 and torch.equal(got, want), (hop, got, want)
    assert window_times(0).shape == (0,)
    assert window_times(1)[0].item() == pytest.approx(2.4)


def test_tracker_is_exported():
    import synchformer_amd as sa
    from synchformer_amd import track
    assert sa.OffsetTracker is track.OffsetTracker and sa.OffsetTrack is track.OffsetTrack
