"""No GPU: the float64 oracle of the posterior read-out (tests/track_posterior_oracle.py) against a brute-force marginaliser over all C^W paths, the
identities the contract states (lam = 0, W = 1, reversed rows, log_z <= 0), sf_track_posterior's argument handling (rejected before the device is touched),
its ABI entry, and the shape of the OffsetTrack dataclass."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_posterior_oracle as TP  # noqa: E402


def _softmax64(x):
    p = np.exp(x - x.max(1, keepdims=True))
    return p / p.sum(1, keepdims=True)


@pytest.mark.parametrize('lam', [0.0, 0.5, 3.0])
@pytest.mark.parametrize('C, W', [(2, 1), (3, 5), (4, 4), (2, 10)])
def test_oracle_equals_brute_force(C, W, lam):
    rng = np.random.default_rng(100 * C + W)
    x = 3 * rng.standard_normal((W, C))
    o = TP.posterior(x, lam, np.linspace(-1, 1, C))
    post, log_z = TP.brute_force(x, lam)
    assert np.abs(o['post'] - post).max() <= 1e-12 and abs(o['log_z'] - log_z) <= 1e-12, (np.abs(o['post'] - post).max(), o['log_z'], log_z)
    assert np.abs(o['post'].sum(1) - 1).max() <= 1e-12 and o['log_z'] <= 1e-12
    if lam == 0 or W == 1:
        assert np.abs(o['post'] - _softmax64(x)).max() <= 1e-12 and abs(o['log_z']) <= 1e-12
    r = TP.posterior(x[::-1], lam, np.linspace(-1, 1, C))                       # reversed rows: reversed marginals, the same partition sum
    assert np.abs(r['post'][::-1] - o['post']).max() <= 1e-12 and abs(r['log_z'] - o['log_z']) <= 1e-12


@pytest.mark.parametrize('lam', [0.0, 0.5, 3.0])
def test_oracle_equals_brute_force_with_a_masked_class(lam):
    """Column 1 is -inf in every row (a class that does not exist), column 3 in two rows: exactly 0 there, no NaN, everything else as enumerated."""
    rng = np.random.default_rng(5)
    x = 3 * rng.standard_normal((4, 4))
    x[:, 1] = -np.inf
    x[[0, 2], 3] = -np.inf
    o = TP.posterior(x, lam, np.arange(4.0))
    post, log_z = TP.brute_force(x, lam)
    assert np.isfinite(o['post']).all() and np.isfinite(o['offset_mean']).all() and np.isfinite(o['log_z'])
    assert (o['post'][:, 1] == 0).all() and (o['post'][[0, 2], 3] == 0).all() and (o['post'][[1, 3], 3] > 0).all()
    assert np.abs(o['post'] - post).max() <= 1e-12 and abs(o['log_z'] - log_z) <= 1e-12


def _ptr(buf):
    p = ctypes.addressof(buf)
    return p + (-p) % 16


def test_track_posterior_argument_validation_without_gpu():
    """The launcher's convention (test_track_decode_argument_validation_without_gpu): -1 plus a message, nothing launched - safe without a device."""
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = _ptr(buf)
    names = ('logits', 'ldl', 'W', 'C', 'lam', 'grid', 'post', 'ldp', 'cls_post', 'conf_post', 'offset_mean', 'log_z', 'workspace')
    good = dict(logits=p, ldl=21, W=3, C=21, lam=1.0, grid=p, post=p, ldp=21, cls_post=p, conf_post=p, offset_mean=p, log_z=p, workspace=p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sf_track_posterior(*[a[n] for n in names], None)

    for name in ('logits', 'grid', 'post', 'cls_post', 'conf_post', 'offset_mean', 'log_z', 'workspace'):
        assert call(**{name: None}) == -1 and b'null pointer' in lib.sf_last_error(), name
    for C in (1, 0, -3, 65):
        assert call(C=C, ldl=128, ldp=128) == -1 and b'classes out of range' in lib.sf_last_error(), C
    assert call(ldl=20) == -1 and b'row stride ldl' in lib.sf_last_error()
    assert call(ldp=20) == -1 and b'post row stride' in lib.sf_last_error()
    for lam in (-0.5, float('inf'), float('-inf'), float('nan')):
        assert call(lam=lam) == -1 and b'lam must be finite' in lib.sf_last_error(), lam
    assert call(W=-1) == -1 and b'windows' in lib.sf_last_error()
    assert call(W=0) == 0                                                       # nothing to do: returns before any launch
    assert call(W=0, logits=None, post=None, workspace=None) == 0               # and needs no buffers for it


def test_abi_lists_track_posterior():
    from synchformer_amd import _lib
    assert _lib.ABI_VERSION >= 18 and len(_lib.SIGNATURES['sf_track_posterior']) == 14
    assert hasattr(_lib.load(), 'sf_track_posterior') and hasattr(_lib.load_ablation(), 'sf_track_posterior')


def test_offset_track_fields():
    """The fields OffsetTrack had keep their order (positional construction keeps working); the posterior ones come after them and default to None."""
    from synchformer_amd.track import OffsetTrack
    names = [f.name for f in dataclasses.fields(OffsetTrack)]
    old = ['t_sec', 'logits', 'cls_raw', 'conf_raw', 'cls_path', 'conf_path', 'offset_sec_raw', 'offset_sec_path', 'n_segments']
    new = ['post', 'cls_post', 'conf_post', 'offset_sec_post', 'offset_sec_mean', 'log_z']
    assert names == old + new, names
    tr = OffsetTrack(*range(len(old)))
    assert [getattr(tr, n) for n in old] == list(range(len(old))) and all(getattr(tr, n) is None for n in new)


def test_tracker_takes_posterior_flag():
    import inspect
    from synchformer_amd.track import OffsetTracker
    p = inspect.signature(OffsetTracker.__init__).parameters
    assert list(p)[:6] == ['self', 'engine', 'mel', 'hop_segments', 'lam', 'grid'] and p['posterior'].default is False
