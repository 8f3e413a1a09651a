"""No GPU: the float64 oracle of the wide chain (tests/track_wide_oracle.py) against a brute force over all S^W paths and against the plain chain's oracle, the states
table (ops.track_wide_states), the window arithmetic of a search over lags (frontend.lagged_window_geometry), the ABI entries and the launchers' argument handling
(rejected before the device is touched)."""
import ctypes
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_posterior_oracle as TP  # noqa: E402
import track_wide_oracle as TW  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


def _case(D, C, W, gate, seed):
    rng = np.random.default_rng(seed)
    x = 3 * rng.standard_normal((W, D, C))
    z = 2 * rng.standard_normal((W, D, 2)) if gate else None
    return (x, z) + _tables(range(-(D // 2), D - D // 2), 0.2 * np.arange(C) - 0.2)


def _tables(lags, grid):
    """The states table the product builds (ops.track_wide_states), checked against the oracle's own and handed on in float64 -> (src, pos, off, lag_of)."""
    from synchformer_amd import ops
    src, pos, off, lag_of, cls_of = ops.track_wide_states(lags, grid)
    o = TW.states(lags, grid)
    assert np.array_equal(src.numpy(), o[0]) and np.array_equal(lag_of.numpy(), o[3]) and np.array_equal(cls_of.numpy(), o[4])
    assert np.array_equal(pos.numpy(), o[1].astype(np.float32)) and np.array_equal(off.numpy(), o[2].astype(np.float32))
    return src.numpy().astype(np.int64), pos.double().numpy(), off.double().numpy(), lag_of.numpy().astype(np.int64)


def _check_against_brute_force(x, z, src, pos, off, lag_of, lam):
    D = x.shape[1]
    e = TW.emission(x, src, z)
    o = TW.posterior(e, pos, lam, off, lag_of, D)
    post, log_z, best, _ = TW.brute_force(e, pos, lam)
    assert np.abs(o['post'] - post).max() <= 1e-12 and abs(o['log_z'] - log_z) <= 1e-12, (np.abs(o['post'] - post).max(), o['log_z'], log_z)
    assert np.abs(o['post'].sum(1) - 1).max() <= 1e-12 and np.abs(o['p_lag'].sum(1) - 1).max() <= 1e-12
    assert np.abs(o['offset_mean'] - post @ off).max() <= 1e-12
    if z is None:                                                                # every window's emissions sum to D over the states (one softmax per lag): Z <= D^W,
        assert o['log_z'] <= x.shape[0] * np.log(D) + 1e-12                      # with equality at lam = 0; a bound of log D holds only in the limit of a large lam
        if lam == 0:
            assert abs(o['log_z'] - x.shape[0] * np.log(D)) <= 1e-12
    for rc in (True, False):                                                     # the row constant changes the score of every path by the same amount, not the path
        ev = TW.emission(x, src, z, row_constant=rc)
        raw, path = TW.viterbi(ev, pos, lam)
        assert abs(TW.path_score(e, pos, lam, path) - best) <= 1e-12, (path, best)
        assert np.array_equal(raw, e.argmax(1))
    return o


@pytest.mark.parametrize('gate', [False, True])
@pytest.mark.parametrize('lam', [0.0, 0.5, 3.0])
@pytest.mark.parametrize('D, C, W', [(1, 2, 4), (2, 2, 5), (3, 3, 3)])
def test_oracle_equals_brute_force(D, C, W, lam, gate):
    x, z, src, pos, off, lag_of = _case(D, C, W, gate, 100 * D + 10 * C + W)
    assert np.all(np.diff(pos) >= 0)
    _check_against_brute_force(x, z, src, pos, off, lag_of, lam)


def test_oracle_equals_brute_force_with_a_masked_state():
    """One (lag, class) pair is -inf in every window, another in one window: exactly 0 there, no NaN, everything else as enumerated."""
    x, z, src, pos, off, lag_of = _case(2, 3, 4, False, 7)
    x[:, 1, 0] = -np.inf
    x[2, 0, 2] = -np.inf
    o = _check_against_brute_force(x, z, src, pos, off, lag_of, 0.5)
    s_all, s_one = int(np.nonzero(src == 3)[0][0]), int(np.nonzero(src == 2)[0][0])
    assert np.isfinite(o['post']).all() and (o['post'][:, s_all] == 0).all() and o['post'][2, s_one] == 0 and (o['post'][[0, 1, 3], s_one] > 0).all()


def _plain_viterbi(x, lam):
    """The plain chain's mode in float64: e = log-softmax, cost lam |p - c|, the lowest predecessor and the lowest end state on ties."""
    e = TP.log_softmax(x)
    W, C = e.shape
    pen = lam * np.abs(np.arange(C)[:, None] - np.arange(C)[None, :])
    s, back = e[0].copy(), np.zeros((W, C), np.int64)
    for w in range(1, W):
        cand = s[:, None] - pen
        back[w] = cand.argmax(0)
        s = cand.max(0) + e[w]
    path = [int(s.argmax())]
    for w in range(W - 1, 0, -1):
        path.append(int(back[w, path[-1]]))
    return np.array(path[::-1])


@pytest.mark.parametrize('lam', [0.0, 0.5, 3.0])
@pytest.mark.parametrize('C, W', [(2, 3), (21, 40), (64, 9)])
def test_one_lag_is_the_plain_chain(C, W, lam):
    """lags = (0,) (pos = arange(C) - 10: the same chain as arange(C)), no gate: the wide oracle's posterior is track_posterior_oracle's, its path a plain float64 Viterbi's."""
    x = 3 * np.random.default_rng(C + W).standard_normal((W, C))
    src, pos, grid, lag_of = _tables((0,), 0.2 * np.arange(C) - 2.0)                 # ops.track_wide_states: pos = c - 10, the class grid as the offsets
    assert np.array_equal(src, np.arange(C)) and np.array_equal(pos, np.arange(C) - 10.0)
    e = TW.emission(x[:, None, :], src)
    o = TW.posterior(e, pos, lam, grid, lag_of, 1)
    ref = TP.posterior(x, lam, grid)
    assert np.abs(o['post'] - ref['post']).max() <= 1e-12 and abs(o['log_z'] - ref['log_z']) <= 1e-12
    assert np.abs(o['offset_mean'] - ref['offset_mean']).max() <= 1e-12 and np.array_equal(o['state_post'], ref['cls_post'])
    assert np.abs(o['p_lag'] - 1).max() <= 1e-12
    assert np.array_equal(TW.viterbi(e, pos, lam)[1], _plain_viterbi(x, lam))


def test_track_wide_states():
    import torch
    from synchformer_amd import ops
    from synchformer_amd.postprocess import class_grid
    grid = class_grid(-2, 2, 21)
    src, pos, off, lag_of, cls_of = ops.track_wide_states(range(-5, 6), grid)
    assert [t.dtype for t in (src, pos, off, lag_of, cls_of)] == [torch.int32, torch.float32, torch.float32, torch.int32, torch.int32]
    assert src.shape == pos.shape == off.shape == (231,) and torch.equal(src, lag_of * 21 + cls_of) and sorted(src.tolist()) == list(range(231))
    assert (off[1:] >= off[:-1]).all() and (pos[1:] >= pos[:-1]).all()
    lags = list(range(-5, 6))
    want = 0.32 * torch.tensor([lags[d] for d in lag_of.tolist()], dtype=torch.float64) + grid.double()[cls_of.long()]
    assert (off.double() - want).abs().max() <= 1e-6
    assert (pos.double() - off.double() / 0.2).abs().max() <= 1e-5
    # lag 5 / class 2 (1.6 - 1.6) and lag 0 / class 10 (0.0) coincide, and stand in the order (offset, lag, class): lag 0 first
    s_a = int(torch.nonzero((lag_of == 5) & (cls_of == 10))[0])      # lag index 5 = lag 0
    s_b = int(torch.nonzero((lag_of == 10) & (cls_of == 2))[0])      # lag index 10 = lag 5
    assert pos[s_a] == pos[s_b] == 0.0 and off[s_a] == off[s_b] == 0.0 and s_b == s_a + 1
    key = [(float(p), int(d), int(c)) for p, d, c in zip(pos, lag_of, cls_of)]
    assert key == sorted(key)
    # the float64 oracle's table is the same table
    o = TW.states(range(-5, 6), grid.double().numpy())
    assert np.array_equal(o[0], src.numpy()) and np.array_equal(o[1].astype(np.float32), pos.numpy()) and np.array_equal(o[2].astype(np.float32), off.numpy())
    # one lag: the class grid itself
    src, pos, off, lag_of, cls_of = ops.track_wide_states((0,), grid)
    assert torch.equal(pos, torch.arange(21, dtype=torch.float32) - 10) and torch.equal(src, torch.arange(21, dtype=torch.int32))
    assert torch.equal(off, grid) and int(lag_of.max()) == 0
    for bad in ((), (1, 1), (2, 1)):
        with pytest.raises(ValueError):
            ops.track_wide_states(bad, grid)
    with pytest.raises(ValueError, match='microsecond'):                             # a step of 1/3 s is not on the lattice the offsets are taken to
        ops.track_wide_states((0, 1), torch.arange(7, dtype=torch.float64) / 3)
    assert ops.track_wide_states((0, 1), torch.arange(7, dtype=torch.float64) / 4)[0].numel() == 14


def test_lagged_window_geometry():
    from synchformer_amd.frontend import lagged_window_geometry as G
    for lags, hop, N in [((-3, -1), 1, 24), ((1, 4), 1, 24), ((-3, 0, 2), 1, 24), ((-3, 0, 2), 3, 24), ((0,), 1, 14), ((-2, 5), 3, 40), ((-3, 0, 2), 2, 19)]:
        g = G(N, lags, hop)
        W, v0 = g['n_windows'], g['v0']
        assert v0 == max(0, -lags[0]) and W == (N - 14 - v0 - max(0, lags[-1])) // hop + 1 and W >= 1
        lo = min(v0 + d for d in lags)
        hi = max(v0 + d + (W - 1) * hop + 14 for d in list(lags) + [0])
        assert lo >= 0 and hi <= N and hi + hop > N, (lags, hop, N, lo, hi)     # inside the bank, and one more hop would leave it
    assert G(24, (-3, 0, 2), 1)['n_windows'] == 6 and G(24, (-3, 0, 2), 2)['n_windows'] == 3
    assert G(19, (-3, 0, 2), 1)['n_windows'] == 1                               # the last (only) window's audio at lag 2 touches segment 18
    assert G(20, (0,), 1, n_window=13)['n_windows'] == 8
    with pytest.raises(ValueError):
        G(18, (-3, 0, 2), 1)
    for bad in ((0, 0), (2, 1), ()):
        with pytest.raises(ValueError):
            G(40, bad, 1)
    with pytest.raises(ValueError):
        G(40, (0,), 0)


def test_abi_lists_the_wide_entries():
    from synchformer_amd import _lib
    text = (ROOT / 'include' / 'synchformer_hip.h').read_text()
    assert int(re.search(r'#define SF_ABI_VERSION (\d+)', text).group(1)) == 25 == _lib.ABI_VERSION
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, n in (('sf_track_wide_workspace_bytes', 5), ('sf_track_decode_wide', 21), ('sf_track_posterior_wide', 25)):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', text, flags=re.S)
        assert m is not None, f'{name} is not declared'
        assert len(m.group(1).split(',')) == n == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load_ablation(), name)
    assert _lib.load().sf_abi_version() == 25


def _ptr(buf):
    p = ctypes.addressof(buf)
    return p + (-p) % 16


def test_wide_argument_validation_without_gpu():
    """The launchers' convention: -1 plus a message, nothing launched - safe without a device."""
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = _ptr(buf)
    D, C, S = 3, 4, 12
    src = (ctypes.c_int32 * S)(*range(S))
    pos = (ctypes.c_float * S)(*[0.5 * s for s in range(S)])
    head = ('logits', 'ldw', 'ldd', 'gate', 'ldgw', 'ldgd', 'W', 'D', 'C', 'S', 'src_host', 'pos_host', 'src_dev', 'pos_dev', 'lam')
    good = dict(logits=p, ldw=D * C, ldd=C, gate=None, ldgw=2 * D, ldgd=2, W=3, D=D, C=C, S=S, src_host=ctypes.addressof(src), pos_host=ctypes.addressof(pos), src_dev=p,
                pos_dev=p, lam=1.0)
    tails = {'sf_track_decode_wide': ('state_raw', 'conf_raw', 'state_path', 'conf_path', 'workspace'),
             'sf_track_posterior_wide': ('off', 'post', 'ldp', 'state_post', 'conf_post', 'offset_mean', 'p_lag', 'log_z', 'workspace')}
    for entry, tail in tails.items():
        fn = getattr(lib, entry)

        def call(**kw):
            a = dict(good, **{n: p for n in tail})
            a['ldp'] = S
            a.update(kw)
            return fn(*[a[n] for n in head + tail], None)

        for name in ('logits', 'src_host', 'pos_host', 'src_dev', 'pos_dev') + tuple(n for n in tail if n != 'ldp'):
            assert call(**{name: None}) == -1 and b'null pointer' in lib.sf_last_error(), (entry, name)
        for bad in (1, 0, -3, 1025):
            assert call(S=bad) == -1 and b'states out of range' in lib.sf_last_error(), bad
        for bad in (1, 0, 65):
            assert call(C=bad, ldd=128, ldw=1024) == -1 and b'classes out of range' in lib.sf_last_error(), bad
        for bad in (0, -1, 1025):
            assert call(D=bad, ldw=1 << 20) == -1 and b'lags out of range' in lib.sf_last_error(), bad
        assert call(S=13) == -1 and b'pairs' in lib.sf_last_error()
        assert call(ldd=C - 1) == -1 and b'lag stride' in lib.sf_last_error()
        assert call(ldw=D * C - 1) == -1 and b'row stride' in lib.sf_last_error()
        assert call(gate=p, ldgd=1) == -1 and b'gate lag stride' in lib.sf_last_error()
        assert call(gate=p, ldgw=2 * D - 1) == -1 and b'gate row stride' in lib.sf_last_error()
        for lam in (-0.5, float('inf'), float('nan')):
            assert call(lam=lam) == -1 and b'lam must be finite' in lib.sf_last_error(), lam
        assert call(W=-1) == -1 and b'windows' in lib.sf_last_error()
        down = (ctypes.c_float * S)(*[0.5 * s for s in range(S)])
        down[5] = 1.0                                                            # below pos[4] = 2.0
        assert call(pos_host=ctypes.addressof(down)) == -1 and b'ascending' in lib.sf_last_error()
        down[5] = float('nan')
        assert call(pos_host=ctypes.addressof(down)) == -1 and b'ascending' in lib.sf_last_error()
        twice = (ctypes.c_int32 * S)(*range(S))
        twice[7] = 2
        assert call(src_host=ctypes.addressof(twice)) == -1 and b'repeats' in lib.sf_last_error()
        twice[7] = D * C
        assert call(src_host=ctypes.addressof(twice)) == -1 and b'outside' in lib.sf_last_error()
        twice[7] = -1
        assert call(src_host=ctypes.addressof(twice)) == -1 and b'outside' in lib.sf_last_error()
        assert call(W=0) == 0                                                    # nothing to do: returns before any launch
        assert call(W=0, logits=None, workspace=None, src_host=None, pos_host=None) == 0
    assert call(ldp=S - 1) == -1 and b'post row stride' in lib.sf_last_error()   # (the posterior entry, the last of the loop)
    n = ctypes.c_int64(-1)
    assert lib.sf_track_wide_workspace_bytes(300, 25, 525, 0, ctypes.addressof(n)) == 0 and n.value >= 300 * 25 * 4 + 300 * 525 * 2
    assert lib.sf_track_wide_workspace_bytes(300, 25, 525, 1, ctypes.addressof(n)) == 0 and n.value >= 300 * 25 * 4 + 2 * 300 * 525 * 4 and n.value % 16 == 0
    assert lib.sf_track_wide_workspace_bytes(11000, 48, 1008, 1, ctypes.addressof(n)) == 0 and n.value > 2 * 11000 * 1008 * 4
    assert lib.sf_track_wide_workspace_bytes(3, 25, 1025, 0, ctypes.addressof(n)) == -1 and lib.sf_track_wide_workspace_bytes(3, 25, 525, 0, None) == -1


def test_wide_track_dataclass_and_tracker_methods():
    import dataclasses
    import inspect
    from synchformer_amd.track import OffsetTrack, OffsetTracker, WideOffsetTrack
    names = [f.name for f in dataclasses.fields(WideOffsetTrack)]
    assert names[:16] == ['t_sec', 'lags', 'logits', 'gate_logits', 'lag_raw', 'cls_raw', 'conf_raw', 'offset_sec_raw', 'state_path', 'lag_path', 'cls_path', 'conf_path',
                          'offset_sec_path', 'n_segments', 'first_segment', 'post'], names
    assert names[16:] == ['p_lag', 'state_post', 'conf_post', 'offset_sec_post', 'offset_sec_mean', 'log_z']
    assert [f.name for f in dataclasses.fields(OffsetTrack)][:9] == ['t_sec', 'logits', 'cls_raw', 'conf_raw', 'cls_path', 'conf_path', 'offset_sec_raw', 'offset_sec_path',
                                                                      'n_segments']
    for m in ('track_features_wide', 'track_wide', 'track_raw_wide', 'track_logits_wide'):
        assert 'lags' in inspect.signature(getattr(OffsetTracker, m)).parameters
