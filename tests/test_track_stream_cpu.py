"""CPU: the fixed-lag read-out of a stream - the oracle's two statements agree, what the fixed lag changes against the offline path and the argmax,
the ABI table, and the launchers' argument checks (no device is touched)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_stream_oracle as TS  # noqa: E402

C21 = 21
INT_KEYS = ('cls_raw', 'cls_lag', 'cls_tail')


def _ints(W: int, lam: float, C: int = C21) -> np.ndarray:
    """the seed rule of tests/test_track_gpu.py::test_decode_exact"""
    return np.random.default_rng(1000 * W + int(2 * lam)).integers(-8, 9, (W, C)).astype(np.float64)


def _pushes(sizes, flush: bool):
    """sizes -> [(n, final)]: flush=True ends with an empty final push, otherwise the last push is the final one."""
    return [(n, False) for n in sizes] + [(0, True)] if flush else [(n, i == len(sizes) - 1) for i, n in enumerate(sizes)]


@pytest.mark.parametrize('lag', [0, 1, 7, 8, 9, 63])
@pytest.mark.parametrize('name', TS.CHUNKINGS)
def test_oracle_forms_agree(name, lag):
    """The incremental statement (carried scores, rings of `lag` rows) equals the definition (one offline read-out per prefix): classes exactly - integer logits,
    dyadic lam: both are exact -, probabilities and marginals to float64 rounding.  Its rings never hold more than `lag` rows."""
    grid = np.linspace(-2, 2, C21)
    for W, lam in ((1, 0.5), (2, 2.0), (lag + 2, 0.5), (70, 2.0)):
        x = _ints(W, lam)
        pushes = _pushes(TS.chunking(name, W, lag), flush=(W % 2 == 0))
        ref = TS.by_definition(x, lam, lag, pushes, grid)
        inc = TS.StreamOracle(C21, lam, lag, grid)
        rows = 0
        for (n, final), want in zip(pushes, ref):
            got = inc.push(x[rows:rows + n], final)
            rows += n
            assert inc.held() <= lag
            assert got['w0'] == want['w0']
            for k in INT_KEYS + ('cls_post_lag',):
                assert np.array_equal(got[k], want[k]), (k, W, lam, got[k], want[k])
            for k in ('conf_raw', 'conf_lag', 'conf_tail', 'post_lag', 'conf_post_lag', 'offset_mean_lag'):
                assert got[k].shape == want[k].shape and (got[k].size == 0 or np.abs(got[k] - want[k]).max() <= 1e-12), k
            assert abs(got['log_z'] - want['log_z']) <= 1e-9 * max(1.0, abs(want['log_z']))
        assert sum(len(d['cls_lag']) for d in ref) == W


def test_full_lag_is_the_offline_path():
    for W, lam in ((1, 0.5), (9, 0.5), (70, 2.0)):
        x = _ints(W, lam)
        for lag in (W - 1, W, 255):
            if lag < 0:
                continue
            out = TS.by_definition(x, lam, lag, _pushes(TS.chunking('ragged', W, lag), flush=True))
            assert np.array_equal(np.concatenate([d['cls_lag'] for d in out]), TS.viterbi(x, lam))
            assert all(len(d['cls_lag']) == 0 for d in out[:-1]) or lag < W


def test_fixed_lag_differs_from_offline_and_argmax():
    """What a stream that returned the offline path, the argmax, or ignored `lag` would get wrong: W = 70, lam = 2 on test_decode_exact's input."""
    x = _ints(70, 2.0)
    offline, raw = TS.viterbi(x, 2.0), x.argmax(1)
    pre = TS.prefix_readouts(x, 2.0)
    diff = {}
    for lag in (0, 1, 7, 8, 9, 63):
        cls = np.concatenate([d['cls_lag'] for d in TS.by_definition(x, 2.0, lag, [(70, False), (0, True)], pre=pre)])
        diff[lag] = int((cls != offline).sum())
        if lag < 63:
            assert (cls != raw).sum() >= 47, (lag, (cls != raw).sum())
    print(diff)
    assert diff == {0: 46, 1: 36, 7: 12, 8: 10, 9: 9, 63: 0}, diff


def test_signatures_and_abi():
    from synchformer_amd import _lib
    assert _lib.ABI_VERSION >= 19
    assert len(_lib.SIGNATURES['sf_track_stream_push']) == 25 and len(_lib.SIGNATURES['sf_track_stream_bytes']) == 3
    assert len(_lib.SIGNATURES['sf_track_stream_workspace_bytes']) == 3
    lib = _lib.load()
    assert lib.sf_abi_version() >= 19
    # the state's size: bounded, independent of the rows that pass, growing with lag and with the posterior
    sizes = {(C, lag, post): lib.sf_track_stream_bytes(C, lag, post) for C in (2, 21, 64) for lag in (0, 16, 255) for post in (0, 1)}
    assert all(0 < v <= 16 + 512 + 255 * 64 * 9 + 16 and v % 16 == 0 for v in sizes.values()), sizes
    assert sizes[(21, 16, 0)] >= 16 * 21 * 5 and sizes[(21, 16, 1)] >= 16 * 21 * 9 and sizes[(64, 255, 1)] > sizes[(64, 255, 0)] > sizes[(64, 16, 0)]
    assert lib.sf_track_stream_workspace_bytes(21, 1000, 1) >= 1000 * (21 * 5 + 4)


def test_bad_arguments_are_rejected_without_a_device():
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)

    def push(state=p, C=21, lag=16, rows=0, n=1, lam=1.0, logits=p):
        return lib.sf_track_stream_push(state, C, lag, 0, rows, logits, C, n, lam, None, 0, p, p, p, p, None, C, None, None, None, p, p, None, p, None)

    for kw, msg in ((dict(C=1), b'classes out of range'), (dict(C=65), b'classes out of range'), (dict(lag=256), b'lag = 256'), (dict(lag=-1), b'lag = -1'),
                    (dict(lam=-1.0), b'lam must be finite'), (dict(lam=float('nan')), b'lam must be finite'), (dict(state=None), b'null state'),
                    (dict(n=-1), b'rows in one push'), (dict(rows=-1), b'rows pushed so far'), (dict(logits=None), b'null pointer')):
        assert push(**kw) == -1 and msg in lib.sf_last_error(), (kw, lib.sf_last_error())
    assert lib.sf_track_stream_bytes(1, 16, 0) == -1 and lib.sf_track_stream_bytes(65, 16, 0) == -1 and lib.sf_track_stream_bytes(21, 256, 1) == -1
    assert lib.sf_track_stream_workspace_bytes(21, -1, 0) == -1
    assert push(n=0) == 0                                                          # an empty push on an empty stream: nothing to launch
    from synchformer_amd import ops
    with pytest.raises(RuntimeError, match='lag = 256'):
        ops.track_stream_state(21, 256, False, 'cpu')
    assert ops.track_stream_counts(0, 5, 16) == (0, 0, 5) and ops.track_stream_counts(5, 20, 16) == (0, 9, 16) and ops.track_stream_counts(25, 0, 16, True) == (9, 16, 0)
    for rows, n, lag, final in ((0, 0, 3, False), (0, 1, 0, False), (7, 3, 3, False), (2, 9, 3, True), (40, 0, 255, True)):
        assert ops.track_stream_counts(rows, n, lag, final) == TS.counts(rows, n, lag, final)


def test_pinned_digest_inputs():
    """tests/golden/track_stream_digests.json (the bytes tests/test_track_pinned_gpu.py holds the read-outs to) against its generator, without a GPU: the recorded case
    set is the generator's, every case's inputs - drawn on the CPU under fixed seeds - still hash to what was recorded, and the chunk pattern has the pushes it must
    have: 0 rows on the empty stream, the first row alone, a push below the lag, one equal to it, one above it, 0 rows in mid-stream, and rows left for the rest."""
    import json
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import make_track_stream_digests as TD
    with open(TD.OUT) as f:
        rec = json.load(f)
    assert len(rec['recorded_from']) == 40 and set(rec['cases']) == set(TD.CASES)
    for name in TD.CASES:
        assert TD.input_digest(name) == rec['cases'][name]['input'], f'{name}: the generated INPUT differs from the recorded one'
    for lag in (0, 1, 16, 255):
        c = TD.chunks(lag)
        assert c[:2] == (0, 1) and c[2] <= lag // 2 and c[3] == lag and c[4] > lag and c[5] == 0 and c[6] is None
        assert TD.n_rows(lag) >= 300 and TD.n_rows(lag) - sum(c[:6]) >= 20
