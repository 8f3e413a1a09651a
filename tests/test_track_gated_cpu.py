"""No GPU: the float64 oracle of the gated read-outs (tests/track_gated_oracle.py) against a brute force over all (2C)^W state paths, the
identities and the two scenarios the design states, the launchers' argument handling (rejected before the device is touched), the ABI entries, the
sync-module-only engine's argument handling, checkpoint.same_towers, the tracker's argument errors and OffsetTrack.spans()."""
import ctypes
import inspect
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_gated_oracle as TG  # noqa: E402
from synchformer_amd.ops import track_decode_gated, track_posterior_gated  # noqa: E402,F401  what the oracle is the oracle OF: without the two entries nothing here stands


def _inputs(C: int, W: int):
    rng = np.random.default_rng(100 * C + W)
    return 3 * rng.standard_normal((W, C)), 3 * rng.standard_normal((W, 2))


@pytest.mark.parametrize('lam, mu', [(0.0, 0.0), (0.5, 1.0), (1.0, 4.0)])
@pytest.mark.parametrize('C, W', [(2, 5), (3, 4)])
def test_oracle_equals_brute_force(C, W, lam, mu):
    l, z = _inputs(C, W)
    E = TG.emission(l, z)
    assert np.abs(TG.lse(E, axis=1)).max() <= 1e-12                              # a true log-probability: every row sums to 1 over the 2C states
    bf = TG.brute_force(l, z, lam, mu)
    v = TG.viterbi(l, z, lam, mu)
    assert abs(v['score'] - bf['best']) <= 1e-12 and abs(TG.path_score(l, z, lam, mu, v['states']) - bf['best']) <= 1e-12
    assert np.array_equal(v['states'], v['sync_path'] * C + v['cls_path'])
    o = TG.posterior(l, z, lam, mu, np.linspace(-1, 1, C))
    assert np.abs(o['post2'] - bf['post2']).max() <= 1e-12 and abs(o['log_z'] - bf['log_z']) <= 1e-12
    assert np.abs(o['post'] - (bf['post2'][:, :C] + bf['post2'][:, C:])).max() <= 1e-12 and np.abs(o['p_sync'] - bf['post2'][:, C:].sum(1)).max() <= 1e-12
    assert np.abs(o['post'].sum(1) - 1).max() <= 1e-12 and o['log_z'] <= 1e-12
    if lam == 0 and mu == 0:                                                     # independent windows: the emission itself, log_z = 0
        assert np.abs(o['post2'] - np.exp(E)).max() <= 1e-12 and abs(o['log_z']) <= 1e-12


@pytest.mark.parametrize('lam, mu', [(0.5, 1.0), (1.0, 4.0)])
def test_oracle_row_reversal(lam, mu):
    """Reversed rows: reversed marginals of both the class and the flag, the same partition sum."""
    l, z = _inputs(3, 7)
    grid = np.linspace(-1, 1, 3)
    o, r = TG.posterior(l, z, lam, mu, grid), TG.posterior(l[::-1], z[::-1], lam, mu, grid)
    assert np.abs(r['post'][::-1] - o['post']).max() <= 1e-12 and np.abs(r['p_sync'][::-1] - o['p_sync']).max() <= 1e-12
    assert abs(r['log_z'] - o['log_z']) <= 1e-12


@pytest.mark.parametrize('mu', [0.0, 2.0, 16.0])
@pytest.mark.parametrize('lam', [0.5, 1.0])
def test_gap_scenario_on_the_oracle(lam, mu):
    """Sixty windows vote class 13 (+6), fifteen in the middle vote class 2 (+6) while the gate says 'not synchronizable' there: the joint path holds class 13
    throughout and flags exactly the gap; the ungated float64 chain follows the decoy (13 -> 2 -> 13)."""
    l, z = TG.gap_scenario()
    v = TG.viterbi(l, z, lam, mu)
    assert (v['cls_path'] == 13).all()
    assert np.array_equal(np.flatnonzero(v['sync_path'] == 0), np.arange(22, 37))
    plain = TG.ungated_viterbi(l, lam)
    assert (plain[22:37] == 2).all() and (plain[:22] == 13).all() and (plain[37:] == 13).all()


@pytest.mark.parametrize('lam', [0.0, 0.5, 1.0, 8.0])
def test_confident_gate_gives_the_ungated_path(lam):
    """d = +30 everywhere: plane 0 lies 30 below plane 1 in every window, the joint path is the ungated path with the flag set."""
    l = 3 * np.random.default_rng(17).standard_normal((80, 21))                  # continuous logits: no exact ties in either chain
    z = np.zeros((80, 2))
    z[:, 1] = 30.0
    v = TG.viterbi(l, z, lam, 2.0)
    assert (v['sync_path'] == 1).all() and np.array_equal(v['cls_path'], TG.ungated_viterbi(l, lam))
    l2, z2 = TG.gap_scenario()
    z2[:, 1] = 30.0
    assert np.array_equal(TG.viterbi(l2, z2, lam, 2.0)['cls_path'], TG.ungated_viterbi(l2, lam))


def _ptr(buf):
    p = ctypes.addressof(buf)
    return p + (-p) % 16


def test_abi_lists_the_gated_read_outs():
    from synchformer_amd import _lib
    assert _lib.ABI_VERSION >= 24
    assert len(_lib.SIGNATURES['sf_track_decode_gated']) == 16 and len(_lib.SIGNATURES['sf_track_posterior_gated']) == 18
    for lib in (_lib.load(), _lib.load_ablation()):
        assert lib.sf_abi_version() >= 24 and hasattr(lib, 'sf_track_decode_gated') and hasattr(lib, 'sf_track_posterior_gated')


def test_gated_argument_validation_without_gpu():
    """-1 plus a message, nothing launched - safe without a device."""
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = _ptr(buf)
    dec = ('logits', 'ldl', 'gate', 'ldg', 'W', 'C', 'lam', 'mu', 'cls_raw', 'conf_raw', 'sync_raw', 'cls_path', 'sync_path', 'conf_path', 'backptr')
    pos = ('logits', 'ldl', 'gate', 'ldg', 'W', 'C', 'lam', 'mu', 'grid', 'post', 'ldp', 'p_sync', 'cls_post', 'conf_post', 'offset_mean', 'log_z', 'workspace')
    good = dict(ldl=21, ldg=2, W=3, C=21, lam=1.0, mu=2.0, ldp=21)
    for fn, names in ((lib.sf_track_decode_gated, dec), (lib.sf_track_posterior_gated, pos)):
        ptrs = [n for n in names if n not in good]

        def call(**kw):
            a = dict({n: p for n in ptrs}, **good)
            a.update(kw)
            return fn(*[a[n] for n in names], None)

        for name in ptrs:
            assert call(**{name: None}) == -1 and b'null pointer' in lib.sf_last_error(), name
        for C in (1, 0, -3, 33, 64):
            assert call(C=C, ldl=128, ldp=128) == -1 and b'classes out of range' in lib.sf_last_error(), C
        assert call(C=32, ldl=31, ldp=32) == -1 and b'row stride ldl' in lib.sf_last_error()
        assert call(ldl=20) == -1 and b'row stride ldl' in lib.sf_last_error()
        assert call(ldg=1) == -1 and b'gate row stride' in lib.sf_last_error()
        for bad in (-0.5, float('inf'), float('-inf'), float('nan')):
            assert call(lam=bad) == -1 and b'lam must be finite' in lib.sf_last_error(), bad
            assert call(mu=bad) == -1 and b'mu must be finite' in lib.sf_last_error(), bad
        assert call(W=-1) == -1 and b'windows' in lib.sf_last_error()
        assert call(W=0) == 0                                                   # nothing to do: returns before any launch
        assert call(W=0, **{n: None for n in ptrs}) == 0                        # and needs no buffers for it
    assert lib.sf_track_posterior_gated(*[dict({n: p for n in pos}, **dict(good, ldp=20))[n] for n in pos], None) == -1 and b'post row stride' in lib.sf_last_error()


def test_sync_only_engine_argument_handling():
    """towers=False: a keyword after the existing ones, default True; it contradicts fp8_towers; the tower methods of such an engine raise before touching anything."""
    from synchformer_amd.engine import SynchformerEngine
    p = inspect.signature(SynchformerEngine.__init__).parameters
    assert list(p)[:5] == ['self', 'state_dict', 'device', 'seg_chunk', 'fp8_towers'] and p['towers'].default is True
    with pytest.raises(RuntimeError, match='HIP device'):
        SynchformerEngine({}, 'cpu', towers=False)
    with pytest.raises(ValueError, match='fp8_towers'):
        SynchformerEngine({}, 'cuda:0', fp8_towers=True, towers=False)           # rejected before the device is touched
    eng = object.__new__(SynchformerEngine)
    eng.towers = False
    for call in (lambda: eng.load_tower_weights({}), lambda: eng.extract_afeats(None), lambda: eng._visual_chunk(None, None)):
        with pytest.raises(RuntimeError, match='towers=False'):
            call()
    eng.towers = True
    eng._need_towers('x')


def test_same_towers():
    from synchformer_amd.checkpoint import same_towers
    g = torch.Generator().manual_seed(3)
    a = {'vfeat_extractor.w': torch.randn(4, 3, generator=g), 'afeat_extractor.b': torch.randn(5, generator=g), 'transformer.off_head.weight': torch.randn(21, 8, generator=g)}
    b = {k: v.clone() for k, v in a.items() if not k.startswith('transformer')}
    b['transformer.sync_head.weight'] = torch.randn(2, 8, generator=g)           # another sync module: not compared
    assert same_towers(a, b) and same_towers(b, a)
    c = dict(b)
    c['afeat_extractor.b'] = b['afeat_extractor.b'].clone()
    c['afeat_extractor.b'][2] += 1e-3
    assert not same_towers(a, c)
    assert not same_towers(a, {k: v for k, v in b.items() if k != 'afeat_extractor.b'})                # a key missing
    assert not same_towers(a, dict(b, **{'vfeat_extractor.extra': torch.zeros(1)}))                   # a key too many
    assert not same_towers(a, dict(b, **{'vfeat_extractor.w': b['vfeat_extractor.w'].reshape(3, 4)}))  # another shape
    assert not same_towers(a, dict(b, **{'vfeat_extractor.w': b['vfeat_extractor.w'].double()}))       # another dtype
    assert not same_towers({'transformer.x': torch.zeros(1)}, {'transformer.x': torch.zeros(1)})       # no towers at all: nothing vouches for the pairing


def _fake(n_out, n_window, dev='cpu'):
    return SimpleNamespace(n_out=n_out, n_window=n_window, dev=torch.device(dev))


def test_tracker_gate_argument_errors():
    from synchformer_amd.track import OffsetTracker
    p = inspect.signature(OffsetTracker.__init__).parameters
    assert list(p)[:7] == ['self', 'engine', 'mel', 'hop_segments', 'lam', 'grid', 'posterior'] and p['gate'].default is None and p['mu'].default == 2.0
    eng = _fake(21, 14)
    tr = OffsetTracker(eng, None, gate=_fake(2, 13), mu=0.0)
    assert tr.gate.n_window == 13 and tr.mu == 0.0 and OffsetTracker(eng, None).gate is None
    with pytest.raises(ValueError, match='syncability head has 2'):
        OffsetTracker(eng, None, gate=_fake(21, 14))
    with pytest.raises(ValueError, match='gate: on'):
        OffsetTracker(eng, None, gate=_fake(2, 13, 'meta'))
    with pytest.raises(ValueError, match='does not fit'):
        OffsetTracker(eng, None, gate=_fake(2, 15))
    with pytest.raises(ValueError, match='at most 32 classes'):
        OffsetTracker(_fake(33, 14), None, grid=torch.zeros(33), gate=_fake(2, 13))
    for mu in (-1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='mu ='):
            OffsetTracker(eng, None, gate=_fake(2, 13), mu=mu)
    with pytest.raises(NotImplementedError, match='3.20'):
        tr.stream()
    with pytest.raises(NotImplementedError, match='3.20'):
        tr.pool(4)


def test_spans():
    from synchformer_amd.track import OffsetTrack, window_times
    grid = torch.linspace(-2, 2, 21)
    cls = torch.tensor([13, 13, 13, 13, 2, 12, 12, 12], dtype=torch.int32)
    sync = torch.tensor([1, 1, 0, 0, 0, 1, 1, 1], dtype=torch.int32)
    t = window_times(8)
    tr = OffsetTrack(t_sec=t, logits=None, cls_raw=None, conf_raw=None, cls_path=cls, conf_path=None, offset_sec_raw=None, offset_sec_path=grid[cls.long()], n_segments=21)
    assert tr.gate_logits is None and tr.sync_raw is None and tr.sync_path is None and tr.p_sync is None
    plain = tr.spans()                                                           # no gate: runs of the class
    assert [s[2] for s in plain] == pytest.approx([0.6, -1.6, 0.4]) and plain[0][0] == pytest.approx(2.4) and plain[-1][1] == pytest.approx(2.4 + 7 * 0.32)
    tr.sync_path = sync
    sp = tr.spans()
    assert len(sp) == 4 and [s[2] is None for s in sp] == [False, True, True, False]
    assert sp[0][2] == pytest.approx(0.6) and sp[3][2] == pytest.approx(0.4)
    assert sp[0][0] == pytest.approx(2.4) and sp[0][1] == sp[1][0] == pytest.approx(2.4 + 1.5 * 0.32)      # spans meet half-way between the windows' centres
    assert sp[1][1] == sp[2][0] == pytest.approx(2.4 + 3.5 * 0.32) and sp[2][1] == sp[3][0] == pytest.approx(2.4 + 4.5 * 0.32)
    assert sp[3][1] == pytest.approx(2.4 + 7 * 0.32)
    one = OffsetTrack(t_sec=t[:1], logits=None, cls_raw=None, conf_raw=None, cls_path=cls[:1], conf_path=None, offset_sec_raw=None, offset_sec_path=grid[cls[:1].long()],
                      n_segments=14)
    assert one.spans() == [(pytest.approx(2.4), pytest.approx(2.4), pytest.approx(0.6))]
