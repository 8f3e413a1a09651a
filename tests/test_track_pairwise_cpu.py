"""No GPU: the float64 oracle of the pairwise read-out (tests/track_pairwise_oracle.py) against a brute-force enumeration of all paths, the identities the contract
states (marginals of xi = post, sum jump_abs = -d log_z / d lam, sum p_flip = -d log_z / d mu, lam = 0, reversed rows), the argument handling of sf_track_pairwise /
sf_track_pairwise_gated (rejected before the device is touched), their ABI entries, and the host side of OffsetTrack: changes() and expected_changes()."""
import ctypes
import dataclasses
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_gated_oracle as TG  # noqa: E402
import track_pairwise_oracle as PW  # noqa: E402
import track_posterior_oracle as TP  # noqa: E402


def _softmax64(x):
    p = np.exp(x - x.max(1, keepdims=True))
    return p / p.sum(1, keepdims=True)


def _class_pairs(xi2, C):
    return xi2[:, :C, :C] + xi2[:, :C, C:] + xi2[:, C:, :C] + xi2[:, C:, C:]


def _check_derived(o, xi):
    """p_change, jump_abs and the top pair of the oracle's dict against their definitions on xi (W-1, C, C), by loops."""
    n, C = xi.shape[:2]
    for w in range(n):
        off = [(xi[w, p, c], -p, -c) for p in range(C) for c in range(C) if p != c]
        best = max(off)                                                          # the largest mass, then the lowest p, then the lowest c
        assert (o['top_from'][w], o['top_to'][w]) == (-best[1], -best[2]) and o['p_top'][w] == best[0]
        assert abs(o['p_change'][w] - sum(v for v, _, _ in off)) <= 1e-12
        assert abs(o['jump_abs'][w] - sum(xi[w, p, c] * abs(p - c) for p in range(C) for c in range(C))) <= 1e-12


@pytest.mark.parametrize('lam', [0.0, 0.5, 3.0])
@pytest.mark.parametrize('C, W', [(3, 5), (4, 4), (2, 10)])
def test_oracle_equals_brute_force(C, W, lam):
    x = 3 * np.random.default_rng(100 * C + W).standard_normal((W, C))
    o = PW.pairwise(x, lam)
    xi, log_z = PW.brute_force(x, lam)
    assert o['xi'].shape == (W - 1, C, C) and np.abs(o['xi'] - xi).max() <= 1e-12 and abs(o['log_z'] - log_z) <= 1e-12
    _check_derived(o, o['xi'])


@pytest.mark.parametrize('lam, mu', [(0.0, 0.0), (0.5, 2.0), (3.0, 0.5)])
@pytest.mark.parametrize('C, W', [(2, 6), (3, 4)])
def test_gated_oracle_equals_brute_force(C, W, lam, mu):
    rng = np.random.default_rng(200 * C + W)
    x, z = 3 * rng.standard_normal((W, C)), 2 * rng.standard_normal((W, 2))
    o = PW.pairwise_gated(x, z, lam, mu)
    xi2, log_z = PW.brute_force(x, lam, z, mu)
    assert np.abs(o['xi2'] - xi2).max() <= 1e-12 and abs(o['log_z'] - log_z) <= 1e-12
    assert np.abs(o['xi'] - _class_pairs(xi2, C)).max() <= 1e-12
    assert np.abs(o['p_flip'] - (xi2[:, :C, C:].sum((1, 2)) + xi2[:, C:, :C].sum((1, 2)))).max() <= 1e-12
    _check_derived(o, o['xi'])


def test_oracle_equals_brute_force_with_a_masked_class():
    """Column 1 is -inf in every row, column 3 in two rows: pairs with a masked end are exactly 0, nothing is NaN, the rest is as enumerated."""
    x = 3 * np.random.default_rng(5).standard_normal((4, 4))
    x[:, 1] = -np.inf
    x[[0, 2], 3] = -np.inf
    o = PW.pairwise(x, 0.5)
    xi, log_z = PW.brute_force(x, 0.5)
    assert all(np.isfinite(o[k]).all() for k in ('xi', 'p_change', 'jump_abs', 'p_top'))
    assert np.abs(o['xi'] - xi).max() <= 1e-12 and abs(o['log_z'] - log_z) <= 1e-12
    assert (o['xi'][:, 1, :] == 0).all() and (o['xi'][:, :, 1] == 0).all()
    assert (o['xi'][0, 3, :] == 0).all() and (o['xi'][1, :, 3] == 0).all() and (o['xi'][2, 3, :] == 0).all() and (o['xi'][1, 0, :].sum() > 0)
    _check_derived(o, o['xi'])


def test_no_off_diagonal_mass_names_the_first_pair():
    """Two classes, one of them masked: all mass on one diagonal entry -> (0, 1) with p_top = 0, the contract's tie rule."""
    x = np.zeros((3, 2))
    x[:, 1] = -np.inf
    o = PW.pairwise(x, 1.0)
    assert o['top_from'].tolist() == [0, 0] and o['top_to'].tolist() == [1, 1] and o['p_top'].tolist() == [0.0, 0.0] and o['p_change'].tolist() == [0.0, 0.0]


@pytest.mark.parametrize('lam', [0.0, 0.5, 3.0])
def test_marginals_of_xi_are_the_posterior(lam):
    x = 3 * np.random.default_rng(11).standard_normal((30, 7))
    o, post = PW.pairwise(x, lam), TP.posterior(x, lam, np.arange(7.0))
    assert np.abs(o['xi'].sum(2) - post['post'][:-1]).max() <= 1e-12 and np.abs(o['xi'].sum(1) - post['post'][1:]).max() <= 1e-12
    assert abs(o['log_z'] - post['log_z']) <= 1e-12 and np.abs(o['xi'].sum((1, 2)) - 1).max() <= 1e-12
    z = 2 * np.random.default_rng(12).standard_normal((30, 2))
    g, gpost = PW.pairwise_gated(x, z, lam, 1.5), TG.posterior(x, z, lam, 1.5, np.arange(7.0))
    assert np.abs(g['xi'].sum(2) - gpost['post'][:-1]).max() <= 1e-12 and np.abs(g['xi'].sum(1) - gpost['post'][1:]).max() <= 1e-12
    assert np.abs(g['xi2'].sum(2) - gpost['post2'][:-1]).max() <= 1e-12 and abs(g['log_z'] - gpost['log_z']) <= 1e-12


def test_expected_jumps_and_flips_are_the_gradient_of_log_z():
    """sum_w jump_abs = -d log_z / d lam and sum_w p_flip = -d log_z / d mu (central differences, 1e-6 relative): what makes the fit of lam / mu a root search."""
    rng = np.random.default_rng(13)
    x, z, h = 3 * rng.standard_normal((300, 21)), 2 * rng.standard_normal((300, 2)), 1e-5
    for lam in (0.5, 1.0, 2.0):
        got = PW.pairwise(x, lam)['jump_abs'].sum()
        fd = -(PW.pairwise(x, lam + h)['log_z'] - PW.pairwise(x, lam - h)['log_z']) / (2 * h)
        assert abs(got - fd) <= 1e-6 * abs(fd), (lam, got, fd)
    x, z = x[:120, :9], z[:120]
    for lam, mu in ((0.5, 2.0), (2.0, 0.5)):
        o = PW.pairwise_gated(x, z, lam, mu)
        fd_lam = -(PW.pairwise_gated(x, z, lam + h, mu)['log_z'] - PW.pairwise_gated(x, z, lam - h, mu)['log_z']) / (2 * h)
        fd_mu = -(PW.pairwise_gated(x, z, lam, mu + h)['log_z'] - PW.pairwise_gated(x, z, lam, mu - h)['log_z']) / (2 * h)
        assert abs(o['jump_abs'].sum() - fd_lam) <= 1e-6 * abs(fd_lam) and abs(o['p_flip'].sum() - fd_mu) <= 1e-6 * abs(fd_mu), (o['p_flip'].sum(), fd_mu)


def test_independent_windows_and_reversed_rows():
    x = 3 * np.random.default_rng(14).standard_normal((12, 5))
    p = _softmax64(x)
    o = PW.pairwise(x, 0.0)                                                      # lam = 0: the outer product of neighbouring softmaxes
    assert np.abs(o['xi'] - p[:-1, :, None] * p[1:, None, :]).max() <= 1e-12 and abs(o['log_z']) <= 1e-12
    o, r = PW.pairwise(x, 0.7), PW.pairwise(x[::-1], 0.7)                        # reversed rows: reversed boundaries, transposed pairs
    assert np.abs(r['xi'][::-1].transpose(0, 2, 1) - o['xi']).max() <= 1e-12 and abs(r['log_z'] - o['log_z']) <= 1e-12
    assert np.abs(r['p_change'][::-1] - o['p_change']).max() <= 1e-12 and np.abs(r['jump_abs'][::-1] - o['jump_abs']).max() <= 1e-12


def test_sample_path_draws_from_the_chain():
    """The empirical pair frequencies of 4000 draws on a tiny chain against the enumerated pair marginals (5 standard errors of a frequency)."""
    rng = np.random.default_rng(15)
    x = rng.standard_normal((4, 3))
    xi, _ = PW.brute_force(x, 1.0)
    n = 4000
    paths = np.stack([PW.sample_path(rng, x, 1.0) for _ in range(n)])
    freq = np.zeros_like(xi)
    for w in range(3):
        np.add.at(freq[w], (paths[:, w], paths[:, w + 1]), 1.0 / n)
    assert np.abs(freq - xi).max() <= 5 * np.sqrt(0.25 / n), np.abs(freq - xi).max()
    z = rng.standard_normal((4, 2))
    states = PW.sample_path(rng, x, 1.0, z, 2.0)
    assert states.shape == (4,) and states.min() >= 0 and states.max() < 6


def _ptr(buf):
    p = ctypes.addressof(buf)
    return p + (-p) % 16


def test_track_pairwise_argument_validation_without_gpu():
    """The launcher's convention (test_track_posterior_argument_validation_without_gpu): -1 plus a message, nothing launched - safe without a device."""
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = _ptr(buf)
    names = ('logits', 'ldl', 'W', 'C', 'lam', 'p_change', 'jump_abs', 'top_from', 'top_to', 'p_top', 'xi', 'log_z', 'workspace')
    good = dict(logits=p, ldl=21, W=3, C=21, lam=1.0, p_change=p, jump_abs=p, top_from=p, top_to=p, p_top=p, xi=None, log_z=p, workspace=p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sf_track_pairwise(*[a[n] for n in names], None)

    for name in ('logits', 'p_change', 'jump_abs', 'top_from', 'top_to', 'p_top', 'log_z', 'workspace'):
        assert call(**{name: None}) == -1 and b'null pointer' in lib.sf_last_error(), name
    for C in (1, 0, -3, 65):
        assert call(C=C, ldl=128) == -1 and b'classes out of range' in lib.sf_last_error(), C
    assert call(ldl=20) == -1 and b'row stride ldl' in lib.sf_last_error()
    for lam in (-0.5, float('inf'), float('-inf'), float('nan')):
        assert call(lam=lam) == -1 and b'lam must be finite' in lib.sf_last_error(), lam
    assert call(W=-1) == -1 and b'windows' in lib.sf_last_error()
    assert call(W=0) == 0                                                       # nothing to do: returns before any launch
    assert call(W=0, logits=None, p_change=None, log_z=None, workspace=None) == 0


def test_track_pairwise_gated_argument_validation_without_gpu():
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = _ptr(buf)
    names = ('logits', 'ldl', 'gate_logits', 'ldg', 'W', 'C', 'lam', 'mu', 'p_change', 'jump_abs', 'p_flip', 'top_from', 'top_to', 'p_top', 'xi', 'log_z', 'workspace')
    good = dict(logits=p, ldl=21, gate_logits=p, ldg=2, W=3, C=21, lam=1.0, mu=2.0, p_change=p, jump_abs=p, p_flip=p, top_from=p, top_to=p, p_top=p, xi=None, log_z=p,
                workspace=p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sf_track_pairwise_gated(*[a[n] for n in names], None)

    for name in ('logits', 'gate_logits', 'p_change', 'jump_abs', 'p_flip', 'top_from', 'top_to', 'p_top', 'log_z', 'workspace'):
        assert call(**{name: None}) == -1 and b'null pointer' in lib.sf_last_error(), name
    for C in (1, 0, -3, 33, 64):
        assert call(C=C, ldl=128) == -1 and b'classes out of range' in lib.sf_last_error(), C
    assert call(ldl=20) == -1 and b'row stride ldl' in lib.sf_last_error()
    assert call(ldg=1) == -1 and b'gate row stride' in lib.sf_last_error()
    for bad in (-0.5, float('inf'), float('nan')):
        assert call(lam=bad) == -1 and b'lam must be finite' in lib.sf_last_error(), bad
        assert call(mu=bad) == -1 and b'mu must be finite' in lib.sf_last_error(), bad
    assert call(W=-1) == -1 and b'windows' in lib.sf_last_error()
    assert call(W=0) == 0
    assert call(W=0, logits=None, gate_logits=None, p_flip=None, log_z=None, workspace=None) == 0


def test_abi_lists_the_pairwise_entries():
    from synchformer_amd import _lib
    assert _lib.ABI_VERSION == 25 and _lib.load().sf_abi_version() == 25         # additions under v25
    assert len(_lib.SIGNATURES['sf_track_pairwise']) == 14 and len(_lib.SIGNATURES['sf_track_pairwise_gated']) == 18
    for lib in (_lib.load(), _lib.load_ablation()):
        assert hasattr(lib, 'sf_track_pairwise') and hasattr(lib, 'sf_track_pairwise_gated')


def test_tracker_takes_pairwise_flag_and_the_track_keeps_its_fields():
    from synchformer_amd.track import OffsetTrack, OffsetTracker
    p = inspect.signature(OffsetTracker.__init__).parameters
    assert list(p)[-2:] == ['mu', 'pairwise'] and p['pairwise'].default is False
    names = [f.name for f in dataclasses.fields(OffsetTrack)]
    assert names == ['t_sec', 'logits', 'cls_raw', 'conf_raw', 'cls_path', 'conf_path', 'offset_sec_raw', 'offset_sec_path', 'n_segments', 'post', 'cls_post',
                     'conf_post', 'offset_sec_post', 'offset_sec_mean', 'log_z'], names
    tr = OffsetTrack(*range(9))
    assert all(getattr(tr, n) is None for n in ('t_change', 'p_change', 'jump_abs', 'p_change_top', 'change_from_sec', 'change_to_sec', 'p_flip'))
    with pytest.raises(ValueError, match='pairwise=True'):
        tr.changes()
    with pytest.raises(ValueError, match='pairwise=True'):
        tr.expected_changes()


def test_changes_and_expected_changes_of_a_hand_built_track():
    from synchformer_amd.track import OffsetTrack
    tr = OffsetTrack(*([None] * 9))
    tr.t_change = torch.tensor([2.56, 2.88, 3.20, 3.52])
    tr.p_change = torch.tensor([0.05, 0.50, 0.90, 0.25])
    tr.p_change_top = torch.tensor([0.03, 0.40, 0.85, 0.20])
    tr.change_from_sec = torch.tensor([0.0, -0.4, -0.4, 0.6])
    tr.change_to_sec = torch.tensor([0.2, 0.6, 0.6, 0.4])
    ch = tr.changes()
    assert len(ch) == 2 and all(len(row) == 5 and all(isinstance(v, float) for v in row) for row in ch)
    assert ch[0] == pytest.approx((2.88, -0.4, 0.6, 0.50, 0.40), abs=1e-6) and ch[1] == pytest.approx((3.20, -0.4, 0.6, 0.90, 0.85), abs=1e-6)
    assert [row[0] for row in tr.changes(0.85)] == pytest.approx([3.20], abs=1e-6) and tr.changes(0.95) == [] and len(tr.changes(0.0)) == 4
    assert tr.expected_changes() == pytest.approx(1.70, abs=1e-6) and isinstance(tr.expected_changes(), float)
