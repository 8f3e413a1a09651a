"""CPU: the gated fixed-lag read-out (ABI v25) - the float64 oracle against itself (definition vs carried state, max-marginals vs brute force, the
criterion's power on the GPU tests' inputs), the ABI table, the launchers' argument checks (no device is touched), the state's documented layout and the
`gated=` keyword of OffsetTracker.stream / .pool."""
import ctypes
import itertools
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_gated_oracle as TG  # noqa: E402
import track_gated_stream_oracle as GS  # noqa: E402
import track_stream_oracle as TS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('sf_track_stream_gated_bytes', 'sf_track_stream_gated_workspace_bytes', 'sf_track_stream_push_gated', 'sf_track_pool_gated_workspace_bytes',
       'sf_track_pool_push_gated')


def _pushes(chunks):
    return [(n, False) for n in chunks] + [(0, True)]


@pytest.mark.parametrize('C, lag', [(2, 0), (2, 3), (5, 1), (5, 8), (21, 7)])
def test_carried_state_equals_the_definition(C, lag):
    """One offline gated read-out per prefix (the definition, literally) against the incremental statement with a 2C-wide carried state and rings of `lag` rows.
    The two statements do the same float64 operations in the same order (no renormalisation in either), so ties break alike and indices compare exactly."""
    rng = np.random.default_rng(100 * C + lag)
    W = 23
    l, z = rng.integers(-8, 9, (W, C)) / 4.0, rng.integers(-8, 9, (W, 2)) / 4.0
    grid = np.linspace(-2, 2, C)
    for lam, mu in ((0.0, 0.0), (0.5, 2.0), (2.0, 0.25)):
        pre = GS.prefix_readouts(l, z, lam, mu, grid)
        for name in TS.CHUNKINGS:
            pushes = _pushes(TS.chunking(name, W, lag))
            want = GS.by_definition(l, z, lam, mu, lag, pushes, grid, pre)
            orc, row = GS.GatedStreamOracle(C, lam, mu, lag, grid), 0
            for (n, final), d in zip(pushes, want):
                got = orc.push(l[row:row + n], z[row:row + n], final)
                row += n
                assert got['w0'] == d['w0']
                for k in ('cls_raw', 'cls_lag', 'sync_lag', 'cls_tail', 'sync_tail'):
                    assert np.array_equal(got[k], d[k]), (name, lam, mu, k, row)
                for k in ('conf_raw', 'sync_raw', 'conf_lag', 'conf_tail', 'post_lag', 'p_sync_lag', 'conf_post_lag', 'offset_mean_lag'):
                    assert np.allclose(got[k], d[k], rtol=0, atol=1e-12), (name, lam, mu, k, row)
                assert abs(got['log_z'] - d['log_z']) <= 1e-10
                assert orc.held() <= lag                                            # the carried rings never grow
    # lag >= W: nothing is committed before the flush, which gives the offline read-outs
    pushes = _pushes([W])
    last = GS.by_definition(l, z, 0.5, 2.0, W, pushes, grid)[-1]
    off, post = TG.viterbi(l, z, 0.5, 2.0), TG.posterior(l, z, 0.5, 2.0, grid)
    assert last['w0'] == 0 and np.array_equal(last['cls_lag'], off['cls_path']) and np.array_equal(last['sync_lag'], off['sync_path'])
    assert np.array_equal(last['post_lag'], post['post']) and np.array_equal(last['p_sync_lag'], post['p_sync'])


@pytest.mark.parametrize('C, W', [(2, 1), (2, 2), (2, 5), (2, 6), (3, 4), (4, 4)])
def test_max_marginals_against_brute_force(C, W):
    """M[w, j] = the best score of any path through state j at row w, against every one of the (2C)^W <= 4096 paths."""
    assert (2 * C) ** W <= 4096
    l, z = GS.stream_inputs(7 * C + W, W, C)
    for lam, mu in ((0.0, 0.0), (0.5, 2.0), (2.0, 16.0)):
        M = GS.max_marginals(l, z, lam, mu)
        brute = np.full((W, 2 * C), -np.inf)
        for path in itertools.product(range(2 * C), repeat=W):
            s = TG.path_score(l, z, lam, mu, np.array(path))
            for w, j in enumerate(path):
                brute[w, j] = max(brute[w, j], s)
        assert np.abs(M - brute).max() <= 1e-10
        assert abs(M.max(1) - TG.brute_force(l, z, lam, mu)['best']).max() <= 1e-10       # every row's maximum is the optimum
        vit = TG.viterbi(l, z, lam, mu)
        assert all(GS.gap(M, w, vit['cls_path'][w], vit['sync_path'][w]) <= 1e-10 for w in range(W))


@pytest.mark.parametrize('lam', [0.5, 1.0, 2.0])
def test_the_criterion_rejects_plausible_wrong_read_outs(lam):
    """On the random input of the GPU tests (C = 21, W = 70): the float64 read-out at `lag` passes the max-marginal bound in every window; the offline path, the
    read-out at lag + 1 and the per-row argmax each violate it somewhere - so a kernel returning one of those cannot pass."""
    l, z = GS.stream_inputs(2100, 70, 21)
    pre, mm = GS.prefix_readouts(l, z, lam, 2.0), GS.prefix_max_marginals(l, z, lam, 2.0)
    for lag in (0, 1, 7, 8, 9):
        bad = GS.discriminations(l, z, lam, 2.0, lag, pre, mm)
        assert bad['oracle'] == 0 and bad['offline'] >= 1 and bad['lag+1'] >= 1 and bad['argmax'] >= 1, (lam, lag, bad)


def test_gap_scenario_margins():
    """The decisions of TG.gap_scenario under every lag of the GPU test are at least half a logit clear: fp32 cannot flip them, indices compare exactly."""
    l, z = TG.gap_scenario()
    worst = np.inf
    for lam in (0.5, 1.0):
        for mu in (0.0, 2.0, 16.0):
            for M in GS.prefix_max_marginals(l, z, lam, mu):
                top = np.sort(M, axis=1)
                worst = min(worst, float((top[:, -1] - top[:, -2]).min()))
    assert worst >= 0.5 - 1e-9, worst


def test_counts_are_the_ungated_ones():
    from synchformer_amd import ops
    for rows, n, lag, final in itertools.product((0, 1, 9, 300), (0, 1, 8, 70), (0, 1, 8, 255), (False, True)):
        assert ops.track_stream_counts(rows, n, lag, final) == GS.counts(rows, n, lag, final) == TS.counts(rows, n, lag, final)


def test_header_signatures_and_exports_agree():
    from synchformer_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'synchformer_hip.h')).read()
    assert int(re.search(r'#define SF_ABI_VERSION (\d+)', header).group(1)) == 25 == _lib.ABI_VERSION
    for name in NEW:
        decl = re.search(r'^int ' + name + r'\((.*?)\);', header, re.S | re.M)
        assert decl, name
        assert len(decl.group(1).split(',')) == len(_lib.SIGNATURES[name]), name
    assert len(_lib.SIGNATURES['sf_track_stream_push_gated']) == len(_lib.SIGNATURES['sf_track_stream_push']) + 7
    assert len(_lib.SIGNATURES['sf_track_pool_push_gated']) == len(_lib.SIGNATURES['sf_track_pool_push']) + 7
    for lib in (_lib.load(), _lib.load_ablation()):
        assert lib.sf_abi_version() == 25 and all(hasattr(lib, name) for name in NEW)
    assert ops.TrackGatedStreamOut._fields == ops.TrackStreamOut._fields + ('sync_raw', 'sync_lag', 'sync_tail', 'p_sync_lag')


def _layout_bytes(C: int, lag: int, posterior: bool) -> int:
    """DESIGN 3.21's layout, restated: header 16, s 256, [a 256], logits ring, gate ring, [a ring], back pointer ring; rounded up to 16."""
    n = 16 + 64 * 4 + (64 * 4 if posterior else 0) + lag * C * 4 + lag * 2 * 4 + (lag * 2 * C * 4 if posterior else 0) + lag * 2 * C
    return (n + 15) // 16 * 16


def test_state_bytes_are_the_documented_layout():
    from synchformer_amd import _lib
    lib = _lib.load()
    for C, lag, post in itertools.product((2, 3, 21, 32), (0, 1, 7, 16, 255), (0, 1)):
        got = lib.sf_track_stream_gated_bytes(C, lag, post)
        assert got == _layout_bytes(C, lag, bool(post)) and got % 16 == 0, (C, lag, post, got)
    assert lib.sf_track_stream_gated_bytes(21, 16, 1) > lib.sf_track_stream_bytes(21, 16, 1)
    for C, n, post in ((21, 1000, 1), (2, 0, 0), (32, 7, 1), (21, 1 << 20, 1)):
        want = ((n * 2 * C * 4 if post else 0) + n * 4 + n * 2 * C + 15) // 16 * 16
        assert lib.sf_track_stream_gated_workspace_bytes(C, n, post) == want == lib.sf_track_pool_gated_workspace_bytes(C, n, post)
    for fn in (lib.sf_track_stream_gated_bytes, lib.sf_track_stream_gated_workspace_bytes, lib.sf_track_pool_gated_workspace_bytes):
        assert fn(33, 4, 0) == -1 and b'classes out of range' in lib.sf_last_error()
        assert fn(1, 4, 0) == -1
    assert lib.sf_track_stream_gated_bytes(21, 256, 0) == -1 and b'lag = 256' in lib.sf_last_error()
    assert lib.sf_track_stream_gated_workspace_bytes(21, (1 << 20) + 1, 0) == -1 and lib.sf_track_stream_gated_workspace_bytes(21, -1, 0) == -1


def _ptr(buf):
    p = ctypes.addressof(buf)
    return p + (-p) % 16


STREAM_ARGS = ('state', 'C', 'lag', 'posterior', 'rows_done', 'logits', 'ldl', 'gate', 'ldg', 'n', 'lam', 'mu', 'grid', 'final', 'cls_raw', 'conf_raw', 'sync_raw',
               'cls_lag', 'sync_lag', 'conf_lag', 'post_lag', 'ldp', 'p_sync_lag', 'cls_post_lag', 'conf_post_lag', 'offset_mean_lag', 'cls_tail', 'sync_tail',
               'conf_tail', 'log_z', 'workspace')


def test_stream_push_refusals_without_a_device():
    """Every refusal returns -1 with a message before anything is launched (the pointers are host memory: a launch would fail)."""
    from synchformer_amd import _lib
    lib = _lib.load()
    p = _ptr(ctypes.create_string_buffer(256))
    good = dict(C=21, lag=4, posterior=0, rows_done=10, ldl=21, ldg=2, n=6, lam=1.0, mu=2.0, final=0, ldp=21)      # commits 6, tail 4

    def call(**kw):
        a = dict({n: p for n in STREAM_ARGS if n not in good}, **good)
        a.update(kw)
        return lib.sf_track_stream_push_gated(*[a[n] for n in STREAM_ARGS], None)

    cases = [(dict(C=33), b'classes out of range'), (dict(C=1), b'classes out of range'), (dict(C=64), b'classes out of range'), (dict(lag=256), b'lag = 256'),
             (dict(lag=-1), b'lag = -1'), (dict(n=-1), b'n = -1'), (dict(n=(1 << 20) + 1), b'rows in one push'), (dict(rows_done=-1), b'rows pushed so far'),
             (dict(ldl=20), b'row stride ldl'), (dict(ldg=1), b'gate row stride'), (dict(state=None), b'null state')]
    for bad in (-0.5, float('inf'), float('nan')):
        cases += [(dict(lam=bad), b'lam must be finite'), (dict(mu=bad), b'mu must be finite')]
    cases += [(dict(**{n: None}), b'null pointer (new rows)') for n in ('logits', 'gate', 'cls_raw', 'conf_raw', 'sync_raw', 'workspace')]
    cases += [(dict(**{n: None}), b'null pointer (committed block)') for n in ('cls_lag', 'sync_lag', 'conf_lag')]
    cases += [(dict(**{n: None}), b'null pointer (tail)') for n in ('cls_tail', 'sync_tail', 'conf_tail')]
    cases += [(dict(posterior=1, log_z=None), b'null log_z'), (dict(posterior=1, ldp=20), b'ldp = 20')]
    cases += [(dict(posterior=1, **{n: None}), b'posterior block') for n in ('grid', 'post_lag', 'p_sync_lag', 'cls_post_lag', 'conf_post_lag', 'offset_mean_lag')]
    for kw, msg in cases:
        assert call(**kw) == -1 and msg in lib.sf_last_error(), (kw, lib.sf_last_error())
    # an empty push onto an empty stream: nothing to do, no buffers needed
    assert call(rows_done=0, n=0, **{n: None for n in STREAM_ARGS if n not in good and n != 'state'}) == 0, lib.sf_last_error()
    assert call(rows_done=0, n=0, final=1, ldl=0, ldg=0) == 0                    # (the strides are not looked at without rows)


def test_pool_push_refusals_without_a_device():
    from synchformer_amd import _lib, ops
    lib = _lib.load()
    p = _ptr(ctypes.create_string_buffer(256))
    C, lag = 21, 16
    stride, stride_post = lib.sf_track_stream_gated_bytes(C, lag, 0), lib.sf_track_stream_gated_bytes(C, lag, 1)
    good = ops.track_pool_plan([0, 20, 5], [3, 2, 0], lag, [False, False, True], [4, 2, 0])     # rows 5, commits 2 + 5, tails 3 + 16 + 0

    def push(table=good.table, state=p, stride=stride, n_slots=7, C=C, lag=lag, post=0, n_active=None, logits=p, ldl=None, gate=p, ldg=2, total=5, lam=1.0, mu=2.0,
             grid=None, raw=p, sync_raw=p, commit=p, sync_lag=p, post_blk=None, p_sync=None, ldp=None, tail=p, sync_tail=p, log_z=None, table_host=True, table_dev=p, ws=p):
        t = table.contiguous()
        return lib.sf_track_pool_push_gated(state, stride, n_slots, C, lag, post, t.data_ptr() if table_host else None, table_dev,
                                            t.shape[0] if n_active is None else n_active, logits, C if ldl is None else ldl, gate, ldg, total, lam, mu, grid, raw, raw,
                                            sync_raw, commit, sync_lag, commit, post_blk, C if ldp is None else ldp, p_sync, post_blk, post_blk, post_blk, tail, sync_tail,
                                            tail, log_z, ws, None)

    def edited(row, col, value):
        t = good.table.clone()
        t[row, col] = value
        return t

    cases = [
        (dict(C=1), b'classes out of range'), (dict(C=33), b'classes out of range'), (dict(lag=256), b'lag = 256'), (dict(lam=-1.0), b'lam must be finite'),
        (dict(mu=-1.0), b'mu must be finite'), (dict(mu=float('nan')), b'mu must be finite'), (dict(n_active=0), b'n_active = 0'), (dict(n_active=4097), b'n_active = 4097'),
        (dict(table=edited(2, 0, 4)), b'slot 4 named twice'), (dict(table=edited(1, 0, 7)), b'slot 7 outside the 7 slots'),
        (dict(table=edited(1, 3, 2)), b'overlap'), (dict(table=edited(1, 3, 4)), b'outside the 5 rows'), (dict(total=4), b'outside the 4 rows'),
        (dict(table=edited(1, 1, -1)), b'rows pushed so far'),
        (dict(table=edited(1, 5, 1)), b'commit0 = 1'), (dict(table=edited(2, 5, 0)), b'commit0 = 0'), (dict(table=edited(1, 6, 0)), b'tail0 = 0'),
        (dict(table=edited(2, 6, 20)), b'tail0 = 20'),
        (dict(state=None), b'null pointer (states or table)'), (dict(table_host=False), b'null pointer (states or table)'), (dict(table_dev=None), b'null pointer (states or table)'),
        (dict(logits=None), b'null pointer (new rows)'), (dict(gate=None), b'null pointer (new rows)'), (dict(raw=None), b'null pointer (new rows)'),
        (dict(sync_raw=None), b'null pointer (new rows)'), (dict(ws=None), b'null pointer (new rows)'),
        (dict(commit=None), b'null pointer (committed block)'), (dict(sync_lag=None), b'null pointer (committed block)'),
        (dict(tail=None), b'null pointer (tail)'), (dict(sync_tail=None), b'null pointer (tail)'),
        (dict(ldl=20), b'row stride ldl = 20'), (dict(ldg=1), b'gate row stride ldg = 1'), (dict(stride=stride - 16), b'state stride'), (dict(stride=stride + 8), b'state stride'),
        (dict(stride=lib.sf_track_stream_bytes(C, lag, 0)), b'state stride'),                                  # an ungated state is too small
        (dict(post=1, stride=stride), b'state stride'),
        (dict(post=1, stride=stride_post, grid=p, post_blk=p, p_sync=p), b'null log_z'),
        (dict(post=1, stride=stride_post, grid=p, post_blk=p, log_z=p), b'posterior block'), (dict(post=1, stride=stride_post, post_blk=p, p_sync=p, log_z=p), b'posterior block'),
        (dict(post=1, stride=stride_post, grid=p, post_blk=p, p_sync=p, log_z=p, ldp=20), b'ldp = 20'),
        (dict(n_slots=0), b'n_slots = 0'), (dict(total=-1), b'total_rows = -1'),
    ]
    for kw, msg in cases:
        assert push(**kw) == -1 and msg in lib.sf_last_error(), (kw, lib.sf_last_error())
    empty = ops.track_pool_plan([0, 0], [0, 0], lag, [False, False], [1, 5])
    for post in (0, 1):
        assert push(table=empty.table, total=0, logits=None, gate=None, raw=None, sync_raw=None, commit=None, sync_lag=None, tail=None, sync_tail=None, ws=None, post=post,
                    stride=stride_post) == 0, lib.sf_last_error()


def test_a_state_knows_its_kind():
    from synchformer_amd import ops
    C, lag = 5, 3
    plain, gated = ops.track_stream_state(C, lag, False, 'cpu'), ops.track_stream_state_gated(C, lag, False, 'cpu')
    assert (plain.gated, gated.gated) == (False, True) and gated.buf.numel() == _layout_bytes(C, lag, False) and not gated.buf.any()
    pool, gpool = ops.track_pool_state(2, C, lag, True, 'cpu'), ops.track_pool_state_gated(2, C, lag, True, 'cpu')
    assert (pool.gated, gpool.gated) == (False, True) and gpool.buf.shape == (2, _layout_bytes(C, lag, True))
    x, z = torch.zeros(2, C), torch.zeros(2, 2)
    with pytest.raises(TypeError, match='not gated'):
        ops.track_stream_push_gated(plain, x, z, 1.0, 2.0)
    with pytest.raises(TypeError, match='is gated'):
        ops.track_stream_push(gated, x, 1.0)
    with pytest.raises(TypeError, match='not gated'):
        ops.track_pool_push_gated(pool, [0], x, z, [2], 1.0, 2.0)
    with pytest.raises(TypeError, match='is gated'):
        ops.track_pool_push(gpool, [0], x, [2], 1.0)
    with pytest.raises(AssertionError, match='gate logits'):
        ops.track_stream_push_gated(gated, x, torch.zeros(3, 2), 1.0, 2.0)
    with pytest.raises(RuntimeError, match='classes out of range'):
        ops.track_stream_state_gated(33, lag, False, 'cpu')
    with pytest.raises(ValueError, match='n_slots'):
        ops.track_pool_state_gated(0, C, lag, False, 'cpu')


def _fake(n_out, n_window, dev='cpu'):
    return SimpleNamespace(n_out=n_out, n_window=n_window, dev=torch.device(dev), seg_chunk=5)


def test_the_gated_keyword():
    """tracker with a gate: True -> the gated stream / pool, False -> the ungated one, None -> NotImplementedError that keeps DESIGN 3.20 and names the two choices;
    tracker without a gate: True -> ValueError, None / False -> what it gave before."""
    from synchformer_amd import ops
    from synchformer_amd.track import OffsetStream, OffsetStreamPool, OffsetTracker, OffsetUpdate
    eng = _fake(21, 14)
    with_gate, without = OffsetTracker(eng, None, gate=_fake(2, 13), posterior=True), OffsetTracker(eng, None, posterior=True)
    for make in (lambda tr, **kw: tr.stream(lag=7, **kw), lambda tr, **kw: tr.pool(4, lag=7, **kw)):
        g = make(with_gate, gated=True)
        assert g.gated and isinstance(g.state, (ops.TrackGatedStreamState, ops.TrackGatedPoolState))
        assert g.state.buf.shape[-1] == _layout_bytes(21, 7, True)
        for plain in (make(with_gate, gated=False), make(without), make(without, gated=False), make(without, gated=None)):
            assert not plain.gated and not plain.state.gated and plain.state.buf.shape[-1] == ops.track_stream_state(21, 7, True, 'cpu').buf.numel()
        with pytest.raises(NotImplementedError, match='3.20') as err:
            make(with_gate)
        assert 'gated=True' in str(err.value) and 'gated=False' in str(err.value) and '3.21' in str(err.value)
        with pytest.raises(NotImplementedError, match='3.20'):
            make(with_gate, gated=None)
        with pytest.raises(ValueError, match='has no gate'):
            make(without, gated=True)
    s = with_gate.stream(lag=7, gated=True)
    assert isinstance(s, OffsetStream) and s.held['state_bytes'] == s.held_bound['state_bytes'] == _layout_bytes(21, 7, True)
    p = with_gate.pool(3, lag=7, gated=True)
    assert isinstance(p, OffsetStreamPool) and p.open().held['state_bytes'] == _layout_bytes(21, 7, True)
    with pytest.raises(ValueError, match='needs a tracker with a gate'):
        OffsetStreamPool(without, 2, gated=True)
    # the gate's outputs are optional attributes of OffsetUpdate, not dataclass fields
    import dataclasses
    names = [f.name for f in dataclasses.fields(OffsetUpdate)]
    assert not {'gate_logits', 'sync_raw', 'sync_lag', 'sync_tail', 'p_sync_lag'} & set(names) and names[0] == 'w_new' and names[-1] == 'log_z'
    assert all(getattr(OffsetUpdate, n) is None for n in ('gate_logits', 'sync_raw', 'sync_lag', 'sync_tail', 'p_sync_lag'))
