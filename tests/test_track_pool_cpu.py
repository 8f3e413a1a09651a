"""CPU: the pool of streams - the ABI table, the descriptor table against the single stream's counts, the launcher's argument checks (no device is
touched) and the host schedule of a pool tick against each feed's own stream_geometry."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_stream_oracle as TS  # noqa: E402


def test_signatures_and_abi():
    from synchformer_amd import _lib
    assert _lib.ABI_VERSION >= 20
    assert len(_lib.SIGNATURES['sf_track_pool_push']) == 28 and len(_lib.SIGNATURES['sf_track_pool_workspace_bytes']) == 3
    assert len(_lib.SIGNATURES['sf_track_stream_push']) == 25                      # the single-stream entry keeps its signature
    for lib in (_lib.load(), _lib.load_ablation()):
        assert lib.sf_abi_version() >= 20 and hasattr(lib, 'sf_track_pool_push') and hasattr(lib, 'sf_track_pool_workspace_bytes')
        for C, n, post in ((21, 1000, 1), (2, 0, 0), (64, 7, 1), (21, 256, 0)):      # the pool's workspace is one stream's over the packed rows
            assert lib.sf_track_pool_workspace_bytes(C, n, post) == lib.sf_track_stream_workspace_bytes(C, n, post)
        assert lib.sf_track_pool_workspace_bytes(1, 4, 0) == -1 and lib.sf_track_pool_workspace_bytes(21, -1, 0) == -1
    import synchformer_amd
    from synchformer_amd.track import OffsetStreamPool
    assert synchformer_amd.OffsetStreamPool is OffsetStreamPool and 'OffsetStreamPool' in synchformer_amd.__all__


def test_plan_equals_the_single_stream_counts():
    """Random (rows, n, final) per entry: every table row carries track_stream_counts' blocks of its stream, the rows / committed blocks / tails lie back to back
    in table order (contiguous, so disjoint), and the totals are the sums.  n = 0, rows = 0, n > lag and lag = 0 are among the cases."""
    from synchformer_amd import ops
    rng = np.random.default_rng(20)
    seen = dict(n0=0, rows0=0, long=0, final_empty=0)
    for lag in (0, 1, 16, 255):
        for trial in range(40):
            k = int(rng.integers(1, 9))
            rows = [int(r) for r in rng.choice([0, 0, 1, lag, lag + 1, 40, 1000], k)]
            counts = [int(c) for c in rng.choice([0, 0, 1, 2, lag + 1, lag + 7, 70], k)]
            final = [bool(f) for f in rng.integers(0, 2, k)]
            slots = [int(s) for s in rng.permutation(12)[:k]]
            plan = ops.track_pool_plan(rows, counts, lag, final, slots)
            t = plan.table
            assert t.dtype == torch.int64 and t.shape == (k, ops.TRACK_POOL_ROW) and t.device.type == 'cpu'
            row0 = commit0 = tail0 = 0
            for i in range(k):
                w0, kc, m = TS.counts(rows[i], counts[i], lag, final[i])
                assert ops.track_stream_counts(rows[i], counts[i], lag, final[i]) == (w0, kc, m) == plan.blocks[i]
                assert t[i].tolist() == [slots[i], rows[i], counts[i], row0, int(final[i]), commit0, tail0, 0], (lag, i, t[i].tolist())
                row0, commit0, tail0 = row0 + counts[i], commit0 + kc, tail0 + m
                seen['n0'] += counts[i] == 0
                seen['rows0'] += rows[i] == 0
                seen['long'] += counts[i] > lag
                seen['final_empty'] += final[i] and counts[i] == 0
            assert (plan.total_rows, plan.total_commit, plan.total_tail) == (row0, commit0, tail0)
    assert all(v > 20 for v in seen.values()), seen
    assert ops.track_pool_plan([3], [2], 1, [False]).table[0, 0].item() == 0        # slots default to the table order
    with pytest.raises(ValueError):
        ops.track_pool_plan([0, 1], [1], 4, [False, False])
    with pytest.raises(ValueError):
        ops.track_pool_plan([0], [-1], 4, [False])


def test_bad_arguments_are_rejected_without_a_device():
    """Every case of the launcher's validation list returns -1 with a message before anything is launched (the pointers are host memory: a launch would fail)."""
    from synchformer_amd import _lib, ops
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    C, lag = 21, 16
    stride = lib.sf_track_stream_bytes(C, lag, 0)
    stride_post = lib.sf_track_stream_bytes(C, lag, 1)
    assert stride > 0 and stride % 16 == 0 and stride_post > stride
    good = ops.track_pool_plan([0, 20, 5], [3, 2, 0], lag, [False, False, True], [4, 2, 0])     # rows 5, commits 2 + 5, tails 3 + 16 + 0
    assert (good.total_rows, good.total_commit, good.total_tail) == (5, 7, 19)

    def push(table=good.table, state=p, stride=stride, n_slots=7, C=C, lag=lag, post=0, n_active=None, logits=p, ldl=None, total=5, lam=1.0, grid=None, raw=p, commit=p,
             post_blk=None, ldp=None, tail=p, log_z=None, table_host=True, table_dev=p, ws=p):
        t = table.contiguous()
        return lib.sf_track_pool_push(state, stride, n_slots, C, lag, post, t.data_ptr() if table_host else None, table_dev, t.shape[0] if n_active is None else n_active,
                                      logits, C if ldl is None else ldl, total, lam, grid, raw, raw, commit, commit, post_blk, C if ldp is None else ldp, post_blk, post_blk,
                                      post_blk, tail, tail, log_z, ws, None)

    def edited(row, col, value):
        t = good.table.clone()
        t[row, col] = value
        return t

    cases = [
        (dict(C=1), b'classes out of range'), (dict(C=65), b'classes out of range'), (dict(lag=256), b'lag = 256'), (dict(lag=-1), b'lag = -1'),
        (dict(lam=-1.0), b'lam must be finite'), (dict(lam=float('nan')), b'lam must be finite'), (dict(lam=float('inf')), b'lam must be finite'),
        (dict(n_active=0), b'n_active = 0'), (dict(n_active=4097), b'n_active = 4097'),
        (dict(table=edited(2, 0, 4)), b'slot 4 named twice'), (dict(table=edited(1, 0, 7)), b'slot 7 outside the 7 slots'), (dict(table=edited(1, 0, -1)), b'outside the 7 slots'),
        (dict(table=edited(1, 3, 2)), b'overlap'), (dict(table=edited(1, 3, 4)), b'outside the 5 rows'), (dict(table=edited(0, 2, 6)), b'outside the 5 rows'),
        (dict(table=edited(0, 3, -1)), b'outside the 5 rows'), (dict(table=edited(0, 2, -1)), b'outside the 5 rows'), (dict(total=4), b'outside the 4 rows'),
        (dict(table=edited(1, 1, -1)), b'rows pushed so far'),
        (dict(table=edited(1, 5, 1)), b'commit0 = 1'), (dict(table=edited(2, 5, 0)), b'commit0 = 0'), (dict(table=edited(1, 6, 0)), b'tail0 = 0'),
        (dict(table=edited(2, 6, 20)), b'tail0 = 20'),
        (dict(state=None), b'null pointer (states or table)'), (dict(table_host=False), b'null pointer (states or table)'), (dict(table_dev=None), b'null pointer (states or table)'),
        (dict(logits=None), b'null pointer (new rows)'), (dict(raw=None), b'null pointer (new rows)'), (dict(ws=None), b'null pointer (new rows)'),
        (dict(commit=None), b'null pointer (committed block)'), (dict(tail=None), b'null pointer (tail)'),
        (dict(ldl=20), b'row stride ldl = 20'), (dict(stride=stride - 16), b'state stride'), (dict(stride=stride + 8), b'state stride'),
        (dict(post=1, stride=stride), b'state stride'),                                                       # a state sized without the posterior
        (dict(post=1, stride=stride_post, grid=p, post_blk=p), b'null log_z'),
        (dict(post=1, stride=stride_post, grid=p, log_z=p), b'posterior block'), (dict(post=1, stride=stride_post, post_blk=p, log_z=p), b'posterior block'),
        (dict(post=1, stride=stride_post, grid=p, post_blk=p, log_z=p, ldp=20), b'ldp = 20'),
        (dict(n_slots=0), b'n_slots = 0'), (dict(total=-1), b'total_rows = -1'),
    ]
    for kw, msg in cases:
        assert push(**kw) == -1 and msg in lib.sf_last_error(), (kw, lib.sf_last_error())
    # a table of only empty, non-final entries on empty streams: nothing to launch, 0 - with every block null
    empty = ops.track_pool_plan([0, 0], [0, 0], lag, [False, False], [1, 5])
    for post in (0, 1):
        assert push(table=empty.table, total=0, logits=None, raw=None, commit=None, tail=None, ws=None, post=post, stride=stride_post) == 0, lib.sf_last_error()
    assert push(table=ops.track_pool_plan([0], [0], lag, [True]).table, total=0, logits=None, raw=None, commit=None, tail=None, ws=None) == 0      # closing an empty stream
    # the host op's own checks
    state = ops.TrackPoolState(torch.zeros(3, stride, dtype=torch.uint8), C, lag, False)
    x = torch.zeros(2, C)
    for slots, counts, final, exc in (([0, 0], [1, 1], (), ValueError), ([3], [2], (), ValueError), ([0], [1], (), ValueError), ([0, 1], [2], (), ValueError),
                                      ([0], [2], (1,), ValueError), ([], [], (), ValueError)):
        with pytest.raises(exc):
            ops.track_pool_push(state, slots, x, counts, 1.0, final=final)
    state.closed[1] = True
    with pytest.raises(RuntimeError, match='closed'):
        ops.track_pool_push(state, [1], x, [2], 1.0)
    state.rows[1] = 9
    state.reopen(1)
    assert state.rows[1] == 0 and not state.closed[1]
    with pytest.raises(RuntimeError, match='lag = 256'):
        ops.track_pool_state(4, 21, 256, False, 'cpu')
    with pytest.raises(ValueError):
        ops.track_pool_state(0, 21, 16, False, 'cpu')


class _Solo:
    """One feed through its own stream, as integers: OffsetStream's host arithmetic (accept, stream_geometry, trim) without tensors."""

    def __init__(self, hop):
        self.hop = hop
        self.n_frames = self.n_samples = self.n_segments = self.f0 = self.a0 = self.s0 = 0
        self.held_feat = 0

    def push(self, nf, na):
        from synchformer_amd.frontend import stream_geometry
        self.n_frames, self.n_samples = self.n_frames + nf, self.n_samples + na
        g = stream_geometry(self.n_frames, self.n_samples, self.n_segments, self.hop)
        (s0, s1), (w0, w1) = g['new_segments'], g['new_windows']
        segs = [(s, 8 * s - self.f0, 5120 * s - self.a0) for s in range(s0, s1)]            # where segment s lies in the held frames / samples
        assert all(flo >= 0 and flo + 16 <= self.n_frames - self.f0 and alo >= 0 and alo + 10240 <= self.n_samples - self.a0 for _, flo, alo in segs)
        self.held_feat += s1 - s0
        wins = [(w, self.hop * w - self.s0) for w in range(w0, w1)]                        # where window w starts in the held features
        assert all(lo >= 0 and lo + 14 <= self.held_feat for _, lo in wins)
        self.held_feat -= g['features_from'] - self.s0
        self.f0, self.a0, self.s0, self.n_segments = g['frames_from'], g['samples_from'], g['features_from'], s1
        return segs, wins, (self.n_frames - self.f0, self.n_samples - self.a0, self.held_feat)


@pytest.mark.parametrize('hop, seg_chunk', [(1, 5), (2, 3), (1, 224)])
def test_pool_schedule_equals_each_feeds_own_geometry(hop, seg_chunk):
    """Three feeds with unrelated ragged pushes (one joins late, one stops early, ticks in which a feed is not named): the staging order of the segments, the
    window rows and the trimmed buffers of every tick equal what each feed's own stream does with the same pushes."""
    from synchformer_amd.track import pool_schedule
    f_runs = [(1, 7, 40, 0, 3, 25), (50, 0, 0, 13, 200, 2), (8, 8, 8, 8, 160, 0, 31)]
    a_runs = [(16000, 0, 333, 40000, 5120, 0, 1), (0, 52000, 5119, 1, 0, 90000), (5120, 5120, 0, 20480, 7, 81920)]
    solo = [_Solo(hop) for _ in range(3)]
    pool = [dict(n_frames=0, n_samples=0, n_segments=0, f0=0, a0=0, s0=0, held_feat=0) for _ in range(3)]
    n_seg_total = n_win_total = 0
    for tick in range(24):
        named = [i for i in range(3) if not (i == 1 and tick < 3) and not (i == 2 and tick >= 15) and (tick + i) % 4 != 3]
        if not named:
            continue
        want_seg, want_win, want_held = [], [], []
        for j, i in enumerate(named):
            nf, na = f_runs[i][tick % len(f_runs[i])], a_runs[i][tick % len(a_runs[i])]
            pool[i]['n_frames'] += nf
            pool[i]['n_samples'] += na
            segs, wins, held = solo[i].push(nf, na)
            want_seg += [(j, s, flo, alo) for s, flo, alo in segs]
            want_win += [(j, w, lo) for w, lo in wins]
            want_held.append(held)
        plan = pool_schedule([pool[i] for i in named], hop, seg_chunk, win_chunk=4)
        assert plan['segments'] == want_seg and plan['windows'] == want_win, (tick, plan['segments'], want_seg)
        assert plan['counts'] == [sum(1 for k, _, _ in want_win if k == j) for j in range(len(named))]
        for name, size, items in (('groups', seg_chunk, want_seg), ('passes', 4, want_win)):       # launch groups: consecutive, full but the last, whatever the feed
            ranges = plan[name]
            assert [b - a for a, b in ranges] == [size] * (len(items) // size) + ([len(items) % size] if len(items) % size else [])
            assert [a for a, _ in ranges] == [size * k for k in range(len(ranges))]
        for j, i in enumerate(named):                                                    # the trims: what the pool's feed does with its geometry
            f, (ff, sf, ft), g = pool[i], plan['trims'][j], plan['geometry'][j]
            f['held_feat'] += g['new_segments'][1] - g['new_segments'][0]
            f['held_feat'] -= ft - f['s0']
            f['f0'], f['a0'], f['s0'], f['n_segments'] = ff, sf, ft, g['new_segments'][1]
            assert (f['n_frames'] - f['f0'], f['n_samples'] - f['a0'], f['held_feat']) == want_held[j]
            assert f['held_feat'] <= 13 + hop - 1
        n_seg_total += len(want_seg)
        n_win_total += len(want_win)
    assert n_seg_total >= 40 and n_win_total >= 10 and all(s.n_segments >= 14 for s in solo), (n_seg_total, n_win_total)
    assert len({s.n_segments for s in solo}) == 3                                        # the feeds are at different places
