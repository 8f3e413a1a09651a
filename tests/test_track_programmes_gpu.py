"""GPU, end to end: several audio programmes of one recording against one pass of the picture.  The fixture geometry of tests/test_track_stream_gpu.py
(144 frames of 256 x 256, 92160 samples at 16 kHz equivalent: 17 segments, 4 windows) with 4 channels of 48 kHz int16 and the programmes [0, (2, 3), {1: 1.0}]:
the shared-picture entry points against the single-programme ones on each programme's channels alone, bit for bit - the engine runs the un-fused schedule
(seg_chunk = 5), on which a segment's features do not depend on its place in a launch."""
import dataclasses
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_track_stream_gpu import N_REC, N_SEG, N_WIN, T_REC, _check_stream_against, _ragged  # noqa: E402

pytestmark = pytest.mark.gpu

PROGRAMMES = [0, (2, 3), {1: 1.0}]
CHANNELS = [slice(0, 1), slice(2, 4), slice(1, 2)]                               # the rows of the raw wave each programme is made of
LAG = 3


@pytest.fixture(scope='module')
def rec(gpu):
    """One engine (synthetic weights, seg_chunk = 5), one recording as 256 x 256 raw frames with 4 channels of 48 kHz int16 - each a differently seeded
    synth.make_wave - and, per programme, the reference: track_raw through a default ingest on that programme's channels alone.  Computed once, read-only."""
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.ingest import RecordingIngest
    from synchformer_amd.track import OffsetTracker
    eng = SynchformerEngine(synth.make_state_dict(1337), gpu, seg_chunk=5)
    mel = MelFrontend(gpu)
    raw = torch.randint(0, 256, (T_REC, 3, 256, 256), generator=torch.Generator().manual_seed(99), dtype=torch.uint8)
    wave = torch.stack([synth.make_wave(1, 1, 200 + c, n=3 * N_REC).reshape(3 * N_REC) for c in range(4)])
    wave = (wave / wave.abs().max() * 30000).round().to(torch.int16)            # (4, 276480) planar
    tracker = OffsetTracker(eng, mel, lam=0.5, posterior=True)
    ing = RecordingIngest(gpu, 25, (256, 256), 48000, audio_channels=4, programmes=PROGRAMMES)
    ing_il = RecordingIngest(gpu, 25, (256, 256), 48000, audio_channels=4, audio_interleaved=True, programmes=PROGRAMMES)
    plain = RecordingIngest(gpu, 25, (256, 256), 48000)
    raw_d = raw.to(gpu)
    refs = [tracker.track_raw(raw_d, wave[rows], plain) for rows in CHANNELS]
    torch.cuda.synchronize()
    assert all(r.logits.shape == (N_WIN, 21) and r.n_segments == N_SEG for r in refs)
    return dict(eng=eng, mel=mel, tracker=tracker, raw=raw, raw_d=raw_d, wave=wave, wave_il=wave.t().contiguous(), ing=ing, ing_il=ing_il, plain=plain, refs=refs)


def _same(a, b, what):
    """every field of two OffsetTrack / OffsetUpdate: equal bits (tensors), equal values (the rest)"""
    for f in dataclasses.fields(a):
        u, v = getattr(a, f.name), getattr(b, f.name)
        if isinstance(u, torch.Tensor):
            assert isinstance(v, torch.Tensor) and u.dtype == v.dtype and u.shape == v.shape and torch.equal(u, v), (what, f.name)
        else:
            assert u == v, (what, f.name, u, v)


def test_waves_are_the_single_programme_waves(gpu, rec):
    waves = rec['ing'].waves(rec['wave'])
    assert waves.shape == (3, N_REC)
    for p, rows in enumerate(CHANNELS):
        assert torch.equal(waves[p], rec['plain'].wave(rec['wave'][rows])), p
    assert torch.equal(rec['ing_il'].waves(rec['wave_il']), waves)


def test_banks_and_windows_equal_the_single_programme_calls(gpu, rec):
    eng, mel, ing = rec['eng'], rec['mel'], rec['ing']
    waves = ing.waves(rec['wave'])
    frame_fn = lambda f0, f1: ing.frames(rec['raw_d'], f0, f1)                   # noqa: E731
    vbank, abanks = eng.extract_recording_programmes_from(frame_fn, ing.n_frames(T_REC), waves, mel)
    assert vbank.shape == (N_SEG, 8, 768) and abanks.shape == (3, N_SEG, 6, 768)
    logits = eng.sync_windows_programmes(vbank, abanks)
    assert logits.shape == (3, N_WIN, 21)
    for p in range(3):
        vb, ab = eng.extract_recording_from(frame_fn, ing.n_frames(T_REC), waves[p], mel)
        assert torch.equal(vbank, vb) and torch.equal(abanks[p], ab), p
        assert torch.equal(logits[p], eng.sync_windows(vb, ab)), p
    v2, a2 = eng.extract_segments_programmes_from(frame_fn, waves, mel, 3, 7, seg_chunk=2)       # the last chunk: 1 segment x 3 programmes in groups of 2, one straddling two programmes
    assert torch.equal(v2, vbank[3:10]) and torch.equal(a2, abanks[:, 3:10])
    with pytest.raises(ValueError, match='one window'):
        eng.extract_recording_programmes_from(frame_fn, 100, waves, mel)
    with pytest.raises(ValueError):
        eng.sync_windows_programmes(vbank, abanks[0])


def test_track_raw_programmes_equals_track_raw_per_programme(gpu, rec):
    for ing, wave in ((rec['ing'], rec['wave']), (rec['ing_il'], rec['wave_il'].to(gpu))):
        tracks = rec['tracker'].track_raw_programmes(rec['raw'], wave, ing)
        assert len(tracks) == 3
        for p, (t, ref) in enumerate(zip(tracks, rec['refs'])):
            assert t.post is not None and t.log_z is not None
            _same(t, ref, f'programme {p}')
    assert not torch.equal(tracks[0].logits, tracks[1].logits) and not torch.equal(tracks[0].logits, tracks[2].logits)   # not every programme from one channel


def test_programme_stream_equals_plain_streams(gpu, rec):
    """Ragged pushes: every programme's updates equal, update for update and field for field, a plain OffsetStream fed that programme's channels in the same
    pieces; the concatenation passes test_track_stream_gpu's comparison against the offline track; held <= held_bound after every push; a push after flush raises."""
    from synchformer_amd.track import ProgrammeStream
    tracker = rec['tracker']
    pieces = _ragged(T_REC, 3 * N_REC, a_runs=(48000, 0, 1001, 120000, 15360, 0, 1))
    assert any(f0 == f1 and a1 > a0 for f0, f1, a0, a1 in pieces) and any(a0 == a1 and f1 > f0 for f0, f1, a0, a1 in pieces)
    stream = tracker.stream(lag=LAG, ingest=rec['ing_il'])
    assert isinstance(stream, ProgrammeStream) and stream.P == 3
    plains = [tracker.stream(lag=LAG, ingest=rec['plain']) for _ in CHANNELS]
    ups, refs = [], [[] for _ in CHANNELS]
    for f0, f1, a0, a1 in pieces:
        ups.append(stream.push(rec['raw'][f0:f1], rec['wave_il'][a0:a1]))
        held, bound = stream.held, stream.held_bound
        assert set(bound) == {'frames', 'samples', 'segments', 'audio_segments', 'state_bytes'}
        assert all(held[k] <= bound[k] for k in bound), (held, bound)
        for p, rows in enumerate(CHANNELS):
            refs[p].append(plains[p].push(rec['raw'][f0:f1], rec['wave'][rows, a0:a1]))
            assert bound['samples'] == 3 * plains[p].held_bound['samples'] and bound['frames'] == plains[p].held_bound['frames']
    ups.append(stream.flush())
    for p in range(3):
        refs[p].append(plains[p].flush())
    torch.cuda.synchronize()
    assert stream.held['state_bytes'] == 3 * plains[0].held['state_bytes'] and stream.n_segments == N_SEG and stream.n_windows == N_WIN
    with pytest.raises(RuntimeError, match='closed'):
        stream.push(rec['raw'][:0], rec['wave_il'][:0])
    with pytest.raises(RuntimeError, match='closed'):
        stream.flush()
    for p in range(3):
        mine = [u[p] for u in ups]
        assert all(len(u) == 3 for u in ups)
        for i, (a, b) in enumerate(zip(mine, refs[p])):
            _same(a, b, f'programme {p}, push {i}')
        _check_stream_against(mine, rec['refs'][p], LAG)


def test_programmes_are_refused_where_one_wave_is_expected(gpu, rec):
    tracker = rec['tracker']
    with pytest.raises(ValueError, match='track_raw_programmes'):
        tracker.track_raw(rec['raw'], rec['wave'], rec['ing'])
    with pytest.raises(ValueError, match='programmes'):
        tracker.pool(2, lag=LAG).open(rec['ing'])
    with pytest.raises(ValueError, match='track_raw'):
        tracker.track_raw_programmes(rec['raw'], rec['wave'][:2], rec['plain'])
    pool = tracker.pool(2, lag=LAG)
    assert pool.open(rec['plain']).slot == 0                                     # a plain ingest is still served
