"""CPU: the host arithmetic of the streaming path - frontend.stream_geometry against recording_geometry, the streamed frame-rate table against
fps_frame_table, and the resampler's context plan against the taps every output reads."""
import math

import numpy as np
import pytest
import torch

from synchformer_amd.frontend import recording_geometry, stream_geometry
from synchformer_amd.ingest import fps_final_slots, fps_frame_table, fps_slot_source, resample_kernel, resample_stream_plan


@pytest.mark.parametrize('hop', [1, 2, 5])
def test_stream_geometry_matches_recording_geometry(hop):
    """Ragged pushes, frames and samples at unrelated paces, some empty on one side: the new segments and windows of the pushes tile those of the prefix without
    gap or overlap, nothing a later segment or window reads is dropped, and what stays held is bounded."""
    rng = np.random.default_rng(hop)
    T = N = seg = win = 0
    f_from = a_from = s_from = 0
    for step in range(200):
        T += int(rng.choice([0, 1, 7, 40, 25]))
        N += int(rng.choice([0, 16000, 333, 5120, 40000]))
        g = stream_geometry(T, N, seg, hop)
        ref = recording_geometry(T, N, hop)
        assert g['n_segments'] == ref['n_segments'] and g['n_windows'] == ref['n_windows']
        assert g['new_segments'] == (seg, ref['n_segments']) and g['new_windows'] == (win, ref['n_windows'])
        for s in range(*g['new_segments']):                                       # every new segment reads only what is still held, and what has arrived
            assert 8 * s >= f_from and 8 * s + 16 <= T and 5120 * s >= a_from and 5120 * s + 10240 <= N
        for w in range(*g['new_windows']):                                        # every new window reads held features only
            assert hop * w >= s_from and hop * w + 14 <= g['n_segments']
        seg, win = ref['n_segments'], ref['n_windows']
        f_from, a_from, s_from = g['frames_from'], g['samples_from'], g['features_from']
        assert f_from >= 0 and a_from >= 0 and seg - s_from <= 13 + hop - 1
        nv, na = max(0, (T - 16) // 8 + 1), max(0, (N - 10240) // 5120 + 1)
        assert T - f_from <= 15 + 8 * (nv - seg) and N - a_from <= 10239 + 5120 * (na - seg)
    assert seg > 100 and win > 10
    with pytest.raises(ValueError):
        stream_geometry(16, 10240, 2)
    assert stream_geometry(144, 92160, 0)['new_windows'] == (0, 4) and stream_geometry(144, 92160, 16)['new_windows'] == (3, 4)


def _streamed_table(pushes, fps):
    """the table IngestStream emits: after each push the final slots, at the end the last one"""
    out, n = [], 0
    for k in pushes:
        n += k
        for j in range(len(out), fps_final_slots(n, fps)):
            i = fps_slot_source(j, fps)
            assert max(0, n - k - 1) <= i < n, (j, i, n, k)                       # inside the push, or the one held frame before it
            out.append(i)
    if n:
        assert len(out) == fps_final_slots(n, fps)
        out.append(min(fps_slot_source(len(out), fps), n - 1))
    return out


@pytest.mark.parametrize('fps', [25, 50, (30000, 1001), 24, 12.5])
def test_streamed_fps_table_equals_offline(fps):
    for n_in in (1, 2, 40, 131):
        ref = fps_frame_table(n_in, fps).tolist()
        assert _streamed_table([1] * n_in, fps) == ref
        rng = np.random.default_rng(n_in)
        pushes, left = [], n_in
        while left:
            pushes.append(min(left, int(rng.choice([0, 1, 2, 7, 30]))))
            left -= pushes[-1]
        assert _streamed_table(pushes, fps) == ref, (n_in, pushes)
    assert _streamed_table([], fps) == [] and fps_final_slots(0, fps) == 0


@pytest.mark.parametrize('rate', [48000, 44100, 22050, 8000, 32000])
def test_resample_plan_covers_every_tap(rate):
    """Output p + n q reads raw samples [q o - width, q o + width + o).  For chunks of 1, 100 and 1000 samples: every output is emitted exactly once, in order;
    when it is emitted all its taps have arrived (or the stream has ended) and lie at or after the chunk's start c0 - or before the recording, where the offline
    call zero-pads too; c0 keeps the polyphase grid (a multiple of o) and never reaches back before what the previous call said it would hold."""
    _, width, o, n = resample_kernel(rate)
    total = 4411
    for chunk in (1, 100, 1000):
        emitted = seen = hold = 0
        while True:
            final = seen >= total
            seen = min(total, seen + chunk) if not final else seen
            c0, k0, k1, new_hold = resample_stream_plan(emitted, seen, o, width, n, final)
            assert c0 % o == 0 and hold <= c0 <= seen and k0 >= 0 and k1 >= k0 and k0 == emitted - n * (c0 // o)
            for k in ([k0, k1 - 1] if k1 > k0 else []):                          # (monotone in k: the first and the last output of the call)
                q = (k + n * (c0 // o)) // n
                lo, hi = q * o - width, q * o + width + o
                assert lo >= c0 or (c0 == 0 and lo < 0), (k, lo, c0)
                assert hi <= seen or final, (k, hi, seen)
            emitted += k1 - k0
            assert new_hold % o == 0 and new_hold <= max(0, (emitted // n) * o - width) and seen - new_hold <= chunk + 2 * (width + o)
            hold = new_hold
            if final:
                break
        assert emitted == math.ceil(n * total / o)


def test_stream_api_exists():
    from synchformer_amd.ingest import IngestStream, RecordingIngest
    from synchformer_amd.track import OffsetStream, OffsetTracker, OffsetUpdate, window_times, window_times64
    assert hasattr(RecordingIngest, 'stream') and hasattr(OffsetTracker, 'stream') and hasattr(IngestStream, 'flush') and hasattr(OffsetStream, 'held')
    assert 'cls_lag' in OffsetUpdate.__dataclass_fields__ and 'offset_sec_tail' in OffsetUpdate.__dataclass_fields__
    day = 270000                                                                  # a day of windows at hop 1: float64 keeps the milliseconds fp32 loses
    t = window_times64(2, 1, first_window=day)
    assert t.dtype == torch.float64 and t[0].item() == (8 * day + 60) / 25 and (t[1] - t[0]).item() == pytest.approx(0.32, abs=1e-9)
    assert torch.equal(window_times64(5).float(), window_times(5))
