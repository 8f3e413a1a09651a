"""GPU: the ingest stage.  sf_ingest_video against torch's own CPU F.interpolate on float64, sf_resample_wave against the float64 restatement of
torchaudio's resampler (tests/ingest_oracle.py), the output bytes of both video launchers against the digests recorded in tests/golden/ingest_digests.json, and
OffsetTracker.track_raw end to end on the identity case (bit-equal to track) and on a 50 fps / 48 kHz case."""
import functools
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import ingest_oracle as R  # noqa: E402
import make_ingest_digests as D  # noqa: E402

pytestmark = pytest.mark.gpu

TABLE = R.TABLE
VIDEO_SIZES = [(270, 480), (360, 202), (144, 176), (540, 960), (301, 517), (1080, 608)]


@functools.lru_cache(maxsize=None)
def _video_case(H, W, side=256):
    """(raw planar uint8 (5, 3, H, W), oracle uint8 (5, 3, 224, 224) of the 5 SOURCE frames, crop origin) - computed once per size, read-only."""
    from synchformer_amd.ingest import resized_dims
    raw = R.random_frames(5, H, W, H * 10000 + W + side)
    Hr, Wr = resized_dims(H, W, side)
    y0, x0 = int(round((Hr - 224) / 2.)), int(round((Wr - 224) / 2.))
    ref = R.resize64(raw, (Hr, Wr))[..., y0:y0 + 224, x0:x0 + 224].round().clamp(0, 255).to(torch.uint8)
    return raw, ref


@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('H, W', VIDEO_SIZES)
def test_ingest_video_matches_interpolate(gpu, H, W, channels_last):
    from synchformer_amd.ingest import RecordingIngest
    raw, ref = _video_case(H, W)
    ing = RecordingIngest(gpu, 25, (H, W), 16000, channels_last=channels_last)
    ing._tables = {5: torch.tensor(TABLE, dtype=torch.int32)}                    # the frame pick under test: a repeat and a skip
    assert (ing.taps_y, ing.taps_x) == {(270, 480): (7, 7), (360, 202): (5, 5), (144, 176): (5, 5), (540, 960): (11, 11), (301, 517): (7, 7),
                                        (1080, 608): (11, 11)}[(H, W)]
    src = raw.permute(0, 2, 3, 1).contiguous() if channels_last else raw
    for where in (src.to(gpu), src):                                             # on the device, and uploaded from the host (only frames [0, 5) -> all of them)
        got = ing.frames(where, 0, 5)
        torch.cuda.synchronize()
        R.check_pixels(got, ref[TABLE], f'{H} x {W} taps {ing.taps_y} x {ing.taps_x} {"channels-last" if channels_last else "planar"}')
    # a slice of the output frames: [2, 5) reads source frames 2 .. 4 only
    part = ing.frames(src, 2, 5)
    assert torch.equal(part, got[2:5])


@pytest.mark.parametrize('H, W, Wr, taps_y, taps_x, rows', [(2160, 260, 256, 35, 7, 8), (260, 2160, 256, 7, 35, 8), (260, 3400, 400, 7, 35, 4), (1040, 1030, 256, 19, 19, 8)])
def test_ingest_video_many_taps(gpu, H, W, Wr, taps_y, taps_x, rows):
    """The launcher's range and its chunking, on the smallest inputs that reach them: 35 taps along one axis only (an anisotropic resize to 256 x Wr through
    ops.ingest_video with its own tables - F.interpolate scales each axis by itself), so that a tile of 8 output rows spans ~100 source rows (13 chunks of 8), or
    the staged row is wide (2204 bytes: chunks of 8 rows still; 3444 bytes: chunks of 4); and 19 x 19 taps (a short side above 1024, what 1080p gives).
    `rows` restates the launcher's chunk size: what 64 KiB of LDS leave after the padded horizontal table and the tile's vertical weights, over the bytes of one
    staged row plus one row of the horizontal pass, at most 8 and at most 20 dwords per lane of staging registers, rounded down to a multiple of 4."""
    from synchformer_amd import ops
    from synchformer_amd.ingest import aa_bicubic_table
    raw = R.random_frames(3, H, W, H + W)
    x0 = (Wr - 224) // 2
    ref = R.resize64(raw, (256, Wr))[..., 16:240, x0:x0 + 224].round().clamp(0, 255).to(torch.uint8)
    yf, yw, ty = aa_bicubic_table(H, 256)
    xf, xw, tx = aa_bicubic_table(W, Wr)
    assert (ty, tx) == (taps_y, taps_x)
    fixed = 4 * ((4 * ((tx + 6) // 4) + 3) * 224 + 8 * ty)
    row_bytes = (W + tx + 3) // 4 * 4 + 8
    assert min(8, (65536 - fixed) // (row_bytes + 896), 20 * 256 * 4 // row_bytes) // 4 * 4 == rows
    tabs = [yf[16:240], yw[16:240], xf[x0:x0 + 224], xw[x0:x0 + 224]]
    tabs = [t.contiguous().to(gpu) for t in tabs]
    pick = torch.tensor([2, 0, 1], dtype=torch.int32, device=gpu)
    got = ops.ingest_video(raw.to(gpu), False, pick, *tabs)
    torch.cuda.synchronize()
    R.check_pixels(got, ref[[2, 0, 1]], f'{H} x {W} taps {ty} x {tx}')
    with pytest.raises(RuntimeError, match='out of range'):
        ops.ingest_video(raw.to(gpu), False, pick, tabs[0], torch.zeros(224, 36, device=gpu), tabs[2], tabs[3])


def test_ingest_video_strided_rows(gpu):
    """The source is a window of a wider, taller buffer (row stride 517 > W, frame stride beyond H rows) filled with a value that would show."""
    from synchformer_amd.ingest import RecordingIngest
    H, W = 270, 480
    raw, ref = _video_case(H, W)
    buf = torch.full((5, 3, H + 3, 517), 255, dtype=torch.uint8)
    buf[:, :, 2:2 + H, 30:30 + W] = raw
    view = buf.to(gpu)[:, :, 2:2 + H, 30:30 + W]
    assert not view.is_contiguous()
    ing = RecordingIngest(gpu, 25, (H, W), 16000)
    ing._tables = {5: torch.tensor(TABLE, dtype=torch.int32)}
    got = ing.frames(view, 0, 5)
    torch.cuda.synchronize()
    R.check_pixels(got, ref[TABLE], 'strided rows')


@pytest.mark.parametrize('H, W', [(270, 480), (360, 202)])
def test_ingest_video_border(gpu, H, W):
    """resize_side = 224: the crop is the whole short side, so the first and last output rows (columns) use the filter rows clamped at the picture's edge."""
    from synchformer_amd.ingest import RecordingIngest
    raw, ref = _video_case(H, W, 224)
    ing = RecordingIngest(gpu, 25, (H, W), 16000, resize_side=224)
    assert min(ing.y0, ing.x0) == 0 and int(min(ing.y_first.min(), ing.x_first.min())) == 0
    ing._tables = {5: torch.tensor(TABLE, dtype=torch.int32)}
    got = ing.frames(raw.to(gpu), 0, 5)
    torch.cuda.synchronize()
    R.check_pixels(got, ref[TABLE], f'{H} x {W} resize_side 224')


@pytest.mark.parametrize('channels_last', [False, True])
def test_ingest_video_identity_is_the_centre_crop(gpu, channels_last):
    from synchformer_amd.ingest import RecordingIngest
    g = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 256, (3, 3, 256, 256), generator=g, dtype=torch.uint8)
    src = raw.permute(0, 2, 3, 1).contiguous() if channels_last else raw
    ing = RecordingIngest(gpu, 25, (256, 256), 16000, channels_last=channels_last)
    got = ing.frames(src.to(gpu), 0, 3)
    assert torch.equal(got.cpu(), raw[:, :, 16:240, 16:240])


with open(D.OUT) as _f:
    DIGESTS = json.load(_f)['cases']


@pytest.mark.parametrize('name', list(D.CASES))
def test_ingest_outputs_are_pinned(gpu, name):
    """The pixel tests above allow one level against float64 and would pass a changed summation order; this one holds the output BYTES of the smallest inputs
    that reach every branch of the resize pipeline (tests/golden/make_ingest_digests.py lists them) to the SHA-256 recorded once, on the commit the file names.
    The input's own digest is checked first: a mismatch there is a changed random stream, not a changed kernel."""
    assert set(DIGESTS) == set(D.CASES)
    src, out = D.CASES[name](gpu)
    torch.cuda.synchronize()
    assert D.sha256(src) == DIGESTS[name]['input'], f'{name}: the generated INPUT differs from the recorded one'
    assert D.sha256(out) == DIGESTS[name]['output'], f'{name}: output bytes differ from the recording'


# ---- audio ----------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wave_case(rate, n):
    g = torch.Generator().manual_seed(rate + n)
    x = torch.rand(n, generator=g) * 2 - 1
    return x, R.resample64(x, rate)


@pytest.mark.parametrize('n', [4411, 100, 1])
@pytest.mark.parametrize('rate', [48000, 44100, 22050, 8000, 32000])
def test_resample_wave_matches_float64(gpu, rate, n):
    """U(-1, 1) noise against the float64 restatement: max abs error <= 1e-5 (the fp32 restatement on the CPU measures 3e-7; 1e-5 leaves room for another
    summation order and is below one 16-bit step, 3e-5).  n = 100 is shorter than the 475-tap kernel, n = 1 is a single sample."""
    from synchformer_amd.ingest import RecordingIngest
    x, ref = _wave_case(rate, n)
    ing = RecordingIngest(gpu, 25, (256, 256), rate)
    y = ing.wave(x.to(gpu))
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and y.shape == ref.shape == (ing.n_samples(n),) and y.is_cuda
    err = (y.cpu().double() - ref).abs().max().item()
    print(f'{rate} Hz, {n} samples -> {y.numel()}: {ing.n} phases x {ing.kernel.shape[1]} taps, max |gpu - float64| {err:.3e}')
    assert err <= 1e-5, err
    assert torch.equal(ing.wave(x), y)                                           # from host memory


@pytest.mark.parametrize('rate', [48000, 44100])
def test_resample_wave_int16_and_stereo(gpu, rate):
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 25, (256, 256), rate)
    g = torch.Generator().manual_seed(rate)
    pcm = torch.randint(-32768, 32768, (4411,), generator=g, dtype=torch.int32).to(torch.int16)
    y_pcm = ing.wave(pcm.to(gpu))
    y_f32 = ing.wave((pcm.float() / 32768).to(gpu))
    assert torch.equal(y_pcm, y_f32)                                             # x / 32768 is exact in fp32
    x2 = torch.rand(2, 4411, generator=g) * 2 - 1
    ref = R.resample64(x2.double().mean(0), rate)
    y2 = ing.wave(x2.to(gpu))
    err = (y2.cpu().double() - ref).abs().max().item()
    print(f'{rate} Hz stereo: max |gpu - float64 of the mean| {err:.3e}')
    assert err <= 1e-5, err
    wide = torch.zeros(2, 5000)                                                  # a channel stride above the length
    wide[:, :4411] = x2
    assert torch.equal(ing.wave(wide.to(gpu)[:, :4411]), y2)


def test_wave_at_16k_is_the_input(gpu):
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 25, (256, 256), 16000)
    g = torch.Generator().manual_seed(16)
    x = torch.rand(4411, generator=g) * 2 - 1
    assert torch.equal(ing.wave(x.to(gpu)).cpu(), x) and torch.equal(ing.wave(x[None]).cpu(), x)
    # stereo / PCM at 16 kHz: the down-mix and the scaling alone, no filter
    x2 = torch.stack([x, x.flip(0)])
    assert torch.equal(ing.wave(x2.to(gpu)).cpu(), (x2[0] + x2[1]) * 0.5)
    pcm = (x * 32767).to(torch.int16)
    assert torch.equal(ing.wave(pcm.to(gpu)).cpu(), pcm.float() / 32768)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------------
T25, N16 = 136, 86400                                                            # 16 video segments, 15 audio segments -> 15 segments, 2 windows


@pytest.fixture(scope='module')
def rec(gpu):
    """One engine (synthetic weights, seg_chunk = 4: the schedule on which a segment's features do not depend on its place in a launch), one raw recording at
    25 fps, 256 x 256, 16 kHz and its track through the existing entry point on the centre-cropped frames - computed once, read-only."""
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.track import OffsetTracker
    eng = SynchformerEngine(synth.make_state_dict(1337), gpu, seg_chunk=4)
    mel = MelFrontend(gpu)
    g = torch.Generator().manual_seed(77)
    raw = torch.randint(0, 256, (T25, 3, 256, 256), generator=g, dtype=torch.uint8)
    wave = synth.make_wave(1, 1, 77, n=N16).reshape(N16)
    crop = raw[:, :, 16:240, 16:240].contiguous()
    tracker = OffsetTracker(eng, mel)
    ref = tracker.track(crop.to(gpu), wave.to(gpu))
    vbank, abank = eng.extract_recording(crop.to(gpu), wave.to(gpu), mel)
    torch.cuda.synchronize()
    return dict(eng=eng, mel=mel, tracker=tracker, raw=raw, wave=wave, crop=crop, ref=ref, vbank=vbank, abank=abank)


def test_track_raw_identity_is_track(gpu, rec):
    from synchformer_amd.frontend import recording_geometry
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 25, (256, 256), 16000)
    geo = recording_geometry(T25, N16)
    assert (geo['n_segments'], geo['n_windows']) == (15, 2)
    for raw, wave in ((rec['raw'].to(gpu), rec['wave'].to(gpu)), (rec['raw'], rec['wave'])):             # device, host
        tr = rec['tracker'].track_raw(raw, wave, ing)
        assert tr.n_segments == 15 and tr.logits.shape == (2, 21)
        assert torch.equal(tr.logits, rec['ref'].logits), (tr.logits - rec['ref'].logits).abs().max().item()
        assert torch.equal(tr.cls_path, rec['ref'].cls_path) and torch.equal(tr.cls_raw, rec['ref'].cls_raw) and torch.equal(tr.t_sec, rec['ref'].t_sec)


def test_track_raw_rate_conversion(gpu, rec):
    """The same frames, each shown twice, declared as 50 fps and channels-last; the audio at 48 kHz.  The frame pick takes frame 2 j for slot j (and frame 271 for
    the extra slot 136, which no segment of the 15 reads), so the visual bank is the 25 fps bank bit for bit; the audio bank is extract_recording's on the
    resampled wave."""
    from synchformer_amd.frontend import recording_geometry
    from synchformer_amd.ingest import RecordingIngest
    eng, mel = rec['eng'], rec['mel']
    raw50 = rec['raw'].repeat_interleave(2, 0).permute(0, 2, 3, 1).contiguous()                          # (272, 256, 256, 3)
    g = torch.Generator().manual_seed(48)
    wave48 = torch.rand(2, 3 * N16, generator=g) * 2 - 1
    ing = RecordingIngest(gpu, 50, (256, 256), 48000, channels_last=True)
    assert ing.n_frames(272) == 137 and ing.n_samples(3 * N16) == N16
    w16 = ing.wave(wave48)
    geo = recording_geometry(137, N16)
    assert geo['n_segments'] == 15
    vb, ab = eng.extract_recording_from(lambda f0, f1: ing.frames(raw50, f0, f1), 137, w16, mel)
    assert torch.equal(vb, rec['vbank'])
    _, ab_ref = eng.extract_recording(rec['crop'], w16, mel)
    assert torch.equal(ab, ab_ref) and not torch.equal(ab, rec['abank'])
    tr = rec['tracker'].track_raw(raw50, wave48, ing)
    assert tr.n_segments == geo['n_segments'] and tr.logits.shape == (geo['n_windows'], 21) and torch.isfinite(tr.logits).all()
    assert torch.equal(tr.logits, rec['tracker'].track_features(vb, ab).logits)


def test_track_raw_error_paths(gpu, rec):
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 50, (256, 256), 16000)
    with pytest.raises(ValueError, match='13 segments'):                         # 237 frames at 50 fps -> 119 at 25 fps: 13 segments, below one window
        rec['tracker'].track_raw(rec['raw'].repeat_interleave(2, 0)[:237], rec['wave'], ing)
    with pytest.raises(ValueError, match='raw frames'):
        rec['tracker'].track_raw(rec['crop'], rec['wave'], RecordingIngest(gpu, 25, (256, 256), 16000))   # 224 x 224 frames, 256 x 256 declared
