"""GPU: ingest of 10-bit YUV 4:2:0 frames (P010, yuv420p10le) and sited chroma.  sf_ingest_video_yuv16 against the float64 oracle of
tests/ingest_yuv16_oracle.py (a dense shifted filter per axis, its own 10-bit matrix, one rounding) under the project's pixel bar, bit for bit against the 8-bit
kernel on frames that hold 4 v8, the chroma_loc tables on the 8-bit kernels, and OffsetTracker.track_raw from a P010 recording against the same recording as NV12."""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_yuv_oracle as Y8  # noqa: E402
import ingest_yuv16_oracle as Y  # noqa: E402

pytestmark = pytest.mark.gpu

FMTS = list(Y.FMTS)
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ingest16_digests.json')


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """(10-bit planes of 5 source frames, oracle uint8 (5, 3, 224, 224) of those frames, colour setting, siting) - computed once per size, read-only."""
    cs, full, loc = Y.CASES[(H, W)]
    planes = Y.random_planes(5, H, W, H * 10000 + W + 256)
    Hr, Wr, y0, x0 = Y.origin(H, W)
    ref, outside = Y.oracle(planes, (Hr, Wr), y0, x0, *Y.matrix64_10(cs, full), loc)
    return planes, ref, cs, full, loc, outside


def _ingest(gpu, H, W, pix_fmt, cs='bt601', full=False, loc='center', **kw):
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 25, (H, W), 16000, pix_fmt=pix_fmt, colorspace=cs, full_range=full, chroma_loc=loc, **kw)
    ing._tables = {5: torch.tensor(Y.TABLE, dtype=torch.int32)}                  # the frame pick under test: a repeat and a skip
    return ing


@pytest.mark.parametrize('pix_fmt', FMTS)
@pytest.mark.parametrize('H, W', list(Y.CASES))
def test_yuv16_matches_oracle(gpu, H, W, pix_fmt):
    """The four settings of the pixel bar ((270, 480) and (144, 176) bt709 limited left, (1080, 608) bt601 full centre, (540, 960) bt601 limited left) and
    (360, 202) top-left: portrait, chroma width 101, so P010's chroma rows are only 4-byte aligned and yuv420p10le's only 2-byte aligned."""
    planes, ref, cs, full, loc, outside = _case(H, W)
    ing = _ingest(gpu, H, W, pix_fmt, cs, full, loc)
    src = Y.pack(*planes, pix_fmt)
    assert src.shape == (5, H * 3 // 2, W) and src.dtype == torch.uint16
    for where in (src.to(gpu), src):                                             # on the device, and uploaded from the host
        got = ing.frames(where, 0, 5)
        torch.cuda.synchronize()
        Y.check_pixels(got, ref[Y.TABLE], f'{H} x {W} {pix_fmt} {cs} {"full" if full else "limited"} {loc} taps {ing.taps_y} x {ing.taps_x} / {ing.taps_cy} x '
                                          f'{ing.taps_cx}, {outside:.0%} outside [0, 255] before the clamp')
    part = ing.frames(src, 2, 5)                                                 # a slice of the output frames reads source frames 2 .. 4 only
    assert torch.equal(part, got[2:5])
    assert torch.equal(ing.frames(src.view(torch.int16).to(gpu), 0, 5), got)     # int16: the same bits


def _own_tables(gpu, H, W, size, y0, x0):
    """The test's own tables for ops.ingest_video_yuv16: luma and chroma resized to `size`, cropped at (y0, x0); and their taps."""
    from synchformer_amd.ingest import aa_bicubic_table
    tabs, taps = [], []
    for h, w in ((H, W), (H // 2, W // 2)):
        yf, yw, ty = aa_bicubic_table(h, size[0])
        xf, xw, tx = aa_bicubic_table(w, size[1])
        taps.append((ty, tx))
        tabs += [t[o:o + 224].contiguous().to(gpu) for t, o in ((yf, y0), (yw, y0), (xf, x0), (xw, x0))]
    return tabs, taps


def _taps_case(gpu, H, W, size, y0, x0, pix_fmt):
    """2 source frames, the pick [1, 0], through ops.ingest_video_yuv16 with the test's own tables, bt601 limited: (got, oracle, taps)."""
    from synchformer_amd import ops
    planes = Y.random_planes(2, H, W, H + W)
    ref, _ = Y.oracle(planes, size, y0, x0, *Y.matrix64_10('bt601', False))
    tabs, taps = _own_tables(gpu, H, W, size, y0, x0)
    M, off = Y.matrix64_10('bt601', False)
    pick = torch.tensor([1, 0], dtype=torch.int32, device=gpu)
    got = ops.ingest_video_yuv16(Y.pack(*planes, pix_fmt).to(gpu), pix_fmt, pick, *tabs, torch.cat([M.reshape(9), off]).float())
    torch.cuda.synchronize()
    return got, ref[[1, 0]], taps


@pytest.mark.parametrize('H, W, size, x0, luma, chroma', [(2160, 260, (256, 256), 16, (35, 7), (19, 5)), (260, 3840, (256, 454), 115, (7, 35), (5, 19)),
                                                          (1040, 1030, (256, 256), 16, (19, 19), (11, 11)), (144, 176, (256, 256), 16, (5, 5), (5, 5))])
def test_yuv16_tap_range_and_widest_row(gpu, H, W, size, x0, luma, chroma):
    """The launcher's range on the smallest inputs that reach its ends: 35 vertical taps; 35 horizontal taps on a 3840-wide row (four staged 16-bit luma rows: the
    LDS above 64 KiB and the largest staging-register count); 19 x 19 taps; both planes upscaled."""
    for pix_fmt in FMTS:
        got, ref, taps = _taps_case(gpu, H, W, size, 16, x0, pix_fmt)
        assert taps == [luma, chroma]
        Y.check_pixels(got, ref, f'{H} x {W} {pix_fmt} taps {luma} / {chroma}')


def _times4(v8_planes, pix_fmt):
    return Y.pack(*[4 * p.int() for p in v8_planes], pix_fmt)


@pytest.mark.parametrize('loc', ['center', 'left'])
@pytest.mark.parametrize('H, W', [(270, 480), (360, 202)])
def test_times_four_is_the_8_bit_kernel_bit_for_bit(gpu, H, W, loc):
    """Frames that hold 4 v8 (P010: (4 v8) << 6) through the 16-bit pipeline are torch.equal to v8 through the 8-bit one: every product and sum is the 8-bit one
    times a power of two (the limited-range matrix is the 8-bit one / 4, the offsets 4 times the 8-bit ones), the order of the sums is the same, and the zero rows
    of the two padded tables add exact zeros.  This ties the new instantiation to the pipeline that tests/golden/ingest_digests.json pins."""
    v8 = Y8.random_planes(5, H, W, H * 10000 + W + 256)
    want = {f: _ingest(gpu, H, W, f, 'bt709', False, loc).frames(Y8.pack(*v8, f).to(gpu), 0, 5) for f in ('nv12', 'yuv420p')}
    assert torch.equal(want['nv12'], want['yuv420p'])
    for pix_fmt in FMTS:
        got = _ingest(gpu, H, W, pix_fmt, 'bt709', False, loc).frames(_times4(v8, pix_fmt).to(gpu), 0, 5)
        torch.cuda.synchronize()
        assert torch.equal(got, want['nv12']), (pix_fmt, loc, (got.int() - want['nv12'].int()).abs().max().item())


@pytest.mark.parametrize('pix_fmt', ['nv12', 'yuv420p'])
@pytest.mark.parametrize('loc', ['left', 'topleft'])
def test_siting_on_8_bit(gpu, pix_fmt, loc):
    """chroma_loc on the 8-bit kernels (tables only) against the shifted oracle with the 8-bit matrix."""
    H, W = 270, 480
    planes = Y8.random_planes(5, H, W, H * 10000 + W + 256)
    Hr, Wr, y0, x0 = Y.origin(H, W)
    ref, _ = Y.oracle(planes, (Hr, Wr), y0, x0, *Y8.matrix64('bt601', False), loc)
    ing = _ingest(gpu, H, W, pix_fmt, 'bt601', False, loc)
    got = ing.frames(Y8.pack(*planes, pix_fmt).to(gpu), 0, 5)
    torch.cuda.synchronize()
    Y.check_pixels(got, ref[Y.TABLE], f'{H} x {W} {pix_fmt} {loc}')
    centre = _ingest(gpu, H, W, pix_fmt, 'bt601', False, 'center').frames(Y8.pack(*planes, pix_fmt).to(gpu), 0, 5)
    assert not torch.equal(centre, got)                                          # and the siting is seen in the picture


def test_stray_bits_are_dropped(gpu):
    """P010 with random low six bits and yuv420p10le with random high six bits give the bytes of the clean input."""
    H, W = 270, 480
    planes, _, cs, full, loc, _ = _case(H, W)
    g = torch.Generator().manual_seed(5)
    for pix_fmt, up in (('p010', 0), ('yuv420p10le', 10)):
        clean = Y.pack(*planes, pix_fmt)
        dirty = (clean.int() | (torch.randint(0, 64, clean.shape, generator=g, dtype=torch.int32) << up)).to(torch.uint16)
        assert not torch.equal(clean, dirty)
        ing = _ingest(gpu, H, W, pix_fmt, cs, full, loc)
        assert torch.equal(ing.frames(dirty.to(gpu), 0, 5), ing.frames(clean.to(gpu), 0, 5)), pix_fmt


def _pitched(gpu, planes, H, W):
    buf = torch.full((5, H * 3 // 2, W + 32), 0xffff, dtype=torch.int32).to(torch.uint16)
    buf[:, :, :W] = Y.pack(*planes, 'p010')
    view = buf.to(gpu)[:, :, :W]
    assert not view.is_contiguous() and view.stride() == (H * 3 // 2 * (W + 32), W + 32, 1)
    return view


def test_p010_pitched_surface(gpu):
    """A 270 x 480 P010 frame inside a surface of row pitch W + 32 elements filled with a value that would show, read in place as a non-contiguous view."""
    H, W = 270, 480
    planes, ref, cs, full, loc, _ = _case(H, W)
    view = _pitched(gpu, planes, H, W)
    got = _ingest(gpu, H, W, 'p010', cs, full, loc).frames(view, 0, 5)
    torch.cuda.synchronize()
    assert torch.equal(got, _ingest(gpu, H, W, 'p010', cs, full, loc).frames(Y.pack(*planes, 'p010').to(gpu), 0, 5))
    Y.check_pixels(got, ref[Y.TABLE], 'P010 at pitch W + 32')
    with pytest.raises(ValueError, match='contiguous rows'):                     # yuv420p10le has no pitch to give
        _ingest(gpu, H, W, 'yuv420p10le', cs, full, loc).frames(view, 0, 5)


def _constant(gpu, yuv, pix_fmt, cs='bt709', full=False):
    from synchformer_amd.ingest import RecordingIngest
    planes = [torch.full((1, s, s), v, dtype=torch.int32) for s, v in zip((256, 128, 128), yuv)]
    ing = RecordingIngest(gpu, 25, (256, 256), 16000, pix_fmt=pix_fmt, colorspace=cs, full_range=full)
    out = ing.frames(Y.pack(*planes, pix_fmt).to(gpu), 0, 1).cpu()
    assert all(int((out[0, c].int() - int(out[0, c, 0, 0])).abs().max()) <= 1 for c in range(3))    # the resize of a constant is the constant, to fp32 rounding
    return out[0, :, 112, 112].int().tolist()


@pytest.mark.parametrize('pix_fmt', FMTS)
def test_colour_known_answers_10_bit(gpu, pix_fmt):
    """Constant planes, so only the matrix is at work: 10-bit limited-range black and white and the BT.709 primaries (code values from the BT.709 quantisation,
    Y = 64 + 876 E'y, C = 512 + 896 E'c, rounded: within 1 level), and the ends of the full-range grey axis (exact).  Independent of the oracle's formula."""
    assert _constant(gpu, (64, 512, 512), pix_fmt) == [0, 0, 0]
    assert _constant(gpu, (940, 512, 512), pix_fmt) == [255, 255, 255]
    for yuv, rgb in (((250, 409, 960), (255, 0, 0)), ((691, 167, 105), (0, 255, 0)), ((127, 960, 471), (0, 0, 255))):
        got = _constant(gpu, yuv, pix_fmt)
        print(f'{pix_fmt} bt709 limited {yuv} -> {got} (exact {rgb})')
        assert max(abs(a - b) for a, b in zip(got, rgb)) <= 1, (yuv, got)
    for cs in ('bt601', 'bt709'):
        assert _constant(gpu, (0, 512, 512), pix_fmt, cs, True) == [0, 0, 0]
        assert _constant(gpu, (1023, 512, 512), pix_fmt, cs, True) == [255, 255, 255]


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------------
T25, N16 = 120, 76800                                                            # 15 - 1 = 14 video and 14 audio segments: the shortest recording with one window


@pytest.fixture(scope='module')
def rec(gpu):
    """One engine (synthetic weights, seg_chunk = 4), one 8-bit recording at 25 fps, 256 x 256, 16 kHz with random luma and chroma, and its track as NV12 through
    the 8-bit path - computed once, read-only."""
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend, recording_geometry
    from synchformer_amd.ingest import RecordingIngest
    from synchformer_amd.track import OffsetTracker
    geo = recording_geometry(T25, N16)
    assert geo['n_windows'] == 1, geo
    eng = SynchformerEngine(synth.make_state_dict(1337), gpu, seg_chunk=4)
    mel = MelFrontend(gpu)
    g = torch.Generator().manual_seed(79)
    v8 = [torch.randint(0, 256, (T25, s, s), generator=g, dtype=torch.uint8) for s in (256, 128, 128)]
    wave = synth.make_wave(1, 1, 79, n=N16).reshape(N16)
    tracker = OffsetTracker(eng, mel)
    ref = tracker.track_raw(Y8.pack(*v8, 'nv12').to(gpu), wave.to(gpu), RecordingIngest(gpu, 25, (256, 256), 16000, pix_fmt='nv12'))
    torch.cuda.synchronize()
    return dict(tracker=tracker, v8=v8, wave=wave, ref=ref)


def test_track_from_p010_is_the_track_from_nv12(gpu, rec):
    """track_raw from P010 frames that hold 4 v8, on the device and in pinned host memory, equals track_raw from the NV12 recording of v8 in logits and paths."""
    from synchformer_amd.ingest import RecordingIngest
    raw = _times4(rec['v8'], 'p010')
    ing = RecordingIngest(gpu, 25, (256, 256), 16000, pix_fmt='p010')
    ref = rec['ref']
    for frames, wave in ((raw.to(gpu), rec['wave'].to(gpu)), (raw.pin_memory(), rec['wave'].pin_memory())):
        tr = rec['tracker'].track_raw(frames, wave, ing)
        assert tr.logits.shape == ref.logits.shape and tr.logits.shape[0] == 1
        assert torch.equal(tr.logits, ref.logits), (tr.logits - ref.logits).abs().max().item()
        assert torch.equal(tr.cls_raw, ref.cls_raw) and torch.equal(tr.cls_path, ref.cls_path)


def test_yuv16_error_paths(gpu):
    from synchformer_amd import ops
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 25, (256, 256), 16000, pix_fmt='p010')
    tabs = (ing.y_first, ing.y_w, ing.x_first, ing.x_w, ing.cy_first, ing.cy_w, ing.cx_first, ing.cx_w, ing.csc)
    pick = torch.zeros(1, dtype=torch.int32, device=gpu)
    with pytest.raises(RuntimeError, match='device tensor'):                     # a CPU tensor handed to the op itself
        ops.ingest_video_yuv16(torch.zeros(1, 384, 256, dtype=torch.uint16), 'p010', pick, *tabs)
    with pytest.raises(ValueError, match='expected uint16'):
        ops.ingest_video_yuv16(torch.zeros(1, 384, 256, dtype=torch.uint8, device=gpu), 'p010', pick, *tabs)
    with pytest.raises(ValueError, match='raw frames'):                          # NV12 frames, P010 declared
        ing.frames(torch.zeros(4, 384, 256, dtype=torch.uint8, device=gpu), 0, 1)
    bad = list(tabs)
    bad[5] = torch.zeros(224, 36, device=gpu)
    with pytest.raises(RuntimeError, match='out of range'):
        ops.ingest_video_yuv16(torch.zeros(1, 384, 256, dtype=torch.uint16, device=gpu), 'p010', pick, *bad)
    empty = ops.ingest_video_yuv16(torch.zeros(1, 384, 256, dtype=torch.uint16, device=gpu), 'p010', pick[:0], *tabs)
    assert empty.shape == (0, 3, 224, 224)


# ---- regression pin ---------------------------------------------------------------------------------------------------------------------------------------------
def sha256(t: torch.Tensor) -> str:
    return hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _pin_frames(H, W, pix_fmt, pitched=False):
    def run(gpu):
        planes, _, cs, full, loc, _ = _case(H, W)
        src = Y.pack(*planes, pix_fmt)
        return src, _ingest(gpu, H, W, pix_fmt, cs, full, loc).frames(_pitched(gpu, planes, H, W) if pitched else src.to(gpu), 0, 5)
    return run


def _pin_taps(H, W, size, x0, pix_fmt):
    def run(gpu):
        return Y.pack(*Y.random_planes(2, H, W, H + W), pix_fmt), _taps_case(gpu, H, W, size, 16, x0, pix_fmt)[0]
    return run


# name -> run(device) -> (the input as generated on the CPU, the uint8 output on the device)
PINNED = {
    'p010_270x480_bt709_left_pitched': _pin_frames(270, 480, 'p010', pitched=True),          # the 16-byte interleaved fetch, a pitched surface
    'yuv420p10le_360x202_bt601_topleft': _pin_frames(360, 202, 'yuv420p10le'),               # 2-byte loads on the unaligned chroma rows
    'p010_260x3840_to_256x454_taps35': _pin_taps(260, 3840, (256, 454), 115, 'p010'),        # 35 horizontal taps on the widest row
    'yuv420p10le_2160x260_to_256x256_taps35': _pin_taps(2160, 260, (256, 256), 16, 'yuv420p10le'),    # 35 vertical taps
}


@pytest.mark.parametrize('name', list(PINNED))
def test_yuv16_outputs_are_pinned(gpu, name):
    """Guards LATER refactors only: the SHA-256 of the output bytes of four of the cases above, recorded after this kernel's first passing run, on the code that
    this file arrived with.  It proves nothing about that code - the oracle, the x4 identity and the known answers do; it shows a later change of the summation
    order or of the addressing that the one-level pixel bar would pass.  The input's own digest is checked first: a mismatch there is a changed random stream."""
    with open(DIGESTS) as f:
        digests = json.load(f)['cases']
    assert set(digests) == set(PINNED)
    src, out = PINNED[name](gpu)
    torch.cuda.synchronize()
    print(f'{name}: input {sha256(src)} output {sha256(out)}')
    assert sha256(src) == digests[name]['input'], f'{name}: the generated INPUT differs from the recorded one'
    assert sha256(out) == digests[name]['output'], f'{name}: the output bytes differ from the recorded ones'
