"""GPU: ingest of 8-bit YUV 4:2:0 frames.  sf_ingest_video_yuv against the float64 oracle of tests/ingest_yuv_oracle.py (F.interpolate on each
plane, the colour matrix written out there, one rounding) under the pixel bar of test_ingest_gpu.py, the matrix against published 8-bit triples, and
OffsetTracker.track_raw on a grey full-range YUV recording against the same recording as RGB through the existing path, bit for bit."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_yuv_oracle as Y  # noqa: E402

pytestmark = pytest.mark.gpu

FMTS = ['nv12', 'yuv420p']


@functools.lru_cache(maxsize=None)
def _case(H, W, side=256):
    """(planes of 5 source frames, oracle uint8 (5, 3, 224, 224) of those frames, colour setting) - computed once per size, read-only."""
    cs, full, _, _ = Y.CASES[(H, W)]
    planes = Y.random_planes(5, H, W, H * 10000 + W + side)
    Hr, Wr, y0, x0 = Y.origin(H, W, side)
    ref, outside = Y.oracle(planes, (Hr, Wr), y0, x0, cs, full)
    return planes, ref, cs, full, outside


def _ingest(gpu, H, W, pix_fmt, cs, full, **kw):
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 25, (H, W), 16000, pix_fmt=pix_fmt, colorspace=cs, full_range=full, **kw)
    ing._tables = {5: torch.tensor(Y.TABLE, dtype=torch.int32)}                  # the frame pick under test: a repeat and a skip
    return ing


@pytest.mark.parametrize('pix_fmt', FMTS)
@pytest.mark.parametrize('H, W', list(Y.CASES))
def test_yuv_matches_oracle(gpu, H, W, pix_fmt):
    """(270, 480): H % 4 = 2, I420's U plane ends in the middle of a row of the (3 H / 2, W) array; (360, 202): portrait, chroma width 101, so chroma rows start
    unaligned; (144, 176): both planes upscale; (540, 960): taps 11 / 7; (302, 518); (1080, 608).  bt601 limited range and bt709 full range alternate."""
    planes, ref, cs, full, outside = _case(H, W)
    ing = _ingest(gpu, H, W, pix_fmt, cs, full)
    assert ((ing.taps_y, ing.taps_x), (ing.taps_cy, ing.taps_cx)) == Y.CASES[(H, W)][2:]
    src = Y.pack(*planes, pix_fmt)
    assert src.shape == (5, H * 3 // 2, W)
    for where in (src.to(gpu), src):                                             # on the device, and uploaded from the host
        got = ing.frames(where, 0, 5)
        torch.cuda.synchronize()
        Y.check_pixels(got, ref[Y.TABLE], f'{H} x {W} {pix_fmt} {cs} {"full" if full else "limited"} taps {ing.taps_y} x {ing.taps_x} / {ing.taps_cy} x {ing.taps_cx}, '
                                          f'{outside:.0%} outside [0, 255] before the clamp')
    part = ing.frames(src, 2, 5)                                                 # a slice of the output frames reads source frames 2 .. 4 only
    assert torch.equal(part, got[2:5])


@pytest.mark.parametrize('H, W, luma, chroma', [(2160, 260, (35, 7), (19, 5)), (260, 2160, (7, 35), (5, 19)), (1040, 1030, (19, 19), (11, 11))])
def test_yuv_many_taps(gpu, H, W, luma, chroma):
    """The launcher's tap range on the smallest inputs that reach its ends: an anisotropic resize to 256 x 256 through ops.ingest_video_yuv with its own tables."""
    from synchformer_amd import ops
    from synchformer_amd.ingest import aa_bicubic_table, csc_matrix
    planes = Y.random_planes(2, H, W, H + W)
    ref, _ = Y.oracle(planes, (256, 256), 16, 16, 'bt601', False)
    tabs, taps = [], []
    for h, w in ((H, W), (H // 2, W // 2)):
        yf, yw, ty = aa_bicubic_table(h, 256)
        xf, xw, tx = aa_bicubic_table(w, 256)
        taps.append((ty, tx))
        tabs += [t[16:240].contiguous().to(gpu) for t in (yf, yw, xf, xw)]
    assert taps == [luma, chroma]
    M, off = csc_matrix('bt601', False)
    csc = torch.cat([M.reshape(9), off]).float()
    pick = torch.tensor([1, 0], dtype=torch.int32, device=gpu)
    for pix_fmt in FMTS:
        got = ops.ingest_video_yuv(Y.pack(*planes, pix_fmt).to(gpu), pix_fmt, pick, *tabs, csc)
        torch.cuda.synchronize()
        Y.check_pixels(got, ref[[1, 0]], f'{H} x {W} {pix_fmt} taps {luma} / {chroma}')
    raw = Y.pack(*planes, 'nv12').to(gpu)
    for i in (1, 3, 5, 7):                                                       # a 36-tap table in each of the four places
        bad = list(tabs)
        bad[i] = torch.zeros(224, 36, device=gpu)
        with pytest.raises(RuntimeError, match='out of range'):
            ops.ingest_video_yuv(raw, 'nv12', pick, *bad, csc)


def test_nv12_pitched_surface(gpu):
    """A 270 x 480 NV12 frame inside a (5, 405, 512) surface filled with a value that would show, read in place as a non-contiguous view."""
    H, W = 270, 480
    planes, ref, cs, full, _ = _case(H, W)
    buf = torch.full((5, 405, 512), 255, dtype=torch.uint8)
    buf[:, :, :W] = Y.pack(*planes, 'nv12')
    view = buf.to(gpu)[:, :, :W]
    assert not view.is_contiguous() and view.stride() == (405 * 512, 512, 1)
    got = _ingest(gpu, H, W, 'nv12', cs, full).frames(view, 0, 5)
    torch.cuda.synchronize()
    Y.check_pixels(got, ref[Y.TABLE], 'NV12 at pitch 512')
    with pytest.raises(ValueError, match='contiguous rows'):                     # I420 has no pitch to give
        _ingest(gpu, H, W, 'yuv420p', cs, full).frames(view, 0, 5)


@pytest.mark.parametrize('pix_fmt', FMTS)
@pytest.mark.parametrize('H, W', [(270, 480), (360, 202)])
def test_yuv_border(gpu, H, W, pix_fmt):
    """resize_side = 224: the crop is the whole short side, so the first and last output rows (columns) use filter rows clamped at the edge of the luma AND of
    the chroma planes."""
    planes, ref, cs, full, _ = _case(H, W, 224)
    ing = _ingest(gpu, H, W, pix_fmt, cs, full, resize_side=224)
    assert min(ing.y0, ing.x0) == 0 and int(min(ing.y_first.min(), ing.x_first.min())) == 0 and int(min(ing.cy_first.min(), ing.cx_first.min())) == 0
    got = ing.frames(Y.pack(*planes, pix_fmt).to(gpu), 0, 5)
    torch.cuda.synchronize()
    Y.check_pixels(got, ref[Y.TABLE], f'{H} x {W} {pix_fmt} resize_side 224')


def _constant(gpu, yuv, pix_fmt, cs='bt601', full=False):
    from synchformer_amd.ingest import RecordingIngest
    planes = [torch.full((1, s, s), v, dtype=torch.uint8) for s, v in zip((256, 128, 128), yuv)]
    ing = RecordingIngest(gpu, 25, (256, 256), 16000, pix_fmt=pix_fmt, colorspace=cs, full_range=full)
    out = ing.frames(Y.pack(*planes, pix_fmt).to(gpu), 0, 1).cpu()
    assert all(bool((out[0, c] == out[0, c, 0, 0]).all()) for c in range(3))    # the resize of a constant is the constant
    return out[0, :, 0, 0].int().tolist()


@pytest.mark.parametrize('pix_fmt', FMTS)
def test_colour_known_answers(gpu, pix_fmt):
    """Constant planes, so only the matrix is at work: the published 8-bit BT.601 triples of black, white and the primaries (themselves rounded: within 2
    levels), and the grey axis of full range (exact).  Independent of the oracle's formula."""
    assert _constant(gpu, (16, 128, 128), pix_fmt) == [0, 0, 0]
    assert _constant(gpu, (235, 128, 128), pix_fmt) == [255, 255, 255]
    for yuv, rgb in (((81, 90, 240), (255, 0, 0)), ((145, 54, 34), (0, 255, 0)), ((41, 240, 110), (0, 0, 255))):
        got = _constant(gpu, yuv, pix_fmt)
        print(f'{pix_fmt} bt601 limited {yuv} -> {got} (published {rgb})')
        assert max(abs(a - b) for a, b in zip(got, rgb)) <= 2, (yuv, got)
    for y in (0, 1, 77, 128, 254, 255):
        assert _constant(gpu, (y, 128, 128), pix_fmt, full=True) == [y, y, y]
        assert _constant(gpu, (y, 128, 128), pix_fmt, 'bt709', True) == [y, y, y]


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------------
T25, N16 = 136, 86400                                                            # 16 video segments, 15 audio segments -> 15 segments, 2 windows


@pytest.fixture(scope='module')
def rec(gpu):
    """One engine (synthetic weights, seg_chunk = 4), one grey recording at 25 fps, 256 x 256, 16 kHz: random luma, and its track as the RGB recording (Y, Y, Y)
    through the existing rgb24 path - computed once, read-only."""
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.ingest import RecordingIngest
    from synchformer_amd.track import OffsetTracker
    eng = SynchformerEngine(synth.make_state_dict(1337), gpu, seg_chunk=4)
    mel = MelFrontend(gpu)
    g = torch.Generator().manual_seed(78)
    luma = torch.randint(0, 256, (T25, 256, 256), generator=g, dtype=torch.uint8)
    wave = synth.make_wave(1, 1, 78, n=N16).reshape(N16)
    tracker = OffsetTracker(eng, mel)
    rgb = luma[:, None].expand(T25, 3, 256, 256).contiguous()
    ref = tracker.track_raw(rgb.to(gpu), wave.to(gpu), RecordingIngest(gpu, 25, (256, 256), 16000))
    torch.cuda.synchronize()
    return dict(tracker=tracker, luma=luma, wave=wave, ref=ref)


@pytest.mark.parametrize('pix_fmt', FMTS)
def test_grey_full_range_identity_and_track(gpu, rec, pix_fmt):
    """U = V = 128 in full range: the matrix is the identity on the grey axis and the 256 x 256 luma resize is the identity, so frames() is the centre crop of Y
    in all three channels, bit for bit (the chroma term is below 3e-5 of a level: the chroma weights sum to 1 within fp32 rounding), and the track of the YUV
    recording is the track of the RGB recording (Y, Y, Y)."""
    from synchformer_amd.frontend import recording_geometry
    from synchformer_amd.ingest import RecordingIngest
    luma = rec['luma']
    grey = torch.full((T25, 128, 128), 128, dtype=torch.uint8)
    raw = Y.pack(luma, grey, grey, pix_fmt)
    ing = RecordingIngest(gpu, 25, (256, 256), 16000, pix_fmt=pix_fmt, full_range=True)
    got = ing.frames(raw.to(gpu), 0, T25).cpu()
    assert all(torch.equal(got[:, c], luma[:, 16:240, 16:240]) for c in range(3))
    geo = recording_geometry(T25, N16)
    assert (geo['n_segments'], geo['n_windows']) == (15, 2)
    ref = rec['ref']
    for frames, wave in ((raw.to(gpu), rec['wave'].to(gpu)), (raw, rec['wave'])):                        # device, host
        tr = rec['tracker'].track_raw(frames, wave, ing)
        assert tr.n_segments == 15 and tr.logits.shape == (2, 21)
        assert torch.equal(tr.logits, ref.logits), (tr.logits - ref.logits).abs().max().item()
        assert torch.equal(tr.cls_raw, ref.cls_raw) and torch.equal(tr.cls_path, ref.cls_path)


def test_yuv_error_paths(gpu, rec):
    from synchformer_amd import ops
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 25, (256, 256), 16000, pix_fmt='nv12')
    with pytest.raises(ValueError, match='raw frames'):                          # RGB frames, NV12 declared
        rec['tracker'].track_raw(torch.zeros(T25, 3, 256, 256, dtype=torch.uint8), rec['wave'], ing)
    with pytest.raises(ValueError, match='raw frames'):                          # 224-row luma: (T, 336, 224) frames, 256 x 256 declared
        ing.frames(torch.zeros(4, 336, 224, dtype=torch.uint8, device=gpu), 0, 1)
    with pytest.raises(RuntimeError, match='device tensor'):                     # a CPU tensor handed to the op itself
        ops.ingest_video_yuv(torch.zeros(1, 384, 256, dtype=torch.uint8), 'nv12', torch.zeros(1, dtype=torch.int32, device=gpu), ing.y_first, ing.y_w, ing.x_first,
                             ing.x_w, ing.cy_first, ing.cy_w, ing.cx_first, ing.cx_w, ing.csc)
    empty = ops.ingest_video_yuv(torch.zeros(1, 384, 256, dtype=torch.uint8, device=gpu), 'nv12', torch.zeros(0, dtype=torch.int32, device=gpu), ing.y_first,
                                 ing.y_w, ing.x_first, ing.x_w, ing.cy_first, ing.cy_w, ing.cx_first, ing.cx_w, ing.csc)
    assert empty.shape == (0, 3, 224, 224)
