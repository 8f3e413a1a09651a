"""GPU: ingest of 4:2:2 frames.  sf_ingest_video_yuv_planes through RecordingIngest and ops.ingest_video_planes against the float64 oracle of
tests/ingest_yuv422_oracle.py under the pixel bar of test_ingest_gpu.py; the seven layouts, the staging forms and the older entries against each other bit for
bit; the matrix against published triples; and OffsetTracker.track_raw / RecordingIngest.stream on a grey full-range 4:2:2 recording against the same recording
as RGB through the rgb24 path, bit for bit."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_yuv422_oracle as Y  # noqa: E402

pytestmark = pytest.mark.gpu

FMTS8 = ('uyvy422', 'yuyv422', 'yuv422p', 'nv16')
SIZES = [(270, 480), (271, 202)]                                                 # (271, 202): odd H, chroma width 101 - chroma rows and packed rows start unaligned


def _bits(pix_fmt):
    return 10 if pix_fmt in Y.FMTS_16 else 8


@functools.lru_cache(maxsize=None)
def _case(H, W, bits, side=256):
    """(planes of 5 source frames, oracle uint8 (5, 3, 224, 224) of those frames, colour setting, share outside [0, 255]) - computed once, read-only."""
    cs, full, loc, _, _ = Y.CASES[(H, W)]
    planes = Y.random_planes(5, H, W, H * 10000 + W + side + bits, 1 << bits)
    Hr, Wr, y0, x0 = Y.origin(H, W, side)
    ref, outside = Y.oracle(planes, (Hr, Wr), y0, x0, *Y.matrix(cs, full, bits), loc)
    return planes, ref, cs, full, loc, outside


def _ingest(gpu, H, W, pix_fmt, cs, full, loc='center', **kw):
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 25, (H, W), 16000, pix_fmt=pix_fmt, colorspace=cs, full_range=full, chroma_loc=loc, **kw)
    ing._tables = {5: torch.tensor(Y.TABLE, dtype=torch.int32)}                  # the frame pick under test: a repeat and a skip
    return ing


def _tabs(ing):
    return (ing.y_first, ing.y_w, ing.x_first, ing.x_w, ing.cy_first, ing.cy_w, ing.cx_first, ing.cx_w)


# ---- 1. oracle parity ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pix_fmt', Y.FMTS)
@pytest.mark.parametrize('H, W', list(Y.CASES))
def test_422_matches_oracle(gpu, H, W, pix_fmt):
    """(270, 480); (271, 202): odd H, portrait, chroma width 101; (144, 176): both planes upscale; (540, 960): taps 11 / 7.  Frames on the device and from the host."""
    planes, ref, cs, full, loc, outside = _case(H, W, _bits(pix_fmt))
    ing = _ingest(gpu, H, W, pix_fmt, cs, full, loc)
    assert ((ing.taps_y, ing.taps_x), (ing.taps_cy, ing.taps_cx)) == Y.CASES[(H, W)][3:]
    src = Y.pack(planes, pix_fmt)
    assert src.shape == ((5, H, W, 2) if pix_fmt in ('uyvy422', 'yuyv422', 'y210') else (5, 2 * H, W))
    for where in (src.to(gpu), src):
        got = ing.frames(where, 0, 5)
        torch.cuda.synchronize()
        Y.check_pixels(got, ref[Y.TABLE], f'{H} x {W} {pix_fmt} {cs} {"full" if full else "limited"} {loc} taps {ing.taps_y} x {ing.taps_x} / {ing.taps_cy} x '
                                          f'{ing.taps_cx}, {outside:.0%} outside [0, 255] before the clamp')
    part = ing.frames(src, 2, 5)                                                 # a slice of the output frames reads source frames 2 .. 4 only
    assert torch.equal(part, got[2:5])


# ---- 2. the ends of the tap range ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H, W, luma, chroma', [(2160, 260, (35, 7), (35, 5)), (260, 2160, (7, 35), (7, 19))])
def test_422_many_taps(gpu, H, W, luma, chroma):
    """An anisotropic resize to 256 x 256, crop origin 16, through ops.ingest_video_planes with the test's own tables: (2160, 260) is the first chroma pass of 35
    vertical taps (4:2:0 never passed 19)."""
    from synchformer_amd import ops
    from synchformer_amd.ingest import aa_bicubic_table, csc_matrix, plane_layout
    tabs, taps = [], []
    for h, w in ((H, W), (H, W // 2)):
        yf, yw, ty = aa_bicubic_table(h, 256)
        xf, xw, tx = aa_bicubic_table(w, 256)
        taps.append((ty, tx))
        tabs += [t[16:240].contiguous().to(gpu) for t in (yf, yw, xf, xw)]
    assert taps == [luma, chroma]
    pick = torch.tensor([1, 0], dtype=torch.int32, device=gpu)
    for pix_fmt in ('uyvy422', 'yuv422p', 'y210'):
        bits = _bits(pix_fmt)
        planes = Y.random_planes(2, H, W, H + W + bits, 1 << bits)
        ref, _ = Y.oracle(planes, (256, 256), 16, 16, *Y.matrix('bt601', False, bits))
        M, off = csc_matrix('bt601', False, bits)
        csc = torch.cat([M.reshape(9), off]).float()
        raw = Y.pack(planes, pix_fmt).to(gpu)
        got = ops.ingest_video_planes(raw, plane_layout(pix_fmt, H, W, raw.stride()), pick, *tabs, csc)
        torch.cuda.synchronize()
        Y.check_pixels(got, ref[[1, 0]], f'{H} x {W} {pix_fmt} taps {luma} / {chroma}')
    for i in (1, 3, 5, 7):                                                       # a 36-tap table in each of the four places
        bad = list(tabs)
        bad[i] = torch.zeros(224, 36, device=gpu)
        with pytest.raises(RuntimeError, match='out of range'):
            ops.ingest_video_planes(raw, plane_layout('y210', H, W), pick, *bad, csc)


def test_y210_row_too_wide_for_the_packed_form(gpu):
    """64 x 2600 to 256 x 320 (35 x 19 horizontal taps): a y210 row of 2600 + 35 columns does not fit the half chunk of the packed 16-bit staging, so the launcher
    takes the strided 2-byte loads; same oracle, same bar."""
    from synchformer_amd import ops
    from synchformer_amd.ingest import aa_bicubic_table, csc_matrix, plane_layout
    H, W = 64, 2600
    tabs, taps = [], []
    for w in (W, W // 2):
        yf, yw, ty = aa_bicubic_table(H, 256)
        xf, xw, tx = aa_bicubic_table(w, 320)
        taps.append((ty, tx))
        tabs += [yf[16:240].contiguous().to(gpu), yw[16:240].contiguous().to(gpu), xf[48:272].contiguous().to(gpu), xw[48:272].contiguous().to(gpu)]
    assert taps == [(5, 35), (5, 19)]
    planes = Y.random_planes(2, H, W, H + W, 1024)
    ref, _ = Y.oracle(planes, (256, 320), 16, 48, *Y.matrix('bt601', False, 10))
    M, off = csc_matrix('bt601', False, 10)
    raw = Y.pack(planes, 'y210').to(gpu)
    got = ops.ingest_video_planes(raw, plane_layout('y210', H, W), torch.tensor([1, 0], dtype=torch.int32, device=gpu), *tabs, torch.cat([M.reshape(9), off]).float())
    torch.cuda.synchronize()
    Y.check_pixels(got, ref[[1, 0]], f'{H} x {W} y210, strided loads, taps {taps}')


# ---- 3. bit for bit -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H, W', SIZES)
def test_422_layouts_agree(gpu, H, W):
    """The same samples as uyvy422, yuyv422, yuv422p and nv16: four staging paths, one output.  The 10-bit formats holding 4 v8 (limited range: the 10-bit
    matrix is the 8-bit one / 4 exactly) give the 8-bit output, and stray low bits in y210 / p210 words change nothing."""
    planes, _, cs, _, loc, _ = _case(H, W, 8)
    outs = {f: _ingest(gpu, H, W, f, cs, False, loc).frames(Y.pack(planes, f).to(gpu), 0, 5) for f in FMTS8}
    for f in FMTS8[1:]:
        assert torch.equal(outs[f], outs['uyvy422']), f
    g = torch.Generator().manual_seed(H + W)
    for f in Y.FMTS_16:
        raw = Y.pack([4 * p for p in planes], f)
        ing = _ingest(gpu, H, W, f, cs, False, loc)
        assert torch.equal(ing.frames(raw.to(gpu), 0, 5), outs['uyvy422']), f
        if Y.SHIFT[f] == 6:
            dirty = (raw.int() | torch.randint(0, 64, raw.shape, generator=g, dtype=torch.int32)).to(torch.uint16)
            assert not torch.equal(dirty, raw)
            assert torch.equal(ing.frames(dirty.to(gpu), 0, 5), outs['uyvy422']), f
            assert torch.equal(ing.frames(dirty.view(torch.int16).to(gpu), 0, 5), outs['uyvy422']), f            # int16 is read as the same bits


@pytest.mark.parametrize('pix_fmt', ['uyvy422', 'yuyv422', 'y210', 'nv16', 'p210'])
@pytest.mark.parametrize('H, W', SIZES)
def test_422_pitched_surface(gpu, H, W, pix_fmt):
    """A frame inside a 512-column surface filled with a value that would show, read in place as a non-contiguous view: equal to the contiguous frame."""
    bits = _bits(pix_fmt)
    planes, _, cs, full, loc, _ = _case(H, W, bits)
    src = Y.pack(planes, pix_fmt)
    buf = torch.full((5, src.shape[1], 512, *src.shape[3:]), 255 if bits == 8 else 0xffff, dtype=torch.int32).to(src.dtype)
    buf[:, :, :W] = src
    view = buf.to(gpu)[:, :, :W]
    assert not view.is_contiguous() and view.shape == src.shape
    ing = _ingest(gpu, H, W, pix_fmt, cs, full, loc)
    want = ing.frames(src.to(gpu), 0, 5)
    assert torch.equal(ing.frames(view, 0, 5), want)
    if src.dim() == 4:                                                           # a packed frame that starts one column into the surface: 2 bytes (8-bit: every row
        buf[:, :, 1:W + 1] = src                                                 # off the 4-byte grid, so the strided loads serve it) or 4 bytes (y210: no 16-byte loads)
        assert torch.equal(ing.frames(buf.to(gpu)[:, :, 1:W + 1], 0, 5), want)
    if pix_fmt == 'nv16':                                                        # the planar arrays have no pitch to give
        with pytest.raises(ValueError, match='contiguous rows'):
            _ingest(gpu, H, W, 'yuv422p', cs, full, loc).frames(view, 0, 5)


@pytest.mark.parametrize('H, W', SIZES)
def test_planes_against_the_rgb_kernel(gpu, H, W):
    """csc = identity, zero offsets: the three output channels are the three resized planes, and each equals ops.ingest_video - the kernel the recorded digests
    pin - on that plane with that plane's tables.  A 4:2:2 layout of each staging form, and a 4:4:4 planar layout (Hc = H, Wc = W, the luma tables for chroma)."""
    from synchformer_amd import ops
    from synchformer_amd.ingest import PlaneLayout, plane_layout
    planes, _, cs, full, loc, _ = _case(H, W, 8)
    ing = _ingest(gpu, H, W, 'uyvy422', cs, full, loc)
    pick = torch.tensor(Y.TABLE, dtype=torch.int32, device=gpu)
    eye = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]
    Yp, U, V = (p.to(torch.uint8).to(gpu) for p in planes)
    luma = ops.ingest_video(torch.stack([Yp, Yp, Yp], 1), False, pick, ing.y_first, ing.y_w, ing.x_first, ing.x_w)
    chroma = ops.ingest_video(torch.stack([U, V, U], 1), False, pick, ing.cy_first, ing.cy_w, ing.cx_first, ing.cx_w)
    for pix_fmt in FMTS8:
        raw = Y.pack(planes, pix_fmt).to(gpu)
        got = ops.ingest_video_planes(raw, plane_layout(pix_fmt, H, W, raw.stride()), pick, *_tabs(ing), eye)
        assert torch.equal(got[:, 0], luma[:, 0]) and torch.equal(got[:, 1], chroma[:, 0]) and torch.equal(got[:, 2], chroma[:, 1]), pix_fmt
    g = torch.Generator().manual_seed(H * W)
    full3 = torch.randint(0, 256, (5, 3, H, W), generator=g, dtype=torch.uint8).to(gpu)                  # 4:4:4 planar: (n, 3 H, W)
    L = PlaneLayout(1, H, W, H, W, 3 * H * W, 0, W, 1, H * W, 2 * H * W, W, 1, 0)
    got = ops.ingest_video_planes(full3.reshape(5, 3 * H, W), L, pick, ing.y_first, ing.y_w, ing.x_first, ing.x_w, ing.y_first, ing.y_w, ing.x_first, ing.x_w, eye)
    assert torch.equal(got, ops.ingest_video(full3, False, pick, ing.y_first, ing.y_w, ing.x_first, ing.x_w))


@pytest.mark.parametrize('H, W', [(270, 480), (270, 202)])
def test_planes_serve_the_420_layouts(gpu, H, W):
    """ops.ingest_video_planes on the nv12, yuv420p, p010 and yuv420p10le layouts against ops.ingest_video_yuv / ops.ingest_video_yuv16 on the same frames (4:2:0
    takes an even H: 270 x 202 stands in for 271 x 202 and keeps the chroma width of 101)."""
    import ingest_yuv16_oracle as Y16
    import ingest_yuv_oracle as Y8
    from synchformer_amd import ops
    from synchformer_amd.ingest import RecordingIngest, plane_layout
    pick = torch.tensor(Y.TABLE, dtype=torch.int32, device=gpu)
    for pix_fmt in ('nv12', 'yuv420p', 'p010', 'yuv420p10le'):
        ing = RecordingIngest(gpu, 25, (H, W), 16000, pix_fmt=pix_fmt, chroma_loc='topleft')
        if pix_fmt in Y16.FMTS:
            raw = Y16.pack(*Y16.random_planes(5, H, W, H + W), pix_fmt).to(gpu)
            want = ops.ingest_video_yuv16(raw, pix_fmt, pick, *_tabs(ing), ing.csc)
        else:
            raw = Y8.pack(*Y8.random_planes(5, H, W, H + W), pix_fmt).to(gpu)
            want = ops.ingest_video_yuv(raw, pix_fmt, pick, *_tabs(ing), ing.csc)
        got = ops.ingest_video_planes(raw, plane_layout(pix_fmt, H, W, raw.stride()), pick, *_tabs(ing), ing.csc)
        assert torch.equal(got, want), pix_fmt


# ---- 4. border ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pix_fmt', ['uyvy422', 'yuv422p10le'])
@pytest.mark.parametrize('H, W', SIZES)
def test_422_border(gpu, H, W, pix_fmt):
    """resize_side = 224: the crop is the whole short side, so the first and last output rows (columns) use filter rows clamped at the edge of both planes."""
    planes, ref, cs, full, loc, _ = _case(H, W, _bits(pix_fmt), 224)
    ing = _ingest(gpu, H, W, pix_fmt, cs, full, loc, resize_side=224)
    assert min(ing.y0, ing.x0) == 0 and int(min(ing.y_first.min(), ing.x_first.min())) == 0 and int(min(ing.cy_first.min(), ing.cx_first.min())) == 0
    got = ing.frames(Y.pack(planes, pix_fmt).to(gpu), 0, 5)
    torch.cuda.synchronize()
    Y.check_pixels(got, ref[Y.TABLE], f'{H} x {W} {pix_fmt} resize_side 224')


# ---- 5. colours -----------------------------------------------------------------------------------------------------------------------------------------------------
def _constant(gpu, yuv, pix_fmt, cs='bt601', full=False):
    from synchformer_amd.ingest import RecordingIngest
    planes = [torch.full((1, 256, w), v, dtype=torch.int32) for w, v in zip((256, 128, 128), yuv)]
    ing = RecordingIngest(gpu, 25, (256, 256), 16000, pix_fmt=pix_fmt, colorspace=cs, full_range=full)
    out = ing.frames(Y.pack(planes, pix_fmt).to(gpu), 0, 1).cpu()
    assert all(bool((out[0, c] == out[0, c, 0, 0]).all()) for c in range(3))    # the resize of a constant is the constant
    return out[0, :, 0, 0].int().tolist()


def test_422_colour_known_answers(gpu):
    """Uniform frames, so only the matrix is at work.  uyvy422: the published 8-bit BT.601 triples of black, white and the primaries; y210: the BT.709 primaries
    on the 10-bit limited scale, their codes computed here from Kr, Kb (Y = 64 + 876 Y', C = 512 + 896 C', rounded to a code); all within 1 level.  The ends of the
    full-range grey axis come out exactly."""
    assert _constant(gpu, (16, 128, 128), 'uyvy422') == [0, 0, 0]
    assert _constant(gpu, (235, 128, 128), 'uyvy422') == [255, 255, 255]
    for yuv, rgb in (((81, 90, 240), (255, 0, 0)), ((145, 54, 34), (0, 255, 0)), ((41, 240, 110), (0, 0, 255))):
        got = _constant(gpu, yuv, 'uyvy422')
        print(f'uyvy422 bt601 limited {yuv} -> {got} (published {rgb})')
        assert max(abs(a - b) for a, b in zip(got, rgb)) <= 1, (yuv, got)
    kr, kb = 0.2126, 0.0722
    for rgb in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        y = kr * rgb[0] + (1 - kr - kb) * rgb[1] + kb * rgb[2]
        yuv = (round(64 + 876 * y), round(512 + 896 * (rgb[2] - y) / (2 * (1 - kb))), round(512 + 896 * (rgb[0] - y) / (2 * (1 - kr))))
        got = _constant(gpu, yuv, 'y210', 'bt709')
        print(f'y210 bt709 limited {yuv} -> {got} (primary {rgb})')
        assert max(abs(a - 255 * b) for a, b in zip(got, rgb)) <= 1, (yuv, got)
    for cs in ('bt601', 'bt709'):
        assert _constant(gpu, (0, 128, 128), 'uyvy422', cs, True) == [0, 0, 0] and _constant(gpu, (255, 128, 128), 'uyvy422', cs, True) == [255, 255, 255]
        assert _constant(gpu, (0, 512, 512), 'y210', cs, True) == [0, 0, 0] and _constant(gpu, (1023, 512, 512), 'y210', cs, True) == [255, 255, 255]


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------------------------------------------
T25, N16 = 136, 86400                                                            # 16 video segments, 15 audio segments -> 15 segments, 2 windows


@pytest.fixture(scope='module')
def rec(gpu):
    """One engine (synthetic weights, seg_chunk = 4), one grey recording at 25 fps, 256 x 256, 16 kHz: random luma, and its track as the RGB recording (Y, Y, Y)
    through the rgb24 path - computed once, read-only."""
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


def _grey(luma, pix_fmt):
    mid = torch.full((luma.shape[0], 256, 128), 128, dtype=torch.int32)
    k = 4 if pix_fmt in Y.FMTS_16 else 1
    return Y.pack([k * luma.int(), k * mid, k * mid], pix_fmt)


def _grey_ingest(gpu, pix_fmt, fps=25):
    """Full range, U = V = mid: the matrix is the identity on the grey axis.  y210 holds 4 v8, so its matrix is the 8-bit full-range one / 4 on offsets x 4
    (the 10-bit full-range matrix maps 1023, not 1020, to 255)."""
    from synchformer_amd.ingest import RecordingIngest, csc_matrix
    M, off = csc_matrix('bt601', True)
    return RecordingIngest(gpu, fps, (256, 256), 16000, pix_fmt=pix_fmt, full_range=True, csc=(M / 4, off * 4) if pix_fmt in Y.FMTS_16 else None)


@pytest.mark.parametrize('pix_fmt', ['uyvy422', 'y210'])
def test_422_grey_identity_and_track(gpu, rec, pix_fmt):
    """The 256 x 256 luma resize is the identity, so frames() is the centre crop of Y in all three channels, bit for bit, and the track of the 4:2:2 recording is
    the track of the RGB recording (Y, Y, Y), from the device and from pinned host memory."""
    from synchformer_amd.frontend import recording_geometry
    luma = rec['luma']
    raw = _grey(luma, pix_fmt)
    ing = _grey_ingest(gpu, pix_fmt)
    got = ing.frames(raw.to(gpu), 0, T25).cpu()
    assert all(torch.equal(got[:, c], luma[:, 16:240, 16:240]) for c in range(3))
    geo = recording_geometry(T25, N16)
    assert (geo['n_segments'], geo['n_windows']) == (15, 2)
    ref = rec['ref']
    for frames, wave in ((raw.to(gpu), rec['wave'].to(gpu)), (raw.pin_memory(), rec['wave'].pin_memory())):        # device, pinned host
        tr = rec['tracker'].track_raw(frames, wave, ing)
        assert tr.n_segments == 15 and tr.logits.shape == (2, 21)
        assert torch.equal(tr.logits, ref.logits), (tr.logits - ref.logits).abs().max().item()
        assert torch.equal(tr.cls_raw, ref.cls_raw) and torch.equal(tr.cls_path, ref.cls_path)


def test_422_stream_is_the_recording(gpu, rec):
    """The same frames repeated to 50 fps, pushed through RecordingIngest.stream() in ragged chunks, empty pushes included, then flush(): the concatenated output is
    frames(raw_all, 0, n), bit for bit."""
    raw = _grey(rec['luma'], 'uyvy422').repeat_interleave(2, 0)
    ing = _grey_ingest(gpu, 'uyvy422', fps=50)
    n = ing.n_frames(raw.shape[0])
    assert n == T25 + 1                                                          # slot j shows source frame 2 j; the last source frame lands on a slot of its own
    whole = ing.frames(raw.to(gpu), 0, n)
    st, outs, i = ing.stream(), [], 0
    for step in (1, 0, 7, 2, 0, 31, 64, 1, 3, 100, 0, 17, 1000):
        f, _ = st.push(raw[i:i + step] if step else None if i % 2 else raw[:0], None)
        outs.append(f)
        i = min(i + step, raw.shape[0])
    assert i == raw.shape[0]
    outs.append(st.flush()[0])
    got = torch.cat(outs)
    assert got.shape == whole.shape and torch.equal(got, whole)
    assert torch.equal(whole.cpu()[:T25, 1], rec['luma'][:, 16:240, 16:240])


# ---- 7. error paths -------------------------------------------------------------------------------------------------------------------------------------------------
def test_422_error_paths(gpu):
    from synchformer_amd import ops
    from synchformer_amd.ingest import RecordingIngest, plane_layout
    ing = RecordingIngest(gpu, 25, (256, 256), 16000, pix_fmt='uyvy422')
    tabs = _tabs(ing)
    pick = torch.zeros(1, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError, match='raw frames'):                          # an NV16-shaped frame, uyvy422 declared
        ing.frames(torch.zeros(4, 512, 256, dtype=torch.uint8, device=gpu), 0, 1)
    with pytest.raises(ValueError, match='raw frames'):                          # 16-bit words, 8-bit declared
        ing.frames(torch.zeros(4, 256, 256, 2, dtype=torch.uint16, device=gpu), 0, 1)
    with pytest.raises(ValueError, match=r'inner strides \(2, 1\)'):             # every other column of a wider frame: the macropixels are torn
        ing.frames(torch.zeros(4, 256, 512, 2, dtype=torch.uint8, device=gpu)[:, :, ::2], 0, 1)
    with pytest.raises(ValueError, match=r'inner strides \(2, 1\)'):
        ing.frames(torch.zeros(4, 256, 2, 256, dtype=torch.uint8, device=gpu).transpose(2, 3), 0, 1)
    with pytest.raises(ValueError, match='even W'):                              # odd W has no 4:2:2 layout
        ops.ingest_video_planes(torch.zeros(1, 256, 255, 2, dtype=torch.uint8, device=gpu), plane_layout('uyvy422', 256, 255), pick, *tabs, ing.csc)
    with pytest.raises(ValueError, match='even W'):
        RecordingIngest(gpu, 25, (256, 255), 16000, pix_fmt='uyvy422')
    raw = torch.zeros(1, 256, 256, 2, dtype=torch.uint8, device=gpu)
    L = plane_layout('uyvy422', 256, 256)
    with pytest.raises(ValueError, match='expected uint8'):
        ops.ingest_video_planes(raw.view(torch.int16), L, pick, *tabs, ing.csc)
    with pytest.raises(ValueError, match='reaches byte'):                        # a layout larger than the tensor is refused on the host
        ops.ingest_video_planes(raw[:, :255], L, pick, *tabs, ing.csc)
    with pytest.raises(RuntimeError, match='chroma planes'):                     # what the launcher refuses arrives as a RuntimeError with its message
        ops.ingest_video_planes(raw, L._replace(H=128, Hc=256), pick, *tabs, ing.csc)
    with pytest.raises(RuntimeError, match='device tensor'):                     # a CPU tensor handed to the op itself
        ops.ingest_video_planes(raw.cpu(), L, pick, *tabs, ing.csc)
    empty = ops.ingest_video_planes(raw, L, torch.zeros(0, dtype=torch.int32, device=gpu), *tabs, ing.csc)
    assert empty.shape == (0, 3, 224, 224)
