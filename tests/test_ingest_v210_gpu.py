"""GPU: ingest of v210 frames.  sf_ingest_video_v210 / sf_ingest_video_v210_fields through RecordingIngest(pix_fmt='v210') and the two ops: bit for bit
against the yuv422p10le path on the same samples (the defining property), against the float64 oracle of tests/ingest_yuv422_oracle.py / ingest_fields_oracle.py on
the unpacked planes under the project's pixel bar, with garbage in every bit the format leaves unused, at the ends of the tap and width range, on fields, and through
IngestStream, OffsetTracker.track_raw, .stream and the pool."""
import dataclasses
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_fields_oracle as F  # noqa: E402
import ingest_v210_oracle as V  # noqa: E402

pytestmark = pytest.mark.gpu

# (270, 480): W % 12 == 0; (271, 202): odd H, W % 6 == 4, chroma width 101; (144, 176): W % 6 == 2, both planes upscale; (540, 958): W % 12 == 10, taps 11 / 7;
# (480, 202): portrait, the row is upscaled.  Between them: chroma_loc 'left' and 'center', bt601 limited and bt709 full (V.CASES).
SIZES = [(270, 480), (271, 202), (144, 176), (540, 958), (480, 202)]
# The share of pre-clamp values outside [0, 255] that ingest_yuv422_oracle.oracle returns for the 10-bit planes of test_ingest_yuv422_gpu._case (5 frames of
# random_planes(seed H 10000 + W + 256 + 10), the case's matrix and siting) - computed on the CPU with that oracle when this test was written.  The fourth case of
# ingest_yuv422_oracle.CASES, (540, 960), gives 0.05929660926870748; the largest of the four is (144, 176)'s, the bound for the two widths that are not in CASES.
OUTSIDE_422 = {(270, 480): 0.26607940051020407, (271, 202): 0.2199484481292517, (144, 176): 0.28113174957482995}
OUTSIDE_MAX = 0.28113174957482995


def _words(shape, seed):
    """Uniform random 32-bit words, int32: a valid v210 frame (every field is some 10-bit sample, bits 30 - 31 are stray)."""
    return torch.randint(-(1 << 31), 1 << 31, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """(10-bit planes of 5 source frames - the planes test_ingest_yuv422_gpu uses at this size -, oracle uint8 (5, 3, 224, 224), colorspace, full, loc, share outside
    [0, 255]) - computed once, read-only."""
    cs, full, loc, _, _ = V.CASES[(H, W)]
    planes = V.random_planes(5, H, W, H * 10000 + W + 256 + 10, 1024)
    Hr, Wr, y0, x0 = V.origin(H, W, 256)
    ref, outside = V.oracle(planes, (Hr, Wr), y0, x0, *V.matrix(cs, full, 10), loc)
    return planes, ref, cs, full, loc, outside


def _ingest(gpu, H, W, pix_fmt, table=V.TABLE, n=5, **kw):
    from synchformer_amd.ingest import RecordingIngest
    cs, full, loc, _, _ = V.CASES[(H, W)]
    ing = RecordingIngest(gpu, 25, (H, W), 16000, pix_fmt=pix_fmt, colorspace=cs, full_range=full, chroma_loc=loc, **kw)
    ing._tables = {n: torch.tensor(table, dtype=torch.int32)}                    # the pick under test: a repeat and a skip
    return ing


@functools.lru_cache(maxsize=None)
def _want(gpu, H, W):
    """frames() of the yuv422p10le ingest on the case's planes: the kernel the v210 output has to equal (device tensor, read-only)."""
    out = _ingest(gpu, H, W, 'yuv422p10le').frames(V.pack(_case(H, W)[0], 'yuv422p10le').to(gpu), 0, 5)
    torch.cuda.synchronize()
    return out


# ---- 1. bit for bit against the existing kernel; 2. the float64 oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H, W', SIZES)
def test_v210_equals_yuv422p10le(gpu, H, W):
    """The same planes packed as v210 (conventional pitch) and as yuv422p10le: identical output bytes, with the frames on the device and in pinned host memory; a slice
    of the output reads the source frames it spans only."""
    from synchformer_amd.ingest import v210_row_words
    planes = _case(H, W)[0]
    ing = _ingest(gpu, H, W, 'v210')
    assert ((ing.taps_y, ing.taps_x), (ing.taps_cy, ing.taps_cx)) == V.CASES[(H, W)][3:]
    raw = V.pack_v210(planes, v210_row_words(W))
    assert raw.shape == (5, H, 32 * ((W + 47) // 48)) and raw.dtype == torch.int32
    want = _want(gpu, H, W)
    for where in (raw.to(gpu), raw.pin_memory(), raw.view(torch.uint32).to(gpu)):
        got = ing.frames(where, 0, 5)
        assert torch.equal(got, want), (got.int() - want.int()).abs().max().item()
    assert torch.equal(ing.frames(raw, 2, 5), want[2:5])


@pytest.mark.parametrize('H, W', SIZES)
def test_v210_matches_oracle(gpu, H, W):
    """The project's pixel bar (every pixel within 1 level, at most 1e-3 of them different) against the float64 oracle on the planes; the share of oracle values outside
    [0, 255] before the clamp is the one the yuv422p10le test meets at this size, or - the two widths that test does not have - below the largest of its four."""
    planes, ref, cs, full, loc, outside = _case(H, W)
    print(f'{H} x {W}: {outside!r} of the oracle values outside [0, 255] before the clamp')
    if (H, W) in OUTSIDE_422:
        assert outside == OUTSIDE_422[(H, W)]
    else:
        assert outside < OUTSIDE_MAX
    got = _ingest(gpu, H, W, 'v210').frames(V.pack_v210(planes).to(gpu), 0, 5)
    torch.cuda.synchronize()
    V.check_pixels(got, ref[V.TABLE], f'{H} x {W} v210 {cs} {"full" if full else "limited"} {loc}, {outside:.0%} outside [0, 255] before the clamp')


# ---- 3. padding and stray bits ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H, W', [(271, 202), (144, 176), (270, 480)])
def test_v210_padding_and_stray_bits(gpu, H, W):
    """Whatever the format leaves unused never reaches the output: padding words and the unused fields of the last group (W % 6 == 4, 2; 0 has only the padding) full of
    ones, bits 30 - 31 set in every word, the conventional and the minimal pitch, a pitch of one word more than minimal - rows 4 bytes off the 16-byte grid from row 1
    on: only the 4-byte alignment the format guarantees -, and a view that skips every other frame: each is the output of the clean frames."""
    from synchformer_amd.ingest import v210_row_words
    planes = _case(H, W)[0]
    ing = _ingest(gpu, H, W, 'v210')
    need, conv = V.min_words(W), v210_row_words(W)
    want = _want(gpu, H, W)
    clean = V.pack_v210(planes, need, 0)
    assert torch.equal(ing.frames(clean.to(gpu), 0, 5), want)                   # the minimal pitch
    for row_words in (conv, need + 1):
        for fill in (0, 0xffffffff):
            raw = V.pack_v210(planes, row_words, fill)
            assert (row_words * 4) % 16 == (4 if row_words == need + 1 else 0)
            assert torch.equal(ing.frames(raw.to(gpu), 0, 5), want), (row_words, fill)
    dirty = V.pack_v210(planes, need, 0xffffffff)
    assert torch.equal(dirty, clean) == (W % 6 == 0)
    assert torch.equal(ing.frames(dirty.to(gpu), 0, 5), want)
    assert torch.equal(ing.frames(V.set_stray_bits(V.pack_v210(planes, conv, 0xffffffff)).to(gpu), 0, 5), want)
    buf = _words((10, H, conv), H + W)                                          # the frames in the even slots of a buffer of random words
    buf[::2] = V.pack_v210(planes, conv, 0x12345678)
    view = buf.to(gpu)[::2]
    assert not view.is_contiguous() and view.stride(0) == 2 * H * conv
    assert torch.equal(ing.frames(view, 0, 5), want)
    view = buf.to(gpu)[::2, :, :need]                                            # and a row pitch above the row
    assert torch.equal(ing.frames(view, 0, 5), want)


# ---- 4. tile and tap edges (the ops, tables built here) --------------------------------------------------------------------------------------------------------------
def _both_ops(gpu, planes, tabs_y, tabs_x, tabs_cx, csc, pick, row_words=None):
    """ops.ingest_video_v210 and ops.ingest_video_planes on the yuv422p10le layout, on the same samples."""
    from synchformer_amd import ops
    from synchformer_amd.ingest import plane_layout
    H, W = planes[0].shape[1:]
    got = ops.ingest_video_v210(V.pack_v210(planes, row_words).to(gpu), W, pick, *tabs_y, *tabs_x, *tabs_cx, csc)
    want = ops.ingest_video_planes(V.pack(planes, 'yuv422p10le').to(gpu), plane_layout('yuv422p10le', H, W), pick, *tabs_y, *tabs_x, *tabs_y, *tabs_cx, csc)
    torch.cuda.synchronize()
    return got, want


def _tables(gpu, n_in, n_out, origin):
    from synchformer_amd.ingest import aa_bicubic_table
    first, w, taps = aa_bicubic_table(n_in, n_out)
    return (first[origin:origin + 224].contiguous().to(gpu), w[origin:origin + 224].contiguous().to(gpu)), taps


@pytest.mark.parametrize('H, W, luma, chroma_x', [(2160, 260, (35, 7), 5), (260, 2160, (7, 35), 19), (8, 2, (5, 5), 5), (8, 6, (5, 5), 5)])
def test_v210_tap_and_width_ends(gpu, H, W, luma, chroma_x):
    """An anisotropic resize to 256 x 256, crop origin 16: the ends of the tap range (35 vertical taps; 35 horizontal ones over 19 for chroma), and rows of one partial
    group (W = 2: one chroma column) and of one whole group (W = 6) - bit for bit the yuv422p10le op, at the minimal and at the conventional pitch."""
    from synchformer_amd.ingest import csc_matrix, v210_row_words
    (ty, t_y), (tx, t_x), (tcx, t_cx) = _tables(gpu, H, 256, 16), _tables(gpu, W, 256, 16), _tables(gpu, W // 2, 256, 16)
    assert ((t_y, t_x), t_cx) == (luma, chroma_x)
    M, off = csc_matrix('bt601', False, 10)
    csc = torch.cat([M.reshape(9), off]).float()
    planes = V.random_planes(2, H, W, H + W + 10, 1024)
    pick = torch.tensor([1, 0], dtype=torch.int32, device=gpu)
    for row_words in (None, v210_row_words(W)):
        got, want = _both_ops(gpu, planes, ty, tx, tcx, csc, pick, row_words)
        assert torch.equal(got, want), (row_words, (got.int() - want.int()).abs().max().item())
    assert int(want.max()) > int(want.min())


def test_v210_2160p(gpu):
    """One 2160 x 3840 frame with the tables of its RecordingIngest: 35 x 35 luma taps and the widest staged row - four 16-bit rows of 3840 + 35 columns pass the v210
    form's own staging budget, so the launcher takes the instantiation with the plain 16-bit budget.  Bit for bit the yuv422p10le op."""
    from synchformer_amd.ingest import RecordingIngest
    H, W = 2160, 3840
    ing = RecordingIngest(gpu, 25, (H, W), 16000, pix_fmt='v210', colorspace='bt709', chroma_loc='left')
    assert (ing.taps_y, ing.taps_x, ing.taps_cx) == (35, 35, 19)
    planes = V.random_planes(1, H, W, H + W, 1024)
    pick = torch.zeros(1, dtype=torch.int32, device=gpu)
    got, want = _both_ops(gpu, planes, (ing.y_first, ing.y_w), (ing.x_first, ing.x_w), (ing.cx_first, ing.cx_w), ing.csc, pick)
    assert torch.equal(got, want), (got.int() - want.int()).abs().max().item()


# ---- 5. fields -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', F.ORDERS)
@pytest.mark.parametrize('H, W', [(270, 480), (480, 202)])
def test_v210_fields(gpu, H, W, order):
    """The field pick [0, 1, 1, 4, 7] over 4 frames, both orders: v210 equals yuv422p10le with the same field_order bit for bit and meets the float64 field oracle under
    the pixel bar - at a pitch that is 16 (mod 32) bytes, so the rows of both parities keep 16-byte alignment, at one that is 4 (mod 16), so those of every frame row
    but the first lose it, and from the host."""
    from synchformer_amd.ingest import RecordingIngest
    cs, full, loc, luma, _ = F.CASES[(H, W)]
    planes = F.yuv_planes(H, W, 10)
    kw = dict(colorspace=cs, full_range=full, chroma_loc=loc, field_order=order)
    ings = {f: RecordingIngest(gpu, 25, (H, W), 16000, pix_fmt=f, **kw) for f in ('v210', 'yuv422p10le')}
    for ing in ings.values():
        ing._tables = {4: torch.tensor(F.TABLE, dtype=torch.int32)}
        assert (ing.taps_y, ing.taps_x) == luma and ing.interlaced
    want = ings['yuv422p10le'].frames(F.pack(planes, 'yuv422p10le').to(gpu), 0, 5)
    need = V.min_words(W)
    w16 = need + 4 if (4 * need) % 32 == 0 else need                             # whole groups: a multiple of 16 bytes; make it an odd multiple
    assert (4 * w16) % 32 == 16 and (4 * (need + 1)) % 16 == 4
    for row_words in (w16, need + 1):
        raw = V.pack_v210(planes, row_words, 0xffffffff)
        got = ings['v210'].frames(raw.to(gpu), 0, 5)
        assert torch.equal(got, want), (row_words, (got.int() - want.int()).abs().max().item())
    assert torch.equal(ings['v210'].frames(raw, 0, 5), want) and torch.equal(ings['v210'].frames(raw, 3, 5), want[3:5])      # fields 4 and 7: source frames 2 and 3 only
    Hr, Wr, y0, x0 = F.origin(H, W)
    ref, outside = F.oracle_yuv(planes, order, F.TABLE, (Hr, Wr), y0, x0, *F.matrix(cs, full, 10), loc)
    F.check_pixels(got, ref, f'{H} x {W} v210 {order} taps {luma}, {outside:.0%} outside [0, 255] before the clamp')


# ---- 6. stream and tracker ---------------------------------------------------------------------------------------------------------------------------------------------
def test_streamed_v210_fields_equal_offline(gpu):
    """41 v210 frames of random words at 30000/1001, top field first, pushed in ragged chunks - an empty push, a None and one-frame pushes among them - then flush(): the
    output is frames(raw, 0, n) bit for bit, and never more than one source frame is held (the test DESIGN 3.18 has for uyvy422)."""
    from synchformer_amd.ingest import RecordingIngest, v210_row_words
    n, H, W = 41, 270, 480
    raw = _words((n, H, v210_row_words(W)), 18)
    ing = RecordingIngest(gpu, (30000, 1001), (H, W), 16000, pix_fmt='v210', field_order='tff')
    n_out = ing.n_frames(n)
    assert n_out == 35 and {int(f) & 1 for f in ing.frame_table(n)} == {0, 1}
    whole = ing.frames(raw, 0, n_out)
    st, outs, i = ing.stream(), [], 0
    for step in (1, 0, 1, 7, 2, None, 13, 1, 100):
        f, _ = st.push(None if step is None else raw[i:i + step], None)
        outs.append(f)
        i = min(i + (step or 0), n)
        assert st.held['frames'] <= 1
    assert i == n
    outs.append(st.flush()[0])
    got = torch.cat(outs)
    torch.cuda.synchronize()
    assert got.shape == whole.shape and torch.equal(got, whole) and not torch.equal(whole[0], whole[1])
    st = ing.stream()                                                            # uint32 frames: the same bits
    again = torch.cat([st.push(raw[:20].view(torch.uint32), None)[0], st.push(raw[20:].view(torch.uint32), None)[0], st.flush()[0]])
    assert torch.equal(again, whole)


N_SRC, N16 = 165, 86400                                                          # 165 frames at 30000/1001 -> 138 frames at 25 fps: 16 video segments; 15 audio segments


@pytest.fixture(scope='module')
def rec(gpu):
    """One engine (synthetic weights, seg_chunk = 4), one interlaced v210 recording of 256 x 256 at 30000/1001 with 16 kHz sound - the geometry of
    test_ingest_fields_gpu.py -, its ingest, the 25 fps frames ingested beforehand and their track: computed once, read-only."""
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.ingest import RecordingIngest, v210_row_words
    from synchformer_amd.track import OffsetTracker
    tracker = OffsetTracker(SynchformerEngine(synth.make_state_dict(1337), gpu, seg_chunk=4), MelFrontend(gpu))
    raw = _words((N_SRC, 256, v210_row_words(256)), 79)
    wave = synth.make_wave(1, 1, 79, n=N16).reshape(N16)
    ing = RecordingIngest(gpu, (30000, 1001), (256, 256), 16000, pix_fmt='v210', field_order='tff')
    frames = ing.frames(raw.to(gpu), 0, ing.n_frames(N_SRC))
    ref = tracker.track(frames, wave.to(gpu))
    torch.cuda.synchronize()
    return dict(tracker=tracker, raw=raw, wave=wave, ing=ing, frames=frames, ref=ref)


def test_track_raw_on_a_v210_recording(gpu, rec):
    """track_raw only goes through RecordingIngest: its logits are those of track() on the frames ingested beforehand, from the device and from the host."""
    assert rec['frames'].shape[0] == 138 and rec['ref'].logits.shape == (2, 21)
    for frames, wave in ((rec['raw'].to(gpu), rec['wave'].to(gpu)), (rec['raw'], rec['wave'])):
        tr = rec['tracker'].track_raw(frames, wave, rec['ing'])
        assert tr.n_segments == 15 and torch.equal(tr.logits, rec['ref'].logits), (tr.logits - rec['ref'].logits).abs().max().item()
        assert torch.equal(tr.cls_raw, rec['ref'].cls_raw) and torch.equal(tr.cls_path, rec['ref'].cls_path)


def test_pool_feed_equals_stream_on_a_v210_feed(gpu, rec):
    """One feed of an OffsetStreamPool opened with the v210 ingest against tracker.stream(ingest=) on the same pushes, update for update; the logits are the
    recording's."""
    tracker, raw, wave, ing = rec['tracker'], rec['raw'], rec['wave'], rec['ing']
    pieces, f, a = [], 0, 0
    for nf, na in ((1, 0), (40, 30000), (0, 7), (63, 40000), (61, 16393)):
        pieces.append((f, f + nf, a, a + na))
        f, a = f + nf, a + na
    assert (f, a) == (N_SRC, N16)
    stream = tracker.stream(lag=2, ingest=ing)
    want = [stream.push(raw[f0:f1], wave[a0:a1]) for f0, f1, a0, a1 in pieces] + [stream.flush()]
    pool = tracker.pool(2, lag=2)
    feed = pool.open(ingest=ing)
    got = [pool.push({feed: (raw[f0:f1], wave[a0:a1])})[feed] for f0, f1, a0, a1 in pieces] + [pool.push({}, flush=[feed])[feed]]
    torch.cuda.synchronize()
    for i, (u, v) in enumerate(zip(got, want)):
        for fld in dataclasses.fields(u):
            x, y = getattr(u, fld.name), getattr(v, fld.name)
            if isinstance(x, torch.Tensor):
                assert isinstance(y, torch.Tensor) and x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (i, fld.name)
            else:
                assert x == y, (i, fld.name, x, y)
    assert torch.equal(torch.cat([u.logits for u in got]), rec['ref'].logits)


# ---- 7. error paths ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_v210_error_paths(gpu):
    """What the launcher refuses arrives as a RuntimeError with its message; an empty pick launches nothing."""
    from synchformer_amd import ops
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(gpu, 25, (256, 256), 16000, pix_fmt='v210', field_order='bff')
    raw = torch.zeros(2, 256, 192, dtype=torch.int32, device=gpu)
    pick = torch.zeros(1, dtype=torch.int32, device=gpu)
    wide = (torch.zeros(224, dtype=torch.int32, device=gpu), torch.zeros(224, 36, device=gpu))
    y, x, cx = ing.y_tables[0], (ing.x_first, ing.x_w), (ing.cx_first, ing.cx_w)
    with pytest.raises(RuntimeError, match=r'sf_ingest_video_v210: 36 filter taps out of range'):
        ops.ingest_video_v210(raw, 256, pick, *wide, *x, *cx, ing.csc)
    with pytest.raises(RuntimeError, match=r'sf_ingest_video_v210_fields: 36 filter taps out of range'):
        ops.ingest_video_v210_fields(raw, 256, pick, ing.y_tables, *x, *wide, ing.csc, True)
    with pytest.raises(ValueError, match='raw frames'):
        ing.frames(torch.zeros(2, 256, 256, 2, dtype=torch.uint16, device=gpu), 0, 1)
    assert ops.ingest_video_v210(raw, 256, pick[:0], *y, *x, *cx, ing.csc).shape == (0, 3, 224, 224)
    assert ops.ingest_video_v210_fields(raw, 256, pick[:0], ing.y_tables, *x, *cx, ing.csc, False).shape == (0, 3, 224, 224)
    out = ops.ingest_video_v210(raw[:, :, :172], 256, pick, *y, *x, *cx, ing.csc)      # the minimal row of 256 pixels inside the pitched frames
    assert out.shape == (1, 3, 224, 224)
