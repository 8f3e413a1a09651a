"""GPU: ingest of interlaced recordings.  sf_ingest_video_fields / sf_ingest_video_yuv_planes_fields through RecordingIngest(field_order=) against the
float64 oracle of tests/ingest_fields_oracle.py under the pixel bar of test_ingest_gpu.py; pitched surfaces and the seven 4:2:2 layouts bit for bit; constant fields
that show which field was picked; a still picture against the progressive ingest (the siting's sign); recorded digests; IngestStream against frames(); and
OffsetTracker.track_raw / .stream / the pool on an interlaced recording."""
import dataclasses
import functools
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, 'golden')]
import ingest_fields_oracle as F  # noqa: E402
import make_ingest_fields_digests as D  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(270, 480), (480, 202)]
LAYOUTS = ('rgb_planar', 'rgb_channels_last') + F.FMTS
PARITY = [(H, W, k, o) for H, W in SIZES for k in LAYOUTS for o in F.ORDERS] + [(1080, 1920, k, o) for k in ('uyvy422', 'y210') for o in F.ORDERS]


def _fmt(layout):
    return ('rgb24', layout == 'rgb_channels_last') if layout.startswith('rgb') else (layout, False)


@functools.lru_cache(maxsize=None)
def _ref(H, W, kind, order):
    """The float64 oracle of a case - kind 'rgb', 8 or 10 (bits of the 4:2:2 planes) - computed once, read-only: (uint8 (5, 3, 224, 224), share outside [0, 255])."""
    cs, full, loc, _, _ = F.CASES[(H, W)]
    Hr, Wr, y0, x0 = F.origin(H, W)
    if kind == 'rgb':
        return F.oracle_rgb(F.rgb_frames(H, W), order, F.TABLE, (Hr, Wr), y0, x0), 0.0
    return F.oracle_yuv(F.yuv_planes(H, W, kind), order, F.TABLE, (Hr, Wr), y0, x0, *F.matrix(cs, full, kind), loc)


# ---- 1. oracle parity ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H, W, layout, order', PARITY)
def test_fields_match_oracle(gpu, H, W, layout, order):
    """The field pick [0, 1, 1, 4, 7] over 4 frames: both parities, a repeat and a skip.  (270, 480): a field of 135 rows; (480, 202): portrait, the field is upscaled
    vertically, chroma width 101 - packed rows and chroma rows start unaligned; (1080, 1920): wide-row chunks, 11 vertical taps, the halved staging of y210."""
    pix_fmt, cl = _fmt(layout)
    ing = D.ingest(gpu, H, W, pix_fmt, order, cl)
    assert (ing.taps_y, ing.taps_x) == F.CASES[(H, W)][3] and ing.interlaced
    raw = D.raw_frames(H, W, pix_fmt, cl)
    ref, outside = _ref(H, W, 'rgb' if pix_fmt == 'rgb24' else 10 if pix_fmt in F.FMTS_16 else 8, order)
    got = ing.frames(raw.to(gpu), 0, 5)
    torch.cuda.synchronize()
    F.check_pixels(got, ref, f'{H} x {W} {layout} {order} taps {ing.taps_y} x {ing.taps_x}, {outside:.0%} outside [0, 255] before the clamp')
    assert torch.equal(ing.frames(raw, 0, 5), got)                               # from the host: the frames that hold fields 0 .. 7
    assert torch.equal(ing.frames(raw, 3, 5), got[3:5])                          # fields 4 and 7: source frames 2 and 3 only


# ---- 2. bit for bit -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', F.ORDERS)
@pytest.mark.parametrize('pix_fmt', ['uyvy422', 'nv16'])
def test_fields_pitched_surface(gpu, pix_fmt, order):
    """A row pitch of 2 bytes beyond a multiple of 4: the rows of the bottom field (odd frame rows) start 2 bytes off the 4-byte grid, those of the top field on it,
    so the packed and the interleaved fetches serve one parity and the per-sample loads the other.  Bit-equal to the contiguous copy, at both sizes."""
    for H, W in SIZES:
        src = D.raw_frames(H, W, pix_fmt)
        pad = 1 if pix_fmt == 'uyvy422' else 4 - W % 4 + 2 if W % 4 else 2        # uyvy422: one more column of two bytes; nv16: a pitch of 2 (mod 4) bytes
        buf = torch.full((4, src.shape[1], W + pad, *src.shape[3:]), 255, dtype=torch.uint8)
        buf[:, :, :W] = src
        view = buf.to(gpu)[:, :, :W]
        pitch = view.stride(1)                                                   # elements are bytes
        assert not view.is_contiguous() and pitch % 4 == 2, pitch
        ing = D.ingest(gpu, H, W, pix_fmt, order)
        assert torch.equal(ing.frames(view, 0, 5), ing.frames(src.to(gpu), 0, 5)), (H, W)


@pytest.mark.parametrize('order', F.ORDERS)
@pytest.mark.parametrize('H, W', SIZES)
def test_field_layouts_agree(gpu, H, W, order):
    """The same planes in the seven 4:2:2 packings (the 10-bit ones holding 4 v8, limited range: their matrix is the 8-bit one / 4 exactly): identical bytes."""
    planes = F.yuv_planes(H, W, 8)
    cs, _, loc, _, _ = F.CASES[(H, W)]
    from synchformer_amd.ingest import RecordingIngest
    outs = {}
    for f in F.FMTS:
        ing = RecordingIngest(gpu, 25, (H, W), 16000, pix_fmt=f, colorspace=cs, full_range=False, chroma_loc=loc, field_order=order)
        ing._tables = {4: torch.tensor(F.TABLE, dtype=torch.int32)}
        outs[f] = ing.frames(F.pack([4 * p for p in planes] if f in F.FMTS_16 else planes, f).to(gpu), 0, 5)
    for f in F.FMTS[1:]:
        assert torch.equal(outs[f], outs['uyvy422']), f


# ---- 3. which field ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels_last', [False, True])
def test_the_pick_is_the_fields(gpu, channels_last):
    """6 frames at 30000/1001 = 12 fields; every row of the f-th field in top-field-first order holds the constant 10 f.  'tff': output j is 10 table[j] exactly;
    'bff' on the same frames shows the other field of the same frame, 10 (table[j] ^ 1).  Any mix-up of order, parity or row offset shows."""
    from synchformer_amd.ingest import RecordingIngest
    H, W = 270, 480
    raw = torch.zeros(6, 3, H, W, dtype=torch.uint8)
    for f in range(12):
        raw[f >> 1, :, f & 1::2] = 10 * f
    raw = raw.permute(0, 2, 3, 1).contiguous() if channels_last else raw
    table = [1, 3, 5, 8, 10, 11]
    for order, want in (('tff', table), ('bff', [f ^ 1 for f in table])):
        ing = RecordingIngest(gpu, (30000, 1001), (H, W), 16000, channels_last=channels_last, field_order=order)
        assert ing.frame_table(6).tolist() == table
        got = ing.frames(raw.to(gpu), 0, 6).cpu()
        for j, f in enumerate(want):
            assert bool((got[j] == 10 * f).all()), (order, j, f, got[j].unique().tolist())


@pytest.mark.parametrize('H, W', [(270, 480), (1080, 1920)])
def test_still_picture_matches_progressive(gpu, H, W):
    """round(128 + 100 sin(2 pi 3 (y + 1/2) / H) cos(2 pi (x + 1/2) / W)) as grey rgb24 and as full-range uyvy422 with neutral chroma: every field, either order,
    ingested on its own is within 2 levels of the progressive ingest of the frame - the float64 restatement gives at most 1 here and the kernel may add 1; the
    opposite siting sign is 8 levels off at (270, 480)."""
    from synchformer_amd.ingest import RecordingIngest
    pic = F.still(H, W)
    rgb = pic[None, None].expand(3, 3, H, W).contiguous()
    mid = torch.full((3, H, W // 2), 128, dtype=torch.int32)
    uyvy = F.pack([pic[None].expand(3, H, W).int(), mid, mid], 'uyvy422')
    for raw, kw in ((rgb, {}), (uyvy, dict(pix_fmt='uyvy422', full_range=True))):
        prog = RecordingIngest(gpu, 25, (H, W), 16000, **kw).frames(raw.to(gpu), 0, 3).cpu().int()
        assert torch.equal(prog[0], prog[2]) and int(prog.max()) > 200 and int(prog.min()) < 56
        for order in F.ORDERS:
            ing = RecordingIngest(gpu, 25, (H, W), 16000, field_order=order, **kw)
            ing._tables = {3: torch.arange(6, dtype=torch.int32)}                # every field: both parities
            got = ing.frames(raw.to(gpu), 0, 6).cpu().int()
            d = (got - prog[:1]).abs().amax((1, 2, 3)).tolist()
            print(f'{H} x {W} {kw.get("pix_fmt", "rgb24")} {order}: max |field - progressive| per field {d}')
            assert max(d) <= 2, d
            assert torch.equal(got[0], got[2]) and torch.equal(got[1], got[3])


# ---- 4. digests ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_digest_cases_are_oracle_cases():
    """Every recorded case is one that test_fields_match_oracle holds to the oracle."""
    names = {f'{"rgb_planar" if k == "rgb_planar" else k}_{H}x{W}_{o}' for H, W, k, o in PARITY}
    assert set(D.CASES) <= names and len(D.CASES) >= 10


@pytest.mark.parametrize('name', list(D.CASES))
def test_field_outputs_are_pinned(gpu, name):
    """The output bytes of the field kernels against the SHA-256 recorded once (tests/golden/ingest_fields_digests.json): a later change of the summation order or of
    the addressing that the one-level pixel bar would pass.  The input's own digest is checked first: a mismatch there is a changed random stream."""
    with open(os.path.join(HERE, 'golden', 'ingest_fields_digests.json')) as f:
        digests = json.load(f)['cases']
    assert set(digests) == set(D.CASES)
    src, out = D.CASES[name](gpu)
    torch.cuda.synchronize()
    assert D.sha256(src) == digests[name]['input'], f'{name}: the generated INPUT differs from the recorded one'
    assert D.sha256(out) == digests[name]['output'], f'{name}: the output bytes differ from the recorded ones'


# ---- 5. stream -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_streamed_fields_equal_offline(gpu):
    """41 uyvy422 frames at 30000/1001, top field first, pushed in ragged chunks - an empty push, a None and one-frame pushes among them - then flush(): the output is
    frames(raw, 0, n) bit for bit, and never more than one source frame is held."""
    from synchformer_amd.ingest import RecordingIngest
    n, H, W = 41, 270, 480
    raw = torch.randint(0, 256, (n, H, W, 2), generator=torch.Generator().manual_seed(18), dtype=torch.uint8)
    ing = RecordingIngest(gpu, (30000, 1001), (H, W), 16000, pix_fmt='uyvy422', field_order='tff')
    n_out = ing.n_frames(n)
    table = ing.frame_table(n)
    assert n_out == 35 and {int(f) & 1 for f in table} == {0, 1}
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


# ---- 6. tracker ----------------------------------------------------------------------------------------------------------------------------------------------------
N_SRC, N16 = 165, 86400                                                          # 165 frames at 30000/1001 -> 138 frames at 25 fps: 16 video segments; 15 audio segments


@pytest.fixture(scope='module')
def rec(gpu):
    """One engine (synthetic weights, seg_chunk = 4), one interlaced uyvy422 recording of 256 x 256 at 30000/1001 with 16 kHz sound, its ingest, the 25 fps frames
    ingested beforehand and their track - computed once, read-only."""
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    from synchformer_amd.ingest import RecordingIngest
    from synchformer_amd.track import OffsetTracker
    tracker = OffsetTracker(SynchformerEngine(synth.make_state_dict(1337), gpu, seg_chunk=4), MelFrontend(gpu))
    raw = torch.randint(0, 256, (N_SRC, 256, 256, 2), generator=torch.Generator().manual_seed(79), dtype=torch.uint8)
    wave = synth.make_wave(1, 1, 79, n=N16).reshape(N16)
    ing = RecordingIngest(gpu, (30000, 1001), (256, 256), 16000, pix_fmt='uyvy422', field_order='tff')
    frames = ing.frames(raw.to(gpu), 0, ing.n_frames(N_SRC))
    ref = tracker.track(frames, wave.to(gpu))
    torch.cuda.synchronize()
    return dict(tracker=tracker, raw=raw, wave=wave, ing=ing, frames=frames, ref=ref)


def test_track_raw_on_an_interlaced_recording(gpu, rec):
    """track_raw only goes through RecordingIngest: with an interlaced ingest its logits are those of track() on the frames ingested beforehand."""
    assert rec['frames'].shape[0] == 138 and rec['ref'].logits.shape == (2, 21)
    for frames, wave in ((rec['raw'].to(gpu), rec['wave'].to(gpu)), (rec['raw'], rec['wave'])):
        tr = rec['tracker'].track_raw(frames, wave, rec['ing'])
        assert tr.n_segments == 15 and torch.equal(tr.logits, rec['ref'].logits), (tr.logits - rec['ref'].logits).abs().max().item()
        assert torch.equal(tr.cls_raw, rec['ref'].cls_raw) and torch.equal(tr.cls_path, rec['ref'].cls_path)


def test_pool_feed_equals_stream_on_an_interlaced_feed(gpu, rec):
    """One feed of an OffsetStreamPool opened with the interlaced ingest against tracker.stream(ingest=) on the same pushes, update for update; the logits are the
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


# ---- 7. error paths ------------------------------------------------------------------------------------------------------------------------------------------------
def test_field_error_paths(gpu):
    from synchformer_amd import ops
    from synchformer_amd.ingest import RecordingIngest, plane_layout
    pick = torch.zeros(1, dtype=torch.int32, device=gpu)
    wide = (torch.zeros(224, dtype=torch.int32, device=gpu), torch.zeros(224, 36, device=gpu))
    rgb = RecordingIngest(gpu, 25, (256, 256), 16000, field_order='tff')
    raw = torch.zeros(1, 3, 256, 256, dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError, match=r'sf_ingest_video_fields: 36 filter taps out of range'):      # what the launcher refuses arrives with its message
        ops.ingest_video_fields(raw, False, pick, (wide, wide), rgb.x_first, rgb.x_w, False)
    with pytest.raises(RuntimeError, match=r'sf_ingest_video_fields: 36 filter taps out of range'):
        ops.ingest_video_fields(raw, False, pick, rgb.y_tables, *wide, False)
    with pytest.raises(ValueError, match='even H'):
        ops.ingest_video_fields(raw[:, :, :255], False, pick, rgb.y_tables, rgb.x_first, rgb.x_w, False)
    with pytest.raises(RuntimeError, match='device tensor'):
        ops.ingest_video_fields(raw.cpu(), False, pick, rgb.y_tables, rgb.x_first, rgb.x_w, False)
    with pytest.raises(ValueError, match='raw frames'):                          # fields handed over as frames
        rgb.frames(raw[:, :, ::2], 0, 1)
    ing = RecordingIngest(gpu, 25, (256, 256), 16000, pix_fmt='y210', field_order='bff')
    L = plane_layout('y210', 256, 256)
    raw = torch.zeros(1, 256, 256, 2, dtype=torch.uint16, device=gpu)
    with pytest.raises(RuntimeError, match=r'sf_ingest_video_yuv_planes_fields: 36 filter taps out of range'):
        ops.ingest_video_planes_fields(raw, L, pick, ing.y_tables, ing.x_first, ing.x_w, (wide, wide), ing.cx_first, ing.cx_w, ing.csc, True)
    with pytest.raises(RuntimeError, match=r'sf_ingest_video_yuv_planes_fields: shift = 9'):
        ops.ingest_video_planes_fields(raw, L._replace(shift=9), pick, ing.y_tables, ing.x_first, ing.x_w, ing.y_tables, ing.cx_first, ing.cx_w, ing.csc, True)
    with pytest.raises(ValueError, match='chroma planes of H rows'):
        ops.ingest_video_planes_fields(raw, L._replace(Hc=128), pick, ing.y_tables, ing.x_first, ing.x_w, ing.y_tables, ing.cx_first, ing.cx_w, ing.csc, True)
    empty = ops.ingest_video_planes_fields(raw, L, pick[:0], ing.y_tables, ing.x_first, ing.x_w, ing.y_tables, ing.cx_first, ing.cx_w, ing.csc, True)
    assert empty.shape == (0, 3, 224, 224)
    assert ops.ingest_video_fields(torch.zeros(1, 3, 256, 256, dtype=torch.uint8, device=gpu), False, pick[:0], rgb.y_tables, rgb.x_first, rgb.x_w, True).shape[0] == 0
