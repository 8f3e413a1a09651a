"""No GPU: the host side of the interlaced ingest - the field pick against the brute-force frame pick on the field recording, RecordingIngest's two
vertical tables and the sign of their siting, its argument validation, the ABI entries of the two field launchers and every refusal of theirs (before the device
is touched), the field arithmetic of IngestStream, and the margin of the pixel bar: the kernel's arithmetic restated in fp32 against the float64 oracle of
tests/ingest_fields_oracle.py."""
import ctypes
import os
import re
import sys
from fractions import Fraction

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_fields_oracle as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')


# ---- time ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fps', [25, (30000, 1001), 30, 50, 24])
def test_field_table_is_the_frame_table_of_the_field_recording(fps):
    from synchformer_amd.ingest import fps_field_table, fps_frame_table
    f = Fraction(*fps) if isinstance(fps, tuple) else Fraction(fps)
    for n in (1, 2, 7, 12):
        got = fps_field_table(n, fps)
        assert got.dtype == torch.int32 and got.tolist() == F.frame_table_bruteforce(2 * n, 2 * f), (fps, n)
        assert torch.equal(got, fps_frame_table(2 * n, 2 * f))
        assert int(got.max()) == 2 * n - 1                                       # the last field is shown
    assert fps_field_table(0, fps).numel() == 0


def test_field_table_known_picks():
    from synchformer_amd.ingest import RecordingIngest, fps_field_table
    assert fps_field_table(6, 25).tolist() == [0, 2, 4, 6, 8, 10, 11]            # 25i: the first field of every frame, and the end-of-stream slot
    assert fps_field_table(6, (30000, 1001)).tolist() == [1, 3, 5, 8, 10, 11]    # 59.94 fields / s: the parities alternate
    ing = RecordingIngest(CPU, (30000, 1001), (270, 480), 16000, field_order='bff')
    assert ing.frame_table(6).tolist() == [1, 3, 5, 8, 10, 11] and ing.n_frames(6) == 6 and ing.fps_in == Fraction(30000, 1001)
    assert RecordingIngest(CPU, (30000, 1001), (270, 480), 16000).frame_table(6).tolist() == [0, 1, 2, 4, 5]          # progressive: frames, as before


# ---- space --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H, W, pix_fmt', [(270, 480, 'rgb24'), (480, 202, 'uyvy422'), (1080, 1920, 'y210'), (1080, 1920, 'rgb24')])
def test_recording_ingest_field_tables(H, W, pix_fmt):
    """The vertical table of parity p is aa_bicubic_table(H / 2, Hr, shift = 0.25 - p / 2) cut to the frame's crop; everything horizontal, the target size and the
    crop origin are the progressive ingest's; 4:2:2 chroma rows take the same two tables."""
    from synchformer_amd.ingest import RecordingIngest, aa_bicubic_table
    prog = RecordingIngest(CPU, 25, (H, W), 16000, pix_fmt=pix_fmt)
    for order in F.ORDERS:
        ing = RecordingIngest(CPU, 25, (H, W), 16000, pix_fmt=pix_fmt, field_order=order)
        assert ing.interlaced and ing.field_order == order and not prog.interlaced and prog.field_order == 'progressive'
        assert (ing.Hr, ing.Wr, ing.y0, ing.x0) == (prog.Hr, prog.Wr, prog.y0, prog.x0) == F.origin(H, W)
        assert torch.equal(ing.x_first, prog.x_first) and torch.equal(ing.x_w, prog.x_w) and ing.taps_x == prog.taps_x
        assert len(ing.y_tables) == 2 and (ing.taps_y, ing.taps_x) == F.CASES[(H, W)][3]
        for p, shift in ((0, 0.25), (1, -0.25)):
            first, w, taps = aa_bicubic_table(H // 2, ing.Hr, shift=shift)
            assert taps == ing.taps_y and torch.equal(ing.y_tables[p][0], first[ing.y0:ing.y0 + 224]) and torch.equal(ing.y_tables[p][1], w[ing.y0:ing.y0 + 224])
        assert not torch.equal(ing.y_tables[0][1], ing.y_tables[1][1])
        if pix_fmt != 'rgb24':
            assert torch.equal(ing.cx_first, prog.cx_first) and torch.equal(ing.cx_w, prog.cx_w) and torch.equal(ing.csc, prog.csc)
    assert RecordingIngest(CPU, 25, (1080, 1920), 16000).taps_y == 19            # the field reads half the rows through 11 taps instead of 19


@pytest.mark.parametrize('H, W', [(270, 480), (480, 202), (1080, 1920)])
def test_ramp_guards_the_sign_of_the_siting(H, W):
    """A ramp of 0.5 level per FRAME row through either field table (float64) gives what the progressive table gives on the whole frame, within 0.01: the field's
    rows are placed where they sit in the frame.  The opposite sign is off by 0.5."""
    from synchformer_amd.ingest import aa_bicubic_table
    Hr, _, y0, _ = F.origin(H, W)
    ramp = 0.5 * torch.arange(H, dtype=torch.float64)

    def through(first, w, x):
        return torch.stack([(w[i] * torch.nn.functional.pad(x, (0, w.shape[1]))[int(first[i]):int(first[i]) + w.shape[1]]).sum() for i in range(y0, y0 + 224)])

    want = through(*aa_bicubic_table(H, Hr, dtype=torch.float64)[:2], ramp)
    for p, shift in ((0, 0.25), (1, -0.25)):
        got = through(*aa_bicubic_table(H // 2, Hr, dtype=torch.float64, shift=shift)[:2], ramp[p::2])
        wrong = through(*aa_bicubic_table(H // 2, Hr, dtype=torch.float64, shift=-shift)[:2], ramp[p::2])
        err, bad = (got - want).abs().max().item(), (wrong - want).abs().max().item()
        print(f'{H} x {W} parity {p}: ramp error {err:.4f}, opposite sign {bad:.4f}')
        assert err <= 0.01, err
        assert bad >= 0.4, bad


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_recording_ingest_field_order_validation():
    from synchformer_amd.ingest import FIELD_ORDERS, PIX_FMTS_422, RecordingIngest
    assert FIELD_ORDERS == ('progressive', 'tff', 'bff')
    with pytest.raises(ValueError, match='field_order'):
        RecordingIngest(CPU, 25, (270, 480), 16000, field_order='interlaced')
    with pytest.raises(ValueError, match='field_order'):
        RecordingIngest(CPU, 25, (270, 480), 16000, field_order=None)
    for order in F.ORDERS:
        with pytest.raises(ValueError, match='even H'):
            RecordingIngest(CPU, 25, (271, 480), 16000, field_order=order)
        with pytest.raises(ValueError, match='even H'):
            RecordingIngest(CPU, 25, (271, 202), 16000, pix_fmt='uyvy422', field_order=order)
        for pix_fmt in ('nv12', 'yuv420p', 'p010', 'yuv420p10le'):
            with pytest.raises(ValueError, match='4:2:0'):
                RecordingIngest(CPU, 25, (270, 480), 16000, pix_fmt=pix_fmt, field_order=order)
        for pix_fmt in ('rgb24',) + PIX_FMTS_422:
            RecordingIngest(CPU, 25, (270, 480), 16000, pix_fmt=pix_fmt, field_order=order)
        RecordingIngest(CPU, 25, (270, 480), 16000, channels_last=True, field_order=order)
    RecordingIngest(CPU, 25, (271, 480), 16000)                                   # progressive keeps its odd H
    # the 35-tap limit looks at the field's vertical taps (19 where the frame has 35) beside the unchanged horizontal ones
    big = RecordingIngest(CPU, 25, (2160, 3840), 16000, field_order='tff')
    assert (big.taps_y, big.taps_x) == (19, 35) and big.y_tables[1][1].shape == (224, 19)
    with pytest.raises(ValueError, match='taps'):
        RecordingIngest(CPU, 25, (2400, 4000), 16000, field_order='tff')         # 39 horizontal taps
    ing = RecordingIngest(CPU, 25, (270, 480), 16000, pix_fmt='uyvy422', field_order='tff')
    with pytest.raises(ValueError, match='raw frames'):                          # the raw frames are whole frames, not fields
        ing.frames(torch.zeros(4, 135, 480, 2, dtype=torch.uint8), 0, 1)
    with pytest.raises(ValueError, match='frames'):
        ing.frames(torch.zeros(4, 270, 480, 2, dtype=torch.uint8), 0, 9)          # 4 frames at 25i give 0, 2, 4, 6 and the last field: 5 slots


def test_abi_lists_the_field_launchers():
    from synchformer_amd import _lib
    assert _lib.ABI_VERSION >= 22
    header = open(os.path.join(ROOT, 'include', 'synchformer_hip.h')).read()
    assert int(re.search(r'#define SF_ABI_VERSION (\d+)', header).group(1)) >= 22
    for name, base, extra in (('sf_ingest_video_fields', 'sf_ingest_video', 3), ('sf_ingest_video_yuv_planes_fields', 'sf_ingest_video_yuv_planes', 5)):
        decl = re.search(r'\nint %s\((.*?)\);' % name, header, re.S).group(1)
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) == len(_lib.SIGNATURES[base]) + extra, name
    for lib in (_lib.load(), _lib.load_ablation()):
        assert hasattr(lib, 'sf_ingest_video_fields') and hasattr(lib, 'sf_ingest_video_yuv_planes_fields') and lib.sf_abi_version() >= 22


def _aligned(buf):
    p = ctypes.addressof(buf)
    return p + (-p) % 16


def test_rgb_field_launcher_rejects_bad_arguments_without_gpu():
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = _aligned(buf)
    order = ('raw', 'sf', 'sc', 'sy', 'sx', 'n_src', 'H', 'W', 'ft', 'yf0', 'yw0', 'yf1', 'yw1', 'ty', 'xf', 'xw', 'tx', 'bff', 'out', 'T')
    v = dict(raw=p, sf=100, sc=1, sy=10, sx=1, n_src=1, H=10, W=10, ft=p, yf0=p, yw0=p, yf1=p, yw1=p, ty=5, xf=p, xw=p, tx=5, bff=0, out=p, T=1)

    def fields(**kw):
        a = dict(v, **kw)
        return lib.sf_ingest_video_fields(*[a[k] for k in order], None)

    def err():
        return lib.sf_last_error()

    for name in ('raw', 'ft', 'yf0', 'yw0', 'yf1', 'yw1', 'xf', 'xw', 'out'):                    # both table pairs
        assert fields(**{name: None}) == -1 and b'null pointer' in err(), name
    for H in (1, 9, 11, 271):
        assert fields(H=H) == -1 and b'even H' in err(), H
        assert fields(H=H, T=0) == -1, H
    assert fields(H=0) == -1 and fields(H=-2) == -1
    for H in (2, 10, 1080):
        assert fields(H=H, T=0) == 0, H
    for bff in (2, -1):
        assert fields(bff=bff) == -1 and b'bottom_first' in err(), bff
    assert fields(bff=1, T=0) == 0
    # and everything sf_ingest_video refuses
    for name in ('ty', 'tx'):
        assert fields(**{name: 0}) == -1 and b'out of range' in err(), name
        assert fields(**{name: 36}) == -1 and b'out of range' in err(), name
        assert fields(**{name: 35, 'T': 0}) == 0, name
    assert fields(out=p + 1) == -1 and b'aligned' in err()
    assert fields(sx=0) == -1 and b'stride' in err()
    for name in ('sf', 'sc', 'sy'):
        assert fields(**{name: -1}) == -1 and b'stride' in err(), name
    assert fields(W=70000) == -1 and b'too wide' in err()
    assert fields(W=5200, tx=35) == -1 and b'too wide' in err()                  # the LDS geometry, at the field's taps
    assert fields(T=-1) == -1 and fields(T=65536) == -1 and fields(W=0) == -1 and fields(n_src=0) == -1 and fields(n_src=1 << 30) == -1
    assert fields(T=0) == 0                                                      # nothing to do: returns before any launch


def test_planes_field_launcher_rejects_bad_arguments_without_gpu():
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = _aligned(buf)
    order = ('raw', 'bs', 'sf', 'yo', 'sy', 'sx', 'uo', 'vo', 'csy', 'csx', 'shift', 'n_src', 'H', 'W', 'Hc', 'Wc', 'ft', 'yf0', 'yw0', 'yf1', 'yw1', 'ty', 'xf', 'xw', 'tx',
             'cyf0', 'cyw0', 'cyf1', 'cyw1', 'tcy', 'cxf', 'cxw', 'tcx', 'csc', 'bff', 'out', 'T')
    v = dict(raw=p, bs=2, sf=400, yo=0, sy=40, sx=4, uo=2, vo=6, csy=40, csx=8, shift=6, n_src=1, H=10, W=10, Hc=10, Wc=5, ft=p, yf0=p, yw0=p, yf1=p, yw1=p, ty=5, xf=p,
             xw=p, tx=5, cyf0=p, cyw0=p, cyf1=p, cyw1=p, tcy=5, cxf=p, cxw=p, tcx=5, csc=p, bff=0, out=p, T=1)                 # a y210 frame of 10 x 10

    def planes(**kw):
        a = dict(v, **kw)
        return lib.sf_ingest_video_yuv_planes_fields(*[a[k] for k in order], None)

    def err():
        return lib.sf_last_error()

    for name in ('raw', 'ft', 'yf0', 'yw0', 'yf1', 'yw1', 'xf', 'xw', 'cyf0', 'cyw0', 'cyf1', 'cyw1', 'cxf', 'cxw', 'csc', 'out'):
        assert planes(**{name: None}) == -1 and b'null pointer' in err(), name
    for H in (1, 9, 11):
        assert planes(H=H, Hc=H) == -1 and b'even H' in err(), H
        assert planes(H=H, Hc=H, T=0) == -1, H
    for Hc in (5, 9, 1):                                                         # 4:2:0 and anything else below full vertical chroma resolution
        assert planes(Hc=Hc) == -1 and b'full vertical chroma' in err(), Hc
        assert planes(Hc=Hc, T=0) == -1, Hc
    for bff in (2, -1):
        assert planes(bff=bff) == -1 and b'bottom_first' in err(), bff
    assert planes(bff=1, T=0) == 0 and planes(H=2, Hc=2, T=0) == 0 and planes(Wc=10, T=0) == 0                      # 4:4:4 is served
    # and everything sf_ingest_video_yuv_planes refuses
    for bs in (0, 3, 4, -1):
        assert planes(bs=bs) == -1 and b'bytes_per_sample' in err(), bs
    for name, odd in (('sf', 401), ('yo', 1), ('sy', 41), ('sx', 5), ('uo', 3), ('vo', 7), ('csy', 41), ('csx', 9)):
        assert planes(**{name: odd}) == -1 and b'odd' in err(), name
        assert planes(**{name: odd, 'bs': 1, 'T': 0}) == 0, name
    assert planes(raw=p + 1) == -1 and b'2-byte aligned' in err()
    for shift in (7, -1, 16):
        assert planes(shift=shift) == -1 and b'shift' in err(), shift
    for kw in (dict(Hc=0), dict(Hc=11), dict(Wc=0), dict(Wc=11), dict(Wc=-3)):
        assert planes(**kw) == -1 and b'chroma planes' in err(), kw
    for kw in (dict(sx=0), dict(sx=1), dict(csx=0), dict(csx=1), dict(bs=1, sx=0), dict(bs=1, csx=0)):
        assert planes(**kw) == -1 and b'stride' in err(), kw
    for name in ('sf', 'yo', 'sy', 'uo', 'vo', 'csy'):
        assert planes(**{name: -2}) == -1 and b'stride' in err(), name
    for name in ('ty', 'tx', 'tcy', 'tcx'):
        assert planes(**{name: 0}) == -1 and b'out of range' in err(), name
        assert planes(**{name: 36}) == -1 and b'out of range' in err(), name
        assert planes(**{name: 35, 'T': 0}) == 0, name
    assert planes(out=p + 1) == -1 and b'aligned' in err()
    assert planes(W=70000) == -1 and b'too wide' in err()
    assert planes(W=5200, tx=35) == -1 and b'too wide' in err()
    assert planes(W=5100, Wc=2550, tcx=35) == -1 and b'too wide' in err() and b'chroma' in err()
    assert planes(T=-1) == -1 and planes(T=65536) == -1 and planes(H=0) == -1 and planes(W=0) == -1 and planes(n_src=0) == -1 and planes(n_src=1 << 30) == -1
    assert planes(T=0) == 0


def test_field_ops_refuse_before_the_device():
    from synchformer_amd import ops
    from synchformer_amd.ingest import RecordingIngest, plane_layout
    pick = torch.zeros(1, dtype=torch.int32)
    rgb = RecordingIngest(CPU, 25, (270, 480), 16000, field_order='tff')
    with pytest.raises(ValueError, match='expected uint8 frames'):
        ops.ingest_video_fields(torch.zeros(1, 4, 270, 480, dtype=torch.uint8), False, pick, rgb.y_tables, rgb.x_first, rgb.x_w, False)
    with pytest.raises(ValueError, match='even H'):
        ops.ingest_video_fields(torch.zeros(1, 3, 271, 480, dtype=torch.uint8), False, pick, rgb.y_tables, rgb.x_first, rgb.x_w, False)
    with pytest.raises(ValueError, match='one tap count'):
        ops.ingest_video_fields(torch.zeros(1, 3, 270, 480, dtype=torch.uint8), False, pick, (rgb.y_tables[0], (rgb.y_tables[1][0], torch.zeros(224, 7))), rgb.x_first,
                                rgb.x_w, False)
    for channels_last, shape in ((False, (1, 3, 270, 480)), (True, (1, 270, 480, 3))):
        with pytest.raises(RuntimeError, match='device tensor'):                 # a CPU tensor: no fallback
            ops.ingest_video_fields(torch.zeros(*shape, dtype=torch.uint8), channels_last, pick, rgb.y_tables, rgb.x_first, rgb.x_w, True)
    ing = RecordingIngest(CPU, 25, (270, 480), 16000, pix_fmt='uyvy422', field_order='bff')
    L = plane_layout('uyvy422', 270, 480)
    tabs = (ing.y_tables, ing.x_first, ing.x_w, ing.y_tables, ing.cx_first, ing.cx_w, ing.csc, True)
    raw = torch.zeros(1, 270, 480, 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match='expected uint8'):
        ops.ingest_video_planes_fields(raw.view(torch.int16), L, pick, *tabs)
    with pytest.raises(ValueError, match='expected uint16'):
        ops.ingest_video_planes_fields(raw, plane_layout('y210', 270, 480), pick, *tabs)
    with pytest.raises(ValueError, match='reaches byte'):
        ops.ingest_video_planes_fields(raw[:, :269], L, pick, *tabs)
    with pytest.raises(ValueError, match='even H'):                              # an odd H, and a 4:2:0 layout
        ops.ingest_video_planes_fields(torch.zeros(1, 271, 480, 2, dtype=torch.uint8), plane_layout('uyvy422', 271, 480), pick, *tabs)
    with pytest.raises(ValueError, match='chroma planes of H rows'):
        ops.ingest_video_planes_fields(torch.zeros(1, 405, 480, dtype=torch.uint8), plane_layout('nv12', 270, 480), pick, *tabs)
    with pytest.raises(RuntimeError, match='device tensor'):
        ops.ingest_video_planes_fields(raw, L, pick, *tabs)
    with pytest.raises(RuntimeError, match='device tensor'):                     # and through RecordingIngest: frames on the host, tables on the host, nothing to fall back to
        ing.frames(raw, 0, 1)


# ---- stream -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pushes', [[7], [1, 1, 1, 1, 1, 1, 1], [0, 3, 0, 1, 3]])
def test_ingest_stream_counts_fields(pushes, monkeypatch):
    """7 frames at 30000/1001, top field first, in three chunkings: the field indices IngestStream hands to _resize (relative to the frames it holds) are, in absolute
    terms and concatenated, the offline field table; every one lies inside the frames handed over with it; at most one source FRAME stays held."""
    from synchformer_amd.ingest import RecordingIngest, fps_field_table
    ing = RecordingIngest(CPU, (30000, 1001), (270, 480), 16000, field_order='tff')
    calls = []

    def record(src, t):
        calls.append((int(src.shape[0]), t.tolist()))
        return torch.zeros(len(t), 3, 224, 224, dtype=torch.uint8)

    monkeypatch.setattr(ing, '_resize', record)
    st, got, seen, n_out = ing.stream(), [], 0, 0
    for k in pushes + [None]:
        held = st.held['frames']
        before = len(calls)
        frames = st.flush()[0] if k is None else st.push(torch.zeros(k, 3, 270, 480, dtype=torch.uint8), None)[0]
        seen += k or 0
        n_out += frames.shape[0]
        for n_src, t in calls[before:]:
            base = seen - n_src                                                  # src[0] is source frame `base`: the held frame, then the push
            assert n_src == held + (k or 0) and all(0 <= f < 2 * n_src for f in t), (n_src, t)
            got += [f + 2 * base for f in t]
        assert st.held['frames'] <= 1
    want = fps_field_table(7, (30000, 1001)).tolist()
    assert want == F.frame_table_bruteforce(14, Fraction(60000, 1001)) and {f & 1 for f in want} == {0, 1}
    assert got == want and n_out == len(want) == ing.n_frames(7), (got, want)


# ---- the pixel bar ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H, W', list(F.CASES))
def test_fp32_restatement_stays_inside_the_pixel_bar(H, W):
    """The margin the GPU bar leaves for fields: the package's tables (and matrix) evaluated in fp32 on the CPU - horizontal pass first, taps ascending, the kernel's
    order up to its fused multiply-adds - on the field sliced out by plain indexing, against the float64 oracle at the GPU test sizes: rgb24, and 4:2:2 in 8 and
    10 bits.  Every pixel within 1 level and at most 1e-3 of the pixels differing (the project's bar)."""
    from synchformer_amd.ingest import RecordingIngest
    cs, full, loc, luma, chroma = F.CASES[(H, W)]
    Hr, Wr, y0, x0 = F.origin(H, W)
    table = [1, 2] if H > 1000 else F.TABLE
    for order in F.ORDERS:
        if H <= 1000:
            frames = F.random_frames(4, H, W, H * 10000 + W)
            ref = F.oracle_rgb(frames, order, table, (Hr, Wr), y0, x0)
            ing = RecordingIngest(CPU, 25, (H, W), 16000, field_order=order)
            got = torch.stack([F.apply_tables32(F.field(frames, f, order), *ing.y_tables[F.parity(f, order)], ing.x_first, ing.x_w) for f in table])
            F.check_pixels(got.round().clamp(0, 255).to(torch.uint8), ref, f'{H} x {W} rgb24 {order}: fp32 restatement')
        for bits, pix_fmt in ((8, 'uyvy422'), (10, 'y210')):
            planes = F.random_planes(4 if H <= 1000 else 2, H, W, H * 10000 + W + bits, 1 << bits)
            ref, outside = F.oracle_yuv(planes, order, table, (Hr, Wr), y0, x0, *F.matrix(cs, full, bits), loc)
            ing = RecordingIngest(CPU, 25, (H, W), 16000, pix_fmt=pix_fmt, colorspace=cs, full_range=full, chroma_loc=loc, field_order=order)
            assert ((ing.taps_y, ing.taps_x), (ing.taps_y, ing.taps_cx)) == (luma, chroma)
            m, o = ing.csc[:9].reshape(3, 3), ing.csc[9:]
            got = []
            for f in table:
                yt = ing.y_tables[F.parity(f, order)]
                r = [F.apply_tables32(F.field(planes[0], f, order)[None], *yt, ing.x_first, ing.x_w)[0]] + \
                    [F.apply_tables32(F.field(pl, f, order)[None], *yt, ing.cx_first, ing.cx_w)[0] for pl in planes[1:]]
                got.append(torch.einsum('ck,kyx->cyx', m, torch.stack([r[0] - o[0], r[1] - o[1], r[2] - o[2]])))
            got = torch.stack(got).round().clamp(0, 255).to(torch.uint8)
            F.check_pixels(got, ref, f'{H} x {W} {bits}-bit {order} {cs} {"full" if full else "limited"} {loc}: fp32 restatement, {outside:.1%} outside [0, 255] before '
                                     f'the clamp')
