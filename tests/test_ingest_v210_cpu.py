"""No GPU: the host side of the v210 ingest - the packing of tests/ingest_v210_oracle.py against literal words worked out from the published layout,
ingest.v210_row_words, the argument validation of ops.ingest_video_v210 / _fields and of RecordingIngest(pix_fmt='v210'), the two ABI entries and every refusal of
their launcher (it returns before the device is touched)."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_v210_oracle as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')


def _u32(raw):
    return [w & 0xffffffff for w in raw.reshape(-1).tolist()]


# ---- 1. the packing -------------------------------------------------------------------------------------------------------------------------------------------------
def test_first_word_literal():
    """Cb0 = 1, Y0 = 2, Cr0 = 3: 1 | 2 << 10 | 3 << 20 = 0x00300801 (W = 2: one word of samples, then the three unused words of the group)."""
    raw = V.pack_v210([torch.tensor([[[2, 0]]]), torch.tensor([[[1]]]), torch.tensor([[[3]]])])
    assert raw.dtype == torch.int32 and raw.shape == (1, 1, 4)
    assert _u32(raw) == [0x00300801, 0, 0, 0]                                   # Y1 = 0 is field 3: word 1, bit 0


def test_group_of_six_pixels_literal():
    """The published layout of a group: word 0 = Cb0 Y0 Cr0, word 1 = Y1 Cb1 Y2, word 2 = Cr1 Y3 Cb2, word 3 = Y4 Cr2 Y5, each from bit 0 up in steps of 10.  With the
    twelve fields numbered 1 .. 12 in stream order (Cb = 1 5 9, Y = 2 4 6 8 10 12, Cr = 3 7 11):
        word 0 = 1 | 2 << 10 | 3 << 20 = 0x00300801          word 1 = 4 | 5 << 10 | 6 << 20 = 0x00601404
        word 2 = 7 | 8 << 10 | 9 << 20 = 0x00902007          word 3 = 10 | 11 << 10 | 12 << 20 = 0x00C02C0A
    and with every field 1023 each word is 0x3FFFFFFF."""
    planes = [torch.tensor([[[2, 4, 6, 8, 10, 12]]]), torch.tensor([[[1, 5, 9]]]), torch.tensor([[[3, 7, 11]]])]
    assert _u32(V.pack_v210(planes)) == [0x00300801, 0x00601404, 0x00902007, 0x00C02C0A]
    full = [torch.full((1, 1, 6), 1023), torch.full((1, 1, 3), 1023), torch.full((1, 1, 3), 1023)]
    assert _u32(V.pack_v210(full)) == [0x3FFFFFFF] * 4
    got = V.unpack_v210(torch.tensor([[[0x00300801, 0x00601404, 0x00902007, 0x00C02C0A]]], dtype=torch.int32), 6)
    assert [p.reshape(-1).tolist() for p in got] == [[2, 4, 6, 8, 10, 12], [1, 5, 9], [3, 7, 11]]


@pytest.mark.parametrize('W', [2, 4, 6, 8, 10, 12, 14, 46, 48, 50, 176, 202])
def test_unpack_inverts_pack(W):
    """unpack(pack(x)) == x at every W % 6 and W % 48 class, with garbage in the padding words and in the unused fields of the last group, and with bits 30 - 31 set in
    every word; the padding really holds the garbage."""
    planes = V.random_planes(2, 3, W, W, 1024)
    need = V.min_words(W)
    for row_words, fill in ((need, 0), (need, 0xffffffff), (need + 5, 0xdeadbeef)):
        raw = V.pack_v210(planes, row_words, fill)
        assert raw.shape == (2, 3, row_words)
        for r in (raw, V.set_stray_bits(raw)):
            assert all(torch.equal(a, b) for a, b in zip(V.unpack_v210(r, W), planes)), (row_words, fill)
        if row_words > need:
            assert set(_u32(raw[..., need:])) == {fill}
    if W % 6:                                                                   # the unused trailing fields of the last group hold the fill's fields
        a, b = V.pack_v210(planes, need, 0), V.pack_v210(planes, need, 0xffffffff)
        assert not torch.equal(a, b) and torch.equal(a[..., :(2 * W - 1) // 3], b[..., :(2 * W - 1) // 3])


def test_row_words():
    from synchformer_amd.ingest import PIX_FMTS, PIX_FMTS_422, PIX_FMTS_V210, v210_row_words
    assert PIX_FMTS_V210 == ('v210',) and 'v210' not in PIX_FMTS + PIX_FMTS_422
    assert (v210_row_words(1920), v210_row_words(1280), v210_row_words(720)) == (1280, 864, 480)      # pitches of 5120, 3456 and 1920 bytes
    for W in (2, 4, 6, 8, 46, 48, 50, 202, 958, 1920, 3840):
        assert v210_row_words(W, aligned=False) == V.min_words(W) == 4 * ((W + 5) // 6)
        assert v210_row_words(W) == 32 * ((W + 47) // 48) >= v210_row_words(W, aligned=False) and v210_row_words(W) % 32 == 0
    with pytest.raises(ValueError):
        v210_row_words(0)


# ---- 2. host validation -----------------------------------------------------------------------------------------------------------------------------------------------
def _op_args(H=270, W=480, **kw):
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(CPU, 25, (H, W), 16000, pix_fmt='v210', **kw)
    return ing, (ing.y_first, ing.y_w, ing.x_first, ing.x_w, ing.cx_first, ing.cx_w, ing.csc)


def test_op_value_errors():
    from synchformer_amd import ops
    ing, tabs = _op_args()
    pick = torch.zeros(1, dtype=torch.int32)
    ok = torch.zeros(1, 270, 320, dtype=torch.int32)
    for bad, msg in ((ok.to(torch.int16), 'expected int32'), (ok.view(torch.uint8), 'expected int32'), (ok[0], 'expected int32'), (ok[None], 'expected int32'),
                     (ok[:, :, :319], 'rows of 319 words'), (torch.zeros(1, 270, 640, dtype=torch.int32)[:, :, ::2], 'strides')):
        with pytest.raises(ValueError, match=msg):
            ops.ingest_video_v210(bad, 480, pick, *tabs)
    with pytest.raises(ValueError, match='even W'):
        ops.ingest_video_v210(ok, 479, pick, *tabs)
    with pytest.raises(ValueError, match='even W'):
        ops.ingest_video_v210(ok, 0, pick, *tabs)
    with pytest.raises(ValueError, match='on the host'):                        # everything else in order: a host tensor is what is left
        ops.ingest_video_v210(ok, 480, pick, *tabs)
    with pytest.raises(ValueError, match='on the host'):
        ops.ingest_video_v210(ok.view(torch.uint32), 480, pick, *tabs)
    fing, ftabs = _op_args(field_order='tff')
    tail = (fing.y_tables, fing.x_first, fing.x_w, fing.cx_first, fing.cx_w, fing.csc, False)
    with pytest.raises(ValueError, match='even H'):
        ops.ingest_video_v210_fields(ok[:, :269], 480, pick, *tail)
    with pytest.raises(ValueError, match='rows of 319 words'):
        ops.ingest_video_v210_fields(ok[:, :, :319], 480, pick, *tail)
    with pytest.raises(ValueError, match='on the host'):
        ops.ingest_video_v210_fields(ok, 480, pick, *tail)
    assert 'ingest_video_v210' not in ops.DISPATCHER_OPS and 'ingest_video_v210_fields' not in ops.DISPATCHER_OPS


def test_recording_ingest_v210():
    """The tables are those of yuv422p10le (cy = y, cx over W / 2 with the siting shift, the 10-bit matrix); even W, any H, no channels_last; interlaced orders are
    admitted; _check_frames takes int32 / uint32 (T, H, Pw >= 4 ceil(W / 6)) and names .view(torch.int32)."""
    from synchformer_amd.ingest import RecordingIngest, csc_matrix
    for (H, W), (cs, full, loc, luma, chroma) in V.CASES.items():
        a = RecordingIngest(CPU, 25, (H, W), 16000, pix_fmt='v210', colorspace=cs, full_range=full, chroma_loc=loc)
        b = RecordingIngest(CPU, 25, (H, W), 16000, pix_fmt='yuv422p10le', colorspace=cs, full_range=full, chroma_loc=loc)
        assert ((a.taps_y, a.taps_x), (a.taps_cy, a.taps_cx)) == (luma, chroma)
        for name in ('y_first', 'y_w', 'x_first', 'x_w', 'cy_first', 'cy_w', 'cx_first', 'cx_w', 'csc'):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert a.cy_first is a.y_first and a.cy_w is a.y_w
        M, off = csc_matrix(cs, full, 10)
        assert torch.equal(a.csc, torch.cat([M.reshape(9), off]).float())
    left, topleft = (RecordingIngest(CPU, 25, (270, 480), 16000, pix_fmt='v210', chroma_loc=loc) for loc in ('left', 'topleft'))
    assert torch.equal(left.cx_w, topleft.cx_w) and torch.equal(left.y_w, topleft.cy_w)
    for order in ('tff', 'bff'):
        f = RecordingIngest(CPU, (30000, 1001), (270, 480), 16000, pix_fmt='v210', field_order=order)
        assert f.interlaced and len(f.y_tables) == 2
    with pytest.raises(ValueError, match='even W'):
        RecordingIngest(CPU, 25, (270, 479), 16000, pix_fmt='v210')
    with pytest.raises(ValueError, match='channels_last'):
        RecordingIngest(CPU, 25, (270, 480), 16000, pix_fmt='v210', channels_last=True)
    with pytest.raises(ValueError, match='even H'):
        RecordingIngest(CPU, 25, (271, 480), 16000, pix_fmt='v210', field_order='tff')
    with pytest.raises(ValueError, match='pix_fmt'):
        RecordingIngest(CPU, 25, (270, 480), 16000, pix_fmt='v216')
    ing = RecordingIngest(CPU, 25, (271, 202), 16000, pix_fmt='v210')           # an odd H is legal
    ing._check_frames(torch.zeros(2, 271, 136, dtype=torch.int32))
    ing._check_frames(torch.zeros(2, 271, 160, dtype=torch.uint32))             # the conventional pitch, the other dtype
    for bad in (torch.zeros(2, 271, 135, dtype=torch.int32), torch.zeros(2, 270, 136, dtype=torch.int32), torch.zeros(2, 271, 544, dtype=torch.uint8),
                torch.zeros(2, 271, 136, 1, dtype=torch.int32), torch.zeros(2, 271, 136, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r'raw frames.*view\(torch\.int32\)'):
            ing._check_frames(bad)


# ---- 3. ABI and launcher ------------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_lists_the_v210_launchers():
    from synchformer_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'synchformer_hip.h')).read()
    for name, n_args in (('sf_ingest_video_v210', 20), ('sf_ingest_video_v210_fields', 23)):
        decl = re.search(r'\nint %s\((.*?)\);' % name, header, re.S).group(1)
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) == n_args, name
        for lib in (_lib.load(), _lib.load_ablation()):
            assert hasattr(lib, name), name


ORDER = ('raw', 'sf', 'sy', 'n_src', 'H', 'W', 'ft', 'yf', 'yw', 'ty', 'xf', 'xw', 'tx', 'cxf', 'cxw', 'tcx', 'csc', 'out', 'T')
ORDER_F = ('raw', 'sf', 'sy', 'n_src', 'H', 'W', 'ft', 'yf', 'yw', 'yf1', 'yw1', 'ty', 'xf', 'xw', 'tx', 'cxf', 'cxw', 'tcx', 'csc', 'bff', 'out', 'T')


@pytest.mark.parametrize('fields', [False, True])
def test_launchers_reject_bad_arguments_without_gpu(fields):
    """Every refusal of the header comment; all of them return -1 before a launch, so no device is needed.  The frame is 10 x 10: two groups, 32 bytes a row."""
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    v = dict(raw=p, sf=320, sy=32, n_src=1, H=10, W=10, ft=p, yf=p, yw=p, yf1=p, yw1=p, ty=5, xf=p, xw=p, tx=5, cxf=p, cxw=p, tcx=5, csc=p, bff=0, out=p, T=1)
    fn, order = (lib.sf_ingest_video_v210_fields, ORDER_F) if fields else (lib.sf_ingest_video_v210, ORDER)
    who = b'sf_ingest_video_v210_fields' if fields else b'sf_ingest_video_v210'

    def call(**kw):
        a = dict(v, **kw)
        return fn(*[a[k] for k in order], None)

    def err():
        return lib.sf_last_error()

    for name in ('raw', 'ft', 'yf', 'yw', 'xf', 'xw', 'cxf', 'cxw', 'csc', 'out') + (('yf1', 'yw1') if fields else ()):
        assert call(**{name: None}) == -1 and b'null pointer' in err() and who in err(), name
        assert call(**{name: None, 'T': 0}) == 0, name                          # nothing to launch: the pointers are not looked at
    for mis in (1, 2, 3):
        assert call(raw=p + mis) == -1 and b'4-byte aligned' in err(), mis
    for kw in (dict(sy=28), dict(W=14, sy=44), dict(W=2, sy=12), dict(W=14, sy=32)):                # 16 ceil(W / 6) - 4, and a pitch of two groups under three
        assert call(**kw) == -1 and b'stride_row' in err() and b'below' in err(), kw
        assert call(T=0, **kw) == -1, kw
    for kw in (dict(sy=34), dict(sy=33), dict(sy=38), dict(sf=322), dict(sf=321), dict(sy=-32), dict(sf=-320)):
        assert call(**kw) == -1 and b'multiples of 4' in err(), kw
        assert call(T=0, **kw) == -1, kw
    for kw in (dict(sy=36), dict(sy=5120), dict(sf=0), dict(W=2, sy=16), dict(W=6, sy=16), dict(W=8, sy=32)):
        assert call(T=0, **kw) == 0, kw
    for kw in (dict(W=9), dict(W=1), dict(W=0), dict(W=-2), dict(H=0), dict(n_src=0)):
        assert call(**kw) == -1 and call(T=0, **kw) == -1, kw
    assert call(W=11) == -1 and b'even W' in err()
    assert call(T=0, H=11) == (-1 if fields else 0)                             # an odd H is legal for frames
    for name in ('ty', 'tx', 'tcx'):
        assert call(**{name: 0}) == -1 and b'out of range' in err(), name
        assert call(**{name: 36}) == -1 and b'out of range' in err(), name
        assert call(**{name: 35, 'T': 0}) == 0, name
    assert call(out=p + 1) == -1 and b'aligned' in err()
    assert call(T=-1) == -1 and call(T=65536) == -1
    assert call(W=70000, sy=16 * 11667) == -1 and b'too wide' in err()
    assert call(W=5200, sy=16 * 867, tx=35) == -1 and b'too wide' in err()      # what the plain 16-bit geometry refuses (test_ingest_yuv422_cpu.py), nothing narrower
    if fields:
        for kw in (dict(H=11), dict(H=1), dict(bff=2), dict(bff=-1), dict(n_src=1 << 30)):
            assert call(**kw) == -1 and call(T=0, **kw) == -1, kw
        assert call(H=11) == -1 and b'even H' in err()
        assert call(bff=2) == -1 and b'bottom_first' in err()
        assert call(T=0, n_src=(1 << 30) - 1, bff=1) == 0
    assert call(T=0) == 0
