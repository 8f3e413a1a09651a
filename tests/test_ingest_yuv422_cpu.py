"""No GPU: the host side of the 4:2:2 ingest - ingest.plane_layout against the layout table written out here, the tables and matrices of
RecordingIngest per format, its argument validation, the ABI entry of sf_ingest_video_yuv_planes and every refusal of its launcher (before the device is
touched), and the margin of the pixel bar: the kernel's arithmetic restated in fp32 against the float64 oracle of tests/ingest_yuv422_oracle.py."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_yuv422_oracle as Y  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(pix_fmt, H, W, P, sf):
    """The layout table of the issue, written out: (bytes, H, W, Hc, Wc, stride_frame, y_off, stride_row, stride_col, u_off, v_off, stride_crow, stride_ccol, shift);
    P: the row pitch in bytes, sf: the frame stride in bytes."""
    h2, w2 = H // 2, W // 2
    return {'uyvy422': (1, H, W, H, w2, sf, 1, P, 2, 0, 2, P, 4, 0),
            'yuyv422': (1, H, W, H, w2, sf, 0, P, 2, 1, 3, P, 4, 0),
            'yuv422p': (1, H, W, H, w2, sf, 0, W, 1, H * W, H * W * 3 // 2, w2, 1, 0),
            'nv16': (1, H, W, H, w2, sf, 0, P, 1, P * H, P * H + 1, P, 2, 0),
            'yuv422p10le': (2, H, W, H, w2, sf, 0, 2 * W, 2, 2 * H * W, 3 * H * W, W, 2, 0),
            'p210': (2, H, W, H, w2, sf, 0, P, 2, P * H, P * H + 2, P, 4, 6),
            'y210': (2, H, W, H, w2, sf, 0, P, 4, 2, 6, P, 8, 6),
            'nv12': (1, H, W, h2, w2, sf, 0, P, 1, P * H, P * H + 1, P, 2, 0),
            'yuv420p': (1, H, W, h2, w2, sf, 0, W, 1, H * W, H * W + h2 * w2, w2, 1, 0),
            'p010': (2, H, W, h2, w2, sf, 0, P, 2, P * H, P * H + 2, P, 4, 6),
            'yuv420p10le': (2, H, W, h2, w2, sf, 0, 2 * W, 2, 2 * H * W, 2 * (H * W + h2 * w2), W, 2, 0)}[pix_fmt]


def _raw_shape(pix_fmt, H, W):
    return (H, W, 2) if pix_fmt in ('uyvy422', 'yuyv422', 'y210') else (2 * H, W) if pix_fmt in Y.FMTS else (3 * H // 2, W)


@pytest.mark.parametrize('H, W', [(270, 480), (271, 202)])
def test_plane_layout_is_the_table(H, W):
    from synchformer_amd.ingest import PIX_FMTS, PIX_FMTS_422, PlaneLayout, plane_layout
    names = PIX_FMTS[1:] + PIX_FMTS_422
    assert len(names) == 11
    for pix_fmt in names:
        b = 2 if pix_fmt in ('p010', 'yuv420p10le') + Y.FMTS_16 else 1
        dtype = torch.uint16 if b == 2 else torch.uint8
        if H % 2 and pix_fmt not in PIX_FMTS_422:                                # 4:2:0 has no odd H
            with pytest.raises(ValueError, match='even'):
                plane_layout(pix_fmt, H, W)
            continue
        shape = _raw_shape(pix_fmt, H, W)
        packed = len(shape) == 3
        frame = torch.zeros(3, *shape, dtype=dtype)
        elems = frame[0].numel()
        P = W * b * (2 if packed else 1)
        want = PlaneLayout(*_row(pix_fmt, H, W, P, elems * b))
        assert plane_layout(pix_fmt, H, W) == want, pix_fmt
        assert plane_layout(pix_fmt, H, W, frame.stride()) == want, pix_fmt
        # a 512-column surface: a view of its first W columns
        wide = torch.zeros(3, shape[0], 512, *shape[2:], dtype=dtype)
        view = wide[:, :, :W]
        assert view.shape[1:] == shape and not view.is_contiguous()
        if pix_fmt in ('yuv422p', 'yuv420p', 'yuv422p10le', 'yuv420p10le'):      # the planar arrays have no pitch to give
            with pytest.raises(ValueError, match='contiguous rows'):
                plane_layout(pix_fmt, H, W, view.stride())
        else:
            Pw = 512 * b * (2 if packed else 1)
            assert plane_layout(pix_fmt, H, W, view.stride()) == PlaneLayout(*_row(pix_fmt, H, W, Pw, wide[0].numel() * b)), pix_fmt
    with pytest.raises(ValueError, match='pix_fmt'):
        plane_layout('yuv444p', H, W)
    with pytest.raises(ValueError, match='pix_fmt'):
        plane_layout('rgb24', H, W)
    for pix_fmt in names:
        with pytest.raises(ValueError, match='even'):
            plane_layout(pix_fmt, 270, W + 1)
    for pix_fmt in ('uyvy422', 'yuyv422', 'y210'):                               # a packed macropixel cannot be strided
        with pytest.raises(ValueError, match=r'inner strides \(2, 1\)'):
            plane_layout(pix_fmt, H, W, (H * W * 4, W * 4, 4, 1))
        with pytest.raises(ValueError, match='strides'):
            plane_layout(pix_fmt, H, W, (H * W * 2, W * 2, 1))


@pytest.mark.parametrize('pix_fmt', Y.FMTS)
def test_plane_layout_reads_back_the_packed_planes(pix_fmt):
    """The oracle's pack (byte orders written out there) and plane_layout (offsets and strides) meet: reading the raw bytes at the layout's addresses returns the
    planes, at an odd H and a chroma width of 101."""
    import numpy as np
    from synchformer_amd.ingest import plane_layout
    H, W = 271, 202
    planes = Y.random_planes(2, H, W, 3, 1024 if pix_fmt in Y.FMTS_16 else 256)
    raw = Y.pack(planes, pix_fmt)
    L = plane_layout(pix_fmt, H, W, raw.stride())
    a = np.frombuffer(raw.numpy().tobytes(), dtype=np.uint8).astype(np.int64)
    for p, off, h, sr, w, sc in ((planes[0], L.y_off, L.H, L.stride_row, L.W, L.stride_col), (planes[1], L.u_off, L.Hc, L.stride_crow, L.Wc, L.stride_ccol),
                                 (planes[2], L.v_off, L.Hc, L.stride_crow, L.Wc, L.stride_ccol)):
        idx = np.arange(2)[:, None, None] * L.stride_frame + off + np.arange(h)[None, :, None] * sr + np.arange(w)[None, None] * sc
        got = a[idx] if L.bytes_per_sample == 1 else ((a[idx] | (a[idx + 1] << 8)) >> L.shift) & 1023
        assert (got == p.numpy()).all()


def test_recording_ingest_422_tables_and_matrices():
    from synchformer_amd.ingest import PIX_FMTS_422, PIX_FMTS_422_16, RecordingIngest, aa_bicubic_table, csc_matrix
    assert PIX_FMTS_422 == ('uyvy422', 'yuyv422', 'yuv422p', 'nv16', 'yuv422p10le', 'p210', 'y210') and PIX_FMTS_422_16 == ('yuv422p10le', 'p210', 'y210')
    cpu = torch.device('cpu')
    yf, yw, ty = aa_bicubic_table(1080, 256)
    xf, xw, tx = aa_bicubic_table(1920, 454)
    for pix_fmt in PIX_FMTS_422:
        ings = {loc: RecordingIngest(cpu, 25, (1080, 1920), 48000, pix_fmt=pix_fmt, chroma_loc=loc) for loc in ('center', 'left', 'topleft')}
        for loc, ing in ings.items():
            assert ing.chroma_loc == loc and ((ing.taps_y, ing.taps_x), (ing.taps_cy, ing.taps_cx)) == ((19, 19), (19, 11))
            assert torch.equal(ing.y_first, yf[16:240]) and torch.equal(ing.y_w, yw[16:240]) and torch.equal(ing.x_first, xf[115:339]) and torch.equal(ing.x_w, xw[115:339])
            assert torch.equal(ing.cy_first, ing.y_first) and torch.equal(ing.cy_w, ing.y_w) and ing.taps_cy == ing.taps_y
            cxf, cxw, tcx = aa_bicubic_table(960, 454, shift=0.0 if loc == 'center' else 0.25)
            assert tcx == 11 and torch.equal(ing.cx_first, cxf[115:339]) and torch.equal(ing.cx_w, cxw[115:339])
        assert not torch.equal(ings['center'].cx_w, ings['left'].cx_w)
        for k in ('y_first', 'y_w', 'x_first', 'x_w', 'cy_first', 'cy_w', 'cx_first', 'cx_w', 'csc'):                # no vertical subsampling: no vertical shift
            assert torch.equal(getattr(ings['topleft'], k), getattr(ings['left'], k)), k
        depth = 10 if pix_fmt in PIX_FMTS_422_16 else 8
        for cs, full in (('bt601', False), ('bt709', True), ('bt709', False)):
            ing = RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt=pix_fmt, colorspace=cs, full_range=full)
            M, off = csc_matrix(cs, full, depth)
            assert ing.csc.dtype == torch.float32 and ing.csc.device.type == 'cpu' and torch.equal(ing.csc, torch.cat([M.reshape(9), off]).float())
            Mo, oo = Y.matrix(cs, full, depth)                                   # and the oracle's own formula agrees
            assert (M - Mo).abs().max().item() <= 1e-15 and torch.equal(off, oo)


def test_recording_ingest_422_argument_validation():
    from synchformer_amd import ingest
    from synchformer_amd.ingest import RecordingIngest
    cpu = torch.device('cpu')
    assert ingest.PIX_FMTS == ('rgb24', 'nv12', 'yuv420p', 'p010', 'yuv420p10le')
    with pytest.raises(ValueError, match='pix_fmt'):
        RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt='yuv444p')
    for pix_fmt in Y.FMTS:
        with pytest.raises(ValueError, match='even W'):
            RecordingIngest(cpu, 25, (302, 517), 16000, pix_fmt=pix_fmt)
        odd = RecordingIngest(cpu, 25, (271, 202), 16000, pix_fmt=pix_fmt)        # an odd H is legal
        assert (odd.H, odd.W, odd.Hr, odd.Wr) == (271, 202, 342, 256)
        with pytest.raises(ValueError, match='channels_last'):
            RecordingIngest(cpu, 25, (270, 480), 16000, channels_last=True, pix_fmt=pix_fmt)
        ing = RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt=pix_fmt)
        good = torch.uint16 if pix_fmt in Y.FMTS_16 else torch.uint8
        bad = torch.uint8 if pix_fmt in Y.FMTS_16 else torch.uint16
        shape = _raw_shape(pix_fmt, 270, 480)
        with pytest.raises(ValueError, match='raw frames'):                      # the other sample width
            ing.frames(torch.zeros(4, *shape, dtype=bad), 0, 1)
        with pytest.raises(ValueError, match='raw frames'):
            ing.frames(torch.zeros(4, *shape, dtype=torch.float16), 0, 1)
        with pytest.raises(ValueError, match='raw frames'):                      # a 4:2:0 frame
            ing.frames(torch.zeros(4, 405, 480, dtype=good), 0, 1)
        with pytest.raises(ValueError, match='raw frames'):                      # the other family's shape
            ing.frames(torch.zeros(4, *((540, 480) if len(shape) == 3 else (270, 480, 2)), dtype=good), 0, 1)
        with pytest.raises(ValueError, match='raw frames'):
            ing.stream().push(torch.zeros(4, 405, 480, dtype=good))
    odd = RecordingIngest(cpu, 25, (271, 202), 16000, pix_fmt='yuv422p')
    odd._check_frames(torch.zeros(1, 542, 202, dtype=torch.uint8))                # yuv422p at odd H still fills 2 H rows


def test_abi_lists_the_planes_launcher():
    from synchformer_amd import _lib
    assert _lib.ABI_VERSION >= 21
    header = open(os.path.join(ROOT, 'include', 'synchformer_hip.h')).read()
    decl = re.search(r'\nint sf_ingest_video_yuv_planes\((.*?)\);', header, re.S).group(1)
    assert len(_lib.SIGNATURES['sf_ingest_video_yuv_planes']) == len(decl.split(',')) == len(_lib.SIGNATURES['sf_ingest_video_yuv16']) + 5 == 33
    for lib in (_lib.load(), _lib.load_ablation()):
        assert hasattr(lib, 'sf_ingest_video_yuv_planes') and lib.sf_abi_version() >= 21


def test_planes_launcher_rejects_bad_arguments_without_gpu():
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    order = ('raw', 'bs', 'sf', 'yo', 'sy', 'sx', 'uo', 'vo', 'csy', 'csx', 'shift', 'n_src', 'H', 'W', 'Hc', 'Wc', 'ft', 'yf', 'yw', 'ty', 'xf', 'xw', 'tx', 'cyf', 'cyw',
             'tcy', 'cxf', 'cxw', 'tcx', 'csc', 'out', 'T')
    v = dict(raw=p, bs=2, sf=400, yo=0, sy=40, sx=4, uo=2, vo=6, csy=40, csx=8, shift=6, n_src=1, H=10, W=10, Hc=10, Wc=5, ft=p, yf=p, yw=p, ty=5, xf=p, xw=p, tx=5,
             cyf=p, cyw=p, tcy=5, cxf=p, cxw=p, tcx=5, csc=p, out=p, T=1)                                             # a y210 frame of 10 x 10

    def planes(**kw):
        a = dict(v, **kw)
        return lib.sf_ingest_video_yuv_planes(*[a[k] for k in order], None)

    def err():
        return lib.sf_last_error()

    for name in ('raw', 'ft', 'yf', 'yw', 'xf', 'xw', 'cyf', 'cyw', 'cxf', 'cxw', 'csc', 'out'):
        assert planes(**{name: None}) == -1 and b'null pointer' in err(), name
    for bs in (0, 3, 4, -1):
        assert planes(bs=bs) == -1 and b'bytes_per_sample' in err(), bs
        assert planes(bs=bs, T=0) == -1, bs
    for name, odd in (('sf', 401), ('yo', 1), ('sy', 41), ('sx', 5), ('uo', 3), ('vo', 7), ('csy', 41), ('csx', 9)):
        assert planes(**{name: odd}) == -1 and b'odd' in err(), name
        assert planes(**{name: odd, 'T': 0}) == -1, name
        assert planes(**{name: odd, 'bs': 1, 'T': 0}) == 0, name                 # bytes have no alignment
    assert planes(raw=p + 1) == -1 and b'2-byte aligned' in err()
    for shift in (7, -1, 16):
        assert planes(shift=shift) == -1 and b'shift' in err(), shift
    for shift in range(7):
        assert planes(shift=shift, T=0) == 0, shift
    for kw in (dict(Hc=0), dict(Hc=11), dict(Wc=0), dict(Wc=11), dict(Hc=-1), dict(Wc=-3)):
        assert planes(**kw) == -1 and b'chroma planes' in err(), kw
    for kw in (dict(Hc=1, Wc=1), dict(Hc=10, Wc=10), dict(H=11, W=9, Hc=11, Wc=9), dict(H=1, W=1, Hc=1, Wc=1)):      # any Hc <= H, Wc <= W; odd H and W
        assert planes(T=0, **kw) == 0, kw
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
    assert planes(W=5100, Wc=2550, tcx=35) == -1 and b'too wide' in err() and b'chroma' in err()                      # luma fits, chroma does not
    assert planes(bs=1, H=2160, W=3840, Hc=2160, Wc=3840, ty=35, tx=19, tcy=35, tcx=19) == -1 and b'too wide' in err() and b'chroma' in err()   # 8-bit 4:4:4 at 3840
    assert planes(T=-1) == -1 and planes(T=65536) == -1 and planes(H=0) == -1 and planes(W=0) == -1 and planes(n_src=0) == -1
    assert planes(T=0) == 0                                                      # nothing to do: returns before any launch


def test_ops_ingest_video_planes_refuses_before_the_device():
    from synchformer_amd import ops
    from synchformer_amd.ingest import RecordingIngest, plane_layout
    ing = RecordingIngest(torch.device('cpu'), 25, (270, 480), 16000, pix_fmt='uyvy422')
    tabs = (ing.y_first, ing.y_w, ing.x_first, ing.x_w, ing.cy_first, ing.cy_w, ing.cx_first, ing.cx_w, ing.csc)
    pick = torch.zeros(1, dtype=torch.int32)
    L = plane_layout('uyvy422', 270, 480)
    with pytest.raises(ValueError, match='expected uint8'):
        ops.ingest_video_planes(torch.zeros(1, 270, 480, 2, dtype=torch.uint16), L, pick, *tabs)
    with pytest.raises(ValueError, match='expected uint16'):
        ops.ingest_video_planes(torch.zeros(1, 270, 480, 2, dtype=torch.uint8), plane_layout('y210', 270, 480), pick, *tabs)
    with pytest.raises(ValueError, match='reaches byte'):                        # a frame one row short of its layout
        ops.ingest_video_planes(torch.zeros(1, 269, 480, 2, dtype=torch.uint8), L, pick, *tabs)
    with pytest.raises(ValueError, match='reaches byte'):                        # two frames declared by the stride, room for one and a half
        ops.ingest_video_planes(torch.zeros(2, 135, 480, 2, dtype=torch.uint8), L, pick, *tabs)
    with pytest.raises(ValueError, match='column stride'):
        ops.ingest_video_planes(torch.zeros(1, 270, 480, 2, dtype=torch.uint8), L._replace(stride_ccol=0), pick, *tabs)
    with pytest.raises(RuntimeError, match='device tensor'):                     # a CPU tensor: no fallback
        ops.ingest_video_planes(torch.zeros(1, 270, 480, 2, dtype=torch.uint8), L, pick, *tabs)


@pytest.mark.parametrize('H, W', list(Y.CASES))
def test_fp32_restatement_stays_inside_the_pixel_bar(H, W):
    """The margin the GPU bar leaves for 4:2:2: the package's tables and matrix evaluated in fp32 on the CPU (horizontal pass first, taps ascending - the kernel's
    order up to its fused multiply-adds) against the float64 oracle on uniform random planes, 8-bit and 10-bit.  Every pixel within 1 level and at most 1e-3 of
    the pixels differing (the project's bar); measured 6.6e-6 .. 3.3e-5, so the definition alone stays well inside the cap."""
    from synchformer_amd.ingest import RecordingIngest
    cs, full, loc, luma, chroma = Y.CASES[(H, W)]
    Hr, Wr, y0, x0 = Y.origin(H, W)
    for bits, pix_fmt in ((8, 'uyvy422'), (10, 'y210')):
        planes = Y.random_planes(2, H, W, H * 10000 + W + bits, 1 << bits)
        ref, outside = Y.oracle(planes, (Hr, Wr), y0, x0, *Y.matrix(cs, full, bits), loc)
        ing = RecordingIngest(torch.device('cpu'), 25, (H, W), 16000, pix_fmt=pix_fmt, colorspace=cs, full_range=full, chroma_loc=loc)
        assert ((ing.taps_y, ing.taps_x), (ing.taps_cy, ing.taps_cx)) == (luma, chroma)
        r = [Y.apply_tables32(planes[0], ing.y_first, ing.y_w, ing.x_first, ing.x_w)] + \
            [Y.apply_tables32(p, ing.cy_first, ing.cy_w, ing.cx_first, ing.cx_w) for p in planes[1:]]
        m, o = ing.csc[:9].reshape(3, 3), ing.csc[9:]
        pre = torch.einsum('ck,nkyx->ncyx', m, torch.stack([r[0] - o[0], r[1] - o[1], r[2] - o[2]], 1))
        got = pre.round().clamp(0, 255).to(torch.uint8)
        Y.check_pixels(got, ref, f'{H} x {W} {bits}-bit {cs} {"full" if full else "limited"} {loc}: fp32 restatement, {outside:.1%} outside [0, 255] before the clamp')
        assert outside > 0, outside
