"""No GPU: the host side of the YUV 4:2:0 ingest - the colour matrix against published values, the chroma tables and argument handling of
RecordingIngest, the ABI entry of sf_ingest_video_yuv and its argument rejection (before the device is touched), and the margin of the pixel bar: the oracle
module's fp32 restatement of the kernel's arithmetic against its float64 oracle."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_yuv_oracle as Y  # noqa: E402


def test_csc_matrix_published_values():
    from synchformer_amd.ingest import csc_matrix
    M, off = csc_matrix('bt601', False)
    assert M.dtype == off.dtype == torch.float64 and M.shape == (3, 3) and off.tolist() == [16.0, 128.0, 128.0]
    want = torch.tensor([[1.164384, 0.0, 1.596027], [1.164384, -0.391762, -0.812968], [1.164384, 2.017232, 0.0]], dtype=torch.float64)
    assert (M - want).abs().max().item() <= 1e-6, M
    M, off = csc_matrix('bt709', False)
    want = torch.tensor([[1.164384, 0.0, 1.792741], [1.164384, -0.213249, -0.532909], [1.164384, 2.112402, 0.0]], dtype=torch.float64)
    assert (M - want).abs().max().item() <= 1e-6 and off.tolist() == [16.0, 128.0, 128.0], M
    M, off = csc_matrix('bt601', True)
    want = torch.tensor([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], dtype=torch.float64)
    assert (M - want).abs().max().item() <= 1e-6 and off.tolist() == [0.0, 128.0, 128.0], M
    assert csc_matrix()[0].equal(csc_matrix('bt601', False)[0])                 # the default: what swscale assumes for an untagged stream
    for cs in ('bt601', 'bt709'):                                                # and the oracle's own formula agrees
        for full in (False, True):
            M, off = csc_matrix(cs, full)
            Mo, oo = Y.matrix64(cs, full)
            assert (M - Mo).abs().max().item() <= 1e-12 and torch.equal(off, oo)
    with pytest.raises(ValueError, match='colorspace'):
        csc_matrix('bt2020')


def test_recording_ingest_yuv_tables():
    from synchformer_amd.ingest import RecordingIngest, aa_bicubic_table
    cpu = torch.device('cpu')
    ing = RecordingIngest(cpu, 25, (1080, 1920), 48000, pix_fmt='nv12')
    assert (ing.taps_y, ing.taps_x, ing.taps_cy, ing.taps_cx) == (19, 19, 11, 11) and (ing.Hr, ing.Wr, ing.y0, ing.x0) == (256, 454, 16, 115)
    cyf, cyw, _ = aa_bicubic_table(540, 256)
    cxf, cxw, _ = aa_bicubic_table(960, 454)
    assert torch.equal(ing.cy_first, cyf[16:240]) and torch.equal(ing.cy_w, cyw[16:240])
    assert torch.equal(ing.cx_first, cxf[115:339]) and torch.equal(ing.cx_w, cxw[115:339])
    assert ing.pix_fmt == 'nv12' and ing.colorspace == 'bt601' and ing.full_range is False
    M, off = Y.matrix64('bt601', False)
    assert ing.csc.dtype == torch.float32 and ing.csc.device.type == 'cpu' and torch.equal(ing.csc, torch.cat([M.reshape(9), off]).float())
    ing = RecordingIngest(cpu, 25, (360, 202), 16000, pix_fmt='yuv420p', colorspace='bt709', full_range=True)
    M, off = Y.matrix64('bt709', True)
    assert torch.equal(ing.csc, torch.cat([M.reshape(9), off]).float()) and (ing.taps_cy, ing.taps_cx) == (5, 5)
    # frames of the wrong shape are refused before anything else happens
    with pytest.raises(ValueError, match='raw frames'):
        ing.frames(torch.zeros(4, 3, 360, 202, dtype=torch.uint8), 0, 1)
    with pytest.raises(ValueError, match='raw frames'):
        ing.frames(torch.zeros(4, 360, 202, dtype=torch.uint8), 0, 1)
    for (H, W), (_, _, luma, chroma) in Y.CASES.items():
        ing = RecordingIngest(cpu, 25, (H, W), 16000, pix_fmt='nv12')
        assert (ing.taps_y, ing.taps_x) == luma and (ing.taps_cy, ing.taps_cx) == chroma, (H, W)
        assert (ing.Hr, ing.Wr, ing.y0, ing.x0) == Y.origin(H, W)


def test_recording_ingest_yuv_argument_validation():
    from synchformer_amd.ingest import RecordingIngest
    cpu = torch.device('cpu')
    with pytest.raises(ValueError, match='even'):
        RecordingIngest(cpu, 25, (301, 518), 16000, pix_fmt='nv12')
    with pytest.raises(ValueError, match='even'):
        RecordingIngest(cpu, 25, (302, 517), 16000, pix_fmt='yuv420p')
    with pytest.raises(ValueError, match='pix_fmt'):
        RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt='yuv444p')
    with pytest.raises(ValueError, match='colorspace'):
        RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt='nv12', colorspace='bt2020')
    with pytest.raises(ValueError, match='colorspace'):
        RecordingIngest(cpu, 25, (270, 480), 16000, colorspace='bt2020')
    with pytest.raises(ValueError, match='channels_last'):
        RecordingIngest(cpu, 25, (270, 480), 16000, channels_last=True, pix_fmt='nv12')


def test_rgb24_objects_are_unchanged():
    """pix_fmt='rgb24' is the path of before: every attribute it had keeps its value, odd sizes stay legal, and nothing of the chroma side is built."""
    from synchformer_amd.ingest import RecordingIngest, aa_bicubic_table
    cpu = torch.device('cpu')
    for kw in ({}, {'pix_fmt': 'rgb24'}):
        ing = RecordingIngest(cpu, (30000, 1001), (301, 517), 48000, channels_last=True, **kw)
        assert (ing.H, ing.W, ing.Hr, ing.Wr, ing.y0, ing.x0, ing.taps_y, ing.taps_x) == (301, 517, 256, 438, 16, 107, 7, 7)
        assert ing.channels_last is True and ing.rate_in == 48000 and (ing.o, ing.n, ing.width) == (3, 1, 19) and ing.pix_fmt == 'rgb24'
        yf, yw, _ = aa_bicubic_table(301, 256)
        xf, xw, _ = aa_bicubic_table(517, 438)
        assert torch.equal(ing.y_first, yf[16:240]) and torch.equal(ing.y_w, yw[16:240]) and torch.equal(ing.x_first, xf[107:331]) and torch.equal(ing.x_w, xw[107:331])
        before = {'dev', 'fps_in', 'rate_in', 'channels_last', 'H', 'W', 'Hr', 'Wr', 'y0', 'x0', 'taps_y', 'taps_x', 'y_first', 'y_w', 'x_first', 'x_w', 'kernel',
                  'width', 'o', 'n', '_tables'}
        assert set(vars(ing)) == before | {'pix_fmt'}, set(vars(ing)) ^ before
        with pytest.raises(ValueError, match='raw frames'):
            ing.frames(torch.zeros(4, 3, 301, 517, dtype=torch.uint8), 0, 1)     # planar given, channels-last declared


def test_abi_lists_the_yuv_launcher():
    from synchformer_amd import _lib
    assert _lib.ABI_VERSION >= 16
    assert len(_lib.SIGNATURES['sf_ingest_video_yuv']) == 27
    for lib in (_lib.load(), _lib.load_ablation()):
        assert hasattr(lib, 'sf_ingest_video_yuv') and lib.sf_abi_version() >= 16


def test_yuv_launcher_rejects_bad_arguments_without_gpu():
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    v = dict(raw=p, sf=150, sy=10, uo=100, vo=101, csy=10, csx=2, n_src=1, H=10, W=10, ft=p, yf=p, yw=p, ty=5, xf=p, xw=p, tx=5, cyf=p, cyw=p, tcy=5, cxf=p,
             cxw=p, tcx=5, csc=p, out=p, T=1)

    def yuv(**kw):
        a = dict(v, **kw)
        return lib.sf_ingest_video_yuv(a['raw'], a['sf'], a['sy'], a['uo'], a['vo'], a['csy'], a['csx'], a['n_src'], a['H'], a['W'], a['ft'], a['yf'], a['yw'],
                                       a['ty'], a['xf'], a['xw'], a['tx'], a['cyf'], a['cyw'], a['tcy'], a['cxf'], a['cxw'], a['tcx'], a['csc'], a['out'], a['T'], None)

    for name in ('raw', 'ft', 'yf', 'yw', 'xf', 'xw', 'cyf', 'cyw', 'cxf', 'cxw', 'csc', 'out'):
        assert yuv(**{name: None}) == -1 and b'null pointer' in lib.sf_last_error(), name
    assert yuv(H=11) == -1 and b'even' in lib.sf_last_error()
    assert yuv(W=9) == -1 and b'even' in lib.sf_last_error()
    for name in ('ty', 'tx', 'tcy', 'tcx'):
        assert yuv(**{name: 0}) == -1 and b'out of range' in lib.sf_last_error(), name
        assert yuv(**{name: 36}) == -1 and b'out of range' in lib.sf_last_error(), name
        assert yuv(**{name: 35, 'T': 0}) == 0, name
    assert yuv(out=p + 1) == -1 and b'aligned' in lib.sf_last_error()
    assert yuv(csx=0) == -1 and b'stride' in lib.sf_last_error()
    assert yuv(sy=-1) == -1 and b'stride' in lib.sf_last_error()
    assert yuv(W=70000) == -1 and b'too wide' in lib.sf_last_error()
    assert yuv(W=5000, tcx=35) == -1 and b'too wide' in lib.sf_last_error() and b'chroma' in lib.sf_last_error()
    assert yuv(T=-1) == -1 and yuv(T=65536) == -1 and yuv(H=0) == -1
    assert yuv(T=0) == 0                                                         # nothing to do: returns before any launch


def test_ops_ingest_video_yuv_refuses_before_the_device():
    from synchformer_amd import ops
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(torch.device('cpu'), 25, (270, 480), 16000, pix_fmt='nv12')
    tabs = (ing.y_first, ing.y_w, ing.x_first, ing.x_w, ing.cy_first, ing.cy_w, ing.cx_first, ing.cx_w, ing.csc)
    pick = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match='pix_fmt'):
        ops.ingest_video_yuv(torch.zeros(1, 405, 480, dtype=torch.uint8), 'p010', pick, *tabs)
    with pytest.raises(ValueError, match='even H and W'):
        ops.ingest_video_yuv(torch.zeros(1, 404, 480, dtype=torch.uint8), 'nv12', pick, *tabs)
    with pytest.raises(ValueError, match='contiguous rows'):
        ops.ingest_video_yuv(torch.zeros(1, 405, 512, dtype=torch.uint8)[:, :, :480], 'yuv420p', pick, *tabs)
    with pytest.raises(RuntimeError, match='device tensor'):                     # a CPU tensor: no fallback
        ops.ingest_video_yuv(torch.zeros(1, 405, 480, dtype=torch.uint8), 'nv12', pick, *tabs)


@pytest.mark.parametrize('H, W', [(270, 480), (360, 202)])
def test_fp32_restatement_stays_inside_the_pixel_bar(H, W):
    """The margin the GPU bar leaves: the same tables and matrix evaluated in fp32 on the CPU (horizontal pass first, taps ascending - another summation order than
    the kernel's fused multiply-adds only in the last bits) against the float64 oracle, on uniform random planes, under the GPU tests' own bar (measured: at most
    1 level, <= 2.7e-5 of the pixels differ, so the bar leaves the kernel's summation order ~40x of room); the clamp is exercised (11-33 % of the values lie outside
    [0, 255] before it)."""
    from synchformer_amd.ingest import RecordingIngest
    cs, full, _, _ = Y.CASES[(H, W)]
    planes = Y.random_planes(2, H, W, H * 10000 + W)
    Hr, Wr, y0, x0 = Y.origin(H, W)
    ref, outside = Y.oracle(planes, (Hr, Wr), y0, x0, cs, full)
    ing = RecordingIngest(torch.device('cpu'), 25, (H, W), 16000, pix_fmt='nv12', colorspace=cs, full_range=full)
    r = [Y.apply_tables32(planes[0], ing.y_first, ing.y_w, ing.x_first, ing.x_w)] + \
        [Y.apply_tables32(p, ing.cy_first, ing.cy_w, ing.cx_first, ing.cx_w) for p in planes[1:]]
    m, o = ing.csc[:9].reshape(3, 3), ing.csc[9:]
    pre = torch.einsum('ck,nkyx->ncyx', m, torch.stack([r[0] - o[0], r[1] - o[1], r[2] - o[2]], 1))
    got = pre.round().clamp(0, 255).to(torch.uint8)
    Y.check_pixels(got, ref, f'{H} x {W} {cs} {"full" if full else "limited"}: fp32 restatement, {outside:.1%} outside [0, 255] before the clamp')
    assert outside > 0, outside
